// dm_gain.h — visible-unknown count of a viewpoint: the device
// code of dm_gain_views and dm_assign_goals_gain, and of the overlap-aware
// dm_gain_views_joint, dm_assign_goals_coord and dm_gain_claimed (§9.4),
// included by dm_goals.hip.
//
// Definition (integers only, so every result is unique and bit-exact), for a
// view cell (vx, vy) and radius_cells = R in [1, kMaxR]:
//   rays     one to each of the 8R offsets (ex, ey) with max(|ex|, |ey|) == R
//   line     the SPEC a5 line of dm_ray.h from the view: major axis x iff
//            |ex| >= |ey|, n = R, adb = min(|ex|, |ey|); step k (0..R) is at
//            major = k * ia, minor = ib * floor((2 k adb + n) / (2 n))
//   walk     from k = 0; the ray ends before the first cell that is out of the
//            grid, has dx^2 + dy^2 > R^2, or has state 100
//   marking  every cell visited before that with an unknown state (neither 0
//            nor 100) is marked; gain = the number of distinct marked cells
// The host restatement is dm/gain.py.
//
// Workgroup = view.  The marked set is a bitmap in LDS, (2R + 1) rows of
// ceil((2R + 1) / 32) words, addressed by (dy + R, dx + R): |dx|, |dy| <= k <= R
// on every step, so every address is inside it.  Lanes take the rays
// tid, tid + kThreads, ... and walk each with PieceWalk's incremental carry
// (rem starts at n, rem += 2 adb per step, carry at rem >= 2 n; n = R for every
// ray).  state is read from global memory: a view's window is at most
// 1023 x 1023 bytes and L2-resident.  A bit is set with an LDS atomic OR only
// after a plain read shows it clear: near the view every ray shares the same
// cells, and unconditional atomics there serialise.  Then popcount, reduce,
// one uint32 per view.
//
// LDS: 4 (2R + 1) ceil((2R + 1) / 32) bytes, 30,784 B at R = 240 and
// 130,944 B at R = 511 (gfx950's 160 KiB LDS holds it; this is where kMaxR
// comes from).  Up to kDynBytes the bitmap is dynamic LDS sized per launch
// (k_gain_views<false>); above, the kernel declares the largest bitmap
// statically (k_gain_views<true>), the form of a > 64 KiB launch that is known
// to work on this part.
#pragma once

#include "dm_internal.h"

namespace dm_gain {

constexpr int kThreads = 256;
constexpr int kMaxR = 511;
constexpr int kMaxWords = (2 * kMaxR + 1) * ((2 * kMaxR + 1 + 31) / 32);  // 32,736 words
constexpr int kDynBytes = 64 * 1024;

inline int64_t bitmap_words(int32_t R) { return (int64_t)(2 * R + 1) * ((2 * R + 1 + 31) / 32); }

// Views that dm_assign_goals_gain need not cast: clusters below min_size and
// clusters the robot's field does not reach.
__global__ void k_gain_skip(const dm_cluster* __restrict__ recs, const uint32_t* __restrict__ cost, int64_t K,
                            int64_t min_size, uint8_t* __restrict__ skip) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= K) return;
  skip[c] = (recs[c].size < min_size || cost[c] == DM_PLAN_UNREACHABLE) ? 1 : 0;
}

// The same for dm_assign_goals_team's R x K views: view r * K + c is cluster
// c under robot r's field, cost[r * K + c].
__global__ void k_gain_skip_team(const dm_cluster* __restrict__ recs, const uint32_t* __restrict__ cost, int64_t K,
                                 int64_t n, int64_t min_size, uint8_t* __restrict__ skip) {
  const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= n) return;
  skip[v] = (recs[v % K].size < min_size || cost[v] == DM_PLAN_UNREACHABLE) ? 1 : 0;
}

// Words of a row of the claimed set (below): bit x & 31 of word
// y * claimed_wpr(W) + (x >> 5) is cell (x, y).
__host__ __device__ inline int32_t claimed_wpr(int32_t W) { return (W + 31) >> 5; }

// The claimed word at (row y, word index q); 0 outside the grid.
__device__ inline uint32_t claimed_load(const uint32_t* claimed, int32_t cwpr, int32_t H, int32_t y, int32_t q) {
  return (y >= 0 && y < H && q >= 0 && q < cwpr) ? claimed[(int64_t)y * cwpr + q] : 0u;
}

// cells[v]: the view's linear cell, < 0 for none (gain 0).  skip (may be
// null): skip[v] != 0 gives gain 0 without a cast.  memo_cell / memo_gain (may
// be null): the cell and gain of the last cast of view slot v; a view on the
// same cell takes the gain from there.
//
// The overlap-aware calls (dm_gain_views_joint, dm_assign_goals_coord; DESIGN
// §9.4) keep a claimed set C, a global bitmap of H rows of claimed_wpr(W)
// words.  The LDS word (row, wi) of a view covers map row y = vy + row - R and
// the columns x0 .. x0 + 31, x0 = vx - R + 32 wi; its claimed bits are the two
// global words at floor(x0 / 32) and + 1 of row y, shifted down by x0 mod 32
// (floor division and modulo: x0 < 0 within R of the left edge).
//   kMask    after the walk the claimed bits are taken out of the LDS bitmap,
//            so the count is the marginal gain, |V minus C|; a memo is then
//            only good for the C it was filled under (dm_api.cpp drops it
//            after every commit)
//   kCommit  after that every non-zero LDS word is ORed into the one or two
//            global words it overlaps: C := C u V
// With both, all reads of C come before a barrier and all ORs after it.
// Between workgroups nothing waits: a launch that reports marginals has no
// concurrent writer of C (kMask && kCommit is launched one view at a time,
// kMask alone only reads, kCommit alone counts nothing and ORs commute).
template <bool kStatic, bool kMask = false, bool kCommit = false>
__global__ __launch_bounds__(kThreads) void k_gain_views(const int8_t* __restrict__ state, int32_t W, int32_t H,
                                                         const int64_t* __restrict__ cells,
                                                         const uint8_t* __restrict__ skip, int32_t R,
                                                         int64_t* __restrict__ memo_cell,
                                                         uint32_t* __restrict__ memo_gain,
                                                         uint32_t* __restrict__ out_gain,
                                                         uint32_t* claimed) {
  extern __shared__ __attribute__((aligned(16))) uint32_t s_dyn[];
  __shared__ uint32_t s_fix[kStatic ? kMaxWords : 1];
  __shared__ uint32_t s_sum;
  uint32_t* const bits = kStatic ? s_fix : s_dyn;

  const int64_t v = blockIdx.x;
  const int tid = threadIdx.x;
  // every branch up to the cast is uniform over the workgroup
  const int64_t cell = cells[v];
  constexpr bool kCount = kMask || !kCommit;  // kCommit alone reports nothing: out_gain is not touched
  if (cell < 0 || (skip && skip[v])) {
    if (kCount && tid == 0) out_gain[v] = 0u;
    return;
  }
  if (memo_cell && memo_cell[v] == cell) {
    if (tid == 0) out_gain[v] = memo_gain[v];
    return;
  }
  const int32_t vx = (int32_t)(cell % W), vy = (int32_t)(cell / W);
  const int32_t side = 2 * R + 1, wpr = (side + 31) >> 5, nwords = side * wpr;
  for (int32_t i = tid; i < nwords; i += kThreads) bits[i] = 0u;
  if (tid == 0) s_sum = 0u;
  __syncthreads();

  const int32_t two_n = 2 * R, r2 = R * R;
  for (int32_t ray = tid; ray < 8 * R; ray += kThreads) {
    // the square's perimeter: bottom and top rows (2R + 1 each), then the
    // left and right columns without their corners (2R - 1 each)
    int32_t ex, ey;
    if (ray < 2 * side) {
      const bool top = ray >= side;
      ex = (top ? ray - side : ray) - R;
      ey = top ? R : -R;
    } else {
      const int32_t j = ray - 2 * side;
      const bool right = j >= side - 2;
      ey = (right ? j - (side - 2) : j) - R + 1;
      ex = right ? R : -R;
    }
    const int32_t ax = ex < 0 ? -ex : ex, ay = ey < 0 ? -ey : ey;
    const int32_t sx = (ex > 0) - (ex < 0), sy = (ey > 0) - (ey < 0);
    const bool xmajor = ax >= ay;
    const int32_t two_adb = 2 * (xmajor ? ay : ax);
    const int32_t dxa = xmajor ? sx : 0, dya = xmajor ? 0 : sy;  // per step
    const int32_t dxb = xmajor ? 0 : sx, dyb = xmajor ? sy : 0;  // per carry
    int32_t dx = 0, dy = 0, rem = R;
    for (int32_t k = 0; k <= R; ++k) {
      const int32_t x = vx + dx, y = vy + dy;
      if (x < 0 || x >= W || y < 0 || y >= H || dx * dx + dy * dy > r2) break;
      const int8_t s = state[(int64_t)y * W + x];
      if (s == 100) break;
      if (s != 0) {
        const int32_t col = dx + R;
        const int32_t w = (dy + R) * wpr + (col >> 5);
        const uint32_t b = 1u << (col & 31);
        if (!(bits[w] & b)) atomicOr(&bits[w], b);
      }
      dx += dxa;
      dy += dya;
      rem += two_adb;
      if (rem >= two_n) {
        rem -= two_n;
        dx += dxb;
        dy += dyb;
      }
    }
  }
  __syncthreads();

  if constexpr (kMask || kCommit) {
    const int32_t cwpr = claimed_wpr(W);
    if constexpr (kMask) {
      for (int32_t i = tid; i < nwords; i += kThreads) {
        const uint32_t m = bits[i];
        if (!m) continue;
        const int32_t row = i / wpr, x0 = vx - R + 32 * (i - row * wpr), y = vy + row - R;
        const int32_t q = x0 >> 5, sh = x0 & 31;  // floor division and modulo
        const uint32_t lo = claimed_load(claimed, cwpr, H, y, q), hi = claimed_load(claimed, cwpr, H, y, q + 1);
        bits[i] = m & ~(uint32_t)((((uint64_t)hi << 32) | lo) >> sh);
      }
      __syncthreads();  // every read of C is before every OR below
    }
    if constexpr (kCommit) {
      for (int32_t i = tid; i < nwords; i += kThreads) {
        const uint32_t m = bits[i];
        if (!m) continue;
        const int32_t row = i / wpr, x0 = vx - R + 32 * (i - row * wpr), y = vy + row - R;
        if (y < 0 || y >= H) continue;
        const int32_t q = x0 >> 5, sh = x0 & 31;
        const uint32_t lo = m << sh, hi = sh ? m >> (32 - sh) : 0u;
        if (lo && q >= 0 && q < cwpr) atomicOr(&claimed[(int64_t)y * cwpr + q], lo);
        if (hi && q + 1 >= 0 && q + 1 < cwpr) atomicOr(&claimed[(int64_t)y * cwpr + q + 1], hi);
      }
    }
  }
  if constexpr (!kCount) return;

  uint32_t c = 0u;
  for (int32_t i = tid; i < nwords; i += kThreads) c += (uint32_t)__popc(bits[i]);
  for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off);
  if ((tid & 63) == 0 && c) atomicAdd(&s_sum, c);
  __syncthreads();
  if (tid == 0) {
    out_gain[v] = s_sum;
    if (memo_cell) {
      memo_cell[v] = cell;
      memo_gain[v] = s_sum;
    }
  }
}

// Cells of n view points (metres): floor((x - origin) / resolution) per axis,
// -1 outside the grid or non-finite.
__global__ void k_gain_cells(const double* __restrict__ xy, int64_t n, int64_t W, int64_t H, double ox, double oy,
                             double res, int64_t* __restrict__ out_cell) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double fx = floor((xy[2 * i] - ox) / res), fy = floor((xy[2 * i + 1] - oy) / res);
  const bool in = fx >= 0.0 && fx < (double)W && fy >= 0.0 && fy < (double)H;  // NaN: out of grid
  out_cell[i] = in ? (int64_t)fy * W + (int64_t)fx : -1;
}

// The claimed set as bytes, 1 / 0 per cell (dm_gain_claimed).
__global__ void k_gain_expand(const uint32_t* __restrict__ claimed, int32_t W, int32_t H,
                              uint8_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)W * H) return;
  const int32_t x = (int32_t)(i % W), y = (int32_t)(i / W);
  out[i] = (uint8_t)((claimed[(int64_t)y * claimed_wpr(W) + (x >> 5)] >> (x & 31)) & 1u);
}

}  // namespace dm_gain
