// dm_match_global.h — whole-window scan relocalisation: the
// device code of dm_match_global, included by dm_goals.hip after dm_match.h.
// The result is dm_match_scans' best candidate at sub = 1, stride = 1 over a
// window of up to 8193 x 8193 translations and 1024 yaws; it is found by
// bounds from a max-pooled response field instead of a score volume.
//
//   M_B[c]   max of V over cells [cx, cx + B - 1] x [cy, cy + B - 1], cells out
//            of the grid reading 0, for cx in [-(B-1), W-1] (likewise cy)
//   bound    sum over used beams of M_B[qx + i0, qy + j0] >= score[k][j][i] for
//            every i in [i0, i0 + B), j in [j0, j0 + B): a block of B x B
//            translations of yaw k cannot beat its bound
//
// M_B is held over the extended coordinates e = c + B - 1 >= 0, padded to a
// multiple of B per axis (the padding's windows lie out of the grid: 0), and
// decimated by phase: plane (ey % B, ex % B) holds M_B at (ey / B, ex / B).  A
// beam's lookups for the blocks bi, bi + 1, ... of one block row are e, e + B,
// ...: one phase, adjacent bytes of one plane.  k_mg_bound's lanes run over
// bi, so a wave reads one line per beam where the plain layout would touch a
// line every B bytes.  The pool kernel pays for it with scattered byte stores,
// once per (map version, table, block).
//
// Kernels: k_mg_pool (workgroup = 64 x 64 tile of extended coordinates),
// k_mg_bound (thread = block of translations), k_mg_hist / k_mg_pick /
// k_mg_compact (the round's blocks: the highest bounds first, by histogram),
// k_mg_refine (workgroup = block, thread = translation, exact scores against
// V) and k_mg_fold (the round's candidates into the running best).  Ordering
// comes from kernel boundaries on one stream; no workgroup waits for another.
#pragma once

#include "dm_match.h"

namespace dm_mg {

constexpr int kThreads = 256;
constexpr int kBins = 2048;              // histogram bins over [lo, hi]
constexpr int kMaxB = 32;
constexpr int32_t kFar = -(1 << 29);     // coordinate of a beam that is not used: out of every window

// ctl words (device)
enum { C_COUNT = 0, C_BIN = 1, C_CAP = 2, C_WORDS = 4 };

struct Cand {
  uint32_t score;
  int32_t k, i, j;
};

// (score descending, then the SPEC's tie tuple ascending)
__device__ inline bool better(const Cand& a, const Cand& b, int32_t k0) {
  if (a.score != b.score) return a.score > b.score;
  const int32_t da = a.i * a.i + a.j * a.j, db = b.i * b.i + b.j * b.j;  // <= 2^25
  if (da != db) return da < db;
  const int32_t ka = a.k < k0 ? k0 - a.k : a.k - k0, kb = b.k < k0 ? k0 - b.k : b.k - k0;
  if (ka != kb) return ka < kb;
  if (a.k != b.k) return a.k < b.k;
  if (a.j != b.j) return a.j < b.j;
  return a.i < b.i;
}

// The workgroup's best of every thread's `c`; valid in thread 0.
__device__ inline Cand wg_best(Cand c, int32_t k0, Cand* s_c /*[kThreads / 64]*/) {
  for (int off = 32; off > 0; off >>= 1) {
    Cand o;
    o.score = (uint32_t)__shfl_down((int)c.score, off);
    o.k = __shfl_down(c.k, off);
    o.i = __shfl_down(c.i, off);
    o.j = __shfl_down(c.j, off);
    if (better(o, c, k0)) c = o;
  }
  if ((threadIdx.x & 63) == 0) s_c[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0)
    for (int w = 1; w < kThreads / 64; ++w)
      if (better(s_c[w], c, k0)) c = s_c[w];
  return c;
}

// best = (0, k0, 0, 0): the least tie tuple, so it stands exactly when nothing scores above 0
__global__ void k_mg_init(Cand* __restrict__ best, int32_t k0, int32_t* __restrict__ n_used) {
  if (threadIdx.x == 0) {
    Cand c = {0u, k0, 0, 0};
    *best = c;
    *n_used = 0;
  }
}

// ---- 1. pool --------------------------------------------------------------------
// Workgroup = tile (px, py) of 64 x 64 extended coordinates.  The patch of V it
// needs, cells [64 px - (B-1), 64 px + 63] per axis, goes to LDS (0 out of the
// grid); a row pass and a column pass of B - 1 maxima each.
__global__ __launch_bounds__(kThreads) void k_mg_pool(const uint8_t* __restrict__ V, int64_t W, int64_t H, int32_t lb,
                                                      int32_t EWB, int32_t EHB, int32_t PTX,
                                                      const int32_t* __restrict__ tile_list,
                                                      uint8_t* __restrict__ M) {
  __shared__ uint8_t s_v[64 + kMaxB - 1][64 + kMaxB];
  __shared__ uint8_t s_h[64 + kMaxB - 1][64];
  const int32_t B = 1 << lb, P = 64 + B - 1;
  const int32_t tile = tile_list[blockIdx.x];
  const int32_t e0x = (tile % PTX) * 64, e0y = (tile / PTX) * 64;
  for (int idx = threadIdx.x; idx < P * P; idx += kThreads) {
    const int r = idx / P, c = idx - r * P;
    const int64_t gx = (int64_t)e0x - (B - 1) + c, gy = (int64_t)e0y - (B - 1) + r;
    uint8_t v = 0;
    if (gx >= 0 && gx < W && gy >= 0 && gy < H) v = V[gy * W + gx];
    s_v[r][c] = v;
  }
  __syncthreads();
  for (int idx = threadIdx.x; idx < P * 64; idx += kThreads) {
    const int r = idx >> 6, x = idx & 63;
    int m = 0;
    for (int d = 0; d < B; ++d) m = max(m, (int)s_v[r][x + d]);
    s_h[r][x] = (uint8_t)m;
  }
  __syncthreads();
  const int64_t plane = (int64_t)EWB * EHB;
  for (int idx = threadIdx.x; idx < 64 * 64; idx += kThreads) {
    const int y = idx >> 6, x = idx & 63;
    int m = 0;
    for (int d = 0; d < B; ++d) m = max(m, (int)s_h[y + d][x]);
    const int32_t ex = e0x + x, ey = e0y + y;
    if ((ex >> lb) < EWB && (ey >> lb) < EHB)
      M[(int64_t)(((ey & (B - 1)) << lb) + (ex & (B - 1))) * plane + (int64_t)(ey >> lb) * EWB + (ex >> lb)] = (uint8_t)m;
  }
}

// ---- 2. bounds ------------------------------------------------------------------
// blockIdx.y = yaw k, thread = block t = bj * nbx + bi of the scan's window.  The
// beams go through LDS 256 at a time as (ex >> lb, ey >> lb, plane offset) of
// block (0, 0); block (bi, bj) adds (bi, bj).
__global__ __launch_bounds__(kThreads) void k_mg_bound(const int2* __restrict__ q, int32_t N,
                                                       const uint8_t* __restrict__ M, int32_t lb, int32_t EWB,
                                                       int32_t EHB, int32_t half_x, int32_t half_y, int32_t nbx,
                                                       int32_t nb, uint32_t* __restrict__ bound) {
  __shared__ int4 s_b[kThreads];
  const int32_t B = 1 << lb;
  const int32_t k = blockIdx.y;
  const int32_t t = (int32_t)(blockIdx.x * kThreads + threadIdx.x);
  const int32_t bj = t / nbx, bi = t - bj * nbx;
  const int32_t plane = EWB * EHB;  // B * B * plane <= (4096 + 64)^2
  uint32_t acc = 0;
  for (int32_t b0 = 0; b0 < N; b0 += kThreads) {
    const int32_t nbm = min(kThreads, N - b0);
    if ((int)threadIdx.x < nbm) {
      const int2 v = q[(int64_t)k * N + b0 + threadIdx.x];
      int4 b = make_int4(kFar, kFar, 0, 0);
      if (v.x != dm_match::kUnused) {
        const int32_t ex = v.x - half_x + (B - 1), ey = v.y - half_y + (B - 1);  // |v| < 2^30
        b.x = ex >> lb;  // floor for negative values too
        b.y = ey >> lb;
        b.z = (((ey & (B - 1)) << lb) + (ex & (B - 1))) * plane;
      }
      s_b[threadIdx.x] = b;
    }
    __syncthreads();
    for (int32_t b = 0; b < nbm; ++b) {
      const int4 bm = s_b[b];  // broadcast
      const int32_t X = bm.x + bi, Y = bm.y + bj;
      if ((uint32_t)X < (uint32_t)EWB && (uint32_t)Y < (uint32_t)EHB) acc += M[(int64_t)bm.z + (int64_t)Y * EWB + X];
    }
    __syncthreads();
  }
  if (t < nb) bound[(int64_t)k * nb + t] = acc;
}

// ---- 3. the round's blocks --------------------------------------------------------
__device__ inline int32_t bin_of(uint32_t b, uint32_t lo, uint32_t hi) {
  const unsigned long long v = (unsigned long long)(b - lo) * kBins / ((unsigned long long)(hi - lo) + 1ull);
  return (int32_t)(v < (unsigned long long)kBins ? v : (unsigned long long)(kBins - 1));
}

// hist[bin] = blocks with lo <= bound (refined blocks hold bound 0 < lo)
__global__ __launch_bounds__(kThreads) void k_mg_hist(const uint32_t* __restrict__ bound, int64_t n, uint32_t lo,
                                                      uint32_t hi, uint32_t* __restrict__ hist) {
  __shared__ uint32_t s_h[kBins];
  for (int j = threadIdx.x; j < kBins; j += kThreads) s_h[j] = 0;
  __syncthreads();
  for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < n; e += (int64_t)gridDim.x * kThreads) {
    const uint32_t b = bound[e];
    if (b >= lo) atomicAdd(&s_h[bin_of(b, lo, hi)], 1u);
  }
  __syncthreads();
  for (int j = threadIdx.x; j < kBins; j += kThreads)
    if (s_h[j]) atomicAdd(&hist[j], s_h[j]);
}

// ctl = the lowest non-empty bin such that the bins from it up hold at most cap
// blocks; the highest non-empty bin if that alone holds more (k_mg_compact
// then stops at cap); kBins if there is no block.
// One workgroup; thread t owns the bins [t * kPer, (t + 1) * kPer).  above(bin)
// = blocks in the bins from `bin` up does not increase with bin, so the pick
// is the lowest non-empty bin with above(bin) <= cap.
__global__ __launch_bounds__(kThreads) void k_mg_pick(const uint32_t* __restrict__ hist, uint32_t cap,
                                                      uint32_t* __restrict__ ctl) {
  constexpr int kPer = kBins / kThreads;
  __shared__ unsigned long long s_sum[kThreads];  // blocks in the bins of the threads above t
  __shared__ int s_pick, s_top;
  const int t = threadIdx.x;
  uint32_t h[kPer];
  unsigned long long own = 0;
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    h[j] = hist[t * kPer + j];
    own += h[j];
  }
  s_sum[t] = own;
  if (t == 0) {
    s_pick = kBins;
    s_top = -1;
  }
  __syncthreads();
  if (t == 0) {
    unsigned long long run = 0;
    for (int u = kThreads - 1; u >= 0; --u) {
      const unsigned long long c = s_sum[u];
      s_sum[u] = run;
      run += c;
    }
  }
  __syncthreads();
  unsigned long long above = s_sum[t];
#pragma unroll
  for (int j = kPer - 1; j >= 0; --j) {
    if (!h[j]) continue;
    above += h[j];
    atomicMax(&s_top, t * kPer + j);
    if (above <= (unsigned long long)cap) atomicMin(&s_pick, t * kPer + j);
  }
  __syncthreads();
  if (t == 0) {
    ctl[C_COUNT] = 0;
    ctl[C_BIN] = (uint32_t)(s_pick < kBins ? s_pick : (s_top >= 0 ? s_top : kBins));
    ctl[C_CAP] = cap;
  }
}

// list[0 .. min(count, cap)) = the picked blocks; a listed block's bound becomes
// 0: it is refined in this round and never again
__global__ __launch_bounds__(kThreads) void k_mg_compact(uint32_t* __restrict__ bound, int64_t n, uint32_t lo,
                                                         uint32_t hi, uint32_t* __restrict__ ctl,
                                                         int32_t* __restrict__ list) {
  const int32_t pick = (int32_t)ctl[C_BIN];
  const uint32_t cap = ctl[C_CAP];
  if (pick >= kBins) return;
  for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < n; e += (int64_t)gridDim.x * kThreads) {
    const uint32_t b = bound[e];
    if (b < lo || bin_of(b, lo, hi) < pick) continue;
    const uint32_t slot = atomicAdd(&ctl[C_COUNT], 1u);
    if (slot < cap) {
      list[slot] = (int32_t)e;
      bound[e] = 0u;
    }
  }
}

// ---- 4. exact scores of a block ---------------------------------------------------
// blockIdx.x = slot of the list (or block base + slot when list is NULL).  A
// thread owns up to four of the block's B x B translations (B = 32; one
// otherwise), lanes along i: adjacent bytes of V per beam.  Translations past
// half_x / half_y (the last blocks' overhang) are not candidates.
__global__ __launch_bounds__(kThreads) void k_mg_refine(const int2* __restrict__ q, int32_t N,
                                                        const uint8_t* __restrict__ V, int64_t W, int64_t H,
                                                        int32_t lb, int32_t half_x, int32_t half_y, int32_t nbx,
                                                        int32_t nb, int32_t k0, const int32_t* __restrict__ list,
                                                        int32_t base, const uint32_t* __restrict__ ctl,
                                                        int32_t n_fixed, Cand* __restrict__ cand) {
  __shared__ int2 s_b[kThreads];
  __shared__ Cand s_c[kThreads / 64];
  const int32_t n = ctl ? (int32_t)min(ctl[C_COUNT], ctl[C_CAP]) : n_fixed;
  const int32_t slot = blockIdx.x;
  if (slot >= n) return;  // uniform
  const int32_t B = 1 << lb;
  const int32_t id = list ? list[slot] : base + slot;
  const int32_t k = id / nb, t = id - k * nb;
  const int32_t bj = t / nbx, bi = t - bj * nbx;
  const int32_t i0 = -half_x + bi * B, j0 = -half_y + bj * B;
  const int32_t per = (B * B + kThreads - 1) / kThreads;  // 4 at B = 32, else 1
  int32_t ti[4], tj[4];
  bool ok[4];
  uint32_t acc[4] = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    const int32_t tr = (int32_t)threadIdx.x + m * kThreads;
    ti[m] = i0 + (tr & (B - 1));
    tj[m] = j0 + (tr >> lb);
    ok[m] = m < per && tr < B * B && ti[m] <= half_x && tj[m] <= half_y;
  }
  const uint32_t uW = (uint32_t)W, uH = (uint32_t)H;  // W, H <= 2^30
  for (int32_t b0 = 0; b0 < N; b0 += kThreads) {
    const int32_t nbm = min(kThreads, N - b0);
    if ((int)threadIdx.x < nbm) {
      int2 v = q[(int64_t)k * N + b0 + threadIdx.x];
      if (v.x == dm_match::kUnused) v = make_int2(kFar, kFar);
      s_b[threadIdx.x] = v;
    }
    __syncthreads();
    for (int32_t b = 0; b < nbm; ++b) {
      const int2 bm = s_b[b];  // broadcast
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        if (!ok[m]) continue;
        const int32_t cx = bm.x + ti[m], cy = bm.y + tj[m];
        if ((uint32_t)cx < uW && (uint32_t)cy < uH) acc[m] += V[(int64_t)cy * W + cx];
      }
    }
    __syncthreads();
  }
  Cand c = {0u, k0, 0, 0};
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    if (!ok[m]) continue;
    const Cand o = {acc[m], k, ti[m], tj[m]};
    if (better(o, c, k0)) c = o;
  }
  c = wg_best(c, k0, s_c);
  if (threadIdx.x == 0) cand[slot] = c;
}

// ---- 5. the running best ------------------------------------------------------------
// One workgroup: *best = the best of *best and cand[0 .. n).  h_out (mapped host
// memory) = score, k, i, j, n, used beams.
__global__ __launch_bounds__(kThreads) void k_mg_fold(const Cand* __restrict__ cand,
                                                      const uint32_t* __restrict__ ctl, int32_t n_fixed,
                                                      int32_t k0, Cand* __restrict__ best,
                                                      const int32_t* __restrict__ n_used,
                                                      volatile uint32_t* __restrict__ h_out) {
  __shared__ Cand s_c[kThreads / 64];
  const int32_t n = ctl ? (int32_t)min(ctl[C_COUNT], ctl[C_CAP]) : n_fixed;
  Cand c = {0u, k0, 0, 0};
  for (int32_t e = threadIdx.x; e < n; e += kThreads) {
    const Cand o = cand[e];
    if (better(o, c, k0)) c = o;
  }
  c = wg_best(c, k0, s_c);
  if (threadIdx.x == 0) {
    const Cand cur = *best;
    if (better(cur, c, k0)) c = cur;
    *best = c;
    h_out[0] = c.score;
    h_out[1] = (uint32_t)c.k;
    h_out[2] = (uint32_t)c.i;
    h_out[3] = (uint32_t)c.j;
    h_out[4] = (uint32_t)n;
    h_out[5] = (uint32_t)*n_used;
    __threadfence_system();
  }
}

}  // namespace dm_mg
