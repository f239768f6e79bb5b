// dm_match.h — correlative scan matcher over the tiled map:
// the device code of dm_match_field and dm_match_scans, included by
// dm_goals.hip.  Takes over slam_toolbox's correlative scan matcher
// (slam_config.yaml:35, 50-53, 64-66).
//
// Definitions (include/dm.h; integers and separately rounded doubles, no FMA,
// so every result is unique and bit-exact):
//   V[c]      max over in-grid occupied cells o (state 100) with
//             d2 = dx^2 + dy^2 <= r^2 of kern[d2]; 0 if there is none
//   (qx, qy)  floor((e - origin) / step) of a used beam's endpoint e for one
//             candidate yaw, step = resolution / sub (dm_match_endpoint,
//             dm_ray.h)
//   score     sum over used beams of V[floordiv(qx + i*stride, sub),
//             floordiv(qy + j*stride, sub)], 0 for cells out of the grid
//   best      maximal score, ties to the least (i*i + j*j, |k - k0|, k, j, i)
// The host restatement is dm/match.py.
//
// Four kernels: k_match_field (workgroup = tile, only the tiles the search
// windows reach), k_match_prep (thread = candidate yaw x beam), k_match_score
// (workgroup = candidate yaw x beam chunk, thread = translation) and
// k_match_best (workgroup = scan).  Score sums are integers: the chunks'
// atomic adds commute, so the volume does not depend on their order.
#pragma once

#include "dm_internal.h"

namespace dm_match {

constexpr int kThreads = 256;
constexpr int kMaxR = 16;                 // smear_cells limit = the halo read around a tile
constexpr int32_t kUnused = (int32_t)0x80000000;  // qx of a beam that is not used
constexpr int kBeamsPerChunk = 256;       // beams one k_match_score workgroup stages in LDS

// ---- 1. response field --------------------------------------------------------
// Workgroup = tile.  The occupied bits of the tile's rows with a 16-row halo
// above and below, three 64-bit words per row (the tile's columns and the 64
// to either side; only the r nearest halo columns are read).  A cell takes,
// for every |dy| <= r, the bits of row y + dy within hw(|dy|) =
// floor(sqrt(r^2 - dy^2)) columns of it as one word.  With a table that does
// not increase in d2 (mono) the row's nearest set bit decides (clz / ffs);
// otherwise every set bit of the window is looked up, which is the
// definition itself.  Tiles nothing has touched (tile_seen == 0) hold no
// occupied cell and are not read, as halo or as centre; their V is still
// computed, from the neighbours' bits.
__global__ __launch_bounds__(kThreads) void k_match_field(const int8_t* __restrict__ state,
                                                          const uint8_t* __restrict__ tile_seen, int64_t W,
                                                          int64_t H, int64_t TX, int32_t r,
                                                          const uint8_t* __restrict__ kern, int32_t mono,
                                                          const int32_t* __restrict__ tile_list,
                                                          uint8_t* __restrict__ V) {
  __shared__ unsigned long long s_occ[DM_TILE + 2 * kMaxR][3];
  __shared__ uint8_t s_kern[kMaxR * kMaxR + 1];
  __shared__ int s_hw[kMaxR + 1];
  __shared__ int s_any;
  const int64_t tile = tile_list ? (int64_t)tile_list[blockIdx.x] : (int64_t)blockIdx.x;
  const int64_t tx = tile % TX, ty = tile / TX;
  const int64_t x0 = tx * DM_TILE, y0 = ty * DM_TILE;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x == 0) s_any = 0;
  for (int j = threadIdx.x; j <= r * r; j += kThreads) s_kern[j] = kern[j];
  if ((int)threadIdx.x <= r) {
    const int d = threadIdx.x;
    int h = 0;
    while ((h + 1) * (h + 1) + d * d <= r * r) ++h;
    s_hw[d] = h;
  }
  __syncthreads();
  for (int j = wave; j < (DM_TILE + 2 * kMaxR) * 3; j += kThreads / 64) {
    const int row = j / 3, wc = j % 3;
    const int64_t gy = y0 - kMaxR + row, gx = x0 + (int64_t)(wc - 1) * DM_TILE + lane;
    bool occ = false;
    if (row >= kMaxR - r && row < kMaxR + DM_TILE + r && gy >= 0 && gy < H && gx >= 0 && gx < W && gx >= x0 - r &&
        gx < x0 + DM_TILE + r && tile_seen[(gy >> 6) * TX + (gx >> 6)])
      occ = state[gy * W + gx] == 100;
    const unsigned long long word = __ballot(occ);
    if (lane == 0) {
      s_occ[row][wc] = word;
      if (word) atomicOr(&s_any, 1);
    }
  }
  __syncthreads();
  const bool any = s_any != 0;  // uniform
  for (int y = wave; y < DM_TILE; y += kThreads / 64) {
    const int64_t gy = y0 + y, gx = x0 + lane;
    int best = 0;
    if (any) {
      for (int dy = -r; dy <= r; ++dy) {
        const int row = y + kMaxR + dy;
        const unsigned long long L = s_occ[row][0], C = s_occ[row][1], R = s_occ[row][2];
        if ((L | C | R) == 0ull) continue;  // wave-uniform
        const int ady = dy < 0 ? -dy : dy;
        const int h = s_hw[ady];
        // win: bit b = the row's cell of tile column lane - 32 + b
        const int p = lane + 32;
        unsigned long long win;
        if (p < 64) win = (L >> p) | (C << (64 - p));
        else if (p == 64) win = C;
        else win = (C >> (p - 64)) | (R << (128 - p));
        unsigned long long m = (win >> (32 - h)) & ((2ull << (2 * h)) - 1ull);  // bit h = dx 0
        if (!m) continue;
        if (mono) {
          const unsigned long long lo = m & ((2ull << h) - 1ull), hi = m >> h;
          int d = 64;
          if (lo) d = h - (63 - __clzll((long long)lo));
          if (hi) d = min(d, __ffsll((long long)hi) - 1);
          best = max(best, (int)s_kern[ady * ady + d * d]);
        } else {
          while (m) {
            const int dx = __ffsll((long long)m) - 1 - h;
            m &= m - 1ull;
            best = max(best, (int)s_kern[ady * ady + dx * dx]);
          }
        }
      }
    }
    if (gy < H && gx < W) V[gy * W + gx] = (uint8_t)best;
  }
}

// ---- 2. fine coordinates ------------------------------------------------------
// blockIdx.x = s * A + k, blockIdx.y = block of 256 beams.  q[(s*A + k)*N + i]
// = (qx, qy), or qx = kUnused.  n_used[s] counts the used beams of k0.
__global__ __launch_bounds__(kThreads) void k_match_prep(MatchArgs a, const double* __restrict__ pose4,
                                                         const float* __restrict__ ranges,
                                                         const double* __restrict__ trig, int32_t A, int32_t k0,
                                                         int2* __restrict__ q, int32_t* __restrict__ n_used) {
  const int64_t sk = blockIdx.x;
  const int64_t s = sk / A;
  const int32_t k = (int32_t)(sk % A);
  const int32_t i = (int32_t)(blockIdx.y * kThreads + threadIdx.x);
  bool used = false;
  if (i < a.N) {
    int32_t qx = kUnused, qy = kUnused;
    used = dm_match_endpoint(a, pose4 + 4 * sk, ranges[s * a.N + i], trig + 2 * i, &qx, &qy);
    q[sk * a.N + i] = make_int2(qx, qy);
  }
  if (k == k0) {  // workgroup-uniform
    const int c = __popcll(__ballot(used));
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(&n_used[s], c);
  }
}

// ---- 3. scores ----------------------------------------------------------------
// blockIdx.x = s * A + k, blockIdx.y = chunk of chunk_len <= kBeamsPerChunk
// beams.  The chunk's beams go to LDS once as (cx0, cy0, rx, ry) with
// qx = cx0 * sub + rx, 0 <= rx < sub (the only divisions: two per beam).  A
// thread owns translations t = j' * (2 half + 1) + i'; with i * stride =
// dq * sub + dr (0 <= dr < sub) the candidate's cell is cx0 + dq + (rx + dr
// >= sub), integer adds only.  It sums V over the chunk's beams in a register
// and adds the sum to the volume: no two threads of a workgroup share an
// address, chunks meet in an atomic add.
__global__ __launch_bounds__(kThreads) void k_match_score(const int2* __restrict__ q, int32_t N,
                                                          int32_t chunk_len, const uint8_t* __restrict__ V,
                                                          int64_t W, int64_t H, int32_t sub, int32_t half,
                                                          int32_t stride, uint32_t* __restrict__ vol) {
  __shared__ int4 s_b[kBeamsPerChunk];
  const int64_t sk = blockIdx.x;
  const int32_t b0 = (int32_t)blockIdx.y * chunk_len;
  const int32_t nb = min(chunk_len, N - b0);
  if (nb <= 0) return;  // uniform
  const int32_t T1 = 2 * half + 1, T = T1 * T1;
  if ((int)threadIdx.x < nb) {
    const int2 v = q[sk * N + b0 + threadIdx.x];
    int4 b;
    if (v.x == kUnused) {
      b = make_int4(kUnused / 2, kUnused / 2, 0, 0);  // stays out of the grid for every translation
    } else {
      b.x = dm_floordiv32(v.x, sub);
      b.y = dm_floordiv32(v.y, sub);
      b.z = v.x - b.x * sub;
      b.w = v.y - b.y * sub;
    }
    s_b[threadIdx.x] = b;
  }
  __syncthreads();
  const uint32_t uW = (uint32_t)W, uH = (uint32_t)H;  // W, H <= 2^30
  for (int32_t t = threadIdx.x; t < T; t += kThreads) {
    const int32_t dj = (t / T1 - half) * stride, di = (t % T1 - half) * stride;
    const int32_t dqx = dm_floordiv32(di, sub), drx = di - dqx * sub;
    const int32_t dqy = dm_floordiv32(dj, sub), dry = dj - dqy * sub;
    uint32_t acc = 0;
    for (int32_t b = 0; b < nb; ++b) {
      const int4 bm = s_b[b];  // broadcast
      const int32_t cx = bm.x + dqx + (bm.z + drx >= sub ? 1 : 0);
      const int32_t cy = bm.y + dqy + (bm.w + dry >= sub ? 1 : 0);
      if ((uint32_t)cx < uW && (uint32_t)cy < uH) acc += V[(int64_t)cy * W + cx];
    }
    if (acc) atomicAdd(&vol[sk * T + t], acc);
  }
}

// ---- 4. best candidate --------------------------------------------------------
// Workgroup = scan.  Candidates compare by (score descending, tie ascending),
// tie = i*i + j*j (12 bits) | |k - k0| (6) | k (6) | j + half (7) | i + half
// (7): the SPEC's tuple, every field non-negative.  out[s] = (k, i, j, score).
struct Cand {
  uint32_t score, tie_hi, tie_lo;
};
__device__ inline bool better(const Cand& a, const Cand& b) {
  if (a.score != b.score) return a.score > b.score;
  if (a.tie_hi != b.tie_hi) return a.tie_hi < b.tie_hi;
  return a.tie_lo < b.tie_lo;
}

__global__ __launch_bounds__(kThreads) void k_match_best(const uint32_t* __restrict__ vol, int32_t A, int32_t half,
                                                         int32_t k0, int32_t* __restrict__ out) {
  __shared__ Cand s_c[kThreads / 64];
  const int64_t s = blockIdx.x;
  const int32_t T1 = 2 * half + 1, T = T1 * T1, n = A * T;
  Cand best = {0u, 0xFFFFFFFFu, 0xFFFFFFFFu};  // loses to every candidate
  for (int32_t e = threadIdx.x; e < n; e += kThreads) {
    const int32_t k = e / T, rem = e % T, j = rem / T1 - half, i = rem % T1 - half;
    const int32_t adk = k < k0 ? k0 - k : k - k0;
    const unsigned long long tie = ((unsigned long long)(i * i + j * j) << 26) | ((unsigned long long)adk << 20) |
                                   ((unsigned long long)k << 14) | ((unsigned long long)(j + half) << 7) |
                                   (unsigned long long)(i + half);
    const Cand c = {vol[s * n + e], (uint32_t)(tie >> 32), (uint32_t)tie};
    if (better(c, best)) best = c;
  }
  for (int off = 32; off > 0; off >>= 1) {
    Cand o;
    o.score = (uint32_t)__shfl_down((int)best.score, off);
    o.tie_hi = (uint32_t)__shfl_down((int)best.tie_hi, off);
    o.tie_lo = (uint32_t)__shfl_down((int)best.tie_lo, off);
    if (better(o, best)) best = o;
  }
  if ((threadIdx.x & 63) == 0) s_c[threadIdx.x >> 6] = best;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kThreads / 64; ++w)
      if (better(s_c[w], best)) best = s_c[w];
    out[4 * s + 0] = (int32_t)((best.tie_lo >> 14) & 63u);
    out[4 * s + 1] = (int32_t)(best.tie_lo & 127u) - half;
    out[4 * s + 2] = (int32_t)((best.tie_lo >> 7) & 127u) - half;
    out[4 * s + 3] = (int32_t)best.score;
  }
}

}  // namespace dm_match
