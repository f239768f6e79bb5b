// dm_goals.hip — frontier goal selection on the device.
//
// Policy (the host restatement is dm/goals.py, the test reference): robot r
// at (rx, ry) scores cluster c with
//   dx = cx_m - rx; dy = cy_m - ry; dist = sqrt(dx*dx + dy*dy)
//   util = size / (1 + w * dist)            (IEEE double, no FMA)
// over the clusters with size >= min_size and dist >= min_distance, takes the
// best util, ties to the smaller label.  Robots choose in order, each taking
// the best cluster no earlier robot took (greedy assignment; the reference
// explores reactively, main.py:123-188, so there is no reference policy).
//
// Robot r's choice is among its R best clusters (at most R - 1 are taken
// before its turn), so the device computes every robot's top R — one
// bitonic sort per (robot, 4096-record chunk) in LDS, then merges of the
// chunk lists — and the host runs the O(R^2) greedy over those lists.  The
// records are the label-sorted list of the last collected frontier result, so
// "smaller label" is "smaller record index".
#include <algorithm>

#include "dm_gain.h"
#include "dm_internal.h"
#include "dm_match.h"
#include "dm_match_global.h"
#include "dm_plan.h"

namespace {

constexpr int kGoalN = 4096;       // keys per sort (one workgroup)
constexpr int kGoalThreads = 256;

// Key of a candidate: the util's IEEE bits (util > 0, so larger util = larger
// unsigned bits); 0 = not eligible.  Order: larger key first, then smaller
// index.
__device__ inline bool goal_better(unsigned long long ka, uint32_t ia, unsigned long long kb, uint32_t ib) {
  return ka > kb || (ka == kb && ia < ib);
}

// Sort s_k / s_i (kGoalN entries) best-first.
__device__ inline void goal_sort(unsigned long long* s_k, uint32_t* s_i) {
  for (int k = 2; k <= kGoalN; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = threadIdx.x; i < kGoalN; i += kGoalThreads) {
        const int l = i ^ j;
        if (l <= i) continue;
        const unsigned long long ka = s_k[i], kb = s_k[l];
        const uint32_t ia = s_i[i], ib = s_i[l];
        // blocks with (i & k) == 0 put the better one first, the others last
        const bool swap = ((i & k) == 0) ? goal_better(kb, ib, ka, ia) : goal_better(ka, ia, kb, ib);
        if (swap) {
          s_k[i] = kb; s_k[l] = ka;
          s_i[i] = ib; s_i[l] = ia;
        }
      }
      __syncthreads();
    }
  }
}

// Workgroup (chunk, robot): the chunk's best T records for the robot.
// kPath (dm_assign_goals_path): the distance is the path length to the
// cluster's snapped centroid, cost_rows[r][c] * res / 5 (two rounded
// operations), and a cluster that is not reached is not eligible; `robots`
// is not read.
// kGain (dm_assign_goals_gain, with kPath): the numerator is the cluster's
// visible-unknown count gain_row[c] in place of its size, and a cluster with
// gain < min_gain is not eligible; a gain of 0 gives util 0, the key of "not
// eligible".
template <bool kPath, bool kGain>
__global__ __launch_bounds__(kGoalThreads) void k_goal_topk(const dm_cluster* __restrict__ recs, int64_t K,
                                                            const double* __restrict__ robots, int32_t T,
                                                            int64_t min_size, double w, double min_dist,
                                                            unsigned long long* __restrict__ out_k,
                                                            uint32_t* __restrict__ out_i,
                                                            const uint32_t* __restrict__ cost_rows, double res,
                                                            const uint32_t* __restrict__ gain_row,
                                                            int64_t min_gain) {
  __shared__ unsigned long long s_k[kGoalN];
  __shared__ uint32_t s_i[kGoalN];
  const int64_t chunk = blockIdx.x, r = blockIdx.y, nch = gridDim.x;
  const double rx = kPath ? 0.0 : robots[2 * r], ry = kPath ? 0.0 : robots[2 * r + 1];
  for (int e = threadIdx.x; e < kGoalN; e += kGoalThreads) {
    const int64_t c = chunk * kGoalN + e;
    unsigned long long key = 0ull;
    if (c < K) {
      const dm_cluster q = recs[c];
      double dist;
      bool reached = true;
      if (kPath) {
        const uint32_t pc = cost_rows[r * K + c];
        reached = pc != DM_PLAN_UNREACHABLE;
        dist = __ddiv_rn(__dmul_rn((double)pc, res), 5.0);
      } else {
        const double dx = q.cx_m - rx, dy = q.cy_m - ry;
        dist = __dsqrt_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)));
      }
      const uint32_t gain = kGain ? gain_row[c] : 0u;
      if (reached && q.size >= min_size && dist >= min_dist && (!kGain || (int64_t)gain >= min_gain)) {
        const double num = kGain ? (double)gain : (double)q.size;
        const double util = __ddiv_rn(num, __dadd_rn(1.0, __dmul_rn(w, dist)));
        key = (unsigned long long)__double_as_longlong(util);
      }
    }
    s_k[e] = key;
    s_i[e] = c < K ? (uint32_t)c : 0xFFFFFFFFu;
  }
  __syncthreads();
  goal_sort(s_k, s_i);
  for (int t = threadIdx.x; t < T; t += kGoalThreads) {
    const int64_t o = (r * nch + chunk) * T + t;
    out_k[o] = s_k[t];
    out_i[o] = s_i[t];
  }
}

// Workgroup (group, robot): merge `per` consecutive T-lists of the robot's
// nlists into one (the best T of their union).
__global__ __launch_bounds__(kGoalThreads) void k_goal_merge(const unsigned long long* __restrict__ in_k,
                                                             const uint32_t* __restrict__ in_i, int64_t nlists,
                                                             int32_t T, int32_t per,
                                                             unsigned long long* __restrict__ out_k,
                                                             uint32_t* __restrict__ out_i) {
  __shared__ unsigned long long s_k[kGoalN];
  __shared__ uint32_t s_i[kGoalN];
  const int64_t grp = blockIdx.x, r = blockIdx.y, ngrp = gridDim.x;
  const int64_t l0 = grp * per;
  const int64_t n = min((int64_t)per, nlists - l0) * T;
  for (int e = threadIdx.x; e < kGoalN; e += kGoalThreads) {
    const bool in = e < n;
    const int64_t src = (r * nlists + l0) * T + e;
    s_k[e] = in ? in_k[src] : 0ull;
    s_i[e] = in ? in_i[src] : 0xFFFFFFFFu;
  }
  __syncthreads();
  goal_sort(s_k, s_i);
  for (int t = threadIdx.x; t < T; t += kGoalThreads) {
    const int64_t o = (r * ngrp + grp) * T + t;
    out_k[o] = s_k[t];
    out_i[o] = s_i[t];
  }
}

// Centroids of the chosen records (idx < 0: none -> NaN).
__global__ void k_goal_gather(const dm_cluster* __restrict__ recs, const int64_t* __restrict__ idx, int32_t R,
                              double* __restrict__ xy) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= R) return;
  const int64_t c = idx[r];
  xy[2 * r] = c >= 0 ? recs[c].cx_m : __builtin_nan("");
  xy[2 * r + 1] = c >= 0 ? recs[c].cy_m : __builtin_nan("");
}

}  // namespace

int dm_launch_goal_gather(dm_grid* g, const dm_cluster* d_recs, const int64_t* d_idx, int32_t R, double* d_xy) {
  hipLaunchKernelGGL(k_goal_gather, dim3((R + 63) / 64), dim3(64), 0, g->stream, d_recs, d_idx, R, d_xy);
  DM_HIP(hipGetLastError());
  return DM_OK;
}

// Top-T lists of R robots over K label-sorted records; on return *d_k / *d_i
// point at the final [R][T] lists (in g->goal_* workspace).  T <= 256.
// d_cost: [R][K] path costs in place of the Euclidean distance (d_robots is
// then not read), or nullptr.  d_gain (with d_cost, R == 1): [K] gains, the
// numerator in place of the size, with min_gain; or nullptr.
int dm_launch_goal_topk(dm_grid* g, const dm_cluster* d_recs, int64_t K, const double* d_robots, int32_t R,
                        int32_t T, int64_t min_size, double w, double min_dist,
                        const unsigned long long** d_k, const uint32_t** d_i, const uint32_t* d_cost,
                        const uint32_t* d_gain, int64_t min_gain) {
  const int64_t nch = (K + kGoalN - 1) / kGoalN;
  const int64_t need = (int64_t)R * std::max<int64_t>(nch, 1) * T;
  if (need > g->goal_cap) {
    for (int b = 0; b < 2; ++b) {
      if (g->goal_k[b]) (void)hipFree(g->goal_k[b]);
      if (g->goal_i[b]) (void)hipFree(g->goal_i[b]);
      g->goal_k[b] = nullptr;
      g->goal_i[b] = nullptr;
    }
    g->goal_cap = 0;
    for (int b = 0; b < 2; ++b) {
      DM_HIP(hipMalloc((void**)&g->goal_k[b], sizeof(unsigned long long) * (size_t)need));
      DM_HIP(hipMalloc((void**)&g->goal_i[b], sizeof(uint32_t) * (size_t)need));
    }
    g->goal_cap = need;
  }
  int cur = 0;
  KernelTimer t;
  dm_timer_begin(g, "goal_topk", &t);
  const dim3 tgrid((unsigned)std::max<int64_t>(nch, 1), (unsigned)R);
  const uint32_t* const no_row = nullptr;
  if (d_cost && d_gain)
    hipLaunchKernelGGL((k_goal_topk<true, true>), tgrid, dim3(kGoalThreads), 0, g->stream, d_recs, K, d_robots, T,
                       min_size, w, min_dist, g->goal_k[0], g->goal_i[0], d_cost, g->p.resolution, d_gain, min_gain);
  else if (d_cost)
    hipLaunchKernelGGL((k_goal_topk<true, false>), tgrid, dim3(kGoalThreads), 0, g->stream, d_recs, K, d_robots, T,
                       min_size, w, min_dist, g->goal_k[0], g->goal_i[0], d_cost, g->p.resolution, no_row,
                       (int64_t)0);
  else
    hipLaunchKernelGGL((k_goal_topk<false, false>), tgrid, dim3(kGoalThreads), 0, g->stream, d_recs, K, d_robots, T,
                       min_size, w, min_dist, g->goal_k[0], g->goal_i[0], no_row, 0.0, no_row, (int64_t)0);
  DM_HIP(hipGetLastError());
  int64_t nl = std::max<int64_t>(nch, 1);
  const int32_t per = kGoalN / T;  // lists one merge workgroup takes (>= 16)
  while (nl > 1) {
    const int64_t ng = (nl + per - 1) / per;
    hipLaunchKernelGGL(k_goal_merge, dim3((unsigned)ng, (unsigned)R), dim3(kGoalThreads), 0, g->stream,
                       g->goal_k[cur], g->goal_i[cur], nl, T, per, g->goal_k[cur ^ 1], g->goal_i[cur ^ 1]);
    DM_HIP(hipGetLastError());
    cur ^= 1;
    nl = ng;
  }
  dm_timer_end(g, &t);
  *d_k = g->goal_k[cur];
  *d_i = g->goal_i[cur];
  return DM_OK;
}

// ---- path planning (dm_plan.h) ----------------------------------------------

int dm_plan_launch_travers(dm_grid* g, int32_t inflate_cells) {
  DM_HIP(hipMemsetAsync(g->plan_stat + dm_plan::ST_TRAV, 0, sizeof(unsigned long long), g->stream));
  KernelTimer t;
  dm_timer_begin(g, "plan_travers", &t);
  hipLaunchKernelGGL(dm_plan::k_plan_travers, dim3((unsigned)g->NT), dim3(dm_plan::kThreads), 0, g->stream,
                     g->state, g->tile_seen, g->W, g->H, g->TX, inflate_cells, g->plan_trav, g->plan_stat);
  DM_HIP(hipGetLastError());
  dm_timer_end(g, &t);
  return DM_OK;
}

int dm_plan_launch_expand(dm_grid* g, uint8_t* d_out) {
  const int64_t cells = g->W * g->H;
  hipLaunchKernelGGL(dm_plan::k_plan_expand, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, g->stream,
                     g->plan_trav, g->W, g->H, g->TX, d_out);
  DM_HIP(hipGetLastError());
  return DM_OK;
}

int dm_plan_run_field(dm_grid* g, const int64_t* cells, int32_t n, const int32_t* tiles, int32_t n_tiles,
                      uint32_t max_cost, uint64_t* stats) {
  using namespace dm_plan;
  const int64_t ncell = g->W * g->H;
  hipStream_t s = g->stream;
  DM_HIP(hipMemcpyAsync(g->plan_travs, g->plan_trav, sizeof(uint64_t) * (size_t)g->NT * DM_TILE,
                        hipMemcpyDeviceToDevice, s));
  DM_HIP(hipMemsetAsync(g->plan_cost, 0xFF, sizeof(uint32_t) * (size_t)ncell, s));
  DM_HIP(hipMemsetAsync(g->plan_stamp, 0, sizeof(uint32_t) * (size_t)g->NT, s));
  const unsigned long long zero3[3] = {0ull, 0ull, 0ull};
  DM_HIP(hipMemcpyAsync(g->plan_stat + ST_REACHED, zero3, sizeof(unsigned long long), hipMemcpyHostToDevice, s));
  DM_HIP(hipMemcpyAsync(g->plan_stat + ST_ROUNDS, zero3, 2 * sizeof(unsigned long long), hipMemcpyHostToDevice, s));
  const unsigned int len3[3] = {(unsigned int)n_tiles, 0u, 0u};
  DM_HIP(hipMemcpyAsync(g->plan_len, len3, sizeof len3, hipMemcpyHostToDevice, s));
  DM_HIP(hipMemcpyAsync(g->plan_src, cells, sizeof(int64_t) * (size_t)n, hipMemcpyHostToDevice, s));
  DM_HIP(hipMemcpyAsync(g->plan_list[0], tiles, sizeof(int32_t) * (size_t)n_tiles, hipMemcpyHostToDevice, s));
  for (int i = 0; i < 4; ++i) g->h_plan[i] = 0ull;
  hipLaunchKernelGGL(k_plan_sources, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, g->plan_src, n, g->W, g->TX,
                     g->plan_travs, g->plan_cost);
  DM_HIP(hipGetLastError());
  // Round bound.  Induction over rounds: after round k every cell whose
  // shortest path crosses at most k tile borders holds its final cost (round
  // k's visit of a tile relaxes it to its fixpoint against ring values that
  // were final after round k - 1, and a tile whose ring changed is on the
  // list).  A shortest path visits no cell twice, so it has fewer moves, and
  // crosses fewer tile borders, than there are traversable cells T (sources
  // included: T + n).  Two more rounds see the last lowered border cell's
  // neighbours find nothing to lower and the list run empty; a visit that
  // stops at its sweep bound (kMaxSweeps) lists its tile again, at most
  // 4096 / kMaxSweeps + 1 = 5 visits for one ring state.
  // The traversable count is on the host after the first wait; until then
  // the bound is the map's cell count.
  const auto bound_of = [&](unsigned long long trav) { return (int64_t)(5 * (trav + (unsigned long long)n) + 2); };
  int64_t bound = g->plan_max_rounds > 0 ? g->plan_max_rounds : bound_of((unsigned long long)ncell);
  // The list length comes back through mapped host memory, read after a wait
  // for the rounds enqueued so far; several rounds go out per wait (4, 8, 16,
  // ...: short fields end after one wait, long ones pay ~ one wait per 32
  // rounds), the launches after the list ran empty exit at once.
  const unsigned grid = (unsigned)std::min<int64_t>(g->NT, 4 * (int64_t)(g->n_cu > 0 ? g->n_cu : 256));
  int64_t done = 0;
  int batch = 4;
  bool empty = false;
  KernelTimer t;
  while (!empty && done < bound) {
    const int64_t nb = std::min<int64_t>(batch, bound - done);
    dm_timer_begin(g, "plan_relax", &t);
    for (int64_t k = 0; k < nb; ++k, ++done) {
      hipLaunchKernelGGL(k_plan_relax, dim3(grid), dim3(kThreads), 0, s, g->plan_cost, g->plan_travs, g->W, g->H,
                         g->TX, g->TY, max_cost, g->plan_list[done & 1], g->plan_list[(done + 1) & 1], g->plan_len,
                         g->plan_stamp, (uint32_t)done, g->plan_stat, g->h_plan_dev);
      DM_HIP(hipGetLastError());
    }
    dm_timer_end(g, &t);
    DM_HIP(hipStreamSynchronize(s));
    empty = g->h_plan[HS_LEN] == 0ull;
    if (g->plan_max_rounds <= 0) bound = std::min(bound, bound_of(g->h_plan[HS_TRAV]));
    batch = std::min(batch * 2, 32);
  }
  if (!empty) {  // the bound is reached: did the last round leave work?
    unsigned int len[3];
    DM_HIP(hipMemcpy(len, g->plan_len, sizeof len, hipMemcpyDeviceToHost));
    if (len[done % 3] != 0u)
      return dm_set_error(DM_ERR_INCOMPLETE, "the distance field did not settle within %lld rounds (%u tiles "
                          "still active)%s", (long long)bound, len[done % 3],
                          g->plan_max_rounds > 0 ? "; DM_PLAN_MAX_ROUNDS is set" : "");
  }
  if (stats) {
    hipLaunchKernelGGL(k_plan_count, dim3((unsigned)std::min<int64_t>((ncell + kThreads - 1) / kThreads, 1024)),
                       dim3(kThreads), 0, s, g->plan_cost, ncell, g->plan_stat);
    DM_HIP(hipGetLastError());
    unsigned long long st[4];
    DM_HIP(hipMemcpyAsync(st, g->plan_stat, sizeof st, hipMemcpyDeviceToHost, s));
    DM_HIP(hipStreamSynchronize(s));
    for (int i = 0; i < 4; ++i) stats[i] = st[i];
  }
  return DM_OK;
}

int dm_plan_launch_query(dm_grid* g, const double* d_xy, int64_t stride, int64_t n, int32_t snap_cells,
                         uint32_t* d_cost, int64_t* d_cell) {
  if (n <= 0) return DM_OK;
  KernelTimer t;
  dm_timer_begin(g, "plan_query", &t);
  hipLaunchKernelGGL(dm_plan::k_plan_query, dim3((unsigned)((n + 127) / 128)), dim3(128), 0, g->stream,
                     g->plan_cost, g->W, g->H, g->p.origin_x, g->p.origin_y, g->p.resolution, d_xy, stride, n,
                     snap_cells, d_cost, d_cell);
  DM_HIP(hipGetLastError());
  dm_timer_end(g, &t);
  return DM_OK;
}

int dm_plan_launch_path(dm_grid* g, const int64_t* d_start, int64_t cap) {
  KernelTimer t;
  dm_timer_begin(g, "plan_path", &t);
  hipLaunchKernelGGL(dm_plan::k_plan_path, dim3(1), dim3(64), 0, g->stream, g->plan_cost, g->plan_travs, g->W,
                     g->H, g->TX, d_start, g->plan_path, cap, g->plan_stat + 4);
  DM_HIP(hipGetLastError());
  dm_timer_end(g, &t);
  return DM_OK;
}

// ---- scan matcher (dm_match.h) ------------------------------------------------

int dm_match_launch_field(dm_grid* g, int32_t n_tiles, int32_t r, bool mono) {
  if (n_tiles <= 0) return DM_OK;
  KernelTimer t;
  dm_timer_begin(g, "match_field", &t);
  hipLaunchKernelGGL(dm_match::k_match_field, dim3((unsigned)n_tiles), dim3(dm_match::kThreads), 0, g->stream,
                     g->state, g->tile_seen, g->W, g->H, g->TX, r, g->match_kern, mono ? 1 : 0, g->match_tiles,
                     g->match_V);
  DM_HIP(hipGetLastError());
  dm_timer_end(g, &t);
  return DM_OK;
}

int dm_match_launch_scans(dm_grid* g, int32_t S, int32_t N, int32_t A, int32_t k0, int32_t sub, int32_t half,
                          int32_t stride) {
  using namespace dm_match;
  hipStream_t s = g->stream;
  const int64_t SA = (int64_t)S * A, T = (int64_t)(2 * half + 1) * (2 * half + 1);
  int32_t* d_used = g->match_out + 4 * (int64_t)S;
  DM_HIP(hipMemsetAsync(d_used, 0, sizeof(int32_t) * (size_t)S, s));
  DM_HIP(hipMemsetAsync(g->match_vol, 0, sizeof(uint32_t) * (size_t)(SA * T), s));
  KernelTimer t;
  if (N > 0) {
    MatchArgs a;
    a.N = N;
    a.ox = g->p.origin_x;
    a.oy = g->p.origin_y;
    a.step = g->p.resolution / (double)sub;
    a.range_min = g->p.range_min;
    a.range_max = g->p.range_max;
    dm_timer_begin(g, "match_prep", &t);
    hipLaunchKernelGGL(k_match_prep, dim3((unsigned)SA, (unsigned)((N + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                       s, a, g->match_pose4, g->match_ranges, g->match_trig, A, k0, g->match_q, d_used);
    DM_HIP(hipGetLastError());
    dm_timer_end(g, &t);
    // beam chunks: at least what one workgroup's LDS stage holds; more (down
    // to 32 beams each) while the candidate yaws alone leave the chip idle
    const int64_t want = (2048 + SA - 1) / SA;
    int64_t chunks = std::max<int64_t>((N + kBeamsPerChunk - 1) / kBeamsPerChunk,
                                       std::min<int64_t>(want, (N + 31) / 32));
    const int32_t chunk_len = (int32_t)((N + chunks - 1) / chunks);
    chunks = (N + chunk_len - 1) / chunk_len;
    dm_timer_begin(g, "match_score", &t);
    hipLaunchKernelGGL(k_match_score, dim3((unsigned)SA, (unsigned)chunks), dim3(kThreads), 0, s, g->match_q, N,
                       chunk_len, g->match_V, g->W, g->H, sub, half, stride, g->match_vol);
    DM_HIP(hipGetLastError());
    dm_timer_end(g, &t);
  }
  dm_timer_begin(g, "match_best", &t);
  hipLaunchKernelGGL(k_match_best, dim3((unsigned)S), dim3(kThreads), 0, s, g->match_vol, A, half, k0, g->match_out);
  DM_HIP(hipGetLastError());
  dm_timer_end(g, &t);
  return DM_OK;
}

// ---- whole-window relocalisation (dm_match_global.h) ---------------------------

int dm_mg_launch_pool(dm_grid* g, int32_t n_tiles, int32_t lb, int32_t EWB, int32_t EHB, int32_t PTX) {
  if (n_tiles <= 0) return DM_OK;
  KernelTimer t;
  dm_timer_begin(g, "mg_pool", &t);
  hipLaunchKernelGGL(dm_mg::k_mg_pool, dim3((unsigned)n_tiles), dim3(dm_mg::kThreads), 0, g->stream, g->match_V, g->W,
                     g->H, lb, EWB, EHB, PTX, g->mg_ptiles, g->mg_pool);
  DM_HIP(hipGetLastError());
  dm_timer_end(g, &t);
  return DM_OK;
}

int dm_mg_run_scan(dm_grid* g, const MgShape& sh, const double* d_pose4, const float* d_ranges, int32_t* res,
                   uint64_t* stats) {
  using namespace dm_mg;
  hipStream_t s = g->stream;
  Cand* best = (Cand*)g->mg_best;
  Cand* cand = (Cand*)g->mg_cand;
  const int32_t N = sh.N, A = sh.A, nb = sh.nbx * sh.nby;
  const int64_t blocks = (int64_t)A * nb;
  KernelTimer t;
  hipLaunchKernelGGL(k_mg_init, dim3(1), dim3(64), 0, s, best, sh.k0, g->mg_nused);
  DM_HIP(hipGetLastError());
  {
    MatchArgs a;
    a.N = N;
    a.ox = g->p.origin_x;
    a.oy = g->p.origin_y;
    a.step = g->p.resolution;  // sub = 1
    a.range_min = g->p.range_min;
    a.range_max = g->p.range_max;
    dm_timer_begin(g, "match_prep", &t);
    hipLaunchKernelGGL(dm_match::k_match_prep, dim3((unsigned)A, (unsigned)((N + kThreads - 1) / kThreads)),
                       dim3(dm_match::kThreads), 0, s, a, d_pose4, d_ranges, g->match_trig, A, sh.k0, g->match_q,
                       g->mg_nused);
    DM_HIP(hipGetLastError());
    dm_timer_end(g, &t);
  }
  uint64_t refined = 0, rounds = 0;
  if (sh.exhaustive) {
    for (int64_t base = 0; base < blocks; base += dm_grid::kMgExhaustiveBatch) {
      const int32_t n = (int32_t)std::min<int64_t>(dm_grid::kMgExhaustiveBatch, blocks - base);
      dm_timer_begin(g, "mg_refine", &t);
      hipLaunchKernelGGL(k_mg_refine, dim3((unsigned)n), dim3(kThreads), 0, s, g->match_q, N, g->match_V, g->W, g->H,
                         sh.lb, sh.half_x, sh.half_y, sh.nbx, nb, sh.k0, (const int32_t*)nullptr, (int32_t)base,
                         (const uint32_t*)nullptr, n, cand);
      DM_HIP(hipGetLastError());
      dm_timer_end(g, &t);
      dm_timer_begin(g, "mg_fold", &t);
      hipLaunchKernelGGL(k_mg_fold, dim3(1), dim3(kThreads), 0, s, cand, (const uint32_t*)nullptr, n, sh.k0, best,
                         g->mg_nused, g->h_mg_dev);
      DM_HIP(hipGetLastError());
      dm_timer_end(g, &t);
      refined += (uint64_t)n;
      ++rounds;
    }
    DM_HIP(hipStreamSynchronize(s));
  } else {
    dm_timer_begin(g, "mg_bound", &t);
    hipLaunchKernelGGL(k_mg_bound, dim3((unsigned)((nb + kThreads - 1) / kThreads), (unsigned)A), dim3(kThreads), 0, s,
                       g->match_q, N, g->mg_pool, sh.lb, sh.EWB, sh.EHB, sh.half_x, sh.half_y, sh.nbx, nb,
                       g->mg_bound);
    DM_HIP(hipGetLastError());
    dm_timer_end(g, &t);
    // rounds: the blocks whose bound reaches the best exact score so far (and
    // 1), the highest bounds first; few in the first round, when nothing is
    // known yet, then up to mg_batch
    const uint32_t hi = 255u * (uint32_t)N;
    const unsigned scan_grid = (unsigned)std::min<int64_t>((blocks + kThreads - 1) / kThreads, 2048);
    uint32_t s_best = 0;
    uint32_t cap = (uint32_t)std::min<int64_t>(g->mg_batch, 8);
    for (;;) {
      const uint32_t lo = std::max(s_best, 1u);
      DM_HIP(hipMemsetAsync(g->mg_hist, 0, sizeof(uint32_t) * kBins, s));
      dm_timer_begin(g, "mg_select", &t);
      hipLaunchKernelGGL(k_mg_hist, dim3(scan_grid), dim3(kThreads), 0, s, g->mg_bound, blocks, lo, hi, g->mg_hist);
      hipLaunchKernelGGL(k_mg_pick, dim3(1), dim3(kThreads), 0, s, g->mg_hist, cap, g->mg_ctl);
      hipLaunchKernelGGL(k_mg_compact, dim3(scan_grid), dim3(kThreads), 0, s, g->mg_bound, blocks, lo, hi, g->mg_ctl,
                         g->mg_list);
      DM_HIP(hipGetLastError());
      dm_timer_end(g, &t);
      dm_timer_begin(g, "mg_refine", &t);
      hipLaunchKernelGGL(k_mg_refine, dim3(cap), dim3(kThreads), 0, s, g->match_q, N, g->match_V, g->W, g->H, sh.lb,
                         sh.half_x, sh.half_y, sh.nbx, nb, sh.k0, g->mg_list, 0, g->mg_ctl, 0, cand);
      DM_HIP(hipGetLastError());
      dm_timer_end(g, &t);
      dm_timer_begin(g, "mg_fold", &t);
      hipLaunchKernelGGL(k_mg_fold, dim3(1), dim3(kThreads), 0, s, cand, g->mg_ctl, 0, sh.k0, best, g->mg_nused,
                         g->h_mg_dev);
      DM_HIP(hipGetLastError());
      dm_timer_end(g, &t);
      DM_HIP(hipStreamSynchronize(s));
      const uint32_t n = g->h_mg[4];
      if (n == 0) break;  // no unrefined block can reach the best score: it is exact
      refined += n;
      ++rounds;
      s_best = g->h_mg[0];
      cap = (uint32_t)std::min<int64_t>(g->mg_batch, (int64_t)cap * 4);
    }
  }
  res[0] = (int32_t)g->h_mg[1];
  res[1] = (int32_t)g->h_mg[2];
  res[2] = (int32_t)g->h_mg[3];
  res[3] = (int32_t)g->h_mg[0];
  res[4] = (int32_t)g->h_mg[5];
  stats[0] = (uint64_t)blocks;
  stats[1] = sh.exhaustive ? 0 : (uint64_t)blocks;
  stats[2] = refined;
  stats[3] = rounds;
  return DM_OK;
}

// ---- information gain (dm_gain.h) ---------------------------------------------

int dm_gain_launch_cells(dm_grid* g, int64_t n) {
  if (n <= 0) return DM_OK;
  hipLaunchKernelGGL(dm_gain::k_gain_cells, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, g->stream, g->gain_xy, n,
                     g->W, g->H, g->p.origin_x, g->p.origin_y, g->p.resolution, g->gain_cell);
  DM_HIP(hipGetLastError());
  return DM_OK;
}

int dm_gain_launch_skip(dm_grid* g, const dm_cluster* d_recs, const uint32_t* d_cost, int64_t K, int64_t min_size) {
  if (K <= 0) return DM_OK;
  hipLaunchKernelGGL(dm_gain::k_gain_skip, dim3((unsigned)((K + 255) / 256)), dim3(256), 0, g->stream, d_recs, d_cost,
                     K, min_size, g->gain_skip);
  DM_HIP(hipGetLastError());
  return DM_OK;
}

namespace {

// One launch of k_gain_views<., kMask, kCommit> over n views; the bitmap is
// dynamic LDS up to kDynBytes and the static form above.
template <bool kMask, bool kCommit>
void gain_launch(dm_grid* g, const int64_t* d_cell, const uint8_t* d_skip, int64_t n, int32_t R, int64_t* mc,
                 uint32_t* mg, uint32_t* d_out, uint32_t* d_claimed) {
  using namespace dm_gain;
  const size_t bytes = sizeof(uint32_t) * (size_t)bitmap_words(R);
  if (bytes <= (size_t)kDynBytes)
    hipLaunchKernelGGL((k_gain_views<false, kMask, kCommit>), dim3((unsigned)n), dim3(kThreads), bytes, g->stream,
                       g->state, (int32_t)g->W, (int32_t)g->H, d_cell, d_skip, R, mc, mg, d_out, d_claimed);
  else
    hipLaunchKernelGGL((k_gain_views<true, kMask, kCommit>), dim3((unsigned)n), dim3(kThreads), 0, g->stream,
                       g->state, (int32_t)g->W, (int32_t)g->H, d_cell, d_skip, R, mc, mg, d_out, d_claimed);
}

}  // namespace

int dm_gain_launch_views(dm_grid* g, const int64_t* d_cell, const uint8_t* d_skip, int64_t n, int32_t R, bool memo) {
  if (n <= 0) return DM_OK;
  int64_t* const mc = memo ? g->gain_memo_cell : nullptr;
  uint32_t* const mg = memo ? g->gain_memo_gain : nullptr;
  KernelTimer t;
  dm_timer_begin(g, "gain_views", &t);
  gain_launch<false, false>(g, d_cell, d_skip, n, R, mc, mg, g->gain_out, nullptr);
  DM_HIP(hipGetLastError());
  dm_timer_end(g, &t);
  return DM_OK;
}

int dm_gain_launch_marginal(dm_grid* g, const int64_t* d_cell, const uint8_t* d_skip, int64_t n, int32_t R,
                            bool memo) {
  if (n <= 0) return DM_OK;
  int64_t* const mc = memo ? g->gain_memo_cell : nullptr;
  uint32_t* const mg = memo ? g->gain_memo_gain : nullptr;
  KernelTimer t;
  dm_timer_begin(g, "gain_marginal", &t);
  gain_launch<true, false>(g, d_cell, d_skip, n, R, mc, mg, g->gain_out, g->gain_claimed);
  DM_HIP(hipGetLastError());
  dm_timer_end(g, &t);
  return DM_OK;
}

int dm_gain_launch_commit(dm_grid* g, const int64_t* d_cell, int64_t n, int32_t R) {
  if (n <= 0) return DM_OK;
  KernelTimer t;
  dm_timer_begin(g, "gain_commit", &t);
  gain_launch<false, true>(g, d_cell, nullptr, n, R, nullptr, nullptr, nullptr, g->gain_claimed);
  DM_HIP(hipGetLastError());
  dm_timer_end(g, &t);
  return DM_OK;
}

int dm_gain_launch_joint(dm_grid* g, const int64_t* d_cell, int64_t n, int32_t R, uint32_t* d_out) {
  if (n <= 0) return DM_OK;
  KernelTimer t;
  dm_timer_begin(g, "gain_joint", &t);
  // one view per launch: view i's marginal is against the views before it
  for (int64_t i = 0; i < n; ++i) {
    gain_launch<true, true>(g, d_cell + i, nullptr, 1, R, nullptr, nullptr, d_out + i, g->gain_claimed);
    DM_HIP(hipGetLastError());
  }
  dm_timer_end(g, &t);
  return DM_OK;
}

int dm_gain_launch_expand(dm_grid* g, uint8_t* d_out) {
  const int64_t cells = g->W * g->H;
  hipLaunchKernelGGL(dm_gain::k_gain_expand, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, g->stream,
                     g->gain_claimed, (int32_t)g->W, (int32_t)g->H, d_out);
  DM_HIP(hipGetLastError());
  return DM_OK;
}
