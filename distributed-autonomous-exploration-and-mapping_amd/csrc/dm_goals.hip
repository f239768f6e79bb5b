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
//
// The planner (dm_plan.h) and the information gain (dm_gain.h) live here too,
// kernels' launchers and entry points: dm_assign_goals_path, _gain and _coord
// are one loop (assign_goals_field) over a robot's distance field, the snapped
// cells of the cluster centroids, their gains and the same top-R lists.
// dm_plan_team* and dm_assign_goals_team (dm_plan.h §4) compute all robots'
// fields in the same rounds and pick the best (robot, cluster) pair first,
// from the same top-R lists of one launch.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "dm_gain.h"
#include "dm_internal.h"
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
// visible-unknown count gain_rows[r][c] in place of its size, and a cluster with
// gain < min_gain is not eligible; a gain of 0 gives util 0, the key of "not
// eligible".
template <bool kPath, bool kGain>
__global__ __launch_bounds__(kGoalThreads) void k_goal_topk(const dm_cluster* __restrict__ recs, int64_t K,
                                                            const double* __restrict__ robots, int32_t T,
                                                            int64_t min_size, double w, double min_dist,
                                                            unsigned long long* __restrict__ out_k,
                                                            uint32_t* __restrict__ out_i,
                                                            const uint32_t* __restrict__ cost_rows, double res,
                                                            const uint32_t* __restrict__ gain_rows,
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
      const uint32_t gain = kGain ? gain_rows[r * K + c] : 0u;
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

static int dm_launch_goal_gather(dm_grid* g, const dm_cluster* d_recs, const int64_t* d_idx, int32_t R, double* d_xy) {
  hipLaunchKernelGGL(k_goal_gather, dim3((R + 63) / 64), dim3(64), 0, g->stream, d_recs, d_idx, R, d_xy);
  DM_HIP(hipGetLastError());
  return DM_OK;
}

// Top-T lists of R robots over K label-sorted records; on return *d_k / *d_i
// point at the final [R][T] lists (in g->goal_* workspace).  T <= 256.
// d_cost: [R][K] path costs in place of the Euclidean distance (d_robots is
// then not read), or nullptr.  d_gain (with d_cost): [R][K] gains, the
// numerator in place of the size, with min_gain; or nullptr.
static int dm_launch_goal_topk(dm_grid* g, const dm_cluster* d_recs, int64_t K, const double* d_robots, int32_t R,
                               int32_t T, int64_t min_size, double w, double min_dist,
                               const unsigned long long** d_k, const uint32_t** d_i, const uint32_t* d_cost = nullptr,
                               const uint32_t* d_gain = nullptr, int64_t min_gain = 0) {
  const int64_t nch = (K + kGoalN - 1) / kGoalN;
  const int64_t need = (int64_t)R * std::max<int64_t>(nch, 1) * T;
  if (need > g->goal_i[1].size()) {  // the four lists have one size; goal_i[1] is allocated last
    for (int b = 0; b < 2; ++b) { g->goal_k[b].reset(); g->goal_i[b].reset(); }
    for (int b = 0; b < 2; ++b) {
      int rc = g->goal_k[b].alloc(need, "goal keys");
      if (rc || (rc = g->goal_i[b].alloc(need, "goal indices"))) return rc;
    }
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

static int dm_plan_launch_travers(dm_grid* g, int32_t inflate_cells) {
  DM_HIP(hipMemsetAsync(g->plan_stat + dm_plan::ST_TRAV, 0, sizeof(unsigned long long), g->stream));
  KernelTimer t;
  dm_timer_begin(g, "plan_travers", &t);
  hipLaunchKernelGGL(dm_plan::k_plan_travers, dim3((unsigned)g->NT), dim3(dm_plan::kThreads), 0, g->stream,
                     g->state, g->tile_seen, g->W, g->H, g->TX, inflate_cells, g->plan_trav, g->plan_stat);
  DM_HIP(hipGetLastError());
  dm_timer_end(g, &t);
  return DM_OK;
}

static int dm_plan_launch_expand(dm_grid* g, uint8_t* d_out) {
  const int64_t cells = g->W * g->H;
  hipLaunchKernelGGL(dm_plan::k_plan_expand, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, g->stream,
                     g->plan_trav, g->W, g->H, g->TX, d_out);
  DM_HIP(hipGetLastError());
  return DM_OK;
}

// clearance for clear_cells: d_pen_tab == nullptr: the uint16 d2 into d_d2; else
// the penalty bytes d_pen_tab[d2] into g->plan_pen
static int dm_plan_launch_clear(dm_grid* g, int32_t clear_cells, const uint8_t* d_pen_tab, uint16_t* d_d2) {
  KernelTimer t;
  dm_timer_begin(g, "plan_clear", &t);
  if (d_pen_tab)
    hipLaunchKernelGGL(dm_plan::k_plan_clear<true>, dim3((unsigned)g->NT), dim3(dm_plan::kThreads), 0, g->stream,
                       g->state, g->tile_seen, g->W, g->H, g->TX, clear_cells, d_pen_tab, nullptr, g->plan_pen);
  else
    hipLaunchKernelGGL(dm_plan::k_plan_clear<false>, dim3((unsigned)g->NT), dim3(dm_plan::kThreads), 0, g->stream,
                       g->state, g->tile_seen, g->W, g->H, g->TX, clear_cells, nullptr, d_d2, nullptr);
  DM_HIP(hipGetLastError());
  dm_timer_end(g, &t);
  return DM_OK;
}

// What the rounds of a relaxation work on: the single field's members of
// dm_grid (plan_*) or the team's (team_*), and the two nouns of its error text.
struct PlanRounds {
  int32_t* list[2];
  unsigned int* len;
  uint32_t* stamp;
  unsigned long long* stat;
  const unsigned long long* host;      // the mapped words (dm_plan::HS_*) as the host reads them
  volatile unsigned long long* hstat;  // and as k_plan_relax writes them
  const char* what;                    // "distance field" / "team fields"
  const char* items;                   // "tiles" / "(field, tile) items"
};

// The rounds of one relaxation, until the list runs empty; synchronous.
// n_src: the sources of one field (the bound).  max_items: the longest list
// there can be.  launch(round, grid): one round, k_plan_relax<., .> reading
// r.list[round & 1] and appending to r.list[(round + 1) & 1].
template <class Launch>
static int dm_plan_run_rounds(dm_grid* g, const PlanRounds& r, int32_t n_src, int64_t max_items, const char* timer,
                              Launch launch) {
  using namespace dm_plan;
  // Round bound.  Induction over rounds: after round k every cell whose
  // shortest path crosses at most k tile borders holds its final cost (round
  // k's visit of a tile relaxes it to its fixpoint against ring values that
  // were final after round k - 1, and a tile whose ring changed is on the
  // list).  A shortest path visits no cell twice, so it has fewer moves, and
  // crosses fewer tile borders, than there are traversable cells T (sources
  // included: T + n_src).  Two more rounds see the last lowered border cell's
  // neighbours find nothing to lower and the list run empty; a visit that
  // stops at its sweep bound (kMaxSweeps) lists its tile again, at most
  // 4096 / kMaxSweeps + 1 = 5 visits for one ring state.  The team's fields
  // settle side by side, each under this bound with its one source, so the
  // team's rounds are the slowest field's.
  // The traversable count is on the host after the first wait; until then
  // the bound is the map's cell count.
  const auto bound_of = [&](unsigned long long trav) { return (int64_t)(5 * (trav + (unsigned long long)n_src) + 2); };
  int64_t bound = g->plan_max_rounds > 0 ? g->plan_max_rounds : bound_of((unsigned long long)(g->W * g->H));
  // A visit holds 23.5 KB of LDS (6 workgroups in a CU's 160 KiB) and 4 waves
  // of 112 VGPRs (4 waves per SIMD; the weighted kernel's 160 give 3):
  // registers bound it at 4 resident workgroups per CU, the grid.  One field's
  // list rarely fills that; with n fields the items of a round spread over
  // all of it.
  const unsigned grid = (unsigned)std::min<int64_t>(max_items, 4 * (int64_t)(g->n_cu > 0 ? g->n_cu : 256));
  // The list length comes back through mapped host memory, read after a wait
  // for the rounds enqueued so far; several rounds go out per wait (4, 8, 16,
  // ...: short fields end after one wait, long ones pay ~ one wait per 32
  // rounds), the launches after the list ran empty exit at once.
  int64_t done = 0;
  int batch = 4;
  bool empty = false;
  KernelTimer t;
  while (!empty && done < bound) {
    const int64_t nb = std::min<int64_t>(batch, bound - done);
    dm_timer_begin(g, timer, &t);
    for (int64_t k = 0; k < nb; ++k, ++done) {
      launch((uint32_t)done, grid);
      DM_HIP(hipGetLastError());
    }
    dm_timer_end(g, &t);
    DM_HIP(hipStreamSynchronize(g->stream));
    empty = r.host[HS_LEN] == 0ull;
    if (g->plan_max_rounds <= 0) bound = std::min(bound, bound_of(r.host[HS_TRAV]));
    batch = std::min(batch * 2, 32);
  }
  if (!empty) {  // the bound is reached: did the last round leave work?
    unsigned int len[3];
    DM_HIP(hipMemcpy(len, r.len, sizeof len, hipMemcpyDeviceToHost));
    if (len[done % 3] != 0u)
      return dm_set_error(DM_ERR_INCOMPLETE, "the %s did not settle within %lld rounds (%u %s still active)%s", r.what,
                          (long long)bound, len[done % 3], r.items,
                          g->plan_max_rounds > 0 ? "; DM_PLAN_MAX_ROUNDS is set" : "");
  }
  return DM_OK;
}

// The field from n source cells (host arrays: cells, and their distinct
// tiles) over g->plan_trav; synchronous.  stats: [4] or nullptr.  weighted:
// by k_plan_relax<true, false> over g->plan_pen.
static int dm_plan_run_field(dm_grid* g, const int64_t* cells, int32_t n, const int32_t* tiles, int32_t n_tiles,
                      uint32_t max_cost, uint64_t* stats, bool weighted) {
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
  const PlanRounds r = {{g->plan_list[0], g->plan_list[1]}, g->plan_len, g->plan_stamp, g->plan_stat, g->h_plan,
                        g->h_plan.dev(), "distance field", "tiles"};
  const auto kernel = weighted ? k_plan_relax<true, false> : k_plan_relax<false, false>;
  const char* const timer = weighted ? "plan_relax_w" : "plan_relax";
  int rc = dm_plan_run_rounds(g, r, n, g->NT, timer, [&](uint32_t k, unsigned grid) {
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(kThreads), 0, s, g->plan_cost, g->plan_travs,
                       weighted ? g->plan_pen : nullptr, nullptr, g->W, g->H, g->TX, g->TY, max_cost, r.list[k & 1],
                       r.list[(k + 1) & 1], r.len, r.stamp, k, r.stat, r.hstat);
  });
  if (rc) return rc;
  if (stats) {
    hipLaunchKernelGGL(k_plan_team_count, dim3((unsigned)std::min<int64_t>((ncell + kThreads - 1) / kThreads, 1024)),
                       dim3(kThreads), 0, s, g->plan_cost, ncell, g->plan_stat + ST_REACHED);
    DM_HIP(hipGetLastError());
    unsigned long long st[4];
    DM_HIP(hipMemcpyAsync(st, g->plan_stat, sizeof st, hipMemcpyDeviceToHost, s));
    DM_HIP(hipStreamSynchronize(s));
    for (int i = 0; i < 4; ++i) stats[i] = st[i];
  }
  return DM_OK;
}

// snap n targets (d_xy, `stride` doubles apart) to the nr fields at d_field: [nr][n] into d_cost / d_cell
static int dm_plan_launch_snap(dm_grid* g, const char* timer, const uint32_t* d_field, int32_t nr, const double* d_xy,
                               int64_t stride, int64_t n, int32_t snap_cells, uint32_t* d_cost, int64_t* d_cell) {
  if (n <= 0 || nr <= 0) return DM_OK;
  KernelTimer t;
  dm_timer_begin(g, timer, &t);
  hipLaunchKernelGGL(dm_plan::k_plan_team_query, dim3((unsigned)((n * nr + 127) / 128)), dim3(128), 0, g->stream,
                     d_field, nr, g->W, g->H, g->p.origin_x, g->p.origin_y, g->p.resolution, d_xy, stride, n,
                     snap_cells, d_cost, d_cell);
  DM_HIP(hipGetLastError());
  dm_timer_end(g, &t);
  return DM_OK;
}

// to the handle's single field
static int dm_plan_launch_query(dm_grid* g, const double* d_xy, int64_t stride, int64_t n, int32_t snap_cells,
                         uint32_t* d_cost, int64_t* d_cell) {
  return dm_plan_launch_snap(g, "plan_query", g->plan_cost, 1, d_xy, stride, n, snap_cells, d_cost, d_cell);
}

// walk back from *d_start into g->plan_path (cap entries) by the rule of the
// field the handle holds; length and error word go to g->plan_stat[4], [5]
static int dm_plan_launch_path(dm_grid* g, const int64_t* d_start, int64_t cap) {
  KernelTimer t;
  dm_timer_begin(g, "plan_path", &t);
  if (g->plan_weighted)
    hipLaunchKernelGGL(dm_plan::k_plan_path<true>, dim3(1), dim3(64), 0, g->stream, g->plan_cost, g->plan_travs,
                       g->plan_pen, g->W, g->H, g->TX, d_start, g->plan_path, cap, g->plan_stat + 4);
  else
    hipLaunchKernelGGL(dm_plan::k_plan_path<false>, dim3(1), dim3(64), 0, g->stream, g->plan_cost, g->plan_travs,
                       nullptr, g->W, g->H, g->TX, d_start, g->plan_path, cap, g->plan_stat + 4);
  DM_HIP(hipGetLastError());
  dm_timer_end(g, &t);
  return DM_OK;
}

// ---- team fields (dm_plan.h §4) -------------------------------------------------

// device order of g->team_stat behind plan_stat's four words
enum { TEAM_ST_PATH = 4, TEAM_ST_REACHED = 8, TEAM_ST_N = TEAM_ST_REACHED + DM_PLAN_TEAM_MAX };

// The n fields from the source cells (host array) over g->team_trav, which
// this computes for inflate_cells; synchronous.  stats: [3 + n] or nullptr.
static int dm_plan_run_team(dm_grid* g, const int64_t* cells, int32_t n, int32_t inflate_cells, uint32_t max_cost,
                            uint64_t* stats) {
  using namespace dm_plan;
  const int64_t ncell = g->W * g->H;
  hipStream_t s = g->stream;
  DM_HIP(hipMemsetAsync(g->team_stat, 0, sizeof(unsigned long long) * TEAM_ST_N, s));
  KernelTimer t;
  dm_timer_begin(g, "plan_team_travers", &t);
  hipLaunchKernelGGL(k_plan_travers, dim3((unsigned)g->NT), dim3(kThreads), 0, s, g->state, g->tile_seen, g->W, g->H,
                     g->TX, inflate_cells, g->team_trav, g->team_stat);
  DM_HIP(hipGetLastError());
  dm_timer_end(g, &t);
  DM_HIP(hipMemsetAsync(g->team_cost, 0xFF, sizeof(uint32_t) * (size_t)n * (size_t)ncell, s));
  DM_HIP(hipMemsetAsync(g->team_stamp, 0, sizeof(uint32_t) * (size_t)n * (size_t)g->NT, s));
  const unsigned int len3[3] = {(unsigned int)n, 0u, 0u};
  DM_HIP(hipMemcpyAsync(g->team_len, len3, sizeof len3, hipMemcpyHostToDevice, s));
  DM_HIP(hipMemcpyAsync(g->team_src, cells, sizeof(int64_t) * (size_t)n, hipMemcpyHostToDevice, s));
  for (int i = 0; i < 4; ++i) g->h_team[i] = 0ull;
  dm_timer_begin(g, "plan_team_seed", &t);
  hipLaunchKernelGGL(k_plan_team_seed, dim3(1), dim3(DM_PLAN_TEAM_MAX), 0, s, g->team_src, n, g->W, g->TX, g->NT,
                     ncell, g->team_cost, g->team_list[0]);
  DM_HIP(hipGetLastError());
  dm_timer_end(g, &t);
  const PlanRounds r = {{g->team_list[0], g->team_list[1]}, g->team_len, g->team_stamp, g->team_stat, g->h_team,
                        g->h_team.dev(), "team fields", "(field, tile) items"};
  int rc = dm_plan_run_rounds(g, r, 1, (int64_t)n * g->NT, "plan_team_relax", [&](uint32_t k, unsigned grid) {
    hipLaunchKernelGGL((k_plan_relax<false, true>), dim3(grid), dim3(kThreads), 0, s, g->team_cost, g->team_trav,
                       nullptr, g->team_src, g->W, g->H, g->TX, g->TY, max_cost, r.list[k & 1], r.list[(k + 1) & 1],
                       r.len, r.stamp, k, r.stat, r.hstat);
  });
  if (rc) return rc;
  if (stats) {
    dm_timer_begin(g, "plan_team_count", &t);
    hipLaunchKernelGGL(k_plan_team_count,
                       dim3((unsigned)std::min<int64_t>((ncell + kThreads - 1) / kThreads, 1024), (unsigned)n),
                       dim3(kThreads), 0, s, g->team_cost, ncell, g->team_stat + TEAM_ST_REACHED);
    DM_HIP(hipGetLastError());
    dm_timer_end(g, &t);
    unsigned long long st[TEAM_ST_N];
    DM_HIP(hipMemcpyAsync(st, g->team_stat, sizeof st, hipMemcpyDeviceToHost, s));
    DM_HIP(hipStreamSynchronize(s));
    stats[0] = st[ST_TRAV];
    stats[1] = st[ST_ROUNDS];
    stats[2] = st[ST_RELAX];
    for (int32_t k = 0; k < n; ++k) stats[3 + k] = st[TEAM_ST_REACHED + k];
  }
  return DM_OK;
}

// to fields [r0, r0 + nr) of the team
static int dm_plan_launch_team_query(dm_grid* g, int32_t r0, int32_t nr, const double* d_xy, int64_t stride, int64_t n,
                                     int32_t snap_cells, uint32_t* d_cost, int64_t* d_cell) {
  return dm_plan_launch_snap(g, "plan_team_query", g->team_cost + (int64_t)r0 * g->W * g->H, nr, d_xy, stride, n,
                             snap_cells, d_cost, d_cell);
}

// walk back from *d_start on field `robot` into g->plan_path (cap entries):
// k_plan_path<false> on the layer, over a copy of the team's bit rows that
// holds this robot's source bit; length and error word go to g->team_stat[4], [5]
static int dm_plan_launch_team_path(dm_grid* g, int32_t robot, const int64_t* d_start, int64_t cap) {
  uint32_t* const layer = g->team_cost + (int64_t)robot * g->W * g->H;
  DM_HIP(hipMemcpyAsync(g->team_travp, g->team_trav, sizeof(uint64_t) * (size_t)g->NT * DM_TILE,
                        hipMemcpyDeviceToDevice, g->stream));
  KernelTimer t;
  dm_timer_begin(g, "plan_team_path", &t);
  // the source's bit (and its cost 0 once more, which the layer holds already)
  hipLaunchKernelGGL(dm_plan::k_plan_sources, dim3(1), dim3(64), 0, g->stream, g->team_src + robot, 1, g->W, g->TX,
                     g->team_travp, layer);
  DM_HIP(hipGetLastError());
  hipLaunchKernelGGL(dm_plan::k_plan_path<false>, dim3(1), dim3(64), 0, g->stream, layer, g->team_travp, nullptr, g->W,
                     g->H, g->TX, d_start, g->plan_path, cap, g->team_stat + TEAM_ST_PATH);
  DM_HIP(hipGetLastError());
  dm_timer_end(g, &t);
  return DM_OK;
}

// ---- information gain (dm_gain.h) ---------------------------------------------

// cells of n view points in g->gain_xy into g->gain_cell
static int dm_gain_launch_cells(dm_grid* g, int64_t n) {
  if (n <= 0) return DM_OK;
  hipLaunchKernelGGL(dm_gain::k_gain_cells, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, g->stream, g->gain_xy, n,
                     g->W, g->H, g->p.origin_x, g->p.origin_y, g->p.resolution, g->gain_cell);
  DM_HIP(hipGetLastError());
  return DM_OK;
}

// skip flags of K clusters (size < min_size or d_cost unreachable) into g->gain_skip
static int dm_gain_launch_skip(dm_grid* g, const dm_cluster* d_recs, const uint32_t* d_cost, int64_t K, int64_t min_size) {
  if (K <= 0) return DM_OK;
  hipLaunchKernelGGL(dm_gain::k_gain_skip, dim3((unsigned)((K + 255) / 256)), dim3(256), 0, g->stream, d_recs, d_cost,
                     K, min_size, g->gain_skip);
  DM_HIP(hipGetLastError());
  return DM_OK;
}

// the same for R robots' rows of costs d_cost[R][K]: R * K flags into g->gain_skip
static int dm_gain_launch_skip_team(dm_grid* g, const dm_cluster* d_recs, const uint32_t* d_cost, int64_t K, int32_t R,
                                    int64_t min_size) {
  const int64_t n = K * R;
  if (n <= 0) return DM_OK;
  hipLaunchKernelGGL(dm_gain::k_gain_skip_team, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, g->stream, d_recs,
                     d_cost, K, n, min_size, g->gain_skip);
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

// gains of n view cells into g->gain_out; d_skip and the memo (g->gain_memo_*) are optional
static int dm_gain_launch_views(dm_grid* g, const int64_t* d_cell, const uint8_t* d_skip, int64_t n, int32_t R, bool memo) {
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

// The overlap-aware forms, over the claimed set g->gain_claimed:
// marginal gains of n view cells into g->gain_out, reading the claimed set only
static int dm_gain_launch_marginal(dm_grid* g, const int64_t* d_cell, const uint8_t* d_skip, int64_t n, int32_t R,
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

// the n views' visible sets into the claimed set, in one launch; reports nothing
static int dm_gain_launch_commit(dm_grid* g, const int64_t* d_cell, int64_t n, int32_t R) {
  if (n <= 0) return DM_OK;
  KernelTimer t;
  dm_timer_begin(g, "gain_commit", &t);
  gain_launch<false, true>(g, d_cell, nullptr, n, R, nullptr, nullptr, nullptr, g->gain_claimed);
  DM_HIP(hipGetLastError());
  dm_timer_end(g, &t);
  return DM_OK;
}

// view i's marginal gain into d_out[i], then its commit, for i = 0..n-1 in order (one launch each)
static int dm_gain_launch_joint(dm_grid* g, const int64_t* d_cell, int64_t n, int32_t R, uint32_t* d_out) {
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

// the claimed set as H * W bytes
static int dm_gain_launch_expand(dm_grid* g, uint8_t* d_out) {
  const int64_t cells = g->W * g->H;
  hipLaunchKernelGGL(dm_gain::k_gain_expand, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, g->stream,
                     g->gain_claimed, (int32_t)g->W, (int32_t)g->H, d_out);
  DM_HIP(hipGetLastError());
  return DM_OK;
}

extern "C" {

// ---- path planning (csrc/dm_plan.h): traversability, distance field, snapped
// queries, paths, path-length goals ---------------------------------------------

static int ensure_plan(dm_grid* g) {
  if (g->plan_cost) return DM_OK;  // allocated last: everything else is there too
  int rc = DM_OK;
  if (!g->h_plan && (rc = g->h_plan.alloc_zeroed(16, hipHostMallocMapped | hipHostMallocCoherent, "plan rounds")))
    return rc;
  const int64_t rows = g->NT * DM_TILE;
  if ((rc = g->plan_trav.alloc(rows, "traversable bit rows"))) return rc;
  if ((rc = g->plan_travs.alloc(rows, "traversable bit rows with sources"))) return rc;
  if ((rc = g->plan_list[0].alloc(g->NT, "plan tile list"))) return rc;
  if ((rc = g->plan_list[1].alloc(g->NT, "plan tile list"))) return rc;
  if ((rc = g->plan_stamp.alloc(g->NT, "plan tile stamps"))) return rc;
  if ((rc = g->plan_len.alloc(4, "plan list lengths"))) return rc;
  if ((rc = g->plan_stat.alloc_zeroed(8, "plan statistics"))) return rc;
  if ((rc = g->plan_src.alloc(256, "plan sources"))) return rc;
  return g->plan_cost.alloc(g->W * g->H, "distance field");
}

static int grow_plan_query(dm_grid* g, int64_t n) {
  if (n <= g->plan_qcap) return DM_OK;
  return g->plan_qcap.grow(n, [&] {
    int rc = g->plan_qxy.alloc(2 * n, "plan query targets");
    if (!rc) rc = g->plan_qcost.alloc(n, "plan query costs");
    if (!rc) rc = g->plan_qcell.alloc(n, "plan query cells");
    return rc;
  });
}

// SPEC a4's cell of a point: floor((x - origin) / resolution) per axis
static bool plan_cell_of(const dm_grid* g, double x, double y, int64_t* cell) {
  const double fx = floor((x - g->p.origin_x) / g->p.resolution);
  const double fy = floor((y - g->p.origin_y) / g->p.resolution);
  if (!(fx >= 0.0 && fx < (double)g->W && fy >= 0.0 && fy < (double)g->H)) return false;  // NaN too
  *cell = (int64_t)fy * g->W + (int64_t)fx;
  return true;
}

static int plan_need_field(const dm_grid* g, const char* what) {
  if (!g->plan_cost || !g->plan_valid)
    return dm_set_error(DM_ERR_STATE, "%s: no distance field (call dm_plan_field first)", what);
  if (g->plan_version != dm_map_version(g))
    return dm_set_error(DM_ERR_STATE, "%s: the map changed since the distance field was computed (call "
                        "dm_plan_field again)", what);
  return DM_OK;
}

// The field from n sources (metres) over g->plan_trav, which the caller
// computed; weighted: over g->plan_pen too (dm_plan_field_cost).
static int plan_field_from(dm_grid* g, const double* sources_xy, int32_t n, uint32_t max_cost, uint64_t* stats,
                           bool weighted = false) {
  std::vector<int64_t> cells((size_t)n);
  std::vector<int32_t> tiles;
  for (int32_t i = 0; i < n; ++i) {
    if (!plan_cell_of(g, sources_xy[2 * i], sources_xy[2 * i + 1], &cells[(size_t)i]))
      return dm_set_error(DM_ERR_INVALID_ARG, "source %d (%g, %g) is outside the grid", i, sources_xy[2 * i],
                          sources_xy[2 * i + 1]);
    const int64_t x = cells[(size_t)i] % g->W, y = cells[(size_t)i] / g->W;
    const int32_t t = (int32_t)((y / DM_TILE) * g->TX + x / DM_TILE);
    if (std::find(tiles.begin(), tiles.end(), t) == tiles.end()) tiles.push_back(t);
  }
  const uint32_t cap = weighted ? DM_PLAN_COST_MAX : 0xFFFFFFEFu;
  if (max_cost == 0u || max_cost > cap) max_cost = cap;
  g->plan_valid = false;
  int rc = dm_plan_run_field(g, cells.data(), n, tiles.data(), (int32_t)tiles.size(), max_cost, stats, weighted);
  if (rc) return rc;
  g->plan_weighted = weighted;
  g->plan_valid = true;
  g->plan_version = dm_map_version(g);
  return DM_OK;
}

static int plan_check_inflate(int32_t inflate_cells) {
  if (inflate_cells < 0 || inflate_cells > 32)
    return dm_set_error(DM_ERR_INVALID_ARG, "inflate_cells must be in [0, 32] (got %d)", inflate_cells);
  return DM_OK;
}

static int plan_check_snap(int32_t snap_cells) {
  if (snap_cells < 0 || snap_cells > 16)
    return dm_set_error(DM_ERR_INVALID_ARG, "snap_cells must be in [0, 16] (got %d)", snap_cells);
  return DM_OK;
}

int dm_plan_traversable(dm_grid* g, int32_t inflate_cells, uint8_t* out) {
  int rc = dm_check_whole_map(g, "dm_plan_traversable");
  if (rc || (rc = use_device(g))) return rc;
  if (!out) return dm_set_error(DM_ERR_INVALID_ARG, "out is NULL");
  if ((rc = plan_check_inflate(inflate_cells)) || (rc = ensure_plan(g))) return rc;
  DM_HIP(dm_join_pass_stream(g));
  const int64_t cells = g->W * g->H;
  DevBuf<uint8_t> d;
  if ((rc = d.alloc(cells, "traversable image"))) return rc;
  if ((rc = dm_plan_launch_travers(g, inflate_cells)) || (rc = dm_plan_launch_expand(g, d))) return rc;
  hipError_t e = hipMemcpyAsync(out, d, (size_t)cells, hipMemcpyDeviceToHost, g->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(g->stream);
  if (e != hipSuccess) return dm_hip_check(e, "dm_plan_traversable");
  return DM_OK;
}

int dm_plan_field(dm_grid* g, const double* sources_xy, int32_t n_sources, int32_t inflate_cells,
                  uint32_t max_cost, uint64_t* out_stats) {
  int rc = dm_check_whole_map(g, "dm_plan_field");
  if (rc || (rc = use_device(g))) return rc;
  if (n_sources < 1 || n_sources > 256)
    return dm_set_error(DM_ERR_INVALID_ARG, "n_sources must be in [1, 256] (got %d)", n_sources);
  if (!sources_xy) return dm_set_error(DM_ERR_INVALID_ARG, "sources_xy is NULL");
  if ((rc = plan_check_inflate(inflate_cells)) || (rc = ensure_plan(g))) return rc;
  DM_HIP(dm_join_pass_stream(g));
  if ((rc = dm_plan_launch_travers(g, inflate_cells))) return rc;
  return plan_field_from(g, sources_xy, n_sources, max_cost, out_stats);
}

static int plan_check_clear(int32_t clear_cells) {
  if (clear_cells < 1 || clear_cells > 32)
    return dm_set_error(DM_ERR_INVALID_ARG, "clear_cells must be in [1, 32] (got %d)", clear_cells);
  return DM_OK;
}

int dm_plan_clearance(dm_grid* g, int32_t clear_cells, uint16_t* out) {
  int rc = dm_check_whole_map(g, "dm_plan_clearance");
  if (rc || (rc = use_device(g))) return rc;
  if (!out) return dm_set_error(DM_ERR_INVALID_ARG, "out is NULL");
  if ((rc = plan_check_clear(clear_cells))) return rc;
  DM_HIP(dm_join_pass_stream(g));
  const int64_t cells = g->W * g->H;
  DevBuf<uint16_t> d;
  if ((rc = d.alloc(cells, "clearance image"))) return rc;
  if ((rc = dm_plan_launch_clear(g, clear_cells, nullptr, d))) return rc;
  hipError_t e = hipMemcpyAsync(out, d, sizeof(uint16_t) * (size_t)cells, hipMemcpyDeviceToHost, g->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(g->stream);
  if (e != hipSuccess) return dm_hip_check(e, "dm_plan_clearance");
  return DM_OK;
}

int dm_plan_field_cost(dm_grid* g, const double* sources_xy, int32_t n_sources, int32_t inflate_cells,
                       int32_t clear_cells, const uint8_t* pen, uint32_t max_cost, uint64_t* out_stats) {
  int rc = dm_check_whole_map(g, "dm_plan_field_cost");
  if (rc || (rc = use_device(g))) return rc;
  if (n_sources < 1 || n_sources > 256)
    return dm_set_error(DM_ERR_INVALID_ARG, "n_sources must be in [1, 256] (got %d)", n_sources);
  if (!sources_xy) return dm_set_error(DM_ERR_INVALID_ARG, "sources_xy is NULL");
  if (!pen) return dm_set_error(DM_ERR_INVALID_ARG, "pen is NULL");
  if ((rc = plan_check_inflate(inflate_cells)) || (rc = plan_check_clear(clear_cells))) return rc;
  g->plan_valid = false;  // an allocation that fails below leaves no field
  if ((rc = ensure_plan(g))) return rc;
  if (!g->plan_pen && (rc = g->plan_pen.alloc(g->W * g->H, "cell penalties"))) return rc;
  if (!g->plan_pen_tab && (rc = g->plan_pen_tab.alloc(32 * 32 + 2, "penalty table"))) return rc;
  DM_HIP(dm_join_pass_stream(g));
  // pen is the caller's: on the device before this call returns (the field's wait at the latest)
  DM_HIP(hipMemcpyAsync(g->plan_pen_tab, pen, (size_t)(clear_cells * clear_cells + 2), hipMemcpyHostToDevice,
                        g->stream));
  if ((rc = dm_plan_launch_clear(g, clear_cells, g->plan_pen_tab, nullptr))) return rc;
  if ((rc = dm_plan_launch_travers(g, inflate_cells))) return rc;
  return plan_field_from(g, sources_xy, n_sources, max_cost, out_stats, true);
}

int dm_plan_get_field(dm_grid* g, uint32_t* out) {
  int rc = dm_check_whole_map(g, "dm_plan_get_field");
  if (rc || (rc = use_device(g))) return rc;
  if (!out) return dm_set_error(DM_ERR_INVALID_ARG, "out is NULL");
  if ((rc = plan_need_field(g, "dm_plan_get_field"))) return rc;
  DM_HIP(hipMemcpyAsync(out, g->plan_cost, sizeof(uint32_t) * (size_t)(g->W * g->H), hipMemcpyDeviceToHost,
                        g->stream));
  DM_HIP(hipStreamSynchronize(g->stream));
  return DM_OK;
}

int dm_plan_query(dm_grid* g, const double* targets_xy, int64_t n, int32_t snap_cells, uint32_t* out_cost,
                  int64_t* out_cell) {
  int rc = dm_check_whole_map(g, "dm_plan_query");
  if (rc || (rc = use_device(g))) return rc;
  if (n < 0) return dm_set_error(DM_ERR_INVALID_ARG, "n must be >= 0");
  if (n > 0 && (!targets_xy || !out_cost || !out_cell))
    return dm_set_error(DM_ERR_INVALID_ARG, "targets_xy / out_cost / out_cell is NULL");
  if ((rc = plan_check_snap(snap_cells)) || (rc = plan_need_field(g, "dm_plan_query"))) return rc;
  if (n == 0) return DM_OK;
  if ((rc = grow_plan_query(g, n))) return rc;
  DM_HIP(hipMemcpyAsync(g->plan_qxy, targets_xy, sizeof(double) * 2 * (size_t)n, hipMemcpyHostToDevice, g->stream));
  if ((rc = dm_plan_launch_query(g, g->plan_qxy, 2, n, snap_cells, g->plan_qcost, g->plan_qcell))) return rc;
  DM_HIP(hipMemcpyAsync(out_cost, g->plan_qcost, sizeof(uint32_t) * (size_t)n, hipMemcpyDeviceToHost, g->stream));
  DM_HIP(hipMemcpyAsync(out_cell, g->plan_qcell, sizeof(int64_t) * (size_t)n, hipMemcpyDeviceToHost, g->stream));
  DM_HIP(hipStreamSynchronize(g->stream));
  return DM_OK;
}

int dm_plan_path(dm_grid* g, double tx, double ty, int32_t snap_cells, int64_t* out_cells, int64_t cap,
                 int64_t* n_out) {
  int rc = dm_check_whole_map(g, "dm_plan_path");
  if (rc || (rc = use_device(g))) return rc;
  if (!n_out) return dm_set_error(DM_ERR_INVALID_ARG, "n_out is NULL");
  *n_out = 0;
  if (cap < 0 || (cap > 0 && !out_cells)) return dm_set_error(DM_ERR_INVALID_ARG, "cap < 0 or out_cells is NULL");
  if ((rc = plan_check_snap(snap_cells)) || (rc = plan_need_field(g, "dm_plan_path"))) return rc;
  if ((rc = grow_plan_query(g, 1))) return rc;
  // a path visits no cell twice: H * W entries hold any
  const int64_t dcap = std::max<int64_t>(1, std::min<int64_t>(cap, g->W * g->H));
  if ((rc = g->plan_path.ensure(dcap, "path cells"))) return rc;
  const double txy[2] = {tx, ty};
  DM_HIP(hipMemcpyAsync(g->plan_qxy, txy, sizeof txy, hipMemcpyHostToDevice, g->stream));
  if ((rc = dm_plan_launch_query(g, g->plan_qxy, 2, 1, snap_cells, g->plan_qcost, g->plan_qcell))) return rc;
  if ((rc = dm_plan_launch_path(g, g->plan_qcell, std::min(cap, dcap)))) return rc;
  unsigned long long st[2] = {0ull, 0ull};
  DM_HIP(hipMemcpyAsync(st, g->plan_stat + 4, sizeof st, hipMemcpyDeviceToHost, g->stream));
  DM_HIP(hipStreamSynchronize(g->stream));
  if (st[1])
    return dm_set_error(DM_ERR_INCOMPLETE, "dm_plan_path: the walk found no predecessor after %llu cells (the "
                        "field is not a fixpoint)", st[0]);
  const int64_t n = (int64_t)st[0];
  *n_out = n;
  if (n > cap)
    return dm_set_error(DM_ERR_CAPACITY, "the path has %lld cells, cap is %lld", (long long)n, (long long)cap);
  if (n > 0) {
    std::vector<int64_t> rev((size_t)n);
    DM_HIP(hipMemcpy(rev.data(), g->plan_path, sizeof(int64_t) * (size_t)n, hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < n; ++i) out_cells[i] = rev[(size_t)(n - 1 - i)];  // source first
  }
  return DM_OK;
}

// ---- team fields: one field per robot, relaxed together (dm_plan.h §4) ----------

// Everything the team needs for n robots; the arrays sized by n grow, the
// others are allocated once (team_stat last).
static int ensure_team(dm_grid* g, int32_t n) {
  int rc = DM_OK;
  if (!g->team_stat) {
    if (!g->h_team && (rc = g->h_team.alloc_zeroed(16, hipHostMallocMapped | hipHostMallocCoherent, "team rounds")))
      return rc;
    const int64_t rows = g->NT * DM_TILE;
    if ((rc = g->team_trav.alloc(rows, "team traversable bit rows"))) return rc;
    if ((rc = g->team_travp.alloc(rows, "team traversable bit rows with a source"))) return rc;
    if ((rc = g->team_src.alloc(DM_PLAN_TEAM_MAX, "team sources"))) return rc;
    if ((rc = g->team_len.alloc(4, "team list lengths"))) return rc;
    if ((rc = g->team_stat.alloc_zeroed(TEAM_ST_N, "team statistics"))) return rc;
  }
  const int64_t items = (int64_t)n * g->NT;
  if ((rc = g->team_list[0].ensure(items, "team item list")) || (rc = g->team_list[1].ensure(items, "team item list")) ||
      (rc = g->team_stamp.ensure(items, "team item stamps")))
    return rc;
  return g->team_cost.ensure((int64_t)n * g->W * g->H, "team distance fields");
}

static int plan_need_team(const dm_grid* g, const char* what) {
  if (!g->team_cost || !g->team_valid)
    return dm_set_error(DM_ERR_STATE, "%s: no team fields (call dm_plan_team first)", what);
  if (g->team_version != dm_map_version(g))
    return dm_set_error(DM_ERR_STATE, "%s: the map changed since the team fields were computed (call dm_plan_team "
                        "again)", what);
  return DM_OK;
}

static int plan_check_team_robot(const dm_grid* g, int32_t robot) {
  if (robot < 0 || robot >= g->team_n)
    return dm_set_error(DM_ERR_INVALID_ARG, "robot must be in [0, %d) (got %d)", g->team_n, robot);
  return DM_OK;
}

// The team fields of n robots (metres), after the argument checks of the
// entry point; leaves them in the handle.  stats: [3 + n] or nullptr.
static int plan_team_from(dm_grid* g, const double* robots_xy, int32_t n, int32_t inflate_cells, uint32_t max_cost,
                          uint64_t* stats) {
  int64_t cells[DM_PLAN_TEAM_MAX];
  for (int32_t k = 0; k < n; ++k)
    if (!plan_cell_of(g, robots_xy[2 * k], robots_xy[2 * k + 1], &cells[k]))
      return dm_set_error(DM_ERR_INVALID_ARG, "robot %d (%g, %g) is outside the grid", k, robots_xy[2 * k],
                          robots_xy[2 * k + 1]);
  if ((int64_t)n * g->NT >= (1ll << 31))
    return dm_set_error(DM_ERR_CAPACITY, "n_robots * tiles = %lld does not fit the int32 work items",
                        (long long)((int64_t)n * g->NT));
  if (max_cost == 0u || max_cost > 0xFFFFFFEFu) max_cost = 0xFFFFFFEFu;
  g->team_valid = false;
  int rc = ensure_team(g, n);
  if (rc) return rc;
  DM_HIP(dm_join_pass_stream(g));
  if ((rc = dm_plan_run_team(g, cells, n, inflate_cells, max_cost, stats))) return rc;
  g->team_n = n;
  g->team_valid = true;
  g->team_version = dm_map_version(g);
  return DM_OK;
}

int dm_plan_team(dm_grid* g, const double* robots_xy, int32_t n_robots, int32_t inflate_cells, uint32_t max_cost,
                 uint64_t* out_stats) {
  int rc = dm_check_whole_map(g, "dm_plan_team");
  if (rc || (rc = use_device(g))) return rc;
  if (n_robots < 1 || n_robots > DM_PLAN_TEAM_MAX)
    return dm_set_error(DM_ERR_INVALID_ARG, "n_robots must be in [1, %d] (got %d)", DM_PLAN_TEAM_MAX, n_robots);
  if (!robots_xy) return dm_set_error(DM_ERR_INVALID_ARG, "robots_xy is NULL");
  if ((rc = plan_check_inflate(inflate_cells))) return rc;
  return plan_team_from(g, robots_xy, n_robots, inflate_cells, max_cost, out_stats);
}

int dm_plan_team_get_field(dm_grid* g, int32_t robot, uint32_t* out) {
  int rc = dm_check_whole_map(g, "dm_plan_team_get_field");
  if (rc || (rc = use_device(g))) return rc;
  if (!out) return dm_set_error(DM_ERR_INVALID_ARG, "out is NULL");
  if ((rc = plan_need_team(g, "dm_plan_team_get_field")) || (rc = plan_check_team_robot(g, robot))) return rc;
  const int64_t ncell = g->W * g->H;
  DM_HIP(hipMemcpyAsync(out, g->team_cost + (int64_t)robot * ncell, sizeof(uint32_t) * (size_t)ncell,
                        hipMemcpyDeviceToHost, g->stream));
  DM_HIP(hipStreamSynchronize(g->stream));
  return DM_OK;
}

int dm_plan_team_query(dm_grid* g, const double* targets_xy, int64_t n, int32_t snap_cells, uint32_t* out_cost,
                       int64_t* out_cell) {
  int rc = dm_check_whole_map(g, "dm_plan_team_query");
  if (rc || (rc = use_device(g))) return rc;
  if (n < 0) return dm_set_error(DM_ERR_INVALID_ARG, "n must be >= 0");
  if (n > 0 && (!targets_xy || !out_cost || !out_cell))
    return dm_set_error(DM_ERR_INVALID_ARG, "targets_xy / out_cost / out_cell is NULL");
  if ((rc = plan_check_snap(snap_cells)) || (rc = plan_need_team(g, "dm_plan_team_query"))) return rc;
  if (n == 0) return DM_OK;
  const int64_t total = n * g->team_n;
  if ((rc = grow_plan_query(g, n)) || (rc = g->team_qcost.ensure(total, "team query costs")) ||
      (rc = g->team_qcell.ensure(total, "team query cells")))
    return rc;
  DM_HIP(hipMemcpyAsync(g->plan_qxy, targets_xy, sizeof(double) * 2 * (size_t)n, hipMemcpyHostToDevice, g->stream));
  if ((rc = dm_plan_launch_team_query(g, 0, g->team_n, g->plan_qxy, 2, n, snap_cells, g->team_qcost, g->team_qcell)))
    return rc;
  DM_HIP(hipMemcpyAsync(out_cost, g->team_qcost, sizeof(uint32_t) * (size_t)total, hipMemcpyDeviceToHost, g->stream));
  DM_HIP(hipMemcpyAsync(out_cell, g->team_qcell, sizeof(int64_t) * (size_t)total, hipMemcpyDeviceToHost, g->stream));
  DM_HIP(hipStreamSynchronize(g->stream));
  return DM_OK;
}

int dm_plan_team_path(dm_grid* g, int32_t robot, double tx, double ty, int32_t snap_cells, int64_t* out_cells,
                      int64_t cap, int64_t* n_out) {
  int rc = dm_check_whole_map(g, "dm_plan_team_path");
  if (rc || (rc = use_device(g))) return rc;
  if (!n_out) return dm_set_error(DM_ERR_INVALID_ARG, "n_out is NULL");
  *n_out = 0;
  if (cap < 0 || (cap > 0 && !out_cells)) return dm_set_error(DM_ERR_INVALID_ARG, "cap < 0 or out_cells is NULL");
  if ((rc = plan_check_snap(snap_cells)) || (rc = plan_need_team(g, "dm_plan_team_path")) ||
      (rc = plan_check_team_robot(g, robot)))
    return rc;
  if ((rc = grow_plan_query(g, 1))) return rc;
  const int64_t dcap = std::max<int64_t>(1, std::min<int64_t>(cap, g->W * g->H));
  if ((rc = g->plan_path.ensure(dcap, "path cells"))) return rc;
  const double txy[2] = {tx, ty};
  DM_HIP(hipMemcpyAsync(g->plan_qxy, txy, sizeof txy, hipMemcpyHostToDevice, g->stream));
  if ((rc = dm_plan_launch_team_query(g, robot, 1, g->plan_qxy, 2, 1, snap_cells, g->plan_qcost, g->plan_qcell)))
    return rc;
  if ((rc = dm_plan_launch_team_path(g, robot, g->plan_qcell, std::min(cap, dcap)))) return rc;
  unsigned long long st[2] = {0ull, 0ull};
  DM_HIP(hipMemcpyAsync(st, g->team_stat + TEAM_ST_PATH, sizeof st, hipMemcpyDeviceToHost, g->stream));
  DM_HIP(hipStreamSynchronize(g->stream));
  if (st[1])
    return dm_set_error(DM_ERR_INCOMPLETE, "dm_plan_team_path: the walk found no predecessor after %llu cells (the "
                        "field is not a fixpoint)", st[0]);
  const int64_t n = (int64_t)st[0];
  *n_out = n;
  if (n > cap)
    return dm_set_error(DM_ERR_CAPACITY, "the path has %lld cells, cap is %lld", (long long)n, (long long)cap);
  if (n > 0) {
    std::vector<int64_t> rev((size_t)n);
    DM_HIP(hipMemcpy(rev.data(), g->plan_path, sizeof(int64_t) * (size_t)n, hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < n; ++i) out_cells[i] = rev[(size_t)(n - 1 - i)];  // source first
  }
  return DM_OK;
}

// ---- information gain (csrc/dm_gain.h): visible-unknown counts of view
// points, gain-scored goals ---------------------------------------------------------

static int grow_gain(dm_grid* g, int64_t n) {
  if (n <= g->gain_cap) return DM_OK;
  return g->gain_cap.grow(n, [&] {
    int rc = g->gain_xy.alloc(2 * n, "view points");
    if (!rc) rc = g->gain_cell.alloc(n, "view cells");
    if (!rc) rc = g->gain_out.alloc(n, "view gains");
    if (!rc) rc = g->gain_skip.alloc(n, "view skip flags");
    if (!rc) rc = g->gain_memo_cell.alloc(n, "gain memo cells");
    if (!rc) rc = g->gain_memo_gain.alloc(n, "gain memo gains");
    return rc;
  });
}

static int gain_check_radius(int32_t radius_cells) {
  if (radius_cells < 1 || radius_cells > 511)
    return dm_set_error(DM_ERR_INVALID_ARG, "radius_cells must be in [1, 511] (got %d)", radius_cells);
  return DM_OK;
}

int dm_gain_views(dm_grid* g, const double* views_xy, int64_t n, int32_t radius_cells, uint32_t* out_gain,
                  int64_t* out_cell) {
  int rc = dm_check_whole_map(g, "dm_gain_views");
  if (rc || (rc = use_device(g))) return rc;
  if (n < 0 || n > (1ll << 20))
    return dm_set_error(DM_ERR_INVALID_ARG, "n must be in [0, 2^20] (got %lld)", (long long)n);
  if (n > 0 && (!views_xy || !out_gain || !out_cell))
    return dm_set_error(DM_ERR_INVALID_ARG, "views_xy / out_gain / out_cell is NULL");
  if ((rc = gain_check_radius(radius_cells))) return rc;
  if (n == 0) return DM_OK;
  if ((rc = grow_gain(g, n))) return rc;
  DM_HIP(dm_sync_all(g));  // after everything enqueued on the handle, on every stream of it
  DM_HIP(hipMemcpyAsync(g->gain_xy, views_xy, sizeof(double) * 2 * (size_t)n, hipMemcpyHostToDevice, g->stream));
  if ((rc = dm_gain_launch_cells(g, n))) return rc;
  if ((rc = dm_gain_launch_views(g, g->gain_cell, nullptr, n, radius_cells, false))) return rc;
  DM_HIP(hipMemcpyAsync(out_gain, g->gain_out, sizeof(uint32_t) * (size_t)n, hipMemcpyDeviceToHost, g->stream));
  DM_HIP(hipMemcpyAsync(out_cell, g->gain_cell, sizeof(int64_t) * (size_t)n, hipMemcpyDeviceToHost, g->stream));
  DM_HIP(hipStreamSynchronize(g->stream));
  return DM_OK;
}

// The claimed set of the overlap-aware calls: allocated by the first of them.
static int64_t claimed_words(const dm_grid* g) { return g->H * ((g->W + 31) / 32); }

static int ensure_claimed(dm_grid* g) {
  if (g->gain_claimed) return DM_OK;
  return g->gain_claimed.alloc(claimed_words(g), "claimed set");
}

// n points (metres) to g->gain_xy and their cells to g->gain_cell.
static int gain_upload_views(dm_grid* g, const double* xy, int64_t n) {
  if (n <= 0) return DM_OK;
  DM_HIP(hipMemcpyAsync(g->gain_xy, xy, sizeof(double) * 2 * (size_t)n, hipMemcpyHostToDevice, g->stream));
  return dm_gain_launch_cells(g, n);
}

int dm_gain_views_joint(dm_grid* g, const double* views_xy, int64_t n, int32_t radius_cells, uint32_t* out_marginal,
                        int64_t* out_cell) {
  int rc = dm_check_whole_map(g, "dm_gain_views_joint");
  if (rc || (rc = use_device(g))) return rc;
  if (n < 0 || n > 1024) return dm_set_error(DM_ERR_INVALID_ARG, "n must be in [0, 1024] (got %lld)", (long long)n);
  if (n > 0 && (!views_xy || !out_marginal || !out_cell))
    return dm_set_error(DM_ERR_INVALID_ARG, "views_xy / out_marginal / out_cell is NULL");
  if ((rc = gain_check_radius(radius_cells))) return rc;
  if ((rc = ensure_claimed(g)) || (rc = grow_gain(g, std::max<int64_t>(n, 1)))) return rc;
  DM_HIP(dm_sync_all(g));  // after everything enqueued on the handle, on every stream of it
  g->gain_claimed_valid = false;
  DM_HIP(hipMemsetAsync(g->gain_claimed, 0, sizeof(uint32_t) * (size_t)claimed_words(g), g->stream));
  if ((rc = gain_upload_views(g, views_xy, n))) return rc;
  if ((rc = dm_gain_launch_joint(g, g->gain_cell, n, radius_cells, g->gain_out))) return rc;
  if (n > 0) {
    DM_HIP(hipMemcpyAsync(out_marginal, g->gain_out, sizeof(uint32_t) * (size_t)n, hipMemcpyDeviceToHost, g->stream));
    DM_HIP(hipMemcpyAsync(out_cell, g->gain_cell, sizeof(int64_t) * (size_t)n, hipMemcpyDeviceToHost, g->stream));
  }
  DM_HIP(hipStreamSynchronize(g->stream));
  g->gain_claimed_valid = true;
  return DM_OK;
}

int dm_gain_claimed(dm_grid* g, uint8_t* out) {
  int rc = dm_check_whole_map(g, "dm_gain_claimed");
  if (rc || (rc = use_device(g))) return rc;
  if (!out) return dm_set_error(DM_ERR_INVALID_ARG, "out is NULL");
  if (!g->gain_claimed || !g->gain_claimed_valid)
    return dm_set_error(DM_ERR_STATE, "dm_gain_claimed: no claimed set (call dm_gain_views_joint or "
                        "dm_assign_goals_coord first)");
  const int64_t cells = g->W * g->H;
  DevBuf<uint8_t> d;
  if ((rc = d.alloc(cells, "claimed image")) || (rc = dm_gain_launch_expand(g, d))) return rc;
  hipError_t e = hipMemcpyAsync(out, d, (size_t)cells, hipMemcpyDeviceToHost, g->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(g->stream);
  if (e != hipSuccess) return dm_hip_check(e, "dm_gain_claimed");
  return DM_OK;
}

// ---- goal assignment: dm_assign_goals (Euclidean distance to the centroid)
// and the three calls that score by a robot's own distance field --------------

// What every goal call checks first, in this order; `null_names`: the
// buffers of the call, for the message, and whether one of them is NULL.
static int check_goal_args(int32_t n_robots, bool any_null, const char* null_names, double distance_weight,
                           double min_distance) {
  if (n_robots < 0 || n_robots > 256)
    return dm_set_error(DM_ERR_INVALID_ARG, "n_robots must be in [0, 256] (got %d)", n_robots);
  if (n_robots > 0 && any_null) return dm_set_error(DM_ERR_INVALID_ARG, "%s is NULL", null_names);
  if (!isfinite(distance_weight) || !isfinite(min_distance))
    return dm_set_error(DM_ERR_INVALID_ARG, "distance_weight / min_distance must be finite");
  // the device ranks by the util's IEEE bits, an order that holds for util > 0
  // only: w >= 0 keeps util = numerator / (1 + w*dist) positive and finite
  if (distance_weight < 0.0)
    return dm_set_error(DM_ERR_INVALID_ARG, "distance_weight must be >= 0");
  return DM_OK;
}

// The label-sorted device records of the last collected frontier result
// (dm_api.cpp: note_goal_source), if its readback slot still holds them.
static int goal_source(const dm_grid* g, const dm_cluster** recs, int64_t* K) {
  const dm_grid::GoalSource& s = g->goal;
  if (!s.slot || s.gen != g->rb_gen || (s.kind == 1 ? s.slot->wepoch : s.slot->mepoch) != s.epoch)
    return dm_set_error(DM_ERR_INVALID_ARG, "no collected frontier result on the device (call dm_frontiers, "
                                            "dm_frontiers_end or dm_merge_bands first; a later pass may have "
                                            "reused its readback slot)");
  *recs = s.kind == 1 ? s.slot->out_clu.records() : s.slot->m_out.get();
  *K = s.n;
  return DM_OK;
}

// Robot r's turn of the greedy assignment: the first cluster of its best-first
// list (T keys and indices; key 0: no eligible cluster left) that none of the
// robots before it took, or -1.  Its choice is within the first r + 1 entries:
// r clusters are taken before its turn.
static int64_t greedy_pick(const unsigned long long* hk, const uint32_t* hi, int32_t T,
                           const std::vector<int64_t>& idx, int32_t r) {
  for (int32_t t = 0; t < T; ++t) {
    if (hk[t] == 0ull) break;
    const int64_t c = hi[t];
    if (std::find(idx.begin(), idx.begin() + r, c) == idx.begin() + r) return c;
  }
  return -1;
}

// The centre of a cell (linear index) in metres.
static void cell_centre(const dm_grid* g, int64_t cell, double* xy) {
  xy[0] = g->p.origin_x + ((double)(cell % g->W) + 0.5) * g->p.resolution;
  xy[1] = g->p.origin_y + ((double)(cell / g->W) + 0.5) * g->p.resolution;
}

int dm_assign_goals(dm_grid* g, const double* robots_xy, int32_t n_robots, int64_t min_size,
                    double distance_weight, double min_distance, int64_t* out_index, double* out_xy) {
  if (g && g->sh) return dm_sh_assign_goals(g, robots_xy, n_robots, min_size, distance_weight, min_distance, out_index, out_xy);
  int rc = check_grid(g);
  if (rc || (rc = use_device(g))) return rc;
  if ((rc = check_goal_args(n_robots, !robots_xy || !out_index || !out_xy, "robots_xy / out_index / out_xy",
                            distance_weight, min_distance)))
    return rc;
  const dm_cluster* recs = nullptr;
  int64_t K = 0;
  if ((rc = goal_source(g, &recs, &K))) return rc;
  if (n_robots == 0) return DM_OK;
  if (!g->goal_io) {  // allocated last: goal_idx is there too
    if ((rc = g->goal_idx.alloc(256, "goal indices out")) || (rc = g->goal_io.alloc(4 * 256, "goal robots and centroids")))
      return rc;
  }
  DM_HIP(dm_join_pass_stream(g));
  const int32_t R = n_robots, T = n_robots;
  DM_HIP(hipMemcpyAsync(g->goal_io, robots_xy, sizeof(double) * 2 * (size_t)R, hipMemcpyHostToDevice,
                        g->stream));
  std::vector<int64_t> idx((size_t)R, -1);
  if (K > 0) {
    const unsigned long long* dk = nullptr;
    const uint32_t* di = nullptr;
    if ((rc = dm_launch_goal_topk(g, recs, K, g->goal_io, R, T, min_size, distance_weight, min_distance, &dk,
                                  &di)))
      return rc;
    std::vector<unsigned long long> hk((size_t)R * T);
    std::vector<uint32_t> hi((size_t)R * T);
    DM_HIP(hipMemcpyAsync(hk.data(), dk, sizeof(unsigned long long) * hk.size(), hipMemcpyDeviceToHost,
                          g->stream));
    DM_HIP(hipMemcpyAsync(hi.data(), di, sizeof(uint32_t) * hi.size(), hipMemcpyDeviceToHost, g->stream));
    DM_HIP(hipStreamSynchronize(g->stream));
    for (int32_t r = 0; r < R; ++r) idx[(size_t)r] = greedy_pick(&hk[(size_t)r * T], &hi[(size_t)r * T], T, idx, r);
  }
  DM_HIP(hipMemcpyAsync(g->goal_idx, idx.data(), sizeof(int64_t) * (size_t)R, hipMemcpyHostToDevice,
                        g->stream));
  if ((rc = dm_launch_goal_gather(g, recs, g->goal_idx, R, g->goal_io + 2 * 256))) return rc;
  DM_HIP(hipMemcpyAsync(out_xy, g->goal_io + 2 * 256, sizeof(double) * 2 * (size_t)R, hipMemcpyDeviceToHost,
                        g->stream));
  DM_HIP(hipStreamSynchronize(g->stream));
  memcpy(out_index, idx.data(), sizeof(int64_t) * (size_t)R);
  return DM_OK;
}

// How a field-scored goal call scores a cluster: util = numerator / (1 + w *
// dist), dist the path length from the robot to the cluster's snapped centroid.
struct GoalScoring {
  const char* what;  // the entry point, for messages
  // the numerator: the cluster's size (dm_assign_goals_path), the
  // visible-unknown count of its snapped cell (dm_assign_goals_gain), or what
  // that cell sees outside the claimed set (dm_assign_goals_coord), which
  // starts as the held views and takes every goal's view as it is assigned
  enum { kSize, kGain, kMarginal } numerator;
  int64_t min_gain;        // the rest is not read with kSize
  int32_t radius_cells;
  const double* held_xy;   // kMarginal only
  int32_t n_held;
};

// out_gain: nullptr with kSize.  The field left in the handle is the last robot's.
static int assign_goals_field(dm_grid* g, const GoalScoring& sc, const double* robots_xy, int32_t n_robots,
                              int64_t min_size, double distance_weight, double min_distance, int32_t inflate_cells,
                              uint32_t max_cost, int32_t snap_cells, int64_t* out_index, double* out_xy,
                              int64_t* out_cell, uint32_t* out_gain) {
  const bool gain = sc.numerator != GoalScoring::kSize, coord = sc.numerator == GoalScoring::kMarginal;
  int rc = dm_check_whole_map(g, sc.what);
  if (rc || (rc = use_device(g))) return rc;
  if ((rc = check_goal_args(n_robots, !robots_xy || !out_index || !out_xy || !out_cell || (gain && !out_gain),
                            gain ? "robots_xy / out_index / out_xy / out_cell / out_gain"
                                 : "robots_xy / out_index / out_xy / out_cell",
                            distance_weight, min_distance)))
    return rc;
  if (gain) {
    if (sc.min_gain < 0)
      return dm_set_error(DM_ERR_INVALID_ARG, "min_gain must be >= 0 (got %lld)", (long long)sc.min_gain);
    if (sc.n_held < 0 || sc.n_held > 1024)
      return dm_set_error(DM_ERR_INVALID_ARG, "n_held must be in [0, 1024] (got %d)", sc.n_held);
    if (sc.n_held > 0 && !sc.held_xy) return dm_set_error(DM_ERR_INVALID_ARG, "held_xy is NULL");
  }
  if ((rc = plan_check_inflate(inflate_cells)) || (rc = plan_check_snap(snap_cells)) ||
      (gain && (rc = gain_check_radius(sc.radius_cells))))
    return rc;
  const dm_cluster* recs = nullptr;
  int64_t K = 0;
  if ((rc = goal_source(g, &recs, &K))) return rc;
  if (n_robots == 0 && !coord) return DM_OK;
  for (int32_t r = 0; r < n_robots; ++r) {
    int64_t c;
    if (!plan_cell_of(g, robots_xy[2 * r], robots_xy[2 * r + 1], &c))
      return dm_set_error(DM_ERR_INVALID_ARG, "robot %d (%g, %g) is outside the grid", r, robots_xy[2 * r],
                          robots_xy[2 * r + 1]);
  }
  if ((rc = ensure_plan(g)) || (rc = grow_plan_query(g, std::max<int64_t>(K, 1)))) return rc;
  if (gain && (rc = grow_gain(g, std::max<int64_t>(std::max<int64_t>(K, sc.n_held), 1)))) return rc;
  if (coord && (rc = ensure_claimed(g))) return rc;
  DM_HIP(dm_join_pass_stream(g));
  if (coord) {
    // C: empty, then the held views, all in one launch (ORs commute)
    g->gain_claimed_valid = false;
    DM_HIP(hipMemsetAsync(g->gain_claimed, 0, sizeof(uint32_t) * (size_t)claimed_words(g), g->stream));
    if ((rc = gain_upload_views(g, sc.held_xy, sc.n_held))) return rc;
    if ((rc = dm_gain_launch_commit(g, g->gain_cell, sc.n_held, sc.radius_cells))) return rc;
    if (n_robots == 0) {
      DM_HIP(hipStreamSynchronize(g->stream));
      g->gain_claimed_valid = true;
      return DM_OK;
    }
  }
  if ((rc = dm_plan_launch_travers(g, inflate_cells))) return rc;
  // the memo of this call: no cluster has a cast yet (every byte 0xFF: cell -1,
  // which no cast view has)
  if (gain && K > 0) DM_HIP(hipMemsetAsync(g->gain_memo_cell, 0xFF, sizeof(int64_t) * (size_t)K, g->stream));
  const int32_t R = n_robots, T = n_robots;
  std::vector<int64_t> idx((size_t)R, -1);
  std::vector<unsigned long long> hk((size_t)T);
  std::vector<uint32_t> hi((size_t)T);
  for (int32_t r = 0; r < R; ++r) {
    // robot r's field, its path cost to every cluster's snapped centroid, then
    // (gain) the numerator of every snapped cell that can still be a goal
    if ((rc = plan_field_from(g, robots_xy + 2 * r, 1, max_cost, nullptr))) return rc;
    out_cell[r] = -1;
    if (gain) out_gain[r] = 0u;
    out_xy[2 * r] = out_xy[2 * r + 1] = NAN;
    if (K == 0) continue;
    if ((rc = dm_plan_launch_query(g, &recs[0].cx_m, (int64_t)(sizeof(dm_cluster) / sizeof(double)), K, snap_cells,
                                   g->plan_qcost, g->plan_qcell)))
      return rc;
    if (gain) {
      if ((rc = dm_gain_launch_skip(g, recs, g->plan_qcost, K, min_size))) return rc;
      if ((rc = coord ? dm_gain_launch_marginal(g, g->plan_qcell, g->gain_skip, K, sc.radius_cells, true)
                      : dm_gain_launch_views(g, g->plan_qcell, g->gain_skip, K, sc.radius_cells, true)))
        return rc;
    }
    const unsigned long long* dk = nullptr;
    const uint32_t* di = nullptr;
    if ((rc = dm_launch_goal_topk(g, recs, K, nullptr, 1, T, min_size, distance_weight, min_distance, &dk, &di,
                                  g->plan_qcost, gain ? g->gain_out : nullptr, gain ? sc.min_gain : 0)))
      return rc;
    DM_HIP(hipMemcpyAsync(hk.data(), dk, sizeof(unsigned long long) * (size_t)T, hipMemcpyDeviceToHost, g->stream));
    DM_HIP(hipMemcpyAsync(hi.data(), di, sizeof(uint32_t) * (size_t)T, hipMemcpyDeviceToHost, g->stream));
    DM_HIP(hipStreamSynchronize(g->stream));
    const int64_t c = idx[(size_t)r] = greedy_pick(hk.data(), hi.data(), T, idx, r);
    if (c < 0) continue;
    int64_t cell = -1;
    DM_HIP(hipMemcpy(&cell, g->plan_qcell + c, sizeof cell, hipMemcpyDeviceToHost));
    if (gain) DM_HIP(hipMemcpy(&out_gain[r], g->gain_out + c, sizeof out_gain[r], hipMemcpyDeviceToHost));
    out_cell[r] = cell;
    cell_centre(g, cell, out_xy + 2 * r);  // a reachable goal, not the centroid
    if (coord) {
      // the goal's view joins C before the next robot is scored; its gain
      // is > 0, so C changed and no memo entry holds any longer
      if ((rc = dm_gain_launch_commit(g, g->plan_qcell + c, 1, sc.radius_cells))) return rc;
      DM_HIP(hipMemsetAsync(g->gain_memo_cell, 0xFF, sizeof(int64_t) * (size_t)K, g->stream));
    }
  }
  if (coord) {
    DM_HIP(hipStreamSynchronize(g->stream));
    g->gain_claimed_valid = true;
  }
  memcpy(out_index, idx.data(), sizeof(int64_t) * (size_t)R);
  return DM_OK;
}

int dm_assign_goals_path(dm_grid* g, const double* robots_xy, int32_t n_robots, int64_t min_size,
                         double distance_weight, double min_distance, int32_t inflate_cells, uint32_t max_cost,
                         int32_t snap_cells, int64_t* out_index, double* out_xy, int64_t* out_cell) {
  const GoalScoring sc = {"dm_assign_goals_path", GoalScoring::kSize, 0, 0, nullptr, 0};
  return assign_goals_field(g, sc, robots_xy, n_robots, min_size, distance_weight, min_distance, inflate_cells,
                            max_cost, snap_cells, out_index, out_xy, out_cell, nullptr);
}

int dm_assign_goals_gain(dm_grid* g, const double* robots_xy, int32_t n_robots, int64_t min_size, int64_t min_gain,
                         double distance_weight, double min_distance, int32_t inflate_cells, uint32_t max_cost,
                         int32_t snap_cells, int32_t radius_cells, int64_t* out_index, double* out_xy,
                         int64_t* out_cell, uint32_t* out_gain) {
  const GoalScoring sc = {"dm_assign_goals_gain", GoalScoring::kGain, min_gain, radius_cells, nullptr, 0};
  return assign_goals_field(g, sc, robots_xy, n_robots, min_size, distance_weight, min_distance, inflate_cells,
                            max_cost, snap_cells, out_index, out_xy, out_cell, out_gain);
}

int dm_assign_goals_coord(dm_grid* g, const double* robots_xy, int32_t n_robots, const double* held_xy,
                          int32_t n_held, int64_t min_size, int64_t min_gain, double distance_weight,
                          double min_distance, int32_t inflate_cells, uint32_t max_cost, int32_t snap_cells,
                          int32_t radius_cells, int64_t* out_index, double* out_xy, int64_t* out_cell,
                          uint32_t* out_gain) {
  const GoalScoring sc = {"dm_assign_goals_coord", GoalScoring::kMarginal, min_gain, radius_cells, held_xy, n_held};
  return assign_goals_field(g, sc, robots_xy, n_robots, min_size, distance_weight, min_distance, inflate_cells,
                            max_cost, snap_cells, out_index, out_xy, out_cell, out_gain);
}

// The global-greedy assignment over R best-first lists of T entries (key 0:
// no eligible cluster left): among the pairs (r, c) with r unassigned and c
// untaken take the greatest key, ties to the smaller record index (the
// smaller label), then the smaller r; until no pair is left.  A robot's goal
// is among its R best eligible clusters, since the others take at most R - 1.
static void team_pick(const unsigned long long* hk, const uint32_t* hi, int32_t R, int32_t T,
                      std::vector<int64_t>& idx) {
  std::vector<int32_t> pos((size_t)R, 0);  // the first entry of r's list that may still be free
  for (;;) {
    int32_t br = -1;
    unsigned long long bk = 0ull;
    uint32_t bi = 0u;
    for (int32_t r = 0; r < R; ++r) {
      if (idx[(size_t)r] >= 0) continue;
      int32_t& t = pos[(size_t)r];
      while (t < T && hk[(size_t)r * T + t] != 0ull &&
             std::find(idx.begin(), idx.end(), (int64_t)hi[(size_t)r * T + t]) != idx.end())
        ++t;
      if (t >= T || hk[(size_t)r * T + t] == 0ull) continue;
      const unsigned long long k = hk[(size_t)r * T + t];
      const uint32_t i = hi[(size_t)r * T + t];
      if (br < 0 || k > bk || (k == bk && i < bi)) {  // equal (k, i): the smaller r stays
        br = r;
        bk = k;
        bi = i;
      }
    }
    if (br < 0) return;
    idx[(size_t)br] = (int64_t)bi;
  }
}

int dm_assign_goals_team(dm_grid* g, const double* robots_xy, int32_t n_robots, int64_t min_size, int64_t min_gain,
                         double distance_weight, double min_distance, int32_t inflate_cells, uint32_t max_cost,
                         int32_t snap_cells, int32_t radius_cells, int64_t* out_index, double* out_xy,
                         int64_t* out_cell, uint32_t* out_gain) {
  const bool gain = radius_cells != 0;
  int rc = dm_check_whole_map(g, "dm_assign_goals_team");
  if (rc || (rc = use_device(g))) return rc;
  if (n_robots > DM_PLAN_TEAM_MAX)
    return dm_set_error(DM_ERR_INVALID_ARG, "n_robots must be in [0, %d] (got %d)", DM_PLAN_TEAM_MAX, n_robots);
  if ((rc = check_goal_args(n_robots, !robots_xy || !out_index || !out_xy || !out_cell || (gain && !out_gain),
                            gain ? "robots_xy / out_index / out_xy / out_cell / out_gain"
                                 : "robots_xy / out_index / out_xy / out_cell",
                            distance_weight, min_distance)))
    return rc;
  if (gain && min_gain < 0)
    return dm_set_error(DM_ERR_INVALID_ARG, "min_gain must be >= 0 (got %lld)", (long long)min_gain);
  if ((rc = plan_check_inflate(inflate_cells)) || (rc = plan_check_snap(snap_cells)) ||
      (gain && (rc = gain_check_radius(radius_cells))))
    return rc;
  const dm_cluster* recs = nullptr;
  int64_t K = 0;
  if ((rc = goal_source(g, &recs, &K))) return rc;
  if (n_robots == 0) return DM_OK;
  const int32_t R = n_robots, T = n_robots;
  const int64_t total = (int64_t)R * K;
  // every robot's field, then the whole R x K matrix of snapped centroids, the
  // gains of its cells and every robot's top R: one launch each
  if ((rc = plan_team_from(g, robots_xy, R, inflate_cells, max_cost, nullptr))) return rc;
  std::vector<int64_t> idx((size_t)R, -1);
  for (int32_t r = 0; r < R; ++r) {
    out_cell[r] = -1;
    if (gain) out_gain[r] = 0u;
    out_xy[2 * r] = out_xy[2 * r + 1] = NAN;
  }
  if (K > 0) {
    if ((rc = g->team_qcost.ensure(total, "team query costs")) || (rc = g->team_qcell.ensure(total, "team query cells")))
      return rc;
    if (gain && (rc = grow_gain(g, total))) return rc;
    if ((rc = dm_plan_launch_team_query(g, 0, R, &recs[0].cx_m, (int64_t)(sizeof(dm_cluster) / sizeof(double)), K,
                                        snap_cells, g->team_qcost, g->team_qcell)))
      return rc;
    if (gain) {
      if ((rc = dm_gain_launch_skip_team(g, recs, g->team_qcost, K, R, min_size))) return rc;
      if ((rc = dm_gain_launch_views(g, g->team_qcell, g->gain_skip, total, radius_cells, false))) return rc;
    }
    const unsigned long long* dk = nullptr;
    const uint32_t* di = nullptr;
    if ((rc = dm_launch_goal_topk(g, recs, K, nullptr, R, T, min_size, distance_weight, min_distance, &dk, &di,
                                  g->team_qcost, gain ? g->gain_out.get() : nullptr, gain ? min_gain : 0)))
      return rc;
    std::vector<unsigned long long> hk((size_t)R * T);
    std::vector<uint32_t> hi((size_t)R * T);
    DM_HIP(hipMemcpyAsync(hk.data(), dk, sizeof(unsigned long long) * hk.size(), hipMemcpyDeviceToHost, g->stream));
    DM_HIP(hipMemcpyAsync(hi.data(), di, sizeof(uint32_t) * hi.size(), hipMemcpyDeviceToHost, g->stream));
    DM_HIP(hipStreamSynchronize(g->stream));
    team_pick(hk.data(), hi.data(), R, T, idx);
    for (int32_t r = 0; r < R; ++r) {
      const int64_t c = idx[(size_t)r];
      if (c < 0) continue;
      const int64_t at = (int64_t)r * K + c;
      DM_HIP(hipMemcpyAsync(&out_cell[r], g->team_qcell + at, sizeof(int64_t), hipMemcpyDeviceToHost, g->stream));
      if (gain)
        DM_HIP(hipMemcpyAsync(&out_gain[r], g->gain_out + at, sizeof(uint32_t), hipMemcpyDeviceToHost, g->stream));
    }
    DM_HIP(hipStreamSynchronize(g->stream));
    for (int32_t r = 0; r < R; ++r)
      if (idx[(size_t)r] >= 0) cell_centre(g, out_cell[r], out_xy + 2 * r);  // a reachable goal, not the centroid
  }
  memcpy(out_index, idx.data(), sizeof(int64_t) * (size_t)R);
  return DM_OK;
}

}  // extern "C"
