// dm_match.hip — the two scan matchers against the device-resident map: the
// correlative matcher around a prior (dm_match_field, dm_match_scans; kernels
// in dm_match.h) and the whole-window relocalisation (dm_match_global; kernels
// in dm_match_global.h).  Kernels' launchers first, then the entry points;
// the match_* and mg_* arrays of the handle are allocated here.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "dm_internal.h"
#include "dm_match.h"
#include "dm_match_global.h"

// The shape of one dm_match_global call.
struct MgShape {
  int32_t N, A, k0, half_x, half_y, lb;  // block = 1 << lb
  int32_t nbx, nby;                      // blocks per yaw along x and y
  int32_t EWB, EHB;                      // the pooled field's planes: [EHB][EWB]
  int32_t exhaustive;
};

// ---- scan matcher (dm_match.h) ------------------------------------------------

// the response field of the first n_tiles tiles of g->match_tiles into g->match_V
static int dm_match_launch_field(dm_grid* g, int32_t n_tiles, int32_t r, bool mono) {
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

// fine coordinates (g->match_q, used beams at g->match_out + 4 S), the score
// volume (g->match_vol) and the best candidates (g->match_out) of S scans
static int dm_match_launch_scans(dm_grid* g, int32_t S, int32_t N, int32_t A, int32_t k0, int32_t sub, int32_t half,
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

// M_B of the first n_tiles tiles of g->mg_ptiles (PTX tiles per row) into g->mg_pool
static int dm_mg_launch_pool(dm_grid* g, int32_t n_tiles, int32_t lb, int32_t EWB, int32_t EHB, int32_t PTX) {
  if (n_tiles <= 0) return DM_OK;
  KernelTimer t;
  dm_timer_begin(g, "mg_pool", &t);
  hipLaunchKernelGGL(dm_mg::k_mg_pool, dim3((unsigned)n_tiles), dim3(dm_mg::kThreads), 0, g->stream, g->match_V, g->W,
                     g->H, lb, EWB, EHB, PTX, g->mg_ptiles, g->mg_pool);
  DM_HIP(hipGetLastError());
  dm_timer_end(g, &t);
  return DM_OK;
}

// One scan: candidate poses d_pose4 [A][4], ranges d_ranges [N], g->match_trig.
// Synchronous.  res = k, i, j, score, used beams; stats [4] as dm_match_global's.
// off_map: the window reaches no cell of the map, so only the used beams are
// counted and nothing is bounded or scored.
static int dm_mg_run_scan(dm_grid* g, const MgShape& sh, bool off_map, const double* d_pose4, const float* d_ranges,
                          int32_t* res, uint64_t* stats) {
  using namespace dm_mg;
  hipStream_t s = g->stream;
  Cand* best = (Cand*)g->mg_best.get();
  Cand* cand = (Cand*)g->mg_cand.get();
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
  if (off_map) {
    // every candidate reads cells out of the grid only: the initial best stands
    hipLaunchKernelGGL(k_mg_fold, dim3(1), dim3(kThreads), 0, s, cand, (const uint32_t*)nullptr, 0, sh.k0, best,
                       g->mg_nused, g->h_mg.dev());
    DM_HIP(hipGetLastError());
    DM_HIP(hipStreamSynchronize(s));
  } else if (sh.exhaustive) {
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
                         g->mg_nused, g->h_mg.dev());
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
                         g->h_mg.dev());
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
  stats[1] = sh.exhaustive || off_map ? 0 : (uint64_t)blocks;
  stats[2] = refined;
  stats[3] = rounds;
  return DM_OK;
}

extern "C" {

// ---- scan matcher (csrc/dm_match.h): response field, score volume, best
// candidate ----------------------------------------------------------------------

static int match_check_table(int32_t smear_cells, const uint8_t* kern) {
  if (smear_cells < 0 || smear_cells > 16)
    return dm_set_error(DM_ERR_INVALID_ARG, "smear_cells must be in [0, 16] (got %d)", smear_cells);
  if (!kern) return dm_set_error(DM_ERR_INVALID_ARG, "kern is NULL");
  return DM_OK;
}

// The field's table and map version: a change drops every built tile.
static int match_set_table(dm_grid* g, int32_t r, const uint8_t* kern) {
  int rc = DM_OK;
  if (!g->match_V) {
    if ((rc = g->match_kern.alloc(16 * 16 + 1, "smear table"))) return rc;
    if ((rc = g->match_tiles.alloc(g->NT, "match tile list"))) return rc;
    if ((rc = g->match_V.alloc(g->W * g->H, "response field"))) return rc;
    g->match_r = -1;
  }
  const size_t n = (size_t)r * r + 1;
  const uint64_t version = dm_map_version(g);
  if (g->match_r == r && g->match_version == version && g->match_kern_h.size() == n &&
      memcmp(g->match_kern_h.data(), kern, n) == 0)
    return DM_OK;
  g->match_r = -1;
  g->match_built.assign((size_t)g->NT, 0);
  ++g->match_epoch;
  g->match_kern_h.assign(kern, kern + n);
  // pageable source: the copy is staged before the call returns
  DM_HIP(hipMemcpyAsync(g->match_kern, g->match_kern_h.data(), n, hipMemcpyHostToDevice, g->stream));
  g->match_r = r;
  g->match_version = version;
  return DM_OK;
}

// Build the tiles of `want` (one flag per tile) that the field does not hold yet.
static int match_build_tiles(dm_grid* g, const std::vector<uint8_t>& want) {
  std::vector<int32_t> list;
  for (int64_t t = 0; t < g->NT; ++t)
    if (want[(size_t)t] && !g->match_built[(size_t)t]) list.push_back((int32_t)t);
  if (list.empty()) return DM_OK;
  bool mono = true;  // kern does not increase in d2: the nearest occupied cell decides
  for (size_t i = 1; i < g->match_kern_h.size(); ++i) mono = mono && g->match_kern_h[i] <= g->match_kern_h[i - 1];
  DM_HIP(hipMemcpyAsync(g->match_tiles, list.data(), sizeof(int32_t) * list.size(), hipMemcpyHostToDevice, g->stream));
  DM_HIP(hipStreamSynchronize(g->stream));  // `list` is a local
  int rc = dm_match_launch_field(g, (int32_t)list.size(), g->match_r, mono);
  if (rc) return rc;
  for (int32_t t : list) g->match_built[(size_t)t] = 1;
  return DM_OK;
}

// Diagnostic: the tiles match_V holds for the current table and map version,
// and how many 64 x 64 tiles of the pooled field stand on them.
int dm_match_built(dm_grid* g, uint8_t* field_tiles, int64_t cap, int64_t* n_field, int64_t* n_pool) {
  int rc = dm_check_whole_map(g, "dm_match_built");
  if (rc) return rc;
  if (!n_field || !n_pool) return dm_set_error(DM_ERR_INVALID_ARG, "n_field / n_pool is NULL");
  if (field_tiles && cap < g->NT)
    return dm_set_error(DM_ERR_CAPACITY, "field_tiles holds %lld flags, the map has %lld tiles", (long long)cap,
                        (long long)g->NT);
  const bool valid = g->match_V && g->match_r >= 0 && g->match_version == dm_map_version(g) &&
                     g->match_built.size() == (size_t)g->NT;
  int64_t nf = 0, np = 0;
  for (int64_t t = 0; t < g->NT; ++t) {
    const uint8_t b = valid && g->match_built[(size_t)t] ? 1 : 0;
    if (field_tiles) field_tiles[t] = b;
    nf += b;
  }
  if (valid && g->mg_pool && g->mg_pool_epoch == g->match_epoch)
    for (uint8_t b : g->mg_pool_built) np += b ? 1 : 0;
  *n_field = nf;
  *n_pool = np;
  return DM_OK;
}

// Mark in `want` (one flag per field tile) the tiles that the cells
// [fx0, fx1] x [fy0, fy1] lie in; the part outside the map marks nothing.
static void match_want_cells(const dm_grid* g, double fx0, double fx1, double fy0, double fy1,
                             std::vector<uint8_t>& want) {
  if (!(fx1 >= 0.0 && fy1 >= 0.0 && fx0 < (double)g->W && fy0 < (double)g->H)) return;
  const int64_t tx0 = (int64_t)std::max(fx0, 0.0) / DM_TILE, ty0 = (int64_t)std::max(fy0, 0.0) / DM_TILE;
  const int64_t tx1 = (int64_t)std::min(fx1, (double)(g->W - 1)) / DM_TILE;
  const int64_t ty1 = (int64_t)std::min(fy1, (double)(g->H - 1)) / DM_TILE;
  for (int64_t ty = ty0; ty <= ty1; ++ty)
    for (int64_t tx = tx0; tx <= tx1; ++tx) want[(size_t)(ty * g->TX + tx)] = 1;
}

// The buffers both matchers read their scans from: S * A candidate poses, the
// beam-angle table, the ranges, and n_q fine coordinates.
static int match_grow_inputs(dm_grid* g, int32_t S, int32_t N, int32_t A, int64_t n_q) {
  int rc = DM_OK;
  if ((rc = g->match_pose4.ensure(4 * (int64_t)S * A, "candidate poses")) ||
      (rc = g->match_trig.ensure(2 * (int64_t)N, "beam angle table")) ||
      (rc = g->match_ranges.ensure((int64_t)S * N, "ranges")) ||
      (rc = g->match_q.ensure(n_q, "fine coordinates")))
    return rc;
  return DM_OK;
}

// Fill and enqueue the uploads of those inputs: host trigonometry with the C
// library, as dm_integrate: the beam angle table and (x, y, cos, sin) of every
// candidate yaw (one double add each).  Does not wait: `trig` and `pose4`
// are the caller's, to keep until it has synchronised the stream.
static int match_upload_inputs(dm_grid* g, int32_t S, const double* poses, int32_t N, const float* ranges,
                               float angle_min, float angle_increment, int32_t A, const double* yaw_offsets,
                               std::vector<double>& trig, std::vector<double>& pose4) {
  trig.resize(2 * (size_t)N);
  pose4.resize(4 * (size_t)S * A);
  for (int32_t i = 0; i < N; ++i) {
    const double phi = (double)angle_min + (double)i * (double)angle_increment;
    trig[2 * (size_t)i] = cos(phi);
    trig[2 * (size_t)i + 1] = sin(phi);
  }
  for (int32_t s = 0; s < S; ++s)
    for (int32_t k = 0; k < A; ++k) {
      const double yk = poses[3 * s + 2] + yaw_offsets[k];
      double* p4 = &pose4[4 * ((size_t)s * A + k)];
      p4[0] = poses[3 * s];
      p4[1] = poses[3 * s + 1];
      p4[2] = cos(yk);
      p4[3] = sin(yk);
    }
  hipStream_t st = g->stream;
  DM_HIP(hipMemcpyAsync(g->match_pose4, pose4.data(), sizeof(double) * pose4.size(), hipMemcpyHostToDevice, st));
  if (N > 0) {
    DM_HIP(hipMemcpyAsync(g->match_trig, trig.data(), sizeof(double) * trig.size(), hipMemcpyHostToDevice, st));
    DM_HIP(hipMemcpyAsync(g->match_ranges, ranges, sizeof(float) * (size_t)S * N, hipMemcpyHostToDevice, st));
  }
  return DM_OK;
}

int dm_match_field(dm_grid* g, int32_t smear_cells, const uint8_t* kern, uint8_t* out) {
  int rc = dm_check_whole_map(g, "dm_match_field");
  if (rc || (rc = use_device(g))) return rc;
  if ((rc = match_check_table(smear_cells, kern))) return rc;
  if (!out) return dm_set_error(DM_ERR_INVALID_ARG, "out is NULL");
  DM_HIP(dm_sync_all(g));
  if ((rc = match_set_table(g, smear_cells, kern))) return rc;
  if ((rc = match_build_tiles(g, std::vector<uint8_t>((size_t)g->NT, 1)))) return rc;
  DM_HIP(hipMemcpyAsync(out, g->match_V, (size_t)(g->W * g->H), hipMemcpyDeviceToHost, g->stream));
  DM_HIP(hipStreamSynchronize(g->stream));
  return DM_OK;
}

int dm_match_scans(dm_grid* g, int32_t S, const double* poses, int32_t N, const float* ranges, float angle_min,
                   float angle_increment, int32_t A, const double* yaw_offsets, int32_t k0, int32_t sub,
                   int32_t half, int32_t stride, int32_t smear_cells, const uint8_t* kern, int32_t* out_best,
                   uint32_t* out_score, int32_t* out_n_used, double* out_pose, uint32_t* out_volume) {
  int rc = dm_check_whole_map(g, "dm_match_scans");
  if (rc || (rc = use_device(g))) return rc;
  if ((rc = check_integrate_args(S, N, poses, ranges))) return rc;
  if (A < 1 || A > 64) return dm_set_error(DM_ERR_INVALID_ARG, "A must be in [1, 64] (got %d)", A);
  if (k0 < 0 || k0 >= A) return dm_set_error(DM_ERR_INVALID_ARG, "k0 must be in [0, A) (got %d, A = %d)", k0, A);
  if (sub < 1 || sub > 16) return dm_set_error(DM_ERR_INVALID_ARG, "sub must be in [1, 16] (got %d)", sub);
  if (half < 0 || half > 32) return dm_set_error(DM_ERR_INVALID_ARG, "half must be in [0, 32] (got %d)", half);
  if (stride < 1 || stride > 16)
    return dm_set_error(DM_ERR_INVALID_ARG, "stride must be in [1, 16] (got %d)", stride);
  if ((rc = match_check_table(smear_cells, kern))) return rc;
  if (!yaw_offsets) return dm_set_error(DM_ERR_INVALID_ARG, "yaw_offsets is NULL");
  if (S > 0 && (!poses || !out_best || !out_score || !out_n_used || !out_pose))
    return dm_set_error(DM_ERR_INVALID_ARG, "poses / out_best / out_score / out_n_used / out_pose is NULL");
  if ((int64_t)S * A * std::max(N, 1) > (1ll << 31) - 1)
    return dm_set_error(DM_ERR_SHAPE, "S*A*N must be < 2^31");
  if (S == 0) return DM_OK;
  DM_HIP(dm_sync_all(g));  // after everything enqueued on the handle, on every stream of it
  if ((rc = match_set_table(g, smear_cells, kern))) return rc;

  const int64_t SA = (int64_t)S * A, T1 = 2 * half + 1, T = T1 * T1;
  if ((rc = match_grow_inputs(g, S, N, A, SA * N)) ||
      (rc = g->match_vol.ensure(SA * T, "score volume")) ||
      (rc = g->match_out.ensure(5 * (int64_t)S, "match results")))
    return rc;

  // the tiles the search windows reach: every used beam ends within range_max
  // of its pose and a translation moves it by at most half * stride fine
  // steps; two cells of slack cover the rounding of the endpoint arithmetic
  const double step = g->p.resolution / (double)sub;
  std::vector<uint8_t> want((size_t)g->NT, 0);
  const double reach = (double)g->p.range_max + (double)(half * stride + 1) * step + 2.0 * g->p.resolution;
  for (int32_t s = 0; s < S; ++s) {
    const double x = poses[3 * s], y = poses[3 * s + 1];
    if (!(isfinite(x) && isfinite(y)) || N == 0) continue;
    match_want_cells(g, floor((x - reach - g->p.origin_x) / g->p.resolution) - 1.0,
                     floor((x + reach - g->p.origin_x) / g->p.resolution) + 1.0,
                     floor((y - reach - g->p.origin_y) / g->p.resolution) - 1.0,
                     floor((y + reach - g->p.origin_y) / g->p.resolution) + 1.0, want);
  }
  if ((rc = match_build_tiles(g, want))) return rc;

  hipStream_t st = g->stream;
  std::vector<double> trig, pose4;  // alive until the wait below
  if ((rc = match_upload_inputs(g, S, poses, N, ranges, angle_min, angle_increment, A, yaw_offsets, trig, pose4)))
    return rc;
  if ((rc = dm_match_launch_scans(g, S, N, A, k0, sub, half, stride))) return rc;
  std::vector<int32_t> res(5 * (size_t)S);
  DM_HIP(hipMemcpyAsync(res.data(), g->match_out, sizeof(int32_t) * res.size(), hipMemcpyDeviceToHost, st));
  if (out_volume)
    DM_HIP(hipMemcpyAsync(out_volume, g->match_vol, sizeof(uint32_t) * (size_t)(SA * T), hipMemcpyDeviceToHost, st));
  DM_HIP(hipStreamSynchronize(st));
  for (int32_t s = 0; s < S; ++s) {
    const int32_t k = res[4 * (size_t)s], i = res[4 * (size_t)s + 1], j = res[4 * (size_t)s + 2];
    out_best[3 * s] = k;
    out_best[3 * s + 1] = i;
    out_best[3 * s + 2] = j;
    out_score[s] = (uint32_t)res[4 * (size_t)s + 3];
    out_n_used[s] = res[4 * (size_t)S + s];
    out_pose[3 * s] = poses[3 * s] + (double)(i * stride) * step;
    out_pose[3 * s + 1] = poses[3 * s + 1] + (double)(j * stride) * step;
    out_pose[3 * s + 2] = poses[3 * s + 2] + yaw_offsets[k];
  }
  return DM_OK;
}

// ---- whole-window relocalisation (csrc/dm_match_global.h) -----------------------

static int ensure_match_global(dm_grid* g) {
  int rc = DM_OK;
  if (!g->h_mg) {
    if ((rc = g->h_mg.alloc(8, hipHostMallocMapped | hipHostMallocCoherent, "relocalisation rounds"))) return rc;
    memset(g->h_mg, 0, sizeof(uint32_t) * 8);
  }
  if (g->mg_best) return DM_OK;  // allocated last
  if ((rc = g->mg_hist.alloc(2048, "bound histogram"))) return rc;
  if ((rc = g->mg_ctl.alloc(4, "round control words"))) return rc;
  if ((rc = g->mg_list.alloc(dm_grid::kMgExhaustiveBatch, "round block list"))) return rc;
  if ((rc = g->mg_cand.alloc(dm_grid::kMgExhaustiveBatch, "round candidates"))) return rc;
  if ((rc = g->mg_nused.alloc(1, "used beams"))) return rc;
  return g->mg_best.alloc(1, "best candidate");
}

int dm_match_global(dm_grid* g, int32_t S, const double* poses, int32_t N, const float* ranges, float angle_min,
                    float angle_increment, int32_t A, const double* yaw_offsets, int32_t k0, int32_t half_x,
                    int32_t half_y, int32_t block, int32_t exhaustive, int32_t smear_cells, const uint8_t* kern,
                    int32_t* out_best, uint32_t* out_score, int32_t* out_n_used, double* out_pose,
                    uint64_t* out_stats) {
  int rc = dm_check_whole_map(g, "dm_match_global");
  if (rc || (rc = use_device(g))) return rc;
  if ((rc = check_integrate_args(S, N, poses, ranges))) return rc;
  if (A < 1 || A > 1024) return dm_set_error(DM_ERR_INVALID_ARG, "A must be in [1, 1024] (got %d)", A);
  if (k0 < 0 || k0 >= A) return dm_set_error(DM_ERR_INVALID_ARG, "k0 must be in [0, A) (got %d, A = %d)", k0, A);
  if (half_x < 0 || half_x > 4096 || half_y < 0 || half_y > 4096)
    return dm_set_error(DM_ERR_INVALID_ARG, "half_x and half_y must be in [0, 4096] (got %d, %d)", half_x, half_y);
  if (block != 4 && block != 8 && block != 16 && block != 32)
    return dm_set_error(DM_ERR_INVALID_ARG, "block must be 4, 8, 16 or 32 (got %d)", block);
  if (exhaustive != 0 && exhaustive != 1)
    return dm_set_error(DM_ERR_INVALID_ARG, "exhaustive must be 0 or 1 (got %d)", exhaustive);
  if ((rc = match_check_table(smear_cells, kern))) return rc;
  if (!yaw_offsets) return dm_set_error(DM_ERR_INVALID_ARG, "yaw_offsets is NULL");
  if (S > 0 && (!poses || !out_best || !out_score || !out_n_used || !out_pose))
    return dm_set_error(DM_ERR_INVALID_ARG, "poses / out_best / out_score / out_n_used / out_pose is NULL");
  if ((int64_t)A * std::max(N, 1) > (1ll << 31) - 1) return dm_set_error(DM_ERR_SHAPE, "A*N must be < 2^31");
  if (g->W > (1ll << 20) || g->H > (1ll << 20))
    return dm_set_error(DM_ERR_SHAPE, "dm_match_global needs a map of at most 2^20 cells a side");
  MgShape sh;
  sh.N = N;
  sh.A = A;
  sh.k0 = k0;
  sh.half_x = half_x;
  sh.half_y = half_y;
  sh.lb = block == 4 ? 2 : block == 8 ? 3 : block == 16 ? 4 : 5;
  sh.nbx = (2 * half_x + 1 + block - 1) / block;
  sh.nby = (2 * half_y + 1 + block - 1) / block;
  sh.exhaustive = exhaustive;
  const int64_t blocks = (int64_t)A * sh.nbx * sh.nby;
  if (blocks > (1ll << 26))
    return dm_set_error(DM_ERR_CAPACITY, "%lld blocks per scan, the limit is 2^26: use a larger block (got %d)",
                        (long long)blocks, block);
  // the pooled field's extended coordinates e = c + block - 1, padded to whole blocks
  const int64_t EWB = (g->W + block - 1 + block - 1) / block, EHB = (g->H + block - 1 + block - 1) / block;
  if ((int64_t)block * block * EWB * EHB > (1ll << 31) - 1)
    return dm_set_error(DM_ERR_SHAPE, "dm_match_global: the pooled field of this map needs 2^31 bytes or more");
  sh.EWB = (int32_t)EWB;
  sh.EHB = (int32_t)EHB;
  const int64_t PTX = (EWB * block + 63) / 64, PTY = (EHB * block + 63) / 64;
  if (S == 0) return DM_OK;
  DM_HIP(dm_sync_all(g));  // after everything enqueued on the handle, on every stream of it
  if ((rc = match_set_table(g, smear_cells, kern))) return rc;
  if ((rc = ensure_match_global(g))) return rc;

  if ((rc = match_grow_inputs(g, S, N, A, (int64_t)A * N))) return rc;
  if (!exhaustive) {
    if ((rc = g->mg_bound.ensure(blocks, "block bounds")) ||
        (rc = g->mg_pool.ensure((int64_t)block * block * EWB * EHB, "pooled response field")) ||
        (rc = g->mg_ptiles.ensure(PTX * PTY, "pool tile list")))
      return rc;
    if (g->mg_pool_block != block || g->mg_pool_epoch != g->match_epoch ||
        g->mg_pool_built.size() != (size_t)(PTX * PTY)) {
      g->mg_pool_built.assign((size_t)(PTX * PTY), 0);
      g->mg_pool_block = block;
      g->mg_pool_epoch = g->match_epoch;
    }
  }

  const double res = g->p.resolution;
  hipStream_t st = g->stream;
  std::vector<double> trig, pose4;
  if ((rc = match_upload_inputs(g, S, poses, N, ranges, angle_min, angle_increment, A, yaw_offsets, trig, pose4)))
    return rc;
  DM_HIP(hipStreamSynchronize(st));  // pose4 and trig are locals

  for (int32_t s = 0; s < S; ++s) {
    const double x = poses[3 * s], y = poses[3 * s + 1];
    int32_t r5[5] = {k0, 0, 0, 0, 0};
    uint64_t stats[4] = {(uint64_t)blocks, 0, 0, 0};
    if (N > 0 && isfinite(x) && isfinite(y)) {
      // the cells the window reaches: every used beam ends within range_max of
      // the pose and a translation moves it by at most half cells; two cells
      // of slack cover the rounding of the endpoint arithmetic
      const double reach_x = (double)g->p.range_max + (double)(half_x + 1) * res + 2.0 * res;
      const double reach_y = (double)g->p.range_max + (double)(half_y + 1) * res + 2.0 * res;
      const double fx0 = floor((x - reach_x - g->p.origin_x) / res) - 1.0;
      const double fx1 = floor((x + reach_x - g->p.origin_x) / res) + 1.0;
      const double fy0 = floor((y - reach_y - g->p.origin_y) / res) - 1.0;
      const double fy1 = floor((y + reach_y - g->p.origin_y) / res) + 1.0;
      std::vector<uint8_t> want((size_t)g->NT, 0);
      std::vector<int32_t> plist;
      if (exhaustive) {
        match_want_cells(g, fx0, fx1, fy0, fy1, want);
      } else {
        // M_B is read at the cells c in [f0, f1] with c >= -(block - 1): the
        // pool tiles that hold them, and for each the field tiles its patch
        // [64 p - (block - 1), 64 p + 63] meets
        const double lo = -(double)(block - 1);
        if (fx1 >= lo && fy1 >= lo && fx0 < (double)g->W && fy0 < (double)g->H) {
          const int64_t px0 = ((int64_t)std::max(fx0, lo) + block - 1) / 64;
          const int64_t py0 = ((int64_t)std::max(fy0, lo) + block - 1) / 64;
          const int64_t px1 = ((int64_t)std::min(fx1, (double)(g->W - 1)) + block - 1) / 64;
          const int64_t py1 = ((int64_t)std::min(fy1, (double)(g->H - 1)) + block - 1) / 64;
          for (int64_t py = py0; py <= py1; ++py)
            for (int64_t px = px0; px <= px1; ++px) {
              if (!g->mg_pool_built[(size_t)(py * PTX + px)]) plist.push_back((int32_t)(py * PTX + px));
              match_want_cells(g, (double)(64 * px - (block - 1)), (double)(64 * px + 63),
                               (double)(64 * py - (block - 1)), (double)(64 * py + 63), want);
            }
        }
      }
      if ((rc = match_build_tiles(g, want))) return rc;
      if (!plist.empty()) {
        DM_HIP(hipMemcpyAsync(g->mg_ptiles, plist.data(), sizeof(int32_t) * plist.size(), hipMemcpyHostToDevice, st));
        DM_HIP(hipStreamSynchronize(st));  // `plist` is a local
        if ((rc = dm_mg_launch_pool(g, (int32_t)plist.size(), sh.lb, sh.EWB, sh.EHB, (int32_t)PTX))) return rc;
        for (int32_t t : plist) g->mg_pool_built[(size_t)t] = 1;
      }
      const bool off_map = !(fx1 >= 0.0 && fy1 >= 0.0 && fx0 < (double)g->W && fy0 < (double)g->H);
      if ((rc = dm_mg_run_scan(g, sh, off_map, g->match_pose4 + 4 * (size_t)s * A, g->match_ranges + (size_t)s * N,
                               r5, stats)))
        return rc;
    }
    const int32_t k = r5[0], i = r5[1], j = r5[2];
    out_best[3 * s] = k;
    out_best[3 * s + 1] = i;
    out_best[3 * s + 2] = j;
    out_score[s] = (uint32_t)r5[3];
    out_n_used[s] = r5[4];
    out_pose[3 * s] = poses[3 * s] + (double)i * res;
    out_pose[3 * s + 1] = poses[3 * s + 1] + (double)j * res;
    out_pose[3 * s + 2] = poses[3 * s + 2] + yaw_offsets[k];
    if (out_stats)
      for (int m = 0; m < 4; ++m) out_stats[4 * s + m] = stats[m];
  }
  return DM_OK;
}

}  // extern "C"
