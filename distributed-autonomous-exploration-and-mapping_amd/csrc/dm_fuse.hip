// dm_fuse.hip — map fusion (include/dm.h: dm_fuse_logodds, dm_fuse_state,
// dm_fuse_grid): a peer's occupancy map, placed in our frame by a rigid
// transform, folded into the device-resident map.  The reference has no such
// step (its robots share no map, server/thymio_project/thymio_project/
// main.py:80-81); it is the merge step of a multi-robot stack.
//
// One kernel, k_fuse<T>: one workgroup per 64 x 64 destination tile of the
// tiles the transformed source can reach, a wave per row (lanes along x, so L
// and state move in full lines), the source read by direct global gathers:
// under rotation a row of destination cells reads the source along a slanted
// line, adjacent lanes hitting adjacent or identical cells.  Every destination
// cell has one writer: no atomics on map cells.  The tile summaries
// (tile_free, tile list, fmask, fedge, tile_seen) are rebuilt by the full
// dm_launch_recount that follows, as after dm_set_logodds.
#include <math.h>

#include <algorithm>

#include "dm_internal.h"

namespace {

constexpr int kFuseThreads = 256;
constexpr int kFuseBatch = 8;  // rows a lane has in flight
static_assert(DM_TILE % ((kFuseThreads / 64) * kFuseBatch) == 0, "batches cover a tile's rows");

struct FuseArgs {
  // destination: global geometry and the rows this handle owns
  double ox, oy, res;
  // source -> destination transform and the source's geometry
  double tx, ty, c, s;
  double sox, soy, sres;
  double sw_d, sh_d;  // (double)width, (double)height of the source
  int64_t W, R, row0;
  int64_t sw;
  float l_occ, l_free, l_min, l_max, occ_t, free_t;
  int32_t tile_x0, tile_y0;  // first tile of the launched rectangle
  int32_t fill;              // DM_FUSE_FILL
  int32_t pad;
};

// the source's contribution at source cell i (include/dm.h)
__device__ inline float fuse_value(const FuseArgs&, const float* __restrict__ src, int64_t i) {
  const float v = src[i];
  return isfinite(v) ? v : 0.0f;
}
__device__ inline float fuse_value(const FuseArgs& a, const int8_t* __restrict__ src, int64_t i) {
  const int8_t v = src[i];
  return v == 100 ? a.l_occ : (v == 0 ? a.l_free : 0.0f);
}

__device__ inline uint32_t wave_sum(uint32_t v) {
  for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
  return v;
}

template <class T>
__global__ __launch_bounds__(kFuseThreads) void k_fuse(FuseArgs a, const T* __restrict__ src, float* __restrict__ L,
                                                       int8_t* __restrict__ state, unsigned long long* __restrict__ stats) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t cx = ((int64_t)a.tile_x0 + blockIdx.x) * DM_TILE + lane;
  const int64_t ly0 = ((int64_t)a.tile_y0 + blockIdx.y) * DM_TILE;
  uint32_t n_cov = 0, n_con = 0, n_chg = 0;
  const bool in_x = cx < a.W;
  const double wx = a.ox + ((double)cx + 0.5) * a.res;
  const double dx = wx - a.tx;
  const double cdx = a.c * dx, sdx = a.s * dx;
  // A lane's 16 rows in batches of kFuseBatch: the batch's source gathers and
  // L loads are all issued before the first is used (a row at a time, the
  // gather and then the L load behind its test, is two dependent memory
  // latencies per row: 3x the byte model's time).  Lanes with
  // nothing to read load element 0.
  for (int b = 0; b < DM_TILE / (kFuseThreads / 64) / kFuseBatch; ++b) {
    bool cov[kFuseBatch];
    int64_t si[kFuseBatch], di[kFuseBatch];
    bool any = false;
#pragma unroll
    for (int j = 0; j < kFuseBatch; ++j) {
      const int64_t ly = ly0 + wave + (kFuseThreads / 64) * (b * kFuseBatch + j);  // band-local row
      const double wy = a.oy + ((double)(a.row0 + ly) + 0.5) * a.res;
      const double dy = wy - a.ty;
      const double sx = cdx + a.s * dy;
      const double sy = a.c * dy - sdx;
      const double qx = floor((sx - a.sox) / a.sres);
      const double qy = floor((sy - a.soy) / a.sres);
      // NaN compares false: a non-finite sx / sy is never covered
      cov[j] = in_x && ly < a.R && isfinite(sx) && isfinite(sy) && qx >= 0.0 && qx < a.sw_d && qy >= 0.0 &&
               qy < a.sh_d;
      // converted only where covered: elsewhere qx / qy may be NaN or beyond int64
      si[j] = (int64_t)(cov[j] ? qy : 0.0) * a.sw + (int64_t)(cov[j] ? qx : 0.0);
      di[j] = cov[j] ? ly * a.W + cx : 0;
      any |= cov[j];
    }
    if (__ballot(any) == 0ull) continue;  // wave-uniform: no cell of these rows is covered
    float l[kFuseBatch], old[kFuseBatch];
#pragma unroll
    for (int j = 0; j < kFuseBatch; ++j) {
      l[j] = fuse_value(a, src, si[j]);
      old[j] = L[di[j]];
    }
#pragma unroll
    for (int j = 0; j < kFuseBatch; ++j) {
      const bool con = cov[j] && l[j] != 0.0f && !(a.fill && old[j] != 0.0f);
      const float v = dm_clamp_a6(a.fill ? l[j] : old[j] + l[j], a.l_min, a.l_max);
      // the state byte is a7 of L everywhere (dm_internal.h, INVARIANT 2): no need to read it
      const int8_t st = dm_state_a7(v, a.occ_t, a.free_t), st_old = dm_state_a7(old[j], a.occ_t, a.free_t);
      n_cov += cov[j];
      n_con += con;
      if (con) {
        L[di[j]] = v;
        if (st != st_old) {
          state[di[j]] = st;
          ++n_chg;
        }
      }
    }
  }
  __shared__ uint32_t s_sum[kFuseThreads / 64][3];
  n_cov = wave_sum(n_cov);
  n_con = wave_sum(n_con);
  n_chg = wave_sum(n_chg);
  if (lane == 0) {
    s_sum[wave][0] = n_cov;
    s_sum[wave][1] = n_con;
    s_sum[wave][2] = n_chg;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    uint32_t t = 0;
    for (int w = 0; w < kFuseThreads / 64; ++w) t += s_sum[w][threadIdx.x];
    if (t) atomicAdd(stats + threadIdx.x, (unsigned long long)t);
  }
}

int check_source(const dm_fuse_source* src) {
  if (!src) return dm_set_error(DM_ERR_INVALID_ARG, "src is NULL");
  if (src->width < 1 || src->width > 32768 || src->height < 1 || src->height > 32768)
    return dm_set_error(DM_ERR_INVALID_ARG, "source size %lld x %lld outside [1, 32768]", (long long)src->width,
                        (long long)src->height);
  if (!isfinite(src->resolution) || !(src->resolution > 0.0))
    return dm_set_error(DM_ERR_INVALID_ARG, "source resolution must be finite and > 0");
  if (!isfinite(src->origin_x) || !isfinite(src->origin_y))
    return dm_set_error(DM_ERR_INVALID_ARG, "source origin must be finite");
  return DM_OK;
}

int check_transform(double tx, double ty, double yaw, int32_t mode) {
  if (!isfinite(tx) || !isfinite(ty) || !isfinite(yaw))
    return dm_set_error(DM_ERR_INVALID_ARG, "tx, ty and yaw must be finite");
  if (mode != DM_FUSE_ADD && mode != DM_FUSE_FILL) return dm_set_error(DM_ERR_INVALID_ARG, "unknown mode %d", mode);
  return DM_OK;
}

// The destination tiles the source can cover: the bounding box of its four
// transformed corners in destination cells (band-local rows), widened by one
// cell, clipped to the handle's tiles.  The kernel decides coverage per cell
// by the definition; this only has to be a superset, and a cell of slack is
// orders of magnitude above the doubles' rounding unless the coordinates are
// astronomically large, in which case every tile is launched.  false: no tile.
bool fuse_tile_rect(const dm_grid* g, const dm_fuse_source& src, double tx, double ty, double c, double s,
                    int64_t* x0, int64_t* y0, int64_t* x1, int64_t* y1) {
  const double ux[2] = {src.origin_x, src.origin_x + (double)src.width * src.resolution};
  const double uy[2] = {src.origin_y, src.origin_y + (double)src.height * src.resolution};
  double lox = INFINITY, loy = INFINITY, hix = -INFINITY, hiy = -INFINITY;
  bool all = false;
  for (int i = 0; i < 2; ++i)
    for (int j = 0; j < 2; ++j) {
      const double px = (c * ux[i] - s * uy[j] + tx - g->p.origin_x) / g->p.resolution;
      const double py = (s * ux[i] + c * uy[j] + ty - g->p.origin_y) / g->p.resolution - (double)g->row0;
      if (!isfinite(px) || !isfinite(py) || fabs(px) > 1e12 || fabs(py) > 1e12) all = true;
      lox = std::min(lox, px); hix = std::max(hix, px);
      loy = std::min(loy, py); hiy = std::max(hiy, py);
    }
  int64_t cx0 = 0, cy0 = 0, cx1 = g->W - 1, cy1 = g->R - 1;
  if (!all) {
    if (hix < -1.0 || hiy < -1.0 || lox > (double)g->W + 1.0 || loy > (double)g->R + 1.0) return false;
    cx0 = std::max<int64_t>(cx0, (int64_t)floor(lox) - 1);
    cy0 = std::max<int64_t>(cy0, (int64_t)floor(loy) - 1);
    cx1 = std::min<int64_t>(cx1, (int64_t)std::min(floor(hix) + 1.0, (double)g->W));
    cy1 = std::min<int64_t>(cy1, (int64_t)std::min(floor(hiy) + 1.0, (double)g->R));
    if (cx0 > cx1 || cy0 > cy1) return false;
  }
  *x0 = cx0 / DM_TILE; *x1 = cx1 / DM_TILE;
  *y0 = cy0 / DM_TILE; *y1 = cy1 / DM_TILE;
  return true;
}

// The fusion on one (non-sharded) handle from a device-resident source.
template <class T>
int fuse_device(dm_grid* g, const dm_fuse_source& src, const T* d_src, double tx, double ty, double yaw,
                int32_t mode, uint64_t* out_stats) {
  const double c = cos(yaw), s = sin(yaw);
  // three device words kept in the handle: no allocation (and no hipFree, which waits for the whole device) per call
  int rc = g->fuse_stats.ensure(3, "fuse stats");
  if (rc) return rc;
  unsigned long long* d_stats = g->fuse_stats;
  unsigned long long h_stats[3] = {0ull, 0ull, 0ull};
  hipError_t e = dm_sync_all(g);  // ordered after everything enqueued on the handle, on every stream of it
  if (e == hipSuccess) e = hipMemsetAsync(d_stats, 0, sizeof(h_stats), g->stream);
  int64_t x0, y0, x1, y1;
  if (e == hipSuccess && fuse_tile_rect(g, src, tx, ty, c, s, &x0, &y0, &x1, &y1)) {
    FuseArgs a;
    a.ox = g->p.origin_x; a.oy = g->p.origin_y; a.res = g->p.resolution;
    a.tx = tx; a.ty = ty; a.c = c; a.s = s;
    a.sox = src.origin_x; a.soy = src.origin_y; a.sres = src.resolution;
    a.sw_d = (double)src.width; a.sh_d = (double)src.height;
    a.W = g->W; a.R = g->R; a.row0 = g->row0;
    a.sw = src.width;
    a.l_occ = g->p.l_occ; a.l_free = g->p.l_free;
    // zero bounds and thresholds read as +0 (include/dm.h, dm_params)
    a.l_min = g->p.l_min == 0.0f ? 0.0f : g->p.l_min;
    a.l_max = g->p.l_max == 0.0f ? 0.0f : g->p.l_max;
    a.occ_t = g->p.occ_thresh == 0.0f ? 0.0f : g->p.occ_thresh;
    a.free_t = g->p.free_thresh == 0.0f ? 0.0f : g->p.free_thresh;
    a.tile_x0 = (int32_t)x0; a.tile_y0 = (int32_t)y0;
    a.fill = mode == DM_FUSE_FILL ? 1 : 0;
    a.pad = 0;
    KernelTimer t;
    dm_timer_begin(g, "fuse", &t);
    DM_LAUNCH(k_fuse<T>, dim3((unsigned)(x1 - x0 + 1), (unsigned)(y1 - y0 + 1)), dim3(kFuseThreads), 0, g->stream, a,
              d_src, g->L, g->state, d_stats);
    e = hipGetLastError();
    dm_timer_end(g, &t);
    if (e == hipSuccess) {
      // the tile summaries the frontier pass reads (dm_internal.h, INVARIANT)
      rc = dm_launch_recount(g);
    }
  }
  if (e == hipSuccess && !rc)
    e = hipMemcpyAsync(h_stats, d_stats, sizeof(h_stats), hipMemcpyDeviceToHost, g->stream);
  if (e == hipSuccess && !rc) e = hipStreamSynchronize(g->stream);
  if (rc) return rc;
  if (e != hipSuccess) return dm_hip_check(e, "dm_fuse");
  g->frontier_valid = false;
  ++g->integrate_seq;
  if (out_stats)
    for (int i = 0; i < 3; ++i) out_stats[i] = h_stats[i];
  return DM_OK;
}

// from a host source: staged on the handle's device for the call
template <class T>
int fuse_host(dm_grid* g, const dm_fuse_source* src, const T* h_src, double tx, double ty, double yaw, int32_t mode,
              uint64_t* out_stats) {
  int rc = check_grid(g);
  if (rc) return rc;
  if ((rc = check_source(src))) return rc;
  if (!h_src) return dm_set_error(DM_ERR_INVALID_ARG, "the source map is NULL");
  if ((rc = check_transform(tx, ty, yaw, mode))) return rc;
  if ((rc = use_device(g))) return rc;
  const int64_t cells = src->width * src->height;
  DevBuf<T> d;
  if ((rc = d.alloc(cells, "fuse source staging"))) return rc;
  const hipError_t e = hipMemcpy(d, h_src, sizeof(T) * (size_t)cells, hipMemcpyHostToDevice);
  if (e != hipSuccess) return dm_hip_check(e, "fuse source upload");
  return fuse_device(g, *src, d.get(), tx, ty, yaw, mode, out_stats);
}


// the arguments of one call, handed to every band of a sharded parent (dm_sh_fuse)
struct BandCall {
  const dm_fuse_source* src;
  const void* values;
  dm_grid* src_grid;
  double tx, ty, yaw;
  int32_t mode;
};

}  // namespace

extern "C" {

int dm_fuse_logodds(dm_grid* g, const dm_fuse_source* src, const float* L_src, double tx, double ty, double yaw,
                    int32_t mode, uint64_t* out_stats) {
  if (g && g->sh) {
    BandCall c{src, L_src, nullptr, tx, ty, yaw, mode};
    return dm_sh_fuse(g, -1, out_stats, [](dm_grid* b, void* p, uint64_t* st) {
      const BandCall& k = *static_cast<const BandCall*>(p);
      return dm_fuse_logodds(b, k.src, static_cast<const float*>(k.values), k.tx, k.ty, k.yaw, k.mode, st);
    }, &c);
  }
  return fuse_host(g, src, L_src, tx, ty, yaw, mode, out_stats);
}

int dm_fuse_state(dm_grid* g, const dm_fuse_source* src, const int8_t* state_src, double tx, double ty, double yaw,
                  int32_t mode, uint64_t* out_stats) {
  if (g && g->sh) {
    BandCall c{src, state_src, nullptr, tx, ty, yaw, mode};
    return dm_sh_fuse(g, -1, out_stats, [](dm_grid* b, void* p, uint64_t* st) {
      const BandCall& k = *static_cast<const BandCall*>(p);
      return dm_fuse_state(b, k.src, static_cast<const int8_t*>(k.values), k.tx, k.ty, k.yaw, k.mode, st);
    }, &c);
  }
  return fuse_host(g, src, state_src, tx, ty, yaw, mode, out_stats);
}

int dm_fuse_grid(dm_grid* g, dm_grid* s, double tx, double ty, double yaw, int32_t mode, uint64_t* out_stats) {
  if (g && g->sh) {
    if (!s) return dm_set_error(DM_ERR_INVALID_ARG, "src_grid is NULL");
    BandCall c{nullptr, nullptr, s, tx, ty, yaw, mode};
    return dm_sh_fuse(g, s->device, out_stats, [](dm_grid* b, void* p, uint64_t* st) {
      const BandCall& k = *static_cast<const BandCall*>(p);
      return dm_fuse_grid(b, k.src_grid, k.tx, k.ty, k.yaw, k.mode, st);
    }, &c);
  }
  int rc = check_grid(g);
  if (rc) return rc;
  if (!s) return dm_set_error(DM_ERR_INVALID_ARG, "src_grid is NULL");
  if (s == g) return dm_set_error(DM_ERR_INVALID_ARG, "src_grid is the destination");
  if (s->sh || s->row0 != 0 || s->R != s->H)
    return dm_set_error(DM_ERR_INVALID_ARG, "src_grid must be a whole-map dm_create handle");
  if (s->device != g->device)
    return dm_set_error(DM_ERR_INVALID_ARG, "src_grid is on device %d, the destination on %d", s->device, g->device);
  if ((rc = check_transform(tx, ty, yaw, mode))) return rc;
  dm_fuse_source src;
  src.width = s->W; src.height = s->H;
  src.resolution = s->p.resolution;
  src.origin_x = s->p.origin_x; src.origin_y = s->p.origin_y;
  if ((rc = check_source(&src))) return rc;
  if ((rc = use_device(g))) return rc;
  DM_HIP(hipStreamSynchronize(s->stream));
  return fuse_device(g, src, (const float*)s->L, tx, ty, yaw, mode, out_stats);
}

}  // extern "C"
