// dm_plan.h — geodesic distance field over the tiled map:
// the device code of dm_plan_* and dm_assign_goals_path, included by
// dm_goals.hip.
//
// Definitions (integers only, so every result is unique and bit-exact):
//   traversable(c)  state[c] == 0 and no in-grid occupied cell o (state 100)
//                   with dx^2 + dy^2 <= r^2; source cells are traversable
//                   whatever their state; out-of-grid cells are neither
//                   obstacles nor traversable
//   moves           8-connected, orthogonal 5, diagonal 7; a diagonal
//                   (x, y) -> (x+sx, y+sy) needs (x+sx, y) and (x, y+sy)
//                   traversable (no corner cutting); the rule is symmetric
//   cost[c]         least total move cost from any source over traversable
//                   cells, kUnreach where none is <= max_cost
//   d2[c]           clearance for R: the least dx^2 + dy^2 <= R^2 to an in-grid
//                   occupied cell, R^2 + 1 if none (k_plan_clear)
//   weighted move   entering c costs b * (1 + pen[d2[c]]), b = 5 / 7, pen the
//                   caller's uint8 table; the weighted field (k_plan_relax<true, .>,
//                   dm_plan_field_cost) is cost[c] with that move cost
// The host restatement (Dijkstra) is dm/plan.py.
//
// Round structure (k_plan_relax): the host launches rounds over a worklist of
// active tiles.  One workgroup owns a listed tile for the round: it loads the
// tile's 64x64 costs plus a one-cell ring of its 8 neighbours' costs and
// traversable bits into LDS, sweeps min-relaxation there until nothing
// changes, writes back the cells that changed and lists (for the next round)
// every neighbour that faces a changed border cell.  Only the owner writes a
// tile's cells, so the field needs no atomics; values only decrease and every
// stored value is the cost of a real path, so a ring value read while its
// owner is still lowering it is merely an upper bound that the owner's
// listing of this tile corrects in the next round.  Correctness rests on
// kernel boundaries alone: no workgroup waits for another.
//
// A sweep: each wave owns 16 consecutive rows and walks them in alternating
// order, so costs travel down (or up) a wave's band within one sweep; per row
// the 64 lanes relax their cells against the 8 neighbours and then run a
// prefix-min scan along the row from both sides, so costs travel along a
// run of traversable cells within one row visit.  Measured against plain
// one-cell-per-sweep relaxation with the rows interleaved over the waves:
// the scan with interleaved rows 2x slower, the scan with the bands 2.3x
// faster.
#pragma once

#include "dm_internal.h"

namespace dm_plan {

constexpr uint32_t kUnreach = DM_PLAN_UNREACHABLE;
constexpr int kThreads = 256;
constexpr int kRing = DM_TILE + 2;  // tile + one-cell ring
// In-LDS sweeps of one tile visit.  A sweep moves the front by at least one
// cell along a shortest path, a tile-local path has < 4096 cells; a visit
// that stops at the bound lists its own tile again, so the bound only splits
// the work of a maze-like tile over rounds.
constexpr int kMaxSweeps = 1024;

// dm_grid::plan_stat / out_stats order
enum { ST_REACHED = 0, ST_TRAV = 1, ST_ROUNDS = 2, ST_RELAX = 3 };
// mapped host words written by k_plan_relax's first workgroup
enum { HS_LEN = 0, HS_ROUNDS = 1, HS_RELAX = 2, HS_TRAV = 3 };

__device__ inline int trav_bit(const uint64_t* __restrict__ trav, int64_t TX, int64_t x, int64_t y) {
  return (int)((trav[((y >> 6) * TX + (x >> 6)) * DM_TILE + (y & 63)] >> (x & 63)) & 1ull);
}

// The occupied bit rows into s_occ[row = y - y0 + 32][left, centre, right
// word], for k_plan_travers and k_plan_clear.  Called by all kThreads
// threads; the caller places the barrier.
__device__ inline void load_occ_halo(const int8_t* __restrict__ state, const uint8_t* __restrict__ tile_seen,
                                     int64_t W, int64_t H, int64_t TX, int64_t x0, int64_t y0, int32_t r,
                                     unsigned long long (*s_occ)[3]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int j = wave; j < 2 * DM_TILE * 3; j += kThreads / 64) {
    const int row = j / 3, wc = j % 3;
    const int64_t gy = y0 - 32 + row, gx = x0 + (int64_t)(wc - 1) * DM_TILE + lane;
    bool occ = false;
    if (row >= 32 - r && row < 32 + DM_TILE + r && gy >= 0 && gy < H && gx >= 0 && gx < W && gx >= x0 - r &&
        gx < x0 + DM_TILE + r && tile_seen[(gy >> 6) * TX + (gx >> 6)])
      occ = state[gy * W + gx] == 100;
    const unsigned long long word = __ballot(occ);
    if (lane == 0) s_occ[row][wc] = word;
  }
}

// ---- 1. traversability ------------------------------------------------------
// Workgroup = tile.  The occupied bits of the tile's rows with a 32-row halo
// above and below, three 64-bit words per row (the tile's columns and the 64
// to either side; only the r nearest halo columns are read), are dilated by
// the disc: row y takes, for every |dy| <= r, the row y + dy widened by
// hw(|dy|) = floor(sqrt(r^2 - dy^2)) through word shifts.  Tiles no integrate
// item or bulk write has touched (tile_seen == 0) are all unknown: they are
// not read, as halo or as centre.
__global__ __launch_bounds__(kThreads) void k_plan_travers(const int8_t* __restrict__ state,
                                                           const uint8_t* __restrict__ tile_seen, int64_t W,
                                                           int64_t H, int64_t TX, int32_t r,
                                                           uint64_t* __restrict__ trav,
                                                           unsigned long long* __restrict__ stat) {
  __shared__ unsigned long long s_occ[2 * DM_TILE][3];
  __shared__ unsigned long long s_free[DM_TILE];
  __shared__ unsigned long long s_blk[DM_TILE];
  __shared__ int s_hw[33];
  const int64_t tile = blockIdx.x, tx = tile % TX, ty = tile / TX;
  const int64_t x0 = tx * DM_TILE, y0 = ty * DM_TILE;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (!tile_seen[tile]) {  // uniform: every cell unknown, nothing traversable
    if (threadIdx.x < DM_TILE) trav[tile * DM_TILE + threadIdx.x] = 0ull;
    return;
  }
  if ((int)threadIdx.x <= r) {
    const int d = threadIdx.x;
    int h = 0;
    while ((h + 1) * (h + 1) + d * d <= r * r) ++h;
    s_hw[d] = h;
  }
  load_occ_halo(state, tile_seen, W, H, TX, x0, y0, r, s_occ);
  for (int row = wave; row < DM_TILE; row += kThreads / 64) {
    const int64_t gy = y0 + row, gx = x0 + lane;
    const bool fr = gy < H && gx < W && state[gy * W + gx] == 0;
    const unsigned long long word = __ballot(fr);
    if (lane == 0) {
      s_free[row] = word;
      s_blk[row] = 0ull;
    }
  }
  __syncthreads();
  {
    const int y = threadIdx.x >> 2, q = threadIdx.x & 3;
    unsigned long long acc = 0ull;
    for (int dy = -r + q; dy <= r; dy += 4) {
      const int row = y + 32 + dy;
      const unsigned long long L = s_occ[row][0], C = s_occ[row][1], Rr = s_occ[row][2];
      if ((L | C | Rr) == 0ull) continue;
      const int h = s_hw[dy < 0 ? -dy : dy];
      unsigned long long m = C;
      for (int d = 1; d <= h; ++d) m |= (C >> d) | (Rr << (64 - d)) | (C << d) | (L >> (64 - d));
      acc |= m;
    }
    if (acc) atomicOr(&s_blk[y], acc);
  }
  __syncthreads();
  if (threadIdx.x < DM_TILE) {  // wave 0
    const unsigned long long t = s_free[threadIdx.x] & ~s_blk[threadIdx.x];
    trav[tile * DM_TILE + threadIdx.x] = t;
    int c = __popcll(t);
    for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off);
    if (lane == 0 && c) atomicAdd(&stat[ST_TRAV], (unsigned long long)c);
  }
}

// bit rows -> one byte per cell, row-major (dm_plan_traversable's output)
__global__ void k_plan_expand(const uint64_t* __restrict__ trav, int64_t W, int64_t H, int64_t TX,
                              uint8_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= W * H) return;
  out[i] = (uint8_t)trav_bit(trav, TX, i % W, i / W);
}

// ---- 1b. clearance ------------------------------------------------------------
// d2[c] = the least dx^2 + dy^2 <= R^2 to an occupied cell, R^2 + 1 ("far")
// if there is none; for every cell, whatever its state and its tile's
// tile_seen (an untouched tile holds no obstacle but lies near others').
// Workgroup = tile, over the same halo words as k_plan_travers.  A wave
// takes 16 rows, a lane a column: for each dy the three words of row y + dy
// are one LDS address for the whole wave (a broadcast read, and an empty row
// is skipped by a wave-uniform branch), the lane aligns the 128 columns
// around its own to bit 63 (leftwards) and bit 0 (rightwards) and takes the
// nearest set bit by clz / ffs: |dx|, exact, and d2 = min(|dx|^2 + dy^2).
// The other exact form, a vertical distance per column of the 64 + 2R and
// then a minimum over dx, reads one distinct LDS value per lane and dx,
// (2R + 1) non-broadcast reads per cell against (2R + 1) broadcasts here, and
// cannot skip empty rows.
// kPen: write pen[d2] as one byte per cell (the table in LDS), for
// the weighted k_plan_relax; else the uint16 d2 itself (dm_plan_clearance).
template <bool kPen>
__global__ __launch_bounds__(kThreads) void k_plan_clear(const int8_t* __restrict__ state,
                                                         const uint8_t* __restrict__ tile_seen, int64_t W,
                                                         int64_t H, int64_t TX, int32_t R,
                                                         const uint8_t* __restrict__ pen,
                                                         uint16_t* __restrict__ out_d2,
                                                         uint8_t* __restrict__ out_pen) {
  __shared__ unsigned long long s_occ[2 * DM_TILE][3];
  __shared__ uint8_t s_pen[kPen ? 32 * 32 + 2 : 1];
  const int64_t tile = blockIdx.x, tx = tile % TX, ty = tile / TX;
  const int64_t x0 = tx * DM_TILE, y0 = ty * DM_TILE;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  load_occ_halo(state, tile_seen, W, H, TX, x0, y0, R, s_occ);
  if (kPen)
    for (int i = threadIdx.x; i < R * R + 2; i += kThreads) s_pen[i] = pen[i];
  __syncthreads();
  const int far = R * R + 1;
  const int64_t gx = x0 + lane;
  for (int i = 0; i < 16; ++i) {
    const int y = wave * 16 + i;
    int best = far;
    for (int dy = -R; dy <= R; ++dy) {
      const int row = y + 32 + dy;
      const unsigned long long L = s_occ[row][0], C = s_occ[row][1], Rr = s_occ[row][2];
      if ((L | C | Rr) == 0ull) continue;
      // columns x, x - 1, ... from bit 63 down; columns x, x + 1, ... from bit 0 up
      const unsigned long long lw = (C << (63 - lane)) | ((L >> 1) >> lane);
      const unsigned long long rw = (C >> lane) | ((Rr << 1) << (63 - lane));
      const int dl = lw ? __clzll((long long)lw) : 64, dr = rw ? __ffsll((long long)rw) - 1 : 64;
      const int d = min(dl, dr);
      best = min(best, d * d + dy * dy);  // a candidate outside the disc is > R^2: "far" stays below it
    }
    const int64_t gy = y0 + y;
    if (gy < H && gx < W) {
      if (kPen)
        out_pen[gy * W + gx] = s_pen[best];
      else
        out_d2[gy * W + gx] = (uint16_t)best;
    }
  }
}

// ---- 2. relaxation ----------------------------------------------------------
// Source cells: cost 0 and traversable whatever their state.
__global__ void k_plan_sources(const int64_t* __restrict__ src, int32_t n, int64_t W, int64_t TX,
                               uint64_t* __restrict__ travs, uint32_t* __restrict__ cost) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t c = src[i], x = c % W, y = c / W;
  cost[c] = 0u;
  atomicOr((unsigned long long*)&travs[((y >> 6) * TX + (x >> 6)) * DM_TILE + (y & 63)], 1ull << (x & 63));
}

// One round of the plain field (k_plan_relax<false, false>, dm_plan_field), the
// penalty-weighted field (<true, false>, dm_plan_field_cost) or the team's
// fields (<false, true>, dm_plan_team).  The round structure and the argument
// that the field needs no atomics are the file header's and hold for all
// three; the two switches are compile-time, so each instantiation carries
// only its own code.
//
// len[3]: round k reads its list length from len[k % 3], appends to
// len[(k + 1) % 3] and clears len[(k + 2) % 3] (round k - 1's input, which
// nothing reads any more), so no launch between rounds resets a counter.
// stamp[item] == k + 2: the item is already on round k + 1's list.
//
// kW: entering cell c by a legal move costs b * (1 + pen[c]), b = 5 / 7, in
// place of b.
//   * only the cells this workgroup relaxes are ever entered, so the entering
//     costs are loaded for the tile's own 64 x 64 cells, not for the ring; they
//     are kept as the row's prefix sums s_P[row][k] = sum of 5 * (1 + pen) over
//     columns < k (at most 64 * 1280), built once per visit by a wave scan;
//     a cell's own orthogonal cost is s_P[k + 1] - s_P[k], its diagonal 7/5 of
//     it.  s_P has one row where kW is off;
//   * the row scan: within a run of traversable cells, moving right from x' to
//     x enters x' + 1 .. x, moving left from x' to x enters x .. x' - 1, so
//     best[x] = min over x' of best[x'] + |s_P[..x] - s_P[..x']| (5 |x - x'|
//     where kW is off); each Kogge-Stone step shuffles the prefix sum along
//     with best.  A candidate that ends <= max_cost is <= max_cost at every
//     step on the way (weights are positive), so the guard
//     delta <= max_cost - o drops nothing valid.
//
// kTeam: K single-source fields cost[field][H][W] relaxed in the same rounds
// (DESIGN.md §7.5).  Field k is the plain field from src[k] alone; the fields
// are independent, so a work item is one (field, tile), listed as
// field * NT + tile with stamps [K][NT], and one launch is one round of all
// of them; the no-atomics argument holds per field, one workgroup owning a
// (field, tile) in a round.  All fields read one copy of the traversable bit
// rows, without any source in it: a field's source cell is traversable in
// that field only, so its bit is ORed into the row words as they are loaded
// into LDS (the centre word or a ring word, wherever the source's row and
// tile column are among the 66 x 3 loaded), before the per-cell flags, the
// ring costs and the row scan's gaps are derived from them.  The bit rows in
// memory are never written.  Where kTeam is off, `cost` is the one field and
// travs holds its sources' bits already (k_plan_sources).
//
// pen is read where kW, src where kTeam; the other is nullptr.
template <bool kW, bool kTeam>
__global__ __launch_bounds__(kThreads) void k_plan_relax(uint32_t* __restrict__ cost_all,
                                                         const uint64_t* __restrict__ travs,
                                                         const uint8_t* __restrict__ pen,
                                                         const int64_t* __restrict__ src, int64_t W, int64_t H,
                                                         int64_t TX, int64_t TY, uint32_t max_cost,
                                                         const int32_t* __restrict__ list_in,
                                                         int32_t* __restrict__ list_out, unsigned int* len,
                                                         uint32_t* __restrict__ stamp, uint32_t round,
                                                         unsigned long long* __restrict__ stat,
                                                         volatile unsigned long long* hstat) {
  __shared__ uint32_t s_c[kRing][kRing];
  __shared__ uint32_t s_P[kW ? DM_TILE : 1][DM_TILE + 1];
  __shared__ unsigned long long s_tw[kRing][3];
  __shared__ uint8_t s_t[kRing][kRing + 2];
  __shared__ int s_flags;
  // The 16-row loop of a sweep, stated: the compiler unrolls it fully in the
  // unweighted kernels (192 row-scan shuffles in a row, their schedule) and
  // not at all in the weighted one, and left to its heuristic it changes its
  // mind with the shape of the surrounding code.
  constexpr int kRowUnroll = kW ? 1 : 16;
  const unsigned int n_in = len[round % 3u];
  unsigned int* const len_out = &len[(round + 1u) % 3u];
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    len[(round + 2u) % 3u] = 0u;
    hstat[HS_LEN] = n_in;
    if (n_in) {
      const unsigned long long relax = stat[ST_RELAX] + n_in;
      stat[ST_ROUNDS] = round + 1u;
      stat[ST_RELAX] = relax;
      hstat[HS_ROUNDS] = round + 1u;
      hstat[HS_RELAX] = relax;
      hstat[HS_TRAV] = stat[ST_TRAV];
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t NT = TX * TY;
  for (unsigned int item = blockIdx.x; item < n_in; item += gridDim.x) {
    const int64_t it = list_in[item], field = kTeam ? it / NT : 0, tile = kTeam ? it % NT : it;
    const int64_t tx = tile % TX, ty = tile / TX;
    const int64_t x0 = tx * DM_TILE, y0 = ty * DM_TILE;
    uint32_t* const cost = kTeam ? cost_all + field * (W * H) : cost_all;
    int64_t sy = 0, stx = 0;
    unsigned long long sbit = 0ull;
    if constexpr (kTeam) {
      const int64_t sc = src[field];
      sy = sc / W;
      stx = (sc % W) >> 6;
      sbit = 1ull << ((sc % W) & 63);
    }
    if (threadIdx.x == 0) s_flags = 0;
    // traversable words of the ring rows: left neighbour, tile, right neighbour
    // (kTeam: with this field's source bit where its row and tile column are loaded)
    for (int j = threadIdx.x; j < kRing * 3; j += kThreads) {
      const int row = j / 3, wc = j % 3;
      const int64_t gy = y0 - 1 + row, ntx = tx + wc - 1;
      unsigned long long w = 0ull;
      if (gy >= 0 && gy < H && ntx >= 0 && ntx < TX) w = travs[((gy >> 6) * TX + ntx) * DM_TILE + (gy & 63)];
      if constexpr (kTeam)
        if (gy == sy && ntx == stx) w |= sbit;  // the source is in the grid
      s_tw[row][wc] = w;
    }
    if constexpr (kW) {
      // prefix sums of the rows' orthogonal entering costs (cells outside the grid are never entered)
      for (int i = 0; i < 16; ++i) {
        const int row = wave * 16 + i;
        const int64_t gy = y0 + row, gx = x0 + lane;
        uint32_t p = gy < H && gx < W ? 5u * (1u + pen[gy * W + gx]) : 0u;
#pragma unroll
        for (int d = 1; d < DM_TILE; d <<= 1) {
          const uint32_t o = (uint32_t)__shfl_up((int)p, d);
          if (lane >= d) p += o;
        }
        s_P[row][lane + 1] = p;
        if (lane == 0) s_P[row][0] = 0u;
      }
    }
    __syncthreads();
    for (int j = threadIdx.x; j < kRing * kRing; j += kThreads) {
      const int row = j / kRing, col = j % kRing;
      const int wc = col == 0 ? 0 : (col == kRing - 1 ? 2 : 1);
      const int bit = col == 0 ? 63 : (col == kRing - 1 ? 0 : col - 1);
      const int t = (int)((s_tw[row][wc] >> bit) & 1ull);
      // traversable bits are set for in-grid cells only; the others hold no cost
      s_t[row][col] = (uint8_t)t;
      s_c[row][col] = t ? cost[(y0 - 1 + row) * W + (x0 - 1 + col)] : kUnreach;
    }
    __syncthreads();
    uint32_t init[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) init[i] = s_c[wave * 16 + i + 1][lane + 1];
    bool converged = false;
    for (int sweep = 0; sweep < kMaxSweeps; ++sweep) {
      int ch = 0;
#pragma unroll kRowUnroll
      for (int ii = 0; ii < 16; ++ii) {  // wave-uniform: the row scans below shuffle across all lanes
        const int i = (sweep & 1) ? 15 - ii : ii;
        const int rr = wave * 16 + i + 1, cc = lane + 1;
        const int t = s_t[rr][cc];
        const uint32_t cur = s_c[rr][cc];  // kUnreach > max_cost where the cell is not traversable
        uint32_t Pl = 0u, Pr = 0u;  // kW: the row's sums before / through this column
        if constexpr (kW) {
          Pl = s_P[rr - 1][lane];
          Pr = s_P[rr - 1][lane + 1];
        }
        uint32_t best = cur;
        if (t) {
          // entering this cell; weighted <= 1792 < kUnreach - max_cost
          const uint32_t e5 = kW ? Pr - Pl : 5u, e7 = kW ? e5 / 5u * 7u : 7u;
          const uint32_t cn = s_c[rr - 1][cc], cs = s_c[rr + 1][cc], cw = s_c[rr][cc - 1], ce = s_c[rr][cc + 1];
          if (cn <= max_cost) best = min(best, cn + e5);
          if (cs <= max_cost) best = min(best, cs + e5);
          if (cw <= max_cost) best = min(best, cw + e5);
          if (ce <= max_cost) best = min(best, ce + e5);
          const int tn = s_t[rr - 1][cc], ts = s_t[rr + 1][cc], tw = s_t[rr][cc - 1], te = s_t[rr][cc + 1];
          if (tn && tw) { const uint32_t v = s_c[rr - 1][cc - 1]; if (v <= max_cost) best = min(best, v + e7); }
          if (tn && te) { const uint32_t v = s_c[rr - 1][cc + 1]; if (v <= max_cost) best = min(best, v + e7); }
          if (ts && tw) { const uint32_t v = s_c[rr + 1][cc - 1]; if (v <= max_cost) best = min(best, v + e7); }
          if (ts && te) { const uint32_t v = s_c[rr + 1][cc + 1]; if (v <= max_cost) best = min(best, v + e7); }
          if (best > max_cost) best = cur;
        }
        // Along the row at once: orthogonal moves between adjacent traversable
        // cells are always legal, so within a run of traversable cells
        // best[x] = min over x' of best[x'] + the cost of walking from x' to x,
        // a prefix-min scan from either side in 6 shuffle steps each.  run_l /
        // run_r: the traversable cells in a row up to and from this one (0 if
        // it is not).
        const unsigned long long gaps = ~s_tw[rr][1];
        const unsigned long long gl = gaps & ((2ull << lane) - 1ull), gr = gaps >> lane;
        const int run_l = gl ? lane - (63 - __clzll((long long)gl)) : lane + 1;
        const int run_r = gr ? __ffsll((long long)gr) - 1 : 64 - lane;
#pragma unroll
        for (int d = 1; d < DM_TILE; d <<= 1) {  // from x - d: enters x - d + 1 .. x
          const uint32_t o = (uint32_t)__shfl_up((int)best, d);
          uint32_t delta = 5u * d;
          if constexpr (kW) delta = Pr - (uint32_t)__shfl_up((int)Pr, d);
          if (run_l > d && o <= max_cost && delta <= max_cost - o) best = min(best, o + delta);
        }
#pragma unroll
        for (int d = 1; d < DM_TILE; d <<= 1) {  // from x + d: enters x .. x + d - 1
          const uint32_t o = (uint32_t)__shfl_down((int)best, d);
          uint32_t delta = 5u * d;
          if constexpr (kW) delta = (uint32_t)__shfl_down((int)Pl, d) - Pl;
          if (run_r > d && o <= max_cost && delta <= max_cost - o) best = min(best, o + delta);
        }
        if (best < cur) {
          s_c[rr][cc] = best;
          ch = 1;
        }
      }
      // also the sweep's barrier: a sweep in which no thread stored anything
      // read settled values only, so the tile is at its fixpoint
      if (!__syncthreads_or(ch)) {
        converged = true;
        break;
      }
    }
    int flags = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int row = wave * 16 + i, col = lane;
      const uint32_t v = s_c[row + 1][col + 1];
      // v != init only where the cell is traversable, and those are in the grid
      if (v != init[i]) cost[(y0 + row) * W + (x0 + col)] = v;
      // round 0 publishes the sources themselves: nobody has seen their zeros
      if (v != (round == 0u ? kUnreach : init[i])) {
        const int n = row == 0, s = row == DM_TILE - 1, w = col == 0, e = col == DM_TILE - 1;
        // bit = (dy + 1) * 3 + (dx + 1) of the neighbour that sees the cell
        flags |= (n << 1) | (s << 7) | (w << 3) | (e << 5) | ((n & w) << 0) | ((n & e) << 2) | ((s & w) << 6) |
                 ((s & e) << 8);
      }
    }
    if (!converged) flags |= 1 << 4;  // stopped at the sweep bound: this item again
    if (flags) atomicOr(&s_flags, flags);
    __syncthreads();
    if (threadIdx.x < 9 && ((s_flags >> threadIdx.x) & 1)) {
      const int64_t ntx = tx + (int)(threadIdx.x % 3) - 1, nty = ty + (int)(threadIdx.x / 3) - 1;
      if (ntx >= 0 && ntx < TX && nty >= 0 && nty < TY) {
        const int64_t nt = field * NT + nty * TX + ntx;  // kTeam: < 2^31, dm_plan_team checks n_robots * NT
        if (atomicExch(&stamp[nt], round + 2u) != round + 2u) list_out[atomicAdd(len_out, 1u)] = (int32_t)nt;
      }
    }
    __syncthreads();  // s_flags / LDS reuse by the next item
  }
}

// Reached cells per field of cost[gridDim.y][ncell]: blockIdx.y = field, into
// reached[field].  The single field is one layer, into plan_stat + ST_REACHED.
__global__ __launch_bounds__(kThreads) void k_plan_team_count(const uint32_t* __restrict__ cost, int64_t ncell,
                                                              unsigned long long* __restrict__ reached) {
  __shared__ int s_n;
  if (threadIdx.x == 0) s_n = 0;
  __syncthreads();
  const uint32_t* const layer = cost + (int64_t)blockIdx.y * ncell;
  int c = 0;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < ncell; i += (int64_t)gridDim.x * kThreads)
    c += layer[i] != kUnreach;
  for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off);
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(&s_n, c);
  __syncthreads();
  if (threadIdx.x == 0 && s_n) atomicAdd(&reached[blockIdx.y], (unsigned long long)s_n);
}

// ---- 3. query, path -----------------------------------------------------------
// Thread = (robot, target), target at (xy[tg * stride], xy[tg * stride + 1])
// metres, under field `robot` of cost[n_robots][H][W] (the single field is
// one layer): the reached in-grid cell within Chebyshev distance s of the
// target's cell that minimises (dx^2 + dy^2, linear index), into
// out[robot * n + target]; (kUnreach, -1) if there is none or the target is
// out of grid.
__global__ void k_plan_team_query(const uint32_t* __restrict__ cost, int32_t n_robots, int64_t W, int64_t H,
                                  double ox, double oy, double res, const double* __restrict__ xy, int64_t stride,
                                  int64_t n, int32_t s, uint32_t* __restrict__ out_cost,
                                  int64_t* __restrict__ out_cell) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * n_robots) return;
  const int64_t r = i / n, tg = i % n;
  const uint32_t* const layer = cost + r * (W * H);
  const double fx = floor((xy[tg * stride] - ox) / res), fy = floor((xy[tg * stride + 1] - oy) / res);
  uint32_t bc = kUnreach;
  int64_t bcell = -1;
  if (fx >= 0.0 && fx < (double)W && fy >= 0.0 && fy < (double)H) {  // NaN: out of grid
    const int64_t cx = (int64_t)fx, cy = (int64_t)fy;
    int bd = 0x7FFFFFFF;
    for (int dy = -s; dy <= s; ++dy) {  // rows, then columns: ascending linear index
      const int64_t y = cy + dy;
      if (y < 0 || y >= H) continue;
      for (int dx = -s; dx <= s; ++dx) {
        const int64_t x = cx + dx;
        if (x < 0 || x >= W) continue;
        const int d = dx * dx + dy * dy;
        if (d >= bd) continue;
        const uint32_t c = layer[y * W + x];
        if (c == kUnreach) continue;
        bd = d;
        bc = c;
        bcell = y * W + x;
      }
    }
  }
  out_cost[i] = bc;
  out_cell[i] = bcell;
}

// One wave walks back from *start: lanes 0..7 test the 8 neighbours in the
// order (dy, dx) = (-1,-1), (-1,0), (-1,1), (0,-1), (0,1), (1,-1), (1,0),
// (1,1); the first that is reached, moves legally and has
// cost + w == the cell's cost is the predecessor.  out[] takes the cells
// target-first up to cap; n_out[0] the full length, n_out[1] != 0 if the walk
// found no predecessor (a field that is no fixpoint: never for a complete one).
// kWeighted: the field is the weighted k_plan_relax's, a move into the cell costs
// 5 / 7 times 1 + pen[cell]; false is the unweighted kernel, pen unused.
template <bool kWeighted>
__global__ __launch_bounds__(64) void k_plan_path(const uint32_t* __restrict__ cost,
                                                  const uint64_t* __restrict__ travs,
                                                  const uint8_t* __restrict__ pen, int64_t W, int64_t H,
                                                  int64_t TX, const int64_t* __restrict__ start,
                                                  int64_t* __restrict__ out, int64_t cap,
                                                  unsigned long long* __restrict__ n_out) {
  const int lane = threadIdx.x;
  const int k = lane < 4 ? lane : lane + 1;  // skip the centre of the 3x3
  const int dy = lane < 8 ? k / 3 - 1 : 0, dx = lane < 8 ? k % 3 - 1 : 0;
  int64_t cur = *start;
  unsigned long long n = 0, err = 0;
  if (cur >= 0) {
    uint32_t c = cost[cur];
    const unsigned long long bound = (unsigned long long)(c / 5u) + 1ull;
    for (;;) {
      if (lane == 0 && (int64_t)n < cap) out[n] = cur;
      ++n;
      if (c == 0u) break;
      if (n > bound) { err = 1; break; }
      const int64_t x = cur % W, y = cur / W, nx = x + dx, ny = y + dy;
      bool ok = false;
      uint32_t nc = kUnreach;
      if (lane < 8 && nx >= 0 && nx < W && ny >= 0 && ny < H) {
        nc = cost[ny * W + nx];
        uint32_t w = (dx != 0 && dy != 0) ? 7u : 5u;
        if (kWeighted) w *= 1u + pen[cur];
        ok = nc != kUnreach && (unsigned long long)nc + w == (unsigned long long)c;
        if (ok && dx != 0 && dy != 0) ok = trav_bit(travs, TX, x, ny) && trav_bit(travs, TX, nx, y);
      }
      const unsigned long long m = __ballot(ok);
      if (!m) { err = 1; break; }
      const int j = __ffsll((long long)m) - 1;
      const int jk = j < 4 ? j : j + 1;
      cur = (y + jk / 3 - 1) * W + (x + jk % 3 - 1);
      c = (uint32_t)__shfl((int)nc, j);
    }
  }
  if (lane == 0) {
    n_out[0] = n;
    n_out[1] = err;
  }
}

// ---- 4. team fields (dm_plan_team) -----------------------------
// The rounds are k_plan_relax<false, true>'s, the reached counts and the
// snapped queries the layered kernels' above; what the team adds is its seed.

// Thread = field: cost 0 at its source, and (field, source tile) on round 0's list.
__global__ void k_plan_team_seed(const int64_t* __restrict__ src, int32_t n, int64_t W, int64_t TX, int64_t NT,
                                 int64_t ncell, uint32_t* __restrict__ cost, int32_t* __restrict__ list) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const int64_t c = src[k], x = c % W, y = c / W;
  cost[(int64_t)k * ncell + c] = 0u;
  list[k] = (int32_t)((int64_t)k * NT + (y >> 6) * TX + (x >> 6));
}

}  // namespace dm_plan
