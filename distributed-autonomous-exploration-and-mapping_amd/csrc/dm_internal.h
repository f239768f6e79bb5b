// dm_internal.h — internal types of libdm (not part of the C-ABI).
//
// Device data layout in HBM (one handle = one row band of the map):
//   L      float [R][W]  log-odds, row-major (band-local row = gy - row0)
//   state  int8  [R][W]  OccupancyGrid.data encoding (-1/0/100)
//   tile_* int32 [TY][TX] per 64x64 tile summaries (TX = ceil(W/64),
//          TY = ceil(R/64)): per-call segment counts, active slots, and the
//          number of free cells (drives which tiles the frontier pass visits)
// Per-call workspace (grown on demand, reused across calls):
//   beams  Beam[S*N]     endpoint cells + Bresenham parameters per beam
//   pieces PackedPiece[] ray pieces binned by tile, tile-local addresses
//   active tile lists, frontier slots (one per tile-local component), borders.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>
#include <chrono>
#include <string>
#include <vector>

#include "../../include/dm.h"

#include "dm_buf.h"
#include "dm_ray.h"


// device counters (uint64 each)
enum {
  CNT_ACTIVE = 0,   // active tiles this integrate call
  CNT_U = 1,        // beam-cell updates
  CNT_T = 2,        // touched cells
  CNT_SEGS = 3,     // segments emitted
  CNT_FTILES = 4,   // tiles visited by the frontier pass (tile_free > 0)
  CNT_SLOTS = 5,    // tile-local frontier components
  CNT_CLUSTERS = 6, // output clusters
  CNT_OVERFLOW = 7, // frontier flags: kOvSlots (slot arrays full), kOvUnionFind (bound hit)
  CNT_ITEMS = 8,    // heavy work items (<= 256 pieces of a heavy tile each)
  CNT_HEAVY = 9,    // heavy tiles (> 256 pieces)
  CNT_TH = 10,      // touched cells of heavy tiles
  CNT_SORTED = 11,  // 1: out_clu holds the clusters sorted by label
  CNT_FL0 = 12,     // frontier tile-list length of the pass (copied by k_frontier_bits)
  CNT_STAMP = 13,   // the pass's stamp (k_frontier_bits: ++ the handle's stamp word), tile-edge hand-offs
  CNT_LITEMS = 14,  // light work items (= light tiles)
  CNT_IOVERFLOW = 15,  // integrate capacity overflow flags (1 first-touch list, 2 pieces, 4 work lists)
  CNT_BIG = 16,     // frontier tiles with more runs than a tile-wave holds (big-tile list length)
  CNT_SITEMS = 17,  // sparse light work items (<= sparse_pieces pieces; stored from the top of litems)
  CNT_N = 18
};
// CNT_OVERFLOW bits of a frontier pass
constexpr unsigned long long kOvSlots = 4ull;      // a slot shard region overflowed
constexpr unsigned long long kOvUnionFind = 8ull;  // a union-find loop hit its bound (dm_uf.h)
constexpr unsigned long long kOvPipeline = 32ull;  // the handle's sticky hand-off error was set (kHaltWord)
// fe_flag[kHaltWord]: sticky error word of the overlapped pipeline.  The
// integrate front-end -> map update gate sets bit 1 when it times out; from
// then on k_tile_accum and k_fmask_items return at once (the workspace they
// would read was not written), k_frontier_bits flags every pass kOvPipeline,
// and the host reports DM_ERR_PIPELINE until dm_reset clears it.
constexpr int kHaltWord = 8;
// Hand-off words (fe_flag, bits_flag): k_seq_signal increments [kSigWord],
// k_seq_gate increments [kGateWord] and waits until [kSigWord] reaches it:
// the n-th gate waits for the n-th signal, with no host-side sequence number
// in the kernel arguments.
constexpr int kSigWord = 0;
constexpr int kGateWord = 4;
constexpr int kStampWord = 8;  // bits_flag: the last frontier pass's stamp (k_frontier_bits)
// Integrate counters, zeroed by each integrate call; the others belong to the
// frontier pass, which may still be running when the next call's front-end
// starts (dm_set_overlap), so the integrate reset never touches them.
constexpr int kIntegrateCounters[] = {CNT_ACTIVE, CNT_U, CNT_T, CNT_SEGS, CNT_ITEMS,
                                      CNT_HEAVY, CNT_TH, CNT_LITEMS, CNT_IOVERFLOW, CNT_SITEMS};

// k_plan's work-item classes (dm_integrate.hip): tiles with more pieces than
// kIntegrateChunk are split into items of kIntegrateChunk pieces, tiles with
// more than kIntegrateMedium are heavy (merged in a slab)
constexpr int kIntegrateChunk = 256;
constexpr int kIntegrateMedium = 1024;


// Sharded counters: same-address device atomics serialise at the memory side
// (~12 ns each, MI355X_MICROARCH.md price list "fanin"), so per-workgroup
// totals go to one of kShards counters, each on its own 128-B line
// (shard = blockIdx.x % kShards); readers sum the shards.
constexpr int kShards = 32;
constexpr int kShardWords = 16;  // 128 B per shard
static_assert(kShards * kShardWords == 512, "k_integrate_reset covers 512 shard words");
// integrate shard fields
enum { SH_U = 0, SH_T = 1, SH_TH = 2, SH_ACT = 3 };
// frontier shard fields: slots allocated, runs and tiles with frontier
// cells (the next pass picks its tile kernel from their ratio)
// and tiles too run-rich for a tile-wave (the next pass sizes the big kernel's grid);
// tiles the workgroup kernel labelled from the label cache / in full
enum { SH_SLOT = 0, SH_RUNS = 1, SH_FTF = 2, SH_BIG = 3, SH_CHIT = 4, SH_CMISS = 5 };
// 64-bit words of one tile's label-cache entry (dm_frontier.hip): 1.25 KB
constexpr int kFcWords = 160;

// dm_last_stats entries (include/dm.h)
constexpr int kNStats = 11;
constexpr bool dm_stat_is_frontier(int i) { return i >= 7 && i <= 9; }  // the others: integrate

// Readback header in front of the sorted cluster records (device out_clu and
// pinned h_out both point kRbRecords records into their allocation): the
// frontier counters [CNT_N] and the fullest slot shard [CNT_N], written by
// k_rank_sort into the mapped host buffer together with the first records.
// header words: [0, CNT_N) counters, [CNT_N] fullest slot shard, [CNT_N + 1]
// runs, [CNT_N + 2] tiles with frontier cells, [CNT_N + 3] run-rich tiles,
// [CNT_N + 4] label-cache hits, [CNT_N + 5] misses (shard sums)
constexpr int kRbRecords = 6;  // 6 * 48 B = 288 B >= (CNT_N + 6) * 8 B
static_assert(kRbRecords * sizeof(dm_cluster) >= (CNT_N + 6) * sizeof(unsigned long long), "readback header");
// The mapped host readback carries 32-byte records (label, size, sum_x,
// sum_y): the host computes the centroids with the SPEC's double formula
// (one division, then add; no FMA), bit-identical to the device's, so a third
// fewer bytes cross PCIe than whole dm_cluster records.
struct dm_raw_record {
  long long label, size, sum_x, sum_y;
};
constexpr int kRbHostRecords = 6;  // 6 * 32 B = 192 B of header in front of the host records
static_assert(kRbHostRecords * sizeof(dm_raw_record) >= (CNT_N + 6) * sizeof(unsigned long long),
              "readback header");
__host__ __device__ inline unsigned long long* dm_rb_header(dm_raw_record* records) {
  return reinterpret_cast<unsigned long long*>(records - kRbHostRecords);
}
__host__ __device__ inline const unsigned long long* dm_rb_header(const dm_raw_record* records) {
  return reinterpret_cast<const unsigned long long*>(records - kRbHostRecords);
}
// SPEC a10 centroid: origin + (sum / size + 0.5) * res,
// one IEEE division, then add (compiled with -ffp-contract=off, host and device)
__host__ __device__ inline double dm_centroid(double origin, long long sum, long long size, double res) {
  const double m = (double)sum / (double)size;
  return origin + (m + 0.5) * res;
}

// SPEC a7: L == 0 -> -1, else L >= occ_t -> 100, else L <= free_t -> 0, else
// -1, as selects, lowest priority first (thresholds without signed zeros).
// The one statement of a7 on the device: the map update's state_of
// (dm_integrate.hip) and the fusion (dm_fuse.hip) both call it.
__host__ __device__ inline int8_t dm_state_a7(float L, float occ_t, float free_t) {
  int32_t r = -1;
  r = L <= free_t ? 0 : r;
  r = L >= occ_t ? 100 : r;
  r = L == 0.0f ? -1 : r;
  return (int8_t)r;
}
// SPEC a6's clamp as the SPEC writes it (bounds without signed zeros): what
// the map update's v_med3 form (apply_one, dm_integrate.hip) computes for
// finite L and l_min <= l_max, spelled out for callers outside that loop.
__host__ __device__ inline float dm_clamp_a6(float L, float l_min, float l_max) {
  if (L < l_min) L = l_min;
  if (L > l_max) L = l_max;
  return L;
}

struct dm_grid;
// async D2H of both shard-counter blocks into g->h_sh (pinned)
hipError_t dm_copy_shards(dm_grid* g);
inline unsigned long long dm_shard_sum(const unsigned long long* sh, int field) {
  unsigned long long s = 0;
  for (int i = 0; i < kShards; ++i) s += sh[i * kShardWords + field];
  return s;
}

struct dm_shard_set;  // dm_sharded.cpp

// Every allocation, event, stream and pending timer of a handle is a member
// that owns it (dm_buf.h) and goes with the handle: dm_destroy has no list of them.  The
// only raw handles left in it are hipEvent_t's that name an event one of those
// owners holds (PassEnd::ev, IntWs::free_wait), each said so where it is
// declared.  Nothing in it means "the slot / workspace set / tile list in
// use": a pass's readback slot is an argument of the functions that write or
// read it, its workspace set is fw[fparity], the tile list flist[flist_cur].
struct dm_grid {
  dm_params p;
  // non-null: a sharded parent (dm_create_sharded); every call runs on its
  // band handles (dm_sharded.cpp) and none of the fields below is allocated
  dm_shard_set* sh = nullptr;
  int device = 0;
  int n_cu = 256;  // compute units of the device: sizes the resident (one-pass) grids
  // what every launch uses: owned_stream, or the caller's (dm_set_stream) while owned_stream is null
  hipStream_t stream = nullptr;
  DevStream owned_stream;
  // dm_set_overlap: the integrate front-end (reset, beam_prep, plan, scatter)
  // runs on fe_stream, so it overlaps a frontier pass still running on
  // `stream`; the accumulation waits for it (ev_fe).  The workspace the
  // front-end hands to the accumulation is double-buffered (iw[2], calls
  // alternate): call k+1's front-end only waits for call k-1's accumulation
  // (iw[p].ev_free), which is long done when the steps are pipelined, so no
  // marker sits behind the accumulation of call k.
  bool overlap = false;
  // One front-end stream: consecutive calls' front-ends queue behind each
  // other.  Two alternating streams (so call k+1's front-end could start
  // before call k's finished) left the full step where it was and slowed
  // C1 / C5: DESIGN.md §3.3.3, §5.7.
  DevStream fe_stream;
  DevEvent ev_fe;
  // front-end completion word (k_fe_signal / k_fe_gate, dm_integrate.hip):
  // the sequence number of the last call whose front-end finished
  DevBuf<unsigned long long> fe_flag;  // [kSigWord] / [kGateWord] hand-off counts, [kHaltWord] sticky error
  // DM_FAULT_GATE=1 (read at dm_create; fault-injection tests only): the
  // front-end gate waits for a sequence number that never comes, ~10 us
  bool fault_gate = false;
  // ev_bits[parity]: the end of a split pass's bit rows on `stream` (the pass
  // stream waits for it); it also frees the integrate workspaces whose
  // accumulations are ahead of it (dm_mark_ws_free), so the next front-end
  // using them can start right away instead of after the whole pass
  DevEvent ev_bits[2];
  uint64_t integrate_seq = 0;  // map changes so far
  // Asynchronous passes (dm_frontiers_begin / dm_merge_bands_begin) use a
  // ring of kRbSlots readback slots, so a pass can be started before the
  // previous one was collected.  Each slot owns what its _end reads: the
  // mapped readback buffer (header + first records), the device sorted
  // records, the event marking the pass's end.  The entry point that starts or
  // collects a pass picks the slot and hands it to everything that writes or
  // reads it (dm_enqueue_frontiers, dm_launch_merge, dm_launch_export,
  // dm_frontiers_readback).
  struct RbSlot {
    Headed<DevBuf<dm_cluster>, kRbRecords> out_clu;         // device sorted band records behind the header
    Headed<HostBuf<dm_raw_record>, kRbHostRecords> h_out;   // mapped host readback behind the header, 32-byte records
    DevBuf<dm_cluster> m_out;      // device sorted merged records
    DevEvent ev;
    int kind = 0;                     // pending pass: 0 none, 1 band frontiers, 2 band merge
    uint64_t seq = 0;                 // integrate_seq at the pass's start
    uint64_t gen = 0;                 // rb_gen at the pass's start
    uint64_t pass = 0;                // fr_pass / m_pass of the pass
    int64_t merge_n = 0;              // nranks * rec_cap of a merge
    uint64_t wepoch = 0, mepoch = 0;  // passes / merges that wrote out_clu / m_out so far
  };
#ifndef DM_RB_SLOTS
#define DM_RB_SLOTS 2
#endif
  static constexpr int kRbSlots = DM_RB_SLOTS;  // ring slots of asynchronous passes
  static constexpr int kRbSync = kRbSlots;      // the slot of synchronous calls (dm_frontiers, dm_merge_bands)
  RbSlot rb[kRbSlots + 1];
  int rb_head = 0, rb_count = 0;      // oldest pending slot, pending passes
  uint64_t rb_gen = 0;                // bumped when device record buffers are reallocated
  // frontier / merge passes enqueued so far: an unsorted result (more
  // clusters than the sort kernel takes) lives in the shared raw arrays
  // (clusters / m_clu), valid only while no later pass of its kind ran
  uint64_t fr_pass = 0, m_pass = 0;
  int64_t W = 0, H = 0, R = 0, row0 = 0;
  int64_t TX = 0, TY = 0, NT = 0;
  int32_t nmax = 0;  // max ray length (cells) bound

  DevBuf<float> L;
  DevBuf<int8_t> state;
  // free cells per tile (bits 0..29) | kTileListed: the tile is on the
  // persistent frontier tile list (flist[flist_cur] below)
  DevBuf<int32_t> tile_free;
  // [NT][64 rows][16] per tile: byte j of row y holds the free bits of cells
  // 4j..4j+3 (low nibble) and their unknown bits (high nibble); out-of-grid
  // cells are neither.  Kept in step with `state` by every kernel that writes
  // it (k_tile_accum's apply: each thread stores its 4 cells' byte;
  // k_recount after bulk writes); the frontier pass reads these 1 KB per tile
  // instead of the state bytes.  Maintained only while passes list many tiles
  // (fmask_on: a pass listing >= kFmaskOnTiles switches it on, one listing
  // fewer than kFmaskOnTiles / 4 off): a few thousand listed tiles (C3) are
  // latency-bound either way and the per-call update would only add a
  // kernel.  fmask_valid: the records match the state (a full rebuild,
  // k_recount, precedes switching on otherwise).
  DevBuf<uint8_t> fmask;
  // fedge: per tile 4 words, the unknown bits of its column 0, column 63
  // (bit = row), row 0 and row 63 (bit = column), written with fmask by the
  // same kernels: a pass reads its neighbours' edges from these 32 B instead
  // of from their 1 KB records (one byte of every 16 B row: all 8 lines)
  DevBuf<uint64_t> fedge;
  // tile_seen: 0 while every cell of the tile is still unknown (since the
  // last bulk write: k_recount sets it from the state), 1 once an
  // integrate item applied the tile (k_tile_accum).  The frontier bit rows
  // take an unseen neighbour's facing cells as unknown without reading them:
  // the explored region's borders face unseen tiles, whose halo column would
  // otherwise cost a 128-byte line per row.
  // INVARIANT (the frontier pass is wrong without it): every kernel that
  // writes `state` either sets tile_seen[tile] = 1 for the tiles it wrote
  // (k_tile_accum: light / medium items, the heavy finisher, sparse items)
  // or is followed by k_recount over the map (dm_launch_recount: dm_reset,
  // dm_set_state, dm_set_logodds, dm_load, the dm_fuse_* calls).  A new state writer must do one
  // of the two; tests/test_gpu_tile_seen.py fails against a library whose
  // bit rows trust a stale flag (mutation-checked in round 5).
  // INVARIANT 2 (k_fuse, dm_fuse.hip, is wrong without it): in every cell
  // state == dm_state_a7(L) with the handle's thresholds.  Every state writer
  // derives the byte from the L it stores (k_tile_accum's apply,
  // k_state_from_l, k_set_state, dm_reset's L = 0 / state = -1).  The fusion
  // does not read the old state byte: it recomputes it from the old L, for
  // its "state changed" count and to store the byte only where it differs.  A
  // writer that stores a state not derived from L would break both.
  DevBuf<uint8_t> tile_seen;
  bool fmask_on = false, fmask_valid = false;
  int fmask_mode = 0;  // DM_FMASK=auto|on|off (read at dm_create; tests / A/B): 0 auto, 1 on, 2 off
  // Label cache of the workgroup tile kernel: [NT][kFcWords], one entry per
  // tile, valid exactly when its stored bit rows equal the pass's (nothing
  // else ever has to touch it: dm_reset, dm_set_state, dm_load and relists
  // leave it alone).  Allocated zero-filled with the first frontier pass;
  // fcache_mode: DM_FRONTIER_CACHE=on|off (read at dm_create; tests / A/B),
  // 1 on, 0 off -- also after a failed allocation, which is no error.
  DevBuf<uint64_t> fcache;
  int fcache_mode = 1;
  // hits and misses of the last collected pass (readback header), or of the
  // last export pass (fc_collected false: read from its shards on demand)
  unsigned long long fc_hits = 0, fc_misses = 0;
  bool fc_collected = true;
  HostBuf<unsigned long long> h_cnt;  // pinned mirror: [CNT_N] frontier counters, [CNT_N] integrate counters
  HostBuf<unsigned long long> h_sh;   // pinned mirror of the last call's integrate shards, then the last pass's fsh

  // The capacities kept beside the buffers (these, slot_cap, bs_cap, rs_rows,
  // m_cap, plan_qcap, gain_cap) are not one buffer's size, which the buffer
  // knows (size()): each is a bound the kernels are told, or covers a group of
  // arrays that grow together.  Only GroupCap::grow sets one: it is 0 until
  // every array of its group is allocated and after a failed growth.
  // integrate workspace capacities (the arrays are per set, IntWs)
  GroupCap beams_cap;
  GroupCap blk_cap;            // workgroups blk_hist / blk_n hold
  GroupCap segs_cap;           // pieces per workspace
  GroupCap act_cap;
  GroupCap hitem_cap;
  GroupCap heavy_cap;
  // what the front-end hands to the accumulation, one set per call parity
  struct IntWs {
    // the front-end's own scratch (k_beam_prep -> k_plan / k_scatter): per
    // set, like everything it hands over: call k+1's front-end overlaps call
    // k's accumulation
    DevBuf<Beam> beams;          // [beams_cap]
    DevBuf<int2> blk_hist;       // [beam blocks][1024] k_beam_prep's (tile, pieces | hash slot << 16) histogram
    DevBuf<int32_t> blk_n;       // [beam blocks] its entries
    DevBuf<int32_t> act_raw;     // [kShards][act_cap] first-touch lists per shard
    DevBuf<PackedPiece> pieces;    // [segs_cap] ray pieces binned by tile
    DevBuf<int4> hitems;           // heavy work items {tile, first piece, pieces, heavy ordinal}
    DevBuf<int4> litems;           // light work items {tile, first piece, pieces, -1} [act_cap]
    DevBuf<int32_t> heavy_list;    // heavy ordinal -> tile
    DevBuf<uint32_t> slabs;        // [heavy][2][64*64] merged hit / miss counts
    DevBuf<int32_t> heavy_done;    // [heavy] items finished this call (the last one applies the slab)
    DevBuf<int32_t> tile_count;    // [NT] pieces per tile (zeroed again by the accumulation)
    DevBuf<int32_t> tile_cur;      // [NT] k_scatter's bin cursor per active tile (k_plan)
    DevBuf<unsigned long long> cnt;  // [CNT_N] the integrate counters (kIntegrateCounters)
    DevBuf<unsigned long long> sh;   // [kShards][kShardWords] integrate shards
    // device copy of the host ranges (dm_integrate / _async) of the calls
    // using this set, reused only when the set is (free_wait)
    DevBuf<float> ranges;
    // the next front-end using this set waits for free_wait: an event on
    // `stream` after the set's last accumulation, recorded lazily (at the next
    // frontier pass or integrate call) -- ev_free, or the readback-slot event
    // of an asynchronous frontier pass enqueued after that accumulation
    // (dm_frontiers_begin records one anyway: no extra marker)
    DevEvent ev_free;
    hipEvent_t free_wait = nullptr;  // a view: ev_free or a readback slot's ev
    bool free_owed = false;
  };
  // calls alternate between the two sets
  static constexpr int kIntSets = 2;
  IntWs iw[kIntSets];
  int iw_cur = 0;                // set of the last integrate call
  DevBuf<double> trig; int32_t trig_n = -1; float trig_amin = 0, trig_inc = 0;
  // pinned, mapped (x, y, cos, sin) staging of host poses: a ring of two, each
  // reusable once the front-end that read it (k_beam_prep, through the device
  // address) is done (ev_pose), so a host-input call never waits for the
  // previous call (dm_integrate_async)
  static constexpr int kPoseRing = 2;
  HostBuf<double> h_pose4[kPoseRing];
  DevEvent ev_pose[kPoseRing];
  int pose_head = 0;
  int32_t last_S = 0, last_N = 0;

  // frontier workspace
  // Where a pass ended (dm_note_pass_end); pending until the host has seen it
  // end or `stream` was ordered after it.
  struct PassEnd {
    hipEvent_t ev = nullptr;  // names a readback slot's ev or a set's ev_split
    bool pending = false;
    uint64_t pass = 0;        // fr_pass of the pass; UINT64_MAX: a merge, which no band pass's end implies
    // the host saw pass `done` end: passes end in order, so every earlier one has
    void seen(uint64_t done) { if (pass <= done) pending = false; }
  };
  // What a pass's bit-row kernel writes on `stream` while the previous
  // pass's labelling may still run on pass_stream is double-buffered by pass
  // parity (fparity): counters, shards, list, frontier bit rows, edge slots,
  // slot parents.  The last pass's set is dm_last_fw(g).  A set is reused two
  // passes later; its previous pass must be done by then (busy: waited on by
  // `stream` unless the host already saw it complete).
  struct FrWs {
    DevBuf<unsigned long long> cnt;  // [CNT_N] device counters (frontier fields)
    DevBuf<unsigned long long> fsh;  // [kShards][kShardWords] frontier shards
    DevBuf<int32_t> big_tiles;       // [NT] per list position: 1 = too many runs for a tile-wave (k_frontier_bits)
    DevBuf<uint64_t> fbits;          // [NT][64] frontier bit rows of the listed tiles (k_frontier_bits)
    DevBuf<int32_t> edge_slot;       // [2][W] slots of the band's first / last row
    DevBuf<int32_t> slot_parent;     // [slot_cap]
    PassEnd busy;                       // the set's last pass
    DevEvent ev_split;                  // end of a split export pass on the pass stream
  };
  FrWs fw[2];
  // the pass's list lengths (snapshots of the tile list's length taken by k_frontier_bits),
  // a ring of three on separate lines: pass n uses fl_n[16 * (n % 3)]
  DevBuf<unsigned long long> fl_n;
  // pass_stream (dm_set_overlap + dm_frontiers_begin): the labelling half of
  // a pass (tile kernels, resolve, sort) runs there, after the bit-row
  // kernel on `stream` (which alone reads the map), so the next
  // batch's map update overlaps it.  bits_flag / bits_seq: the bit rows'
  // hand-off (k_seq_signal on `stream`, k_seq_gate on pass_stream).
  DevStream pass_stream;
  // big_stream: k_frontier_tile_big over the tiles k_frontier_bits listed as
  // too run-rich for a tile-wave, beside the wave kernel on the pass stream
  // (forked after the bit rows, joined before the resolve)
  DevStream big_stream;
  DevEvent ev_bigfork, ev_big;
  DevBuf<unsigned long long> bits_flag;  // [kSigWord] / [kGateWord] counts, [kStampWord] pass stamp
  PassEnd p_tail;  // the last pass_stream pass or merge; pending: `stream` has not been ordered after it
  // The persistent frontier tile list: every tile that has held a free cell
  // since the last bulk state write, in the order its first free cell
  // appeared (only free cells can be frontier cells).  Appended by the
  // integrate apply (the item that raises a tile's free count above 0 while
  // kTileListed is clear sets it and takes a list position), rebuilt after
  // bulk writes (dm_launch_recount: k_list_tiles).  Append-only between
  // rebuilds, so a pass reads the first flist_n[flist_cur][0] entries (its
  // snapshot, taken on the map stream after its batch) while later batches
  // append behind them.
  // Two lists: the periodic rebuild in tile order (dm_launch_relist) writes
  // the other one and switches, so passes still labelling go on reading the
  // old one (nothing appends to it after the switch) and the map stream never
  // waits for them; flist_ev[i]: the pass stream's position when list i was
  // left, which a rebuild into list i waits for (long done 16 passes later)
  DevBuf<int32_t> flist[2];               // [NT]
  DevBuf<unsigned long long> flist_n[2];  // [16]: [0] the list's length
  DevEvent flist_ev[2];
  bool flist_ev_set[2] = {false, false};
  int flist_cur = 0;      // the current list
  int relist_age = 0;     // passes since the list was last put in tile order
  int relist_period = 1;  // passes between those rebuilds: 1, 2, 4, ... up to kRelistPasses
                          // (a fresh map's list grows fastest in its first passes)
  DevBuf<int32_t> border;   // [tile][4][64] slot ids of a tile's edges (published sides only)
  // tile-edge hand-off words of k_frontier_tile, [4][NT]: horizontal (t, t+1),
  // vertical (t, t+TX), diagonal (t, t+TX+1), anti-diagonal (t, t+TX-1) pairs,
  // each (pass stamp << 2 | arrived sides); never reset (stamped)
  DevBuf<unsigned long long> rel;
  int32_t fparity = 0;         // workspace set (fw) of the last frontier pass
  // 0 after a failed growth, which the next pass repeats at the create-time size (dm_enqueue_frontiers)
  GroupCap slot_cap;
  DevBuf<long long> slot_label;
  DevBuf<int32_t> slot_root;
  DevBuf<long long> slot_own;  // [slot][3] size, sum_x, sum_y
  DevBuf<long long> slot_acc;  // [slot][3]
  DevBuf<long long> clusters;  // [cap][4] label,size,sum_x,sum_y (unsorted)
  DevBuf<int32_t> slot_k;      // [slot_cap] root slot -> compact cluster index
  DevBuf<int32_t> rank_of;     // [slot_cap] compact cluster index -> sorted position
  DevBuf<int32_t> cell_slot;   // dense [R][W] (only when labels requested)
  DevBuf<long long> edge_label;// [2][W]
  DevBuf<uint8_t> mask;        // dense [R][W] (only when mask requested)
  DevBuf<long long> labels;    // dense [R][W] int64 (only when requested)
  DevBuf<int8_t> halo;         // [2][W]: row before band, row after band
  int has_halo[2] = {0, 0};
  bool frontier_valid = false;

  // large-K cluster sort (row buckets, dm_frontier.hip k_rs_*): used when
  // the last collected pass of its kind had more than sort_min clusters
  DevBuf<unsigned long long> bs_key;   // [bs_cap] sort keys (label - base), two buffers
  DevBuf<unsigned long long> bs_key2;
  DevBuf<int32_t> bs_idx;      // [bs_cap] their record indices, two buffers
  DevBuf<int32_t> bs_idx2;
  GroupCap bs_cap;
  // per-row counters (zero between sorts) and offsets
  DevBuf<int32_t> rs_cnt;      // [rs_rows]
  DevBuf<int32_t> rs_off;      // [rs_rows + 1]
  DevBuf<unsigned long long> rs_status;  // [rs_rows / 8192 + 2] k_rs_scan's workgroup totals + failure word
  GroupCap rs_rows;
  int64_t sort_hint = 0, msort_hint = 0;  // clusters of the last band / merge readback
  int64_t ftile_hint = 0;                 // listed tiles of the last collected frontier pass
  int64_t runs_hint = 0, ftf_hint = 0;    // its runs and tiles with frontier cells
  int64_t big_hint = 0;                   // its tiles left to k_frontier_tile_big by k_frontier_tile
  // the cluster count above which the row sort replaces the rank sort
  // (DM_SORT_MIN, read at dm_create: tests run small maps through both)
  int64_t sort_min = 4096;
  // tile kernel choice: 0 from those statistics, 1 always the wave-per-tile
  // kernel, 2 always the 256-thread kernel (DM_FRONTIER_KERNEL=auto|wave|wg,
  // read at dm_create, for A/B measurements; all three are exact)
  int frontier_kernel = 0;
  // k_tile_accum's largest grid (the kernel grid-strides)
  static constexpr int kAccumGrid = 16384;
  // beams are split into k-ranges below this many threads per CU
  // (dm_integrate_chunks)
  static constexpr int kChunkThreadsPerCu = 512;
  // light tiles with at most this many pieces are sparse work items: walked
  // first, then only their touched cells are loaded (DM_SPARSE_PIECES, read
  // at dm_create: 0 sends every light tile through the dense path, tests)
  int sparse_pieces = 15;

  // cross-band merge workspace (dm_merge.hip), sized nranks * rec_cap
  GroupCap m_cap;
  DevBuf<int32_t> m_parent;
  DevBuf<long long> m_label;
  DevBuf<long long> m_acc;     // [m_cap][3] size, sum_x, sum_y
  DevBuf<long long> m_clu;     // [m_cap][4] merged records (unsorted)
  DevBuf<unsigned long long> m_cnt;    // [4] device: K, flags, sorted, max band K
  HostBuf<unsigned long long> h_mcnt;   // pinned mirror
  // [0] workgroups the last accumulation needed (dense items + sparse items
  // / 4), [1] its work items: written by k_tile_accum's workgroup 0 into
  // mapped host memory, read without a wait when the next call is enqueued
  // (a finished earlier call's value; 0 until one finished) to size the
  // accumulation and fmask grids to the work instead of to the capacity
  HostBuf<unsigned long long> h_hint;

  // goal selection (dm_goals.hip): the last collected sorted result on the
  // device (a readback slot's out_clu / m_out while that slot's epoch is
  // unchanged), top-T workspaces, robot / index / centroid staging
  struct GoalSource {
    const RbSlot* slot = nullptr;  // nullptr: none, or not sorted on the device
    int kind = 0;                  // 1: band frontiers (out_clu), 2: merge (m_out)
    uint64_t epoch = 0, gen = 0;   // the slot's wepoch / mepoch and rb_gen when it was collected
    int64_t n = 0;
  };
  GoalSource goal;
  DevBuf<unsigned long long> goal_k[2];
  DevBuf<uint32_t> goal_i[2];
  DevBuf<double> goal_io;          // [4 * 256] robots xy, then centroids xy
  DevBuf<int64_t> goal_idx;        // [256]

  // path planning (dm_plan.h; dm_plan_* and dm_assign_goals_path), allocated
  // on first use (ensure_plan).  The field is valid for the map version it was
  // computed on: integrate_seq + reset_seq, which every state writer bumps
  // (the integrate calls, dm_set_state, dm_set_logodds and through it dm_load:
  // integrate_seq; dm_reset: reset_seq).
  DevBuf<uint32_t> plan_cost;      // [H][W] row-major field
  DevBuf<uint64_t> plan_trav;      // [NT][64] traversable bit rows of the last inflation
  DevBuf<uint64_t> plan_travs;     // [NT][64] the same with the field's source cells set
  DevBuf<int32_t> plan_list[2];  // [NT] active tiles of even / odd rounds
  DevBuf<uint32_t> plan_stamp;     // [NT] round + 2 of the list the tile was last put on
  DevBuf<unsigned int> plan_len;   // [3] list lengths (k_plan_relax)
  DevBuf<unsigned long long> plan_stat;    // [4] reached, traversable, rounds, tile relaxations; [4..5] path length, error
  HostBuf<unsigned long long> h_plan;       // mapped: the last round's list length, rounds, relaxations, traversable
  DevBuf<int64_t> plan_src;        // [256] source cells
  DevBuf<double> plan_qxy;         // [plan_qcap][2] query targets
  DevBuf<uint32_t> plan_qcost;     // [plan_qcap]
  DevBuf<int64_t> plan_qcell;      // [plan_qcap]
  GroupCap plan_qcap;
  DevBuf<int64_t> plan_path;       // a path, target first
  // dm_plan_field_cost: the per-cell penalty bytes pen[d2] the weighted field
  // was relaxed over (k_plan_clear<true> writes them, k_plan_relax<true, .> and the
  // weighted k_plan_path read them), allocated on the first such call
  DevBuf<uint8_t> plan_pen;        // [H][W] row-major
  DevBuf<uint8_t> plan_pen_tab;    // [32 * 32 + 2] the caller's table
  bool plan_weighted = false;         // the field held is dm_plan_field_cost's
  bool plan_valid = false;
  uint64_t plan_version = 0;
  uint64_t reset_seq = 0;             // dm_reset calls so far
  // DM_PLAN_MAX_ROUNDS (read at dm_create; the test of DM_ERR_INCOMPLETE):
  // overrides the relaxation's round bound; 0: the derived bound
  int64_t plan_max_rounds = 0;
  // team fields (dm_plan_team, dm_assign_goals_team; dm_plan.h §4), beside the
  // single field and independent of it; allocated on first use, the arrays
  // sized by the number of robots grown when a later call brings more
  DevBuf<uint32_t> team_cost;      // [team_n][H][W]
  DevBuf<uint64_t> team_trav;      // [NT][64] the team's traversable bit rows, no source in them
  DevBuf<uint64_t> team_travp;     // [NT][64] dm_plan_team_path: the same with one robot's source bit
  DevBuf<int64_t> team_src;        // [DM_PLAN_TEAM_MAX] source cell of field k
  DevBuf<int32_t> team_list[2];    // [n * NT] active (field, tile) items of even / odd rounds
  DevBuf<uint32_t> team_stamp;     // [n][NT]
  DevBuf<unsigned int> team_len;   // [3] list lengths
  // [0..3] as plan_stat (0 unused), [4..5] path length, error, [8 + k] reached cells of field k
  DevBuf<unsigned long long> team_stat;
  HostBuf<unsigned long long> h_team;  // mapped, as h_plan
  DevBuf<uint32_t> team_qcost;     // [team_n][n] dm_plan_team_query's matrix
  DevBuf<int64_t> team_qcell;
  int32_t team_n = 0;              // fields held
  bool team_valid = false;
  uint64_t team_version = 0;

  // scan matcher (dm_match.h; dm_match_field and dm_match_scans), allocated
  // on first use.  match_V is the response field of (match_r, match_kern_h)
  // on map version match_version, built for the tiles flagged in match_built
  // only: a call builds the tiles its search windows reach and are not built
  // yet, so the fine stage of a two-stage match reuses the coarse stage's.
  DevBuf<uint8_t> match_V;         // [H][W] row-major
  DevBuf<uint8_t> match_kern;      // [16 * 16 + 1] the smear table
  DevBuf<int32_t> match_tiles;     // [NT] tiles to build
  std::vector<uint8_t> match_built;   // [NT] host flags
  std::vector<uint8_t> match_kern_h;  // the table match_V was built from
  int32_t match_r = -1;
  uint64_t match_version = 0;
  // per-call scratch, grown on demand
  DevBuf<double> match_pose4;      // [S * A][4] x, y, cos, sin of every candidate yaw
  DevBuf<double> match_trig;       // [N][2] cos, sin of the beam angles
  DevBuf<float> match_ranges;      // [S][N]
  DevBuf<int2> match_q;            // [S * A][N] fine coordinates
  DevBuf<uint32_t> match_vol;      // [S][A][2 half + 1][2 half + 1] scores
  DevBuf<int32_t> match_out;       // [S][4] k, i, j, score, then [S] used beams
  uint64_t match_epoch = 0;           // bumped whenever match_built is dropped (new table or map version)

  // whole-window relocalisation (dm_match_global.h; dm_match_global), allocated
  // on first use.  mg_pool is the max-pooled field M_B of match_V for block
  // size mg_pool_block, decimated by phase, built for the 64 x 64 tiles of
  // extended coordinates flagged in mg_pool_built; it is dropped with the
  // field (mg_pool_epoch != match_epoch) and on another block size.
  DevBuf<uint8_t> mg_pool;         // [B][B][EHB][EWB]
  DevBuf<int32_t> mg_ptiles;       // pool tiles to build
  std::vector<uint8_t> mg_pool_built; // [PTY][PTX] host flags
  int32_t mg_pool_block = 0;
  uint64_t mg_pool_epoch = 0;
  DevBuf<uint32_t> mg_bound;       // [A][nby][nbx] bounds of one scan; 0 once refined
  DevBuf<uint32_t> mg_hist;        // [kBins]
  DevBuf<uint32_t> mg_ctl;         // [C_WORDS] the round's count, bin and cap
  DevBuf<int32_t> mg_list;         // [mg_batch] the round's blocks
  DevBuf<int4> mg_cand;            // [kMgExhaustiveBatch >= mg_batch] dm_mg::Cand (16 bytes)
  DevBuf<int4> mg_best;            // dm_mg::Cand, the running best
  DevBuf<int32_t> mg_nused;        // the scan's used beams
  HostBuf<uint32_t> h_mg;           // mapped [8]: score, k, i, j, blocks of the round, used beams
  // DM_MATCH_GLOBAL_BATCH (read at dm_create): the most blocks one round
  // refines; any value gives the same result
  int64_t mg_batch = 4096;
  static constexpr int32_t kMgExhaustiveBatch = 65536;

  // information gain (dm_gain.h; dm_gain_views and dm_assign_goals_gain),
  // grown on demand
  DevBuf<double> gain_xy;          // [gain_cap][2] view points
  DevBuf<int64_t> gain_cell;       // [gain_cap] view cells
  DevBuf<uint32_t> gain_out;       // [gain_cap] gains (dm_assign_goals_gain: one robot's row)
  DevBuf<uint8_t> gain_skip;       // [gain_cap] views not to cast
  DevBuf<int64_t> gain_memo_cell;  // [gain_cap] per cluster: the cell of its last cast (one call)
  DevBuf<uint32_t> gain_memo_gain; // [gain_cap] and its gain
  GroupCap gain_cap;
  // the claimed set of dm_gain_views_joint / dm_assign_goals_coord: H rows of
  // ceil(W / 32) words, allocated by the first of the two calls
  DevBuf<uint32_t> gain_claimed;
  bool gain_claimed_valid = false;    // one of the two calls has run (dm_gain_claimed)

  // map fusion (dm_fuse.hip): covered, contributing, state-changed cells of the call, allocated on first use
  DevBuf<unsigned long long> fuse_stats;

  // profiling
  bool profile = false;
  std::vector<KernelTimer> pending;
  std::vector<dm_kernel_stat> stats;
};

// The workspace set of the last frontier pass.
inline dm_grid::FrWs& dm_last_fw(dm_grid* g) { return g->fw[g->fparity]; }

// the set the next integrate call will use
inline int dm_next_set(const dm_grid* g) { return (g->iw_cur + 1) % dm_grid::kIntSets; }

// Settle the free events owed by the integrate workspaces (their last
// accumulation is enqueued on g->stream before this point): `recorded`, an
// event just recorded on g->stream, or each set's own ev_free recorded now.
inline hipError_t dm_mark_ws_free(dm_grid* g, hipEvent_t recorded = nullptr) {
  for (int i = 0; i < dm_grid::kIntSets; ++i) {
    dm_grid::IntWs& w = g->iw[i];
    if (!w.free_owed) continue;
    w.free_owed = false;
    w.free_wait = recorded ? recorded : w.ev_free;
    if (recorded) continue;
    const hipError_t e = hipEventRecord(w.ev_free, g->stream);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// Host wait for an event the pipelined caller expects within tens of
// microseconds (a readback slot's pass): poll it instead of
// hipEventSynchronize, which after a short active wait sleeps on an
// interrupt and wakes up tens of microseconds late (the bench's step
// cadence showed +20-80 us spikes on ~10 % of the steps).  After kSpinNs of
// polling it blocks as before: 2 ms, like ShardedMapper._poll's window (a
// pipelined C3 pass ends ~70 us after the host starts waiting; longer waits
// should not keep a host core busy, which several ranks' threads would
// compete for).
inline void dm_cpu_relax() {
#if defined(__x86_64__) || defined(__i386__)
  __builtin_ia32_pause();
#elif defined(__aarch64__)
  asm volatile("yield" ::: "memory");
#else
  std::atomic_signal_fence(std::memory_order_seq_cst);
#endif
}

inline hipError_t dm_event_wait(hipEvent_t ev) {
  constexpr long long kSpinNs = 2000000;  // 2 ms
  const auto t0 = std::chrono::steady_clock::now();
  for (unsigned it = 0;; ++it) {
    const hipError_t e = hipEventQuery(ev);
    if (e != hipErrorNotReady) return e;
    if ((it & 63u) == 63u &&
        std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count() > kSpinNs)
      return hipEventSynchronize(ev);
    dm_cpu_relax();
  }
}

// Order `stream` after the pass_stream work enqueued so far (the frontier
// arrays other than the parity sets are shared by all passes).
inline hipError_t dm_join_pass_stream(dm_grid* g) {
  if (!g->p_tail.pending) return hipSuccess;
  g->p_tail.pending = false;
  return hipStreamWaitEvent(g->stream, g->p_tail.ev, 0);
}

// A pass of workspace set `set` (nullptr: a merge, which uses none) with
// number `pass` ends here on stream `s`: record `ev` there and note it as the
// set's last pass and, on a stream other than the handle's, as the work
// `stream` has yet to be ordered after.
inline hipError_t dm_note_pass_end(dm_grid* g, dm_grid::FrWs* set, hipEvent_t ev, hipStream_t s, uint64_t pass) {
  const hipError_t e = hipEventRecord(ev, s);
  if (e != hipSuccess) return e;
  const dm_grid::PassEnd end{ev, true, pass};
  if (set) set->busy = end;
  if (s != g->stream) g->p_tail = end;
  return hipSuccess;
}

// A call with too few beams to fill the chip enumerates each beam's pieces
// in `chunks` k-ranges on different threads (k_beam_prep / k_scatter): one
// thread per beam would walk up to 2*nmax/64 pieces serially on a mostly
// idle GPU (sparse scans, 1 cm maps).  Chunks stay >= 64 steps long.
inline int32_t dm_integrate_chunks(const dm_grid* g, int64_t nb) {
  const int64_t want = (int64_t)dm_grid::kChunkThreadsPerCu * (int64_t)(g->n_cu > 0 ? g->n_cu : 256);
  if (nb <= 0 || nb >= want) return 1;
  const int64_t by_len = (g->nmax + 1) / 64 > 1 ? (g->nmax + 1) / 64 : 1;
  const int64_t by_fill = (want + nb - 1) / nb;
  return (int32_t)(by_fill < by_len ? by_fill : by_len);
}


// ---- launchers (dm_integrate.hip / dm_frontier.hip) -----------------------
int dm_launch_integrate(dm_grid* g, int32_t S, const double* d_pose4, int32_t N,
                        const float* d_ranges, const double* d_trig);
int dm_launch_recount(dm_grid* g);
// swap: rebuild into the other list and switch (passes may be in flight);
// otherwise into the current one (every stream joined: bulk writes)
int dm_launch_relist(dm_grid* g, bool swap);
// Passes between rebuilds of the tile list in tile order (dm_launch_relist),
// once the doubling period from a fresh list reaches it.
constexpr int kRelistPasses = 16;
int dm_launch_state_from_logodds(dm_grid* g);
int dm_launch_map_image(dm_grid* g, uint8_t* d_img);
int dm_launch_set_state(dm_grid* g, const int8_t* d_state_in);
// The pass's sorted records and readback go to slot `r`.  split: the labelling
// half on g->pass_stream (dm_frontiers_begin with overlap); *end_stream
// receives the stream the pass ends on.
int dm_enqueue_frontiers(dm_grid* g, dm_grid::RbSlot& r, bool want_mask, bool want_labels, bool split = false,
                         hipStream_t* end_stream = nullptr);
// Hand-off between streams (dm_integrate.hip): k_seq_signal counts
// flag[kSigWord] up; k_seq_gate (one lane) counts flag[kGateWord] up and waits
// until flag[kSigWord] reaches it (+ fault: fault-injection tests), or sets
// err_bit in *err after a bounded time (ticks of the 100 MHz clock, 0: 5 s).
int dm_launch_signal(hipStream_t s, unsigned long long* flag);
int dm_launch_gate(hipStream_t s, unsigned long long* flag, unsigned long long* err, unsigned long long err_bit,
                   unsigned long long ticks = 0, unsigned long long fault = 0);
int dm_launch_edge_labels(dm_grid* g);
int dm_frontiers_readback(dm_grid* g, const dm_grid::RbSlot& r, int64_t* n_clusters, int64_t* copied);
int dm_launch_frontiers(dm_grid* g, dm_grid::RbSlot& r, bool want_mask, bool want_labels, int64_t* n_clusters,
                        int64_t* copied);
// What both device sorts take (the band pass's and the merge's records).
struct SortArgs {
  long long* clusters;  // [max_records][4] raw records
  // slot sums (slot_acc) and slot labels when the records were written by the
  // fused compaction (-(slot + 1) in place of the size), else nullptr
  const long long* sums;
  const long long* labels;
  const unsigned long long* d_count;  // device: the record count
  int64_t max_records;
  dm_cluster* out;                    // sorted records
  int32_t* rank_of;                   // record -> sorted position, or nullptr
  unsigned long long* d_sorted;       // device flag: 1 when `out` holds them sorted
  const unsigned long long* cnt;      // the counter block copied into the readback header,
  int ncnt, sorted_idx;               // its length, the flag's index in it
  const unsigned long long* fsh;      // frontier shards for the header, or nullptr
  dm_raw_record* host_out;            // mapped readback records (device address) and their capacity
  int64_t host_cap;
};
// expect: the last collected count of its kind (sizes the grid).
int dm_launch_rank_sort(const dm_grid* g, hipStream_t stream, const SortArgs& a, int64_t expect);
// Listed tiles from which a frontier pass reads fmask instead of state bytes.
constexpr int64_t kFmaskOnTiles = 8192;
// tile_free: the listed flag above the free count (<= 4096)
constexpr int32_t kTileListed = 1 << 30;
constexpr int32_t kTileFreeMask = kTileListed - 1;
// Frontier slots (tile-local components) per map tile allocated at dm_create.
constexpr int64_t kSlotsPerTile = 4;
// The slot group (slot_cap) for at least `need` slots and twice what it held.
int dm_grow_slots(dm_grid* g, int64_t need);
int dm_grow_bucket_sort(dm_grid* g, int64_t n);
// Row-bucket sort of the raw records (labels of rows [row_base, row_base +
// rows)): same outputs, readback header and flags as dm_launch_rank_sort.
int dm_launch_bucket_sort(dm_grid* g, hipStream_t stream, const SortArgs& a, int64_t row_base, int64_t rows);
// cross-band exchange (dm_merge.hip): the export reads the band pass's sorted
// records from slot `r`, the merge writes its own there
int64_t dm_export_nbytes(int64_t W, int64_t rec_cap);
int dm_launch_export(dm_grid* g, const dm_grid::RbSlot& r, hipStream_t s, void* d_export, int64_t rec_cap);
int dm_launch_merge(dm_grid* g, dm_grid::RbSlot& r, hipStream_t s, const void* d_gathered, int32_t nranks,
                    int64_t rec_cap, int64_t min_size);
// The stream band exports end on and merges run on (dm_exchange_stream).
inline hipStream_t dm_exchange_stream_of(const dm_grid* g) { return g->overlap ? g->pass_stream : g->stream; }
int dm_launch_ld06(dm_grid* g, int32_t S, const dm_ld06_point* d_pts, const int64_t* d_offsets,
                   int32_t N, int dir, float* d_ranges, float* d_intensities);

// sharded parents (dm_sharded.cpp): the public calls dispatch here
int dm_sh_destroy(dm_grid* g);
int dm_sh_reset(dm_grid* g);
int dm_sh_integrate(dm_grid* g, int32_t S, const double* poses, int32_t N, const float* ranges, float amin,
                    float inc, uint64_t* U, uint64_t* T);
int dm_sh_integrate_async(dm_grid* g, int32_t S, const double* poses, int32_t N, const float* ranges,
                          float amin, float inc);
int dm_sh_integrate_device(dm_grid* g, int32_t S, const double* d_pose4, int32_t N, const float* d_ranges,
                           float amin, float inc);
int dm_sh_last_counts(dm_grid* g, uint64_t* U, uint64_t* T);
int dm_sh_last_stats(dm_grid* g, uint64_t* out, int32_t cap, int32_t* n_out);
int dm_sh_frontier_cache_stats(dm_grid* g, uint64_t* hits, uint64_t* misses);
int dm_sh_get_state(dm_grid* g, int8_t* out);
int dm_sh_get_logodds(dm_grid* g, float* out);
int dm_sh_set_logodds(dm_grid* g, const float* in);
int dm_sh_set_state(dm_grid* g, const int8_t* in);
// dm_fuse_* on a sharded parent: one_band(band, ctx, stats[3]) on every band, stats summed
typedef int (*dm_fuse_band_fn)(dm_grid* band, void* ctx, uint64_t* stats);
int dm_sh_fuse(dm_grid* g, int same_device, uint64_t* out_stats, dm_fuse_band_fn one_band, void* ctx);
int dm_sh_frontiers(dm_grid* g, uint8_t* mask, int64_t* labels, dm_cluster* out, int64_t cap, int64_t* n_out);
int dm_sh_frontiers_begin(dm_grid* g);
int dm_sh_frontiers_end(dm_grid* g, dm_cluster* out, int64_t cap, int64_t* n_out);
int dm_sh_frontiers_poll(dm_grid* g, int32_t* ready);
int dm_sh_assign_goals(dm_grid* g, const double* robots_xy, int32_t n_robots, int64_t min_size, double w,
                       double min_distance, int64_t* out_index, double* out_xy);
int dm_sh_set_overlap(dm_grid* g, int32_t on);
int dm_sh_synchronize(dm_grid* g);
int dm_sh_profile_enable(dm_grid* g, int enable);
int dm_sh_profile_read(dm_grid* g, dm_kernel_stat* out, int32_t cap, int32_t* n_out);
int dm_sh_profile_reset(dm_grid* g);
int dm_sh_map_image(dm_grid* g, uint8_t* out);
int dm_sh_ld06_to_scans(dm_grid* g, int32_t S, const dm_ld06_point* points, const int64_t* offsets, int32_t N,
                        int dir, float* ranges, float* intensities);
int dm_sh_ld06_to_scans_device(dm_grid* g, int32_t S, const dm_ld06_point* d_points, const int64_t* d_offsets,
                               int32_t N, int dir, float* d_ranges, float* d_intensities);

// error plumbing (dm_api.cpp)
int dm_set_error(int code, const char* fmt, ...);
int dm_hip_check(hipError_t e, const char* what);
void dm_timer_begin(dm_grid* g, const char* name, KernelTimer* t, hipStream_t s = nullptr);
void dm_timer_end(dm_grid* g, KernelTimer* t);

#define DM_HIP(call)                                         \
  do {                                                       \
    hipError_t _e = (call);                                  \
    if (_e != hipSuccess) return dm_hip_check(_e, #call);    \
  } while (0)

// ---- what the entry points of every file share (dm_api.cpp, dm_goals.hip,
// dm_match.hip) ---------------------------------------------------------------
int check_grid(const dm_grid* g);   // the handle is not NULL
int use_device(const dm_grid* g);   // hipSetDevice(the handle's)
int check_integrate_args(int32_t S, int32_t N, const void* poses, const void* ranges);
// Wait for all four streams; nothing of this handle is in flight afterwards.
hipError_t dm_sync_all(dm_grid* g);
// The planner, the gain calls, the goal calls that use them and both matchers
// need the whole map in one handle: not a sharded parent, not a row band.
int dm_check_whole_map(const dm_grid* g, const char* what);
// What a field, a response field or a claimed set was computed for: any map
// change moves it.
inline uint64_t dm_map_version(const dm_grid* g) { return g->integrate_seq + g->reset_seq; }

// Kernel launch.
#define DM_LAUNCH(kernel, grid, block, shmem, stream, ...) \
  hipLaunchKernelGGL(kernel, grid, block, shmem, stream, __VA_ARGS__)

// Round n up to a quarter-octave step (1, 1.25, 1.5, 1.75 x 2^k; exact below
// 8): grid sizes derived from the last pass's statistics take few values.
inline int64_t dm_quantize_up(int64_t n) {
  if (n <= 8) return n;
  int sh = 0;
  while ((n >> sh) >= 8) ++sh;
  const int64_t step = (int64_t)1 << sh;  // n in [4, 8) x 2^sh: steps of a quarter octave
  return ((n + step - 1) / step) * step;
}
