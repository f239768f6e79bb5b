/*
 * dm.h — C-ABI of libdm.so: MI355X-native occupancy-grid integration and
 * exploration-frontier extraction (the BASELINE.json north-star hot path).
 *
 * WHAT THIS REPLACES
 *   The reference has no FFI for this path: its boundary is ROS 2 topics.
 *   `/scan` (sensor_msgs/LaserScan, produced by the LD06 driver's
 *   ToLaserscanMessagePublish, pi/src/ldlidar_ros2_ws/install/ldlidar_stl_ros2/
 *   lib/ldlidar_stl_ros2/ldlidar_stl_ros2_node @0x7f853) goes into slam_toolbox
 *   (launched at server/thymio_project/launch/pc_server.launch.py:12-19,
 *   configured by server/thymio_project/config/slam_config.yaml:16-28), which
 *   publishes `/map` (nav_msgs/OccupancyGrid, int8 -1/0/100 row-major) consumed
 *   by ThymioBrain.map_cb (server/thymio_project/thymio_project/main.py:46,80-81)
 *   and get_map_image (main.py:241-279).  Frontier extraction exists nowhere in
 *   the reference; its contract is SURVEY.md §8(a) rows a8-a10.
 *   Each entry point below names the step of that pipeline it takes over.  The
 *   ctypes binding a ROS node would add is shown in INTEGRATION.md.
 *   The dm_plan_* calls and dm_assign_goals_path go past the reference: they
 *   are the map-based navigation its report lists as future work (§VI-2,
 *   Nav2): an inflated traversability mask, a shortest-path distance field,
 *   reachable goals and the paths to them, all on the device-resident map.
 *
 * CONVENTIONS
 *   - Every function returns int: DM_OK (0) or a negative DM_ERR_* code; on
 *     error dm_last_error() (thread-local) describes it.  Nothing aborts.
 *   - Host pointers are caller-owned, C-contiguous, borrowed for the call only.
 *   - Functions without a `_device` suffix are synchronous: they return after
 *     their outputs are in host memory.  `_device` functions take device
 *     pointers, enqueue on the handle's stream and return immediately.
 *   - A handle is NOT internally thread-safe (the Python wrapper locks).
 *   - Grid layout: row-major, idx = (cy - band_row0) * width + cx, row 0 at the
 *     map origin (bottom-left), exactly the OccupancyGrid.data layout read by
 *     get_map_image (main.py:256, flipud at :266).
 */
#ifndef DM_H
#define DM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DM_OK 0
#define DM_ERR_INVALID_ARG (-1)
#define DM_ERR_SHAPE (-2)
#define DM_ERR_HIP (-3)
#define DM_ERR_OOM (-4)
#define DM_ERR_CAPACITY (-5)
#define DM_ERR_IO (-6)
#define DM_ERR_STATE (-7)
#define DM_ERR_INCOMPLETE (-8) /* a pass has no result: an export record was incomplete, a
                                  union-find loop hit its iteration bound, or dm_plan_field's
                                  relaxation hit its round bound */
#define DM_ERR_PIPELINE (-9)   /* a cross-stream hand-off of the overlapped pipeline (dm_set_overlap)
                                  timed out: the map update it guarded was skipped, so the map
                                  misses batches; sticky until dm_reset */
#define DM_ERR_COLLECTIVE (-10) /* a cross-device exchange of a sharded map failed or did not finish
                                  within its timeout (a peer copy of a dm_create_sharded handle; the
                                  RCCL collectives of the multi-process layer, dm/sharded.py);
                                  sticky: the sharded map must be recreated */

/* Tile edge (cells) used by the kernels; band_row0 must be a multiple of it. */
#define DM_TILE 64

/* Distance-field value of a cell no path reaches (dm_plan_field). */
#define DM_PLAN_UNREACHABLE 0xFFFFFFFFu

/* Map parameters.  Defaults (dm_default_params) come from the reference where
 * it has them: resolution 0.05 (slam_config.yaml:26), max range 12.0
 * (slam_config.yaml:27), LD06 range_min 0.02f (driver rodata 0xbc840).  The
 * log-odds constants are this build's SPEC.
 * Signed zeros: a -0.0 in l_min, l_max, occ_thresh or free_thresh is read as
 * +0.0, so a cell clamped to a zero bound stores +0.0, never -0.0.
 * occ_thresh / free_thresh may be +-inf ("never occupied" / "never free") but
 * not NaN (DM_ERR_INVALID_ARG). */
typedef struct dm_params {
  int64_t width;            /* cells along x (columns), global */
  int64_t height;           /* cells along y (rows), global */
  double resolution;        /* metres per cell */
  double origin_x;          /* world x of the lower-left corner of cell (0,0) */
  double origin_y;          /* world y of the lower-left corner of cell (0,0) */
  float range_min;          /* beams with r < range_min (or NaN) are skipped */
  float range_max;          /* r > range_max: ray truncated there, no hit */
  float l_occ;              /* log-odds added per hit */
  float l_free;             /* log-odds added per miss (negative) */
  float l_min;              /* clamp low */
  float l_max;              /* clamp high */
  float occ_thresh;         /* L >= occ_thresh (and L != 0) -> 100 */
  float free_thresh;        /* L <= free_thresh (and L != 0) -> 0 */
  int64_t min_frontier_size;/* clusters smaller than this are dropped */
  int64_t band_row0;        /* first global row owned by this handle */
  int64_t band_rows;        /* rows owned; 0 means height - band_row0 */
} dm_params;

/* One frontier cluster.  label = min global row-major
 * linear index (cy*width+cx) of the component; sums are over global cell
 * coordinates; cx_m = origin_x + ((double)sum_x/(double)size + 0.5)*resolution. */
typedef struct dm_cluster {
  int64_t label;
  int64_t size;
  int64_t sum_x;
  int64_t sum_y;
  double cx_m;
  double cy_m;
} dm_cluster;

/* Per-kernel timing collected with HIP events when profiling is enabled. */
typedef struct dm_kernel_stat {
  char name[32];
  uint64_t launches;
  double total_ms;
} dm_kernel_stat;

typedef struct dm_grid dm_grid;

/* Fill p with defaults for a width x height map centred on the world origin. */
int dm_default_params(dm_params* p, int64_t width, int64_t height);

/* Create a grid on HIP device `device`: L = 0, state = -1 everywhere.
 * Replaces slam_toolbox's map allocation (grid sized from the scan bounding
 * box on every rebuild upstream; here fixed, device-resident). */
int dm_create(dm_grid** out, const dm_params* p, int device);
int dm_destroy(dm_grid* g);
/* Reset to the empty map (L = 0, state = -1). */
int dm_reset(dm_grid* g);
int dm_get_params(const dm_grid* g, dm_params* out);

/* Integrate S scans of N beams.  poses: [S][3] =
 * (x_m, y_m, yaw_rad) of the laser in the map frame (main.py:202-215 TF chain
 * + pi_hardware.launch.py:26-30 static offset); ranges: [S][N] metres as
 * LaserScan.ranges (NaN = no return); beam i angle = angle_min + i*angle_increment
 * (LaserScan.angle_min / angle_increment).  cos/sin are evaluated on the host
 * with the C library.  out_updates (may be NULL) receives the number of
 * in-band beam-cell updates U; out_touched (may be NULL) the touched cells T.
 * Replaces: slam_toolbox's per-scan ray trace + grid update that produces /map. */
int dm_integrate(dm_grid* g, int32_t S, const double* poses, int32_t N,
                 const float* ranges, float angle_min, float angle_increment,
                 uint64_t* out_updates, uint64_t* out_touched);

/* Asynchronous host-input variant of dm_integrate: the same inputs (host
 * pointers), enqueued and not waited for — the H2D copies of poses and
 * ranges run on the library's streams and, when `ranges` is pinned host
 * memory (hipHostMalloc / torch pin_memory), overlap work in flight (with
 * dm_set_overlap: the previous frontier pass).  `ranges` must stay valid and
 * unchanged until the copy is done: until the second dm_integrate_async call
 * after this one returns, or dm_synchronize / dm_last_counts.  `poses` is
 * read before the call returns.  Read U and T with dm_last_counts.  This is
 * the PCIe-inclusive form of the ROS node's per-scan call. */
int dm_integrate_async(dm_grid* g, int32_t S, const double* poses, int32_t N,
                       const float* ranges, float angle_min, float angle_increment);

/* Device-resident variant (asynchronous on the handle's stream).
 * d_pose4: [S][4] = (x, y, cos(yaw), sin(yaw)) doubles in device memory;
 * d_ranges: [S][N] floats in device memory.  Counters for the call are
 * accumulated on the device; read them with dm_last_counts. */
int dm_integrate_device(dm_grid* g, int32_t S, const double* d_pose4,
                        int32_t N, const float* d_ranges, float angle_min,
                        float angle_increment);
/* U and T of the most recent integrate call (synchronises the stream). */
int dm_last_counts(dm_grid* g, uint64_t* updates, uint64_t* touched);

/* Diagnostics of the most recent calls (synchronises the stream):
 * out[0..6] = integrate: U, T, T applied by the heavy-tile pass, pieces (ray
 * pieces binned by tile), active tiles, apply work items, heavy tiles;
 * out[7..9] = frontiers: tiles visited, tile-local components, clusters;
 * out[10] = integrate: sparse work items (light tiles with at most 15
 * pieces, which load only the cells they touch; counted in out[5] too).
 * *n_out = the number of entries the library has (11); a caller's smaller
 * cap gets the first cap of them. */
int dm_last_stats(dm_grid* g, uint64_t* out, int32_t cap, int32_t* n_out);

/* The frontier label cache.  The dense-pass tile kernel keeps, per map tile,
 * the tile-local labelling (components, their sizes and sums, the component
 * of every edge cell) together with the 64 frontier bit rows it was computed
 * from; a pass whose bit rows for a tile equal the stored ones reuses it (a
 * hit), any other tile with frontier cells is labelled in full (a miss).
 * Validity is by content only, so no call invalidates it and results are the
 * same with and without it (DM_FRONTIER_CACHE=off, read at dm_create,
 * switches it off).  *hits / *misses = the counts of the last collected
 * frontier pass (on a sharded handle: summed over the bands' last passes).
 * 1.25 KB of device memory per tile, allocated with the first pass; if that
 * allocation fails the passes run uncached. */
int dm_frontier_cache_stats(dm_grid* g, uint64_t* hits, uint64_t* misses);

/* OccupancyGrid.data for the band: int8[band_rows*width] (-1 / 0 / 100). */
int dm_get_state(dm_grid* g, int8_t* out);
/* Log-odds for the band: float[band_rows*width]. */
int dm_get_logodds(dm_grid* g, float* out);
/* Overwrite L (and derived state / tile summaries) from host floats. */
int dm_set_logodds(dm_grid* g, const float* in);
/* Same as dm_set_logodds but from a host int8 state image: L := +l_occ for
 * 100, l_free for 0, 0 for -1 (testing and map import). */
int dm_set_state(dm_grid* g, const int8_t* in);

/* Frontier extraction: mask (uint8[band_rows*width],
 * may be NULL), labels (int64[band_rows*width], -1 off-frontier, may be NULL),
 * clusters sorted by label (capacity cap).  *n_out receives the number of
 * clusters; if it exceeds cap, DM_ERR_CAPACITY is returned and only cap were
 * written.  For a band, labels are band-local (the min index within the band's
 * part of a component); the sharded layer merges them across bands. */
int dm_frontiers(dm_grid* g, uint8_t* mask, int64_t* labels, dm_cluster* out,
                 int64_t cap, int64_t* n_out);

/* Pipelined frontier passes.  dm_frontiers_begin enqueues a clusters-only
 * frontier pass (the same pipeline as dm_frontiers with mask = labels = NULL)
 * on the handle's stream and returns; dm_frontiers_end waits for THAT pass
 * (an event, not the stream: integrate calls made in between keep running)
 * and returns its clusters exactly as dm_frontiers would have on the map as
 * it was at dm_frontiers_begin.  One pass may be in flight per handle; on
 * DM_ERR_CAPACITY (*n_out = clusters) the pass stays pending, so call _end
 * again with cap >= *n_out.  If
 * the pass overflowed the slot arrays they are grown and DM_ERR_INCOMPLETE
 * is returned with *n_out = 0: that pass has no result (run dm_frontiers).
 * The reference (main.py:123-188) has no frontier step; this is the
 * planner-facing form of SURVEY.md §8 a8-a10 used by a ROS node that keeps
 * integrating scans while the last frontier request completes. */
int dm_frontiers_begin(dm_grid* g);
int dm_frontiers_end(dm_grid* g, dm_cluster* out, int64_t cap, int64_t* n_out);
/* Non-blocking test of the oldest asynchronous pass (dm_frontiers_begin or
 * dm_merge_bands_begin): *ready = 1 when it has completed (its _end call then
 * returns without waiting), else 0.  DM_ERR_INVALID_ARG if no pass is in
 * flight.  Lets a ROS callback thread publish frontiers without ever
 * blocking on the GPU. */
int dm_frontiers_poll(dm_grid* g, int32_t* ready);
/* The number of asynchronous passes (dm_frontiers_begin /
 * dm_merge_bands_begin) a handle holds in flight: the readback ring's size. */
int dm_max_passes_in_flight(void);

/* Overlap mode (default off).  When on, the integrate front-end of
 * dm_integrate / dm_integrate_device (beam preparation, tile planning, piece
 * scatter: everything that reads poses / ranges and not the map) runs on an
 * internal stream that waits only for the previous integrate call's map
 * update, so it overlaps a frontier pass still in flight on the handle's
 * stream; the map update itself stays in the handle's stream order, after
 * every earlier call.  Results are identical with overlap on or off.  With
 * overlap on, the device inputs of dm_integrate_device must be complete when
 * the call is made (e.g. produced by work the host already synchronised).
 * The streams hand off through bounded device-side waits (5 s); one that
 * times out (a tool that runs one dispatch at a time, e.g. rocprofv3 --pmc,
 * can cause it) skips the map update it guarded and every later call that
 * reads results returns DM_ERR_PIPELINE until dm_reset. */
int dm_set_overlap(dm_grid* g, int32_t on);


/* ---- One map sharded over several devices of this process (SURVEY.md §8(b)
 * "sharded variants: dm_create_sharded(..., int nranks, const int* devices)
 * with the same calls"; §8(e) row bands).  Band r (rows from
 * dm_sharded_band_rows: equal multiples of 64, the last ragged) lives on
 * HIP device devices[r]; a device may repeat (tests run {0, 0, ...} on one
 * GPU).  p covers the whole grid (band_row0 = 0, band_rows = 0).  The handle
 * takes the calls of a dm_create handle — dm_integrate(_async / _device),
 * dm_last_counts / _stats, dm_get_state / _logodds, dm_set_state / _logodds,
 * dm_frontiers (mask and labels are whole-map arrays with global min-index
 * labels), dm_frontiers_begin / _end / _poll, dm_assign_goals,
 * dm_map_image, dm_save / dm_load (the same checkpoint format as one
 * full-map handle), dm_reset, dm_set_overlap, dm_synchronize, dm_profile_*,
 * dm_ld06_to_scans(_device), dm_destroy — with results identical to one
 * dm_create handle of the same params.  Integration sends each band the
 * scans whose max-range disk reaches it; frontier extraction exchanges halo
 * rows and band export records between the devices with peer copies (xGMI)
 * and merges on band 0's device (dm_merge_bands).  The multi-process building
 * blocks below (halos, edge rows / labels, exports, merges, dm_set_stream)
 * return DM_ERR_INVALID_ARG on such a handle, and so do the path planning
 * calls (dm_plan_*, dm_assign_goals_path) and the scan matcher (dm_match_*),
 * and the information-gain calls (dm_gain_views, dm_assign_goals_gain),
 * which need the whole map in one handle: sharded planning and matching are
 * not implemented.  Replaces: slam_toolbox's
 * single map thread for a map too large (or too many robots) for one GPU;
 * the caller is the ROS node wired at pc_server.launch.py:12-19. */
int dm_create_sharded(dm_grid** out, const dm_params* p, int32_t nranks, const int32_t* devices);
/* The rows [*row0, *row0 + *rows) of band `rank` of `nranks` (the partition
 * of dm_create_sharded and of the multi-process layer, dm/sharded.py). */
int dm_sharded_band_rows(int64_t height, int32_t nranks, int32_t rank, int64_t* row0, int64_t* rows);
/* nranks of a handle (1 for dm_create handles) and the export record
 * capacity its exchange uses now (0 for dm_create handles). */
int dm_sharded_info(const dm_grid* g, int32_t* nranks, int64_t* rec_cap);

/* Sharding support (row bands).  Halo rows are the global
 * rows band_row0-1 (top, "above" = lower row index) and band_row0+band_rows
 * (bottom); NULL = no neighbour there.  Host and device variants. */
int dm_set_halo(dm_grid* g, const int8_t* row_before, const int8_t* row_after);
int dm_set_halo_device(dm_grid* g, const int8_t* d_row_before,
                       const int8_t* d_row_after);
/* Copy the band's first and last state rows (W bytes each). */
int dm_get_edge_rows(dm_grid* g, int8_t* first_row, int8_t* last_row);
int dm_get_edge_rows_device(dm_grid* g, int8_t* d_first_row, int8_t* d_last_row);
/* After dm_frontiers: band-local labels of the first/last rows (int64[W]). */
int dm_get_edge_labels(dm_grid* g, int64_t* first_row, int64_t* last_row);

/* ---- Cross-band frontier exchange, device-resident
 * Replaces the host-side label merge of a row-band sharded map: every band
 * writes an export record into a caller-owned device buffer, the caller
 * all-gathers the records with RCCL (rank order = band order, bands
 * contiguous), and dm_merge_bands resolves labels across band edges and
 * merges the clusters on the device.  Export record (little-endian,
 * dm_export_bytes bytes):
 *   int64 hdr[8]  K (band clusters), flags (0 = complete; bit0 slot overflow,
 *                 bit1 K > rec_cap, bit2 too many clusters to sort on the
 *                 device, bit5 union-find iteration bound hit), band_row0,
 *                 band_rows, width, 0, 0, 0
 *   int32 edge[2][width]  component of each cell of the band's first / last
 *                 row as an index into rec[], -1 off-frontier
 *   int64 rec[rec_cap][4] (label, size, sum_x, sum_y), sorted by label;
 *                 band-local min-index labels, global cell coordinates
 * The band handle must have min_frontier_size <= 1 (the size filter applies
 * to merged clusters: dm_merge_bands' min_size). */
int dm_export_bytes(const dm_grid* g, int64_t rec_cap, int64_t* bytes);
/* Band frontier extraction + export record, asynchronous (no host
 * synchronisation).  Halo rows must be set first.  With dm_set_overlap on,
 * the pass is split as in dm_frontiers_begin: the map reads stay on the
 * handle's stream and the labelling, the sort and the export record run on
 * the handle's exchange stream (dm_exchange_stream), so the next integrate
 * call's map update overlaps them; the caller's all-gather of the record and
 * dm_merge_bands(_begin) then belong on that stream. */
int dm_frontiers_export_device(dm_grid* g, void* d_export, int64_t rec_cap);
/* The hipStream_t the export record of dm_frontiers_export_device is
 * complete on and the merges run on: the handle's stream, or with overlap on
 * its pass stream.  Work ordered after it on that stream (an RCCL all-gather
 * of the record, dm_merge_bands) needs no other synchronisation. */
int dm_exchange_stream(dm_grid* g, void** stream);
/* Merge nranks gathered export records (d_gathered = nranks consecutive
 * records of dm_export_bytes(rec_cap) bytes) into global clusters sorted by
 * label, keeping those with size >= min_size.  Synchronous; runs on
 * dm_exchange_stream, so the gathered buffer must be complete in that
 * stream's order (e.g. all-gathered on it).  Returns
 * DM_ERR_INCOMPLETE (*n_out = largest band K) when a record is flagged
 * incomplete, DM_ERR_CAPACITY (*n_out = clusters) when cap is too small. */
int dm_merge_bands(dm_grid* g, const void* d_gathered, int32_t nranks, int64_t rec_cap,
                   int64_t min_size, dm_cluster* out, int64_t cap, int64_t* n_out);
/* dm_merge_bands split like dm_frontiers_begin / _end: _begin enqueues the
 * merge and returns, _end waits for it (event) and returns its result with
 * dm_merge_bands' error behaviour, except that on DM_ERR_CAPACITY the pass
 * stays pending (call _end again with cap >= *n_out).  d_gathered must stay
 * valid until _end. */
int dm_merge_bands_begin(dm_grid* g, const void* d_gathered, int32_t nranks, int64_t rec_cap,
                         int64_t min_size);
int dm_merge_bands_end(dm_grid* g, dm_cluster* out, int64_t cap, int64_t* n_out);
/* The largest band cluster count K of the last collected merge (every rank
 * merges the same gathered records, so every rank reads the same value: a
 * caller can size rec_cap for the next exports from it consistently). */
int dm_merge_max_band_k(const dm_grid* g, int64_t* max_k);

/* LD06 driver point (ldlidar::PointData fields the LaserScan conversion uses). */
typedef struct dm_ld06_point {
  float angle_deg;      /* 0..360 */
  uint16_t distance_mm;
  uint8_t intensity;
  uint8_t pad;
} dm_ld06_point;

/* LD06 PointData -> LaserScan.ranges/intensities for S revolutions, exactly
 * as the driver's ToLaserscanMessagePublish (ldlidar_stl_ros2_node @0x7f853;
 * SURVEY.md §8 a1): scan s holds points[offsets[s] .. offsets[s+1]), N beams,
 * angle_min 0, angle_increment 6.2831855f/(N-1), NaN = no return, keep the
 * nearest return per beam; laser_scan_dir mirrors the index
 * (pi_hardware.launch.py:20).  ranges_out: float[S][N]; intensities_out may
 * be NULL.  N must be in [2, 8192]. */
int dm_ld06_to_scans(dm_grid* g, int32_t S, const dm_ld06_point* points,
                     const int64_t* offsets, int32_t N, int laser_scan_dir,
                     float* ranges_out, float* intensities_out);
int dm_ld06_to_scans_device(dm_grid* g, int32_t S, const dm_ld06_point* d_points,
                            const int64_t* d_offsets, int32_t N, int laser_scan_dir,
                            float* d_ranges_out, float* d_intensities_out);

/* Checkpoint: raw little-endian {magic, params, float L[band]} . */
int dm_save(dm_grid* g, const char* path);
int dm_load(dm_grid* g, const char* path);

/* Streams and profiling. stream is a hipStream_t (NULL = library's own). */
int dm_set_stream(dm_grid* g, void* stream);
int dm_synchronize(dm_grid* g);
int dm_profile_enable(dm_grid* g, int enable);
int dm_profile_read(dm_grid* g, dm_kernel_stat* out, int32_t cap, int32_t* n_out);
int dm_profile_reset(dm_grid* g);

/* PNG-ready grayscale image of the band's state (f2, main.py:256-266):
 * 0 -> 255, 100 -> 0, anything else -> 127, rows flipped (flipud).
 * out: uint8[band_rows*width]. */
int dm_map_image(dm_grid* g, uint8_t* out);

/* Frontier goals for n_robots robots (replaces the
 * reactive IR / LiDAR policy, server/thymio_project/thymio_project/main.py:
 * 123-188, with map-based exploration).  Over the clusters of the last
 * collected result (dm_frontiers, dm_frontiers_end or dm_merge_bands; on the
 * device), robot r at robots_xy[2r], [2r+1] (metres) scores cluster c:
 *   dist = sqrt(dx*dx + dy*dy), dx = cx_m - x, dy = cy_m - y
 *   util = size / (1 + distance_weight * dist)   (double, no FMA)
 * over clusters with size >= min_size and dist >= min_distance, best util
 * first, ties to the smaller label; robots choose in order, each skipping the
 * clusters earlier robots took.  out_index[r] = index into that result's
 * label-sorted list (-1: none), out_xy[2r], [2r+1] = its centroid (NaN if
 * none).  n_robots <= 256; distance_weight >= 0 (DM_ERR_INVALID_ARG otherwise).
 * DM_ERR_INVALID_ARG if no result is on the device
 * (none collected yet, or a later pass reused its readback slot). */
int dm_assign_goals(dm_grid* g, const double* robots_xy, int32_t n_robots, int64_t min_size,
                    double distance_weight, double min_distance, int64_t* out_index, double* out_xy);

/* ---- Path planning on the device-resident map.  The reference has none: its
 * robots move by the reactive IR / LiDAR policy of main.py:123-188, and its
 * report (§VI-2) names Nav2 as future work.  These calls take over what Nav2's
 * global costmap (inflation layer) and global planner would compute, from the
 * map this library already holds.  All of them are synchronous, ordered after
 * everything enqueued on the handle, and need a handle that covers the whole
 * map: a band handle (band_rows != height) or a dm_create_sharded handle
 * returns DM_ERR_INVALID_ARG.
 *
 * Definitions (integers only: every result is unique and bit-exact).
 *   Traversable cell, for inflate_cells = r in [0, 32]: state == 0 and no
 *     in-grid cell with state == 100 within dx*dx + dy*dy <= r*r.  Out-of-grid
 *     cells are not obstacles; unknown cells are not traversable; the source
 *     cells of a field are traversable whatever their state.
 *   Moves: 8-connected, orthogonal cost 5, diagonal cost 7; a diagonal move
 *     (x, y) -> (x+sx, y+sy) is legal only if (x+sx, y) and (x, y+sy) are both
 *     traversable (no corner cutting).
 *   Field: uint32 cost[height*width], the least total move cost from any
 *     source cell over traversable cells; sources have cost 0;
 *     DM_PLAN_UNREACHABLE marks cells that are not reached.  SATURATION: a
 *     cost above max_cost is never stored, such cells stay
 *     DM_PLAN_UNREACHABLE; max_cost == 0 (or any value above it) means
 *     0xFFFFFFEF, so a stored cost plus a move cost never wraps.
 *     metres = (double)cost * resolution / 5.0 (two rounded operations).
 *   Cell of a point: floor((x - origin_x) / resolution), likewise y (as the
 *     integration's endpoints).
 *   Snap, for snap_cells = s in [0, 16]: the reached in-grid cell within
 *     Chebyshev distance s of the target's cell that minimises (dx*dx + dy*dy,
 *     linear index); none, or a target out of the grid: cost
 *     DM_PLAN_UNREACHABLE and cell -1.
 *   Path: from the snapped cell back to cost 0; the predecessor of c is the
 *     first neighbour n, in the order (dy, dx) = (-1,-1), (-1,0), (-1,1),
 *     (0,-1), (0,1), (1,-1), (1,0), (1,1), that is reached, whose move n -> c
 *     is legal and with cost[n] + w(n, c) == cost[c].
 * The field lives on the device in the handle (allocated on first use,
 * DM_ERR_OOM if that fails; freed by dm_destroy) and is stamped with the map's
 * version: after any call that writes the map (dm_integrate*, dm_set_state,
 * dm_set_logodds, dm_reset, dm_load) dm_plan_get_field, dm_plan_query and
 * dm_plan_path return DM_ERR_STATE until dm_plan_field ran again. */

/* The traversability mask: out[height*width] = 1 / 0, row-major.  Replaces
 * the inflation layer of Nav2's global costmap (binary: lethal within the
 * inflation radius; the graded cost around it: dm_plan_field_cost below).
 * Does not touch the handle's field. */
int dm_plan_traversable(dm_grid* g, int32_t inflate_cells, uint8_t* out);
/* Compute the field from n_sources (1..256) points sources_xy[2i], [2i+1]
 * (metres; one outside the grid: DM_ERR_INVALID_ARG).  out_stats (may be
 * NULL) receives [4]: reached cells, traversable cells (sources not
 * counted), relaxation rounds, tile relaxations.  DM_ERR_INCOMPLETE if the
 * relaxation did not settle within its round bound (the handle then has no
 * field); the environment variable DM_PLAN_MAX_ROUNDS, read at dm_create,
 * overrides the bound (tests).  Replaces Nav2's global planner's expansion
 * (NavFn's potential field), from the robots instead of from the goal. */
int dm_plan_field(dm_grid* g, const double* sources_xy, int32_t n_sources, int32_t inflate_cells,
                  uint32_t max_cost, uint64_t* out_stats);
/* The field: out[height*width] row-major. */
int dm_plan_get_field(dm_grid* g, uint32_t* out);
/* Snap n targets (metres) to the field: out_cost[i], out_cell[i] (linear
 * index cy*width + cx, or -1). */
int dm_plan_query(dm_grid* g, const double* targets_xy, int64_t n, int32_t snap_cells,
                  uint32_t* out_cost, int64_t* out_cell);
/* The path to the target's snapped cell, source first, as linear indices
 * cy*width + cx; *n_out = its length.  An unreachable target is DM_OK with
 * *n_out = 0; cap too small is DM_ERR_CAPACITY with *n_out = the full length
 * (out_cells unspecified).  Replaces the path Nav2's planner server returns
 * for the goal published on /goal_pose. */
int dm_plan_path(dm_grid* g, double tx, double ty, int32_t snap_cells, int64_t* out_cells, int64_t cap,
                 int64_t* n_out);

/* ---- Clearance-aware planning: the graded half of Nav2's inflation layer.
 * dm_plan_field's paths are shortest, so they pass every inside corner at
 * exactly the inflation radius; a cost that grows towards obstacles keeps them
 * in the middle of a corridor.  Same conventions as the block above.
 *   Clearance, for clear_cells = R in [1, 32]: d2[c] = the least dx*dx + dy*dy
 *     over in-grid cells with state == 100 within dx*dx + dy*dy <= R*R, and
 *     R*R + 1 ("far") if there is none; 0 on an occupied cell; defined for
 *     every cell whatever its state.  Out-of-grid cells are not obstacles.
 *   Penalty table: the caller's uint8 pen[R*R + 2], indexed by d2 (the last
 *     entry is "far"); any table is valid.  The library computes no exp (as
 *     with the matcher's kern); dm/plan.py's inflation_table is Nav2's curve.
 *   Weighted move: entering cell c by a legal move costs b * (1 + pen[d2[c]]),
 *     b = 5 orthogonal, 7 diagonal, so at most 1792.  Legality is as above, for
 *     inflate_cells.
 *   Weighted field: as the field above with that move cost; max_cost == 0 (or
 *     any value above it) means DM_PLAN_COST_MAX, so a stored cost plus a move
 *     never wraps and never equals DM_PLAN_UNREACHABLE.  With pen all zero it
 *     is dm_plan_field's field bit for bit wherever both stay below their caps.
 *   Path on a weighted field: the rule above with w = b * (1 + pen[d2[c]]). */
#define DM_PLAN_COST_MAX 0xFFFFF7FFu

/* The clearance: out[height*width] row-major.  A diagnostic and test entry,
 * like dm_plan_traversable.  Does not touch the handle's field. */
int dm_plan_clearance(dm_grid* g, int32_t clear_cells, uint16_t* out);
/* dm_plan_field with the weighted move: arguments, out_stats and errors as
 * there (DM_ERR_INCOMPLETE and DM_PLAN_MAX_ROUNDS included); clear_cells out
 * of range or pen NULL: DM_ERR_INVALID_ARG; any error leaves the handle with
 * no field.  The handle then holds a weighted field, and the penalty byte of
 * every cell beside it on the device (allocated on the first such call):
 * dm_plan_get_field and dm_plan_query read it like any field, dm_plan_path
 * walks it by the weighted rule.  A later dm_plan_field, dm_assign_goals_path,
 * _gain or _coord leaves an unweighted field as before. */
int dm_plan_field_cost(dm_grid* g, const double* sources_xy, int32_t n_sources, int32_t inflate_cells,
                       int32_t clear_cells, const uint8_t* pen, uint32_t max_cost, uint64_t* out_stats);
/* dm_assign_goals scored by path length: over the same clusters, with the
 * same availability rule, errors, greedy order, ties and n_robots <= 256
 * limit.  For robot r the field is computed from r's cell alone (a robot
 * outside the grid: DM_ERR_INVALID_ARG), every centroid is snapped to it, and
 *   dist = (double)cost * resolution / 5.0
 *   util = size / (1 + distance_weight * dist)
 * over clusters with size >= min_size that are reached and have
 * dist >= min_distance.  out_index[r] as dm_assign_goals; out_cell[r] = the
 * snapped cell (-1: none) and out_xy[2r], [2r+1] = its centre,
 * origin + (c + 0.5) * resolution (NaN if none): a goal that can be driven
 * to, where a concave frontier's centroid may lie in unknown or occupied
 * space.  The handle's field is left as the last robot's.  Replaces the
 * reactive policy of main.py:123-188 like dm_assign_goals, with the distance
 * Nav2's planner would report. */
int dm_assign_goals_path(dm_grid* g, const double* robots_xy, int32_t n_robots, int64_t min_size,
                         double distance_weight, double min_distance, int32_t inflate_cells,
                         uint32_t max_cost, int32_t snap_cells, int64_t* out_index, double* out_xy,
                         int64_t* out_cell);

/* ---- Information gain of a viewpoint on the device-resident map.  The
 * reference has no next-best-view step: its robots move by the reactive IR /
 * LiDAR policy of main.py:123-188.  dm_assign_goals and dm_assign_goals_path
 * score a frontier cluster by its size, a proxy for what exploration is after;
 * these calls count what the sensor would see from the goal: the unknown cells
 * its rays reach on the current map before an obstacle.  Both are synchronous,
 * ordered after everything enqueued on the handle, read the map as it is at
 * the call (the states dm_get_state returns: 100, 0, anything else unknown),
 * never write it and do not change the map version (a dm_plan_field result
 * and the matcher's cached field stay valid; dm_assign_goals_gain itself
 * leaves its last robot's field).  They need a handle that covers the whole
 * map: a band handle (band_rows != height) or a dm_create_sharded handle
 * returns DM_ERR_INVALID_ARG.
 *
 * Definition (integers only: every result is unique and bit-exact).
 *   Visible-unknown count of a view cell (vx, vy), for radius_cells = R in
 *     [1, 511]:
 *   Rays: one to each of the 8R offsets (ex, ey) with max(|ex|, |ey|) == R.
 *   Line: each ray is the integration's line from (vx, vy)
 *     to (vx + ex, vy + ey): the major axis is x iff |ex| >= |ey|, n = R,
 *     adb = min(|ex|, |ey|), ia / ib the signs of the major / minor offset;
 *     step k (0..R) is at major = k * ia,
 *     minor = ib * floor((2 * k * adb + n) / (2 * n)).
 *   Walk: a ray is walked from k = 0 and ends before the first cell that is
 *     out of the grid, has dx*dx + dy*dy > R*R, or has state 100.
 *   Marking: every cell it visits before that with an unknown state is
 *     marked.  Rays pass through unknown and free cells alike; k = 0 is the
 *     view cell itself, so a view on an occupied cell marks nothing.
 *   gain = the number of distinct marked cells, as uint32.
 * The limit 511 is the largest radius whose bitmap of marked cells, 1023 rows
 * of 32 words, fits the 160 KiB of local memory of one compute unit. */

/* The gains of n view points (n in [0, 2^20]; views_xy[2i], [2i+1] metres).
 * The cell of a point is the planner's, floor((x - origin_x) / resolution),
 * likewise y; out_cell[i] = its linear index cy*width + cx.  A view outside
 * the grid, or a non-finite one, gets out_cell[i] = -1 and out_gain[i] = 0.
 * radius_cells or n out of range, or a NULL pointer with n > 0:
 * DM_ERR_INVALID_ARG.  Replaces nothing of the reference; it is the
 * next-best-view score of an exploration stack that takes over from the
 * reactive policy of main.py:123-188. */
int dm_gain_views(dm_grid* g, const double* views_xy, int64_t n, int32_t radius_cells, uint32_t* out_gain,
                  int64_t* out_cell);
/* dm_assign_goals_path with the information gain as the numerator of the
 * utility.  The same: the clusters, the availability rule and the errors, the
 * per-robot field and the snap of every centroid to it,
 * dist = (double)cost * resolution / 5.0, the greedy robot order, ties to the
 * smaller label, n_robots <= 256, out_index / out_xy / out_cell, and the
 * handle's field is left as the last robot's.  What changes: for robot r and
 * cluster c, gain(r, c) is the visible-unknown count of c's snapped cell under
 * r's field; a cluster is eligible iff size >= min_size, it is reached,
 * dist >= min_distance and gain >= min_gain (min_gain >= 0, a negative value:
 * DM_ERR_INVALID_ARG); and
 *   util = (double)gain / (1 + distance_weight * dist)
 * as separately rounded doubles.  A gain of 0 gives util 0, which reads as
 * "not eligible": a cluster with nothing to see is never a goal, even with
 * min_gain = 0.  out_gain[r] = the chosen cluster's gain (0: none).  A
 * cluster taken by an earlier robot does not discount what the others would
 * see: that is dm_assign_goals_coord, below.  Replaces the reactive
 * policy of main.py:123-188 like dm_assign_goals, with the next-best-view
 * score in place of the frontier's size. */
int dm_assign_goals_gain(dm_grid* g, const double* robots_xy, int32_t n_robots, int64_t min_size,
                         int64_t min_gain, double distance_weight, double min_distance, int32_t inflate_cells,
                         uint32_t max_cost, int32_t snap_cells, int32_t radius_cells, int64_t* out_index,
                         double* out_xy, int64_t* out_cell, uint32_t* out_gain);

/* ---- Overlap-aware information gain.  Two frontier clusters that open onto
 * the same unmapped hall both score the whole hall under dm_assign_goals_gain,
 * and two robots are sent to look at the same cells.  These calls discount a
 * view by what the views before it already see: the greedy coordinated
 * assignment of multi-robot exploration.  The reference has no counterpart
 * (its robots do not share goals; main.py:123-188).  All three are
 * synchronous, ordered after everything enqueued on the handle, read the map
 * and never write it, and do not change the map version (a dm_plan_field
 * result and the matcher's cached field stay valid; dm_assign_goals_coord
 * leaves its last robot's field, as dm_assign_goals_gain does).  They need a
 * handle that covers the whole map: a band handle or a dm_create_sharded
 * handle returns DM_ERR_INVALID_ARG.
 *
 * Definitions (integers only: every result is unique and bit-exact).
 *   Visible set V(cell, R): the set of marked cells of the visible-unknown
 *     count above; |V| is dm_gain_views' gain.
 *   Claimed set C: a set of map cells, kept in the handle.
 *   Marginal gain of a view: |V(cell, R) \ C|.
 *   Commit of a view: C := C u V(cell, R).
 * C is allocated by the first of the calls (height * ceil(width / 32) words;
 * DM_ERR_OOM if that fails) and freed by dm_destroy. */

/* The marginal gains of n views taken in order (n in [0, 1024]; radius_cells
 * in [1, 511]).  The cell of a view is dm_gain_views'; a view outside the
 * grid, or a non-finite one, gets out_cell[i] = -1 and out_marginal[i] = 0 and
 * commits nothing.  C starts empty; for i = 0 .. n-1 in order
 * out_marginal[i] = |V_i \ C|, then V_i is committed.  The sum of out_marginal
 * is the number of distinct unknown cells the n views see together.  n or
 * radius_cells out of range, or a NULL pointer with n > 0: DM_ERR_INVALID_ARG. */
int dm_gain_views_joint(dm_grid* g, const double* views_xy, int64_t n, int32_t radius_cells,
                        uint32_t* out_marginal, int64_t* out_cell);
/* dm_assign_goals_gain with the marginal gain as the numerator.  The same:
 * the clusters of the last collected result, the errors, the per-robot field
 * and snap, dist, the eligibility tests ("gain 0 is never a goal" included),
 * the greedy robot order, ties to the smaller label, the taken-cluster rule,
 * n_robots <= 256, and the field left behind is the last robot's.  What
 * changes: C starts as the union of V over the n_held held views (n_held in
 * [0, 1024]; held_xy may be NULL when it is 0; a held view outside the grid or
 * non-finite adds nothing) - the goals that teammates who are not replanning
 * in this call already hold; a caller may also pass robot poses.  For robot r,
 *   gain(r, c) = |V(snapped cell of c under r's field, R) \ C|
 * with C as it stands when r chooses; when r gets a goal its view is committed
 * before robot r + 1 is scored, and out_gain[r] is that marginal gain.  With
 * n_held = 0, robot 0's result equals dm_assign_goals_gain's for the same
 * inputs, bit for bit.  n_held out of range, or held_xy NULL with n_held > 0:
 * DM_ERR_INVALID_ARG. */
int dm_assign_goals_coord(dm_grid* g, const double* robots_xy, int32_t n_robots, const double* held_xy,
                          int32_t n_held, int64_t min_size, int64_t min_gain, double distance_weight,
                          double min_distance, int32_t inflate_cells, uint32_t max_cost, int32_t snap_cells,
                          int32_t radius_cells, int64_t* out_index, double* out_xy, int64_t* out_cell,
                          uint32_t* out_gain);
/* The claimed set left by the last dm_gain_views_joint or
 * dm_assign_goals_coord on the handle: out[height * width] = 1 / 0, row-major.
 * A diagnostic and test entry, like dm_plan_traversable and dm_match_field.
 * DM_ERR_STATE if neither call has run yet (or the last one failed). */
int dm_gain_claimed(dm_grid* g, uint8_t* out);

/* ---- Team planning: one distance field per robot, relaxed together, and a
 * goal assignment that does not depend on the order of the robots.  The
 * reference's robots explore independently (main.py:123-188); this is what a
 * multi-robot task allocator starts from, the robot x target path-cost matrix.
 * Conventions as the path planning block: synchronous, ordered after
 * everything enqueued on the handle, whole-map handles only (a band or a
 * dm_create_sharded handle: DM_ERR_INVALID_ARG), integers only, the map is
 * read and never written and its version does not change.
 *   Team field k of n_robots in [1, DM_PLAN_TEAM_MAX]: bit for bit what
 *     dm_plan_field(&robots_xy[2k], 1, inflate_cells, max_cost) leaves on the
 *     same map: the same moves, legality, max_cost saturation and
 *     DM_PLAN_UNREACHABLE.  Robot k's own cell is traversable in field k
 *     whatever its state, and in no other field: a robot on an unknown or
 *     inflated cell opens no passage for its teammates.  Two robots may share
 *     a cell.  A robot outside the grid: DM_ERR_INVALID_ARG.
 *   The fields live in the handle beside dm_plan_field's, n_robots * height *
 *     width * 4 bytes, allocated on first use and grown when a later call
 *     needs more (DM_ERR_OOM if that fails; freed by dm_destroy), with the
 *     team's own copy of the traversable bit rows.  The two results do not
 *     disturb each other: dm_plan_team leaves what dm_plan_get_field,
 *     dm_plan_query and dm_plan_path return, dm_plan_field (with any inflation)
 *     leaves what the team readers return.  The fields are stamped with the
 *     map's version: after any call that writes the map the three readers
 *     return DM_ERR_STATE until dm_plan_team (or dm_assign_goals_team) ran again.
 * Out of scope: a penalty-weighted team field (dm_plan_field_cost's move), a
 * coordinated (marginal-gain, dm_assign_goals_coord's) team assignment, and
 * sharded handles. */
#define DM_PLAN_TEAM_MAX 64

/* Compute the n_robots fields.  out_stats (may be NULL) receives
 * [3 + n_robots]: [0] traversable cells (sources not counted), [1] rounds,
 * [2] (field, tile) relaxations, [3 + k] reached cells of field k.  The
 * rounds are the maximum over the fields, not their sum; the round bound is
 * dm_plan_field's with one source, DM_PLAN_MAX_ROUNDS applies, and
 * DM_ERR_INCOMPLETE leaves the handle with no team fields.  n_robots * tiles
 * >= 2^31: DM_ERR_CAPACITY. */
int dm_plan_team(dm_grid* g, const double* robots_xy, int32_t n_robots, int32_t inflate_cells,
                 uint32_t max_cost, uint64_t* out_stats /* [3 + n_robots], may be NULL */);
/* Field `robot`: out[height*width] row-major.  robot outside [0, n_robots) of
 * the last dm_plan_team: DM_ERR_INVALID_ARG (here and in dm_plan_team_path). */
int dm_plan_team_get_field(dm_grid* g, int32_t robot, uint32_t* out /* [height*width] */);
/* The robot x target matrix: dm_plan_query's snap of target i under field r
 * in out_cost[r * n + i], out_cell[r * n + i]. */
int dm_plan_team_query(dm_grid* g, const double* targets_xy, int64_t n, int32_t snap_cells,
                       uint32_t* out_cost /* [n_robots][n] */, int64_t* out_cell /* [n_robots][n] */);
/* dm_plan_path on field `robot`: the same snap, predecessor rule, outputs
 * and errors. */
int dm_plan_team_path(dm_grid* g, int32_t robot, double tx, double ty, int32_t snap_cells,
                      int64_t* out_cells, int64_t cap, int64_t* n_out);
/* Global-greedy goals over the clusters of the last collected result, with
 * dm_assign_goals' errors; n_robots in [0, DM_PLAN_TEAM_MAX].  Row r is robot
 * r's team field and every centroid is snapped to it.  With radius_cells == 0
 * dist, the eligibility tests and util are dm_assign_goals_path's (score by
 * size; min_gain is not read, out_gain may be NULL and is not written); with
 * radius_cells in [1, 511] they are dm_assign_goals_gain's: gain(r, c) is the
 * visible-unknown count of c's snapped cell under r's field, gain >= min_gain,
 * and a gain of 0 is never a goal.  Then, repeatedly: among the eligible pairs
 * (r, c) with r unassigned and c untaken the one with the greatest util is
 * assigned, ties to the smaller label, then the smaller r; until no pair is
 * left.  So robot 0 does not take the frontier next to robot 1 only because
 * it chooses first.  Outputs as dm_assign_goals_gain.  With n_robots == 1 the
 * result is dm_assign_goals_path's / dm_assign_goals_gain's bit for bit.  The
 * call leaves the team fields of these robots in the handle (dm_plan_team_path
 * can follow it) and does not touch dm_plan_field's field. */
int dm_assign_goals_team(dm_grid* g, const double* robots_xy, int32_t n_robots, int64_t min_size,
                         int64_t min_gain, double distance_weight, double min_distance,
                         int32_t inflate_cells, uint32_t max_cost, int32_t snap_cells,
                         int32_t radius_cells /* 0: score by size */, int64_t* out_index,
                         double* out_xy, int64_t* out_cell, uint32_t* out_gain /* may be NULL when radius_cells == 0 */);

/* ---- Correlative scan matching against the device-resident map.  In the
 * reference the pose of a scan comes from slam_toolbox's correlative scan
 * matcher (slam_config.yaml:35 use_scan_matching; :50-53 the correlation
 * search space, :64-66 the angle search), which corrects odometry and
 * publishes the correction as map -> odom.  slam_toolbox is not vendored, so
 * the definitions below are this build's SPEC (parity unpinned).  Everything
 * is integer arithmetic or separately rounded doubles (no FMA): every result
 * is unique and bit-exact.  Both calls are synchronous, ordered after
 * everything enqueued on the handle, read the map as it is at the call, never
 * write it and do not change the map version (a dm_plan_field result stays
 * valid).  They need a handle that covers the whole map: a band handle
 * (band_rows != height) or a dm_create_sharded handle returns
 * DM_ERR_INVALID_ARG.
 *
 *   Response field, for smear_cells = r in [0, 16] and a caller-supplied table
 *     kern[r*r + 1] of uint8: V[c] = max over in-grid cells o with
 *     state[o] == 100 and d2 = dx*dx + dy*dy <= r*r of kern[d2]; 0 if there is
 *     none.  Out-of-grid cells are never occupied.  The library computes no
 *     exp; a Gaussian smear of deviation sigma is kern[d2] =
 *     floor(255 * exp(-0.5 * d2 * resolution^2 / sigma^2) + 0.5) (dm/match.py
 *     kernel_table).  The max holds for any table, monotone or not.
 *   Fine coordinates, for sub in [1, 16]: step = resolution / (double)sub.
 *     Candidate angle k has yaw + yaw_offsets[k] (one double add); its cos /
 *     sin, and those of the beam angles, come from the host C library as in
 *     dm_integrate.  A beam is used iff range_min <= r <= range_max (NaN and
 *     beams past range_max are not: the matcher scores hits only).  Its
 *     endpoint ex, ey is that of dm_integrate, product by
 *     product; qx = floor((ex - origin_x) / step), likewise qy.  A beam of a
 *     non-finite pose, or with |qx| or |qy| >= 2^30, is not used.
 *     n_used[s] = the used beams of candidate k0.
 *   Score, for translation indices i, j in [-half, half], half in [0, 32],
 *     stride in [1, 16]: cell = (floordiv(qx + i*stride, sub),
 *     floordiv(qy + j*stride, sub)), floor division for negative values too;
 *     score[s][k][j][i] = sum over used beams of V[cell] as uint32, a cell
 *     out of the grid adding 0.
 *   Best candidate: the maximal score, ties to the lexicographically least
 *     (i*i + j*j, |k - k0|, k, j, i); k0 in [0, A) is the caller's "no
 *     rotation" candidate, so an empty or unknown map gives (k0, 0, 0), score 0.
 *   Output pose: x + (double)(i*stride) * step, y + (double)(j*stride) * step,
 *     yaw + yaw_offsets[k].
 *   Limits: A in [1, 64]; S, N as for dm_integrate; anything outside the
 *     limits above is DM_ERR_INVALID_ARG.
 * The field lives on the device in the handle (allocated on first use,
 * DM_ERR_OOM if that or the per-call scratch cannot be allocated; freed by
 * dm_destroy).  It is kept per (map version, smear_cells, kern): a second
 * call on an unchanged map with the same table rebuilds nothing. */

/* The response field: out[height*width] row-major.  Diagnostic and test entry
 * (like dm_plan_traversable).  Replaces the smeared correlation grid of
 * slam_toolbox's correlative matcher (slam_config.yaml:50-53:
 * correlation_search_space_smear_deviation). */
int dm_match_field(dm_grid* g, int32_t smear_cells, const uint8_t* kern, uint8_t* out);
/* Score every candidate pose of S scans and pick the best of each.  poses
 * [S][3], ranges [S][N], angle_min, angle_increment as dm_integrate;
 * yaw_offsets[A].  out_best: int32[S][3] = (k, i, j); out_score: uint32[S];
 * out_n_used: int32[S]; out_pose: double[S][3]; out_volume (may be NULL):
 * uint32[S][A][2*half+1][2*half+1], index order k, j, i.  Only the tiles the
 * search windows reach are built into the field; only the S results cross to
 * the host unless out_volume is asked for.  Replaces slam_toolbox's
 * correlative scan matcher (one search stage of it; slam_config.yaml:50-53
 * correlation_search_space_*, :64-66 fine_search_angle_offset,
 * coarse_search_angle_offset, coarse_angle_resolution); its variance penalties
 * and covariance are not computed, out_volume holds what they need. */
int dm_match_scans(dm_grid* g, int32_t S, const double* poses, int32_t N, const float* ranges, float angle_min,
                   float angle_increment, int32_t A, const double* yaw_offsets, int32_t k0, int32_t sub,
                   int32_t half, int32_t stride, int32_t smear_cells, const uint8_t* kern, int32_t* out_best,
                   uint32_t* out_score, int32_t* out_n_used, double* out_pose, uint32_t* out_volume);

/* Whole-window relocalisation: the best candidate of dm_match_scans'
 * definition at sub = 1, stride = 1 over a window far larger than its volume
 * could hold, found exactly by bounds from a max-pooled response field
 * (DESIGN.md §8.5).  It takes over slam_toolbox's localisation start on a
 * saved map (slam_config.yaml:20) and its wide loop search (:56-58).
 *
 *   The response field V, the used beams, n_used and the endpoint cells
 *     qx = floor((ex - origin_x) / resolution), qy likewise, are those of
 *     dm_match_scans at sub = 1; the candidate yaw is yaw + yaw_offsets[k].
 *   score[s][k][j][i] = sum over used beams of V[qx + i, qy + j], cells out of
 *     the grid adding 0, for i in [-half_x, half_x], j in [-half_y, half_y].
 *   Best: the maximal score over all A * (2 half_x + 1) * (2 half_y + 1)
 *     candidates, ties to the lexicographically least
 *     (i*i + j*j, |k - k0|, k, j, i); an empty or unknown map gives
 *     (k0, 0, 0) with score 0.
 *   Output pose: x + (double)i * resolution, y + (double)j * resolution,
 *     yaw + yaw_offsets[k].
 *   Limits: half_x, half_y in [0, 4096]; A in [1, 1024]; k0 in [0, A); block in
 *     {4, 8, 16, 32}; exhaustive in {0, 1}; S, N, smear_cells, kern as for
 *     dm_match_scans.  Anything else is DM_ERR_INVALID_ARG, and so is a band
 *     handle or a dm_create_sharded handle.  More than 2^26 blocks per scan,
 *     A * ceil((2 half_x + 1) / block) * ceil((2 half_y + 1) / block), is
 *     DM_ERR_CAPACITY (take a larger block); a failed allocation DM_ERR_OOM.
 * The result is defined by the exhaustive search alone: block and exhaustive
 * change how it is found and what out_stats says, never a result bit.  With
 * half_x == half_y <= 32 and A <= 64 the four outputs equal
 * dm_match_scans(sub = 1, stride = 1, half).
 *   exhaustive = 0: M_B[c] = max of V over [cx, cx + block) x [cy, cy + block)
 *     bounds every score of a block of block x block translations of one yaw
 *     by sum over used beams of M_B[qx + i0, qy + j0]; blocks are scored
 *     exactly in rounds, the highest bounds first, until no unscored block's
 *     bound reaches the best exact score (ties included: exact).
 *   exhaustive = 1: every block is scored; the device's own brute force.
 * out_best: int32[S][3] = (k, i, j); out_score: uint32[S]; out_n_used:
 * int32[S]; out_pose: double[S][3]; out_stats (may be NULL): uint64[S][4] =
 * blocks in the search, blocks whose bound was computed (0 when exhaustive),
 * blocks scored exactly, rounds (a scan whose window reaches no cell of the
 * map bounds and scores nothing: blocks, 0, 0, 0).  Synchronous, ordered after everything
 * enqueued on the handle; reads the map and never writes it, the map version
 * is unchanged.  The scans of one call are processed one after another.  The
 * pooled field is kept in the handle per (map version, smear_cells, kern,
 * block), like the field.  DM_MATCH_GLOBAL_BATCH (read at dm_create) sets the
 * most blocks one round scores (default 4096); it changes no result. */
int dm_match_global(dm_grid* g, int32_t S, const double* poses, int32_t N, const float* ranges, float angle_min,
                    float angle_increment, int32_t A, const double* yaw_offsets, int32_t k0, int32_t half_x,
                    int32_t half_y, int32_t block, int32_t exhaustive, int32_t smear_cells, const uint8_t* kern,
                    int32_t* out_best /*[S][3] k,i,j*/, uint32_t* out_score, int32_t* out_n_used,
                    double* out_pose /*[S][3]*/, uint64_t* out_stats /*[S][4], may be NULL*/);

/* Which parts of the matcher's kept fields are valid for the map as it is now.
 * field_tiles (may be NULL; else cap >= TX*TY, DM_ERR_CAPACITY otherwise):
 * out[ty*TX + tx] = 1 iff the response field holds that tile for the current
 * table and map version.  *n_field = their count, *n_pool = the pooled field's
 * built 64x64 tiles (0 when it is stale or absent).  No field yet, or the map
 * written since: all zero, DM_OK.  Host state only: no GPU work, no wait.
 * Band and sharded handles: DM_ERR_INVALID_ARG.  A diagnostic, like
 * dm_frontier_cache_stats: dm_match_scans and dm_match_global build the tiles
 * their windows reach and nothing else, and this is how a test sees that. */
int dm_match_built(dm_grid* g, uint8_t* field_tiles, int64_t cap, int64_t* n_field, int64_t* n_pool);

/* ---- map fusion: merge a peer's occupancy map under a rigid transform ----
 *
 * WHAT THIS REPLACES
 *   Nothing in the reference: its robots share no map (ThymioBrain.map_cb,
 *   server/thymio_project/thymio_project/main.py:80-81, keeps the one /map it
 *   is sent).  It is the merge step of a multi-robot ROS stack
 *   (multirobot_map_merge): a peer's map is placed in our frame by a rigid
 *   transform and folded into ours, here on the device-resident map instead of
 *   dm_get_logodds -> host loop -> dm_set_logodds.
 *
 * Geometry of the source map, in ITS frame. */
typedef struct dm_fuse_source {
  int64_t width, height;     /* cells; each in [1, 32768] */
  double resolution;         /* metres per cell, finite, > 0 (may differ from the destination's) */
  double origin_x, origin_y; /* world coords of the lower-left corner of cell (0,0), finite */
} dm_fuse_source;

#define DM_FUSE_ADD 0  /* independent evidence: log-odds add */
#define DM_FUSE_FILL 1 /* only cells the destination does not know yet; idempotent */

/* (tx, ty, yaw) maps source-frame points into the destination frame:
 * p_dst = R(yaw) p_src + t.  c = cos(yaw) and s = sin(yaw) are evaluated on
 * the host with the C library, as in dm_integrate.  Everything below is
 * integers and separately rounded IEEE doubles / floats (no FMA), so every
 * result is unique and bit-exact (dm/fuse.py restates it in NumPy).
 *   For every destination cell (cx, cy) the handle owns, in global cell
 *   coordinates (a band handle: its rows only), with the destination's params:
 *     wx = origin_x + ((double)cx + 0.5) * resolution, wy likewise from cy;
 *     dx = wx - tx, dy = wy - ty;
 *     sx = c*dx + s*dy, sy = c*dy - s*dx   (two products, one sum / difference,
 *                                           each rounded);
 *     qx = floor((sx - src.origin_x) / src.resolution), qy likewise.
 *   The cell is COVERED iff sx, sy are finite and 0 <= qx < src.width,
 *   0 <= qy < src.height (compared as doubles): nearest-neighbour sampling of
 *   the source at the destination cell's centre.
 *   l = the source value at (qx, qy).  dm_fuse_logodds / dm_fuse_grid: the float
 *   there, a non-finite one reads as 0.  dm_fuse_state: dm_set_state's mapping
 *   with the DESTINATION's parameters: 100 -> l_occ, 0 -> l_free, else 0.
 *   A covered cell CONTRIBUTES iff l != 0 and, in DM_FUSE_FILL, the
 *   destination's L == 0.
 *   A contributing cell gets L' = clamp(L + l) (DM_FUSE_ADD: one float add) or
 *   L' = clamp(l) (DM_FUSE_FILL), clamp = SPEC a6's to the destination's
 *   [l_min, l_max] (if (L' < l_min) L' = l_min; if (L' > l_max) L' = l_max,
 *   zero bounds read as +0), then state = SPEC a7 of L'.  Every other cell
 *   keeps its L and state bit for bit.
 * out_stats (may be NULL): uint64[3] = covered cells, contributing cells,
 * cells whose state byte changed.
 * Synchronous, ordered after everything enqueued on the handle (all its
 * streams are joined, as by dm_set_logodds).  On success the map version is
 * bumped exactly as by dm_set_logodds: the dm_plan_* readers return
 * DM_ERR_STATE until dm_plan_field runs again, the matcher's field, the pooled
 * field and the claimed set are rebuilt on next use; the tile summaries the
 * frontier pass reads are rebuilt.  Whole-map handles, band handles (a band
 * fuses its own rows of the same global picture) and dm_create_sharded handles
 * (every band; stats summed) all work.
 * Errors: DM_ERR_INVALID_ARG for NULL pointers, geometry outside the limits
 * above, non-finite tx, ty or yaw, an unknown mode; DM_ERR_OOM if the staging
 * buffer of the source cannot be allocated; the map and its version are then
 * untouched.  A source that covers no destination cell is DM_OK with stats
 * 0, 0, 0. */
int dm_fuse_logodds(dm_grid* g, const dm_fuse_source* src, const float* L_src, double tx, double ty, double yaw,
                    int32_t mode, uint64_t* out_stats /*[3], may be NULL*/);
int dm_fuse_state(dm_grid* g, const dm_fuse_source* src, const int8_t* state_src, double tx, double ty, double yaw,
                  int32_t mode, uint64_t* out_stats /*[3], may be NULL*/);
/* The same from another handle's log-odds, read on the device with no host
 * round trip.  src_grid must be a whole-map dm_create handle (no band, not
 * sharded) on the same HIP device as g (a sharded g: as all its bands) and not
 * g itself; anything else is DM_ERR_INVALID_ARG.  Its stream is synchronised
 * first; the source geometry comes from its params. */
int dm_fuse_grid(dm_grid* g, dm_grid* src_grid, double tx, double ty, double yaw, int32_t mode,
                 uint64_t* out_stats /*[3], may be NULL*/);

/* Measured uncontended atomic throughput of HIP device `device` (the
 * north star's "atomic throughput against MI355X peak": no vendor figure
 * exists for integer atomics, so the peak is measured in-harness,
 * csrc/dm_probe.hip).  out[0] = LDS ds_add_u32 per second (every lane its own
 * bank: the form k_tile_accum's per-cell counts take), out[1] = global
 * no-return atomicAdd u32 per second (256 contiguous bytes per wave
 * instruction, rows over a 256 MiB buffer: the heavy tiles' slab adds).
 * Runs a few milliseconds of probe kernels on a private stream. */
int dm_atomic_peak(int device, double* out, int32_t cap, int32_t* n_out);

const char* dm_last_error(void);
const char* dm_version(void);

#ifdef __cplusplus
}
#endif
#endif /* DM_H */
