// a-loam_amd/csrc/capi_mapping.hip — host side of the scan-to-map refinement: enable / step, the map pools and their growth, map injection
// and the map getters.
#include <algorithm>
#include <cstring>

#include "capi_internal.hpp"

// ---- stage 3: scan-to-map refinement --------------------------------------------------------------------------------
namespace aloam {
MapArgs map_args(aloam_ctx* c) {
  MapArgs a{};
  a.B = c->B; a.cap = c->cap; a.R = c->R;
  a.meta = c->d_meta.get(); a.odom = c->d_state.get(); a.seq = c->d_mapseq.get();
  a.line_res = c->map_line_res; a.plane_res = c->map_plane_res;
  // after aloam_odometry_step's swap the sweep just processed is the "last" one: exactly what the odometry node publishes
  // as /laser_cloud_corner_last, /laser_cloud_surf_last and /velodyne_cloud_3 (reference src/laserOdometry.cpp:570-591)
  for (int k = 0; k < 2; ++k) { a.less_sharp[k] = c->d_less_sharp[k].get(); a.less_flat[k] = c->d_less_flat[k].get(); }
  a.full = c->d_cloud.get();
  if (!c->dense_valid) { a.slabs = c->d_slabs.get(); a.slab = c->slab; a.ringstart = c->d_ringstart.get(); }   // the sweep just registered lives in its ring slabs; the dense copy is made only for who asks
  a.registered = c->d_registered.get();
  a.cubes = c->d_cubes.get(); a.pool_cap = c->map.points; a.tab = c->d_maptab.get();
  for (int k = 0; k < 2; ++k) {
    a.pool[k] = c->map.pool[k].get(); a.stack[k] = c->d_stack[k].get(); a.stack_world[k] = c->d_stack_world[k].get(); a.stack_cube[k] = c->d_stack_cube[k].get();
    a.grid_sorted[k] = c->map.grid_sorted[k].get(); a.grid_start[k] = c->map.grid_start[k].get();
  }
  a.grid_H = c->map.H; a.grid_sig = c->d_grid_sig.get(); a.live = c->d_map_live.get(); a.report_dev = c->d_map_report.get(); a.report_host = c->d_map_report_host;
  a.addcnt = c->d_addcnt.get(); a.cursor = c->d_cursor.get(); a.compact_flag = c->d_compact_flag.get();
  a.edges = c->d_medges.get(); a.norms = c->d_mnorms.get(); a.knn = c->d_knn.get();
  a.lm_max_iterations = c->cfg.lm_max_iterations;
  a.vox_counters = c->d_vox_counters.get();
  a.rec_tiles = c->d_rec_tiles.get(); a.rec_tiles_per_seq = c->rec_tiles_per_seq; a.rec_tiles_corner = c->rec_tiles_corner;
  return a;
}
VoxArgs vox_args(aloam_ctx* c, int n_segs, int levels) {
  VoxArgs v{};
  v.segs = c->d_segs.get(); v.n_segs = n_segs; v.tile_seg = c->map.tile_seg.get(); v.tile_heads = c->map.tile_heads.get(); v.tile_pref = c->map.tile_pref.get();
  v.counters = c->d_vox_counters.get(); v.keys[0] = c->map.keys[0].get(); v.keys[1] = c->map.keys[1].get(); v.tmp = c->map.voxtmp.get(); v.bbox = c->d_bbox.get();
  v.tile_cap = c->map.tile_cap; v.key_cap = c->map.key_cap; v.levels = levels; v.lists = c->d_vox_lists.get();
  return v;
}
}  // namespace aloam

// Everything whose size follows the pool: the two class pools (contents kept when growing), the bucketed copy of the submap, the scratch of
// the general voxel path (keys, staging = 2 pools per sequence, tile lists) and the bucket tables.  A fresh MapPool is allocated and filled,
// then committed with one move (which releases the old buffers), so a failure at any point leaves the context as it was.
static int map_alloc_pool(aloam_ctx* c, int pool_points) {
  const size_t B = c->B, cap = c->cap, R = c->R, T = kVoxTile, pool = pool_points, old_pool = c->map.points;
  MapPool n;
  n.points = pool_points;
  n.H = 4096;
  while (n.H < (int)(pool / 16) && n.H < kMapGridMaxH) n.H <<= 1;          // ~ submap size
  n.key_cap = (long long)(B * std::max(cap + R * kLessSharpPerRing, 2 * pool));
  n.tile_bound = (int)(B * (2 * pool / T + 2 * kMapValidMax));
  n.tile_cap = std::max(c->map_stack_tile_bound, n.tile_bound);
  while (((size_t)kVoxTile << n.cube_levels) < pool) ++n.cube_levels;     // a 50 m cube may hold the whole pool (unneeded levels cost a skipped tile loop each)
  bool ok = true;
  auto grab = [&](auto& p, size_t count) { if (ok && dalloc(p, count) != hipSuccess) { ok = false; (void)hipGetLastError(); } };
  for (int k = 0; k < 2; ++k) {
    grab(n.pool[k], B * pool);
    grab(n.grid_sorted[k], B * pool);
    grab(n.grid_start[k], B * ((size_t)n.H + 1));
    grab(n.keys[k], (size_t)n.key_cap);
  }
  grab(n.voxtmp, (size_t)n.key_cap);
  grab(n.tile_seg, (size_t)n.tile_cap); grab(n.tile_heads, (size_t)n.tile_cap); grab(n.tile_pref, (size_t)n.tile_cap + 1);
  if (!ok || prepare_map_grid(n.H)) {
    c->err = "map pool of " + std::to_string(pool_points) + " points per sequence and class: allocation failed";
    return ALOAM_E_HIP;
  }
  for (int k = 0; k < 2; ++k) {
    if (old_pool) HIP_TRY(c, hipMemcpy2DAsync(n.pool[k].get(), sizeof(float4) * pool, c->map.pool[k].get(), sizeof(float4) * old_pool, sizeof(float4) * old_pool, B, hipMemcpyDeviceToDevice, c->stream));
    else HIP_TRY(c, hipMemsetAsync(n.pool[k].get(), 0, sizeof(float4) * B * pool, c->stream));
    HIP_TRY(c, hipMemsetAsync(n.grid_start[k].get(), 0, sizeof(int) * B * ((size_t)n.H + 1), c->stream));
  }
  return on_map_pool_reallocated(c, std::move(n));
}

// The reference's cubes are std::vectors: a map grows as long as the sensor travels (src/laserMapping.cpp:737-783).  Here a (sequence,
// class) pool must hold the live points of its cubes plus what the step adds, and the steps are queued asynchronously, so the host sizes
// the pools AHEAD of the device from what k_map_report wrote after the last step that has finished: live points + (steps in flight + 1) x
// the most a step can add.  "The most": the stack sizes of the step are not known before its voxel filter has run, so it is the scan size
// (a stack is a filtered subset of one sweep) until a step has reported, then twice the largest stack any step has produced so far - a
// step that breaks that bound AND fills the pool drops points and raises ALOAM_E_CAPACITY like a full pool at the ceiling does.  When the
// bound exceeds the pool: wait for the device (the report is then exact), double the pool until it holds the bound, move the contents.
// Not called for a step whose active sequences are all frozen (aloam_set_map_frozen): such a step adds nothing to any map.
static int map_ensure_capacity(aloam_ctx* c) {
  if (c->map.points >= c->map_pool_limit) return ALOAM_OK;     // at the ceiling: nothing to decide (the device counts what does not fit)
  const int step_max = std::max(c->nin_max, c->inject_max);   // the last registration's active rows and what was injected since the last step
  const int hard[2] = {std::min(c->R * kLessSharpPerRing, step_max ? step_max : c->cap), std::min(c->cap, step_max ? step_max : c->cap)};
  auto bound = [&](long long lag) {
    const int done = c->h_map_report[0];
    long long worst = 0;
    for (int k = 0; k < 2; ++k) {
      const int inc = done > 0 ? std::min(hard[k], 2 * (int)c->h_map_report[3 + k] + 1024) : hard[k];
      worst = std::max(worst, (long long)c->h_map_report[1 + k] + (lag + 1) * inc);
    }
    return worst;
  };
  const long long lag = c->map_steps - c->h_map_report[0];
  if (bound(lag) <= c->map.points) return ALOAM_OK;
  HIP_TRY(c, hipStreamSynchronize(c->stream));               // now the report is that of the last queued step
  const long long need = bound(std::min<long long>(lag, 3));   // keep room for the run-ahead this caller has shown
  if (need <= c->map.points || c->map.points >= c->map_pool_limit) return ALOAM_OK;
  if (grow_map_pool(c, need, true)) c->map_pool_limit = c->map.points;   // out of device memory: this pool is the ceiling from now on
  return ALOAM_OK;
}

namespace aloam {

// The one place the map pool grows: doubled from its current size until it holds `want` points per sequence and class, moved
// (map_alloc_pool) and counted.  A doubled size above the pool limit is clamped to it, or, without `clamp`, refused with ALOAM_E_CAPACITY.
int grow_map_pool(aloam_ctx* c, long long want, bool clamp) {
  long long np = c->map.points;
  while (np < want) np *= 2;
  if (np > c->map_pool_limit) {
    if (!clamp) { c->err = "the injected map exceeds the pool limit"; return ALOAM_E_CAPACITY; }
    np = c->map_pool_limit;
  }
  if (const int rc = map_alloc_pool(c, (int)np)) return rc;
  c->map_growths += 1;
  return ALOAM_OK;
}

}  // namespace aloam

extern "C" {

int aloam_mapping_enable(aloam_ctx* c, float line_res, float plane_res, int pool_points) {
  DeviceScope device_scope(c);
  if (!c) return ALOAM_E_ARG;
  int rc = require_stage(c, ALOAM_STAGE_MAPPING);
  if (rc) return rc;
  if (c->map_on) { c->err = "mapping already enabled"; return ALOAM_E_STATE; }
  if (!(line_res > 0.f) || !(plane_res > 0.f) || pool_points < 4096 || pool_points > (1 << 26)) { c->err = "bad mapping parameters (4096 <= pool_points <= 2^26)"; return ALOAM_E_ARG; }
  const size_t B = c->B, cap = c->cap, R = c->R;
  c->map_line_res = line_res; c->map_plane_res = plane_res;
  c->map_levels = 0;                                       // incoming clouds: up to max_points
  while (((size_t)kVoxTile << c->map_levels) < cap) ++c->map_levels;
  const size_t T = kVoxTile;
  c->map_stack_tile_bound = (int)(B * ((cap + T - 1) / T + (R * kLessSharpPerRing + T - 1) / T));
  c->map_nsegs_max = (int)(B * 2 * kMapValidMax);
  const int pool0 = (pool_points + 1023) / 1024 * 1024;
  if (c->map_pool_limit < pool0) c->map_pool_limit = pool0;
  if ((rc = map_alloc_pool(c, pool0))) return rc;
  if ((rc = dmalloc(c, c->d_mapseq, B))) return rc;
  if ((rc = dmalloc(c, c->d_cubes, B * 2 * kMapCubes))) return rc;
  if ((rc = dmalloc(c, c->d_maptab, B * kTabInts))) return rc;
  if ((rc = dmalloc(c, c->d_grid_sig, B * 2))) return rc;               // zeros: no grid is valid
  if ((rc = dmalloc(c, c->d_addcnt, B * 2 * kMapCubes))) return rc;
  if ((rc = dmalloc(c, c->d_cursor, B * 2 * kMapCubes))) return rc;
  if ((rc = dmalloc(c, c->d_compact_flag, B * 2))) return rc;
  if ((rc = dmalloc(c, c->d_map_live, B * 2))) return rc;
  if ((rc = dmalloc(c, c->d_map_report, 4))) return rc;
  { int* p = nullptr; HIP_TRY(c, hipHostMalloc((void**)&p, sizeof(int) * 8, hipHostMallocMapped)); c->h_map_report.reset(p); }
  for (int k = 0; k < 8; ++k) c->h_map_report[k] = 0;
  HIP_TRY(c, hipHostGetDevicePointer((void**)&c->d_map_report_host, (void*)c->h_map_report.get(), 0));
  for (Event& e : c->map_step_done) if (!e.h) HIP_TRY(c, hipEventCreateWithFlags(&e.h, hipEventDisableTiming));   // (once: an enable retried after a failure)
  for (int k = 0; k < 2; ++k) {
    const size_t per = k == 0 ? R * kLessSharpPerRing : cap;
    if ((rc = dmalloc(c, c->d_stack[k], B * per))) return rc;
    if ((rc = dmalloc(c, c->d_stack_world[k], B * per))) return rc;
    if ((rc = dmalloc(c, c->d_stack_cube[k], B * per))) return rc;
  }
  c->rec_tiles_corner = (int)((R * kLessSharpPerRing + 255) / 256);
  c->rec_tiles_per_seq = c->rec_tiles_corner + (int)((cap + 255) / 256);
  if ((rc = dmalloc(c, c->d_rec_tiles, B * (size_t)c->rec_tiles_per_seq))) return rc;
  if ((rc = dmalloc(c, c->d_medges, B * R * kLessSharpPerRing))) return rc;
  if ((rc = dmalloc(c, c->d_mnorms, B * cap))) return rc;
  if ((rc = dmalloc(c, c->d_registered, B * cap))) return rc;
  if ((rc = dmalloc(c, c->d_knn, B * cap * 4))) return rc;
  if ((rc = dmalloc(c, c->d_segs, (size_t)c->map_nsegs_max))) return rc;
  if ((rc = dmalloc(c, c->d_vox_counters, 8))) return rc;
  if ((rc = dmalloc(c, c->d_vox_lists, 3 * (size_t)c->map_nsegs_max))) return rc;
  if (prepare_voxel_filter()) { c->err = "k_vox_lds: dynamic LDS size rejected"; return ALOAM_E_HIP; }
  if ((rc = dmalloc(c, c->d_bbox, (size_t)c->map_nsegs_max * 6))) return rc;
  std::vector<MapSeq> init(B);
  std::memset(init.data(), 0, sizeof(MapSeq) * B);
  for (size_t b = 0; b < B; ++b) {                       // reference src/laserMapping.cpp:72-74,109,115
    init[b].par[3] = 1.0; init[b].q_wmap_wodom[3] = 1.0;
    init[b].cen[0] = 10; init[b].cen[1] = 10; init[b].cen[2] = 5;
  }
  HIP_TRY(c, hipMemcpyAsync(c->d_mapseq.get(), init.data(), sizeof(MapSeq) * B, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  c->map_on = true;
  return ALOAM_OK;
}

int aloam_set_voxel_sum_order(aloam_ctx* c, int order) {
  DeviceScope device_scope(c);
  if (!c) return ALOAM_E_ARG;
  if (order != ALOAM_SUM_INPUT_ORDER && order != ALOAM_SUM_REFERENCE_ORDER) { c->err = "unknown summation order"; return ALOAM_E_ARG; }
  if (order == ALOAM_SUM_REFERENCE_ORDER && prepare_reference_order()) { c->err = "k_vox_reference_order: dynamic LDS size rejected"; return ALOAM_E_HIP; }
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  c->sum_order = order;
  return ALOAM_OK;
}

int aloam_mapping_set_pool_limit(aloam_ctx* c, int max_pool_points) {
  if (!c) return ALOAM_E_ARG;
  if (max_pool_points < 4096 || max_pool_points > (1 << 26)) { c->err = "bad pool limit (4096 .. 2^26 points)"; return ALOAM_E_ARG; }
  c->map_pool_limit = std::max((max_pool_points + 1023) / 1024 * 1024, c->map.points);
  return ALOAM_OK;
}

int aloam_get_map_pool_info(aloam_ctx* c, int out[4]) {
  DeviceScope device_scope(c);
  if (!c || !out) return ALOAM_E_ARG;
  if (!c->map_on) { c->err = "mapping not enabled"; return ALOAM_E_STATE; }
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  out[0] = c->map.points; out[1] = c->map_growths; out[2] = c->map_pool_limit;
  out[3] = std::max((int)c->h_map_report[1], (int)c->h_map_report[2]);
  return ALOAM_OK;
}

int aloam_mapping_step(aloam_ctx* c) {
  DeviceScope device_scope(c);
  if (!c) return ALOAM_E_ARG;
  if (!c->map_on) { c->err = "aloam_mapping_step before aloam_mapping_enable"; return ALOAM_E_STATE; }
  for (int b = 0; b < c->B; ++b)
    if (c->seq[b].needs_odom && takes_part(c, b)) {
      c->err = "sequence " + std::to_string(b) + " was loaded (aloam_load_sequences) and has not had its odometry step yet: it may not map";
      return ALOAM_E_STATE;
    }
  if (const int rc = atlas_step_check(c)) return rc;
  // Per sequence: kSeqActive = takes part, kSeqMapGrow = takes part and extends its map (not frozen).  The kernels get no mask at all when
  // every sequence grows: the launches of a lock-step batch are those of a context without aloam_set_active / aloam_set_map_frozen.
  StageMask m;
  if (const int rc = stage_mask(c, c->d_mask_map, [](const SeqHost& s) { return s.frozen ? 0 : (int)kSeqMapGrow; },
                                [](const aloam_ctx* x, const StageMask&) { return x->all_active && !x->any_frozen; }, &m)) return rc;
  const int* mask = m.dev;
  const bool sizes_pools = m.any_grow || !m.any_active;       // every active sequence frozen: nothing is inserted, the pools are neither sized nor waited for
  // at most four steps queued ahead of the device: the occupancy report the pools are sized from is never older than that
  hipEvent_t done = c->map_step_done[c->map_steps & 3];
  if (sizes_pools && c->map_steps >= 4) HIP_TRY(c, hipEventSynchronize(done));
  int rc = sizes_pools ? map_ensure_capacity(c) : ALOAM_OK;
  if (rc) return rc;
  c->inject_max = 0;
  MapArgs a = map_args(c);
  a.active = mask;
  { ProfScope p(c, K_MAP_BEGIN);
    if (c->spill_on) queue_map_spill(c, mask);                              // the cubes this step's shift empties, while they are still there
    if (c->any_attached) queue_atlas_window(c, mask);                       // attached sequences: the window cut from the atlas where it is stale or about to shift
    launch_map_begin(a, c->stream); }
  { ProfScope p(c, K_MAP_VOXEL_STACK);                                      // downSizeFilterCorner / Surf on the incoming clouds (:542-550)
    const VoxArgs v = vox_args(c, c->B * 2, c->map_levels);
    HIP_TRY(c, hipMemsetAsync(c->d_vox_counters.get() + 4, 0, 4 * sizeof(int), c->stream));   // general-path count, the two LDS-filter lists
    launch_map_stack_segments(a, v, c->stream);
    if (c->sum_order) launch_voxel_filter_reference_order(v, a, true, c->stream);
    else launch_voxel_filter(v, c->map_stack_tile_bound, c->stream); }
  { ProfScope p(c, K_MAP_GRID); launch_map_grid(a, c->stream); }            // kdtree*FromMap->setInputCloud (:558-559); kept by frozen sequences whose submap is unchanged
  for (int iter = 0; iter < 2; ++iter) {                                    // :562
    { ProfScope p(c, K_MAP_ASSOC); launch_map_associate(a, iter, c->stream); }
    { ProfScope p(c, K_MAP_SOLVE); launch_map_solve(a, iter, iter == 1, c->stream); }
  }
  { ProfScope p(c, K_MAP_INSERT); launch_map_insert(a, c->map.voxtmp.get(), c->stream); }        // :737-783 (not for frozen sequences)
  { ProfScope p(c, K_MAP_VOXEL_CUBES);                                      // per-cube re-filter (:788-801; frozen: empty segments)
    const VoxArgs v = vox_args(c, c->B * 2 * kMapValidMax, c->map.cube_levels);
    HIP_TRY(c, hipMemsetAsync(c->d_vox_counters.get() + 4, 0, 4 * sizeof(int), c->stream));
    launch_map_cube_segments(a, v, c->stream);
    if (c->sum_order) launch_voxel_filter_reference_order(v, a, false, c->stream);
    else launch_voxel_filter(v, c->map.tile_bound, c->stream); }
  { ProfScope p(c, K_MAP_REGISTER); launch_map_register(a, c->stream);      // :836-846
    c->map_steps += 1;
    launch_map_report(a, (int)c->map_steps, c->stream); }
  HIP_TRY(c, hipEventRecord(done, c->stream));
  HIP_TRY(c, hipGetLastError());
  on_mapping_step_queued(c);
  return ALOAM_OK;
}

// The mapping node's globals for one sequence (reference src/laserMapping.cpp:72-74,84-91,115-116): what a test or a restarted node
// injects to continue from a known map.
int aloam_set_map(aloam_ctx* c, int seq, int cls, const int* cube_ids, const int* counts, int n_cubes, const float* points_xyzw) {
  DeviceScope device_scope(c);
  int rc = check_seq(c, seq);
  if (rc) return rc;
  if (!c->map_on) { c->err = "mapping not enabled"; return ALOAM_E_STATE; }
  if (cls < 0 || cls > 1 || n_cubes < 0 || (n_cubes && (!cube_ids || !counts))) { c->err = "bad class / cube list"; return ALOAM_E_ARG; }
  long long total = 0;
  std::vector<CubeDesc> d(kMapCubes, CubeDesc{0, 0, 0, 0});
  for (int i = 0; i < n_cubes; ++i) {
    if (cube_ids[i] < 0 || cube_ids[i] >= kMapCubes || counts[i] < 0 || d[cube_ids[i]].cap) { c->err = "bad or repeated cube index"; return ALOAM_E_ARG; }
    d[cube_ids[i]] = CubeDesc{(int)total, counts[i], counts[i], 0};
    total += counts[i];
  }
  if (total && !points_xyzw) return ALOAM_E_ARG;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (total > c->map.points && (rc = grow_map_pool(c, total, false))) return rc;
  if ((rc = on_map_replaced(c, seq))) return rc;
  HIP_TRY(c, hipMemcpy(c->d_cubes.get() + ((size_t)seq * 2 + cls) * kMapCubes, d.data(), sizeof(CubeDesc) * kMapCubes, hipMemcpyHostToDevice));
  if (total) HIP_TRY(c, hipMemcpy(c->map.pool[cls].get() + (size_t)seq * c->map.points, points_xyzw, sizeof(float4) * (size_t)total, hipMemcpyHostToDevice));
  if ((rc = edit_seq(c, c->d_mapseq.get() + seq, [&](MapSeq& ms) { ms.pool_used[cls] = (int)total; }))) return rc;
  c->h_map_report[1 + cls] = std::max((int)c->h_map_report[1 + cls], (int)total);   // the pools are sized from this until the next step reports
  return ALOAM_OK;
}

int aloam_set_map_frame(aloam_ctx* c, int seq, const int cen[3], const double q_wmap_wodom[4], const double t_wmap_wodom[3], int frame_count) {
  DeviceScope device_scope(c);
  int rc = check_seq(c, seq);
  if (rc) return rc;
  if (!c->map_on) { c->err = "mapping not enabled"; return ALOAM_E_STATE; }
  if (!cen || !q_wmap_wodom || !t_wmap_wodom) return ALOAM_E_ARG;
  if ((rc = edit_seq(c, c->d_mapseq.get() + seq, [&](MapSeq& ms) {
         for (int k = 0; k < 3; ++k) { ms.cen[k] = cen[k]; ms.t_wmap_wodom[k] = t_wmap_wodom[k]; }
         for (int k = 0; k < 4; ++k) ms.q_wmap_wodom[k] = q_wmap_wodom[k];
         ms.frame_count = frame_count;
       }))) return rc;
  return on_map_replaced(c, seq);
}

int aloam_set_map_frozen(aloam_ctx* c, const int* frozen) {
  DeviceScope device_scope(c);
  if (!c) return ALOAM_E_ARG;
  if (const int rc = require_stage(c, ALOAM_STAGE_MAPPING)) return rc;
  if (!c->map_on) { c->err = "aloam_set_map_frozen before aloam_mapping_enable"; return ALOAM_E_STATE; }
  on_frozen_mask_set(c, frozen);
  return ALOAM_OK;
}

static int fetch_mapseq(aloam_ctx* c, int seq, MapSeq* ms) {
  int rc = check_seq(c, seq);
  if (rc) return rc;
  if (!c->map_on) { c->err = "mapping not enabled"; return ALOAM_E_STATE; }
  return read_seq(c, c->d_mapseq.get() + seq, ms);
}

int aloam_get_map_pose(aloam_ctx* c, int seq, double q_w_curr[4], double t_w_curr[3], double q_wmap_wodom[4], double t_wmap_wodom[3]) {
  DeviceScope device_scope(c);
  MapSeq ms;
  const int rc = fetch_mapseq(c, seq, &ms);
  if (rc) return rc;
  for (int k = 0; k < 4; ++k) { q_w_curr[k] = ms.par[k]; q_wmap_wodom[k] = ms.q_wmap_wodom[k]; }
  for (int k = 0; k < 3; ++k) { t_w_curr[k] = ms.par[4 + k]; t_wmap_wodom[k] = ms.t_wmap_wodom[k]; }
  return ALOAM_OK;
}

int aloam_get_map_info(aloam_ctx* c, int seq, int out[16]) {
  DeviceScope device_scope(c);
  MapSeq ms;
  const int rc = fetch_mapseq(c, seq, &ms);
  if (rc) return rc;
  const int v[16] = {ms.cen[0], ms.cen[1], ms.cen[2], ms.frame_count, ms.from_total[0], ms.from_total[1], ms.n_stack[0], ms.n_stack[1],
                     ms.factor_num[0][0], ms.factor_num[1][0], ms.factor_num[0][1], ms.factor_num[1][1], ms.lm_iterations[0], ms.lm_iterations[1],
                     ms.lm_termination[0], ms.compactions};
  std::memcpy(out, v, sizeof(v));
  return ALOAM_OK;
}

int aloam_map_cube_counts(aloam_ctx* c, int seq, int cls, int* out) {
  DeviceScope device_scope(c);
  MapSeq ms;
  const int rc = fetch_mapseq(c, seq, &ms);
  if (rc) return rc;
  if (cls < 0 || cls > 1) { c->err = "class must be 0 (corner) or 1 (surf)"; return ALOAM_E_ARG; }
  std::vector<CubeDesc> d(kMapCubes);
  HIP_TRY(c, hipMemcpy(d.data(), c->d_cubes.get() + ((size_t)seq * 2 + cls) * kMapCubes, sizeof(CubeDesc) * kMapCubes, hipMemcpyDeviceToHost));
  for (int i = 0; i < kMapCubes; ++i) out[i] = d[i].cnt;
  return kMapCubes;
}

int aloam_get_map_cube(aloam_ctx* c, int seq, int cls, int cube, float* out, int cap_points) {
  DeviceScope device_scope(c);
  MapSeq ms;
  const int rc = fetch_mapseq(c, seq, &ms);
  if (rc) return rc;
  if (cls < 0 || cls > 1 || cube < 0 || cube >= kMapCubes) { c->err = "bad class / cube index"; return ALOAM_E_ARG; }
  CubeDesc d;
  HIP_TRY(c, hipMemcpy(&d, c->d_cubes.get() + ((size_t)seq * 2 + cls) * kMapCubes + cube, sizeof(CubeDesc), hipMemcpyDeviceToHost));
  const int k = d.cnt < cap_points ? d.cnt : cap_points;
  if (k > 0) HIP_TRY(c, hipMemcpy(out, c->map.pool[cls].get() + (size_t)seq * c->map.points + d.off, sizeof(float4) * k, hipMemcpyDeviceToHost));
  return d.cnt;
}

int aloam_get_map_cloud(aloam_ctx* c, int seq, int which, float* out, int cap_points) {
  DeviceScope device_scope(c);
  MapSeq ms;
  int rc = fetch_mapseq(c, seq, &ms);
  if (rc) return rc;
  if (which == ALOAM_MAP_SURROUND || which == ALOAM_MAP_FULL) return get_cube_list(c, seq, which, out, cap_points);
  if (which != ALOAM_MAP_REGISTERED && which != ALOAM_MAP_CORNER_STACK && which != ALOAM_MAP_SURF_STACK) { c->err = "unknown map cloud id"; return ALOAM_E_ARG; }
  const float4* p;
  int n;
  if ((rc = find_cloud(c, seq, ALOAM_EXPORT_MAP + which, &p, &n))) return rc;
  const int k = n < cap_points ? n : cap_points;
  if (k > 0) HIP_TRY(c, hipMemcpy(out, p, sizeof(float4) * k, hipMemcpyDeviceToHost));
  return n;
}

}  // extern "C"
