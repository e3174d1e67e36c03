// a-loam_amd/csrc/capi_atlas.hip — host side of maps larger than the window.  The map spill: the rows that receive the cubes a window shift
// empties, the launch in front of k_map_begin, the stream-ordered drain and the counters.  The atlas: building the tile store (directory,
// merge of the cubes that several tiles make up, largest window), attaching sequences to it, the stale marks and the window launch.
#include <algorithm>
#include <cstring>
#include <unordered_map>

#include "capi_internal.hpp"

namespace aloam {

// k_map_spill for the mapping step that is being queued (inside its map_begin scope): the same mask, the pools as they are now.
void queue_map_spill(aloam_ctx* c, const int* mask) {
  SpillArgs a{};
  a.B = c->B; a.active = mask; a.attached = c->any_attached ? c->d_at_attached.get() : nullptr; a.seq = c->d_mapseq.get(); a.odom = c->d_state.get(); a.cubes = c->d_cubes.get();
  a.pool[0] = c->map.pool[0].get(); a.pool[1] = c->map.pool[1].get(); a.pool_cap = c->map.points;
  a.tiles = c->d_sp_tiles.get(); a.points = c->d_sp_points.get(); a.counters = c->d_sp_counters.get();
  a.max_tiles = c->spill_max_tiles; a.max_points = c->spill_max_points;
  launch_map_spill(a, c->stream);
}

// aloam_synchronize: tiles dropped since the last call (0 = none).  The stream has drained.
int spill_dropped_since(aloam_ctx* c, long long* fresh) {
  *fresh = 0;
  if (!c->spill_on) return ALOAM_OK;
  std::vector<int> cnt((size_t)c->B * kSpillInts);
  HIP_TRY(c, hipMemcpy(cnt.data(), c->d_sp_counters.get(), sizeof(int) * cnt.size(), hipMemcpyDeviceToHost));
  long long dropped = 0;
  for (int b = 0; b < c->B; ++b) dropped += cnt[(size_t)b * kSpillInts + kSpillDroppedTiles];
  *fresh = dropped - c->spill_dropped_reported;
  c->spill_dropped_reported = dropped;
  return ALOAM_OK;
}

int atlas_step_check(aloam_ctx* c) {
  if (!c->any_attached) return ALOAM_OK;
  for (int b = 0; b < c->B; ++b)
    if (c->seq[b].attached && takes_part(c, b) && !(c->any_frozen && c->seq[b].frozen)) {
      c->err = "sequence " + std::to_string(b) + " is attached to the atlas and active but not frozen (aloam_set_map_frozen): an attached window is never extended";
      return ALOAM_E_STATE;
    }
  return ALOAM_OK;
}

bool queue_atlas_window(aloam_ctx* c, const int* mask) {
  bool any = false;
  for (int b = 0; b < c->B; ++b) any |= c->seq[b].attached && takes_part(c, b);
  if (!any) return false;
  AtlasArgs a{};
  a.B = c->B; a.active = mask; a.attached = c->d_at_attached.get(); a.stale = c->d_at_stale.get();
  a.seq = c->d_mapseq.get(); a.odom = c->d_state.get(); a.cubes = c->d_cubes.get(); a.grid_sig = c->d_grid_sig.get();
  for (int k = 0; k < 2; ++k) { a.pool[k] = c->map.pool[k].get(); a.dir[k] = c->d_at_dir[k].get(); a.dir_mask[k] = c->at_dir_mask[k]; a.points[k] = c->d_at_points[k].get(); }
  a.pool_cap = c->map.points;
  launch_atlas_window(a, c->stream);
  return true;
}

}  // namespace aloam

// The largest number of points any 21 x 21 x 11 box of cubes holds: sliding sums over the occupied bounding box (exact), or, when that box
// has more than 2^24 cells, the class total (an upper bound).  *exact says which.
long long aloam::largest_window(const std::vector<int>& keys, const std::vector<int>& counts, const int lo[3], const int hi[3], bool* exact) {
  long long total = 0;
  for (int n : counts) total += n;
  const long long d[3] = {hi[0] - lo[0] + 1LL, hi[1] - lo[1] + 1LL, hi[2] - lo[2] + 1LL};
  if (keys.empty()) { *exact = true; return 0; }
  if (d[0] * d[1] * d[2] > (1LL << 24)) { *exact = false; return total; }
  *exact = true;
  std::vector<long long> vol((size_t)(d[0] * d[1] * d[2]), 0), tmp(vol.size());
  const long long stride[3] = {1, d[0], d[0] * d[1]};
  for (size_t i = 0; i < keys.size(); ++i) {
    const int x = (keys[i] >> 20) - kAtlasBias, y = ((keys[i] >> 10) & 1023) - kAtlasBias, z = (keys[i] & 1023) - kAtlasBias;
    vol[(size_t)((x - lo[0]) + d[0] * (y - lo[1]) + d[0] * d[1] * (z - lo[2]))] = counts[i];
  }
  const int win[3] = {kMapW, kMapH, kMapD};
  for (int axis = 0; axis < 3; ++axis) {                   // vol[x] := the sum of the win cells that end at x, along each axis in turn
    for (long long i = 0; i < (long long)vol.size(); ++i) {
      const long long pos = (i / stride[axis]) % d[axis];
      long long v = vol[(size_t)i] + (pos > 0 ? tmp[(size_t)(i - stride[axis])] : 0);    // running sum along the axis
      tmp[(size_t)i] = v;
    }
    for (long long i = 0; i < (long long)vol.size(); ++i) {
      const long long pos = (i / stride[axis]) % d[axis];
      vol[(size_t)i] = tmp[(size_t)i] - (pos >= win[axis] ? tmp[(size_t)(i - win[axis] * stride[axis])] : 0);
    }
  }
  return *std::max_element(vol.begin(), vol.end());
}

// tiles / points of aloam_atlas_load into host memory, wherever the caller keeps them.
static int fetch_host(aloam_ctx* c, const void* p, size_t bytes, const char* what, std::vector<char>* out) {
  out->resize(bytes);
  if (!bytes) return ALOAM_OK;
  if (!p) { c->err = std::string(what) + " is NULL"; return ALOAM_E_ARG; }
  void* d = nullptr;
  switch (classify_pointer(c, p, &d)) {
    case kMemManaged: case kMemOtherDevice: c->err = std::string(what) + " must be device memory of the context's device, pinned or pageable host memory"; return ALOAM_E_ARG;
    case kMemDevice: HIP_TRY(c, hipMemcpy(out->data(), p, bytes, hipMemcpyDeviceToHost)); break;
    default: std::memcpy(out->data(), p, bytes); break;
  }
  return ALOAM_OK;
}

static int require_spill(aloam_ctx* c) {
  if (!c->spill_on) { c->err = "the map spill is not enabled (aloam_map_spill_enable)"; return ALOAM_E_STATE; }
  return ALOAM_OK;
}

extern "C" {

int aloam_map_spill_enable(aloam_ctx* c, int max_tiles, int max_points) {
  DeviceScope device_scope(c);
  if (!c) return ALOAM_E_ARG;
  if (const int rc = require_stage(c, ALOAM_STAGE_MAPPING)) return rc;
  if (!c->map_on) { c->err = "aloam_map_spill_enable before aloam_mapping_enable"; return ALOAM_E_STATE; }
  if (c->spill_on) { c->err = "map spill already enabled"; return ALOAM_E_STATE; }
  if (max_tiles < 1 || max_tiles > (1 << 20) || max_points < 1 || max_points > (1 << 26)) { c->err = "bad spill capacities (1 <= max_tiles <= 2^20, 1 <= max_points <= 2^26)"; return ALOAM_E_ARG; }
  const size_t B = c->B;
  int rc;
  // a failure half way leaves spill_on false: the buffers that were allocated are released with the context or replaced by the next call
  if ((rc = dmalloc(c, c->d_sp_counters, B * kSpillInts))) return rc;
  if ((rc = dmalloc(c, c->d_sp_tiles, B * 2 * (size_t)max_tiles))) return rc;
  if (dalloc(c->d_sp_points, B * 2 * (size_t)max_points) != hipSuccess) {
    (void)hipGetLastError();
    c->err = "map spill of " + std::to_string(max_points) + " points per sequence and class: allocation failed";
    return ALOAM_E_HIP;
  }
  HIP_TRY(c, dalloc(c->d_sp_seqs, B)); HIP_TRY(c, dalloc(c->d_sp_cnt, 2 * B)); HIP_TRY(c, dalloc(c->d_sp_chunk, 2 * (B + 1))); HIP_TRY(c, dalloc(c->d_sp_off, 2 * (B + 1)));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  c->spill_max_tiles = max_tiles; c->spill_max_points = max_points; c->spill_dropped_reported = 0;
  c->spill_on = true;
  return ALOAM_OK;
}

int aloam_export_map_spill(aloam_ctx* c, const int* seqs, int n, aloam_map_tile* tiles_dst, long long cap_tiles, float* points_dst_xyzw,
                           long long cap_points, long long* dst_offsets, int clear) {
  DeviceScope device_scope(c);
  if (!c) return ALOAM_E_ARG;
  if (const int rc = require_spill(c)) return rc;
  if (const int rc = check_ids(c, seqs, n)) return rc;
  if (cap_tiles < 0 || cap_points < 0) { c->err = "negative cap_tiles / cap_points"; return ALOAM_E_ARG; }
  void *d_off = nullptr, *d_tiles = nullptr, *d_pts = nullptr;
  if (const int rc = export_target(c, dst_offsets, alignof(long long), "dst_offsets", &d_off)) return rc;
  if ((tiles_dst || cap_tiles > 0) && export_target(c, tiles_dst, alignof(aloam_map_tile), "tiles_dst", &d_tiles)) return ALOAM_E_ARG;
  if ((points_dst_xyzw || cap_points > 0) && export_target(c, points_dst_xyzw, 16, "points_dst", &d_pts)) return ALOAM_E_ARG;
  if (n > 0) if (const int rc = stage_ints(c, seqs, n, c->d_sp_seqs.get())) return rc;
  const size_t B = c->B;
  SpillExportArgs a{};
  a.seqs = c->d_sp_seqs.get(); a.n = n;
  a.tiles = c->d_sp_tiles.get(); a.points = c->d_sp_points.get(); a.counters = c->d_sp_counters.get();
  a.max_tiles = c->spill_max_tiles; a.max_points = c->spill_max_points;
  a.tile_off = c->d_sp_off.get(); a.point_off = c->d_sp_off.get() + (B + 1);
  a.tiles_dst = static_cast<aloam_map_tile*>(d_tiles); a.cap_tiles = d_tiles ? cap_tiles : 0;
  a.points_dst = static_cast<float4*>(d_pts); a.cap_points = d_pts ? cap_points : 0;
  launch_spill_count(a, c->d_sp_cnt.get(), c->d_sp_cnt.get() + B, c->stream);
  for (int k = 0; k < 2; ++k) {                            // k_export_scan: one segment per listed sequence; tiles, then points
    ExportArgs e{};
    e.n_ids = 1; e.nseq = n;
    e.seg_cnt = c->d_sp_cnt.get() + k * B; e.chunk_off = c->d_sp_chunk.get() + k * (B + 1); e.seg_off = c->d_sp_off.get() + k * (B + 1);
    e.dst_off = static_cast<long long*>(d_off) + (size_t)k * (n + 1);
    launch_export_scan(e, c->stream);
  }
  launch_spill_gather(a, clear != 0, c->stream);
  HIP_TRY(c, hipGetLastError());
  return ALOAM_OK;
}

int aloam_atlas_load(aloam_ctx* c, const aloam_map_tile* tiles, long long n_tiles, const float* points_xyzw, long long n_points) {
  DeviceScope device_scope(c);
  if (!c) return ALOAM_E_ARG;
  if (const int rc = require_stage(c, ALOAM_STAGE_MAPPING)) return rc;
  if (!c->map_on) { c->err = "aloam_atlas_load before aloam_mapping_enable"; return ALOAM_E_STATE; }
  if (n_tiles < 0 || n_points < 0 || n_points > 0x7fffffffLL || n_tiles > 0x7fffffffLL) { c->err = "bad tile / point counts"; return ALOAM_E_ARG; }
  if (c->any_attached) { c->err = "a sequence is attached to the atlas: detach (aloam_atlas_attach) before it is replaced or unloaded"; return ALOAM_E_STATE; }
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (n_tiles == 0) {
    for (int k = 0; k < 2; ++k) { c->d_at_dir[k].reset(); c->d_at_points[k].reset(); c->at_dir_mask[k] = 0; }
    std::fill(c->at_info, c->at_info + 12, 0LL);
    c->atlas_on = false;
    return ALOAM_OK;
  }
  std::vector<char> hb_t, hb_p;
  int rc;
  if ((rc = fetch_host(c, tiles, sizeof(aloam_map_tile) * (size_t)n_tiles, "tiles", &hb_t))) return rc;
  if ((rc = fetch_host(c, points_xyzw, sizeof(float4) * (size_t)n_points, "points", &hb_p))) return rc;
  const aloam_map_tile* T = reinterpret_cast<const aloam_map_tile*>(hb_t.data());
  const float4* P = reinterpret_cast<const float4*>(hb_p.data());
  for (long long i = 0; i < n_tiles; ++i) {                // everything is validated before anything changes
    const aloam_map_tile& t = T[i];
    if (t.feature_class < 0 || t.feature_class > 1 || t.count < 0 || t.first_point < 0 || t.first_point + t.count > n_points || !atlas_in_range(t.cube[0], t.cube[1], t.cube[2])) {
      c->err = "tile " + std::to_string(i) + ": bad class, count, point range or cube (absolute cubes -512 .. 511)";
      return ALOAM_E_ARG;
    }
  }
  // per class: the cubes in first-seen order, each the concatenation of its tiles in array order
  struct Cube { int key; long long first; int raw, n_tiles, count; };
  std::vector<Cube> cubes[2];
  std::vector<float4> packed[2];
  std::vector<AtlasMergeJob> jobs;
  int largest_concat = 0;
  for (int cls = 0; cls < 2; ++cls) {
    std::unordered_map<int, int> at;
    std::vector<std::vector<long long>> members;
    for (long long i = 0; i < n_tiles; ++i) {
      if (T[i].feature_class != cls || T[i].count == 0) continue;
      const int key = atlas_key(T[i].cube[0], T[i].cube[1], T[i].cube[2]);
      auto it = at.find(key);
      if (it == at.end()) { it = at.emplace(key, (int)members.size()).first; members.emplace_back(); cubes[cls].push_back(Cube{key, 0, 0, 0, 0}); }
      members[it->second].push_back(i);
    }
    for (size_t g = 0; g < members.size(); ++g) {
      Cube& cb = cubes[cls][g];
      cb.first = (long long)packed[cls].size();
      for (long long i : members[g]) { packed[cls].insert(packed[cls].end(), P + T[i].first_point, P + T[i].first_point + T[i].count); cb.raw += T[i].count; }
      cb.n_tiles = (int)members[g].size(); cb.count = cb.raw;
      if (cb.n_tiles > 1) { jobs.push_back(AtlasMergeJob{cb.first, 0, cb.raw, cls, (int)g, 0}); largest_concat = std::max(largest_concat, cb.raw); }
    }
    if (packed[cls].size() > 0x7fffffffULL) { c->err = "more than 2^31 points of one class"; return ALOAM_E_CAPACITY; }
  }
  // a concatenation is filtered through the scratch of the per-cube filter, which holds a pool row: larger ones grow the pools first
  if (largest_concat > c->map.points && (rc = grow_map_pool(c, largest_concat, false))) return rc;
  DevBuf<float4> d_pts[2];
  DevBuf<AtlasEntry> d_dir[2];
  for (int cls = 0; cls < 2; ++cls) {
    HIP_TRY(c, dalloc(d_pts[cls], std::max<size_t>(1, packed[cls].size())));
    if (!packed[cls].empty()) HIP_TRY(c, hipMemcpy(d_pts[cls].get(), packed[cls].data(), sizeof(float4) * packed[cls].size(), hipMemcpyHostToDevice));
  }
  if (!jobs.empty()) {                                     // rounds of at most map_nsegs_max segments that fit the key scratch and the tile lists
    DevBuf<AtlasMergeJob> d_jobs; DevBuf<int> d_counts;
    HIP_TRY(c, dalloc(d_jobs, (size_t)c->map_nsegs_max)); HIP_TRY(c, dalloc(d_counts, jobs.size()));
    std::vector<int> slot_of(jobs.size());
    for (size_t j = 0; j < jobs.size(); ++j) { slot_of[j] = jobs[j].count_slot; jobs[j].count_slot = (int)j; }
    for (size_t j0 = 0; j0 < jobs.size();) {
      size_t j1 = j0; long long keys = 0, vtiles = 0;
      while (j1 < jobs.size() && (long long)(j1 - j0) < c->map_nsegs_max && keys + jobs[j1].n <= c->map.key_cap && vtiles + (jobs[j1].n + kVoxTile - 1) / kVoxTile <= c->map.tile_cap) {
        jobs[j1].tmp_off = keys; keys += jobs[j1].n; vtiles += (jobs[j1].n + kVoxTile - 1) / kVoxTile; ++j1;
      }
      if (j1 == j0) { c->err = "a merged cube does not fit the voxel-filter scratch"; return ALOAM_E_CAPACITY; }
      HIP_TRY(c, hipMemcpy(d_jobs.get(), jobs.data() + j0, sizeof(AtlasMergeJob) * (j1 - j0), hipMemcpyHostToDevice));
      const VoxArgs v = vox_args(c, (int)(j1 - j0), c->map.cube_levels);
      AtlasMergeArgs m{};
      m.jobs = d_jobs.get(); m.n_jobs = (int)(j1 - j0); m.points[0] = d_pts[0].get(); m.points[1] = d_pts[1].get(); m.counts = d_counts.get();
      m.leaf[0] = c->map_line_res; m.leaf[1] = c->map_plane_res;
      HIP_TRY(c, hipMemsetAsync(c->d_vox_counters.get() + 4, 0, 4 * sizeof(int), c->stream));
      launch_atlas_merge_segments(m, v, c->stream);
      launch_voxel_filter(v, c->map.tile_bound, c->stream);   // always the input-order sum, whatever aloam_set_voxel_sum_order says
      HIP_TRY(c, hipStreamSynchronize(c->stream));
      j0 = j1;
    }
    std::vector<int> merged(jobs.size());
    HIP_TRY(c, hipMemcpy(merged.data(), d_counts.get(), sizeof(int) * jobs.size(), hipMemcpyDeviceToHost));
    for (size_t j = 0; j < jobs.size(); ++j) cubes[jobs[j].cls][slot_of[j]].count = merged[j];
  }
  long long info[12] = {0};
  info[0] = n_tiles;
  int lo[3] = {kAtlasBias, kAtlasBias, kAtlasBias}, hi[3] = {-kAtlasBias, -kAtlasBias, -kAtlasBias};
  for (int cls = 0; cls < 2; ++cls)
    for (const Cube& cb : cubes[cls]) {
      const int xyz[3] = {(cb.key >> 20) - kAtlasBias, ((cb.key >> 10) & 1023) - kAtlasBias, (cb.key & 1023) - kAtlasBias};
      for (int k = 0; k < 3; ++k) { lo[k] = std::min(lo[k], xyz[k]); hi[k] = std::max(hi[k], xyz[k]); }
    }
  int mask[2];
  long long bytes = 0;
  bool all_exact = true;
  for (int cls = 0; cls < 2; ++cls) {
    size_t size = 16;
    while (size < 2 * cubes[cls].size()) size <<= 1;
    std::vector<AtlasEntry> dir(size, AtlasEntry{-1, 0, 0, 0});
    std::vector<int> keys, counts;
    for (const Cube& cb : cubes[cls]) {
      unsigned h = atlas_hash(cb.key) & (unsigned)(size - 1);
      while (dir[h].key != -1) h = (h + 1) & (unsigned)(size - 1);
      dir[h] = AtlasEntry{cb.key, (int)cb.first, cb.count, 0};
      keys.push_back(cb.key); counts.push_back(cb.count);
      info[3 + cls] += cb.count;
    }
    info[1 + cls] = (long long)cubes[cls].size();
    HIP_TRY(c, dalloc(d_dir[cls], size));
    HIP_TRY(c, hipMemcpy(d_dir[cls].get(), dir.data(), sizeof(AtlasEntry) * size, hipMemcpyHostToDevice));
    mask[cls] = (int)size - 1;
    bool exact = true;
    info[8 + cls] = largest_window(keys, counts, lo, hi, &exact);
    all_exact &= exact;
    bytes += (long long)(sizeof(AtlasEntry) * size + sizeof(float4) * std::max<size_t>(1, packed[cls].size()));
  }
  for (int k = 0; k < 3; ++k) info[5 + k] = hi[k] >= lo[k] ? hi[k] - lo[k] + 1 : 0;
  info[10] = all_exact ? 1 : 0;
  info[11] = bytes;
  for (int cls = 0; cls < 2; ++cls) { c->d_at_points[cls] = std::move(d_pts[cls]); c->d_at_dir[cls] = std::move(d_dir[cls]); c->at_dir_mask[cls] = mask[cls]; }
  std::copy(info, info + 12, c->at_info);
  c->atlas_on = true;
  return ALOAM_OK;
}

int aloam_atlas_attach(aloam_ctx* c, const int* attached) {
  DeviceScope device_scope(c);
  if (!c) return ALOAM_E_ARG;
  if (const int rc = require_stage(c, ALOAM_STAGE_MAPPING)) return rc;
  if (!c->map_on) { c->err = "aloam_atlas_attach before aloam_mapping_enable"; return ALOAM_E_STATE; }
  std::vector<int> m(c->B, 0);
  if (attached) for (int b = 0; b < c->B; ++b) m[b] = attached[b] != 0 ? 1 : 0;
  const bool any = std::find(m.begin(), m.end(), 1) != m.end();
  if (any && !c->atlas_on) { c->err = "no atlas is loaded (aloam_atlas_load)"; return ALOAM_E_STATE; }
  if (any) {
    const long long need = std::max(c->at_info[8], c->at_info[9]);      // a pool row must hold the largest window
    if (need > c->map.points) {
      HIP_TRY(c, hipStreamSynchronize(c->stream));
      if (const int rc = grow_map_pool(c, need, false)) { c->err = "the largest window of the atlas exceeds the pool limit"; return rc; }
    }
  }
  if (!c->d_at_attached) { if (const int rc = dmalloc(c, c->d_at_attached, c->B)) return rc; if (const int rc = dmalloc(c, c->d_at_stale, c->B)) return rc; }
  if (const int rc = stage_ints(c, m.data(), c->B, c->d_at_attached.get())) return rc;
  return on_atlas_attached(c, m);
}

int aloam_atlas_info(aloam_ctx* c, long long out[12]) {
  if (!c || !out) return ALOAM_E_ARG;
  if (!c->map_on) { c->err = "mapping not enabled"; return ALOAM_E_STATE; }
  std::copy(c->at_info, c->at_info + 12, out);
  return ALOAM_OK;
}

int aloam_get_map_spill_info(aloam_ctx* c, int seq, int out[8]) {
  DeviceScope device_scope(c);
  int rc = check_seq(c, seq);
  if (rc) return rc;
  if (!out) return ALOAM_E_ARG;
  if ((rc = require_spill(c))) return rc;
  int cnt[kSpillInts];
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, hipMemcpy(cnt, c->d_sp_counters.get() + (size_t)seq * kSpillInts, sizeof(cnt), hipMemcpyDeviceToHost));
  const int v[8] = {cnt[kSpillTiles], cnt[kSpillTiles + 1], cnt[kSpillPoints], cnt[kSpillPoints + 1], cnt[kSpillDroppedTiles], cnt[kSpillDroppedPoints],
                    c->spill_max_tiles, c->spill_max_points};
  std::copy(v, v + 8, out);
  return ALOAM_OK;
}

}  // extern "C"
