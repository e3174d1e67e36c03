// a-loam_amd/csrc/capi_graphmap.hip — host side of the keyframe clouds of the pose graphs and of the map assembled from them at the graph's
// poses (aloam_graph_keyframes_enable / aloam_graph_export_keyframes / aloam_graph_keyframe_info / aloam_graph_export_map).
// Keyframe points never pass through host memory.  aloam_graph_export_map synchronises the context's stream once, after the transform
// pass (once more per doubling of a directory that proved too small), and reads back the directory of (cube, class, piece) counts: from it the host lays out the grouped points and plans the rounds of
// the voxel filter as aloam_atlas_load does.
#include <algorithm>
#include <cstring>

#include "capi_internal.hpp"

int aloam::require_keyframes(aloam_ctx* c) {
  if (!c->kf.on) { c->err = "keyframe clouds are not enabled (aloam_graph_keyframes_enable)"; return ALOAM_E_STATE; }
  return ALOAM_OK;
}

KfStore aloam::kf_store(aloam_ctx* c) {
  KfStore k{};
  k.points[0] = c->kf.points[0].get(); k.points[1] = c->kf.points[1].get(); k.desc = c->kf.desc.get(); k.counters = c->kf.counters.get();
  k.cap[0] = c->kf.cap[0]; k.cap[1] = c->kf.cap[1]; k.max_nodes = c->pg.max_nodes;
  return k;
}

// Two scratch buffers that share one size: both released, then both allocated anew (their contents are not needed), or neither.
template <typename T>
static int grow_together(aloam_ctx* c, Scratch<T>& a, Scratch<T>& b, long long need) {
  if (a.cap >= need && b.cap >= need) return ALOAM_OK;
  a.release(); b.release();
  if (dalloc(a.p, (size_t)need) != hipSuccess || dalloc(b.p, (size_t)need) != hipSuccess) {
    (void)hipGetLastError(); a.release(); b.release(); c->err = "map at the graph's poses: scratch allocation failed"; return ALOAM_E_HIP;
  }
  a.cap = b.cap = need;
  return ALOAM_OK;
}

namespace aloam {

// aloam_graph_add_nodes with the store enabled: every listed sequence must hold the stacks of a mapping step.
int keyframe_add_check(aloam_ctx* c, const int* seqs, int n) {
  if (!c->kf.on) return ALOAM_OK;
  for (int i = 0; i < n; ++i)
    if (!c->seq[seqs[i]].has_stacks) {
      c->err = "sequence " + std::to_string(seqs[i]) + " has not been active in a mapping step since it was created, reset or loaded: it holds no stacks to keep as a keyframe";
      return ALOAM_E_STATE;
    }
  return ALOAM_OK;
}

// Behind k_graph_add_nodes: pg.add holds the (sequence, node) items of the call.
void queue_keyframe_capture(aloam_ctx* c, int n) {
  if (!c->kf.on || n <= 0) return;
  KfCaptureArgs a{};
  a.n = n; a.items = c->pg.add.get(); a.mapseq = c->d_mapseq.get();
  a.stack[0] = c->d_stack[0].get(); a.stack[1] = c->d_stack[1].get();
  a.stack_row[0] = (long long)c->R * kLessSharpPerRing; a.stack_row[1] = c->cap;
  a.kf = kf_store(c);
  ProfScope p(c, K_GRAPH_MAP);
  launch_keyframe_capture(a, c->stream);
}

// aloam_graph_clear: the listed sequences' cursors back to 0, in stream order (node 0 of the next drive starts its rows again).
int queue_keyframe_rewind(aloam_ctx* c, const int* seqs, int n) {
  if (!c->kf.on) return ALOAM_OK;
  for (int i = 0; i < n; ++i) HIP_TRY(c, hipMemsetAsync(c->kf.counters.get() + (size_t)seqs[i] * kKfInts + kKfCursor, 0, 2 * sizeof(int), c->stream));
  return ALOAM_OK;
}

// aloam_synchronize: nodes kept without clouds since the last call (0 = none).  The stream has drained.
int keyframes_dropped_since(aloam_ctx* c, long long* fresh) {
  *fresh = 0;
  if (!c->kf.on) return ALOAM_OK;
  std::vector<int> cnt((size_t)c->B * kKfInts);
  HIP_TRY(c, hipMemcpy(cnt.data(), c->kf.counters.get(), sizeof(int) * cnt.size(), hipMemcpyDeviceToHost));
  long long dropped = 0;
  for (int b = 0; b < c->B; ++b) dropped += cnt[(size_t)b * kKfInts + kKfDroppedNodes];
  *fresh = dropped - c->kf.dropped_reported;
  c->kf.dropped_reported = dropped;
  return ALOAM_OK;
}

// The point scratch of a map export, sized for the host's bounds: transformed points, grouped points, directory slots.
int graph_map_scratch(aloam_ctx* c, long long bound_points) {
  if (const int rc = grow_together(c, c->gm.world, c->gm.grouped, std::max<long long>(bound_points, 1))) return rc;
  return c->gm.slot.grow(c, std::max<long long>(bound_points, 1));
}

// The half of a map export that does not care whether a key's group came from a request or from a group of parts: the directory grown
// until the transform fits it, its read-back and sort, the segment and job layout, the rounds, the pool growth, the grouping pass, the
// filter and the emit.  n groups (requests, or groups of parts) of n_pieces pieces; `passes` launches the two passes over the piece table.
int graph_map_run(aloam_ctx* c, int n, int n_pieces, int* d_outside, int* d_flags, const GmPasses& passes, const GmDst& dst, const char* unit) {
  // The directory starts at 128 slots per piece (a sweep's points fall into about a dozen cubes), or where an earlier call had to grow it
  // to; a call whose pieces scatter over more cubes than that runs the transform again with the directory doubled, up to kGmDirMax.
  long long dir_size = std::max<long long>(4096, c->gm.dir_hint);
  while (dir_size < 128LL * n_pieces && dir_size < kGmDirMax) dir_size <<= 1;
  int rc;
  std::vector<unsigned long long> keys;
  std::vector<int> counts;
  for (;;) {
    if ((rc = c->gm.dir_key.grow(c, dir_size))) return rc;
    if ((rc = c->gm.dir_count.grow(c, dir_size))) return rc;
    if ((rc = c->gm.dir_base.grow(c, dir_size))) return rc;
    HIP_TRY(c, hipMemsetAsync(d_outside, 0, sizeof(int) * ((size_t)n + 1), c->stream));   // (and the flag behind it)
    HIP_TRY(c, hipMemsetAsync(c->gm.dir_key.get(), 0xff, sizeof(unsigned long long) * (size_t)dir_size, c->stream));
    HIP_TRY(c, hipMemsetAsync(c->gm.dir_count.get(), 0, sizeof(int) * (size_t)dir_size, c->stream));
    {
      ProfScope p(c, K_GRAPH_MAP);
      passes.transform((unsigned)(dir_size - 1));
    }
    HIP_TRY(c, hipGetLastError());
    // ---- the synchronisation: the directory comes back, the points stay where they are
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    int overflow = 0;
    HIP_TRY(c, hipMemcpy(&overflow, d_flags, sizeof(int), hipMemcpyDeviceToHost));
    if (!overflow) break;
    if (dir_size >= kGmDirMax) {
      c->err = "the keyframes fall into more (cube, piece) pairs than the largest directory (2^22 entries) holds: export fewer nodes per call";
      return ALOAM_E_CAPACITY;
    }
    dir_size <<= 1;
  }
  c->gm.dir_hint = dir_size;
  keys.resize((size_t)dir_size); counts.resize((size_t)dir_size);
  HIP_TRY(c, hipMemcpy(keys.data(), c->gm.dir_key.get(), sizeof(unsigned long long) * keys.size(), hipMemcpyDeviceToHost));
  HIP_TRY(c, hipMemcpy(counts.data(), c->gm.dir_count.get(), sizeof(int) * counts.size(), hipMemcpyDeviceToHost));
  struct Entry { unsigned long long key; int slot; };
  std::vector<Entry> ent;
  for (long long h = 0; h < dir_size; ++h) if (keys[(size_t)h] != kGmEmpty) ent.push_back(Entry{keys[(size_t)h], (int)h});
  std::sort(ent.begin(), ent.end(), [](const Entry& a, const Entry& b) { return a.key < b.key; });
  // one segment per (request, class, cube): its pieces follow each other in member order
  std::vector<AtlasMergeJob> jobs;
  std::vector<GmSegInfo> segs;
  std::vector<long long> dir_base((size_t)dir_size, 0);
  std::vector<GmRequestOut> out((size_t)n + 1, GmRequestOut{0, 0, {0, 0}});
  long long total = 0, largest = 0;
  {
    size_t e = 0;
    for (int grp = 0; grp < 2 * n; ++grp) {
      const int r = grp >> 1, cls = grp & 1;
      if (cls == 0) out[r].seg_first = (int)jobs.size(); else out[r].surf_first = (int)jobs.size();
      long long raw = 0;
      while (e < ent.size() && (int)(ent[e].key >> 46) == grp) {
        const unsigned long long cube = ent[e].key >> 16;                    // (group, cube)
        long long seg_n = 0;
        const long long first = total;
        for (; e < ent.size() && (ent[e].key >> 16) == cube; ++e) { dir_base[(size_t)ent[e].slot] = total; total += counts[(size_t)ent[e].slot]; seg_n += counts[(size_t)ent[e].slot]; }
        if (seg_n > 0x7fffffffLL) { c->err = "more than 2^31 points in one cube"; return ALOAM_E_CAPACITY; }
        jobs.push_back(AtlasMergeJob{first, 0, (int)seg_n, cls, (int)jobs.size(), 0});
        segs.push_back(GmSegInfo{(int)(cube & 0x3fffffffULL), r});
        raw += seg_n; largest = std::max(largest, seg_n);
      }
      if (raw > 0x7fffffffLL) { c->err = std::string("more than 2^31 points of one class in a ") + unit; return ALOAM_E_CAPACITY; }
      out[r].raw[cls] = (int)raw;
    }
  }
  const int n_segs = (int)jobs.size();
  out[(size_t)n].seg_first = n_segs; out[(size_t)n].surf_first = n_segs;
  // a (cube, class) is filtered through the scratch of the per-cube filter, which holds a pool row: larger ones grow the pools first
  if (largest > c->map.points && (rc = grow_map_pool(c, largest, false))) { c->err = "a cube of the exported map exceeds the pool limit"; return rc; }
  // rounds of at most map_nsegs_max segments that fit the key scratch and the tile lists, as aloam_atlas_load plans them
  std::vector<int> round_end;
  for (size_t j0 = 0; j0 < jobs.size();) {
    size_t j1 = j0; long long nkeys = 0, vtiles = 0;
    while (j1 < jobs.size() && (long long)(j1 - j0) < c->map_nsegs_max && nkeys + jobs[j1].n <= c->map.key_cap && vtiles + (jobs[j1].n + kVoxTile - 1) / kVoxTile <= c->map.tile_cap) {
      jobs[j1].tmp_off = nkeys; nkeys += jobs[j1].n; vtiles += (jobs[j1].n + kVoxTile - 1) / kVoxTile; ++j1;
    }
    if (j1 == j0) { c->err = "a cube of the exported map does not fit the voxel-filter scratch"; return ALOAM_E_CAPACITY; }
    round_end.push_back((int)j1);
    j0 = j1;
  }
  if ((rc = c->gm.jobs.grow(c, (long long)std::max(n_segs, 1)))) return rc;
  if ((rc = c->gm.seg.grow(c, (long long)std::max(n_segs, 1)))) return rc;
  if ((rc = c->gm.counts.grow(c, (long long)std::max(n_segs, 1)))) return rc;
  if ((rc = c->gm.point_off.grow(c, (long long)n_segs + 1))) return rc;
  // ---- from here everything is stream-ordered
  HIP_TRY(c, hipMemcpyAsync(c->gm.dir_base.get(), dir_base.data(), sizeof(long long) * dir_base.size(), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemsetAsync(c->gm.dir_count.get(), 0, sizeof(int) * (size_t)dir_size, c->stream));
  HIP_TRY(c, hipMemcpyAsync(c->gm.req_out.get(), out.data(), sizeof(GmRequestOut) * out.size(), hipMemcpyHostToDevice, c->stream));
  if (n_segs > 0) {
    HIP_TRY(c, hipMemcpyAsync(c->gm.jobs.get(), jobs.data(), sizeof(AtlasMergeJob) * jobs.size(), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->gm.seg.get(), segs.data(), sizeof(GmSegInfo) * segs.size(), hipMemcpyHostToDevice, c->stream));
  }
  {
    ProfScope p(c, K_GRAPH_MAP);
    passes.group();
    int j0 = 0;
    for (const int j1 : round_end) {
      const VoxArgs v = vox_args(c, j1 - j0, c->map.cube_levels);
      AtlasMergeArgs m{};
      m.jobs = c->gm.jobs.get() + j0; m.n_jobs = j1 - j0; m.points[0] = c->gm.grouped.get(); m.points[1] = c->gm.grouped.get(); m.counts = c->gm.counts.get();
      m.leaf[0] = c->map_line_res; m.leaf[1] = c->map_plane_res;
      HIP_TRY(c, hipMemsetAsync(c->d_vox_counters.get() + 4, 0, 4 * sizeof(int), c->stream));
      launch_atlas_merge_segments(m, v, c->stream);
      launch_voxel_filter(v, c->map.tile_bound, c->stream);   // always the input-order sum, whatever aloam_set_voxel_sum_order says
      j0 = j1;
    }
    GmEmitArgs e{};
    e.n = n; e.n_segs = n_segs; e.req = c->gm.req_out.get(); e.jobs = c->gm.jobs.get(); e.seg = c->gm.seg.get(); e.counts = c->gm.counts.get();
    e.point_off = c->gm.point_off.get(); e.outside = d_outside; e.grouped = c->gm.grouped.get();
    e.tiles_dst = static_cast<aloam_map_tile*>(dst.tiles); e.cap_tiles = dst.tiles ? dst.cap_tiles : 0;
    e.points_dst = static_cast<float4*>(dst.points); e.cap_points = dst.points ? dst.cap_points : 0;
    e.dst_off = static_cast<long long*>(dst.offsets); e.stats = static_cast<aloam_graph_map_stats*>(dst.stats);
    launch_graph_map_emit(e, c->stream);
  }
  HIP_TRY(c, hipGetLastError());
  c->gm.last_raw = total; c->gm.last_segs = n_segs;
  return ALOAM_OK;
}

}  // namespace aloam

extern "C" {

int aloam_graph_keyframes_enable(aloam_ctx* c, int max_corner_points, int max_surf_points) {
  DeviceScope device_scope(c);
  if (!c) return ALOAM_E_ARG;
  if (!c->pg.on) { c->err = "aloam_graph_keyframes_enable before aloam_graph_enable"; return ALOAM_E_STATE; }
  if (!c->map_on) { c->err = "aloam_graph_keyframes_enable before aloam_mapping_enable"; return ALOAM_E_STATE; }
  if (c->kf.on) { c->err = "keyframe clouds already enabled"; return ALOAM_E_STATE; }
  for (int b = 0; b < c->B; ++b)
    if (c->seq[b].graph_nodes > 0) { c->err = "the graph of sequence " + std::to_string(b) + " already holds nodes: enable the keyframe clouds while every graph is empty"; return ALOAM_E_STATE; }
  if (max_corner_points < 1 || max_corner_points > kKfRowMax || max_surf_points < 1 || max_surf_points > kKfRowMax) {
    c->err = "bad keyframe capacities (1 <= max_corner_points, max_surf_points <= 2^26)";
    return ALOAM_E_ARG;
  }
  const size_t B = c->B;
  KeyframeStore k;                     // committed with one move: nothing stays allocated behind a refusal
  const bool ok = dalloc(k.points[0], B * (size_t)max_corner_points) == hipSuccess && dalloc(k.points[1], B * (size_t)max_surf_points) == hipSuccess &&
                  dalloc(k.desc, B * (size_t)c->pg.max_nodes) == hipSuccess && dalloc(k.counters, B * kKfInts) == hipSuccess &&
                  hipMemsetAsync(k.counters.get(), 0, sizeof(int) * B * kKfInts, c->stream) == hipSuccess;
  if (!ok) {
    (void)hipGetLastError();
    c->err = "keyframe store of " + std::to_string(max_corner_points) + " + " + std::to_string(max_surf_points) + " points per sequence: allocation failed";
    return ALOAM_E_HIP;
  }
  k.cap[0] = max_corner_points; k.cap[1] = max_surf_points;
  k.on = true;
  c->kf = std::move(k);
  return ALOAM_OK;
}

int aloam_graph_export_keyframes(aloam_ctx* c, int seq, int first, int count, int feature_class, float* points_dst_xyzw, long long cap_points, long long* dst_offsets) {
  DeviceScope device_scope(c);
  if (!c) return ALOAM_E_ARG;
  if (const int rc = require_keyframes(c)) return rc;
  if (const int rc = check_seq(c, seq)) return rc;
  if (first < 0 || count < 0 || first + (long long)count > c->seq[seq].graph_nodes) { c->err = "[first, first + count) must lie inside what the sequence's graph holds"; return ALOAM_E_ARG; }
  if (feature_class < 0 || feature_class > 1) { c->err = "feature_class must be 0 (corner) or 1 (surf)"; return ALOAM_E_ARG; }
  if (cap_points < 0) { c->err = "negative cap_points"; return ALOAM_E_ARG; }
  void *d_off = nullptr, *d_pts = nullptr;
  if (const int rc = export_target(c, dst_offsets, alignof(long long), "dst_offsets", &d_off)) return rc;
  if ((points_dst_xyzw || cap_points > 0) && export_target(c, points_dst_xyzw, 16, "points_dst", &d_pts)) return ALOAM_E_ARG;
  KfExportArgs a{};
  a.desc = c->kf.desc.get() + (size_t)seq * c->pg.max_nodes;
  a.points = c->kf.points[feature_class].get() + (size_t)seq * c->kf.cap[feature_class];
  a.first = first; a.count = count; a.cls = feature_class;
  a.dst = static_cast<float4*>(d_pts); a.cap = d_pts ? cap_points : 0; a.dst_off = static_cast<long long*>(d_off);
  launch_keyframe_export(a, c->stream);
  HIP_TRY(c, hipGetLastError());
  return ALOAM_OK;
}

int aloam_graph_keyframe_info(aloam_ctx* c, int seq, long long out[8]) {
  DeviceScope device_scope(c);
  if (!c || !out) return ALOAM_E_ARG;
  if (const int rc = require_keyframes(c)) return rc;
  if (const int rc = check_seq(c, seq)) return rc;
  int cnt[kKfInts];
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, hipMemcpy(cnt, c->kf.counters.get() + (size_t)seq * kKfInts, sizeof(cnt), hipMemcpyDeviceToHost));
  const long long v[8] = {cnt[kKfCursor], cnt[kKfCursor + 1], c->kf.cap[0], c->kf.cap[1], cnt[kKfDroppedNodes], cnt[kKfDroppedPoints], 0, 0};
  std::copy(v, v + 8, out);
  return ALOAM_OK;
}

int aloam_graph_export_map(aloam_ctx* c, const aloam_graph_map_request* req, int n, aloam_map_tile* tiles_dst, long long cap_tiles, float* points_dst_xyzw,
                           long long cap_points, long long* dst_offsets, aloam_graph_map_stats* stats_dst) {
  DeviceScope device_scope(c);
  if (!c) return ALOAM_E_ARG;
  if (const int rc = require_keyframes(c)) return rc;
  // ---- everything is checked before anything is queued
  if (n < 0 || n > kGmMaxRequests || (n > 0 && !req)) { c->err = "bad request list (0 <= n <= 32768)"; return ALOAM_E_ARG; }
  if (n > 0) if (const int rc = require_host_list(c, req, "req")) return rc;
  for (int r = 0; r < n; ++r) {
    const aloam_graph_map_request& q = req[r];
    auto fail = [&](const char* what) { c->err = "request " + std::to_string(r) + ": " + what; return ALOAM_E_ARG; };
    if (q.seq < 0 || q.seq >= c->B) return fail("seq out of range");
    if (q.first < 0 || q.count < 0 || q.first + (long long)q.count > c->seq[q.seq].graph_nodes) return fail("[first, first + count) must lie inside what the sequence's graph holds");
    if (q.pose != ALOAM_GRAPH_POSE_ENTERED && q.pose != ALOAM_GRAPH_POSE_OPTIMIZED) return fail("pose must be ALOAM_GRAPH_POSE_ENTERED or ALOAM_GRAPH_POSE_OPTIMIZED");
  }
  if (cap_tiles < 0 || cap_points < 0) { c->err = "negative cap_tiles / cap_points"; return ALOAM_E_ARG; }
  void *d_off = nullptr, *d_tiles = nullptr, *d_pts = nullptr, *d_stats = nullptr;
  if (const int rc = export_target(c, dst_offsets, alignof(long long), "dst_offsets", &d_off)) return rc;
  if ((tiles_dst || cap_tiles > 0) && export_target(c, tiles_dst, alignof(aloam_map_tile), "tiles_dst", &d_tiles)) return ALOAM_E_ARG;
  if ((points_dst_xyzw || cap_points > 0) && export_target(c, points_dst_xyzw, 16, "points_dst", &d_pts)) return ALOAM_E_ARG;
  if (stats_dst && export_target(c, stats_dst, alignof(aloam_graph_map_stats), "stats_dst", &d_stats)) return ALOAM_E_ARG;
  // ---- lay out the transform: what a (request, class) can hold at most is known without asking the device
  std::vector<GmRequest> rq((size_t)std::max(n, 1));
  std::vector<int> piece_first(2 * (size_t)n + 1, 0);
  long long bound_points = 0;
  int n_pieces = 0;
  const long long row[2] = {(long long)c->R * kLessSharpPerRing, (long long)c->cap};
  for (int r = 0; r < n; ++r) {
    rq[r] = GmRequest{req[r].seq, req[r].first, req[r].count, req[r].pose, {0, 0}};
    for (int cls = 0; cls < 2; ++cls) {
      const long long bound = std::min<long long>(c->kf.cap[cls], row[cls] * req[r].count);
      rq[r].at[cls] = bound_points;
      piece_first[2 * r + cls] = n_pieces;
      bound_points += bound;
      n_pieces += (int)((bound + kGmPiece - 1) / kGmPiece);
      if (n_pieces > (1 << 28)) { c->err = "the requests cover more than 2^40 keyframe points"; return ALOAM_E_ARG; }
    }
  }
  piece_first[2 * (size_t)n] = n_pieces;
  int rc;
  if ((rc = graph_map_scratch(c, bound_points))) return rc;
  if ((rc = c->gm.req.grow(c, (long long)std::max(n, 1)))) return rc;
  if ((rc = c->gm.req_out.grow(c, (long long)n + 1))) return rc;
  if ((rc = c->gm.ints.grow(c, 3LL * n + 2))) return rc;   // piece_first [2 n + 1], outside [n], flags [1]
  int* d_piece_first = c->gm.ints.get();
  int* d_outside = d_piece_first + 2 * (size_t)n + 1;
  int* d_flags = d_outside + n;
  if (n > 0) HIP_TRY(c, hipMemcpyAsync(c->gm.req.get(), rq.data(), sizeof(GmRequest) * (size_t)n, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(d_piece_first, piece_first.data(), sizeof(int) * piece_first.size(), hipMemcpyHostToDevice, c->stream));
  c->gm.last_segs = -1;                                    // the scratch of the last call's algorithmic bytes is about to be reused
  GmArgs g{};
  GmPasses passes;
  passes.transform = [&](unsigned dir_mask) {
    g = GmArgs{};
    g.n = n; g.req = c->gm.req.get(); g.piece_first = d_piece_first; g.n_pieces = n_pieces; g.kf = kf_store(c);
    g.nodes = c->pg.nodes.get(); g.max_nodes = c->pg.max_nodes;
    g.world = c->gm.world.get(); g.slot = c->gm.slot.get(); g.grouped = c->gm.grouped.get();
    g.dir_key = c->gm.dir_key.get(); g.dir_count = c->gm.dir_count.get(); g.dir_base = c->gm.dir_base.get(); g.dir_mask = dir_mask;
    g.outside = d_outside; g.flags = d_flags;
    launch_graph_map_transform(g, c->stream);
  };
  passes.group = [&] { launch_graph_map_group(g, c->stream); };
  GmDst dst{d_tiles, cap_tiles, d_pts, cap_points, d_off, d_stats};
  return graph_map_run(c, n, n_pieces, d_outside, d_flags, passes, dst, "request");
}

}  // extern "C"
