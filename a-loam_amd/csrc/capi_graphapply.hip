// a-loam_amd/csrc/capi_graphapply.hip — host side of aloam_graph_apply: a solved pose graph carried into the live pose and
// the window map of its sequence.  With ALOAM_GRAPH_APPLY_MAP the map of the listed nodes is made by aloam_graph_export_map's own transform,
// group and filter passes into the context's scratch (no tiles or points are emitted); the host then reads back the filtered size of every
// (request, class, cube), grows the map pools when the largest window of a map exceeds a pool row, and queues k_graph_apply.  Keyframe
// points never pass through host memory.
#include <algorithm>

#include "capi_internal.hpp"

extern "C" {

int aloam_graph_apply(aloam_ctx* c, const aloam_graph_apply_request* req, int n, aloam_graph_apply_result* dst) {
  DeviceScope device_scope(c);
  if (!c) return ALOAM_E_ARG;
  // ---- everything is checked before anything is queued
  if (!c->pg.on) { c->err = "aloam_graph_apply before aloam_graph_enable"; return ALOAM_E_STATE; }
  if (!c->map_on) { c->err = "aloam_graph_apply before aloam_mapping_enable"; return ALOAM_E_STATE; }
  if (n < 0 || n > c->B || (n > 0 && !req)) { c->err = "bad request list (0 <= n <= batch)"; return ALOAM_E_ARG; }
  if (n == 0) return ALOAM_OK;
  if (const int rc = require_host_list(c, req, "req")) return rc;
  std::vector<char> listed((size_t)c->B, 0);
  bool any_map = false;
  for (int r = 0; r < n; ++r) {
    const aloam_graph_apply_request& q = req[r];
    auto fail = [&](const char* what) { c->err = "request " + std::to_string(r) + ": " + what; return ALOAM_E_ARG; };
    if (q.seq < 0 || q.seq >= c->B) return fail("seq out of range");
    if (listed[(size_t)q.seq]) return fail("sequence listed twice");
    listed[(size_t)q.seq] = 1;
    if (q.first < 0 || q.count < 0 || q.first + (long long)q.count > c->seq[q.seq].graph_nodes) return fail("[first, first + count) must lie inside what the sequence's graph holds");
    if (q.flags != ALOAM_GRAPH_APPLY_POSE && q.flags != (ALOAM_GRAPH_APPLY_POSE | ALOAM_GRAPH_APPLY_MAP)) return fail("flags must be ALOAM_GRAPH_APPLY_POSE or ALOAM_GRAPH_APPLY_POSE | ALOAM_GRAPH_APPLY_MAP");
    any_map |= (q.flags & ALOAM_GRAPH_APPLY_MAP) != 0;
  }
  if (any_map && !c->kf.on) { c->err = "ALOAM_GRAPH_APPLY_MAP before aloam_graph_keyframes_enable"; return ALOAM_E_STATE; }
  for (int r = 0; r < n; ++r) {
    const SeqHost& s = c->seq[req[r].seq];
    if (s.frozen || s.attached) {
      c->err = "sequence " + std::to_string(req[r].seq) + " is " + (s.attached ? "attached to the atlas" : "frozen") + ": its map is not its own";
      return ALOAM_E_STATE;
    }
  }
  void* d_dst = nullptr;
  if (const int rc = export_target(c, dst, alignof(aloam_graph_apply_result), "dst", &d_dst)) return rc;
  // ---- the items, and the map of every request that wants one
  std::vector<GaItem> items((size_t)n);
  std::vector<aloam_graph_map_request> maps;
  std::vector<int> seqs((size_t)n);
  for (int r = 0; r < n; ++r) {
    const aloam_graph_apply_request& q = req[r];
    const int nodes = c->seq[q.seq].graph_nodes;
    const bool with_map = (q.flags & ALOAM_GRAPH_APPLY_MAP) != 0 && nodes > 0;
    items[(size_t)r] = GaItem{q.seq, q.first, q.count, with_map ? q.flags : ALOAM_GRAPH_APPLY_POSE, nodes, with_map ? (int)maps.size() : -1, {0, 0}};
    if (with_map) maps.push_back(aloam_graph_map_request{q.seq, q.first, q.count, ALOAM_GRAPH_POSE_OPTIMIZED});
    seqs[(size_t)r] = q.seq;
  }
  int rc;
  if ((rc = c->ga.items.grow(c, c->B))) return rc;
  const int n_maps = (int)maps.size();
  if (n_maps > 0) {
    if ((rc = c->ga.off.grow(c, 2LL * c->B + 2))) return rc;
    // transform, group, filter and offsets into the scratch of the map pass; nothing is emitted (caps of 0).  Synchronises.
    if ((rc = aloam_graph_export_map(c, maps.data(), n_maps, nullptr, 0, nullptr, 0, c->ga.off.get(), nullptr))) return rc;
    // One more synchronisation: the filtered size of every (request, class, cube) comes back.  Where the sensor will be is known on the
    // device only, so a pool row is sized for the largest 21 x 21 x 11 box of each map (the sliding sums of aloam_atlas_load).
    const int n_segs = c->gm.last_segs;
    std::vector<GmRequestOut> out((size_t)n_maps + 1);
    std::vector<GmSegInfo> seg((size_t)std::max(n_segs, 0));
    std::vector<int> cnt(seg.size());
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipMemcpy(out.data(), c->gm.req_out.get(), sizeof(GmRequestOut) * out.size(), hipMemcpyDeviceToHost));
    if (n_segs > 0) {
      HIP_TRY(c, hipMemcpy(seg.data(), c->gm.seg.get(), sizeof(GmSegInfo) * seg.size(), hipMemcpyDeviceToHost));
      HIP_TRY(c, hipMemcpy(cnt.data(), c->gm.counts.get(), sizeof(int) * cnt.size(), hipMemcpyDeviceToHost));
    }
    long long need[2] = {0, 0};
    for (int m = 0; m < n_maps; ++m)
      for (int cls = 0; cls < 2; ++cls) {
        const int s0 = cls ? out[(size_t)m].surf_first : out[(size_t)m].seg_first, s1 = cls ? out[(size_t)m + 1].seg_first : out[(size_t)m].surf_first;
        std::vector<int> keys, counts;
        int lo[3] = {kAtlasBias, kAtlasBias, kAtlasBias}, hi[3] = {-kAtlasBias, -kAtlasBias, -kAtlasBias};
        for (int s = s0; s < s1; ++s) {
          const int key = seg[(size_t)s].cube_key, xyz[3] = {(key >> 20) - kAtlasBias, ((key >> 10) & 1023) - kAtlasBias, (key & 1023) - kAtlasBias};
          for (int k = 0; k < 3; ++k) { lo[k] = std::min(lo[k], xyz[k]); hi[k] = std::max(hi[k], xyz[k]); }
          keys.push_back(key); counts.push_back(cnt[(size_t)s]);
        }
        bool exact = true;
        need[cls] = std::max(need[cls], largest_window(keys, counts, lo, hi, &exact));
      }
    const long long want = std::max(need[0], need[1]);
    if (want > c->map.points && (rc = grow_map_pool(c, want, false))) {
      if (rc == ALOAM_E_CAPACITY) c->err = "the map of the listed nodes (a window of " + std::to_string(want) + " points of one class) exceeds the pool limit";
      return rc;
    }
    for (int k = 0; k < 2; ++k) c->h_map_report[1 + k] = std::max((int)c->h_map_report[1 + k], (int)need[k]);   // the pools are sized from this until the next step reports
  }
  // ---- from here everything is stream-ordered
  HIP_TRY(c, hipMemcpyAsync(c->ga.items.get(), items.data(), sizeof(GaItem) * items.size(), hipMemcpyHostToDevice, c->stream));
  GraphApplyArgs a{};
  a.n = n; a.items = c->ga.items.get();
  a.nodes = c->pg.nodes.get(); a.max_nodes = c->pg.max_nodes;
  a.seq = c->d_mapseq.get(); a.cubes = c->d_cubes.get();
  a.pool[0] = c->map.pool[0].get(); a.pool[1] = c->map.pool[1].get(); a.pool_cap = c->map.points;
  a.req = c->gm.req_out.get(); a.jobs = c->gm.jobs.get(); a.seg = c->gm.seg.get(); a.counts = c->gm.counts.get(); a.grouped = c->gm.grouped.get();
  a.dst = static_cast<aloam_graph_apply_result*>(d_dst);
  {
    ProfScope p(c, K_GRAPH_MAP);
    launch_graph_apply(a, c->stream);
  }
  HIP_TRY(c, hipGetLastError());
  return on_graph_applied(c, seqs.data(), n);
}

}  // extern "C"
