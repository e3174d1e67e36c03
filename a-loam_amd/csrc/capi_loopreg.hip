// a-loam_amd/csrc/capi_loopreg.hip — host side of the loop edges measured on the device (aloam_graph_loops_enable /
// aloam_graph_register_loops / aloam_graph_loop_export_target).  A request runs in a scratch slot; the slots are the
// "sequences" of a scratch MapArgs, so association, fit, solve and information are the launches of the mapping step over other buffers.
// Everything is checked before anything is queued; nothing synchronises the host (a slot of the pinned request ring is waited for only when
// kLoopStageSlots later rounds have been queued behind it).  aloam_graph_search_loops is the same call with a pose grid
// scored around every guess between the grid build and the first association (loopsearch_kernels.hip).
#include <algorithm>
#include <cmath>

#include "capi_internal.hpp"
#include "information_device.hpp"

static int require_loops(aloam_ctx* c) {
  if (!c->lr.on) { c->err = "loop registration is not enabled (aloam_graph_loops_enable)"; return ALOAM_E_STATE; }
  return ALOAM_OK;
}

// The scratch MapArgs of `n` slots: what launch_map_associate, launch_map_solve and launch_pose_information_map index by "sequence".
static MapArgs loop_map_args(aloam_ctx* c, int n, int lm_max_iterations) {
  MapArgs a{};
  a.B = n; a.cap = c->cap; a.R = c->R;
  a.seq = c->lr.seq.get();
  a.line_res = c->map_line_res; a.plane_res = c->map_plane_res;
  a.pool_cap = (int)std::max(c->lr.cap[0], c->lr.cap[1]);
  for (int k = 0; k < 2; ++k) { a.stack[k] = c->lr.stack[k].get(); a.grid_sorted[k] = c->lr.sorted[k].get(); a.grid_start[k] = c->lr.start[k].get(); }
  a.grid_H = c->lr.H;
  a.knn = c->lr.knn.get(); a.edges = c->lr.edges.get(); a.norms = c->lr.norms.get();
  a.lm_max_iterations = lm_max_iterations;
  a.rec_tiles = c->lr.rec_tiles.get(); a.rec_tiles_per_seq = c->rec_tiles_per_seq; a.rec_tiles_corner = c->rec_tiles_corner;
  a.active = nullptr;
  return a;
}

// The feature's own voxel-filter scratch (the mapping step's is in use by the live sequences' steps in the same stream).
static VoxArgs loop_vox_args(aloam_ctx* c, int n_segs) {
  VoxArgs v{};
  v.segs = c->lr.segs.get(); v.n_segs = n_segs; v.tile_seg = c->lr.tile_seg.get(); v.tile_heads = c->lr.tile_heads.get(); v.tile_pref = c->lr.tile_pref.get();
  v.counters = c->lr.vox_counters.get(); v.keys[0] = c->lr.keys[0].get(); v.keys[1] = c->lr.keys[1].get(); v.tmp = c->lr.voxtmp.get();
  v.bbox = c->lr.bbox.get(); v.tile_cap = c->lr.tile_cap; v.key_cap = c->lr.key_cap; v.levels = c->lr.levels; v.lists = c->lr.vox_lists.get();
  return v;
}

extern "C" {

void aloam_graph_loop_default_options(aloam_graph_loop_options* opt) {
  if (!opt) return;
  opt->outer_iterations = 2; opt->lm_max_iterations = 4;
}

int aloam_graph_loops_enable(aloam_ctx* c, int max_requests, int max_target_corner_points, int max_target_surf_points) {
  DeviceScope device_scope(c);
  if (!c) return ALOAM_E_ARG;
  if (!c->kf.on) { c->err = "aloam_graph_loops_enable before aloam_graph_keyframes_enable"; return ALOAM_E_STATE; }
  if (c->lr.on) { c->err = "loop registration already enabled"; return ALOAM_E_STATE; }
  if (max_requests < 1 || max_requests > kLoopMaxRequests || max_target_corner_points < 1 || max_target_corner_points > kLoopTargetMax || max_target_surf_points < 1 ||
      max_target_surf_points > kLoopTargetMax) {
    c->err = "bad loop registration sizes (1 <= max_requests <= 32768, 1 <= max_target_corner_points, max_target_surf_points <= 2^24)";
    return ALOAM_E_ARG;
  }
  const size_t S = (size_t)max_requests, cap = c->cap, rowc = (size_t)c->R * kLessSharpPerRing, T = kVoxTile;
  const size_t tc[2] = {(size_t)max_target_corner_points, (size_t)max_target_surf_points}, pool = std::max(tc[0], tc[1]);
  int H = 4096, levels = 0;
  while (H < (int)(pool / 16) && H < kMapGridMaxH) H <<= 1;
  while ((T << levels) < pool) ++levels;
  // the general path of the voxel filter takes whatever the single-workgroup filters pass on (more runs than their tables hold): sized for all of it
  const size_t key_cap = S * (tc[0] + tc[1]), tile_cap = S * ((tc[0] + T - 1) / T + (tc[1] + T - 1) / T);
  if (tile_cap > 0x7fffffffu) { c->err = "loop registration scratch: more voxel-filter tiles than an int counts"; return ALOAM_E_ARG; }
  LoopScratch l;                       // committed with one move: nothing stays allocated behind a refusal
  bool ok = true;
  const char* cause = "device allocation failed";
  auto grab = [&](auto& p, size_t count) { if (ok && dalloc(p, count) != hipSuccess) { ok = false; (void)hipGetLastError(); } };
  for (int k = 0; k < 2; ++k) {
    grab(l.raw[k], S * tc[k]); grab(l.target[k], S * tc[k]); grab(l.sorted[k], S * pool); grab(l.start[k], S * ((size_t)H + 1));
    grab(l.stack[k], S * (k == 0 ? rowc : cap)); grab(l.keys[k], key_cap);
  }
  grab(l.voxtmp, key_cap); grab(l.tile_seg, tile_cap); grab(l.tile_heads, tile_cap); grab(l.tile_pref, tile_cap + 1);
  grab(l.req, S); grab(l.knn, S * cap * 4); grab(l.edges, S * rowc); grab(l.norms, S * cap);
  grab(l.rec_tiles, S * (size_t)c->rec_tiles_per_seq); grab(l.seq, S); grab(l.plan, S * kLoopPlanInts); grab(l.list, S);
  grab(l.segs, 2 * S); grab(l.vox_lists, 3 * 2 * S); grab(l.vox_counters, 8); grab(l.bbox, 2 * S * 6); grab(l.info, S);
  if (ok) if (const char* what = l.ring.create(sizeof(aloam_graph_loop_request) * S)) { ok = false; cause = what; }
  if (ok && prepare_loop_grid(H) != 0) { ok = false; cause = "k_loop_grid: dynamic LDS size rejected"; }
  if (ok) {
    // every slot counts as solved for k_pose_information_map: a slot whose gate is false holds no record and comes back without factors
    std::vector<int> list(S);
    for (size_t s = 0; s < S; ++s) list[s] = (int)s | kInfoSolvedBit;
    ok = hipMemcpyAsync(l.list.get(), list.data(), sizeof(int) * S, hipMemcpyHostToDevice, c->stream) == hipSuccess &&
         hipMemsetAsync(l.vox_counters.get(), 0, 8 * sizeof(int), c->stream) == hipSuccess &&
         hipMemsetAsync(l.seq.get(), 0, sizeof(MapSeq) * S, c->stream) == hipSuccess &&
         hipMemsetAsync(l.plan.get(), 0, sizeof(int) * S * kLoopPlanInts, c->stream) == hipSuccess &&
         hipStreamSynchronize(c->stream) == hipSuccess;                          // (list is a local)
    if (!ok) cause = "initialising the scratch failed";
  }
  if (!ok) {
    (void)hipGetLastError();
    c->err = "loop registration scratch of " + std::to_string(max_requests) + " slots: " + cause;
    return ALOAM_E_HIP;
  }
  l.slots = max_requests; l.H = H; l.levels = levels; l.cap[0] = (long long)tc[0]; l.cap[1] = (long long)tc[1];
  l.key_cap = (long long)key_cap; l.tile_cap = (int)tile_cap; l.tile_bound = (int)std::max<size_t>(tile_cap, 1);
  l.on = true;
  c->lr = std::move(l);
  return ALOAM_OK;
}

void aloam_graph_loop_default_search(aloam_graph_loop_search* s) {
  if (!s) return;
  s->radius_m = 3.0; s->step_m = 0.5; s->yaw_deg = 12.5; s->yaw_step_deg = 2.5;
}

// What a searched call adds to a plain one: the grid with its yaw table, and where the search record and the score table go.
struct LoopSearchCall {
  LoopSearchGrid grid;
  void* d_search = nullptr;            // aloam_graph_loop_search_result [n], as the device reaches it
  void* d_scores = nullptr;            // aloam_map_score [n][K] or nullptr
};

// The axes and the yaw table of a grid (a-loam_amd/loopreg.py search_grid restates this); ALOAM_E_ARG for what cannot be searched.
static int loop_search_grid(aloam_ctx* c, const aloam_graph_loop_search& s, LoopSearchGrid* g) {
  const double v[4] = {s.radius_m, s.step_m, s.yaw_deg, s.yaw_step_deg};
  for (double x : v) if (!std::isfinite(x) || x < 0.0) { c->err = "the search grid's values must be finite and >= 0"; return ALOAM_E_ARG; }
  const double md = s.step_m > 0.0 ? std::floor(s.radius_m / s.step_m + 1e-9) : 0.0;
  const double ad = s.yaw_step_deg > 0.0 ? std::floor(s.yaw_deg / s.yaw_step_deg + 1e-9) : 0.0;
  if (!(ad <= (double)kLoopSearchMaxYaw)) { c->err = "the search grid has more than 31 yaw steps to either side"; return ALOAM_E_ARG; }
  if (!(md <= 64.0)) { c->err = "the search grid has more than 2^14 nodes"; return ALOAM_E_ARG; }
  const int m = (int)md, a = (int)ad;
  const long long K = (long long)(2 * a + 1) * (2 * m + 1) * (2 * m + 1);
  if (K < 1 || K > kLoopSearchMaxNodes) { c->err = "the search grid has more than 2^14 nodes"; return ALOAM_E_ARG; }
  *g = LoopSearchGrid{};
  g->m = m; g->a = a; g->K = (int)K; g->step_m = s.step_m;
  for (int iyaw = -a; iyaw <= a; ++iyaw) {
    const double dyaw = (double)iyaw * s.yaw_step_deg;
    const double h = (dyaw * (M_PI / 180.0)) / 2;
    g->half[iyaw + a][0] = std::sin(h); g->half[iyaw + a][1] = std::cos(h);
  }
  return ALOAM_OK;
}

}  // extern "C"

// What a loop request and a link request share: the target window and node i against the node count of the sequence that holds the
// target (seq for a loop, seq_i for a link, which the message names), a loop's node j (a link's lives in seq_j: check_link), pose, and
// the guess, whose q is normalised in place as aloam_graph_add_edges does.  nullptr, or what is wrong.
static const char* check_target_and_guess(int first, int count, int i, int j, long long nodes, int pose, double q[4], const double t[3], bool link) {
  if (first < 0 || count < 1 || first + (long long)count > nodes)
    return link ? "need count >= 1 and [first, first + count) inside what seq_i's graph holds" : "need count >= 1 and [first, first + count) inside what the sequence's graph holds";
  if (i < first || i >= first + (long long)count) return "node i must be one of the target nodes (first <= i < first + count)";
  if (!link && (j < 0 || j >= nodes || (j >= first && j < first + (long long)count))) return "node j must be a node outside [first, first + count)";
  if (pose != ALOAM_GRAPH_POSE_ENTERED && pose != ALOAM_GRAPH_POSE_OPTIMIZED) return "pose must be ALOAM_GRAPH_POSE_ENTERED or ALOAM_GRAPH_POSE_OPTIMIZED";
  double nn = 0.0;
  for (int a = 0; a < 4; ++a) { if (!std::isfinite(q[a])) return "the guess q is not finite"; nn += q[a] * q[a]; }
  nn = std::sqrt(nn);
  if (!(std::fabs(nn - 1.0) <= 1e-6)) return "the guess q is not within 1e-6 of unit norm";
  for (int a = 0; a < 3; ++a) if (!std::isfinite(t[a])) return "the guess t is not finite";
  for (int a = 0; a < 4; ++a) q[a] /= nn;
  return nullptr;
}

// A link request: both sequences, j against seq_j's nodes, the rest against seq_i's; there is no "j outside the window" rule.  On success
// the record is as it is staged for k_link_gather: the guess normalised, pad and reserved zero.
static const char* check_link(const aloam_ctx* c, aloam_graph_link_request& l) {
  if (l.seq_i < 0 || l.seq_i >= c->B) return "seq_i out of range";
  if (l.seq_j < 0 || l.seq_j >= c->B) return "seq_j out of range";
  if (l.seq_i == l.seq_j) return "seq_i and seq_j must differ (for one sequence there is aloam_graph_register_loops)";
  if (l.j < 0 || l.j >= c->seq[l.seq_j].graph_nodes) return "node j must be a node of seq_j's graph";
  if (const char* what = check_target_and_guess(l.first, l.count, l.i, l.j, c->seq[l.seq_i].graph_nodes, l.pose, l.q, l.t, true)) return what;
  l.pad = 0; l.reserved = 0.0;
  return nullptr;
}

// The loop request the kernels behind the gather read for a checked link: the frame's sequence, the indices and the normalised guess.
static aloam_graph_loop_request loop_request_of(const aloam_graph_link_request& l) {
  aloam_graph_loop_request q{};
  q.seq = l.seq_i; q.i = l.i; q.j = l.j; q.first = l.first; q.count = l.count; q.pose = l.pose;
  for (int a = 0; a < 4; ++a) q.q[a] = l.q[a];
  for (int a = 0; a < 3; ++a) q.t[a] = l.t[a];
  return q;
}

// The staging of a link call's records (aloam_graph_register_links / aloam_graph_search_links), on first use: a ring whose slots hold as many
// records as the request ring's, and the round's device copy.  Nothing stays allocated behind a refusal.
static int link_staging(aloam_ctx* c) {
  if (c->lk.req) return ALOAM_OK;
  if (dalloc(c->lk.req, (size_t)c->lr.slots) == hipSuccess && !c->lk.ring.create(sizeof(aloam_graph_link_request) * (size_t)c->lr.slots)) return ALOAM_OK;
  (void)hipGetLastError();
  c->lk.req.reset();
  c->err = "link registration: allocating the staging of " + std::to_string(c->lr.slots) + " link records failed";
  return ALOAM_E_HIP;
}

// aloam_graph_register_loops (search == nullptr) and aloam_graph_search_loops: checks, ring, gather, filter, grid, then search and pick when a
// grid is given, rounds, information, result.  The plain call queues exactly the launches it queued before the search existed.
// aloam_graph_register_links / aloam_graph_search_links (capi_graphlink.hip) come through here with `links` in place of `req`: a link round
// differs in its checks, in which gather is launched and in what is staged - the link records for k_link_gather, and plain loop requests
// (seq = seq_i, the normalised guess) for the kernels behind it, which read nothing of a request but its guess.
int aloam::register_loops(aloam_ctx* c, const aloam_graph_loop_request* req, const aloam_graph_link_request* links, int n, const aloam_graph_loop_options* opt,
                          aloam_graph_loop_result* dst, const aloam_graph_loop_search* search_or_default, bool searched, aloam_graph_loop_search_result* search_dst,
                          aloam_map_score* scores) {
  if (const int rc = require_loops(c)) return rc;
  // ---- everything is checked before anything is queued
  const bool linked = links != nullptr;
  if (n < 0 || (n > 0 && !req && !linked)) { c->err = "bad request list"; return ALOAM_E_ARG; }
  aloam_graph_loop_options o;
  aloam_graph_loop_default_options(&o);
  if (opt) o = *opt;
  if (o.outer_iterations < 1 || o.lm_max_iterations < 0) { c->err = "need outer_iterations >= 1 and lm_max_iterations >= 0"; return ALOAM_E_ARG; }
  LoopSearchCall sc;
  if (searched) {
    aloam_graph_loop_search g;
    aloam_graph_loop_default_search(&g);
    if (search_or_default) g = *search_or_default;
    if (const int rc = loop_search_grid(c, g, &sc.grid)) return rc;
  }
  if (n == 0) return ALOAM_OK;
  if (const int rc = require_host_list(c, linked ? (const void*)links : (const void*)req, "req")) return rc;
  void* d_dst = nullptr;
  if (const int rc = export_target(c, dst, 8, "dst", &d_dst)) return rc;
  if (searched) {
    if (const int rc = export_target(c, search_dst, 8, "search_dst", &sc.d_search)) return rc;
    if (scores) if (const int rc = export_target(c, scores, 8, "scores", &sc.d_scores)) return rc;
  }
  std::vector<aloam_graph_loop_request> checked(linked ? (size_t)n : 0);
  if (!linked) checked.assign(req, req + n);
  std::vector<aloam_graph_link_request> checked_links(links, links + (linked ? n : 0));
  for (int r = 0; r < n; ++r) {
    const char* what = nullptr;
    if (linked) {
      what = check_link(c, checked_links[r]);
      if (!what) checked[r] = loop_request_of(checked_links[r]);
    } else {
      aloam_graph_loop_request& q = checked[r];
      if (q.seq < 0 || q.seq >= c->B) what = "seq out of range";
      else what = check_target_and_guess(q.first, q.count, q.i, q.j, c->seq[q.seq].graph_nodes, q.pose, q.q, q.t, false);
      q.pad[0] = 0; q.pad[1] = 0; q.reserved = 0.0;
    }
    if (what) { c->err = "request " + std::to_string(r) + ": " + what; return ALOAM_E_ARG; }
  }
  if (linked) if (const int rc = link_staging(c)) return rc;
  // ---- rounds of at most lr_slots requests (searched: and at most 2^18 (slot, node) pairs) over the same scratch, in stream order
  const int per_round = searched ? (int)std::min<long long>(c->lr.slots, kLoopSearchMaxPairs / sc.grid.K) : c->lr.slots;
  if (searched)
    if (const int rc = c->lr.search_part.grow(c, (long long)std::min(per_round, n) * sc.grid.K * kLoopSearchParts)) {
      (void)hipGetLastError();
      c->err = "search scratch of " + std::to_string(std::min(per_round, n)) + " x " + std::to_string(sc.grid.K) + " (request, node) pairs: device allocation failed";
      return rc;
    }
  ProfScope prof(c, K_LOOP_REGISTER);
  // A slot of the pinned ring holds lr_slots requests: one round of the plain call, as many whole rounds of a searched call as fit (its
  // rounds are the shorter of the two bounds), so that a searched call waits for the ring no sooner than a plain call of the same n.
  aloam_graph_loop_request* ring_slot = nullptr; int ns = 0, ring_at = 0, ring_left = 0;
  aloam_graph_link_request* link_slot = nullptr; int link_ns = 0;           // a link call's second ring, acquired in step with the first
  for (int r0 = 0; r0 < n; r0 += per_round) {
    const int m = std::min(per_round, n - r0);
    if (ring_left < m) {
      if (const int rc = c->lr.ring.acquire(c, &ring_slot, &ns)) return rc;
      if (linked) if (const int rc = c->lk.ring.acquire(c, &link_slot, &link_ns)) return rc;
      ring_at = 0; ring_left = c->lr.slots;
    }
    aloam_graph_loop_request* slot = ring_slot + ring_at;
    if (linked) {
      aloam_graph_link_request* ls = link_slot + ring_at;
      std::copy(checked_links.begin() + r0, checked_links.begin() + r0 + m, ls);
      if (const int rc = c->lk.ring.queue(c, link_ns, ls, sizeof(aloam_graph_link_request) * (size_t)m, c->lk.req.get(), c->stream)) return rc;
    }
    ring_at += m; ring_left -= m;
    std::copy(checked.begin() + r0, checked.begin() + r0 + m, slot);
    if (const int rc = c->lr.ring.queue(c, ns, slot, sizeof(aloam_graph_loop_request) * (size_t)m, c->lr.req.get(), c->stream)) return rc;
    LoopArgs a{};
    a.n = m; a.req = c->lr.req.get();
    a.kf = kf_store(c);
    a.nodes = c->pg.nodes.get(); a.max_nodes = c->pg.max_nodes;
    a.map = loop_map_args(c, m, o.lm_max_iterations);
    for (int k = 0; k < 2; ++k) { a.raw[k] = c->lr.raw[k].get(); a.raw_cap[k] = c->lr.cap[k]; a.target[k] = c->lr.target[k].get(); }
    a.plan = c->lr.plan.get(); a.outer_iterations = o.outer_iterations;
    a.info = c->lr.info.get(); a.dst = static_cast<aloam_graph_loop_result*>(d_dst) + r0;
    const VoxArgs v = loop_vox_args(c, 2 * m);
    HIP_TRY(c, hipMemsetAsync(c->lr.vox_counters.get() + 4, 0, 4 * sizeof(int), c->stream));   // general-path count, the three LDS-filter lists
    if (linked) {
      LinkGatherArgs g{};
      g.n = m; g.req = c->lk.req.get(); g.kf = a.kf; g.nodes = a.nodes; g.max_nodes = a.max_nodes; g.map = a.map;
      for (int k = 0; k < 2; ++k) { g.raw[k] = a.raw[k]; g.raw_cap[k] = a.raw_cap[k]; g.target[k] = a.target[k]; }
      g.plan = a.plan; g.plan_ints = kLoopPlanInts;
      launch_link_gather(g, v, c->stream);
    } else {
      launch_loop_gather(a, v, c->stream);
    }
    launch_voxel_filter(v, c->lr.tile_bound, c->stream);   // always the input-order sum, whatever aloam_set_voxel_sum_order says
    launch_loop_grid(a, c->stream);
    if (searched) {
      LoopSearchArgs sa{};
      sa.n = m;
      sa.splits = m < 8 ? std::max(1, std::min(8 / m, sc.grid.K)) : 1;   // fewer than 8 slots: their nodes are dealt over the XCDs left idle
      sa.kper = (sc.grid.K + sa.splits - 1) / sa.splits;
      sa.req = a.req; sa.map = a.map; sa.plan = a.plan; sa.plan_ints = kLoopPlanInts; sa.grid = sc.grid; sa.part = c->lr.search_part.get();
      sa.scores = sc.d_scores ? static_cast<aloam_map_score*>(sc.d_scores) + (size_t)r0 * sc.grid.K : nullptr;
      sa.dst = static_cast<aloam_graph_loop_search_result*>(sc.d_search) + r0;
      launch_loop_search(sa, c->stream);
    }
    for (int it = 0; it < o.outer_iterations; ++it) {
      launch_map_associate(a.map, it, c->stream);
      launch_map_solve(a.map, it & 1, false, c->stream);   // no transformUpdate: a slot has no odometry frame
    }
    launch_pose_information_map(a.map, c->lr.list.get(), m, c->lr.info.get(), c->stream);
    launch_loop_result(a, c->stream);
  }
  HIP_TRY(c, hipGetLastError());
  return ALOAM_OK;
}

extern "C" {

int aloam_graph_register_loops(aloam_ctx* c, const aloam_graph_loop_request* req, int n, const aloam_graph_loop_options* opt, aloam_graph_loop_result* dst) {
  DeviceScope device_scope(c);
  if (!c) return ALOAM_E_ARG;
  return register_loops(c, req, nullptr, n, opt, dst, nullptr, false, nullptr, nullptr);
}

int aloam_graph_search_loops(aloam_ctx* c, const aloam_graph_loop_request* req, int n, const aloam_graph_loop_search* search, const aloam_graph_loop_options* opt,
                             aloam_graph_loop_result* dst, aloam_graph_loop_search_result* search_dst, aloam_map_score* scores) {
  DeviceScope device_scope(c);
  if (!c) return ALOAM_E_ARG;
  return register_loops(c, req, nullptr, n, opt, dst, search, true, search_dst, scores);
}

int aloam_graph_loop_export_target(aloam_ctx* c, int slot, int feature_class, float* dst_xyzw, long long cap, int* count) {
  DeviceScope device_scope(c);
  if (!c) return ALOAM_E_ARG;
  if (const int rc = require_loops(c)) return rc;
  if (slot < 0 || slot >= c->lr.slots) { c->err = "slot out of range"; return ALOAM_E_ARG; }
  if (feature_class < 0 || feature_class > 1) { c->err = "feature_class must be 0 (corner) or 1 (surf)"; return ALOAM_E_ARG; }
  if (cap < 0) { c->err = "negative cap"; return ALOAM_E_ARG; }
  void *d_cnt = nullptr, *d_pts = nullptr;
  if (const int rc = export_target(c, count, alignof(int), "count", &d_cnt)) return rc;
  if ((dst_xyzw || cap > 0) && export_target(c, dst_xyzw, 16, "dst", &d_pts)) return ALOAM_E_ARG;
  launch_loop_export_target(c->lr.seq.get() + slot, feature_class, c->lr.target[feature_class].get() + (size_t)slot * c->lr.cap[feature_class],
                            static_cast<float4*>(d_pts), d_pts ? cap : 0, static_cast<int*>(d_cnt), c->stream);
  HIP_TRY(c, hipGetLastError());
  return ALOAM_OK;
}

}  // extern "C"
