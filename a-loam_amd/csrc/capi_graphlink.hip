// a-loam_amd/csrc/capi_graphlink.hip — host side of the links measured on the device (aloam_graph_register_links /
// aloam_graph_search_links / aloam_graph_propose_links).  The two registrations are entry points of the one body in
// capi_loopreg.hip, which the per-sequence calls use: a link round differs in its checks, in the gather it launches and in what it stages.
// The proposal checks every argument and every query before anything is queued; the checked queries, each with its frame, go through a
// pinned staging ring of their own and run in rounds of as many as a slot holds, in stream order; nothing synchronises the host (a slot of
// the ring is waited for only when kProposeStageSlots later rounds have been queued behind it).  Nothing is allocated before the first
// call, and the graphs are only read.
#include <algorithm>
#include <cmath>

#include "capi_internal.hpp"

static_assert(sizeof(aloam_graph_link_request) == 96 && offsetof(aloam_graph_link_request, q) == 32 && offsetof(aloam_graph_loop_request, q) == 32,
              "the size include/aloam_mi355x.h states, and the guess where a loop request has it");
static_assert(kProposeHits % 64 == 0 && kProposeMaxK <= 64, "the list is filled a wave at a time; lane k of the first wave writes record k");

// The ring and the device copy of a round's queries, on first use; nothing stays allocated behind a refusal.
static int link_propose_staging(aloam_ctx* c) {
  if (c->lk.queries) return ALOAM_OK;
  if (dalloc(c->lk.queries, kProposeStageItems) == hipSuccess && !c->lk.query_ring.create(sizeof(LinkProposeQuery) * kProposeStageItems)) return ALOAM_OK;
  (void)hipGetLastError();
  c->lk.queries.reset();
  c->err = "link proposal: allocating the query ring failed";
  return ALOAM_E_HIP;
}

extern "C" {

int aloam_graph_register_links(aloam_ctx* c, const aloam_graph_link_request* req, int n, const aloam_graph_loop_options* opt, aloam_graph_loop_result* dst) {
  DeviceScope device_scope(c);
  if (!c) return ALOAM_E_ARG;
  return register_loops(c, nullptr, req, n, opt, dst, nullptr, false, nullptr, nullptr);
}

int aloam_graph_search_links(aloam_ctx* c, const aloam_graph_link_request* req, int n, const aloam_graph_loop_search* search, const aloam_graph_loop_options* opt,
                             aloam_graph_loop_result* dst, aloam_graph_loop_search_result* search_dst, aloam_map_score* scores) {
  DeviceScope device_scope(c);
  if (!c) return ALOAM_E_ARG;
  return register_loops(c, nullptr, req, n, opt, dst, search, true, search_dst, scores);
}

int aloam_graph_propose_links(aloam_ctx* c, const int* queries, const double* frames, int n, int pose, double radius_m, int half_window, int separation, int K,
                              aloam_graph_link_request* dst, int* counts, double* dist2) {
  DeviceScope device_scope(c);
  if (!c) return ALOAM_E_ARG;
  if (const int rc = require_graph(c)) return rc;
  // ---- everything is checked before anything is queued
  if (n < 0 || (n > 0 && !queries)) { c->err = "bad query list"; return ALOAM_E_ARG; }
  if (pose != ALOAM_GRAPH_POSE_ENTERED && pose != ALOAM_GRAPH_POSE_OPTIMIZED) { c->err = "pose must be ALOAM_GRAPH_POSE_ENTERED or ALOAM_GRAPH_POSE_OPTIMIZED"; return ALOAM_E_ARG; }
  if (!std::isfinite(radius_m) || radius_m < 0.0) { c->err = "radius_m must be finite and >= 0"; return ALOAM_E_ARG; }
  if (half_window < 0 || separation < 0 || K < 1 || K > kProposeMaxK) {
    c->err = "bad parameters (half_window >= 0, separation >= 0, 1 <= K <= " + std::to_string(kProposeMaxK) + ")";
    return ALOAM_E_ARG;
  }
  if (n == 0) return ALOAM_OK;
  if (const int rc = require_host_list(c, queries, "queries")) return rc;
  if (frames) if (const int rc = require_host_list(c, frames, "frames")) return rc;
  void *d_dst = nullptr, *d_counts = nullptr, *d_dist2 = nullptr;
  if (const int rc = export_target(c, dst, 8, "dst", &d_dst)) return rc;
  if (const int rc = export_target(c, counts, 4, "counts", &d_counts)) return rc;
  if (dist2) if (const int rc = export_target(c, dist2, 8, "dist2", &d_dist2)) return rc;
  std::vector<LinkProposeQuery> checked((size_t)n);
  for (int r = 0; r < n; ++r) {
    LinkProposeQuery& q = checked[r];
    auto fail = [&](const char* what) { c->err = "query " + std::to_string(r) + ": " + what; return ALOAM_E_ARG; };
    q = LinkProposeQuery{};
    q.seq_j = queries[3 * r]; q.j = queries[3 * r + 1]; q.seq_i = queries[3 * r + 2];
    if (q.seq_j < 0 || q.seq_j >= c->B) return fail("seq_j out of range");
    if (q.seq_i < 0 || q.seq_i >= c->B) return fail("seq_i out of range");
    if (q.seq_i == q.seq_j) return fail("seq_i and seq_j must differ (for one sequence there is aloam_graph_propose_loops)");
    if (q.j < 0 || q.j >= c->seq[q.seq_j].graph_nodes) return fail("j is not a node of seq_j's graph");
    q.nodes_i = c->seq[q.seq_i].graph_nodes;
    if (frames) {
      const double* f = frames + 7 * (size_t)r;
      double nn = 0.0;
      for (int a = 0; a < 4; ++a) { if (!std::isfinite(f[a])) return fail("the frame's q is not finite"); nn += f[a] * f[a]; }
      nn = std::sqrt(nn);
      if (!(std::fabs(nn - 1.0) <= 1e-6)) return fail("the frame's q is not within 1e-6 of unit norm");
      for (int a = 0; a < 4; ++a) q.frame[a] = f[a] / nn;
      for (int a = 0; a < 3; ++a) { if (!std::isfinite(f[4 + a])) return fail("the frame's t is not finite"); q.frame[4 + a] = f[4 + a]; }
      q.has_frame = 1;
    }
  }
  if (const int rc = link_propose_staging(c)) return rc;
  // ---- rounds of at most kProposeStageItems queries, in stream order
  ProfScope prof(c, K_POSE_GRAPH);
  for (int r0 = 0; r0 < n; r0 += kProposeStageItems) {
    const int m = std::min(kProposeStageItems, n - r0);
    LinkProposeQuery* slot = nullptr; int ns = 0;
    if (const int rc = c->lk.query_ring.acquire(c, &slot, &ns)) return rc;
    std::copy(checked.begin() + r0, checked.begin() + r0 + m, slot);
    if (const int rc = c->lk.query_ring.queue(c, ns, slot, sizeof(LinkProposeQuery) * (size_t)m, c->lk.queries.get(), c->stream)) return rc;
    LinkProposeArgs a{};
    a.n = m; a.queries = c->lk.queries.get(); a.nodes = c->pg.nodes.get(); a.max_nodes = c->pg.max_nodes;
    a.pose = pose; a.radius2 = radius_m * radius_m; a.half_window = half_window; a.separation = separation; a.K = K;
    a.dst = static_cast<aloam_graph_link_request*>(d_dst) + (size_t)r0 * K;
    a.counts = static_cast<int*>(d_counts) + r0;
    a.dist2 = d_dist2 ? static_cast<double*>(d_dist2) + (size_t)r0 * K : nullptr;
    launch_link_propose(a, c->stream);
  }
  HIP_TRY(c, hipGetLastError());
  return ALOAM_OK;
}

}  // extern "C"
