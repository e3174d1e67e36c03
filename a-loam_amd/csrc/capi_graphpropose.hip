// a-loam_amd/csrc/capi_graphpropose.hip — host side of the loop proposal by pose proximity (aloam_graph_propose_loops).  Every
// argument and every query is checked before anything is queued; the checked queries go through a pinned staging ring of their own and run
// in rounds of as many as a slot holds, in stream order; nothing synchronises the host (a slot of the ring is waited for only when
// kProposeStageSlots later rounds have been queued behind it).  Nothing is allocated before the first call, and the graph is only read.
#include <algorithm>
#include <cmath>

#include "capi_internal.hpp"

static_assert(sizeof(GraphProposeQuery) == 2 * sizeof(int), "a query is the caller's (seq, j)");
static_assert(sizeof(aloam_graph_loop_request) == 96, "the size include/aloam_mi355x.h states");
static_assert(kProposeHits % 64 == 0 && kProposeMaxK <= 64, "the list is filled a wave at a time; lane k of the first wave writes record k");

// The ring and the device copy of a round's queries, on first use; nothing stays allocated behind a refusal.
static int propose_staging(aloam_ctx* c) {
  if (c->pp.queries) return ALOAM_OK;
  if (dalloc(c->pp.queries, kProposeStageItems) == hipSuccess && !c->pp.ring.create(sizeof(GraphProposeQuery) * kProposeStageItems)) return ALOAM_OK;
  (void)hipGetLastError();
  c->pp.queries.reset();
  c->err = "loop proposal: allocating the query ring failed";
  return ALOAM_E_HIP;
}

extern "C" {

int aloam_graph_propose_loops(aloam_ctx* c, const int* queries, int n, int pose, double radius_m, double growth_m_per_node, int min_gap, int half_window,
                              int separation, int K, aloam_graph_loop_request* dst, int* counts, double* dist2) {
  DeviceScope device_scope(c);
  if (!c) return ALOAM_E_ARG;
  if (const int rc = require_graph(c)) return rc;
  // ---- everything is checked before anything is queued
  if (n < 0 || (n > 0 && !queries)) { c->err = "bad query list"; return ALOAM_E_ARG; }
  if (pose != ALOAM_GRAPH_POSE_ENTERED && pose != ALOAM_GRAPH_POSE_OPTIMIZED) { c->err = "pose must be ALOAM_GRAPH_POSE_ENTERED or ALOAM_GRAPH_POSE_OPTIMIZED"; return ALOAM_E_ARG; }
  if (!std::isfinite(radius_m) || radius_m < 0.0 || !std::isfinite(growth_m_per_node) || growth_m_per_node < 0.0) {
    c->err = "radius_m and growth_m_per_node must be finite and >= 0";
    return ALOAM_E_ARG;
  }
  if (min_gap < 1 || half_window < 0 || half_window >= min_gap || separation < 0 || K < 1 || K > kProposeMaxK) {
    c->err = "bad parameters (min_gap >= 1, 0 <= half_window < min_gap, separation >= 0, 1 <= K <= " + std::to_string(kProposeMaxK) + ")";
    return ALOAM_E_ARG;
  }
  if (n == 0) return ALOAM_OK;
  if (const int rc = require_host_list(c, queries, "queries")) return rc;
  void *d_dst = nullptr, *d_counts = nullptr, *d_dist2 = nullptr;
  if (const int rc = export_target(c, dst, 8, "dst", &d_dst)) return rc;
  if (const int rc = export_target(c, counts, 4, "counts", &d_counts)) return rc;
  if (dist2) if (const int rc = export_target(c, dist2, 8, "dist2", &d_dist2)) return rc;
  const GraphProposeQuery* qs = reinterpret_cast<const GraphProposeQuery*>(queries);
  for (int r = 0; r < n; ++r) {
    if (const int rc = check_seq(c, qs[r].seq)) { c->err = "query " + std::to_string(r) + ": " + c->err; return rc; }
    if (qs[r].j < 0 || qs[r].j >= c->seq[qs[r].seq].graph_nodes) { c->err = "query " + std::to_string(r) + ": j is not a node of the sequence's graph"; return ALOAM_E_ARG; }
  }
  if (const int rc = propose_staging(c)) return rc;
  // ---- rounds of at most kProposeStageItems queries, in stream order
  ProfScope prof(c, K_POSE_GRAPH);
  for (int r0 = 0; r0 < n; r0 += kProposeStageItems) {
    const int m = std::min(kProposeStageItems, n - r0);
    GraphProposeQuery* slot = nullptr; int ns = 0;
    if (const int rc = c->pp.ring.acquire(c, &slot, &ns)) return rc;
    std::copy(qs + r0, qs + r0 + m, slot);
    if (const int rc = c->pp.ring.queue(c, ns, slot, sizeof(GraphProposeQuery) * (size_t)m, c->pp.queries.get(), c->stream)) return rc;
    GraphProposeArgs a{};
    a.n = m; a.queries = c->pp.queries.get(); a.nodes = c->pg.nodes.get(); a.max_nodes = c->pg.max_nodes;
    a.pose = pose; a.radius_m = radius_m; a.growth_m_per_node = growth_m_per_node;
    a.min_gap = min_gap; a.half_window = half_window; a.separation = separation; a.K = K;
    a.dst = static_cast<aloam_graph_loop_request*>(d_dst) + (size_t)r0 * K;
    a.counts = static_cast<int*>(d_counts) + r0;
    a.dist2 = d_dist2 ? static_cast<double*>(d_dist2) + (size_t)r0 * K : nullptr;
    launch_graph_propose(a, c->stream);
  }
  HIP_TRY(c, hipGetLastError());
  return ALOAM_OK;
}

}  // extern "C"
