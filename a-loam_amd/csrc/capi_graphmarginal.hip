// a-loam_amd/csrc/capi_graphmarginal.hip — host side of the pose-graph marginals (aloam_graph_marginals).  Every request is
// checked before anything is queued; the checked requests go through a pinned staging ring of their own and run in rounds of as many as
// there are scratch rows, in stream order; nothing synchronises the host (a slot of the ring is waited for only when kMarginalStageSlots
// later rounds have been queued behind it).  Nothing is allocated before the first call.
#include <algorithm>
#include <cmath>
#include <vector>

#include "capi_internal.hpp"
#include "information_device.hpp"

static_assert(kMarginalPivotTol == kInfoPivotTol, "the positive-definiteness rule of k_graph_marginals is k_loop_result's");
static_assert(sizeof(GraphMarginalItem) % 8 == 0, "items lie back to back in the ring and on the device");

// The ring and the device copy of a round's requests, on first use; nothing stays allocated behind a refusal.
static int marginal_staging(aloam_ctx* c) {
  if (c->mg.items) return ALOAM_OK;
  if (dalloc(c->mg.items, kMarginalStageItems) == hipSuccess && !c->mg.ring.create(sizeof(GraphMarginalItem) * kMarginalStageItems)) return ALOAM_OK;
  (void)hipGetLastError();
  c->mg.items.reset();
  c->err = "pose-graph marginals: allocating the request ring failed";
  return ALOAM_E_HIP;
}

extern "C" {

void aloam_graph_marginal_default_options(aloam_graph_marginal_options* opt) {
  if (!opt) return;
  opt->pcg_max_iterations = 200; opt->pad = 0; opt->pcg_tolerance = 1e-10; opt->huber_delta = 1.0;
}

int aloam_graph_marginals(aloam_ctx* c, const aloam_graph_marginal_request* req, int n, const aloam_graph_marginal_options* opt, aloam_graph_marginal_result* dst) {
  DeviceScope device_scope(c);
  if (!c) return ALOAM_E_ARG;
  if (const int rc = require_graph(c)) return rc;
  // ---- everything is checked before anything is queued
  if (n < 0 || (n > 0 && !req)) { c->err = "bad request list"; return ALOAM_E_ARG; }
  aloam_graph_marginal_options o;
  aloam_graph_marginal_default_options(&o);
  if (opt) o = *opt;
  if (o.pcg_max_iterations < 1 || !std::isfinite(o.pcg_tolerance) || o.pcg_tolerance < 0.0 || !(o.huber_delta > 0.0) || !std::isfinite(o.huber_delta)) {
    c->err = "bad options (pcg_max_iterations >= 1, pcg_tolerance finite and >= 0, huber_delta > 0)";
    return ALOAM_E_ARG;
  }
  o.pad = 0;
  if (n == 0) return ALOAM_OK;
  if (const int rc = require_host_list(c, req, "req")) return rc;
  void* d_dst = nullptr;
  if (const int rc = export_target(c, dst, 8, "dst", &d_dst)) return rc;
  std::vector<GraphMarginalItem> checked(n);
  int row_nodes = 1, row_edges = 1;
  long long nodes = 0, edges = 0;
  for (int r = 0; r < n; ++r) {
    GraphMarginalItem& it = checked[r];
    it.rq = req[r];
    auto fail = [&](const char* what) { c->err = "request " + std::to_string(r) + ": " + what; return ALOAM_E_ARG; };
    if (it.rq.mode != ALOAM_GRAPH_MARGINAL_MEASURED && it.rq.mode != ALOAM_GRAPH_MARGINAL_AT_ESTIMATE) return fail("mode must be ALOAM_GRAPH_MARGINAL_MEASURED or ALOAM_GRAPH_MARGINAL_AT_ESTIMATE");
    if (const char* what = graph_edge_check(c, it.rq.edge, it.rq.mode == ALOAM_GRAPH_MARGINAL_MEASURED)) return fail(what);
    it.rq.pad = 0;
    const SeqHost& s = c->seq[it.rq.edge.seq];
    it.nodes = s.graph_nodes; it.edges = s.graph_edges;
    row_nodes = std::max(row_nodes, it.nodes); row_edges = std::max(row_edges, it.edges);
    nodes += it.nodes; edges += it.edges;
  }
  if (const int rc = marginal_staging(c)) return rc;
  // ---- scratch rows: as many as fit the budget, at least one, no more than a slot of the ring holds
  const long long f64_row = graph_f64_row(row_nodes, row_edges), i32_row = graph_i32_row(row_nodes, row_edges);
  const long long fit = std::max(1LL, kMarginalScratchBytes / (8 * f64_row + 4 * i32_row));
  const int rows = (int)std::min<long long>({fit, (long long)n, (long long)kMarginalStageItems});
  if (const int rc = c->mg.f64.grow(c, f64_row * rows)) return rc;
  if (const int rc = c->mg.i32.grow(c, i32_row * rows)) return rc;
  // ---- rounds of at most `rows` requests over the same rows, in stream order
  ProfScope prof(c, K_GRAPH_MARGINALS);
  for (int r0 = 0; r0 < n; r0 += rows) {
    const int m = std::min(rows, n - r0);
    GraphMarginalItem* slot = nullptr; int ns = 0;
    if (const int rc = c->mg.ring.acquire(c, &slot, &ns)) return rc;
    std::copy(checked.begin() + r0, checked.begin() + r0 + m, slot);
    if (const int rc = c->mg.ring.queue(c, ns, slot, sizeof(GraphMarginalItem) * (size_t)m, c->mg.items.get(), c->stream)) return rc;
    GraphMarginalArgs a{};
    a.n = m; a.items = c->mg.items.get(); a.nodes = c->pg.nodes.get(); a.edges = c->pg.edges.get();
    a.max_nodes = c->pg.max_nodes; a.max_edges = c->pg.max_edges; a.row_nodes = row_nodes; a.row_edges = row_edges; a.opt = o;
    a.f64 = c->mg.f64.get(); a.f64_row = f64_row; a.i32 = c->mg.i32.get(); a.i32_row = i32_row;
    a.dst = static_cast<aloam_graph_marginal_result*>(d_dst) + r0;
    launch_graph_marginals(a, c->stream);
  }
  HIP_TRY(c, hipGetLastError());
  c->mg.last_nodes = nodes; c->mg.last_edges = edges; c->mg.last_n = n;
  return ALOAM_OK;
}

}  // extern "C"
