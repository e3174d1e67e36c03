// a-loam_amd/csrc/capi_graphrobust.hip — host side of the robust pose-graph solve (aloam_graph_optimize_robust).  Every
// argument is checked before anything is queued; the listed sequences go through the pose graphs' staging ring and the solve's scratch
// rows (GraphStore), which this call grows by the scaled copy of the edges; nothing synchronises the host and nothing is kept between calls.
#include <algorithm>
#include <cmath>

#include "capi_internal.hpp"
#include "graphrobust_kernels.hpp"

static_assert(sizeof(aloam_graph_robust_options) == 32 && sizeof(aloam_graph_robust_result) == 128, "the sizes include/aloam_mi355x.h states");

extern "C" {

void aloam_graph_robust_default_options(aloam_graph_robust_options* opt) {
  if (!opt) return;
  opt->max_outer_iterations = 100; opt->pad = 0; opt->inlier_chi2 = 22.46; opt->mu_step = 1.4; opt->reserved = 0.0;
}

int aloam_graph_optimize_robust(aloam_ctx* c, const int* seqs, int n, const aloam_graph_options* opt, const aloam_graph_robust_options* robust,
                                aloam_graph_robust_result* dst, double* weights_dst, long long weights_stride) {
  DeviceScope device_scope(c);
  if (!c) return ALOAM_E_ARG;
  if (const int rc = require_graph(c)) return rc;
  if (const int rc = check_ids(c, seqs, n)) return rc;
  aloam_graph_options o;
  aloam_graph_default_options(&o);
  if (opt) o = *opt;
  auto tol_ok = [](double v) { return std::isfinite(v) && v >= 0.0; };
  if (o.max_iterations < 0 || o.pcg_max_iterations < 1 || !tol_ok(o.function_tolerance) || !tol_ok(o.gradient_tolerance) || !tol_ok(o.pcg_tolerance) ||
      !(o.huber_delta > 0.0) || !std::isfinite(o.huber_delta)) {
    c->err = "bad options (max_iterations >= 0, pcg_max_iterations >= 1, tolerances finite and >= 0, huber_delta > 0)";
    return ALOAM_E_ARG;
  }
  aloam_graph_robust_options r;
  aloam_graph_robust_default_options(&r);
  if (robust) r = *robust;
  if (r.max_outer_iterations < 1 || !(r.inlier_chi2 > 0.0) || !std::isfinite(r.inlier_chi2) || !(r.mu_step > 1.0) || !std::isfinite(r.mu_step)) {
    c->err = "bad robust options (max_outer_iterations >= 1, inlier_chi2 > 0 and finite, mu_step > 1 and finite)";
    return ALOAM_E_ARG;
  }
  r.pad = 0; r.reserved = 0.0;
  int row_nodes = 1, row_edges = 1, most_edges = 0;
  long long nodes = 0, edges = 0;
  for (int i = 0; i < n; ++i) {
    const SeqHost& s = c->seq[seqs[i]];
    row_nodes = std::max(row_nodes, s.graph_nodes); row_edges = std::max(row_edges, s.graph_edges); most_edges = std::max(most_edges, s.graph_edges);
    nodes += s.graph_nodes; edges += s.graph_edges;
  }
  void* d = nullptr;
  void* d_w = nullptr;
  if (n > 0) if (const int rc = export_target(c, dst, alignof(aloam_graph_robust_result), "dst", &d)) return rc;
  if (n > 0 && weights_dst) {
    if (const int rc = export_target(c, weights_dst, alignof(double), "weights_dst", &d_w)) return rc;
    if (weights_stride < most_edges) { c->err = "weights_stride is below the largest edge count listed (" + std::to_string(most_edges) + ")"; return ALOAM_E_ARG; }
  }
  if (n == 0) return ALOAM_OK;
  const long long f64_row = graph_robust_f64_row(row_nodes, row_edges), i32_row = graph_i32_row(row_nodes, row_edges);
  if (const int rc = c->pg.f64.grow(c, f64_row * n)) return rc;
  if (const int rc = c->pg.i32.grow(c, i32_row * n)) return rc;
  GraphSolveItem* items = nullptr;
  int slot = 0;
  if (const int rc = c->pg.ring.acquire(c, &items, &slot)) return rc;
  for (int i = 0; i < n; ++i) items[i] = GraphSolveItem{seqs[i], c->seq[seqs[i]].graph_nodes, c->seq[seqs[i]].graph_edges, 0};
  if (const int rc = c->pg.ring.queue(c, slot, items, sizeof(GraphSolveItem) * (size_t)n, c->pg.items.get(), c->stream)) return rc;
  GraphRobustArgs a{};
  a.g.n = n; a.g.items = c->pg.items.get(); a.g.nodes = c->pg.nodes.get(); a.g.edges = c->pg.edges.get();
  a.g.max_nodes = c->pg.max_nodes; a.g.max_edges = c->pg.max_edges; a.g.row_nodes = row_nodes; a.g.row_edges = row_edges; a.g.opt = o;
  a.g.f64 = c->pg.f64.get(); a.g.f64_row = f64_row; a.g.i32 = c->pg.i32.get(); a.g.i32_row = i32_row;
  a.g.dst = nullptr;
  a.robust = r;
  a.dst = static_cast<aloam_graph_robust_result*>(d);
  a.weights = static_cast<double*>(d_w); a.weights_stride = weights_stride;
  {
    ProfScope p(c, K_POSE_GRAPH);
    launch_graph_robust(a, c->stream);
  }
  HIP_TRY(c, hipGetLastError());
  c->pg.last_nodes = nodes; c->pg.last_edges = edges; c->pg.last_trim_bytes = -1;
  return ALOAM_OK;
}

}  // extern "C"
