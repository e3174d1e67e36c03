// a-loam_amd/csrc/capi_posegraph.hip — host side of the pose graphs (aloam_graph_*): the store and its per-sequence rows, the stream-ordered
// add / export / clear, and the batched solve.  Every argument is checked before anything is queued; the counts are SeqHost fields changed
// by the events of capi_seq.hip.
#include <algorithm>
#include <cmath>
#include <vector>

#include "capi_internal.hpp"

int aloam::require_graph(aloam_ctx* c) {
  if (!c->pg.on) { c->err = "pose graphs are not enabled (aloam_graph_enable)"; return ALOAM_E_STATE; }
  return ALOAM_OK;
}

// The upper triangle of a 6 x 6 information matrix: finite, and a Cholesky factorisation succeeds.
static bool info_positive_definite(const double* u) {
  double A[6][6], L[6][6];
  int o = 0;
  for (int i = 0; i < 6; ++i)
    for (int j = i; j < 6; ++j) { if (!std::isfinite(u[o])) return false; A[i][j] = A[j][i] = u[o++]; }
  for (int i = 0; i < 6; ++i)
    for (int j = 0; j <= i; ++j) {
      double s = A[i][j];
      for (int k = 0; k < j; ++k) s -= L[i][k] * L[j][k];
      if (i == j) { if (!(s > 0.0) || !std::isfinite(s)) return false; L[i][i] = std::sqrt(s); }
      else L[i][j] = s / L[j][j];
    }
  return true;
}

const char* aloam::graph_edge_check(const aloam_ctx* c, aloam_graph_edge& e, bool measurement) {
  if (e.seq < 0 || e.seq >= c->B) return "seq out of range";
  const int nodes = c->seq[e.seq].graph_nodes;
  if (e.i < -1 || e.i >= nodes || e.j < 0 || e.j >= nodes || e.i == e.j) return "need -1 <= i < nodes, 0 <= j < nodes, i != j";
  if (!measurement) return nullptr;
  if (e.flags & ~ALOAM_GRAPH_EDGE_ROBUST) return "unknown flags";
  double nn = 0.0;
  for (int a = 0; a < 4; ++a) { if (!std::isfinite(e.q[a])) return "q is not finite"; nn += e.q[a] * e.q[a]; }
  nn = std::sqrt(nn);
  if (!(std::fabs(nn - 1.0) <= 1e-6)) return "q is not within 1e-6 of unit norm";
  for (int a = 0; a < 4; ++a) e.q[a] /= nn;
  for (int a = 0; a < 3; ++a) if (!std::isfinite(e.t[a])) return "t is not finite";
  if (!info_positive_definite(e.info)) return "info is not finite and positive definite";
  return nullptr;
}

// (seq has been checked by the caller, which read `have` from its SeqHost)
static int export_rows(aloam_ctx* c, int seq, int first, int count, int have, const void* base, size_t row, size_t item, void* dst) {
  if (first < 0 || count < 0 || first + (long long)count > have) { c->err = "[first, first + count) must lie inside what the sequence's graph holds"; return ALOAM_E_ARG; }
  void* d = nullptr;
  if (count > 0) if (const int rc = export_target(c, dst, 8, "dst", &d)) return rc;
  if (count == 0) return ALOAM_OK;
  const char* src = static_cast<const char*>(base) + ((size_t)seq * row + (size_t)first) * item;
  HIP_TRY(c, hipMemcpyAsync(d, src, item * (size_t)count, hipMemcpyDefault, c->stream));
  return ALOAM_OK;
}

extern "C" {

void aloam_graph_default_options(aloam_graph_options* opt) {
  if (!opt) return;
  opt->max_iterations = 20; opt->pcg_max_iterations = 200;
  opt->function_tolerance = 1e-10; opt->gradient_tolerance = 1e-10; opt->pcg_tolerance = 1e-8; opt->huber_delta = 1.0;
}

int aloam_graph_enable(aloam_ctx* c, int max_nodes, int max_edges) {
  DeviceScope device_scope(c);
  if (!c) return ALOAM_E_ARG;
  if (const int rc = require_stage(c, ALOAM_STAGE_ODOMETRY)) return rc;
  if (c->pg.on) { c->err = "pose graphs already enabled"; return ALOAM_E_STATE; }
  if (max_nodes < 1 || max_nodes > (1 << 20) || max_edges < 1 || max_edges > (1 << 22)) { c->err = "need 1 <= max_nodes <= 2^20 and 1 <= max_edges <= 2^22"; return ALOAM_E_ARG; }
  const size_t B = c->B;
  static_assert(sizeof(GraphAddItem) >= sizeof(GraphSolveItem) && sizeof(GraphAddItem) % 8 == 0, "a slot of the ring holds B items of either kind");
  GraphStore g;                        // committed with one move: nothing stays allocated behind a refusal
  const bool ok = dalloc(g.nodes, B * max_nodes) == hipSuccess && dalloc(g.edges, B * max_edges) == hipSuccess &&
                  dalloc(g.add, B) == hipSuccess && dalloc(g.items, B) == hipSuccess && !g.ring.create(B * sizeof(GraphAddItem));
  if (!ok) { (void)hipGetLastError(); c->err = "pose graph store: allocation failed"; return ALOAM_E_HIP; }
  g.max_nodes = max_nodes; g.max_edges = max_edges;
  g.on = true;
  c->pg = std::move(g);
  return ALOAM_OK;
}

int aloam_graph_add_nodes(aloam_ctx* c, const int* seqs, int n, const double* odom_info) {
  DeviceScope device_scope(c);
  if (!c) return ALOAM_E_ARG;
  if (const int rc = require_graph(c)) return rc;
  if (const int rc = check_ids(c, seqs, n)) return rc;
  if (n > 0 && !odom_info) { c->err = "odom_info is NULL"; return ALOAM_E_ARG; }
  for (int i = 0; i < n; ++i) {                 // everything is checked before the ring is touched
    const SeqHost& s = c->seq[seqs[i]];
    if (!info_positive_definite(odom_info + 21 * (size_t)i)) { c->err = "odom_info " + std::to_string(i) + " is not finite and positive definite"; return ALOAM_E_ARG; }
    if (s.graph_nodes >= c->pg.max_nodes || (s.graph_nodes > 0 && s.graph_edges >= c->pg.max_edges)) {
      c->err = "the graph of sequence " + std::to_string(seqs[i]) + " is full (" + std::to_string(s.graph_nodes) + " nodes, " + std::to_string(s.graph_edges) + " edges)";
      return ALOAM_E_CAPACITY;
    }
  }
  if (const int rc = keyframe_add_check(c, seqs, n)) return rc;
  if (n == 0) return ALOAM_OK;
  GraphAddItem* items = nullptr;
  int slot = 0;
  if (const int rc = c->pg.ring.acquire(c, &items, &slot)) return rc;
  for (int i = 0; i < n; ++i) {
    const SeqHost& s = c->seq[seqs[i]];
    items[i].seq = seqs[i]; items[i].node = s.graph_nodes; items[i].edge = s.graph_edges; items[i].pad = 0;
    std::copy(odom_info + 21 * (size_t)i, odom_info + 21 * (size_t)(i + 1), items[i].info);
  }
  if (const int rc = c->pg.ring.queue(c, slot, items, sizeof(GraphAddItem) * (size_t)n, c->pg.add.get(), c->stream)) return rc;
  GraphAddArgs a{};
  a.n = n; a.items = c->pg.add.get(); a.odom = c->d_state.get(); a.mapseq = c->map_on ? c->d_mapseq.get() : nullptr;
  a.nodes = c->pg.nodes.get(); a.edges = c->pg.edges.get(); a.max_nodes = c->pg.max_nodes; a.max_edges = c->pg.max_edges;
  launch_graph_add_nodes(a, c->stream);
  queue_keyframe_capture(c, n);        // the stacks of the listed sequences become the new nodes' clouds (aloam_graph_keyframes_enable)
  HIP_TRY(c, hipGetLastError());
  on_graph_nodes_added(c, seqs, n);
  return ALOAM_OK;
}

int aloam_graph_add_edges(aloam_ctx* c, const aloam_graph_edge* edges, int n) {
  DeviceScope device_scope(c);
  if (!c) return ALOAM_E_ARG;
  if (const int rc = require_graph(c)) return rc;
  if (n < 0 || (n > 0 && !edges)) { c->err = "bad edge list"; return ALOAM_E_ARG; }
  if (n > 0) if (const int rc = require_host_list(c, edges, "edges")) return rc;
  std::vector<aloam_graph_edge> checked(edges, edges + n);
  std::vector<int> added(c->B, 0);
  for (int k = 0; k < n; ++k) {
    aloam_graph_edge& e = checked[k];
    if (const char* what = graph_edge_check(c, e, true)) { c->err = "edge " + std::to_string(k) + ": " + what; return ALOAM_E_ARG; }
    if (c->seq[e.seq].graph_edges + ++added[e.seq] > c->pg.max_edges) {
      c->err = "edge " + std::to_string(k) + ": the edge row of sequence " + std::to_string(e.seq) + " is full";
      return ALOAM_E_CAPACITY;
    }
  }
  // runs of one sequence go to its row with one copy each
  for (int k = 0; k < n;) {
    int m = k + 1;
    while (m < n && checked[m].seq == checked[k].seq) ++m;
    const int seq = checked[k].seq;
    aloam_graph_edge* at = c->pg.edges.get() + (size_t)seq * c->pg.max_edges + c->seq[seq].graph_edges;
    HIP_TRY(c, hipMemcpyAsync(at, checked.data() + k, sizeof(aloam_graph_edge) * (size_t)(m - k), hipMemcpyHostToDevice, c->stream));
    on_graph_edges_added(c, seq, m - k);
    k = m;
  }
  return ALOAM_OK;
}

int aloam_graph_export(aloam_ctx* c, int seq, int first, int count, aloam_graph_node* dst) {
  DeviceScope device_scope(c);
  if (!c) return ALOAM_E_ARG;
  if (const int rc = require_graph(c)) return rc;
  if (const int rc = check_seq(c, seq)) return rc;
  return export_rows(c, seq, first, count, c->seq[seq].graph_nodes, c->pg.nodes.get(), c->pg.max_nodes, sizeof(aloam_graph_node), dst);
}

int aloam_graph_export_edges(aloam_ctx* c, int seq, int first, int count, aloam_graph_edge* dst) {
  DeviceScope device_scope(c);
  if (!c) return ALOAM_E_ARG;
  if (const int rc = require_graph(c)) return rc;
  if (const int rc = check_seq(c, seq)) return rc;
  return export_rows(c, seq, first, count, c->seq[seq].graph_edges, c->pg.edges.get(), c->pg.max_edges, sizeof(aloam_graph_edge), dst);
}

int aloam_graph_clear(aloam_ctx* c, const int* seqs, int n) {
  if (!c) return ALOAM_E_ARG;
  if (const int rc = require_graph(c)) return rc;
  if (const int rc = check_ids(c, seqs, n)) return rc;
  on_graph_cleared(c, seqs, n);       // later adds overwrite the rows in stream order; nothing on the device depends on the counts
  return queue_keyframe_rewind(c, seqs, n);
}

int aloam_graph_info(aloam_ctx* c, int seq, int out[4]) {
  if (!c || !out) return ALOAM_E_ARG;
  if (const int rc = require_graph(c)) return rc;
  if (const int rc = check_seq(c, seq)) return rc;
  out[0] = c->seq[seq].graph_nodes; out[1] = c->seq[seq].graph_edges; out[2] = c->pg.max_nodes; out[3] = c->pg.max_edges;
  return ALOAM_OK;
}

int aloam_graph_optimize(aloam_ctx* c, const int* seqs, int n, const aloam_graph_options* opt, aloam_graph_result* dst) {
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
  void* d = nullptr;
  if (n > 0) if (const int rc = export_target(c, dst, alignof(aloam_graph_result), "dst", &d)) return rc;
  if (n == 0) return ALOAM_OK;
  int row_nodes = 1, row_edges = 1;
  long long nodes = 0, edges = 0;
  for (int i = 0; i < n; ++i) {
    const SeqHost& s = c->seq[seqs[i]];
    row_nodes = std::max(row_nodes, s.graph_nodes); row_edges = std::max(row_edges, s.graph_edges);
    nodes += s.graph_nodes; edges += s.graph_edges;
  }
  const long long f64_row = graph_f64_row(row_nodes, row_edges), i32_row = graph_i32_row(row_nodes, row_edges);
  if (const int rc = c->pg.f64.grow(c, f64_row * n)) return rc;
  if (const int rc = c->pg.i32.grow(c, i32_row * n)) return rc;
  GraphSolveItem* items = nullptr;
  int slot = 0;
  if (const int rc = c->pg.ring.acquire(c, &items, &slot)) return rc;
  for (int i = 0; i < n; ++i) items[i] = GraphSolveItem{seqs[i], c->seq[seqs[i]].graph_nodes, c->seq[seqs[i]].graph_edges, 0};
  if (const int rc = c->pg.ring.queue(c, slot, items, sizeof(GraphSolveItem) * (size_t)n, c->pg.items.get(), c->stream)) return rc;
  GraphSolveArgs a{};
  a.n = n; a.items = c->pg.items.get(); a.nodes = c->pg.nodes.get(); a.edges = c->pg.edges.get();
  a.max_nodes = c->pg.max_nodes; a.max_edges = c->pg.max_edges; a.row_nodes = row_nodes; a.row_edges = row_edges; a.opt = o;
  a.f64 = c->pg.f64.get(); a.f64_row = f64_row; a.i32 = c->pg.i32.get(); a.i32_row = i32_row;
  a.dst = static_cast<aloam_graph_result*>(d);
  {
    ProfScope p(c, K_POSE_GRAPH);
    launch_pose_graph(a, c->stream);
  }
  HIP_TRY(c, hipGetLastError());
  c->pg.last_nodes = nodes; c->pg.last_edges = edges; c->pg.last_trim_bytes = -1;
  return ALOAM_OK;
}

}  // extern "C"
