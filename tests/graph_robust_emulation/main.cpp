// tests/graph_robust_emulation/main.cpp - runs k_graph_robust of the host build (tests/posegraph_emulation/emulation.hpp) on one graph read
// from files:
//   main NODES EDGES PAD OUT [key=value ...]      keys: the fields of aloam_graph_options and of aloam_graph_robust_options
// The graph is sequence 0; sequence 1 holds one node and is listed first (it reports NO_EDGES).  The rows of the store have PAD spare
// records, the scratch rows are followed by guard words and a weight row is longer than the edge count.  OUT receives the graph's result,
// its weight row and its nodes after the call.
#include "graphrobust_kernels_host.cpp"
#include <string>
using namespace aloam;
template <class T> std::vector<T> rd(const char* p) { FILE* f = fopen(p, "rb"); fseek(f, 0, SEEK_END); long n = ftell(f); fseek(f, 0, SEEK_SET); std::vector<T> v(n / sizeof(T)); if (fread(v.data(), 1, n, f) != (size_t)n) abort(); fclose(f); return v; }
int main(int argc, char** argv) {
  auto nodes = rd<aloam_graph_node>(argv[1]); auto edges = rd<aloam_graph_edge>(argv[2]);
  const int N = nodes.size(), E = edges.size(), pad = atoi(argv[3]);
  GraphRobustArgs a{}; a.g.n = 2;
  GraphSolveItem items[2] = {{1, 1, 0, 0}, {0, N, E, 0}};
  std::vector<aloam_graph_node> store(2 * (N + pad)); std::vector<aloam_graph_edge> es(2 * (E + pad));
  memset(store.data(), 0, sizeof(aloam_graph_node) * store.size()); memset(es.data(), 0, sizeof(aloam_graph_edge) * es.size());
  std::copy(nodes.begin(), nodes.end(), store.begin()); std::copy(edges.begin(), edges.end(), es.begin());
  store[N + pad] = nodes[0];
  const std::vector<aloam_graph_edge> es0 = es;
  a.g.items = items; a.g.nodes = store.data(); a.g.edges = es.data(); a.g.max_nodes = N + pad; a.g.max_edges = E + pad; a.g.row_nodes = N + 1; a.g.row_edges = E + 2;
  a.g.opt.max_iterations = 20; a.g.opt.pcg_max_iterations = 200; a.g.opt.function_tolerance = 1e-10; a.g.opt.gradient_tolerance = 1e-10;
  a.g.opt.pcg_tolerance = 1e-8; a.g.opt.huber_delta = 1.0;
  a.robust.max_outer_iterations = 100; a.robust.pad = 0; a.robust.inlier_chi2 = 22.46; a.robust.mu_step = 1.4; a.robust.reserved = 0.0;
  for (int k = 5; k < argc; ++k) {
    const char* eq = strchr(argv[k], '=');
    if (!eq) { fprintf(stderr, "bad option %s\n", argv[k]); return 2; }
    const std::string key(argv[k], eq - argv[k]);
    if (key == "max_iterations") a.g.opt.max_iterations = atoi(eq + 1);
    else if (key == "pcg_max_iterations") a.g.opt.pcg_max_iterations = atoi(eq + 1);
    else if (key == "function_tolerance") a.g.opt.function_tolerance = atof(eq + 1);
    else if (key == "gradient_tolerance") a.g.opt.gradient_tolerance = atof(eq + 1);
    else if (key == "pcg_tolerance") a.g.opt.pcg_tolerance = atof(eq + 1);
    else if (key == "huber_delta") a.g.opt.huber_delta = atof(eq + 1);
    else if (key == "max_outer_iterations") a.robust.max_outer_iterations = atoi(eq + 1);
    else if (key == "inlier_chi2") a.robust.inlier_chi2 = atof(eq + 1);
    else if (key == "mu_step") a.robust.mu_step = atof(eq + 1);
    else { fprintf(stderr, "unknown option %s\n", argv[k]); return 2; }
  }
  a.g.f64_row = graph_robust_f64_row(a.g.row_nodes, a.g.row_edges); a.g.i32_row = graph_i32_row(a.g.row_nodes, a.g.row_edges);
  std::vector<double> f(2 * a.g.f64_row + 8, -7.0); std::vector<int> g(2 * a.g.i32_row + 8, -7);
  a.g.f64 = f.data(); a.g.i32 = g.data();
  std::vector<aloam_graph_robust_result> res(2);
  memset(res.data(), 0xff, sizeof(aloam_graph_robust_result) * res.size());
  a.dst = res.data();
  a.weights_stride = E + 3;
  std::vector<double> wts(2 * a.weights_stride, -7.0);
  a.weights = wts.data();
  launch_graph_robust(a, nullptr);
  for (int k = 0; k < 8; ++k) if (f[2 * a.g.f64_row + k] != -7.0 || g[2 * a.g.i32_row + k] != -7) printf("GUARD OVERWRITTEN\n");
  for (int k = 0; k < a.weights_stride; ++k) if (wts[k] != -7.0 || (k >= E && wts[a.weights_stride + k] != -7.0)) printf("GUARD OVERWRITTEN (weights)\n");
  if (memcmp(es.data(), es0.data(), sizeof(aloam_graph_edge) * es.size())) printf("EDGES CHANGED\n");
  for (int k = 0; k < N; ++k)
    if (memcmp(store[k].q, nodes[k].q, 56) || store[k].frame != nodes[k].frame || (k == 0 && memcmp(&store[k], &nodes[k], sizeof(aloam_graph_node)))) printf("ENTERED POSES CHANGED\n");
  if (memcmp(&store[N + pad], &nodes[0], sizeof(aloam_graph_node))) printf("OTHER GRAPH CHANGED\n");
  for (int i = 0; i < 2; ++i) {
    const aloam_graph_robust_result& r = res[i];
    printf("status %d termination %d lm %d accepted %d pcg %d nodes %d edges %d outer %d robust %d inliers %d outliers %d mu %.17g s_max %.17g\n", r.solve.status, r.solve.termination,
           r.solve.lm_iterations, r.solve.accepted_steps, r.solve.pcg_iterations, r.solve.nodes, r.solve.edges, r.outer_iterations, r.robust_edges, r.inliers, r.outliers, r.mu, r.s_max);
  }
  FILE* o = fopen(argv[4], "wb");
  fwrite(&res[1], sizeof(aloam_graph_robust_result), 1, o); fwrite(wts.data() + a.weights_stride, sizeof(double), E, o); fwrite(store.data(), sizeof(aloam_graph_node), N, o);
  fclose(o);
}
