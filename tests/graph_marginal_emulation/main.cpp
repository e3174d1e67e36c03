// tests/graph_marginal_emulation/main.cpp - runs k_graph_marginals of the host build (tests/posegraph_emulation/emulation.hpp) on one graph and
// a list of requests read from files:
//   main NODES EDGES REQUESTS PAD OUT [pcg_max_iterations=K] [pcg_tolerance=X] [huber_delta=X]
// The graph is sequence 0; sequence 1 holds one node, and a request on it is put first (it reports NO_EDGES).  The rows of the store have PAD
// spare records and the scratch rows are followed by guard words.  OUT receives the results of the requests read, in order.
#include "graphmarginal_kernels_host.cpp"
#include <string>
using namespace aloam;
template <class T> std::vector<T> rd(const char* p) { FILE* f = fopen(p, "rb"); fseek(f, 0, SEEK_END); long n = ftell(f); fseek(f, 0, SEEK_SET); std::vector<T> v(n / sizeof(T)); if (fread(v.data(), 1, n, f) != (size_t)n) abort(); fclose(f); return v; }
int main(int argc, char** argv) {
  auto nodes = rd<aloam_graph_node>(argv[1]); auto edges = rd<aloam_graph_edge>(argv[2]); auto reqs = rd<aloam_graph_marginal_request>(argv[3]);
  const int N = nodes.size(), E = edges.size(), R = reqs.size(), pad = atoi(argv[4]);
  GraphMarginalArgs a{}; a.n = R + 1;
  std::vector<GraphMarginalItem> items(R + 1);
  memset(items.data(), 0, sizeof(GraphMarginalItem) * items.size());
  items[0].rq = reqs[0]; items[0].rq.edge.seq = 1; items[0].rq.edge.i = -1; items[0].rq.edge.j = 0; items[0].nodes = 1; items[0].edges = 0;
  for (int r = 0; r < R; ++r) { items[r + 1].rq = reqs[r]; items[r + 1].nodes = N; items[r + 1].edges = E; }
  std::vector<aloam_graph_node> store(2 * (N + pad)); std::vector<aloam_graph_edge> es(2 * (E + pad));
  std::copy(nodes.begin(), nodes.end(), store.begin()); std::copy(edges.begin(), edges.end(), es.begin());
  const std::vector<aloam_graph_node> store0 = store; const std::vector<aloam_graph_edge> es0 = es;
  a.items = items.data(); a.nodes = store.data(); a.edges = es.data(); a.max_nodes = N + pad; a.max_edges = E + pad; a.row_nodes = N + 1; a.row_edges = E + 2;
  a.opt.pcg_max_iterations = 200; a.opt.pad = 0; a.opt.pcg_tolerance = 1e-10; a.opt.huber_delta = 1.0;
  for (int k = 6; k < argc; ++k) {
    const char* eq = strchr(argv[k], '=');
    if (!eq) { fprintf(stderr, "bad option %s\n", argv[k]); return 2; }
    const std::string key(argv[k], eq - argv[k]);
    if (key == "pcg_max_iterations") a.opt.pcg_max_iterations = atoi(eq + 1);
    else if (key == "pcg_tolerance") a.opt.pcg_tolerance = atof(eq + 1);
    else if (key == "huber_delta") a.opt.huber_delta = atof(eq + 1);
    else { fprintf(stderr, "unknown option %s\n", argv[k]); return 2; }
  }
  a.f64_row = graph_f64_row(a.row_nodes, a.row_edges); a.i32_row = graph_i32_row(a.row_nodes, a.row_edges);
  std::vector<double> f((R + 1) * a.f64_row + 8, -7.0); std::vector<int> g((R + 1) * a.i32_row + 8, -7);
  a.f64 = f.data(); a.i32 = g.data();
  std::vector<aloam_graph_marginal_result> res(R + 1);
  memset(res.data(), 0xff, sizeof(aloam_graph_marginal_result) * res.size());
  a.dst = res.data();
  launch_graph_marginals(a, nullptr);
  for (int k = 0; k < 8; ++k) if (f[(R + 1) * a.f64_row + k] != -7.0 || g[(R + 1) * a.i32_row + k] != -7) printf("GUARD OVERWRITTEN\n");
  if (memcmp(store.data(), store0.data(), sizeof(aloam_graph_node) * store.size()) || memcmp(es.data(), es0.data(), sizeof(aloam_graph_edge) * es.size())) printf("GRAPH CHANGED\n");
  for (int i = 0; i <= R; ++i) printf("status %d mode %d seq %d i %d j %d pcg %d nodes %d edges %d chi2 %.17g s_edge %.17g\n", res[i].status, res[i].mode, res[i].seq, res[i].i, res[i].j,
         res[i].pcg_iterations, res[i].nodes, res[i].edges, res[i].chi2, res[i].s_edge);
  FILE* o = fopen(argv[5], "wb"); fwrite(res.data() + 1, sizeof(aloam_graph_marginal_result), R, o); fclose(o);
}
