// tests/posegraph_emulation/main.cpp - runs k_graph_incidence + k_pose_graph of the host build on one graph read from files:
//   main NODES EDGES PAD OUT [function_tolerance] [max_iterations=K] [pcg_max_iterations=K] [pcg_tolerance=X] [huber_delta=X] [function_tolerance=X]
// The graph is the second of two listed items (the first has one node and reports NO_EDGES), its rows have PAD spare records, and the scratch
// rows are followed by guard words.
#include "posegraph_kernels_host.cpp"
#include <string>
using namespace aloam;
template <class T> std::vector<T> rd(const char* p) { FILE* f = fopen(p, "rb"); fseek(f, 0, SEEK_END); long n = ftell(f); fseek(f, 0, SEEK_SET); std::vector<T> v(n / sizeof(T)); if (fread(v.data(), 1, n, f) != (size_t)n) abort(); fclose(f); return v; }
int main(int argc, char** argv) {
  auto nodes = rd<aloam_graph_node>(argv[1]); auto edges = rd<aloam_graph_edge>(argv[2]);
  const int N = nodes.size(), E = edges.size(), pad = atoi(argv[3]);   // pad: extra row capacity, and a second (empty) item first
  GraphSolveArgs a{}; a.n = 2;
  GraphSolveItem items[2] = {{1, 1, 0, 0}, {0, N, E, 0}};
  std::vector<aloam_graph_node> store(2 * (N + pad)); std::vector<aloam_graph_edge> es(2 * (E + pad));
  std::copy(nodes.begin(), nodes.end(), store.begin()); std::copy(edges.begin(), edges.end(), es.begin());
  a.items = items; a.nodes = store.data(); a.edges = es.data(); a.max_nodes = N + pad; a.max_edges = E + pad; a.row_nodes = N; a.row_edges = E;
  a.opt.max_iterations = 50; a.opt.pcg_max_iterations = 200; a.opt.function_tolerance = 0; a.opt.gradient_tolerance = 1e-10; a.opt.pcg_tolerance = 1e-8; a.opt.huber_delta = 1.0;
  for (int k = 5; k < argc; ++k) {
    const char* eq = strchr(argv[k], '=');
    const std::string key = eq ? std::string(argv[k], eq - argv[k]) : std::string("function_tolerance");
    const char* value = eq ? eq + 1 : argv[k];
    if (key == "max_iterations") a.opt.max_iterations = atoi(value);
    else if (key == "pcg_max_iterations") a.opt.pcg_max_iterations = atoi(value);
    else if (key == "pcg_tolerance") a.opt.pcg_tolerance = atof(value);
    else if (key == "huber_delta") a.opt.huber_delta = atof(value);
    else if (key == "function_tolerance") a.opt.function_tolerance = atof(value);
    else { fprintf(stderr, "unknown option %s\n", argv[k]); return 2; }
  }
  a.f64_row = graph_f64_row(N, E); a.i32_row = graph_i32_row(N, E);
  std::vector<double> f(2 * a.f64_row + 8, -7.0); std::vector<int> g(2 * a.i32_row + 8, -7);
  a.f64 = f.data(); a.i32 = g.data();
  aloam_graph_result res[2]; a.dst = res;
  launch_pose_graph(a, nullptr);
  for (int k = 0; k < 8; ++k) if (f[2 * a.f64_row + k] != -7.0 || g[2 * a.i32_row + k] != -7) printf("GUARD OVERWRITTEN\n");
  for (int i = 0; i < 2; ++i) printf("status %d term %d lm %d acc %d pcg %d nodes %d edges %d cost %.17g -> %.17g gmax %.17g\n", res[i].status, res[i].termination, res[i].lm_iterations,
         res[i].accepted_steps, res[i].pcg_iterations, res[i].nodes, res[i].edges, res[i].initial_cost, res[i].final_cost, res[i].gradient_max);
  FILE* o = fopen(argv[4], "wb"); fwrite(store.data(), sizeof(aloam_graph_node), N, o); fclose(o);
}
