// a-loam_amd/csrc/graphrobust_kernels.hpp — the robust pose-graph solve (aloam_graph_optimize_robust): what capi_graphrobust.hip
// hands to graphrobust_kernels.hip.
#pragma once
#include "posegraph_kernels.hpp"

namespace aloam {

// A scratch row of the robust solve: the row of aloam_graph_optimize, then per edge the scaled copy (an aloam_graph_edge, 30 doubles), w
// and s.
constexpr long long kRobustEdgeRow = 32;
static_assert(sizeof(aloam_graph_edge) == 8 * (kRobustEdgeRow - 2), "the scaled copy of an edge takes 30 doubles of a scratch row");
inline long long graph_robust_f64_row(int nodes, int edges) { return graph_f64_row(nodes, edges) + kRobustEdgeRow * edges; }

struct GraphRobustArgs {
  GraphSolveArgs g;                  // as for aloam_graph_optimize, with f64_row = graph_robust_f64_row and dst unused
  aloam_graph_robust_options robust;
  aloam_graph_robust_result* dst;    // [n]
  double* weights;                   // [n][weights_stride], or nullptr
  long long weights_stride;
};
void launch_graph_robust(const GraphRobustArgs& a, hipStream_t stream);

}  // namespace aloam
