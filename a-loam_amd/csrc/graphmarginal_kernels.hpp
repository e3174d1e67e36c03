// a-loam_amd/csrc/graphmarginal_kernels.hpp — pose-graph marginals (aloam_graph_marginals): what capi_graphmarginal.hip hands to
// graphmarginal_kernels.hip.
#pragma once
#include "posegraph_kernels.hpp"

namespace aloam {

constexpr int kMarginalStageSlots = 4;        // pinned ring of requests: rounds in flight before the host waits for one
constexpr int kMarginalStageItems = 1024;     // requests a slot of the ring holds = the most one round takes
constexpr long long kMarginalScratchBytes = 1LL << 30;   // what the scratch rows of a round may take together (one row at least)
constexpr double kMarginalPivotTol = 1e-12;   // = kInfoPivotTol (information_device.hpp; capi_graphmarginal.hip asserts it): the rule of k_loop_result

// One request as checked by the host, with the counts of its sequence's graph (host state).
struct GraphMarginalItem { aloam_graph_marginal_request rq; int nodes, edges; };
struct GraphMarginalArgs {
  int n;
  const GraphMarginalItem* items;    // [n]
  const aloam_graph_node* nodes;     // [B][max_nodes]
  const aloam_graph_edge* edges;     // [B][max_edges]
  int max_nodes, max_edges;
  int row_nodes, row_edges;          // the largest counts listed: what a scratch row is laid out for (graph_f64_row / graph_i32_row)
  aloam_graph_marginal_options opt;
  double* f64; long long f64_row;    // [n][f64_row]: row w belongs to workgroup w
  int* i32; long long i32_row;       // [n][i32_row]
  aloam_graph_marginal_result* dst;  // [n]
};
void launch_graph_marginals(const GraphMarginalArgs& a, hipStream_t stream);

}  // namespace aloam
