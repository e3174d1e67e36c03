// a-loam_amd/csrc/graphpropose_kernels.hpp — loop candidates by pose proximity (aloam_graph_propose_loops): what
// capi_graphpropose.hip hands to graphpropose_kernels.hip.
#pragma once
#include "posegraph_kernels.hpp"

namespace aloam {

constexpr int kProposeHits = 1024;            // hits (d2, i) a workgroup keeps in LDS: 8 KiB of d2 and 4 KiB of i; a query with more rescans the nodes in every round
constexpr int kProposeMaxK = 16;              // candidates per query at the most
constexpr int kProposeStageSlots = 4;         // pinned ring of queries: rounds in flight before the host waits for one
constexpr int kProposeStageItems = 2048;      // queries a slot of the ring holds = the most one round (one launch) takes

struct GraphProposeQuery { int seq, j; };     // as the caller lists them: queries[n][2]
struct GraphProposeArgs {
  int n;
  const GraphProposeQuery* queries;  // [n]
  const aloam_graph_node* nodes;     // [B][max_nodes]
  int max_nodes;
  int pose;                          // ALOAM_GRAPH_POSE_ENTERED / ALOAM_GRAPH_POSE_OPTIMIZED
  double radius_m, growth_m_per_node;
  int min_gap, half_window, separation, K;
  aloam_graph_loop_request* dst;     // [n][K]
  int* counts;                       // [n]
  double* dist2;                     // [n][K] or nullptr
};
void launch_graph_propose(const GraphProposeArgs& a, hipStream_t stream);

}  // namespace aloam
