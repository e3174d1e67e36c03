// a-loam_amd/csrc/posegraph_kernels.hpp — the pose-graph store and its batched solve (aloam_graph_*): what capi_posegraph.hip
// hands to posegraph_kernels.hip.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/aloam_mi355x.h"
#include "aloam_device.hpp"
#include "mapping_kernels.hpp"

namespace aloam {

constexpr int kGraphThreads = 256;

// One new node: the sequence it reads its pose from, its index in that sequence's row, the index of its odometry edge (unused for node 0)
// and that edge's information.
struct GraphAddItem { int seq, node, edge, pad; double info[21]; };
struct GraphAddArgs {
  int n;
  const GraphAddItem* items;         // [n]
  const OdomState* odom;
  const MapSeq* mapseq;              // nullptr without mapping: the odometry pose is entered
  aloam_graph_node* nodes;           // [B][max_nodes]
  aloam_graph_edge* edges;           // [B][max_edges]
  int max_nodes, max_edges;
};
void launch_graph_add_nodes(const GraphAddArgs& a, hipStream_t stream);

// One listed sequence of a solve with its counts (host state), and the scratch rows of the call: row w belongs to workgroup w.
struct GraphSolveItem { int seq, nodes, edges, pad; };
struct GraphSolveArgs {
  int n;
  const GraphSolveItem* items;       // [n]
  aloam_graph_node* nodes;
  const aloam_graph_edge* edges;
  int max_nodes, max_edges;
  int row_nodes, row_edges;          // the largest counts listed: what a scratch row is laid out for
  aloam_graph_options opt;
  double* f64; long long f64_row;    // [n][f64_row]
  int* i32; long long i32_row;       // [n][i32_row]
  aloam_graph_result* dst;           // [n]
};
inline long long graph_f64_row(int nodes, int edges) { return 200LL * nodes + 115LL * edges; }
inline long long graph_i32_row(int nodes, int edges) { return 3LL * nodes + 1 + 2LL * edges; }
void launch_pose_graph(const GraphSolveArgs& a, hipStream_t stream);

}  // namespace aloam
