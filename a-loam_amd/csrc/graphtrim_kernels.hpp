// a-loam_amd/csrc/graphtrim_kernels.hpp — trimming pose graphs in place (aloam_graph_trim): what capi_graphtrim.hip hands to
// graphtrim_kernels.hip.
#pragma once
#include "graphmap_kernels.hpp"
#include "posegraph_kernels.hpp"

namespace aloam {

constexpr int kTrimChunk = 2048;              // points the tail kernel's one workgroup holds in registers per step: 8 x 16 bytes per lane
constexpr int kTrimHeadBlocks = 64;           // workgroups per (listed sequence, class) of the head kernel (the grid's y)
constexpr int kTrimHeadUnroll = 4;            // 16-byte loads a lane of the head kernel keeps in flight
constexpr int kTrimStageSlots = 4;            // pinned ring of items: calls in flight before the host waits for one
constexpr int kTrimInts = 8;                  // the result per listed sequence: nodes, edges, anchored, removed_fixed, removed_reverse, corner / surf points freed, 0
constexpr int kTrimRecordInts = 10;           // the pinned staging record: the result, then the points that stayed (corner, surf), for the algorithmic bytes
static_assert(kTrimChunk % kGraphThreads == 0, "a chunk is a whole number of points per lane");

struct GraphTrimItem { int seq, first, nodes, edges; };   // a listed sequence with its counts (host state) before the trim
struct GraphTrimArgs {
  int n;
  const GraphTrimItem* items;        // [n]
  aloam_graph_node* nodes;           // [B][max_nodes]
  aloam_graph_edge* edges;           // [B][max_edges]
  int max_nodes, max_edges;
  KfStore kf;                        // kf.desc == nullptr: the keyframe store is not enabled
  int* out;                          // [n][kTrimRecordInts], pinned host memory as the device sees it
};
// The three launches, in this order: the head and the tail of the point rows read desc[first] and the cursors, which k_graph_trim rewrites.
void launch_graph_trim(const GraphTrimArgs& a, hipStream_t stream);

}  // namespace aloam
