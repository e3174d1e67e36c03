// a-loam_amd/csrc/graphapply_kernels.hpp — a solved pose graph carried into the live pose and the window map (aloam_graph_apply,
// DESIGN.md §7m): what capi_graphapply.hip hands to graphapply_kernels.hip.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/aloam_mi355x.h"
#include "aloam_device.hpp"
#include "atlas_kernels.hpp"
#include "graphmap_kernels.hpp"
#include "mapping_kernels.hpp"

namespace aloam {

// One listed sequence.  nodes: what its graph holds (host state, so stream-ordered like the counts of aloam_graph_add_nodes); gm: the index
// of its request in the map pass that ran before (the scratch of aloam_graph_export_map), -1 without ALOAM_GRAPH_APPLY_MAP.
struct GaItem { int seq, first, count, flags, nodes, gm, pad[2]; };
static_assert(sizeof(GaItem) == 32, "32-byte items");

struct GraphApplyArgs {
  int n;
  const GaItem* items;           // [n]
  aloam_graph_node* nodes; int max_nodes;
  MapSeq* seq;
  CubeDesc* cubes;               // [B][2][kMapCubes]
  float4* pool[2]; int pool_cap; // the class pools, points per sequence
  // the map pass: per request the range of its segments (sorted by class, then cube), per segment its cube, where its filtered points
  // start in `grouped` and how many they are
  const GmRequestOut* req;
  const AtlasMergeJob* jobs;
  const GmSegInfo* seg;
  const int* counts;
  const float4* grouped;
  aloam_graph_apply_result* dst; // [n]
};
void launch_graph_apply(const GraphApplyArgs& a, hipStream_t s);

}  // namespace aloam
