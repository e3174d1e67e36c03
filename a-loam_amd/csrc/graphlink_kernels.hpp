// a-loam_amd/csrc/graphlink_kernels.hpp — links measured on the device (aloam_graph_register_links / aloam_graph_search_links /
// aloam_graph_propose_links): what the host hands to graphlink_kernels.hip.  A link request registers the clouds of node j of
// sequence seq_j against the clouds of nodes [first, first + count) of sequence seq_i, moved into the frame of node i.  It runs in a scratch
// slot of the batched keyframe registration: the gather of this unit writes what that feature's own gather writes, into the same scratch,
// so the voxel filter, the grid build, the search, association, fit, solve, information and the result run behind it as they are.  The
// unit declares arguments of its own (the scratch as pointers, the plan row's stride as a number), as loopsearch_kernels.hpp does.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/aloam_mi355x.h"
#include "graphmap_kernels.hpp"
#include "graphpropose_kernels.hpp"
#include "mapping_kernels.hpp"

namespace aloam {

constexpr int kLinkGatherBlocks = 16;                      // workgroups per (slot, class) of the gather
constexpr int kLinkCopyChunk = 2048;                       // source points a workgroup copies at a time

struct LinkGatherArgs {
  int n;                                                   // slots in use this round
  const aloam_graph_link_request* req;                     // [n] checked, the guess normalised
  KfStore kf;
  const aloam_graph_node* nodes; int max_nodes;
  MapArgs map;                                             // the scratch of the registration: seq / stack are the slots'
  float4* raw[2]; long long raw_cap[2];                    // [slots][raw_cap[cls]] the target before the filter
  float4* target[2];                                       // [slots][raw_cap[cls]] the filtered target, in the frame of node i
  int* plan; int plan_ints;                                // [slots][plan_ints]: status, raw target corner / surf, source corner / surf, spare
};
void launch_link_gather(const LinkGatherArgs& a, const VoxArgs& v, hipStream_t s);

// A query as the host stages it: the caller's (seq_j, j, seq_i), the node count of seq_i at the time of the call, and the frame A.
struct LinkProposeQuery {
  int seq_j, j, seq_i, nodes_i;
  int has_frame, pad;
  double frame[7];                                         // q_A (normalised), t_A; zero without a frame
};
static_assert(sizeof(LinkProposeQuery) == 80, "a staged query is ten 8-byte words");
struct LinkProposeArgs {
  int n;
  const LinkProposeQuery* queries;   // [n]
  const aloam_graph_node* nodes;     // [B][max_nodes]
  int max_nodes;
  int pose;                          // ALOAM_GRAPH_POSE_ENTERED / ALOAM_GRAPH_POSE_OPTIMIZED
  double radius2;                    // radius_m * radius_m, one rounded f64 product, formed by the host
  int half_window, separation, K;
  aloam_graph_link_request* dst;     // [n][K]
  int* counts;                       // [n]
  double* dist2;                     // [n][K] or nullptr
};
void launch_link_propose(const LinkProposeArgs& a, hipStream_t stream);

}  // namespace aloam
