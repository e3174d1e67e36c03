// a-loam_amd/csrc/loopreg_kernels.hpp — batched keyframe registration: loop edges measured on the device (aloam_graph_loops_enable /
// aloam_graph_register_loops): what capi_loopreg.hip hands to loopreg_kernels.hip.  A request registers the clouds of node j
// against the clouds of nodes [first, first + count) of the same sequence, moved into the frame of node i; it runs in a scratch SLOT, and
// the slots are the "sequences" of a scratch MapArgs, so that association, fit, solve and information are the mapping step's own kernels.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/aloam_mi355x.h"
#include "aloam_device.hpp"
#include "graphmap_kernels.hpp"
#include "mapping_kernels.hpp"

namespace aloam {

constexpr int kLoopMaxRequests = 1 << 15;                  // slots of one context
constexpr long long kLoopTargetMax = 1LL << 24;            // raw target points of one class and slot
constexpr int kLoopGatherBlocks = 16;                      // workgroups per (slot, class) of the gather
constexpr int kLoopStageSlots = 4;                         // pinned ring of requests: rounds in flight before the host waits for one

struct LoopArgs {
  int n;                                                   // slots in use this round
  const aloam_graph_loop_request* req;                     // [n] checked, the guess normalised
  KfStore kf;
  const aloam_graph_node* nodes; int max_nodes;
  MapArgs map;                                             // the scratch: B = n, seq / stack / grid_* / knn / edges / norms / rec_tiles are the slots'
  float4* raw[2]; long long raw_cap[2];                    // [slots][raw_cap[cls]] the target before the filter
  float4* target[2];                                       // [slots][raw_cap[cls]] the filtered target, in the frame of node i
  int* plan;                                               // [slots][kLoopPlanInts]
  int outer_iterations;
  const aloam_pose_information* info;                      // [n] k_pose_information_map's record of every slot
  aloam_graph_loop_result* dst;                            // [n] as the device reaches it
};
constexpr int kLoopPlanInts = 8;                           // status before the solve, raw target corner / surf, source corner / surf, three spare

void launch_loop_gather(const LoopArgs& a, const VoxArgs& v, hipStream_t s);
int prepare_loop_grid(int H);
void launch_loop_grid(const LoopArgs& a, hipStream_t s);
void launch_loop_result(const LoopArgs& a, hipStream_t s);
// the filtered target of one (slot, class): *count always, the points when they fit cap (dst == nullptr: the count only)
void launch_loop_export_target(const MapSeq* ms, int cls, const float4* src, float4* dst, long long cap, int* count, hipStream_t s);

}  // namespace aloam
