// a-loam_amd/csrc/loopsearch_kernels.hpp — a pose grid searched around every loop request's guess (aloam_graph_search_loops, DESIGN.md
// §7q): what capi_loopreg.hip hands to loopsearch_kernels.hip.  The requests sit in the scratch slots of the batched keyframe
// registration, which are the "sequences" of a scratch MapArgs: a slot's stack rows hold node j's clouds, its grid rows the bucketed
// filtered target.  Every node of a slot's grid is scored against them, and the best node's pose becomes the slot's `parameters`.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/aloam_mi355x.h"
#include "mapping_kernels.hpp"

namespace aloam {

// Workgroups per (slot, node): workgroup p takes the tiles of 256 source points p, p + 4, ... of the corner row, then of the surf row.  A
// constant, so that the order in which a node's cost is summed depends on the source clouds alone.  A keyframe's two clouds hold 1 to 5 k
// points, 4 to 20 tiles: with four parts every workgroup has one whole tile at the small end and five at the large one, against the fixed
// work of a workgroup (the node's pose, the reduction, one partial).  The parallelism comes from the nodes - the default grid has 1859 of
// them, 7436 workgroups for ONE request - so more parts would add partials and nothing else.  (kScoreParts = 8 was sized for the mapping
// step's full stacks, five to ten times as large.)
constexpr int kLoopSearchParts = 4;
constexpr int kLoopSearchThreads = 256;
constexpr int kLoopSearchMaxYaw = 31;                      // yaw steps to either side: the (sin, cos) table then fits a launch argument
constexpr int kLoopSearchMaxNodes = 1 << 14;               // nodes of one grid
constexpr long long kLoopSearchMaxPairs = 1ll << 18;       // (slot, node) pairs of one round, as kScoreMaxPairs

struct LoopSearchPartial { int corner_factors, surf_factors, corner_found, surf_found; double cost; int pad[2]; };   // one per workgroup, in a fixed slot
static_assert(sizeof(LoopSearchPartial) == 32 && sizeof(aloam_map_score) == 32 && sizeof(aloam_graph_loop_search_result) == 160, "ABI sizes");

// The grid of every request: m steps of step_m to either side along x and y, a yaw steps of yaw_step_deg to either side; node index
// c = ((iyaw + a) (2m + 1) + (iy + m)) (2m + 1) + (ix + m).  half[iyaw + a] = (sin h, cos h), h = (iyaw * yaw_step_deg * (pi / 180)) / 2,
// computed on the HOST (the C library's sin / cos): the kernels multiply and add only.
struct LoopSearchGrid {
  int m, a, K, pad;
  double step_m;
  double half[2 * kLoopSearchMaxYaw + 1][2];
};

struct LoopSearchArgs {
  int n;                                                   // slots in use this round
  int splits, kper;                                        // node ranges per slot (n < 8: a slot's nodes are dealt over 8 / n XCDs), nodes per range
  const aloam_graph_loop_request* req;                     // [n] checked, the guess normalised
  MapArgs map;                                             // the scratch of the registration: seq / stack / grid_* are the slots'
  const int* plan; int plan_ints;                          // [slots][plan_ints]: [0] the status known before any point is touched
  LoopSearchGrid grid;
  LoopSearchPartial* part;                                 // [n][K][kLoopSearchParts]
  aloam_map_score* scores;                                 // [n][K] as the device reaches it, or nullptr
  aloam_graph_loop_search_result* dst;                     // [n] as the device reaches it
};
static_assert(sizeof(LoopSearchArgs) <= 4096, "the arguments of k_loop_search must fit the kernel argument segment");

void launch_loop_search(const LoopSearchArgs& a, hipStream_t s);

}  // namespace aloam
