// a-loam_amd/csrc/graphmap_kernels.hpp — the keyframe store of the pose graphs and the map assembled from it at the graph's poses
// (aloam_graph_keyframes_enable / aloam_graph_export_keyframes / aloam_graph_export_map): what capi_graphmap.hip hands to
// graphmap_kernels.hip.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/aloam_mi355x.h"
#include "aloam_device.hpp"
#include "atlas_kernels.hpp"
#include "mapping_kernels.hpp"
#include "posegraph_kernels.hpp"

namespace aloam {

// ---- the store -------------------------------------------------------------------------------------------------------------------------
// One descriptor per node: where its corner / surf cloud sits in the sequence's class rows.  Clouds are appended back to back, so
// first[cls] of node k is first[cls] + count[cls] of node k - 1 (0 for node 0), also behind a node that was kept without clouds (count 0).
// Invariant that readers rely on (k_graph_map_transform, k_keyframe_export, and k_loop_gather of loopreg_kernels.hip, which takes a class's
// raw target as first + count of the last node minus first of the first): EVERY node's descriptor carries the row's fill position in
// first[cls], a node kept without clouds included, so the clouds of nodes a .. b are the one range [first_a, first_b + count_b) of the row.
struct KfDesc { int first[2], count[2]; };
static_assert(sizeof(KfDesc) == 16, "16-byte descriptors");
// Per sequence: the append cursors (points held, corner / surf), nodes kept without clouds and their points so far, four spare.
constexpr int kKfInts = 8;
enum KfCounter { kKfCursor = 0, kKfDroppedNodes = 2, kKfDroppedPoints = 3 };

struct KfStore {
  float4* points[2];             // [B][cap[cls]] sensor-frame points
  KfDesc* desc;                  // [B][max_nodes]
  int* counters;                 // [B][kKfInts]
  int cap[2];
  int max_nodes;
};

// aloam_graph_add_nodes, behind k_graph_add_nodes: the stacks of the listed sequences become the clouds of their new nodes.
struct KfCaptureArgs {
  int n;
  const GraphAddItem* items;     // [n] (seq, node) of the call
  const MapSeq* mapseq;          // n_stack
  const float4* stack[2];        // laserCloudCornerStack / SurfStack, rows of stack_row[cls] points
  long long stack_row[2];
  KfStore kf;
};
void launch_keyframe_capture(const KfCaptureArgs& a, hipStream_t s);

struct KfExportArgs {
  const KfDesc* desc;            // the sequence's row
  const float4* points;          // its row of the class
  int first, count, cls;
  float4* dst; long long cap;    // dst == nullptr: offsets only
  long long* dst_off;            // [count + 1]
};
void launch_keyframe_export(const KfExportArgs& a, hipStream_t s);

// ---- the map at the graph's poses ------------------------------------------------------------------------------------------------------
// The points of request r and class cls are one range of the sequence's class row (nodes first .. first + count - 1 back to back).  It is
// cut into pieces of kGmPiece points; piece p of (r, cls) is the work of one wave in the transform and in the grouping pass, and the
// directory counts the members of a cube per piece: sorted by (request, class, cube, piece) its entries are in member order.
constexpr int kGmPiece = 4096;
constexpr unsigned long long kGmEmpty = ~0ull;
__host__ __device__ inline unsigned long long gm_dir_key(int group, int cube_key, int piece) {   // group = 2 * request + class
  return ((unsigned long long)group << 46) | ((unsigned long long)cube_key << 16) | (unsigned long long)piece;
}
constexpr int kGmMaxRequests = 1 << 15;
constexpr long long kGmDirMax = 1LL << 22;                 // slots of the largest directory
constexpr long long kKfRowMax = 1LL << 26;                 // points of a keyframe row (aloam_graph_keyframes_enable)
static_assert(kKfRowMax / kGmPiece <= (1 << 16), "a (request, class) range is at most one row: its piece index fits the 16 bits gm_dir_key gives it");
static_assert(2 * kGmMaxRequests <= (1 << 16), "group = 2 * request + class fits bits 46 .. 61 of gm_dir_key, below the empty key");

struct GmRequest {
  int seq, first, count, pose;
  long long at[2];               // where its class ranges start in `world` / `slot` (laid out for the host's bounds)
};
struct GmArgs {
  int n;                         // requests
  const GmRequest* req;          // [n]
  const int* piece_first;        // [2 n + 1] first piece of every (request, class) group, as the host's bounds lay them out
  int n_pieces;
  KfStore kf;
  const aloam_graph_node* nodes; int max_nodes;
  float4* world;                 // transformed points
  int* slot;                     // directory slot of every transformed point, -1 outside the atlas range
  unsigned long long* dir_key;   // [dir_mask + 1] open addressing, linear probing
  int* dir_count;                // members per slot (transform); append cursors (grouping, zeroed in between)
  const long long* dir_base;     // [dir_mask + 1] where a slot's members start in `grouped` (from the host's sort)
  unsigned dir_mask;
  int* outside;                  // [n]
  int* flags;                    // [0] != 0: the directory overflowed
  float4* grouped;
};
void launch_graph_map_transform(const GmArgs& a, hipStream_t s);
void launch_graph_map_group(const GmArgs& a, hipStream_t s);

// Emit: per request the range of its segments (sorted by class, then cube) and what the host knows of it.
struct GmRequestOut { int seg_first, surf_first, raw[2]; };
struct GmSegInfo { int cube_key, req; };
struct GmEmitArgs {
  int n, n_segs;
  const GmRequestOut* req;       // [n + 1] (the last: seg_first = n_segs)
  const AtlasMergeJob* jobs;     // [n_segs] first / cls of every segment
  const GmSegInfo* seg;          // [n_segs]
  const int* counts;             // [n_segs] filtered sizes
  long long* point_off;          // [n_segs + 1] scratch
  const int* outside;            // [n]
  const float4* grouped;
  aloam_map_tile* tiles_dst; long long cap_tiles;
  float4* points_dst; long long cap_points;
  long long* dst_off;            // [2][n + 1]
  aloam_graph_map_stats* stats;  // [n] or nullptr
};
void launch_graph_map_emit(const GmEmitArgs& a, hipStream_t s);

}  // namespace aloam
