// a-loam_amd/csrc/graphmapjoint_kernels.hpp — the map of joined sequences (aloam_graph_export_map_joint): what
// capi_graphmapjoint.hip hands to graphmapjoint_kernels.hip.  A group is a list of parts, a part a node range of any sequence under an
// optional frame; the two passes over the piece table are restated for parts, everything behind them (directory, segments, voxel filter,
// offsets, emit) is graphmap_kernels.hpp's and runs as it is, indexed by group instead of by request.
#pragma once
#include <hip/hip_runtime.h>

#include "graphmap_kernels.hpp"

namespace aloam {

// The points of part p and class cls are one range of the sequence's class row, cut into pieces of kGmPiece points as a request's are; the
// piece index that goes into the directory key counts on from the pieces the host's bounds gave the parts before it in its (group, class):
// sorted by (group, class, cube, piece) the entries of a cube are in member order across parts.
struct GmPart {
  int seq, first, count, frame;  // frame: -1 = the poses as stored, else an index into `frames`
  int group, pose;               // the group it belongs to; ALOAM_GRAPH_POSE_* of that group
  int piece_base[2];             // first piece index of this part inside its (group, class)
  long long at[2];               // where its class ranges start in `world` / `slot` (laid out for the host's bounds)
};
static_assert(sizeof(GmPart) == 48, "48-byte parts");
constexpr int kGmPieceIndexMax = 1 << 16;                  // piece indices gm_dir_key has room for

struct GmPartsArgs {
  int n_parts, n_groups;
  const GmPart* parts;           // [n_parts]
  const double* frames;          // [n_frames][7] (q_A xyzw, t_A), nullptr when no part names one
  const int* piece_first;        // [2 n_parts + 1] first piece of every (part, class), as the host's bounds lay them out
  int n_pieces;
  KfStore kf;
  const aloam_graph_node* nodes; int max_nodes;
  float4* world;                 // transformed points
  int* slot;                     // directory slot of every transformed point, -1 outside the atlas range
  unsigned long long* dir_key;   // [dir_mask + 1] open addressing, linear probing
  int* dir_count;                // members per slot (transform); append cursors (grouping, zeroed in between)
  const long long* dir_base;     // [dir_mask + 1] where a slot's members start in `grouped` (from the host's sort)
  unsigned dir_mask;
  int* outside;                  // [n_groups]
  int* flags;                    // [0] != 0: the directory overflowed
  float4* grouped;
};
void launch_graph_map_transform_parts(const GmPartsArgs& a, hipStream_t s);
void launch_graph_map_group_parts(const GmPartsArgs& a, hipStream_t s);

}  // namespace aloam
