// a-loam_amd/csrc/graphrecord_kernels.hpp — layout and launchers of the graph records (aloam_graph_save / aloam_graph_load):
// the pose graph of a sequence and, with the keyframe store, the clouds of its nodes, in a position-independent byte layout, packed and
// unpacked on the device in stream order.  What capi_graphrecords.hip hands to graphrecord_kernels.hip.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/aloam_mi355x.h"
#include "checkpoint_kernels.hpp"
#include "export_kernels.hpp"
#include "graphmap_kernels.hpp"

namespace aloam {

static_assert(sizeof(aloam_graph_record_header) == 128, "the record header is 128 bytes");
static_assert(sizeof(aloam_graph_node) == 128 && sizeof(aloam_graph_edge) == 240, "nodes are 8 and edges 15 units of 16 bytes");
constexpr int kGraphRecHeaderUnits = sizeof(aloam_graph_record_header) / 16;
constexpr int kGraphRecNodeUnits = sizeof(aloam_graph_node) / 16;
constexpr int kGraphRecEdgeUnits = sizeof(aloam_graph_edge) / 16;

// Byte offsets of the sections of one record, from its counts.  Every section is a whole number of 16-byte units:
//   header | nodes[N] | edges[E]  [ | KfDesc[N] | corner points | surf points ]  | zeros up to a multiple of kRecAlign.
struct GraphRecLayout { long long nodes, edges, desc, corner, surf, end, bytes; };
__host__ __device__ inline GraphRecLayout graph_rec_layout(bool keyframes, long long nodes, long long edges, long long corner_points, long long surf_points) {
  GraphRecLayout L{};
  L.nodes = sizeof(aloam_graph_record_header);
  L.edges = L.nodes + (long long)sizeof(aloam_graph_node) * nodes;
  L.end = L.edges + (long long)sizeof(aloam_graph_edge) * edges;
  L.desc = L.corner = L.surf = L.end;
  if (keyframes) {
    L.corner = L.desc + (long long)sizeof(KfDesc) * nodes;
    L.surf = L.corner + 16ll * corner_points;
    L.end = L.surf + 16ll * surf_points;
  }
  L.bytes = (L.end + kRecAlign - 1) / kRecAlign * kRecAlign;
  return L;
}

// One record of a save or a load as the kernels see it (staged by the host; the point totals are filled in by k_graph_rec_count in a save,
// taken from the checked header in a load).
struct GraphRecItem { int seq, nodes, edges, corner_points, surf_points, pad0, pad1, pad2; };
static_assert(sizeof(GraphRecItem) == 32, "two units per item");

// The verdict of k_graph_rec_check about one record's payload: 0, or the rules it breaks.
enum GraphRecVerdict {
  kGraphRecBadHeader = 1,          // the counts are negative or do not give the record's length: the payload was not looked at (the host names the field)
  kGraphRecBadEdgeIndex = 2,       // an edge outside -1 <= i < nodes, 0 <= j < nodes, i != j
  kGraphRecBadEdgeFlags = 4,       // a flag outside ALOAM_GRAPH_EDGE_ROBUST
  kGraphRecBadDescChain = 8,       // a descriptor that does not start where the one before ends, or a negative count
  kGraphRecBadDescTotal = 16       // the last descriptor does not end at the header's kf_points
};

// The rows of the store, writable (the load) or read (the save).
struct GraphRecStore {
  aloam_graph_node* nodes; aloam_graph_edge* edges;          // [B][max_nodes], [B][max_edges]
  int max_nodes, max_edges;
  bool keyframes;                                            // the records hold the keyframe part
  KfStore kf;
  unsigned int line_res_bits, plane_res_bits;                // 0 without the keyframe part
};

// Save: count -> scan -> offsets + pack, on stream s.
struct GraphRecSaveArgs {
  int n;
  GraphRecItem* items;                                       // [n] seq, nodes, edges from the host; points from the count
  GraphRecStore store;
  int* units;                                                // [n]      record lengths in 16-byte units (k_export_scan's segment counts)
  int* chunk_off;                                            // [n + 1]  chunks of kExportChunk units before each record
  long long* unit_off;                                       // [n + 1]  units before each record
  long long* dst_off;                                        // the caller's byte offsets (device address)
  char* dst; long long cap_bytes;                            // nullptr / 0: the size query
};
void launch_graph_save(const GraphRecSaveArgs& a, int pack_blocks, hipStream_t s);

// Load, before the host decides: the header of every record gathered into `headers`, and one verdict word per record.  The offsets have been
// checked on the host (ascending, whole records of at least a header): nothing outside [off[i], off[i + 1]) is read.
struct GraphRecCheckArgs {
  int n;
  const char* src; const long long* off;                     // device addresses; off [n + 1]
  aloam_graph_record_header* headers;                        // [n] pinned host memory through its device mapping
  int* verdicts;                                             // [n] idem
};
void launch_graph_check(const GraphRecCheckArgs& a, hipStream_t s);

// Load, behind the host's checks: record i into slot items[i].seq.
struct GraphRecLoadArgs {
  int n;
  const char* src; const long long* off;                     // [n + 1]
  const int* chunk_off;                                      // [n + 1]
  const GraphRecItem* items;                                 // [n] the target slot and the checked counts
  GraphRecStore store;
};
void launch_graph_load(const GraphRecLoadArgs& a, int copy_blocks, hipStream_t s);

}  // namespace aloam
