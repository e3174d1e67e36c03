// a-loam_amd/csrc/atlas_kernels.hpp — layouts and launchers of the map spill: the cubes a window shift of the mapping step empties
// (reference src/laserMapping.cpp:323-507) are captured as tiles (aloam_map_tile) before k_map_begin shifts, and drained in stream order;
// and of the atlas: the directory of an immutable tile store, the merge jobs of its load, and the window cut of an attached sequence.
#pragma once
#include "../../include/aloam_mi355x.h"
#include "aloam_device.hpp"
#include "mapping_kernels.hpp"

namespace aloam {

static_assert(sizeof(aloam_map_tile) == 32, "aloam_map_tile is 32 bytes");

// Per sequence: tiles held per class, points held per class, tiles and points dropped so far (a tile that did not fit its rows), two spare.
constexpr int kSpillInts = 8;
enum SpillCounter { kSpillTiles = 0, kSpillPoints = 2, kSpillDroppedTiles = 4, kSpillDroppedPoints = 5 };

struct SpillArgs {
  int B;
  const int* active;             // [B] SeqBits of this mapping step, nullptr = all sequences take part
  const int* attached;           // [B] attached to the atlas (aloam_atlas_attach), nullptr = none
  const MapSeq* seq;             // [B]
  const OdomState* odom;         // [B]
  const CubeDesc* cubes;         // [B][2][kMapCubes]
  const float4* pool[2];         // [B][pool_cap]
  long long pool_cap;
  aloam_map_tile* tiles;         // [B][2][max_tiles]   first_point indexes the class row of `points`
  float4* points;                // [B][2][max_points]
  int* counters;                 // [B][kSpillInts]
  int max_tiles, max_points;
};

// aloam_export_map_spill: count -> k_export_scan (tiles), k_export_scan (points) -> gather -> clear.
struct SpillExportArgs {
  const int* seqs; int n;        // [n] distinct sequence ids
  const aloam_map_tile* tiles; const float4* points; int* counters;   // the spill rows, as in SpillArgs
  int max_tiles, max_points;
  const long long* tile_off;     // [n + 1] scratch: what k_export_scan made of the tile counts
  const long long* point_off;    // [n + 1] ... of the point counts
  aloam_map_tile* tiles_dst; long long cap_tiles;
  float4* points_dst; long long cap_points;
};

// ---- the atlas: one immutable tile store per context, shared by its sequences (aloam_atlas_load / aloam_atlas_attach) ------------------
// Directory entry of one (absolute cube, class): open addressing, linear probing, load factor <= 1/2.  key packs the cube (10 bits per axis,
// biased by kAtlasBias) and is -1 for a free slot.
struct AtlasEntry { int key, first, count, pad; };
static_assert(sizeof(AtlasEntry) == 16, "16-byte directory entries");
constexpr int kAtlasBias = 512;                            // absolute cubes -512 .. 511 per axis (25 km either way)
__host__ __device__ inline int atlas_key(int x, int y, int z) { return ((x + kAtlasBias) << 20) | ((y + kAtlasBias) << 10) | (z + kAtlasBias); }
__host__ __device__ inline bool atlas_in_range(int x, int y, int z) {
  return x >= -kAtlasBias && x < kAtlasBias && y >= -kAtlasBias && y < kAtlasBias && z >= -kAtlasBias && z < kAtlasBias;
}
__host__ __device__ inline unsigned atlas_hash(int key) { return (unsigned)key * 2654435761u; }

struct AtlasArgs {
  int B;
  const int* active;             // [B] SeqBits of this mapping step, nullptr = all
  const int* attached;           // [B]
  int* stale;                    // [B] != 0: the window must be cut anew whatever the shift (cleared here)
  MapSeq* seq; const OdomState* odom;
  CubeDesc* cubes;               // [B][2][kMapCubes]
  float4* pool[2]; long long pool_cap;
  MapGridSig* grid_sig;          // [B][2]
  const AtlasEntry* dir[2]; int dir_mask[2];   // per class: the directory (size dir_mask + 1) ...
  const float4* points[2];       // ... and its points
};

// One merge job of aloam_atlas_load: the concatenated tiles of one (cube, class) at points[first .. first + n) are filtered in place.
struct AtlasMergeJob { long long first, tmp_off; int n, cls, count_slot, pad; };   // tmp_off: its staging range in VoxArgs::tmp
struct AtlasMergeArgs {
  const AtlasMergeJob* jobs; int n_jobs;
  float4* points[2];
  int* counts;                   // [.] device ints that receive the filtered sizes
  float leaf[2];
};

void launch_atlas_window(const AtlasArgs& a, hipStream_t s);
void launch_atlas_merge_segments(const AtlasMergeArgs& m, const VoxArgs& v, hipStream_t s);
void launch_map_spill(const SpillArgs& a, hipStream_t s);
void launch_spill_count(const SpillExportArgs& a, int* tile_cnt, int* point_cnt, hipStream_t s);
void launch_spill_gather(const SpillExportArgs& a, bool clear, hipStream_t s);

}  // namespace aloam
