// a-loam_amd/csrc/places_kernels.hpp — layouts and launchers of place recognition (aloam_places_*): the Scan Context descriptor of a
// sweep (Kim & Kim, IROS 2018) made from the ring slabs, the place store, and the match of descriptors against ranges of the store on
// the f32-input matrix cores.
#pragma once
#include "../../include/aloam_mi355x.h"
#include "aloam_device.hpp"
#include "mapping_kernels.hpp"

namespace aloam {

constexpr int kPlaceRings = ALOAM_PLACE_RINGS, kPlaceSectors = ALOAM_PLACE_SECTORS;
constexpr int kPlaceCells = kPlaceRings * kPlaceSectors;      // 1200, sector-major: cell (ring r, sector s) at s * 20 + r
constexpr int kPlaceDescThreads = 512;
constexpr int kPlaceMatchThreads = 256;                       // 4 waves, each 64 shifts x 32 entries
constexpr int kPlaceTile = 128;                               // entries per k_place_match workgroup
constexpr int kPlaceMaxT = 8;
static_assert(sizeof(aloam_place) == 4880 && sizeof(aloam_place_match) == 16, "ABI sizes");
static_assert(kPlaceCells % 8 == 0, "the K loop of k_place_match takes 8 cells per step");

// The descriptor of the sweep a sequence holds: what k_place_descriptor writes, one per sequence.
struct alignas(16) PlaceDesc {
  float cells[kPlaceCells];          // raw cells, sector-major
  float norms[kPlaceSectors];        // Euclidean norm of every column (sector), summed over the rings in ascending order
  unsigned long long mask;           // bit s: column s is non-zero
  int n_points;                      // points of the sweep (SeqMeta::n_cloud)
  int pad;
};

struct PlaceDescArgs {
  int B, R, slab;
  const float4* slabs;               // [B][R][slab]
  const int* ringstart;              // [B][R + 1]
  const int* wanted;                 // [B] != 0: this sequence's descriptor is asked for and not yet made; the others are neither read nor written
  float ring_scale, height;          // 20 / max_range; sensor_height
  PlaceDesc* desc;                   // [B]
};

struct PlaceAddArgs {
  int n, first;                      // listed sequences; store index of the first new entry
  const int* seqs;                   // [n]
  const PlaceDesc* desc;             // [B]
  const OdomState* odom;             // [B]
  const MapSeq* mapseq;              // [B] or nullptr without mapping
  aloam_place* store;                // [capacity]
  float* unit;                       // [capacity][1200] unit-normalised columns
  unsigned long long* masks;         // [capacity]
};

struct PlaceMatchArgs {
  int n, T, max_range;               // listed sequences; results per sequence; the longest [lo, hi)
  const int* seqs;                   // [n]
  const int* lo;                     // [n] first entry of each sequence's range
  const int* hi;                     // [n] one past its last
  const PlaceDesc* desc;             // [B]
  const float* unit;                 // [capacity][1200]
  const unsigned long long* masks;   // [capacity]
  int2* pairs;                       // [n][max_range] {distance bits, shift or -1} per entry of the range
  aloam_place_match* dst;            // [n][T]
};

void launch_place_descriptor(const PlaceDescArgs& a, hipStream_t s);
void launch_place_add(const PlaceAddArgs& a, hipStream_t s);
// unit / masks of store entries [first, first + count) from their raw cells (after a load)
void launch_place_finish(const aloam_place* store, float* unit, unsigned long long* masks, int first, int count, hipStream_t s);
void launch_place_match(const PlaceMatchArgs& a, hipStream_t s);

}  // namespace aloam
