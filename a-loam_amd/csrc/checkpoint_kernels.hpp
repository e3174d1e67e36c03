// a-loam_amd/csrc/checkpoint_kernels.hpp — layouts and launchers of the sequence records (aloam_save_sequences / aloam_load_sequences): the
// whole state of a sequence between two frames in a position-independent byte layout, packed and unpacked on the device in stream order.
#pragma once
#include "../../include/aloam_mi355x.h"
#include "aloam_device.hpp"
#include "export_kernels.hpp"
#include "mapping_kernels.hpp"

namespace aloam {

static_assert(sizeof(aloam_seq_record_header) == 128, "the record header is 128 bytes");
static_assert(sizeof(SeqMeta) % 16 == 0 && sizeof(OdomState) % 16 == 0 && sizeof(MapSeq) % 16 == 0, "fixed sections are whole float4s");
constexpr int kRecAlign = 256;                            // every record starts and ends on this (bytes)
constexpr int kRecInfo = 8;                               // ints per record of the scratch: n_corner_last, n_surf_last, n_cubes[2], map_points[2], slot, 0

// Byte offsets of the sections of one record, from its counts.  All 16-byte aligned:
//   header | SeqMeta | OdomState | corner_last | surf_last  [ | MapSeq | tab | live (4 ints) | corner (cube, count) pairs | corner points
//   | surf pairs | surf points ]  | zeros up to a multiple of kRecAlign.
struct RecLayout { long long meta, odom, corner, surf, mapseq, tab, live, list[2], pts[2], end, bytes; };
__host__ __device__ inline long long rec_align16(long long x) { return (x + 15) & ~15ll; }
__host__ __device__ inline RecLayout rec_layout(bool map, int n_corner, int n_surf, const int n_cubes[2], const int n_points[2]) {
  RecLayout L{};
  L.meta = sizeof(aloam_seq_record_header);
  L.odom = L.meta + sizeof(SeqMeta);
  L.corner = L.odom + sizeof(OdomState);
  L.surf = L.corner + 16ll * n_corner;
  L.end = L.surf + 16ll * n_surf;
  if (map) {
    L.mapseq = L.end;
    L.tab = L.mapseq + sizeof(MapSeq);
    L.live = L.tab + sizeof(int) * kTabInts;
    long long p = L.live + 16;
    for (int k = 0; k < 2; ++k) {
      L.list[k] = p;
      L.pts[k] = L.list[k] + rec_align16(8ll * n_cubes[k]);
      p = L.pts[k] + 16ll * n_points[k];
    }
    L.end = p;
  }
  L.bytes = (L.end + kRecAlign - 1) / kRecAlign * kRecAlign;
  return L;
}

// Save: seqs[0 .. n) of the context into dst (the device address of the caller's buffer; nullptr for the size query).
struct CkptSaveArgs {
  const int* seqs; int n;
  int R, cap;
  const SeqMeta* meta; const OdomState* state;
  const float4* less_sharp[2]; const float4* less_flat[2];   // the last clouds of sequence b are row [1 - SeqMeta::parity]; nullptr: no odometry part
  const MapSeq* mapseq;                                      // nullptr: no map part
  const CubeDesc* cubes; const int* tab; const int* live;
  const float4* pool[2]; long long pool_cap;
  aloam_seq_record_header hdr;                               // the configuration fields of every header; the counts are filled in per record
  int* info;                                                 // [n][kRecInfo] scratch
  int* units;                                                // [n]      record lengths in float4s (k_export_scan's segment counts)
  int* chunk_off;                                            // [n + 1]  chunks of kExportChunk float4s before each record
  long long* unit_off;                                       // [n + 1]  float4s before each record
  int* cube_pref;                                            // [n][2][kMapCubes + 1] exclusive prefix of the cube counts per class
  long long* dst_off;                                        // the caller's byte offsets (device address)
  char* dst; long long cap_bytes;
};
// count -> scan -> pack, on stream s.  pack_blocks: workgroups of the persistent copy.
void launch_save_sequences(const CkptSaveArgs& a, int pack_blocks, hipStream_t s);

// Load: record i (at src + off[i], checked on the host) into slot info[i][6], after k_reset_sequences has run on the slots.
struct CkptLoadArgs {
  const char* src; const long long* off;                     // device addresses (record bytes: device memory, pinned host memory or staging)
  const int* info; const int* chunk_off; int n;              // [n][kRecInfo], [n + 1]: staged by the host from the validated headers
  int R, cap;
  SeqMeta* meta; OdomState* state;
  float4* corner_last; float4* surf_last;                    // row 1 of the double-buffered clouds (a reset slot has parity 0); nullptr: no odometry part
  MapSeq* mapseq;                                            // nullptr: no map part
  CubeDesc* cubes; int* tab; int* live;
  float4* pool[2]; long long pool_cap;
};
void launch_load_sequences(const CkptLoadArgs& a, int copy_blocks, hipStream_t s);
// The headers of records src + off[0 .. n) (device addresses, the offsets already checked on the host) into out[0 .. n).
void launch_read_headers(const char* src, const long long* off, int n, aloam_seq_record_header* out, hipStream_t s);

}  // namespace aloam
