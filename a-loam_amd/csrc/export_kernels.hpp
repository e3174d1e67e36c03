// a-loam_amd/csrc/export_kernels.hpp — layouts and launchers of the batched export (aloam_export_poses / aloam_export_clouds): what the
// nodes publish (reference src/laserOdometry.cpp:508-591, src/laserMapping.cpp:803-863), for every sequence of a batch, in stream order.
#pragma once
#include "../../include/aloam_mi355x.h"
#include "aloam_device.hpp"
#include "mapping_kernels.hpp"

namespace aloam {

constexpr int kExportChunk = 4096;                         // points per unit of work of k_export_gather (64 KiB read + 64 KiB written)
constexpr int kExportSurroundEntries = 2 * kMapValidMax;   // (cube, class) entries of /laser_cloud_surround: corner then surf per window cube
constexpr int kExportFullEntries = 2 * kMapCubes;          // ... of /laser_cloud_map: corner then surf for each of the 4851 cubes

// Where one cloud id's points and counts live.  Plain clouds: row b of base[...] holds count[b * count_stride] points.  Cube lists
// (SURROUND, FULL): the points of entry e of sequence b are cube list(e / 2) of class e % 2 in the map pools, and the counts come from the
// cube descriptors.
enum ExportKind { kExportPlain = 0, kExportSurround = 1, kExportFull = 2 };
enum ExportSel { kSelFixed = 0, kSelCurrent = 1, kSelLast = 2 };   // base[0] / base[SeqMeta::parity] / base[1 - SeqMeta::parity]
struct ExportSrc {
  const float4* base[2];
  long long stride;        // points between the rows of two sequences
  const int* count;        // plain: the count of sequence b is count[b * count_stride] (a field of SeqMeta or MapSeq)
  int count_stride;        // in ints
  int sel;                 // ExportSel
  int kind;                // ExportKind
  int pad;
};

struct ExportArgs {
  int n_ids, seq0, nseq;               // segments (i, bl), i < n_ids, bl < nseq, numbered s = i * nseq + bl: cloud ids[i] of sequence seq0 + bl
  ExportSrc src[ALOAM_EXPORT_MAX_IDS];
  const SeqMeta* meta;                 // [B] (parity of every sequence)
  const CubeDesc* cubes;               // [B][2][kMapCubes]
  const int* tab;                      // [B][kTabInts] the last step's window: [0 .. MapSeq::n_valid) = cube ids in the reference's loop order
  const MapSeq* mapseq;                // [B]
  const float4* pool[2];               // [B][pool_cap]
  long long pool_cap;
  int* seg_cnt;                        // [n_ids * nseq]      scratch: points per segment
  int* chunk_off;                      // [n_ids * nseq + 1]  scratch: exclusive prefix of the chunks per segment; [S] = all chunks
  long long* seg_off;                  // [n_ids * nseq + 1]  scratch: exclusive prefix of the points (what the gather reads)
  long long* dst_off;                  // the caller's offsets (device memory or the device mapping of pinned host memory)
  int* cube_pref[2];                   // [nseq][entries + 1] scratch of SURROUND / FULL: exclusive prefix of the entries of a sequence
  float4* dst;                         // the caller's points (idem); nullptr when cap_points == 0
  long long cap_points;
};

void launch_export_poses(const OdomState* odom, const MapSeq* mapseq, int B, aloam_pose_record* dst, hipStream_t s);
// count (+ cube prefixes) -> scan -> gather, all on stream s.  gather_blocks: workgroups of the persistent gather.
void launch_export_clouds(const ExportArgs& a, int gather_blocks, hipStream_t s);

}  // namespace aloam
