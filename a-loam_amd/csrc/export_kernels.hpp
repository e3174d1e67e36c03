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

// ---- device helpers of the export, shared with the sequence records (checkpoint_kernels.hip) ---------------------------------------
__device__ __forceinline__ int ceil_chunks(int n) { return (n + kExportChunk - 1) / kExportChunk; }

// n points from s to d: tiles of 8 x 256 points with the 8 loads of a thread in flight before its stores (named registers: a local array
// indexed in an unrolled loop was left in scratch memory), the rest point by point.  Consecutive lanes take consecutive points.
__device__ __forceinline__ void copy_points(float4* d, const float4* s, int n) {
  const int tid = threadIdx.x;
  int base = 0;
  for (; base + 8 * 256 <= n; base += 8 * 256) {
    const float4* sp = s + base + tid;
    float4* dp = d + base + tid;
    const float4 v0 = sp[0], v1 = sp[256], v2 = sp[512], v3 = sp[768], v4 = sp[1024], v5 = sp[1280], v6 = sp[1536], v7 = sp[1792];
    dp[0] = v0; dp[256] = v1; dp[512] = v2; dp[768] = v3; dp[1024] = v4; dp[1280] = v5; dp[1536] = v6; dp[1792] = v7;
  }
  for (int k = base + tid; k < n; k += 256) d[k] = s[k];
}

// Last index j in [lo, hi) with v[j] <= x (v non-decreasing, v[lo] <= x).
template <typename T>
__device__ __forceinline__ int last_le(const T* v, int lo, int hi, long long x) {
  while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (v[mid] <= x) lo = mid; else hi = mid; }
  return lo;
}

// The part of [q0, q1) (float4s of a record: the chunk a workgroup holds) that falls into [lo, lo + n): its start and length, 0 if none.
__device__ __forceinline__ int overlap(long long q0, long long q1, long long lo, int n, long long* at) {
  const long long a = q0 > lo ? q0 : lo, b = q1 < lo + n ? q1 : lo + n;
  *at = a;
  return b > a ? (int)(b - a) : 0;
}

void launch_export_poses(const OdomState* odom, const MapSeq* mapseq, int B, aloam_pose_record* dst, hipStream_t s);
// count (+ cube prefixes) -> scan -> gather, all on stream s.  gather_blocks: workgroups of the persistent gather.
void launch_export_clouds(const ExportArgs& a, int gather_blocks, hipStream_t s);
// k_export_scan alone (one workgroup): a.seg_cnt of a.n_ids * a.nseq segments -> a.seg_off, a.dst_off and a.chunk_off.
void launch_export_scan(const ExportArgs& a, hipStream_t s);

}  // namespace aloam
