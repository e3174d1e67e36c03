// a-loam_amd/csrc/export_kernels.hip — the batched export: the poses of every sequence (k_export_poses) and any set of its clouds packed
// back to back (k_export_count -> k_export_cube_count -> k_export_scan -> k_export_gather), written in stream order into device memory or
// the device mapping of pinned host memory.  Nothing here synchronises with the host; the host learns the sizes from the offsets it gets.
#include "export_kernels.hpp"

namespace aloam {

// ---- poses: one lane per sequence -----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_export_poses(const OdomState* odom, const MapSeq* mapseq, int B, aloam_pose_record* dst) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  const OdomState& s = odom[b];
  aloam_pose_record r;
  for (int k = 0; k < 4; ++k) { r.q_w[k] = s.q_w[k]; r.q_last_curr[k] = s.para_q[k]; }
  for (int k = 0; k < 3; ++k) { r.t_w[k] = s.t_w[k]; r.t_last_curr[k] = s.para_t[k]; }
  if (mapseq) {                                          // what aloam_get_map_pose reads: `parameters` and the map <- odom correction
    const MapSeq& m = mapseq[b];
    for (int k = 0; k < 4; ++k) { r.map_q_w[k] = m.par[k]; r.q_wmap_wodom[k] = m.q_wmap_wodom[k]; }
    for (int k = 0; k < 3; ++k) { r.map_t_w[k] = m.par[4 + k]; r.t_wmap_wodom[k] = m.t_wmap_wodom[k]; }
    r.map_frames = m.frame_count;
  } else {
    for (int k = 0; k < 4; ++k) { r.map_q_w[k] = 0.0; r.q_wmap_wodom[k] = 0.0; }
    for (int k = 0; k < 3; ++k) { r.map_t_w[k] = 0.0; r.t_wmap_wodom[k] = 0.0; }
    r.map_frames = -1;
  }
  r.inited = s.inited;
  r.pad[0] = r.pad[1] = 0;
  dst[b] = r;
}

// ---- clouds ------------------------------------------------------------------------------------------------------------------------
// Points of every plain segment: the getters' own counts (SeqMeta for the ALOAM_CLOUD_* ids and REGISTERED, MapSeq::n_stack for the stacks).
__global__ __launch_bounds__(256) void k_export_count(ExportArgs a) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= a.n_ids * a.nseq) return;
  const ExportSrc& src = a.src[g / a.nseq];
  if (src.kind != kExportPlain) return;                  // k_export_cube_count writes those
  const long long b = a.seq0 + g % a.nseq;
  a.seg_cnt[g] = src.count[b * src.count_stride];
}

// Cube of entry e of a cube list (corner then surf per cube): the window of the last step in the reference's i, j, k order, or every cube.
__device__ __forceinline__ int entry_cube(int kind, const int* window, int e) { return kind == kExportFull ? e >> 1 : window[e >> 1]; }
__device__ __forceinline__ int entry_max(int kind) { return kind == kExportFull ? kExportFullEntries : kExportSurroundEntries; }

// One workgroup per sequence and cube-list id: the prefix of its entries (what the gather walks) and the segment's point count.
__global__ __launch_bounds__(256) void k_export_cube_count(ExportArgs a, int i) {
  __shared__ int s_scan[256];
  const int bl = blockIdx.x, tid = threadIdx.x;
  const long long b = a.seq0 + bl;
  const int kind = a.src[i].kind;
  const int E = kind == kExportFull ? kExportFullEntries : 2 * a.mapseq[b].n_valid;
  const int* window = a.tab + b * kTabInts;
  const CubeDesc* T = a.cubes + b * 2 * kMapCubes;
  int* pref = (kind == kExportFull ? a.cube_pref[1] : a.cube_pref[0]) + (long long)bl * (entry_max(kind) + 1);
  const int per = (E + 255) / 256, lo = min(E, tid * per), hi = min(E, lo + per);
  int sum = 0;
  for (int e = lo; e < hi; ++e) sum += T[(e & 1) * kMapCubes + entry_cube(kind, window, e)].cnt;
  int total = 0;
  int run = block_exclusive_scan<int, 256>(sum, s_scan, &total);
  for (int e = lo; e < hi; ++e) {
    pref[e] = run;
    run += T[(e & 1) * kMapCubes + entry_cube(kind, window, e)].cnt;
  }
  if (tid == 0) { pref[E] = total; a.seg_cnt[i * a.nseq + bl] = total; }
}

// One workgroup: point offsets (scratch + the caller's copy) and chunk offsets of all segments.  Each thread owns a run of consecutive segments.
__global__ __launch_bounds__(1024) void k_export_scan(ExportArgs a) {
  __shared__ long long s_p[1024];
  __shared__ int s_c[1024];
  const int S = a.n_ids * a.nseq, tid = threadIdx.x;
  const int per = (S + 1023) / 1024, lo = min(S, tid * per), hi = min(S, lo + per);
  long long sp = 0;
  int sc = 0;
  for (int s = lo; s < hi; ++s) { const int n = a.seg_cnt[s]; sp += n; sc += ceil_chunks(n); }
  long long total_p = 0;
  int total_c = 0;
  long long run_p = block_exclusive_scan<long long, 1024>(sp, s_p, &total_p);
  int run_c = block_exclusive_scan<int, 1024>(sc, s_c, &total_c);
  for (int s = lo; s < hi; ++s) {
    const int n = a.seg_cnt[s];
    a.seg_off[s] = run_p; a.dst_off[s] = run_p; a.chunk_off[s] = run_c;
    run_p += n; run_c += ceil_chunks(n);
  }
  if (tid == 0) { a.seg_off[S] = total_p; a.dst_off[S] = total_p; a.chunk_off[S] = total_c; }
}

// Persistent segmented copy: the workgroups take chunks of <= kExportChunk points in turn; a chunk finds its segment by binary search over the
// chunk offsets (the segments of one workgroup's chunks only move forward).  A segment that does not end at or before cap_points is skipped whole.
__global__ __launch_bounds__(256) void k_export_gather(ExportArgs a) {
  const int S = a.n_ids * a.nseq, chunks = a.chunk_off[S];
  int s = 0;
  for (int ch = blockIdx.x; ch < chunks; ch += gridDim.x) {
    s = last_le(a.chunk_off, s, S, ch);                  // empty segments share their chunk offset with the next: the last one is the owner
    const long long off = a.seg_off[s];
    if (a.seg_off[s + 1] > a.cap_points) continue;
    const ExportSrc& src = a.src[s / a.nseq];
    const int bl = s % a.nseq;
    const long long b = a.seq0 + bl;
    const int p0 = (ch - a.chunk_off[s]) * kExportChunk, p1 = min(p0 + kExportChunk, a.seg_cnt[s]);
    float4* d = a.dst + off;
    if (src.kind == kExportPlain) {
      const int row = src.sel == kSelFixed ? 0 : src.sel == kSelCurrent ? a.meta[b].parity : 1 - a.meta[b].parity;
      copy_points(d + p0, (row ? src.base[1] : src.base[0]) + b * src.stride + p0, p1 - p0);   // (selects: no dynamic index into the arguments)
      continue;
    }
    const int* window = a.tab + b * kTabInts;
    const int E = src.kind == kExportFull ? kExportFullEntries : 2 * a.mapseq[b].n_valid;
    const int* pref = (src.kind == kExportFull ? a.cube_pref[1] : a.cube_pref[0]) + (long long)bl * (entry_max(src.kind) + 1);
    int e = last_le(pref, 0, E, p0);                     // the entry that holds point p0 (empty entries before it share its prefix)
    for (int p = p0; p < p1; ++e) {
      const int q = min(p1, pref[e + 1]);
      if (q > p) {
        const int cls = e & 1;
        const CubeDesc c = a.cubes[(b * 2 + cls) * kMapCubes + entry_cube(src.kind, window, e)];
        copy_points(d + p, (cls ? a.pool[1] : a.pool[0]) + b * a.pool_cap + c.off + (p - pref[e]), q - p);
        p = q;
      }
    }
  }
}

void launch_export_poses(const OdomState* odom, const MapSeq* mapseq, int B, aloam_pose_record* dst, hipStream_t s) {
  hipLaunchKernelGGL(k_export_poses, dim3((B + 63) / 64), dim3(64), 0, s, odom, mapseq, B, dst);
}

void launch_export_scan(const ExportArgs& a, hipStream_t s) { hipLaunchKernelGGL(k_export_scan, dim3(1), dim3(1024), 0, s, a); }

void launch_export_clouds(const ExportArgs& a, int gather_blocks, hipStream_t s) {
  const int S = a.n_ids * a.nseq;
  if (S > 0) hipLaunchKernelGGL(k_export_count, dim3((S + 255) / 256), dim3(256), 0, s, a);
  for (int i = 0; i < a.n_ids; ++i)
    if (a.src[i].kind != kExportPlain) hipLaunchKernelGGL(k_export_cube_count, dim3(a.nseq), dim3(256), 0, s, a, i);
  hipLaunchKernelGGL(k_export_scan, dim3(1), dim3(1024), 0, s, a);   // also for n_ids = 0: the total
  if (S > 0 && a.cap_points > 0) hipLaunchKernelGGL(k_export_gather, dim3(gather_blocks), dim3(256), 0, s, a);
}

}  // namespace aloam
