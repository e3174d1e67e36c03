// a-loam_amd/csrc/checkpoint_kernels.hip — the sequence records.  Save: k_ckpt_count (record sizes, cube prefixes) -> k_export_scan (record
// and chunk offsets) -> k_ckpt_pack_fixed (header, fixed structs, cube lists, the caller's byte offsets) + k_ckpt_pack_points (clouds and cube
// points, persistent and chunked like k_export_gather).  Load, after k_reset_sequences on the slots: k_ckpt_unpack_fixed (structs and the cube
// descriptors of a pool packed back to back) + k_ckpt_unpack_points.  Nothing here synchronises with the host.
#include "checkpoint_kernels.hpp"

namespace aloam {

__device__ __forceinline__ const float4* row_ptr(const float4* const (&buf)[2], int k) { return k ? buf[1] : buf[0]; }

// n 16-byte words from s to d by the threads of a workgroup (the fixed sections: SeqMeta, OdomState, MapSeq, tab).
__device__ __forceinline__ void copy_words(void* d, const void* s, int n) {
  for (int k = threadIdx.x; k < n; k += 256) static_cast<int4*>(d)[k] = static_cast<const int4*>(s)[k];
}

__device__ __forceinline__ RecLayout layout_of(const int* info, bool map) {
  const int nc[2] = {info[2], info[3]}, np[2] = {info[4], info[5]};
  return rec_layout(map, info[0], info[1], nc, np);
}

// ---- save -------------------------------------------------------------------------------------------------------------------
// One workgroup per record: the last clouds' sizes, and per class the exclusive prefix of the cube counts over the 4851 descriptors (what
// the pack walks), their total and the number of non-empty cubes.
__global__ __launch_bounds__(256) void k_ckpt_count(CkptSaveArgs a) {
  __shared__ int s_scan[256];
  const int i = blockIdx.x, tid = threadIdx.x;
  const long long b = a.seqs[i];
  int nc[2] = {0, 0}, np[2] = {0, 0};
  if (a.mapseq) {
    const int per = (kMapCubes + 255) / 256, lo = min(kMapCubes, tid * per), hi = min(kMapCubes, lo + per);
    for (int cls = 0; cls < 2; ++cls) {
      const CubeDesc* T = a.cubes + (b * 2 + cls) * kMapCubes;
      int* pref = a.cube_pref + ((long long)i * 2 + cls) * (kMapCubes + 1);
      static_assert((kMapCubes + 255) / 256 == 19, "19 descriptors per thread");
      int cnt[19], sum = 0, nz = 0;
#pragma unroll
      for (int k = 0; k < 19; ++k) { cnt[k] = lo + k < hi ? T[lo + k].cnt : 0; sum += cnt[k]; nz += cnt[k] > 0; }
      int total = 0, nz_total = 0;
      int run = block_exclusive_scan<int, 256>(sum, s_scan, &total);
      (void)block_exclusive_scan<int, 256>(nz, s_scan, &nz_total);
#pragma unroll
      for (int k = 0; k < 19; ++k) if (lo + k < hi) { pref[lo + k] = run; run += cnt[k]; }
      if (tid == 0) pref[kMapCubes] = total;
      np[cls] = total; nc[cls] = nz_total;
    }
  }
  if (tid == 0) {
    const SeqMeta& m = a.meta[b];
    int* info = a.info + (long long)i * kRecInfo;
    info[0] = a.less_sharp[0] || a.less_sharp[1] ? m.n_corner_last : 0;
    info[1] = a.less_sharp[0] || a.less_sharp[1] ? m.n_surf_last : 0;
    info[2] = nc[0]; info[3] = nc[1]; info[4] = np[0]; info[5] = np[1]; info[6] = (int)b; info[7] = 0;
    a.units[i] = (int)(layout_of(info, a.mapseq != nullptr).bytes / 16);
  }
}

// One workgroup per record: the caller's byte offsets (always), then - when the record ends at or before cap_bytes - the header, the fixed
// sections, the (cube, count) pairs of the non-empty cubes in index order and the zero padding.
__global__ __launch_bounds__(256) void k_ckpt_pack_fixed(CkptSaveArgs a) {
  __shared__ int s_scan[256];
  const int i = blockIdx.x, tid = threadIdx.x;
  const long long u0 = a.unit_off[i], u1 = a.unit_off[i + 1];
  if (tid == 0) {
    a.dst_off[i] = 16 * u0;
    if (i == a.n - 1) a.dst_off[a.n] = 16 * u1;
  }
  if (!a.dst || 16 * u1 > a.cap_bytes) return;
  const int* info = a.info + (long long)i * kRecInfo;
  const long long b = info[6];
  const bool map = a.mapseq != nullptr;
  const RecLayout L = layout_of(info, map);
  char* r = a.dst + 16 * u0;
  if (tid == 0) {
    aloam_seq_record_header h = a.hdr;
    h.bytes = L.bytes;
    h.inited = a.state[b].inited;
    h.n_corner_last = info[0]; h.n_surf_last = info[1];
    h.n_cubes[0] = info[2]; h.n_cubes[1] = info[3]; h.map_points[0] = info[4]; h.map_points[1] = info[5];
    h.err_events = map ? a.mapseq[b].err_steps + ((a.mapseq[b].err & kMapErrPool) ? 1 : 0) : 0;
    *reinterpret_cast<aloam_seq_record_header*>(r) = h;
  }
  copy_words(r + L.meta, a.meta + b, sizeof(SeqMeta) / 16);
  copy_words(r + L.odom, a.state + b, sizeof(OdomState) / 16);
  if (map) {
    copy_words(r + L.mapseq, a.mapseq + b, sizeof(MapSeq) / 16);
    copy_words(r + L.tab, a.tab + b * kTabInts, kTabInts / 4);
    if (tid == 0) *reinterpret_cast<int4*>(r + L.live) = make_int4(a.live[2 * b], a.live[2 * b + 1], 0, 0);
    const int per = (kMapCubes + 255) / 256, lo = min(kMapCubes, tid * per), hi = min(kMapCubes, lo + per);
    for (int cls = 0; cls < 2; ++cls) {
      const CubeDesc* T = a.cubes + (b * 2 + cls) * kMapCubes;
      int nz = 0;
      for (int e = lo; e < hi; ++e) nz += T[e].cnt > 0;
      int total = 0;
      int at = block_exclusive_scan<int, 256>(nz, s_scan, &total);
      int2* list = reinterpret_cast<int2*>(r + L.list[cls]);
      for (int e = lo; e < hi; ++e) {
        const int n = T[e].cnt;
        if (n > 0) list[at++] = make_int2(e, n);
      }
      if (tid == 0 && (total & 1)) list[total] = make_int2(0, 0);   // the list ends on 16 bytes
    }
  }
  for (long long k = L.end / 16 + tid; k < L.bytes / 16; k += 256) reinterpret_cast<int4*>(r)[k] = make_int4(0, 0, 0, 0);
}

// Persistent chunked copy of the point sections: the workgroups take chunks of <= kExportChunk float4s of the records in turn (binary search
// of the chunk prefix, as k_export_gather), and copy what of the last clouds and the cube points falls into their chunk.  A record that does
// not end at or before cap_bytes is skipped whole.
__global__ __launch_bounds__(256) void k_ckpt_pack_points(CkptSaveArgs a) {
  const int chunks = a.chunk_off[a.n];
  int s = 0;
  for (int ch = blockIdx.x; ch < chunks; ch += gridDim.x) {
    s = last_le(a.chunk_off, s, a.n, ch);
    if (16 * a.unit_off[s + 1] > a.cap_bytes) continue;
    const int* info = a.info + (long long)s * kRecInfo;
    const long long b = info[6];
    const bool map = a.mapseq != nullptr;
    const RecLayout L = layout_of(info, map);
    const long long q0 = (long long)(ch - a.chunk_off[s]) * kExportChunk, q1 = min(q0 + kExportChunk, L.bytes / 16);
    float4* d = reinterpret_cast<float4*>(a.dst) + a.unit_off[s];
    long long at;
    int n;
    if (info[0] + info[1] > 0) {
      const int last = 1 - a.meta[b].parity;
      if ((n = overlap(q0, q1, L.corner / 16, info[0], &at)))
        copy_points(d + at, row_ptr(a.less_sharp, last) + b * a.R * kLessSharpPerRing + (at - L.corner / 16), n);
      if ((n = overlap(q0, q1, L.surf / 16, info[1], &at)))
        copy_points(d + at, row_ptr(a.less_flat, last) + b * a.cap + (at - L.surf / 16), n);
    }
    if (!map) continue;
    for (int cls = 0; cls < 2; ++cls) {
      if (!(n = overlap(q0, q1, L.pts[cls] / 16, info[4 + cls], &at))) continue;
      const CubeDesc* T = a.cubes + (b * 2 + cls) * kMapCubes;
      const int* pref = a.cube_pref + ((long long)s * 2 + cls) * (kMapCubes + 1);
      const float4* pool = (cls ? a.pool[1] : a.pool[0]) + b * a.pool_cap;
      const int p0 = (int)(at - L.pts[cls] / 16), p1 = p0 + n;
      for (int p = p0, e = last_le(pref, 0, kMapCubes, p0); p < p1; ++e) {   // cubes in index order; empty ones share the prefix of the next
        const int q = min(p1, pref[e + 1]);
        if (q > p) {
          copy_points(d + L.pts[cls] / 16 + p, pool + T[e].off + (p - pref[e]), q - p);
          p = q;
        }
      }
    }
  }
}

__global__ __launch_bounds__(64) void k_ckpt_offsets_empty(long long* dst_off) { if (threadIdx.x == 0) dst_off[0] = 0; }   // n = 0: the total only

void launch_save_sequences(const CkptSaveArgs& a, int pack_blocks, hipStream_t s) {
  if (a.n > 0) hipLaunchKernelGGL(k_ckpt_count, dim3(a.n), dim3(256), 0, s, a);
  ExportArgs e{};
  e.n_ids = 1; e.seq0 = 0; e.nseq = a.n;
  e.seg_cnt = a.units; e.chunk_off = a.chunk_off; e.seg_off = a.unit_off; e.dst_off = a.unit_off;
  launch_export_scan(e, s);
  if (a.n > 0) hipLaunchKernelGGL(k_ckpt_pack_fixed, dim3(a.n), dim3(256), 0, s, a);
  else hipLaunchKernelGGL(k_ckpt_offsets_empty, dim3(1), dim3(64), 0, s, a.dst_off);
  if (a.n > 0 && a.dst && a.cap_bytes > 0) hipLaunchKernelGGL(k_ckpt_pack_points, dim3(pack_blocks), dim3(256), 0, s, a);
}

// ---- load -------------------------------------------------------------------------------------------------------------------
// One workgroup per record, after the reset of its slot: SeqMeta as a reset leaves it but for the last clouds' sizes (parity 0: the last
// clouds go to row 1), OdomState and MapSeq as saved with pool_used recomputed, the window table, the live counts, and the descriptors of the
// listed cubes packed back to back in the pool with cap = count (an exclusive scan of the counts in list order).
__global__ __launch_bounds__(256) void k_ckpt_unpack_fixed(CkptLoadArgs a) {
  __shared__ int s_scan[256];
  const int i = blockIdx.x, tid = threadIdx.x;
  const int* info = a.info + (long long)i * kRecInfo;
  const long long slot = info[6];
  const bool map = a.mapseq != nullptr;
  const RecLayout L = layout_of(info, map);
  const char* r = a.src + a.off[i];
  if (tid == 0) {
    SeqMeta m{};
    m.n_corner_last = info[0]; m.n_surf_last = info[1];
    m.parity = 0;
    a.meta[slot] = m;
  }
  copy_words(a.state + slot, r + L.odom, sizeof(OdomState) / 16);
  if (!map) return;
  if (tid == 0) {
    MapSeq ms = *reinterpret_cast<const MapSeq*>(r + L.mapseq);
    ms.pool_used[0] = info[4]; ms.pool_used[1] = info[5];
    a.mapseq[slot] = ms;
    const int4 lv = *reinterpret_cast<const int4*>(r + L.live);
    a.live[2 * slot] = lv.x; a.live[2 * slot + 1] = lv.y;
  }
  copy_words(a.tab + slot * kTabInts, r + L.tab, kTabInts / 4);
  for (int cls = 0; cls < 2; ++cls) {
    const int nc = info[2 + cls], total_pts = info[4 + cls];
    const int2* list = reinterpret_cast<const int2*>(r + L.list[cls]);
    const int per = (nc + 255) / 256, lo = min(nc, tid * per), hi = min(nc, lo + per);
    int sum = 0;
    for (int k = lo; k < hi; ++k) sum += max(0, list[k].y);
    int total = 0;
    int off = block_exclusive_scan<int, 256>(sum, s_scan, &total);
    CubeDesc* T = a.cubes + (slot * 2 + cls) * kMapCubes;
    for (int k = lo; k < hi; ++k) {
      const int2 c = list[k];
      const int cnt = max(0, min(c.y, total_pts - off));       // (a record whose list disagrees with its header stays inside the pool)
      if (c.x >= 0 && c.x < kMapCubes) T[c.x] = CubeDesc{off, cnt, cnt, 0};
      off += max(0, c.y);
    }
  }
}

// Persistent chunked copy of the point sections into the slots: the last clouds into row 1, the cube points of a class back to back from
// the start of the slot's pool row.
__global__ __launch_bounds__(256) void k_ckpt_unpack_points(CkptLoadArgs a) {
  const int chunks = a.chunk_off[a.n];
  int s = 0;
  for (int ch = blockIdx.x; ch < chunks; ch += gridDim.x) {
    s = last_le(a.chunk_off, s, a.n, ch);
    const int* info = a.info + (long long)s * kRecInfo;
    const long long slot = info[6];
    const bool map = a.mapseq != nullptr;
    const RecLayout L = layout_of(info, map);
    const long long q0 = (long long)(ch - a.chunk_off[s]) * kExportChunk, q1 = min(q0 + kExportChunk, L.bytes / 16);
    const float4* r = reinterpret_cast<const float4*>(a.src + a.off[s]);
    long long at;
    int n;
    if (a.corner_last) {
      if ((n = overlap(q0, q1, L.corner / 16, info[0], &at))) copy_points(a.corner_last + slot * a.R * kLessSharpPerRing + (at - L.corner / 16), r + at, n);
      if ((n = overlap(q0, q1, L.surf / 16, info[1], &at))) copy_points(a.surf_last + slot * a.cap + (at - L.surf / 16), r + at, n);
    }
    if (!map) continue;
    for (int cls = 0; cls < 2; ++cls)
      if ((n = overlap(q0, q1, L.pts[cls] / 16, info[4 + cls], &at)))
        copy_points((cls ? a.pool[1] : a.pool[0]) + slot * a.pool_cap + (at - L.pts[cls] / 16), r + at, n);
  }
}

// The n headers of a load (records in device or pinned host memory) gathered into `out` (pinned host memory, through its device mapping).
__global__ __launch_bounds__(64) void k_ckpt_read_headers(const char* src, const long long* off, int n, aloam_seq_record_header* out) {
  const int i = blockIdx.x, k = threadIdx.x;
  constexpr int words = sizeof(aloam_seq_record_header) / 16;
  if (i < n && k < words) reinterpret_cast<int4*>(out + i)[k] = reinterpret_cast<const int4*>(src + off[i])[k];
}
void launch_read_headers(const char* src, const long long* off, int n, aloam_seq_record_header* out, hipStream_t s) {
  if (n > 0) hipLaunchKernelGGL(k_ckpt_read_headers, dim3(n), dim3(64), 0, s, src, off, n, out);
}

void launch_load_sequences(const CkptLoadArgs& a, int copy_blocks, hipStream_t s) {
  if (a.n <= 0) return;
  hipLaunchKernelGGL(k_ckpt_unpack_fixed, dim3(a.n), dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_ckpt_unpack_points, dim3(copy_blocks), dim3(256), 0, s, a);
}

}  // namespace aloam
