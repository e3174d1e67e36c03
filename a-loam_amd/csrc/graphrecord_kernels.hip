// a-loam_amd/csrc/graphrecord_kernels.hip — gfx950 kernels of the graph records.
//   k_graph_rec_count    save: per record the point totals from the last node's descriptor, and the record's length in 16-byte units
//   k_graph_rec_offsets  save: the caller's byte offsets from the scanned lengths (k_export_scan of export_kernels.hip ran in between)
//   k_graph_rec_pack     save: persistent and chunked like k_export_gather; a workgroup copies what of the header, the nodes, the edges, the
//                        descriptors, the points and the zero padding falls into its chunk of kExportChunk units
//   k_graph_rec_check    load, before the host decides: one workgroup per record gathers the header and reduces the payload's index rules
//                        (edges inside the nodes, descriptors back to back) to one verdict word
//   k_graph_rec_unpack   load: the same chunks into the target slot's rows; an edge's seq is rewritten in the unit that holds its first 16
//                        bytes; the workgroup that holds a record's first chunk sets the slot's two append cursors
// Integer work and 16-byte copies, coalesced across the wave: HBM- and latency-bound, no MFMA, no LDS but the verdict word, no
// floating-point atomics.  All stores are plain vector stores.
#include "graphrecord_kernels.hpp"

namespace aloam {

namespace {

__device__ __forceinline__ GraphRecLayout layout_of(const GraphRecItem& it, bool keyframes) {
  return graph_rec_layout(keyframes, it.nodes, it.edges, it.corner_points, it.surf_points);
}

// The same layout in 16-byte units, as ints (a record is shorter than 2^31 units: its length is one of k_export_scan's segment counts), and
// the part of a chunk [q0, q1) that falls into a section: the persistent loops keep these in scalar registers.
struct UnitLayout { int nodes, edges, desc, corner, surf, end, total; };
__device__ __forceinline__ UnitLayout unit_layout(const GraphRecItem& it, bool keyframes) {
  const GraphRecLayout L = layout_of(it, keyframes);
  return UnitLayout{(int)(L.nodes / 16), (int)(L.edges / 16), (int)(L.desc / 16), (int)(L.corner / 16), (int)(L.surf / 16), (int)(L.end / 16), (int)(L.bytes / 16)};
}
__device__ __forceinline__ int part(int q0, int q1, int lo, int n, int* at) {
  long long a;
  const int m = overlap(q0, q1, lo, n, &a);
  *at = (int)a;
  return m;
}

// Unit k (16 bytes) of the header of a record, built in registers (selects: a struct indexed at run time would live in scratch).
__device__ __forceinline__ int4 header_unit(int k, long long bytes, const GraphRecItem& it, const GraphRecStore& st) {
  const int parts = ALOAM_GRAPH_PART_GRAPH | (st.keyframes ? ALOAM_GRAPH_PART_KEYFRAMES : 0);
  if (k == 0) return make_int4((int)ALOAM_GRAPH_RECORD_MAGIC, ALOAM_GRAPH_RECORD_VERSION, (int)(bytes & 0xffffffffll), (int)(bytes >> 32));
  if (k == 1) return make_int4(parts, it.nodes, it.edges, it.corner_points);
  if (k == 2) return make_int4(it.surf_points, it.seq, (int)st.line_res_bits, (int)st.plane_res_bits);
  if (k == 3) return make_int4((int)sizeof(aloam_graph_node), (int)sizeof(aloam_graph_edge), (int)sizeof(KfDesc), 16);
  return make_int4(0, 0, 0, 0);
}

__device__ __forceinline__ const float4* units(const void* p) { return static_cast<const float4*>(p); }
__device__ __forceinline__ float4* units(void* p) { return static_cast<float4*>(p); }

}  // namespace

// ---- save -------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_graph_rec_count(GraphRecSaveArgs a) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= a.n) return;
  GraphRecItem it = a.items[i];
  it.corner_points = it.surf_points = 0;
  if (a.store.keyframes && it.nodes > 0) {                   // every descriptor carries the row's fill position: the last one ends the clouds
    const KfDesc d = a.store.kf.desc[(long long)it.seq * a.store.kf.max_nodes + it.nodes - 1];
    it.corner_points = d.first[0] + d.count[0]; it.surf_points = d.first[1] + d.count[1];
  }
  a.items[i] = it;
  a.units[i] = (int)(layout_of(it, a.store.keyframes).bytes / 16);
}

__global__ __launch_bounds__(64) void k_graph_rec_offsets(const long long* unit_off, int n, long long* dst_off) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i <= n) dst_off[i] = 16 * unit_off[i];
}

// A record that does not end at or before cap_bytes is skipped whole.
__global__ __launch_bounds__(256) void k_graph_rec_pack(GraphRecSaveArgs a) {
  const int chunks = a.chunk_off[a.n], tid = threadIdx.x;
  int s = 0;
  for (int ch = blockIdx.x; ch < chunks; ch += gridDim.x) {
    s = last_le(a.chunk_off, s, a.n, ch);
    if (16 * a.unit_off[s + 1] > a.cap_bytes) continue;
    const GraphRecItem it = a.items[s];
    const UnitLayout L = unit_layout(it, a.store.keyframes);
    const int q0 = (ch - a.chunk_off[s]) * kExportChunk, q1 = min(q0 + kExportChunk, L.total);
    float4* d = units(a.dst) + a.unit_off[s];
    const long long b = it.seq;
    if (q0 == 0 && tid < kGraphRecHeaderUnits) reinterpret_cast<int4*>(d)[tid] = header_unit(tid, 16ll * L.total, it, a.store);
    int at, n;
    if ((n = part(q0, q1, L.nodes, kGraphRecNodeUnits * it.nodes, &at)))
      copy_points(d + at, units(a.store.nodes + b * a.store.max_nodes) + (at - L.nodes), n);
    if ((n = part(q0, q1, L.edges, kGraphRecEdgeUnits * it.edges, &at)))
      copy_points(d + at, units(a.store.edges + b * a.store.max_edges) + (at - L.edges), n);
    if (a.store.keyframes) {
      if ((n = part(q0, q1, L.desc, it.nodes, &at)))
        copy_points(d + at, units(a.store.kf.desc + b * a.store.kf.max_nodes) + (at - L.desc), n);
      if ((n = part(q0, q1, L.corner, it.corner_points, &at)))
        copy_points(d + at, a.store.kf.points[0] + b * a.store.kf.cap[0] + (at - L.corner), n);
      if ((n = part(q0, q1, L.surf, it.surf_points, &at)))
        copy_points(d + at, a.store.kf.points[1] + b * a.store.kf.cap[1] + (at - L.surf), n);
    }
    if ((n = part(q0, q1, L.end, L.total - L.end, &at)))
      for (int k = tid; k < n; k += 256) d[at + k] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
}

void launch_graph_save(const GraphRecSaveArgs& a, int pack_blocks, hipStream_t s) {
  if (a.n > 0) hipLaunchKernelGGL(k_graph_rec_count, dim3((a.n + 63) / 64), dim3(64), 0, s, a);
  ExportArgs e{};
  e.n_ids = 1; e.seq0 = 0; e.nseq = a.n;
  e.seg_cnt = a.units; e.chunk_off = a.chunk_off; e.seg_off = a.unit_off; e.dst_off = a.unit_off;
  launch_export_scan(e, s);                                  // also for n = 0: the total
  hipLaunchKernelGGL(k_graph_rec_offsets, dim3(a.n / 64 + 1), dim3(64), 0, s, a.unit_off, a.n, a.dst_off);
  if (a.n > 0 && a.dst && a.cap_bytes > 0) hipLaunchKernelGGL(k_graph_rec_pack, dim3(pack_blocks), dim3(256), 0, s, a);
}

// ---- load -------------------------------------------------------------------------------------------------------------------------------
// The index rules only: what the solve and the gather kernels index with.  The numeric payload is trusted.
__global__ __launch_bounds__(256) void k_graph_rec_check(GraphRecCheckArgs a) {
  __shared__ int s_verdict;
  const int i = blockIdx.x, tid = threadIdx.x;
  const char* r = a.src + a.off[i];
  const long long len = a.off[i + 1] - a.off[i];
  if (tid == 0) s_verdict = 0;
  if (tid < kGraphRecHeaderUnits) reinterpret_cast<int4*>(a.headers + i)[tid] = reinterpret_cast<const int4*>(r)[tid];
  const int4 h1 = reinterpret_cast<const int4*>(r)[1], h2 = reinterpret_cast<const int4*>(r)[2];   // parts, nodes, edges, corner points | surf points ..
  const int parts = h1.x, nodes = h1.y, edges = h1.z, p0 = h1.w, p1 = h2.x;
  const bool keyframes = (parts & ALOAM_GRAPH_PART_KEYFRAMES) != 0;
  const GraphRecLayout L = graph_rec_layout(keyframes, nodes, edges, p0, p1);
  const bool sound = nodes >= 0 && edges >= 0 && p0 >= 0 && p1 >= 0 && (keyframes || (p0 == 0 && p1 == 0)) && L.bytes == len;
  __syncthreads();
  int v = 0;
  if (!sound) {
    v = kGraphRecBadHeader;
  } else {
    for (int e = tid; e < edges; e += 256) {
      const int4 w = *reinterpret_cast<const int4*>(r + L.edges + (long long)sizeof(aloam_graph_edge) * e);   // seq, i, j, flags
      if (w.y < -1 || w.y >= nodes || w.z < 0 || w.z >= nodes || w.y == w.z) v |= kGraphRecBadEdgeIndex;
      if (w.w & ~ALOAM_GRAPH_EDGE_ROBUST) v |= kGraphRecBadEdgeFlags;
    }
    if (keyframes) {
      const int4* D = reinterpret_cast<const int4*>(r + L.desc);   // first[2], count[2]
      for (int k = tid; k < nodes; k += 256) {
        const int4 d = D[k], p = k > 0 ? D[k - 1] : make_int4(0, 0, 0, 0);
        if (d.z < 0 || d.w < 0 || (long long)p.x + p.z != d.x || (long long)p.y + p.w != d.y) v |= kGraphRecBadDescChain;
        if (k == nodes - 1 && ((long long)d.x + d.z != p0 || (long long)d.y + d.w != p1)) v |= kGraphRecBadDescTotal;
      }
      if (nodes == 0 && (p0 != 0 || p1 != 0)) v |= kGraphRecBadDescTotal;
    }
  }
  if (v) atomicOr(&s_verdict, v);
  __syncthreads();
  if (tid == 0) a.verdicts[i] = s_verdict;
}

void launch_graph_check(const GraphRecCheckArgs& a, hipStream_t s) {
  if (a.n > 0) hipLaunchKernelGGL(k_graph_rec_check, dim3(a.n), dim3(256), 0, s, a);
}

__global__ __launch_bounds__(256) void k_graph_rec_unpack(GraphRecLoadArgs a) {
  const int chunks = a.chunk_off[a.n], tid = threadIdx.x;
  int s = 0;
  for (int ch = blockIdx.x; ch < chunks; ch += gridDim.x) {
    s = last_le(a.chunk_off, s, a.n, ch);
    const GraphRecItem it = a.items[s];
    const UnitLayout L = unit_layout(it, a.store.keyframes);
    const int q0 = (ch - a.chunk_off[s]) * kExportChunk, q1 = min(q0 + kExportChunk, L.total);
    const float4* r = units(a.src + a.off[s]);
    const long long slot = it.seq;
    int at, n;
    if ((n = part(q0, q1, L.nodes, kGraphRecNodeUnits * it.nodes, &at)))
      copy_points(units(a.store.nodes + slot * a.store.max_nodes) + (at - L.nodes), r + at, n);
    if ((n = part(q0, q1, L.edges, kGraphRecEdgeUnits * it.edges, &at))) {
      const int k0 = at - L.edges;                  // unit of the edge section this chunk's part starts at
      int4* row = reinterpret_cast<int4*>(a.store.edges + slot * a.store.max_edges);
      const int4* src = reinterpret_cast<const int4*>(r);
#pragma unroll 4
      for (int k = tid; k < n; k += 256) {
        const int4 v = src[at + k];
        const bool first = (k0 + k) % kGraphRecEdgeUnits == 0;   // aloam_graph_edge::seq names the slot that holds the edge
        row[k0 + k] = make_int4(first ? it.seq : v.x, v.y, v.z, v.w);
      }
    }
    if (!a.store.keyframes) continue;
    if ((n = part(q0, q1, L.desc, it.nodes, &at)))
      copy_points(units(a.store.kf.desc + slot * a.store.kf.max_nodes) + (at - L.desc), r + at, n);
    if ((n = part(q0, q1, L.corner, it.corner_points, &at)))
      copy_points(a.store.kf.points[0] + slot * a.store.kf.cap[0] + (at - L.corner), r + at, n);
    if ((n = part(q0, q1, L.surf, it.surf_points, &at)))
      copy_points(a.store.kf.points[1] + slot * a.store.kf.cap[1] + (at - L.surf), r + at, n);
    if (q0 == 0 && tid == 0) {
      int* cn = a.store.kf.counters + slot * kKfInts;
      cn[kKfCursor] = it.corner_points; cn[kKfCursor + 1] = it.surf_points;
    }
  }
}

void launch_graph_load(const GraphRecLoadArgs& a, int copy_blocks, hipStream_t s) {
  if (a.n > 0) hipLaunchKernelGGL(k_graph_rec_unpack, dim3(copy_blocks), dim3(256), 0, s, a);
}

}  // namespace aloam
