// a-loam_amd/csrc/graphtrim_kernels.hip — gfx950 kernels of the in-place trim of pose graphs (aloam_graph_trim).  A translation
// unit of its own, so that every other kernel is compiled exactly as before; an anchored edge's Z' = X_opt[i] o Z is formed with the device
// functions k_loop_gather composes poses with (quat_mul, quat_rotate, through map_search_device.hpp).
//   k_trim_cloud_head   grid (listed sequence x class, kTrimHeadBlocks).  With d = desc[first].first[cls] and m = cursor[cls] - d it moves the
//                       points p in [0, min(d, m)) from p + d: source [d, d + min(d, m)) and destination [0, min(d, m)) are disjoint, so
//                       the workgroups need no order.  16-byte accesses, kTrimHeadUnroll loads in flight per lane.
//   k_trim_cloud_tail   one workgroup per (listed sequence, class), behind the head.  It moves the points p in [d, m) from p + d in ascending
//                       chunks of kTrimChunk and exits at once when m <= d (a trim that drops at least half of the points).
//   k_graph_trim        one workgroup of kGraphThreads per listed sequence, queued last.  Edges in tiles of 256, one 240-byte record per
//                       thread: classified, an anchored one composed with the estimate of its dropped node (the node row has not moved
//                       yet), ranked by wave64 ballot + mbcnt and a scan over the four waves, stored at the tile's output base + rank.
//                       Then the node row and the descriptor row shift down by `first` records (the descriptors with first -= d), then
//                       the cursors and the eight integers of the result.
// The hazard argument, the same for every in-place move here.  A step loads [s + k, s + k + L) and stores [s, s + L) (k = d points, `first`
// records; for the edges the stores of a tile end at or below the tile's own base).  (1) Within a step every load is complete before any
// store: each wave executes s_waitcnt vmcnt(0) - which also covers the loads whose values it has not used yet - and then the workgroup's
// barrier, and the stores stand behind the barrier.  The wait is written out because __syncthreads() alone orders LDS and waits for no
// outstanding global load; it was chosen over staging the step through LDS because the step is then bounded by registers, not by 160 KiB
// shared with nothing, and the registers were needed anyway.  (2) Across steps the loads run ahead of the stores by k >= 0: step s + 1 loads
// at or above the end of step s's stores, so nothing written in a launch is ever read in it - no store has to become visible to a later
// load, which is also why the per-CU L1 cannot serve a stale line here - and step s + 1's stores come behind barrier s + 1, which every
// wave reaches only with its loads of step s long complete.  There is no communication between workgroups inside a launch, no spinning
// and no floating-point atomic; the three kernels are ordered by the stream.  Every store to global memory is a vector store.
#include "graphtrim_kernels.hpp"

#include "map_search_device.hpp"             // quat_mul, quat_rotate only

namespace aloam {

namespace {

constexpr int kEdgeUnits = sizeof(aloam_graph_edge) / 16, kNodeUnits = sizeof(aloam_graph_node) / 16;
static_assert(sizeof(aloam_graph_edge) == 240 && sizeof(aloam_graph_node) == 128 && sizeof(KfDesc) == 16, "records are moved as 16-byte units");
typedef unsigned int unit_t __attribute__((ext_vector_type(4)));   // a 16-byte unit of a record or a point, moved as bits
enum TrimClass { kTrimKept = 0, kTrimAnchored = 1, kTrimKeptOnFirst = 2, kTrimReverse = 3, kTrimFixed = 4, kTrimNone = 5 };

// Every vector memory operation this wave has issued has completed.  In front of the barrier: then every load of the workgroup has.
__device__ __forceinline__ void loads_complete() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

__device__ __forceinline__ double unit_double(unsigned lo, unsigned hi) { return __hiloint2double((int)hi, (int)lo); }
__device__ __forceinline__ unit_t unit_of(double a, double b) {
  return unit_t{(unsigned)__double2loint(a), (unsigned)__double2hiint(a), (unsigned)__double2loint(b), (unsigned)__double2hiint(b)};
}

// The rules of the header, in its order; f > 0.
__device__ __forceinline__ int trim_class(int i, int j, int f) {
  if (j > f && (i >= f || i == -1)) return kTrimKept;
  if (j > f && i >= 0 && i < f) return kTrimAnchored;
  if (i > f && j == f) return kTrimKeptOnFirst;
  if (i > f && j >= 0 && j < f) return kTrimReverse;
  return kTrimFixed;
}

// d and m of a (listed sequence, class) as the two cloud kernels and k_graph_trim read them: desc[first] and the cursor are rewritten only by
// the last statements of k_graph_trim, which is queued behind both cloud kernels.
__device__ __forceinline__ void trim_range(const GraphTrimArgs& a, const GraphTrimItem& it, int cls, int& d, int& m) {
  d = a.kf.desc[(long long)it.seq * a.kf.max_nodes + it.first].first[cls];
  m = a.kf.counters[(long long)it.seq * kKfInts + kKfCursor + cls] - d;
}

}  // namespace

__global__ __launch_bounds__(kGraphThreads) void k_trim_cloud_head(GraphTrimArgs a) {
  const int cls = blockIdx.x & 1, tid = threadIdx.x;
  const GraphTrimItem it = a.items[blockIdx.x >> 1];
  if (it.first == 0) return;                                                   // (uniform) nothing of this sequence changes
  int d, m;
  trim_range(a, it, cls, d, m);
  const int n = d < m ? d : m;
  unit_t* row = reinterpret_cast<unit_t*>(a.kf.points[cls] + (long long)it.seq * a.kf.cap[cls]);
  constexpr int kStep = kTrimHeadUnroll * kGraphThreads;
  for (long long base = (long long)blockIdx.y * kStep; base < n; base += (long long)gridDim.y * kStep) {
    unit_t v[kTrimHeadUnroll];
#pragma unroll
    for (int u = 0; u < kTrimHeadUnroll; ++u) {
      const long long p = base + u * kGraphThreads + tid;
      v[u] = row[(p < n ? p : n - 1) + d];                                     // every lane loads, clamped: p + d < min(d, m) + d <= the cursor
    }
#pragma unroll
    for (int u = 0; u < kTrimHeadUnroll; ++u) {
      const long long p = base + u * kGraphThreads + tid;
      if (p < n) row[p] = v[u];
    }
  }
}

__global__ __launch_bounds__(kGraphThreads) void k_trim_cloud_tail(GraphTrimArgs a) {
  const int cls = blockIdx.x & 1, tid = threadIdx.x;
  const GraphTrimItem it = a.items[blockIdx.x >> 1];
  if (it.first == 0) return;
  int d, m;
  trim_range(a, it, cls, d, m);
  if (d == 0 || m <= d) return;                                                // (uniform) nothing moves, or the head moved everything
  unit_t* row = reinterpret_cast<unit_t*>(a.kf.points[cls] + (long long)it.seq * a.kf.cap[cls]);
  constexpr int kPer = kTrimChunk / kGraphThreads;
  for (int base = d; base < m; base += kTrimChunk) {
    unit_t v[kPer];
#pragma unroll
    for (int u = 0; u < kPer; ++u) {
      const int p = base + u * kGraphThreads + tid;
      v[u] = row[(p < m ? p : m - 1) + d];                                     // every lane loads, clamped: p + d < m + d = the cursor
    }
    loads_complete();
    __syncthreads();                                                           // the chunk is in registers; only now may [base, base + kTrimChunk) be written
#pragma unroll
    for (int u = 0; u < kPer; ++u) {
      const int p = base + u * kGraphThreads + tid;
      if (p < m) row[p] = v[u];
    }
  }
}

__global__ __launch_bounds__(kGraphThreads) void k_graph_trim(GraphTrimArgs a) {
  __shared__ int s_wave[2][kGraphThreads / 64];                                // kept edges per wave, by the tile's parity
  __shared__ int s_stat[3];                                                    // anchored, removed_fixed, removed_reverse
  const int w = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const GraphTrimItem it = a.items[w];
  const int f = it.first;
  int* out = a.out + (long long)w * kTrimRecordInts;
  if (f == 0) {                                                                // (uniform) nothing of this sequence changes
    if (tid < kTrimRecordInts) out[tid] = tid == 0 ? it.nodes : tid == 1 ? it.edges : 0;
    return;
  }
  aloam_graph_node* N = a.nodes + (long long)it.seq * a.max_nodes;
  aloam_graph_edge* E = a.edges + (long long)it.seq * a.max_edges;
  KfDesc* D = a.kf.desc ? a.kf.desc + (long long)it.seq * a.kf.max_nodes : nullptr;
  int d[2] = {0, 0}, m[2] = {0, 0};
  if (D) { trim_range(a, it, 0, d[0], m[0]); trim_range(a, it, 1, d[1], m[1]); }
  if (tid < 3) s_stat[tid] = 0;
  __syncthreads();
  // ---- the edges, a stable compaction in tiles of one record per thread
  int out_base = 0, anchored = 0, fixed = 0, reverse = 0;
  for (int base = 0, par = 0; base < it.edges; base += kGraphThreads, par ^= 1) {
    const int e = base + tid;
    unit_t r[kEdgeUnits];
    int cls = kTrimNone;
    {
      const unit_t* src = reinterpret_cast<const unit_t*>(E + (e < it.edges ? e : it.edges - 1));   // every lane loads, clamped
#pragma unroll
      for (int k = 0; k < kEdgeUnits; ++k) r[k] = src[k];
    }
    if (e < it.edges) {
      const int i = (int)r[0].y, j = (int)r[0].z;
      cls = trim_class(i, j, f);
      if (cls == kTrimAnchored) {                                              // Z' = X_opt[i] o Z = (q_i q_Z, q_i t_Z + t_i), stored as computed
        const aloam_graph_node& x = N[i];
        const double qi[4] = {x.q_opt[0], x.q_opt[1], x.q_opt[2], x.q_opt[3]};
        const double qz[4] = {unit_double(r[1].x, r[1].y), unit_double(r[1].z, r[1].w), unit_double(r[2].x, r[2].y), unit_double(r[2].z, r[2].w)};
        double qo[4], to[3];
        quat_mul(qi, qz, qo);
        quat_rotate(qi, unit_double(r[3].x, r[3].y), unit_double(r[3].z, r[3].w), unit_double(r[4].x, r[4].y), to);
        to[0] = to[0] + x.t_opt[0]; to[1] = to[1] + x.t_opt[1]; to[2] = to[2] + x.t_opt[2];
        r[1] = unit_of(qo[0], qo[1]); r[2] = unit_of(qo[2], qo[3]); r[3] = unit_of(to[0], to[1]);
        r[4].x = (unsigned)__double2loint(to[2]); r[4].y = (unsigned)__double2hiint(to[2]);
      }
      r[0].y = (unsigned)((cls == kTrimAnchored || i < 0) ? -1 : i - f);
      r[0].z = (unsigned)(j - f);
      anchored += cls == kTrimAnchored; fixed += cls == kTrimFixed; reverse += cls == kTrimReverse;
    }
    const bool keep = cls <= kTrimKeptOnFirst;
    const unsigned long long mask = __ballot(keep);
    const int rank = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
    if (lane == 0) s_wave[par][wave] = __popcll(mask);
    loads_complete();
    __syncthreads();                                                           // the tile (and the nodes it composed with) is in registers: its outputs land at or below its base
    int before = 0, total = 0;
#pragma unroll
    for (int v = 0; v < kGraphThreads / 64; ++v) { const int c = s_wave[par][v]; before += v < wave ? c : 0; total += c; }
    if (keep) {
      unit_t* dst = reinterpret_cast<unit_t*>(E + out_base + before + rank);
#pragma unroll
      for (int k = 0; k < kEdgeUnits; ++k) dst[k] = r[k];
    }
    out_base += total;                                                         // (s_wave[par] is written again two tiles on, behind the next tile's barrier)
  }
  if (anchored) atomicAdd(&s_stat[0], anchored);
  if (fixed) atomicAdd(&s_stat[1], fixed);
  if (reverse) atomicAdd(&s_stat[2], reverse);
  // ---- the node row and the descriptor row, down by f records; no anchored edge reads a node behind this barrier
  const int kept = it.nodes - f;
  for (int base = 0; base < kept; base += kGraphThreads) {
    const int n = base + tid;
    unit_t r[kNodeUnits];
    unit_t ds = {0u, 0u, 0u, 0u};
    {
      const int at = (n < kept ? n : kept - 1) + f;                            // every lane loads, clamped
      const unit_t* src = reinterpret_cast<const unit_t*>(N + at);
#pragma unroll
      for (int k = 0; k < kNodeUnits; ++k) r[k] = src[k];
      if (D) ds = *reinterpret_cast<const unit_t*>(D + at);
    }
    loads_complete();
    __syncthreads();
    if (n < kept) {
      unit_t* dst = reinterpret_cast<unit_t*>(N + n);
#pragma unroll
      for (int k = 0; k < kNodeUnits; ++k) dst[k] = r[k];
      if (D) { ds.x -= (unsigned)d[0]; ds.y -= (unsigned)d[1]; *reinterpret_cast<unit_t*>(D + n) = ds; }
    }
  }
  // ---- the cursors and the result (kept >= 1: the loop above has passed a barrier behind the counters' adds)
  if (tid == 0) {
    if (D) {
      int* cnt = a.kf.counters + (long long)it.seq * kKfInts;
      cnt[kKfCursor] = m[0]; cnt[kKfCursor + 1] = m[1];
    }
    out[0] = kept; out[1] = out_base; out[2] = s_stat[0]; out[3] = s_stat[1]; out[4] = s_stat[2]; out[5] = d[0]; out[6] = d[1]; out[7] = 0;
    out[kTrimInts] = m[0]; out[kTrimInts + 1] = m[1];
  }
}

void launch_graph_trim(const GraphTrimArgs& a, hipStream_t stream) {
  if (a.n <= 0) return;
  if (a.kf.desc) {
    hipLaunchKernelGGL(k_trim_cloud_head, dim3(2 * a.n, kTrimHeadBlocks), dim3(kGraphThreads), 0, stream, a);
    hipLaunchKernelGGL(k_trim_cloud_tail, dim3(2 * a.n), dim3(kGraphThreads), 0, stream, a);
  }
  hipLaunchKernelGGL(k_graph_trim, dim3(a.n), dim3(kGraphThreads), 0, stream, a);
}

}  // namespace aloam
