// a-loam_amd/csrc/graphlink_kernels.hip — gfx950 kernels of the links measured on the device (aloam_graph_register_links /
// aloam_graph_search_links / aloam_graph_propose_links).  A translation unit of its own, so that every other kernel is
// compiled exactly as before.  The plan arithmetic, the scan and the arg-min of the per-sequence kernels are restated here because they
// differ in which rows they read: the target and the eligible nodes are seq_i's, the source cloud and the query node are seq_j's.
//   k_link_gather    (16, slot, class) workgroups of 256: the clouds of the target nodes of seq_i moved into the frame of node i
//                    (T_k = X_i^-1 o X_k, once per node and workgroup, by one lane, f64, separately rounded), node j's cloud of seq_j copied
//                    into the slot's stack row, and - by one lane per (slot, class) - the segment of the voxel filter, the slot's zeroed
//                    scratch MapSeq with `parameters` = the guess, and the plan ints.  The descriptors come from two rows: the target
//                    range from seq_i's, the source range and the tests on it from seq_j's.  What it writes is what the per-sequence
//                    gather writes, so everything behind it runs unchanged.
//   k_link_propose   one workgroup of kGraphThreads per query (seq_j, j, seq_i).  One lane forms X_j' (X_j, or A o X_j) and broadcasts it.
//                    Pass 1: the threads stride over ALL nodes of seq_i, form d2 and the radius test in separately rounded f64, and the
//                    hits are compacted as (d2, i) into an LDS list of kProposeHits entries (wave64 ballot + mbcnt ranks; a wave takes its
//                    range of the list with one integer LDS add).  Then up to K rounds of a block arg-min over (d2, i), after each of which
//                    every hit within `separation` of the winner dies; over the list when it holds every hit, else by scanning the nodes
//                    again (the same operations, so the same bits).  Lane k then writes record k, field by field.
// No floating-point atomics.  Points move as 16-byte loads and stores, four loads in flight per lane, at clamped indices so that no load
// stands under a condition, loads ahead of stores.  Every store to global memory is a vector store.
#include "graphlink_kernels.hpp"

#include "map_search_device.hpp"             // quat_mul, quat_rotate, associate_to_map
#include "map_window_device.hpp"             // vox_enlist

namespace aloam {

namespace {

// What a request covers, from the descriptors as they are at this point of the stream (uniform in the workgroup).  A sequence's clouds sit
// back to back in its class rows (graphmap_kernels.hpp), so the target of a class is ONE range of seq_i's row.
struct LinkPlan {
  int status;                      // ALOAM_LOOP_OK, or what is known before any point is touched: NO_CLOUDS, TOO_LARGE
  int base[2], raw[2];             // the target range of every class row of seq_i
  int src[2], src_n[2];            // node j's clouds in the class rows of seq_j
};

__device__ __forceinline__ LinkPlan link_plan(const LinkGatherArgs& a, const aloam_graph_link_request& rq) {
  const KfDesc* Di = a.kf.desc + (long long)rq.seq_i * a.kf.max_nodes;
  const KfDesc* Dj = a.kf.desc + (long long)rq.seq_j * a.kf.max_nodes;
  const KfDesc d0 = Di[rq.first], d1 = Di[rq.first + rq.count - 1], dj = Dj[rq.j];
  LinkPlan p;
  p.base[0] = d0.first[0]; p.base[1] = d0.first[1];
  p.raw[0] = d1.first[0] + d1.count[0] - d0.first[0]; p.raw[1] = d1.first[1] + d1.count[1] - d0.first[1];
  p.src[0] = dj.first[0]; p.src[1] = dj.first[1];
  p.src_n[0] = dj.count[0]; p.src_n[1] = dj.count[1];
  p.status = ALOAM_LOOP_OK;
  if (p.raw[0] > a.raw_cap[0] || p.raw[1] > a.raw_cap[1] || p.src_n[0] > a.map.R * kLessSharpPerRing || p.src_n[1] > a.map.cap) p.status = ALOAM_LOOP_TOO_LARGE;
  if (p.src_n[0] + p.src_n[1] <= 0 || p.raw[0] + p.raw[1] <= 0 || p.raw[0] < 0 || p.raw[1] < 0) p.status = ALOAM_LOOP_NO_CLOUDS;
  return p;
}

__device__ __forceinline__ long long link_stack_row(const MapArgs& m, int cls) { return cls ? (long long)m.cap : (long long)m.R * kLessSharpPerRing; }

constexpr int kLinkUnroll = 4;               // 16-byte loads in flight per lane

}  // namespace

__global__ __launch_bounds__(256) void k_link_gather(LinkGatherArgs a, VoxArgs v) {
  const int s = blockIdx.y, cls = blockIdx.z, tid = threadIdx.x;
  const aloam_graph_link_request rq = a.req[s];
  const LinkPlan pl = link_plan(a, rq);
  const bool ok = pl.status == ALOAM_LOOP_OK;
  float4* raw = (cls ? a.raw[1] + (long long)s * a.raw_cap[1] : a.raw[0] + (long long)s * a.raw_cap[0]);
  MapSeq& ms = a.map.seq[s];
  if (blockIdx.x == 0 && tid == 0) {
    // the segment of this (slot, class): one pcl::VoxelGrid over the whole target cloud of the class, its size into from_total
    VoxSeg sg{};
    sg.in = raw;
    sg.out = (cls ? a.target[1] + (long long)s * a.raw_cap[1] : a.target[0] + (long long)s * a.raw_cap[0]);
    sg.out_count = cls ? &ms.from_total[1] : &ms.from_total[0];
    sg.n = ok ? (cls ? pl.raw[1] : pl.raw[0]) : 0;
    sg.leaf = cls ? a.map.plane_res : a.map.line_res;
    v.segs[2 * s + cls] = sg;
    vox_enlist(v, 2 * s + cls, sg.n);
    if (cls == 0) {
      // the scratch MapSeq: `parameters` = the guess, the stacks = node j's clouds; everything else as a new sequence has it
      static_assert(sizeof(MapSeq) % sizeof(double) == 0 && alignof(MapSeq) >= alignof(double), "the scratch MapSeq is zeroed as doubles");
      double* w = reinterpret_cast<double*>(&ms);
      for (int k = 0; k < (int)(sizeof(MapSeq) / sizeof(double)); ++k) w[k] = 0.0;
      for (int k = 0; k < 4; ++k) ms.par[k] = rq.q[k];
      for (int k = 0; k < 3; ++k) ms.par[4 + k] = rq.t[k];
      ms.q_wmap_wodom[3] = 1.0; ms.q_wodom[3] = 1.0;
      ms.n_stack[0] = ok ? pl.src_n[0] : 0; ms.n_stack[1] = ok ? pl.src_n[1] : 0;
      int* P = a.plan + (long long)s * a.plan_ints;
      P[0] = pl.status; P[1] = pl.raw[0]; P[2] = pl.raw[1]; P[3] = pl.src_n[0]; P[4] = pl.src_n[1]; P[5] = 0; P[6] = 0; P[7] = 0;
    }
  }
  if (!ok) return;                                                             // (uniform)
  // ---- the target: seq_i's nodes, node after node, T_k once per node
  __shared__ double s_par[7];                                                  // q_d, t_d of T_k
  const KfDesc* D = a.kf.desc + (long long)rq.seq_i * a.kf.max_nodes;
  const aloam_graph_node* N = a.nodes + (long long)rq.seq_i * a.max_nodes;
  const float4* row_i = cls ? a.kf.points[1] + (long long)rq.seq_i * a.kf.cap[1] : a.kf.points[0] + (long long)rq.seq_i * a.kf.cap[0];
  const int base = cls ? pl.base[1] : pl.base[0];
  for (int k = rq.first + (int)blockIdx.x; k < rq.first + rq.count; k += (int)gridDim.x) {
    const KfDesc d = D[k];
    const int at = cls ? d.first[1] : d.first[0], cnt = cls ? d.count[1] : d.count[0];
    if (cnt <= 0 || at < base || at - base + cnt > (cls ? pl.raw[1] : pl.raw[0])) continue;   // (uniform; the second: never, while the row is back to back)
    __syncthreads();                                                           // s_par of the node before has been read
    if (tid == 0) {
      // T_k = X_i^-1 o X_k as the header defines a relative pose: q_d = q_i* q_k, t_d = q_i* (t_k - t_i); node i like every other node
      const aloam_graph_node& xi = N[rq.i];
      const aloam_graph_node& xk = N[k];
      double qi[4], qk[4], ti[3], tk[3], qd[4], td[3];
      for (int c = 0; c < 4; ++c) { qi[c] = rq.pose ? xi.q_opt[c] : xi.q[c]; qk[c] = rq.pose ? xk.q_opt[c] : xk.q[c]; }
      for (int c = 0; c < 3; ++c) { ti[c] = rq.pose ? xi.t_opt[c] : xi.t[c]; tk[c] = rq.pose ? xk.t_opt[c] : xk.t[c]; }
      const double qc[4] = {-qi[0], -qi[1], -qi[2], qi[3]};
      quat_mul(qc, qk, qd);
      quat_rotate(qc, tk[0] - ti[0], tk[1] - ti[1], tk[2] - ti[2], td);
      for (int c = 0; c < 4; ++c) s_par[c] = qd[c];
      for (int c = 0; c < 3; ++c) s_par[4 + c] = td[c];
    }
    __syncthreads();
    double par[7];
#pragma unroll
    for (int c = 0; c < 7; ++c) par[c] = s_par[c];
    const float4* src = row_i + at;
    float4* dst = raw + (at - base);
    for (int p0 = 0; p0 < cnt; p0 += kLinkUnroll * 256) {
      float4 pt[kLinkUnroll];
#pragma unroll
      for (int u = 0; u < kLinkUnroll; ++u) { const int p = p0 + u * 256 + tid; pt[u] = src[p < cnt ? p : cnt - 1]; }
#pragma unroll
      for (int u = 0; u < kLinkUnroll; ++u) { const int p = p0 + u * 256 + tid; if (p < cnt) dst[p] = associate_to_map(pt[u], par); }
    }
  }
  // ---- the source: node j's cloud as stored in seq_j's row, into the slot's stack row (chunks of 2048 points dealt over the workgroups)
  {
    const int n = cls ? pl.src_n[1] : pl.src_n[0];
    const float4* row_j = cls ? a.kf.points[1] + (long long)rq.seq_j * a.kf.cap[1] : a.kf.points[0] + (long long)rq.seq_j * a.kf.cap[0];
    const float4* src = row_j + (cls ? pl.src[1] : pl.src[0]);
    float4* dst = (cls ? a.map.stack[1] : a.map.stack[0]) + (long long)s * link_stack_row(a.map, cls);
    for (int q0 = (int)blockIdx.x * kLinkCopyChunk; q0 < n; q0 += (int)gridDim.x * kLinkCopyChunk) {
      const int end = min(q0 + kLinkCopyChunk, n);                             // (end > q0, so end - 1 is a point of the cloud)
      static_assert(kLinkUnroll == 4, "four named registers (a local array here was promoted to LDS)");
      for (int p0 = q0 + tid; p0 < end + tid; p0 += kLinkUnroll * 256) {
        const int p1 = p0 + 256, p2 = p0 + 512, p3 = p0 + 768, last = end - 1;
        const float4 v0 = src[p0 < end ? p0 : last], v1 = src[p1 < end ? p1 : last], v2 = src[p2 < end ? p2 : last], v3 = src[p3 < end ? p3 : last];
        if (p0 < end) dst[p0] = v0;
        if (p1 < end) dst[p1] = v1;
        if (p2 < end) dst[p2] = v2;
        if (p3 < end) dst[p3] = v3;
      }
    }
  }
}

void launch_link_gather(const LinkGatherArgs& a, const VoxArgs& v, hipStream_t s) {
  if (a.n > 0) hipLaunchKernelGGL(k_link_gather, dim3(kLinkGatherBlocks, a.n, 2), dim3(256), 0, s, a, v);
}

// ---- the proposal ------------------------------------------------------------------------------------------------------------------------
namespace {

constexpr int kLinkNone = 0x7fffffff;        // the index of "no candidate"; its d2 is +infinity
constexpr int kLinkScanUnroll = 4;           // node records in flight per lane before the f64 work

// The order of the selection: lower d2 first, then the lower index.
__device__ __forceinline__ bool link_before(double d2a, int ia, double d2b, int ib) { return d2a < d2b || (d2a == d2b && ia < ib); }

// Every node of seq_i once: visit(i, hit, d2) is called by all lanes of a wave together (lanes past the end with hit = false), so that it
// may ballot.  d2 = (dx dx + dy dy) + dz dz of t_i - t_j', hit = d2 <= radius radius; each operation rounded on its own.
template <typename Visit>
__device__ __forceinline__ void link_scan(const LinkProposeArgs& a, const aloam_graph_node* N, int eligible, const double tj[3], Visit visit) {
  for (int base = 0; base < eligible; base += kLinkScanUnroll * kGraphThreads) {
    double ti[kLinkScanUnroll][3];
#pragma unroll
    for (int u = 0; u < kLinkScanUnroll; ++u) {
      const int i = base + u * kGraphThreads + (int)threadIdx.x;
      const aloam_graph_node& x = N[i < eligible ? i : eligible - 1];
      const double* t = a.pose ? x.t_opt : x.t;
      ti[u][0] = t[0]; ti[u][1] = t[1]; ti[u][2] = t[2];
    }
#pragma unroll
    for (int u = 0; u < kLinkScanUnroll; ++u) {
      const int i = base + u * kGraphThreads + (int)threadIdx.x;
      const double dx = ti[u][0] - tj[0], dy = ti[u][1] - tj[1], dz = ti[u][2] - tj[2];
      const double d2 = (dx * dx + dy * dy) + dz * dz;
      visit(i, i < eligible && d2 <= a.radius2, d2);
    }
  }
}

// The least (d2, i) of the workgroup, in every thread.  s_d2 / s_i: one entry per wave; the caller synchronises before their next use.
__device__ __forceinline__ void link_argmin(double& d2, int& i, double* s_d2, int* s_i) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const double od = __shfl_xor(d2, off);
    const int oi = __shfl_xor(i, off);
    if (link_before(od, oi, d2, i)) { d2 = od; i = oi; }
  }
  if ((threadIdx.x & 63) == 0) { s_d2[threadIdx.x >> 6] = d2; s_i[threadIdx.x >> 6] = i; }
  __syncthreads();
  d2 = s_d2[0]; i = s_i[0];
#pragma unroll
  for (int w = 1; w < kGraphThreads / 64; ++w)
    if (link_before(s_d2[w], s_i[w], d2, i)) { d2 = s_d2[w]; i = s_i[w]; }
}

}  // namespace

__global__ __launch_bounds__(kGraphThreads) void k_link_propose(LinkProposeArgs a) {
  __shared__ double s_hit_d2[kProposeHits];
  __shared__ int s_hit_i[kProposeHits];                                        // -1: dead
  __shared__ double s_red_d2[kGraphThreads / 64], s_win_d2[kProposeMaxK], s_xj[7];     // s_xj: q_j', t_j'
  __shared__ int s_red_i[kGraphThreads / 64], s_win_i[kProposeMaxK];
  __shared__ int s_hits;
  const int w = blockIdx.x, tid = threadIdx.x;
  const LinkProposeQuery qu = a.queries[w];
  const aloam_graph_node* N = a.nodes + (long long)qu.seq_i * a.max_nodes;
  const int eligible = qu.nodes_i;
  if (tid == 0) {
    // X_j' = X_j (its bits), or A o X_j = (quat_mul(q_A, q_j), quat_rotate(q_A, t_j) + t_A)
    const aloam_graph_node& xj = a.nodes[(long long)qu.seq_j * a.max_nodes + qu.j];
    double qj[4], tj[3];
    for (int c = 0; c < 4; ++c) qj[c] = a.pose ? xj.q_opt[c] : xj.q[c];
    for (int c = 0; c < 3; ++c) tj[c] = a.pose ? xj.t_opt[c] : xj.t[c];
    if (qu.has_frame) {
      double qa[4], qo[4], to[3];
      for (int c = 0; c < 4; ++c) qa[c] = qu.frame[c];
      quat_mul(qa, qj, qo);
      quat_rotate(qa, tj[0], tj[1], tj[2], to);
      for (int c = 0; c < 4; ++c) qj[c] = qo[c];
      for (int c = 0; c < 3; ++c) tj[c] = to[c] + qu.frame[4 + c];
    }
    for (int c = 0; c < 4; ++c) s_xj[c] = qj[c];
    for (int c = 0; c < 3; ++c) s_xj[4 + c] = tj[c];
    s_hits = 0;
  }
  __syncthreads();
  const double tj[3] = {s_xj[4], s_xj[5], s_xj[6]};
  // ---- pass 1: the hits into the list
  link_scan(a, N, eligible, tj, [&](int i, bool hit, double d2) {
    const unsigned long long m = __ballot(hit);
    if (!m) return;                                                            // (wave-uniform)
    const int rank = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
    int first = 0;
    if ((tid & 63) == 0) first = atomicAdd(&s_hits, __popcll(m));
    first = __shfl(first, 0);
    if (hit && first + rank < kProposeHits) { s_hit_d2[first + rank] = d2; s_hit_i[first + rank] = i; }
  });
  __syncthreads();
  const int hits = s_hits;
  const bool listed = hits <= kProposeHits;                                    // the list holds every hit (uniform)
  // ---- the rounds
  int taken = 0;
  for (int k = 0; k < a.K; ++k) {
    double bd = __builtin_huge_val();
    int bi = kLinkNone;
    if (listed) {
      for (int h = tid; h < hits; h += kGraphThreads) {
        const int i = s_hit_i[h];
        if (i >= 0 && link_before(s_hit_d2[h], i, bd, bi)) { bd = s_hit_d2[h]; bi = i; }
      }
    } else {
      link_scan(a, N, eligible, tj, [&](int i, bool hit, double d2) {
        for (int e = 0; e < k; ++e) hit = hit && abs(i - s_win_i[e]) > a.separation;
        if (hit && link_before(d2, i, bd, bi)) { bd = d2; bi = i; }
      });
    }
    link_argmin(bd, bi, s_red_d2, s_red_i);
    if (bi == kLinkNone) break;                                                // (uniform) nothing is live
    if (tid == 0) { s_win_d2[k] = bd; s_win_i[k] = bi; }
    taken = k + 1;
    if (listed)
      for (int h = tid; h < hits; h += kGraphThreads) {
        const int i = s_hit_i[h];
        if (i >= 0 && abs(i - bi) <= a.separation) s_hit_i[h] = -1;
      }
    __syncthreads();
  }
  // ---- record k by lane k; rows behind the last one taken are zero
  if (tid < a.K) {
    const bool have = tid < taken;
    int i = 0, first = 0, count = 0;
    double d2 = 0.0, qd[4] = {0.0, 0.0, 0.0, 0.0}, td[3] = {0.0, 0.0, 0.0};
    if (have) {
      i = s_win_i[tid]; d2 = s_win_d2[tid];
      // X_i^-1 o X_j' as the header defines a relative pose: q_d = q_i* q_j', t_d = q_i* (t_j' - t_i)
      const aloam_graph_node& xi = N[i];
      double qi[4], qj[4], ti[3];
      for (int c = 0; c < 4; ++c) { qi[c] = a.pose ? xi.q_opt[c] : xi.q[c]; qj[c] = s_xj[c]; }
      for (int c = 0; c < 3; ++c) ti[c] = a.pose ? xi.t_opt[c] : xi.t[c];
      const double qc[4] = {-qi[0], -qi[1], -qi[2], qi[3]};
      quat_mul(qc, qj, qd);
      quat_rotate(qc, tj[0] - ti[0], tj[1] - ti[1], tj[2] - ti[2], td);
      first = i > a.half_window ? i - a.half_window : 0;
      const int last = a.half_window < eligible - 1 - i ? i + a.half_window : eligible - 1;   // min(i + half_window, nodes - 1), no overflow
      count = last - first + 1;
    }
    const long long at = (long long)w * a.K + tid;
    aloam_graph_link_request& r = a.dst[at];
    r.seq_i = have ? qu.seq_i : 0; r.i = i;
    r.first = first; r.count = count;
    r.seq_j = have ? qu.seq_j : 0; r.j = have ? qu.j : 0;
    r.pose = have ? a.pose : 0; r.pad = 0;
    for (int c = 0; c < 4; ++c) r.q[c] = qd[c];
    for (int c = 0; c < 3; ++c) r.t[c] = td[c];
    r.reserved = 0.0;
    if (a.dist2) a.dist2[at] = d2;
  }
  if (tid == 0) a.counts[w] = taken;
}

void launch_link_propose(const LinkProposeArgs& a, hipStream_t stream) {
  if (a.n > 0) hipLaunchKernelGGL(k_link_propose, dim3(a.n), dim3(kGraphThreads), 0, stream, a);
}

}  // namespace aloam
