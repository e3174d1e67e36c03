// a-loam_amd/csrc/graphpropose_kernels.hip — gfx950 kernel of the loop proposal by pose proximity (aloam_graph_propose_loops).
// A translation unit of its own, so that every other kernel is compiled exactly as before; the relative pose of a proposal is formed with
// the device functions k_loop_gather forms T_k with (quat_mul, quat_rotate, through map_search_device.hpp).
//   k_graph_propose   one workgroup of kGraphThreads per query (seq, j).  Pass 1: the threads stride over the eligible nodes 0 .. j - min_gap,
//                     each reads the 24 bytes of t (or t_opt) of a node record, forms d2 and the radius test in separately rounded f64, and
//                     the hits are compacted as (d2, i) into an LDS list of kProposeHits entries (wave64 ballot + mbcnt ranks; the waves take
//                     their ranges of the list with one integer LDS add each).  A hit that does not fit is dropped, the count carries on.
//                     Then up to K rounds: a block arg-min over (d2, i) - wave shuffles, one LDS stage across the four waves - and every
//                     hit within `separation` of the winner dies.  The rounds run over the list when it holds every hit; when it
//                     overflowed, every round scans the nodes again (propose_scan, the same operations, so the same bits) and a hit is live
//                     when no earlier winner lies within `separation`.  Both give the same output.  Lane k then writes record k.
// No floating-point atomics.  The order of the list's entries depends on which wave adds first; nothing read from the list does, since the
// least (d2, i) of a set does not depend on the set's order.  Every store to global memory is a vector store, field by field from one lane.
#include "graphpropose_kernels.hpp"

#include "map_search_device.hpp"             // quat_mul, quat_rotate only

namespace aloam {

namespace {

constexpr int kProposeNone = 0x7fffffff;     // the index of "no candidate"; its d2 is +infinity
constexpr int kProposeUnroll = 4;            // node records in flight per lane before the f64 work

// The order of the selection: lower d2 first, then the lower index.
__device__ __forceinline__ bool propose_before(double d2a, int ia, double d2b, int ib) { return d2a < d2b || (d2a == d2b && ia < ib); }

// Every eligible node once: visit(i, hit, d2) is called by all lanes of a wave together (lanes past the end with hit = false), so that it
// may ballot.  d2 = (dx dx + dy dy) + dz dz of t_i - t_j, r = (j - i) growth + radius, hit = d2 <= r r; each operation rounded on its own.
template <typename Visit>
__device__ __forceinline__ void propose_scan(const GraphProposeArgs& a, const aloam_graph_node* N, int eligible, int j, const double tj[3], Visit visit) {
  for (int base = 0; base < eligible; base += kProposeUnroll * kGraphThreads) {
    double ti[kProposeUnroll][3];
#pragma unroll
    for (int u = 0; u < kProposeUnroll; ++u) {
      const int i = base + u * kGraphThreads + (int)threadIdx.x;
      const aloam_graph_node& x = N[i < eligible ? i : eligible - 1];
      const double* t = a.pose ? x.t_opt : x.t;
      ti[u][0] = t[0]; ti[u][1] = t[1]; ti[u][2] = t[2];
    }
#pragma unroll
    for (int u = 0; u < kProposeUnroll; ++u) {
      const int i = base + u * kGraphThreads + (int)threadIdx.x;
      const double dx = ti[u][0] - tj[0], dy = ti[u][1] - tj[1], dz = ti[u][2] - tj[2];
      const double d2 = (dx * dx + dy * dy) + dz * dz;
      const double r = (double)(j - i) * a.growth_m_per_node + a.radius_m;
      visit(i, i < eligible && d2 <= r * r, d2);
    }
  }
}

// The least (d2, i) of the workgroup, in every thread.  s_d2 / s_i: one entry per wave; the caller synchronises before their next use.
__device__ __forceinline__ void propose_argmin(double& d2, int& i, double* s_d2, int* s_i) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const double od = __shfl_xor(d2, off);
    const int oi = __shfl_xor(i, off);
    if (propose_before(od, oi, d2, i)) { d2 = od; i = oi; }
  }
  if ((threadIdx.x & 63) == 0) { s_d2[threadIdx.x >> 6] = d2; s_i[threadIdx.x >> 6] = i; }
  __syncthreads();
  d2 = s_d2[0]; i = s_i[0];
#pragma unroll
  for (int w = 1; w < kGraphThreads / 64; ++w)
    if (propose_before(s_d2[w], s_i[w], d2, i)) { d2 = s_d2[w]; i = s_i[w]; }
}

}  // namespace

__global__ __launch_bounds__(kGraphThreads) void k_graph_propose(GraphProposeArgs a) {
  __shared__ double s_hit_d2[kProposeHits];
  __shared__ int s_hit_i[kProposeHits];                                        // -1: dead
  __shared__ double s_red_d2[kGraphThreads / 64], s_win_d2[kProposeMaxK];
  __shared__ int s_red_i[kGraphThreads / 64], s_win_i[kProposeMaxK];
  __shared__ int s_hits;
  const int w = blockIdx.x, tid = threadIdx.x;
  const GraphProposeQuery qu = a.queries[w];
  const aloam_graph_node* N = a.nodes + (long long)qu.seq * a.max_nodes;
  const int eligible = qu.j >= a.min_gap ? qu.j - a.min_gap + 1 : 0;
  double tj[3];
  {
    const double* t = a.pose ? N[qu.j].t_opt : N[qu.j].t;
    tj[0] = t[0]; tj[1] = t[1]; tj[2] = t[2];
  }
  if (tid == 0) s_hits = 0;
  __syncthreads();
  // ---- pass 1: the hits into the list
  propose_scan(a, N, eligible, qu.j, tj, [&](int i, bool hit, double d2) {
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
    int bi = kProposeNone;
    if (listed) {
      for (int h = tid; h < hits; h += kGraphThreads) {
        const int i = s_hit_i[h];
        if (i >= 0 && propose_before(s_hit_d2[h], i, bd, bi)) { bd = s_hit_d2[h]; bi = i; }
      }
    } else {
      propose_scan(a, N, eligible, qu.j, tj, [&](int i, bool hit, double d2) {
        for (int e = 0; e < k; ++e) hit = hit && abs(i - s_win_i[e]) > a.separation;
        if (hit && propose_before(d2, i, bd, bi)) { bd = d2; bi = i; }
      });
    }
    propose_argmin(bd, bi, s_red_d2, s_red_i);
    if (bi == kProposeNone) break;                                             // (uniform) nothing is live
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
      // X_i^-1 o X_j as the header defines a relative pose: q_d = q_i* q_j, t_d = q_i* (t_j - t_i)
      const aloam_graph_node& xi = N[i];
      const aloam_graph_node& xj = N[qu.j];
      double qi[4], qj[4], ti[3];
      for (int c = 0; c < 4; ++c) { qi[c] = a.pose ? xi.q_opt[c] : xi.q[c]; qj[c] = a.pose ? xj.q_opt[c] : xj.q[c]; }
      for (int c = 0; c < 3; ++c) ti[c] = a.pose ? xi.t_opt[c] : xi.t[c];
      const double qc[4] = {-qi[0], -qi[1], -qi[2], qi[3]};
      quat_mul(qc, qj, qd);
      quat_rotate(qc, tj[0] - ti[0], tj[1] - ti[1], tj[2] - ti[2], td);
      first = i > a.half_window ? i - a.half_window : 0;
      count = i + a.half_window - first + 1;
    }
    const long long at = (long long)w * a.K + tid;
    aloam_graph_loop_request& r = a.dst[at];
    r.seq = have ? qu.seq : 0; r.i = i; r.j = have ? qu.j : 0;
    r.first = first; r.count = count; r.pose = have ? a.pose : 0;
    r.pad[0] = 0; r.pad[1] = 0;
    for (int c = 0; c < 4; ++c) r.q[c] = qd[c];
    for (int c = 0; c < 3; ++c) r.t[c] = td[c];
    r.reserved = 0.0;
    if (a.dist2) a.dist2[at] = d2;
  }
  if (tid == 0) a.counts[w] = taken;
}

void launch_graph_propose(const GraphProposeArgs& a, hipStream_t stream) {
  if (a.n > 0) hipLaunchKernelGGL(k_graph_propose, dim3(a.n), dim3(kGraphThreads), 0, stream, a);
}

}  // namespace aloam
