// a-loam_amd/csrc/loopsearch_kernels.hip — gfx950 kernels of the pose grid searched around a loop guess (aloam_graph_search_loops,
// DESIGN.md §7q).  They run between the grid build and the first association of the batched keyframe registration, over its scratch slots:
//   k_loop_search        one workgroup per (slot, node, part): the node's pose from its index (one lane, f64, separately rounded, through
//                        LDS), then score_point<0> over its part of the slot's corner row and score_point<1> over its part of the surf row
//                        - what round 0 of a registration started from that node would count - the wave butterfly, the waves in order, one
//                        partial into a fixed slot
//   k_loop_search_pick   one workgroup per slot: a node's partials summed in slot order, the score table when asked for, the winner by
//                        `better` (most factors, lower cost, lower index; no factor at all: the centre node), the slot's `parameters` :=
//                        the winner's pose, the search record written field by field from one lane
// A slot whose target failed the gate is not searched.  No floating-point atomics, no integer ones either; every store to global memory is a
// vector store.  The per-point body, the sums and the ranking are those of the map-pose hypothesis scoring (map_score_device.hpp).
#include "loopsearch_kernels.hpp"

#include "map_score_device.hpp"

namespace aloam {

namespace {

// Node c of the grid around the request's guess: q_c = dq q_g with dq = (0, 0, sin h, cos h) from the host's table, t_c = t_g + (dx, dy, 0).
// iyaw == 0 keeps q_g itself and a zero index keeps its coordinate, so the centre node is the guess bit for bit.
__device__ __forceinline__ void node_pose(const LoopSearchGrid& g, const aloam_graph_loop_request& rq, int c, int idx[3], double par[7]) {
  const int S = 2 * g.m + 1;
  const int ix = c % S - g.m, iy = (c / S) % S - g.m, iyaw = c / (S * S) - g.a;
  idx[0] = ix; idx[1] = iy; idx[2] = iyaw;
  double qg[4];
  for (int k = 0; k < 4; ++k) qg[k] = rq.q[k];
  if (iyaw != 0) {
    const double dq[4] = {0.0, 0.0, g.half[iyaw + g.a][0], g.half[iyaw + g.a][1]};
    quat_mul(dq, qg, par);
  } else {
    for (int k = 0; k < 4; ++k) par[k] = qg[k];
  }
  par[4] = ix != 0 ? rq.t[0] + (double)ix * g.step_m : rq.t[0];
  par[5] = iy != 0 ? rq.t[1] + (double)iy * g.step_m : rq.t[1];
  par[6] = rq.t[2];
}

template <int CLS>
__device__ __forceinline__ void search_class(const MapArgs& m, int s, int part, const MapSeq& ms, const double par[7], ScoreAcc& acc) {
  const int n = ms.n_stack[CLS], H = m.grid_H;
  const float4* __restrict__ stack = m.stack[CLS] + (long long)s * (CLS == 0 ? m.R * kLessSharpPerRing : m.cap);
  const int* __restrict__ start = m.grid_start[CLS] + (long long)s * (H + 1);
  const float4* __restrict__ sorted = m.grid_sorted[CLS] + (long long)s * m.pool_cap;
  for (int i = part * kLoopSearchThreads + (int)threadIdx.x; i < n; i += kLoopSearchParts * kLoopSearchThreads) score_point<CLS>(stack[i], par, start, sorted, H, acc);
}

// The partials of node c of slot i, in slot order.
__device__ __forceinline__ aloam_map_score node_score(const LoopSearchArgs& a, int i, int c) {
  const LoopSearchPartial* p = a.part + ((long long)i * a.grid.K + c) * kLoopSearchParts;
  aloam_map_score s = {0, 0, 0, 0, 0.0, {0, 0}};
  for (int k = 0; k < kLoopSearchParts; ++k) {
    const LoopSearchPartial v = p[k];
    s.corner_factors += v.corner_factors; s.surf_factors += v.surf_factors; s.corner_found += v.corner_found; s.surf_found += v.surf_found;
    s.cost = s.cost + v.cost;
  }
  return s;
}

__device__ __forceinline__ void store_score(aloam_map_score* o, const aloam_map_score& s) {
  o->corner_factors = s.corner_factors; o->surf_factors = s.surf_factors; o->corner_found = s.corner_found; o->surf_found = s.surf_found;
  o->cost = s.cost; o->pad[0] = 0; o->pad[1] = 0;
}

}  // namespace

// XCD-aware decoding of the 1-D grid, as the map-pose hypothesis scoring does it: workgroups are dealt round-robin over the 8 XCDs by linear
// id and every XCD has an L2 of its own, so all workgroups of a slot - every node reads the same bucketed target and the same source rows -
// sit on one XCD; with fewer than 8 slots the nodes of a slot are cut into `splits` = 8 / n ranges on XCDs of their own.  Placement decides
// the speed only: every (slot, node, part) is visited exactly once whatever the hardware does with the ids.
__global__ __launch_bounds__(kLoopSearchThreads) void k_loop_search(LoopSearchArgs a) {
  const int L = blockIdx.x, xcd = L & 7, slot = L >> 3;
  const int per = a.kper * kLoopSearchParts;
  const int v = (slot / per) * 8 + xcd, w = slot % per;
  if (v >= a.n * a.splits) return;
  const int i = v / a.splits, c = (v % a.splits) * a.kper + w / kLoopSearchParts, part = w % kLoopSearchParts;
  if (c >= a.grid.K) return;
  const MapSeq& ms = a.map.seq[i];
  if (!ms.gate) return;                                                       // not searched: k_loop_search_pick reads no partial of it
  __shared__ double s_par[7];
  if (threadIdx.x == 0) {
    int idx[3];
    double p[7];
    node_pose(a.grid, a.req[i], c, idx, p);
    for (int k = 0; k < 7; ++k) s_par[k] = p[k];
  }
  __syncthreads();
  double par[7];
#pragma unroll
  for (int k = 0; k < 7; ++k) par[k] = s_par[k];
  ScoreAcc acc = {{0, 0}, {0, 0}, 0.0};
  search_class<0>(a.map, i, part, ms, par, acc);
  search_class<1>(a.map, i, part, ms, par, acc);
  __shared__ int s_cnt[kLoopSearchThreads / 64][4];
  __shared__ double s_cost[kLoopSearchThreads / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int f0 = wave_sum(acc.factors[0]), f1 = wave_sum(acc.factors[1]), n0 = wave_sum(acc.found[0]), n1 = wave_sum(acc.found[1]);
  const double cost = wave_sum(acc.cost);
  if (lane == 0) { s_cnt[wave][0] = f0; s_cnt[wave][1] = f1; s_cnt[wave][2] = n0; s_cnt[wave][3] = n1; s_cost[wave] = cost; }
  __syncthreads();
  if (threadIdx.x == 0) {
    LoopSearchPartial p = {0, 0, 0, 0, 0.0, {0, 0}};
    for (int k = 0; k < kLoopSearchThreads / 64; ++k) {                       // waves in order
      p.corner_factors += s_cnt[k][0]; p.surf_factors += s_cnt[k][1]; p.corner_found += s_cnt[k][2]; p.surf_found += s_cnt[k][3];
      p.cost = p.cost + s_cost[k];
    }
    a.part[((long long)i * a.grid.K + c) * kLoopSearchParts + part] = p;
  }
}

__global__ __launch_bounds__(256) void k_loop_search_pick(LoopSearchArgs a) {
  const int i = blockIdx.x, tid = threadIdx.x, K = a.grid.K;
  MapSeq& ms = a.map.seq[i];
  int status = a.plan[(long long)i * a.plan_ints];
  if (status == ALOAM_LOOP_OK && !ms.gate) status = ALOAM_LOOP_TARGET_TOO_SMALL;
  const bool searched = status == ALOAM_LOOP_OK;                              // (uniform)
  BestKey mine = {-1, 0.0, 0x7fffffff};
  for (int c = tid; c < K; c += 256) {
    aloam_map_score s = {0, 0, 0, 0, 0.0, {0, 0}};
    if (searched) s = node_score(a, i, c);
    if (a.scores) store_score(a.scores + ((long long)i * K + c), s);
    const BestKey key = {s.corner_factors + s.surf_factors, s.cost, c};
    if (searched && better(key, mine)) mine = key;
  }
  __shared__ int s_f[256], s_i[256];
  __shared__ double s_c[256];
  s_f[tid] = mine.factors; s_c[tid] = mine.cost; s_i[tid] = mine.idx;
  __syncthreads();
  for (int d = 128; d >= 1; d >>= 1) {
    if (tid < d) {
      const BestKey x = {s_f[tid], s_c[tid], s_i[tid]}, y = {s_f[tid + d], s_c[tid + d], s_i[tid + d]};
      if (better(y, x)) { s_f[tid] = y.factors; s_c[tid] = y.cost; s_i[tid] = y.idx; }
    }
    __syncthreads();
  }
  if (tid != 0) return;
  const aloam_graph_loop_request& rq = a.req[i];
  aloam_graph_loop_search_result* out = a.dst + i;
  const int centre = (K - 1) / 2;
  const aloam_map_score zero = {0, 0, 0, 0, 0.0, {0, 0}};
  int best = -1, idx[3] = {0, 0, 0};
  double par[7];
  for (int k = 0; k < 4; ++k) par[k] = rq.q[k];
  for (int k = 0; k < 3; ++k) par[4 + k] = rq.t[k];
  aloam_map_score sb = zero, sg = zero;
  if (searched) {
    best = s_f[0] > 0 ? s_i[0] : centre;                                     // no factor anywhere: the guess, not a corner of the grid
    node_pose(a.grid, rq, best, idx, par);
    sb = node_score(a, i, best); sg = node_score(a, i, centre);
    for (int k = 0; k < 7; ++k) ms.par[k] = par[k];                           // `parameters` := the best node's pose
  }
  out->status = status; out->nodes = K; out->best = best;
  out->ix = idx[0]; out->iy = idx[1]; out->iyaw = idx[2];
  out->pad[0] = 0; out->pad[1] = 0;
  for (int k = 0; k < 4; ++k) out->q[k] = par[k];
  for (int k = 0; k < 3; ++k) out->t[k] = par[4 + k];
  out->reserved = 0.0;
  store_score(&out->best_score, sb);
  store_score(&out->guess_score, sg);
}

void launch_loop_search(const LoopSearchArgs& a, hipStream_t s) {
  if (a.n <= 0) return;
  const int groups = (a.n * a.splits + 7) / 8;
  hipLaunchKernelGGL(k_loop_search, dim3((unsigned)groups * 8u * (unsigned)a.kper * kLoopSearchParts), dim3(kLoopSearchThreads), 0, s, a);
  hipLaunchKernelGGL(k_loop_search_pick, dim3(a.n), dim3(256), 0, s, a);
}

}  // namespace aloam
