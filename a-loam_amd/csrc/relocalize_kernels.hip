// a-loam_amd/csrc/relocalize_kernels.hip — gfx950 kernels that score and apply batches of map-pose hypotheses.
//
// A frozen mapping step (aloam_set_map_frozen) leaves on the device everything its first data association read: the down-sampled stacks
// (laserCloudCornerStack / SurfStack, reference src/laserMapping.cpp:542-550), the odometry pose the frame started from (:290-296) and the
// bucketed submap (k_mapgrid_build, standing in for :558-559).  Only the map <- odometry correction differs between the hypotheses of a
// relocalization search, so K of them are scored against that state without a step each:
//   k_score_corrections   per (sequence, candidate): :142-146 transformAssociateToMap with the candidate, then per stack point
//                         :576-706 of the first association - pointAssociateToMap, the exact 5-NN within 1 m, line fit / plane fit and
//                         their validity tests - and the residual of every valid factor at the start pose (src/lidarFactor.hpp:36-51,
//                         :116-123 under HuberLoss(0.1)).  The five neighbours go from the search to the fit in registers and no factor
//                         record is written: with K in the thousands the knn / record buffers of the step would be K times as large.
//   k_score_finalize      per sequence: the per-workgroup partials, in slot order, into scores[n][K]; the best candidate
//   k_apply_corrections   q_wmap_wodom, t_wmap_wodom := cand[choice[i]], read on the device in stream order
// The search, the fits and every decision (d < 1.0f, vals[2] > 3 * vals[1], > 0.2) are the device functions of the mapping step
// (map_search_device.hpp), called in the same order on the same values: the counts are those of the step, as integers.
// Integer / f32 / f64 scalar work like the mapping kernels: latency- and issue-bound, no MFMA.
#include "relocalize_kernels.hpp"

#include "map_score_device.hpp"

namespace aloam {

namespace {

template <int CLS>
__device__ __forceinline__ void score_class(const ScoreArgs& a, int b, int part, const MapSeq& ms, const double par[7], ScoreAcc& acc) {
  const int n = ms.n_stack[CLS], H = a.grid_H;
  const float4* __restrict__ stack = a.stack[CLS] + (long long)b * (CLS == 0 ? a.R * kLessSharpPerRing : a.cap);
  const int* __restrict__ start = a.grid_start[CLS] + (long long)b * (H + 1);
  const float4* __restrict__ sorted = a.grid_sorted[CLS] + (long long)b * a.pool_cap;
  for (int i = part * kScoreThreads + (int)threadIdx.x; i < n; i += kScoreParts * kScoreThreads) score_point<CLS>(stack[i], par, start, sorted, H, acc);
}

}  // namespace

// One workgroup per (sequence, candidate, part).  XCD-aware decoding of the 1-D grid as in k_map_search: workgroups are dealt round-robin
// over the 8 XCDs by linear id and every XCD has its own L2, so all workgroups of a listed sequence - every candidate reads the same
// bucketed submap - sit on one XCD.  With fewer than 8 listed sequences that would leave XCDs idle (n = 1, K = 2000: seven of eight), so
// the candidates of a sequence are cut into `splits` = 8 / n ranges that go to XCDs of their own: the submap is then fetched by several
// L2s, which is cheap next to K searches of it.
__global__ __launch_bounds__(kScoreThreads) void k_score_corrections(ScoreArgs a) {
  const int L = blockIdx.x, xcd = L & 7, slot = L >> 3;
  const int per = a.kper * kScoreParts;
  const int v = (slot / per) * 8 + xcd, w = slot % per;
  if (v >= a.n * a.splits) return;
  const int i = v / a.splits, c = (v % a.splits) * a.kper + w / kScoreParts, part = w % kScoreParts;
  if (c >= a.K) return;
  const int b = a.seqs[i];
  const MapSeq& ms = a.seq[b];
  ScoreAcc acc = {{0, 0}, {0, 0}, 0.0};
  if (ms.gate) {                                                              // :554
    const aloam_map_correction& cd = a.cand[c];
    double qo[4], to[3], qm[4], q[4], rt[3], par[7];
    for (int k = 0; k < 4; ++k) { qo[k] = ms.q_wodom[k]; qm[k] = cd.q_wmap_wodom[k]; }
    for (int k = 0; k < 3; ++k) to[k] = ms.t_wodom[k];
    quat_mul(qm, qo, q);                                                      // transformAssociateToMap (:142-146), as k_map_begin
    quat_rotate(qm, to[0], to[1], to[2], rt);
    for (int k = 0; k < 4; ++k) par[k] = q[k];
    for (int k = 0; k < 3; ++k) par[4 + k] = rt[k] + cd.t_wmap_wodom[k];
    score_class<0>(a, b, part, ms, par, acc);
    score_class<1>(a, b, part, ms, par, acc);
  }
  __shared__ int s_cnt[kScoreThreads / 64][4];
  __shared__ double s_cost[kScoreThreads / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int f0 = wave_sum(acc.factors[0]), f1 = wave_sum(acc.factors[1]), n0 = wave_sum(acc.found[0]), n1 = wave_sum(acc.found[1]);
  const double cost = wave_sum(acc.cost);
  if (lane == 0) { s_cnt[wave][0] = f0; s_cnt[wave][1] = f1; s_cnt[wave][2] = n0; s_cnt[wave][3] = n1; s_cost[wave] = cost; }
  __syncthreads();
  if (threadIdx.x == 0) {
    ScorePartial p = {0, 0, 0, 0, 0.0, {0, 0}};
    for (int k = 0; k < kScoreThreads / 64; ++k) {                            // waves in order
      p.corner_factors += s_cnt[k][0]; p.surf_factors += s_cnt[k][1]; p.corner_found += s_cnt[k][2]; p.surf_found += s_cnt[k][3];
      p.cost = p.cost + s_cost[k];
    }
    a.part[((long long)i * a.K + c) * kScoreParts + part] = p;
  }
}

// One workgroup per listed sequence: the partials of every candidate summed in slot order, the score written, the best candidate kept.
__global__ __launch_bounds__(256) void k_score_finalize(ScoreArgs a) {
  const int i = blockIdx.x, tid = threadIdx.x;
  BestKey mine = {-1, 0.0, 0x7fffffff};
  for (int c = tid; c < a.K; c += 256) {
    const ScorePartial* p = a.part + ((long long)i * a.K + c) * kScoreParts;
    aloam_map_score s = {0, 0, 0, 0, 0.0, {0, 0}};
    for (int k = 0; k < kScoreParts; ++k) {
      const ScorePartial v = p[k];
      s.corner_factors += v.corner_factors; s.surf_factors += v.surf_factors; s.corner_found += v.corner_found; s.surf_found += v.surf_found;
      s.cost = s.cost + v.cost;
    }
    a.scores[(long long)i * a.K + c] = s;
    const BestKey key = {s.corner_factors + s.surf_factors, s.cost, c};
    if (better(key, mine)) mine = key;
  }
  if (!a.best) return;
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
  if (tid == 0) a.best[i] = s_i[0];
}

// A choice outside 0 .. K-1 leaves its sequence untouched and is counted (aloam_synchronize reports the count once, as ALOAM_E_ARG).
__global__ __launch_bounds__(256) void k_apply_corrections(ApplyArgs a) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n) return;
  const int ch = a.choice[i];
  if (ch < 0 || ch >= a.K) { atomicAdd(a.bad_choice, 1); return; }
  MapSeq& ms = a.seq[a.seqs[i]];
  const aloam_map_correction& cd = a.cand[ch];
  for (int k = 0; k < 4; ++k) ms.q_wmap_wodom[k] = cd.q_wmap_wodom[k];
  for (int k = 0; k < 3; ++k) ms.t_wmap_wodom[k] = cd.t_wmap_wodom[k];
}

void launch_score_corrections(const ScoreArgs& a, hipStream_t s) {
  if (a.n <= 0) return;
  const int groups = (a.n * a.splits + 7) / 8;
  hipLaunchKernelGGL(k_score_corrections, dim3((unsigned)groups * 8u * (unsigned)a.kper * kScoreParts), dim3(kScoreThreads), 0, s, a);
  hipLaunchKernelGGL(k_score_finalize, dim3(a.n), dim3(256), 0, s, a);
}

void launch_apply_corrections(const ApplyArgs& a, hipStream_t s) {
  if (a.n > 0) hipLaunchKernelGGL(k_apply_corrections, dim3((a.n + 255) / 256), dim3(256), 0, s, a);
}

}  // namespace aloam
