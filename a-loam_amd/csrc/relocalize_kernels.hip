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

#include "lm_device.hpp"
#include "map_search_device.hpp"

namespace aloam {

namespace {

constexpr int kScoreU = 4;           // bucket loads in flight per lane, as k_map_search (kMapSearchU)

struct ScoreAcc { int factors[2], found[2]; double cost; };

// One stack point of class CLS under the pose par: search, fit, residual.  Only the leaf functions are shared with the mapping step
// (map_search_device.hpp); this body MIRRORS, statement for statement, three bodies of mapping_kernels.hip that write their results to
// global memory and therefore cannot be called from here: the query loop of k_map_search (cell and neighbour-cell choice, the eight bucket
// heads, `visit`, the kScoreU-wide bucket walk, the `top.k[4] >> 32 < 0x3f800000` found test), both branches of k_map_fit (centroid and
// covariance sums, `vals[2] > 3 * vals[1]`; the 5 x 3 system, `> 0.2`), and edge_term / norm_term of map_evaluate<false>.  The start
// pose in k_score_corrections mirrors k_map_begin's transformAssociateToMap.  A change to any of those must be made here too;
// test_factor_counts_equal_a_frozen_step_from_the_candidate (GPU) is what notices a divergence.
template <int CLS>
__device__ __forceinline__ void score_point(const float4& ori, const double par[7], const int* __restrict__ start, const float4* __restrict__ sorted, int H,
                                            ScoreAcc& acc) {
  const float4 sel = associate_to_map(ori, par);                            // pointSel (:580, :646)
  const float gx = sel.x * kMapCellInv, gy = sel.y * kMapCellInv, gz = sel.z * kMapCellInv;
  const int cx = (int)floorf(gx), cy = (int)floorf(gy), cz = (int)floorf(gz);
  const int nx = gx - (float)cx >= 0.5f ? cx + 1 : cx - 1, ny = gy - (float)cy >= 0.5f ? cy + 1 : cy - 1, nz = gz - (float)cz >= 0.5f ? cz + 1 : cz - 1;
  Top5P top;
  top.init();
  int s0[8], s1[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) {                                              // the 8 bucket heads first: independent 8-byte loads
    const unsigned h = map_bucket((c & 1) ? nx : cx, (c & 2) ? ny : cy, (c & 4) ? nz : cz, H);
    const MapIntPair v = *reinterpret_cast<const MapIntPair*>(reinterpret_cast<const char*>(start) + (h << 2));
    s0[c] = v.a; s1[c] = v.b;
  }
  auto visit = [&](const float4& p, int at) {
    const float ddx = p.x - sel.x, ddy = p.y - sel.y, ddz = p.z - sel.z;
    const float d = (ddx * ddx + ddy * ddy) + ddz * ddz;                     // FLANN L2_Simple, f32
    if (d < 1.0f) top.insert(d, __float_as_int(p.w), at);
  };
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    for (int k = s0[c]; k < s1[c]; k += kScoreU) {
      const int m = s1[c] - k;
      float4 p[kScoreU];
#pragma unroll
      for (int u = 0; u < kScoreU; ++u) p[u] = sorted[u < m ? k + u : k];    // a lane past the end of its bucket re-reads its own entry k
#pragma unroll
      for (int u = 0; u < kScoreU; ++u) if (u < m) visit(p[u], k + u);
    }
  }
  if (!((unsigned)(top.k[4] >> 32) < 0x3f800000u)) return;                   // pointSearchSqDis[4] < 1.0 (:582, :650)
  acc.found[CLS] += 1;
  float nxs[5], nys[5], nzs[5];
#pragma unroll
  for (int s = 0; s < 5; ++s) { const float4 q = sorted[top.pos[s]]; nxs[s] = q.x; nys[s] = q.y; nzs[s] = q.z; }
  const double* q = par;
  const double* t = par + 4;
  if (CLS == 0) {
    double cxs = 0.0, cys = 0.0, czs = 0.0;
#pragma unroll
    for (int j = 0; j < 5; ++j) { cxs = cxs + (double)nxs[j]; cys = cys + (double)nys[j]; czs = czs + (double)nzs[j]; }
    const double ctr[3] = {cxs / 5.0, cys / 5.0, czs / 5.0};
    double cov[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
#pragma unroll
    for (int j = 0; j < 5; ++j) {
      const double zm[3] = {(double)nxs[j] - ctr[0], (double)nys[j] - ctr[1], (double)nzs[j] - ctr[2]};
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) cov[r][c] = cov[r][c] + zm[r] * zm[c];
    }
    double vals[3], dir[3];
    sym_eigen3(cov, vals, dir);
    if (!(vals[2] > 3 * vals[1])) return;                                    // :611
    acc.factors[0] += 1;
    double ea[3], eb[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { ea[k] = 0.1 * dir[k] + ctr[k]; eb[k] = -0.1 * dir[k] + ctr[k]; }
    // LidarEdgeFactor(curr_point, point_a, point_b, 1.0) at the start pose, as map_evaluate's edge_term
    double rcp[3];
    quat_rotate(q, ori.x, ori.y, ori.z, rcp);
    const double lp[3] = {rcp[0] + t[0], rcp[1] + t[1], rcp[2] + t[2]};
    const double dex = ea[0] - eb[0], dey = ea[1] - eb[1], dez = ea[2] - eb[2];
    const double inv = 1.0 / sqrt(dex * dex + dey * dey + dez * dez);
    const double ux = lp[0] - ea[0], uy = lp[1] - ea[1], uz = lp[2] - ea[2], vx = lp[0] - eb[0], vy = lp[1] - eb[1], vz = lp[2] - eb[2];
    const double r0 = (uy * vz - uz * vy) * inv, r1 = (uz * vx - ux * vz) * inv, r2 = (ux * vy - uy * vx) * inv;
    double rho0, rho1;
    huber(r0 * r0 + r1 * r1 + r2 * r2, &rho0, &rho1);
    acc.cost += 0.5 * rho0;
  } else {
    double A[5][3], B[5] = {-1, -1, -1, -1, -1}, x[3];
#pragma unroll
    for (int j = 0; j < 5; ++j) { A[j][0] = nxs[j]; A[j][1] = nys[j]; A[j][2] = nzs[j]; }
    lstsq_5x3(A, B, x);
    const double len = sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]);
    const double d = 1 / len;                                                // negative_OA_dot_norm (:664)
    const double pnx = x[0] / len, pny = x[1] / len, pnz = x[2] / len;
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 5; ++j)
      if (fabs(pnx * (double)nxs[j] + pny * (double)nys[j] + pnz * (double)nzs[j] + d) > 0.2) ok = false;   // :672-678
    if (!ok) return;
    acc.factors[1] += 1;
    // LidarPlaneNormFactor (reference src/lidarFactor.hpp:116-123) at the start pose, as map_evaluate's norm_term
    double rcp[3];
    quat_rotate(q, ori.x, ori.y, ori.z, rcp);
    const double r = (pnx * (rcp[0] + t[0]) + pny * (rcp[1] + t[1]) + pnz * (rcp[2] + t[2])) + d;
    double rho0, rho1;
    huber(r * r, &rho0, &rho1);
    acc.cost += 0.5 * rho0;
  }
}

template <int CLS>
__device__ __forceinline__ void score_class(const ScoreArgs& a, int b, int part, const MapSeq& ms, const double par[7], ScoreAcc& acc) {
  const int n = ms.n_stack[CLS], H = a.grid_H;
  const float4* __restrict__ stack = a.stack[CLS] + (long long)b * (CLS == 0 ? a.R * kLessSharpPerRing : a.cap);
  const int* __restrict__ start = a.grid_start[CLS] + (long long)b * (H + 1);
  const float4* __restrict__ sorted = a.grid_sorted[CLS] + (long long)b * a.pool_cap;
  for (int i = part * kScoreThreads + (int)threadIdx.x; i < n; i += kScoreParts * kScoreThreads) score_point<CLS>(stack[i], par, start, sorted, H, acc);
}

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
  return v;
}
__device__ __forceinline__ double wave_sum(double v) {                       // a fixed butterfly: every lane ends with the same bits
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v = v + __shfl_xor(v, d);
  return v;
}

// (factors, cost, index) of a candidate: more factors first, then the lower cost, then the lower index.  A NaN cost (a non-finite
// candidate: quaternions are used as given) ranks as +infinity, so this is a total order and the reduction below gives the same winner in
// whatever order it combines.
struct BestKey { int factors; double cost; int idx; };
__device__ __forceinline__ bool better(const BestKey& x, const BestKey& y) {
  if (x.factors != y.factors) return x.factors > y.factors;
  const double inf = __longlong_as_double(0x7ff0000000000000ll);
  const double cx = x.cost == x.cost ? x.cost : inf, cy = y.cost == y.cost ? y.cost : inf;
  if (cx != cy) return cx < cy;
  return x.idx < y.idx;
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
