// a-loam_amd/csrc/map_score_device.hpp — what one pose scores against a bucketed target: the per-point body of the hypothesis scoring
// (search, fit, residual), the wave sums and the ranking.  Shared by relocalize_kernels.hip (aloam_score_map_corrections) and
// loopsearch_kernels.hip (aloam_graph_search_loops); every function is internal to the unit that includes it.
#pragma once
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

}  // namespace aloam
