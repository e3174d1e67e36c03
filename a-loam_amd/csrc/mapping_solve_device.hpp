// a-loam_amd/csrc/mapping_solve_device.hpp — the evaluation of the scan-to-map factors at one pose (LidarEdgeFactor / LidarPlaneNormFactor over the
// records k_map_fit compacted per tile), shared by k_map_solve (mapping_kernels.hip) and k_pose_information_map (information_kernels.hip).
#pragma once
#include "aloam_device.hpp"
#include "lm_device.hpp"
#include "mapping_kernels.hpp"

namespace aloam {

constexpr int kMapSolveThreads = 256;    // more waves do not pay: the kernel needs 256 VGPRs per lane for the f64 sums
template <bool WITH_JAC>
__device__ void map_evaluate(const MapArgs& a, int b, const int* s_pref, const double q[4], const double t[3], double* acc, int* n_edge, int* n_norm) {
  const int tid = threadIdx.x;
  const MapSeq& ms = a.seq[b];
  const MapEdgeRec* E = a.edges + (long long)b * a.R * kLessSharpPerRing;
  const MapNormRec* P = a.norms + (long long)b * a.cap;
  int ne = 0, np = 0;
  // records are fetched a few at a time ahead of the f64 work (same per-thread order as a plain strided loop)
  auto edge_term = [&](const MapEdgeRec& e) {
    ++ne;
    double rcp[3];
    quat_rotate(q, e.cp[0], e.cp[1], e.cp[2], rcp);
    const double lp[3] = {rcp[0] + t[0], rcp[1] + t[1], rcp[2] + t[2]};
    const double dex = e.a[0] - e.b[0], dey = e.a[1] - e.b[1], dez = e.a[2] - e.b[2];
    const double inv = 1.0 / sqrt(dex * dex + dey * dey + dez * dez);
    const double ux = lp[0] - e.a[0], uy = lp[1] - e.a[1], uz = lp[2] - e.a[2], vx = lp[0] - e.b[0], vy = lp[1] - e.b[1], vz = lp[2] - e.b[2];
    const double r0 = (uy * vz - uz * vy) * inv, r1 = (uz * vx - ux * vz) * inv, r2 = (ux * vy - uy * vx) * inv;
    double rho0, rho1;
    huber(r0 * r0 + r1 * r1 + r2 * r2, &rho0, &rho1);
    acc[27] += 0.5 * rho0;
    if (WITH_JAC) {
      const double wx = -dex * inv, wy = -dey * inv, wz = -dez * inv;
      const double A[3][3] = {{0, -wz, wy}, {wz, 0, -wx}, {-wy, wx, 0}};
      const double Bm[3][3] = {{0, 2 * rcp[2], -2 * rcp[1]}, {-2 * rcp[2], 0, 2 * rcp[0]}, {2 * rcp[1], -2 * rcp[0], 0}};
      const double rr[3] = {r0, r1, r2};
#pragma unroll
      for (int row = 0; row < 3; ++row) {
        double J[6];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          J[c] = A[row][0] * Bm[0][c] + A[row][1] * Bm[1][c] + A[row][2] * Bm[2][c];
          J[3 + c] = A[row][c];
        }
        add_row(acc, J, rr[row], rho1);
      }
    }
  };
  constexpr int U = 4;
  // dense index d over the valid records -> tile by binary search in the tile prefixes (LDS, built once per launch), then the
  // record at tile * 256 + (d - prefix[tile])
  const int nt0 = (ms.n_stack[0] + 255) >> 8, nt1 = (ms.n_stack[1] + 255) >> 8;
  const int* pre0 = s_pref, *pre1 = s_pref + nt0 + 1;
  const int n0 = pre0[nt0], n1 = pre1[nt1];
  auto locate = [](const int* pre, int nt, int d) {
    int lo = 0, hi = nt - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (pre[mid] <= d) lo = mid; else hi = mid - 1; }
    return (lo << 8) + (d - pre[lo]);
  };
  for (int d0 = tid; d0 < n0; d0 += U * kMapSolveThreads) {
    MapEdgeRec e[U];
#pragma unroll
    for (int u = 0; u < U; ++u) { const int d = d0 + u * kMapSolveThreads; e[u] = E[locate(pre0, nt0, d < n0 ? d : d0)]; }
#pragma unroll
    for (int u = 0; u < U; ++u) if (d0 + u * kMapSolveThreads < n0) edge_term(e[u]);
  }
  auto norm_term = [&](const MapNormRec& p) {
    ++np;
    double rcp[3];
    quat_rotate(q, p.cp[0], p.cp[1], p.cp[2], rcp);
    // LidarPlaneNormFactor (reference src/lidarFactor.hpp:116-123): r = n . (q cp + t) + d
    const double r = (p.n[0] * (rcp[0] + t[0]) + p.n[1] * (rcp[1] + t[1]) + p.n[2] * (rcp[2] + t[2])) + p.d;
    double rho0, rho1;
    huber(r * r, &rho0, &rho1);
    acc[27] += 0.5 * rho0;
    if (WITH_JAC) {
      const double J[6] = {2.0 * (p.n[2] * rcp[1] - p.n[1] * rcp[2]), 2.0 * (p.n[0] * rcp[2] - p.n[2] * rcp[0]), 2.0 * (p.n[1] * rcp[0] - p.n[0] * rcp[1]),
                           p.n[0], p.n[1], p.n[2]};
      add_row(acc, J, r, rho1);
    }
  };
  for (int d0 = tid; d0 < n1; d0 += U * kMapSolveThreads) {
    MapNormRec pr[U];
#pragma unroll
    for (int u = 0; u < U; ++u) { const int d = d0 + u * kMapSolveThreads; pr[u] = P[locate(pre1, nt1, d < n1 ? d : d0)]; }
#pragma unroll
    for (int u = 0; u < U; ++u) if (d0 + u * kMapSolveThreads < n1) norm_term(pr[u]);
  }
  *n_edge = ne;
  *n_norm = np;
}

}  // namespace aloam
