// a-loam_amd/csrc/odometry_solve_device.hpp — the evaluation of the odometry factors at one pose (LidarEdgeFactor / LidarPlaneFactor residuals,
// closed-form Jacobians, Huber re-weighting, the thread's share of J^T J / J^T r / cost), shared by k_solve (odometry_kernels.hip), which calls it
// at every point of its Levenberg-Marquardt loop, and k_pose_information_odom (information_kernels.hip), which calls it once at the pose the solve left.
#pragma once
#include "aloam_device.hpp"
#include "aloam_trig.hpp"
#include "lm_device.hpp"

namespace aloam {

// ---- DISTORTION 1 (reference src/laserOdometry.cpp:59 ships 0) ---------------------------------------------------------
// Interpolation ratio of a point: (intensity - int(intensity)) / SCAN_PERIOD, an f32 difference divided by the double 0.1
// (:115-116, :376-377, :474-475).
__device__ __forceinline__ double interpolation_ratio(float frac) { return (double)frac / 0.1; }

// Identity.slerp(s, q) as Eigen's QuaternionBase::slerp evaluates it: the result is scale0 * Identity + scale1 * q (a
// coefficient blend, not re-normalised); both scales depend on q only through d = q.w, so their derivatives do too.
__device__ __forceinline__ void slerp_scales(double w, double s, double* c0, double* c1, double* dc0, double* dc1) {
  const double one = 1.0 - 2.220446049250313e-16;
  const double absD = fabs(w);
  if (absD >= one) { *c0 = 1.0 - s; *c1 = s; *dc0 = 0.0; *dc1 = 0.0; }
  else {
    // acos / sin / cos of aloam_trig.hpp: the same IEEE operations as the CPU side performs, so the scales — and with them the f32
    // query points and the correspondences — are bit-identical by construction, not merely to an ulp of the device libm
    const double theta = acos_port(absD), st = sin_port(theta), ct = cos_port(theta);
    const double a0 = (1.0 - s) * theta, a1 = s * theta;
    const double s0 = sin_port(a0), s1 = sin_port(a1);
    *c0 = s0 / st;
    *c1 = s1 / st;
    // d/dtheta of sin(k theta) / sin(theta), then d theta / d absD = -1 / sin(theta), d absD / d w = sign(w)
    const double g = (w < 0.0 ? 1.0 : -1.0) / st;
    *dc0 = ((1.0 - s) * cos_port(a0) * st - s0 * ct) / (st * st) * g;
    *dc1 = (s * cos_port(a1) * st - s1 * ct) / (st * st) * g;
  }
  if (w < 0.0) { *c1 = -*c1; *dc1 = -*dc1; }
}

// lp = slerp(I, q, s) * cp + s t (reference src/lidarFactor.hpp:27-32 / :79-84 and TransformToStart) and, if M is given, the
// 3x4 matrix d lp / d (qx, qy, qz, qw) that forward-mode autodiff of those lines produces.
__device__ __forceinline__ void deskew_point(const double q[4], const double t[3], double s, double vx, double vy, double vz,
                                             double lp[3], double (*M)[4]) {
  double c0, c1, dc0, dc1;
  slerp_scales(q[3], s, &c0, &c1, &dc0, &dc1);
  const double u[3] = {c1 * q[0], c1 * q[1], c1 * q[2]}, w = c0 + c1 * q[3];
  const double v[3] = {vx, vy, vz};
  // Eigen: uv = 2 u x v; result = v + w uv + u x uv
  const double uv[3] = {2.0 * (u[1] * v[2] - u[2] * v[1]), 2.0 * (u[2] * v[0] - u[0] * v[2]), 2.0 * (u[0] * v[1] - u[1] * v[0])};
  lp[0] = v[0] + w * uv[0] + (u[1] * uv[2] - u[2] * uv[1]) + s * t[0];
  lp[1] = v[1] + w * uv[1] + (u[2] * uv[0] - u[0] * uv[2]) + s * t[1];
  lp[2] = v[2] + w * uv[2] + (u[0] * uv[1] - u[1] * uv[0]) + s * t[2];
  if (!M) return;
  // d result / d u_k = 2 w (e_k x v) + e_k x uv + u x (2 e_k x v);   d result / d w = uv
  double Du[3][3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    double e[3] = {0.0, 0.0, 0.0};
    e[k] = 1.0;
    const double ev[3] = {2.0 * (e[1] * v[2] - e[2] * v[1]), 2.0 * (e[2] * v[0] - e[0] * v[2]), 2.0 * (e[0] * v[1] - e[1] * v[0])};
    Du[0][k] = w * ev[0] + (e[1] * uv[2] - e[2] * uv[1]) + (u[1] * ev[2] - u[2] * ev[1]);
    Du[1][k] = w * ev[1] + (e[2] * uv[0] - e[0] * uv[2]) + (u[2] * ev[0] - u[0] * ev[2]);
    Du[2][k] = w * ev[2] + (e[0] * uv[1] - e[1] * uv[0]) + (u[0] * ev[1] - u[1] * ev[0]);
  }
  const double dw = dc0 + dc1 * q[3] + c1;                                   // d w / d qw
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    M[r][0] = c1 * Du[r][0];
    M[r][1] = c1 * Du[r][1];
    M[r][2] = c1 * Du[r][2];
    M[r][3] = dc1 * (Du[r][0] * q[0] + Du[r][1] * q[1] + Du[r][2] * q[2]) + uv[r] * dw;
  }
}

// Row of the residual Jacobian in the tangent space Ceres solves in: (d r / d lp) (d lp / d q) Plus'(q), and d lp / d t = s I.
__device__ __forceinline__ void deskew_jacobian_row(const double a[3], const double (*M)[4], const double q[4], double s, double J[6]) {
  double g[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) g[j] = a[0] * M[0][j] + a[1] * M[1][j] + a[2] * M[2][j];
  // EigenQuaternionParameterization Plus Jacobian at delta = 0 (rows x, y, z, w)
  J[0] = g[0] * q[3] - g[1] * q[2] + g[2] * q[1] - g[3] * q[0];
  J[1] = g[0] * q[2] + g[1] * q[3] - g[2] * q[0] - g[3] * q[1];
  J[2] = -g[0] * q[1] + g[1] * q[0] + g[2] * q[3] - g[3] * q[2];
  J[3] = a[0] * s; J[4] = a[1] * s; J[5] = a[2] * s;
}

// -------------------------------------------------------------------------------------------------------
constexpr int kSolveWaves = 2;   // waves per sequence in k_solve; measured at batch 512: 1: 0.62 ms, 2: 0.44, 4: 0.53, 8: 0.87 (two launches)
constexpr int kSolveThreads = 64 * kSolveWaves;
template <bool WITH_JAC, bool DISTORT>
__device__ void evaluate(const OdomArgs& a, int b, const double q[4], const double t[3], double* acc, int* n_edge, int* n_plane) {
  const int tid = threadIdx.x;
  const SeqMeta m = a.meta[b];
  const EdgeRec* E = a.edges + (long long)b * a.R * kSharpPerRing;
  const PlaneRec* P = a.planes + (long long)b * a.R * kFlatPerRing;
  int ne = 0, np = 0;
  for (int i = tid; i < m.n_sharp; i += kSolveThreads) {
    const EdgeRec e = E[i];
    if (!e.valid) continue;
    ++ne;
    double rcp[3], lp[3], M[3][4];
    const double s = DISTORT ? interpolation_ratio(__int_as_float(e.pad[0])) : 1.0;
    if (DISTORT) deskew_point(q, t, s, (double)e.cp[0], (double)e.cp[1], (double)e.cp[2], lp, WITH_JAC ? M : nullptr);
    else {
      quat_rotate(q, (double)e.cp[0], (double)e.cp[1], (double)e.cp[2], rcp);
      lp[0] = rcp[0] + t[0]; lp[1] = rcp[1] + t[1]; lp[2] = rcp[2] + t[2];
    }
    const double ax = e.a[0], ay = e.a[1], az = e.a[2], bx = e.b[0], by = e.b[1], bz = e.b[2];
    const double dex = ax - bx, dey = ay - by, dez = az - bz;
    const double inv = 1.0 / sqrt(dex * dex + dey * dey + dez * dez);
    const double ux = lp[0] - ax, uy = lp[1] - ay, uz = lp[2] - az, vx = lp[0] - bx, vy = lp[1] - by, vz = lp[2] - bz;
    const double r0 = (uy * vz - uz * vy) * inv, r1 = (uz * vx - ux * vz) * inv, r2 = (ux * vy - uy * vx) * inv;
    double rho0, rho1;
    huber(r0 * r0 + r1 * r1 + r2 * r2, &rho0, &rho1);
    acc[27] += 0.5 * rho0;
    if (WITH_JAC) {
      // d r / d lp = [w]x, w = (b - a)/|a-b|;  d lp / d delta = -2 [R cp]x;  d lp / d t = I
      const double wx = -dex * inv, wy = -dey * inv, wz = -dez * inv;
      const double A[3][3] = {{0, -wz, wy}, {wz, 0, -wx}, {-wy, wx, 0}};
      const double Bm[3][3] = {{0, 2 * rcp[2], -2 * rcp[1]}, {-2 * rcp[2], 0, 2 * rcp[0]}, {2 * rcp[1], -2 * rcp[0], 0}};
      const double rr[3] = {r0, r1, r2};
#pragma unroll
      for (int row = 0; row < 3; ++row) {
        double J[6];
        if (DISTORT) deskew_jacobian_row(A[row], M, q, s, J);
        else {
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            J[c] = A[row][0] * Bm[0][c] + A[row][1] * Bm[1][c] + A[row][2] * Bm[2][c];
            J[3 + c] = A[row][c];
          }
        }
        add_row(acc, J, rr[row], rho1);
      }
    }
  }
  for (int i = tid; i < m.n_flat; i += kSolveThreads) {
    const PlaneRec p = P[i];
    if (!p.valid) continue;
    ++np;
    // LidarPlaneFactor ctor: n = normalize((j - l) x (j - m))  (reference src/lidarFactor.hpp:64-65)
    const double jx = p.j[0], jy = p.j[1], jz = p.j[2];
    const double e1x = jx - (double)p.l[0], e1y = jy - (double)p.l[1], e1z = jz - (double)p.l[2];
    const double e2x = jx - (double)p.m[0], e2y = jy - (double)p.m[1], e2z = jz - (double)p.m[2];
    double nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
    const double len = sqrt(nx * nx + ny * ny + nz * nz);
    nx /= len; ny /= len; nz /= len;
    double rcp[3] = {0.0, 0.0, 0.0}, lp[3], M[3][4];
    const double s = DISTORT ? interpolation_ratio(__int_as_float(p.pad[0])) : 1.0;
    if (DISTORT) deskew_point(q, t, s, (double)p.cp[0], (double)p.cp[1], (double)p.cp[2], lp, WITH_JAC ? M : nullptr);
    else {
      quat_rotate(q, (double)p.cp[0], (double)p.cp[1], (double)p.cp[2], rcp);
      lp[0] = rcp[0] + t[0]; lp[1] = rcp[1] + t[1]; lp[2] = rcp[2] + t[2];
    }
    const double r = (lp[0] - jx) * nx + (lp[1] - jy) * ny + (lp[2] - jz) * nz;
    double rho0, rho1;
    huber(r * r, &rho0, &rho1);
    acc[27] += 0.5 * rho0;
    if (WITH_JAC) {
      double J[6];
      const double nn[3] = {nx, ny, nz};
      if (DISTORT) deskew_jacobian_row(nn, M, q, s, J);
      else { J[0] = 2.0 * (nz * rcp[1] - ny * rcp[2]); J[1] = 2.0 * (nx * rcp[2] - nz * rcp[0]); J[2] = 2.0 * (ny * rcp[0] - nx * rcp[1]); J[3] = nx; J[4] = ny; J[5] = nz; }
      add_row(acc, J, r, rho1);
    }
  }
  *n_edge = ne;
  *n_plane = np;
}

}  // namespace aloam
