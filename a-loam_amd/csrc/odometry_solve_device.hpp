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
// Waves per sequence in k_solve.  Measured at batch 512 on the kernel of rounds 1 - 9, whose every factor cost two dependent global round trips in every
// pass: 1: 0.62 ms, 2: 0.44, 4: 0.53, 8: 0.87 (two launches).  Not measured again since the records are fetched ahead and kept in LDS (HISTORY round 10): the
// LDS layout below and the thread's validity masks are sized for this value.
constexpr int kSolveWaves = 2;
constexpr int kSolveThreads = 64 * kSolveWaves;
constexpr int kSolveAhead = 2;   // records k_solve fetches ahead of the one it works on: 16 registers each; the kernel must stay within 512 with nothing in scratch

// ---- a thread's factor records: its slots ----------------------------------------------------------------
// Thread t owns records t, t + kSolveThreads, ... of each class, its slots 0, 1, ..., and adds their terms to its sums in that order, edges first, invalid
// records skipped in place (the order of the f64 sums is part of the result).  A record is fetched whole, `valid` with it, and the fetch of the thread's
// next record(s) is issued before the f64 work of the current one: k_solve runs one wave per SIMD, nothing else covers a round trip to memory.
//
// k_solve keeps in LDS what the evaluations after the first need of a valid record: the pose-independent values the first one has computed anyway,
//   plane   cp, j as f32; the unit normal as three f64           48 B   (l and m are needed for the normal only)
//   edge    cp, a, b as f32; 1 / |a - b| as f64                  44 B
// plus the f32 interpolation fraction with distortion, field-major and thread-minor (a wave's ds_read_b64 / b32 of one field are consecutive: no bank
// conflict), and which of its slots are valid in two registers.  The writer of a slot is its only reader: no barrier.  Every later value is produced by
// the same operations on the same operands as without the copy.  One wave per SIMD means two workgroups per CU, so a workgroup may take half of the
// 160 KiB; the planes are kept first (they save the normal: a cross product, a square root and three divisions), the edges take what is left, and the
// slots that do not fit are read from global memory in every pass, as all are with ALOAM_SOLVE_STAGE=0.
// Beside a grid build: aloam_odometry_step called on its own builds the next step's grids beside association and solve (k_build_grids_fused_next, 1024
// threads and 98 KB of LDS per workgroup).  With 448 B a solve workgroup fitted on a CU that holds a build workgroup; with 80 KiB it does not (178 of
// 160 KiB) and waits for a CU without one.  That build's persistent workgroups number half the CUs and, at the headline shape, end 2.9 ms into a chain whose
// first solve starts behind both associations, 4.5 ms in (HISTORY round 9), so the two rarely meet; the headline path (aloam_process_*) builds beside
// k_ring_features and never beside the solve.  The step called on its own is measured at batch 1 only (bench.py's latency leg, faster than before).
constexpr int kSolveLdsBudget = 80 * 1024;
constexpr int kSolveStaticLds = kSolveWaves * 28 * (int)sizeof(double);     // s_red of the block reductions
constexpr int kPlaneKeepBytes = 6 * 4 + 3 * 8, kEdgeKeepBytes = 9 * 4 + 8;
struct SolveStage { int plane_slots, edge_slots, bytes; };                  // slots per thread kept in LDS, and the dynamic LDS they take
__host__ __device__ constexpr int solve_slots(int records) { return (records + kSolveThreads - 1) / kSolveThreads; }
__host__ __device__ constexpr SolveStage solve_stage(int R, bool distort) {
  const int per_plane = (kPlaneKeepBytes + (distort ? 4 : 0)) * kSolveThreads, per_edge = (kEdgeKeepBytes + (distort ? 4 : 0)) * kSolveThreads;
  const int room = kSolveLdsBudget - kSolveStaticLds;
  const int all_p = solve_slots(R * kFlatPerRing), all_e = solve_slots(R * kSharpPerRing);
  const int np = room / per_plane < all_p ? room / per_plane : all_p;
  const int ne = (room - np * per_plane) / per_edge < all_e ? (room - np * per_plane) / per_edge : all_e;
  return SolveStage{np, ne, np * per_plane + ne * per_edge};
}
static_assert(solve_slots(kMaxRings * kFlatPerRing) <= 32 && solve_slots(kMaxRings * kSharpPerRing) <= 32, "a thread's validity masks are 32 bits per class");
struct SolveKeep { SolveStage lds; unsigned plane_valid, edge_valid; };     // per thread, from the first evaluation of a solve to its last

struct EdgeFetch { float4 v[3]; };                // cp a | a b | b valid pad pad
struct PlaneFetch { float4 v[4]; };               // cp j | j l | l m | valid pad pad pad
struct EdgeKept { float cp[3], a[3], b[3], frac; double inv; };
struct PlaneKept { float cp[3], j[3], frac; double n[3]; };

// Slots k0 .. k1 - 1 in order: term(load(k), k), with the loads of the next AHEAD slots issued before the term of the current one (past the last slot
// the last one's address is loaded again, not the one behind it).
template <int AHEAD, class Load, class Term>
__device__ __forceinline__ void walk_ahead(int k0, int k1, Load&& load, Term&& term) {
  if (k0 >= k1) return;
  if constexpr (AHEAD == 0) {
    for (int k = k0; k < k1; ++k) term(load(k), k);
    return;
  }
  decltype(load(0)) r[AHEAD > 0 ? AHEAD : 1];
#pragma unroll
  for (int d = 0; d < AHEAD; ++d) r[d] = load(k0 + d < k1 ? k0 + d : k1 - 1);
  for (int k = k0; k < k1; k += AHEAD) {
#pragma unroll
    for (int d = 0; d < AHEAD; ++d) {
      if (k + d < k1) {
        const auto cur = r[d];
        r[d] = load(k + d + AHEAD < k1 ? k + d + AHEAD : k1 - 1);
        term(cur, k + d);
      }
    }
  }
}

// STAGE 0: every record from global memory (k_pose_information_odom; any evaluation is correct in this form).  1: the same, and what the slots of
// keep->lds need later goes to LDS (the first evaluation of a solve).  2: those slots from LDS, the others from global memory.
template <bool WITH_JAC, bool DISTORT, int STAGE = 0, int AHEAD = 1>
__device__ __forceinline__ void evaluate(const OdomArgs& a, int b, const double q[4], const double t[3], double* acc, int* n_edge, int* n_plane, SolveKeep* keep = nullptr) {
  constexpr int T = kSolveThreads, NPF = 6 + (DISTORT ? 1 : 0), NEF = 9 + (DISTORT ? 1 : 0);
  extern __shared__ double s_keep[];
  const int tid = threadIdx.x;
  const SeqMeta m = a.meta[b];
  const float4* E = reinterpret_cast<const float4*>(a.edges + (long long)b * a.R * kSharpPerRing);
  const float4* P = reinterpret_cast<const float4*>(a.planes + (long long)b * a.R * kFlatPerRing);
  const int slots_e = tid < m.n_sharp ? (m.n_sharp - tid + T - 1) / T : 0, slots_p = tid < m.n_flat ? (m.n_flat - tid + T - 1) / T : 0;
  const int kept_p = STAGE ? keep->lds.plane_slots : 0, kept_e = STAGE ? keep->lds.edge_slots : 0;
  double* const s_pn = s_keep + tid;                                            // [kept_p][3][T]
  double* const s_inv = s_keep + kept_p * 3 * T + tid;                          // [kept_e][T]
  float* const s_pf = reinterpret_cast<float*>(s_keep + (kept_p * 3 + kept_e) * T) + tid;   // [kept_p][NPF][T]
  float* const s_ef = reinterpret_cast<float*>(s_keep + (kept_p * 3 + kept_e) * T) + kept_p * NPF * T + tid;   // [kept_e][NEF][T]
  int ne = 0, np = 0;

  auto edge_term = [&](const EdgeKept& e) {
    ++ne;
    double rcp[3], lp[3], M[3][4];
    const double s = DISTORT ? interpolation_ratio(e.frac) : 1.0;
    if (DISTORT) deskew_point(q, t, s, (double)e.cp[0], (double)e.cp[1], (double)e.cp[2], lp, WITH_JAC ? M : nullptr);
    else {
      quat_rotate(q, (double)e.cp[0], (double)e.cp[1], (double)e.cp[2], rcp);
      lp[0] = rcp[0] + t[0]; lp[1] = rcp[1] + t[1]; lp[2] = rcp[2] + t[2];
    }
    const double ax = e.a[0], ay = e.a[1], az = e.a[2], bx = e.b[0], by = e.b[1], bz = e.b[2];
    const double dex = ax - bx, dey = ay - by, dez = az - bz;
    const double inv = e.inv;
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
  };
  // a record as it lies in global memory: LidarEdgeFactor's 1 / |a - b| computed here, kept if the slot is
  auto edge_record = [&](const EdgeFetch& f, int k) {
    if (!__float_as_int(f.v[2].y)) return;
    EdgeKept e = {{f.v[0].x, f.v[0].y, f.v[0].z}, {f.v[0].w, f.v[1].x, f.v[1].y}, {f.v[1].z, f.v[1].w, f.v[2].x}, f.v[2].z, 0.0};
    const double dex = (double)e.a[0] - (double)e.b[0], dey = (double)e.a[1] - (double)e.b[1], dez = (double)e.a[2] - (double)e.b[2];
    e.inv = 1.0 / sqrt(dex * dex + dey * dey + dez * dez);
    if (STAGE == 1 && k < kept_e) {
      keep->edge_valid |= 1u << k;
      float* const f32 = s_ef + k * NEF * T;
#pragma unroll
      for (int c = 0; c < 3; ++c) { f32[c * T] = e.cp[c]; f32[(3 + c) * T] = e.a[c]; f32[(6 + c) * T] = e.b[c]; }
      if (DISTORT) f32[9 * T] = e.frac;
      s_inv[k * T] = e.inv;
    }
    edge_term(e);
  };
  auto edge_global = [&](int k) { const float4* p = E + (long long)(tid + k * T) * 3; return EdgeFetch{{p[0], p[1], p[2]}}; };
  int first_e = 0;
  if (STAGE == 1) keep->edge_valid = 0;
  if (STAGE == 2) {
    first_e = slots_e < kept_e ? slots_e : kept_e;
    walk_ahead<1>(0, first_e, [&](int k) {
      EdgeKept e;
      const float* const f32 = s_ef + k * NEF * T;
#pragma unroll
      for (int c = 0; c < 3; ++c) { e.cp[c] = f32[c * T]; e.a[c] = f32[(3 + c) * T]; e.b[c] = f32[(6 + c) * T]; }
      e.frac = DISTORT ? f32[9 * T] : 0.0f;
      e.inv = s_inv[k * T];
      return e;
    }, [&](const EdgeKept& e, int k) { if (keep->edge_valid >> k & 1u) edge_term(e); });
  }
  walk_ahead<AHEAD>(first_e, slots_e, edge_global, edge_record);

  auto plane_term = [&](const PlaneKept& p) {
    ++np;
    const double jx = p.j[0], jy = p.j[1], jz = p.j[2];
    const double nx = p.n[0], ny = p.n[1], nz = p.n[2];
    double rcp[3] = {0.0, 0.0, 0.0}, lp[3], M[3][4];
    const double s = DISTORT ? interpolation_ratio(p.frac) : 1.0;
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
  };
  auto plane_record = [&](const PlaneFetch& f, int k) {
    if (!__float_as_int(f.v[3].x)) return;
    PlaneKept p = {{f.v[0].x, f.v[0].y, f.v[0].z}, {f.v[0].w, f.v[1].x, f.v[1].y}, f.v[3].y, {0.0, 0.0, 0.0}};
    // LidarPlaneFactor ctor: n = normalize((j - l) x (j - m))  (reference src/lidarFactor.hpp:64-65)
    const double jx = p.j[0], jy = p.j[1], jz = p.j[2];
    const double e1x = jx - (double)f.v[1].z, e1y = jy - (double)f.v[1].w, e1z = jz - (double)f.v[2].x;
    const double e2x = jx - (double)f.v[2].y, e2y = jy - (double)f.v[2].z, e2z = jz - (double)f.v[2].w;
    double nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
    const double len = sqrt(nx * nx + ny * ny + nz * nz);
    p.n[0] = nx / len; p.n[1] = ny / len; p.n[2] = nz / len;
    if (STAGE == 1 && k < kept_p) {
      keep->plane_valid |= 1u << k;
      float* const f32 = s_pf + k * NPF * T;
#pragma unroll
      for (int c = 0; c < 3; ++c) { f32[c * T] = p.cp[c]; f32[(3 + c) * T] = p.j[c]; s_pn[(k * 3 + c) * T] = p.n[c]; }
      if (DISTORT) f32[6 * T] = p.frac;
    }
    plane_term(p);
  };
  auto plane_global = [&](int k) { const float4* p = P + (long long)(tid + k * T) * 4; return PlaneFetch{{p[0], p[1], p[2], p[3]}}; };
  int first_p = 0;
  if (STAGE == 1) keep->plane_valid = 0;
  if (STAGE == 2) {
    first_p = slots_p < kept_p ? slots_p : kept_p;
    walk_ahead<1>(0, first_p, [&](int k) {
      PlaneKept p;
      const float* const f32 = s_pf + k * NPF * T;
#pragma unroll
      for (int c = 0; c < 3; ++c) { p.cp[c] = f32[c * T]; p.j[c] = f32[(3 + c) * T]; p.n[c] = s_pn[(k * 3 + c) * T]; }
      p.frac = DISTORT ? f32[6 * T] : 0.0f;
      return p;
    }, [&](const PlaneKept& p, int k) { if (keep->plane_valid >> k & 1u) plane_term(p); });
  }
  walk_ahead<AHEAD>(first_p, slots_p, plane_global, plane_record);
  *n_edge = ne;
  *n_plane = np;
}

}  // namespace aloam
