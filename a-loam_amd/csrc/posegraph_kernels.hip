// a-loam_amd/csrc/posegraph_kernels.hip — pose graphs over keyframes (include/aloam_mi355x.h "pose graphs"; DESIGN.md §7k;
// a-loam_amd/posegraph.py restates every operation in numpy).  k_graph_add_nodes enters the listed sequences' poses as nodes with their
// odometry edges; k_pose_graph optimises one graph per workgroup: Levenberg-Marquardt with the trust-region rules of lm_solve_block, every
// step solved by conjugate gradients preconditioned with the block-tridiagonal chain.  All f64, no floating-point atomics: every sum is
// taken in an order fixed by the graph alone (a thread per edge, a thread per node over its incident edges in edge order, block_sum), so a
// sequence's result does not depend on the list it was in.
#include "lm_device.hpp"
#include "posegraph_kernels.hpp"

namespace aloam {
namespace {

constexpr long long kNodeRow = 200, kEdgeRow = 115;   // doubles per node / per edge of a scratch row (graph_f64_row)

// ---- poses ------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void pg_qmul(const double a[4], const double b[4], double o[4]) {
  o[0] = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
  o[1] = a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2];
  o[2] = a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0];
  o[3] = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
}
__device__ __forceinline__ void pg_conj(const double q[4], double o[4]) { o[0] = -q[0]; o[1] = -q[1]; o[2] = -q[2]; o[3] = q[3]; }
// X_i^-1 o X_j
__device__ __forceinline__ void pg_relative(const double qi[4], const double ti[3], const double qj[4], const double tj[3], double qz[4], double tz[3]) {
  double qc[4];
  pg_conj(qi, qc);
  pg_qmul(qc, qj, qz);
  quat_rotate(qc, tj[0] - ti[0], tj[1] - ti[1], tj[2] - ti[2], tz);
}
__device__ __forceinline__ int sym21(int i, int j) { return i <= j ? 6 * i - i * (i - 1) / 2 + (j - i) : 6 * j - j * (j - 1) / 2 + (i - j); }

__device__ __forceinline__ void load_pose(const double* q, const double* t, int k, double oq[4], double ot[3]) {
  if (k < 0) { oq[0] = oq[1] = oq[2] = 0.0; oq[3] = 1.0; ot[0] = ot[1] = ot[2] = 0.0; return; }
  for (int c = 0; c < 4; ++c) oq[c] = q[kNodeRow * k + c];
  for (int c = 0; c < 3; ++c) ot[c] = t[kNodeRow * k + c];
}

// E = Z^-1 o X_i^-1 o X_j, q_E with w >= 0, r = (2 q_E.xyz, t_E); qic = conj(q_i), qzc = conj(q_Z) are left for the Jacobians.
__device__ __forceinline__ void edge_residual(const aloam_graph_edge& ed, const double qi[4], const double ti[3], const double qj[4], const double tj[3],
                                              double r[6], double qe[4], double qic[4], double qzc[4]) {
  double qd[4], td[3], te[3];
  pg_conj(qi, qic);
  pg_qmul(qic, qj, qd);
  quat_rotate(qic, tj[0] - ti[0], tj[1] - ti[1], tj[2] - ti[2], td);
  pg_conj(ed.q, qzc);
  pg_qmul(qzc, qd, qe);
  quat_rotate(qzc, td[0] - ed.t[0], td[1] - ed.t[1], td[2] - ed.t[2], te);
  if (qe[3] < 0.0) { qe[0] = -qe[0]; qe[1] = -qe[1]; qe[2] = -qe[2]; qe[3] = -qe[3]; }
  r[0] = 2.0 * qe[0]; r[1] = 2.0 * qe[1]; r[2] = 2.0 * qe[2];
  r[3] = te[0]; r[4] = te[1]; r[5] = te[2];
}

// s = r^T Omega r and Ceres' HuberLoss(delta) for flagged edges (lm_device.hpp huber(), with the caller's delta)
__device__ __forceinline__ void edge_rho(const aloam_graph_edge& ed, const double r[6], double delta, double* rho0, double* rho1) {
  double s = 0.0;
#pragma unroll
  for (int a = 0; a < 6; ++a) {
    double o = 0.0;
#pragma unroll
    for (int b = 0; b < 6; ++b) o += ed.info[sym21(a, b)] * r[b];
    s += r[a] * o;
  }
  const double bb = delta * delta;
  if ((ed.flags & ALOAM_GRAPH_EDGE_ROBUST) && s > bb) { const double rs = sqrt(s); *rho0 = 2.0 * delta * rs - bb; *rho1 = fmax(2.2250738585072014e-308, delta / rs); }
  else { *rho0 = s; *rho1 = 1.0; }
}

__device__ __forceinline__ double block_max(double v, double* s_red) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int d = 32; d > 0; d >>= 1) v = fmax(v, shfl_down_f64(v, d));
  if (lane == 0) s_red[wave] = v;
  __syncthreads();
  v = fmax(fmax(s_red[0], s_red[1]), fmax(s_red[2], s_red[3]));
  __syncthreads();
  return v;
}

// exp(th / 2) as a quaternion.  Not inlined: the constants of sin and cos would otherwise be kept in three dozen scalar registers for the
// whole of the solve's loop, which does not have them to spare.
struct Quat { double x, y, z, w; };       // (returned in registers: an array argument would go through the stack)
__device__ __noinline__ Quat pg_exp_half(double tx, double ty, double tz) {
  const double nn = sqrt(tx * tx + ty * ty + tz * tz), h = 0.5 * nn;
  const double kk = nn > 0.0 ? sin(h) / nn : 0.5;
  return Quat{kk * tx, kk * ty, kk * tz, cos(h)};
}

// What one workgroup works on: the graph, and its scratch row.
struct Work {
  int N, E;
  const aloam_graph_edge* edges;
  double huber_delta;
  // The scratch row: one record of kNodeRow doubles per node, then one of kEdgeRow per edge.  An accessor returns the field of record 0 and
  // callers step by the record, so a field is one base register plus an immediate offset (a pointer per array cost sixty scalar registers).
  double* f; int* gi; int Nr;                 // node records (the edge records lie behind them), the integers, nodes a row is laid out for
  __device__ __forceinline__ double* q() const { return f; }                                  // current pose [4], [3]
  __device__ __forceinline__ double* t() const { return f + 4; }
  __device__ __forceinline__ double* qc() const { return f + 7; }                             // candidate pose
  __device__ __forceinline__ double* tc() const { return f + 11; }
  __device__ __forceinline__ double* Hd() const { return f + 14; }                            // diagonal block [36]
  __device__ __forceinline__ double* C() const { return f + 50; }                             // chain block (k, k - 1) [36]
  __device__ __forceinline__ double* L() const { return f + 86; }                             // Cholesky factor of the chain's diagonal (lower, 1 / pivot on it)
  __device__ __forceinline__ double* Ls() const { return f + 122; }                           // its block (k, k - 1)
  __device__ __forceinline__ double* g() const { return f + 158; }                            // gradient [6]
  __device__ __forceinline__ double* dg() const { return f + 164; }                           // LM diagonal [6]
  __device__ __forceinline__ double* x() const { return f + 170; }                            // PCG vectors [6] each
  __device__ __forceinline__ double* r() const { return f + 176; }
  __device__ __forceinline__ double* z() const { return f + 182; }
  __device__ __forceinline__ double* p() const { return f + 188; }
  __device__ __forceinline__ double* Ap() const { return f + 194; }
  __device__ __forceinline__ double* er() const { return f + kNodeRow * Nr; }                 // per edge: r [6]
  __device__ __forceinline__ double* ew() const { return f + kNodeRow * Nr + 6; }             //   rho' [1]
  __device__ __forceinline__ double* eJi() const { return f + kNodeRow * Nr + 7; }            //   J_i, J_j, w J_i^T Omega J_j [36] each
  __device__ __forceinline__ double* eJj() const { return f + kNodeRow * Nr + 43; }
  __device__ __forceinline__ double* eH() const { return f + kNodeRow * Nr + 79; }
  // incidence: entries 2 e + side (0: the node is i, 1: it is j), per node in ascending order
  __device__ __forceinline__ int* cnt() const { return gi; }
  __device__ __forceinline__ int* start() const { return gi + Nr; }
  __device__ __forceinline__ int* cursor() const { return gi + 2 * Nr + 1; }
  __device__ __forceinline__ int* inc() const { return gi + 3 * Nr + 1; }
};

// 1/2 sum rho at the poses (q, t): a thread per edge, block_sum.
__device__ double graph_cost(const Work& w, const double* q, const double* t, double* s_red) {
  double c = 0.0;
  for (int e = threadIdx.x; e < w.E; e += kGraphThreads) {
    const aloam_graph_edge& ed = w.edges[e];
    double qi[4], ti[3], qj[4], tj[3], r[6], qe[4], qic[4], qzc[4], rho0, rho1;
    load_pose(q, t, ed.i, qi, ti);
    load_pose(q, t, ed.j, qj, tj);
    edge_residual(ed, qi, ti, qj, tj, r, qe, qic, qzc);
    edge_rho(ed, r, w.huber_delta, &rho0, &rho1);
    c += rho0;
  }
  block_sum<1, 4>(&c, s_red);
  return 0.5 * c;
}

// A thread per edge: r, rho', J_i, J_j (left tangent of the two nodes, order (theta, t)) and the off-diagonal block w J_i^T Omega J_j.
__device__ double graph_linearize_edges(const Work& w, double* s_red) {
  double c = 0.0;
  for (int e = threadIdx.x; e < w.E; e += kGraphThreads) {
    const aloam_graph_edge& ed = w.edges[e];
    double qi[4], ti[3], qj[4], tj[3], r[6], qe[4], qic[4], qzc[4], rho0, rho1;
    load_pose(w.q(), w.t(), ed.i, qi, ti);
    load_pose(w.q(), w.t(), ed.j, qj, tj);
    edge_residual(ed, qi, ti, qj, tj, r, qe, qic, qzc);
    edge_rho(ed, r, w.huber_delta, &rho0, &rho1);
    c += rho0;
    for (int k = 0; k < 6; ++k) w.er()[kEdgeRow * e + k] = r[k];
    w.ew()[kEdgeRow * e] = rho1;
    // R_A, A = Z^-1 o X_i^-1: column k is A's rotation of the unit vector k
    double qa[4], RA[3][3], col[3];
    pg_qmul(qzc, qic, qa);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      quat_rotate(qa, k == 0 ? 1.0 : 0.0, k == 1 ? 1.0 : 0.0, k == 2 ? 1.0 : 0.0, col);
      RA[0][k] = col[0]; RA[1][k] = col[1]; RA[2][k] = col[2];
    }
    // B = (w I - [v]x) R_A = d(2 q_E.xyz) / d theta_j;  S = R_A [t_j - t_i]x
    const double K[3][3] = {{qe[3], qe[2], -qe[1]}, {-qe[2], qe[3], qe[0]}, {qe[1], -qe[0], qe[3]}};
    const double d[3] = {tj[0] - ti[0], tj[1] - ti[1], tj[2] - ti[2]};
    const double X[3][3] = {{0.0, -d[2], d[1]}, {d[2], 0.0, -d[0]}, {-d[1], d[0], 0.0}};
    // J_j = [B 0; 0 R_A], J_i = [-B 0; S -R_A] (zero for an anchor): the 3 x 3 blocks stay in registers, the 6 x 6 matrices go to memory
    double Bm[3][3], Sm[3][3];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int b = 0; b < 3; ++b) {
        Bm[a][b] = K[a][0] * RA[0][b] + K[a][1] * RA[1][b] + K[a][2] * RA[2][b];
        Sm[a][b] = RA[a][0] * X[0][b] + RA[a][1] * X[1][b] + RA[a][2] * X[2][b];
      }
    const bool has_i = ed.i >= 0;
    double* oJi = w.eJi() + kEdgeRow * e; double* oJj = w.eJj() + kEdgeRow * e; double* oH = w.eH() + kEdgeRow * e;
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int b = 0; b < 3; ++b) {
        oJj[6 * a + b] = Bm[a][b]; oJj[6 * a + 3 + b] = 0.0; oJj[6 * (3 + a) + b] = 0.0; oJj[6 * (3 + a) + 3 + b] = RA[a][b];
        oJi[6 * a + b] = has_i ? -Bm[a][b] : 0.0; oJi[6 * a + 3 + b] = 0.0;
        oJi[6 * (3 + a) + b] = has_i ? Sm[a][b] : 0.0; oJi[6 * (3 + a) + 3 + b] = has_i ? -RA[a][b] : 0.0;
      }
    // H_ij = w J_i^T (Omega J_j), a column of Omega J_j at a time: column b of J_j is (B[:, b]; 0) or (0; R_A[:, b - 3])
#pragma unroll
    for (int b = 0; b < 6; ++b) {
      double T[6];
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        double o = 0.0;
#pragma unroll
        for (int m = 0; m < 3; ++m) o += ed.info[sym21(k, b < 3 ? m : 3 + m)] * (b < 3 ? Bm[m][b] : RA[m][b - 3]);
        T[k] = o;
      }
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        double top = 0.0, bottom = 0.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) { top += Sm[k][a] * T[3 + k] - Bm[k][a] * T[k]; bottom -= RA[k][a] * T[3 + k]; }
        oH[6 * a + b] = has_i ? rho1 * top : 0.0;
        oH[6 * (3 + a) + b] = has_i ? rho1 * bottom : 0.0;
      }
    }
  }
  block_sum<1, 4>(&c, s_red);
  return 0.5 * c;
}

// A thread per node over its incident edges in edge order: the diagonal block sum w J^T Omega J, the gradient sum w J^T Omega r, and the
// chain block (k, k - 1) = the sum of the off-diagonal blocks of its edges to node k - 1.  Returns the gradient's max-norm over nodes >= 1.
__device__ double graph_linearize_nodes(const Work& w, double* s_red) {
  double gm = 0.0;
  for (int k = threadIdx.x; k < w.N; k += kGraphThreads) {
    double A[6][6], g[6];
#pragma unroll
    for (int a = 0; a < 6; ++a) { g[a] = 0.0;
#pragma unroll
      for (int b = 0; b < 6; ++b) A[a][b] = 0.0; }
    const int lo = w.start()[k], hi = w.start()[k + 1];
    for (int n = lo; n < hi; ++n) {
      const int code = w.inc()[n], e = code >> 1;
      const aloam_graph_edge& ed = w.edges[e];
      const double* Jp = (code & 1 ? w.eJj() : w.eJi()) + kEdgeRow * e;
      const double rho1 = w.ew()[kEdgeRow * e];
      double J[6][6], r[6];
#pragma unroll
      for (int a = 0; a < 6; ++a) { r[a] = w.er()[kEdgeRow * e + a];
#pragma unroll
        for (int b = 0; b < 6; ++b) J[a][b] = Jp[6 * a + b]; }
#pragma unroll
      for (int b = 0; b < 6; ++b) {
        double T[6], tr = 0.0;
#pragma unroll
        for (int m = 0; m < 6; ++m) {
          double o = 0.0;
#pragma unroll
          for (int c = 0; c < 6; ++c) o += ed.info[sym21(m, c)] * J[c][b];
          T[m] = o;
          tr += o * r[m];
        }
        g[b] += rho1 * tr;
#pragma unroll
        for (int a = 0; a <= b; ++a) {           // J^T Omega J is symmetric: the upper triangle is accumulated, and mirrored when it is stored
          double o = 0.0;
#pragma unroll
          for (int m = 0; m < 6; ++m) o += J[m][a] * T[m];
          A[a][b] += rho1 * o;
        }
      }
    }
#pragma unroll
    for (int a = 0; a < 6; ++a) { w.g()[kNodeRow * k + a] = g[a];
#pragma unroll
      for (int b = a; b < 6; ++b) { w.Hd()[kNodeRow * k + 6 * a + b] = A[a][b]; w.Hd()[kNodeRow * k + 6 * b + a] = A[a][b]; } }
    if (k >= 1) {
#pragma unroll
      for (int a = 0; a < 6; ++a) gm = fmax(gm, fabs(g[a]));
    }
    // chain block: rows of node k, columns of node k - 1
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
      for (int b = 0; b < 6; ++b) A[a][b] = 0.0;
    for (int n = lo; n < hi; ++n) {
      const int code = w.inc()[n], e = code >> 1;
      const aloam_graph_edge& ed = w.edges[e];
      const int other = code & 1 ? ed.i : ed.j;
      if (other != k - 1 || k < 2) continue;
      const double* H = w.eH() + kEdgeRow * e;     // rows of i, columns of j
#pragma unroll
      for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int b = 0; b < 6; ++b) A[a][b] += code & 1 ? H[6 * b + a] : H[6 * a + b];
    }
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
      for (int b = 0; b < 6; ++b) w.C()[kNodeRow * k + 6 * a + b] = A[a][b];
  }
  return block_max(gm, s_red);
}

// out = (H + diag(dg / radius)) v over the nodes 1 .. N - 1 (node 0 is fixed: its entries are never read), a thread per node.
__device__ void graph_matvec(const Work& w, const double* v, double* out, double inv_radius) {
  for (int k = 1 + threadIdx.x; k < w.N; k += kGraphThreads) {
    double o[6], vk[6];
#pragma unroll
    for (int a = 0; a < 6; ++a) vk[a] = v[kNodeRow * k + a];
#pragma unroll
    for (int a = 0; a < 6; ++a) {
      double s = w.dg()[kNodeRow * k + a] * inv_radius * vk[a];
#pragma unroll
      for (int b = 0; b < 6; ++b) s += w.Hd()[kNodeRow * k + 6 * a + b] * vk[b];
      o[a] = s;
    }
    for (int n = w.start()[k]; n < w.start()[k + 1]; ++n) {
      const int code = w.inc()[n], e = code >> 1;
      const aloam_graph_edge& ed = w.edges[e];
      const int other = code & 1 ? ed.i : ed.j;
      if (other < 1) continue;               // an anchor, or the fixed node
      const double* H = w.eH() + kEdgeRow * e;
      double vo[6];
#pragma unroll
      for (int a = 0; a < 6; ++a) vo[a] = v[kNodeRow * other + a];
#pragma unroll
      for (int a = 0; a < 6; ++a) {
        double s = 0.0;
#pragma unroll
        for (int b = 0; b < 6; ++b) s += (code & 1 ? H[6 * b + a] : H[6 * a + b]) * vo[b];
        o[a] += s;
      }
    }
#pragma unroll
    for (int a = 0; a < 6; ++a) out[kNodeRow * k + a] = o[a];
  }
}

__device__ double graph_dot(const Work& w, const double* u, const double* v, double* s_red) {
  double s = 0.0;
  for (int k = 1 + threadIdx.x; k < w.N; k += kGraphThreads)
    for (int a = 0; a < 6; ++a) s += u[kNodeRow * k + a] * v[kNodeRow * k + a];
  block_sum<1, 4>(&s, s_red);
  return s;
}

// M = the chain (every diagonal block with its LM diagonal, and the blocks (k, k - 1)) = L L^T with L block-bidiagonal, by one thread with the
// front (one 6 x 6 factor) in registers: the recurrence is sequential in k, and one lane keeps it free of any cross-lane order.
// L[k]: lower triangle, 1 / pivot on the diagonal.  Ls[k] = C[k] L[k - 1]^-T.  false when a pivot is not positive.
__device__ bool graph_factor_chain(const Work& w, double inv_radius) {
  double Lp[6][6];                           // the factor of node k - 1; the identity ahead of node 1, whose chain block is zero
#pragma unroll
  for (int a = 0; a < 6; ++a)
#pragma unroll
    for (int b = 0; b < 6; ++b) Lp[a][b] = a == b ? 1.0 : 0.0;
  for (int k = 1; k < w.N; ++k) {
    double M[6][6], S[6][6];
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
      for (int b = 0; b < 6; ++b) M[a][b] = w.Hd()[kNodeRow * k + 6 * a + b] + (a == b ? w.dg()[kNodeRow * k + a] * inv_radius : 0.0);
    {
      // S L_prev^T = C: row a of S by forward substitution
#pragma unroll
      for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int b = 0; b < 6; ++b) {
          double s = w.C()[kNodeRow * k + 6 * a + b];
#pragma unroll
          for (int m = 0; m < b; ++m) s -= S[a][m] * Lp[b][m];
          S[a][b] = s * Lp[b][b];
        }
#pragma unroll
      for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int b = 0; b < 6; ++b) {
          w.Ls()[kNodeRow * k + 6 * a + b] = S[a][b];
          if (b <= a) {
            double s = 0.0;
#pragma unroll
            for (int m = 0; m < 6; ++m) s += S[a][m] * S[b][m];
            M[a][b] -= s;
          }
        }
    }
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
      for (int b = 0; b <= a; ++b) {
        double s = M[a][b];
#pragma unroll
        for (int m = 0; m < b; ++m) s -= Lp[a][m] * Lp[b][m];
        if (a == b) {
          if (!(s > 0.0)) return false;
          Lp[a][a] = 1.0 / sqrt(s);
        } else {
          Lp[a][b] = s * Lp[b][b];
        }
      }
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
      for (int b = 0; b < 6; ++b) w.L()[kNodeRow * k + 6 * a + b] = b <= a ? Lp[a][b] : 0.0;
  }
  return true;
}

// z = M^-1 r: forward and backward substitution along the chain, by the same one thread.
__device__ void graph_apply_chain(const Work& w, const double* r, double* z) {
  double y[6] = {0, 0, 0, 0, 0, 0};
  for (int k = 1; k < w.N; ++k) {
    const double* Lk = w.L() + kNodeRow * k; const double* Sk = w.Ls() + kNodeRow * k;
    double v[6];
#pragma unroll
    for (int a = 0; a < 6; ++a) {
      double s = r[kNodeRow * k + a];
#pragma unroll
      for (int b = 0; b < 6; ++b) s -= Sk[6 * a + b] * y[b];     // (node 1: Ls is zero and so is y)
      v[a] = s;
    }
#pragma unroll
    for (int a = 0; a < 6; ++a) {
      double s = v[a];
#pragma unroll
      for (int b = 0; b < a; ++b) s -= Lk[6 * a + b] * y[b];
      y[a] = s * Lk[6 * a + a];
    }
#pragma unroll
    for (int a = 0; a < 6; ++a) z[kNodeRow * k + a] = y[a];
  }
  double xk[6] = {0, 0, 0, 0, 0, 0};
  for (int k = w.N - 1; k >= 1; --k) {
    const double* Lk = w.L() + kNodeRow * k;
    double v[6];
#pragma unroll
    for (int a = 0; a < 6; ++a) {
      double s = z[kNodeRow * k + a];
      if (k + 1 < w.N) {
        const double* Sn = w.Ls() + kNodeRow * (k + 1);
#pragma unroll
        for (int b = 0; b < 6; ++b) s -= Sn[6 * b + a] * xk[b];
      }
      v[a] = s;
    }
#pragma unroll
    for (int a = 5; a >= 0; --a) {
      double s = v[a];
#pragma unroll
      for (int b = a + 1; b < 6; ++b) s -= Lk[6 * b + a] * xk[b];
      xk[a] = s * Lk[6 * a + a];
    }
#pragma unroll
    for (int a = 0; a < 6; ++a) z[kNodeRow * k + a] = xk[a];
  }
}

// The incidence list, once per call: counts (integer atomics), an exclusive scan, the fill, and every node's entries sorted ascending, which
// is edge order.
__device__ void graph_build_incidence(const Work& w, int* s_scan) {
  const int tid = threadIdx.x;
  for (int k = tid; k < w.N; k += kGraphThreads) { w.cnt()[k] = 0; w.cursor()[k] = 0; }
  __syncthreads();
  for (int e = tid; e < w.E; e += kGraphThreads) {
    atomicAdd(&w.cnt()[w.edges[e].j], 1);
    if (w.edges[e].i >= 0) atomicAdd(&w.cnt()[w.edges[e].i], 1);
  }
  __syncthreads();
  const int chunk = (w.N + kGraphThreads - 1) / kGraphThreads, lo = min(w.N, tid * chunk), hi = min(w.N, lo + chunk);
  int s = 0;
  for (int k = lo; k < hi; ++k) s += w.cnt()[k];
  s_scan[tid] = s;
  __syncthreads();
  if (tid == 0) {
    int run = 0;
    for (int k = 0; k < kGraphThreads; ++k) { const int v = s_scan[k]; s_scan[k] = run; run += v; }
    w.start()[w.N] = run;
  }
  __syncthreads();
  int base = s_scan[tid];
  for (int k = lo; k < hi; ++k) { w.start()[k] = base; base += w.cnt()[k]; }
  __syncthreads();
  for (int e = tid; e < w.E; e += kGraphThreads) {
    const int i = w.edges[e].i, j = w.edges[e].j;
    w.inc()[w.start()[j] + atomicAdd(&w.cursor()[j], 1)] = 2 * e + 1;
    if (i >= 0) w.inc()[w.start()[i] + atomicAdd(&w.cursor()[i], 1)] = 2 * e;
  }
  __syncthreads();
  for (int k = tid; k < w.N; k += kGraphThreads) {
    const int a = w.start()[k], b = w.start()[k + 1];
    for (int n = a + 1; n < b; ++n) {
      const int v = w.inc()[n];
      int m = n - 1;
      while (m >= a && w.inc()[m] > v) { w.inc()[m + 1] = w.inc()[m]; --m; }
      w.inc()[m + 1] = v;
    }
  }
  __syncthreads();
}

}  // namespace

#ifndef ALOAM_GRAPH_DEVICE_FUNCTIONS_ONLY      // graphmarginal_kernels.hip includes this file for the device functions above, without the kernels
// ---- the store --------------------------------------------------------------------------------------------------------------------------
// A thread per new node: the pose as aloam_export_poses reports it, the odometry edge Z = X[k-1]^-1 o X[k] of the entered poses, and the
// estimate X_opt[k-1] o Z.
__global__ __launch_bounds__(64) void k_graph_add_nodes(GraphAddArgs a) {
  const int n = blockIdx.x * 64 + threadIdx.x;
  if (n >= a.n) return;
  const GraphAddItem& it = a.items[n];
  const int b = it.seq, k = it.node;
  aloam_graph_node* row = a.nodes + (long long)b * a.max_nodes;
  aloam_graph_node nd;
  if (a.mapseq) {
    const MapSeq& m = a.mapseq[b];
    for (int c = 0; c < 4; ++c) nd.q[c] = m.par[c];
    for (int c = 0; c < 3; ++c) nd.t[c] = m.par[4 + c];
    nd.frame = m.frame_count;
  } else {
    const OdomState& s = a.odom[b];
    for (int c = 0; c < 4; ++c) nd.q[c] = s.q_w[c];
    for (int c = 0; c < 3; ++c) nd.t[c] = s.t_w[c];
    nd.frame = -1;
  }
  nd.pad[0] = nd.pad[1] = nd.pad[2] = 0;
  if (k == 0) {
    for (int c = 0; c < 4; ++c) nd.q_opt[c] = nd.q[c];
    for (int c = 0; c < 3; ++c) nd.t_opt[c] = nd.t[c];
  } else {
    const aloam_graph_node& pv = row[k - 1];
    aloam_graph_edge& ed = a.edges[(long long)b * a.max_edges + it.edge];
    double qz[4], tz[3], rt[3];
    pg_relative(pv.q, pv.t, nd.q, nd.t, qz, tz);
    pg_qmul(pv.q_opt, qz, nd.q_opt);
    quat_rotate(pv.q_opt, tz[0], tz[1], tz[2], rt);
    for (int c = 0; c < 3; ++c) nd.t_opt[c] = rt[c] + pv.t_opt[c];
    ed.seq = b; ed.i = k - 1; ed.j = k; ed.flags = 0;
    for (int c = 0; c < 4; ++c) ed.q[c] = qz[c];
    for (int c = 0; c < 3; ++c) ed.t[c] = tz[c];
    for (int c = 0; c < 21; ++c) ed.info[c] = it.info[c];
  }
  row[k] = nd;
}

void launch_graph_add_nodes(const GraphAddArgs& a, hipStream_t stream) {
  hipLaunchKernelGGL(k_graph_add_nodes, dim3((a.n + 63) / 64), dim3(64), 0, stream, a);
}

// ---- the solve --------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ Work graph_work(const GraphSolveArgs& a, const GraphSolveItem& item) {
  Work w;
  w.N = item.nodes; w.E = item.edges;
  w.edges = a.edges + (long long)item.seq * a.max_edges;
  w.Nr = a.row_nodes;
  w.f = a.f64 + (long long)blockIdx.x * a.f64_row;
  w.gi = a.i32 + (long long)blockIdx.x * a.i32_row;
  return w;
}

// The incidence lists of the listed graphs, once per call and ahead of the solve: a kernel of its own keeps its counters and its scan out of
// the solve's register and LDS budget.
__global__ __launch_bounds__(kGraphThreads) void k_graph_incidence(GraphSolveArgs a) {
  __shared__ int s_scan[kGraphThreads];
  const GraphSolveItem item = a.items[blockIdx.x];
  if (item.nodes < 2 || item.edges < 1) return;
  graph_build_incidence(graph_work(a, item), s_scan);
}

__global__ __launch_bounds__(kGraphThreads) void k_pose_graph(GraphSolveArgs a) {
  __shared__ double s_red[4];
  __shared__ int s_flag;
  __shared__ aloam_graph_options s_opt;      // the options, read where they are used: ten scalar registers less for the whole solve
  const int tid = threadIdx.x;
  const GraphSolveItem item = a.items[blockIdx.x];
  aloam_graph_node* nodes = a.nodes + (long long)item.seq * a.max_nodes;
  Work w = graph_work(a, item);
  if (tid == 0) s_opt = a.opt;
  __syncthreads();
  w.huber_delta = s_opt.huber_delta;

  aloam_graph_result res;
  res.status = ALOAM_GRAPH_OK; res.termination = 0; res.lm_iterations = 0; res.accepted_steps = 0; res.pcg_iterations = 0;
  res.nodes = w.N; res.edges = w.E; res.pad = 0;
  res.initial_cost = 0.0; res.final_cost = 0.0; res.gradient_max = 0.0; res.reserved = 0.0;
  if (w.N < 2 || w.E < 1) {
    res.status = ALOAM_GRAPH_NO_EDGES;
    if (tid == 0) a.dst[blockIdx.x] = res;
    return;
  }
  for (int k = tid; k < w.N; k += kGraphThreads) {
    for (int c = 0; c < 4; ++c) w.q()[kNodeRow * k + c] = nodes[k].q_opt[c];
    for (int c = 0; c < 3; ++c) w.t()[kNodeRow * k + c] = nodes[k].t_opt[c];
  }
  __syncthreads();

  // The trust-region loop of lm_solve_block (lm_device.hpp), every thread running the uniform scalar logic: no Jacobi scaling, no parameter
  // tolerance, the gradient's plain max-norm, and a step that comes from PCG (DESIGN.md §7k names the deviations).  The linearisation has
  // one call site, at the head of the loop: before the first iteration and after every accepted step.
  const double kMinRelDecrease = 1e-3, kMinDiag = 1e-6, kMaxDiag = 1e32, kMaxRadius = 1e16, kMinRadius = 1e-32;
  double cost = 0.0, gmax = 0.0, initial_cost = 0.0;
  double radius = 1e4, decrease_factor = 2.0;
  bool reuse_diagonal = false, linearize = true;
  int n_invalid = 0, iter = 0, termination = 0, accepted = 0, pcg_total = 0;
  while (true) {
    if (linearize) {
      cost = graph_linearize_edges(w, s_red);
      __syncthreads();
      gmax = graph_linearize_nodes(w, s_red);
      if (accepted == 0) initial_cost = cost;
      linearize = false;
      if (!isfinite(cost) || !isfinite(gmax)) { termination = 5; break; }     // a non-finite cost, gradient or block: FAILURE, as lm_solve_block
    }
    if (iter >= s_opt.max_iterations) { termination = 0; break; }
    if (gmax <= s_opt.gradient_tolerance) { termination = 3; break; }
    if (radius <= kMinRadius) { termination = 6; break; }
    ++iter;
    if (!reuse_diagonal)
      for (int k = 1 + tid; k < w.N; k += kGraphThreads)
        for (int c = 0; c < 6; ++c) w.dg()[kNodeRow * k + c] = fmin(fmax(w.Hd()[kNodeRow * k + 7 * c], kMinDiag), kMaxDiag);
    reuse_diagonal = true;
    const double inv_radius = 1.0 / radius;
    __syncthreads();
    if (tid == 0) s_flag = graph_factor_chain(w, inv_radius) ? 1 : 0;
    __syncthreads();
    bool ok = s_flag != 0;
    double model_change = 0.0;
    if (ok) {
      // PCG on (H + D) x = g from x = 0
      for (int k = 1 + tid; k < w.N; k += kGraphThreads)
        for (int c = 0; c < 6; ++c) { w.x()[kNodeRow * k + c] = 0.0; w.r()[kNodeRow * k + c] = w.g()[kNodeRow * k + c]; }
      __syncthreads();
      if (tid == 0) graph_apply_chain(w, w.r(), w.z());
      __syncthreads();
      for (int k = 1 + tid; k < w.N; k += kGraphThreads)
        for (int c = 0; c < 6; ++c) w.p()[kNodeRow * k + c] = w.z()[kNodeRow * k + c];
      double rz = graph_dot(w, w.r(), w.z(), s_red);
      const double rz0 = rz, stop = s_opt.pcg_tolerance * s_opt.pcg_tolerance * rz0;
      ok = rz0 > 0.0 && isfinite(rz0);
      int it = 0;
      while (ok && it < s_opt.pcg_max_iterations) {
        __syncthreads();
        graph_matvec(w, w.p(), w.Ap(), inv_radius);
        const double pAp = graph_dot(w, w.p(), w.Ap(), s_red);
        if (!(pAp > 0.0)) { ok = false; break; }
        const double alpha = rz / pAp;
        for (int k = 1 + tid; k < w.N; k += kGraphThreads)
          for (int c = 0; c < 6; ++c) { w.x()[kNodeRow * k + c] += alpha * w.p()[kNodeRow * k + c]; w.r()[kNodeRow * k + c] -= alpha * w.Ap()[kNodeRow * k + c]; }
        ++it;
        __syncthreads();
        if (tid == 0) graph_apply_chain(w, w.r(), w.z());
        __syncthreads();
        const double rz_new = graph_dot(w, w.r(), w.z(), s_red);
        if (!(rz_new > stop)) break;
        const double beta = rz_new / rz;
        for (int k = 1 + tid; k < w.N; k += kGraphThreads)
          for (int c = 0; c < 6; ++c) w.p()[kNodeRow * k + c] = w.z()[kNodeRow * k + c] + beta * w.p()[kNodeRow * k + c];
        rz = rz_new;
      }
      pcg_total += it;
      if (ok) {
        // model_change = x^T g - 1/2 x^T H x, H x = (H + D) x - D x
        __syncthreads();
        graph_matvec(w, w.x(), w.Ap(), inv_radius);
        double s = 0.0;
        for (int k = 1 + tid; k < w.N; k += kGraphThreads)
          for (int c = 0; c < 6; ++c) {
            const double xv = w.x()[kNodeRow * k + c];
            s += xv * w.g()[kNodeRow * k + c] - 0.5 * xv * (w.Ap()[kNodeRow * k + c] - w.dg()[kNodeRow * k + c] * inv_radius * xv);
          }
        block_sum<1, 4>(&s, s_red);
        model_change = s;
        ok = isfinite(s);
      }
    }
    if (!ok || !(model_change > 0.0)) {
      if (++n_invalid >= 5) { termination = 5; break; }
      radius = radius / decrease_factor;
      decrease_factor *= 2.0;
      continue;
    }
    n_invalid = 0;
    // the candidate: q' = exp(-x_theta / 2) q, t' = t - x_t
    for (int k = tid; k < w.N; k += kGraphThreads) {
      double q[4], qn[4];
      for (int c = 0; c < 4; ++c) q[c] = w.q()[kNodeRow * k + c];
      if (k == 0) { for (int c = 0; c < 4; ++c) qn[c] = q[c]; for (int c = 0; c < 3; ++c) w.tc()[c] = w.t()[c]; }
      else {
        const Quat e = pg_exp_half(-w.x()[kNodeRow * k], -w.x()[kNodeRow * k + 1], -w.x()[kNodeRow * k + 2]);
        const double dq[4] = {e.x, e.y, e.z, e.w};
        pg_qmul(dq, q, qn);
        for (int c = 0; c < 3; ++c) w.tc()[kNodeRow * k + c] = w.t()[kNodeRow * k + c] - w.x()[kNodeRow * k + 3 + c];
      }
      for (int c = 0; c < 4; ++c) w.qc()[kNodeRow * k + c] = qn[c];
    }
    __syncthreads();
    const double cost_c = graph_cost(w, w.qc(), w.tc(), s_red);
    if (fabs(cost - cost_c) <= s_opt.function_tolerance * cost) { termination = 2; break; }
    const double rel = (cost - cost_c) / model_change;
    if (rel > kMinRelDecrease && isfinite(cost_c)) {
      for (int k = tid; k < w.N; k += kGraphThreads) {
        for (int c = 0; c < 4; ++c) w.q()[kNodeRow * k + c] = w.qc()[kNodeRow * k + c];
        for (int c = 0; c < 3; ++c) w.t()[kNodeRow * k + c] = w.tc()[kNodeRow * k + c];
      }
      __syncthreads();
      ++accepted;
      linearize = true;
      const double c3 = 2.0 * rel - 1.0;
      radius = fmin(kMaxRadius, radius / fmax(1.0 / 3.0, 1.0 - c3 * c3 * c3));
      decrease_factor = 2.0;
      reuse_diagonal = false;
    } else {
      radius = radius / decrease_factor;
      decrease_factor *= 2.0;
    }
  }

  const bool usable = termination != 5 && cost <= initial_cost;
  if (!usable) res.status = ALOAM_GRAPH_FAILED;
  res.initial_cost = initial_cost;
  res.termination = termination; res.lm_iterations = iter; res.accepted_steps = accepted; res.pcg_iterations = pcg_total;
  res.final_cost = usable ? cost : initial_cost; res.gradient_max = gmax;
  __syncthreads();
  if (usable && accepted > 0)
    for (int k = 1 + tid; k < w.N; k += kGraphThreads) {
      for (int c = 0; c < 4; ++c) nodes[k].q_opt[c] = w.q()[kNodeRow * k + c];
      for (int c = 0; c < 3; ++c) nodes[k].t_opt[c] = w.t()[kNodeRow * k + c];
    }
  if (tid == 0) a.dst[blockIdx.x] = res;
}

void launch_pose_graph(const GraphSolveArgs& a, hipStream_t stream) {
  hipLaunchKernelGGL(k_graph_incidence, dim3(a.n), dim3(kGraphThreads), 0, stream, a);
  hipLaunchKernelGGL(k_pose_graph, dim3(a.n), dim3(kGraphThreads), 0, stream, a);
}

#endif  // ALOAM_GRAPH_DEVICE_FUNCTIONS_ONLY

}  // namespace aloam
