// a-loam_amd/csrc/graphmarginal_kernels.hip — pose-graph marginals (include/aloam_mi355x.h "pose-graph marginals"; DESIGN.md §7p;
// a-loam_amd/posegraph.py marginals() restates it in numpy).  k_graph_marginals: one workgroup per request on a scratch row of its own.  It
// linearises the request's graph at the estimates, factors the chain without damping, solves H y_c = (J^T)_c for the six rows of the
// candidate's Jacobian by the chain-preconditioned conjugate gradients of k_pose_graph, and one thread assembles Sigma_r = J H^-1 J^T and
// the innovation chi-square.  The linearisation, the matrix-vector product, the dot product, the chain factor and substitution and the
// incidence build are posegraph_kernels.hip's device functions, included here without its kernels; all f64, no floating-point atomics.
#define ALOAM_GRAPH_DEVICE_FUNCTIONS_ONLY
#include "posegraph_kernels.hip"
#include "graphmarginal_kernels.hpp"

namespace aloam {
namespace {

// What the workgroup shares about its candidate: the edge as it is evaluated (flags 0; Z of the estimates in AT_ESTIMATE mode), its
// residual and Jacobians at the estimates, and Sigma_r column by column.
struct Candidate {
  aloam_graph_edge ed;
  double r[6], Ji[36], Jj[36];
  double cov[36];                    // M = J H^-1 J^T before it is symmetrised: column c from solve c
  double m[4][36];                   // the one thread's 6 x 6 work: L(Omega), L^-1, S, L(S)
};

// r, J_i, J_j of one edge: the arithmetic of graph_linearize_edges, for the one candidate.
__device__ void candidate_linearize(Candidate& c, const double qi[4], const double ti[3], const double qj[4], const double tj[3]) {
  double r[6], qe[4], qic[4], qzc[4];
  edge_residual(c.ed, qi, ti, qj, tj, r, qe, qic, qzc);
  for (int k = 0; k < 6; ++k) c.r[k] = r[k];
  double qa[4], RA[3][3], col[3];
  pg_qmul(qzc, qic, qa);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    quat_rotate(qa, k == 0 ? 1.0 : 0.0, k == 1 ? 1.0 : 0.0, k == 2 ? 1.0 : 0.0, col);
    RA[0][k] = col[0]; RA[1][k] = col[1]; RA[2][k] = col[2];
  }
  const double K[3][3] = {{qe[3], qe[2], -qe[1]}, {-qe[2], qe[3], qe[0]}, {qe[1], -qe[0], qe[3]}};
  const double d[3] = {tj[0] - ti[0], tj[1] - ti[1], tj[2] - ti[2]};
  const double X[3][3] = {{0.0, -d[2], d[1]}, {d[2], 0.0, -d[0]}, {-d[1], d[0], 0.0}};
  const bool has_i = c.ed.i >= 0;
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      const double Bm = K[a][0] * RA[0][b] + K[a][1] * RA[1][b] + K[a][2] * RA[2][b];
      const double Sm = RA[a][0] * X[0][b] + RA[a][1] * X[1][b] + RA[a][2] * X[2][b];
      c.Jj[6 * a + b] = Bm; c.Jj[6 * a + 3 + b] = 0.0; c.Jj[6 * (3 + a) + b] = 0.0; c.Jj[6 * (3 + a) + 3 + b] = RA[a][b];
      c.Ji[6 * a + b] = has_i ? -Bm : 0.0; c.Ji[6 * a + 3 + b] = 0.0;
      c.Ji[6 * (3 + a) + b] = has_i ? Sm : 0.0; c.Ji[6 * (3 + a) + 3 + b] = has_i ? -RA[a][b] : 0.0;
    }
}

// Lower Cholesky factor of the symmetric 6 x 6 A (row by row, each sum in index order); false when a pivot is not above kMarginalPivotTol of
// its diagonal entry.
__device__ bool cholesky6(const double* A, double* L) {
  for (int a = 0; a < 6; ++a)
    for (int b = 0; b <= a; ++b) {
      double s = A[6 * a + b];
      for (int m = 0; m < b; ++m) s -= L[6 * a + m] * L[6 * b + m];
      if (a == b) {
        if (!(s > kMarginalPivotTol * A[6 * a + a])) return false;
        L[6 * a + a] = sqrt(s);
      } else {
        L[6 * a + b] = s / L[6 * b + b];
      }
    }
  return true;
}

// chi2 = r^T (cov + Omega^-1)^-1 r by one thread: Omega^-1 = L^-T L^-1 from the factor of Omega, S = cov + Omega^-1 = L_S L_S^T, |L_S^-1 r|^2.
// c.cov is symmetric here.  false when a factorisation fails.
__device__ bool candidate_chi2(Candidate& c, double* chi2) {
  double* Om = c.m[0]; double* L = c.m[1]; double* X = c.m[2]; double* S = c.m[3];
  for (int a = 0; a < 6; ++a)
    for (int b = 0; b < 6; ++b) { Om[6 * a + b] = c.ed.info[sym21(a, b)]; X[6 * a + b] = 0.0; }
  if (!cholesky6(Om, L)) return false;
  for (int k = 0; k < 6; ++k)                  // column k of L^-1 by forward substitution
    for (int a = k; a < 6; ++a) {
      double s = a == k ? 1.0 : 0.0;
      for (int m = k; m < a; ++m) s -= L[6 * a + m] * X[6 * m + k];
      X[6 * a + k] = s / L[6 * a + a];
    }
  for (int a = 0; a < 6; ++a)
    for (int b = 0; b <= a; ++b) {
      double s = 0.0;
      for (int m = a; m < 6; ++m) s += X[6 * m + a] * X[6 * m + b];
      S[6 * a + b] = S[6 * b + a] = c.cov[6 * a + b] + s;
    }
  double* Ls = Om;                             // (Omega itself is no longer needed)
  if (!cholesky6(S, Ls)) return false;
  double y[6], sum = 0.0;
  for (int a = 0; a < 6; ++a) {
    double s = c.r[a];
    for (int m = 0; m < a; ++m) s -= Ls[6 * a + m] * y[m];
    y[a] = s / Ls[6 * a + a];
    sum += y[a] * y[a];
  }
  *chi2 = sum;
  return true;
}

}  // namespace

__global__ __launch_bounds__(kGraphThreads) void k_graph_marginals(GraphMarginalArgs a) {
  __shared__ double s_red[4];
  __shared__ int s_scan[kGraphThreads];
  __shared__ int s_flag;
  __shared__ Candidate s_c;
  const int tid = threadIdx.x;
  const GraphMarginalItem& item = a.items[blockIdx.x];
  const int seq = item.rq.edge.seq, ci = item.rq.edge.i, cj = item.rq.edge.j, mode = item.rq.mode;
  const aloam_graph_node* nodes = a.nodes + (long long)seq * a.max_nodes;
  aloam_graph_marginal_result* out = a.dst + blockIdx.x;
  Work w;
  w.N = item.nodes; w.E = item.edges;
  w.edges = a.edges + (long long)seq * a.max_edges;
  w.huber_delta = a.opt.huber_delta;
  w.Nr = a.row_nodes;
  w.f = a.f64 + (long long)blockIdx.x * a.f64_row;
  w.gi = a.i32 + (long long)blockIdx.x * a.i32_row;

  if (tid == 0) {
    out->mode = mode; out->seq = seq; out->i = ci; out->j = cj; out->nodes = w.N; out->edges = w.E;
    for (int k = 0; k < 4; ++k) out->q[k] = item.rq.edge.q[k];
    for (int k = 0; k < 3; ++k) out->t[k] = item.rq.edge.t[k];
    for (int k = 0; k < 6; ++k) out->r[k] = 0.0;
    for (int k = 0; k < 36; ++k) out->cov[k] = 0.0;
    out->chi2 = 0.0; out->s_edge = 0.0; out->pcg_iterations = 0;
  }
  if (w.N < 2 || w.E < 1) {
    if (tid == 0) out->status = ALOAM_GRAPH_MARGINAL_NO_EDGES;
    return;
  }
  for (int k = tid; k < w.N; k += kGraphThreads) {
    for (int c = 0; c < 4; ++c) w.q()[kNodeRow * k + c] = nodes[k].q_opt[c];
    for (int c = 0; c < 3; ++c) w.t()[kNodeRow * k + c] = nodes[k].t_opt[c];
    for (int c = 0; c < 6; ++c) w.dg()[kNodeRow * k + c] = 0.0;                // no damping: the chain factor and the product read dg * 0
  }
  __syncthreads();
  // the candidate at the estimates, by one thread while the others start on the incidence lists
  if (tid == 0) {
    double qi[4], ti[3], qj[4], tj[3];
    load_pose(w.q(), w.t(), ci, qi, ti);
    load_pose(w.q(), w.t(), cj, qj, tj);
    s_c.ed = item.rq.edge;
    s_c.ed.flags = 0;                          // never robustified
    if (mode == ALOAM_GRAPH_MARGINAL_AT_ESTIMATE) pg_relative(qi, ti, qj, tj, s_c.ed.q, s_c.ed.t);
    candidate_linearize(s_c, qi, ti, qj, tj);
    for (int k = 0; k < 36; ++k) s_c.cov[k] = 0.0;
  }
  graph_build_incidence(w, s_scan);
  const double cost = graph_linearize_edges(w, s_red);
  __syncthreads();
  const double gmax = graph_linearize_nodes(w, s_red);
  bool failed = !isfinite(cost) || !isfinite(gmax);
  if (!failed) {
    if (tid == 0) s_flag = graph_factor_chain(w, 0.0) ? 1 : 0;
    __syncthreads();
    failed = s_flag == 0;
  }

  // Six solves H y = (J^T)_col from y = 0, one after the other in the row's five vectors: the PCG of k_pose_graph without damping.
  bool capped = false;
  int pcg_total = 0;
  for (int col = 0; col < 6 && !failed; ++col) {
    for (int k = 1 + tid; k < w.N; k += kGraphThreads)
      for (int c = 0; c < 6; ++c) {
        w.x()[kNodeRow * k + c] = 0.0;
        w.r()[kNodeRow * k + c] = k == ci ? s_c.Ji[6 * col + c] : k == cj ? s_c.Jj[6 * col + c] : 0.0;
      }
    __syncthreads();
    if (tid == 0) graph_apply_chain(w, w.r(), w.z());
    __syncthreads();
    for (int k = 1 + tid; k < w.N; k += kGraphThreads)
      for (int c = 0; c < 6; ++c) w.p()[kNodeRow * k + c] = w.z()[kNodeRow * k + c];
    double rz = graph_dot(w, w.r(), w.z(), s_red);
    const double rz0 = rz, stop = a.opt.pcg_tolerance * a.opt.pcg_tolerance * rz0;
    if (!isfinite(rz0) || rz0 < 0.0) { failed = true; break; }
    int it = 0;
    bool met = !(rz0 > 0.0);                   // a zero right-hand side (i = -1, j = 0): 0 iterations, y = 0
    while (!met && it < a.opt.pcg_max_iterations) {
      __syncthreads();
      graph_matvec(w, w.p(), w.Ap(), 0.0);
      const double pAp = graph_dot(w, w.p(), w.Ap(), s_red);
      if (!(pAp > 0.0)) { failed = true; break; }
      const double alpha = rz / pAp;
      for (int k = 1 + tid; k < w.N; k += kGraphThreads)
        for (int c = 0; c < 6; ++c) { w.x()[kNodeRow * k + c] += alpha * w.p()[kNodeRow * k + c]; w.r()[kNodeRow * k + c] -= alpha * w.Ap()[kNodeRow * k + c]; }
      ++it;
      __syncthreads();
      if (tid == 0) graph_apply_chain(w, w.r(), w.z());
      __syncthreads();
      const double rz_new = graph_dot(w, w.r(), w.z(), s_red);
      if (!(rz_new > stop)) { met = true; break; }
      const double beta = rz_new / rz;
      for (int k = 1 + tid; k < w.N; k += kGraphThreads)
        for (int c = 0; c < 6; ++c) w.p()[kNodeRow * k + c] = w.z()[kNodeRow * k + c] + beta * w.p()[kNodeRow * k + c];
      rz = rz_new;
    }
    pcg_total += it;
    if (failed) break;
    if (!met) capped = true;
    // Sigma_r[:, col] = J_i y[i] + J_j y[j] (the block of node 0 and of an anchor's i is zero)
    __syncthreads();
    if (tid == 0)
      for (int r = 0; r < 6; ++r) {
        double si = 0.0, sj = 0.0;
        if (ci >= 1) for (int b = 0; b < 6; ++b) si += s_c.Ji[6 * r + b] * w.x()[kNodeRow * ci + b];
        if (cj >= 1) for (int b = 0; b < 6; ++b) sj += s_c.Jj[6 * r + b] * w.x()[kNodeRow * cj + b];
        s_c.cov[6 * r + col] = si + sj;
      }
    __syncthreads();
  }

  if (tid != 0) return;
  int status = failed ? ALOAM_GRAPH_MARGINAL_FAILED : capped ? ALOAM_GRAPH_MARGINAL_NOT_CONVERGED : ALOAM_GRAPH_MARGINAL_OK;
  double chi2 = 0.0, s_edge = 0.0;
  if (!failed) {
    bool zero = true;
    for (int r = 0; r < 6; ++r)
      for (int c = 0; c <= r; ++c) {
        const double v = 0.5 * (s_c.cov[6 * r + c] + s_c.cov[6 * c + r]);
        s_c.cov[6 * r + c] = s_c.cov[6 * c + r] = v;
        if (v != 0.0) zero = false;
      }
    if (mode == ALOAM_GRAPH_MARGINAL_MEASURED) {
      double rho1;
      edge_rho(s_c.ed, s_c.r, w.huber_delta, &s_edge, &rho1);     // flags 0: rho = s = r^T Omega r
      if (zero) chi2 = s_edge;
      else if (!candidate_chi2(s_c, &chi2)) { status = ALOAM_GRAPH_MARGINAL_FAILED; chi2 = 0.0; }
    }
  }
  const bool keep = status != ALOAM_GRAPH_MARGINAL_FAILED;
  out->status = status; out->pcg_iterations = pcg_total;
  out->chi2 = chi2; out->s_edge = s_edge;
  for (int k = 0; k < 6; ++k) out->r[k] = s_c.r[k];
  for (int k = 0; k < 4; ++k) out->q[k] = s_c.ed.q[k];
  for (int k = 0; k < 3; ++k) out->t[k] = s_c.ed.t[k];
  for (int k = 0; k < 36; ++k) out->cov[k] = keep ? s_c.cov[k] : 0.0;
}

void launch_graph_marginals(const GraphMarginalArgs& a, hipStream_t stream) {
  if (a.n > 0) hipLaunchKernelGGL(k_graph_marginals, dim3(a.n), dim3(kGraphThreads), 0, stream, a);
}

}  // namespace aloam
