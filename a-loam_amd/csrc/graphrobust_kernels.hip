// a-loam_amd/csrc/graphrobust_kernels.hip — the robust pose-graph solve (include/aloam_mi355x.h "the robust solve"; DESIGN.md §7s;
// a-loam_amd/posegraph.py optimize_robust() restates it in numpy).  k_graph_robust: one workgroup per listed graph runs the whole of
// GNC-TLS, graduated non-convexity with a truncated least-squares loss over the edges flagged ALOAM_GRAPH_EDGE_ROBUST: an outer loop that
// evaluates s = r^T Omega r of every edge, turns it into a weight, and solves the weighted problem by the Levenberg-Marquardt of
// k_pose_graph.  The workgroup keeps a scratch copy of its graph's edges with the information scaled by the weight and the flag cleared,
// and points Work::edges at it: the cost, the linearisation, the matrix-vector product, the dot product, the chain factor and substitution
// and the incidence build are then posegraph_kernels.hip's device functions unchanged, included here without its kernels.  A weight of 0
// is an all-zero information to them: s = 0, rho' = 1, zero blocks.  All f64, no floating-point atomics: every sum is taken in an order
// fixed by the graph alone, so a sequence's result does not depend on the list it was in.
#define ALOAM_GRAPH_DEVICE_FUNCTIONS_ONLY
#include "posegraph_kernels.hip"
#include "graphrobust_kernels.hpp"

namespace aloam {
namespace {

// s = r^T Omega r of one edge at the poses (q, t), with the edge's own information whatever its flag: the sum of edge_rho.
__device__ __forceinline__ double robust_edge_s(const aloam_graph_edge& ed, const double* q, const double* t) {
  double qi[4], ti[3], qj[4], tj[3], r[6], qe[4], qic[4], qzc[4];
  load_pose(q, t, ed.i, qi, ti);
  load_pose(q, t, ed.j, qj, tj);
  edge_residual(ed, qi, ti, qj, tj, r, qe, qic, qzc);
  double s = 0.0;
#pragma unroll
  for (int a = 0; a < 6; ++a) {
    double o = 0.0;
#pragma unroll
    for (int b = 0; b < 6; ++b) o += ed.info[sym21(a, b)] * r[b];
    s += r[a] * o;
  }
  return s;
}

// The weight of a flagged edge at mu: 1 up to lo = mu / (mu + 1) c2, 0 from hi = (mu + 1) / mu c2, sqrt(c2 mu (mu + 1) / s) - mu between.
__device__ __forceinline__ double robust_weight(double s, double mu, double c2) {
  const double lo = mu / (mu + 1.0) * c2, hi = (mu + 1.0) / mu * c2;
  if (s <= lo) return 1.0;
  if (s >= hi) return 0.0;
  return sqrt(c2 * mu * (mu + 1.0) / s) - mu;
}

// The part of a scratch row behind the row of k_pose_graph: the scaled copies of the edges back to back (Work::edges indexes them), then
// (w, s) per edge.  (kNodeRow and kEdgeRow are what graph_f64_row multiplies by.)
__device__ __forceinline__ aloam_graph_edge* robust_scaled(const GraphRobustArgs& a, double* row) {
  return reinterpret_cast<aloam_graph_edge*>(row + kNodeRow * a.g.row_nodes + kEdgeRow * a.g.row_edges);
}
__device__ __forceinline__ double* robust_ws(const GraphRobustArgs& a, double* row) {
  return row + kNodeRow * a.g.row_nodes + kEdgeRow * a.g.row_edges + (kRobustEdgeRow - 2) * a.g.row_edges;
}

struct RobustState {
  aloam_graph_node* nodes;           // the sequence's rows of the store; the edges as entered: read, never written
  const aloam_graph_edge* src;
  double* ws; double* wout;          // (w, s) per edge of the scratch row; the caller's weight row or nullptr
  double mu, undecided;
  int outer, lm_total, accepted_total, pcg_total;
};

__device__ __forceinline__ Work robust_work(const GraphRobustArgs& a, const GraphSolveItem& item) {
  Work w;
  w.N = item.nodes; w.E = item.edges;
  w.Nr = a.g.row_nodes;
  w.f = a.g.f64 + (long long)blockIdx.x * a.g.f64_row;
  w.gi = a.g.i32 + (long long)blockIdx.x * a.g.i32_row;
  w.edges = robust_scaled(a, w.f);
  w.huber_delta = 1.0;                       // unused: the scaled copies carry no flag
  return w;
}

}  // namespace

// The incidence lists of the listed graphs, once per call and ahead of the solve, as k_graph_incidence: they depend on the edges' i and j
// alone, which the scaled copies share with the store.
__global__ __launch_bounds__(kGraphThreads) void k_graph_robust_incidence(GraphRobustArgs a) {
  __shared__ int s_scan[kGraphThreads];
  const GraphSolveItem item = a.g.items[blockIdx.x];
  if (item.nodes < 2 || item.edges < 1) return;
  Work w = robust_work(a, item);
  w.edges = a.g.edges + (long long)item.seq * a.g.max_edges;
  graph_build_incidence(w, s_scan);
}

__global__ __launch_bounds__(kGraphThreads) void k_graph_robust(GraphRobustArgs a) {
  __shared__ double s_red[4];
  __shared__ int s_flag;
  __shared__ aloam_graph_options s_opt;      // the options, read where they are used, as k_pose_graph
  __shared__ aloam_graph_robust_options s_rb;
  // What lives across the outer loop lies in LDS and is read where it is used, for the reason s_opt does: the inner solve has no scalar
  // registers to spare.  Thread 0 writes between barriers; the result is assembled there field by field.
  __shared__ RobustState s_st;
  __shared__ aloam_graph_robust_result s_res;
  const int tid = threadIdx.x;
  const GraphSolveItem item = a.g.items[blockIdx.x];
  const Work w = robust_work(a, item);
  if (tid == 0) {
    s_opt = a.g.opt; s_rb = a.robust;
    s_st.nodes = a.g.nodes + (long long)item.seq * a.g.max_nodes;
    s_st.src = a.g.edges + (long long)item.seq * a.g.max_edges;
    s_st.ws = robust_ws(a, w.f);
    s_st.wout = a.weights ? a.weights + (long long)blockIdx.x * a.weights_stride : nullptr;
    s_st.mu = 0.0; s_st.undecided = 0.0; s_st.outer = 0; s_st.lm_total = 0; s_st.accepted_total = 0; s_st.pcg_total = 0;
  }
  __syncthreads();

  aloam_graph_robust_result& res = s_res;    // (written by thread 0 alone)
  if (tid == 0) {
    res.solve.status = ALOAM_GRAPH_OK; res.solve.termination = 0; res.solve.lm_iterations = 0; res.solve.accepted_steps = 0; res.solve.pcg_iterations = 0;
    res.solve.nodes = w.N; res.solve.edges = w.E; res.solve.pad = 0;
    res.solve.initial_cost = 0.0; res.solve.final_cost = 0.0; res.solve.gradient_max = 0.0; res.solve.reserved = 0.0;
    res.outer_iterations = 0; res.robust_edges = 0; res.inliers = 0; res.outliers = 0;
    res.mu = 0.0; res.s_max = 0.0; res.truncated_cost = 0.0; res.reserved[0] = res.reserved[1] = res.reserved[2] = 0.0;
  }
  if (w.N < 2 || w.E < 1) {
    if (s_st.wout) for (int e = tid; e < w.E; e += kGraphThreads) s_st.wout[e] = 1.0;
    if (tid == 0) { res.solve.status = ALOAM_GRAPH_NO_EDGES; a.dst[blockIdx.x] = res; }
    return;
  }

  // ---- step 1: the poses, and s of every edge at the entry estimates
  double bad = 0.0;
  for (int k = tid; k < w.N; k += kGraphThreads) {
    const aloam_graph_node* nodes = s_st.nodes;
    for (int c = 0; c < 4; ++c) { const double v = nodes[k].q_opt[c]; w.q()[kNodeRow * k + c] = v; if (!isfinite(v)) bad = 1.0; }
    for (int c = 0; c < 3; ++c) { const double v = nodes[k].t_opt[c]; w.t()[kNodeRow * k + c] = v; if (!isfinite(v)) bad = 1.0; }
  }
  __syncthreads();
  double s_sum = 0.0, s_max = 0.0, n_robust = 0.0;
  for (int e = tid; e < w.E; e += kGraphThreads) {
    const aloam_graph_edge* src = s_st.src; double* ws = s_st.ws;
    const double s = robust_edge_s(src[e], w.q(), w.t());
    s_sum += s;
    if (!isfinite(s)) bad = 1.0;
    if (src[e].flags & ALOAM_GRAPH_EDGE_ROBUST) { n_robust += 1.0; s_max = fmax(s_max, s); }
    ws[2 * e] = 1.0; ws[2 * e + 1] = s;
  }
  block_sum<1, 4>(&s_sum, s_red);
  block_sum<1, 4>(&n_robust, s_red);         // (a count: exact in f64)
  s_max = block_max(s_max, s_red);
  bad = block_max(bad, s_red);
  if (tid == 0) { res.solve.initial_cost = res.solve.final_cost = 0.5 * s_sum; res.robust_edges = (int)n_robust; }
  if (bad != 0.0) {
    if (s_st.wout) for (int e = tid; e < w.E; e += kGraphThreads) s_st.wout[e] = 1.0;
    if (tid == 0) { res.solve.status = ALOAM_GRAPH_FAILED; res.solve.termination = 5; a.dst[blockIdx.x] = res; }
    return;
  }

  // ---- steps 2 and 3: the outer loop.  skip: no flagged edge, or none beyond c2 / 2: one solve with every weight 1.
  const bool skip = n_robust == 0.0 || !(2.0 * s_max - s_rb.inlier_chi2 > 0.0);
  if (tid == 0) { res.s_max = s_max; s_st.mu = skip ? 0.0 : s_rb.inlier_chi2 / (2.0 * s_max - s_rb.inlier_chi2); }
  int termination = 0;
  double cost = 0.0, gmax = 0.0;
  bool failed = false;
  while (true) {
    __syncthreads();                         // mu and the counters as thread 0 left them
    // the weights at the current estimates and the scaled copy of the edges; undecided: a weight strictly between 0 and 1
    double undecided = 0.0;
    for (int e = tid; e < w.E; e += kGraphThreads) {
      const double mu = s_st.mu, c2 = s_rb.inlier_chi2;
      double* ws = s_st.ws;
      const aloam_graph_edge& ed = s_st.src[e];
      double wgt = 1.0;
      if (!skip) {
        const double s = robust_edge_s(ed, w.q(), w.t());
        ws[2 * e + 1] = s;
        if (ed.flags & ALOAM_GRAPH_EDGE_ROBUST) wgt = robust_weight(s, mu, c2);
      }
      ws[2 * e] = wgt;
      if (wgt != 0.0 && wgt != 1.0) undecided = 1.0;
      aloam_graph_edge& o = const_cast<aloam_graph_edge*>(w.edges)[e];        // the row's own scaled copy (robust_scaled)
      o.seq = ed.seq; o.i = ed.i; o.j = ed.j; o.flags = 0;
      for (int c = 0; c < 4; ++c) o.q[c] = ed.q[c];
      for (int c = 0; c < 3; ++c) o.t[c] = ed.t[c];
      for (int c = 0; c < 21; ++c) o.info[c] = wgt * ed.info[c];
    }
    undecided = block_max(undecided, s_red);           // (its barriers stand between the copy's writes and the solve's reads)
    if (tid == 0) { s_st.undecided = undecided; ++s_st.outer; }

    // The inner solve: the trust-region loop of k_pose_graph restated statement for statement.  posegraph_kernels.hip keeps that loop
    // inside its kernel and is pinned as it stands (its kernels, their register counts and its include lines are tested), so the loop
    // cannot be shared and is duplicated here; a change to one is a change to both.
    const double kMinRelDecrease = 1e-3, kMinDiag = 1e-6, kMaxDiag = 1e32, kMaxRadius = 1e16, kMinRadius = 1e-32;
    double inner_initial = 0.0;
    double radius = 1e4, decrease_factor = 2.0;
    bool reuse_diagonal = false, linearize = true;
    int n_invalid = 0, iter = 0, accepted = 0, pcg_inner = 0;
    termination = 0;
    while (true) {
      if (linearize) {
        cost = graph_linearize_edges(w, s_red);
        __syncthreads();
        gmax = graph_linearize_nodes(w, s_red);
        if (accepted == 0) inner_initial = cost;
        linearize = false;
        if (!isfinite(cost) || !isfinite(gmax)) { termination = 5; break; }
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
        pcg_inner += it;
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
    __syncthreads();
    if (tid == 0) { s_st.lm_total += iter; s_st.accepted_total += accepted; s_st.pcg_total += pcg_inner; }
    if (termination == 5 || !(cost <= inner_initial)) { failed = true; break; }       // the inner solve ended as a failure
    if (skip || s_st.undecided == 0.0 || s_st.outer >= s_rb.max_outer_iterations) break;
    __syncthreads();
    if (tid == 0) s_st.mu *= s_rb.mu_step;
  }
  __syncthreads();

  // ---- step 4 and the result: after a failure everything is reported at the entry estimates
  if (failed) {
    for (int k = tid; k < w.N; k += kGraphThreads) {
      const aloam_graph_node* nodes = s_st.nodes;
      for (int c = 0; c < 4; ++c) w.q()[kNodeRow * k + c] = nodes[k].q_opt[c];
      for (int c = 0; c < 3; ++c) w.t()[kNodeRow * k + c] = nodes[k].t_opt[c];
    }
    __syncthreads();
  }
  double truncated = 0.0, n_in = 0.0, n_out = 0.0;
  for (int e = tid; e < w.E; e += kGraphThreads) {
    const aloam_graph_edge* src = s_st.src; double* ws = s_st.ws; double* wout = s_st.wout;
    const double s = robust_edge_s(src[e], w.q(), w.t());
    ws[2 * e + 1] = s;
    if (src[e].flags & ALOAM_GRAPH_EDGE_ROBUST) {
      truncated += fmin(s, s_rb.inlier_chi2);
      if (ws[2 * e] == 1.0) n_in += 1.0;
      if (ws[2 * e] == 0.0) n_out += 1.0;
    } else {
      truncated += s;
    }
    if (wout) wout[e] = ws[2 * e];
  }
  block_sum<1, 4>(&truncated, s_red);
  block_sum<1, 4>(&n_in, s_red);
  block_sum<1, 4>(&n_out, s_red);
  if (tid == 0) {
    res.solve.status = failed ? ALOAM_GRAPH_FAILED : ALOAM_GRAPH_OK;
    res.solve.termination = termination; res.solve.gradient_max = gmax;
    res.solve.lm_iterations = s_st.lm_total; res.solve.accepted_steps = s_st.accepted_total; res.solve.pcg_iterations = s_st.pcg_total;
    if (!failed) res.solve.final_cost = cost;          // (after a failure: the entry cost)
    res.outer_iterations = s_st.outer; res.inliers = (int)n_in; res.outliers = (int)n_out;
    res.mu = s_st.mu; res.truncated_cost = 0.5 * truncated;
  }
  if (!failed && s_st.accepted_total > 0)
    for (int k = 1 + tid; k < w.N; k += kGraphThreads) {
      aloam_graph_node* nodes = s_st.nodes;
      for (int c = 0; c < 4; ++c) nodes[k].q_opt[c] = w.q()[kNodeRow * k + c];
      for (int c = 0; c < 3; ++c) nodes[k].t_opt[c] = w.t()[kNodeRow * k + c];
    }
  if (tid == 0) a.dst[blockIdx.x] = res;
}

void launch_graph_robust(const GraphRobustArgs& a, hipStream_t stream) {
  if (a.g.n <= 0) return;
  hipLaunchKernelGGL(k_graph_robust_incidence, dim3(a.g.n), dim3(kGraphThreads), 0, stream, a);
  hipLaunchKernelGGL(k_graph_robust, dim3(a.g.n), dim3(kGraphThreads), 0, stream, a);
}

}  // namespace aloam
