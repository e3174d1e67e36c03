// a-loam_amd/csrc/graphapply_kernels.hip — gfx950 kernel that carries a solved pose graph into the live state.
//   k_graph_apply   one workgroup of 1024 per listed sequence, modelled on k_atlas_window.  One lane forms the correction D from the last
//                   node, the corrected poses and the new window centre.  With ALOAM_GRAPH_APPLY_MAP the filtered segments of the map pass
//                   that ran before (sorted by class, then cube[0], cube[1], cube[2]) are scattered into a table of the 4851 window cubes in
//                   LDS - the window is cube[2]-major, so that is a permutation -, both class totals are tested against the pool row, then
//                   per class a block scan, the descriptors and a flat copy with four loads of a thread in flight before its stores.
//                   MapSeq is written behind a barrier, then the nodes are rebased and the result record is written.
// Integer work, a few dozen f64 operations of one lane and 16-byte point copies: HBM- and latency-bound, no MFMA.  No atomics; all stores
// are plain vector stores.
#include "graphapply_kernels.hpp"

#include "export_kernels.hpp"
#include "lm_device.hpp"
#include "map_window_device.hpp"

namespace aloam {

namespace {

__device__ __forceinline__ void ga_qmul(const double a[4], const double b[4], double o[4]) {
  o[0] = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
  o[1] = a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2];
  o[2] = a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0];
  o[3] = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
}

// X := D o X
__device__ __forceinline__ void ga_correct(const double qd[4], const double td[3], const double q[4], const double t[3], double qo[4], double to[3]) {
  double r[3];
  ga_qmul(qd, q, qo);
  quat_rotate(qd, t[0], t[1], t[2], r);
  to[0] = r[0] + td[0]; to[1] = r[1] + td[1]; to[2] = r[2] + td[2];
}

// Window index of the absolute cube in `key` (atlas_key) for a window centred at (cx, cy, cz); -1 outside the window.
__device__ __forceinline__ int ga_window_index(int key, int cx, int cy, int cz) {
  const int x = (key >> 20) - kAtlasBias + cx, y = ((key >> 10) & 1023) - kAtlasBias + cy, z = (key & 1023) - kAtlasBias + cz;
  return (x >= 0 && x < kMapW && y >= 0 && y < kMapH && z >= 0 && z < kMapD) ? x + kMapW * y + kMapW * kMapH * z : -1;
}

// Of segments [lo, hi): filtered points and non-empty cubes inside the window, filtered points outside it.
__device__ __forceinline__ void ga_totals(const GraphApplyArgs& a, int lo, int hi, int cx, int cy, int cz, int* lds, int* points, int* cubes, int* outside) {
  int np = 0, nc = 0, no = 0;
  for (int s = lo + (int)threadIdx.x; s < hi; s += 1024) {
    const int n = a.counts[s];
    if (ga_window_index(a.seg[s].cube_key, cx, cy, cz) >= 0) { np += n; nc += n > 0; } else no += n;
  }
  (void)block_exclusive_scan<int, 1024>(np, lds, points);
  (void)block_exclusive_scan<int, 1024>(nc, lds, cubes);
  (void)block_exclusive_scan<int, 1024>(no, lds, outside);
}

constexpr int kGaPer = (kMapCubes + 1023) / 1024;          // 5 cubes per thread

enum GaPose { kGaQd = 0, kGaTd = 4, kGaQm = 7, kGaTm = 11, kGaPar = 14, kGaDoubles = 21 };

}  // namespace

__global__ __launch_bounds__(1024) void k_graph_apply(GraphApplyArgs a) {
  const int i = blockIdx.x, tid = threadIdx.x;
  const GaItem it = a.items[i];
  MapSeq& ms = a.seq[it.seq];
  aloam_graph_node* N = a.nodes + (long long)it.seq * a.max_nodes;
  __shared__ double s_pose[kGaDoubles];
  __shared__ int s_cen[3], s_scan[1024], s_pref[kMapCubes + 1], s_first[kMapCubes];
  const bool with_map = (it.flags & ALOAM_GRAPH_APPLY_MAP) != 0;
  aloam_graph_apply_result res{};
  res.nodes = it.nodes;
  if (it.nodes <= 0) {                                                       // an empty graph: nothing to apply
    if (tid == 0) {
      res.status = ALOAM_GRAPH_APPLY_NO_NODES;
      res.cen[0] = ms.cen[0]; res.cen[1] = ms.cen[1]; res.cen[2] = ms.cen[2];
      res.q_corr[3] = 1.0;
      a.dst[i] = res;
    }
    return;
  }
  if (tid == 0) {
    const aloam_graph_node& x = N[it.nodes - 1];                             // the live pose is the last node's frame
    double q[4], t[3], qo[4], to[3], qd[4], td[3], r[3];
#pragma unroll
    for (int k = 0; k < 4; ++k) { q[k] = k < 3 ? -x.q[k] : x.q[k]; qo[k] = x.q_opt[k]; }
#pragma unroll
    for (int k = 0; k < 3; ++k) { t[k] = x.t[k]; to[k] = x.t_opt[k]; }
    ga_qmul(qo, q, qd);                                                      // q_opt conj(q)
    const double nrm = sqrt(qd[0] * qd[0] + qd[1] * qd[1] + qd[2] * qd[2] + qd[3] * qd[3]);
#pragma unroll
    for (int k = 0; k < 4; ++k) qd[k] = qd[k] / nrm;
    quat_rotate(qd, t[0], t[1], t[2], r);
#pragma unroll
    for (int k = 0; k < 3; ++k) td[k] = to[k] - r[k];
    double qm[4], tm[3], qp[4], tp[3], qn[4], tn[3];
#pragma unroll
    for (int k = 0; k < 4; ++k) { qm[k] = ms.q_wmap_wodom[k]; qp[k] = ms.par[k]; }
#pragma unroll
    for (int k = 0; k < 3; ++k) { tm[k] = ms.t_wmap_wodom[k]; tp[k] = ms.par[4 + k]; }
#pragma unroll
    for (int k = 0; k < 4; ++k) s_pose[kGaQd + k] = qd[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) s_pose[kGaTd + k] = td[k];
    ga_correct(qd, td, qm, tm, qn, tn);
#pragma unroll
    for (int k = 0; k < 4; ++k) s_pose[kGaQm + k] = qn[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) s_pose[kGaTm + k] = tn[k];
    ga_correct(qd, td, qp, tp, qn, tn);
#pragma unroll
    for (int k = 0; k < 4; ++k) s_pose[kGaPar + k] = qn[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) s_pose[kGaPar + 4 + k] = tn[k];
    // the sensor's cube at the centre of the window (with ALOAM_GRAPH_APPLY_POSE alone the window stays where it is)
    s_cen[0] = with_map ? 10 - cube_coord(tn[0], 0) : ms.cen[0];
    s_cen[1] = with_map ? 10 - cube_coord(tn[1], 0) : ms.cen[1];
    s_cen[2] = with_map ? 5 - cube_coord(tn[2], 0) : ms.cen[2];
  }
  __syncthreads();
  const int cx = s_cen[0], cy = s_cen[1], cz = s_cen[2];
  res.cen[0] = cx; res.cen[1] = cy; res.cen[2] = cz;
#pragma unroll
  for (int k = 0; k < 4; ++k) res.q_corr[k] = s_pose[kGaQd + k];
#pragma unroll
  for (int k = 0; k < 3; ++k) res.t_corr[k] = s_pose[kGaTd + k];
  if (with_map) {
    const GmRequestOut q0 = a.req[it.gm];
    const int seg_end = a.req[it.gm + 1].seg_first;
    res.raw_points[0] = q0.raw[0]; res.raw_points[1] = q0.raw[1];
    int out0 = 0, out1 = 0;
    ga_totals(a, q0.seg_first, q0.surf_first, cx, cy, cz, s_scan, &res.points[0], &res.cubes[0], &out0);
    ga_totals(a, q0.surf_first, seg_end, cx, cy, cz, s_scan, &res.points[1], &res.cubes[1], &out1);
    res.outside_window = out0 + out1;
    if (res.points[0] > a.pool_cap || res.points[1] > a.pool_cap) {          // does not fit its pool row: the sequence stays as it is
      if (tid == 0) { res.status = ALOAM_GRAPH_APPLY_NO_ROOM; a.dst[i] = res; }
      return;
    }
    for (int cls = 0; cls < 2; ++cls) {
      const int lo = cls ? q0.surf_first : q0.seg_first, hi = cls ? seg_end : q0.surf_first;
      for (int c = tid; c < kMapCubes; c += 1024) { s_pref[c] = 0; s_first[c] = 0; }
      __syncthreads();
      const long long base = lo < hi ? a.jobs[lo].first : 0;                 // a class's segments follow each other in `grouped`
      for (int s = lo + tid; s < hi; s += 1024) {
        const int w = ga_window_index(a.seg[s].cube_key, cx, cy, cz);
        if (w >= 0) { s_pref[w] = a.counts[s]; s_first[w] = (int)(a.jobs[s].first - base); }
      }
      __syncthreads();
      int sum = 0;
      for (int k = 0; k < kGaPer; ++k) { const int c = tid * kGaPer + k; if (c < kMapCubes) sum += s_pref[c]; }
      int t = 0;
      int run = block_exclusive_scan<int, 1024>(sum, s_scan, &t);
      CubeDesc* T = a.cubes + ((long long)it.seq * 2 + cls) * kMapCubes;
      for (int k = 0; k < kGaPer; ++k) {
        const int c = tid * kGaPer + k;
        if (c < kMapCubes) {
          const int n = s_pref[c];
          T[c] = CubeDesc{n ? run : 0, n, n, 0};                             // packed back to back from the start of the pool row, as aloam_set_map writes them
          s_pref[c] = run;
          run += n;
        }
      }
      if (tid == 0) s_pref[kMapCubes] = t;
      __syncthreads();
      float4* dst = (cls ? a.pool[1] : a.pool[0]) + (long long)it.seq * a.pool_cap;
      const float4* src = a.grouped + base;
      auto fetch = [&](int p) { const int c = last_le(s_pref, 0, kMapCubes, p); return src[s_first[c] + (p - s_pref[c])]; };
      int p0 = 0;
      for (; p0 + 4 * 1024 <= t; p0 += 4 * 1024) {                           // four loads of a thread in flight before its stores (named registers)
        const int p = p0 + tid;
        const float4 v0 = fetch(p), v1 = fetch(p + 1024), v2 = fetch(p + 2048), v3 = fetch(p + 3072);
        dst[p] = v0; dst[p + 1024] = v1; dst[p + 2048] = v2; dst[p + 3072] = v3;
      }
      for (int p = p0 + tid; p < t; p += 1024) dst[p] = fetch(p);
      __syncthreads();                                                       // s_pref / s_first are rewritten by the next class
    }
  }
  if (tid == 0) {                                                            // MapSeq last, behind the barriers above
    if (with_map) { ms.cen[0] = cx; ms.cen[1] = cy; ms.cen[2] = cz; ms.pool_used[0] = res.points[0]; ms.pool_used[1] = res.points[1]; }
#pragma unroll
    for (int k = 0; k < 4; ++k) { ms.q_wmap_wodom[k] = s_pose[kGaQm + k]; ms.par[k] = s_pose[kGaPar + k]; }
#pragma unroll
    for (int k = 0; k < 3; ++k) { ms.t_wmap_wodom[k] = s_pose[kGaTm + k]; ms.par[4 + k] = s_pose[kGaPar + 4 + k]; }
  }
  // the rebase: the live frame is the optimised one from here on, so the entered poses become the estimates (bit copies)
  for (int k = tid; k < it.nodes; k += 1024) {
    aloam_graph_node& x = N[k];
    const double q0 = x.q_opt[0], q1 = x.q_opt[1], q2 = x.q_opt[2], q3 = x.q_opt[3], t0 = x.t_opt[0], t1 = x.t_opt[1], t2 = x.t_opt[2];
    x.q[0] = q0; x.q[1] = q1; x.q[2] = q2; x.q[3] = q3; x.t[0] = t0; x.t[1] = t1; x.t[2] = t2;
  }
  if (tid == 0) { res.status = ALOAM_GRAPH_APPLIED; a.dst[i] = res; }
}

void launch_graph_apply(const GraphApplyArgs& a, hipStream_t s) {
  if (a.n > 0) hipLaunchKernelGGL(k_graph_apply, dim3(a.n), dim3(1024), 0, s, a);
}

}  // namespace aloam
