// a-loam_amd/csrc/loopreg_kernels.hip — gfx950 kernels of the batched keyframe registration (aloam_graph_register_loops).
// A translation unit of its own, so that the mapping, information and graph-map kernels are compiled exactly as before; it shares their
// device functions through map_search_device.hpp / map_window_device.hpp / information_device.hpp.
//   k_loop_gather   (16, slot, class) workgroups: the clouds of the target nodes moved into the frame of node i (T_k = X_i^-1 o X_k, once per
//                   node and workgroup, by one lane, f64, separately rounded), the source cloud copied into the slot's stack row, and - by
//                   one lane per (slot, class) - the segment of the voxel filter and the slot's scratch MapSeq, from the device-side counts
//   k_loop_grid     one 1024-thread workgroup per (slot, class): the 2 m-cell hash grid (map_bucket) over the FILTERED target by an LDS
//                   counting sort (count -> scan -> fill, as k_mapgrid_build); an entry's .w is the point's index in the filtered target,
//                   which is what k_map_search ranks by; the gate of src/laserMapping.cpp:554 is decided here
//   k_loop_result   one thread per request: status, Z, counts, cost, the left-tangent information and its rotation into the edge's tangent
// Between them run the voxel filter, k_map_search / k_map_fit / k_map_solve and k_pose_information_map of the mapping step, unchanged, over a
// MapArgs whose sequences are the slots.  No floating-point atomics; the integer LDS atomics of the grid build decide only the order of the
// entries inside a bucket, which the search does not depend on.  Every store to global memory is a vector store (points as 16 bytes; the
// descriptors, the scratch MapSeq and the result field by field from one lane).
#include "loopreg_kernels.hpp"

#include "export_kernels.hpp"                // copy_points only
#include "information_device.hpp"
#include "map_search_device.hpp"
#include "map_window_device.hpp"

namespace aloam {

namespace {

// What a request covers, from the descriptors as they are at this point of the stream (uniform in the workgroup).  A sequence's clouds sit
// back to back in its class rows (graphmap_kernels.hpp), so the target of a class is ONE range of the row, nodes kept without clouds included.
struct LoopPlan {
  int status;                      // ALOAM_LOOP_OK, or what is known before any point is touched: NO_CLOUDS, TOO_LARGE
  int base[2], raw[2];             // the target range of every class row
  int src[2], src_n[2];            // node j's clouds
};

__device__ __forceinline__ LoopPlan loop_plan(const LoopArgs& a, const aloam_graph_loop_request& rq) {
  const KfDesc* D = a.kf.desc + (long long)rq.seq * a.kf.max_nodes;
  const KfDesc d0 = D[rq.first], d1 = D[rq.first + rq.count - 1], dj = D[rq.j];
  LoopPlan p;
  p.base[0] = d0.first[0]; p.base[1] = d0.first[1];
  p.raw[0] = d1.first[0] + d1.count[0] - d0.first[0]; p.raw[1] = d1.first[1] + d1.count[1] - d0.first[1];
  p.src[0] = dj.first[0]; p.src[1] = dj.first[1];
  p.src_n[0] = dj.count[0]; p.src_n[1] = dj.count[1];
  p.status = ALOAM_LOOP_OK;
  // (a source larger than a stack row cannot come out of aloam_graph_add_nodes, which copied it from one; refused all the same)
  if (p.raw[0] > a.raw_cap[0] || p.raw[1] > a.raw_cap[1] || p.src_n[0] > a.map.R * kLessSharpPerRing || p.src_n[1] > a.map.cap) p.status = ALOAM_LOOP_TOO_LARGE;
  if (p.src_n[0] + p.src_n[1] <= 0 || p.raw[0] + p.raw[1] <= 0 || p.raw[0] < 0 || p.raw[1] < 0) p.status = ALOAM_LOOP_NO_CLOUDS;
  return p;
}

__device__ __forceinline__ long long stack_row(const MapArgs& m, int cls) { return cls ? (long long)m.cap : (long long)m.R * kLessSharpPerRing; }

}  // namespace

__global__ __launch_bounds__(256) void k_loop_gather(LoopArgs a, VoxArgs v) {
  const int s = blockIdx.y, cls = blockIdx.z, tid = threadIdx.x;
  const aloam_graph_loop_request rq = a.req[s];
  const LoopPlan pl = loop_plan(a, rq);
  const bool ok = pl.status == ALOAM_LOOP_OK;
  float4* raw = (cls ? a.raw[1] + (long long)s * a.raw_cap[1] : a.raw[0] + (long long)s * a.raw_cap[0]);
  MapSeq& ms = a.map.seq[s];
  if (blockIdx.x == 0 && tid == 0) {
    // the segment of this (slot, class): one pcl::VoxelGrid over the whole target cloud of the class, its size into from_total
    VoxSeg sg{};
    sg.in = raw;
    sg.out = (cls ? a.target[1] + (long long)s * a.raw_cap[1] : a.target[0] + (long long)s * a.raw_cap[0]);
    sg.out_count = cls ? &ms.from_total[1] : &ms.from_total[0];
    sg.n = ok ? (cls ? pl.raw[1] : pl.raw[0]) : 0;
    sg.leaf = cls ? a.map.plane_res : a.map.line_res;
    v.segs[2 * s + cls] = sg;
    vox_enlist(v, 2 * s + cls, sg.n);
    if (cls == 0) {
      // the scratch MapSeq: `parameters` = the guess, the stacks = node j's clouds; everything else as a new sequence has it
      static_assert(sizeof(MapSeq) % sizeof(double) == 0 && alignof(MapSeq) >= alignof(double), "the scratch MapSeq is zeroed as doubles");
      double* w = reinterpret_cast<double*>(&ms);
      for (int k = 0; k < (int)(sizeof(MapSeq) / sizeof(double)); ++k) w[k] = 0.0;
      for (int k = 0; k < 4; ++k) ms.par[k] = rq.q[k];
      for (int k = 0; k < 3; ++k) ms.par[4 + k] = rq.t[k];
      ms.q_wmap_wodom[3] = 1.0; ms.q_wodom[3] = 1.0;
      ms.n_stack[0] = ok ? pl.src_n[0] : 0; ms.n_stack[1] = ok ? pl.src_n[1] : 0;
      int* P = a.plan + (long long)s * kLoopPlanInts;
      P[0] = pl.status; P[1] = pl.raw[0]; P[2] = pl.raw[1]; P[3] = pl.src_n[0]; P[4] = pl.src_n[1]; P[5] = 0; P[6] = 0; P[7] = 0;
    }
  }
  if (!ok) return;                                                             // (uniform)
  // ---- the target: node after node, T_k once per node
  __shared__ double s_par[8];
  const KfDesc* D = a.kf.desc + (long long)rq.seq * a.kf.max_nodes;
  const aloam_graph_node* N = a.nodes + (long long)rq.seq * a.max_nodes;
  const float4* row = cls ? a.kf.points[1] + (long long)rq.seq * a.kf.cap[1] : a.kf.points[0] + (long long)rq.seq * a.kf.cap[0];
  const int base = cls ? pl.base[1] : pl.base[0];
  for (int k = rq.first + (int)blockIdx.x; k < rq.first + rq.count; k += (int)gridDim.x) {
    const KfDesc d = D[k];
    const int at = cls ? d.first[1] : d.first[0], cnt = cls ? d.count[1] : d.count[0];
    if (cnt <= 0 || at < base || at - base + cnt > (cls ? pl.raw[1] : pl.raw[0])) continue;   // (uniform; the second: never, while the row is back to back)
    __syncthreads();                                                           // s_par of the node before has been read
    if (tid == 0) {
      // T_k = X_i^-1 o X_k as the header defines a relative pose: q_d = q_i* q_k, t_d = q_i* (t_k - t_i); node i like every other node
      const aloam_graph_node& xi = N[rq.i];
      const aloam_graph_node& xk = N[k];
      double qi[4], qk[4], ti[3], tk[3], qd[4], td[3];
      for (int c = 0; c < 4; ++c) { qi[c] = rq.pose ? xi.q_opt[c] : xi.q[c]; qk[c] = rq.pose ? xk.q_opt[c] : xk.q[c]; }
      for (int c = 0; c < 3; ++c) { ti[c] = rq.pose ? xi.t_opt[c] : xi.t[c]; tk[c] = rq.pose ? xk.t_opt[c] : xk.t[c]; }
      const double qc[4] = {-qi[0], -qi[1], -qi[2], qi[3]};
      quat_mul(qc, qk, qd);
      quat_rotate(qc, tk[0] - ti[0], tk[1] - ti[1], tk[2] - ti[2], td);
      for (int c = 0; c < 4; ++c) s_par[c] = qd[c];
      for (int c = 0; c < 3; ++c) s_par[4 + c] = td[c];
    }
    __syncthreads();
    double par[7];
#pragma unroll
    for (int c = 0; c < 7; ++c) par[c] = s_par[c];
    const float4* src = row + at;
    float4* dst = raw + (at - base);
    constexpr int U = 4;                                                       // 16-byte loads in flight per lane before the f64 work
    for (int p0 = 0; p0 < cnt; p0 += U * 256) {
      float4 pt[U];
#pragma unroll
      for (int u = 0; u < U; ++u) { const int p = p0 + u * 256 + tid; pt[u] = src[p < cnt ? p : cnt - 1]; }
#pragma unroll
      for (int u = 0; u < U; ++u) { const int p = p0 + u * 256 + tid; if (p < cnt) dst[p] = associate_to_map(pt[u], par); }
    }
  }
  // ---- the source: node j's cloud as stored, into the slot's stack row (chunks of 2048 points dealt over the workgroups)
  {
    const int n = cls ? pl.src_n[1] : pl.src_n[0];
    const float4* src = row + (cls ? pl.src[1] : pl.src[0]);
    float4* dst = (cls ? a.map.stack[1] : a.map.stack[0]) + (long long)s * stack_row(a.map, cls);
    for (int q = (int)blockIdx.x * 2048; q < n; q += (int)gridDim.x * 2048) copy_points(dst + q, src + q, min(2048, n - q));
  }
}

// The kd-tree stand-in over the filtered target (the submap of k_mapgrid_build is a list of cubes of a pool; this one is one array).
__global__ __launch_bounds__(1024) void k_loop_grid(LoopArgs a) {
  const int s = blockIdx.x, cls = blockIdx.y, tid = threadIdx.x;
  MapSeq& ms = a.map.seq[s];
  const int H = a.map.grid_H;
  const bool gate = a.plan[(long long)s * kLoopPlanInts] == ALOAM_LOOP_OK && ms.from_total[0] > 10 && ms.from_total[1] > 50;   // (:554)
  if (cls == 0 && tid == 0) ms.gate = gate ? 1 : 0;
  if (!gate) return;                                                           // nothing will search this slot
  const int n = cls ? ms.from_total[1] : ms.from_total[0];
  extern __shared__ __attribute__((aligned(16))) int lg_lds[];
  int* cnt = lg_lds;                       // [H]
  int* part = cnt + H;                     // [1024]
  int* start = a.map.grid_start[cls] + (long long)s * (H + 1);
  float4* sorted = a.map.grid_sorted[cls] + (long long)s * a.map.pool_cap;
  const float4* pts = cls ? a.target[1] + (long long)s * a.raw_cap[1] : a.target[0] + (long long)s * a.raw_cap[0];
  for (int h = tid; h < H; h += 1024) cnt[h] = 0;
  __syncthreads();
  constexpr int U = 4;
  auto bucket = [&](const float4& p) { return (int)map_bucket((int)floorf(p.x * kMapCellInv), (int)floorf(p.y * kMapCellInv), (int)floorf(p.z * kMapCellInv), H); };
  for (int base = 0; base < n; base += U * 1024) {
    float4 p[U];
#pragma unroll
    for (int u = 0; u < U; ++u) { const int g = base + u * 1024 + tid; p[u] = pts[g < n ? g : n - 1]; }
#pragma unroll
    for (int u = 0; u < U; ++u) if (base + u * 1024 + tid < n) atomicAdd(&cnt[bucket(p[u])], 1);
  }
  __syncthreads();
  const int per = H / 1024;
  int local = 0;
  for (int k = 0; k < per; ++k) local += cnt[tid * per + k];
  int total;
  int run = block_exclusive_scan<int, 1024>(local, part, &total);
  for (int k = 0; k < per; ++k) { const int c = cnt[tid * per + k]; cnt[tid * per + k] = run; start[tid * per + k] = run; run += c; }
  if (tid == 1023) start[H] = run;
  __syncthreads();
  for (int base = 0; base < n; base += U * 1024) {
    float4 p[U];
#pragma unroll
    for (int u = 0; u < U; ++u) { const int g = base + u * 1024 + tid; p[u] = pts[g < n ? g : n - 1]; }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int g = base + u * 1024 + tid;
      if (g < n) { const int pos = atomicAdd(&cnt[bucket(p[u])], 1); sorted[pos] = make_float4(p[u].x, p[u].y, p[u].z, __int_as_float(g)); }
    }
  }
}

// One thread per request, f64, every loop with compile-time bounds (the matrices live in registers).
__global__ __launch_bounds__(64) void k_loop_result(LoopArgs a, int last) {
  const int r = blockIdx.x * 64 + threadIdx.x;
  if (r >= a.n) return;
  const aloam_graph_loop_request& rq = a.req[r];
  const MapSeq& ms = a.map.seq[r];
  const aloam_pose_information& pi = a.info[r];
  const int* P = a.plan + (long long)r * kLoopPlanInts;
  aloam_graph_loop_result* out = a.dst + r;
  int status = P[0];
  if (status == ALOAM_LOOP_OK && !ms.gate) status = ALOAM_LOOP_TARGET_TOO_SMALL;
  const bool solved = status == ALOAM_LOOP_OK;
  double H[6][6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
#pragma unroll
    for (int j = 0; j < 6; ++j) H[i][j] = solved ? pi.info[i * 6 + j] : 0.0;
  }
  if (solved) {
    // positive definite: a Cholesky factorisation succeeds, every pivot above kInfoPivotTol of its diagonal entry
    bool pd = pi.status == ALOAM_INFO_OK || pi.status == ALOAM_INFO_SINGULAR;
    double L[6][6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
#pragma unroll
      for (int j = 0; j <= i; ++j) {
        double sum = H[i][j];
#pragma unroll
        for (int k = 0; k < j; ++k) sum -= L[i][k] * L[j][k];
        if (i == j) { if (!(sum > kInfoPivotTol * H[i][i])) pd = false; L[i][i] = sqrt(pd ? sum : 1.0); }
        else L[i][j] = sum / L[j][j];
      }
    }
    if ((last ? ms.lm_termination[1] : ms.lm_termination[0]) == 5 || !pd) status = ALOAM_LOOP_SOLVE_FAILED;
  }
  const bool good = status == ALOAM_LOOP_OK;
  out->status = status;
  out->n_line = solved ? pi.n_line : 0; out->n_plane = solved ? pi.n_plane : 0;
  out->lm_iterations = solved ? (last ? ms.lm_iterations[1] : ms.lm_iterations[0]) : 0;
  out->lm_termination = solved ? (last ? ms.lm_termination[1] : ms.lm_termination[0]) : 0;
  out->pad = 0;
  out->target_points[0] = ms.from_total[0]; out->target_points[1] = ms.from_total[1];
  out->target_raw[0] = P[1]; out->target_raw[1] = P[2];
  out->source_points[0] = P[3]; out->source_points[1] = P[4];
  out->cost = solved ? pi.cost : 0.0;
  double q[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) { q[k] = good ? ms.par[k] : rq.q[k]; out->q[k] = q[k]; }
#pragma unroll
  for (int k = 0; k < 3; ++k) out->t[k] = good ? ms.par[4 + k] : rq.t[k];
  // The graph's residual perturbs Z on the right (q_Z exp(phi / 2), t_Z + R_Z tau), the registration's tangent is left (exp(theta / 2) q,
  // t + dt): theta = R_Z phi, dt = R_Z tau, so info = T^T info_left T with T = blockdiag(R_Z, R_Z).  R_Z column by column as quat_rotate
  // gives it; M = info_left T, then T^T M, each sum in index order.
  double R[3][3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    double col[3];
    quat_rotate(q, c == 0 ? 1.0 : 0.0, c == 1 ? 1.0 : 0.0, c == 2 ? 1.0 : 0.0, col);
    R[0][c] = col[0]; R[1][c] = col[1]; R[2][c] = col[2];
  }
  double M[6][6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
#pragma unroll
    for (int bl = 0; bl < 2; ++bl) {
#pragma unroll
      for (int c = 0; c < 3; ++c) M[i][3 * bl + c] = (H[i][3 * bl] * R[0][c] + H[i][3 * bl + 1] * R[1][c]) + H[i][3 * bl + 2] * R[2][c];
    }
  }
  int o = 0;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
#pragma unroll
    for (int j = i; j < 6; ++j) {
      const int bi = i / 3, ci = i % 3;
      const double e = (R[0][ci] * M[3 * bi][j] + R[1][ci] * M[3 * bi + 1][j]) + R[2][ci] * M[3 * bi + 2][j];
      out->info[o] = good ? e : 0.0;
      out->info_left[o] = good ? H[i][j] : 0.0;
      ++o;
    }
  }
}

// aloam_graph_loop_export_target: the count always, the points when they fit the cap.
__global__ __launch_bounds__(256) void k_loop_export_target(const MapSeq* ms, int cls, const float4* src, float4* dst, long long cap, int* count) {
  const int n = cls ? ms->from_total[1] : ms->from_total[0];
  if (blockIdx.x == 0 && threadIdx.x == 0) *count = n;
  if (!dst || n > cap) return;
  for (int q = (int)blockIdx.x * 2048; q < n; q += (int)gridDim.x * 2048) copy_points(dst + q, src + q, min(2048, n - q));
}
void launch_loop_export_target(const MapSeq* ms, int cls, const float4* src, float4* dst, long long cap, int* count, hipStream_t s) {
  hipLaunchKernelGGL(k_loop_export_target, dim3(64), dim3(256), 0, s, ms, cls, src, dst, cap, count);
}

void launch_loop_gather(const LoopArgs& a, const VoxArgs& v, hipStream_t s) {
  if (a.n > 0) hipLaunchKernelGGL(k_loop_gather, dim3(kLoopGatherBlocks, a.n, 2), dim3(256), 0, s, a, v);
}
static size_t loop_grid_lds_bytes(int H) { return sizeof(int) * ((size_t)H + 1024); }
static_assert(sizeof(int) * ((size_t)kMapGridMaxH + 1024) <= 163840, "the bucket table of k_loop_grid must fit one CU's LDS");
int prepare_loop_grid(int H) {
  if (H > kMapGridMaxH || H < 1024 || (H & (H - 1))) return -1;
  return hipFuncSetAttribute((const void*)k_loop_grid, hipFuncAttributeMaxDynamicSharedMemorySize, (int)loop_grid_lds_bytes(H)) == hipSuccess ? 0 : -1;
}
void launch_loop_grid(const LoopArgs& a, hipStream_t s) {
  if (a.n > 0) hipLaunchKernelGGL(k_loop_grid, dim3(a.n, 2), dim3(1024), loop_grid_lds_bytes(a.map.grid_H), s, a);
}
void launch_loop_result(const LoopArgs& a, hipStream_t s) {
  if (a.n > 0) hipLaunchKernelGGL(k_loop_result, dim3((a.n + 63) / 64), dim3(64), 0, s, a, (a.outer_iterations - 1) & 1);
}

}  // namespace aloam
