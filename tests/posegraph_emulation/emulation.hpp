// tests/posegraph_emulation/emulation.hpp - what posegraph_kernels.hip needs from HIP and from lm_device.hpp, restated for a host build:
// one std::thread per GPU thread of a workgroup, __syncthreads as a std::barrier, the wave shuffle through a shared array, block_sum in
// the order of lm_device.hpp.  Workgroups run one after the other.  The kernel text itself is compiled unchanged (test_posegraph_emulation.py).
// Coupled by hand to the device headers: block_sum and shfl_down_f64 restate lm_device.hpp, quat_rotate restates aloam_device.hpp, and
// OdomState / MapSeq hold only the members k_graph_add_nodes reads (odometry_kernels.hpp, mapping_kernels.hpp).  A change to one of those
// is restated here; test_posegraph_emulation.py replaces the kernel unit's #include lines by name and fails loudly when they change.
#pragma once
#include <algorithm>
#include <barrier>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>
#define __device__
#define __global__
#define __forceinline__ inline
#define __noinline__
#define __shared__ static
#define __launch_bounds__(...)
struct Idx { int x; };
static thread_local Idx threadIdx, blockIdx;
static std::barrier<>* g_bar;
inline void __syncthreads() { g_bar->arrive_and_wait(); }
inline int atomicAdd(int* p, int v) { return __atomic_fetch_add(p, v, __ATOMIC_SEQ_CST); }
using std::min; using std::max; using std::isfinite;
typedef void* hipStream_t;
struct dim3 { int x; dim3(int x_) : x(x_) {} };
template <class F> void emu_launch(F f, int grid, int block) {
  for (int b = 0; b < grid; ++b) {
    std::barrier<> bar(block); g_bar = &bar;
    std::vector<std::thread> th;
    for (int t = 0; t < block; ++t) th.emplace_back([&, t, b]() { threadIdx.x = t; blockIdx.x = b; f(); });
    for (auto& x : th) x.join();
  }
}
#define hipLaunchKernelGGL(k, grid, block, shm, stream, ...) emu_launch([&]() { k(__VA_ARGS__); }, (grid).x, (block).x)
#include "aloam_mi355x.h"
namespace aloam {
struct OdomState { double q_w[4], t_w[3]; };
struct MapSeq { double par[7]; int frame_count; };
static double g_x[256];
inline double shfl_down_f64(double v, int d) {
  const int t = threadIdx.x; g_x[t] = v; __syncthreads();
  const double r = ((t & 63) + d < 64) ? g_x[t + d] : v; __syncthreads(); return r;
}
inline void quat_rotate(const double q[4], double vx, double vy, double vz, double out[3]) {
  double ux = q[1] * vz - q[2] * vy, uy = q[2] * vx - q[0] * vz, uz = q[0] * vy - q[1] * vx;
  ux += ux; uy += uy; uz += uz;
  out[0] = vx + q[3] * ux + (q[1] * uz - q[2] * uy);
  out[1] = vy + q[3] * uy + (q[2] * ux - q[0] * uz);
  out[2] = vz + q[3] * uz + (q[0] * uy - q[1] * ux);
}
template <int NV, int NW = 4> inline void block_sum(double* v, double* s_red) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int k = 0; k < NV; ++k) { double x = v[k]; for (int d = 32; d > 0; d >>= 1) x += shfl_down_f64(x, d); if (lane == 0) s_red[wave * NV + k] = x; }
  __syncthreads();
  for (int k = 0; k < NV; ++k) v[k] = (s_red[k] + s_red[NV + k]) + (s_red[2 * NV + k] + s_red[3 * NV + k]);
  __syncthreads();
}
}
