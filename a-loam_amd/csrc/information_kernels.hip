// a-loam_amd/csrc/information_kernels.hip — gfx950 kernels of aloam_export_pose_information: the information matrix of the last odometry /
// mapping solve of each listed sequence.  A translation unit of its own, so that the solver kernels are compiled exactly as before: they
// share the evaluation functions through odometry_solve_device.hpp / mapping_solve_device.hpp, not a caller.
#include "information_device.hpp"
#include "mapping_solve_device.hpp"
#include "odometry_kernels.hpp"
#include "odometry_solve_device.hpp"

namespace aloam {

// aloam_export_pose_information(ALOAM_INFO_ODOMETRY): one workgroup per listed sequence evaluates the records of the last outer iteration once
// more, at the pose k_solve left in para_q / para_t, exactly as the solver's own evaluation does (same device function, same thread count, same
// reduction), and thread 0 turns the sums into the public record (information_device.hpp).  What is written for a sequence depends on that
// sequence alone.
template <bool DISTORT>
__global__ __launch_bounds__(kSolveThreads) void k_pose_information_odom(OdomArgs a, const int* __restrict__ list, aloam_pose_information* __restrict__ dst) {
  __shared__ double s_red[kSolveWaves * 28];
  const int code = list[blockIdx.x], b = code & kInfoSeqMask;
  const bool solved = (code & kInfoSolvedBit) != 0;
  double acc[28];
  for (int k = 0; k < 28; ++k) acc[k] = 0.0;
  int ne = 0, np = 0;
  if (solved) {
    const OdomState& st = a.state[b];
    double q[4] = {st.para_q[0], st.para_q[1], st.para_q[2], st.para_q[3]}, t[3] = {st.para_t[0], st.para_t[1], st.para_t[2]};
    if (DISTORT) {
      // With distortion the evaluation derives some sixty values from the pose alone; as wave-uniform values they overflow the scalar file
      // (nine spilled scalars).  Pinned to vector registers (an empty statement, no instruction), the pose and what follows from it stay there.
#pragma unroll
      for (int k = 0; k < 4; ++k) asm volatile("" : "+v"(q[k]));
#pragma unroll
      for (int k = 0; k < 3; ++k) asm volatile("" : "+v"(t[k]));
    }
    // one record fetched ahead without distortion; with it the registers of a second record would pass the budget (tests/test_information_budgets.py)
    evaluate<true, DISTORT, 0, DISTORT ? 0 : 1>(a, b, q, t, acc, &ne, &np);
  }
  double cnt[2] = {(double)ne, (double)np};
  block_sum<28, kSolveWaves>(acc, s_red);
  block_sum<2, kSolveWaves>(cnt, s_red);
  if (threadIdx.x == 0) write_pose_information(dst + blockIdx.x, solved, acc, (int)cnt[0], (int)cnt[1], -1);
}

// aloam_export_pose_information(ALOAM_INFO_MAPPING): one workgroup per listed sequence evaluates the records of the second iteration once more,
// at the pose k_map_solve left in MapSeq::par, through the same tile prefixes, device function and reduction, and thread 0 turns the sums into
// the public record (information_device.hpp).  A step whose gate was false left no record: the prefixes are all zero.
__global__ __launch_bounds__(kMapSolveThreads) void k_pose_information_map(MapArgs a, const int* __restrict__ list, aloam_pose_information* __restrict__ dst) {
  __shared__ double s_red[(kMapSolveThreads / 64) * 28];
  extern __shared__ int s_pref[];
  const int code = list[blockIdx.x], b = code & kInfoSeqMask, tid = threadIdx.x;
  const bool solved = (code & kInfoSolvedBit) != 0;
  const MapSeq& ms = a.seq[b];
  double acc[28];
  for (int k = 0; k < 28; ++k) acc[k] = 0.0;
  int ne = 0, np = 0;
  if (solved) {
    const int nt0 = (ms.n_stack[0] + 255) >> 8, nt1 = (ms.n_stack[1] + 255) >> 8;
    const int* tc = a.rec_tiles + (long long)b * a.rec_tiles_per_seq;
    if (tid == 0) {
      int run = 0;
      for (int k = 0; k < nt0; ++k) { s_pref[k] = run; run += ms.gate ? tc[k] : 0; }
      s_pref[nt0] = run;
      run = 0;
      for (int k = 0; k < nt1; ++k) { s_pref[nt0 + 1 + k] = run; run += ms.gate ? tc[a.rec_tiles_corner + k] : 0; }
      s_pref[nt0 + 1 + nt1] = run;
    }
    __syncthreads();
    const double q[4] = {ms.par[0], ms.par[1], ms.par[2], ms.par[3]}, t[3] = {ms.par[4], ms.par[5], ms.par[6]};
    map_evaluate<true>(a, b, s_pref, q, t, acc, &ne, &np);
  }
  double cnt[2] = {(double)ne, (double)np};
  block_sum<28, kMapSolveThreads / 64>(acc, s_red);
  block_sum<2, kMapSolveThreads / 64>(cnt, s_red);
  if (tid == 0) write_pose_information(dst + blockIdx.x, solved, acc, (int)cnt[0], (int)cnt[1], ms.frame_count);
}

void launch_pose_information_odom(const OdomArgs& a, const int* list, int n, aloam_pose_information* dst, hipStream_t s) {
  if (n <= 0) return;
  if (a.distortion) hipLaunchKernelGGL(k_pose_information_odom<true>, dim3(n), dim3(kSolveThreads), 0, s, a, list, dst);
  else hipLaunchKernelGGL(k_pose_information_odom<false>, dim3(n), dim3(kSolveThreads), 0, s, a, list, dst);
}

void launch_pose_information_map(const MapArgs& a, const int* list, int n, aloam_pose_information* dst, hipStream_t s) {
  if (n > 0) hipLaunchKernelGGL(k_pose_information_map, dim3(n), dim3(kMapSolveThreads), sizeof(int) * (size_t)(a.rec_tiles_per_seq + 2), s, a, list, dst);
}

}  // namespace aloam
