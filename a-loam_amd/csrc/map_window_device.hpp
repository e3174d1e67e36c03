// a-loam_amd/csrc/map_window_device.hpp — device functions of the 21 x 21 x 11 cube window (reference src/laserMapping.cpp:72-80,
// :311-321) and of the routing of voxel-filter segments, shared by the mapping step (mapping_kernels.hip) and the capture of the cubes
// that leave the window (atlas_kernels.hip).  One definition, so that both find the same cube for the same coordinate.
#pragma once
#include "lm_device.hpp"
#include "mapping_kernels.hpp"

namespace aloam {

namespace {

// int((v + 25.0) / 50.0) + cen, minus one when v + 25 < 0  (:312-321, :741-750)
__device__ __forceinline__ int cube_coord(double v, int cen) {
  int c = (int)((v + 25.0) / 50.0) + cen;
  if (v + 25.0 < 0) c--;
  return c;
}

__device__ __forceinline__ CubeDesc* cube_table(const MapArgs& a, int b, int cls) { return a.cubes + ((long long)b * 2 + cls) * kMapCubes; }

// Which filter takes a segment: the single-workgroup LDS filter (k_vox_lds; list 2: <= kVoxTinyN points, one wave; list 0: <= kVoxSmallN
// points, 256 threads; list 1: up to kVoxBigN points, 1024 threads) or, for anything larger, the general tile-sort / rank-merge path
// through global memory.
__device__ __forceinline__ void vox_enlist(const VoxArgs& v, int seg, int n) {
  if (n <= 0) return;
  if (n <= kVoxTinyN) v.lists[2 * (long long)v.n_segs + atomicAdd(&v.counters[7], 1)] = seg;
  else if (n <= kVoxSmallN) v.lists[atomicAdd(&v.counters[5], 1)] = seg;
  else if (n <= kVoxBigN) v.lists[v.n_segs + atomicAdd(&v.counters[6], 1)] = seg;
  else atomicAdd(&v.counters[4], 1);
}

// How far k_map_begin will move the window of this sequence in the step that is about to run: the start of k_map_begin with the same device
// functions in the same order - transformAssociateToMap's translation (:142-146), the centre cube (:311-321) - and the shift loop of
// :323-507 on the three centre indices alone, with k_map_begin's guard of 64 shifts per axis.  One lane calls it.
__device__ __forceinline__ void window_shift(const MapSeq& ms, const OdomState& od, int s[3]) {
  double qm[4], to[3], rt[3];
  for (int k = 0; k < 4; ++k) qm[k] = ms.q_wmap_wodom[k];
  for (int k = 0; k < 3; ++k) to[k] = od.t_w[k];
  quat_rotate(qm, to[0], to[1], to[2], rt);
  const int dim[3] = {kMapW, kMapH, kMapD};
  for (int k = 0; k < 3; ++k) {
    const double t = rt[k] + ms.t_wmap_wodom[k];
    int c = cube_coord(t, ms.cen[k]), d = 0;
    for (int guard = 0; guard < 64; ++guard) {
      const int dir = c < 3 ? 1 : (c >= dim[k] - 3 ? -1 : 0);
      if (dir == 0) break;
      c += dir; d += dir;
    }
    s[k] = d;
  }
}

}  // namespace

}  // namespace aloam
