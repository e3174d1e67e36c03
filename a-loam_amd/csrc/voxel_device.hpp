// a-loam_amd/csrc/voxel_device.hpp — the cell arithmetic of pcl::VoxelGrid<PointXYZI>::applyFilter (PCL 1.8, pcl/filters/impl/voxel_grid.hpp),
// stated ONCE for the four filters of this project and compiled for the device AND for the host:
//   k_vox_keys_sort / k_vox_emit (general path), k_vox_lds (one workgroup per segment)      mapping_kernels.hip
//   k_ring_features / voxel_runs_tail (less-flat points of one ring, float and packed-cell path)   registration_kernels.hip
//   voxel_grid_reference_order (the filter as PCL has it, sort replayed)                    reference_order_kernels.hip
// Every function is a fixed sequence of individually rounded f32 / integer operations (-ffp-contract=off on both sides), so the device and the
// host program that pins this file against the PCL stand-in of the CPU checker (tests/host/test_voxel_port.cpp: bit for bit, count and every float)
// compute the same bits.  No LDS, no barriers, no wave operations: how a kernel finds the box and in which order it adds the members of a cell is the
// kernel's own; what a box, an index and a centroid ARE is here.  PCL's source is quoted by statement (the file is not vendored).
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define ALOAM_VOX_HD __device__ __forceinline__
#define ALOAM_VOX_HD_MEMBER __device__ __forceinline__
#else
#define ALOAM_VOX_HD static inline
#define ALOAM_VOX_HD_MEMBER inline
#endif

namespace aloam {
namespace voxel {

constexpr long long kMaxCells = 2147483647ll;   // std::numeric_limits<int32_t>::max(): a box of more cells is not filtered
// floor(p * inv) is an integer-valued f32; below 2^23 in magnitude so is its difference to (float)min_b, exactly.  Then equal floor triples <=> equal cell
// index inside one box, which is what lets a filter find run heads before it knows the box (cell_differs).
constexpr float kExactCellLimit = 8388608.f;

// `inverse_leaf_size_ = Eigen::Array4f::Ones () / leaf_size_.array ()` (setLeafSize): a division, once per call.
ALOAM_VOX_HD float inverse_leaf(float leaf) { return 1.0f / leaf; }
// `floor (input_->points[*it].x * inverse_leaf_size_[0])`: the cell coordinate of one axis, before any box is known
ALOAM_VOX_HD float cell_coord(float v, float inv) { return floorf(v * inv); }

// ---- the box of a filter call ------------------------------------------------------------------------------------------------------------
struct Box {
  bool unfiltered;   // applyFilter "returns its input unfiltered": `output = *input_; return;`
  float fminb[3];    // static_cast<float> (min_b_[k]), the float the index subtracts
  int divb[3];       // div_b_
};
// mn / mx: getMinMax3D's f32 minimum and maximum of the input, per axis.
//   `int64_t dx = static_cast<int64_t>((max_p[0] - min_p[0]) * inverse_leaf_size_[0])+1;` (dy, dz alike)
//   `if ((dx*dy*dz) > static_cast<int64_t>(std::numeric_limits<int32_t>::max()))` -> warn, copy the input
//   `min_b_[0] = static_cast<int> (floor (min_p[0] * inverse_leaf_size_[0]));  max_b_ ... ;  div_b_ = max_b_ - min_b_ + Eigen::Vector4i::Ones ();`
// fminb / divb are formed in either case (a caller that returns the input never reads them).
ALOAM_VOX_HD Box make_box(const float (&mn)[3], const float (&mx)[3], float inv) {
  Box b;
  const long long dx = (long long)((mx[0] - mn[0]) * inv) + 1, dy = (long long)((mx[1] - mn[1]) * inv) + 1, dz = (long long)((mx[2] - mn[2]) * inv) + 1;
  // (PCL's int64 product wraps for a box beyond 2^63 cells - two corners at +-3e5 m with a 0.2 m leaf; multiplied as unsigned here so that the wrap is
  // defined: the same bits as the signed multiply of an x86-64 build)
  b.unfiltered = (long long)((unsigned long long)dx * (unsigned long long)dy * (unsigned long long)dz) > kMaxCells;
  for (int q = 0; q < 3; ++q) {
    const int minb = (int)floorf(mn[q] * inv);
    b.divb[q] = (int)floorf(mx[q] * inv) - minb + 1;
    b.fminb[q] = (float)minb;
  }
  return b;
}
// Number of cells of a filtered box: every cell index is below it, and it is at most kMaxCells.
ALOAM_VOX_HD long long box_cells(const int (&divb)[3]) { return (long long)divb[0] * divb[1] * divb[2]; }

// ---- the cell index of a point in a box ---------------------------------------------------------------------------------------------------
//   `int ijk0 = static_cast<int> (floor (input_->points[*it].x * inverse_leaf_size_[0]) - static_cast<float> (min_b_[0]));` (ijk1, ijk2 alike)
//   `int idx = ijk0 * divb_mul_[0] + ijk1 * divb_mul_[1] + ijk2 * divb_mul_[2];`  with divb_mul_ = (1, div_b_[0], div_b_[0] * div_b_[1])
ALOAM_VOX_HD unsigned cell_index(const Box& b, float x, float y, float z, float inv) {
  const int i0 = (int)(floorf(x * inv) - b.fminb[0]);
  const int i1 = (int)(floorf(y * inv) - b.fminb[1]);
  const int i2 = (int)(floorf(z * inv) - b.fminb[2]);
  return (unsigned)(i0 + i1 * b.divb[0] + i2 * b.divb[0] * b.divb[1]);
}

// ---- run heads before the box is known (k_vox_lds) -------------------------------------------------------------------------------------------
// (fx, fy, fz) = cell_coord of a point, (px, py, pz) of its predecessor.  Equal to "cell_index differs from the predecessor's" for every box that
// holds both points, as long as cell_exact held for all points of the call.
ALOAM_VOX_HD bool cell_exact(float fx, float fy, float fz) { return fabsf(fx) < kExactCellLimit && fabsf(fy) < kExactCellLimit && fabsf(fz) < kExactCellLimit; }
ALOAM_VOX_HD bool cell_differs(float fx, float fy, float fz, float px, float py, float pz) { return fx != px || fy != py || fz != pz; }

// ---- packed cells (k_ring_features) ---------------------------------------------------------------------------------------------------------
// The cell coordinates of a point as 11 + 11 + 10 bits, biased to be non-negative: box and indices of a ring are then integer work on one LDS word per
// point.  min_b = floor(min * inv) = min over floor(p * inv) because floor and the f32 multiply are monotone; likewise max_b.
constexpr int kPackBiasXY = 1024, kPackBiasZ = 512;
ALOAM_VOX_HD bool cell_packable(float fx, float fy, float fz) { return fabsf(fx) < 1024.f && fabsf(fy) < 1024.f && fabsf(fz) < 512.f; }
ALOAM_VOX_HD unsigned pack_cell(float fx, float fy, float fz) {   // cell_packable(fx, fy, fz) holds
  return (unsigned)((int)fx + kPackBiasXY) | ((unsigned)((int)fy + kPackBiasXY) << 11) | ((unsigned)((int)fz + kPackBiasZ) << 22);
}
ALOAM_VOX_HD void unpack_cell(unsigned c, int (&ijk)[3]) { ijk[0] = (int)(c & 2047u); ijk[1] = (int)((c >> 11) & 2047u); ijk[2] = (int)(c >> 22); }   // still biased
struct PackedBox {
  int minc[3];       // min_b_ + bias
  int divc[3];       // div_b_
};
// The box from the minima / maxima of the unpacked (biased) cells.  Returns whether that DECIDES the call: PCL's guard multiplies
// int64((max - min) * inv) + 1 <= div_b + 1 per axis, so a product of (div_b + 1) within kMaxCells means "filtered" with this very box; anything else
// (no member at all: mx < mn) leaves the call to make_box on the points themselves.
ALOAM_VOX_HD bool make_packed_box(const int (&mn)[3], const int (&mx)[3], PackedBox& b) {
  for (int q = 0; q < 3; ++q) { b.minc[q] = mn[q]; b.divc[q] = mx[q] - mn[q] + 1; }
  return b.divc[0] > 0 && (long long)(b.divc[0] + 1) * (b.divc[1] + 1) * (b.divc[2] + 1) <= kMaxCells;
}
ALOAM_VOX_HD unsigned packed_cell_index(const PackedBox& b, unsigned c) {
  int ijk[3];
  unpack_cell(c, ijk);
  const int i0 = ijk[0] - b.minc[0], i1 = ijk[1] - b.minc[1], i2 = ijk[2] - b.minc[2];
  return (unsigned)(i0 + i1 * b.divc[0] + i2 * b.divc[0] * b.divc[1]);
}

// ---- the centroid of a cell -----------------------------------------------------------------------------------------------------------------
// `centroid.add (input_->points[...]); ... centroid.get (output.points[index]);` (downsample_all_data_: x, y, z and intensity): f32 sums in the order the
// caller adds the members, each DIVIDED by the count - a multiplication by 1 / n rounds differently.
struct Centroid {
  float sx = 0.f, sy = 0.f, sz = 0.f, si = 0.f;
  int n = 0;
  ALOAM_VOX_HD_MEMBER void add(float x, float y, float z, float w) { sx += x; sy += y; sz += z; si += w; ++n; }
  ALOAM_VOX_HD_MEMBER void get(float& x, float& y, float& z, float& w) const { const float fc = (float)n; x = sx / fc; y = sy / fc; z = sz / fc; w = si / fc; }
#if defined(__HIPCC__)
  __device__ __forceinline__ void add(const float4& p) { add(p.x, p.y, p.z, p.w); }
  __device__ __forceinline__ float4 get() const { float4 o; get(o.x, o.y, o.z, o.w); return o; }
#endif
};

}  // namespace voxel
}  // namespace aloam
