// a-loam_amd/csrc/map_search_device.hpp — device functions of the submap search and the line / plane fit (reference
// src/laserMapping.cpp:157-166, :576-706), shared by the mapping step (mapping_kernels.hip) and the scoring of map-pose hypotheses
// (relocalize_kernels.hip).  One definition, so that both count the same factors from the same operations.
#pragma once
#include "lm_device.hpp"
#include "mapping_kernels.hpp"

namespace aloam {

namespace {

__device__ __forceinline__ unsigned hash_cell(int a, int b, int c) {
  return ((unsigned)a * 73856093u) ^ ((unsigned)b * 19349663u) ^ ((unsigned)c * 83492791u);
}
// Bucket of a 2 m map cell: the low kMapLocalBits bits of each cell coordinate, interleaved (x, y, z, x, y, z, ...), are the low bits of
// the bucket, the hash of the super-cell of 2^kMapLocalBits cells per axis the rest.  Neighbouring cells differ in a parity, so the
// eight cells of any 2x2x2 block land in eight DIFFERENT buckets (k_map_search walks them without a duplicate test), and the cells of
// one super-cell are neighbours in the bucket table and therefore in the sorted copy of the submap: the 64 queries of a wave, close
// together in space, read close together in memory.
constexpr int kMapLocalBits = 1;
static_assert(kMapLocalBits >= 1 && kMapLocalBits <= 4, "k_map_search walks the eight cells of a 2x2x2 block without a duplicate test: they must land in eight different buckets");
__device__ __forceinline__ unsigned map_local_bits(int v, int axis) {      // bit i of v -> bit 3 i + axis
  unsigned l = 0;
#pragma unroll
  for (int i = 0; i < kMapLocalBits; ++i) l |= (unsigned)((v >> i) & 1) << (3 * i + axis);
  return l;
}
__device__ __forceinline__ unsigned map_bucket(int x, int y, int z, int H) {
  return ((hash_cell(x >> kMapLocalBits, y >> kMapLocalBits, z >> kMapLocalBits) << (3 * kMapLocalBits)) | map_local_bits(x, 0) | map_local_bits(y, 1) | map_local_bits(z, 2)) & (unsigned)(H - 1);
}

// Hamilton product a * b (x,y,z,w storage), as Eigen evaluates it.
__device__ __forceinline__ void quat_mul(const double a[4], const double b[4], double o[4]) {
  o[0] = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
  o[1] = a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2];
  o[2] = a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0];
  o[3] = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
}

// pointAssociateToMap (reference src/laserMapping.cpp:157-166): f64 rotation + translation, stored back to f32.
__device__ __forceinline__ float4 associate_to_map(const float4& p, const double par[7]) {
  double o[3];
  quat_rotate(par, (double)p.x, (double)p.y, (double)p.z, o);
  return make_float4((float)(o[0] + par[4]), (float)(o[1] + par[5]), (float)(o[2] + par[6]), p.w);
}

// kd-tree stand-in of the submap: 2 m cells.  Every point closer than 1 m to a query lies in the 2x2x2 block of cells made of the
// query's own cell and, per axis, the neighbour on the side of the cell the query sits in (8 bucket look-ups instead of the 27 a
// 1 m grid needs).  Power-of-two cell size: p * 0.5f is exact, so cell membership is decided without rounding.
constexpr float kMapCellInv = 0.5f;

struct __attribute__((packed, aligned(4))) MapIntPair { int a, b; };      // start[h], start[h + 1] by one 8-byte load
typedef float mfloat2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float dist_to_map(const float4& p, mfloat2 sxy, float sz) {
  const mfloat2 pxy = {p.x, p.y};
  const mfloat2 dxy = pxy - sxy, qxy = dxy * dxy;                             // packed f32: the same two subtractions and products
  const float ddz = p.z - sz;
  return (qxy.x + qxy.y) + ddz * ddz;                                         // FLANN L2_Simple, f32: (dx^2 + dy^2) + dz^2
}

// The five nearest as packed keys (f32 distance bits << 32 | submap index: one 64-bit compare orders by (distance, index)) + the position
// of the entry in the bucketed copy; coordinates are fetched through the position at the end: 15 registers instead of the 25 five
// neighbours with coordinates need, which is what takes k_map_search from 72 - 74 to 63 / 65 registers.
struct Top5P {
  unsigned long long k[5]; int pos[5];
  __device__ __forceinline__ void init() {
#pragma unroll
    for (int s = 0; s < 5; ++s) { k[s] = 0x3f800000ull << 32; pos[s] = 0; }    // (1.0f, 0): a key is below it exactly when its distance is < 1.0f
  }
  __device__ __forceinline__ void insert(float dd, int ii, int pp) {          // branch-free; k stays ascending
    const unsigned long long key = (unsigned long long)__float_as_uint(dd) << 32 | (unsigned)ii;
    const bool c0 = key < k[0], c1 = key < k[1], c2 = key < k[2], c3 = key < k[3], c4 = key < k[4];
    k[4] = c3 ? k[3] : (c4 ? key : k[4]); pos[4] = c3 ? pos[3] : (c4 ? pp : pos[4]);
    k[3] = c2 ? k[2] : (c3 ? key : k[3]); pos[3] = c2 ? pos[2] : (c3 ? pp : pos[3]);
    k[2] = c1 ? k[1] : (c2 ? key : k[2]); pos[2] = c1 ? pos[1] : (c2 ? pp : pos[2]);
    k[1] = c0 ? k[0] : (c1 ? key : k[1]); pos[1] = c0 ? pos[0] : (c1 ? pp : pos[1]);
    k[0] = c0 ? key : k[0];               pos[0] = c0 ? pp : pos[0];
  }
};

// Symmetric 3x3 eigen-decomposition by cyclic Jacobi, standing in for Eigen::SelfAdjointEigenSolver<Matrix3d>
// (reference src/laserMapping.cpp:605).  The operation sequence is fixed (DESIGN.md "Mapping") so that CPU restatements of it
// agree bit-for-bit; it is not Eigen's tridiagonal-QL algorithm, results differ from Eigen at the 1e-15 level.
// Returns ascending eigenvalues in vals and the eigenvector of the LARGEST one in dir (the only one the reference uses, :609).
__device__ __forceinline__ void sym_eigen3(const double A0[3][3], double vals[3], double dir[3]) {
  double a[3][3], v[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) a[i][j] = 0.5 * (A0[i][j] + A0[j][i]);
  for (int sweep = 0; sweep < 50; ++sweep) {
    const double off = fabs(a[0][1]) + fabs(a[0][2]) + fabs(a[1][2]);
    if (off <= 1e-22 * (fabs(a[0][0]) + fabs(a[1][1]) + fabs(a[2][2]))) break;
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
      for (int q = p + 1; q < 3; ++q) {
        if (a[p][q] == 0.0) continue;
        const double theta = (a[q][q] - a[p][p]) / (2.0 * a[p][q]);
        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double cs = 1.0 / sqrt(t * t + 1.0), sn = t * cs;
#pragma unroll
        for (int k = 0; k < 3; ++k) { const double akp = a[k][p], akq = a[k][q]; a[k][p] = cs * akp - sn * akq; a[k][q] = sn * akp + cs * akq; }
#pragma unroll
        for (int k = 0; k < 3; ++k) { const double apk = a[p][k], aqk = a[q][k]; a[p][k] = cs * apk - sn * aqk; a[q][k] = sn * apk + cs * aqk; }
        a[p][q] = 0.0; a[q][p] = 0.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) { const double vkp = v[k][p], vkq = v[k][q]; v[k][p] = cs * vkp - sn * vkq; v[k][q] = sn * vkp + cs * vkq; }
      }
  }
  // ascending order of the diagonal, same exchange sequence as the stand-in (order[] = {0,1,2}; swap when a later one is smaller)
  double dg[3] = {a[0][0], a[1][1], a[2][2]};
  double c0[3] = {v[0][0], v[1][0], v[2][0]}, c1[3] = {v[0][1], v[1][1], v[2][1]}, c2[3] = {v[0][2], v[1][2], v[2][2]};
  auto swp = [&](double& x, double& y, double* cx, double* cy) {
    const double tv = x; x = y; y = tv;
#pragma unroll
    for (int k = 0; k < 3; ++k) { const double tc = cx[k]; cx[k] = cy[k]; cy[k] = tc; }
  };
  if (dg[1] < dg[0]) swp(dg[0], dg[1], c0, c1);
  if (dg[2] < dg[0]) swp(dg[0], dg[2], c0, c2);
  if (dg[2] < dg[1]) swp(dg[1], dg[2], c1, c2);
  vals[0] = dg[0]; vals[1] = dg[1]; vals[2] = dg[2];
  dir[0] = c2[0]; dir[1] = c2[1]; dir[2] = c2[2];
}

// min |A x - b| for the 5 x 3 plane fit: Householder QR with column pivoting, standing in for colPivHouseholderQr().solve()
// (reference src/laserMapping.cpp:663); fixed operation sequence, see above.
__device__ __forceinline__ void lstsq_5x3(double a[5][3], double b[5], double x[3]) {
  int perm[3] = {0, 1, 2};
  int rank = 0;
  double maxnorm0 = 0.0;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    if (rank != k) break;
    int piv = k;
    double best = -1.0;
#pragma unroll
    for (int j = k; j < 3; ++j) {
      double s = 0.0;
#pragma unroll
      for (int i = k; i < 5; ++i) s += a[i][j] * a[i][j];
      if (s > best) { best = s; piv = j; }
    }
    if (k == 0) maxnorm0 = best;
    if (!(best > maxnorm0 * 1e-30)) break;
#pragma unroll
    for (int j = k + 1; j < 3; ++j) {
      if (piv == j) {
#pragma unroll
        for (int i = 0; i < 5; ++i) { const double tv = a[i][k]; a[i][k] = a[i][j]; a[i][j] = tv; }
        const int tp = perm[k]; perm[k] = perm[j]; perm[j] = tp;
      }
    }
    const double alpha = (a[k][k] > 0.0 ? -1.0 : 1.0) * sqrt(best);
    double v[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) v[i] = i < k ? 0.0 : a[i][k];
    v[k] -= alpha;
    double vv = 0.0;
#pragma unroll
    for (int i = k; i < 5; ++i) vv += v[i] * v[i];
    if (vv > 0.0) {
#pragma unroll
      for (int j = k; j < 3; ++j) {
        double s = 0.0;
#pragma unroll
        for (int i = k; i < 5; ++i) s += v[i] * a[i][j];
        s = 2.0 * s / vv;
#pragma unroll
        for (int i = k; i < 5; ++i) a[i][j] -= s * v[i];
      }
      double s = 0.0;
#pragma unroll
      for (int i = k; i < 5; ++i) s += v[i] * b[i];
      s = 2.0 * s / vv;
#pragma unroll
      for (int i = k; i < 5; ++i) b[i] -= s * v[i];
    }
    ++rank;
  }
  double y[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int k = 2; k >= 0; --k) {
    if (k < rank) {
      double s = b[k];
#pragma unroll
      for (int j = k + 1; j < 3; ++j) if (j < rank) s -= a[k][j] * y[j];
      y[k] = s / a[k][k];
    }
  }
  x[0] = x[1] = x[2] = 0.0;
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int j = 0; j < 3; ++j) if (perm[k] == j) x[j] = y[k];
}

}  // namespace

}  // namespace aloam
