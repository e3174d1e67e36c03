// a-loam_amd/csrc/information_device.hpp — the second half of aloam_export_pose_information, shared by k_pose_information_odom
// (odometry_kernels.hip) and k_pose_information_map (mapping_kernels.hip): the robust Gauss-Newton sums of one evaluation at the pose a
// solve left (lm_device.hpp: acc[0..20] J^T J, acc[21..26] J^T r, acc[27] cost) become the public record of include/aloam_mi355x.h — scaled
// to radians and metres, decomposed, with both marginals.  One thread does it, in f64; every loop below has compile-time bounds and is
// unrolled, so the matrices live in registers (a runtime index would send them to scratch memory).
#pragma once
#include <cstddef>

#include "../../include/aloam_mi355x.h"
#include "lm_device.hpp"

namespace aloam {

// An entry of the id list the kernels get: the sequence, and the host's "a solve has run and nothing has invalidated it" flag.
constexpr int kInfoSolvedBit = 1 << 30, kInfoSeqMask = kInfoSolvedBit - 1;
constexpr int kInfoJacobiSweeps = 12;        // cyclic Jacobi converges quadratically: 6 x 6 matrices are done after 4-6 sweeps
constexpr double kInfoOffTol = 1e-17;        // a sweep starts only while sum |a_pq| (p < q) > kInfoOffTol * sum |a_pp|
constexpr double kInfoPivotTol = 1e-12;      // a Cholesky pivot counts as positive when it exceeds kInfoPivotTol * its diagonal entry

// Eigenpairs of the symmetric N x N matrix A (both triangles filled, overwritten) by cyclic Jacobi: rotations in the fixed order
// (0,1), (0,2) .. (0,N-1), (1,2) .. (N-2,N-1), sweep after sweep until the off-diagonal sum has fallen below kInfoOffTol of the diagonal
// sum (or kInfoJacobiSweeps sweeps have run), so the result is a function of the matrix alone.  Then ascending order (equal values keep
// their index order) and the sign rule of the public record: the component of largest magnitude of every eigenvector is positive, the
// lowest index deciding a tie.  vec[r][k]: component r of the eigenvector of val[k].
template <int N>
__device__ __forceinline__ void jacobi_eigen(double (&A)[N][N], double (&val)[N], double (&vec)[N][N]) {
#pragma unroll
  for (int i = 0; i < N; ++i) {
#pragma unroll
    for (int j = 0; j < N; ++j) vec[i][j] = i == j ? 1.0 : 0.0;
  }
#pragma unroll 1
  for (int sweep = 0; sweep < kInfoJacobiSweeps; ++sweep) {
    double off = 0.0, dia = 0.0;
#pragma unroll
    for (int p = 0; p < N; ++p) {
      dia += fabs(A[p][p]);
#pragma unroll
      for (int q = p + 1; q < N; ++q) off += fabs(A[p][q]);
    }
    if (!(off > kInfoOffTol * dia)) break;
#pragma unroll
    for (int p = 0; p < N - 1; ++p) {
#pragma unroll
      for (int q = p + 1; q < N; ++q) {
        const double apq = A[p][q];
        // (Golub & Van Loan, symmetric Schur decomposition) t = tan of the rotation that annihilates a_pq, the smaller root
        const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
        double t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
        if (theta < 0.0) t = -t;
        if (apq == 0.0) t = 0.0;                                              // (theta is then inf or nan: nothing to annihilate)
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
        A[p][p] -= t * apq;
        A[q][q] += t * apq;
        A[p][q] = 0.0;
        A[q][p] = 0.0;
#pragma unroll
        for (int k = 0; k < N; ++k) {
          if (k != p && k != q) {
            const double akp = A[k][p], akq = A[k][q];
            const double np_ = c * akp - s * akq, nq_ = s * akp + c * akq;
            A[k][p] = np_; A[p][k] = np_;
            A[k][q] = nq_; A[q][k] = nq_;
          }
          const double vkp = vec[k][p], vkq = vec[k][q];
          vec[k][p] = c * vkp - s * vkq;
          vec[k][q] = s * vkp + c * vkq;
        }
      }
    }
  }
#pragma unroll
  for (int i = 0; i < N; ++i) val[i] = A[i][i];
  // ascending, stable: bubble passes over neighbouring columns (selects, constant indices)
#pragma unroll
  for (int pass = 0; pass < N - 1; ++pass) {
#pragma unroll
    for (int i = 0; i < N - 1 - pass; ++i) {
      const bool sw = val[i + 1] < val[i];
      const double a = val[i], b = val[i + 1];
      val[i] = sw ? b : a; val[i + 1] = sw ? a : b;
#pragma unroll
      for (int r = 0; r < N; ++r) {
        const double x = vec[r][i], y = vec[r][i + 1];
        vec[r][i] = sw ? y : x; vec[r][i + 1] = sw ? x : y;
      }
    }
  }
#pragma unroll
  for (int k = 0; k < N; ++k) {
    double big = vec[0][k];
#pragma unroll
    for (int r = 1; r < N; ++r) if (fabs(vec[r][k]) > fabs(big)) big = vec[r][k];
    if (big < 0.0) {
#pragma unroll
      for (int r = 0; r < N; ++r) vec[r][k] = -vec[r][k];
    }
  }
}

// M = D - C^T A^-1 C for the 3 x 3 blocks of a symmetric matrix (A, D symmetric) through the Cholesky factor of A: A = L L^T, Y = L^-1 C,
// M = D - Y^T Y, the upper triangle computed and mirrored.  false (M untouched) when A is not positive definite (kInfoPivotTol).
__device__ __forceinline__ bool schur3(const double A[3][3], const double Cm[3][3], const double D[3][3], double M[3][3]) {
  double L[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j <= i; ++j) {
      double s = A[i][j];
#pragma unroll
      for (int k = 0; k < j; ++k) s -= L[i][k] * L[j][k];
      if (i == j) {
        if (!(s > kInfoPivotTol * A[i][i])) return false;
        L[i][i] = sqrt(s);
      } else {
        L[i][j] = s / L[j][j];
      }
    }
  }
  double Y[3][3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      double s = Cm[i][c];
#pragma unroll
      for (int k = 0; k < i; ++k) s -= L[i][k] * Y[k][c];
      Y[i][c] = s / L[i][i];
    }
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = i; j < 3; ++j) {
      const double m = D[i][j] - ((Y[0][i] * Y[0][j] + Y[1][i] * Y[1][j]) + Y[2][i] * Y[2][j]);
      M[i][j] = m; M[j][i] = m;
    }
  }
  return true;
}

__device__ __forceinline__ void store_marginal(bool ok, double (&M)[3][3], double* info, double* vals, double* vecs) {
  double val[3] = {0.0, 0.0, 0.0}, vec[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
  if (!ok) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
      for (int j = 0; j < 3; ++j) M[i][j] = 0.0;
    }
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) info[i * 3 + j] = M[i][j];
  }
  if (ok) jacobi_eigen<3>(M, val, vec);
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    vals[i] = val[i];
#pragma unroll
    for (int j = 0; j < 3; ++j) vecs[i * 3 + j] = vec[i][j];
  }
}

// The whole record of one sequence, by the calling thread.  `solved`: a solve has run for the sequence and nothing has invalidated it
// since (the host's flag); acc / n_line / n_plane: the block-wide sums of the evaluation (ignored without `solved`).
__device__ __forceinline__ void write_pose_information(aloam_pose_information* out, bool solved, const double* acc, int n_line, int n_plane, int frame) {
  double* words = reinterpret_cast<double*>(out);
  constexpr int kDoubles = (int)(offsetof(aloam_pose_information, n_line) / sizeof(double));
  for (int k = 0; k < kDoubles; ++k) words[k] = 0.0;
  out->n_line = 0; out->n_plane = 0; out->rows = 0;
  out->frame = frame;
  out->pad[0] = 0; out->pad[1] = 0; out->pad[2] = 0;
  if (!solved) { out->status = ALOAM_INFO_NONE; return; }
  if (n_line + n_plane == 0) { out->status = ALOAM_INFO_NO_FACTORS; return; }
  out->n_line = n_line; out->n_plane = n_plane; out->rows = 3 * n_line + n_plane;
  out->cost = acc[27];
  // unpack, and radians for the rotation part: theta = 2 delta, so H_theta = S H_delta S with S = diag(1/2, 1/2, 1/2, 1, 1, 1)
  double H[6][6];
  {
    int o = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
#pragma unroll
      for (int j = i; j < 6; ++j) {
        const double v = acc[o++] * ((i < 3 ? 0.5 : 1.0) * (j < 3 ? 0.5 : 1.0));
        H[i][j] = v; H[j][i] = v;
      }
    }
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    out->gradient[i] = acc[21 + i] * (i < 3 ? 0.5 : 1.0);
#pragma unroll
    for (int j = 0; j < 6; ++j) out->info[i * 6 + j] = H[i][j];
  }
  double Hrr[3][3], Hrt[3][3], Htr[3][3], Htt[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) { Hrr[i][j] = H[i][j]; Hrt[i][j] = H[i][3 + j]; Htr[i][j] = H[3 + i][j]; Htt[i][j] = H[3 + i][3 + j]; }
  }
  {
    double val[6], vec[6][6];
    jacobi_eigen<6>(H, val, vec);
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      out->eigenvalues[i] = val[i];
#pragma unroll
      for (int j = 0; j < 6; ++j) out->eigenvectors[i * 6 + j] = vec[i][j];
    }
  }
  double M[3][3];
  const bool ok_t = schur3(Hrr, Hrt, Htt, M);                                  // H_tt - H_tr H_rr^-1 H_rt
  store_marginal(ok_t, M, out->trans_info, out->trans_eigenvalues, out->trans_eigenvectors);
  const bool ok_r = schur3(Htt, Htr, Hrr, M);                                  // H_rr - H_rt H_tt^-1 H_tr
  store_marginal(ok_r, M, out->rot_info, out->rot_eigenvalues, out->rot_eigenvectors);
  out->status = ok_t && ok_r ? ALOAM_INFO_OK : ALOAM_INFO_SINGULAR;
}

}  // namespace aloam
