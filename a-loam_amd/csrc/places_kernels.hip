// a-loam_amd/csrc/places_kernels.hip — place recognition beside the reference (A-LOAM has none): the Scan Context descriptor of a sweep
// (Kim & Kim, IROS 2018), the place store and the match.
//   k_place_descriptor  ring slabs -> 20 x 60 cells (LDS unsigned max), column norms, mask of non-zero columns; one workgroup per sweep
//   k_place_add         descriptor + pose at that point of the stream -> one store entry, its unit-normalised columns and its mask
//   k_place_finish      the same derived arrays for entries that were loaded
//   k_place_match       all 60 shifts of one query against 128 entries: a 64 x 1200 x 128 product on v_mfma_f32_32x32x2_f32
//   k_place_select      the T best entries of a range under the total order (distance, index)
#include "places_kernels.hpp"

namespace aloam {

// Euclidean norm of one column (20 rings of one sector), summed in ascending ring order: the descriptor, the add and the load all use this
// one function, so a column has one norm whichever way it came into the store.
__device__ __forceinline__ float place_column_norm(const float* col) {
  float ss = 0.f;
  for (int r = 0; r < kPlaceRings; ++r) ss = ss + col[r] * col[r];
  return sqrtf(ss);
}
__device__ __forceinline__ float place_unit(float cell, float norm) { return norm > 0.f ? cell / norm : 0.f; }

// ---- descriptor -----------------------------------------------------------------------------------------------------------------------
// One workgroup per sweep streams its ring slabs once (16 B per kept point, nothing else is read) and keeps the 1200 cells in LDS.  The
// cell values are non-negative floats, whose order is the order of their bits as unsigned integers, so the cell maximum is one LDS
// atomic per point and does not depend on the order the points arrive in.
__global__ __launch_bounds__(kPlaceDescThreads) void k_place_descriptor(PlaceDescArgs a) {
  const int b = blockIdx.x, tid = threadIdx.x;
  if (!a.wanted[b]) return;
  __shared__ unsigned cells[kPlaceCells];
  __shared__ float fcells[kPlaceCells];
  for (int i = tid; i < kPlaceCells; i += kPlaceDescThreads) cells[i] = 0u;
  __syncthreads();
  const int* rs = a.ringstart + (long long)b * (a.R + 1);
  const float sector_scale = (float)(60.0 / (2.0 * M_PI));
  for (int r = 0; r < a.R; ++r) {
    int n = rs[r + 1] - rs[r];
    n = n < a.slab ? n : a.slab;
    const float4* src = a.slabs + ((long long)b * a.R + r) * a.slab;
    for (int i = tid; i < n; i += kPlaceDescThreads) {
      const float4 p = src[i];
      const float rho = sqrtf(p.x * p.x + p.y * p.y);
      const int ring = (int)(rho * a.ring_scale);
      if (ring >= kPlaceRings || ring < 0) continue;
      const float theta = atan2f_port(p.y, p.x) + (float)M_PI;
      int sec = (int)(theta * sector_scale);
      sec = sec < kPlaceSectors - 1 ? sec : kPlaceSectors - 1;
      sec = sec > 0 ? sec : 0;
      const float v = p.z + a.height;
      if (v > 0.f) atomicMax(&cells[sec * kPlaceRings + ring], __float_as_uint(v));
    }
  }
  __syncthreads();
  PlaceDesc& d = a.desc[b];
  for (int i = tid; i < kPlaceCells; i += kPlaceDescThreads) { const float v = __uint_as_float(cells[i]); fcells[i] = v; d.cells[i] = v; }
  __syncthreads();
  if (tid < 64) {
    float nrm = 0.f;
    if (tid < kPlaceSectors) { nrm = place_column_norm(fcells + tid * kPlaceRings); d.norms[tid] = nrm; }
    const unsigned long long m = __ballot(nrm > 0.f);
    if (tid == 0) { d.mask = m; d.n_points = rs[a.R]; d.pad = 0; }
  }
}

// ---- store ----------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void place_derive(const float* cells, float* unit, unsigned long long* mask, int tid) {   // first wave of a workgroup
  float nrm = 0.f;
  if (tid < kPlaceSectors) {
    nrm = place_column_norm(cells + tid * kPlaceRings);
    for (int r = 0; r < kPlaceRings; ++r) unit[tid * kPlaceRings + r] = place_unit(cells[tid * kPlaceRings + r], nrm);
  }
  const unsigned long long m = __ballot(nrm > 0.f);
  if (tid == 0) *mask = m;
}

__global__ __launch_bounds__(64) void k_place_add(PlaceAddArgs a) {
  const int i = blockIdx.x, tid = threadIdx.x;
  const int b = a.seqs[i];
  const PlaceDesc& d = a.desc[b];
  aloam_place& e = a.store[a.first + i];
  float* cells = &e.cells[0][0];
  for (int k = tid; k < kPlaceCells; k += 64) cells[k] = d.cells[k];
  if (tid == 0) {
    if (a.mapseq) {                                        // what aloam_export_poses writes as map_q_w / map_t_w / map_frames
      const MapSeq& m = a.mapseq[b];
      for (int k = 0; k < 4; ++k) e.q[k] = m.par[k];
      for (int k = 0; k < 3; ++k) e.t[k] = m.par[4 + k];
      e.frame = m.frame_count;
    } else {
      const OdomState& s = a.odom[b];
      for (int k = 0; k < 4; ++k) e.q[k] = s.q_w[k];
      for (int k = 0; k < 3; ++k) e.t[k] = s.t_w[k];
      e.frame = -1;
    }
    e.slot = b; e.n_points = d.n_points;
    e.pad[0] = e.pad[1] = e.pad[2] = 0;
  }
  place_derive(d.cells, a.unit + (long long)(a.first + i) * kPlaceCells, a.masks + a.first + i, tid);
}

__global__ __launch_bounds__(64) void k_place_finish(const aloam_place* store, float* unit, unsigned long long* masks, int first) {
  const int e = first + blockIdx.x;
  place_derive(&store[e].cells[0][0], unit + (long long)e * kPlaceCells, masks + e, threadIdx.x);
}

// ---- match ----------------------------------------------------------------------------------------------------------------------------
// With unit-normalised columns (zero columns stay zero) the sum of the cosines over the columns that are non-zero on both sides is the
// plain dot product of the two 1200-vectors, and a yaw shift of s sectors is an offset of 20 s cells into the sector-major query.  So the
// 60 shifts of one query against a tile of entries are A (64 x 1200, row s = the query read at offset -20 s from a doubled copy in LDS;
// rows 60 .. 63 repeat row 59 and are dropped) times B (1200 x tile, the entries' unit cells).  One wave owns 32 entries and both halves
// of the shifts: two 32 x 32 accumulators fed by one B operand.  v_mfma_f32_32x32x2_f32 takes A[i = lane & 31][k = lane >> 5] and
// B[k = lane >> 5][j = lane & 31]; the K order is chosen so that both operands are 16-byte loads: in step t the lanes below 32 hold cells
// 8 t .. 8 t + 3 and the lanes above hold 8 t + 4 .. 8 t + 7, and the four MFMAs of the step take one component each.  The order is a
// constant of the kernel, every accumulator is an exact f32 fmaf chain in that order, and nothing is combined across lanes before the
// epilogue: a (query, entry, shift) sum has the same bits wherever the entry falls in a tile, a range or a list.
typedef float f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ unsigned long long place_rotl60(unsigned long long m, int s) {
  return ((m << s) | (m >> (kPlaceSectors - s))) & ((1ull << kPlaceSectors) - 1ull);
}
// (d, s) < (bd, bs) in the order: lower distance first, then lower shift
__device__ __forceinline__ bool place_better(float d, int s, float bd, int bs) { return d < bd || (d == bd && s < bs); }

template <int HALF>
__device__ __forceinline__ void place_best_shift(const f32x16& acc, int h, unsigned long long cm, unsigned long long qm, float& bd, int& bs) {
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) {
    const int s = 32 * HALF + (reg & 3) + 8 * (reg >> 2) + 4 * h;      // C/D layout: row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
    if (s >= kPlaceSectors) continue;
    const int cnt = __popcll(cm & place_rotl60(qm, s));
    if (cnt == 0) continue;
    const float d = 1.0f - acc[reg] / (float)cnt;
    if (place_better(d, s, bd, bs) || bs < 0) { if (d == d) { bd = d; bs = s; } }
  }
}

__global__ __launch_bounds__(kPlaceMatchThreads) void k_place_match(PlaceMatchArgs a) {
  const int qi = blockIdx.y, tid = threadIdx.x;
  const int lo = a.lo[qi], hi = a.hi[qi];
  const int e0 = lo + blockIdx.x * kPlaceTile;
  if (e0 >= hi) return;
  __shared__ __attribute__((aligned(16))) float q2[2 * kPlaceCells];
  const PlaceDesc& d = a.desc[a.seqs[qi]];
  for (int i = tid; i < kPlaceCells; i += kPlaceMatchThreads) {
    const float v = place_unit(d.cells[i], d.norms[i / kPlaceRings]);
    q2[i] = v; q2[i + kPlaceCells] = v;
  }
  __syncthreads();
  const int wave = tid >> 6, lane = tid & 63, h = lane >> 5, col = lane & 31;
  const int e = e0 + wave * 32 + col;
  if (e0 + wave * 32 >= hi) return;                        // (no barrier follows)
  const int ec = e < hi ? e : hi - 1;                      // lanes past the range read the last entry of it; their results are dropped
  const float4* brow = reinterpret_cast<const float4*>(a.unit + (long long)ec * kPlaceCells) + h;
  const int s0 = col, s1 = col + 32 < kPlaceSectors ? col + 32 : kPlaceSectors - 1;
  const float4* a0 = reinterpret_cast<const float4*>(q2 + kPlaceRings * (kPlaceSectors - s0)) + h;   // A[s][k] = q2[k + 20 (60 - s)]
  const float4* a1 = reinterpret_cast<const float4*>(q2 + kPlaceRings * (kPlaceSectors - s1)) + h;
  f32x16 acc0, acc1;
#pragma unroll
  for (int r = 0; r < 16; ++r) { acc0[r] = 0.f; acc1[r] = 0.f; }
  float4 bv = brow[0];
  for (int t = 0; t < kPlaceCells / 8; ++t) {
    const int tn = t + 1 < kPlaceCells / 8 ? t + 1 : t;
    const float4 bn = brow[2 * tn];                        // the next step's entry cells, in flight under this step's MFMAs
    const float4 x = a0[2 * t], y = a1[2 * t];
    acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(x.x, bv.x, acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(y.x, bv.x, acc1, 0, 0, 0);
    acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(x.y, bv.y, acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(y.y, bv.y, acc1, 0, 0, 0);
    acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(x.z, bv.z, acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(y.z, bv.z, acc1, 0, 0, 0);
    acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(x.w, bv.w, acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(y.w, bv.w, acc1, 0, 0, 0);
    bv = bn;
  }
  // epilogue: the lane holds 32 of its entry's 64 shifts (its partner lane ^ 32 the others); shifts are visited in ascending order
  const unsigned long long cm = a.masks[ec], qm = d.mask;
  float bd = 0.f; int bs = -1;
  place_best_shift<0>(acc0, h, cm, qm, bd, bs);
  place_best_shift<1>(acc1, h, cm, qm, bd, bs);
  const float od = __shfl_xor(bd, 32, 64);
  const int os = __shfl_xor(bs, 32, 64);
  if (os >= 0 && (bs < 0 || place_better(od, os, bd, bs))) { bd = od; bs = os; }
  if (h == 0 && e < hi) a.pairs[(long long)qi * a.max_range + (e - lo)] = make_int2(__float_as_int(bd), bs);
}

// The T best of one range under the total order (distance, index): T rounds, each the minimum key above the last one taken.  Keys are
// unique (the index is part of them), so the result does not depend on how the range is dealt over the threads.
__device__ __forceinline__ unsigned place_order_bits(int fbits) {   // f32 bits -> unsigned with the same order as the floats
  const unsigned u = (unsigned)fbits;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__global__ __launch_bounds__(256) void k_place_select(PlaceMatchArgs a) {
  const int qi = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const int lo = a.lo[qi], n = a.hi[qi] - lo;
  const int2* pairs = a.pairs + (long long)qi * a.max_range;
  __shared__ unsigned long long part[4];
  unsigned long long prev = 0ull;
  bool have_prev = false;
  for (int t = 0; t < a.T; ++t) {
    unsigned long long best = ~0ull;
    for (int i = tid; i < n; i += 256) {
      const int2 p = pairs[i];
      if (p.y < 0) continue;
      const unsigned long long key = ((unsigned long long)place_order_bits(p.x) << 32) | (unsigned)i;
      if ((!have_prev || key > prev) && key < best) best = key;
    }
    best = wave_extreme_u64<false>(best, lane);
    if (lane == 0) part[tid >> 6] = best;
    __syncthreads();
    best = part[0];
    for (int w = 1; w < 4; ++w) best = part[w] < best ? part[w] : best;
    __syncthreads();
    if (tid == 0) {
      aloam_place_match m;
      if (best == ~0ull) { m.entry = -1; m.shift = -1; m.distance = 0.f; }
      else { const int i = (int)(unsigned)best; const int2 p = pairs[i]; m.entry = lo + i; m.shift = p.y; m.distance = __int_as_float(p.x); }
      m.pad = 0;
      a.dst[(long long)qi * a.T + t] = m;
    }
    if (best == ~0ull) { have_prev = true; prev = ~0ull; } else { have_prev = true; prev = best; }
  }
}

void launch_place_descriptor(const PlaceDescArgs& a, hipStream_t s) { hipLaunchKernelGGL(k_place_descriptor, dim3(a.B), dim3(kPlaceDescThreads), 0, s, a); }
void launch_place_add(const PlaceAddArgs& a, hipStream_t s) { hipLaunchKernelGGL(k_place_add, dim3(a.n), dim3(64), 0, s, a); }
void launch_place_finish(const aloam_place* store, float* unit, unsigned long long* masks, int first, int count, hipStream_t s) {
  hipLaunchKernelGGL(k_place_finish, dim3(count), dim3(64), 0, s, store, unit, masks, first);
}
void launch_place_match(const PlaceMatchArgs& a, hipStream_t s) {
  if (a.max_range > 0) hipLaunchKernelGGL(k_place_match, dim3((a.max_range + kPlaceTile - 1) / kPlaceTile, a.n), dim3(kPlaceMatchThreads), 0, s, a);
  hipLaunchKernelGGL(k_place_select, dim3(a.n), dim3(256), 0, s, a);
}

}  // namespace aloam
