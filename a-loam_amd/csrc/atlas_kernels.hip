// a-loam_amd/csrc/atlas_kernels.hip — gfx950 kernels that keep what the mapping window drops.
//
// The reference's map is the 21 x 21 x 11 window of 50 m cubes around the sensor; when the sensor comes within three cubes of an edge the
// window shifts and the slab that falls off is cleared (src/laserMapping.cpp:323-507).  k_map_begin does the same to the cube descriptors.
//   k_map_spill        runs right before k_map_begin and is read-only for the sequence: it predicts the shift of this step from the
//                      same pose arithmetic and copies every non-empty cube the shift will empty into the sequence's spill rows as a tile
//                      (absolute cube, class, count, frame, points)
//   k_atlas_window     serves an attached, frozen sequence its window from the context's atlas (aloam_atlas_load): whenever the window is
//                      stale or about to shift, all 4851 cubes are looked up in the class directories and copied into the pool row
//   k_atlas_merge_segments   aloam_atlas_load: VoxSegs of the cubes that several tiles make up, for the existing voxel filter
//   k_spill_count / k_spill_gather / k_spill_clear   the drain (aloam_export_map_spill): tiles and points of the listed sequences packed
//                      back to back into the caller's arrays, in stream order; the offsets come from k_export_scan (export_kernels.hip)
// Integer work and 16-byte point copies: HBM- and latency-bound, no MFMA.  All stores are plain vector stores.
#include "atlas_kernels.hpp"

#include "export_kernels.hpp"
#include "lm_device.hpp"
#include "map_window_device.hpp"

namespace aloam {

namespace {

// Does the cube at window index c = x + 21 y + 441 z leave the window when it shifts by s?  The reference shifts axis by axis and a slab
// that re-enters is empty, so a cube survives iff every shifted index stays inside the window.
__device__ __forceinline__ bool cube_falls(int c, const int s[3]) {
  const int x = c % kMapW + s[0], y = (c / kMapW) % kMapH + s[1], z = c / (kMapW * kMapH) + s[2];
  return x < 0 || x >= kMapW || y < 0 || y >= kMapH || z < 0 || z >= kMapD;
}

__device__ __forceinline__ aloam_map_tile make_tile(int c, const int cen[3], int cls, int count, int frame, long long first) {
  aloam_map_tile t;
  t.cube[0] = c % kMapW - cen[0]; t.cube[1] = (c / kMapW) % kMapH - cen[1]; t.cube[2] = c / (kMapW * kMapH) - cen[2];
  t.feature_class = cls; t.count = count; t.frame = frame; t.first_point = first;
  return t;
}

}  // namespace

// One workgroup per sequence, both classes in turn.
__global__ __launch_bounds__(256) void k_map_spill(SpillArgs a) {
  const int b = blockIdx.x, tid = threadIdx.x;
  if (seq_idle(a.active, b)) return;                                         // growing or frozen: both shift, both spill
  if (a.attached && a.attached[b]) return;                                   // its window is cut from the atlas: nothing is lost
  const MapSeq& ms = a.seq[b];
  __shared__ int s_shift[3], s_cen[3], s_scan[256], s_new[2];
  if (tid == 0) {
    int sh[3];
    window_shift(ms, a.odom[b], sh);
    for (int k = 0; k < 3; ++k) { s_shift[k] = sh[k]; s_cen[k] = ms.cen[k]; }
  }
  __syncthreads();
  const int s[3] = {s_shift[0], s_shift[1], s_shift[2]};
  if ((s[0] | s[1] | s[2]) == 0) return;                                     // almost every step
  const int cen[3] = {s_cen[0], s_cen[1], s_cen[2]};
  const int frame = ms.frame_count;
  int* cnt = a.counters + (long long)b * kSpillInts;
  constexpr int PER = (kMapCubes + 255) / 256;
  int dropped_tiles = 0, dropped_points = 0;                                 // (thread 0's)
  for (int cls = 0; cls < 2; ++cls) {
    const CubeDesc* T = a.cubes + ((long long)b * 2 + cls) * kMapCubes;
    aloam_map_tile* row_t = a.tiles + ((long long)b * 2 + cls) * a.max_tiles;
    float4* row_p = a.points + ((long long)b * 2 + cls) * a.max_points;
    const float4* pool = (cls ? a.pool[1] : a.pool[0]) + (long long)b * a.pool_cap;
    const int base_t = cnt[kSpillTiles + cls], base_p = cnt[kSpillPoints + cls];
    // tiles of this class in ascending window index: thread t owns cubes [19 t, 19 t + 19)
    int nt = 0, np = 0;
    for (int k = 0; k < PER; ++k) {
      const int c = tid * PER + k;
      if (c >= kMapCubes) break;
      const int n = T[c].cnt;
      if (n > 0 && cube_falls(c, s)) { nt += 1; np += n; }
    }
    int total_t = 0, total_p = 0;
    int run_t = block_exclusive_scan<int, 256>(nt, s_scan, &total_t);
    int run_p = block_exclusive_scan<int, 256>(np, s_scan, &total_p);
    if (total_t == 0) continue;
    const bool fits = (long long)base_t + total_t <= a.max_tiles && (long long)base_p + total_p <= a.max_points;
    if (fits) {
      for (int k = 0; k < PER && nt > 0; ++k) {
        const int c = tid * PER + k;
        if (c >= kMapCubes) break;
        const int n = T[c].cnt;
        if (n > 0 && cube_falls(c, s)) { row_t[base_t + run_t] = make_tile(c, cen, cls, n, frame, base_p + run_p); run_t += 1; run_p += n; }
      }
      if (tid == 0) s_new[0] = total_t, s_new[1] = total_p;
    } else if (tid == 0) {
      // The rows are full: a tile is written whole or not at all, and one that is dropped takes no room, so the tiles behind it are still
      // kept when they fit.  That is a sequential decision: one lane walks the cubes in order (rare, and reported as ALOAM_E_CAPACITY).
      int wt = 0, wp = 0;
      for (int c = 0; c < kMapCubes; ++c) {
        const int n = T[c].cnt;
        if (n <= 0 || !cube_falls(c, s)) continue;
        if (base_t + wt < a.max_tiles && (long long)base_p + wp + n <= a.max_points) { row_t[base_t + wt] = make_tile(c, cen, cls, n, frame, base_p + wp); wt += 1; wp += n; }
        else { dropped_tiles += 1; dropped_points += n; }
      }
      s_new[0] = wt; s_new[1] = wp;
    }
    __syncthreads();                                                         // the new tile records are visible to the whole workgroup
    const int new_t = s_new[0], new_p = s_new[1];
    for (int t = 0; t < new_t; ++t) {
      const aloam_map_tile tl = row_t[base_t + t];
      const int c = (tl.cube[0] + cen[0]) + kMapW * (tl.cube[1] + cen[1]) + kMapW * kMapH * (tl.cube[2] + cen[2]);
      copy_points(row_p + tl.first_point, pool + T[c].off, tl.count);
    }
    __syncthreads();                                                         // s_new is rewritten by the next class
    if (tid == 0) { cnt[kSpillTiles + cls] = base_t + new_t; cnt[kSpillPoints + cls] = base_p + new_p; }
  }
  if (tid == 0 && dropped_tiles) { cnt[kSpillDroppedTiles] += dropped_tiles; cnt[kSpillDroppedPoints] += dropped_points; }
}

// ---- the drain ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_spill_count(SpillExportArgs a, int* tile_cnt, int* point_cnt) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= a.n) return;
  const int* cnt = a.counters + (long long)a.seqs[g] * kSpillInts;
  tile_cnt[g] = cnt[kSpillTiles] + cnt[kSpillTiles + 1];
  point_cnt[g] = cnt[kSpillPoints] + cnt[kSpillPoints + 1];
}

// A sequence is written when both of its ranges end inside the caps.
__device__ __forceinline__ bool spill_written(const SpillExportArgs& a, int i) { return a.tile_off[i + 1] <= a.cap_tiles && a.point_off[i + 1] <= a.cap_points; }

constexpr int kSpillGatherZ = 8;                           // workgroups per listed sequence: they share its tiles and its chunks of 2048 points

// Workgroup (i, g): its share of sequence seqs[i]'s tiles (corner row, then surf row; first_point rewritten to index points_dst) and of
// its points, in chunks of 8 x 256.  An empty spill - the every-step drain of a recording run - returns after four loads.
__global__ __launch_bounds__(256) void k_spill_gather(SpillExportArgs a) {
  const int i = blockIdx.x, g = blockIdx.y, tid = threadIdx.x;
  const long long b = a.seqs[i];
  const int* cnt = a.counters + b * kSpillInts;
  const int nt[2] = {cnt[kSpillTiles], cnt[kSpillTiles + 1]}, np[2] = {cnt[kSpillPoints], cnt[kSpillPoints + 1]};
  if (nt[0] + nt[1] == 0 || !spill_written(a, i)) return;
  for (int cls = 0; cls < 2; ++cls) {
    const aloam_map_tile* row_t = a.tiles + (b * 2 + cls) * a.max_tiles;
    const float4* row_p = a.points + (b * 2 + cls) * a.max_points;
    const long long t0 = a.tile_off[i] + (cls ? nt[0] : 0), p0 = a.point_off[i] + (cls ? np[0] : 0);
    const int n_t = cls ? nt[1] : nt[0], n_p = cls ? np[1] : np[0];
    for (int t = g * 256 + tid; t < n_t; t += kSpillGatherZ * 256) {
      aloam_map_tile tl = row_t[t];
      tl.first_point += p0;
      a.tiles_dst[t0 + t] = tl;
    }
    for (int q = g * 2048; q < n_p; q += kSpillGatherZ * 2048) copy_points(a.points_dst + p0 + q, row_p + q, min(2048, n_p - q));
  }
}

// After the gather, in stream order: the sequences that were written are emptied (their dropped counts stay: they are "so far").
__global__ __launch_bounds__(256) void k_spill_clear(SpillExportArgs a) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= a.n || !spill_written(a, g)) return;
  int* cnt = a.counters + (long long)a.seqs[g] * kSpillInts;
  cnt[kSpillTiles] = 0; cnt[kSpillTiles + 1] = 0; cnt[kSpillPoints] = 0; cnt[kSpillPoints + 1] = 0;
}

// ---- the atlas ---------------------------------------------------------------------------------------------------------------------
// (first, count) of absolute cube (x, y, z) in a class directory; count 0 when the atlas does not hold it.
__device__ __forceinline__ int2 atlas_lookup(const AtlasEntry* dir, int mask, int x, int y, int z) {
  if (!dir || !atlas_in_range(x, y, z)) return make_int2(0, 0);
  const int key = atlas_key(x, y, z);
  for (unsigned h = atlas_hash(key) & (unsigned)mask;; h = (h + 1) & (unsigned)mask) {   // load factor <= 1/2: a free slot ends every probe
    const AtlasEntry e = dir[h];
    if (e.key == key) return make_int2(e.first, e.count);
    if (e.key == -1) return make_int2(0, 0);
  }
}

// aloam_atlas_load: one VoxSeg per cube that several tiles make up, filtered in place with its class's leaf (what the per-cube re-filter,
// src/laserMapping.cpp:788-801, would have made of the concatenation), routed like the segments of k_map_cube_segments.
__global__ void k_atlas_merge_segments(AtlasMergeArgs m, VoxArgs v) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= m.n_jobs) return;
  const AtlasMergeJob j = m.jobs[g];
  VoxSeg s{};
  float4* p = (j.cls ? m.points[1] : m.points[0]) + j.first;
  s.in = p; s.n = j.n; s.final_out = p; s.final_count = m.counts + j.count_slot;
  s.out = v.tmp + j.tmp_off;                               // staging of the in-place filter
  s.leaf = j.cls ? m.leaf[1] : m.leaf[0];
  v.segs[g] = s;
  vox_enlist(v, g, s.n);
}

constexpr int kAtlasPer = (kMapCubes + 1023) / 1024;       // 5 cubes per thread

// The window of an attached sequence, cut from the atlas.  One workgroup of 1024 per sequence, both classes in turn; MapSeq::cen is written
// last, behind a barrier.  Runs right before k_map_begin, which then finds its centre cube inside 3 .. n-4 and shifts nothing.
__global__ __launch_bounds__(1024) void k_atlas_window(AtlasArgs a) {
  const int b = blockIdx.x, tid = threadIdx.x;
  if (seq_idle(a.active, b) || !a.attached[b]) return;
  MapSeq& ms = a.seq[b];
  __shared__ int s_cen[3], s_go, s_scan[1024], s_pref[kMapCubes + 1], s_first[kMapCubes];
  if (tid == 0) {
    int sh[3];
    window_shift(ms, a.odom[b], sh);
    s_go = a.stale[b] != 0 || (sh[0] | sh[1] | sh[2]) != 0;
    for (int k = 0; k < 3; ++k) s_cen[k] = ms.cen[k] + sh[k];
  }
  __syncthreads();
  if (!s_go) return;                                                         // not stale and no shift: the window is the atlas cut already
  const int cen[3] = {s_cen[0], s_cen[1], s_cen[2]};
  auto look = [&](int cls, int c) {
    return atlas_lookup(cls ? a.dir[1] : a.dir[0], cls ? a.dir_mask[1] : a.dir_mask[0], c % kMapW - cen[0], (c / kMapW) % kMapH - cen[1], c / (kMapW * kMapH) - cen[2]);
  };
  int total[2];
  for (int cls = 0; cls < 2; ++cls) {                                        // both totals first: a window that does not fit leaves the sequence untouched
    int sum = 0;
    for (int k = 0; k < kAtlasPer; ++k) { const int c = tid * kAtlasPer + k; if (c < kMapCubes) sum += look(cls, c).y; }
    int t = 0;
    (void)block_exclusive_scan<int, 1024>(sum, s_scan, &t);
    total[cls] = t;
  }
  if (total[0] > a.pool_cap || total[1] > a.pool_cap) { if (tid == 0) ms.err |= kMapErrPool; return; }   // cannot happen after a successful attach
  for (int cls = 0; cls < 2; ++cls) {
    int sum = 0;
    for (int k = 0; k < kAtlasPer; ++k) {                                    // (no per-thread arrays: the counts wait in LDS for their prefix)
      const int c = tid * kAtlasPer + k;
      if (c < kMapCubes) { const int2 e = look(cls, c); s_first[c] = e.x; s_pref[c] = e.y; sum += e.y; }
    }
    int t = 0;
    int run = block_exclusive_scan<int, 1024>(sum, s_scan, &t);
    CubeDesc* T = a.cubes + ((long long)b * 2 + cls) * kMapCubes;
    for (int k = 0; k < kAtlasPer; ++k) {
      const int c = tid * kAtlasPer + k;
      if (c < kMapCubes) {
        const int n = s_pref[c];
        T[c] = CubeDesc{run, n, n, 0};                                       // packed back to back from the start of the pool row
        s_pref[c] = run;
        run += n;
      }
    }
    if (tid == 0) s_pref[kMapCubes] = t;
    __syncthreads();
    float4* dst = (cls ? a.pool[1] : a.pool[0]) + (long long)b * a.pool_cap;
    const float4* src = cls ? a.points[1] : a.points[0];
    auto fetch = [&](int p) { const int c = last_le(s_pref, 0, kMapCubes, p); return src[s_first[c] + (p - s_pref[c])]; };
    int p0 = 0;
    for (; p0 + 4 * 1024 <= t; p0 += 4 * 1024) {                             // four loads of a thread in flight before its stores (named registers)
      const int p = p0 + tid;
      const float4 v0 = fetch(p), v1 = fetch(p + 1024), v2 = fetch(p + 2048), v3 = fetch(p + 3072);
      dst[p] = v0; dst[p + 1024] = v1; dst[p + 2048] = v2; dst[p + 3072] = v3;
    }
    for (int p = p0 + tid; p < t; p += 1024) dst[p] = fetch(p);
    __syncthreads();                                                         // s_pref / s_first are rewritten by the next class
    if (tid == 0) ms.pool_used[cls] = t;
  }
  if (tid == 0) {
    for (int k = 0; k < 3; ++k) ms.cen[k] = cen[k];
    MapGridSig* g = a.grid_sig + (long long)b * 2;
    g[0].valid = 0; g[0].reuse = 0; g[1].valid = 0; g[1].reuse = 0;           // packed offsets can repeat with other points behind them
    a.stale[b] = 0;
  }
}

void launch_atlas_window(const AtlasArgs& a, hipStream_t s) { hipLaunchKernelGGL(k_atlas_window, dim3(a.B), dim3(1024), 0, s, a); }
void launch_atlas_merge_segments(const AtlasMergeArgs& m, const VoxArgs& v, hipStream_t s) {
  if (m.n_jobs > 0) hipLaunchKernelGGL(k_atlas_merge_segments, dim3((m.n_jobs + 255) / 256), dim3(256), 0, s, m, v);
}

void launch_map_spill(const SpillArgs& a, hipStream_t s) { hipLaunchKernelGGL(k_map_spill, dim3(a.B), dim3(256), 0, s, a); }

void launch_spill_count(const SpillExportArgs& a, int* tile_cnt, int* point_cnt, hipStream_t s) {
  if (a.n > 0) hipLaunchKernelGGL(k_spill_count, dim3((a.n + 255) / 256), dim3(256), 0, s, a, tile_cnt, point_cnt);
}

void launch_spill_gather(const SpillExportArgs& a, bool clear, hipStream_t s) {
  if (a.n <= 0) return;
  if (a.tiles_dst) hipLaunchKernelGGL(k_spill_gather, dim3(a.n, kSpillGatherZ), dim3(256), 0, s, a);
  if (clear) hipLaunchKernelGGL(k_spill_clear, dim3((a.n + 255) / 256), dim3(256), 0, s, a);
}

}  // namespace aloam
