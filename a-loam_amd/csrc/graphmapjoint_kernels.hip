// a-loam_amd/csrc/graphmapjoint_kernels.hip — gfx950 kernels of the map of joined sequences (aloam_graph_export_map_joint, DESIGN.md
// §7za).  A translation unit of its own, so that the kernels of graphmap_kernels.hip are compiled exactly as before.
//   k_graph_map_transform_parts  one wave per piece of kGmPiece points of a (part, class): the node's pose, composed with the part's frame
//                                where it names one (once per node change, f64, separately rounded, nothing renormalised), then what
//                                k_graph_map_transform does - associate_to_map, cube_coord, one directory entry per distinct cube in the
//                                wave under the key (group, class, cube, the part's piece base + piece), integer counts, `outside` per group
//   k_graph_map_group_parts      the same waves again, in the same order: a point's place is its entry's base (host: the entries sorted by
//                                group, class, cube, piece, scanned) + the entry's cursor, which only this wave advances, + its rank in
//                                the wave.  A cube's members stand in part order, then node order, then point order, by construction
// No float atomic, no position that depends on which wave ran first.  Integer work and 16-byte point copies: HBM- and latency-bound, no
// MFMA.  All stores are plain vector stores.
#include "graphmapjoint_kernels.hpp"

#include "export_kernels.hpp"                // last_le
#include "map_search_device.hpp"             // quat_mul, quat_rotate, associate_to_map
#include "map_window_device.hpp"             // cube_coord

namespace aloam {

namespace {
// (selects, not indexed copies: a private array indexed at run time costs the kernel LDS or scratch)
__device__ __forceinline__ int kf_first(const KfDesc& d, int cls) { return cls ? d.first[1] : d.first[0]; }
__device__ __forceinline__ int kf_end(const KfDesc& d, int cls) { return cls ? d.first[1] + d.count[1] : d.first[0] + d.count[0]; }
__device__ __forceinline__ const float4* kf_row(const KfStore& k, int cls, long long seq) { return cls ? k.points[1] + seq * k.cap[1] : k.points[0] + seq * k.cap[0]; }

struct GmPartPiece { int cls, piece, base, p0, p1; };

// Which piece wave w works on: false when the host's bound laid out more pieces than the part has points for.
__device__ __forceinline__ bool gm_part_piece(const GmPartsArgs& a, int w, GmPart* pt, GmPartPiece* pc) {
  const int g = last_le(a.piece_first, 0, 2 * a.n_parts, w);
  pc->cls = g & 1; pc->piece = w - a.piece_first[g];
  *pt = a.parts[g >> 1];
  if (pt->count == 0) return false;
  const KfDesc* D = a.kf.desc + (long long)pt->seq * a.kf.max_nodes + pt->first;
  const KfDesc d0 = D[0], d1 = D[pt->count - 1];
  pc->base = kf_first(d0, pc->cls);
  const int n = kf_end(d1, pc->cls) - pc->base;
  pc->p0 = pc->piece * kGmPiece; pc->p1 = min(n, pc->p0 + kGmPiece);
  return pc->p0 < pc->p1;
}

__device__ __forceinline__ unsigned gm_hash(unsigned long long k) { return (unsigned)((k * 0x9E3779B97F4A7C15ull) >> 32); }

}  // namespace

__global__ __launch_bounds__(256) void k_graph_map_transform_parts(GmPartsArgs a) {
  const int lane = threadIdx.x & 63, w = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // (the wave's index, in a scalar register: the part and the piece are then scalar loads)
  if (w >= a.n_pieces) return;
  GmPart pt; GmPartPiece pc;
  if (!gm_part_piece(a, w, &pt, &pc)) return;                                // (uniform in the wave)
  const int cls = pc.cls;
  const KfDesc* D = a.kf.desc + (long long)pt.seq * a.kf.max_nodes + pt.first;
  const aloam_graph_node* N = a.nodes + (long long)pt.seq * a.max_nodes + pt.first;
  const float4* src = kf_row(a.kf, cls, pt.seq) + pc.base;
  const long long at0 = cls ? pt.at[1] : pt.at[0];
  const int dir_piece = (cls ? pt.piece_base[1] : pt.piece_base[0]) + pc.piece;
  float4* world = a.world + at0;
  int* slot = a.slot + at0;
  int nd = 0, nd_end = -1, n_out = 0;
  double par[7] = {0, 0, 0, 1, 0, 0, 0};
  for (int p = pc.p0 + lane; p - lane < pc.p1; p += 64) {
    const bool live = p < pc.p1;
    int key = -1;
    if (live) {
      const int at = pc.base + p;
      if (at >= nd_end) {                                                    // the node that holds row index `at`: the last one that starts at or before it
        int lo = nd, hi = pt.count;
        while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (kf_first(D[mid], cls) <= at) lo = mid; else hi = mid; }
        nd = lo; nd_end = kf_end(D[nd], cls);
        const aloam_graph_node& x = N[nd];
#pragma unroll
        for (int k = 0; k < 4; ++k) par[k] = pt.pose ? x.q_opt[k] : x.q[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) par[4 + k] = pt.pose ? x.t_opt[k] : x.t[k];
        if (pt.frame >= 0) {                                                 // X_k' = A o X_k = (quat_mul(q_A, q_k), quat_rotate(q_A, t_k) + t_A)
          const double* A = a.frames + 7 * (long long)pt.frame;
          const double qa[4] = {A[0], A[1], A[2], A[3]};
          double qo[4], to[3];
          quat_mul(qa, par, qo);
          quat_rotate(qa, par[4], par[5], par[6], to);
#pragma unroll
          for (int k = 0; k < 4; ++k) par[k] = qo[k];
#pragma unroll
          for (int k = 0; k < 3; ++k) par[4 + k] = to[k] + A[4 + k];
        }
      }
      const float4 v = associate_to_map(src[p], par);
      const int cx = cube_coord((double)v.x, 0), cy = cube_coord((double)v.y, 0), cz = cube_coord((double)v.z, 0);
      if (atlas_in_range(cx, cy, cz)) key = atlas_key(cx, cy, cz);
      world[p] = v;
    }
    // a sweep's points fall into about a dozen cubes: one directory look-up and one count per distinct cube in the wave
    int mine = -1;
    unsigned long long todo = __ballot(key >= 0);
    while (todo) {
      const int leader = __ffsll((long long)todo) - 1;
      const int c = __shfl(key, leader, 64);
      const unsigned long long same = __ballot(key == c);
      int s = -1;
      if (lane == leader) {
        const unsigned long long k64 = gm_dir_key(2 * pt.group + cls, c, dir_piece);
        unsigned h = gm_hash(k64) & a.dir_mask;
        for (unsigned probe = 0; probe <= a.dir_mask; ++probe, h = (h + 1) & a.dir_mask) {
          const unsigned long long old = atomicCAS(&a.dir_key[h], kGmEmpty, k64);
          if (old == kGmEmpty || old == k64) { s = (int)h; break; }
        }
        if (s >= 0) atomicAdd(&a.dir_count[s], __popcll(same)); else atomicOr(&a.flags[0], 1);
      }
      s = __shfl(s, leader, 64);
      if (key == c) mine = s;
      todo &= ~same;
    }
    n_out += __popcll(__ballot(live && key < 0));
    if (live) slot[p] = mine;
  }
  if (lane == 0 && n_out) atomicAdd(&a.outside[pt.group], n_out);
}

__global__ __launch_bounds__(256) void k_graph_map_group_parts(GmPartsArgs a) {
  const int lane = threadIdx.x & 63, w = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= a.n_pieces) return;
  GmPart pt; GmPartPiece pc;
  if (!gm_part_piece(a, w, &pt, &pc)) return;
  const long long at0 = pc.cls ? pt.at[1] : pt.at[0];
  const float4* world = a.world + at0;
  const int* slot = a.slot + at0;
  for (int p = pc.p0 + lane; p - lane < pc.p1; p += 64) {
    const bool live = p < pc.p1;
    const int s = live ? slot[p] : -1;
    const float4 v = live ? world[p] : make_float4(0.f, 0.f, 0.f, 0.f);
    unsigned long long todo = __ballot(s >= 0);
    while (todo) {
      const int leader = __ffsll((long long)todo) - 1;
      const int c = __shfl(s, leader, 64);
      const unsigned long long same = __ballot(s == c);
      int old = 0;
      if (lane == leader) old = atomicAdd(&a.dir_count[c], __popcll(same));  // this entry belongs to this wave alone: its pieces before, in order
      old = __shfl(old, leader, 64);
      if (s == c) a.grouped[a.dir_base[c] + old + __popcll(same & ((1ull << lane) - 1ull))] = v;
      todo &= ~same;
    }
  }
}

void launch_graph_map_transform_parts(const GmPartsArgs& a, hipStream_t s) {
  if (a.n_pieces > 0) hipLaunchKernelGGL(k_graph_map_transform_parts, dim3((a.n_pieces + 3) / 4), dim3(256), 0, s, a);
}
void launch_graph_map_group_parts(const GmPartsArgs& a, hipStream_t s) {
  if (a.n_pieces > 0) hipLaunchKernelGGL(k_graph_map_group_parts, dim3((a.n_pieces + 3) / 4), dim3(256), 0, s, a);
}

}  // namespace aloam
