// a-loam_amd/csrc/capi_graphmapjoint.hip — host side of the map of joined sequences (aloam_graph_export_map_joint): one
// map per group of parts, a part being a node range of any sequence under an optional frame.  The entry checks the lists, lays out the
// piece table per (part, class) and numbers every part's pieces inside its (group, class); everything behind that - the directory, the
// one synchronisation, the segments, the rounds of the voxel filter, the emit - is graph_map_run of capi_graphmap.hip, which
// aloam_graph_export_map calls too.  Nothing about joins is stored: the caller says which ranges make a map.
#include <algorithm>
#include <cmath>

#include "capi_internal.hpp"

extern "C" {

int aloam_graph_export_map_joint(aloam_ctx* c, const aloam_graph_map_part* parts, int n_parts, const double* frames, int n_frames,
                                 const aloam_graph_map_group* groups, int n_groups, aloam_map_tile* tiles_dst, long long cap_tiles,
                                 float* points_dst_xyzw, long long cap_points, long long* dst_offsets, aloam_graph_map_stats* stats_dst) {
  DeviceScope device_scope(c);
  if (!c) return ALOAM_E_ARG;
  if (const int rc = require_keyframes(c)) return rc;
  // ---- everything is checked before anything is queued
  if (n_groups < 0 || n_groups > kGmMaxRequests || (n_groups > 0 && !groups)) { c->err = "bad group list (0 <= n_groups <= 32768)"; return ALOAM_E_ARG; }
  if (n_parts < 0 || (n_parts > 0 && !parts)) { c->err = "bad part list (n_parts >= 0, parts not NULL)"; return ALOAM_E_ARG; }
  if (n_frames < 0 || (n_frames > 0 && !frames)) { c->err = "bad frame list (n_frames >= 0, frames not NULL)"; return ALOAM_E_ARG; }
  if (n_groups > 0) if (const int rc = require_host_list(c, groups, "groups")) return rc;
  if (n_parts > 0) if (const int rc = require_host_list(c, parts, "parts")) return rc;
  if (n_frames > 0) if (const int rc = require_host_list(c, frames, "frames")) return rc;
  for (int f = 0; f < n_frames; ++f) {
    auto fail = [&](const char* what) { c->err = "frames[" + std::to_string(f) + "]: " + what; return ALOAM_E_ARG; };
    const double* A = frames + 7 * (size_t)f;
    double nn = 0.0;
    for (int a = 0; a < 4; ++a) { if (!std::isfinite(A[a])) return fail("q is not finite"); nn += A[a] * A[a]; }
    if (!(std::fabs(std::sqrt(nn) - 1.0) <= 1e-6)) return fail("q is not within 1e-6 of unit norm");
    for (int a = 4; a < 7; ++a) if (!std::isfinite(A[a])) return fail("t is not finite");
  }
  for (int p = 0; p < n_parts; ++p) {
    const aloam_graph_map_part& q = parts[p];
    auto fail = [&](const char* what) { c->err = "part " + std::to_string(p) + ": " + what; return ALOAM_E_ARG; };
    if (q.seq < 0 || q.seq >= c->B) return fail("seq out of range");
    if (q.first < 0 || q.count < 0 || q.first + (long long)q.count > c->seq[q.seq].graph_nodes) return fail("[first, first + count) must lie inside what the sequence's graph holds");
    if (q.frame < -1 || q.frame >= n_frames) return fail("frame must be -1 or an index into frames");
  }
  {
    long long next = 0;
    for (int g = 0; g < n_groups; ++g) {
      const aloam_graph_map_group& q = groups[g];
      auto fail = [&](const char* what) { c->err = "group " + std::to_string(g) + ": " + what; return ALOAM_E_ARG; };
      if (q.part_count < 0) return fail("part_count is negative");
      if (q.part_first != next) return fail("part_first: the groups must tile parts contiguously and in order");
      if (q.pose != ALOAM_GRAPH_POSE_ENTERED && q.pose != ALOAM_GRAPH_POSE_OPTIMIZED) return fail("pose must be ALOAM_GRAPH_POSE_ENTERED or ALOAM_GRAPH_POSE_OPTIMIZED");
      if (q.pad != 0) return fail("pad must be 0");
      next += q.part_count;
      if (next > n_parts) return fail("part_first + part_count exceeds n_parts");
    }
    if (next != n_parts) { c->err = "n_parts: the groups must tile parts contiguously and in order (parts are left over)"; return ALOAM_E_ARG; }
  }
  if (cap_tiles < 0 || cap_points < 0) { c->err = "negative cap_tiles / cap_points"; return ALOAM_E_ARG; }
  void *d_off = nullptr, *d_tiles = nullptr, *d_pts = nullptr, *d_stats = nullptr;
  if (const int rc = export_target(c, dst_offsets, alignof(long long), "dst_offsets", &d_off)) return rc;
  if ((tiles_dst || cap_tiles > 0) && export_target(c, tiles_dst, alignof(aloam_map_tile), "tiles_dst", &d_tiles)) return ALOAM_E_ARG;
  if ((points_dst_xyzw || cap_points > 0) && export_target(c, points_dst_xyzw, 16, "points_dst", &d_pts)) return ALOAM_E_ARG;
  if (stats_dst && export_target(c, stats_dst, alignof(aloam_graph_map_stats), "stats_dst", &d_stats)) return ALOAM_E_ARG;
  // ---- lay out the transform: what a (part, class) can hold at most is known without asking the device; a part's pieces are numbered
  //      on from those of the parts before it in its (group, class), so that the directory's order is the members' order
  const int n = n_groups;
  std::vector<GmPart> pt((size_t)std::max(n_parts, 1));
  std::vector<int> piece_first(2 * (size_t)n_parts + 1, 0);
  long long bound_points = 0;
  int n_pieces = 0;
  const long long row[2] = {(long long)c->R * kLessSharpPerRing, (long long)c->cap};
  for (int g = 0; g < n; ++g) {
    long long in_group[2] = {0, 0};
    for (int p = groups[g].part_first; p < groups[g].part_first + groups[g].part_count; ++p) {
      pt[p] = GmPart{parts[p].seq, parts[p].first, parts[p].count, parts[p].frame, g, groups[g].pose, {0, 0}, {0, 0}};
      for (int cls = 0; cls < 2; ++cls) {
        const long long bound = std::min<long long>(c->kf.cap[cls], row[cls] * parts[p].count);
        const long long pieces = (bound + kGmPiece - 1) / kGmPiece;
        pt[p].at[cls] = bound_points;
        pt[p].piece_base[cls] = (int)in_group[cls];
        piece_first[2 * p + cls] = n_pieces;
        bound_points += bound;
        in_group[cls] += pieces;
        if (in_group[cls] > kGmPieceIndexMax) {
          c->err = "group " + std::to_string(g) + ": its " + (cls ? "surf" : "corner") + " ranges are bounded by more than 65536 pieces of 4096 points: export fewer parts per group";
          return ALOAM_E_CAPACITY;
        }
        n_pieces += (int)pieces;
        if (n_pieces > (1 << 28)) { c->err = "the parts cover more than 2^40 keyframe points"; return ALOAM_E_ARG; }
      }
    }
  }
  piece_first[2 * (size_t)n_parts] = n_pieces;
  int rc;
  if ((rc = graph_map_scratch(c, bound_points))) return rc;
  if ((rc = c->gm.parts.grow(c, (long long)std::max(n_parts, 1)))) return rc;
  if ((rc = c->gm.frames.grow(c, 7LL * std::max(n_frames, 1)))) return rc;
  if ((rc = c->gm.req_out.grow(c, (long long)n + 1))) return rc;
  if ((rc = c->gm.ints.grow(c, 2LL * n_parts + n + 2))) return rc;   // piece_first [2 n_parts + 1], outside [n], flags [1]
  int* d_piece_first = c->gm.ints.get();
  int* d_outside = d_piece_first + 2 * (size_t)n_parts + 1;
  int* d_flags = d_outside + n;
  if (n_parts > 0) HIP_TRY(c, hipMemcpyAsync(c->gm.parts.get(), pt.data(), sizeof(GmPart) * (size_t)n_parts, hipMemcpyHostToDevice, c->stream));
  if (n_frames > 0) HIP_TRY(c, hipMemcpyAsync(c->gm.frames.get(), frames, sizeof(double) * 7 * (size_t)n_frames, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(d_piece_first, piece_first.data(), sizeof(int) * piece_first.size(), hipMemcpyHostToDevice, c->stream));
  c->gm.last_segs = -1;                                    // the scratch of the last call's algorithmic bytes is about to be reused
  GmPartsArgs g{};
  GmPasses passes;
  passes.transform = [&](unsigned dir_mask) {
    g = GmPartsArgs{};
    g.n_parts = n_parts; g.n_groups = n; g.parts = c->gm.parts.get(); g.frames = n_frames > 0 ? c->gm.frames.get() : nullptr;
    g.piece_first = d_piece_first; g.n_pieces = n_pieces; g.kf = kf_store(c);
    g.nodes = c->pg.nodes.get(); g.max_nodes = c->pg.max_nodes;
    g.world = c->gm.world.get(); g.slot = c->gm.slot.get(); g.grouped = c->gm.grouped.get();
    g.dir_key = c->gm.dir_key.get(); g.dir_count = c->gm.dir_count.get(); g.dir_base = c->gm.dir_base.get(); g.dir_mask = dir_mask;
    g.outside = d_outside; g.flags = d_flags;
    launch_graph_map_transform_parts(g, c->stream);
  };
  passes.group = [&] { launch_graph_map_group_parts(g, c->stream); };
  GmDst dst{d_tiles, cap_tiles, d_pts, cap_points, d_off, d_stats};
  return graph_map_run(c, n, n_pieces, d_outside, d_flags, passes, dst, "group");
}

}  // extern "C"
