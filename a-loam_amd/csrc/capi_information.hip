// a-loam_amd/csrc/capi_information.hip — host side of aloam_export_pose_information (the information matrix of the last odometry / mapping
// solve of the listed sequences, in stream order) and of its parity getter aloam_get_map_factors.
#include <algorithm>
#include <vector>

#include "capi_internal.hpp"
#include "information_device.hpp"

extern "C" {

int aloam_export_pose_information(aloam_ctx* c, int which, const int* seqs, int n, aloam_pose_information* dst) {
  DeviceScope device_scope(c);
  if (!c) return ALOAM_E_ARG;
  if (which != ALOAM_INFO_ODOMETRY && which != ALOAM_INFO_MAPPING) { c->err = "which must be ALOAM_INFO_ODOMETRY or ALOAM_INFO_MAPPING"; return ALOAM_E_ARG; }
  if (const int rc = check_ids(c, seqs, n)) return rc;
  if (const int rc = require_stage(c, which == ALOAM_INFO_ODOMETRY ? ALOAM_STAGE_ODOMETRY : ALOAM_STAGE_MAPPING)) return rc;
  if (which == ALOAM_INFO_MAPPING && !c->map_on) { c->err = "ALOAM_INFO_MAPPING before aloam_mapping_enable"; return ALOAM_E_STATE; }
  void* d = nullptr;
  if (n > 0) if (const int rc = export_target(c, dst, alignof(aloam_pose_information), "dst", &d)) return rc;
  if (n == 0) return ALOAM_OK;
  if (!c->d_info_list) HIP_TRY(c, dalloc(c->d_info_list, (size_t)c->B));
  std::vector<int> list(n);
  for (int i = 0; i < n; ++i) {
    const SeqHost& s = c->seq[seqs[i]];
    list[i] = seqs[i] | ((which == ALOAM_INFO_ODOMETRY ? s.info_odom : s.info_map) ? kInfoSolvedBit : 0);
  }
  if (const int rc = stage_ints(c, list.data(), n, c->d_info_list.get())) return rc;
  {
    ProfScope p(c, K_POSE_INFO);
    if (which == ALOAM_INFO_ODOMETRY) launch_pose_information_odom(odom_args(c), c->d_info_list.get(), n, static_cast<aloam_pose_information*>(d), c->stream);
    else launch_pose_information_map(map_args(c), c->d_info_list.get(), n, static_cast<aloam_pose_information*>(d), c->stream);
  }
  HIP_TRY(c, hipGetLastError());
  c->info_last_which = which;
  c->info_last_list = std::move(list);
  return ALOAM_OK;
}

// The records k_map_solve read in its second iteration, as map_evaluate visits them: per class the tiles of 256 stack points in order, and in a
// tile the first rec_tiles[tile] slots.
int aloam_get_map_factors(aloam_ctx* c, int seq, double* lines, int cap_lines, int* n_lines, double* planes, int cap_planes, int* n_planes) {
  DeviceScope device_scope(c);
  int rc = check_seq(c, seq);
  if (rc) return rc;
  if (!c->map_on) { c->err = "mapping not enabled"; return ALOAM_E_STATE; }
  if (!n_lines || !n_planes || cap_lines < 0 || cap_planes < 0 || (cap_lines && !lines) || (cap_planes && !planes)) return ALOAM_E_ARG;
  MapSeq ms;
  if ((rc = read_seq(c, c->d_mapseq.get() + seq, &ms))) return rc;
  *n_lines = 0; *n_planes = 0;
  if (!ms.gate) return ALOAM_OK;
  const int nt0 = (ms.n_stack[0] + 255) >> 8, nt1 = (ms.n_stack[1] + 255) >> 8;
  std::vector<int> tiles(c->rec_tiles_per_seq > 0 ? c->rec_tiles_per_seq : 1);
  HIP_TRY(c, hipMemcpy(tiles.data(), c->d_rec_tiles.get() + (size_t)seq * c->rec_tiles_per_seq, sizeof(int) * c->rec_tiles_per_seq, hipMemcpyDeviceToHost));
  std::vector<MapEdgeRec> E(ms.n_stack[0] > 0 ? nt0 * 256 : 1);
  std::vector<MapNormRec> P(ms.n_stack[1] > 0 ? nt1 * 256 : 1);
  // (the last tile may reach past the end of the sequence's row: read up to the row's end only)
  const size_t row0 = (size_t)c->R * kLessSharpPerRing, row1 = (size_t)c->cap;
  const size_t take0 = std::min(row0, (size_t)nt0 * 256), take1 = std::min(row1, (size_t)nt1 * 256);
  if (take0) HIP_TRY(c, hipMemcpy(E.data(), c->d_medges.get() + (size_t)seq * row0, sizeof(MapEdgeRec) * take0, hipMemcpyDeviceToHost));
  if (take1) HIP_TRY(c, hipMemcpy(P.data(), c->d_mnorms.get() + (size_t)seq * row1, sizeof(MapNormRec) * take1, hipMemcpyDeviceToHost));
  int ne = 0, np = 0;
  for (int tile = 0; tile < nt0; ++tile)
    for (int k = 0; k < tiles[tile]; ++k, ++ne) {
      if (ne >= cap_lines) continue;
      const MapEdgeRec& e = E[(size_t)tile * 256 + k];
      double* o = lines + (size_t)ne * 9;
      for (int j = 0; j < 3; ++j) { o[j] = e.cp[j]; o[3 + j] = e.a[j]; o[6 + j] = e.b[j]; }
    }
  for (int tile = 0; tile < nt1; ++tile)
    for (int k = 0; k < tiles[c->rec_tiles_corner + tile]; ++k, ++np) {
      if (np >= cap_planes) continue;
      const MapNormRec& e = P[(size_t)tile * 256 + k];
      double* o = planes + (size_t)np * 7;
      for (int j = 0; j < 3; ++j) { o[j] = e.cp[j]; o[3 + j] = e.n[j]; }
      o[6] = e.d;
    }
  *n_lines = ne; *n_planes = np;
  return ALOAM_OK;
}

}  // extern "C"
