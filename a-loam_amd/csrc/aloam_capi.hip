// a-loam_amd/csrc/aloam_capi.hip — host side of libaloam_mi355x.so: context creation and teardown, the pinned staging ring, per-sequence
// lifecycle and profiling.  The other entry points of include/aloam_mi355x.h are in the other capi_*.hip files
// (what they share, and which file holds what: capi_internal.hpp).  There is no CPU fallback anywhere: without a HIP device every entry point fails with ALOAM_E_HIP.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "capi_internal.hpp"
#include "information_device.hpp"

namespace aloam {

hipEvent_t prof_event(aloam_ctx* c) {
  if (!c->prof_free.empty()) { hipEvent_t e = c->prof_free.back(); c->prof_free.pop_back(); return e; }
  Event e;
  (void)hipEventCreate(&e.h);
  c->prof_events.push_back(std::move(e));
  return c->prof_events.back();
}

// n ints to device memory through the pinned ring c->nin: returns at once, the H2D copy runs in stream order.
int stage_ints(aloam_ctx* c, const int* src, int n, int* dst) {
  int* slot = nullptr;
  int ns = 0;
  if (const int rc = c->nin.acquire(c, &slot, &ns)) return rc;
  std::memcpy(slot, src, sizeof(int) * n);
  return c->nin.queue(c, ns, slot, sizeof(int) * n, dst, c->stream);
}

int check_seq(aloam_ctx* c, int seq) {
  if (!c) return ALOAM_E_ARG;
  if (seq < 0 || seq >= c->B) { c->err = "sequence index out of range"; return ALOAM_E_ARG; }
  return ALOAM_OK;
}

int require_stage(aloam_ctx* c, int stage) {
  if (c->stages & stage) return ALOAM_OK;
  c->err = std::string("this context was created without ") +
           (stage == ALOAM_STAGE_REGISTRATION ? "ALOAM_STAGE_REGISTRATION" : stage == ALOAM_STAGE_ODOMETRY ? "ALOAM_STAGE_ODOMETRY" : "ALOAM_STAGE_MAPPING");
  return ALOAM_E_STATE;
}

// n distinct ids in 0 .. B-1 (sequences of a reset or a save, slots of a load).
int check_ids(aloam_ctx* c, const int* ids, int n) {
  if (n < 0 || n > c->B || (n > 0 && !ids)) { c->err = "bad sequence list"; return ALOAM_E_ARG; }
  std::vector<char> seen(c->B, 0);
  for (int i = 0; i < n; ++i) {
    if (ids[i] < 0 || ids[i] >= c->B || seen[ids[i]]) { c->err = "sequence index out of range or repeated"; return ALOAM_E_ARG; }
    seen[ids[i]] = 1;
  }
  return ALOAM_OK;
}

}  // namespace aloam

namespace {

void prof_resolve(aloam_ctx* c) {
  for (ProfRec& r : c->prof_pending) {
    float ms = 0.f;
    (void)hipEventSynchronize(r.e1);
    (void)hipEventElapsedTime(&ms, r.e0, r.e1);
    c->prof_ms[r.kernel] += ms;
    c->prof_launches[r.kernel] += 1;
    c->prof_free.push_back(r.e0);
    c->prof_free.push_back(r.e1);
  }
  c->prof_pending.clear();
}

}  // namespace

extern "C" {

void aloam_default_config(aloam_config* cfg) {
  cfg->n_scans = 64;            // launch/aloam_velodyne_HDL_64.launch: scan_line
  cfg->min_range = 5.0f;        // launch/aloam_velodyne_HDL_64.launch: minimum_range
  cfg->ring_from_field = 0;
  cfg->batch = 1;
  cfg->max_points = 140000;
  cfg->max_ring_points = 4107;
  cfg->device = 0;
  cfg->lm_max_iterations = 4;
  cfg->outer_iterations = 2;
  cfg->distortion = 0;
}

int aloam_create(const aloam_config* cfg, aloam_ctx** out) { return aloam_create_stages(cfg, ALOAM_STAGE_ALL, out); }

int aloam_create_stages(const aloam_config* cfg, int stages, aloam_ctx** out) {
  if (!cfg || !out) return ALOAM_E_ARG;
  *out = nullptr;
  aloam_ctx* c = new aloam_ctx();
  c->cfg = *cfg;
  c->stages = stages;
  { const char* e = std::getenv("ALOAM_DEBUG_SYNC"); c->debug_sync = e && e[0] == '1'; }
  *out = c;   // returned even on failure so that aloam_last_error() works; caller destroys it
  if ((stages & ~ALOAM_STAGE_ALL) || !(stages & ALOAM_STAGE_ALL)) { c->err = "stages must be a non-empty combination of ALOAM_STAGE_*"; return ALOAM_E_ARG; }
  if (cfg->batch < 1 || cfg->max_points < 32 || cfg->max_points > 400000 || cfg->lm_max_iterations < 0 || cfg->outer_iterations < 1 ||
      cfg->outer_iterations > 64) { c->err = "bad configuration value"; return ALOAM_E_ARG; }
  if (!cfg->ring_from_field && cfg->n_scans != 16 && cfg->n_scans != 32 && cfg->n_scans != 64) {
    c->err = "only support velodyne with 16, 32 or 64 scan line (or ring_from_field)";   // src/scanRegistration.cpp:472-476
    return ALOAM_E_SCAN_LINES;
  }
  if (cfg->n_scans < 1 || cfg->n_scans > kMaxRings) { c->err = "n_scans out of range"; return ALOAM_E_ARG; }
  if (cfg->max_ring_points < 17 || cfg->max_ring_points > 4107) { c->err = "max_ring_points must be in [17, 4107]"; return ALOAM_E_ARG; }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { c->err = "no HIP device available (this library has no CPU fallback)"; return ALOAM_E_HIP; }
  if (cfg->device < 0 || cfg->device >= ndev) { c->err = "device ordinal out of range"; return ALOAM_E_ARG; }
  DeviceScope device_scope(c);                      // the caller's current device is restored on every return path
  HIP_TRY(c, hipStreamCreateWithFlags(&c->stream.h, hipStreamNonBlocking));
  HIP_TRY(c, hipStreamCreateWithFlags(&c->copy_stream.h, hipStreamNonBlocking));
  for (int k = 0; k < 2; ++k) {
    HIP_TRY(c, hipEventCreateWithFlags(&c->in_copied[k].h, hipEventDisableTiming));
    HIP_TRY(c, hipEventCreateWithFlags(&c->in_consumed[k].h, hipEventDisableTiming));
  }
  c->B = cfg->batch; c->max_points = cfg->max_points; c->R = cfg->n_scans;
  c->seq.assign(c->B, SeqHost{});
  // The per-sequence stride of every [B][cap] buffer is kept OFF the powers of two (131 072 points x 16 B = 2 MiB apart, the workgroups of a launch - one
  // per sequence, all at about the same offset of their sequence - meet on the same memory channels): + 1/32 + 16 points.  Measured on k_build_grids_fused at
  // batch 1024, one box: 1.62 - 1.65 ms at the power-of-two stride, 1.48 - 1.52 ms with 1040 / 4112 / 16 400 points of padding.
  c->cap = cfg->max_points + (((cfg->max_points / 32 + 15) & ~15) + 16);
  { const char* e = std::getenv("ALOAM_GRAPH_MAX_BATCH"); c->use_graph = c->B <= (e ? std::atoi(e) : 0); }   // off unless asked for: measured no gain (below)
  // The next step's search grids are built beside the association and the solve (aloam_odometry_step) unless ALOAM_GRID_OVERLAP=0 asks for the serial
  // build at the start of every step; a captured step stays a single chain, and a step that waits after every stage has nothing to run beside.
  { const char* e = std::getenv("ALOAM_GRID_OVERLAP"); c->grid_overlap = !(e && e[0] == '0') && !c->use_graph && !c->debug_sync; }
  // k_solve reads its factor records from global memory once per solve and from LDS after that unless ALOAM_SOLVE_STAGE=0 asks for global memory in every pass
  // (same results bit for bit; the switch is there to measure and to test one against the other).
  { const char* e = std::getenv("ALOAM_SOLVE_STAGE"); c->solve_stage = !(e && e[0] == '0'); }
  c->NB = (c->cap + kBlockPts - 1) / kBlockPts;
  c->npad = cfg->max_ring_points <= 2059 ? 2048 : 4096;
  const size_t B = c->B, cap = c->cap, R = c->R, NB = c->NB;
  int rc = 0;
  if (const char* what = c->nin.create(sizeof(int) * B)) { c->err = std::string("input counts, ") + what; return ALOAM_E_HIP; }
  const bool reg = stages & ALOAM_STAGE_REGISTRATION, odo = stages & ALOAM_STAGE_ODOMETRY, map = stages & ALOAM_STAGE_MAPPING;
  // hash tables of the correspondence search sized by the clouds they index (power of two; the surf table must fit k_build_grids' LDS)
  c->grid_H[0] = R > 64 ? 8192 : 4096;
  c->grid_H[1] = c->max_points > 160000 ? 32768 : 16384;
  if ((rc = dmalloc(c, c->d_nin, B))) return rc;
  if ((rc = dmalloc(c, c->d_meta, B))) return rc;
  if ((rc = dmalloc(c, c->d_state, B))) return rc;
  if ((rc = dmalloc(c, c->d_cloud, B * cap))) return rc;                    // /velodyne_cloud_2 -> _3 -> mapping's full-resolution input
  if ((rc = dmalloc(c, c->d_exp_cnt, B * ALOAM_EXPORT_MAX_IDS))) return rc;
  if ((rc = dmalloc(c, c->d_exp_chunk, B * ALOAM_EXPORT_MAX_IDS + 1))) return rc;
  if ((rc = dmalloc(c, c->d_exp_off, B * ALOAM_EXPORT_MAX_IDS + 1))) return rc;
  { int cus = 0; if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, cfg->device) == hipSuccess && cus > 0) c->gather_blocks = 8 * cus; }
  if (reg) {                                                                 // working set of scan registration
    c->slab = c->npad + 16;                                                  // >= the longest ring k_ring_features accepts (npad + 11)
    if ((rc = dmalloc(c, c->d_slabs, B * R * (size_t)c->slab))) return rc;
    if ((rc = dmalloc(c, c->d_front_lb, B * NB * (size_t)kFrontSlots))) return rc;
    if ((rc = dmalloc(c, c->d_front_ticket, B))) return rc;
    if ((rc = dmalloc(c, c->d_ringstart, B * (R + 1)))) return rc;
    if ((rc = dmalloc(c, c->d_curv, B * cap))) return rc;
    if ((rc = dmalloc(c, c->d_label, B * cap))) return rc;
    if ((rc = dmalloc(c, c->d_lookback, B * 4 * R))) return rc;
    if ((rc = dmalloc(c, c->d_ring_ticket, B))) return rc;
  }
  if (reg || odo) {
    if ((rc = dmalloc(c, c->d_sharp, B * R * kSharpPerRing))) return rc;
    if ((rc = dmalloc(c, c->d_flat, B * R * kFlatPerRing))) return rc;
  }
  for (int k = 0; k < 2; ++k) {
    // [cur = 0] receives the sweep being registered, [1] is what a mapping-only context is handed as the "last" clouds; odometry flips between both
    if (!(odo || (k == 0 && reg) || (k == 1 && map))) continue;
    if ((rc = dmalloc(c, c->d_less_sharp[k], B * R * kLessSharpPerRing))) return rc;
    if ((rc = dmalloc(c, c->d_less_flat[k], B * cap))) return rc;
  }
  if (odo) {
    for (int p = 0; p < 2; ++p) for (int k = 0; k < 2; ++k) {       // one set of grids per cloud buffer
      const size_t per = k == 0 ? R * kLessSharpPerRing : cap;
      if ((rc = dmalloc(c, c->d_grid_sorted3[p][k], B * per))) return rc;
      if ((rc = dmalloc(c, c->d_grid_sorted2[p][k], B * per))) return rc;
      if ((rc = dmalloc(c, c->d_grid_start3[p][k], B * (c->grid_H[k] + 1)))) return rc;
      if ((rc = dmalloc(c, c->d_grid_start2[p][k], B * (c->grid_H[k] + 1)))) return rc;
      if ((rc = dmalloc(c, c->d_grid_sorted3c[p][k], B * per))) return rc;
      if ((rc = dmalloc(c, c->d_grid_start3c[p][k], B * (c->grid_H[k] + 1)))) return rc;
      if ((rc = dmalloc(c, c->d_grid_flags[p][k], B * 4))) return rc;
      if ((rc = dmalloc(c, c->d_grid_walk[p][k], B * 2 * (R + 8)))) return rc;
    }
    if (c->grid_overlap) {
      HIP_TRY(c, hipStreamCreateWithFlags(&c->grid_stream.h, hipStreamNonBlocking));
      HIP_TRY(c, hipEventCreateWithFlags(&c->grid_fork.h, hipEventDisableTiming));
      HIP_TRY(c, hipEventCreateWithFlags(&c->grids_done.h, hipEventDisableTiming));
    }
    if ((rc = dmalloc(c, c->d_edges, B * R * kSharpPerRing))) return rc;
    if ((rc = dmalloc(c, c->d_planes, B * R * kFlatPerRing))) return rc;
    if ((rc = dmalloc(c, c->d_sel_sharp, B * R * kSharpPerRing))) return rc;
    if ((rc = dmalloc(c, c->d_sel_flat, B * R * kFlatPerRing))) return rc;
    if ((rc = prepare_build_grids(c->grid_H[1]))) { c->err = "k_build_grids: dynamic LDS size rejected"; return ALOAM_E_HIP; }
    if (c->solve_stage && (rc = prepare_solve())) { c->err = "k_solve: dynamic LDS size rejected"; return ALOAM_E_HIP; }
  }
  // identity poses (src/laserOdometry.cpp:93-98)
  std::vector<OdomState> init(B);
  std::memset(init.data(), 0, sizeof(OdomState) * B);
  for (size_t b = 0; b < B; ++b) { init[b].para_q[3] = 1.0; init[b].q_w[3] = 1.0; }
  HIP_TRY(c, hipMemcpyAsync(c->d_state.get(), init.data(), sizeof(OdomState) * B, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return ALOAM_OK;
}

void aloam_destroy(aloam_ctx* c) {
  DeviceScope device_scope(c);
  if (!c) return;
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  if (c->copy_stream) (void)hipStreamSynchronize(c->copy_stream);
  if (c->grid_stream) (void)hipStreamSynchronize(c->grid_stream);
  prof_resolve(c);
  delete c;                                       // the owners release buffers, then graphs, events and streams, on this device
}

const char* aloam_last_error(const aloam_ctx* c) { return c ? c->err.c_str() : "null context"; }
void* aloam_stream(aloam_ctx* c) { return c ? (void*)c->stream : nullptr; }

int aloam_synchronize(aloam_ctx* c) {
  DeviceScope device_scope(c);
  if (!c) return ALOAM_E_ARG;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  std::vector<SeqMeta> m(c->B);
  HIP_TRY(c, hipMemcpy(m.data(), c->d_meta.get(), sizeof(SeqMeta) * c->B, hipMemcpyDeviceToHost));
  for (int b = 0; b < c->B; ++b) {
    if (m[b].err & kErrEmpty) { c->err = "sequence " + std::to_string(b) + ": no point survives the NaN / minimum-range filter"; return ALOAM_E_EMPTY; }
    if (m[b].err & (kErrRingCap | kErrPointCap)) { c->err = "sequence " + std::to_string(b) + ": a ring exceeds max_ring_points or the scan exceeds max_points"; return ALOAM_E_CAPACITY; }
    if (m[b].err & kErrInternal) { c->err = "sequence " + std::to_string(b) + ": internal error, a ring workgroup of k_ring_features never published its counts (look-back wait timed out)"; return ALOAM_E_HIP; }
  }
  if (c->map_on) {
    std::vector<MapSeq> ms(c->B);
    int vc[4] = {0, 0, 0, 0};
    HIP_TRY(c, hipMemcpy(ms.data(), c->d_mapseq.get(), sizeof(MapSeq) * c->B, hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(vc, c->d_vox_counters.get(), sizeof(vc), hipMemcpyDeviceToHost));
    // The per-step flags (MapSeq.err, counters[1]) are folded into running counts when the next step starts (k_map_begin), so a
    // caller that queues many steps and synchronises once still hears about every step that dropped points: reported once, at the
    // first aloam_synchronize after it happened.  The steps themselves have run: poses and map are valid, the points that did not
    // fit were left out of the map.
    // Per-sequence deltas against what has already been reported, pool events and voxel-scratch events apart, so the message names a sequence
    // that dropped points SINCE the last call and says which resource ran out.
    long long fresh_pool = 0;
    int first_seq = -1;
    for (int b = 0; b < c->B; ++b) {
      const long long n = ms[b].err_steps + ((ms[b].err & kMapErrPool) ? 1 : 0);
      const long long fresh = on_pool_events_reported(c, b, n);
      if (fresh > 0) { fresh_pool += fresh; if (first_seq < 0) first_seq = b; }
    }
    const long long vox = vc[3] + (vc[1] ? 1 : 0), fresh_vox = vox > c->map_err_reported ? vox - c->map_err_reported : 0;
    c->map_err_reported = vox;
    if (fresh_pool + fresh_vox > 0) {
      c->err = "mapping, since the last aloam_synchronize:";
      if (fresh_pool) c->err += " " + std::to_string(fresh_pool) + " (sequence, step) pair(s) ran out of map pool (first: sequence " + std::to_string(first_seq) + ")";
      if (fresh_vox) c->err += std::string(fresh_pool ? " and" : "") + " " + std::to_string(fresh_vox) + " step(s) ran out of voxel-filter scratch";
      c->err += "; the points that did not fit were not inserted (raise pool_points)";
      return ALOAM_E_CAPACITY;
    }
    long long fresh_spill = 0;                            // tiles k_map_spill could not keep: reported once, like the capacity events above
    if (const int rc = spill_dropped_since(c, &fresh_spill)) return rc;
    if (fresh_spill > 0) {
      c->err = "map spill full: " + std::to_string(fresh_spill) + " tile(s) dropped since the last aloam_synchronize (drain more often or raise max_tiles / max_points)";
      return ALOAM_E_CAPACITY;
    }
    long long fresh_kf = 0;                               // nodes k_keyframe_capture kept without clouds: reported once, like the dropped tiles
    if (const int rc = keyframes_dropped_since(c, &fresh_kf)) return rc;
    if (fresh_kf > 0) {
      c->err = "keyframe store full: " + std::to_string(fresh_kf) + " node(s) kept without clouds since the last aloam_synchronize (raise max_corner_points / max_surf_points)";
      return ALOAM_E_CAPACITY;
    }
    if (c->d_rl_bad) {                                    // choices k_apply_corrections found outside 0 .. K-1: reported once, like the capacity events
      int bad = 0;
      HIP_TRY(c, hipMemcpy(&bad, c->d_rl_bad.get(), sizeof(bad), hipMemcpyDeviceToHost));
      const long long fresh = bad - c->rl_bad_reported;
      c->rl_bad_reported = bad;
      if (fresh > 0) {
        c->err = "aloam_apply_map_corrections, since the last aloam_synchronize: " + std::to_string(fresh) + " choice(s) outside 0 .. K-1; those sequences were left untouched";
        return ALOAM_E_ARG;
      }
    }
  }
  return ALOAM_OK;
}

// ---- per-sequence lifecycle ----------------------------------------------------------------------------------------
int aloam_set_active(aloam_ctx* c, const int* active) {
  DeviceScope device_scope(c);
  if (!c) return ALOAM_E_ARG;
  if (c->reg_pending && (c->stages & ALOAM_STAGE_REGISTRATION))
    for (int b = 0; b < c->B; ++b)
      if ((!active || active[b] != 0) != (c->seq[b].reg_active != 0)) {
        c->err = "the mask may not change between a registration and the odometry step that consumes it";
        return ALOAM_E_STATE;
      }
  on_active_mask_set(c, active);
  return ALOAM_OK;
}

int aloam_reset_sequences(aloam_ctx* c, const int* seqs, int n) {
  DeviceScope device_scope(c);
  if (!c) return ALOAM_E_ARG;
  if (const int rc = check_ids(c, seqs, n)) return rc;
  return on_slots_reset(c, seqs, n);
}

// ---- profiling -----------------------------------------------------------------------------------------------
int aloam_profile_enable(aloam_ctx* c, int on) {
  DeviceScope device_scope(c);
  if (!c) return ALOAM_E_ARG;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  prof_resolve(c);
  if (on) { for (int k = 0; k < K_COUNT; ++k) { c->prof_ms[k] = 0; c->prof_launches[k] = 0; } }
  c->prof_on = on != 0;
  return ALOAM_OK;
}
int aloam_profile_kernel_count(void) { return K_COUNT; }
const char* aloam_profile_kernel_name(int k) { return (k >= 0 && k < K_COUNT) ? kKernelNames[k] : ""; }

int aloam_profile_get(aloam_ctx* c, int kernel, double* total_ms, long long* launches, double* algorithmic_bytes) {
  DeviceScope device_scope(c);
  if (!c || kernel < 0 || kernel >= K_COUNT) return ALOAM_E_ARG;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  prof_resolve(c);
  if (total_ms) *total_ms = c->prof_ms[kernel];
  if (launches) *launches = c->prof_launches[kernel];
  if (algorithmic_bytes && kernel == K_EXPORT) {
    // the last export: every point read once and written once, one count read and one offset written per segment (DESIGN.md "Batched export")
    long long total = 0;
    HIP_TRY(c, hipMemcpy(&total, c->d_exp_off.get() + c->exp_last_segs, sizeof(total), hipMemcpyDeviceToHost));
    *algorithmic_bytes = 32.0 * total + 16.0 * c->exp_last_segs;
  } else if (algorithmic_bytes && (kernel == K_SAVE || kernel == K_LOAD)) {
    // the last save / load: every record byte - points, fixed sections, cube lists - read once and written once
    long long units = 0;
    if (kernel == K_SAVE && c->d_ck_uoff) HIP_TRY(c, hipMemcpy(&units, c->d_ck_uoff.get() + c->ck_save_n, sizeof(units), hipMemcpyDeviceToHost));
    *algorithmic_bytes = 2.0 * (kernel == K_SAVE ? 16.0 * units : (double)c->ck_load_bytes);
  } else if (algorithmic_bytes) {
    // per-launch algorithmic traffic from the sizes of the LAST sweep (DESIGN.md "Algorithmic bytes")
    std::vector<SeqMeta> m(c->B);
    HIP_TRY(c, hipMemcpy(m.data(), c->d_meta.get(), sizeof(SeqMeta) * c->B, hipMemcpyDeviceToHost));
    std::vector<MapSeq> ms(c->map_on ? c->B : 0);
    if (c->map_on) HIP_TRY(c, hipMemcpy(ms.data(), c->d_mapseq.get(), sizeof(MapSeq) * c->B, hipMemcpyDeviceToHost));
    double bytes = 0;
    for (int b = 0; b < c->B; ++b) {
      const double Nin = m[b].n_in, N = m[b].n_cloud, Fc = m[b].n_sharp, Lc = m[b].n_less_sharp, Fs = m[b].n_flat, Ls = m[b].n_less_flat;
      const double Lcl = m[b].n_corner_last, Lsl = m[b].n_surf_last;
      // the raw sweep: 16-byte records, or a range image at 2 bytes per point + its azimuth header (the last registration's kind)
      const bool ranges = !c->range_cols.empty();
      const double in_pt = ranges ? 2 : 16, in_hdr = ranges ? 2.0 * ((c->range_cols[b] + 7) & ~7) : 0;
      switch (kernel) {
        case K_FIND_ENDS: bytes += 2 * 256 * in_pt; break;
        case K_FRONT: bytes += in_pt * Nin + in_hdr + 16 * N + 16.0 * (c->R + 1) * ((Nin + kBlockPts - 1) / kBlockPts); break;   // k_front: the sweep in, the slabs out, two granules per ring and block
        case K_RING_STARTS: bytes += 12.0 * c->R; break;                                                                  // k_ring_starts
        case K_DENSE_CLOUD: bytes += 32 * N; break;                                                                            // k_dense_cloud (on demand)
        case K_RING_FEATURES: bytes += 16 * N + (c->debug_arrays ? 5 * N : 0) + 16 * (Fc + Lc + Fs + Ls); break;   // ring-ordered cloud in, the four feature clouds out (+ curvature / labels for the parity entry points)
        case K_BUILD_GRIDS: bytes += 16 * (Lcl + Lsl) + 48 * (Lcl + Lsl) + 12.0 * (c->grid_H[0] + c->grid_H[1]); break;   // read once, three sorted copies + three bucket tables out
        case K_TRANSFORM: bytes += 32 * (Fc + Fs); break;
        case K_ASSOC_CORNER: bytes += 16 * (Fc + Lcl) + 48 * Fc; break;
        case K_ASSOC_PLANE: bytes += 16 * (Fs + Lsl) + 64 * Fs; break;
        case K_SOLVE: bytes += 9.0 * (48 * Fc + 64 * Fs); break;
        // mapping: incoming clouds read + stacks written; submap read + grid written; queries + 5 neighbours + records;
        // 9 evaluations of the records; stacks -> cubes; valid cubes read + written; full cloud in + out
        default: break;
      }
      if (c->map_on && kernel >= K_MAP_BEGIN) {
        // scan-to-map stages, from the sizes of the last frame: S = down-sampled stacks, M = submap, F = factors
        const double Sc = ms[b].n_stack[0], Ss = ms[b].n_stack[1], Mc = ms[b].from_total[0], Ms = ms[b].from_total[1];
        const double Fc = ms[b].factor_num[1][0], Fs = ms[b].factor_num[1][1];
        switch (kernel) {
          case K_MAP_BEGIN: bytes += 2.0 * kMapValidMax * sizeof(CubeDesc) + sizeof(MapSeq); break;           // window descriptors + state
          case K_MAP_VOXEL_STACK: bytes += 16 * (Lcl + Lsl) + 16 * (Sc + Ss); break;                          // incoming clouds in, stacks out
          case K_MAP_GRID: bytes += 32 * (Mc + Ms) + 16.0 * c->map.H; break;               // submap in, bucketed copy + tables out
          case K_MAP_ASSOC: bytes += 16 * (Sc + Ss) + 80 * (Sc + Ss) + sizeof(MapEdgeRec) * Sc + sizeof(MapNormRec) * Ss; break;   // query + 5 neighbours in, record out
          case K_MAP_SOLVE: bytes += 9.0 * (sizeof(MapEdgeRec) * Fc + sizeof(MapNormRec) * Fs); break;        // <= 5 Jacobian + 4 cost evaluations
          case K_MAP_INSERT: bytes += 32 * (Sc + Ss); break;                                                  // stacks in, cube appends out
          case K_MAP_VOXEL_CUBES: bytes += 32 * (Mc + Ms + Sc + Ss); break;                                   // valid cubes re-filtered in place
          case K_MAP_REGISTER: bytes += 32 * N; break;                                                        // full cloud in + out
          default: break;
        }
      }
    }
    // the last scoring / apply call: candidates in, scores out, and per listed sequence its stacks and bucketed submap once
    // (what the K candidates re-read comes from L2; the kernel is latency- and issue-bound, not byte-bound).
    if (c->map_on && kernel == K_SCORE) {
      bytes = 64.0 * c->rl_last_K + 32.0 * c->rl_last_seqs.size() * c->rl_last_K;
      for (const int b : c->rl_last_seqs) bytes += 16.0 * (ms[b].n_stack[0] + ms[b].n_stack[1]) + 16.0 * (ms[b].from_total[0] + ms[b].from_total[1]) + 8.0 * c->map.H;
    }
    // the last aloam_export_pose_information: the valid records of the listed sequences that had a solve, read once, and one record written per id
    if (kernel == K_POSE_INFO) {
      bytes = (double)sizeof(aloam_pose_information) * c->info_last_list.size();
      std::vector<OdomState> os(c->info_last_which == ALOAM_INFO_ODOMETRY && !c->info_last_list.empty() ? c->B : 0);
      if (!os.empty()) HIP_TRY(c, hipMemcpy(os.data(), c->d_state.get(), sizeof(OdomState) * c->B, hipMemcpyDeviceToHost));
      const int o = c->cfg.outer_iterations < 2 ? 0 : 1;
      for (const int code : c->info_last_list) {
        if (!(code & kInfoSolvedBit)) continue;
        const int b = code & kInfoSeqMask;
        if (c->info_last_which == ALOAM_INFO_ODOMETRY) bytes += (double)sizeof(EdgeRec) * os[b].corner_corr[o] + (double)sizeof(PlaneRec) * os[b].plane_corr[o];
        else if (c->map_on) bytes += (double)sizeof(MapEdgeRec) * ms[b].factor_num[1][0] + (double)sizeof(MapNormRec) * ms[b].factor_num[1][1];
      }
    }
    // the last aloam_graph_optimize: nodes and edges read once, the estimates and one result written (the iterations run out of L2); or the last
    // aloam_graph_trim: the rows it moved, read and written
    if (kernel == K_POSE_GRAPH) bytes = (double)(sizeof(aloam_graph_node) + 56) * c->pg.last_nodes + (double)sizeof(aloam_graph_edge) * c->pg.last_edges;
    if (kernel == K_POSE_GRAPH && c->pg.last_trim_bytes >= 0) bytes = (double)c->pg.last_trim_bytes;
    // the last aloam_graph_marginals: per request its graph's estimates and edges read once, one request read and one result written (the
    // linearisation and the iterations run out of the request's scratch row)
    if (kernel == K_GRAPH_MARGINALS)
      bytes = 56.0 * c->mg.last_nodes + (double)sizeof(aloam_graph_edge) * c->mg.last_edges + (double)(sizeof(GraphMarginalItem) + sizeof(aloam_graph_marginal_result)) * c->mg.last_n;
    // the last aloam_graph_export_map: 16 B read + 16 B written per raw point (transform), the slot written and read and the point read and
    // written again (grouping, 40 B), 16 B per emitted point and 32 B per tile
    if (kernel == K_GRAPH_MAP && c->gm.last_segs >= 0) {
      long long emitted = 0;
      HIP_TRY(c, hipMemcpy(&emitted, c->gm.point_off.get() + c->gm.last_segs, sizeof(emitted), hipMemcpyDeviceToHost));
      bytes = 72.0 * c->gm.last_raw + 16.0 * emitted + 32.0 * c->gm.last_segs;
    }
    if (kernel == K_APPLY) bytes = c->rl_apply_n * (4.0 + 4.0 + 64.0 + 56.0);   // id, choice, candidate in, correction out
    *algorithmic_bytes = bytes;
  }
  return ALOAM_OK;
}

}  // extern "C"
