// a-loam_amd/csrc/capi_relocalize.hip — host side of the map-pose hypotheses: aloam_score_map_corrections scores K candidate
// map <- odometry corrections per sequence against the state its last frozen mapping step left on the device, aloam_apply_map_corrections
// installs one per sequence in stream order.  Every argument is checked before anything is queued.
#include <algorithm>

#include "capi_internal.hpp"

// Where the kernels read the K candidates from: device memory of the context's device or pinned host memory as they are (*dev), pageable host
// memory through one staged copy (*dev = nullptr; as aloam_load_sequences stages pageable records).  Managed memory, another device's
// memory and NULL are refused.  Queues nothing.
static int check_candidates(aloam_ctx* c, const aloam_map_correction* cand, const aloam_map_correction** dev) {
  void* d = nullptr;
  const CallerMem m = classify_pointer(c, cand, &d);
  if (!cand || m == kMemManaged || m == kMemOtherDevice || (uintptr_t)cand % alignof(aloam_map_correction)) {
    c->err = "cand must be 8-byte aligned device memory of the context's device, pinned or pageable host memory";
    return ALOAM_E_ARG;
  }
  *dev = static_cast<const aloam_map_correction*>(d);
  return ALOAM_OK;
}
static int stage_candidates(aloam_ctx* c, const aloam_map_correction* cand, int K, const aloam_map_correction** dev) {
  if (*dev) return ALOAM_OK;
  if (const int rc = c->d_rl_cand.grow(c, K)) return rc;
  HIP_TRY(c, hipMemcpyAsync(c->d_rl_cand.get(), cand, sizeof(aloam_map_correction) * (size_t)K, hipMemcpyHostToDevice, c->stream));
  *dev = c->d_rl_cand.get();
  return ALOAM_OK;
}

static int check_call(aloam_ctx* c, const int* seqs, int n, int K) {
  if (const int rc = require_stage(c, ALOAM_STAGE_MAPPING)) return rc;
  if (!c->map_on) { c->err = "mapping not enabled"; return ALOAM_E_STATE; }
  if (const int rc = check_ids(c, seqs, n)) return rc;
  if (K < 1) { c->err = "K must be at least 1"; return ALOAM_E_ARG; }
  return ALOAM_OK;
}

extern "C" {

int aloam_score_map_corrections(aloam_ctx* c, const int* seqs, int n, const aloam_map_correction* cand, int K, aloam_map_score* scores, int* best) {
  DeviceScope device_scope(c);
  if (!c) return ALOAM_E_ARG;
  if (const int rc = check_call(c, seqs, n, K)) return rc;
  for (int i = 0; i < n; ++i)
    if (!c->seq[seqs[i]].scorable) {
      c->err = "sequence " + std::to_string(seqs[i]) + ": its last mapping step was not a frozen one, or its map, frame or pools were replaced since: nothing to score against";
      return ALOAM_E_STATE;
    }
  void *d_scores = nullptr, *d_best = nullptr;
  if (const int rc = export_target(c, scores, alignof(aloam_map_score), "scores", &d_scores)) return rc;
  if (best) if (const int rc = export_target(c, best, alignof(int), "best", &d_best)) return rc;
  if ((long long)n * K > kScoreMaxPairs) { c->err = "n * K above " + std::to_string(kScoreMaxPairs) + " (sequence, candidate) pairs: split the call"; return ALOAM_E_ARG; }
  const aloam_map_correction* d_cand = nullptr;
  if (const int rc = check_candidates(c, cand, &d_cand)) return rc;
  if (n == 0) return ALOAM_OK;
  if (!c->d_rl_seqs) HIP_TRY(c, dalloc(c->d_rl_seqs, (size_t)c->B));
  if (const int rc = c->d_rl_part.grow(c, (long long)n * K * kScoreParts)) return rc;
  if (const int rc = stage_candidates(c, cand, K, &d_cand)) return rc;
  if (const int rc = stage_ints(c, seqs, n, c->d_rl_seqs.get())) return rc;
  ScoreArgs a{};
  a.B = c->B; a.cap = c->cap; a.R = c->R; a.n = n; a.K = K;
  a.splits = n < 8 ? std::max(1, std::min(8 / n, K)) : 1;      // fewer than 8 sequences: their candidates are dealt over the XCDs left idle
  a.kper = (K + a.splits - 1) / a.splits;
  a.seqs = c->d_rl_seqs.get(); a.cand = d_cand; a.seq = c->d_mapseq.get();
  for (int k = 0; k < 2; ++k) { a.stack[k] = c->d_stack[k].get(); a.grid_sorted[k] = c->map.grid_sorted[k].get(); a.grid_start[k] = c->map.grid_start[k].get(); }
  a.grid_H = c->map.H; a.pool_cap = c->map.points;
  a.part = c->d_rl_part.get(); a.scores = static_cast<aloam_map_score*>(d_scores); a.best = static_cast<int*>(d_best);
  { ProfScope p(c, K_SCORE); launch_score_corrections(a, c->stream); }
  HIP_TRY(c, hipGetLastError());
  c->rl_last_seqs.assign(seqs, seqs + n); c->rl_last_K = K;
  return ALOAM_OK;
}

int aloam_apply_map_corrections(aloam_ctx* c, const int* seqs, int n, const aloam_map_correction* cand, int K, const int* choice) {
  DeviceScope device_scope(c);
  if (!c) return ALOAM_E_ARG;
  if (const int rc = check_call(c, seqs, n, K)) return rc;
  void* d_choice = nullptr;
  if (const int rc = export_target(c, choice, alignof(int), "choice", &d_choice)) return rc;
  const aloam_map_correction* d_cand = nullptr;
  if (const int rc = check_candidates(c, cand, &d_cand)) return rc;
  if (n == 0) return ALOAM_OK;
  if (!c->d_rl_seqs) HIP_TRY(c, dalloc(c->d_rl_seqs, (size_t)c->B));
  if (!c->d_rl_bad) if (const int rc = dmalloc(c, c->d_rl_bad, 1)) return rc;
  if (const int rc = stage_candidates(c, cand, K, &d_cand)) return rc;
  if (const int rc = stage_ints(c, seqs, n, c->d_rl_seqs.get())) return rc;
  ApplyArgs a{};
  a.n = n; a.K = K; a.seqs = c->d_rl_seqs.get(); a.cand = d_cand; a.choice = static_cast<const int*>(d_choice);
  a.seq = c->d_mapseq.get(); a.bad_choice = c->d_rl_bad.get();
  { ProfScope p(c, K_APPLY); launch_apply_corrections(a, c->stream); }
  HIP_TRY(c, hipGetLastError());
  c->rl_apply_n = n;
  on_map_corrections_applied(c, seqs, n);
  return ALOAM_OK;
}

}  // extern "C"
