// a-loam_amd/csrc/capi_seq.hip — the per-sequence host state (SeqHost, capi_internal.hpp): a stage's mask, and one function per thing that happens
// to a sequence.  An event does the whole consequence, the host fields and the stream-ordered device side that goes with them, and nothing else
// assigns a SeqHost field: the invalidation rules are this file (as a table: DESIGN.md §7b).
#include "capi_internal.hpp"

static int mark_window_stale(aloam_ctx* c, int seq) {   // an attached sequence cuts its window from the atlas anew in its next mapping step
  if (c->any_attached && c->seq[seq].attached) HIP_TRY(c, hipMemsetAsync(c->d_at_stale.get() + seq, 1, sizeof(int), c->stream));   // any non-zero value
  return ALOAM_OK;
}

namespace aloam {

// The mask of one stage's launches: kSeqActive for who takes part plus that stage's `extra_bits`, staged into `dst` (allocated on first use, never
// again: the captured odometry graph holds d_mask_odo) unless the stage says that this step runs `unmasked`.
int stage_mask(aloam_ctx* c, DevBuf<int>& dst, int (*extra_bits)(const SeqHost&), bool (*unmasked)(const aloam_ctx*, const StageMask&), StageMask* m) {
  m->bits.resize(c->B);
  for (int b = 0; b < c->B; ++b) {
    const int v = m->bits[b] = takes_part(c, b) ? (kSeqActive | extra_bits(c->seq[b])) : 0;
    m->any_active |= v != 0; m->any_grow |= (v & kSeqMapGrow) != 0;
    m->any_solve |= (v & kSeqSolve) != 0; m->all_solve &= (v & kSeqSolve) != 0;
  }
  if (unmasked(c, *m)) return ALOAM_OK;
  if (!dst && dmalloc(c, dst, c->B)) return ALOAM_E_HIP;
  if (const int rc = stage_ints(c, m->bits.data(), c->B, dst.get())) return rc;
  m->dev = dst.get();
  return ALOAM_OK;
}

void on_active_mask_set(aloam_ctx* c, const int* active) {   // aloam_set_active / aloam_set_map_frozen: nullptr = every sequence / none
  c->all_active = true;
  for (int b = 0; b < c->B; ++b) { c->seq[b].active = !active || active[b] != 0; c->all_active &= c->seq[b].active != 0; }
}
void on_frozen_mask_set(aloam_ctx* c, const int* frozen) {
  c->any_frozen = false;
  for (int b = 0; b < c->B; ++b) { c->seq[b].frozen = frozen && frozen[b] != 0; c->any_frozen |= c->seq[b].frozen; }
}

// Checked slots are reset (aloam_reset_sequences, or the first half of a load), in stream order: new sequences with nothing registered, built or
// reported.  active, frozen and attached belong to the slot, not to the sequence: they stay, and an attached slot cuts its window anew.
int on_slots_reset(aloam_ctx* c, const int* seqs, int n) {
  if (n == 0) return ALOAM_OK;
  if (!c->d_reset_ids && dmalloc(c, c->d_reset_ids, c->B)) return ALOAM_E_HIP;
  if (const int rc = stage_ints(c, seqs, n, c->d_reset_ids.get())) return rc;
  ResetArgs r{};
  r.seqs = c->d_reset_ids.get(); r.n = n; r.R = c->R;
  r.meta = c->d_meta.get(); r.ringstart = c->d_ringstart.get(); r.state = c->d_state.get();
  r.edges = c->d_edges.get(); r.planes = c->d_planes.get();
  for (int p = 0; p < 2; ++p) for (int k = 0; k < 2; ++k) r.grid_flags[p][k] = c->d_grid_flags[p][k].get();
  for (int k = 0; k < 2; ++k) { r.less_sharp[k] = c->d_less_sharp[k].get(); r.less_flat[k] = c->d_less_flat[k].get(); }
  r.cap = c->cap;
  if (c->map_on) { r.mapseq = c->d_mapseq.get(); r.cubes = c->d_cubes.get(); r.addcnt = c->d_addcnt.get(); r.live = c->d_map_live.get(); r.grid_sig = c->d_grid_sig.get(); }
  launch_reset_sequences(r, c->stream);
  HIP_TRY(c, hipGetLastError());
  for (int i = 0; i < n; ++i) {
    SeqHost& s = c->seq[seqs[i]];
    s.parity = 0; s.inited = 0; s.grid_built = false; s.needs_odom = false; s.map_err_seen = 0; s.scorable = false; s.has_sweep = false; s.desc_valid = false;
    s.info_odom = false; s.info_map = false; s.has_stacks = false;
  }
  for (int i = 0; i < n; ++i) if (const int rc = mark_window_stale(c, seqs[i])) return rc;
  return ALOAM_OK;
}

// k_load_sequences has been queued into a slot that was just reset: the last clouds it brought have met no odometry step, so it may not map before one.
void on_slot_loaded(aloam_ctx* c, int seq, bool inited, long long err_events) {
  SeqHost& s = c->seq[seq];
  s.inited = inited; s.map_err_seen = err_events; s.needs_odom = (c->stages & ALOAM_STAGE_ODOMETRY) != 0;
}

// A registration is being queued: who takes part holds a new sweep with no descriptor yet; the mask stays until the odometry step has consumed the sweep.
void on_sweep_registered(aloam_ctx* c) {
  const bool odo = c->stages & ALOAM_STAGE_ODOMETRY;
  for (int b = 0; b < c->B; ++b) {
    SeqHost& s = c->seq[b];
    if (odo) s.reg_active = s.active;
    if (takes_part(c, b)) { s.has_sweep = true; s.desc_valid = false; s.info_odom = false; }   // (the feature counts its records are read through are the new sweep's)
  }
  if (odo) c->reg_pending = true;
}

// An odometry step has been queued: who took part swapped its clouds (k_advance) and has the grids of the new last ones if the step built them beside its
// solve (built_next; a step whose grids were built beside the registration of the same call builds none, and neither does the serial chain).
void on_odometry_advanced(aloam_ctx* c, const StageMask& m, bool built_next) {
  for (int b = 0; b < c->B; ++b) {
    SeqHost& s = c->seq[b];
    if (m.bits[b] & kSeqActive) {
      s.parity ^= 1; s.inited = 1; s.needs_odom = false; s.grid_built = built_next;
      s.info_odom = (m.bits[b] & kSeqSolve) && c->cfg.outer_iterations > 0;   // a first frame solves nothing
    }
  }
  c->reg_pending = false;
}

void on_last_clouds_replaced(aloam_ctx* c, int seq) { c->seq[seq].grid_built = false; c->seq[seq].info_odom = false; }   // aloam_set_last: the next step builds their grids before it searches
void on_odometry_inputs_replaced(aloam_ctx* c, int seq) { c->seq[seq].info_odom = false; }   // aloam_set_state / aloam_set_features: the pose or the feature counts of its last solve are gone

// aloam_set_map / aloam_set_map_frame: another submap or frame, so its grids are built anew, nothing to score against, an attached window is cut anew.
int on_map_replaced(aloam_ctx* c, int seq) {
  HIP_TRY(c, hipMemsetAsync(c->d_grid_sig.get() + (size_t)seq * 2, 0, sizeof(MapGridSig) * 2, c->stream));
  c->seq[seq].scorable = false; c->seq[seq].info_map = false;
  return mark_window_stale(c, seq);
}

// map_alloc_pool has filled `fresh`: the pool contents were moved, the grids were not.  The old buffers are released once the copies out of them have run.
int on_map_pool_reallocated(aloam_ctx* c, MapPool&& fresh) {
  if (c->d_grid_sig) HIP_TRY(c, hipMemsetAsync(c->d_grid_sig.get(), 0, sizeof(MapGridSig) * c->B * 2, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  c->map = std::move(fresh);
  for (SeqHost& s : c->seq) s.scorable = false;
  return ALOAM_OK;
}

void on_mapping_step_queued(aloam_ctx* c) {   // aloam_score_map_corrections may read the stacks and the grid that a frozen step leaves
  for (int b = 0; b < c->B; ++b) if (takes_part(c, b)) { c->seq[b].scorable = c->seq[b].frozen; c->seq[b].info_map = true; c->seq[b].has_stacks = true; }
}
void on_map_corrections_applied(aloam_ctx* c, const int* seqs, int n) { for (int i = 0; i < n; ++i) c->seq[seqs[i]].info_map = false; }   // the pose of its last solve is in a frame that is gone


// aloam_atlas_attach has staged the mask: a newly attached sequence cuts its window in its next step and has nothing to score against.
int on_atlas_attached(aloam_ctx* c, const std::vector<int>& attached) {
  std::vector<char> fresh(c->B);
  c->any_attached = false;
  for (int b = 0; b < c->B; ++b) { fresh[b] = attached[b] && !c->seq[b].attached; c->any_attached |= c->seq[b].attached = attached[b] != 0; }
  for (int b = 0; b < c->B; ++b) if (fresh[b]) { if (const int rc = mark_window_stale(c, b)) return rc; c->seq[b].scorable = false; }
  return ALOAM_OK;
}

void on_system_inited_forced(aloam_ctx* c, int inited) { for (SeqHost& s : c->seq) s.inited = inited; }   // aloam_set_system_inited, beside its launch
void on_places_enabled(aloam_ctx* c) { for (SeqHost& s : c->seq) s.desc_valid = false; }                    // d_pl_desc is new: it holds nobody's descriptor
void on_descriptors_made(aloam_ctx* c, const int* seqs, int n) { for (int i = 0; i < n; ++i) c->seq[seqs[i]].desc_valid = true; }
// The pose graph of a slot (capi_posegraph.hip): its counts change here and nowhere else.  A node past the first brings its odometry edge.
void on_graph_nodes_added(aloam_ctx* c, const int* seqs, int n) {
  for (int i = 0; i < n; ++i) { SeqHost& s = c->seq[seqs[i]]; if (s.graph_nodes > 0) ++s.graph_edges; ++s.graph_nodes; }
}
void on_graph_edges_added(aloam_ctx* c, int seq, int count) { c->seq[seq].graph_edges += count; }
void on_graph_cleared(aloam_ctx* c, const int* seqs, int n) { for (int i = 0; i < n; ++i) { c->seq[seqs[i]].graph_nodes = 0; c->seq[seqs[i]].graph_edges = 0; } }
// aloam_graph_load has queued the unpack of a checked record into an empty slot: its rows hold the record's nodes and edges.
void on_graph_loaded(aloam_ctx* c, int seq, int nodes, int edges) { c->seq[seq].graph_nodes = nodes; c->seq[seq].graph_edges = edges; }
// aloam_graph_trim has run and the stream has drained: the slot's rows hold what k_graph_trim reported (the kept nodes, the compacted edges).
void on_graph_trimmed(aloam_ctx* c, int seq, int nodes, int edges) { c->seq[seq].graph_nodes = nodes; c->seq[seq].graph_edges = edges; }
// aloam_graph_apply has been queued for the listed sequences: another frame and, with its map rebuilt, another submap, so their grids are built
// anew, there is nothing to score against and the pose of their last mapping solve is gone.  The graph's counts stay, and so does has_stacks:
// the stacks are in the sensor frame.
int on_graph_applied(aloam_ctx* c, const int* seqs, int n) {
  for (int i = 0; i < n; ++i) {
    HIP_TRY(c, hipMemsetAsync(c->d_grid_sig.get() + (size_t)seqs[i] * 2, 0, sizeof(MapGridSig) * 2, c->stream));
    c->seq[seqs[i]].scorable = false; c->seq[seqs[i]].info_map = false;
  }
  return ALOAM_OK;
}
long long on_pool_events_reported(aloam_ctx* c, int seq, long long events) {   // aloam_synchronize has read a sequence's pool capacity events: how many are new
  const long long fresh = events > c->seq[seq].map_err_seen ? events - c->seq[seq].map_err_seen : 0;
  c->seq[seq].map_err_seen = events;
  return fresh;
}

}  // namespace aloam
