// a-loam_amd/csrc/capi_odometry.hip — host side of scan registration and laser odometry: input slabs, the registration and odometry
// launches, the process_* entries, the per-sequence getters and setters and the intermediate arrays.
#include <algorithm>
#include <cstring>
#include <functional>

#include "capi_internal.hpp"

namespace {

RegArgs reg_args(aloam_ctx* c, const void* d_scans, long long seq_stride, int pt_stride) {
  RegArgs a{};
  a.in = (const char*)d_scans; a.seq_stride = seq_stride; a.pt_stride = pt_stride;
  a.B = c->B; a.cap = c->cap; a.R = c->R; a.NB = c->NB;
  a.ring_from_field = c->cfg.ring_from_field; a.min_range = c->cfg.min_range;
  a.meta = c->d_meta.get(); a.slabs = c->d_slabs.get(); a.slab = c->slab; a.front_lb = c->d_front_lb.get(); a.front_ticket = c->d_front_ticket.get();
  a.ringstart = c->d_ringstart.get(); a.cloud = c->d_cloud.get(); a.curv = c->d_curv.get(); a.label = c->d_label.get();
  a.lookback = c->d_lookback.get(); a.epoch = c->reg_epoch; a.store_debug = c->debug_arrays ? 1 : 0; a.ring_ticket = c->d_ring_ticket.get();
  a.sharp = c->d_sharp.get(); a.flat = c->d_flat.get();
  for (int k = 0; k < 2; ++k) { a.less_sharp[k] = c->d_less_sharp[k].get(); a.less_flat[k] = c->d_less_flat[k].get(); }
  a.active = c->reg_mask;
  return a;
}

}  // namespace

namespace aloam {

OdomArgs odom_args(aloam_ctx* c) {
  OdomArgs a{};
  a.B = c->B; a.cap = c->cap; a.R = c->R;
  a.meta = c->d_meta.get(); a.state = c->d_state.get();
  a.sharp = c->d_sharp.get(); a.flat = c->d_flat.get();
  for (int k = 0; k < 2; ++k) { a.less_sharp[k] = c->d_less_sharp[k].get(); a.less_flat[k] = c->d_less_flat[k].get(); }
  for (int p = 0; p < 2; ++p) for (int k = 0; k < 2; ++k) {
    a.grid_sorted3[p][k] = c->d_grid_sorted3[p][k].get(); a.grid_sorted2[p][k] = c->d_grid_sorted2[p][k].get(); a.grid_start3[p][k] = c->d_grid_start3[p][k].get();
    a.grid_sorted3c[p][k] = c->d_grid_sorted3c[p][k].get(); a.grid_start3c[p][k] = c->d_grid_start3c[p][k].get();
    a.grid_start2[p][k] = c->d_grid_start2[p][k].get();
    a.grid_flags[p][k] = c->d_grid_flags[p][k].get(); a.grid_walk[p][k] = c->d_grid_walk[p][k].get();
  }
  a.grid_H_corner = c->grid_H[0]; a.grid_H_surf = c->grid_H[1];
  a.edges = c->d_edges.get(); a.planes = c->d_planes.get();
  a.sel_sharp = c->d_sel_sharp.get(); a.sel_flat = c->d_sel_flat.get();
  a.lm_max_iterations = c->cfg.lm_max_iterations;
  a.distortion = c->cfg.distortion != 0;
  a.solve_stage = c->solve_stage ? 1 : 0;
  return a;
}

}  // namespace aloam

namespace {

// A batch handed to scan registration, checked before anything of it is queued.
int check_batch(aloam_ctx* c, const int* n_in, int stride_bytes) {
  if (const int rc = require_stage(c, ALOAM_STAGE_REGISTRATION)) return rc;
  if (stride_bytes < 12 || (stride_bytes & 3)) { c->err = "stride_bytes must be 12 (x, y, z only) or >= 16, and a multiple of 4"; return ALOAM_E_ARG; }
  if (stride_bytes == 12 && c->cfg.ring_from_field) { c->err = "ring_from_field needs the 4th float of every record: stride_bytes >= 16"; return ALOAM_E_ARG; }
  for (int b = 0; b < c->B; ++b) {
    if (n_in[b] < 0) { c->err = "negative point count"; return ALOAM_E_ARG; }
    if (n_in[b] > c->max_points) { c->err = "scan exceeds max_points"; return ALOAM_E_CAPACITY; }
  }
  return ALOAM_OK;
}

}  // namespace

namespace aloam {

// debug_arrays: also write cloudCurvature / cloudLabel (the per-point entry points aloam_get_curvature / aloam_get_labels);
// the throughput entries (aloam_process_device / aloam_process_host) leave those 5 bytes per point out.  The batch has passed check_batch.
int register_launch(aloam_ctx* c, const void* d_scans, long long seq_stride, const int* n_in, int stride_bytes, int slot, bool debug_arrays, const int* n_cols,
                    const std::function<void()>* after_front) {
  int rc = ALOAM_OK;
  // A sequence that sits out keeps its dense cloud: made now from its slabs if the last registration's was never asked for (a no-op otherwise)
  if (!c->all_active && (rc = ensure_dense(c))) return rc;
  c->nin_max = 0;
  for (int b = 0; b < c->B; ++b) if (takes_part(c, b)) c->nin_max = std::max(c->nin_max, n_in[b]);
  if ((rc = stage_ints(c, n_cols ? n_cols : n_in, c->B, c->d_nin.get()))) return rc;   // what the first kernel reads: points, or columns of a range image
  if (n_cols) c->range_cols.assign(n_cols, n_cols + c->B); else c->range_cols.clear();
  StageMask m;                                                               // nothing but who takes part; no mask when that is everyone
  rc = stage_mask(c, c->d_mask_reg, [](const SeqHost&) { return 0; }, [](const aloam_ctx* x, const StageMask&) { return x->all_active; }, &m);
  c->reg_mask = m.dev;
  if (rc) return rc;
  on_sweep_registered(c);
  c->debug_arrays = debug_arrays || c->sum_order != 0;      // the reference-order pass reads cloudLabel
  if (((++c->reg_epoch) & 0x7fffffffu) == 0) ++c->reg_epoch;                 // 31 bits of it tag the look-back granules; 0 = "never written"
  const RegArgs a = reg_args(c, d_scans, seq_stride, stride_bytes);
  if (n_cols) {
    const RangeArgs d{c->d_nin.get(), c->d_rd_az.get(), c->d_rd_rows.get(), c->rd_rows, c->rd_n_az, c->rd_order == ALOAM_RANGE_ROW_MAJOR ? 1 : 0, c->rd_scale};
    { ProfScope p(c, K_FIND_ENDS); launch_find_ends_range(a, d, c->stream); }
    { ProfScope p(c, K_FRONT); launch_front_range(a, d, c->stream); }
  } else {
    { ProfScope p(c, K_FIND_ENDS); launch_find_ends(a, c->d_nin.get(), c->stream); }
    { ProfScope p(c, K_FRONT); launch_front(a, c->stream); }
  }
  if (after_front) (*after_front)();                         // (aloam_process_*: the grid build of the step is forked here, odometry_fork_build)
  { ProfScope p(c, K_RING_STARTS); launch_ring_starts(a, c->stream); }
  c->dense_valid = false;
  if (slot >= 0) { HIP_TRY(c, hipEventRecord(c->in_consumed[slot], c->stream)); c->in_used[slot] = true; }   // the raw sweep is not read after this
  { ProfScope p(c, K_RING_FEATURES); launch_ring_features(a, c->npad, 0.2f, c->stream);     // leaf 0.2 (src/scanRegistration.cpp:404)
    if (c->sum_order) launch_less_flat_reference_order(reg_args(c, d_scans, seq_stride, stride_bytes), c->npad, 0.2f, c->stream); }
  HIP_TRY(c, hipGetLastError());
  c->have_features = true;
  return ALOAM_OK;
}

// The dense ring-by-ring cloud (laserCloud of src/scanRegistration.cpp:246-252) is made from the slabs when a consumer of the FULL cloud asks for it.
int ensure_dense(aloam_ctx* c) {
  if (c->dense_valid) return ALOAM_OK;                  // (also: nothing registered yet, or the cloud was set from outside)
  { ProfScope p(c, K_DENSE_CLOUD); launch_dense_cloud(reg_args(c, nullptr, 0, 16), c->stream); }
  HIP_TRY(c, hipGetLastError());
  c->dense_valid = true;
  return ALOAM_OK;
}

// Where cloud `id` of every sequence lives, as the export reads it (*s; cloud_row gives one sequence's row): ALOAM_CLOUD_*, or
// ALOAM_EXPORT_MAP + ALOAM_MAP_REGISTERED / CORNER_STACK / SURF_STACK (buffers of aloam_mapping_enable).  Returns the points a row may hold,
// 0 for any other id.  The getters, the setters, the export and the checks of a record's header all read the layout from here.  Queues nothing.
long long cloud_desc(const aloam_ctx* c, int id, ExportSrc* s) {
  const int* meta = reinterpret_cast<const int*>(c->d_meta.get());
  const int* mseq = reinterpret_cast<const int*>(c->d_mapseq.get());
  const int meta_ints = sizeof(SeqMeta) / sizeof(int), map_ints = sizeof(MapSeq) / sizeof(int);
  const long long sharp = (long long)c->R * kSharpPerRing, flat = (long long)c->R * kFlatPerRing, feat = (long long)c->R * kLessSharpPerRing;
  const long long cap = c->cap, pts = c->max_points;
  long long capacity = 0;
  auto set = [&](const float4* b0, const float4* b1, long long stride, long long row_cap, const int* count, int count_stride, int sel) {
    *s = ExportSrc{{b0, b1}, stride, count, count_stride, sel, kExportPlain, 0};
    capacity = row_cap;
  };
#define META_FIELD(f) (meta + offsetof(SeqMeta, f) / sizeof(int)), meta_ints
  // aloam_odometry_step ends with the reference's pointer swap (src/laserOdometry.cpp:554-560): afterwards the sweep
  // just processed is read through CORNER_LAST / SURF_LAST, exactly like laserCloudCornerLast / laserCloudSurfLast.
  switch (id) {
    case ALOAM_CLOUD_FULL: set(c->d_cloud.get(), nullptr, cap, pts, META_FIELD(n_cloud), kSelFixed); break;
    case ALOAM_CLOUD_SHARP: set(c->d_sharp.get(), nullptr, sharp, sharp, META_FIELD(n_sharp), kSelFixed); break;
    case ALOAM_CLOUD_FLAT: set(c->d_flat.get(), nullptr, flat, flat, META_FIELD(n_flat), kSelFixed); break;
    case ALOAM_CLOUD_LESS_SHARP: set(c->d_less_sharp[0].get(), c->d_less_sharp[1].get(), feat, feat, META_FIELD(n_less_sharp), kSelCurrent); break;
    case ALOAM_CLOUD_LESS_FLAT: set(c->d_less_flat[0].get(), c->d_less_flat[1].get(), cap, pts, META_FIELD(n_less_flat), kSelCurrent); break;
    case ALOAM_CLOUD_CORNER_LAST: set(c->d_less_sharp[0].get(), c->d_less_sharp[1].get(), feat, feat, META_FIELD(n_corner_last), kSelLast); break;
    case ALOAM_CLOUD_SURF_LAST: set(c->d_less_flat[0].get(), c->d_less_flat[1].get(), cap, pts, META_FIELD(n_surf_last), kSelLast); break;
    case ALOAM_EXPORT_MAP + ALOAM_MAP_REGISTERED: set(c->d_registered.get(), nullptr, cap, pts, META_FIELD(n_cloud), kSelFixed); break;
    case ALOAM_EXPORT_MAP + ALOAM_MAP_CORNER_STACK: set(c->d_stack[0].get(), nullptr, feat, feat, mseq + offsetof(MapSeq, n_stack) / sizeof(int), map_ints, kSelFixed); break;
    case ALOAM_EXPORT_MAP + ALOAM_MAP_SURF_STACK: set(c->d_stack[1].get(), nullptr, cap, pts, mseq + offsetof(MapSeq, n_stack) / sizeof(int) + 1, map_ints, kSelFixed); break;
    default: break;
  }
#undef META_FIELD
  return capacity;
}

// Where cloud `id` (one of cloud_desc's) of sequence `seq` lives on the device and how many points it holds, as the getters read it.
int find_cloud(aloam_ctx* c, int seq, int id, const float4** ptr, int* n) {
  int rc = check_seq(c, seq);
  if (rc || (id == ALOAM_CLOUD_FULL && (rc = ensure_dense(c)))) return rc;
  ExportSrc s;
  if (!cloud_desc(c, id, &s)) { c->err = "unknown cloud id"; return ALOAM_E_ARG; }
  if ((rc = read_seq(c, s.count + (size_t)seq * s.count_stride, n))) return rc;
  if (!(*ptr = cloud_row(c, s, seq))) { c->err = "this context holds no such cloud (see aloam_create_stages)"; return ALOAM_E_STATE; }
  return ALOAM_OK;
}

// Next device staging slab for a host-resident batch: waits (host side) until the kernels that read the slab two calls ago
// are done with it, grows it if needed (the old slab is released first: its contents are not needed).
static int acquire_slab(aloam_ctx* c, size_t need, int* slot_out) {
  const int s = c->in_slot;
  c->in_slot ^= 1;
  if (c->in_used[s]) HIP_TRY(c, hipEventSynchronize(c->in_consumed[s]));
  if (const int rc = c->d_in[s].grow(c, need)) return rc;
  *slot_out = s;
  return ALOAM_OK;
}

int stage_batch(aloam_ctx* c, const void* h_scans, long long seq_stride_bytes, size_t row, size_t last, size_t d_seq_stride, int* slot_out, char** d_in_out) {
  if (seq_stride_bytes < 0) { c->err = "bad stride"; return ALOAM_E_ARG; }
  if (c->B > 1 && (size_t)seq_stride_bytes < row) { c->err = "seq_stride_bytes smaller than a scan"; return ALOAM_E_ARG; }
  int slot = 0;
  if (const int rc = acquire_slab(c, d_seq_stride * c->B, &slot)) return rc;
  char* d_in = c->d_in[slot].get();
  if (row > 0) {
    // rows 0 .. B-2 as one strided copy of the batch-wide maximum (every row but the last is followed by the next one, so the
    // extra bytes are readable); the last row with its own length, so that a buffer that ends with the last sweep is never over-read
    if (c->B > 1) HIP_TRY(c, hipMemcpy2DAsync(d_in, d_seq_stride, h_scans, (size_t)seq_stride_bytes, row, (size_t)c->B - 1, hipMemcpyHostToDevice, c->copy_stream));
    if (last > 0) HIP_TRY(c, hipMemcpyAsync(d_in + (size_t)(c->B - 1) * d_seq_stride, (const char*)h_scans + (size_t)(c->B - 1) * (size_t)seq_stride_bytes, last, hipMemcpyHostToDevice, c->copy_stream));
  }
  HIP_TRY(c, hipEventRecord(c->in_copied[slot], c->copy_stream));
  HIP_TRY(c, hipStreamWaitEvent(c->stream, c->in_copied[slot], 0));
  *slot_out = slot; *d_in_out = d_in;
  return ALOAM_OK;
}

}  // namespace aloam

namespace {

// The grid stream, forked from the context's stream for one build and joined into it again inside one call (aloam_odometry_step, aloam_process_*), so
// that nothing else has to know about it: however the call ends after the fork, the context's stream has been made to wait for what was forked.
struct GridFork {
  aloam_ctx* c;
  bool open = false;
  hipError_t err = hipSuccess;                          // the first failure of any of its calls
  explicit GridFork(aloam_ctx* c_) : c(c_) {}
  GridFork(const GridFork&) = delete;
  GridFork& operator=(const GridFork&) = delete;
  ~GridFork() { join(); }
  void note(hipError_t e) { if (err == hipSuccess) err = e; }
  void begin() {                                        // everything queued so far, the staged mask included, is in front of the build
    const hipError_t e = hipEventRecord(c->grid_fork, c->stream);
    note(e);
    if (e == hipSuccess) note(hipStreamWaitEvent(c->grid_stream, c->grid_fork, 0));
    open = true;
  }
  void launched() { note(hipEventRecord(c->grids_done, c->grid_stream)); }
  void join() {
    if (open && err == hipSuccess) note(hipStreamWaitEvent(c->stream, c->grids_done, 0));
    open = false;
  }
};

// Workgroups of the persistent build that runs beside k_ring_features.  Measured at batch 2048 (HISTORY, round 9): below 64 the build is bound by its
// CUs and outlasts the ring kernel (48: 6.2 ms), from 64 to 128 the step is flat within 0.1 ms, above that the ring kernel loses more CUs than the
// build gains (192: + 0.35 ms, 256: + 1.0).  96: the build and the ring kernel end together.
constexpr int kGridWgsBesideRegistration = 96;

// One odometry step while it is being queued.  aloam_process_* begin it in front of their registration (odometry_begin) and fork its grid build
// inside the registration (odometry_fork_build); aloam_odometry_step on its own has only odometry_finish.
struct OdomStep {
  StageMask m;
  bool masked = false;                                  // m is this step's mask, staged
  bool beside_registration = false;                     // the grids this step searches are built, or were found built, by the time the fork is joined
  bool build = false;                                   // ... built: the registration of the call forks the build behind its k_front
  GridFork fork;
  explicit OdomStep(aloam_ctx* c) : fork(c) {}
};

// Per sequence: kSeqActive = takes part (swaps), kSeqSolve = takes part and is past its first frame (src/laserOdometry.cpp:267-271).  The
// kernels get no mask at all when every sequence solves: the launches of a lock-step batch are those of a context without the feature.
int odometry_mask(aloam_ctx* c, OdomStep* st) {         // (a first frame of the whole batch needs no mask either: k_advance swaps all)
  if (const int rc = stage_mask(c, c->d_mask_odo, [](const SeqHost& s) { return s.inited ? (int)kSeqSolve : 0; },
                                [](const aloam_ctx* x, const StageMask& k) { return k.all_solve || (!k.any_solve && x->all_active); }, &st->m)) return rc;
  st->masked = true;
  return ALOAM_OK;
}

// A call that registers a sweep and runs its odometry step (aloam_process_*) knows the step's mask before it queues anything: who takes part and who
// is past its first frame do not depend on the registration.  So it stages the mask first, and its registration can fork the build of the last
// clouds' grids - complete since the previous step swapped - onto the grid stream.  A context without the odometry stage, or with the serial chain
// (ALOAM_GRID_OVERLAP=0, use_graph, debug_sync), begins nothing here.
int odometry_begin(aloam_ctx* c, OdomStep* st) {
  if (!(c->stages & ALOAM_STAGE_ODOMETRY) || !c->grid_overlap) return ALOAM_OK;
  if (const int rc = odometry_mask(c, st)) return rc;
  st->beside_registration = true;                       // (a sequence that comes from an aloam_odometry_step of its own has its grids already)
  for (int b = 0; b < c->B; ++b) st->build |= (st->m.bits[b] & kSeqSolve) && !c->seq[b].grid_built;
  return ALOAM_OK;
}

// The fork, called by the registration between k_front and k_ring_starts.  The registration shares no data with the build: it writes the slabs,
// the feature buffers [parity] and its own SeqMeta fields (field stores, find_ends_body), the build reads the clouds [1 - parity], parity and
// n_*_last.  Where the fork stands is measured (HISTORY, round 9).  At the start of the call the build runs beside k_front, two kernels bound by
// memory traffic: k_front takes 3.9 instead of 2.1 ms and the build 7.9 instead of 3.2, which loses what the association gains.  k_ring_features is
// bound by instruction issue and shares better (5.2 instead of 3.7 ms for a build hidden whole).  Forked here, the build's 1024-thread workgroups
// are placed on an empty chip while the one-wave k_ring_starts runs; behind the launch of k_ring_features they would wait for it to drain.
void odometry_fork_build(aloam_ctx* c, OdomStep* st) {
  OdomArgs a = odom_args(c);
  a.active = st->m.dev;
  st->fork.begin();
  { ProfScope p(c, K_BUILD_GRIDS, c->grid_stream); launch_build_grids(a, GridBuild::kPersistentLast, kGridWgsBesideRegistration, c->grid_stream); }
  st->fork.launched();
}

// The registration of an aloam_process_* call with its step's fork in it.
int register_with_step(aloam_ctx* c, OdomStep* st, const void* d_scans, long long seq_stride, const int* n_in, int stride_bytes, int slot) {
  const std::function<void()> fork = [c, st]() { odometry_fork_build(c, st); };
  return register_launch(c, d_scans, seq_stride, n_in, stride_bytes, slot, /*debug_arrays=*/false, nullptr, st->build ? &fork : nullptr);
}

int odometry_finish(aloam_ctx* c, OdomStep* st) {
  if (const int rc = require_stage(c, ALOAM_STAGE_ODOMETRY)) return rc;
  if (!c->have_features) { c->err = "aloam_odometry_step before any features were registered / set"; return ALOAM_E_STATE; }
  if (!st->masked) if (const int rc = odometry_mask(c, st)) return rc;
  const StageMask& m = st->m;
  const int* mask = m.dev;
  const bool any_solve = m.any_solve;
  // The kd-tree stand-in of a step (launch_build_grids) covers clouds that were complete before the step began, so it need not wait for the step
  // that searches it.  Where the registration is part of the call, the build has run beside its k_ring_features (odometry_fork_build) and is joined
  // here, in front of the first k_transform_queries; such a step builds nothing for the next one.  An aloam_odometry_step on its own has no such
  // window: with grid_overlap it builds, on the grid stream and beside its own association and solve, the grids of the sweep it is about to make
  // the last one (the "next" form, into the grid set of that cloud buffer); the step after it finds them built (grid_built) and starts with the
  // association.  Either way the build is forked from and joined into the main stream inside the call.  A solving sequence of such a step whose
  // last clouds came from somewhere else (aloam_set_last, a loaded record, a step that built beside its registration) sends the step through the
  // serial "last" build first, which is also the whole schedule without grid_overlap.
  st->fork.join();
  const bool overlap = c->grid_overlap && !st->beside_registration;
  bool build_last = !c->grid_overlap;
  if (overlap) for (int b = 0; b < c->B; ++b) build_last |= (m.bits[b] & kSeqSolve) && !c->seq[b].grid_built;
  const int cus = c->gather_blocks / 8;                                           // (aloam_create: eight gather workgroups per CU)
  auto launch_all = [&]() {
    OdomArgs a = odom_args(c);
    a.active = mask;
    if (overlap) {
      st->fork.begin();
      { ProfScope p(c, K_BUILD_GRIDS, c->grid_stream); launch_build_grids(a, GridBuild::kPersistentNext, cus / 2, c->grid_stream); }
      st->fork.launched();
    }
    if (any_solve && build_last) {
      if (overlap) launch_build_grids(a, GridBuild::kSerialLast, 0, c->stream);        // (K_BUILD_GRIDS stays the one launch per step on the grid stream)
      else { ProfScope p(c, K_BUILD_GRIDS); launch_build_grids(a, GridBuild::kSerialLast, 0, c->stream); }   // kd-tree stand-in over the last clouds
    }
    for (int outer = 0; any_solve && outer < c->cfg.outer_iterations; ++outer) {  // (a first frame of every active sequence: no solve, src/laserOdometry.cpp:267-271)
      a.outer = outer;
      a.last_outer = outer == c->cfg.outer_iterations - 1;
      { ProfScope p(c, K_TRANSFORM); launch_transform_queries(a, c->stream); }    // TransformToStart of the features (:300, :388)
      { ProfScope p(c, K_ASSOC_CORNER); launch_associate(a, false, c->stream); }
      { ProfScope p(c, K_ASSOC_PLANE); launch_associate(a, true, c->stream); }
      { ProfScope p(c, K_SOLVE); launch_solve(a, c->stream); }
    }
    st->fork.join();                                               // the next step's grids, in front of the swap
    { ProfScope p(c, K_ADVANCE); launch_advance(a, c->stream); }   // swap (src/laserOdometry.cpp:554-563)
  };
  if (!any_solve) {
    launch_all();
  } else if (c->use_graph && !c->prof_on && !c->debug_sync) {
    // The kernel arguments of a step are the same every step (the buffer parity is per sequence, on the device; the mask is staged into the
    // same buffer), so the step is captured once per mask mode and replayed: one launch instead of ~15.  Measured at batch 1 (bench.py latency leg):
    // 0.418 ms per step against 0.416 ms with separate launches — the step is bound by the execution of its dependent kernels (one sequence fills
    // a fraction of the chip), not by launching them, so the path is kept (tested bit for bit) but off by default.
    GraphExec& ge = c->odom_graph[mask ? 1 : 0];
    if (!ge) {
      // A failed capture must not leave the stream in capture mode or leak the graph: the capture is always ended, the graph always
      // destroyed, and on any error this context goes back to separate launches for good (the step itself is then launched normally).
      hipGraph_t g = nullptr;
      hipError_t e = hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal);
      if (e == hipSuccess) {
        launch_all();
        e = hipStreamEndCapture(c->stream, &g);                  // launch errors inside the capture surface here
        if (e == hipSuccess) e = hipGraphInstantiate(&ge.h, g, nullptr, nullptr, 0);
        if (g) (void)hipGraphDestroy(g);
      }
      if (e != hipSuccess) {
        (void)hipGetLastError();                                 // clear the sticky capture error; the cause is not lost: the plain launches below report theirs
        ge.reset();
        c->use_graph = false;
      }
    }
    if (ge) HIP_TRY(c, hipGraphLaunch(ge, c->stream));
    else launch_all();
  } else {
    launch_all();
  }
  HIP_TRY(c, st->fork.err);
  HIP_TRY(c, hipGetLastError());
  on_odometry_advanced(c, m, /*built_next=*/overlap);
  return ALOAM_OK;
}

}  // namespace

extern "C" {

int aloam_scan_register_device(aloam_ctx* c, const void* d_scans, long long seq_stride_bytes, const int* n_in, int stride_bytes) {
  DeviceScope device_scope(c);
  if (!c || !d_scans || !n_in) return ALOAM_E_ARG;
  if (const int rc = check_batch(c, n_in, stride_bytes)) return rc;
  return register_launch(c, d_scans, seq_stride_bytes, n_in, stride_bytes);
}

int aloam_scan_register(aloam_ctx* c, const void* const* scans, const int* n_in, int stride_bytes) {
  DeviceScope device_scope(c);
  if (!c || !scans || !n_in) return ALOAM_E_ARG;
  int rc = check_batch(c, n_in, stride_bytes);
  if (rc) return rc;
  const size_t seq_stride = (size_t)c->cap * stride_bytes;
  int slot = 0;
  if ((rc = acquire_slab(c, seq_stride * c->B, &slot))) return rc;
  char* d_in = c->d_in[slot].get();
  for (int b = 0; b < c->B; ++b)
    if (n_in[b] > 0) HIP_TRY(c, hipMemcpyAsync(d_in + b * seq_stride, scans[b], (size_t)n_in[b] * stride_bytes, hipMemcpyHostToDevice, c->stream));
  if ((rc = register_launch(c, d_in, (long long)seq_stride, n_in, stride_bytes, slot))) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));   // the host buffers may be reused on return
  return ALOAM_OK;
}

// Host-resident batch in ONE buffer (sequence b at h_scans + b * seq_stride_bytes): one batched H2D copy on the context's copy
// stream into the next of two device slabs, the kernels wait for it on the compute stream — so the copy of call k + 1 runs
// under the kernels of call k.  Truly asynchronous only from pinned memory (hipHostMalloc / hipHostRegister); the runtime stages
// pageable memory synchronously.  The buffer must stay unmodified until aloam_input_consumed() / aloam_synchronize().
// step: the odometry step of the same call (aloam_process_host), begun as soon as the batch has passed its checks; the throughput entry keeps no debug arrays.
static int stage_and_register(aloam_ctx* c, const void* h_scans, long long seq_stride_bytes, const int* n_in, int stride_bytes, bool debug_arrays, OdomStep* step = nullptr) {
  if (!c || !h_scans || !n_in) return ALOAM_E_ARG;
  int rc = check_batch(c, n_in, stride_bytes);
  if (rc || (step && (rc = odometry_begin(c, step)))) return rc;
  const size_t d_seq_stride = (size_t)c->cap * stride_bytes;
  int slot = 0;
  char* d_in = nullptr;
  if ((rc = stage_batch(c, h_scans, seq_stride_bytes, (size_t)*std::max_element(n_in, n_in + c->B) * stride_bytes, (size_t)n_in[c->B - 1] * stride_bytes, d_seq_stride, &slot, &d_in))) return rc;
  if (step) return register_with_step(c, step, d_in, (long long)d_seq_stride, n_in, stride_bytes, slot);
  return register_launch(c, d_in, (long long)d_seq_stride, n_in, stride_bytes, slot, debug_arrays);
}

int aloam_scan_register_host(aloam_ctx* c, const void* h_scans, long long seq_stride_bytes, const int* n_in, int stride_bytes) {
  DeviceScope device_scope(c);
  return stage_and_register(c, h_scans, seq_stride_bytes, n_in, stride_bytes, true);
}

int aloam_process_host(aloam_ctx* c, const void* h_scans, long long seq_stride_bytes, const int* n_in, int stride_bytes) {
  DeviceScope device_scope(c);
  if (!c) return ALOAM_E_ARG;
  OdomStep st(c);
  if (const int rc = stage_and_register(c, h_scans, seq_stride_bytes, n_in, stride_bytes, false, &st)) return rc;
  return odometry_finish(c, &st);
}

int aloam_input_consumed(aloam_ctx* c) {
  DeviceScope device_scope(c);
  if (!c) return ALOAM_E_ARG;
  for (int s = 0; s < 2; ++s) if (c->in_used[s]) HIP_TRY(c, hipEventSynchronize(c->in_consumed[s]));
  return ALOAM_OK;
}

int aloam_odometry_step(aloam_ctx* c) {
  DeviceScope device_scope(c);
  if (!c) return ALOAM_E_ARG;
  OdomStep st(c);
  return odometry_finish(c, &st);
}

int aloam_process_device(aloam_ctx* c, const void* d_scans, long long seq_stride_bytes, const int* n_in, int stride_bytes) {
  DeviceScope device_scope(c);
  if (!c || !d_scans || !n_in) return ALOAM_E_ARG;
  int rc = check_batch(c, n_in, stride_bytes);
  if (rc) return rc;
  OdomStep st(c);                                       // (joins the grid stream on every way out)
  if ((rc = odometry_begin(c, &st)) || (rc = register_with_step(c, &st, d_scans, seq_stride_bytes, n_in, stride_bytes, -1))) return rc;
  return odometry_finish(c, &st);
}

// ---- results ---------------------------------------------------------------------------------------------
int aloam_cloud_size(aloam_ctx* c, int seq, int which) {
  DeviceScope device_scope(c);
  const float4* p; int n;
  const int rc = find_cloud(c, seq, which < ALOAM_EXPORT_MAP ? which : -1, &p, &n);   // (the map clouds: aloam_get_map_cloud)
  return rc ? rc : n;
}

int aloam_get_cloud(aloam_ctx* c, int seq, int which, float* out, int cap_points) {
  DeviceScope device_scope(c);
  const float4* p; int n;
  if (const int rc = find_cloud(c, seq, which < ALOAM_EXPORT_MAP ? which : -1, &p, &n)) return rc;
  const int k = n < cap_points ? n : cap_points;
  if (k > 0) HIP_TRY(c, hipMemcpy(out, p, sizeof(float4) * k, hipMemcpyDeviceToHost));
  return n;
}

int aloam_get_pose(aloam_ctx* c, int seq, double q_w[4], double t_w[3], double q_lc[4], double t_lc[3]) {
  DeviceScope device_scope(c);
  int rc = check_seq(c, seq);
  if (rc) return rc;
  OdomState s;
  if ((rc = read_seq(c, c->d_state.get() + seq, &s))) return rc;
  for (int k = 0; k < 4; ++k) { q_w[k] = s.q_w[k]; q_lc[k] = s.para_q[k]; }
  for (int k = 0; k < 3; ++k) { t_w[k] = s.t_w[k]; t_lc[k] = s.para_t[k]; }
  return ALOAM_OK;
}

int aloam_get_odom_stats(aloam_ctx* c, int seq, aloam_odom_stats* out) {
  DeviceScope device_scope(c);
  int rc = check_seq(c, seq);
  if (rc) return rc;
  OdomState s;
  if ((rc = read_seq(c, c->d_state.get() + seq, &s))) return rc;
  for (int k = 0; k < 2; ++k) {
    out->corner_corr[k] = s.corner_corr[k]; out->plane_corr[k] = s.plane_corr[k];
    out->lm_iterations[k] = s.lm_iterations[k]; out->lm_successful[k] = s.lm_successful[k];
    out->initial_cost[k] = s.initial_cost[k]; out->final_cost[k] = s.final_cost[k]; out->termination[k] = s.termination[k];
  }
  return ALOAM_OK;
}

// ---- state injection -----------------------------------------------------------------------------------------
int aloam_set_features(aloam_ctx* c, int seq, const float* sharp, int n_sharp, const float* less_sharp, int n_less_sharp,
                       const float* flat, int n_flat, const float* less_flat, int n_less_flat) {
  DeviceScope device_scope(c);
  int rc = check_seq(c, seq);
  if (rc) return rc;
  struct { int id, n; const float* pts; ExportSrc s; } in[4] = {
      {ALOAM_CLOUD_SHARP, n_sharp, sharp}, {ALOAM_CLOUD_LESS_SHARP, n_less_sharp, less_sharp}, {ALOAM_CLOUD_FLAT, n_flat, flat}, {ALOAM_CLOUD_LESS_FLAT, n_less_flat, less_flat}};
  for (auto& x : in) if (x.n < 0 || x.n > cloud_desc(c, x.id, &x.s)) { c->err = "feature cloud larger than the selection rules allow"; return ALOAM_E_CAPACITY; }
  for (auto& x : in) if (!cloud_row(c, x.s, seq)) { c->err = "this context has no feature buffers (created for the mapping stage only)"; return ALOAM_E_STATE; }
  c->inject_max = std::max(c->inject_max, std::max(n_less_sharp, n_less_flat));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  for (auto& x : in) if (x.n) HIP_TRY(c, hipMemcpy(cloud_row(c, x.s, seq), x.pts, sizeof(float4) * x.n, hipMemcpyHostToDevice));
  if ((rc = edit_seq(c, c->d_meta.get() + seq, [&](SeqMeta& m) { m.n_sharp = n_sharp; m.n_less_sharp = n_less_sharp; m.n_flat = n_flat; m.n_less_flat = n_less_flat; m.err = 0; }))) return rc;
  c->have_features = true;
  on_odometry_inputs_replaced(c, seq);
  return ALOAM_OK;
}

int aloam_set_last(aloam_ctx* c, int seq, const float* corner_last, int n_corner, const float* surf_last, int n_surf) {
  DeviceScope device_scope(c);
  int rc = check_seq(c, seq);
  if (rc) return rc;
  struct { int id, n; const float* pts; ExportSrc s; } in[2] = {{ALOAM_CLOUD_CORNER_LAST, n_corner, corner_last}, {ALOAM_CLOUD_SURF_LAST, n_surf, surf_last}};
  for (auto& x : in) if (x.n < 0 || x.n > cloud_desc(c, x.id, &x.s)) { c->err = "last cloud too large"; return ALOAM_E_CAPACITY; }
  for (auto& x : in) if (!cloud_row(c, x.s, seq)) { c->err = "this context has no buffers for the last clouds (created for the registration stage only)"; return ALOAM_E_STATE; }
  c->inject_max = std::max(c->inject_max, std::max(n_corner, n_surf));   // what the next mapping step may add (never lowers the bound)
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  on_last_clouds_replaced(c, seq);
  for (auto& x : in) if (x.n) HIP_TRY(c, hipMemcpy(cloud_row(c, x.s, seq), x.pts, sizeof(float4) * x.n, hipMemcpyHostToDevice));
  return edit_seq(c, c->d_meta.get() + seq, [&](SeqMeta& m) { m.n_corner_last = n_corner; m.n_surf_last = n_surf; });
}

int aloam_set_state(aloam_ctx* c, int seq, const double para_q[4], const double para_t[3], const double q_w[4], const double t_w[3]) {
  DeviceScope device_scope(c);
  int rc = check_seq(c, seq);
  if (rc) return rc;
  on_odometry_inputs_replaced(c, seq);
  return edit_seq(c, c->d_state.get() + seq, [&](OdomState& s) {
    for (int k = 0; k < 4; ++k) { s.para_q[k] = para_q[k]; s.q_w[k] = q_w[k]; }
    for (int k = 0; k < 3; ++k) { s.para_t[k] = para_t[k]; s.t_w[k] = t_w[k]; }
  });
}

int aloam_set_system_inited(aloam_ctx* c, int inited) {
  DeviceScope device_scope(c);
  if (!c) return ALOAM_E_ARG;
  on_system_inited_forced(c, inited != 0 ? 1 : 0);
  launch_set_inited(c->d_state.get(), c->B, inited != 0 ? 1 : 0, c->stream);
  HIP_TRY(c, hipGetLastError());
  return ALOAM_OK;
}

int aloam_set_full_cloud(aloam_ctx* c, int seq, const float* cloud, int n) {
  DeviceScope device_scope(c);
  int rc = check_seq(c, seq);
  if (rc) return rc;
  ExportSrc s;
  if (n < 0 || n > cloud_desc(c, ALOAM_CLOUD_FULL, &s)) { c->err = "cloud too large"; return ALOAM_E_CAPACITY; }
  if ((rc = ensure_dense(c))) return rc;                // the other sequences' clouds of the last registration, before this one is replaced
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (n) HIP_TRY(c, hipMemcpy(cloud_row(c, s, seq), cloud, sizeof(float4) * n, hipMemcpyHostToDevice));   // (every context has the full cloud)
  return edit_seq(c, c->d_meta.get() + seq, [&](SeqMeta& m) { m.n_cloud = n; });
}

// ---- intermediate arrays ---------------------------------------------------------------------------------------
int aloam_get_ring_ranges(aloam_ctx* c, int seq, int* start, int* count) {
  DeviceScope device_scope(c);
  int rc = check_seq(c, seq);
  if (rc) return rc;
  if ((rc = require_stage(c, ALOAM_STAGE_REGISTRATION))) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  std::vector<int> rs(c->R + 1);
  HIP_TRY(c, hipMemcpy(rs.data(), c->d_ringstart.get() + (size_t)seq * (c->R + 1), sizeof(int) * (c->R + 1), hipMemcpyDeviceToHost));
  for (int r = 0; r < c->R; ++r) { start[r] = rs[r]; count[r] = rs[r + 1] - rs[r]; }
  return c->R;
}

int aloam_get_curvature(aloam_ctx* c, int seq, float* out, int cap) {
  DeviceScope device_scope(c);
  int rc = check_seq(c, seq);
  if (rc) return rc;
  if ((rc = require_stage(c, ALOAM_STAGE_REGISTRATION))) return rc;
  if (!c->debug_arrays) { c->err = "curvature is only kept by aloam_scan_register*; the throughput entries (aloam_process_*) skip it"; return ALOAM_E_STATE; }
  SeqMeta m;
  if ((rc = read_seq(c, c->d_meta.get() + seq, &m))) return rc;
  const int k = m.n_cloud < cap ? m.n_cloud : cap;
  if (k > 0) HIP_TRY(c, hipMemcpy(out, c->d_curv.get() + (size_t)seq * c->cap, sizeof(float) * k, hipMemcpyDeviceToHost));
  return m.n_cloud;
}

int aloam_get_labels(aloam_ctx* c, int seq, int* out, int cap) {
  DeviceScope device_scope(c);
  int rc = check_seq(c, seq);
  if (rc) return rc;
  if ((rc = require_stage(c, ALOAM_STAGE_REGISTRATION))) return rc;
  if (!c->debug_arrays) { c->err = "labels are only kept by aloam_scan_register*; the throughput entries (aloam_process_*) skip them"; return ALOAM_E_STATE; }
  SeqMeta m;
  if ((rc = read_seq(c, c->d_meta.get() + seq, &m))) return rc;
  const int k = m.n_cloud < cap ? m.n_cloud : cap;
  std::vector<int8_t> tmp(k > 0 ? k : 1);
  if (k > 0) HIP_TRY(c, hipMemcpy(tmp.data(), c->d_label.get() + (size_t)seq * c->cap, k, hipMemcpyDeviceToHost));
  for (int i = 0; i < k; ++i) out[i] = tmp[i];
  return m.n_cloud;
}

// What the k_solve launches of this context keep in LDS (odometry_solve_device.hpp): plane slots and edge slots per thread, bytes of dynamic LDS.
int aloam_get_solve_lds(aloam_ctx* c, int out[3]) {
  if (!c || !out) return ALOAM_E_ARG;
  if (!c->d_edges) { c->err = "this context has no odometry stage"; return ALOAM_E_STATE; }
  solve_launch_lds(odom_args(c), out);
  return ALOAM_OK;
}

// Which association kernels owned the clouds the sequence's last step searched (k_build_grids_fused): per cloud 0 = ring-sorted keys (pair kernel), 1 = nearly
// ring-sorted (pair kernel with the index-range walk window), 2 = not sorted (literal walks), -1 = keys / coordinates out of range (literal search).
int aloam_get_last_cloud_order(aloam_ctx* c, int seq, int out[2]) {
  DeviceScope device_scope(c);
  int rc = check_seq(c, seq);
  if (rc) return rc;
  if (!c->d_grid_flags[0][0]) { c->err = "this context has no odometry stage"; return ALOAM_E_STATE; }
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  // The step searched the grids of cloud buffer 1 - parity and flipped the parity afterwards: that set is the one of the buffer `parity` names now.
  const int set = c->seq[seq].parity;
  for (int k = 0; k < 2; ++k) {
    int f[4];
    HIP_TRY(c, hipMemcpy(f, c->d_grid_flags[set][k].get() + (size_t)seq * 4, sizeof(f), hipMemcpyDeviceToHost));
    out[k] = f[0] ? -1 : f[1];
  }
  return ALOAM_OK;
}

int aloam_get_correspondences(aloam_ctx* c, int seq, float* edges, int cap_edges, int* n_edges, int* edge_query,
                              float* planes, int cap_planes, int* n_planes, int* plane_query) {
  DeviceScope device_scope(c);
  int rc = check_seq(c, seq);
  if (rc) return rc;
  SeqMeta m;
  if ((rc = read_seq(c, c->d_meta.get() + seq, &m))) return rc;
  std::vector<EdgeRec> E(m.n_sharp > 0 ? m.n_sharp : 1);
  std::vector<PlaneRec> P(m.n_flat > 0 ? m.n_flat : 1);
  if (m.n_sharp > 0) HIP_TRY(c, hipMemcpy(E.data(), c->d_edges.get() + (size_t)seq * c->R * kSharpPerRing, sizeof(EdgeRec) * m.n_sharp, hipMemcpyDeviceToHost));
  if (m.n_flat > 0) HIP_TRY(c, hipMemcpy(P.data(), c->d_planes.get() + (size_t)seq * c->R * kFlatPerRing, sizeof(PlaneRec) * m.n_flat, hipMemcpyDeviceToHost));
  int ne = 0, np = 0;
  for (int i = 0; i < m.n_sharp; ++i) {
    if (!E[i].valid) continue;
    if (ne < cap_edges) {
      float* o = edges + (size_t)ne * 9;
      for (int k = 0; k < 3; ++k) { o[k] = E[i].cp[k]; o[3 + k] = E[i].a[k]; o[6 + k] = E[i].b[k]; }
      if (edge_query) edge_query[ne] = i;
    }
    ++ne;
  }
  for (int i = 0; i < m.n_flat; ++i) {
    if (!P[i].valid) continue;
    if (np < cap_planes) {
      float* o = planes + (size_t)np * 12;
      for (int k = 0; k < 3; ++k) { o[k] = P[i].cp[k]; o[3 + k] = P[i].j[k]; o[6 + k] = P[i].l[k]; o[9 + k] = P[i].m[k]; }
      if (plane_query) plane_query[np] = i;
    }
    ++np;
  }
  *n_edges = ne;
  *n_planes = np;
  return ALOAM_OK;
}

}  // extern "C"
