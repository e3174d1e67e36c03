// a-loam_amd/csrc/aloam_capi.hip — host side of libaloam_mi355x.so: context, device buffers, launch sequencing and
// the extern "C" surface declared in include/aloam_mi355x.h.  There is no CPU fallback anywhere in this file:
// without a HIP device every entry point fails with ALOAM_E_HIP.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "../../include/aloam_mi355x.h"
#include "aloam_device.hpp"
#include "checkpoint_kernels.hpp"
#include "export_kernels.hpp"
#include "mapping_kernels.hpp"
#include "odometry_kernels.hpp"
#include "registration_kernels.hpp"

using namespace aloam;

namespace {
enum KernelId { K_FIND_ENDS = 0, K_FRONT, K_RING_STARTS, K_DENSE_CLOUD, K_RING_FEATURES, K_BUILD_GRIDS, K_TRANSFORM, K_ASSOC_CORNER,
                K_ASSOC_PLANE, K_SOLVE, K_ADVANCE, K_MAP_BEGIN, K_MAP_VOXEL_STACK, K_MAP_GRID, K_MAP_ASSOC, K_MAP_SOLVE, K_MAP_INSERT,
                K_MAP_VOXEL_CUBES, K_MAP_REGISTER, K_EXPORT, K_SAVE, K_LOAD, K_COUNT };
const char* const kKernelNames[] = {"k_find_ends", "k_front", "k_ring_starts", "k_dense_cloud", "k_ring_features",
                                    "k_build_grids", "k_transform_queries", "k_associate[corner]", "k_associate[plane]",
                                    "k_solve", "k_advance", "map_begin", "map_voxel[stacks]", "map_grid", "map_associate", "map_solve",
                                    "map_insert", "map_voxel[cubes]", "map_register", "export_clouds", "save_sequences",
                                    "load_sequences"};
static_assert(sizeof(kKernelNames) / sizeof(kKernelNames[0]) == K_COUNT, "one name per KernelId, in the same order");
struct ProfRec { int kernel; hipEvent_t e0, e1; };
constexpr int kNinSlots = 8;

// Owners of everything the context allocates: released by their destructors when the context is deleted, so a failed
// allocation or copy half way through leaks nothing.
struct DeviceFree { void operator()(void* p) const { (void)hipFree(p); } };
struct PinnedFree { void operator()(const volatile void* p) const { (void)hipHostFree(const_cast<void*>(p)); } };
template <typename T> using DevBuf = std::unique_ptr<T[], DeviceFree>;
template <typename T> using PinnedBuf = std::unique_ptr<T[], PinnedFree>;
// A stream, event or graph: converts to the raw handle, so call sites read as with the handle itself.
template <typename H, hipError_t (*Destroy)(H)>
struct Handle {
  H h = nullptr;
  Handle() = default;
  Handle(Handle&& o) noexcept : h(std::exchange(o.h, nullptr)) {}   // (no copies, no assignment)
  ~Handle() { reset(); }
  void reset() { if (h) (void)Destroy(h); h = nullptr; }
  operator H() const { return h; }
};
using Stream = Handle<hipStream_t, hipStreamDestroy>;
using Event = Handle<hipEvent_t, hipEventDestroy>;
using GraphExec = Handle<hipGraphExec_t, hipGraphExecDestroy>;

template <typename T>
hipError_t dalloc(DevBuf<T>& p, size_t count) {
  T* raw = nullptr;
  const hipError_t e = hipMalloc((void**)&raw, count * sizeof(T));
  p.reset(raw);
  return e;
}

// Everything whose size follows the map pool (map_alloc_pool): built fresh and committed with one move when the pool grows.
struct MapPool {
  int points = 0, H = 0;             // pool points per sequence and class, buckets of the submap grid
  int cube_levels = 0, tile_cap = 0, tile_bound = 0;   // general voxel path: merge levels of a cube, tile list capacity, tiles of the per-cube pass
  long long key_cap = 0;
  DevBuf<float4> pool[2], grid_sorted[2], voxtmp;
  DevBuf<int> grid_start[2], tile_seg, tile_heads, tile_pref;
  DevBuf<unsigned long long> keys[2];
};
}  // namespace

struct aloam_ctx {
  // Streams and events first: members are destroyed in reverse order, so every buffer is released before them.
  Stream stream, copy_stream;
  Event in_copied[2], in_consumed[2], nin_done[kNinSlots], map_step_done[4];
  std::vector<Event> prof_events;    // every profiling event created (prof_event); prof_free lists the idle ones
  // small batches (the ROS shims run batch 1): the ~15 dependent launches of an odometry step as ONE hipGraph launch; [0] every sequence
  // solves (no mask), [1] through the staged mask d_mask_odo
  GraphExec odom_graph[2];
  aloam_config cfg{};
  int stages = ALOAM_STAGE_ALL;      // which stages this context has buffers for (aloam_create_stages)
  int B = 0, cap = 0, R = 0, NB = 0, npad = 0;   // cap: points per sequence the big buffers are laid out for = max_points + padding (below)
  int max_points = 0;                   // what the caller may hand in (aloam_config.max_points)
  std::string err;
  // input staging (host-input path only)
  // two device slabs: the H2D copy of call k + 1 (copy stream) overlaps the kernels of call k (compute stream)
  DevBuf<char> d_in[2]; size_t d_in_bytes[2] = {0, 0};
  int in_slot = 0;
  bool in_used[2] = {false, false};
  DevBuf<int> d_nin;
  PinnedBuf<int> h_nin; int h_nin_slot = 0;         // pinned ring of kNinSlots x B ints (counts, masks, reset ids): an async H2D copy reads its slot later
  bool nin_used[kNinSlots] = {};
  // per-sequence lifecycle (aloam_set_active / aloam_reset_sequences)
  std::vector<int> active;                          // [B] the mask in force, 0 / 1
  bool all_active = true;
  std::vector<int> reg_active;                      // the mask of the last registration, while its odometry step is still to come (reg_pending)
  bool reg_pending = false;
  const int* reg_mask = nullptr;                    // what the last registration's kernels were given (nullptr = all); k_dense_cloud reuses it
  std::vector<int> parity, inited;                  // host mirrors of SeqMeta::parity and OdomState::inited: both change only through host calls
  std::vector<char> needs_odom;                     // [B] loaded by aloam_load_sequences and not yet through an odometry step: may not map
  DevBuf<int> d_mask_reg, d_mask_odo, d_mask_map, d_reset_ids;   // [B] each: masks as the launches of one stage see them, ids of a reset
  DevBuf<SeqMeta> d_meta;
  DevBuf<float4> d_slabs; int slab = 0;             // ring-ordered points, one slab per (sequence, ring): what k_front writes and the feature kernels read
  DevBuf<unsigned long long> d_front_lb; DevBuf<int> d_front_ticket;
  bool dense_valid = true;                          // d_cloud holds the dense concatenation of the current slabs (k_dense_cloud, on demand)
  DevBuf<int> d_ringstart;
  DevBuf<float4> d_cloud; DevBuf<float> d_curv; DevBuf<int8_t> d_label;
  DevBuf<unsigned long long> d_lookback; unsigned reg_epoch = 0;   // ring-count granules of k_ring_features, launch counter
  DevBuf<int> d_ring_ticket;                                       // per sweep: rings handed out to the workgroups of the running k_ring_features
  bool debug_arrays = false;                                       // the last registration wrote curvature / labels
  DevBuf<float4> d_sharp, d_flat;
  DevBuf<float4> d_less_sharp[2], d_less_flat[2];   // a sequence's CURRENT sweep is in [parity[b]], its last clouds in [1 - parity[b]]
  DevBuf<OdomState> d_state;
  DevBuf<float4> d_grid_sorted3[2], d_grid_sorted2[2];
  DevBuf<int> d_grid_start3[2], d_grid_start2[2];
  DevBuf<float4> d_grid_sorted3c[2];   // coarse level of the 3-D grid
  DevBuf<int> d_grid_start3c[2];
  DevBuf<int> d_grid_flags[2], d_grid_walk[2];
  int grid_H[2] = {4096, 16384};
  DevBuf<EdgeRec> d_edges; DevBuf<PlaneRec> d_planes;
  DevBuf<float4> d_sel_sharp, d_sel_flat;
  // scan-to-map refinement (allocated by aloam_mapping_enable)
  bool map_on = false;
  long long map_err_reported = 0;    // voxel-scratch capacity events (vox counters[3]) aloam_synchronize has already returned
  std::vector<long long> map_err_seen;   // per sequence: pool capacity events (MapSeq.err_steps) already returned
  float map_line_res = 0.4f, map_plane_res = 0.8f;
  int map_levels = 0, map_stack_tile_bound = 0, map_nsegs_max = 0;   // general voxel path over the incoming clouds: merge levels, tiles
  MapPool map;                       // the pool-sized state (map_alloc_pool)
  // pool growth (map_ensure_capacity): the reference's cubes are std::vectors that grow without bound (src/laserMapping.cpp:737-783)
  int map_pool_limit = 1 << 26;      // ceiling per sequence and class (aloam_mapping_set_pool_limit); ALOAM_E_CAPACITY only there
  int map_growths = 0;
  long long map_steps = 0;           // mapping steps queued so far
  // What one mapping step can add to a map is bounded by the largest of: the active rows of the last registration, and the clouds injected
  // since the last mapping step (aloam_set_last / aloam_set_features).  An injection raises the bound, never lowers it.
  int nin_max = 0;                   // largest active scan of the last registration call
  int inject_max = 0;                // largest cloud injected since the last mapping step
  PinnedBuf<volatile int> h_map_report;   // pinned: {step, live corner, live surf, stack corner, stack surf} of the last finished step
  int* d_map_report_host = nullptr;       // the same memory as the device sees it
  DevBuf<int> d_map_report, d_map_live;
  DevBuf<MapSeq> d_mapseq; DevBuf<CubeDesc> d_cubes; DevBuf<int> d_maptab;
  DevBuf<float4> d_stack[2], d_stack_world[2]; DevBuf<int> d_stack_cube[2];
  DevBuf<int> d_addcnt, d_cursor, d_compact_flag;
  DevBuf<MapEdgeRec> d_medges; DevBuf<MapNormRec> d_mnorms; DevBuf<float4> d_registered, d_knn;
  DevBuf<int> d_vox_lists;
  DevBuf<int> d_rec_tiles; int rec_tiles_corner = 0, rec_tiles_per_seq = 0;
  DevBuf<VoxSeg> d_segs; DevBuf<int> d_vox_counters, d_bbox;
  // batched export (aloam_export_clouds, and the cube-list clouds of aloam_get_map_cloud): scratch of count / scan / gather, used in stream order
  DevBuf<int> d_exp_cnt, d_exp_chunk; DevBuf<long long> d_exp_off;   // [ALOAM_EXPORT_MAX_IDS * B] points and [.. + 1] chunk / point offsets per segment
  DevBuf<int> d_exp_pref[2];                                         // entry prefixes of the cube lists, [B][151] surround, [B][9703] full map (on first use)
  int exp_last_segs = 0;                                             // segments of the last export (its algorithmic bytes)
  int gather_blocks = 2048;                                          // workgroups of the persistent k_export_gather: 8 per CU
  DevBuf<float4> d_exp_tmp; long long exp_tmp_cap = 0;              // aloam_get_map_cloud(SURROUND / FULL): the segment of one sequence
  DevBuf<long long> d_exp_tmp_off;
  // sequence records (aloam_save_sequences / aloam_load_sequences): scratch sized for `batch` records on first use, used in stream order
  DevBuf<int> d_ck_seqs, d_ck_info, d_ck_units, d_ck_chunk, d_ck_pref; DevBuf<long long> d_ck_uoff;   // save: ids, counts, lengths, prefixes
  PinnedBuf<char> h_ck; char* d_ck_host = nullptr;                  // load: headers read back, then the staged offsets / chunks / counts (pinned, mapped)
  DevBuf<char> d_ck_load;                                           // load: the same staged arrays in device memory
  DevBuf<char> d_ck_stage; size_t ck_stage_bytes = 0;               // load: records from pageable host memory
  int ck_save_n = 0; long long ck_load_bytes = 0;                   // the last save / load (algorithmic bytes)
  int sum_order = 0;                 // ALOAM_SUM_INPUT_ORDER / ALOAM_SUM_REFERENCE_ORDER (aloam_set_voxel_sum_order)
  bool use_graph = false;            // batch <= ALOAM_GRAPH_MAX_BATCH (environment, default 0 = off), read once at creation
  bool have_features = false;
  // profiling
  bool prof_on = false;
  bool debug_sync = false;           // environment ALOAM_DEBUG_SYNC, read once at creation
  std::vector<ProfRec> prof_pending;
  std::vector<hipEvent_t> prof_free;
  double prof_ms[K_COUNT] = {0};
  long long prof_launches[K_COUNT] = {0};
};

#define HIP_TRY(ctx, expr)                                                                                   \
  do {                                                                                                       \
    hipError_t e__ = (expr);                                                                                 \
    if (e__ != hipSuccess) {                                                                                 \
      (ctx)->err = std::string(#expr) + ": " + hipGetErrorString(e__);                                       \
      return ALOAM_E_HIP;                                                                                    \
    }                                                                                                        \
  } while (0)

namespace {

// allocate and zero on the context's stream: the kernels rely on zeroed look-back granules, tickets and counters
template <typename T>
int dmalloc(aloam_ctx* c, DevBuf<T>& p, size_t count) {
  HIP_TRY(c, dalloc(p, count));
  HIP_TRY(c, hipMemsetAsync(p.get(), 0, count * sizeof(T), c->stream));
  return ALOAM_OK;
}

hipEvent_t prof_event(aloam_ctx* c) {
  if (!c->prof_free.empty()) { hipEvent_t e = c->prof_free.back(); c->prof_free.pop_back(); return e; }
  Event e;
  (void)hipEventCreate(&e.h);
  c->prof_events.push_back(std::move(e));
  return c->prof_events.back();
}
struct ProfScope {
  aloam_ctx* c; int k; hipEvent_t e0 = nullptr;
  ProfScope(aloam_ctx* c_, int k_) : c(c_), k(k_) {
    if (c->prof_on) { e0 = prof_event(c); (void)hipEventRecord(e0, c->stream); }
  }
  ~ProfScope() {
    if (c->prof_on) { hipEvent_t e1 = prof_event(c); (void)hipEventRecord(e1, c->stream); c->prof_pending.push_back({k, e0, e1}); }
    if (c->debug_sync) {   // ALOAM_DEBUG_SYNC=1: wait after every stage and name it, so that a device fault can be pinned on a kernel
      const hipError_t e = hipStreamSynchronize(c->stream);
      std::fprintf(stderr, "[aloam] %-22s %s\n", kKernelNames[k], e == hipSuccess ? "ok" : hipGetErrorString(e));
    }
  }
};
// Every entry point runs on the context's device whatever the calling thread's current device is, and leaves the caller's
// choice as it found it (several contexts on several devices in one process; frameworks that switch devices behind our back).
struct DeviceScope {
  int prev = -1;
  explicit DeviceScope(const aloam_ctx* c) {
    int cur = -1;
    if (c && hipGetDevice(&cur) == hipSuccess && cur != c->cfg.device && hipSetDevice(c->cfg.device) == hipSuccess) prev = cur;
  }
  ~DeviceScope() { if (prev >= 0) (void)hipSetDevice(prev); }
  DeviceScope(const DeviceScope&) = delete;
  DeviceScope& operator=(const DeviceScope&) = delete;
};

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

// n ints to device memory through the pinned ring: returns at once, the H2D copy runs in stream order (the slot is reused kNinSlots calls later,
// after the copy that read it has run).
int stage_ints(aloam_ctx* c, const int* src, int n, int* dst) {
  const int ns = c->h_nin_slot;
  c->h_nin_slot = (ns + 1) % kNinSlots;
  int* slot = c->h_nin.get() + (size_t)ns * c->B;
  if (c->nin_used[ns]) HIP_TRY(c, hipEventSynchronize(c->nin_done[ns]));   // the copy queued kNinSlots launches ago has read it
  std::memcpy(slot, src, sizeof(int) * n);
  HIP_TRY(c, hipMemcpyAsync(dst, slot, sizeof(int) * n, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipEventRecord(c->nin_done[ns], c->stream));
  c->nin_used[ns] = true;
  return ALOAM_OK;
}

// The mask in force for one stage's launches: nullptr when every sequence takes part (the kernels then load nothing), else staged into `dst`.
int stage_mask(aloam_ctx* c, DevBuf<int>& dst, const int** out) {
  *out = nullptr;
  if (c->all_active) return ALOAM_OK;
  if (!dst && dmalloc(c, dst, c->B)) return ALOAM_E_HIP;
  if (const int rc = stage_ints(c, c->active.data(), c->B, dst.get())) return rc;
  *out = dst.get();
  return ALOAM_OK;
}

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

// The dense ring-by-ring cloud (laserCloud of src/scanRegistration.cpp:246-252) is made from the slabs when a consumer of the FULL cloud asks for it.
int ensure_dense(aloam_ctx* c) {
  if (c->dense_valid) return ALOAM_OK;                  // (also: nothing registered yet, or the cloud was set from outside)
  { ProfScope p(c, K_DENSE_CLOUD); launch_dense_cloud(reg_args(c, nullptr, 0, 16), c->stream); }
  HIP_TRY(c, hipGetLastError());
  c->dense_valid = true;
  return ALOAM_OK;
}

OdomArgs odom_args(aloam_ctx* c) {
  OdomArgs a{};
  a.B = c->B; a.cap = c->cap; a.R = c->R;
  a.meta = c->d_meta.get(); a.state = c->d_state.get();
  a.sharp = c->d_sharp.get(); a.flat = c->d_flat.get();
  for (int k = 0; k < 2; ++k) { a.less_sharp[k] = c->d_less_sharp[k].get(); a.less_flat[k] = c->d_less_flat[k].get(); }
  for (int k = 0; k < 2; ++k) {
    a.grid_sorted3[k] = c->d_grid_sorted3[k].get(); a.grid_sorted2[k] = c->d_grid_sorted2[k].get(); a.grid_start3[k] = c->d_grid_start3[k].get();
    a.grid_sorted3c[k] = c->d_grid_sorted3c[k].get(); a.grid_start3c[k] = c->d_grid_start3c[k].get();
    a.grid_start2[k] = c->d_grid_start2[k].get();
    a.grid_flags[k] = c->d_grid_flags[k].get(); a.grid_walk[k] = c->d_grid_walk[k].get();
  }
  a.grid_H_corner = c->grid_H[0]; a.grid_H_surf = c->grid_H[1];
  a.edges = c->d_edges.get(); a.planes = c->d_planes.get();
  a.sel_sharp = c->d_sel_sharp.get(); a.sel_flat = c->d_sel_flat.get();
  a.lm_max_iterations = c->cfg.lm_max_iterations;
  a.distortion = c->cfg.distortion != 0;
  return a;
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

int sync_and_check(aloam_ctx* c) {
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return ALOAM_OK;
}

int fetch_meta(aloam_ctx* c, int seq, SeqMeta* m) {
  HIP_TRY(c, hipMemcpyAsync(m, c->d_meta.get() + seq, sizeof(SeqMeta), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return ALOAM_OK;
}

// The per-sequence struct at `dev` (SeqMeta, OdomState, MapSeq) read back after the stream has drained, changed by `edit`, written again.
template <typename T, typename Edit>
int edit_seq(aloam_ctx* c, T* dev, Edit edit) {
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  T v;
  HIP_TRY(c, hipMemcpy(&v, dev, sizeof(T), hipMemcpyDeviceToHost));
  edit(v);
  HIP_TRY(c, hipMemcpy(dev, &v, sizeof(T), hipMemcpyHostToDevice));
  return ALOAM_OK;
}

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

// debug_arrays: also write cloudCurvature / cloudLabel (the per-point entry points aloam_get_curvature / aloam_get_labels);
// the throughput entries (aloam_process_device / aloam_process_host) leave those 5 bytes per point out.  The batch has passed check_batch.
int register_launch(aloam_ctx* c, const void* d_scans, long long seq_stride, const int* n_in, int stride_bytes, int slot = -1, bool debug_arrays = true) {
  int rc = ALOAM_OK;
  // A sequence that sits out keeps its dense cloud: made now from its slabs if the last registration's was never asked for (a no-op otherwise)
  if (!c->all_active && (rc = ensure_dense(c))) return rc;
  c->nin_max = 0;
  for (int b = 0; b < c->B; ++b) if (c->all_active || c->active[b]) c->nin_max = std::max(c->nin_max, n_in[b]);
  if ((rc = stage_ints(c, n_in, c->B, c->d_nin.get()))) return rc;
  if ((rc = stage_mask(c, c->d_mask_reg, &c->reg_mask))) return rc;
  if (c->stages & ALOAM_STAGE_ODOMETRY) { c->reg_active = c->active; c->reg_pending = true; }
  c->debug_arrays = debug_arrays || c->sum_order != 0;      // the reference-order pass reads cloudLabel
  if (((++c->reg_epoch) & 0x7fffffffu) == 0) ++c->reg_epoch;                 // 31 bits of it tag the look-back granules; 0 = "never written"
  const RegArgs a = reg_args(c, d_scans, seq_stride, stride_bytes);
  { ProfScope p(c, K_FIND_ENDS); launch_find_ends(a, c->d_nin.get(), c->stream); }
  { ProfScope p(c, K_FRONT); launch_front(a, c->stream); }
  { ProfScope p(c, K_RING_STARTS); launch_ring_starts(a, c->stream); }
  c->dense_valid = false;
  if (slot >= 0) { HIP_TRY(c, hipEventRecord(c->in_consumed[slot], c->stream)); c->in_used[slot] = true; }   // the raw sweep is not read after this
  { ProfScope p(c, K_RING_FEATURES); launch_ring_features(a, c->npad, 0.2f, c->stream);     // leaf 0.2 (src/scanRegistration.cpp:404)
    if (c->sum_order) launch_less_flat_reference_order(reg_args(c, d_scans, seq_stride, stride_bytes), c->npad, 0.2f, c->stream); }
  HIP_TRY(c, hipGetLastError());
  c->have_features = true;
  return ALOAM_OK;
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
  c->active.assign(c->B, 1); c->parity.assign(c->B, 0); c->inited.assign(c->B, 0); c->needs_odom.assign(c->B, 0);
  // The per-sequence stride of every [B][cap] buffer is kept OFF the powers of two (131 072 points x 16 B = 2 MiB apart, the workgroups of a launch - one
  // per sequence, all at about the same offset of their sequence - meet on the same memory channels): + 1/32 + 16 points.  Measured on k_build_grids_fused at
  // batch 1024, one box: 1.62 - 1.65 ms at the power-of-two stride, 1.48 - 1.52 ms with 1040 / 4112 / 16 400 points of padding.
  c->cap = cfg->max_points + (((cfg->max_points / 32 + 15) & ~15) + 16);
  { const char* e = std::getenv("ALOAM_GRAPH_MAX_BATCH"); c->use_graph = c->B <= (e ? std::atoi(e) : 0); }   // off unless asked for: measured no gain (below)
  c->NB = (c->cap + kBlockPts - 1) / kBlockPts;
  c->npad = cfg->max_ring_points <= 2059 ? 2048 : 4096;
  const size_t B = c->B, cap = c->cap, R = c->R, NB = c->NB;
  int rc = 0;
  { int* p = nullptr; HIP_TRY(c, hipHostMalloc((void**)&p, sizeof(int) * B * kNinSlots, hipHostMallocDefault)); c->h_nin.reset(p); }
  for (Event& e : c->nin_done) HIP_TRY(c, hipEventCreateWithFlags(&e.h, hipEventDisableTiming));
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
    for (int k = 0; k < 2; ++k) {
      const size_t per = k == 0 ? R * kLessSharpPerRing : cap;
      if ((rc = dmalloc(c, c->d_grid_sorted3[k], B * per))) return rc;
      if ((rc = dmalloc(c, c->d_grid_sorted2[k], B * per))) return rc;
      if ((rc = dmalloc(c, c->d_grid_start3[k], B * (c->grid_H[k] + 1)))) return rc;
      if ((rc = dmalloc(c, c->d_grid_start2[k], B * (c->grid_H[k] + 1)))) return rc;
      if ((rc = dmalloc(c, c->d_grid_sorted3c[k], B * per))) return rc;
      if ((rc = dmalloc(c, c->d_grid_start3c[k], B * (c->grid_H[k] + 1)))) return rc;
      if ((rc = dmalloc(c, c->d_grid_flags[k], B * 4))) return rc;
      if ((rc = dmalloc(c, c->d_grid_walk[k], B * 2 * (R + 8)))) return rc;
    }
    if ((rc = dmalloc(c, c->d_edges, B * R * kSharpPerRing))) return rc;
    if ((rc = dmalloc(c, c->d_planes, B * R * kFlatPerRing))) return rc;
    if ((rc = dmalloc(c, c->d_sel_sharp, B * R * kSharpPerRing))) return rc;
    if ((rc = dmalloc(c, c->d_sel_flat, B * R * kFlatPerRing))) return rc;
    if ((rc = prepare_build_grids(c->grid_H[1]))) { c->err = "k_build_grids: dynamic LDS size rejected"; return ALOAM_E_HIP; }
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
    if ((int)c->map_err_seen.size() != c->B) c->map_err_seen.assign(c->B, 0);
    long long fresh_pool = 0;
    int first_seq = -1;
    for (int b = 0; b < c->B; ++b) {
      const long long n = ms[b].err_steps + ((ms[b].err & kMapErrPool) ? 1 : 0);
      if (n > c->map_err_seen[b]) { fresh_pool += n - c->map_err_seen[b]; if (first_seq < 0) first_seq = b; }
      c->map_err_seen[b] = n;
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
  }
  return ALOAM_OK;
}

int aloam_scan_register_device(aloam_ctx* c, const void* d_scans, long long seq_stride_bytes, const int* n_in, int stride_bytes) {
  DeviceScope device_scope(c);
  if (!c || !d_scans || !n_in) return ALOAM_E_ARG;
  if (const int rc = check_batch(c, n_in, stride_bytes)) return rc;
  return register_launch(c, d_scans, seq_stride_bytes, n_in, stride_bytes);
}

// Next device staging slab for a host-resident batch: waits (host side) until the kernels that read the slab two calls ago
// are done with it, grows it if needed (the old slab is released first: its contents are not needed).
static int acquire_slab(aloam_ctx* c, size_t need, int* slot_out) {
  const int s = c->in_slot;
  c->in_slot ^= 1;
  if (c->in_used[s]) HIP_TRY(c, hipEventSynchronize(c->in_consumed[s]));
  if (c->d_in_bytes[s] < need) {
    c->d_in_bytes[s] = 0;
    c->d_in[s].reset();
    HIP_TRY(c, dalloc(c->d_in[s], need));
    c->d_in_bytes[s] = need;
  }
  *slot_out = s;
  return ALOAM_OK;
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
static int stage_and_register(aloam_ctx* c, const void* h_scans, long long seq_stride_bytes, const int* n_in, int stride_bytes, bool debug_arrays) {
  if (!c || !h_scans || !n_in) return ALOAM_E_ARG;
  int rc = check_batch(c, n_in, stride_bytes);
  if (rc) return rc;
  if (seq_stride_bytes < 0) { c->err = "bad stride"; return ALOAM_E_ARG; }
  const size_t row = (size_t)*std::max_element(n_in, n_in + c->B) * stride_bytes;
  if (c->B > 1 && (size_t)seq_stride_bytes < row) { c->err = "seq_stride_bytes smaller than a scan"; return ALOAM_E_ARG; }
  const size_t d_seq_stride = (size_t)c->cap * stride_bytes;
  int slot = 0;
  if ((rc = acquire_slab(c, d_seq_stride * c->B, &slot))) return rc;
  char* d_in = c->d_in[slot].get();
  if (row > 0) {
    // rows 0 .. B-2 as one strided copy of the batch-wide maximum (every row but the last is followed by the next one, so the
    // extra bytes are readable); the last row with its own length, so that a buffer that ends with the last sweep is never over-read
    if (c->B > 1) HIP_TRY(c, hipMemcpy2DAsync(d_in, d_seq_stride, h_scans, (size_t)seq_stride_bytes, row, (size_t)c->B - 1, hipMemcpyHostToDevice, c->copy_stream));
    const size_t last = (size_t)n_in[c->B - 1] * stride_bytes;
    if (last > 0) HIP_TRY(c, hipMemcpyAsync(d_in + (size_t)(c->B - 1) * d_seq_stride, (const char*)h_scans + (size_t)(c->B - 1) * (size_t)seq_stride_bytes, last, hipMemcpyHostToDevice, c->copy_stream));
  }
  HIP_TRY(c, hipEventRecord(c->in_copied[slot], c->copy_stream));
  HIP_TRY(c, hipStreamWaitEvent(c->stream, c->in_copied[slot], 0));
  return register_launch(c, d_in, (long long)d_seq_stride, n_in, stride_bytes, slot, debug_arrays);
}

int aloam_scan_register_host(aloam_ctx* c, const void* h_scans, long long seq_stride_bytes, const int* n_in, int stride_bytes) {
  DeviceScope device_scope(c);
  return stage_and_register(c, h_scans, seq_stride_bytes, n_in, stride_bytes, true);
}

int aloam_process_host(aloam_ctx* c, const void* h_scans, long long seq_stride_bytes, const int* n_in, int stride_bytes) {
  DeviceScope device_scope(c);
  const int rc = stage_and_register(c, h_scans, seq_stride_bytes, n_in, stride_bytes, false);
  if (rc) return rc;
  return aloam_odometry_step(c);
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
  if (const int rc = require_stage(c, ALOAM_STAGE_ODOMETRY)) return rc;
  if (!c->have_features) { c->err = "aloam_odometry_step before any features were registered / set"; return ALOAM_E_STATE; }
  // Per sequence: kSeqActive = takes part (swaps), kSeqSolve = takes part and is past its first frame (src/laserOdometry.cpp:267-271).  The
  // kernels get no mask at all when every sequence solves: the launches of a lock-step batch are those of a context without the feature.
  std::vector<int> bits(c->B);
  bool any_solve = false, all_solve = true;
  for (int b = 0; b < c->B; ++b) {
    const bool on = c->all_active || c->active[b];
    bits[b] = on ? (kSeqActive | (c->inited[b] ? kSeqSolve : 0)) : 0;
    any_solve |= (bits[b] & kSeqSolve) != 0;
    all_solve &= (bits[b] & kSeqSolve) != 0;
  }
  const int* mask = nullptr;
  if (!all_solve && (any_solve || !c->all_active)) {             // (a first frame of the whole batch needs no mask: k_advance swaps all)
    if (!c->d_mask_odo && dmalloc(c, c->d_mask_odo, c->B)) return ALOAM_E_HIP;
    if (const int rc = stage_ints(c, bits.data(), c->B, c->d_mask_odo.get())) return rc;
    mask = c->d_mask_odo.get();
  }
  auto launch_all = [&]() {
    OdomArgs a = odom_args(c);
    a.active = mask;
    { ProfScope p(c, K_BUILD_GRIDS); launch_build_grids(a, c->stream); }          // kd-tree stand-in over the last clouds
    for (int outer = 0; outer < c->cfg.outer_iterations; ++outer) {
      a.outer = outer;
      a.last_outer = outer == c->cfg.outer_iterations - 1;
      { ProfScope p(c, K_TRANSFORM); launch_transform_queries(a, c->stream); }    // TransformToStart of the features (:300, :388)
      { ProfScope p(c, K_ASSOC_CORNER); launch_associate(a, false, c->stream); }
      { ProfScope p(c, K_ASSOC_PLANE); launch_associate(a, true, c->stream); }
      { ProfScope p(c, K_SOLVE); launch_solve(a, c->stream); }
    }
    { ProfScope p(c, K_ADVANCE); launch_advance(a, c->stream); }   // swap (src/laserOdometry.cpp:554-563)
  };
  if (!any_solve) {
    // first frame of every active sequence: no solve (src/laserOdometry.cpp:267-271)
    OdomArgs a = odom_args(c);
    a.active = mask;
    { ProfScope p(c, K_ADVANCE); launch_advance(a, c->stream); }
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
  HIP_TRY(c, hipGetLastError());
  for (int b = 0; b < c->B; ++b) if (bits[b] & kSeqActive) { c->parity[b] ^= 1; c->inited[b] = 1; c->needs_odom[b] = 0; }
  c->reg_pending = false;
  return ALOAM_OK;
}

int aloam_process_device(aloam_ctx* c, const void* d_scans, long long seq_stride_bytes, const int* n_in, int stride_bytes) {
  DeviceScope device_scope(c);
  if (!c || !d_scans || !n_in) return ALOAM_E_ARG;
  int rc = check_batch(c, n_in, stride_bytes);
  if (rc || (rc = register_launch(c, d_scans, seq_stride_bytes, n_in, stride_bytes, -1, /*debug_arrays=*/false))) return rc;
  return aloam_odometry_step(c);
}

// ---- results ---------------------------------------------------------------------------------------------
// Where cloud `which` of sequence `seq` lives on the device and how many points it holds.
static int find_cloud(aloam_ctx* c, int seq, int which, const float4** ptr, int* n) {
  int rc = check_seq(c, seq);
  if (rc || (which == ALOAM_CLOUD_FULL && (rc = ensure_dense(c)))) return rc;
  SeqMeta m;
  if ((rc = fetch_meta(c, seq, &m))) return rc;
  const size_t b = seq;
  const int cur = c->parity[seq];
  auto at = [](const DevBuf<float4>& base, size_t off) -> const float4* { return base ? base.get() + off : nullptr; };
  // aloam_odometry_step ends with the reference's pointer swap (src/laserOdometry.cpp:554-560): afterwards the sweep
  // just processed is read through CORNER_LAST / SURF_LAST, exactly like laserCloudCornerLast / laserCloudSurfLast.
  switch (which) {
    case ALOAM_CLOUD_FULL: *ptr = at(c->d_cloud, b * c->cap); *n = m.n_cloud; break;
    case ALOAM_CLOUD_SHARP: *ptr = at(c->d_sharp, b * c->R * kSharpPerRing); *n = m.n_sharp; break;
    case ALOAM_CLOUD_FLAT: *ptr = at(c->d_flat, b * c->R * kFlatPerRing); *n = m.n_flat; break;
    case ALOAM_CLOUD_LESS_SHARP: *ptr = at(c->d_less_sharp[cur], b * c->R * kLessSharpPerRing); *n = m.n_less_sharp; break;
    case ALOAM_CLOUD_LESS_FLAT: *ptr = at(c->d_less_flat[cur], b * c->cap); *n = m.n_less_flat; break;
    case ALOAM_CLOUD_CORNER_LAST: *ptr = at(c->d_less_sharp[1 - cur], b * c->R * kLessSharpPerRing); *n = m.n_corner_last; break;
    case ALOAM_CLOUD_SURF_LAST: *ptr = at(c->d_less_flat[1 - cur], b * c->cap); *n = m.n_surf_last; break;
    default: c->err = "unknown cloud id"; return ALOAM_E_ARG;
  }
  if (!*ptr) { c->err = "this context holds no such cloud (see aloam_create_stages)"; return ALOAM_E_STATE; }
  return ALOAM_OK;
}

int aloam_cloud_size(aloam_ctx* c, int seq, int which) {
  DeviceScope device_scope(c);
  const float4* p; int n;
  const int rc = find_cloud(c, seq, which, &p, &n);
  return rc ? rc : n;
}

int aloam_get_cloud(aloam_ctx* c, int seq, int which, float* out, int cap_points) {
  DeviceScope device_scope(c);
  const float4* p; int n;
  if (const int rc = find_cloud(c, seq, which, &p, &n)) return rc;
  const int k = n < cap_points ? n : cap_points;
  if (k > 0) HIP_TRY(c, hipMemcpy(out, p, sizeof(float4) * k, hipMemcpyDeviceToHost));
  return n;
}

int aloam_get_pose(aloam_ctx* c, int seq, double q_w[4], double t_w[3], double q_lc[4], double t_lc[3]) {
  DeviceScope device_scope(c);
  int rc = check_seq(c, seq);
  if (rc) return rc;
  if ((rc = sync_and_check(c))) return rc;
  OdomState s;
  HIP_TRY(c, hipMemcpy(&s, c->d_state.get() + seq, sizeof(OdomState), hipMemcpyDeviceToHost));
  for (int k = 0; k < 4; ++k) { q_w[k] = s.q_w[k]; q_lc[k] = s.para_q[k]; }
  for (int k = 0; k < 3; ++k) { t_w[k] = s.t_w[k]; t_lc[k] = s.para_t[k]; }
  return ALOAM_OK;
}

int aloam_get_odom_stats(aloam_ctx* c, int seq, aloam_odom_stats* out) {
  DeviceScope device_scope(c);
  int rc = check_seq(c, seq);
  if (rc) return rc;
  if ((rc = sync_and_check(c))) return rc;
  OdomState s;
  HIP_TRY(c, hipMemcpy(&s, c->d_state.get() + seq, sizeof(OdomState), hipMemcpyDeviceToHost));
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
  if (n_sharp < 0 || n_sharp > c->R * kSharpPerRing || n_less_sharp < 0 || n_less_sharp > c->R * kLessSharpPerRing || n_flat < 0 || n_flat > c->R * kFlatPerRing ||
      n_less_flat < 0 || n_less_flat > c->max_points) { c->err = "feature cloud larger than the selection rules allow"; return ALOAM_E_CAPACITY; }
  const int cur = c->parity[seq];
  if (!c->d_sharp || !c->d_less_sharp[cur]) { c->err = "this context has no feature buffers (created for the mapping stage only)"; return ALOAM_E_STATE; }
  c->inject_max = std::max(c->inject_max, std::max(n_less_sharp, n_less_flat));
  const size_t b = seq;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (n_sharp) HIP_TRY(c, hipMemcpy(c->d_sharp.get() + b * c->R * kSharpPerRing, sharp, sizeof(float4) * n_sharp, hipMemcpyHostToDevice));
  if (n_less_sharp) HIP_TRY(c, hipMemcpy(c->d_less_sharp[cur].get() + b * c->R * kLessSharpPerRing, less_sharp, sizeof(float4) * n_less_sharp, hipMemcpyHostToDevice));
  if (n_flat) HIP_TRY(c, hipMemcpy(c->d_flat.get() + b * c->R * kFlatPerRing, flat, sizeof(float4) * n_flat, hipMemcpyHostToDevice));
  if (n_less_flat) HIP_TRY(c, hipMemcpy(c->d_less_flat[cur].get() + b * c->cap, less_flat, sizeof(float4) * n_less_flat, hipMemcpyHostToDevice));
  if ((rc = edit_seq(c, c->d_meta.get() + seq, [&](SeqMeta& m) { m.n_sharp = n_sharp; m.n_less_sharp = n_less_sharp; m.n_flat = n_flat; m.n_less_flat = n_less_flat; m.err = 0; }))) return rc;
  c->have_features = true;
  return ALOAM_OK;
}

int aloam_set_last(aloam_ctx* c, int seq, const float* corner_last, int n_corner, const float* surf_last, int n_surf) {
  DeviceScope device_scope(c);
  int rc = check_seq(c, seq);
  if (rc) return rc;
  if (n_corner < 0 || n_corner > c->R * kLessSharpPerRing || n_surf < 0 || n_surf > c->max_points) { c->err = "last cloud too large"; return ALOAM_E_CAPACITY; }
  c->inject_max = std::max(c->inject_max, std::max(n_corner, n_surf));   // what the next mapping step may add (never lowers the bound)
  const int last = 1 - c->parity[seq];
  if (!c->d_less_sharp[last]) { c->err = "this context has no buffers for the last clouds (created for the registration stage only)"; return ALOAM_E_STATE; }
  const size_t b = seq;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (n_corner) HIP_TRY(c, hipMemcpy(c->d_less_sharp[last].get() + b * c->R * kLessSharpPerRing, corner_last, sizeof(float4) * n_corner, hipMemcpyHostToDevice));
  if (n_surf) HIP_TRY(c, hipMemcpy(c->d_less_flat[last].get() + b * c->cap, surf_last, sizeof(float4) * n_surf, hipMemcpyHostToDevice));
  return edit_seq(c, c->d_meta.get() + seq, [&](SeqMeta& m) { m.n_corner_last = n_corner; m.n_surf_last = n_surf; });
}

int aloam_set_state(aloam_ctx* c, int seq, const double para_q[4], const double para_t[3], const double q_w[4], const double t_w[3]) {
  DeviceScope device_scope(c);
  int rc = check_seq(c, seq);
  if (rc) return rc;
  return edit_seq(c, c->d_state.get() + seq, [&](OdomState& s) {
    for (int k = 0; k < 4; ++k) { s.para_q[k] = para_q[k]; s.q_w[k] = q_w[k]; }
    for (int k = 0; k < 3; ++k) { s.para_t[k] = para_t[k]; s.t_w[k] = t_w[k]; }
  });
}

int aloam_set_system_inited(aloam_ctx* c, int inited) {
  DeviceScope device_scope(c);
  if (!c) return ALOAM_E_ARG;
  std::fill(c->inited.begin(), c->inited.end(), inited != 0 ? 1 : 0);
  launch_set_inited(c->d_state.get(), c->B, inited != 0 ? 1 : 0, c->stream);
  HIP_TRY(c, hipGetLastError());
  return ALOAM_OK;
}

// ---- per-sequence lifecycle ----------------------------------------------------------------------------------------
int aloam_set_active(aloam_ctx* c, const int* active) {
  DeviceScope device_scope(c);
  if (!c) return ALOAM_E_ARG;
  std::vector<int> m(c->B, 1);
  if (active) for (int b = 0; b < c->B; ++b) m[b] = active[b] != 0 ? 1 : 0;
  if (c->reg_pending && (c->stages & ALOAM_STAGE_REGISTRATION) && m != c->reg_active) {
    c->err = "the mask may not change between a registration and the odometry step that consumes it";
    return ALOAM_E_STATE;
  }
  c->all_active = std::find(m.begin(), m.end(), 0) == m.end();
  c->active = std::move(m);
  return ALOAM_OK;
}

}  // extern "C"

// The reset of aloam_reset_sequences on checked ids, queued, with its host mirrors.
static int queue_reset(aloam_ctx* c, const int* seqs, int n) {
  if (n == 0) return ALOAM_OK;
  if (!c->d_reset_ids && dmalloc(c, c->d_reset_ids, c->B)) return ALOAM_E_HIP;
  if (const int rc = stage_ints(c, seqs, n, c->d_reset_ids.get())) return rc;
  ResetArgs r{};
  r.seqs = c->d_reset_ids.get(); r.n = n; r.R = c->R;
  r.meta = c->d_meta.get(); r.ringstart = c->d_ringstart.get(); r.state = c->d_state.get();
  r.edges = c->d_edges.get(); r.planes = c->d_planes.get();
  for (int k = 0; k < 2; ++k) r.grid_flags[k] = c->d_grid_flags[k].get();
  for (int k = 0; k < 2; ++k) { r.less_sharp[k] = c->d_less_sharp[k].get(); r.less_flat[k] = c->d_less_flat[k].get(); }
  r.cap = c->cap;
  if (c->map_on) { r.mapseq = c->d_mapseq.get(); r.cubes = c->d_cubes.get(); r.addcnt = c->d_addcnt.get(); r.live = c->d_map_live.get(); }
  launch_reset_sequences(r, c->stream);
  HIP_TRY(c, hipGetLastError());
  for (int i = 0; i < n; ++i) {
    c->parity[seqs[i]] = 0; c->inited[seqs[i]] = 0; c->needs_odom[seqs[i]] = 0;
    if ((int)c->map_err_seen.size() == c->B) c->map_err_seen[seqs[i]] = 0;
  }
  return ALOAM_OK;
}

extern "C" {

int aloam_reset_sequences(aloam_ctx* c, const int* seqs, int n) {
  DeviceScope device_scope(c);
  if (!c) return ALOAM_E_ARG;
  if (n < 0 || n > c->B || (n > 0 && !seqs)) { c->err = "bad sequence list"; return ALOAM_E_ARG; }
  std::vector<char> seen(c->B, 0);
  for (int i = 0; i < n; ++i) {
    if (seqs[i] < 0 || seqs[i] >= c->B || seen[seqs[i]]) { c->err = "sequence index out of range or repeated"; return ALOAM_E_ARG; }
    seen[seqs[i]] = 1;
  }
  return queue_reset(c, seqs, n);
}


// ---- intermediate arrays ---------------------------------------------------------------------------------------
int aloam_get_ring_ranges(aloam_ctx* c, int seq, int* start, int* count) {
  DeviceScope device_scope(c);
  int rc = check_seq(c, seq);
  if (rc) return rc;
  if ((rc = require_stage(c, ALOAM_STAGE_REGISTRATION))) return rc;
  if ((rc = sync_and_check(c))) return rc;
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
  if ((rc = fetch_meta(c, seq, &m))) return rc;
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
  if ((rc = fetch_meta(c, seq, &m))) return rc;
  const int k = m.n_cloud < cap ? m.n_cloud : cap;
  std::vector<int8_t> tmp(k > 0 ? k : 1);
  if (k > 0) HIP_TRY(c, hipMemcpy(tmp.data(), c->d_label.get() + (size_t)seq * c->cap, k, hipMemcpyDeviceToHost));
  for (int i = 0; i < k; ++i) out[i] = tmp[i];
  return m.n_cloud;
}

// Which association kernels own the sequence's last clouds (k_build_grids_fused): per cloud 0 = ring-sorted keys (pair kernel), 1 = nearly
// ring-sorted (pair kernel with the index-range walk window), 2 = not sorted (literal walks), -1 = keys / coordinates out of range (literal search).
int aloam_get_last_cloud_order(aloam_ctx* c, int seq, int out[2]) {
  DeviceScope device_scope(c);
  int rc = check_seq(c, seq);
  if (rc) return rc;
  if (!c->d_grid_flags[0]) { c->err = "this context has no odometry stage"; return ALOAM_E_STATE; }
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  for (int k = 0; k < 2; ++k) {
    int f[4];
    HIP_TRY(c, hipMemcpy(f, c->d_grid_flags[k].get() + (size_t)seq * 4, sizeof(f), hipMemcpyDeviceToHost));
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
  if ((rc = fetch_meta(c, seq, &m))) return rc;
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
      switch (kernel) {
        case K_FIND_ENDS: bytes += 2 * 256 * 16; break;
        case K_FRONT: bytes += 16 * Nin + 16 * N + 16.0 * (c->R + 1) * ((Nin + kBlockPts - 1) / kBlockPts); break;   // k_front: the sweep in, the slabs out, two granules per ring and block
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
    *algorithmic_bytes = bytes;
  }
  return ALOAM_OK;
}

// ---- stage 3: scan-to-map refinement --------------------------------------------------------------------------------
static MapArgs map_args(aloam_ctx* c) {
  MapArgs a{};
  a.B = c->B; a.cap = c->cap; a.R = c->R;
  a.meta = c->d_meta.get(); a.odom = c->d_state.get(); a.seq = c->d_mapseq.get();
  a.line_res = c->map_line_res; a.plane_res = c->map_plane_res;
  // after aloam_odometry_step's swap the sweep just processed is the "last" one: exactly what the odometry node publishes
  // as /laser_cloud_corner_last, /laser_cloud_surf_last and /velodyne_cloud_3 (reference src/laserOdometry.cpp:570-591)
  for (int k = 0; k < 2; ++k) { a.less_sharp[k] = c->d_less_sharp[k].get(); a.less_flat[k] = c->d_less_flat[k].get(); }
  a.full = c->d_cloud.get();
  if (!c->dense_valid) { a.slabs = c->d_slabs.get(); a.slab = c->slab; a.ringstart = c->d_ringstart.get(); }   // the sweep just registered lives in its ring slabs; the dense copy is made only for who asks
  a.registered = c->d_registered.get();
  a.cubes = c->d_cubes.get(); a.pool_cap = c->map.points; a.tab = c->d_maptab.get();
  for (int k = 0; k < 2; ++k) {
    a.pool[k] = c->map.pool[k].get(); a.stack[k] = c->d_stack[k].get(); a.stack_world[k] = c->d_stack_world[k].get(); a.stack_cube[k] = c->d_stack_cube[k].get();
    a.grid_sorted[k] = c->map.grid_sorted[k].get(); a.grid_start[k] = c->map.grid_start[k].get();
  }
  a.grid_H = c->map.H; a.live = c->d_map_live.get(); a.report_dev = c->d_map_report.get(); a.report_host = c->d_map_report_host;
  a.addcnt = c->d_addcnt.get(); a.cursor = c->d_cursor.get(); a.compact_flag = c->d_compact_flag.get();
  a.edges = c->d_medges.get(); a.norms = c->d_mnorms.get(); a.knn = c->d_knn.get();
  a.lm_max_iterations = c->cfg.lm_max_iterations;
  a.vox_counters = c->d_vox_counters.get();
  a.rec_tiles = c->d_rec_tiles.get(); a.rec_tiles_per_seq = c->rec_tiles_per_seq; a.rec_tiles_corner = c->rec_tiles_corner;
  return a;
}
static VoxArgs vox_args(aloam_ctx* c, int n_segs, int levels) {
  VoxArgs v{};
  v.segs = c->d_segs.get(); v.n_segs = n_segs; v.tile_seg = c->map.tile_seg.get(); v.tile_heads = c->map.tile_heads.get(); v.tile_pref = c->map.tile_pref.get();
  v.counters = c->d_vox_counters.get(); v.keys[0] = c->map.keys[0].get(); v.keys[1] = c->map.keys[1].get(); v.tmp = c->map.voxtmp.get(); v.bbox = c->d_bbox.get();
  v.tile_cap = c->map.tile_cap; v.key_cap = c->map.key_cap; v.levels = levels; v.lists = c->d_vox_lists.get();
  return v;
}

// Everything whose size follows the pool: the two class pools (contents kept when growing), the bucketed copy of the submap, the scratch of
// the general voxel path (keys, staging = 2 pools per sequence, tile lists) and the bucket tables.  A fresh MapPool is allocated and filled,
// then committed with one move (which releases the old buffers), so a failure at any point leaves the context as it was.
static int map_alloc_pool(aloam_ctx* c, int pool_points) {
  const size_t B = c->B, cap = c->cap, R = c->R, T = kVoxTile, pool = pool_points, old_pool = c->map.points;
  MapPool n;
  n.points = pool_points;
  n.H = 4096;
  while (n.H < (int)(pool / 16) && n.H < kMapGridMaxH) n.H <<= 1;          // ~ submap size
  n.key_cap = (long long)(B * std::max(cap + R * kLessSharpPerRing, 2 * pool));
  n.tile_bound = (int)(B * (2 * pool / T + 2 * kMapValidMax));
  n.tile_cap = std::max(c->map_stack_tile_bound, n.tile_bound);
  while (((size_t)kVoxTile << n.cube_levels) < pool) ++n.cube_levels;     // a 50 m cube may hold the whole pool (unneeded levels cost a skipped tile loop each)
  bool ok = true;
  auto grab = [&](auto& p, size_t count) { if (ok && dalloc(p, count) != hipSuccess) { ok = false; (void)hipGetLastError(); } };
  for (int k = 0; k < 2; ++k) {
    grab(n.pool[k], B * pool);
    grab(n.grid_sorted[k], B * pool);
    grab(n.grid_start[k], B * ((size_t)n.H + 1));
    grab(n.keys[k], (size_t)n.key_cap);
  }
  grab(n.voxtmp, (size_t)n.key_cap);
  grab(n.tile_seg, (size_t)n.tile_cap); grab(n.tile_heads, (size_t)n.tile_cap); grab(n.tile_pref, (size_t)n.tile_cap + 1);
  if (!ok || prepare_map_grid(n.H)) {
    c->err = "map pool of " + std::to_string(pool_points) + " points per sequence and class: allocation failed";
    return ALOAM_E_HIP;
  }
  for (int k = 0; k < 2; ++k) {
    if (old_pool) HIP_TRY(c, hipMemcpy2DAsync(n.pool[k].get(), sizeof(float4) * pool, c->map.pool[k].get(), sizeof(float4) * old_pool, sizeof(float4) * old_pool, B, hipMemcpyDeviceToDevice, c->stream));
    else HIP_TRY(c, hipMemsetAsync(n.pool[k].get(), 0, sizeof(float4) * B * pool, c->stream));
    HIP_TRY(c, hipMemsetAsync(n.grid_start[k].get(), 0, sizeof(int) * B * ((size_t)n.H + 1), c->stream));
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  c->map = std::move(n);
  return ALOAM_OK;
}

// The reference's cubes are std::vectors: a map grows as long as the sensor travels (src/laserMapping.cpp:737-783).  Here a (sequence,
// class) pool must hold the live points of its cubes plus what the step adds, and the steps are queued asynchronously, so the host sizes
// the pools AHEAD of the device from what k_map_report wrote after the last step that has finished: live points + (steps in flight + 1) x
// the most a step can add.  "The most": the stack sizes of the step are not known before its voxel filter has run, so it is the scan size
// (a stack is a filtered subset of one sweep) until a step has reported, then twice the largest stack any step has produced so far - a
// step that breaks that bound AND fills the pool drops points and raises ALOAM_E_CAPACITY like a full pool at the ceiling does.  When the
// bound exceeds the pool: wait for the device (the report is then exact), double the pool until it holds the bound, move the contents.
static int map_ensure_capacity(aloam_ctx* c) {
  if (c->map.points >= c->map_pool_limit) return ALOAM_OK;     // at the ceiling: nothing to decide (the device counts what does not fit)
  const int step_max = std::max(c->nin_max, c->inject_max);   // the last registration's active rows and what was injected since the last step
  const int hard[2] = {std::min(c->R * kLessSharpPerRing, step_max ? step_max : c->cap), std::min(c->cap, step_max ? step_max : c->cap)};
  auto bound = [&](long long lag) {
    const int done = c->h_map_report[0];
    long long worst = 0;
    for (int k = 0; k < 2; ++k) {
      const int inc = done > 0 ? std::min(hard[k], 2 * (int)c->h_map_report[3 + k] + 1024) : hard[k];
      worst = std::max(worst, (long long)c->h_map_report[1 + k] + (lag + 1) * inc);
    }
    return worst;
  };
  const long long lag = c->map_steps - c->h_map_report[0];
  if (bound(lag) <= c->map.points) return ALOAM_OK;
  HIP_TRY(c, hipStreamSynchronize(c->stream));               // now the report is that of the last queued step
  const long long need = bound(std::min<long long>(lag, 3));   // keep room for the run-ahead this caller has shown
  if (need <= c->map.points || c->map.points >= c->map_pool_limit) return ALOAM_OK;
  long long np = c->map.points;
  while (np < need) np *= 2;
  np = std::min<long long>(np, c->map_pool_limit);
  const int rc = map_alloc_pool(c, (int)np);
  if (rc) { c->map_pool_limit = c->map.points; return ALOAM_OK; }   // out of device memory: this pool is the ceiling from now on
  c->map_growths += 1;
  return ALOAM_OK;
}

int aloam_mapping_enable(aloam_ctx* c, float line_res, float plane_res, int pool_points) {
  DeviceScope device_scope(c);
  if (!c) return ALOAM_E_ARG;
  int rc = require_stage(c, ALOAM_STAGE_MAPPING);
  if (rc) return rc;
  if (c->map_on) { c->err = "mapping already enabled"; return ALOAM_E_STATE; }
  if (!(line_res > 0.f) || !(plane_res > 0.f) || pool_points < 4096 || pool_points > (1 << 26)) { c->err = "bad mapping parameters (4096 <= pool_points <= 2^26)"; return ALOAM_E_ARG; }
  const size_t B = c->B, cap = c->cap, R = c->R;
  c->map_line_res = line_res; c->map_plane_res = plane_res;
  c->map_levels = 0;                                       // incoming clouds: up to max_points
  while (((size_t)kVoxTile << c->map_levels) < cap) ++c->map_levels;
  const size_t T = kVoxTile;
  c->map_stack_tile_bound = (int)(B * ((cap + T - 1) / T + (R * kLessSharpPerRing + T - 1) / T));
  c->map_nsegs_max = (int)(B * 2 * kMapValidMax);
  const int pool0 = (pool_points + 1023) / 1024 * 1024;
  if (c->map_pool_limit < pool0) c->map_pool_limit = pool0;
  if ((rc = map_alloc_pool(c, pool0))) return rc;
  if ((rc = dmalloc(c, c->d_mapseq, B))) return rc;
  if ((rc = dmalloc(c, c->d_cubes, B * 2 * kMapCubes))) return rc;
  if ((rc = dmalloc(c, c->d_maptab, B * kTabInts))) return rc;
  if ((rc = dmalloc(c, c->d_addcnt, B * 2 * kMapCubes))) return rc;
  if ((rc = dmalloc(c, c->d_cursor, B * 2 * kMapCubes))) return rc;
  if ((rc = dmalloc(c, c->d_compact_flag, B * 2))) return rc;
  if ((rc = dmalloc(c, c->d_map_live, B * 2))) return rc;
  if ((rc = dmalloc(c, c->d_map_report, 4))) return rc;
  { int* p = nullptr; HIP_TRY(c, hipHostMalloc((void**)&p, sizeof(int) * 8, hipHostMallocMapped)); c->h_map_report.reset(p); }
  for (int k = 0; k < 8; ++k) c->h_map_report[k] = 0;
  HIP_TRY(c, hipHostGetDevicePointer((void**)&c->d_map_report_host, (void*)c->h_map_report.get(), 0));
  for (Event& e : c->map_step_done) HIP_TRY(c, hipEventCreateWithFlags(&e.h, hipEventDisableTiming));
  for (int k = 0; k < 2; ++k) {
    const size_t per = k == 0 ? R * kLessSharpPerRing : cap;
    if ((rc = dmalloc(c, c->d_stack[k], B * per))) return rc;
    if ((rc = dmalloc(c, c->d_stack_world[k], B * per))) return rc;
    if ((rc = dmalloc(c, c->d_stack_cube[k], B * per))) return rc;
  }
  c->rec_tiles_corner = (int)((R * kLessSharpPerRing + 255) / 256);
  c->rec_tiles_per_seq = c->rec_tiles_corner + (int)((cap + 255) / 256);
  if ((rc = dmalloc(c, c->d_rec_tiles, B * (size_t)c->rec_tiles_per_seq))) return rc;
  if ((rc = dmalloc(c, c->d_medges, B * R * kLessSharpPerRing))) return rc;
  if ((rc = dmalloc(c, c->d_mnorms, B * cap))) return rc;
  if ((rc = dmalloc(c, c->d_registered, B * cap))) return rc;
  if ((rc = dmalloc(c, c->d_knn, B * cap * 4))) return rc;
  if ((rc = dmalloc(c, c->d_segs, (size_t)c->map_nsegs_max))) return rc;
  if ((rc = dmalloc(c, c->d_vox_counters, 8))) return rc;
  if ((rc = dmalloc(c, c->d_vox_lists, 3 * (size_t)c->map_nsegs_max))) return rc;
  if (prepare_voxel_filter()) { c->err = "k_vox_lds: dynamic LDS size rejected"; return ALOAM_E_HIP; }
  if ((rc = dmalloc(c, c->d_bbox, (size_t)c->map_nsegs_max * 6))) return rc;
  std::vector<MapSeq> init(B);
  std::memset(init.data(), 0, sizeof(MapSeq) * B);
  for (size_t b = 0; b < B; ++b) {                       // reference src/laserMapping.cpp:72-74,109,115
    init[b].par[3] = 1.0; init[b].q_wmap_wodom[3] = 1.0;
    init[b].cen[0] = 10; init[b].cen[1] = 10; init[b].cen[2] = 5;
  }
  HIP_TRY(c, hipMemcpyAsync(c->d_mapseq.get(), init.data(), sizeof(MapSeq) * B, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  c->map_on = true;
  return ALOAM_OK;
}

int aloam_set_voxel_sum_order(aloam_ctx* c, int order) {
  DeviceScope device_scope(c);
  if (!c) return ALOAM_E_ARG;
  if (order != ALOAM_SUM_INPUT_ORDER && order != ALOAM_SUM_REFERENCE_ORDER) { c->err = "unknown summation order"; return ALOAM_E_ARG; }
  if (order == ALOAM_SUM_REFERENCE_ORDER && prepare_reference_order()) { c->err = "k_vox_reference_order: dynamic LDS size rejected"; return ALOAM_E_HIP; }
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  c->sum_order = order;
  return ALOAM_OK;
}

int aloam_mapping_set_pool_limit(aloam_ctx* c, int max_pool_points) {
  if (!c) return ALOAM_E_ARG;
  if (max_pool_points < 4096 || max_pool_points > (1 << 26)) { c->err = "bad pool limit (4096 .. 2^26 points)"; return ALOAM_E_ARG; }
  c->map_pool_limit = std::max((max_pool_points + 1023) / 1024 * 1024, c->map.points);
  return ALOAM_OK;
}

int aloam_get_map_pool_info(aloam_ctx* c, int out[4]) {
  DeviceScope device_scope(c);
  if (!c || !out) return ALOAM_E_ARG;
  if (!c->map_on) { c->err = "mapping not enabled"; return ALOAM_E_STATE; }
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  out[0] = c->map.points; out[1] = c->map_growths; out[2] = c->map_pool_limit;
  out[3] = std::max((int)c->h_map_report[1], (int)c->h_map_report[2]);
  return ALOAM_OK;
}

int aloam_mapping_step(aloam_ctx* c) {
  DeviceScope device_scope(c);
  if (!c) return ALOAM_E_ARG;
  if (!c->map_on) { c->err = "aloam_mapping_step before aloam_mapping_enable"; return ALOAM_E_STATE; }
  for (int b = 0; b < c->B; ++b)
    if (c->needs_odom[b] && (c->all_active || c->active[b])) {
      c->err = "sequence " + std::to_string(b) + " was loaded (aloam_load_sequences) and has not had its odometry step yet: it may not map";
      return ALOAM_E_STATE;
    }
  // at most four steps queued ahead of the device: the occupancy report the pools are sized from is never older than that
  hipEvent_t done = c->map_step_done[c->map_steps & 3];
  if (c->map_steps >= 4) HIP_TRY(c, hipEventSynchronize(done));
  int rc = map_ensure_capacity(c);
  if (rc) return rc;
  c->inject_max = 0;
  MapArgs a = map_args(c);
  if ((rc = stage_mask(c, c->d_mask_map, &a.active))) return rc;
  { ProfScope p(c, K_MAP_BEGIN); launch_map_begin(a, c->stream); }
  { ProfScope p(c, K_MAP_VOXEL_STACK);                                      // downSizeFilterCorner / Surf on the incoming clouds (:542-550)
    const VoxArgs v = vox_args(c, c->B * 2, c->map_levels);
    HIP_TRY(c, hipMemsetAsync(c->d_vox_counters.get() + 4, 0, 4 * sizeof(int), c->stream));   // general-path count, the two LDS-filter lists
    launch_map_stack_segments(a, v, c->stream);
    if (c->sum_order) launch_voxel_filter_reference_order(v, a, true, c->stream);
    else launch_voxel_filter(v, c->map_stack_tile_bound, c->stream); }
  { ProfScope p(c, K_MAP_GRID); launch_map_grid(a, c->stream); }            // kdtree*FromMap->setInputCloud (:558-559)
  for (int iter = 0; iter < 2; ++iter) {                                    // :562
    { ProfScope p(c, K_MAP_ASSOC); launch_map_associate(a, iter, c->stream); }
    { ProfScope p(c, K_MAP_SOLVE); launch_map_solve(a, iter, iter == 1, c->stream); }
  }
  { ProfScope p(c, K_MAP_INSERT); launch_map_insert(a, c->map.voxtmp.get(), c->stream); }        // :737-783
  { ProfScope p(c, K_MAP_VOXEL_CUBES);                                      // per-cube re-filter (:788-801)
    const VoxArgs v = vox_args(c, c->B * 2 * kMapValidMax, c->map.cube_levels);
    HIP_TRY(c, hipMemsetAsync(c->d_vox_counters.get() + 4, 0, 4 * sizeof(int), c->stream));
    launch_map_cube_segments(a, v, c->stream);
    if (c->sum_order) launch_voxel_filter_reference_order(v, a, false, c->stream);
    else launch_voxel_filter(v, c->map.tile_bound, c->stream); }
  { ProfScope p(c, K_MAP_REGISTER); launch_map_register(a, c->stream);      // :836-846
    c->map_steps += 1;
    launch_map_report(a, (int)c->map_steps, c->stream); }
  HIP_TRY(c, hipEventRecord(done, c->stream));
  HIP_TRY(c, hipGetLastError());
  return ALOAM_OK;
}

int aloam_set_full_cloud(aloam_ctx* c, int seq, const float* cloud, int n) {
  DeviceScope device_scope(c);
  int rc = check_seq(c, seq);
  if (rc) return rc;
  if (n < 0 || n > c->max_points) { c->err = "cloud too large"; return ALOAM_E_CAPACITY; }
  if ((rc = ensure_dense(c))) return rc;                // the other sequences' clouds of the last registration, before this one is replaced
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (n) HIP_TRY(c, hipMemcpy(c->d_cloud.get() + (size_t)seq * c->cap, cloud, sizeof(float4) * n, hipMemcpyHostToDevice));
  return edit_seq(c, c->d_meta.get() + seq, [&](SeqMeta& m) { m.n_cloud = n; });
}

// The mapping node's globals for one sequence (reference src/laserMapping.cpp:72-74,84-91,115-116): what a test or a restarted node
// injects to continue from a known map.
int aloam_set_map(aloam_ctx* c, int seq, int cls, const int* cube_ids, const int* counts, int n_cubes, const float* points_xyzw) {
  DeviceScope device_scope(c);
  int rc = check_seq(c, seq);
  if (rc) return rc;
  if (!c->map_on) { c->err = "mapping not enabled"; return ALOAM_E_STATE; }
  if (cls < 0 || cls > 1 || n_cubes < 0 || (n_cubes && (!cube_ids || !counts))) { c->err = "bad class / cube list"; return ALOAM_E_ARG; }
  long long total = 0;
  std::vector<CubeDesc> d(kMapCubes, CubeDesc{0, 0, 0, 0});
  for (int i = 0; i < n_cubes; ++i) {
    if (cube_ids[i] < 0 || cube_ids[i] >= kMapCubes || counts[i] < 0 || d[cube_ids[i]].cap) { c->err = "bad or repeated cube index"; return ALOAM_E_ARG; }
    d[cube_ids[i]] = CubeDesc{(int)total, counts[i], counts[i], 0};
    total += counts[i];
  }
  if (total && !points_xyzw) return ALOAM_E_ARG;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (total > c->map.points) {
    long long np = c->map.points;
    while (np < total) np *= 2;
    if (np > c->map_pool_limit) { c->err = "the injected map exceeds the pool limit"; return ALOAM_E_CAPACITY; }
    if ((rc = map_alloc_pool(c, (int)np))) return rc;
    c->map_growths += 1;
  }
  HIP_TRY(c, hipMemcpy(c->d_cubes.get() + ((size_t)seq * 2 + cls) * kMapCubes, d.data(), sizeof(CubeDesc) * kMapCubes, hipMemcpyHostToDevice));
  if (total) HIP_TRY(c, hipMemcpy(c->map.pool[cls].get() + (size_t)seq * c->map.points, points_xyzw, sizeof(float4) * (size_t)total, hipMemcpyHostToDevice));
  if ((rc = edit_seq(c, c->d_mapseq.get() + seq, [&](MapSeq& ms) { ms.pool_used[cls] = (int)total; }))) return rc;
  c->h_map_report[1 + cls] = std::max((int)c->h_map_report[1 + cls], (int)total);   // the pools are sized from this until the next step reports
  return ALOAM_OK;
}

int aloam_set_map_frame(aloam_ctx* c, int seq, const int cen[3], const double q_wmap_wodom[4], const double t_wmap_wodom[3], int frame_count) {
  DeviceScope device_scope(c);
  int rc = check_seq(c, seq);
  if (rc) return rc;
  if (!c->map_on) { c->err = "mapping not enabled"; return ALOAM_E_STATE; }
  if (!cen || !q_wmap_wodom || !t_wmap_wodom) return ALOAM_E_ARG;
  return edit_seq(c, c->d_mapseq.get() + seq, [&](MapSeq& ms) {
    for (int k = 0; k < 3; ++k) { ms.cen[k] = cen[k]; ms.t_wmap_wodom[k] = t_wmap_wodom[k]; }
    for (int k = 0; k < 4; ++k) ms.q_wmap_wodom[k] = q_wmap_wodom[k];
    ms.frame_count = frame_count;
  });
}

static int fetch_mapseq(aloam_ctx* c, int seq, MapSeq* ms) {
  int rc = check_seq(c, seq);
  if (rc) return rc;
  if (!c->map_on) { c->err = "mapping not enabled"; return ALOAM_E_STATE; }
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, hipMemcpy(ms, c->d_mapseq.get() + seq, sizeof(MapSeq), hipMemcpyDeviceToHost));
  return ALOAM_OK;
}

// ---- batched export -----------------------------------------------------------------------------------------------------
// The address a kernel writes `p` through: device memory of the context's device as it is, pinned host memory through its device mapping.
// Pageable host memory (with XNACK off a kernel store there faults the device), managed memory, another device's memory and NULL are refused.
static int export_target(aloam_ctx* c, const void* p, size_t align, const char* what, void** out) {
  hipPointerAttribute_t at{};
  const bool known = p && hipPointerGetAttributes(&at, p) == hipSuccess;
  if (!known) (void)hipGetLastError();                    // (pageable memory is an error of the query, not of the context)
  void* d = nullptr;
  if (known && !at.isManaged && at.type == hipMemoryTypeDevice && at.device == c->cfg.device) d = const_cast<void*>(p);
  else if (known && !at.isManaged && at.type == hipMemoryTypeHost && hipHostGetDevicePointer(&d, const_cast<void*>(p), 0) != hipSuccess) { (void)hipGetLastError(); d = nullptr; }
  if (!d) { c->err = std::string(what) + " must be device memory of the context's device or pinned host memory"; return ALOAM_E_ARG; }
  if ((uintptr_t)p % align || (uintptr_t)d % align) { c->err = std::string(what) + " must be " + std::to_string(align) + "-byte aligned"; return ALOAM_E_ARG; }
  *out = d;
  return ALOAM_OK;
}

// Where export id `id` (ALOAM_CLOUD_* or ALOAM_EXPORT_MAP + ALOAM_MAP_*) is read from: the buffers and counts of the matching getter, with the
// checks of find_cloud / aloam_get_map_cloud.  Queues nothing.
static int export_src(aloam_ctx* c, int id, ExportSrc* s) {
  *s = ExportSrc{};
  const int* meta = reinterpret_cast<const int*>(c->d_meta.get());
  const int* mseq = reinterpret_cast<const int*>(c->d_mapseq.get());
  const int meta_ints = sizeof(SeqMeta) / sizeof(int), map_ints = sizeof(MapSeq) / sizeof(int);
  const long long feat = (long long)c->R * kLessSharpPerRing, cap = c->cap;
  auto plain = [&](const float4* b0, const float4* b1, long long stride, const int* count, int count_stride, int sel) {
    s->base[0] = b0; s->base[1] = b1; s->stride = stride; s->count = count; s->count_stride = count_stride; s->sel = sel; s->kind = kExportPlain;
  };
#define META_FIELD(f) (meta + offsetof(SeqMeta, f) / sizeof(int)), meta_ints
  switch (id) {
    case ALOAM_CLOUD_FULL: plain(c->d_cloud.get(), nullptr, cap, META_FIELD(n_cloud), kSelFixed); break;
    case ALOAM_CLOUD_SHARP: plain(c->d_sharp.get(), nullptr, (long long)c->R * kSharpPerRing, META_FIELD(n_sharp), kSelFixed); break;
    case ALOAM_CLOUD_FLAT: plain(c->d_flat.get(), nullptr, (long long)c->R * kFlatPerRing, META_FIELD(n_flat), kSelFixed); break;
    case ALOAM_CLOUD_LESS_SHARP: plain(c->d_less_sharp[0].get(), c->d_less_sharp[1].get(), feat, META_FIELD(n_less_sharp), kSelCurrent); break;
    case ALOAM_CLOUD_LESS_FLAT: plain(c->d_less_flat[0].get(), c->d_less_flat[1].get(), cap, META_FIELD(n_less_flat), kSelCurrent); break;
    case ALOAM_CLOUD_CORNER_LAST: plain(c->d_less_sharp[0].get(), c->d_less_sharp[1].get(), feat, META_FIELD(n_corner_last), kSelLast); break;
    case ALOAM_CLOUD_SURF_LAST: plain(c->d_less_flat[0].get(), c->d_less_flat[1].get(), cap, META_FIELD(n_surf_last), kSelLast); break;
    case ALOAM_EXPORT_MAP + ALOAM_MAP_REGISTERED: case ALOAM_EXPORT_MAP + ALOAM_MAP_CORNER_STACK: case ALOAM_EXPORT_MAP + ALOAM_MAP_SURF_STACK:
    case ALOAM_EXPORT_MAP + ALOAM_MAP_SURROUND: case ALOAM_EXPORT_MAP + ALOAM_MAP_FULL:
      if (!c->map_on) { c->err = "mapping not enabled"; return ALOAM_E_STATE; }
      if (id == ALOAM_EXPORT_MAP + ALOAM_MAP_REGISTERED) plain(c->d_registered.get(), nullptr, cap, META_FIELD(n_cloud), kSelFixed);
      else if (id == ALOAM_EXPORT_MAP + ALOAM_MAP_CORNER_STACK) plain(c->d_stack[0].get(), nullptr, feat, mseq + offsetof(MapSeq, n_stack) / sizeof(int), map_ints, kSelFixed);
      else if (id == ALOAM_EXPORT_MAP + ALOAM_MAP_SURF_STACK) plain(c->d_stack[1].get(), nullptr, cap, mseq + offsetof(MapSeq, n_stack) / sizeof(int) + 1, map_ints, kSelFixed);
      else s->kind = id == ALOAM_EXPORT_MAP + ALOAM_MAP_SURROUND ? kExportSurround : kExportFull;
      return ALOAM_OK;
    default: c->err = "unknown cloud id " + std::to_string(id); return ALOAM_E_ARG;
  }
#undef META_FIELD
  // find_cloud's rule: the row a getter of any sequence would read must exist (aloam_create_stages leaves some buffers out)
  for (int b = 0; b < c->B; ++b) {
    const int row = s->sel == kSelFixed ? 0 : s->sel == kSelCurrent ? c->parity[b] : 1 - c->parity[b];
    if (!s->base[row]) { c->err = "this context holds no such cloud (see aloam_create_stages)"; return ALOAM_E_STATE; }
  }
  return ALOAM_OK;
}

// count -> scan -> gather of n_ids checked sources for sequences seq0 .. seq0 + nseq - 1 into device addresses (dst may be nullptr when cap is 0).
static int queue_export(aloam_ctx* c, const ExportSrc* src, int n_ids, bool full_cloud, int seq0, int nseq, float4* dst, long long cap, long long* dst_off) {
  for (int i = 0; i < n_ids; ++i) {
    const int k = src[i].kind - 1;
    if (k >= 0 && !c->d_exp_pref[k]) HIP_TRY(c, dalloc(c->d_exp_pref[k], (size_t)c->B * ((k == 0 ? kExportSurroundEntries : kExportFullEntries) + 1)));
  }
  if (full_cloud) if (const int rc = ensure_dense(c)) return rc;   // the full cloud is gathered from d_cloud, as aloam_get_cloud reads it
  ExportArgs a{};
  a.n_ids = n_ids; a.seq0 = seq0; a.nseq = nseq;
  for (int i = 0; i < n_ids; ++i) a.src[i] = src[i];
  a.meta = c->d_meta.get();
  if (c->map_on) {
    a.cubes = c->d_cubes.get(); a.tab = c->d_maptab.get(); a.mapseq = c->d_mapseq.get();
    a.pool[0] = c->map.pool[0].get(); a.pool[1] = c->map.pool[1].get(); a.pool_cap = c->map.points;
  }
  a.seg_cnt = c->d_exp_cnt.get(); a.chunk_off = c->d_exp_chunk.get(); a.seg_off = c->d_exp_off.get(); a.dst_off = dst_off;
  a.cube_pref[0] = c->d_exp_pref[0].get(); a.cube_pref[1] = c->d_exp_pref[1].get();
  a.dst = dst; a.cap_points = dst ? cap : 0;
  { ProfScope p(c, K_EXPORT); launch_export_clouds(a, c->gather_blocks, c->stream); }
  HIP_TRY(c, hipGetLastError());
  c->exp_last_segs = n_ids * nseq;
  return ALOAM_OK;
}

// aloam_get_map_cloud(SURROUND / FULL): the export of one sequence into the context's scratch, then one copy to the caller.
static int get_cube_list(aloam_ctx* c, int seq, int which, float* out, int cap_points) {
  ExportSrc src;
  int rc = export_src(c, ALOAM_EXPORT_MAP + which, &src);
  if (rc) return rc;
  if (!c->d_exp_tmp_off) HIP_TRY(c, dalloc(c->d_exp_tmp_off, 2));
  long long off[2] = {0, 0};
  for (int pass = 0; pass < 2; ++pass) {                  // a second pass only when the scratch was too small for the points asked for
    if ((rc = queue_export(c, &src, 1, false, seq, 1, c->d_exp_tmp.get(), c->exp_tmp_cap, c->d_exp_tmp_off.get()))) return rc;
    HIP_TRY(c, hipMemcpyAsync(off, c->d_exp_tmp_off.get(), sizeof(off), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (cap_points <= 0 || off[1] <= c->exp_tmp_cap) break;
    c->d_exp_tmp.reset(); c->exp_tmp_cap = 0;
    HIP_TRY(c, dalloc(c->d_exp_tmp, (size_t)off[1]));
    c->exp_tmp_cap = off[1];
  }
  const long long k = std::min<long long>(off[1], cap_points);
  if (k > 0) HIP_TRY(c, hipMemcpy(out, c->d_exp_tmp.get(), sizeof(float4) * k, hipMemcpyDeviceToHost));
  return (int)off[1];
}

int aloam_get_map_pose(aloam_ctx* c, int seq, double q_w_curr[4], double t_w_curr[3], double q_wmap_wodom[4], double t_wmap_wodom[3]) {
  DeviceScope device_scope(c);
  MapSeq ms;
  const int rc = fetch_mapseq(c, seq, &ms);
  if (rc) return rc;
  for (int k = 0; k < 4; ++k) { q_w_curr[k] = ms.par[k]; q_wmap_wodom[k] = ms.q_wmap_wodom[k]; }
  for (int k = 0; k < 3; ++k) { t_w_curr[k] = ms.par[4 + k]; t_wmap_wodom[k] = ms.t_wmap_wodom[k]; }
  return ALOAM_OK;
}

int aloam_get_map_info(aloam_ctx* c, int seq, int out[16]) {
  DeviceScope device_scope(c);
  MapSeq ms;
  const int rc = fetch_mapseq(c, seq, &ms);
  if (rc) return rc;
  const int v[16] = {ms.cen[0], ms.cen[1], ms.cen[2], ms.frame_count, ms.from_total[0], ms.from_total[1], ms.n_stack[0], ms.n_stack[1],
                     ms.factor_num[0][0], ms.factor_num[1][0], ms.factor_num[0][1], ms.factor_num[1][1], ms.lm_iterations[0], ms.lm_iterations[1],
                     ms.lm_termination[0], ms.compactions};
  std::memcpy(out, v, sizeof(v));
  return ALOAM_OK;
}

int aloam_map_cube_counts(aloam_ctx* c, int seq, int cls, int* out) {
  DeviceScope device_scope(c);
  MapSeq ms;
  const int rc = fetch_mapseq(c, seq, &ms);
  if (rc) return rc;
  if (cls < 0 || cls > 1) { c->err = "class must be 0 (corner) or 1 (surf)"; return ALOAM_E_ARG; }
  std::vector<CubeDesc> d(kMapCubes);
  HIP_TRY(c, hipMemcpy(d.data(), c->d_cubes.get() + ((size_t)seq * 2 + cls) * kMapCubes, sizeof(CubeDesc) * kMapCubes, hipMemcpyDeviceToHost));
  for (int i = 0; i < kMapCubes; ++i) out[i] = d[i].cnt;
  return kMapCubes;
}

int aloam_get_map_cube(aloam_ctx* c, int seq, int cls, int cube, float* out, int cap_points) {
  DeviceScope device_scope(c);
  MapSeq ms;
  const int rc = fetch_mapseq(c, seq, &ms);
  if (rc) return rc;
  if (cls < 0 || cls > 1 || cube < 0 || cube >= kMapCubes) { c->err = "bad class / cube index"; return ALOAM_E_ARG; }
  CubeDesc d;
  HIP_TRY(c, hipMemcpy(&d, c->d_cubes.get() + ((size_t)seq * 2 + cls) * kMapCubes + cube, sizeof(CubeDesc), hipMemcpyDeviceToHost));
  const int k = d.cnt < cap_points ? d.cnt : cap_points;
  if (k > 0) HIP_TRY(c, hipMemcpy(out, c->map.pool[cls].get() + (size_t)seq * c->map.points + d.off, sizeof(float4) * k, hipMemcpyDeviceToHost));
  return d.cnt;
}

int aloam_get_map_cloud(aloam_ctx* c, int seq, int which, float* out, int cap_points) {
  DeviceScope device_scope(c);
  MapSeq ms;
  const int rc = fetch_mapseq(c, seq, &ms);
  if (rc) return rc;
  if (which == ALOAM_MAP_SURROUND || which == ALOAM_MAP_FULL) return get_cube_list(c, seq, which, out, cap_points);
  const float4* p = nullptr;
  int n = 0;
  if (which == ALOAM_MAP_REGISTERED) {
    SeqMeta m;
    HIP_TRY(c, hipMemcpy(&m, c->d_meta.get() + seq, sizeof(SeqMeta), hipMemcpyDeviceToHost));
    p = c->d_registered.get() + (size_t)seq * c->cap; n = m.n_cloud;
  } else if (which == ALOAM_MAP_CORNER_STACK) { p = c->d_stack[0].get() + (size_t)seq * c->R * kLessSharpPerRing; n = ms.n_stack[0]; }
  else if (which == ALOAM_MAP_SURF_STACK) { p = c->d_stack[1].get() + (size_t)seq * c->cap; n = ms.n_stack[1]; }
  else { c->err = "unknown map cloud id"; return ALOAM_E_ARG; }
  const int k = n < cap_points ? n : cap_points;
  if (k > 0) HIP_TRY(c, hipMemcpy(out, p, sizeof(float4) * k, hipMemcpyDeviceToHost));
  return n;
}

// Poses of every sequence (/laser_odom_to_init src/laserOdometry.cpp:511-522 with para_q / para_t, /aft_mapped_to_init src/laserMapping.cpp:851-863
// with q_wmap_wodom / t_wmap_wodom), in stream order.
int aloam_export_poses(aloam_ctx* c, aloam_pose_record* dst) {
  DeviceScope device_scope(c);
  if (!c) return ALOAM_E_ARG;
  void* d = nullptr;
  if (const int rc = export_target(c, dst, alignof(aloam_pose_record), "dst", &d)) return rc;
  launch_export_poses(c->d_state.get(), c->map_on ? c->d_mapseq.get() : nullptr, c->B, static_cast<aloam_pose_record*>(d), c->stream);
  HIP_TRY(c, hipGetLastError());
  return ALOAM_OK;
}

// Clouds ids[0 .. n_ids) of every sequence packed back to back (the cloud topics of src/scanRegistration.cpp:413-441, src/laserOdometry.cpp:574-590,
// src/laserMapping.cpp:803-846), in stream order.  Every argument is checked before anything is queued.
int aloam_export_clouds(aloam_ctx* c, const int* ids, int n_ids, float* dst_xyzw, long long cap_points, long long* dst_offsets) {
  DeviceScope device_scope(c);
  if (!c) return ALOAM_E_ARG;
  if (n_ids < 0 || n_ids > ALOAM_EXPORT_MAX_IDS || (n_ids > 0 && !ids)) { c->err = "n_ids must be 0 .. ALOAM_EXPORT_MAX_IDS"; return ALOAM_E_ARG; }
  if (cap_points < 0) { c->err = "negative cap_points"; return ALOAM_E_ARG; }
  ExportSrc src[ALOAM_EXPORT_MAX_IDS];
  bool full_cloud = false;
  for (int i = 0; i < n_ids; ++i) {
    for (int j = 0; j < i; ++j) if (ids[j] == ids[i]) { c->err = "repeated cloud id " + std::to_string(ids[i]); return ALOAM_E_ARG; }
    if (const int rc = export_src(c, ids[i], &src[i])) return rc;
    full_cloud |= ids[i] == ALOAM_CLOUD_FULL;
  }
  void *d_off = nullptr, *d_pts = nullptr;
  if (const int rc = export_target(c, dst_offsets, alignof(long long), "dst_offsets", &d_off)) return rc;
  if ((dst_xyzw || cap_points > 0) && export_target(c, dst_xyzw, 16, "dst_xyzw", &d_pts)) return ALOAM_E_ARG;
  return queue_export(c, src, n_ids, full_cloud, 0, c->B, static_cast<float4*>(d_pts), cap_points, static_cast<long long*>(d_off));
}

// ---- sequence records ------------------------------------------------------------------------------------------------------
}  // extern "C"

// The header fields a record carries from its context (the counts are the device's): what a load compares.
static aloam_seq_record_header record_template(const aloam_ctx* c) {
  aloam_seq_record_header h{};
  h.magic = ALOAM_SEQ_RECORD_MAGIC; h.version = ALOAM_SEQ_RECORD_VERSION;
  h.parts = ((c->stages & ALOAM_STAGE_ODOMETRY) ? ALOAM_SEQ_PART_ODOMETRY : 0) | (c->map_on ? ALOAM_SEQ_PART_MAP : 0);
  h.n_scans = c->cfg.n_scans; h.ring_from_field = c->cfg.ring_from_field != 0;
  std::memcpy(&h.min_range_bits, &c->cfg.min_range, 4);
  h.distortion = c->cfg.distortion != 0; h.lm_max_iterations = c->cfg.lm_max_iterations; h.outer_iterations = c->cfg.outer_iterations;
  h.sum_order = c->sum_order;
  if (c->map_on) { std::memcpy(&h.line_res_bits, &c->map_line_res, 4); std::memcpy(&h.plane_res_bits, &c->map_plane_res, 4); }
  h.seq_meta_bytes = sizeof(SeqMeta); h.odom_bytes = sizeof(OdomState); h.map_seq_bytes = sizeof(MapSeq);
  return h;
}

// n distinct ids in 0 .. B-1 (slots of a load, sequences of a save).
static int check_ids(aloam_ctx* c, const int* ids, int n) {
  if (n < 0 || n > c->B || (n > 0 && !ids)) { c->err = "bad sequence list"; return ALOAM_E_ARG; }
  std::vector<char> seen(c->B, 0);
  for (int i = 0; i < n; ++i) {
    if (ids[i] < 0 || ids[i] >= c->B || seen[ids[i]]) { c->err = "sequence index out of range or repeated"; return ALOAM_E_ARG; }
    seen[ids[i]] = 1;
  }
  return ALOAM_OK;
}

// Scratch of both calls, sized for `batch` records, allocated once (then only ever used in stream order).
static int ck_scratch(aloam_ctx* c) {
  const size_t B = c->B;
  if (!c->d_ck_seqs) {
    HIP_TRY(c, dalloc(c->d_ck_seqs, B)); HIP_TRY(c, dalloc(c->d_ck_info, B * kRecInfo)); HIP_TRY(c, dalloc(c->d_ck_units, B));
    HIP_TRY(c, dalloc(c->d_ck_chunk, B + 1)); HIP_TRY(c, dalloc(c->d_ck_uoff, B + 1));
  }
  if (c->map_on && !c->d_ck_pref) HIP_TRY(c, dalloc(c->d_ck_pref, B * 2 * (kMapCubes + 1)));
  return ALOAM_OK;
}

// Load staging, pinned and in device memory: [B + 1] offsets, [B + 1] chunk offsets, [B][kRecInfo] counts.  The pinned copy first holds the
// offsets and, behind them, the headers of records in device memory.
static size_t ck_stage_layout(size_t B, size_t* chunk_at, size_t* info_at) {
  *chunk_at = 8 * (B + 1);
  *info_at = (*chunk_at + 4 * (B + 1) + 15) & ~(size_t)15;
  return std::max(*info_at + 4 * kRecInfo * B, *chunk_at + sizeof(aloam_seq_record_header) * B);
}
static int ck_load_scratch(aloam_ctx* c) {
  if (c->h_ck) return ALOAM_OK;
  size_t ca, ia;
  const size_t bytes = ck_stage_layout(c->B, &ca, &ia);
  char* p = nullptr;
  HIP_TRY(c, hipHostMalloc((void**)&p, bytes, hipHostMallocMapped));
  c->h_ck.reset(p);
  HIP_TRY(c, hipHostGetDevicePointer((void**)&c->d_ck_host, p, 0));
  HIP_TRY(c, dalloc(c->d_ck_load, bytes));
  return ALOAM_OK;
}

// Where a load reads `p` from: device memory of the context's device or pinned host memory (*dev = the address the kernels use), or
// pageable host memory (*dev = nullptr: read by the host, staged).  Another device's memory, managed memory and NULL are refused.
static int load_source(aloam_ctx* c, const void* p, const char* what, const void** dev, bool* on_host) {
  hipPointerAttribute_t at{};
  *dev = nullptr; *on_host = true;
  if (!p) { c->err = std::string(what) + " is NULL"; return ALOAM_E_ARG; }
  if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return ALOAM_OK; }   // pageable host memory
  if (at.isManaged) { c->err = std::string(what) + " must be device memory of the context's device, pinned or pageable host memory"; return ALOAM_E_ARG; }
  if (at.type == hipMemoryTypeDevice) {
    if (at.device != c->cfg.device) { c->err = std::string(what) + " is memory of another device"; return ALOAM_E_ARG; }
    *dev = p; *on_host = false;
    return ALOAM_OK;
  }
  void* d = nullptr;
  if (at.type == hipMemoryTypeHost && hipHostGetDevicePointer(&d, const_cast<void*>(p), 0) == hipSuccess) *dev = d;
  else (void)hipGetLastError();
  return ALOAM_OK;                                       // pinned host memory: readable by the host and (through *dev) by the kernels
}

// Checks one header against this context; names the first field that differs.
static int check_header(aloam_ctx* c, int i, const aloam_seq_record_header& h, long long len, const aloam_seq_record_header& want) {
  auto fail = [&](int rc, const std::string& what) { c->err = "record " + std::to_string(i) + ": " + what; return rc; };
  if (h.magic != ALOAM_SEQ_RECORD_MAGIC) return fail(ALOAM_E_ARG, "bad magic (not a sequence record)");
  if (h.version != ALOAM_SEQ_RECORD_VERSION) return fail(ALOAM_E_ARG, "record version " + std::to_string(h.version) + ", this library reads version " + std::to_string(ALOAM_SEQ_RECORD_VERSION));
  if (h.bytes != len) return fail(ALOAM_E_ARG, "record length " + std::to_string(h.bytes) + " differs from the offsets' " + std::to_string(len));
  if (h.seq_meta_bytes != want.seq_meta_bytes || h.odom_bytes != want.odom_bytes || h.map_seq_bytes != want.map_seq_bytes) return fail(ALOAM_E_ARG, "section sizes differ");
  struct { const char* name; long long got, ctx; } fields[] = {
      {"n_scans", h.n_scans, want.n_scans}, {"ring_from_field", h.ring_from_field, want.ring_from_field},
      {"min_range", h.min_range_bits, want.min_range_bits}, {"distortion", h.distortion, want.distortion},
      {"lm_max_iterations", h.lm_max_iterations, want.lm_max_iterations}, {"outer_iterations", h.outer_iterations, want.outer_iterations},
      {"voxel sum order", h.sum_order, want.sum_order},
      {"odometry part (ALOAM_STAGE_ODOMETRY)", h.parts & ALOAM_SEQ_PART_ODOMETRY, want.parts & ALOAM_SEQ_PART_ODOMETRY},
      {"map part (mapping enabled)", h.parts & ALOAM_SEQ_PART_MAP, want.parts & ALOAM_SEQ_PART_MAP},
      {"mapping_line_resolution", h.line_res_bits, want.line_res_bits}, {"mapping_plane_resolution", h.plane_res_bits, want.plane_res_bits}};
  for (const auto& f : fields)
    if (f.got != f.ctx) return fail(ALOAM_E_ARG, std::string(f.name) + " differs from this context's (record " + std::to_string(f.got) + ", context " + std::to_string(f.ctx) + ")");
  if (h.parts & ~(ALOAM_SEQ_PART_ODOMETRY | ALOAM_SEQ_PART_MAP)) return fail(ALOAM_E_ARG, "unknown parts");
  const bool odo = h.parts & ALOAM_SEQ_PART_ODOMETRY, map = h.parts & ALOAM_SEQ_PART_MAP;
  if (h.n_corner_last < 0 || h.n_surf_last < 0 || (!odo && (h.n_corner_last || h.n_surf_last))) return fail(ALOAM_E_ARG, "bad last-cloud sizes");
  for (int k = 0; k < 2; ++k)
    if (h.n_cubes[k] < 0 || h.n_cubes[k] > kMapCubes || h.map_points[k] < 0 || (!map && (h.n_cubes[k] || h.map_points[k]))) return fail(ALOAM_E_ARG, "bad cube counts");
  if (rec_layout(map, h.n_corner_last, h.n_surf_last, h.n_cubes, h.map_points).bytes != h.bytes) return fail(ALOAM_E_ARG, "record length disagrees with its counts");
  if (h.n_corner_last > c->R * kLessSharpPerRing || h.n_surf_last > c->max_points)
    return fail(ALOAM_E_CAPACITY, "its last clouds (" + std::to_string(h.n_corner_last) + " / " + std::to_string(h.n_surf_last) + " points) exceed this context's max_points");
  for (int k = 0; k < 2; ++k)
    if (h.map_points[k] > c->map_pool_limit) return fail(ALOAM_E_CAPACITY, "its map (" + std::to_string(h.map_points[k]) + " points of one class) exceeds the pool limit");
  return ALOAM_OK;
}

extern "C" {

int aloam_save_sequences(aloam_ctx* c, const int* seqs, int n, void* dst, long long cap_bytes, long long* dst_offsets) {
  DeviceScope device_scope(c);
  if (!c) return ALOAM_E_ARG;
  if (const int rc = check_ids(c, seqs, n)) return rc;
  if (cap_bytes < 0) { c->err = "negative cap_bytes"; return ALOAM_E_ARG; }
  if (c->reg_pending) { c->err = "a registration waits for its odometry step: records are saved between frames"; return ALOAM_E_STATE; }
  void *d_off = nullptr, *d_dst = nullptr;
  if (const int rc = export_target(c, dst_offsets, alignof(long long), "dst_offsets", &d_off)) return rc;
  if ((dst || cap_bytes > 0) && export_target(c, dst, 16, "dst", &d_dst)) return ALOAM_E_ARG;
  if (const int rc = ck_scratch(c)) return rc;
  if (n > 0) if (const int rc = stage_ints(c, seqs, n, c->d_ck_seqs.get())) return rc;
  CkptSaveArgs a{};
  a.seqs = c->d_ck_seqs.get(); a.n = n; a.R = c->R; a.cap = c->cap;
  a.meta = c->d_meta.get(); a.state = c->d_state.get();
  if (c->stages & ALOAM_STAGE_ODOMETRY)
    for (int k = 0; k < 2; ++k) { a.less_sharp[k] = c->d_less_sharp[k].get(); a.less_flat[k] = c->d_less_flat[k].get(); }
  if (c->map_on) {
    a.mapseq = c->d_mapseq.get(); a.cubes = c->d_cubes.get(); a.tab = c->d_maptab.get(); a.live = c->d_map_live.get();
    a.pool[0] = c->map.pool[0].get(); a.pool[1] = c->map.pool[1].get(); a.pool_cap = c->map.points;
  }
  a.hdr = record_template(c);
  a.info = c->d_ck_info.get(); a.units = c->d_ck_units.get(); a.chunk_off = c->d_ck_chunk.get(); a.unit_off = c->d_ck_uoff.get();
  a.cube_pref = c->d_ck_pref.get();
  a.dst_off = static_cast<long long*>(d_off); a.dst = static_cast<char*>(d_dst); a.cap_bytes = d_dst ? cap_bytes : 0;
  { ProfScope p(c, K_SAVE); launch_save_sequences(a, c->gather_blocks, c->stream); }
  HIP_TRY(c, hipGetLastError());
  c->ck_save_n = n;
  return ALOAM_OK;
}

int aloam_load_sequences(aloam_ctx* c, const int* slots, int n, const void* src, const long long* src_offsets) {
  DeviceScope device_scope(c);
  if (!c) return ALOAM_E_ARG;
  if (const int rc = check_ids(c, slots, n)) return rc;
  if (c->reg_pending) { c->err = "a registration waits for its odometry step: records are loaded between frames"; return ALOAM_E_STATE; }
  const void *d_src = nullptr, *d_offs = nullptr;   // (the offsets are read by the host, then staged with the counts)
  bool src_host = false, offs_host = false;
  if (const int rc = load_source(c, src_offsets, "src_offsets", &d_offs, &offs_host)) return rc;
  if (n == 0) return ALOAM_OK;
  if (const int rc = load_source(c, src, "src", &d_src, &src_host)) return rc;
  if ((uintptr_t)src % 16) { c->err = "src must be 16-byte aligned"; return ALOAM_E_ARG; }
  if (const int rc = ck_load_scratch(c)) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));          // the one host wait: the pools are sized from the headers
  std::vector<long long> off(n + 1);
  if (offs_host) std::memcpy(off.data(), src_offsets, sizeof(long long) * (n + 1));
  else HIP_TRY(c, hipMemcpy(off.data(), src_offsets, sizeof(long long) * (n + 1), hipMemcpyDeviceToHost));
  for (int i = 0; i < n; ++i)
    if (off[i] < 0 || off[i] % 16 || off[i + 1] - off[i] < (long long)sizeof(aloam_seq_record_header) || (off[i + 1] - off[i]) % kRecAlign) {
      c->err = "record " + std::to_string(i) + ": offsets must rise by whole records (multiples of " + std::to_string(kRecAlign) + " bytes)";
      return ALOAM_E_ARG;
    }
  std::vector<aloam_seq_record_header> hdr(n);
  if (src_host) {
    for (int i = 0; i < n; ++i) std::memcpy(&hdr[i], static_cast<const char*>(src) + off[i], sizeof(aloam_seq_record_header));
  } else {                                                // records in device memory: one small gather of the headers into pinned memory
    long long* h_off = reinterpret_cast<long long*>(c->h_ck.get());
    for (int i = 0; i < n; ++i) h_off[i] = off[i];
    launch_read_headers(static_cast<const char*>(d_src), reinterpret_cast<const long long*>(c->d_ck_host), n, reinterpret_cast<aloam_seq_record_header*>(c->d_ck_host + 8 * (c->B + 1)), c->stream);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    std::memcpy(hdr.data(), c->h_ck.get() + 8 * (c->B + 1), sizeof(aloam_seq_record_header) * n);
  }
  const aloam_seq_record_header want = record_template(c);
  long long need = 0;
  for (int i = 0; i < n; ++i) {
    if (const int rc = check_header(c, i, hdr[i], off[i + 1] - off[i], want)) return rc;
    need = std::max<long long>(need, std::max(hdr[i].map_points[0], hdr[i].map_points[1]));
  }
  // Everything is checked: from here on the load changes the context.
  if (c->map_on && need > c->map.points) {
    long long np = c->map.points;
    while (np < need) np *= 2;
    np = std::min<long long>(np, c->map_pool_limit);
    if (const int rc = map_alloc_pool(c, (int)np)) return rc;
    c->map_growths += 1;
  }
  const char* base = static_cast<const char*>(d_src);
  if (!base) {                                            // pageable host memory: staged into device memory (the span of the n records)
    const size_t span = (size_t)(off[n] - off[0]);
    if (c->ck_stage_bytes < span) {
      c->d_ck_stage.reset(); c->ck_stage_bytes = 0;
      HIP_TRY(c, dalloc(c->d_ck_stage, span));
      c->ck_stage_bytes = span;
    }
    HIP_TRY(c, hipMemcpyAsync(c->d_ck_stage.get(), static_cast<const char*>(src) + off[0], span, hipMemcpyHostToDevice, c->stream));
    base = c->d_ck_stage.get() - off[0];
  }
  size_t chunk_at, info_at;
  ck_stage_layout(c->B, &chunk_at, &info_at);
  char* h = c->h_ck.get();
  long long* s_off = reinterpret_cast<long long*>(h);
  int* s_chunk = reinterpret_cast<int*>(h + chunk_at);
  int* s_info = reinterpret_cast<int*>(h + info_at);
  int chunks = 0;
  for (int i = 0; i < n; ++i) {
    const aloam_seq_record_header& r = hdr[i];
    s_off[i] = off[i];
    s_chunk[i] = chunks;
    chunks += (int)((r.bytes / 16 + kExportChunk - 1) / kExportChunk);
    const int info[kRecInfo] = {r.n_corner_last, r.n_surf_last, r.n_cubes[0], r.n_cubes[1], r.map_points[0], r.map_points[1], slots[i], 0};
    std::memcpy(s_info + (size_t)i * kRecInfo, info, sizeof(info));
  }
  s_off[n] = off[n]; s_chunk[n] = chunks;
  HIP_TRY(c, hipMemcpyAsync(c->d_ck_load.get(), h, info_at + sizeof(int) * kRecInfo * n, hipMemcpyHostToDevice, c->stream));
  if (const int rc = queue_reset(c, slots, n)) return rc;
  CkptLoadArgs a{};
  a.src = base; a.off = reinterpret_cast<const long long*>(c->d_ck_load.get());
  a.chunk_off = reinterpret_cast<const int*>(c->d_ck_load.get() + chunk_at); a.info = reinterpret_cast<const int*>(c->d_ck_load.get() + info_at);
  a.n = n; a.R = c->R; a.cap = c->cap;
  a.meta = c->d_meta.get(); a.state = c->d_state.get();
  if (c->stages & ALOAM_STAGE_ODOMETRY) { a.corner_last = c->d_less_sharp[1].get(); a.surf_last = c->d_less_flat[1].get(); }
  if (c->map_on) {
    a.mapseq = c->d_mapseq.get(); a.cubes = c->d_cubes.get(); a.tab = c->d_maptab.get(); a.live = c->d_map_live.get();
    a.pool[0] = c->map.pool[0].get(); a.pool[1] = c->map.pool[1].get(); a.pool_cap = c->map.points;
  }
  { ProfScope p(c, K_LOAD); launch_load_sequences(a, c->gather_blocks, c->stream); }
  HIP_TRY(c, hipGetLastError());
  // host mirrors: parity 0 (the reset), systemInited from the header, capacity events already seen, no mapping before the next odometry step
  if ((int)c->map_err_seen.size() != c->B) c->map_err_seen.assign(c->B, 0);
  c->ck_load_bytes = off[n] - off[0];
  for (int i = 0; i < n; ++i) {
    const int s = slots[i];
    c->inited[s] = hdr[i].inited != 0;
    c->map_err_seen[s] = hdr[i].err_events;
    c->needs_odom[s] = (c->stages & ALOAM_STAGE_ODOMETRY) ? 1 : 0;
    if (c->map_on) for (int k = 0; k < 2; ++k) c->h_map_report[1 + k] = std::max((int)c->h_map_report[1 + k], hdr[i].map_points[k]);
  }
  return ALOAM_OK;
}

}  // extern "C"
