// a-loam_amd/csrc/capi_internal.hpp — what the host files of libaloam_mi355x.so share: the context and the owners of its buffers, the
// error and scope guards, and the helpers that more than one of them calls.  The host side is split by stage like the kernels:
// aloam_capi.hip (context, staging of input counts, lifecycle, profiling), capi_odometry.hip (registration, odometry, the sequence getters and
// setters), capi_mapping.hip (scan-to-map refinement and its pools), capi_records.hip (batched export, sequence records), capi_information.hip (pose information), capi_posegraph.hip (pose graphs), capi_graphmap.hip (keyframe clouds, the map at the graph's poses), capi_graphapply.hip (a solved graph carried into the live state), capi_loopreg.hip (loop edges: batched keyframe registration), capi_graphmarginal.hip (pose-graph marginals), capi_graphpropose.hip (loop candidates by pose proximity), capi_graphtrim.hip (pose graphs trimmed in place), capi_graphjoint.hip (joined pose graphs: links between sequences and a joint solve), capi_graphrecords.hip (graph records: save / load of pose graphs with their keyframe clouds), capi_relocalize.hip (map-pose hypotheses), capi_atlas.hip (map spill and atlas),
// capi_places.hip (place recognition), capi_range.hip (range-image input), capi_seq.hip (what the host knows about each sequence, SeqHost: the events that change it, the stage masks).
// Stated once here for all of them: the pinned staging ring (StageRing), a scratch buffer with its capacity (Scratch), and one struct per
// graph-family feature (GraphStore ... MarginalScratch) that its enable builds fresh and commits with one move, as MapPool.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdio>
#include <memory>
#include <functional>
#include <string>
#include <utility>
#include <vector>

#include "../../include/aloam_mi355x.h"
#include "aloam_device.hpp"
#include "atlas_kernels.hpp"
#include "checkpoint_kernels.hpp"
#include "export_kernels.hpp"
#include "graphapply_kernels.hpp"
#include "graphjoint_kernels.hpp"
#include "graphlink_kernels.hpp"
#include "graphmap_kernels.hpp"
#include "graphmapjoint_kernels.hpp"
#include "graphmarginal_kernels.hpp"
#include "graphpropose_kernels.hpp"
#include "graphrecord_kernels.hpp"
#include "graphtrim_kernels.hpp"
#include "loopreg_kernels.hpp"
#include "loopsearch_kernels.hpp"
#include "mapping_kernels.hpp"
#include "odometry_kernels.hpp"
#include "places_kernels.hpp"
#include "posegraph_kernels.hpp"
#include "registration_kernels.hpp"
#include "relocalize_kernels.hpp"

using namespace aloam;

struct aloam_ctx;
namespace aloam {
enum KernelId { K_FIND_ENDS = 0, K_FRONT, K_RING_STARTS, K_DENSE_CLOUD, K_RING_FEATURES, K_BUILD_GRIDS, K_TRANSFORM, K_ASSOC_CORNER,
                K_ASSOC_PLANE, K_SOLVE, K_ADVANCE, K_MAP_BEGIN, K_MAP_VOXEL_STACK, K_MAP_GRID, K_MAP_ASSOC, K_MAP_SOLVE, K_MAP_INSERT,
                K_MAP_VOXEL_CUBES, K_MAP_REGISTER, K_GRAPH_MARGINALS, K_EXPORT, K_POSE_INFO, K_POSE_GRAPH, K_GRAPH_MAP, K_LOOP_REGISTER, K_SAVE, K_LOAD, K_SCORE, K_APPLY, K_COUNT };
const char* const kKernelNames[] = {"k_find_ends", "k_front", "k_ring_starts", "k_dense_cloud", "k_ring_features",
                                    "k_build_grids", "k_transform_queries", "k_associate[corner]", "k_associate[plane]",
                                    "k_solve", "k_advance", "map_begin", "map_voxel[stacks]", "map_grid", "map_associate", "map_solve",
                                    "map_insert", "map_voxel[cubes]", "map_register", "graph_marginals", "export_clouds", "pose_information", "pose_graph", "graph_map", "loop_register", "save_sequences",
                                    "load_sequences", "score_corrections", "apply_corrections"};
static_assert(sizeof(kKernelNames) / sizeof(kKernelNames[0]) == K_COUNT, "one name per KernelId, in the same order");
struct ProfRec { int kernel; hipEvent_t e0, e1; };
constexpr int kNinSlots = 8;
constexpr int kGraphStageSlots = 4;

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
  Handle(Handle&& o) noexcept : h(std::exchange(o.h, nullptr)) {}   // (no copies)
  Handle& operator=(Handle&& o) noexcept { if (this != &o) { reset(); h = std::exchange(o.h, nullptr); } return *this; }
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

// A pinned ring of Slots slots: the caller fills the slot that acquire() hands out and queues it (or pieces of it) with queue(); the call
// returns at once and the H2D copy runs in stream order.  A slot comes round again Slots acquires later, and acquire() then waits for
// the copy that last read it, and for nothing else.  The events stand before the memory: they are destroyed after it.
template <int Slots>
struct StageRing {
  Event done[Slots];                 // the copy that last read a slot has run
  PinnedBuf<char> mem;
  size_t slot_bytes = 0;
  int cursor = 0;
  bool used[Slots] = {};
  // Once per ring (a second call changes nothing).  nullptr, or what failed: then nothing stays allocated.
  const char* create(size_t bytes) {
    if (mem) return nullptr;
    char* p = nullptr;
    if (hipHostMalloc((void**)&p, bytes * Slots, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return "pinned request ring: allocation failed"; }
    mem.reset(p); slot_bytes = bytes;
    for (Event& e : done)
      if (hipEventCreateWithFlags(&e.h, hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); *this = StageRing(); return "event creation failed"; }
    return nullptr;
  }
  template <typename T> int acquire(aloam_ctx* c, T** slot, int* index);
  // `bytes` at `src`, which lies in slot `index`, to `dst` on `stream`; the slot counts as read when this copy has run.
  int queue(aloam_ctx* c, int index, const void* src, size_t bytes, void* dst, hipStream_t stream);
};

// A scratch buffer and the elements it holds.  grow(): to `need` elements when it holds fewer; the old buffer is released first (its
// contents are not needed), and a failed allocation leaves it empty.
template <typename T>
struct Scratch {
  DevBuf<T> p;
  long long cap = 0;
  T* get() const { return p.get(); }
  void release() { cap = 0; p.reset(); }
  int grow(aloam_ctx* c, long long need);
};

// Everything whose size follows the map pool (map_alloc_pool): built fresh and committed with one move when the pool grows.
struct MapPool {
  int points = 0, H = 0;             // pool points per sequence and class, buckets of the submap grid
  int cube_levels = 0, tile_cap = 0, tile_bound = 0;   // general voxel path: merge levels of a cube, tile list capacity, tiles of the per-cube pass
  long long key_cap = 0;
  DevBuf<float4> pool[2], grid_sorted[2], voxtmp;
  DevBuf<int> grid_start[2], tile_seg, tile_heads, tile_pref;
  DevBuf<unsigned long long> keys[2];
};

// The graph family, one struct per feature: its buffers, its ring, its sizes and whether it is on.  An enable builds one fresh and moves it
// into the context when everything succeeded, so a refusal leaves nothing allocated and the context as it was.
struct GraphStore {                  // pose graphs (aloam_graph_enable): one row of nodes and one of edges per sequence; the counts are SeqHost fields
  bool on = false;
  int max_nodes = 0, max_edges = 0;
  DevBuf<aloam_graph_node> nodes;                                   // [B][max_nodes]
  DevBuf<aloam_graph_edge> edges;                                   // [B][max_edges]
  DevBuf<GraphAddItem> add;                                         // [B] the nodes of one aloam_graph_add_nodes
  DevBuf<GraphSolveItem> items;                                     // [B] the listed sequences of one aloam_graph_optimize
  StageRing<kGraphStageSlots> ring;                                 // a slot holds the B items of one add / optimize
  Scratch<double> f64; Scratch<int> i32;                            // the solve's scratch rows, grown on first use
  long long last_nodes = 0, last_edges = 0;                         // the last solve (algorithmic bytes)
  long long last_trim_bytes = -1;                                   // >= 0: the last call timed under pose_graph was aloam_graph_trim, and moved this much
};
struct KeyframeStore {               // keyframe clouds (aloam_graph_keyframes_enable): per sequence and class a row of sensor-frame points, per node a descriptor
  bool on = false;
  int cap[2] = {0, 0};                                              // points per sequence: corner, surf
  DevBuf<float4> points[2];                                         // [B][cap[cls]]
  DevBuf<KfDesc> desc;                                              // [B][GraphStore::max_nodes]
  DevBuf<int> counters;                                             // [B][kKfInts]
  long long dropped_reported = 0;                                   // nodes kept without clouds aloam_synchronize has already returned
};
struct GraphMapScratch {             // the map at the graph's poses (aloam_graph_export_map): grown on first use, used in stream order
  Scratch<float4> world, grouped;                                   // transformed points as laid out for the bounds; grouped by (request, class, cube)
  Scratch<int> slot;                                                // directory slot of every transformed point
  Scratch<unsigned long long> dir_key; Scratch<int> dir_count; Scratch<long long> dir_base;   // the directory of (request, class, cube, piece): keys, counts / cursors, bases
  Scratch<GmRequest> req; Scratch<GmRequestOut> req_out;
  Scratch<GmPart> parts; Scratch<double> frames;                    // aloam_graph_export_map_joint: the parts of its groups and the frames they name
  Scratch<int> ints;                                                // first piece per (request, class), points outside per request, the overflow flag
  Scratch<AtlasMergeJob> jobs;                                      // one per (request, class, cube), with its filtered size and point offset
  Scratch<GmSegInfo> seg; Scratch<int> counts; Scratch<long long> point_off;
  long long dir_hint = 0;                                           // the directory size an earlier call had to grow to
  long long last_raw = 0; int last_segs = -1;                       // the last call that succeeded (algorithmic bytes); -1 while its scratch is not valid
};
struct GraphApplyScratch {           // a solved graph carried into the live state (aloam_graph_apply): grown on first use, used in stream order
  Scratch<GaItem> items;                                            // the listed sequences of one call
  Scratch<long long> off;                                           // the offsets the map pass writes for its requests
};
// Loop edges (aloam_graph_loops_enable): the scratch of `slots` registrations, used in stream order; the slots are the "sequences" of a
// scratch MapArgs (loopreg_kernels.hpp), so every per-sequence array of the mapping step has a per-slot twin here.
struct LoopScratch {
  bool on = false;
  int slots = 0, H = 0, tile_bound = 0, tile_cap = 0, levels = 0;
  long long cap[2] = {0, 0}, key_cap = 0;                           // raw target points per slot: corner, surf; keys of the general voxel path
  DevBuf<aloam_graph_loop_request> req;                             // [slots] the round's requests
  StageRing<kLoopStageSlots> ring;                                  // a slot holds `slots` requests
  DevBuf<float4> raw[2], target[2], sorted[2], stack[2], knn, voxtmp;
  DevBuf<int> start[2], plan, rec_tiles, list, vox_counters, vox_lists, bbox, tile_seg, tile_heads, tile_pref;
  DevBuf<unsigned long long> keys[2];
  DevBuf<MapSeq> seq;
  DevBuf<MapEdgeRec> edges; DevBuf<MapNormRec> norms;
  DevBuf<VoxSeg> segs;
  DevBuf<aloam_pose_information> info;
  Scratch<LoopSearchPartial> search_part;                           // aloam_graph_search_loops: [round][K][kLoopSearchParts], nothing before its first call
};
struct MarginalScratch {             // pose-graph marginals (aloam_graph_marginals): nothing is allocated before the first call; used in stream order
  DevBuf<GraphMarginalItem> items;                                  // [kMarginalStageItems] the round's requests
  StageRing<kMarginalStageSlots> ring;                              // a slot holds kMarginalStageItems requests
  Scratch<double> f64; Scratch<int> i32;                            // the scratch rows, one per request of a round
  long long last_nodes = 0, last_edges = 0; int last_n = 0;         // the last call (algorithmic bytes)
};
struct ProposeScratch {              // loop candidates by pose proximity (aloam_graph_propose_loops): nothing is allocated before the first call; used in stream order
  DevBuf<GraphProposeQuery> queries;                                // [kProposeStageItems] the round's queries
  StageRing<kProposeStageSlots> ring;                               // a slot holds kProposeStageItems queries
};
struct TrimScratch {                 // pose graphs trimmed in place (aloam_graph_trim): nothing is allocated before the first call; used in stream order
  DevBuf<GraphTrimItem> items;                                      // [B] the listed sequences of one call
  StageRing<kTrimStageSlots> ring;                                  // a slot holds B items
  PinnedBuf<int> h_out; int* d_out = nullptr;                       // [B][kTrimRecordInts] what k_graph_trim reports (pinned, mapped)
};
struct JointScratch {                // joined pose graphs (aloam_graph_optimize_joint): nothing is allocated before the first call; used in stream order
  StageRing<kJointStageSlots> ring;                                 // a slot holds one call's items, groups, members and links, back to back
  size_t slot_bytes = 0;                                            // what a slot holds; a call that needs more waits for the stream and builds a larger ring
  Scratch<char> staged;                                             // the device copy of one call's slot
  Scratch<aloam_graph_node> nodes;                                  // [n_groups][row_nodes] the joined node rows
  Scratch<aloam_graph_edge> edges;                                  // [n_groups][row_edges] the joined edge rows
  int row_nodes = 0, row_edges = 0;                                 // the rows' strides as the last call laid them out
  std::vector<JointGroup> last;                                     // the last call's groups (aloam_graph_joint_export)
};
// Links measured on the device (aloam_graph_register_links / aloam_graph_search_links / aloam_graph_propose_links): nothing is allocated
// before the first call that needs it; used in stream order.  The registrations run in the scratch of LoopScratch.
struct LinkScratch {
  DevBuf<aloam_graph_link_request> req;                             // [LoopScratch::slots] the round's link records, read by k_link_gather
  StageRing<kLoopStageSlots> ring;                                  // a slot holds `slots` link records; acquired in step with LoopScratch::ring
  DevBuf<LinkProposeQuery> queries;                                 // [kProposeStageItems] the round's queries with their frames
  StageRing<kProposeStageSlots> query_ring;                         // a slot holds kProposeStageItems staged queries
};

struct GraphRecordScratch {          // graph records (aloam_graph_save / aloam_graph_load): sized for `batch` records on first use, used in stream order
  DevBuf<GraphRecItem> items;                                       // [B] the records of one call
  DevBuf<int> units, chunk; DevBuf<long long> uoff;                 // save: lengths, [B + 1] chunk / unit offsets
  PinnedBuf<char> h; char* d_h = nullptr;                           // load (pinned, mapped): the offsets the check reads, the headers and verdicts it
                                                                    // writes; behind them the offsets / chunks / items staged for the unpack
  DevBuf<char> staged;                                              // load: that last part in device memory
  Scratch<char> stage;                                              // load: records from pageable host memory
};

// What the host knows about one sequence without asking the device (mirrors of device state that only host calls change, then its map, then what the device
// holds for its sweep and last clouds).  Written only by aloam_create_stages and the events of capi_seq.hip (the table of events against fields).
struct SeqHost {
  int active = 1;                    // the mask in force (aloam_set_active), 0 / 1
  int reg_active = 1;                // the mask of the last registration, while its odometry step is still to come (reg_pending)
  int parity = 0, inited = 0;        // SeqMeta::parity, OdomState::inited
  bool needs_odom = false;           // loaded by aloam_load_sequences and not yet through an odometry step: may not map
  long long map_err_seen = 0;        // pool capacity events (MapSeq.err_steps) aloam_synchronize has already returned
  bool frozen = false;               // aloam_set_map_frozen: localizes against its map in the mapping steps, does not extend it
  bool scorable = false;             // last took part in a mapping step frozen, and its search grid has not been invalidated since
  bool attached = false;             // mirror of d_at_attached (with the device mark d_at_stale: the next step cuts the window anew)
  bool has_sweep = false;            // holds a registered sweep (since creation / reset / load): a place descriptor can be made
  bool desc_valid = false;           // d_pl_desc[b] is that sweep's
  bool info_odom = false, info_map = false;   // the records and the pose of its last odometry / mapping solve are still in place
                                     // (aloam_export_pose_information; else ALOAM_INFO_NONE).  Host state only: not part of a sequence record
  int graph_nodes = 0, graph_edges = 0;   // its pose graph (aloam_graph_*): what its rows of the store hold.  Host state only, and not the sequence's
                                     // but the slot's: reset and load leave it, aloam_graph_clear empties it
  bool has_stacks = false;           // took part in a mapping step since creation / reset / load: its stacks can be kept as a keyframe's clouds
  bool grid_built = false;           // the grid set of its LAST clouds holds their grids: set by the step that made them the last ones if it built
                                     // them beside its solve (aloam_odometry_step; not aloam_process_*, which build inside the next call),
                                     // cleared by whatever writes or replaces the last clouds outside a step
};
}  // namespace aloam

struct aloam_ctx {
  // Streams and events first: members are destroyed in reverse order, so every buffer is released before them (a StageRing further
  // down keeps its own events: aloam_destroy has drained every stream before anything is destroyed).
  Stream stream, copy_stream;
  Stream grid_stream;                // a step's grid build runs here: beside the registration of the same call (aloam_process_*), or the next step's beside the association and the solve (aloam_odometry_step)
  Event in_copied[2], in_consumed[2], map_step_done[4];
  Event grid_fork, grids_done;       // main stream -> grid stream where the build is forked, grid stream -> main stream where it is joined (GridFork, capi_odometry.hip)
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
  Scratch<char> d_in[2];
  int in_slot = 0;
  bool in_used[2] = {false, false};
  DevBuf<int> d_nin;
  StageRing<kNinSlots> nin;                         // a slot holds B ints (counts, masks, reset ids): stage_ints
  std::vector<SeqHost> seq;                         // [B] per-sequence host state
  bool all_active = true, any_frozen = false, any_attached = false;   // aggregates of seq[].active / frozen / attached, each recomputed by that field's event
  bool reg_pending = false;
  const int* reg_mask = nullptr;                    // what the last registration's kernels were given (nullptr = all); k_dense_cloud reuses it
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
  // search grids, [set][class]: set p of a sequence describes its cloud buffer p (OdomArgs)
  DevBuf<float4> d_grid_sorted3[2][2], d_grid_sorted2[2][2];
  DevBuf<int> d_grid_start3[2][2], d_grid_start2[2][2];
  DevBuf<float4> d_grid_sorted3c[2][2];   // coarse level of the 3-D grid
  DevBuf<int> d_grid_start3c[2][2];
  DevBuf<int> d_grid_flags[2][2], d_grid_walk[2][2];
  int grid_H[2] = {4096, 16384};
  bool solve_stage = true;           // environment ALOAM_SOLVE_STAGE (default on), read once at creation: k_solve keeps its factor records in LDS across the passes of a solve
  bool grid_overlap = false;         // environment ALOAM_GRID_OVERLAP (default on), read once at creation; off with use_graph / debug_sync
  DevBuf<EdgeRec> d_edges; DevBuf<PlaneRec> d_planes;
  DevBuf<float4> d_sel_sharp, d_sel_flat;
  // scan-to-map refinement (allocated by aloam_mapping_enable)
  bool map_on = false;
  long long map_err_reported = 0;    // voxel-scratch capacity events (vox counters[3]) aloam_synchronize has already returned
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
  DevBuf<MapGridSig> d_grid_sig;     // [B][2] what each submap grid was last built from (grid reuse of frozen sequences)
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
  Scratch<float4> d_exp_tmp;                                        // aloam_get_map_cloud(SURROUND / FULL): the segment of one sequence
  DevBuf<long long> d_exp_tmp_off;
  // sequence records (aloam_save_sequences / aloam_load_sequences): scratch sized for `batch` records on first use, used in stream order
  DevBuf<int> d_ck_seqs, d_ck_info, d_ck_units, d_ck_chunk, d_ck_pref; DevBuf<long long> d_ck_uoff;   // save: ids, counts, lengths, prefixes
  PinnedBuf<char> h_ck; char* d_ck_host = nullptr;                  // load: headers read back, then the staged offsets / chunks / counts (pinned, mapped)
  DevBuf<char> d_ck_load;                                           // load: the same staged arrays in device memory
  Scratch<char> d_ck_stage;                                         // load: records from pageable host memory
  int ck_save_n = 0; long long ck_load_bytes = 0;                   // the last save / load (algorithmic bytes)
  // map-pose hypotheses (aloam_score_map_corrections / aloam_apply_map_corrections)
  DevBuf<int> d_rl_seqs, d_rl_bad;                                  // [B] listed ids; [1] choices found outside 0 .. K-1 by k_apply_corrections
  Scratch<ScorePartial> d_rl_part;                                  // [n][K][kScoreParts] per-workgroup partials
  Scratch<aloam_map_correction> d_rl_cand;                          // candidates handed in as pageable host memory
  long long rl_bad_reported = 0;                                    // of d_rl_bad, already returned by aloam_synchronize
  std::vector<int> rl_last_seqs; int rl_last_K = 0;                 // the last scoring call: its listed sequences and K (algorithmic bytes)
  int rl_apply_n = 0;
  // pose information (aloam_export_pose_information)
  DevBuf<int> d_info_list;                                          // [B] listed ids with their "solved" bit
  std::vector<int> info_last_list; int info_last_which = 0;         // the last call (algorithmic bytes)
  // the graph family (aloam_graph_*): each feature's state is one struct, above
  GraphStore pg;
  KeyframeStore kf;
  GraphMapScratch gm;
  GraphApplyScratch ga;
  LoopScratch lr;
  MarginalScratch mg;
  ProposeScratch pp;
  TrimScratch tr;
  JointScratch jt;
  LinkScratch lk;
  GraphRecordScratch gr;
  // map spill (aloam_map_spill_enable): what the window shifts of the mapping steps empty, kept as tiles until the host drains them
  bool spill_on = false;
  int spill_max_tiles = 0, spill_max_points = 0;
  DevBuf<aloam_map_tile> d_sp_tiles; DevBuf<float4> d_sp_points;   // [B][2][max_tiles], [B][2][max_points]
  DevBuf<int> d_sp_counters;                                        // [B][kSpillInts]
  DevBuf<int> d_sp_seqs, d_sp_cnt, d_sp_chunk; DevBuf<long long> d_sp_off;   // the drain: listed ids, [2][B] counts, [2][B + 1] chunk / element offsets (tiles, points)
  // atlas (aloam_atlas_load / aloam_atlas_attach): one immutable tile store, shared by the attached sequences
  bool atlas_on = false;
  DevBuf<int> d_at_attached, d_at_stale;                            // [B] each; stale != 0: the next step cuts the window anew
  DevBuf<AtlasEntry> d_at_dir[2]; int at_dir_mask[2] = {0, 0};      // per class: directory absolute cube -> (first, count)
  DevBuf<float4> d_at_points[2];
  long long at_info[12] = {0};                                      // what aloam_atlas_info returns
  long long spill_dropped_reported = 0;                             // dropped tiles aloam_synchronize has already returned
  // place recognition (aloam_places_enable): one descriptor per sequence, one store per context
  bool places_on = false;
  int pl_capacity = 0, pl_count = 0;                                // entries the store holds / has; the count is host state (adds are stream-ordered)
  float pl_max_range = 80.f, pl_height = 2.f;
  DevBuf<PlaceDesc> d_pl_desc;                                      // [B]
  DevBuf<aloam_place> d_pl_store;                                   // [capacity]
  DevBuf<float> d_pl_unit; DevBuf<unsigned long long> d_pl_masks;   // [capacity][1200] unit-normalised columns, [capacity] non-zero columns
  DevBuf<int> d_pl_seqs, d_pl_wanted, d_pl_lo, d_pl_hi;             // [B] each: listed ids, descriptors to make, the ranges of a match
  Scratch<int2> d_pl_pairs;                                         // [n][longest range] per-entry results of a match
  // range-image input (aloam_set_range_decoder, capi_range.hip): the decoder's scalars and the device copies of its tables
  bool range_on = false;
  int rd_rows = 0, rd_n_az = 0, rd_order = 0; float rd_scale = 0.f;
  DevBuf<float2> d_rd_az;                                           // [n_az] {az_x, az_y}
  DevBuf<float> d_rd_rows;                                          // [kRangeRowTables][kMaxRings]
  std::vector<int> range_cols;                                      // columns per sequence of the last registration when it read range images, else empty (algorithmic bytes)
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

namespace aloam {

// allocate and zero on the context's stream: the kernels rely on zeroed look-back granules, tickets and counters
template <typename T>
int dmalloc(aloam_ctx* c, DevBuf<T>& p, size_t count) {
  HIP_TRY(c, dalloc(p, count));
  HIP_TRY(c, hipMemsetAsync(p.get(), 0, count * sizeof(T), c->stream));
  return ALOAM_OK;
}

hipEvent_t prof_event(aloam_ctx* c);
struct ProfScope {
  aloam_ctx* c; int k; hipStream_t s; hipEvent_t e0 = nullptr;
  // `on`: the stream the scope's launches go to (default: the context's; the grid stream records intervals that overlap the main stream's)
  ProfScope(aloam_ctx* c_, int k_, hipStream_t on = nullptr) : c(c_), k(k_), s(on ? on : (hipStream_t)c_->stream) {
    if (c->prof_on) { e0 = prof_event(c); (void)hipEventRecord(e0, s); }
  }
  ~ProfScope() {
    if (c->prof_on) { hipEvent_t e1 = prof_event(c); (void)hipEventRecord(e1, s); c->prof_pending.push_back({k, e0, e1}); }
    if (c->debug_sync) {   // ALOAM_DEBUG_SYNC=1: wait after every stage and name it, so that a device fault can be pinned on a kernel
      const hipError_t e = hipStreamSynchronize(s);
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

// The per-sequence struct at `dev` (SeqMeta, OdomState, MapSeq, a count in one of them) read back after the stream has drained.
template <typename T>
int read_seq(aloam_ctx* c, const T* dev, T* out) {
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, hipMemcpy(out, dev, sizeof(T), hipMemcpyDeviceToHost));
  return ALOAM_OK;
}

// The per-sequence struct at `dev` read back (read_seq), changed by `edit`, written again.
template <typename T, typename Edit>
int edit_seq(aloam_ctx* c, T* dev, Edit edit) {
  T v;
  if (const int rc = read_seq(c, dev, &v)) return rc;
  edit(v);
  HIP_TRY(c, hipMemcpy(dev, &v, sizeof(T), hipMemcpyHostToDevice));
  return ALOAM_OK;
}

template <typename T>
int Scratch<T>::grow(aloam_ctx* c, long long need) {
  if (cap >= need) return ALOAM_OK;
  release();
  HIP_TRY(c, dalloc(p, (size_t)need));
  cap = need;
  return ALOAM_OK;
}

template <int Slots>
template <typename T>
int StageRing<Slots>::acquire(aloam_ctx* c, T** slot, int* index) {
  const int ns = cursor;
  cursor = (ns + 1) % Slots;
  if (used[ns]) HIP_TRY(c, hipEventSynchronize(done[ns]));
  *slot = reinterpret_cast<T*>(mem.get() + (size_t)ns * slot_bytes);
  *index = ns;
  return ALOAM_OK;
}
template <int Slots>
int StageRing<Slots>::queue(aloam_ctx* c, int index, const void* src, size_t bytes, void* dst, hipStream_t stream) {
  HIP_TRY(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, stream));
  HIP_TRY(c, hipEventRecord(done[index], stream));
  used[index] = true;
  return ALOAM_OK;
}

// The row of sequence `seq` that a getter reads through `s` (cloud_desc): base[0 / parity / 1 - parity] + seq * stride; nullptr when this
// context has no buffer for it (aloam_create_stages leaves some out).  Writable: the setters fill the context's own buffers through it.
inline float4* cloud_row(const aloam_ctx* c, const ExportSrc& s, int seq) {
  const int r = s.sel == kSelFixed ? 0 : s.sel == kSelCurrent ? c->seq[seq].parity : 1 - c->seq[seq].parity;
  return s.base[r] ? const_cast<float4*>(s.base[r]) + (size_t)seq * s.stride : nullptr;
}

// aloam_capi.hip
int stage_ints(aloam_ctx* c, const int* src, int n, int* dst);
int check_seq(aloam_ctx* c, int seq);
int require_stage(aloam_ctx* c, int stage);
int check_ids(aloam_ctx* c, const int* ids, int n);
// capi_odometry.hip
// One registration of a checked batch: n_in = points per sequence; n_cols != nullptr: the sweeps are range images of that many columns (capi_range.hip).
int register_launch(aloam_ctx* c, const void* d_scans, long long seq_stride, const int* n_in, int stride_bytes, int slot = -1, bool debug_arrays = true,
                    const int* n_cols = nullptr, const std::function<void()>* after_front = nullptr);
// A host-resident batch into the next staging slab, on the copy stream: rows 0 .. B-2 with `row` bytes each, the last with `last`; the compute stream waits for it.
int stage_batch(aloam_ctx* c, const void* h_scans, long long seq_stride_bytes, size_t row, size_t last, size_t d_seq_stride, int* slot, char** d_in);
int ensure_dense(aloam_ctx* c);
long long cloud_desc(const aloam_ctx* c, int id, ExportSrc* s);
int find_cloud(aloam_ctx* c, int seq, int id, const float4** ptr, int* n);
// capi_odometry.hip / capi_mapping.hip: the kernel arguments of a stage as the context stands (the caller sets `active`)
OdomArgs odom_args(aloam_ctx* c);
MapArgs map_args(aloam_ctx* c);
// capi_mapping.hip
int grow_map_pool(aloam_ctx* c, long long want, bool clamp);
// capi_atlas.hip
void queue_map_spill(aloam_ctx* c, const int* mask);
int spill_dropped_since(aloam_ctx* c, long long* fresh);
int atlas_step_check(aloam_ctx* c);                      // ALOAM_E_STATE when an attached sequence that is active in this step is not frozen
bool queue_atlas_window(aloam_ctx* c, const int* mask);  // k_atlas_window when an attached sequence takes part
// The largest number of points any 21 x 21 x 11 box of cubes holds (keys: atlas_key of every cube, lo / hi: their bounding box); *exact = false: the class total instead
long long largest_window(const std::vector<int>& keys, const std::vector<int>& counts, const int lo[3], const int hi[3], bool* exact);
// capi_graphmap.hip
KfStore kf_store(aloam_ctx* c);                                      // the keyframe store as the kernels see it
int keyframe_add_check(aloam_ctx* c, const int* seqs, int n);        // ALOAM_E_STATE when a listed sequence holds no stacks (store enabled)
void queue_keyframe_capture(aloam_ctx* c, int n);                    // k_keyframe_capture behind k_graph_add_nodes, for the items in pg.add
int queue_keyframe_rewind(aloam_ctx* c, const int* seqs, int n);     // aloam_graph_clear: the listed cursors back to 0, in stream order
int keyframes_dropped_since(aloam_ctx* c, long long* fresh);
int require_keyframes(aloam_ctx* c);                                 // ALOAM_E_STATE before aloam_graph_keyframes_enable
int graph_map_scratch(aloam_ctx* c, long long bound_points);         // world / grouped / slot of a map export, sized for the host's bounds
// What aloam_graph_export_map and aloam_graph_export_map_joint share: everything behind the layout of the piece table.  The two passes
// over that table are the caller's (per request, or per part); the transform is handed the directory's mask and reads the directory's
// arrays from c->gm at that moment (they grow), the grouping pass runs with what the last transform ran with.
struct GmPasses { std::function<void(unsigned dir_mask)> transform; std::function<void()> group; };
struct GmDst { void* tiles; long long cap_tiles; void* points; long long cap_points; void* offsets; void* stats; };   // classified destinations (nullptr: not given)
int graph_map_run(aloam_ctx* c, int n, int n_pieces, int* d_outside, int* d_flags, const GmPasses& passes, const GmDst& dst, const char* unit);
// capi_seq.hip: the one "does sequence b take part in this step", a stage's mask, and what happens to a sequence, each with its whole consequence
inline bool takes_part(const aloam_ctx* c, int b) { return c->all_active || c->seq[b].active; }
struct StageMask {
  std::vector<int> bits;             // [B] SeqBits of every sequence in this step
  const int* dev = nullptr;          // bits as the launches see them; nullptr: the stage runs unmasked (the kernels then load nothing)
  bool any_active = false, any_solve = false, all_solve = true, any_grow = false;
};
int stage_mask(aloam_ctx* c, DevBuf<int>& dst, int (*extra_bits)(const SeqHost&), bool (*unmasked)(const aloam_ctx*, const StageMask&), StageMask* m);
void on_active_mask_set(aloam_ctx* c, const int* active);
void on_frozen_mask_set(aloam_ctx* c, const int* frozen);
int on_slots_reset(aloam_ctx* c, const int* seqs, int n);
void on_slot_loaded(aloam_ctx* c, int seq, bool inited, long long err_events);
void on_sweep_registered(aloam_ctx* c);
void on_odometry_advanced(aloam_ctx* c, const StageMask& m, bool built_next);
void on_last_clouds_replaced(aloam_ctx* c, int seq);
void on_odometry_inputs_replaced(aloam_ctx* c, int seq);
void on_map_corrections_applied(aloam_ctx* c, const int* seqs, int n);
void on_system_inited_forced(aloam_ctx* c, int inited);
int on_map_replaced(aloam_ctx* c, int seq);
int on_map_pool_reallocated(aloam_ctx* c, MapPool&& fresh);
void on_mapping_step_queued(aloam_ctx* c);
int on_atlas_attached(aloam_ctx* c, const std::vector<int>& attached);
void on_places_enabled(aloam_ctx* c);
void on_descriptors_made(aloam_ctx* c, const int* seqs, int n);
void on_graph_nodes_added(aloam_ctx* c, const int* seqs, int n);
void on_graph_edges_added(aloam_ctx* c, int seq, int count);
void on_graph_cleared(aloam_ctx* c, const int* seqs, int n);
int on_graph_applied(aloam_ctx* c, const int* seqs, int n);
void on_graph_loaded(aloam_ctx* c, int seq, int nodes, int edges);
void on_graph_trimmed(aloam_ctx* c, int seq, int nodes, int edges);
long long on_pool_events_reported(aloam_ctx* c, int seq, long long events);
// capi_posegraph.hip
int require_graph(aloam_ctx* c);
// What aloam_graph_add_edges asks of an edge, for it and for the candidates of aloam_graph_marginals: seq, i and j always; with `measurement`
// also flags, Z (q is normalised in place) and info.  nullptr, or what is wrong.
const char* graph_edge_check(const aloam_ctx* c, aloam_graph_edge& e, bool measurement);
// capi_loopreg.hip: the one body behind aloam_graph_register_loops / _search_loops (links == nullptr) and aloam_graph_register_links /
// _search_links (req == nullptr, links given: the round's gather is k_link_gather, and the link records are staged beside the requests)
int register_loops(aloam_ctx* c, const aloam_graph_loop_request* req, const aloam_graph_link_request* links, int n, const aloam_graph_loop_options* opt,
                   aloam_graph_loop_result* dst, const aloam_graph_loop_search* search_or_default, bool searched, aloam_graph_loop_search_result* search_dst,
                   aloam_map_score* scores);
// capi_mapping.hip
VoxArgs vox_args(aloam_ctx* c, int n_segs, int levels);
// capi_records.hip
enum CallerMem { kMemPageable, kMemDevice, kMemPinned, kMemManaged, kMemOtherDevice };
CallerMem classify_pointer(const aloam_ctx* c, const void* p, void** dev);
int require_host_list(aloam_ctx* c, const void* p, const char* name);   // ALOAM_E_ARG unless a request list is host memory, pinned or pageable
int export_target(aloam_ctx* c, const void* p, size_t align, const char* what, void** out);
int get_cube_list(aloam_ctx* c, int seq, int which, float* out, int cap_points);
// Where a load reads `p` from: *dev = the address the kernels use (device memory of the context's device, pinned host memory), or nullptr for
// pageable host memory, which is staged.  Another device's memory, managed memory and NULL are refused.
int load_source(aloam_ctx* c, const void* p, const char* what, const void** dev, bool* on_host);

}  // namespace aloam
