// a-loam_amd/csrc/capi_records.hip — host side of the batched export (poses and clouds of every sequence) and of the sequence records
// (save / load).
#include <algorithm>
#include <cstring>

#include "capi_internal.hpp"

// ---- batched export -----------------------------------------------------------------------------------------------------
// What a caller's pointer is to the context's device.  *dev is the address its kernels reach `p` through: device memory of the context's
// device as it is, pinned host memory through its device mapping; nullptr for the rest.  kMemPageable: host memory without a device mapping
// (or NULL), which the kernels cannot reach.
namespace aloam {
CallerMem classify_pointer(const aloam_ctx* c, const void* p, void** dev) {
  hipPointerAttribute_t at{};
  *dev = nullptr;
  if (!p || hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return kMemPageable; }   // (pageable memory is an error of the query, not of the context)
  if (at.isManaged) return kMemManaged;
  if (at.type == hipMemoryTypeDevice) {
    if (at.device != c->cfg.device) return kMemOtherDevice;
    *dev = const_cast<void*>(p);
    return kMemDevice;
  }
  if (at.type == hipMemoryTypeHost && hipHostGetDevicePointer(dev, const_cast<void*>(p), 0) == hipSuccess) return kMemPinned;
  (void)hipGetLastError();
  *dev = nullptr;
  return kMemPageable;
}

// A request list that the host reads before anything is queued: host memory, pinned or pageable.
int require_host_list(aloam_ctx* c, const void* p, const char* name) {
  void* dev = nullptr;
  const CallerMem m = classify_pointer(c, p, &dev);
  if (m != kMemPageable && m != kMemPinned) { c->err = std::string(name) + " must be host memory, pinned or pageable"; return ALOAM_E_ARG; }
  return ALOAM_OK;
}

// The address a kernel writes `p` through: device memory of the context's device as it is, pinned host memory through its device mapping.
// Pageable host memory (with XNACK off a kernel store there faults the device), managed memory, another device's memory and NULL are refused.
int export_target(aloam_ctx* c, const void* p, size_t align, const char* what, void** out) {
  void* d = nullptr;
  (void)classify_pointer(c, p, &d);                       // (d is set for device memory of this device and pinned host memory only)
  if (!d) { c->err = std::string(what) + " must be device memory of the context's device or pinned host memory"; return ALOAM_E_ARG; }
  if ((uintptr_t)p % align || (uintptr_t)d % align) { c->err = std::string(what) + " must be " + std::to_string(align) + "-byte aligned"; return ALOAM_E_ARG; }
  *out = d;
  return ALOAM_OK;
}
}  // namespace aloam

// Where export id `id` (ALOAM_CLOUD_* or ALOAM_EXPORT_MAP + ALOAM_MAP_*) is read from: the buffers and counts the getters read (cloud_desc),
// with their checks.  Queues nothing.
static int export_src(aloam_ctx* c, int id, ExportSrc* s) {
  *s = ExportSrc{};
  if (id >= ALOAM_EXPORT_MAP + ALOAM_MAP_REGISTERED && id <= ALOAM_EXPORT_MAP + ALOAM_MAP_FULL && !c->map_on) { c->err = "mapping not enabled"; return ALOAM_E_STATE; }
  if (id == ALOAM_EXPORT_MAP + ALOAM_MAP_SURROUND || id == ALOAM_EXPORT_MAP + ALOAM_MAP_FULL) {
    s->kind = id == ALOAM_EXPORT_MAP + ALOAM_MAP_SURROUND ? kExportSurround : kExportFull;
    return ALOAM_OK;
  }
  if (!cloud_desc(c, id, s)) { c->err = "unknown cloud id " + std::to_string(id); return ALOAM_E_ARG; }
  // find_cloud's rule: the row a getter of any sequence would read must exist (aloam_create_stages leaves some buffers out)
  for (int b = 0; b < c->B; ++b)
    if (!cloud_row(c, *s, b)) { c->err = "this context holds no such cloud (see aloam_create_stages)"; return ALOAM_E_STATE; }
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

namespace aloam {

// aloam_get_map_cloud(SURROUND / FULL): the export of one sequence into the context's scratch, then one copy to the caller.
int get_cube_list(aloam_ctx* c, int seq, int which, float* out, int cap_points) {
  ExportSrc src;
  int rc = export_src(c, ALOAM_EXPORT_MAP + which, &src);
  if (rc) return rc;
  if (!c->d_exp_tmp_off) HIP_TRY(c, dalloc(c->d_exp_tmp_off, 2));
  long long off[2] = {0, 0};
  for (int pass = 0; pass < 2; ++pass) {                  // a second pass only when the scratch was too small for the points asked for
    if ((rc = queue_export(c, &src, 1, false, seq, 1, c->d_exp_tmp.get(), c->d_exp_tmp.cap, c->d_exp_tmp_off.get()))) return rc;
    HIP_TRY(c, hipMemcpyAsync(off, c->d_exp_tmp_off.get(), sizeof(off), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (cap_points <= 0 || off[1] <= c->d_exp_tmp.cap) break;
    if ((rc = c->d_exp_tmp.grow(c, off[1]))) return rc;
  }
  const long long k = std::min<long long>(off[1], cap_points);
  if (k > 0) HIP_TRY(c, hipMemcpy(out, c->d_exp_tmp.get(), sizeof(float4) * k, hipMemcpyDeviceToHost));
  return (int)off[1];
}

}  // namespace aloam

extern "C" {

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
int aloam::load_source(aloam_ctx* c, const void* p, const char* what, const void** dev, bool* on_host) {
  *dev = nullptr; *on_host = true;
  if (!p) { c->err = std::string(what) + " is NULL"; return ALOAM_E_ARG; }
  void* d = nullptr;
  switch (classify_pointer(c, p, &d)) {
    case kMemManaged: c->err = std::string(what) + " must be device memory of the context's device, pinned or pageable host memory"; return ALOAM_E_ARG;
    case kMemOtherDevice: c->err = std::string(what) + " is memory of another device"; return ALOAM_E_ARG;
    case kMemDevice: *on_host = false; break;
    default: break;                                      // pinned host memory: readable by the host and (through *dev) by the kernels; pageable: staged
  }
  *dev = d;
  return ALOAM_OK;
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
  ExportSrc s;
  if (h.n_corner_last > cloud_desc(c, ALOAM_CLOUD_CORNER_LAST, &s) || h.n_surf_last > cloud_desc(c, ALOAM_CLOUD_SURF_LAST, &s))
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
  if (c->map_on && need > c->map.points) if (const int rc = grow_map_pool(c, need, true)) return rc;
  const char* base = static_cast<const char*>(d_src);
  if (!base) {                                            // pageable host memory: staged into device memory (the span of the n records)
    const size_t span = (size_t)(off[n] - off[0]);
    if (const int rc = c->d_ck_stage.grow(c, span)) return rc;
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
  if (const int rc = on_slots_reset(c, slots, n)) return rc;
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
  c->ck_load_bytes = off[n] - off[0];
  for (int i = 0; i < n; ++i) {
    on_slot_loaded(c, slots[i], hdr[i].inited != 0, hdr[i].err_events);
    if (c->map_on) for (int k = 0; k < 2; ++k) c->h_map_report[1 + k] = std::max((int)c->h_map_report[1 + k], hdr[i].map_points[k]);
  }
  return ALOAM_OK;
}

}  // extern "C"
