// a-loam_amd/csrc/capi_graphrecords.hip — host side of the graph records (aloam_graph_save / aloam_graph_load): the pose
// graph of a sequence and the clouds of its nodes as a position-independent record.  The save is stream-ordered with no host wait, as
// aloam_save_sequences.  The load waits for the stream once, behind the check kernel: the host then holds every header and one verdict per
// record and decides everything before anything of the context changes.
#include <algorithm>
#include <cstring>

#include "capi_internal.hpp"

// The rows of the graph store and of the keyframe store as the record kernels see them.
static GraphRecStore rec_store(aloam_ctx* c) {
  GraphRecStore s{};
  s.nodes = c->pg.nodes.get(); s.edges = c->pg.edges.get(); s.max_nodes = c->pg.max_nodes; s.max_edges = c->pg.max_edges;
  s.keyframes = c->kf.on;
  if (c->kf.on) {
    s.kf = kf_store(c);
    std::memcpy(&s.line_res_bits, &c->map_line_res, 4); std::memcpy(&s.plane_res_bits, &c->map_plane_res, 4);
  }
  return s;
}

// Pinned staging of a load: what the check kernel reads and writes (offsets [B + 1], headers [B], verdicts [B]), then what is copied to
// device memory for the unpack (offsets [B + 1], items [B], chunk offsets [B + 1]).  The two parts are written on either side of the call's wait.
struct LoadStage { size_t off, hdr, verdict, u_off, u_items, u_chunk, bytes; };
static LoadStage load_stage(size_t B) {
  LoadStage s{};
  s.off = 0;
  s.hdr = (8 * (B + 1) + 15) & ~(size_t)15;
  s.verdict = s.hdr + sizeof(aloam_graph_record_header) * B;
  s.u_off = (s.verdict + 4 * B + 15) & ~(size_t)15;
  s.u_items = (s.u_off + 8 * (B + 1) + 15) & ~(size_t)15;
  s.u_chunk = s.u_items + sizeof(GraphRecItem) * B;
  s.bytes = s.u_chunk + 4 * (B + 1);
  return s;
}

static int save_scratch(aloam_ctx* c) {
  const size_t B = c->B;
  if (!c->gr.items) HIP_TRY(c, dalloc(c->gr.items, B));
  if (!c->gr.units) { HIP_TRY(c, dalloc(c->gr.units, B)); HIP_TRY(c, dalloc(c->gr.chunk, B + 1)); HIP_TRY(c, dalloc(c->gr.uoff, B + 1)); }
  return ALOAM_OK;
}
static int load_scratch(aloam_ctx* c) {
  const LoadStage st = load_stage(c->B);
  if (c->gr.h) return ALOAM_OK;
  char* p = nullptr;
  HIP_TRY(c, hipHostMalloc((void**)&p, st.bytes, hipHostMallocMapped));
  c->gr.h.reset(p);
  HIP_TRY(c, hipHostGetDevicePointer((void**)&c->gr.d_h, p, 0));
  HIP_TRY(c, dalloc(c->gr.staged, st.bytes - st.u_off));
  return ALOAM_OK;
}

// One header and its verdict against this context; names the first thing that differs.
static int check_record(aloam_ctx* c, int i, const aloam_graph_record_header& h, long long len, int verdict) {
  auto fail = [&](int rc, const std::string& what) { c->err = "record " + std::to_string(i) + ": " + what; return rc; };
  if (h.magic != ALOAM_GRAPH_RECORD_MAGIC) return fail(ALOAM_E_ARG, "bad magic (not a graph record)");
  if (h.version != ALOAM_GRAPH_RECORD_VERSION) return fail(ALOAM_E_ARG, "record version " + std::to_string(h.version) + ", this library reads version " + std::to_string(ALOAM_GRAPH_RECORD_VERSION));
  if (h.bytes != len) return fail(ALOAM_E_ARG, "record length (bytes) " + std::to_string(h.bytes) + " differs from the offsets' " + std::to_string(len));
  if (h.node_bytes != (int)sizeof(aloam_graph_node) || h.edge_bytes != (int)sizeof(aloam_graph_edge) || h.desc_bytes != (int)sizeof(KfDesc) || h.point_bytes != 16)
    return fail(ALOAM_E_ARG, "section sizes differ (node_bytes, edge_bytes, desc_bytes, point_bytes)");
  if (!(h.parts & ALOAM_GRAPH_PART_GRAPH) || (h.parts & ~(ALOAM_GRAPH_PART_GRAPH | ALOAM_GRAPH_PART_KEYFRAMES))) return fail(ALOAM_E_ARG, "unknown parts");
  const bool kf = (h.parts & ALOAM_GRAPH_PART_KEYFRAMES) != 0;
  if (kf != c->kf.on)
    return fail(ALOAM_E_ARG, kf ? "parts: it holds keyframe clouds and this context has no keyframe store (aloam_graph_keyframes_enable)"
                                : "parts: it holds no keyframe clouds and this context keeps them (aloam_graph_keyframes_enable)");
  if (h.nodes < 0 || h.edges < 0 || h.kf_points[0] < 0 || h.kf_points[1] < 0 || (!kf && (h.kf_points[0] || h.kf_points[1]))) return fail(ALOAM_E_ARG, "bad counts (nodes, edges, kf_points)");
  if (graph_rec_layout(kf, h.nodes, h.edges, h.kf_points[0], h.kf_points[1]).bytes != h.bytes) return fail(ALOAM_E_ARG, "record length (bytes) disagrees with its counts");
  unsigned int line = 0, plane = 0;
  if (kf) { std::memcpy(&line, &c->map_line_res, 4); std::memcpy(&plane, &c->map_plane_res, 4); }
  if (h.line_res_bits != line) return fail(ALOAM_E_ARG, "mapping_line_resolution differs from this context's");
  if (h.plane_res_bits != plane) return fail(ALOAM_E_ARG, "mapping_plane_resolution differs from this context's");
  if (h.nodes > c->pg.max_nodes) return fail(ALOAM_E_CAPACITY, "its " + std::to_string(h.nodes) + " nodes exceed this context's max_nodes");
  if (h.edges > c->pg.max_edges) return fail(ALOAM_E_CAPACITY, "its " + std::to_string(h.edges) + " edges exceed this context's max_edges");
  for (int k = 0; k < 2; ++k)
    if (kf && h.kf_points[k] > c->kf.cap[k])
      return fail(ALOAM_E_CAPACITY, "its " + std::to_string(h.kf_points[k]) + (k ? " surf" : " corner") + " keyframe points exceed this context's row");
  if (verdict) {
    const char* what = (verdict & kGraphRecBadHeader)      ? "the counts do not describe a record of this length"
                       : (verdict & kGraphRecBadEdgeIndex) ? "an edge outside -1 <= i < nodes, 0 <= j < nodes, i != j"
                       : (verdict & kGraphRecBadEdgeFlags) ? "an edge with unknown flags"
                       : (verdict & kGraphRecBadDescChain) ? "keyframe descriptors that are not back to back from 0"
                                                           : "keyframe descriptors that do not end at kf_points";
    return fail(ALOAM_E_ARG, std::string("payload: ") + what);
  }
  return ALOAM_OK;
}

extern "C" {

int aloam_graph_save(aloam_ctx* c, const int* seqs, int n, void* dst, long long cap_bytes, long long* dst_offsets) {
  DeviceScope device_scope(c);
  if (!c) return ALOAM_E_ARG;
  if (const int rc = require_graph(c)) return rc;
  if (const int rc = check_ids(c, seqs, n)) return rc;
  if (cap_bytes < 0) { c->err = "negative cap_bytes"; return ALOAM_E_ARG; }
  void *d_off = nullptr, *d_dst = nullptr;
  if (const int rc = export_target(c, dst_offsets, alignof(long long), "dst_offsets", &d_off)) return rc;
  if ((dst || cap_bytes > 0) && export_target(c, dst, 16, "dst", &d_dst)) return ALOAM_E_ARG;
  if (const int rc = save_scratch(c)) return rc;
  if (n > 0) {                                              // the counts are host state: they travel with the ids, through the graph's ring
    static_assert(sizeof(GraphRecItem) <= sizeof(GraphAddItem), "a slot of the graph's ring holds B items");
    GraphRecItem* items = nullptr;
    int slot = 0;
    if (const int rc = c->pg.ring.acquire(c, &items, &slot)) return rc;
    for (int i = 0; i < n; ++i) items[i] = GraphRecItem{seqs[i], c->seq[seqs[i]].graph_nodes, c->seq[seqs[i]].graph_edges, 0, 0, 0, 0, 0};
    if (const int rc = c->pg.ring.queue(c, slot, items, sizeof(GraphRecItem) * (size_t)n, c->gr.items.get(), c->stream)) return rc;
  }
  GraphRecSaveArgs a{};
  a.n = n; a.items = c->gr.items.get(); a.store = rec_store(c);
  a.units = c->gr.units.get(); a.chunk_off = c->gr.chunk.get(); a.unit_off = c->gr.uoff.get();
  a.dst_off = static_cast<long long*>(d_off); a.dst = static_cast<char*>(d_dst); a.cap_bytes = d_dst ? cap_bytes : 0;
  { ProfScope p(c, K_SAVE); launch_graph_save(a, c->gather_blocks, c->stream); }
  HIP_TRY(c, hipGetLastError());
  return ALOAM_OK;
}

int aloam_graph_load(aloam_ctx* c, const int* slots, int n, const void* src, const long long* src_offsets) {
  DeviceScope device_scope(c);
  if (!c) return ALOAM_E_ARG;
  if (const int rc = require_graph(c)) return rc;
  if (const int rc = check_ids(c, slots, n)) return rc;
  for (int i = 0; i < n; ++i)
    if (c->seq[slots[i]].graph_nodes > 0 || c->seq[slots[i]].graph_edges > 0) {
      c->err = "the graph of slot " + std::to_string(slots[i]) + " is not empty (aloam_graph_clear it first)";
      return ALOAM_E_STATE;
    }
  const void *d_src = nullptr, *d_offs = nullptr;
  bool src_host = false, offs_host = false;
  if (const int rc = load_source(c, src_offsets, "src_offsets", &d_offs, &offs_host)) return rc;
  if (n == 0) return ALOAM_OK;
  if (const int rc = load_source(c, src, "src", &d_src, &src_host)) return rc;
  if ((uintptr_t)src % 16) { c->err = "src must be 16-byte aligned"; return ALOAM_E_ARG; }
  if (const int rc = load_scratch(c)) return rc;
  const LoadStage st = load_stage(c->B);
  char* h = c->gr.h.get();
  long long* off = reinterpret_cast<long long*>(h + st.off);
  if (offs_host) std::memcpy(off, src_offsets, sizeof(long long) * (n + 1));
  else HIP_TRY(c, hipMemcpy(off, src_offsets, sizeof(long long) * (n + 1), hipMemcpyDeviceToHost));
  for (int i = 0; i < n; ++i)
    if (off[i] < 0 || off[i] % 16 || off[i + 1] - off[i] < (long long)sizeof(aloam_graph_record_header) || (off[i + 1] - off[i]) % kRecAlign) {
      c->err = "record " + std::to_string(i) + ": offsets must rise by whole records (multiples of " + std::to_string(kRecAlign) + " bytes)";
      return ALOAM_E_ARG;
    }
  const char* base = static_cast<const char*>(d_src);
  if (!base) {                                              // pageable host memory: staged into device memory (the span of the n records)
    const size_t span = (size_t)(off[n] - off[0]);
    if (const int rc = c->gr.stage.grow(c, (long long)span)) return rc;
    HIP_TRY(c, hipMemcpyAsync(c->gr.stage.get(), static_cast<const char*>(src) + off[0], span, hipMemcpyHostToDevice, c->stream));
    base = c->gr.stage.get() - off[0];
  }
  GraphRecCheckArgs k{};
  k.n = n; k.src = base; k.off = reinterpret_cast<const long long*>(c->gr.d_h + st.off);
  k.headers = reinterpret_cast<aloam_graph_record_header*>(c->gr.d_h + st.hdr); k.verdicts = reinterpret_cast<int*>(c->gr.d_h + st.verdict);
  { ProfScope p(c, K_LOAD); launch_graph_check(k, c->stream); }
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipStreamSynchronize(c->stream));              // the one host wait: headers and verdicts are in pinned memory
  const aloam_graph_record_header* hdr = reinterpret_cast<const aloam_graph_record_header*>(h + st.hdr);
  const int* verdict = reinterpret_cast<const int*>(h + st.verdict);
  for (int i = 0; i < n; ++i)
    if (const int rc = check_record(c, i, hdr[i], off[i + 1] - off[i], verdict[i])) return rc;
  // Everything is checked: from here on the load changes the context.
  long long* u_off = reinterpret_cast<long long*>(h + st.u_off);
  GraphRecItem* u_items = reinterpret_cast<GraphRecItem*>(h + st.u_items);
  int* u_chunk = reinterpret_cast<int*>(h + st.u_chunk);
  int chunks = 0;
  for (int i = 0; i < n; ++i) {
    u_off[i] = off[i];
    u_chunk[i] = chunks;
    chunks += (int)((hdr[i].bytes / 16 + kExportChunk - 1) / kExportChunk);
    u_items[i] = GraphRecItem{slots[i], hdr[i].nodes, hdr[i].edges, hdr[i].kf_points[0], hdr[i].kf_points[1], 0, 0, 0};
  }
  u_off[n] = off[n]; u_chunk[n] = chunks;
  HIP_TRY(c, hipMemcpyAsync(c->gr.staged.get(), h + st.u_off, st.bytes - st.u_off, hipMemcpyHostToDevice, c->stream));
  GraphRecLoadArgs a{};
  a.n = n; a.src = base;
  a.off = reinterpret_cast<const long long*>(c->gr.staged.get());
  a.items = reinterpret_cast<const GraphRecItem*>(c->gr.staged.get() + (st.u_items - st.u_off));
  a.chunk_off = reinterpret_cast<const int*>(c->gr.staged.get() + (st.u_chunk - st.u_off));
  a.store = rec_store(c);
  { ProfScope p(c, K_LOAD); launch_graph_load(a, c->gather_blocks, c->stream); }
  HIP_TRY(c, hipGetLastError());
  for (int i = 0; i < n; ++i) on_graph_loaded(c, slots[i], hdr[i].nodes, hdr[i].edges);
  return ALOAM_OK;
}

}  // extern "C"
