// a-loam_amd/csrc/capi_graphjoint.hip — host side of the joined pose graphs (aloam_graph_optimize_joint, aloam_graph_optimize_joint_robust,
// aloam_graph_joint_export).  Every argument is checked before anything is queued.  The host knows the counts and the links,
// so it computes the offsets of the joined rows and every member's tree link; the resolved groups, members, links (as joined edges) and the
// solve's items go through one pinned staging ring in one copy; then three launches in stream order: k_joint_gather, the solve of
// aloam_graph_optimize / aloam_graph_optimize_robust on the joined rows as it is (items[g] = {g, nodes_g, edges_g}), k_joint_scatter.
// Nothing synchronises the host, except a call that outgrows the ring.  No SeqHost field changes: the counts stay.  Nothing is allocated
// before the first call.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "capi_internal.hpp"
#include "graphrobust_kernels.hpp"

static_assert(sizeof(aloam_graph_link) == 256 && sizeof(aloam_graph_joint_group) == 16, "the sizes include/aloam_mi355x.h states");
static_assert(sizeof(GraphSolveItem) == 16, "the staged parts stand back to back in 16-byte units");

namespace {

constexpr long long kMaxJoinedNodes = 1 << 20, kMaxJoinedEdges = 1 << 22;      // the limits of aloam_graph_enable

struct JointPlan {                     // a checked call: what is staged, and the sizes the rows are laid out for
  std::vector<GraphSolveItem> items;
  std::vector<JointGroup> groups;
  std::vector<JointMember> members;
  std::vector<aloam_graph_edge> links;
  int row_nodes = 1, row_edges = 1, most_edges = 0;
  long long nodes = 0, edges = 0;
  size_t bytes() const { return sizeof(GraphSolveItem) * items.size() + sizeof(JointGroup) * groups.size() + sizeof(JointMember) * members.size() + sizeof(aloam_graph_edge) * links.size(); }
};

int refuse(aloam_ctx* c, const std::string& what) { c->err = what; return ALOAM_E_ARG; }

// Everything the header lists, in its order; nothing is queued and nothing changes on a refusal.
int joint_plan(aloam_ctx* c, const int* members, const int* align, int n_members, const aloam_graph_link* links, int n_links,
               const aloam_graph_joint_group* groups, int n_groups, JointPlan* p) {
  if (n_groups < 0 || n_members < 0 || n_links < 0) return refuse(c, "n_members, n_links and n_groups must not be negative");
  if (n_groups == 0) {
    if (n_members != 0 || n_links != 0) return refuse(c, "groups: no group holds the listed members and links");
    return ALOAM_OK;
  }
  if (!groups) return refuse(c, "groups is NULL");
  if (n_members > 0 && !members) return refuse(c, "members is NULL");
  if (n_links > 0 && !links) return refuse(c, "links is NULL");
  if (const int rc = require_host_list(c, groups, "groups")) return rc;
  if (n_members > 0) if (const int rc = require_host_list(c, members, "members")) return rc;
  if (n_members > 0 && align) if (const int rc = require_host_list(c, align, "align")) return rc;
  if (n_links > 0) if (const int rc = require_host_list(c, links, "links")) return rc;
  if (n_members > c->B) return refuse(c, "members: more members than the context has sequences");
  std::vector<int> at(c->B, -1);                                               // sequence -> its index in members
  for (int m = 0; m < n_members; ++m) {
    if (members[m] < 0 || members[m] >= c->B) return refuse(c, "members[" + std::to_string(m) + "] is out of range");
    if (at[members[m]] >= 0) return refuse(c, "members[" + std::to_string(m) + "] repeats sequence " + std::to_string(members[m]));
    at[members[m]] = m;
  }
  p->items.resize(n_groups); p->groups.resize(n_groups); p->members.resize(n_members); p->links.resize(n_links);
  int next_member = 0, next_link = 0;
  for (int g = 0; g < n_groups; ++g) {
    const aloam_graph_joint_group& gr = groups[g];
    const std::string G = "groups[" + std::to_string(g) + "]";
    if (gr.member_count < 1) return refuse(c, G + ".member_count must be at least 1");
    if (gr.link_count < 0) return refuse(c, G + ".link_count must not be negative");
    if (gr.member_first != next_member || gr.member_count > n_members - next_member) return refuse(c, G + ".member_first / member_count: the groups must tile members contiguously and in order");
    if (gr.link_first != next_link || gr.link_count > n_links - next_link) return refuse(c, G + ".link_first / link_count: the groups must tile links contiguously and in order");
    next_member += gr.member_count; next_link += gr.link_count;
    long long nodes = 0, edges = 0;
    for (int m = gr.member_first; m < gr.member_first + gr.member_count; ++m) {
      const SeqHost& s = c->seq[members[m]];
      if (s.graph_nodes < 1) return refuse(c, "members[" + std::to_string(m) + "]: the graph of sequence " + std::to_string(members[m]) + " holds no node");
      if (align && align[m] && m == gr.member_first) return refuse(c, "align[" + std::to_string(m) + "]: the first member of a group defines its frame and cannot be aligned");
      JointMember& jm = p->members[m];
      jm = JointMember{};
      jm.seq = members[m]; jm.nodes = s.graph_nodes; jm.edges = s.graph_edges; jm.group = g;
      jm.node_off = (int)nodes; jm.edge_off = (int)edges; jm.align = align && align[m] ? 1 : 0; jm.tree_link = -1;
      nodes += s.graph_nodes; edges += s.graph_edges;
      if (nodes > kMaxJoinedNodes) return refuse(c, G + ": the members hold more than 2^20 nodes together");
      if (edges + gr.link_count > kMaxJoinedEdges) return refuse(c, G + ": the members' edges and the links are more than 2^22 together");
    }
    for (int l = gr.link_first; l < gr.link_first + gr.link_count; ++l) {
      const aloam_graph_link& k = links[l];
      const std::string L = "links[" + std::to_string(l) + "]";
      const int mi = k.seq_i >= 0 && k.seq_i < c->B ? at[k.seq_i] : -1, mj = k.seq_j >= 0 && k.seq_j < c->B ? at[k.seq_j] : -1;
      if (mi < gr.member_first || mi >= gr.member_first + gr.member_count) return refuse(c, L + ".seq_i is no member of the link's group");
      if (mj < gr.member_first || mj >= gr.member_first + gr.member_count) return refuse(c, L + ".seq_j is no member of the link's group");
      if (mi == mj) return refuse(c, L + ": seq_i and seq_j must differ");
      if (k.i < 0 || k.i >= p->members[mi].nodes) return refuse(c, L + ".i lies outside the nodes of sequence " + std::to_string(k.seq_i));
      if (k.j < 0 || k.j >= p->members[mj].nodes) return refuse(c, L + ".j lies outside the nodes of sequence " + std::to_string(k.seq_j));
      // the measurement rules of aloam_graph_add_edges, on the link as an anchor of node j of seq_j (its index rule holds by the line above)
      aloam_graph_edge e{};
      e.seq = k.seq_j; e.i = -1; e.j = k.j; e.flags = k.flags;
      std::copy(k.q, k.q + 4, e.q); std::copy(k.t, k.t + 3, e.t); std::copy(k.info, k.info + 21, e.info);
      if (const char* what = graph_edge_check(c, e, true)) return refuse(c, L + ": " + what);
      e.seq = k.seq_i; e.i = p->members[mi].node_off + k.i; e.j = p->members[mj].node_off + k.j;   // the joined edge (q is normalised now)
      p->links[l] = e;
      JointMember& later = p->members[std::max(mi, mj)];
      if (later.tree_link < 0) {                                               // the first link that joins this member to an earlier one
        later.tree_link = l;
        later.tree_inverse = mi > mj ? 1 : 0;
        later.tree_other = mi > mj ? e.j : e.i;
        later.tree_own = mi > mj ? k.i : k.j;
      }
    }
    for (int m = gr.member_first + 1; m < gr.member_first + gr.member_count; ++m)
      if (p->members[m].tree_link < 0) return refuse(c, "members[" + std::to_string(m) + "]: no link joins sequence " + std::to_string(members[m]) + " to an earlier member of its group");
    edges += gr.link_count;
    p->groups[g] = JointGroup{gr.member_first, gr.member_count, gr.link_first, gr.link_count, (int)nodes, (int)edges, nodes >= 2 && edges >= 1 ? 1 : 0, 0};
    p->items[g] = GraphSolveItem{g, (int)nodes, (int)edges, 0};
    p->row_nodes = std::max(p->row_nodes, (int)nodes); p->row_edges = std::max(p->row_edges, (int)edges); p->most_edges = std::max(p->most_edges, (int)edges);
    p->nodes += nodes; p->edges += edges;
  }
  if (next_member != n_members) return refuse(c, "groups: the groups must tile members to its end");
  if (next_link != n_links) return refuse(c, "groups: the groups must tile links to its end");
  return ALOAM_OK;
}

int check_options(aloam_ctx* c, const aloam_graph_options* opt, aloam_graph_options* o) {
  aloam_graph_default_options(o);
  if (opt) *o = *opt;
  auto tol_ok = [](double v) { return std::isfinite(v) && v >= 0.0; };
  if (o->max_iterations < 0 || o->pcg_max_iterations < 1 || !tol_ok(o->function_tolerance) || !tol_ok(o->gradient_tolerance) || !tol_ok(o->pcg_tolerance) ||
      !(o->huber_delta > 0.0) || !std::isfinite(o->huber_delta)) {
    c->err = "bad options (max_iterations >= 0, pcg_max_iterations >= 1, tolerances finite and >= 0, huber_delta > 0)";
    return ALOAM_E_ARG;
  }
  return ALOAM_OK;
}

// The ring, the device copy of a slot and the joined rows, grown to what this call needs.  A larger ring replaces the old one only when the
// stream has drained (the old slots may still be read by a copy).
int joint_buffers(aloam_ctx* c, const JointPlan& p) {
  JointScratch& j = c->jt;
  const size_t need = (p.bytes() + 15) / 16 * 16;
  if (need > j.slot_bytes) {
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    const size_t grown = std::max(need, 2 * j.slot_bytes);
    j.ring = StageRing<kJointStageSlots>();
    j.slot_bytes = 0;
    if (const char* what = j.ring.create(grown)) { c->err = std::string("joined graphs: ") + what; return ALOAM_E_HIP; }
    j.slot_bytes = grown;
  }
  if (const int rc = j.staged.grow(c, (long long)j.slot_bytes)) return rc;
  const long long n = (long long)p.groups.size();
  if (j.nodes.cap < n * p.row_nodes || j.edges.cap < n * p.row_edges) j.last.clear();   // the rows are released: nothing is left to export
  if (const int rc = j.nodes.grow(c, n * p.row_nodes)) return rc;
  if (const int rc = j.edges.grow(c, n * p.row_edges)) return rc;
  return ALOAM_OK;
}

// The staged copy of the plan and the arguments of the two kernels.
int joint_stage(aloam_ctx* c, const JointPlan& p, GraphJointArgs* a, const GraphSolveItem** d_items) {
  JointScratch& j = c->jt;
  char* slot_mem = nullptr;
  int slot = 0;
  if (const int rc = j.ring.acquire(c, &slot_mem, &slot)) return rc;
  const size_t o_groups = sizeof(GraphSolveItem) * p.items.size(), o_members = o_groups + sizeof(JointGroup) * p.groups.size(),
               o_links = o_members + sizeof(JointMember) * p.members.size();
  std::memcpy(slot_mem, p.items.data(), o_groups);
  std::memcpy(slot_mem + o_groups, p.groups.data(), o_members - o_groups);
  std::memcpy(slot_mem + o_members, p.members.data(), o_links - o_members);
  if (!p.links.empty()) std::memcpy(slot_mem + o_links, p.links.data(), sizeof(aloam_graph_edge) * p.links.size());
  char* d = j.staged.get();
  if (const int rc = j.ring.queue(c, slot, slot_mem, p.bytes(), d, c->stream)) return rc;
  *d_items = reinterpret_cast<const GraphSolveItem*>(d);
  *a = GraphJointArgs{};
  a->n_groups = (int)p.groups.size(); a->n_members = (int)p.members.size();
  a->groups = reinterpret_cast<const JointGroup*>(d + o_groups);
  a->members = reinterpret_cast<const JointMember*>(d + o_members);
  a->links = reinterpret_cast<const aloam_graph_edge*>(d + o_links);
  a->nodes = c->pg.nodes.get(); a->edges = c->pg.edges.get(); a->max_nodes = c->pg.max_nodes; a->max_edges = c->pg.max_edges;
  a->joined_nodes = j.nodes.get(); a->joined_edges = j.edges.get(); a->row_nodes = p.row_nodes; a->row_edges = p.row_edges;
  j.row_nodes = p.row_nodes; j.row_edges = p.row_edges;
  j.last = p.groups;
  return ALOAM_OK;
}

// The solve's arguments on the joined rows: group g is "sequence" g of rows with the joined strides.
GraphSolveArgs joint_solve_args(aloam_ctx* c, const JointPlan& p, const GraphSolveItem* d_items, const aloam_graph_options& o, long long f64_row, long long i32_row) {
  GraphSolveArgs s{};
  s.n = (int)p.groups.size(); s.items = d_items; s.nodes = c->jt.nodes.get(); s.edges = c->jt.edges.get();
  s.max_nodes = p.row_nodes; s.max_edges = p.row_edges; s.row_nodes = p.row_nodes; s.row_edges = p.row_edges; s.opt = o;
  s.f64 = c->pg.f64.get(); s.f64_row = f64_row; s.i32 = c->pg.i32.get(); s.i32_row = i32_row;
  return s;
}

}  // namespace

extern "C" {

int aloam_graph_optimize_joint(aloam_ctx* c, const int* members, const int* align, int n_members, const aloam_graph_link* links, int n_links,
                               const aloam_graph_joint_group* groups, int n_groups, const aloam_graph_options* opt, aloam_graph_result* dst) {
  DeviceScope device_scope(c);
  if (!c) return ALOAM_E_ARG;
  if (const int rc = require_graph(c)) return rc;
  // ---- everything is checked before anything is queued
  JointPlan p;
  if (const int rc = joint_plan(c, members, align, n_members, links, n_links, groups, n_groups, &p)) return rc;
  aloam_graph_options o;
  if (const int rc = check_options(c, opt, &o)) return rc;
  void* d = nullptr;
  if (n_groups > 0) if (const int rc = export_target(c, dst, alignof(aloam_graph_result), "dst", &d)) return rc;
  if (n_groups == 0) return ALOAM_OK;
  const long long f64_row = graph_f64_row(p.row_nodes, p.row_edges), i32_row = graph_i32_row(p.row_nodes, p.row_edges);
  if (const int rc = c->pg.f64.grow(c, f64_row * n_groups)) return rc;
  if (const int rc = c->pg.i32.grow(c, i32_row * n_groups)) return rc;
  if (const int rc = joint_buffers(c, p)) return rc;
  GraphJointArgs a;
  const GraphSolveItem* d_items = nullptr;
  if (const int rc = joint_stage(c, p, &a, &d_items)) return rc;
  GraphSolveArgs s = joint_solve_args(c, p, d_items, o, f64_row, i32_row);
  s.dst = static_cast<aloam_graph_result*>(d);
  {
    ProfScope prof(c, K_POSE_GRAPH);
    launch_joint_gather(a, c->stream);
    launch_pose_graph(s, c->stream);
    launch_joint_scatter(a, c->stream);
  }
  HIP_TRY(c, hipGetLastError());
  c->pg.last_nodes = p.nodes; c->pg.last_edges = p.edges; c->pg.last_trim_bytes = -1;
  return ALOAM_OK;
}

int aloam_graph_optimize_joint_robust(aloam_ctx* c, const int* members, const int* align, int n_members, const aloam_graph_link* links, int n_links,
                                      const aloam_graph_joint_group* groups, int n_groups, const aloam_graph_options* opt,
                                      const aloam_graph_robust_options* robust, aloam_graph_robust_result* dst, double* weights_dst, long long weights_stride) {
  DeviceScope device_scope(c);
  if (!c) return ALOAM_E_ARG;
  if (const int rc = require_graph(c)) return rc;
  // ---- everything is checked before anything is queued
  JointPlan p;
  if (const int rc = joint_plan(c, members, align, n_members, links, n_links, groups, n_groups, &p)) return rc;
  aloam_graph_options o;
  if (const int rc = check_options(c, opt, &o)) return rc;
  aloam_graph_robust_options r;
  aloam_graph_robust_default_options(&r);
  if (robust) r = *robust;
  if (r.max_outer_iterations < 1 || !(r.inlier_chi2 > 0.0) || !std::isfinite(r.inlier_chi2) || !(r.mu_step > 1.0) || !std::isfinite(r.mu_step)) {
    c->err = "bad robust options (max_outer_iterations >= 1, inlier_chi2 > 0 and finite, mu_step > 1 and finite)";
    return ALOAM_E_ARG;
  }
  r.pad = 0; r.reserved = 0.0;
  void* d = nullptr;
  void* d_w = nullptr;
  if (n_groups > 0) if (const int rc = export_target(c, dst, alignof(aloam_graph_robust_result), "dst", &d)) return rc;
  if (n_groups > 0 && weights_dst) {
    if (const int rc = export_target(c, weights_dst, alignof(double), "weights_dst", &d_w)) return rc;
    if (weights_stride < p.most_edges) { c->err = "weights_stride is below the largest joined edge count (" + std::to_string(p.most_edges) + ")"; return ALOAM_E_ARG; }
  }
  if (n_groups == 0) return ALOAM_OK;
  const long long f64_row = graph_robust_f64_row(p.row_nodes, p.row_edges), i32_row = graph_i32_row(p.row_nodes, p.row_edges);
  if (const int rc = c->pg.f64.grow(c, f64_row * n_groups)) return rc;
  if (const int rc = c->pg.i32.grow(c, i32_row * n_groups)) return rc;
  if (const int rc = joint_buffers(c, p)) return rc;
  GraphJointArgs a;
  const GraphSolveItem* d_items = nullptr;
  if (const int rc = joint_stage(c, p, &a, &d_items)) return rc;
  GraphRobustArgs s{};
  s.g = joint_solve_args(c, p, d_items, o, f64_row, i32_row);
  s.g.dst = nullptr;
  s.robust = r;
  s.dst = static_cast<aloam_graph_robust_result*>(d);
  s.weights = static_cast<double*>(d_w); s.weights_stride = weights_stride;
  {
    ProfScope prof(c, K_POSE_GRAPH);
    launch_joint_gather(a, c->stream);
    launch_graph_robust(s, c->stream);
    launch_joint_scatter(a, c->stream);
  }
  HIP_TRY(c, hipGetLastError());
  c->pg.last_nodes = p.nodes; c->pg.last_edges = p.edges; c->pg.last_trim_bytes = -1;
  return ALOAM_OK;
}

int aloam_graph_joint_export(aloam_ctx* c, int group, aloam_graph_node* nodes_dst, long long cap_nodes, aloam_graph_edge* edges_dst, long long cap_edges, int counts[4]) {
  DeviceScope device_scope(c);
  if (!c || !counts) return ALOAM_E_ARG;
  if (const int rc = require_graph(c)) return rc;
  const JointScratch& j = c->jt;
  if (j.last.empty()) { c->err = "no joint solve has run (aloam_graph_optimize_joint), or its rows have been released"; return ALOAM_E_STATE; }
  if (group < 0 || group >= (int)j.last.size()) { c->err = "group is out of range of the last joint call (" + std::to_string(j.last.size()) + " groups)"; return ALOAM_E_ARG; }
  if (cap_nodes < 0 || cap_edges < 0) { c->err = "cap_nodes and cap_edges must not be negative"; return ALOAM_E_ARG; }
  const JointGroup& g = j.last[group];
  counts[0] = g.nodes; counts[1] = g.edges; counts[2] = g.edges - g.link_count; counts[3] = g.link_count;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (nodes_dst && g.nodes > 0 && g.nodes <= cap_nodes)
    HIP_TRY(c, hipMemcpy(nodes_dst, j.nodes.get() + (size_t)group * j.row_nodes, sizeof(aloam_graph_node) * (size_t)g.nodes, hipMemcpyDeviceToHost));
  if (edges_dst && g.edges > 0 && g.edges <= cap_edges)
    HIP_TRY(c, hipMemcpy(edges_dst, j.edges.get() + (size_t)group * j.row_edges, sizeof(aloam_graph_edge) * (size_t)g.edges, hipMemcpyDeviceToHost));
  return ALOAM_OK;
}

}  // extern "C"
