// a-loam_amd/csrc/graphjoint_kernels.hip — gfx950 kernels of the joined pose graphs (aloam_graph_optimize_joint).  A translation
// unit of its own, so that every other kernel is compiled exactly as before; the solve between the two kernels is launch_pose_graph /
// launch_graph_robust on the joined rows.  Poses are composed with the device functions k_graph_trim composes with (quat_mul, quat_rotate,
// through map_search_device.hpp), every f64 operation rounded on its own.
//   k_joint_gather    one workgroup of kGraphThreads per group.  It walks the group's members in order: a thread per node copies the
//                     member's 128-byte records to the joined row at node_off, a thread per edge its 240-byte records to edge_off with
//                     i >= 0 and j shifted by node_off; then a thread per link copies the staged links behind the members' edges.  A
//                     member with align set is first given A = Xg o Z o X[own]^-1 from its tree link (Z inverted when the member is the
//                     link's seq_i side), q_A divided by its norm; its estimates become A o X_opt and its anchors A o Z.  Xg is read from the joined row, where an
//                     earlier iteration placed it: between two members every wave waits for its stores (s_waitcnt vmcnt(0)) and the
//                     workgroup passes a barrier.  The wait is written out, as in graphtrim_kernels.hip: for this kernel hipcc emits
//                     a bare s_barrier for __syncthreads() (read in the ISA), no wait for outstanding vector memory operations in
//                     front of it, so without the wait the order of an earlier wave's stores and a later wave's load of Xg would rest
//                     on the CU's L1 handling them in issue order alone.  The load itself is a plain load: the waves of a workgroup
//                     share one L1, and a joined node is written once per launch and read only afterwards, so no stale line exists.
//   k_joint_scatter   one workgroup per member, behind the solve.  The member's node records come back from the joined row as bit copies
//                     (q, t and frame are the bytes they were); an aligned member's anchors get their Z' back.  It reads the joined rows
//                     and writes the sequences' rows: nothing it reads is written in the launch.
// Records move as 16-byte units held in registers, every lane loading at a clamped index so that no load stands under a condition, loads
// ahead of stores.  No floating-point atomic, no communication between workgroups, no spinning; every store is a vector store.
#include "graphjoint_kernels.hpp"

#include "map_search_device.hpp"             // quat_mul, quat_rotate only

namespace aloam {

namespace {

constexpr int kEdgeUnits = sizeof(aloam_graph_edge) / 16, kNodeUnits = sizeof(aloam_graph_node) / 16;
static_assert(sizeof(aloam_graph_edge) == 240 && sizeof(aloam_graph_node) == 128, "records are moved as 16-byte units");
static_assert(offsetof(aloam_graph_node, q_opt) == 56 && offsetof(aloam_graph_node, t_opt) == 88, "q_opt: unit 3 high .. unit 5 low; t_opt: unit 5 high, unit 6");
static_assert(offsetof(aloam_graph_edge, i) == 4 && offsetof(aloam_graph_edge, j) == 8 && offsetof(aloam_graph_edge, q) == 16 && offsetof(aloam_graph_edge, t) == 48,
              "i, j: unit 0; q: units 1, 2; t: unit 3, unit 4 low");
typedef unsigned int unit_t __attribute__((ext_vector_type(4)));   // a 16-byte unit of a record, moved as bits

// Every vector memory operation this wave has issued has completed, stores included.  In front of the barrier: then every one of the workgroup has.
__device__ __forceinline__ void memory_complete() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

__device__ __forceinline__ double unit_lo(const unit_t& u) { return __hiloint2double((int)u.y, (int)u.x); }
__device__ __forceinline__ double unit_hi(const unit_t& u) { return __hiloint2double((int)u.w, (int)u.z); }
__device__ __forceinline__ void set_lo(unit_t& u, double v) { u.x = (unsigned)__double2loint(v); u.y = (unsigned)__double2hiint(v); }
__device__ __forceinline__ void set_hi(unit_t& u, double v) { u.z = (unsigned)__double2loint(v); u.w = (unsigned)__double2hiint(v); }

struct Pose { double q[4], t[3]; };

// compose(Xa, Xb) = (q_a q_b, q_a t_b + t_a) and inverse(X) = (q*, -(q* t)), as posegraph.compose and posegraph.inverse.
__device__ __forceinline__ Pose pose_compose(const Pose& a, const Pose& b) {
  Pose o;
  quat_mul(a.q, b.q, o.q);
  quat_rotate(a.q, b.t[0], b.t[1], b.t[2], o.t);
  o.t[0] = o.t[0] + a.t[0]; o.t[1] = o.t[1] + a.t[1]; o.t[2] = o.t[2] + a.t[2];
  return o;
}
__device__ __forceinline__ Pose pose_inverse(const Pose& a) {
  Pose o;
  o.q[0] = -a.q[0]; o.q[1] = -a.q[1]; o.q[2] = -a.q[2]; o.q[3] = a.q[3];
  quat_rotate(o.q, a.t[0], a.t[1], a.t[2], o.t);
  o.t[0] = -o.t[0]; o.t[1] = -o.t[1]; o.t[2] = -o.t[2];
  return o;
}

}  // namespace

__global__ __launch_bounds__(kGraphThreads) void k_joint_gather(GraphJointArgs a) {
  const int tid = threadIdx.x;
  const JointGroup g = a.groups[blockIdx.x];
  aloam_graph_node* JN = a.joined_nodes + (long long)blockIdx.x * a.row_nodes;
  aloam_graph_edge* JE = a.joined_edges + (long long)blockIdx.x * a.row_edges;
  for (int m = 0; m < g.member_count; ++m) {
    const JointMember mb = a.members[g.member_first + m];
    const aloam_graph_node* N = a.nodes + (long long)mb.seq * a.max_nodes;
    const aloam_graph_edge* E = a.edges + (long long)mb.seq * a.max_edges;
    Pose A = {};
    if (mb.align) {                                                            // (uniform) A = Xg o Z o X[own]^-1, Z inverted for the seq_i side
      const aloam_graph_node* o = JN + mb.tree_other;                          // placed by an earlier member, behind the barrier below
      const aloam_graph_edge& l = a.links[mb.tree_link];
      const aloam_graph_node& x = N[mb.tree_own];
      Pose Xg, Z, X;
#pragma unroll
      for (int c = 0; c < 4; ++c) { Xg.q[c] = o->q_opt[c]; Z.q[c] = l.q[c]; X.q[c] = x.q_opt[c]; }
#pragma unroll
      for (int c = 0; c < 3; ++c) { Xg.t[c] = o->t_opt[c]; Z.t[c] = l.t[c]; X.t[c] = x.t_opt[c]; }
      if (mb.tree_inverse) Z = pose_inverse(Z);
      A = pose_compose(pose_compose(Xg, Z), pose_inverse(X));
      // q_A divided by its norm, the squares summed in index order: the estimates it is built from are chained products that are not
      // renormalised (5e-13 off after 70 nodes), and a q_A off unit norm would scale the whole member
      double nn = 0.0;
#pragma unroll
      for (int c = 0; c < 4; ++c) nn = nn + A.q[c] * A.q[c];
      nn = sqrt(nn);
#pragma unroll
      for (int c = 0; c < 4; ++c) A.q[c] = A.q[c] / nn;
    }
    // ---- the node row: a record per thread
    for (int base = 0; base < mb.nodes; base += kGraphThreads) {
      const int n = base + tid;
      unit_t r[kNodeUnits];
      {
        const unit_t* src = reinterpret_cast<const unit_t*>(N + (n < mb.nodes ? n : mb.nodes - 1));   // every lane loads, clamped
#pragma unroll
        for (int k = 0; k < kNodeUnits; ++k) r[k] = src[k];
      }
      if (mb.align) {                                                          // (uniform) X_opt' = A o X_opt
        Pose X;
        X.q[0] = unit_hi(r[3]); X.q[1] = unit_lo(r[4]); X.q[2] = unit_hi(r[4]); X.q[3] = unit_lo(r[5]);
        X.t[0] = unit_hi(r[5]); X.t[1] = unit_lo(r[6]); X.t[2] = unit_hi(r[6]);
        const Pose Y = pose_compose(A, X);
        set_hi(r[3], Y.q[0]); set_lo(r[4], Y.q[1]); set_hi(r[4], Y.q[2]); set_lo(r[5], Y.q[3]);
        set_hi(r[5], Y.t[0]); set_lo(r[6], Y.t[1]); set_hi(r[6], Y.t[2]);
      }
      if (n < mb.nodes) {
        unit_t* dst = reinterpret_cast<unit_t*>(JN + mb.node_off + n);
#pragma unroll
        for (int k = 0; k < kNodeUnits; ++k) dst[k] = r[k];
      }
    }
    // ---- the edge row: a record per thread, i >= 0 and j shifted, an aligned member's anchors composed
    for (int base = 0; base < mb.edges; base += kGraphThreads) {
      const int e = base + tid;
      unit_t r[kEdgeUnits];
      {
        const unit_t* src = reinterpret_cast<const unit_t*>(E + (e < mb.edges ? e : mb.edges - 1));   // every lane loads, clamped
#pragma unroll
        for (int k = 0; k < kEdgeUnits; ++k) r[k] = src[k];
      }
      const int i = (int)r[0].y;
      if (mb.align && i < 0) {                                                 // Z' = A o Z, stored as computed
        Pose Z;
        Z.q[0] = unit_lo(r[1]); Z.q[1] = unit_hi(r[1]); Z.q[2] = unit_lo(r[2]); Z.q[3] = unit_hi(r[2]);
        Z.t[0] = unit_lo(r[3]); Z.t[1] = unit_hi(r[3]); Z.t[2] = unit_lo(r[4]);
        const Pose Y = pose_compose(A, Z);
        set_lo(r[1], Y.q[0]); set_hi(r[1], Y.q[1]); set_lo(r[2], Y.q[2]); set_hi(r[2], Y.q[3]);
        set_lo(r[3], Y.t[0]); set_hi(r[3], Y.t[1]); set_lo(r[4], Y.t[2]);
      }
      r[0].y = (unsigned)(i < 0 ? i : i + mb.node_off);
      r[0].z = (unsigned)((int)r[0].z + mb.node_off);
      if (e < mb.edges) {
        unit_t* dst = reinterpret_cast<unit_t*>(JE + mb.edge_off + e);
#pragma unroll
        for (int k = 0; k < kEdgeUnits; ++k) dst[k] = r[k];
      }
    }
    memory_complete();
    __syncthreads();                                                           // this member's estimates are placed: a later member's tree link may read one
  }
  // ---- the links, staged by the host as joined edges, behind the members' edges
  const int first_link = g.edges - g.link_count;
  for (int base = 0; base < g.link_count; base += kGraphThreads) {
    const int l = base + tid;
    unit_t r[kEdgeUnits];
    {
      const unit_t* src = reinterpret_cast<const unit_t*>(a.links + g.link_first + (l < g.link_count ? l : g.link_count - 1));
#pragma unroll
      for (int k = 0; k < kEdgeUnits; ++k) r[k] = src[k];
    }
    if (l < g.link_count) {
      unit_t* dst = reinterpret_cast<unit_t*>(JE + first_link + l);
#pragma unroll
      for (int k = 0; k < kEdgeUnits; ++k) dst[k] = r[k];
    }
  }
}

__global__ __launch_bounds__(kGraphThreads) void k_joint_scatter(GraphJointArgs a) {
  const int tid = threadIdx.x;
  const JointMember mb = a.members[blockIdx.x];
  const JointGroup g = a.groups[mb.group];
  if (!g.solved) return;                                                       // (uniform) ALOAM_GRAPH_NO_EDGES: nothing is written back
  const aloam_graph_node* JN = a.joined_nodes + (long long)mb.group * a.row_nodes + mb.node_off;
  const aloam_graph_edge* JE = a.joined_edges + (long long)mb.group * a.row_edges + mb.edge_off;
  aloam_graph_node* N = a.nodes + (long long)mb.seq * a.max_nodes;
  aloam_graph_edge* E = a.edges + (long long)mb.seq * a.max_edges;
  for (int base = 0; base < mb.nodes; base += kGraphThreads) {
    const int n = base + tid;
    unit_t r[kNodeUnits];
    {
      const unit_t* src = reinterpret_cast<const unit_t*>(JN + (n < mb.nodes ? n : mb.nodes - 1));   // every lane loads, clamped
#pragma unroll
      for (int k = 0; k < kNodeUnits; ++k) r[k] = src[k];
    }
    if (n < mb.nodes) {
      unit_t* dst = reinterpret_cast<unit_t*>(N + n);
#pragma unroll
      for (int k = 0; k < kNodeUnits; ++k) dst[k] = r[k];
    }
  }
  if (!mb.align) return;                                                       // (uniform) its edges are the bytes they were
  constexpr int kPoseUnits = 5;                                                // unit 0: seq, i, j, flags; units 1 .. 4: q, t and info[0]
  for (int base = 0; base < mb.edges; base += kGraphThreads) {
    const int e = base + tid;
    unit_t r[kPoseUnits];
    {
      const unit_t* src = reinterpret_cast<const unit_t*>(JE + (e < mb.edges ? e : mb.edges - 1));   // every lane loads, clamped
#pragma unroll
      for (int k = 0; k < kPoseUnits; ++k) r[k] = src[k];
    }
    if (e < mb.edges && (int)r[0].y < 0) {                                     // an anchor: Z' comes back, info[0] beside t[2] as the bits it was
      unit_t* dst = reinterpret_cast<unit_t*>(E + e);
#pragma unroll
      for (int k = 1; k < kPoseUnits; ++k) dst[k] = r[k];
    }
  }
}

void launch_joint_gather(const GraphJointArgs& a, hipStream_t stream) {
  if (a.n_groups <= 0) return;
  hipLaunchKernelGGL(k_joint_gather, dim3(a.n_groups), dim3(kGraphThreads), 0, stream, a);
}

void launch_joint_scatter(const GraphJointArgs& a, hipStream_t stream) {
  if (a.n_members <= 0) return;
  hipLaunchKernelGGL(k_joint_scatter, dim3(a.n_members), dim3(kGraphThreads), 0, stream, a);
}

}  // namespace aloam
