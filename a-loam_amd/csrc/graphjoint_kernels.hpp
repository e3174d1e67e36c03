// a-loam_amd/csrc/graphjoint_kernels.hpp — joined pose graphs (aloam_graph_optimize_joint): what capi_graphjoint.hip hands to
// graphjoint_kernels.hip.  The solve between the two kernels is launch_pose_graph / launch_graph_robust on the joined rows, as they are.
#pragma once
#include "posegraph_kernels.hpp"

namespace aloam {

constexpr int kJointStageSlots = 4;           // pinned ring of staged calls: calls in flight before the host waits for one

// A member of a group as the host resolved it: its counts (host state), where its rows start in the joined rows, and - for a member that is
// aligned - its tree link: the staged link `tree_link`, the joined index `tree_other` of the earlier member's node, the member's own node
// `tree_own`, and whether the member is the link's seq_i side (`tree_inverse`: Z is then inverted).
struct JointMember {
  int seq, nodes, edges, group;
  int node_off, edge_off, align, tree_link;
  int tree_other, tree_own, tree_inverse, pad;
};
// A group: its members and links in the call's lists, the joined counts (edges = the members' edges, then the links), and whether the
// solve runs at all (fewer than two nodes or no edge: ALOAM_GRAPH_NO_EDGES, nothing is written back).
struct JointGroup {
  int member_first, member_count, link_first, link_count;
  int nodes, edges, solved, pad;
};
static_assert(sizeof(JointMember) == 48 && sizeof(JointGroup) == 32, "staged back to back in 16-byte units");

struct GraphJointArgs {
  int n_groups, n_members;
  const JointGroup* groups;          // [n_groups]
  const JointMember* members;        // [n_members], the groups' members back to back
  const aloam_graph_edge* links;     // [n_links] the links as joined edges: (seq_i, off[seq_i] + i, off[seq_j] + j, flags), Z, info
  aloam_graph_node* nodes;           // [B][max_nodes] the sequences' rows
  aloam_graph_edge* edges;           // [B][max_edges]
  int max_nodes, max_edges;
  aloam_graph_node* joined_nodes;    // [n_groups][row_nodes]
  aloam_graph_edge* joined_edges;    // [n_groups][row_edges]
  int row_nodes, row_edges;
};
void launch_joint_gather(const GraphJointArgs& a, hipStream_t stream);    // one workgroup per group
void launch_joint_scatter(const GraphJointArgs& a, hipStream_t stream);   // one workgroup per member

}  // namespace aloam
