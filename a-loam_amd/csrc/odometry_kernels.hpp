// a-loam_amd/csrc/odometry_kernels.hpp — host-callable launchers of the odometry kernels.
#pragma once
#include "aloam_device.hpp"

struct aloam_pose_information;

namespace aloam {
size_t build_grids_lds_bytes(int H, int R);
int prepare_build_grids(int H_surf);
// Which clouds a build covers and how its workgroups are laid out: one per cloud of the last clouds (serial, in front of the association), or a
// fixed number placed once that walk through the clouds (beside other kernels): of the sweep just registered, or of the last clouds.
enum class GridBuild { kSerialLast, kPersistentNext, kPersistentLast };
void launch_build_grids(const OdomArgs& a, GridBuild form, int wgs, hipStream_t s);   // wgs: workgroups of a persistent form
void launch_transform_queries(const OdomArgs& a, hipStream_t s);
void launch_associate(const OdomArgs& a, bool plane, hipStream_t s);
int prepare_solve();
void solve_launch_lds(const OdomArgs& a, int out[3]);
void launch_solve(const OdomArgs& a, hipStream_t s);
void launch_advance(const OdomArgs& a, hipStream_t s);             // the swap of every active sequence (a.active bit kSeqActive)
// list[n]: sequence | kInfoSolvedBit (information_device.hpp); dst[n] as the device reaches it
void launch_pose_information_odom(const OdomArgs& a, const int* list, int n, aloam_pose_information* dst, hipStream_t s);
void launch_set_inited(OdomState* state, int B, int inited, hipStream_t s);
}  // namespace aloam
