// a-loam_amd/csrc/relocalize_kernels.hpp — layouts and launchers of the map-pose hypothesis scoring (aloam_score_map_corrections,
// aloam_apply_map_corrections): what a frozen mapping step's first association would count from K candidate map <- odometry corrections.
#pragma once
#include "../../include/aloam_mi355x.h"
#include "mapping_kernels.hpp"

namespace aloam {

// Workgroups per (sequence, candidate): workgroup p takes the tiles of 256 stack points p, p + 8, ... of the corner stack, then of the surf
// stack.  A constant, not a launch parameter: the order in which a candidate's cost is summed then depends on the stacks alone, so the same
// candidate gets the same bits whatever n and K it is scored with.
constexpr int kScoreParts = 8;
constexpr int kScoreThreads = 256;
// (sequence, candidate) pairs of one call: 2^18 pairs are 2^21 workgroups and 64 MiB of partials, the largest launch the tests make; more
// is refused before anything is queued (a caller splits the candidates).
constexpr long long kScoreMaxPairs = 1ll << 18;

struct ScorePartial { int corner_factors, surf_factors, corner_found, surf_found; double cost; int pad[2]; };   // one per workgroup, in a fixed slot
static_assert(sizeof(ScorePartial) == 32 && sizeof(aloam_map_score) == 32 && sizeof(aloam_map_correction) == 64, "ABI sizes");

struct ScoreArgs {
  int B, cap, R;
  int n, K;                          // listed sequences, candidates
  int splits, kper;                  // candidate ranges per sequence (n < 8: a sequence's candidates are dealt over 8 / n XCDs), candidates per range
  const int* seqs;                   // [n]
  const aloam_map_correction* cand;  // [K]
  const MapSeq* seq;                 // [B]
  const float4* stack[2];            // [B][R*kLessSharpPerRing] / [B][cap]
  const float4* grid_sorted[2];      // [B][pool_cap]
  const int* grid_start[2];          // [B][H + 1]
  int grid_H, pool_cap;
  ScorePartial* part;                // [n][K][kScoreParts]
  aloam_map_score* scores;           // [n][K]
  int* best;                         // [n] or nullptr
};

struct ApplyArgs {
  int n, K;
  const int* seqs;                   // [n]
  const aloam_map_correction* cand;  // [K]
  const int* choice;                 // [n]
  MapSeq* seq;                       // [B]
  int* bad_choice;                   // counter of choices outside 0 .. K-1
};

void launch_score_corrections(const ScoreArgs& a, hipStream_t s);
void launch_apply_corrections(const ApplyArgs& a, hipStream_t s);

}  // namespace aloam
