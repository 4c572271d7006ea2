// Launch arguments of the swept collision / clearance kernel (clearance.hip; ramp_obstacles and ramp_traj_clearance in ramp_hip.h).
#pragma once
#include "core.h"

namespace ramp {

struct ClearanceArgs {
  const float* traj = nullptr;        // (B,H,S); positions are channels [0, D)
  int B = 0, H = 0, S = 0, D = 2;     // D = point_dim, 2 or 3, <= S; 2 <= H <= 128
  const int* traj_first = nullptr;    // device (n_scenes + 1): first row of each scene
  int n_scenes = 1;
  const float* box_c = nullptr; const float* box_s = nullptr;      // (n_boxes, D) centres / sizes, scenes concatenated
  const float* sph_c = nullptr; const float* sph_r = nullptr;      // (n_spheres, D) centres, (n_spheres) radii
  const float* cloud = nullptr;                                    // (n_points, D)
  const int* box_off = nullptr; const int* sph_off = nullptr; const int* cloud_off = nullptr;   // device (n_scenes + 1) each; spans are clamped to the totals
  int n_boxes = 0, n_spheres = 0, n_points = 0;
  float margin = 0.f;
  int swept = 1;                      // 0: no segment work, seg_hits / clear_seg are not written
  int* wp_hits = nullptr; int* seg_hits = nullptr;                 // (B) each; any output may be null
  float* clear_wp = nullptr; float* clear_seg = nullptr; float* plen = nullptr; float* smooth = nullptr;
};
// one block per trajectory; the dims are the caller's to check (ramp_traj_clearance does)
int launch_traj_clearance(const ClearanceArgs& a, hipStream_t s);

// ---- robot-robot separation of teams (team.hip; ramp_team_clearance in ramp_hip.h) ----
struct TeamClearanceArgs {
  const float* traj = nullptr;        // (B,H,S); positions are channels [0, D); row b is agent b % team of team b / team
  int B = 0, H = 0, S = 0, D = 2;     // D = point_dim, 2 or 3, <= S; 2 <= H <= 128
  int team = 1;                       // 1 .. 8, B % team == 0
  float min_sep = 0.f;
  int swept = 1;                      // which count decides team_mask: 1 = seg_conflicts, 0 = wp_conflicts
  const int* row_mask = nullptr; const float* row_len = nullptr; const float* row_smooth = nullptr;   // (B) each, or null
  float* sep_wp = nullptr; float* sep_seg = nullptr; int* wp_conflicts = nullptr; int* seg_conflicts = nullptr;   // (B / team) each; any may be null
  int* team_mask = nullptr; float* team_len = nullptr; float* team_smooth = nullptr;                  // (B / team) each; any may be null
};
// one block per team, one launch; the dims are the caller's to check (ramp_team_clearance does)
int launch_team_clearance(const TeamClearanceArgs& a, hipStream_t s);

}  // namespace ramp
