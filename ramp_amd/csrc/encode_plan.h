// Pass planner of ramp_encode_scenes: a pure host function from the two CSR tables of a scene batch and the point budget to the passes
// of consecutive scenes the encoder runs, with the attention tile counts of each.  Nothing of HIP is included, so a stand-alone program
// can call it (tests/encode_plan_probe.cpp).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace ramp {

constexpr int32_t ENCODE_DEFAULT_MAX_POINTS = 32768;   // = RAMP_ENCODE_DEFAULT_MAX_POINTS (include/ramp_hip.h)
constexpr int32_t ENCODE_TILE = 64;                    // queries of one attention block, keys of one LDS tile

// scenes [scene0, scene1), their obstacles [obstacle0, obstacle1) and points [point0, point1) of the concatenated arrays
struct EncodePass {
  int32_t scene0 = 0, scene1 = 0, obstacle0 = 0, obstacle1 = 0, point0 = 0, point1 = 0;
  int32_t point_tiles = 0;       // sum over the pass's scenes of ceil(points / 64): the 2-D encoder's tokens are points
  int32_t obstacle_tiles = 0;    // sum of ceil(obstacles / 64): the 3-D encoder's tokens are obstacles
};

// Checks the tables and fills `passes`; returns "" or the reason of the refusal (the scene or obstacle named).
//   scene_first[n_scenes + 1]                 first obstacle of each scene
//   obstacle_first[scene_first[n_scenes] + 1] first point of each obstacle
//   max_points                                points per pass, 0 = ENCODE_DEFAULT_MAX_POINTS
// A pass holds as many whole consecutive scenes as fit in the budget and always at least one: a scene larger than the budget gets a
// pass of its own.  Refused: n_scenes < 1, a negative budget, tables that do not start at 0 or are not strictly increasing (an empty
// scene or obstacle; entries that wrapped past 31 bits show here too), a scene whose obstacles differ in point count.
inline std::string plan_encode_passes(const int32_t* scene_first, const int32_t* obstacle_first, int32_t n_scenes, int32_t max_points,
                                      std::vector<EncodePass>* passes) {
  passes->clear();
  if (n_scenes < 1) return "n_scenes must be at least 1";
  if (!scene_first || !obstacle_first) return "null table";
  if (max_points < 0) return "max_points must be >= 0 (0 = default)";
  const int64_t budget = max_points ? max_points : ENCODE_DEFAULT_MAX_POINTS;
  if (scene_first[0] != 0) return "scene_first must start at 0";
  if (obstacle_first[0] != 0) return "obstacle_first must start at 0";
  for (int32_t s = 0; s < n_scenes; ++s)
    if (scene_first[s + 1] <= scene_first[s]) return "scene " + std::to_string(s) + " has no obstacle (scene_first must be strictly increasing)";
  for (int32_t s = 0; s < n_scenes; ++s) {
    const int32_t np = obstacle_first[scene_first[s] + 1] - obstacle_first[scene_first[s]];
    for (int32_t o = scene_first[s]; o < scene_first[s + 1]; ++o) {
      const int32_t n = obstacle_first[o + 1] - obstacle_first[o];
      if (n <= 0) return "scene " + std::to_string(s) + ": obstacle " + std::to_string(o) + " has no point (obstacle_first must be strictly increasing)";
      if (n != np) return "scene " + std::to_string(s) + ": obstacle " + std::to_string(o) + " has " + std::to_string(n) + " points, the scene's first " + std::to_string(np);
    }
  }
  EncodePass cur;
  auto tiles = [](int32_t n) { return (n + ENCODE_TILE - 1) / ENCODE_TILE; };
  for (int32_t s = 0; s < n_scenes; ++s) {
    const int32_t o0 = scene_first[s], o1 = scene_first[s + 1];
    const int32_t p0 = obstacle_first[o0], p1 = obstacle_first[o1];
    if (cur.scene1 > cur.scene0 && (int64_t)(p1 - cur.point0) > budget) {
      passes->push_back(cur);
      cur = EncodePass();
    }
    if (cur.scene1 == cur.scene0) { cur.scene0 = s; cur.obstacle0 = o0; cur.point0 = p0; }
    cur.scene1 = s + 1; cur.obstacle1 = o1; cur.point1 = p1;
    cur.point_tiles += tiles(p1 - p0);
    cur.obstacle_tiles += tiles(o1 - o0);
  }
  passes->push_back(cur);
  return "";
}

}  // namespace ramp
