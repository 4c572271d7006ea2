// Stand-alone driver of the pass planner of ramp_encode_scenes (ramp_amd/csrc/encode_plan.h), built by
// tests/test_scenes_encode_host.py with -fsanitize=address,undefined.
//   encode_plan_probe <max_points> <n_scenes> <scene_first ...> -- <obstacle_first ...>
// prints "refused: <reason>" or "ok <n_passes>" followed by one line per pass:
//   scene0 scene1 obstacle0 obstacle1 point0 point1 point_tiles obstacle_tiles
#include "encode_plan.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

int main(int argc, char** argv) {
  if (argc < 3) { std::fprintf(stderr, "usage: %s max_points n_scenes scene_first... -- obstacle_first...\n", argv[0]); return 2; }
  const int32_t max_points = (int32_t)std::atol(argv[1]), n_scenes = (int32_t)std::atol(argv[2]);
  std::vector<int32_t> scene_first, obstacle_first;
  bool second = false;
  for (int i = 3; i < argc; ++i) {
    if (!std::strcmp(argv[i], "--")) { second = true; continue; }
    (second ? obstacle_first : scene_first).push_back((int32_t)std::atol(argv[i]));
  }
  std::vector<ramp::EncodePass> passes;
  const std::string refusal = ramp::plan_encode_passes(scene_first.data(), obstacle_first.data(), n_scenes, max_points, &passes);
  if (!refusal.empty()) { std::printf("refused: %s\n", refusal.c_str()); return 0; }
  std::printf("ok %zu\n", passes.size());
  for (const ramp::EncodePass& p : passes)
    std::printf("%d %d %d %d %d %d %d %d\n", p.scene0, p.scene1, p.obstacle0, p.obstacle1, p.point0, p.point1, p.point_tiles, p.obstacle_tiles);
  return 0;
}
