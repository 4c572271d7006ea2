// Host-only driver of fp16_weight_scale (ramp_amd/csrc/weight_scale.h) for tests/test_host_cpu.py: every argument is the bit
// pattern of a float in hex; prints the bit pattern of its scale, one per line.
#include "weight_scale.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

int main(int argc, char** argv) {
  for (int i = 1; i < argc; ++i) {
    uint32_t u = (uint32_t)std::strtoul(argv[i], nullptr, 16);
    float x;
    std::memcpy(&x, &u, 4);
    const float s = ramp::fp16_weight_scale(x);
    std::memcpy(&u, &s, 4);
    std::printf("%08x\n", (unsigned)u);
  }
  return 0;
}
