// The static weight scale of the fp16x3 kernels, as a pure host function (no HIP: a host-only program can include this file).
#pragma once
#include <algorithm>
#include <cmath>

namespace ramp {
namespace {

// max |w| -> [2^10, 2^11): the power of two every fp16x3 weight is multiplied by before it is split into fp16 planes
// (ramp_finalize_weights and the ramp_op_* entry points; the kernels multiply the result by its inverse).  1 for an all-zero or
// non-finite weight.  Below 2^-117 the exact scale is no float: it saturates at 2^127 (the products then lie below 2^10).
inline float fp16_weight_scale(float max_abs) {
  if (!(max_abs > 0.f) || !std::isfinite(max_abs)) return 1.f;
  int e; std::frexp(max_abs, &e);                        // max_abs in [2^(e-1), 2^e)
  return std::ldexp(1.f, std::min(11 - e, 127));
}

}  // namespace
}  // namespace ramp
