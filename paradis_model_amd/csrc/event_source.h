// The value of an event source at one cell, as csrc/events.hip evaluates it (restated here for fss.hip; events.hip keeps
// its own copy, and tests/test_hip_fss.py pins the two kernels against each other).  Include after common.h, in a unit
// built with -ffp-contract=off.
//   plain    x = v[c0]
//   speed    x = sqrtf(v[c0] * v[c0] + v[c1] * v[c1])        (mul, mul, add, sqrt: uncontracted)
//   anomaly  x = v[c0] - clim[clim_index[b]][c0]
// A cell is valid iff every value it reads is finite.  The event is sign * x >= thr' (sign = +-1: the product is exact).
#pragma once
#include <cmath>

#pragma clang fp contract(off)

constexpr int EVSRC_PLAIN = 0, EVSRC_SPEED = 1, EVSRC_ANOMALY = 2;

// a: the value of channel c0, b: of channel c1 (speed only), cv: the climatology cell (anomaly only); returns whether the
// field's own values are finite (the climatology cell is the caller's to test, once for both fields) and sets sx = sign x
template <int KIND>
__device__ __forceinline__ bool event_source_value(float a, float b, float cv, float sign, float& sx) {
  bool ok = __builtin_isfinite(a);
  float x = a;
  if (KIND == EVSRC_SPEED) {
    ok = ok && __builtin_isfinite(b);
    x = sqrtf(a * a + b * b);
  }
  if (KIND == EVSRC_ANOMALY) x = a - cv;
  sx = sign * x;
  return ok;
}
