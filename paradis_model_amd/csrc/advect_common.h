// What the translation units of the semi-Lagrangian advection share: advect.hip (the C ABI, the workspace layout, the
// schedule choice, the pole-row and fixed-point prologue / epilogue kernels), advect_planes.hip (W == 64 planes and the
// generic kernels, whole-plane and tiled), advect_tilerow.hip (row-wave tiles) and advect_strips.hip (ring strips, the
// full-circle ring, their fix-ups).  The call's arguments, the constants and A/B knobs, the coordinate map and its
// backward chain, interpolation weights and tap blocks, window staging, the fixed-point scatter and the host-side
// helpers of the schedule choice.  Everything below the declarations sits in an anonymous namespace.
#pragma once
#include <stdlib.h>
#include <algorithm>
#include <type_traits>
#include "common.h"

#pragma clang fp contract(off)   // every FMA of the advection units is explicit

// One call of paradis_sl_advect_{fwd,bwd}.  forward: (field, u, v) -> out; backward: (gout, field, u, v) -> (gfield, gu, gv)
struct AdvArgs {
  const float* gout; const float* field; const float* u; const float* v;
  float* out; float* gfield; float* gu; float* gv;
  const float* sin_lat; const float* cos_lat; const float* lat_cells; const float* lon;
  int B, K, H, W;
  int64_t go_bs, f_bs, uv_bs, o_bs, gf_bs, guv_bs;      // strides between samples
  // the grid as the reference holds it (min_lat, min_lon, d_lat = max - min, d_lon: model/advection.py:67-72); AdvGeom,
  // the constants of the coordinate map the kernels take, is a type of each unit: make_geom(a)
  float dt, min_lat, min_lon, d_lat, d_lon;
  int mode, flags;
  int vec4;                 // 16-byte staging path: aligned planes, p even (bicubic), padded width even
  hipStream_t st;
  // regions of the workspace (advect.hip); nullptr where the schedule has none
  float* fmeans; float* gmeans;                 // pole-row means of field and cotangent, two floats per plane
  unsigned* pmax; unsigned long long* gacc;     // deterministic mode: per-plane max |cotangent| bits, 64-bit integer plane
  unsigned* counts; unsigned* wide;             // strips: deferred points per list, displacement class per plane
  unsigned* queue;                              // strips: the deferred-point lists
};

// Launchers, one per schedule and direction (advect.hip picks: adv_schedule).  0 = launched, 1 = bad argument,
// 2 = runtime error; the caller checks the launch (PD_CHECK_LAUNCH).
int pd_adv_fwd_row64(const AdvArgs& a);     // advect_planes.hip
int pd_adv_bwd_row64(const AdvArgs& a);
int pd_adv_fwd_whole(const AdvArgs& a);
int pd_adv_bwd_whole(const AdvArgs& a);
int pd_adv_fwd_tiled(const AdvArgs& a);
int pd_adv_bwd_tiled(const AdvArgs& a);
int pd_adv_fwd_tilerow(const AdvArgs& a);   // advect_tilerow.hip
int pd_adv_bwd_tilerow(const AdvArgs& a);
int pd_adv_fwd_strips(const AdvArgs& a);    // advect_strips.hip
int pd_adv_bwd_strips(const AdvArgs& a);
int pd_adv_bwd_circle(const AdvArgs& a);
#ifdef PARADIS_DEV_KNOBS
int pd_adv_fwd_direct(const AdvArgs& a, int rows);   // development library only
#endif

namespace {

constexpr float CLAMP_HI = 0.9999999f;  // float(1 - 1e-7), as torch.clamp converts its python bound
constexpr float KA = -0.75f;
#ifndef ADV_TILE_H         // (A/B builds: tools/build_variant.sh)
#define ADV_TILE_H 16
#endif
#ifndef ADV_TILED_THREADS_BWD
#define ADV_TILED_THREADS_BWD 512
#endif
#ifndef ADV_HALO_BWD
#define ADV_HALO_BWD 10
#endif
constexpr int TILE_H = ADV_TILE_H, TILE_W = 128;  // arrival tile of the tiled schedule (backward)
// forward tile height: a taller tile amortises the halo (window cells per arrival point 2.6 at 16
// rows, 1.9 at 32, 1.5 at 64 with a halo of 8); the forward window is 4 B/cell, so LDS is not the
// limit.  Measured at 128x256: 1.64 / 1.42 / 1.23 ms per launch for 16 / 32 / 64 rows
constexpr int TILE_HF = 64;
// threads per tile in the tiled schedule: the window fixes the LDS per workgroup, so waves per SIMD
// come from the workgroup size.  Backward (12 B/cell, 2 workgroups per CU): at 256 threads it ran 1.7
// waves per SIMD at 29 % VALU issue, 512 threads measured 6.9 -> 5.6 ms at 128x256
constexpr int TILED_THREADS_FWD = 512, TILED_THREADS_BWD = ADV_TILED_THREADS_BWD;
constexpr int ADV_PF = 2;   // prefetch distance (points) of the operand loads

struct AdvGeom {
  int H, W, p;
  float ndt;              // -dt
  float cx, cy;           // cells per radian: (W-1)/d_lon, (H-1)/d_lat
  float per, inv_per;     // longitude period in cells (2 pi cx) and its reciprocal
  float c0x, c0y;         // p - min_lon cx,  p - min_lat cy
  float qoff;             // -c0x / period: the wrap is taken on [c0x, c0x + period)
  double c0xd;            // c0x in double: folded into the longitude table (lon_cells)
  double cxd;             // cx in double: lon -> cells conversion of the longitude table
};

struct DepState {  // intermediates needed by the backward chain
  float sp, cp, sl, cl, s, n, d;
};

// ---- elementary functions ------------------------------------------------------------------
// sin and cos: cephes minimax polynomials on [-pi/4, pi/4] (<= ~1 ulp) behind a Cody-Waite reduction
// (fdlibm's float split of pi/2); huge arguments take the ocml path.
__device__ __forceinline__ void sincos_kernel(float r, float& ps, float& pc) {
  const float z = r * r;
  ps = fmaf(fmaf(fmaf(-1.9515295891e-4f, z, 8.3321608736e-3f), z, -1.6666654611e-1f) * z, r, r);
  pc = fmaf(fmaf(fmaf(2.443315711809948e-5f, z, -1.388731625493765e-3f), z, 4.166664568298827e-2f), z * z,
            fmaf(-0.5f, z, 1.0f));
}

__device__ __forceinline__ void sincos_reduced(float x, float& s, float& c) {
  if (fabsf(x) > 8192.0f) {
    sincosf(x, &s, &c);
    return;
  }
  const float k = rintf(x * 0.63661977236758134f);
  float r = fmaf(-k, 1.5707855225e+00f, x);   // pi/2 split in three parts with trailing zero bits
  r = fmaf(-k, 1.0804273188e-05f, r);
  r = fmaf(-k, 6.0770999344e-11f, r);
  const int q = (int)k;
  float ps, pc;
  sincos_kernel(r, ps, pc);
  const float ss = (q & 1) ? pc : ps;
  const float cc = (q & 1) ? ps : pc;
  s = (q & 2) ? -ss : ss;
  c = ((q + 1) & 2) ? -cc : cc;
}

// sin/cos of the two rotation angles of a point.  |angle| < 0.78 (< pi/4: the reduction's k is 0 and
// r = x exactly) for every lane of the wave is the normal case - displacements of less than 45 degrees
// per step - and needs no reduction and no quadrant selects: same bits, 10 instead of ~35 operations.
// |r| <= 1/8: the series two terms shorter, same error bounds (sin 0.51 ulp, cos 1.07 ulp)
__device__ __forceinline__ void sincos_kernel_small(float r, float& ps, float& pc) {
  const float z = r * r;
  ps = fmaf(fmaf(8.3333310e-3f, z, -1.6666667e-1f) * z, r, r);
  pc = fmaf(4.1666668e-2f * z, z, fmaf(-0.5f, z, 1.0f));
}

// Returns the tier taken (wave-uniform): 0 = every lane below 0.125 rad, 1 = below 0.78, 2 = general.
__device__ __forceinline__ int sincos_pair(float phi, float lam, float& sp, float& cp, float& sl, float& cl) {
  const float big = fmaxf(fabsf(phi), fabsf(lam));
  if (__all(big < 0.125f)) {     // displacements below 7 degrees per step: the usual case
    sincos_kernel_small(phi, sp, cp);
    sincos_kernel_small(lam, sl, cl);
    return 0;
  }
  if (__all(big < 0.78f)) {
    sincos_kernel(phi, sp, cp);
    sincos_kernel(lam, sl, cl);
    return 1;
  }
  sincos_reduced(phi, sp, cp);
  sincos_reduced(lam, sl, cl);
  return 2;
}

// (asin(x) - x) / x^3 as a polynomial in y = x^2 on [0, 1/4]; with the half-angle identity
// asin(x) = pi/2 - 2 asin(sqrt((1-x)/2)) for |x| >= 1/2 the result is within 2.3 ulp (mean 0.45),
// the host libm's float asin within 3.1 (mean 0.44)
__device__ __forceinline__ float asin_poly(float y) {
  float p = fmaf(0x1.15e14ep-5f, y, 0x1.169fe6p-6f);
  p = fmaf(p, y, 0x1.fe10a0p-6f);
  p = fmaf(p, y, 0x1.6d55e8p-5f);
  p = fmaf(p, y, 0x1.333448p-4f);
  return fmaf(p, y, 0x1.555554p-3f);
}

// asin for |x| < 1.  The lanes of a wave share a latitude row in every schedule, so the branch is
// wave-uniform almost always; the mixed case evaluates one polynomial behind selects.
__device__ __forceinline__ float asin_wave(float x) {
  const float ax = fabsf(x);
  const bool big = ax >= 0.5f;
  if (!__any(big)) {
    const float y = x * x;
    return fmaf(x, y * asin_poly(y), x);
  }
  const float t = fmaf(ax, -0.5f, 0.5f);
  const float r = __builtin_amdgcn_sqrtf(t);   // 1 ulp; contributes <= 0.5 ulp of the result
  float y = t, a = r;
  const bool mixed = !__all(big);
  if (mixed) {
    y = big ? t : ax * ax;
    a = big ? r : ax;
  }
  const float yy = fmaf(a, y * asin_poly(y), a);
  float res = fmaf(-2.0f, yy, 0x1.921fb6p+0f);
  if (mixed) res = big ? res : yy;
  return copysignf(res, x);
}

__device__ __forceinline__ float atan_poly(float t) {   // ocml's degree-8 minimax in t^2, |t| <= 1
  const float z = t * t;
  float pp = fmaf(z, 0x1.5a54bp-9f, -0x1.f4b218p-7f);
  pp = fmaf(z, pp, 0x1.53f67ep-5f);
  pp = fmaf(z, pp, -0x1.2fa9aep-4f);
  pp = fmaf(z, pp, 0x1.b26364p-4f);
  pp = fmaf(z, pp, -0x1.22c1ccp-3f);
  pp = fmaf(z, pp, 0x1.99717ep-3f);
  pp = fmaf(z, pp, -0x1.5554c4p-2f);
  return fmaf(t, z * pp, t);
}

// atan2 for finite arguments of ordinary magnitude (here y^2 + x^2 = cos^2(lat_d) > 1e-7).  When every
// lane of the wave has |y| < x (the departure point is less than 45 degrees of longitude away: the
// normal case) the quotient needs no octant bookkeeping.
__device__ __forceinline__ float atan2_wave(float y, float x) {
  if (__all(fabsf(y) < x)) return atan_poly(y * __builtin_amdgcn_rcpf(x));
  const float ax = fabsf(x), ay = fabsf(y);
  const float mx = fmaxf(ax, ay), mn = fminf(ax, ay);
  float a = atan_poly(mn * __builtin_amdgcn_rcpf(mx));
  a = (ay > ax) ? 0x1.921fb6p+0f - a : a;
  a = (x < 0.f) ? 0x1.921fb6p+1f - a : a;
  a = (y == 0.f) ? ((__float_as_int(x) < 0) ? 0x1.921fb6p+1f : 0.f) : a;   // also covers 0/0
  return copysignf(a, y);
}

// lonc = lon_a cx (cells), sa/ca = sin/cos(lat_a).  Returns the sample coordinates on the padded plane.
__device__ __forceinline__ void departure(float u, float v, float sa, float ca, float lonc,
                                          const AdvGeom& g, float& ix, float& iy, DepState* st) {
  const float lam = u * g.ndt;
  const float phi = v * g.ndt;
  float sp, cp, sl, cl;
  sincos_pair(phi, lam, sp, cp, sl, cl);
  const float cc = cp * cl;
  const float s = fmaf(sp, ca, cc * sa);
  const float sc = __builtin_amdgcn_fmed3f(s, -CLAMP_HI, CLAMP_HI);
  const float lat_d = asin_wave(sc);
  const float n = cp * sl;
  const float d = fmaf(cc, ca, -(sp * sa));
  const float a = atan2_wave(n, d);
  const float t = fmaf(a, g.cx, lonc);                 // unwrapped departure longitude in padded cells
  const float q = floorf(fmaf(t, g.inv_per, g.qoff));
  ix = fmaf(-q, g.per, t);                             // in [c0x, c0x + period) up to one rounding
  iy = fmaf(lat_d, g.cy, g.c0y);
  if (st) {
    st->sp = sp; st->cp = cp; st->sl = sl; st->cl = cl; st->s = s; st->n = n; st->d = d;
  }
}

// The map evaluated per lane, without the wave-uniform branches of the elementary functions above: the branch a point
// takes there depends on the other 63 points of its wave, which is harmless where the assignment of points to waves is
// fixed by the launch geometry, but not for the deferred points of the strip schedule - the order in which waves
// append to a strip's list varies from run to run, and with it a point's wave mates (a polar point amplifies the
// difference between two sin/cos tiers to 2e-4 of its velocity gradient).
__device__ __forceinline__ void departure_lane(float u, float v, float sa, float ca, float lonc,
                                               const AdvGeom& g, float& ix, float& iy, DepState* st) {
  const float lam = u * g.ndt;
  const float phi = v * g.ndt;
  float sp, cp, sl, cl;
  sincos_reduced(phi, sp, cp);
  sincos_reduced(lam, sl, cl);
  const float cc = cp * cl;
  const float s = fmaf(sp, ca, cc * sa);
  const float sc = __builtin_amdgcn_fmed3f(s, -CLAMP_HI, CLAMP_HI);
  // asin: one polynomial behind selects (the mixed case of asin_wave)
  float lat_d;
  {
    const float ax = fabsf(sc);
    const bool big = ax >= 0.5f;
    const float t = fmaf(ax, -0.5f, 0.5f);
    const float r = __builtin_amdgcn_sqrtf(t);
    const float y = big ? t : ax * ax;
    const float a = big ? r : ax;
    const float yy = fmaf(a, y * asin_poly(y), a);
    lat_d = copysignf(big ? fmaf(-2.0f, yy, 0x1.921fb6p+0f) : yy, sc);
  }
  const float n = cp * sl;
  const float d = fmaf(cc, ca, -(sp * sa));
  float a;
  {   // the octant form of atan2_wave
    const float ax = fabsf(d), ay = fabsf(n);
    const float mx = fmaxf(ax, ay), mn = fminf(ax, ay);
    a = atan_poly(mn * __builtin_amdgcn_rcpf(mx));
    a = (ay > ax) ? 0x1.921fb6p+0f - a : a;
    a = (d < 0.f) ? 0x1.921fb6p+1f - a : a;
    a = (n == 0.f) ? ((__float_as_int(d) < 0) ? 0x1.921fb6p+1f : 0.f) : a;
    a = copysignf(a, n);
  }
  const float t = fmaf(a, g.cx, lonc);
  const float q = floorf(fmaf(t, g.inv_per, g.qoff));
  ix = fmaf(-q, g.per, t);
  iy = fmaf(lat_d, g.cy, g.c0y);
  if (st) {
    st->sp = sp; st->cp = cp; st->sl = sl; st->cl = cl; st->s = s; st->n = n; st->d = d;
  }
}

// The same map for a wave that is ONE LATITUDE ROW (separable schedules): sa, ca and iya - the arrival latitude
// in padded cells, p + (lat_a - min_lat) cy - are wave-uniform scalars.  The small-displacement regime is decided
// ONCE per row by a single vector condition - both rotation angles below 0.125 rad, departure less than 45 degrees
// of longitude away, no clamp active - behind which the code is straight-line: short sin/cos series, plain atan
// quotient, and the latitude either from the short asin polynomial (rows within asin's small-argument range for
// every such displacement: |sin(lat_a)| < 1/4) or RELATIVE to the arrival latitude:
//     sin(lat_d - lat_a) = s cos(lat_a) - cos(lat_d) sin(lat_a) = sin(phi') - sin(lat_a) (cos(lat_d) - d),
//     cos(lat_d) = sqrt(n^2 + d^2)
// (expand s and d: the products of sa, ca cancel exactly), iy = iya + cy asin(small argument): no half-angle chain,
// and the rounding of s is not amplified by 1 / cos(lat_d) next to the poles - against the fp64 evaluation this form
// is ~20 x closer than asin(s) in fp32 at every grid size.  Any other wave takes departure().
__device__ __forceinline__ void departure_row(float u, float v, float sa, float ca, float lonc, float iya,
                                              const AdvGeom& g, float& ix, float& iy, DepState* st) {
  const float lam = u * g.ndt;
  const float phi = v * g.ndt;
  float sp, cp, sl, cl;
  sincos_kernel_small(phi, sp, cp);
  sincos_kernel_small(lam, sl, cl);
  const float cc = cp * cl;
  const float s = fmaf(sp, ca, cc * sa);
  const float n = cp * sl;
  const float d = fmaf(cc, ca, -(sp * sa));
#ifndef ADV_NO_REL    // (diagnostic A/B builds only)
  const bool ok = fmaxf(fabsf(phi), fabsf(lam)) < 0.125f && fabsf(n) < d && fabsf(s) <= CLAMP_HI;
#else
  const bool ok = false;
#endif
  if (!__all(ok)) {
    departure(u, v, sa, ca, lonc, g, ix, iy, st);
    return;
  }
  if (fabsf(sa) < 0.25f) {           // scalar: |s| <= |sa| + sin(0.25) < 1/2 for every lane
    const float y2 = s * s;
    iy = fmaf(fmaf(s, y2 * asin_poly(y2), s), g.cy, g.c0y);
  } else {
    const float cosd = __builtin_amdgcn_sqrtf(fmaf(d, d, n * n));
    const float arg = fmaf(-sa, cosd - d, sp);         // |arg| <= sin(0.25)
    const float y2 = arg * arg;
    iy = fmaf(fmaf(arg, y2 * asin_poly(y2), arg), g.cy, iya);
  }
  const float a = atan_poly(n * __builtin_amdgcn_rcpf(d));
  const float t = fmaf(a, g.cx, lonc);
  const float q = floorf(fmaf(t, g.inv_per, g.qoff));
  ix = fmaf(-q, g.per, t);
  if (st) {
    st->sp = sp; st->cp = cp; st->sl = sl; st->cl = cl; st->s = s; st->n = n; st->d = d;
  }
}

// A wave-uniform pointer pinned to scalar registers: `srow(p)[lane]` with an unsigned 32-bit lane then
// becomes a global access with a scalar base and a 32-bit vector offset (no 64-bit vector address
// arithmetic per load: 7 half-rate VALU operations per access in the first version of these loops).
template <typename T>
using global_ptr = __attribute__((address_space(1))) T*;   // explicit: an integer-built pointer would be `flat`
template <typename T>
__device__ __forceinline__ global_ptr<T> srow(T* p) {
  const uint64_t a = (uint64_t)p;
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)a);
  const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(a >> 32));
  return (global_ptr<T>)(((uint64_t)hi << 32) | lo);
}

// arrival longitude in padded cells: lon cx + c0x, one rounding
__device__ __forceinline__ float lon_cells(float lon, const AdvGeom& g) { return (float)fma((double)lon, g.cxd, g.c0xd); }

// ---- interpolation weights -------------------------------------------------------------------
// (the weights and tap sums are not coordinate-critical - an ulp of a weight is 1e-7 relative in the
//  result, whereas an ulp of a sample coordinate is multiplied by the field slope)
__device__ __forceinline__ float cub1(float x) { return fmaf(fmaf(KA + 2.f, x, -(KA + 3.f)) * x, x, 1.f); }
__device__ __forceinline__ float dcub1(float x) { return fmaf(3.f * (KA + 2.f), x, -2.f * (KA + 3.f)) * x; }

template <int MODE>
struct Interp {
  static constexpr int NT = (MODE == PARADIS_INTERP_BICUBIC) ? 4 : 2;
  static constexpr int OFF0 = (MODE == PARADIS_INTERP_BICUBIC) ? -1 : 0;
  // Keys cubic convolution, A = -0.75: taps at -1, 0, 1, 2 carry  A t (1-t)^2,  c1(t),  c1(1-t),  A t^2 (1-t)
  static __device__ __forceinline__ void weights(float t, float* w) {
    if (MODE == PARADIS_INTERP_BICUBIC) {
      // the four weights sum to 1 and w0 + w3 = A t (1-t) (t + (1-t)): the fourth costs two subtractions
      const float um = 1.f - t, atu = (KA * t) * um;
      w[0] = atu * um; w[1] = cub1(t); w[3] = atu * t; w[2] = (1.f - w[1]) - atu;
    } else {
      w[0] = 1.f - t; w[1] = t;
    }
  }
  static __device__ __forceinline__ void dweights(float t, float* dw) {
    if (MODE == PARADIS_INTERP_BICUBIC) {
      const float um = 1.f - t;
      dw[0] = fmaf(fmaf(3.f * KA, t, -4.f * KA), t, KA);     // A (3t^2 - 4t + 1)
      dw[1] = dcub1(t);
      dw[2] = -dcub1(um);
      dw[3] = fmaf(-3.f * KA, t, 2.f * KA) * t;              // A (2t - 3t^2)
    } else {
      dw[0] = -1.f; dw[1] = 1.f;
    }
  }
};

// ATen zeroes taps outside the padded plane; on this path that only happens when a coordinate
// rounds onto the plane edge, where the outside taps carry weight exactly 0.  The tap block is
// therefore shifted inside the plane (by `shift` cells) and the weights re-indexed: cells that left
// the block get weight 0 - same value, no stray reads.
template <int NT>
__device__ __forceinline__ void shift_weights(float* w, int shift) {
  if (shift == 0) return;
  float t[NT];
#pragma unroll
  for (int b = 0; b < NT; ++b) t[b] = w[b];
#pragma unroll
  for (int b = 0; b < NT; ++b) {
    float v = 0.f;
#pragma unroll
    for (int k = 0; k < NT; ++k) v = (k == b + shift) ? t[k] : v;
    w[b] = v;
  }
}

// Top-left tap (padded coordinates), clamped inside the plane; sx/sy = applied shifts.
template <int MODE>
__device__ __forceinline__ void tap_origin(float ix, float iy, int Hp, int Wp, int& bx, int& by,
                                           int& sx, int& sy, float& tx, float& ty) {
  constexpr int NT = Interp<MODE>::NT, OFF0 = Interp<MODE>::OFF0;
  const float x0f = floorf(ix), y0f = floorf(iy);
  tx = ix - x0f;
  ty = iy - y0f;
  // NaN/inf/huge: v_med3 clamps (NaN -> the lower bound), the shift then zeroes every weight
  const int x0 = (int)__builtin_amdgcn_fmed3f(x0f, -8.0f, (float)(Wp + 8)) + OFF0;
  const int y0 = (int)__builtin_amdgcn_fmed3f(y0f, -8.0f, (float)(Hp + 8)) + OFF0;
  bx = min(max(x0, 0), Wp - NT);
  by = min(max(y0, 0), Hp - NT);
  sx = bx - x0;
  sy = by - y0;
}

// Tap block of a point when the window is the WHOLE padded plane: fraction, clamped origin and the
// LDS index in float arithmetic (exact: every value is an integer below 2^24), one conversion.
// Returns true when the clamp moved the origin (a coordinate on the plane edge, or not finite): the
// caller takes the general path.  `cell` indexes tap (0,0) BEFORE the OFF0 shift.
template <int MODE>
__device__ __forceinline__ bool tap_block_whole(float ix, float iy, float Hpf, float Wpf, float& tx, float& ty,
                                                int& cell) {
  constexpr int NT = Interp<MODE>::NT, OFF0 = Interp<MODE>::OFF0;
  tx = __builtin_amdgcn_fractf(ix);
  ty = __builtin_amdgcn_fractf(iy);
  const float x0f = ix - tx, y0f = iy - ty;
  const float xc = __builtin_amdgcn_fmed3f(x0f, (float)(-OFF0), Wpf - (float)(NT + OFF0));
  const float yc = __builtin_amdgcn_fmed3f(y0f, (float)(-OFF0), Hpf - (float)(NT + OFF0));
  cell = (int)fmaf(yc, Wpf, xc);
  return !(xc == x0f && yc == y0f);
}

__device__ __forceinline__ float wave_row_mean(const float* row, int W) {
  float s = 0.f;
  for (int x = threadIdx.x & 63; x < W; x += 64) s += row[x];
  return wave_sum_dpp(s) / (float)W;
}

// Window of the padded plane held in LDS: padded rows [wy0, wy0+WH), padded cols [wx0, wx0+WW).
struct Window {
  int wy0, wx0, WH, WW;
};

// iterate i = tid, tid+nth, ... < th*tw as (yl, xl) without a division per point
struct TileIter {
  int yl, xl, dy, dx, tw;
  __device__ __forceinline__ TileIter(int tid, int tw_, int nth = 256) : tw(tw_) {
    yl = tid / tw_; xl = tid - yl * tw_; dy = nth / tw_; dx = nth - dy * tw_;
  }
  __device__ __forceinline__ void next() {
    yl += dy; xl += dx;
    if (xl >= tw) { xl -= tw; ++yl; }
  }
};

// stage src plane (image H x W) into the window through the geocyclic map; subst: replace source
// rows 0 / H-1 by the given means (tiled schedule; whole-plane schedules compute the means in LDS).
// Flat over the window in batches: all loads of a batch are issued before the first LDS write, so a
// workgroup pays ~one memory round trip for its window.
constexpr int STAGE_BATCH = 6;
__device__ __forceinline__ void stage_window(float* win, const float* __restrict__ F, const Window& w,
                                             int H, int W, int p, bool subst, float m0, float m1,
                                             int nth = 256) {
  // A thread keeps one window column (its longitude wrap - plain and mirrored - is computed once) and
  // walks down the rows; only the cheap row map (mirror beyond a pole) is per element.
  const int Hp = H + 2 * p;
  const int tid = threadIdx.x;
  const int cols = w.WW < nth ? w.WW : nth;          // window columns per pass
  const int rpp = nth / cols;                         // window rows per pass
  const int r0 = tid / cols, c0 = tid - r0 * cols;
  if (r0 >= rpp) return;
  for (int lc = c0; lc < w.WW; lc += cols) {
    int jj = (w.wx0 + lc - p) % W;
    if (jj < 0) jj += W;
    int jm = jj + (W >> 1);
    if (jm >= W) jm -= W;
    for (int l0 = r0; l0 < w.WH; l0 += rpp * STAGE_BATCH) {
      float val[STAGE_BATCH];
#pragma unroll
      for (int j = 0; j < STAGE_BATCH; ++j) {
        // unconditional load from a clamped (always valid) source cell, then select
        const int lr = l0 + rpp * j;
        const int r = w.wy0 + lr;                      // padded row
        const bool valid = lr < w.WH && r >= 0 && r < Hp;
        const int ii = min(max(r, 0), Hp - 1) - p;
        int sr = ii;
        bool mir = false;
        if (ii < 0) { sr = -ii; mir = true; }
        else if (ii >= H) { sr = 2 * (H - 1) - ii; mir = true; }
        float v = F[(int64_t)sr * W + (mir ? jm : jj)];
        if (subst && sr == 0) v = m0;
        if (subst && sr == H - 1) v = m1;
        val[j] = valid ? v : 0.f;
      }
#pragma unroll
      for (int j = 0; j < STAGE_BATCH; ++j) {
        const int lr = l0 + rpp * j;
        if (lr < w.WH) win[lr * w.WW + lc] = val[j];
      }
    }
  }
}

// pole rows of a whole padded plane in LDS <- their mean over the W interior columns (lon halo included)
__device__ __forceinline__ void pole_rows_to_mean_lds(float* win, int H, int W, int p, int Wp) {
  const int wave = threadIdx.x >> 6;
  if (wave < 2) {
    float* row = win + (wave == 0 ? p : H - 1 + p) * Wp;
    const float m = wave_row_mean(row + p, W);
    for (int x = threadIdx.x & 63; x < Wp; x += 64) row[x] = m;
  }
}

// value of one arrival point from a WHOLE-plane window
template <int MODE>
__device__ __forceinline__ float sample_whole(const float* win, float ix, float iy, int Hp, int Wp, float Hpf,
                                              float Wpf) {
  constexpr int NT = Interp<MODE>::NT, OFF0 = Interp<MODE>::OFF0;
  float tx, ty, wx[NT], wy[NT];
  int cell;
  const bool edge = tap_block_whole<MODE>(ix, iy, Hpf, Wpf, tx, ty, cell);
  const float* base = win + OFF0 * (Wp + 1) + cell;
  if (__any(edge)) {   // a coordinate rounded onto the plane edge, or is not finite: general origin + shifted weights
    int bx, by, sx, sy;
    tap_origin<MODE>(ix, iy, Hp, Wp, bx, by, sx, sy, tx, ty);
    Interp<MODE>::weights(tx, wx);
    Interp<MODE>::weights(ty, wy);
    shift_weights<NT>(wx, sx);
    shift_weights<NT>(wy, sy);
    base = win + by * Wp + bx;
  } else {
    Interp<MODE>::weights(tx, wx);
    Interp<MODE>::weights(ty, wy);
  }
  float acc = 0.f;
#pragma unroll
  for (int a = 0; a < NT; ++a) {
    float rowacc = 0.f;
#pragma unroll
    for (int bb = 0; bb < NT; ++bb) rowacc = fmaf(base[a * Wp + bb], wx[bb], rowacc);
    acc = fmaf(rowacc, wy[a], acc);
  }
  return acc;
}

// ======================================================================================
// backward
// ======================================================================================
// round-to-nearest-even integer of x (|x| < 2^51) as a two's-complement 64-bit pattern in three
// instructions: widen, add 1.5*2^52 (the integer lands in the low mantissa bits), strip the exponent
// pattern from the high word.  (A float -> int64 conversion proper is ~12 VALU instructions and the
// scatter does 16 of them per point.)
__device__ __forceinline__ unsigned long long fixed_from_float(float x) {
  const double d = (double)x + 6755399441055744.0;
  return (unsigned long long)(__double_as_longlong(d) - 0x4338000000000000ll);
}

// mx = max |cotangent| of the tile, NaN if any cotangent is NaN (the reduction runs on the bit
// patterns of |g|: as unsigned integers they order like the floats, and every NaN sorts above +inf)
__device__ __forceinline__ void fixed_point_scale(float mx, float& scale, float& inv) {
  scale = 0.f; inv = 0.f;
  if (mx > 0.f && mx < INFINITY) {
    int e = 0;
    frexpf(mx, &e);                       // mx < 2^e
    e = e < -80 ? -80 : (e > 80 ? 80 : e);
    scale = ldexpf(1.0f, 40 - e);
    inv = ldexpf(1.0f, e - 40);
  } else if (!(mx < INFINITY)) {
    inv = NAN;                            // Inf or NaN cotangent: the field gradient is NaN, like float adds would give
  }
}

__device__ __forceinline__ unsigned abs_bits(float g) { return __float_as_uint(g) & 0x7fffffffu; }

__device__ __forceinline__ void departure_backward(const DepState& st, float sa, float ca, float gix,
                                                   float giy, const AdvGeom& g, float& gu, float& gv) {
  const float glam_c = gix * g.cx, gphi_c = giy * g.cy;
  const float sc = __builtin_amdgcn_fmed3f(st.s, -CLAMP_HI, CLAMP_HI);
  // d asin(s) / ds = 1 / sqrt(1 - s^2) = 1 / cos(lat_d), and 1 - s^2 = n^2 + d^2 identically ((s, n, d) is a unit
  // vector): the sum of squares has no cancellation, whereas 1 - s^2 formed from the rounded s loses
  // log2(1 / cos^2(lat_d)) bits next to the poles (at 89.3 degrees: relative error 8e-4 in fp32) - the reference's
  // fp32 autograd carries that error, the fp64 evaluation does not.
  // v_rsq / v_rcp (1 ulp) with one Newton step on the reciprocal: gradient error ~1e-7 relative
  const float den = fmaf(st.n, st.n, st.d * st.d);
#ifdef ADV_GS_FROM_S     // (diagnostic A/B builds only: the reference's form)
  const float gs = (sc == st.s) ? gphi_c * __builtin_amdgcn_rsqf(fmaf(-sc, sc, 1.0f)) : 0.f;
#else
  const float gs = (sc == st.s) ? gphi_c * __builtin_amdgcn_rsqf(den) : 0.f;
#endif
  float rden = __builtin_amdgcn_rcpf(den);
  rden = fmaf(fmaf(-den, rden, 1.0f), rden, rden);
  const float gl = glam_c * rden;
  const float gn = gl * st.d;
  const float gd = -gl * st.n;
  // d s / d phi' = cp ca - sp cl sa,   d n / d phi' = -sp sl,   d d / d phi' = -sp cl ca - cp sa
  const float spcl = st.sp * st.cl, cpsl = st.cp * st.sl;
  const float gphi = fmaf(gs, fmaf(st.cp, ca, -(spcl * sa)),
                          fmaf(gn, -(st.sp * st.sl), gd * -fmaf(spcl, ca, st.cp * sa)));
  // d s / d lam' = -cp sl sa,           d n / d lam' = cp cl,    d d / d lam' = -cp sl ca
  const float glam = fmaf(gs, -(cpsl * sa), fmaf(gn, st.cp * st.cl, gd * -(cpsl * ca)));
  gu = g.ndt * glam;
  gv = g.ndt * gphi;
}

// round-to-nearest-even integer of the product a*b in one double FMA (a, b widened once per row /
// column of the tap block instead of a conversion per tap): a*b is exact in double, the sum with
// 1.5*2^52 rounds it to an integer in the low mantissa bits
__device__ __forceinline__ unsigned long long fixed_from_product(double a, double b) {
  const double d = fma(a, b, 6755399441055744.0);
  return (unsigned long long)(__double_as_longlong(d) - 0x4338000000000000ll);
}

// taps of one arrival point against a window: scatter g w_y w_x into the fixed-point accumulators,
// gather the field for the coordinate gradients.  base = index of tap (0,0) in the window.
template <int MODE>
__device__ __forceinline__ void scatter_gather(unsigned long long* acc, const float* win, int base, int WW,
                                               const float* wx, const float* wy, const float* dwx,
                                               const float* dwy, float gs_, float& gix, float& giy) {
  constexpr int NT = Interp<MODE>::NT;
  gix = 0.f; giy = 0.f;
  double wxd[NT];
#pragma unroll
  for (int bb = 0; bb < NT; ++bb) wxd[bb] = (double)wx[bb];
#pragma unroll
  for (int a = 0; a < NT; ++a) {
    float sxv = 0.f, sdx = 0.f;
    const double gwy = (double)(gs_ * wy[a]);
#pragma unroll
    for (int bb = 0; bb < NT; ++bb) {
      const int cell = base + a * WW + bb;
      const float val = win[cell];
      atomicAdd(&acc[cell], fixed_from_product(gwy, wxd[bb]));
      sxv = fmaf(val, wx[bb], sxv);
      sdx = fmaf(val, dwx[bb], sdx);
    }
    gix = fmaf(wy[a], sdx, gix);
    giy = fmaf(dwy[a], sxv, giy);
  }
}

// workgroup maximum of the |cotangent| bit patterns; contains a barrier
__device__ __forceinline__ float reduce_gmax(unsigned gmaxb, float* misc, int nwaves) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) gmaxb = max(gmaxb, (unsigned)__shfl_xor((int)gmaxb, o, 64));
  if ((threadIdx.x & 63) == 0) misc[2 + (threadIdx.x >> 6)] = __uint_as_float(gmaxb);
  __syncthreads();
  unsigned m = 0;
  for (int q = 0; q < nwaves; ++q) m = max(m, __float_as_uint(misc[2 + q]));
  return __uint_as_float(m);
}

// strip schedules (advect_strips.hip): a strip is 128 arrival columns of a plane, eight rows per step
constexpr int STRIP_W = 128, STRIP_ROWS = 8, STRIP_THREADS = 512, STRIP_CH = 4;   // CH: 64-column chunks of a window row
constexpr int STRIP_MAX_WS = 64 * STRIP_CH;
constexpr int STRIP_LDS_MAX = 160 * 1024 - 1024;   // dynamic LDS a strip kernel may ask for (it also holds a static counter word)

// ======================================================================================
// host side
// ======================================================================================
inline int adv_pad(int mode) { return mode == PARADIS_INTERP_BICUBIC ? 2 : 1; }   // geocyclic padding: half the tap block

// constants of the coordinate map, evaluated in double from the reference's fp32 buffers
// (min_lat, min_lon, d_lat = max - min, d_lon: model/advection.py:67-72)
AdvGeom make_geom(int H, int W, int p, float dt, float min_lat, float min_lon, float d_lat, float d_lon) {
  AdvGeom g;
  g.H = H; g.W = W; g.p = p;
  g.ndt = -dt;
  const double cx = ((double)W - 1.0) / (double)d_lon, cy = ((double)H - 1.0) / (double)d_lat;
  const double per = 6.283185307179586476925286766559 * cx;
  g.cx = (float)cx; g.cy = (float)cy; g.cxd = cx;
  g.per = (float)per; g.inv_per = (float)(1.0 / per);
  g.c0xd = (double)p - (double)min_lon * cx;
  g.c0x = (float)g.c0xd;
  g.qoff = (float)(-g.c0xd / per);
  g.c0y = (float)((double)p - (double)min_lat * cy);
  return g;
}
AdvGeom make_geom(const AdvArgs& a) {
  return make_geom(a.H, a.W, adv_pad(a.mode), a.dt, a.min_lat, a.min_lon, a.d_lat, a.d_lon);
}

// window halos (padded cells) of the tiled schedule.  Forward windows are cheap (4 B/cell); the
// backward holds 12 B/cell (64-bit accumulators + field), so its halo is what LDS allows at 2
// workgroups per CU.  Taps outside the window take the L2 / global-atomic path.
constexpr int HALO_FWD = 8;    // in-model optimum 6-12 at 128x256 and 721x1440; 24 pays only for ~45 px displacements
constexpr int HALO_BWD = ADV_HALO_BWD;   // two workgroups of 512 threads per CU
constexpr int MAX_HALO = 32;

// A dynamic-LDS request above 64 KiB has to be granted per kernel and device: `bytes` on every kernel of `table` - an
// array, of any rank, of one kernel type: the table the launch indexes - once per device (`once`: one per kernel family)
template <typename Table>
int reserve_lds(PerDeviceOnce& once, const Table& table, const char* what, int bytes = 160 * 1024) {
  using Kernel = std::remove_all_extents_t<Table>;
  static_assert(std::is_array_v<Table> && std::is_pointer_v<Kernel>, "a table of kernel pointers");
  if (!once.first()) return 0;
  const Kernel* k = reinterpret_cast<const Kernel*>(&table);
  for (size_t i = 0; i < sizeof(Table) / sizeof(Kernel); ++i)
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(k[i]), hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess) {
      paradis_set_error("%s: cannot reserve LDS", what);
      return 2;
    }
  return 0;
}
// the kernel tables' first index: {PARADIS_INTERP_BILINEAR, PARADIS_INTERP_BICUBIC}
inline int adv_mode_index(int mode) { return mode == PARADIS_INTERP_BICUBIC ? 1 : 0; }

// `flags` of the C ABI (include/paradis_hip.h, PARADIS_ADVECT_*): schedule choice (advect.hip: adv_schedule) and window
// halo are per-call arguments, the library keeps no mutable state
size_t bwd_whole_lds(size_t cells) { return (3 * ((cells + 1) & ~(size_t)1) + 24) * sizeof(float); }   // 64-bit accumulators + field
int halo_of(int flags, int dflt, bool backward) {
  int h = (flags >> PARADIS_ADVECT_HALO_SHIFT) & 0xff;          // 0 = default, else halo + 1
  const int hb = (flags >> PARADIS_ADVECT_HALO_BWD_SHIFT) & 0xff;
  if (backward && hb) h = hb;
  return h == 0 ? dflt : std::min(h - 1, MAX_HALO);
}
// strip schedule: ring rows by grid height (latitude halo 6 / 22 rows: displacements in
// the default model stay below 6 rows at 128 x 256 and below 22 rows for 99 % of the points at 721 x 1440,
// tools/adv_disp_stats.py); longitude halos: what 3 (forward) / 2 (backward) workgroups per CU leave room for
int strip_ring_rows(int H) { return H <= 160 ? 32 : 64; }
int strip_halo_fwd(int W) { return W <= 512 ? 10 : 32; }
int strip_halo_bwd(int W) { return W <= 512 ? 10 : 16; }

// dynamic LDS of the whole-plane schedules (forward: the padded plane and two rows of means)
size_t fwd_whole_lds(int H, int W, int p) { return ((size_t)(H + 2 * p) * (W + 2 * p) + 2 * W) * sizeof(float); }
size_t bwd_whole_lds(int H, int W, int p) { return bwd_whole_lds((size_t)(H + 2 * p) * (W + 2 * p)); }
// arrival tiles of the tiled schedules and the LDS window of one tile
struct AdvTiles { int halo, tx, tiles; size_t lds; };
AdvTiles adv_tiles(int H, int W, int NT, int flags, bool backward) {
  AdvTiles t;
  const int th = backward ? TILE_H : TILE_HF;
  t.halo = halo_of(flags, backward ? HALO_BWD : HALO_FWD, backward);
  t.tx = (W + TILE_W - 1) / TILE_W;
  t.tiles = t.tx * ((H + th - 1) / th);
  const size_t cells = (size_t)(th + 2 * t.halo + NT) * (TILE_W + 2 * t.halo + NT);
  t.lds = backward ? bwd_whole_lds(cells) : cells * sizeof(float);
  return t;
}
// full-circle backward: field and 64-bit sums in a ring of strip_ring_rows(H) rows / the sums alone in a ring of 64 rows
size_t circle_lds(int H, int W, int NT) { return ((size_t)strip_ring_rows(H) * (W + NT) * 3 + 8) * sizeof(float); }
size_t circle_lds_wide(int W, int NT) { return ((size_t)64 * (W + NT) * 2 + 8) * sizeof(float); }

}  // namespace
