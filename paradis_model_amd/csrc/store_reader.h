// The element readers of a device-resident store [T, F, P] (P = H*W), float32 or 16-bit packed, written once for
// feed.hip (batch assembly, paradis_unpack_planes) and climatology.hip (the climatology means): where a (time, feature)
// plane starts, and four / one of its values.
//
// Every including unit is compiled with -ffp-contract=off, so a value decoded here has the same bits whichever kernel
// decodes it: two fp32 roundings, no FMA.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// 16-bit packed planes (GRIB simple packing; DESIGN.md, "The packed store").  A plane is one (time, feature) field of P
// values; it carries (lo, s) in a float32 table [T, F, 2] and 16-bit codes, PACK_MISSING for NaN / +-Inf.  The packed
// quantity of domain 1 (log) is y = log(x + 1e-6), the precipitation normalisation's own shift, of domain 0 (linear)
// y = x.  log and exp are taken in double and rounded once: the correctly rounded float32 value, which every platform's
// libm gives alike (logf / expf differ between libraries in the last bit, and a code would then depend on who packed).
constexpr int PACK_MISSING = 65535;
constexpr float PACK_LOG_EPS = 1e-6f;   // the store format's own shift of the log domain (not a normalisation constant)
constexpr float PACK_TOP = 65534.0f;

// The ONE decode: unpack_planes_kernel, the packed assemble_batch_kernel and the packed clim_mean_kernel all call it, so
// a batch assembled from a packed store equals, bit for bit, the float32 batch assembled from the unpacked store, and a
// climatology of a packed store the climatology of its decoded rows.  Two fp32 roundings, no FMA.
__device__ __forceinline__ float unpack_value(uint32_t code, float lo, float s, int domain) {
  if (code == PACK_MISSING) return __builtin_nanf("");
  const float y = lo + s * (float)code;
  return domain == 1 ? fmaxf((float)exp((double)y) - PACK_LOG_EPS, 0.f) : y;
}

struct FloatPlanes {
  const float* __restrict__ data;
  struct Plane {
    const float* __restrict__ p;
  };
  typedef float4 Quad;
  __device__ __forceinline__ Plane plane(int64_t index, int /*f*/, int64_t P) const { return Plane{data + index * P}; }
  static __device__ __forceinline__ Quad load_quad(const Plane& pl, int64_t i) {
    return *reinterpret_cast<const float4*>(pl.p + i);
  }
  static __device__ __forceinline__ float4 quad_values(const Plane&, const Quad& q) { return q; }
  static __device__ __forceinline__ float value(const Plane& pl, int64_t i) { return pl.p[i]; }
};

struct PackedPlanes {
  const uint16_t* __restrict__ codes;
  const float* __restrict__ params;     // [T, F, 2]: lo, s
  const int* __restrict__ domain;       // [F]
  struct Plane {
    const uint16_t* __restrict__ p;
    float lo, s;
    int domain;
  };
  typedef uint2 Quad;                   // four codes: one 8-byte load
  __device__ __forceinline__ Plane plane(int64_t index, int f, int64_t P) const {
    return Plane{codes + index * P, params[2 * index], params[2 * index + 1], domain[f]};
  }
  static __device__ __forceinline__ Quad load_quad(const Plane& pl, int64_t i) {
    return *reinterpret_cast<const uint2*>(pl.p + i);
  }
  static __device__ __forceinline__ float4 quad_values(const Plane& pl, const Quad& q) {
    float4 o;
    o.x = unpack_value(q.x & 0xffffu, pl.lo, pl.s, pl.domain);
    o.y = unpack_value(q.x >> 16, pl.lo, pl.s, pl.domain);
    o.z = unpack_value(q.y & 0xffffu, pl.lo, pl.s, pl.domain);
    o.w = unpack_value(q.y >> 16, pl.lo, pl.s, pl.domain);
    return o;
  }
  static __device__ __forceinline__ float value(const Plane& pl, int64_t i) {
    return unpack_value(pl.p[i], pl.lo, pl.s, pl.domain);
  }
};

// the address test of the 8-byte (four codes) path
__host__ inline bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }
