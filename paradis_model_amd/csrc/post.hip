// f5: forecast post-processing on the device - one pass over a model output [B, C, H, W] (normalised, fp32) that
// writes the physical-unit state into slot t of a chunk [B, T, C, H, W]: de-normalisation (reference
// utils/postprocessing.py:198-215 with utils/normalization.py:11-13,39-52,69-80), Cartesian -> spherical winds
// (utils/postprocessing.py:74-122,143-187) and, optionally, the dew-point depression the reference's writer derives
// (utils/mhuaes.py:33-96 as called by utils/file_output.py:165-173) into [B, T, L, H, W].  The reference does this on
// the CPU after a .cpu() of the normalised chunk: one torch pass per normalisation kind, then numpy passes with
// float64 temporaries.  The input is never written: it is what the rollout feeds back.
//
// Arithmetic: the de-normalisation is fp32 in the reference's operation order (no contraction: -ffp-contract=off);
// winds and dew point are evaluated in fp64 from the fp32 de-normalised values and rounded once to fp32, which is
// what numpy does when the dataset's lat / lon are float64.  The places where numpy keeps float32 inside those
// expressions (a Python scalar times a float32 array: R * T, EPS1 + EPS2 * q) are float32 here too.
// sin / cos of latitude and longitude come from host-built double tables: no device trigonometry.
//
// Memory-bound: a thread owns 16 bytes along W of one unit - a pressure level (q, T, wind_x, wind_y, wind_z read once,
// written back converted, plus the dew point), the 10 m wind triple, or a single remaining channel.
// Algorithmic HBM bytes: 8*B*C*H*W (+ 4*B*L*H*W with the dew point).
#include "common.h"
#include "normalize.h"
#include "winds.h"

#pragma clang fp contract(off)

namespace {

constexpr int UNIT_INTS = 8;   // type, c0..c4, level, pad
constexpr int U_SINGLE = 0, U_LEVEL = 1;   // 2: the 10 m wind triple (no temperature, no vertical velocity)

struct PostArgs {
  const float* in;
  float* out;
  float* dew;
  const int* kind;
  const float* p0;
  const float* p1;
  const int* units;
  const double* plev;
  const double* trig;   // sin(lat)[H], cos(lat)[H], sin(lon)[W], cos(lon)[W]
  int64_t in_bs, out_bs, dew_bs;
  float eps_q;
  int n_units, B, H, W;
};

// one value back to physical units by its channel's class (normalize.h); a, b: mean, std | q_min, q_max
__device__ __forceinline__ float denorm(float x, int k, float a, float b, float eps_q) {
  if (k == NORM_ZSCORE) return denorm_zscore(x, a, b);
  if (k == NORM_HUMIDITY) {
    const float lmin = logf(a);
    return denorm_humidity(x, lmin, logf(b) - lmin, b, eps_q);
  }
  if (k == NORM_PRECIP) return denorm_precip(x);
  return x;
}

// dew-point depression (water phase, 30 K cap) of one cell; p = plev*100 Pa (an integer in the reference)
__device__ __forceinline__ float dew_depression(float q, float T, double p) {
  const float hu = fmaxf(1e-10f, q);
  const float den = 0.6219800221014f + 0.3780199778986f * hu;      // numpy: Python scalars keep the array's float32
  const double e = fmin(p, ((double)hu * p) / (double)den);
  const double c = log(e / 610.94);
  const double td = (30.11 * c - 17.625 * 273.16) / (c - 17.625);
  return (float)fmin((double)T - td, 30.0);
}

template <int V>
struct Vec;
template <>
struct Vec<4> {
  float v[4];
  __device__ __forceinline__ void load(const float* p) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  }
  __device__ __forceinline__ void store(float* p) const {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  }
};
template <>
struct Vec<1> {
  float v[1];
  __device__ __forceinline__ void load(const float* p) { v[0] = *p; }
  __device__ __forceinline__ void store(float* p) const { *p = v[0]; }
};

// V = 4: W % 4 == 0 and every plane 16-byte aligned; V = 1: the scalar fallback, the same arithmetic per cell
template <int V>
__global__ void __launch_bounds__(256) forecast_post_kernel(PostArgs a) {
  const int WV = a.W / V;
  const int64_t P = (int64_t)a.H * a.W;
  const int64_t per_unit = (int64_t)a.H * WV, per_batch = per_unit * a.n_units, total = per_batch * a.B;
  const double* slat_t = a.trig;
  const double* clat_t = a.trig + a.H;
  const double* slon_t = a.trig + 2 * a.H;
  const double* clon_t = slon_t + a.W;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int b = (int)(i / per_batch);
    const int64_t r = i - (int64_t)b * per_batch;
    const int u = (int)(r / per_unit);
    const int cell = (int)(r - (int64_t)u * per_unit);
    const int y = cell / WV, x0 = (cell - y * WV) * V;
    const int* un = a.units + u * UNIT_INTS;
    const int type = un[0];
    const int64_t pix = (int64_t)y * a.W + x0;
    const float* src = a.in + (int64_t)b * a.in_bs + pix;
    float* dst = a.out + (int64_t)b * a.out_bs + pix;
    if (type == U_SINGLE) {
      const int c = un[1];
      const int k = a.kind[c];
      const float m = a.p0[c], s = a.p1[c];
      Vec<V> t;
      t.load(src + c * P);
#pragma unroll
      for (int j = 0; j < V; ++j) t.v[j] = denorm(t.v[j], k, m, s, a.eps_q);
      t.store(dst + c * P);
      continue;
    }
    const double sla = slat_t[y], cla = clat_t[y];
    const int cq = un[1], ct = un[2], cx = un[3], cy = un[4], cz = un[5];
    Vec<V> q, T, wx, wy, wz;
    if (type == U_LEVEL) {
      const int kt = a.kind[ct];
      const float mt = a.p0[ct], st = a.p1[ct];
      T.load(src + ct * P);
#pragma unroll
      for (int j = 0; j < V; ++j) T.v[j] = denorm(T.v[j], kt, mt, st, a.eps_q);
      T.store(dst + ct * P);
      if (cq >= 0) {
        const int kq = a.kind[cq];
        const float mq = a.p0[cq], sq = a.p1[cq];
        q.load(src + cq * P);
#pragma unroll
        for (int j = 0; j < V; ++j) q.v[j] = denorm(q.v[j], kq, mq, sq, a.eps_q);
        q.store(dst + cq * P);
        if (a.dew != nullptr) {
          const int lev = un[6];
          const double p = a.plev[lev] * 100.0;
          Vec<V> es;
#pragma unroll
          for (int j = 0; j < V; ++j) es.v[j] = dew_depression(q.v[j], T.v[j], p);
          es.store(a.dew + (int64_t)b * a.dew_bs + lev * P + pix);
        }
      }
      if (cx < 0) continue;     // winds switched off
    }
    {
      const int kx = a.kind[cx], ky = a.kind[cy], kz = a.kind[cz];
      const float mx = a.p0[cx], sx = a.p1[cx], my = a.p0[cy], sy = a.p1[cy], mz = a.p0[cz], sz = a.p1[cz];
      wx.load(src + cx * P);
      wy.load(src + cy * P);
      wz.load(src + cz * P);
#pragma unroll
      for (int j = 0; j < V; ++j) {
        wx.v[j] = denorm(wx.v[j], kx, mx, sx, a.eps_q);
        wy.v[j] = denorm(wy.v[j], ky, my, sy, a.eps_q);
        wz.v[j] = denorm(wz.v[j], kz, mz, sz, a.eps_q);
      }
    }
    const double pg = type == U_LEVEL ? a.plev[un[6]] * 100.0 * 9.80616 : 0.0;
    Vec<V> ou, ov, ow;
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const double slo = slon_t[x0 + j], clo = clon_t[x0 + j];
      // (wind_z_10m keeps its de-normalised Cartesian value; T is read for a level only)
      spherical_wind(wx.v[j], wy.v[j], wz.v[j], type == U_LEVEL ? T.v[j] : 0.f, type == U_LEVEL, pg, sla, cla, slo,
                     clo, ou.v[j], ov.v[j], ow.v[j]);
    }
    ou.store(dst + cx * P);
    ov.store(dst + cy * P);
    ow.store(dst + cz * P);
  }
}

}  // namespace

extern "C" int paradis_forecast_post(const float* output, int64_t out_bs, float* chunk, int64_t chunk_bs,
                                     int64_t chunk_off, float* dew, int64_t dew_bs, int64_t dew_off,
                                     const int* kind, const float* p0, const float* p1, float eps_q,
                                     const int* units, int n_units, const double* plev, int n_levels,
                                     const double* trig, int B, int C, int H, int W, void* stream) {
  PD_REQUIRE(B >= 0 && C >= 1 && H >= 1 && W >= 1, "forecast_post: bad shape B=%d C=%d H=%d W=%d", B, C, H, W);
  PD_REQUIRE(n_units >= 1 && n_units <= C && n_levels >= 0 && n_levels <= C,
             "forecast_post: %d units / %d levels for %d channels", n_units, n_levels, C);
  const int64_t P = (int64_t)H * W;
  PD_REQUIRE(P * C < (1ll << 31), "forecast_post: a state of %d x %d x %d cells is too large", C, H, W);
  PD_REQUIRE(out_bs >= P * C && chunk_bs >= P * C && chunk_off >= 0,
             "forecast_post: batch strides shorter than one state");
  PD_REQUIRE(dew == nullptr || (n_levels >= 1 && dew_bs >= P * n_levels && dew_off >= 0),
             "forecast_post: dew-point output needs levels and a batch stride of at least L*H*W");
  if (B == 0) return 0;
  PD_REQUIRE(output && chunk && kind && p0 && p1 && units && trig && (n_levels == 0 || plev),
             "forecast_post: null pointer");
  PostArgs a;
  a.in = output;
  a.out = chunk + chunk_off;
  a.dew = dew ? dew + dew_off : nullptr;
  a.kind = kind; a.p0 = p0; a.p1 = p1; a.units = units; a.plev = plev; a.trig = trig;
  a.in_bs = out_bs; a.out_bs = chunk_bs; a.dew_bs = dew_bs;
  a.eps_q = eps_q;
  a.n_units = n_units; a.B = B; a.H = H; a.W = W;
  const bool vec = (W % 4 == 0) && aligned16(a.in) && aligned16(a.out) && (out_bs % 4 == 0) && (chunk_bs % 4 == 0) &&
                   (a.dew == nullptr || (aligned16(a.dew) && dew_bs % 4 == 0));
  const int64_t total = (int64_t)B * n_units * H * (vec ? W / 4 : W);
  const unsigned blocks = (unsigned)(ceil_div64(total, 256) < 2048 ? ceil_div64(total, 256) : 2048);
  if (vec) hipLaunchKernelGGL(forecast_post_kernel<4>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(forecast_post_kernel<1>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, a);
  PD_CHECK_LAUNCH("forecast_post");
  return 0;
}
