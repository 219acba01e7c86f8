// a11 / a14: resampling on the virtual geocyclic halo (no padded tensor is materialised).
//
//   avgpool_geo  : 5x5 box mean with stride (reference model/blocks.py:57-71)
//   upsample_lonp: lon-periodic bilinear, align_corners=True (reference model/paradis.py:208-220)
//
// Streaming kernels, one thread per output; they share nothing with the depthwise stencil but common.h.
#include <algorithm>
#include "common.h"

namespace {

// ---------------------------------------------------------------------------- avgpool
__global__ void __launch_bounds__(256)
avgpool_geo_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, int64_t planes, int H,
                       int W, int Ho, int Wo, int s) {
  const int64_t per = (int64_t)Ho * Wo, total = planes * per;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total;
       idx += (int64_t)gridDim.x * 256) {
    const int64_t plane = idx / per;
    const int rem = (int)(idx - plane * per);
    const int oy = rem / Wo, ox = rem - oy * Wo;
    const float* xp = x + plane * (int64_t)H * W;
    float sum = 0.f;
    for (int a = 0; a < 5; ++a)
      for (int b = 0; b < 5; ++b) {
        int r, c;
        geo_src(oy * s + a - 2, ox * s + b - 2, H, W, r, c);
        sum += xp[(int64_t)r * W + c];
      }
    y[idx] = sum / 25.0f;
  }
}

__global__ void __launch_bounds__(256)
avgpool_geo_bwd_kernel(const float* __restrict__ gy, float* __restrict__ gx, int64_t planes, int H,
                       int W, int Ho, int Wo, int s) {
  const int64_t per = (int64_t)H * W, total = planes * per;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total;
       idx += (int64_t)gridDim.x * 256) {
    const int64_t plane = idx / per;
    const int rem = (int)(idx - plane * per);
    const int yy = rem / W, xx = rem - yy * W;
    const float* g = gy + plane * (int64_t)Ho * Wo;
    float acc = 0.f;
    geo_for_each_alias(yy, xx, H, W, 2, [&](int ii, int jj) {
      const int r = ii + 2, c = jj + 2;  // padded coordinates
      // windows [o*s, o*s+4] covering r / c
      int oy_lo = (r - 4 + s - 1) / s; if (r - 4 < 0) oy_lo = 0;
      int ox_lo = (c - 4 + s - 1) / s; if (c - 4 < 0) ox_lo = 0;
      const int oy_hi = min(r / s, Ho - 1), ox_hi = min(c / s, Wo - 1);
      for (int oy = oy_lo; oy <= oy_hi; ++oy)
        for (int ox = ox_lo; ox <= ox_hi; ++ox) acc += g[(int64_t)oy * Wo + ox];
    });
    gx[idx] = acc / 25.0f;
  }
}

// ---------------------------------------------------------------------------- upsample
struct Lerp { int i0, i1; float l0, l1; };
__device__ __forceinline__ Lerp lerp_index(int o, int in_size, int out_size) {
  Lerp L;
  if (in_size == out_size) { L.i0 = L.i1 = o; L.l0 = 1.f; L.l1 = 0.f; return L; }
  const float scale = out_size > 1 ? (float)(in_size - 1) / (float)(out_size - 1) : 0.f;
  const float real = scale * (float)o;
  L.i0 = (int)real;
  L.i1 = L.i0 + ((L.i0 < in_size - 1) ? 1 : 0);
  L.l1 = fminf(fmaxf(real - (float)L.i0, 0.f), 1.f);
  L.l0 = 1.f - L.l1;
  return L;
}

__global__ void __launch_bounds__(256)
upsample_lonp_kernel(const float* __restrict__ src, float* __restrict__ dst, int64_t planes, int Hc,
                     int Wc, int H, int W) {
  // src = coarse x, dst = fine y   (the adjoint is the gather kernel below)
  const int64_t per = (int64_t)H * W, total = planes * per;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total;
       idx += (int64_t)gridDim.x * 256) {
    const int64_t plane = idx / per;
    const int rem = (int)(idx - plane * per);
    const int h = rem / W, w = rem - h * W;
    const Lerp lh = lerp_index(h, Hc, H);
    const Lerp lw = lerp_index(w, Wc + 1, W + 1);  // periodic column appended on both sides
    const int c0 = lw.i0 >= Wc ? lw.i0 - Wc : lw.i0, c1 = lw.i1 >= Wc ? lw.i1 - Wc : lw.i1;
    const int64_t base = plane * (int64_t)Hc * Wc;
    const float* xp = src + base;
    const float top = lw.l0 * xp[(int64_t)lh.i0 * Wc + c0] + lw.l1 * xp[(int64_t)lh.i0 * Wc + c1];
    const float bot = lw.l0 * xp[(int64_t)lh.i1 * Wc + c0] + lw.l1 * xp[(int64_t)lh.i1 * Wc + c1];
    dst[idx] = lh.l0 * top + lh.l1 * bot;
  }
}

// Adjoint of the upsampling as a GATHER (round 4; rounds 1-3 scattered four float atomics per fine point): a thread
// owns one coarse cell and walks the fine points that can reference it - a conservative index range per axis, each
// candidate re-evaluated with the forward's own lerp_index, so no inverse of the float index map is needed.  No
// atomics, no zero fill, one fixed summation order: bitwise reproducible.
__global__ void __launch_bounds__(256)
upsample_lonp_bwd_gather_kernel(const float* __restrict__ gy, float* __restrict__ gx, int64_t planes, int Hc, int Wc,
                                int H, int W) {
  const int64_t per = (int64_t)Hc * Wc, total = planes * per;
  const float inv_h = Hc > 1 ? (float)(H - 1) / (float)(Hc - 1) : 0.f;     // fine rows per coarse row
  const float inv_w = (float)W / (float)Wc;                                  // fine columns per coarse column
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
    const int64_t plane = idx / per;
    const int rem = (int)(idx - plane * per);
    const int hc = rem / Wc, wc = rem - hc * Wc;
    const float* g = gy + plane * (int64_t)H * W;
    const int h_lo = Hc > 1 ? max(0, (int)floorf((float)(hc - 1) * inv_h) - 1) : 0;
    const int h_hi = Hc > 1 ? min(H - 1, (int)ceilf((float)(hc + 1) * inv_h) + 1) : H - 1;
    float acc = 0.f;
    for (int h = h_lo; h <= h_hi; ++h) {
      const Lerp lh = lerp_index(h, Hc, H);
      const float wh = (lh.i0 == hc ? lh.l0 : 0.f) + (lh.i1 == hc ? lh.l1 : 0.f);
      if (wh == 0.f) continue;
      float rowacc = 0.f;
      // two candidate ranges of fine columns: around the coarse column, and - column 0 only - the end of the
      // circle, whose right neighbour is the appended periodic column
      for (int part = 0; part < 2; ++part) {
        int w_lo, w_hi;
        if (part == 0) {
          w_lo = max(0, (int)floorf((float)(wc - 1) * inv_w) - 1);
          w_hi = min(W - 1, (int)ceilf((float)(wc + 1) * inv_w) + 1);
        } else {
          if (wc != 0) break;
          w_lo = max(0, (int)floorf((float)(Wc - 1) * inv_w) - 1);
          w_hi = W - 1;
          const int first_hi = min(W - 1, (int)ceilf(inv_w) + 1);      // (do not visit a column twice)
          w_lo = max(w_lo, first_hi + 1);
        }
        for (int w = w_lo; w <= w_hi; ++w) {
          const Lerp lw = lerp_index(w, Wc + 1, W + 1);
          const int c0 = lw.i0 >= Wc ? lw.i0 - Wc : lw.i0, c1 = lw.i1 >= Wc ? lw.i1 - Wc : lw.i1;
          const float ww = (c0 == wc ? lw.l0 : 0.f) + (c1 == wc ? lw.l1 : 0.f);
          if (ww != 0.f) rowacc = fmaf(g[(int64_t)h * W + w], ww, rowacc);
        }
      }
      acc = fmaf(rowacc, wh, acc);
    }
    gx[idx] = acc;
  }
}

}  // namespace

static int check_pool(const char* name, int64_t planes, int H, int W, int s) {
  PD_REQUIRE(planes >= 0 && H >= 4 && W >= 4 && W % 2 == 0, "%s: bad shape %dx%d", name, H, W);
  PD_REQUIRE(s >= 1, "%s: Coarsening factor must be >=1", name);
  return 0;
}

extern "C" int paradis_avgpool_geo_fwd(const float* x, float* y, int64_t planes, int H, int W,
                                       int stride, void* stream) {
  if (int e = check_pool("avgpool_geo_fwd", planes, H, W, stride)) return e;
  if (planes == 0) return 0;
  const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
  const int64_t total = planes * Ho * Wo;
  const int blocks = (int)std::min<int64_t>(ceil_div64(total, 256), 256 * 32);
  hipLaunchKernelGGL(avgpool_geo_fwd_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, x, y,
                     planes, H, W, Ho, Wo, stride);
  PD_CHECK_LAUNCH("avgpool_geo_fwd");
  return 0;
}

extern "C" int paradis_avgpool_geo_bwd(const float* gy, float* gx, int64_t planes, int H, int W,
                                       int stride, void* stream) {
  if (int e = check_pool("avgpool_geo_bwd", planes, H, W, stride)) return e;
  if (planes == 0) return 0;
  const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
  const int64_t total = planes * H * W;
  const int blocks = (int)std::min<int64_t>(ceil_div64(total, 256), 256 * 32);
  hipLaunchKernelGGL(avgpool_geo_bwd_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, gy, gx,
                     planes, H, W, Ho, Wo, stride);
  PD_CHECK_LAUNCH("avgpool_geo_bwd");
  return 0;
}

extern "C" int paradis_upsample_lonp_fwd(const float* x, float* y, int64_t planes, int Hc, int Wc,
                                         int H, int W, void* stream) {
  PD_REQUIRE(planes >= 0 && Hc >= 1 && Wc >= 1 && H >= Hc && W >= Wc, "upsample_lonp_fwd: bad shape");
  if (planes == 0) return 0;
  const int64_t total = planes * H * W;
  const int blocks = (int)std::min<int64_t>(ceil_div64(total, 256), 256 * 32);
  hipLaunchKernelGGL(upsample_lonp_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, x, y,
                     planes, Hc, Wc, H, W);
  PD_CHECK_LAUNCH("upsample_lonp_fwd");
  return 0;
}

extern "C" int paradis_upsample_lonp_bwd(const float* gy, float* gx, int64_t planes, int Hc, int Wc,
                                         int H, int W, void* stream) {
  PD_REQUIRE(planes >= 0 && Hc >= 1 && Wc >= 1 && H >= Hc && W >= Wc, "upsample_lonp_bwd: bad shape");
  if (planes == 0) return 0;
  const int64_t total = planes * Hc * Wc;
  const int blocks = (int)std::min<int64_t>(ceil_div64(total, 256), 256 * 32);
  hipLaunchKernelGGL(upsample_lonp_bwd_gather_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, gy, gx,
                     planes, Hc, Wc, H, W);
  PD_CHECK_LAUNCH("upsample_lonp_bwd");
  return 0;
}
