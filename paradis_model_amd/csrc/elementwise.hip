// The elementwise / reduction glue of the ADR layer step around the GEMMs (reference model/paradis.py:239-253):
// activation, add, transpose, gated blend, bias grads.  All HBM-bound streaming kernels (float4 where alignment allows).
#include <algorithm>
#include "common.h"

namespace {

// ------------------------------------------------------------------ activation
// O16 (round 6, bf16-mixed mode, BWD only): out is a bf16 tensor - d(pre-activation) for the layer's two gradient GEMMs, which
// round that operand to bf16 (to nearest even, as here) when they load it from fp32 words: same values, half the bytes thrice.
template <bool BWD, bool O16 = false>
__global__ void __launch_bounds__(256)
act_kernel(const float* __restrict__ gy, const float* __restrict__ x, float* __restrict__ out,
           int64_t n, int act, bool vec) {
  if constexpr (O16) {
    const int64_t n4 = n >> 2;      // (the host checks n % 4 == 0 and the alignment)
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
      const float4 v = reinterpret_cast<const float4*>(x)[i], g = reinterpret_cast<const float4*>(gy)[i];
      const float o[4] = {g.x * act_grad(v.x, act), g.y * act_grad(v.y, act), g.z * act_grad(v.z, act), g.w * act_grad(v.w, act)};
      uint2 r;
      r.x = (uint32_t)__builtin_bit_cast(uint16_t, (__bf16)o[0]) | ((uint32_t)__builtin_bit_cast(uint16_t, (__bf16)o[1]) << 16);
      r.y = (uint32_t)__builtin_bit_cast(uint16_t, (__bf16)o[2]) | ((uint32_t)__builtin_bit_cast(uint16_t, (__bf16)o[3]) << 16);
      reinterpret_cast<uint2*>(out)[i] = r;
    }
    return;
  }
  if (vec) {
    const int64_t n4 = n >> 2;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
      const float4 v = reinterpret_cast<const float4*>(x)[i];
      float4 o;
      if (BWD) {
        const float4 g = reinterpret_cast<const float4*>(gy)[i];
        o = make_float4(g.x * act_grad(v.x, act), g.y * act_grad(v.y, act), g.z * act_grad(v.z, act),
                        g.w * act_grad(v.w, act));
      } else {
        o = make_float4(act_apply(v.x, act), act_apply(v.y, act), act_apply(v.z, act), act_apply(v.w, act));
      }
      reinterpret_cast<float4*>(out)[i] = o;
    }
  } else {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
      const float o = BWD ? gy[i] * act_grad(x[i], act) : act_apply(x[i], act);
      out[i] = o;
    }
  }
}

__global__ void __launch_bounds__(256)
add_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ y, int64_t n,
           bool vec) {
  if (vec) {
    const int64_t n4 = n >> 2;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
      const float4 u = reinterpret_cast<const float4*>(a)[i], v = reinterpret_cast<const float4*>(b)[i];
      reinterpret_cast<float4*>(y)[i] = make_float4(u.x + v.x, u.y + v.y, u.z + v.z, u.w + v.w);
    }
  } else {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
      y[i] = a[i] + b[i];
  }
}

// y[b, i] = x[b, i] + m[i]   (standalone GlobalBias.forward, reference model/blocks.py:196)
__global__ void __launch_bounds__(256)
add_bcast_kernel(const float* __restrict__ x, const float* __restrict__ m, float* __restrict__ y,
                 int64_t per, int64_t total) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256)
    y[i] = x[i] + m[i % per];
}

// out[c][r] = in[r][c]  (32x32 tiles through LDS; used once per forward per weight matrix)
__global__ void __launch_bounds__(256)
transpose_kernel(const float* __restrict__ in, float* __restrict__ out, int rows, int cols) {
  __shared__ float tile[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 32 x 8
  const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
  for (int i = ty; i < 32; i += 8)
    if (r0 + i < rows && c0 + tx < cols) tile[i][tx] = in[(int64_t)(r0 + i) * cols + c0 + tx];
  __syncthreads();
  for (int i = ty; i < 32; i += 8)
    if (c0 + i < cols && r0 + tx < rows) out[(int64_t)(c0 + i) * rows + r0 + tx] = tile[tx][i];
}

// ------------------------------------------------------------------ gated blend
__global__ void __launch_bounds__(256)
gated_blend_fwd_kernel(const float* __restrict__ h, const float* __restrict__ adv,
                       const float* __restrict__ alpha, float* __restrict__ out, int C, int P) {
  // one workgroup per (b,c) plane
  const int c = blockIdx.x % C;
  const float g = 1.0f / (1.0f + expf(-alpha[c]));
  const int64_t base = (int64_t)blockIdx.x * P;
  for (int p = threadIdx.x; p < P; p += 256) {
    const float hv = h[base + p];
    out[base + p] = fmaf(g, adv[base + p] - hv, hv);     // (the GEMM epilogue's gated form computes the same bits)
  }
}

__global__ void __launch_bounds__(256)
gated_blend_bwd_kernel(const float* __restrict__ gout, const float* __restrict__ h,
                       const float* __restrict__ adv, const float* __restrict__ alpha,
                       float* __restrict__ gh, float* __restrict__ gadv, float* __restrict__ partial,
                       int C, int P) {
  __shared__ float red[4];
  const int c = blockIdx.x % C;
  const float g = 1.0f / (1.0f + expf(-alpha[c]));
  const int64_t base = (int64_t)blockIdx.x * P;
  float acc = 0.f;
  for (int p = threadIdx.x; p < P; p += 256) {
    const float go = gout[base + p];
    gh[base + p] = (1.0f - g) * go;
    gadv[base + p] = g * go;
    acc += go * (adv[base + p] - h[base + p]);
  }
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

// from_out: the partial sums were taken against the blended OUTPUT, sum gout (out - h) = sigmoid sum gout (adv - h)
__global__ void __launch_bounds__(256)
gated_blend_finish(const float* __restrict__ partial, const float* __restrict__ alpha,
                   float* __restrict__ galpha, int B, int C, int from_out) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  float s = 0.f;
  for (int b = 0; b < B; ++b) s += partial[(int64_t)b * C + c];
  const float g = 1.0f / (1.0f + expf(-alpha[c]));
  galpha[c] = from_out ? s * (1.0f - g) : s * g * (1.0f - g);
}

// ------------------------------------------------------------------ bias / bias-map gradients
// grid (C, pchunks): gmap[c,p] = sum_b dz[b,c,p];  gbias[c] += sum over the chunk
__global__ void __launch_bounds__(256)
bias_grads_kernel(const float* __restrict__ dz, float* __restrict__ gmap, float* __restrict__ gbias,
                  int B, int C, int P, int64_t bs, int pchunks) {
  __shared__ float red[4];
  const int c = blockIdx.x / pchunks, chunk = blockIdx.x - c * pchunks;
  float acc = 0.f;
  for (int p = chunk * 256 + threadIdx.x; p < P; p += pchunks * 256) {
    float s = 0.f;
    for (int b = 0; b < B; ++b) s += dz[(int64_t)b * bs + (int64_t)c * P + p];
    if (gmap) gmap[(int64_t)c * P + p] = s;
    acc += s;
  }
  if (!gbias) return;
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) atomicAdd(&gbias[c], red[0] + red[1] + red[2] + red[3]);
}

// the same with 16-byte accesses (P % 4 == 0, 16-byte aligned rows): grid (C, pchunks) over float4 columns
__global__ void __launch_bounds__(256)
bias_grads_vec4_kernel(const float* __restrict__ dz, float* __restrict__ gmap, float* __restrict__ gbias,
                       int B, int C, int P4, int64_t bs, int pchunks) {
  __shared__ float red[4];
  const int c = blockIdx.x / pchunks, chunk = blockIdx.x - c * pchunks;
  const float4* src = reinterpret_cast<const float4*>(dz + (int64_t)c * P4 * 4);
  const int64_t bs4 = bs / 4;
  float acc = 0.f;
  for (int q = chunk * 256 + threadIdx.x; q < P4; q += pchunks * 256) {
    float4 s = {0.f, 0.f, 0.f, 0.f};
    int b = 0;
    for (; b + 8 <= B; b += 8) {     // eight independent loads in flight, summed in batch order
      float4 v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = src[(int64_t)(b + j) * bs4 + q];
#pragma unroll
      for (int j = 0; j < 8; ++j) { s.x += v[j].x; s.y += v[j].y; s.z += v[j].z; s.w += v[j].w; }
    }
    for (; b < B; ++b) {
      const float4 v = src[(int64_t)b * bs4 + q];
      s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
    if (gmap) reinterpret_cast<float4*>(gmap + (int64_t)c * P4 * 4)[q] = s;
    acc += (s.x + s.y) + (s.z + s.w);
  }
  if (!gbias) return;
  acc = wave_sum_dpp(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) atomicAdd(&gbias[c], red[0] + red[1] + red[2] + red[3]);
}

}  // namespace

// (outside the unnamed namespace as it always was: its symbols are part of the library's dynamic table)
// bias / bias-map gradients on a bf16-STORED dz (bf16-mixed mode, round 6): eight columns per thread from one 16-byte load per sample
// (P % 8 == 0, 16-byte aligned rows); fp32 sums in batch order, fp32 outputs
__global__ void __launch_bounds__(256)
bias_grads_b16_kernel(const uint16_t* __restrict__ dz, float* __restrict__ gmap, float* __restrict__ gbias,
                      int B, int C, int P8, int64_t bs, int pchunks) {
  __shared__ float red[4];
  const int c = blockIdx.x / pchunks, chunk = blockIdx.x - c * pchunks;
  const uint4* src = reinterpret_cast<const uint4*>(dz + (int64_t)c * P8 * 8);
  const int64_t bs8 = bs / 8;
  float acc = 0.f;
  for (int q = chunk * 256 + threadIdx.x; q < P8; q += pchunks * 256) {
    float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int b0 = 0; b0 < B; b0 += 8) {
      uint4 v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = src[(int64_t)min(b0 + j, B - 1) * bs8 + q];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        if (b0 + j < B) {
          const uint32_t w[4] = {v[j].x, v[j].y, v[j].z, v[j].w};
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            s[2 * i] += __uint_as_float(w[i] << 16);
            s[2 * i + 1] += __uint_as_float(w[i] & 0xffff0000u);
          }
        }
      }
    }
    if (gmap) {
      float4* o = reinterpret_cast<float4*>(gmap + (int64_t)c * P8 * 8) + 2 * q;
      o[0] = make_float4(s[0], s[1], s[2], s[3]);
      o[1] = make_float4(s[4], s[5], s[6], s[7]);
    }
    acc += ((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7]));
  }
  if (!gbias) return;
  acc = wave_sum_dpp(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) atomicAdd(&gbias[c], red[0] + red[1] + red[2] + red[3]);
}

extern "C" int paradis_act_fwd(const float* x, float* y, int64_t n, int act, void* stream) {
  PD_REQUIRE(n >= 0 && act >= 0 && act <= 2, "act_fwd: bad arguments");
  if (n == 0) return 0;
  const bool vec = (n % 4 == 0) && aligned16(x) && aligned16(y);
  hipLaunchKernelGGL(act_kernel<false>, dim3(stream_blocks(vec ? n / 4 : n)), dim3(256), 0,
                     (hipStream_t)stream, nullptr, x, y, n, act, vec);
  PD_CHECK_LAUNCH("act_fwd");
  return 0;
}

extern "C" int paradis_act_bwd(const float* gy, const float* x, float* gx, int64_t n, int act, void* stream) {
  PD_REQUIRE(n >= 0 && act >= 0 && act <= 2, "act_bwd: bad arguments");
  if (n == 0) return 0;
  const bool vec = (n % 4 == 0) && aligned16(x) && aligned16(gy) && aligned16(gx);
  hipLaunchKernelGGL(act_kernel<true>, dim3(stream_blocks(vec ? n / 4 : n)), dim3(256), 0,
                     (hipStream_t)stream, gy, x, gx, n, act, vec);
  PD_CHECK_LAUNCH("act_bwd");
  return 0;
}

// gx as a bf16 tensor (ABI 9; bf16-mixed mode: gx = d(pre-activation), the operand of the layer's gradient GEMMs).  n % 4 == 0,
// 16-byte aligned gy / x, 8-byte aligned gx.
extern "C" int paradis_act_bwd16(const float* gy, const float* x, void* gx, int64_t n, int act, void* stream) {
  PD_REQUIRE(n >= 0 && act >= 0 && act <= 2, "act_bwd16: bad arguments");
  if (n == 0) return 0;
  PD_REQUIRE(n % 4 == 0 && aligned16(x) && aligned16(gy) && (reinterpret_cast<uintptr_t>(gx) & 7) == 0,
             "act_bwd16: n %% 4 == 0 and aligned tensors required");
  hipLaunchKernelGGL((act_kernel<true, true>), dim3(stream_blocks(n / 4)), dim3(256), 0, (hipStream_t)stream, gy, x,
                     (float*)gx, n, act, true);
  PD_CHECK_LAUNCH("act_bwd16");
  return 0;
}

extern "C" int paradis_add(const float* a, const float* b, float* y, int64_t n, void* stream) {
  PD_REQUIRE(n >= 0, "add: bad arguments");
  if (n == 0) return 0;
  const bool vec = (n % 4 == 0) && aligned16(a) && aligned16(b) && aligned16(y);
  hipLaunchKernelGGL(add_kernel, dim3(stream_blocks(vec ? n / 4 : n)), dim3(256), 0, (hipStream_t)stream,
                     a, b, y, n, vec);
  PD_CHECK_LAUNCH("add");
  return 0;
}

extern "C" int paradis_add_bcast(const float* x, const float* m, float* y, int64_t per_sample, int B,
                                 void* stream) {
  PD_REQUIRE(per_sample >= 1 && B >= 0, "add_bcast: bad arguments");
  if (B == 0) return 0;
  const int64_t total = per_sample * B;
  hipLaunchKernelGGL(add_bcast_kernel, dim3(stream_blocks(total)), dim3(256), 0, (hipStream_t)stream, x, m,
                     y, per_sample, total);
  PD_CHECK_LAUNCH("add_bcast");
  return 0;
}

extern "C" int paradis_transpose(const float* in, float* out, int rows, int cols, void* stream) {
  PD_REQUIRE(rows >= 1 && cols >= 1, "transpose: bad shape");
  hipLaunchKernelGGL(transpose_kernel, dim3((cols + 31) / 32, (rows + 31) / 32), dim3(256), 0,
                     (hipStream_t)stream, in, out, rows, cols);
  PD_CHECK_LAUNCH("transpose");
  return 0;
}

extern "C" int paradis_gated_blend_fwd(const float* h, const float* adv, const float* alpha,
                                       float* out, int B, int C, int P, void* stream) {
  PD_REQUIRE(B >= 0 && C >= 1 && P >= 1, "gated_blend_fwd: bad shape");
  if (B == 0) return 0;
  hipLaunchKernelGGL(gated_blend_fwd_kernel, dim3((unsigned)((int64_t)B * C)), dim3(256), 0,
                     (hipStream_t)stream, h, adv, alpha, out, C, P);
  PD_CHECK_LAUNCH("gated_blend_fwd");
  return 0;
}

extern "C" size_t paradis_gated_blend_bwd_ws_bytes(int B, int C, int P) {
  (void)P;
  return (size_t)std::max(B, 1) * C * sizeof(float) + 256;
}

static int gated_blend_bwd_impl(const float* gout, const float* h, const float* third, const float* alpha, float* gh,
                                float* gadv, float* galpha, int B, int C, int P, void* workspace, void* stream,
                                int from_out) {
  PD_REQUIRE(B >= 0 && C >= 1 && P >= 1, "gated_blend_bwd: bad shape");
  PD_REQUIRE(workspace != nullptr, "gated_blend_bwd: workspace required");
  hipStream_t st = (hipStream_t)stream;
  float* partial = (float*)workspace;
  if (B > 0)
    hipLaunchKernelGGL(gated_blend_bwd_kernel, dim3((unsigned)((int64_t)B * C)), dim3(256), 0, st, gout, h,
                       third, alpha, gh, gadv, partial, C, P);
  hipLaunchKernelGGL(gated_blend_finish, dim3((C + 255) / 256), dim3(256), 0, st, partial, alpha, galpha, B, C,
                     from_out);
  PD_CHECK_LAUNCH("gated_blend_bwd");
  return 0;
}

extern "C" int paradis_gated_blend_bwd(const float* gout, const float* h, const float* adv,
                                       const float* alpha, float* gh, float* gadv, float* galpha, int B,
                                       int C, int P, void* workspace, void* stream) {
  return gated_blend_bwd_impl(gout, h, adv, alpha, gh, gadv, galpha, B, C, P, workspace, stream, 0);
}

// The same gradients when the advected tensor was never materialised (paradis_pw_gemm_fwd_gated): `out` is the
// blended output, adv - h = (out - h) / sigmoid, so galpha = (1 - sigmoid) sum gout (out - h) - no division.
extern "C" int paradis_gated_blend_bwd_out(const float* gout, const float* h, const float* out,
                                           const float* alpha, float* gh, float* gadv, float* galpha, int B,
                                           int C, int P, void* workspace, void* stream) {
  return gated_blend_bwd_impl(gout, h, out, alpha, gh, gadv, galpha, B, C, P, workspace, stream, 1);
}

extern "C" int paradis_bias_grads(const float* dz, float* gmap, float* gbias, int B, int C, int P,
                                  int64_t dz_bs, void* stream) {
  PD_REQUIRE(B >= 0 && C >= 1 && P >= 1, "bias_grads: bad shape");
  hipStream_t st = (hipStream_t)stream;
  if (gbias && pd_zero_async(gbias, (size_t)C * sizeof(float), st) != hipSuccess) {
    paradis_set_error("bias_grads: memset failed");
    return 2;
  }
  if (!gmap && !gbias) return 0;
  if (P % 4 == 0 && dz_bs % 4 == 0 && aligned16(dz) && (!gmap || aligned16(gmap))) {
    const int P4 = P / 4;
    // at most TWO chunks per channel: their atomic adds into the zeroed gbias commute exactly (a + b = b + a), so the
    // result does not depend on which workgroup arrives first
    int pch = std::max(1, std::min(2, std::min((P4 + 255) / 256, std::max(1, 2048 / C))));
    if (paradis_deterministic()) pch = 1;
    hipLaunchKernelGGL(bias_grads_vec4_kernel, dim3((unsigned)((int64_t)C * pch)), dim3(256), 0, st, dz, gmap,
                       gbias, B, C, P4, dz_bs, pch);
    PD_CHECK_LAUNCH("bias_grads");
    return 0;
  }
  int pchunks = std::max(1, std::min(2, std::min((P + 255) / 256, std::max(1, 2048 / C))));   // (two adds commute)
  if (paradis_deterministic()) pchunks = 1;   // one workgroup per channel: no atomics between chunks
  hipLaunchKernelGGL(bias_grads_kernel, dim3((unsigned)((int64_t)C * pchunks)), dim3(256), 0, st, dz, gmap,
                     gbias, B, C, P, dz_bs, pchunks);
  PD_CHECK_LAUNCH("bias_grads");
  return 0;
}

// dz stored as bf16 [B][C,P] (bf16-mixed mode): same outputs, fp32
extern "C" int paradis_bias_grads16(const void* dz, float* gmap, float* gbias, int B, int C, int P,
                                    int64_t dz_bs, void* stream) {
  PD_REQUIRE(B >= 0 && C >= 1 && P >= 1, "bias_grads16: bad shape");
  PD_REQUIRE(P % 8 == 0 && dz_bs % 8 == 0 && aligned16(dz) && (!gmap || aligned16(gmap)),
             "bias_grads16: needs P %% 8 == 0 and 16-byte aligned rows");
  hipStream_t st = (hipStream_t)stream;
  if (gbias && pd_zero_async(gbias, (size_t)C * sizeof(float), st) != hipSuccess) {
    paradis_set_error("bias_grads16: memset failed");
    return 2;
  }
  if ((!gmap && !gbias) || B == 0) {
    if (gmap && pd_zero_async(gmap, (size_t)C * P * sizeof(float), st) != hipSuccess) return 2;
    return 0;
  }
  const int P8 = P / 8;
  int pch = std::max(1, std::min(2, std::min((P8 + 255) / 256, std::max(1, 2048 / C))));   // (two adds commute)
  if (paradis_deterministic()) pch = 1;
  hipLaunchKernelGGL(bias_grads_b16_kernel, dim3((unsigned)((int64_t)C * pch)), dim3(256), 0, st,
                     reinterpret_cast<const uint16_t*>(dz), gmap, gbias, B, C, P8, dz_bs, pch);
  PD_CHECK_LAUNCH("bias_grads16");
  return 0;
}
