// Global-norm gradient clipping over many tensors - torch.nn.utils.clip_grad_norm_(params, max_norm, norm_type=2.0,
// error_if_nonfinite=False) as the reference applies it between the last backward of an accumulation window and the
// optimiser step (train.py:52-53, algorithm "norm") - in three launches (ATen's foreach path: 18 device activities over the
// default model's 335 gradients, measured), and with fewer roundings: the sum of squares is formed in double.
//
// Layout, thread order, chunk table and block fold: stream_common.h.  What is particular here:
// Launch 1, clip_partial_kernel: one sum per chunk, the squares of one gradient, in DOUBLE from the first product on (the
// product of two fp32 values is exact in fp64, so only the additions round); a gradient address of 0 means "absent":
// partial[b] = 0.
// Launch 2, clip_finish_kernel: one workgroup; thread t adds partial[t], partial[t + 1024], .. in double, the shuffle tree,
// the 16 wave sums in wave order; out = {(float)sqrt(S), the clip coefficient}.
// Launch 3, clip_scale_kernel: the chunks of launch 1 again; g *= out[1], one fp32 multiply per element; a coefficient of
// exactly 1.0f returns at once (g * 1.0f is the same bits, NaN payloads aside, and a NaN norm gives a NaN coefficient).
// Algorithmic HBM bytes: 4 per element (norm pass) + 8 per element (scale pass, when it clips).
#include "common.h"
#include "stream_common.h"

#include <cmath>

#pragma clang fp contract(off)

namespace {

constexpr int CLIP_FIN_THREADS = 1024, CLIP_FIN_WAVES = CLIP_FIN_THREADS / 64;

// the gradient's part of chunk c (nullptr, and c.n = 0, for an absent gradient)
__device__ __forceinline__ float* clip_chunk(const int64_t* __restrict__ grads, TableChunk& c) {
  if (c.n == 0) return nullptr;
  const int64_t ga = grads[c.t];
  if (ga == 0) {
    c.n = 0;
    return nullptr;
  }
  return reinterpret_cast<float*>(ga) + c.off;
}

__global__ void __launch_bounds__(256)
clip_partial_kernel(const int64_t* __restrict__ grads, const int64_t* __restrict__ numel,
                    const int* __restrict__ chunk_tensor, const int64_t* __restrict__ chunk_off, int T,
                    double* __restrict__ partial /* [n_chunks] */) {
  TableChunk c = table_chunk(numel, chunk_tensor, chunk_off, T);
  const float* __restrict__ g = clip_chunk(grads, c);
  const int n = c.n;
  double s[1] = {0.0};
  if (n > 0) {       // (workgroup-uniform)
    s[0] = walk_chunk(aligned16(g), n, 0.0, [&](auto vec, double a, int q0) {
      float v[4];
      load_quad<decltype(vec)::value>(g, q0, n, v);
#pragma unroll
      for (int k = 0; k < 4; ++k) a += (double)v[k] * (double)v[k];
      return a;
    });
  }
  s[0] = wave_sum_f64(s[0]);
  block_fold4(s, [&](int, double v) { partial[blockIdx.x] = v; });
}

__global__ void __launch_bounds__(CLIP_FIN_THREADS)
clip_finish_kernel(const double* __restrict__ partial, int n_chunks, double max_norm, float* __restrict__ out) {
  __shared__ double red[CLIP_FIN_WAVES];
  double a = 0.0;
  for (int i = threadIdx.x; i < n_chunks; i += CLIP_FIN_THREADS) a += partial[i];
  a = wave_sum_f64(a);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
  __syncthreads();
  if (threadIdx.x == 0) {
    double S = 0.0;
    for (int w = 0; w < CLIP_FIN_WAVES; ++w) S += red[w];
    const double norm = sqrt(S);
    const double c = max_norm / (norm + 1e-6);
    out[0] = (float)norm;
    out[1] = (float)(c < 1.0 ? c : (c != c ? c : 1.0));      // a NaN norm gives a NaN coefficient, as torch.clamp does
  }
}

__global__ void __launch_bounds__(256)
clip_scale_kernel(const int64_t* __restrict__ grads, const int64_t* __restrict__ numel,
                  const int* __restrict__ chunk_tensor, const int64_t* __restrict__ chunk_off, int T,
                  const float* __restrict__ out) {
  const float coef = out[1];
  if (coef == 1.0f) return;       // (workgroup-uniform) nothing to clip: g * 1.0f is g
  TableChunk c = table_chunk(numel, chunk_tensor, chunk_off, T);
  float* g = clip_chunk(grads, c);
  const int n = c.n;
  if (n == 0) return;
  walk_chunk(aligned16(g), n, NoSums{}, [&](auto vec, NoSums a, int q0) {
    if (decltype(vec)::value) {
      float4 q = *reinterpret_cast<const float4*>(g + q0);
      q.x *= coef; q.y *= coef; q.z *= coef; q.w *= coef;
      *reinterpret_cast<float4*>(g + q0) = q;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (q0 + k < n) g[q0 + k] *= coef;
    }
    return a;
  });
}

}  // namespace

extern "C" int paradis_clip_grad_chunk(void) { return TABLE_CHUNK; }

// the partials [n_chunks] in double
extern "C" size_t paradis_clip_grad_ws_bytes(int n_chunks) {
  if (n_chunks < 0) return 0;
  return (size_t)n_chunks * sizeof(double);
}

extern "C" int paradis_clip_grad_norm(const int64_t* grads, const int64_t* numel, const int* chunk_tensor,
                                      const int64_t* chunk_off, int n_tensors, int n_chunks, double max_norm,
                                      void* workspace, float* out, void* stream) {
  PD_REQUIRE(std::isfinite(max_norm) && max_norm > 0.0, "clip_grad_norm: max_norm must be finite and > 0, got %g",
             max_norm);
  PD_REQUIRE(n_tensors >= 0 && n_chunks >= 0, "clip_grad_norm: bad counts T=%d chunks=%d", n_tensors, n_chunks);
  PD_REQUIRE(out != nullptr, "clip_grad_norm: result row missing");
  PD_REQUIRE(n_chunks == 0 || (grads && numel && chunk_tensor && chunk_off), "clip_grad_norm: tables missing");
  PD_REQUIRE(n_chunks == 0 || n_tensors >= 1, "clip_grad_norm: %d chunks of no tensor", n_chunks);
  PD_REQUIRE(n_chunks == 0 || workspace != nullptr, "clip_grad_norm: workspace missing");
  hipStream_t st = (hipStream_t)stream;
  double* partial = static_cast<double*>(workspace);
  if (n_chunks > 0)
    hipLaunchKernelGGL(clip_partial_kernel, dim3(n_chunks), dim3(256), 0, st, grads, numel, chunk_tensor, chunk_off,
                       n_tensors, partial);
  hipLaunchKernelGGL(clip_finish_kernel, dim3(1), dim3(CLIP_FIN_THREADS), 0, st, partial, n_chunks, max_norm, out);
  if (n_chunks > 0)
    hipLaunchKernelGGL(clip_scale_kernel, dim3(n_chunks), dim3(256), 0, st, grads, numel, chunk_tensor, chunk_off,
                       n_tensors, out);
  PD_CHECK_LAUNCH("clip_grad_norm");
  return 0;
}
