// Global-norm gradient clipping over many tensors - torch.nn.utils.clip_grad_norm_(params, max_norm, norm_type=2.0,
// error_if_nonfinite=False) as the reference applies it between the last backward of an accumulation window and the
// optimiser step (train.py:52-53, algorithm "norm") - in three launches (ATen's foreach path: 18 device activities over the
// default model's 335 gradients, measured), and with fewer roundings: the sum of squares is formed in double.
//
// Launch 1, clip_partial_kernel: workgroup b works on chunk b = (tensor, offset) of the table scheme of adamw_multi_kernel
// (train.hip) and param_stats_kernel (stats.hip): at most CLIP_CHUNK elements of one gradient, read once; a gradient
// address of 0 means "absent".  Thread t adds cells 4 (256 i + t) .. + 3, i = 0 .., in that order, in DOUBLE: the product
// of two fp32 values is exact in fp64, so only the additions round.  One 16-byte load per quad where the chunk start is
// 16-byte aligned, four scalar loads otherwise (DDP's bucket views are often only 4-byte aligned): the same bits either
// way.  Waves by shuffles, the four waves through LDS, one ordinary store per workgroup: partial[b].
// Launch 2, clip_finish_kernel: one workgroup; thread t adds partial[t], partial[t + 1024], .. in double, the shuffle tree,
// the 16 wave sums in wave order; out = {(float)sqrt(S), the clip coefficient}.  No atomics: bit-identical run to run.
// Launch 3, clip_scale_kernel: the chunks of launch 1 again; g *= out[1], one fp32 multiply per element; a coefficient of
// exactly 1.0f returns at once (g * 1.0f is the same bits, NaN payloads aside, and a NaN norm gives a NaN coefficient).
// Algorithmic HBM bytes: 4 per element (norm pass) + 8 per element (scale pass, when it clips).
#include "common.h"

#include <cmath>

#pragma clang fp contract(off)

namespace {

constexpr int CLIP_CHUNK = 32768;                        // elements of one tensor per workgroup: 32 quads per thread
constexpr int CLIP_ITERS = CLIP_CHUNK / (256 * 4);
constexpr int CLIP_FIN_THREADS = 1024, CLIP_FIN_WAVES = CLIP_FIN_THREADS / 64;

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// chunk b of the table: its first element (nullptr: nothing to do) and its length n; a bad table entry and an absent
// gradient give nothing (workgroup-uniform)
__device__ __forceinline__ float* clip_chunk(const int64_t* __restrict__ grads, const int64_t* __restrict__ numel,
                                             const int* __restrict__ chunk_tensor, const int64_t* __restrict__ chunk_off,
                                             int T, int& n) {
  const int t = chunk_tensor[blockIdx.x];
  const int64_t off = chunk_off[blockIdx.x];
  const int64_t left = (t >= 0 && t < T && off >= 0) ? numel[t] - off : 0;
  n = (int)(left < (int64_t)CLIP_CHUNK ? (left > 0 ? left : 0) : (int64_t)CLIP_CHUNK);
  if (n == 0) return nullptr;
  const int64_t ga = grads[t];
  if (ga == 0) {
    n = 0;
    return nullptr;
  }
  return reinterpret_cast<float*>(ga) + off;
}

// VEC: the quad is whole and 16-byte aligned
template <bool VEC>
__device__ __forceinline__ double sum_squares(const float* __restrict__ g, int first, int last, int n, double s) {
  // (the loop vectorizer would interleave two iterations and break the 16-byte accesses into 4-byte ones)
#pragma clang loop vectorize(disable) interleave(disable) unroll_count(4)
  for (int i = first; i < last; ++i) {
    const int q0 = 4 * (256 * i + (int)threadIdx.x);
    if (q0 >= n) break;
    float v[4];
    if (VEC) {
      const float4 q = *reinterpret_cast<const float4*>(g + q0);
      v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
      // cells past the end are +0: a sum that starts at +0 is never -0, so adding them changes no bit
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = q0 + k < n ? g[q0 + k] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) s += (double)v[k] * (double)v[k];
  }
  return s;
}

__global__ void __launch_bounds__(256)
clip_partial_kernel(const int64_t* __restrict__ grads, const int64_t* __restrict__ numel,
                    const int* __restrict__ chunk_tensor, const int64_t* __restrict__ chunk_off, int T,
                    double* __restrict__ partial /* [n_chunks] */) {
  __shared__ double red[4];
  int n;
  const float* g = clip_chunk(grads, numel, chunk_tensor, chunk_off, T, n);
  double s = 0.0;
  if (n > 0) {       // (workgroup-uniform)
    const int whole = aligned16(g) ? n / 1024 : 0;      // iterations whose 256 quads are all whole: 1024 cells each
    s = sum_squares<true>(g, 0, whole, n, s);
    s = sum_squares<false>(g, whole, CLIP_ITERS, n, s);
  }
  s = wave_sum_f64(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
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

template <bool VEC>
__device__ __forceinline__ void scale_quads(float* __restrict__ g, int first, int last, int n, float c) {
  // (the loop vectorizer would interleave two iterations and break the 16-byte accesses into 4-byte ones)
#pragma clang loop vectorize(disable) interleave(disable) unroll_count(4)
  for (int i = first; i < last; ++i) {
    const int q0 = 4 * (256 * i + (int)threadIdx.x);
    if (q0 >= n) break;
    if (VEC) {
      float4 q = *reinterpret_cast<const float4*>(g + q0);
      q.x *= c; q.y *= c; q.z *= c; q.w *= c;
      *reinterpret_cast<float4*>(g + q0) = q;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (q0 + k < n) g[q0 + k] *= c;
    }
  }
}

__global__ void __launch_bounds__(256)
clip_scale_kernel(const int64_t* __restrict__ grads, const int64_t* __restrict__ numel,
                  const int* __restrict__ chunk_tensor, const int64_t* __restrict__ chunk_off, int T,
                  const float* __restrict__ out) {
  const float c = out[1];
  if (c == 1.0f) return;       // (workgroup-uniform) nothing to clip: g * 1.0f is g
  int n;
  float* g = clip_chunk(grads, numel, chunk_tensor, chunk_off, T, n);
  if (n == 0) return;
  const int whole = aligned16(g) ? n / 1024 : 0;
  scale_quads<true>(g, 0, whole, n, c);
  scale_quads<false>(g, whole, CLIP_ITERS, n, c);
}

}  // namespace

extern "C" int paradis_clip_grad_chunk(void) { return CLIP_CHUNK; }

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
