// Training diagnostics - the sums behind the reference's on_before_optimizer_step (trainer.py:844-923): per parameter
// group (top-level submodule) the squared norms of the parameters, the gradients and the optimiser's first moment, and
// the gradient . moment dot product, in ONE streaming read of all tensors instead of up to four ATen reductions and four
// scalar adds per tensor (335 tensors in the default model).
//
// Layout, thread order, chunk table and block fold: stream_common.h.  What is particular here:
// Launch 1, param_stats_kernel: address rows parameter, gradient, first moment; a gradient or moment address of 0 means
// "absent" (the moment of a parameter without a gradient is skipped, as the reference skips it).  Four sums per chunk, in
// DOUBLE from the first product on (the product of two fp32 values is exact in fp64, so only the additions round):
// partial[b] = {Sp2, Sg2, Sgm, Sm2}.  16-byte loads when every present tensor's chunk start is 16-byte aligned.
// Launch 2, param_stats_finish_kernel: one workgroup; the chunk table is sorted by group, group_first_chunk[G + 1]
// delimits each group's chunks; a wave sums its group's partials in double (lane-strided by index, then the shuffle
// tree), the totals are the sum of the group sums in group order.
// Algorithmic HBM bytes: 12 per element where all three tensors are present.
#include "common.h"
#include "stream_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int STATS_FIN_THREADS = 1024, STATS_FIN_WAVES = STATS_FIN_THREADS / 64;
constexpr int STATS_MAX_GROUPS = 1024;                   // group sums of the finishing kernel live in LDS (32 KB)
constexpr int STATS_COLS = 8;                            // out row: Sp2, Sg2, Sgm, Sm2, grad norm, gradratio, pnorm, alignment

// iterations [first, last) of the chunk walk (stream_common.h), three tensors at once; its own loop: under the
// pragmas of walk_chunk_iters this kernel compiles to other code (50 VGPRs for 102, other loads)
template <bool VEC>
__device__ __forceinline__ void add_quads(const float* __restrict__ p, const float* __restrict__ g,
                                          const float* __restrict__ m, int first, int last, int n, double (&s)[4]) {
#pragma unroll 4
  for (int i = first; i < last; ++i) {
    const int q0 = 4 * (256 * i + (int)threadIdx.x);
    if (q0 >= n) break;
    float pv[4], gv[4], mv[4];
    load_quad<VEC>(p, q0, n, pv);
    if (g != nullptr) load_quad<VEC>(g, q0, n, gv);
    if (m != nullptr) load_quad<VEC>(m, q0, n, mv);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      s[0] += (double)pv[k] * (double)pv[k];
      if (g != nullptr) s[1] += (double)gv[k] * (double)gv[k];
      if (m != nullptr) {
        s[2] += (double)gv[k] * (double)mv[k];
        s[3] += (double)mv[k] * (double)mv[k];
      }
    }
  }
}

__global__ void __launch_bounds__(256)
param_stats_kernel(const int64_t* __restrict__ ptrs /* [3][T]: p, g, m */, const int64_t* __restrict__ numel,
                   const int* __restrict__ chunk_tensor, const int64_t* __restrict__ chunk_off, int T,
                   double* __restrict__ partial /* [n_chunks][4] */) {
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  const TableChunk c = table_chunk(numel, chunk_tensor, chunk_off, T);
  const int n = c.n;
  if (n > 0) {       // (workgroup-uniform)
    const float* p = reinterpret_cast<const float*>(ptrs[c.t]) + c.off;
    const int64_t ga = ptrs[T + c.t], ma = ptrs[2 * T + c.t];
    const float* g = ga != 0 ? reinterpret_cast<const float*>(ga) + c.off : nullptr;
    const float* m = (ga != 0 && ma != 0) ? reinterpret_cast<const float*>(ma) + c.off : nullptr;
    const bool vec = ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(m)) & 15u) == 0;
    // iterations whose 256 quads are all whole: 1024 cells each
    const int whole = vec ? n / 1024 : 0;
    add_quads<true>(p, g, m, 0, whole, n, s);
    add_quads<false>(p, g, m, whole, TABLE_ITERS, n, s);
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) s[j] = wave_sum_f64(s[j]);
  block_fold4(s, [&](int j, double v) { partial[(int64_t)blockIdx.x * 4 + j] = v; });
}

__device__ __forceinline__ void write_row(float* __restrict__ o, const double (&a)[4]) {
  const double gn = sqrt(a[1]), pn = fmax(sqrt(a[0]), 1e-12);
  o[0] = (float)a[0]; o[1] = (float)a[1]; o[2] = (float)a[2]; o[3] = (float)a[3];
  o[4] = (float)gn;
  o[5] = (float)(gn / pn);
  o[6] = (float)pn;
  o[7] = a[3] > 0.0 ? (float)(a[2] / (gn * sqrt(a[3]) + 1e-12)) : 0.f;
}

// wave w owns groups w, w + 16, ..; lane 0 writes the group's row and leaves its sums in LDS; thread 0 then adds the
// group sums in group order into row G
__global__ void __launch_bounds__(STATS_FIN_THREADS)
param_stats_finish_kernel(const double* __restrict__ partial, const int* __restrict__ group_first_chunk, int n_chunks,
                          int G, float* __restrict__ out) {
  __shared__ double gsum[STATS_MAX_GROUPS][4];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int g = wave; g < G; g += STATS_FIN_WAVES) {
    const int first = max(0, group_first_chunk[g]), last = min(n_chunks, group_first_chunk[g + 1]);
    double a[4] = {0.0, 0.0, 0.0, 0.0};
    for (int i = first + lane; i < last; i += 64) {
#pragma unroll
      for (int j = 0; j < 4; ++j) a[j] += partial[(int64_t)i * 4 + j];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) a[j] = wave_sum_f64(a[j]);
    if (lane == 0) {
      write_row(out + (int64_t)g * STATS_COLS, a);
#pragma unroll
      for (int j = 0; j < 4; ++j) gsum[g][j] = a[j];
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double tot[4] = {0.0, 0.0, 0.0, 0.0};
    for (int g = 0; g < G; ++g) {
#pragma unroll
      for (int j = 0; j < 4; ++j) tot[j] += gsum[g][j];
    }
    write_row(out + (int64_t)G * STATS_COLS, tot);
  }
}

}  // namespace

extern "C" int paradis_param_stats_chunk(void) { return TABLE_CHUNK; }

// the partials [n_chunks][4] in double
extern "C" size_t paradis_param_stats_ws_bytes(int n_chunks) {
  if (n_chunks < 0) return 0;
  return (size_t)n_chunks * 4 * sizeof(double);
}

extern "C" int paradis_param_stats(const int64_t* ptrs, const int64_t* numel, const int* chunk_tensor,
                                   const int64_t* chunk_off, const int* group_first_chunk, int n_tensors, int n_chunks,
                                   int n_groups, void* workspace, float* out, void* stream) {
  PD_REQUIRE(n_tensors >= 0 && n_chunks >= 0 && n_groups >= 0, "param_stats: bad counts T=%d chunks=%d groups=%d",
             n_tensors, n_chunks, n_groups);
  if (n_groups == 0) return 0;
  PD_REQUIRE(n_groups <= STATS_MAX_GROUPS, "param_stats: %d groups (at most %d)", n_groups, STATS_MAX_GROUPS);
  PD_REQUIRE(group_first_chunk != nullptr, "param_stats: group_first_chunk missing");
  PD_REQUIRE(out != nullptr, "param_stats: result row missing");
  PD_REQUIRE(n_chunks == 0 || (ptrs && numel && chunk_tensor && chunk_off), "param_stats: tables missing");
  PD_REQUIRE(n_chunks == 0 || n_tensors >= 1, "param_stats: %d chunks of no tensor", n_chunks);
  PD_REQUIRE(n_chunks == 0 || workspace != nullptr, "param_stats: workspace missing");
  hipStream_t st = (hipStream_t)stream;
  double* partial = static_cast<double*>(workspace);
  if (n_chunks > 0)
    hipLaunchKernelGGL(param_stats_kernel, dim3(n_chunks), dim3(256), 0, st, ptrs, numel, chunk_tensor, chunk_off,
                       n_tensors, partial);
  hipLaunchKernelGGL(param_stats_finish_kernel, dim3(1), dim3(STATS_FIN_THREADS), 0, st, partial, group_first_chunk,
                     n_chunks, n_groups, out);
  PD_CHECK_LAUNCH("param_stats");
  return 0;
}
