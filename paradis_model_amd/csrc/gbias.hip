// a9 GlobalBias map (reference model/blocks.py:188-196): the low-rank map m8 = sum_r (A U) V, its projection, and the
// adjoints of both.  Small reductions next to the step's GEMMs; every sum in a fixed order.
#include <algorithm>
#include "common.h"

namespace {

// ------------------------------------------------------------------ global bias map, forward
// grid (ceil(W/64), H, Cin): m8[c,h,w] = sum_r (A[c,r] U[r,h]) V[r,w].  64 columns per workgroup, the rank range in
// four quarters (one per wave) summed in quarter order: at W = 64 a 256-column workgroup had three idle waves and
// walked all R ranks in one dependent chain (23 us for 2 M multiply-adds).
__global__ void __launch_bounds__(256)
gbias_m8_kernel(const float* __restrict__ A, const float* __restrict__ U, const float* __restrict__ V,
                float* __restrict__ m8, int Cin, int R, int H, int W) {
  __shared__ float part[4][64];
  const int tx = threadIdx.x & 63, q = threadIdx.x >> 6;
  const int w = min(blockIdx.x * 64 + tx, W - 1), h = blockIdx.y, c = blockIdx.z;
  const int rq = (R + 3) / 4, r1 = min(R, (q + 1) * rq);
  // rank loop in batches of independent loads (one dependent load per iteration made this 50 us)
  float acc = 0.f;
  int r = q * rq;
  for (; r + 8 <= r1; r += 8) {
    float a[8], u[8], v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { a[j] = A[c * R + r + j]; u[j] = U[(r + j) * H + h]; v[j] = V[(r + j) * W + w]; }
#pragma unroll
    for (int j = 0; j < 8; ++j) acc += a[j] * u[j] * v[j];
  }
  for (; r < r1; ++r) acc += A[c * R + r] * U[r * H + h] * V[r * W + w];
  part[q][tx] = acc;
  __syncthreads();
  if (q == 0 && blockIdx.x * 64 + tx < W)
    m8[((int64_t)c * H + h) * W + w] = ((part[0][tx] + part[1][tx]) + part[2][tx]) + part[3][tx];
}

// Large grids: ROWS latitude rows per workgroup.  The rank-dependent factors a[c,r] u[r,h] of the workgroup's rows are
// formed once into LDS (wave-uniform broadcast reads afterwards), so the rank loop is one coalesced V load per rank
// feeding ROWS independent accumulators, eight ranks in flight.  (One row per workgroup, every factor a scalar load
// in front of its use: 398 us for the 33 MB map of 721x1440.)  Per output the same products (a u) v in the same
// order as the kernel above.  R <= GM8_MAXR.
constexpr int GM8_MAXR = 256;
template <int ROWS>
__global__ void __launch_bounds__(256)
gbias_m8_rows_kernel(const float* __restrict__ A, const float* __restrict__ U, const float* __restrict__ V,
                     float* __restrict__ m8, int Cin, int R, int H, int W) {
  __shared__ float part[4][ROWS][64];
  __shared__ float coef[GM8_MAXR][ROWS];
  const int tx = threadIdx.x & 63, q = threadIdx.x >> 6;
  const int w = min(blockIdx.x * 64 + tx, W - 1), h0 = blockIdx.y * ROWS, c = blockIdx.z;
  for (int i = threadIdx.x; i < R * ROWS; i += 256) {
    const int r = i / ROWS, j = i - r * ROWS;
    coef[r][j] = A[c * R + r] * U[r * H + min(h0 + j, H - 1)];
  }
  __syncthreads();
  const int rq = (R + 3) / 4, r1 = min(R, (q + 1) * rq);
  float acc[ROWS];
#pragma unroll
  for (int j = 0; j < ROWS; ++j) acc[j] = 0.f;
  int r = q * rq;
  for (; r + 8 <= r1; r += 8) {
    float v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = V[(r + k) * W + w];
#pragma unroll
    for (int k = 0; k < 8; ++k)
#pragma unroll
      for (int j = 0; j < ROWS; ++j) acc[j] += coef[r + k][j] * v[k];
  }
  for (; r < r1; ++r) {
    const float v = V[r * W + w];
#pragma unroll
    for (int j = 0; j < ROWS; ++j) acc[j] += coef[r][j] * v;
  }
#pragma unroll
  for (int j = 0; j < ROWS; ++j) part[q][j][tx] = acc[j];
  __syncthreads();
  if (q == 0 && blockIdx.x * 64 + tx < W) {
#pragma unroll
    for (int j = 0; j < ROWS; ++j)
      if (h0 + j < H)
        m8[((int64_t)c * H + h0 + j) * W + w] = ((part[0][j][tx] + part[1][j][tx]) + part[2][j][tx]) + part[3][j][tx];
  }
}

// out[o,p] = sum_c Wm[o*ldo + c*ldc] * in[c,p]      (projection and its transpose)
// grid (ceil(P/256), Cout)
__global__ void __launch_bounds__(256)
small_mix_kernel(const float* __restrict__ Wm, int ldo, int ldc, const float* __restrict__ in,
                 float* __restrict__ out, int Cout, int Cin, int64_t P) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int o = blockIdx.y;
  if (p >= P) return;
  float acc = 0.f;
  for (int c = 0; c < Cin; ++c) acc += Wm[(int64_t)o * ldo + (int64_t)c * ldc] * in[(int64_t)c * P + p];
  out[(int64_t)o * P + p] = acc;
}

// gm8[c,p] = sum_o Pw[o,c] * gmap[o,p]   (c < CIN <= 16 kept in registers)
// One workgroup = 64 pixels x 16 slices of the long sum over Co (one wave per slice: the row of Pw is wave-uniform);
// the slices meet in LDS and are added in slice order - no atomics, no zero fill, the same bits on every run.
// (Rounds 1-3 split Co over the grid and combined the chunks with float atomicAdd: run-to-run differences in the
// last bit of the GlobalBias gradients, which AdamW's normalisation can turn into visible parameter differences.)
constexpr int GM8_SLICES = 16;
#ifndef GM8_BATCH                // (A/B builds)
#define GM8_BATCH 16
#endif
template <int CIN>
__global__ void __launch_bounds__(64 * GM8_SLICES)
gbias_gm8_kernel(const float* __restrict__ Pw, const float* __restrict__ gmap, float* __restrict__ gm8,
                 int Cin, int Co, int64_t P) {
  __shared__ float part[GM8_SLICES][CIN][64];
  const int px = threadIdx.x & 63;
  const int slice = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t p = (int64_t)blockIdx.x * 64 + px;
  const int64_t pc = min(p, P - 1);
  const int per = (Co + GM8_SLICES - 1) / GM8_SLICES, o0 = slice * per, o1 = min(o0 + per, Co);
  float acc[CIN];
#pragma unroll
  for (int c = 0; c < CIN; ++c) acc[c] = 0.f;
  int o = o0;
  for (; o + GM8_BATCH <= o1; o += GM8_BATCH) {      // sixteen independent row loads in flight (round 5; eight before: the
    float g[GM8_BATCH];                              //  wave's 64-row walk is a chain of batches, each a memory round trip)
#pragma unroll
    for (int j = 0; j < GM8_BATCH; ++j) g[j] = gmap[(int64_t)(o + j) * P + pc];
#pragma unroll
    for (int j = 0; j < GM8_BATCH; ++j)
#pragma unroll
      for (int c = 0; c < CIN; ++c)
        if (c < Cin) acc[c] += Pw[(int64_t)(o + j) * Cin + c] * g[j];
  }
  for (; o + 8 <= o1; o += 8) {
    float g[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) g[j] = gmap[(int64_t)(o + j) * P + pc];
#pragma unroll
    for (int j = 0; j < 8; ++j)
#pragma unroll
      for (int c = 0; c < CIN; ++c)
        if (c < Cin) acc[c] += Pw[(int64_t)(o + j) * Cin + c] * g[j];
  }
  for (; o < o1; ++o) {
    const float g = gmap[(int64_t)o * P + pc];
#pragma unroll
    for (int c = 0; c < CIN; ++c)
      if (c < Cin) acc[c] += Pw[(int64_t)o * Cin + c] * g;
  }
#pragma unroll
  for (int c = 0; c < CIN; ++c) part[slice][c][px] = acc[c];
  __syncthreads();
  if (slice < Cin && p < P) {          // wave `slice` finishes channel c = slice
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < GM8_SLICES; ++k) s += part[k][slice][px];
    gm8[(int64_t)slice * P + p] = s;
  }
}

// ------------------------------------------------------------------ global bias map, backward
// gPw[o,c] = sum_p gmap[o,p] * m8[c,p]; one workgroup per (o,c).  (A one-workgroup-per-o form that reads the row of
// gmap once - 109 instead of 809 MB at 128x256 - was measured in round 4: 383 us against 180 us, 32 against 15 us at
// 32x64: 1024 workgroups walking 128 dependent iterations lose more than the re-reads through L2 cost.)
__global__ void __launch_bounds__(256)
gbias_gpw_kernel(const float* __restrict__ gmap, const float* __restrict__ m8,
                 float* __restrict__ gPw, int Cin, int64_t P) {
  __shared__ float red[4];
  const int o = blockIdx.x / Cin, c = blockIdx.x - o * Cin;
  float acc = 0.f;
  for (int64_t p = threadIdx.x; p < P; p += 256) acc += gmap[(int64_t)o * P + p] * m8[(int64_t)c * P + p];
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) gPw[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

// The same sums with RW output rows per workgroup and 16-byte loads (round 5; the larger grids): a workgroup walks the
// whole pixel range once - its RW rows of gmap come from HBM once, the Cin rows of m8 from L2 (Co / RW times 4 Cin P
// bytes; the (o, c)-workgroup form above pulls every row of gmap Cin times: 809 MB at 128x256, Co = 1024).  RW + Cin
// float4 loads in flight per thread and iteration.  Needs P % 4 == 0 and 16-byte aligned rows.
template <int RW, int CIN>
__global__ void __launch_bounds__(256)
gbias_gpw_rows_kernel(const float* __restrict__ gmap, const float* __restrict__ m8, float* __restrict__ gPw, int Cin,
                      int Co, int64_t P4) {
  __shared__ float red[4][RW * CIN];
  const int o0 = blockIdx.x * RW;
  float acc[RW][CIN];
#pragma unroll
  for (int j = 0; j < RW; ++j)
#pragma unroll
    for (int c = 0; c < CIN; ++c) acc[j][c] = 0.f;
  const float4* g4 = reinterpret_cast<const float4*>(gmap);
  const float4* m4 = reinterpret_cast<const float4*>(m8);
  for (int64_t q = threadIdx.x; q < P4; q += 256) {
    float4 m[CIN], g[RW];
#pragma unroll
    for (int c = 0; c < CIN; ++c) m[c] = m4[(int64_t)min(c, Cin - 1) * P4 + q];
#pragma unroll
    for (int j = 0; j < RW; ++j) g[j] = g4[(int64_t)min(o0 + j, Co - 1) * P4 + q];
#pragma unroll
    for (int j = 0; j < RW; ++j)
#pragma unroll
      for (int c = 0; c < CIN; ++c)
        acc[j][c] += (g[j].x * m[c].x + g[j].y * m[c].y) + (g[j].z * m[c].z + g[j].w * m[c].w);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < RW; ++j)
#pragma unroll
    for (int c = 0; c < CIN; ++c) {
      const float sum = wave_sum_dpp(acc[j][c]);
      if (lane == 0) red[wave][j * CIN + c] = sum;
    }
  __syncthreads();
  if (threadIdx.x < RW * CIN) {
    const int j = threadIdx.x / CIN, c = threadIdx.x - j * CIN;
    if (o0 + j < Co && c < Cin)
      gPw[(int64_t)(o0 + j) * Cin + c] = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
  }
}

// T1[c,r,h] = sum_w gm8[c,h,w] V[r,w]   (one wave per output)
__global__ void __launch_bounds__(256)
gbias_t1_kernel(const float* __restrict__ gm8, const float* __restrict__ V, float* __restrict__ T1,
                int Cin, int R, int H, int W) {
  const int64_t wid = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
  if (wid >= (int64_t)Cin * R * H) return;
  const int h = (int)(wid % H), r = (int)((wid / H) % R), c = (int)(wid / ((int64_t)H * R));
  float acc = 0.f;
  for (int w = threadIdx.x & 63; w < W; w += 64) acc += gm8[((int64_t)c * H + h) * W + w] * V[r * W + w];
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) T1[wid] = acc;
}

// T2[c,r,w] = sum_h gm8[c,h,w] U[r,h]
__global__ void __launch_bounds__(256)
gbias_t2_kernel(const float* __restrict__ gm8, const float* __restrict__ U, float* __restrict__ T2,
                int Cin, int R, int H, int W) {
  const int64_t total = (int64_t)Cin * R * W;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total;
       idx += (int64_t)gridDim.x * 256) {
    const int w = (int)(idx % W), r = (int)((idx / W) % R), c = (int)(idx / ((int64_t)W * R));
    float acc = 0.f;
    for (int h = 0; h < H; ++h) acc += gm8[((int64_t)c * H + h) * W + w] * U[r * H + h];
    T2[idx] = acc;
  }
}

// gA[c,r] = sum_h T1[c,r,h] U[r,h];  gU[r,h] = sum_c T1[c,r,h] A[c,r];  gV[r,w] = sum_c T2[c,r,w] A[c,r]
// (gA: one WAVE per output, lanes along h - a thread per output walked H dependent iterations of a strided row and set
//  the kernel's duration: 33 us at 128x256; gU, gV: a thread per output, coalesced along h / w)
__global__ void __launch_bounds__(256)
gbias_finish_kernel(const float* __restrict__ T1, const float* __restrict__ T2,
                    const float* __restrict__ A, const float* __restrict__ U,
                    float* __restrict__ gA, float* __restrict__ gU, float* __restrict__ gV, int Cin,
                    int R, int H, int W) {
  const int nA = Cin * R, nU = R * H, nV = R * W;
  const int wavesA = (nA + 3) / 4;               // workgroups that hold the gA waves (four per workgroup)
  if ((int)blockIdx.x < wavesA) {
    const int idx = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (idx >= nA) return;
    const int c = idx / R, r = idx - c * R;
    float acc = 0.f;
    for (int h = lane; h < H; h += 64) acc += T1[((int64_t)c * R + r) * H + h] * U[r * H + h];
    acc = wave_sum_dpp(acc);
    if (lane == 0) gA[idx] = acc;
    return;
  }
  const int idx = ((int)blockIdx.x - wavesA) * 256 + threadIdx.x;
  if (idx < nU) {
    const int r = idx / H, h = idx - r * H;
    float acc = 0.f;
    for (int c = 0; c < Cin; ++c) acc += T1[((int64_t)c * R + r) * H + h] * A[c * R + r];
    gU[idx] = acc;
  } else if (idx < nU + nV) {
    const int j = idx - nU, r = j / W, w = j - r * W;
    float acc = 0.f;
    for (int c = 0; c < Cin; ++c) acc += T2[((int64_t)c * R + r) * W + w] * A[c * R + r];
    gV[j] = acc;
  }
}

void launch_gm8(const float* Pw, const float* gmap, float* gm8, int Cin, int Co, int64_t P, hipStream_t st) {   // Cin <= 16
  const dim3 grid((unsigned)((P + 63) / 64)), block(64 * GM8_SLICES);
  if (Cin <= 8) hipLaunchKernelGGL(gbias_gm8_kernel<8>, grid, block, 0, st, Pw, gmap, gm8, Cin, Co, P);
  else hipLaunchKernelGGL(gbias_gm8_kernel<16>, grid, block, 0, st, Pw, gmap, gm8, Cin, Co, P);
}
#ifndef GBIAS_GPW_ROWS           // (A/B builds: 0 = one workgroup per (o, c) on every grid)
#define GBIAS_GPW_ROWS 1
#endif
#ifndef GBIAS_GPW_ROWS_MINP      // smallest pixel count that takes the rows kernel
#define GBIAS_GPW_ROWS_MINP 2048
#endif
void launch_gpw(const float* gmap, const float* m8, float* gPw, int Cin, int Co, int64_t P, hipStream_t st) {
  if (GBIAS_GPW_ROWS && Cin <= 8 && P % 4 == 0 && P >= GBIAS_GPW_ROWS_MINP && aligned16(gmap) && aligned16(m8)) {
    if (Co >= 1024)
      hipLaunchKernelGGL((gbias_gpw_rows_kernel<4, 8>), dim3((Co + 3) / 4), dim3(256), 0, st, gmap, m8, gPw, Cin, Co, P / 4);
    else
      hipLaunchKernelGGL((gbias_gpw_rows_kernel<2, 8>), dim3((Co + 1) / 2), dim3(256), 0, st, gmap, m8, gPw, Cin, Co, P / 4);
    return;
  }
  hipLaunchKernelGGL(gbias_gpw_kernel, dim3(Co * Cin), dim3(256), 0, st, gmap, m8, gPw, Cin, P);
}

}  // namespace

extern "C" int paradis_global_bias_map_fwd(const float* A, const float* U, const float* V,
                                           const float* Pw, float* m8, float* map, int Cin, int Co,
                                           int R, int H, int W, void* stream) {
  PD_REQUIRE(Cin >= 1 && Co >= 1 && R >= 1 && H >= 1 && W >= 1, "global_bias_map_fwd: bad shape");
  PD_REQUIRE(Pw != nullptr || Cin == Co, "global_bias_map_fwd: projection required when Cin != Co");
  hipStream_t st = (hipStream_t)stream;
  const int64_t P = (int64_t)H * W;
  float* m8_dst = Pw ? m8 : map;
  PD_REQUIRE(H <= 65535 && Cin <= 65535 && Co <= 65535, "global_bias_map_fwd: grid too large");
  if ((int64_t)H * W >= (1 << 17) && R <= GM8_MAXR)
    hipLaunchKernelGGL(gbias_m8_rows_kernel<8>, dim3((W + 63) / 64, (H + 7) / 8, Cin), dim3(256), 0, st, A, U, V, m8_dst,
                       Cin, R, H, W);
  else
    hipLaunchKernelGGL(gbias_m8_kernel, dim3((W + 63) / 64, H, Cin), dim3(256), 0, st, A, U, V, m8_dst, Cin, R, H, W);
  if (Pw)
    hipLaunchKernelGGL(small_mix_kernel, dim3((unsigned)((P + 255) / 256), Co), dim3(256), 0, st, Pw, Cin, 1,
                       m8, map, Co, Cin, P);
  PD_CHECK_LAUNCH("global_bias_map_fwd");
  return 0;
}

extern "C" size_t paradis_global_bias_map_bwd_ws_bytes(int Cin, int Co, int R, int H, int W) {
  (void)Co;
  return ((size_t)Cin * H * W + (size_t)Cin * R * H + (size_t)Cin * R * W) * sizeof(float) + 256;
}

extern "C" int paradis_global_bias_map_bwd(const float* gmap, const float* A, const float* U,
                                           const float* V, const float* Pw, const float* m8, float* gA,
                                           float* gU, float* gV, float* gPw, int Cin, int Co, int R,
                                           int H, int W, void* workspace, void* stream) {
  PD_REQUIRE(Cin >= 1 && Co >= 1 && R >= 1 && H >= 1 && W >= 1, "global_bias_map_bwd: bad shape");
  PD_REQUIRE(workspace != nullptr, "global_bias_map_bwd: workspace required");
  PD_REQUIRE(Pw != nullptr || Cin == Co, "global_bias_map_bwd: projection required when Cin != Co");
  hipStream_t st = (hipStream_t)stream;
  const int64_t P = (int64_t)H * W;
  float* gm8 = (float*)workspace;
  float* T1 = gm8 + (size_t)Cin * P;
  float* T2 = T1 + (size_t)Cin * R * H;
  const float* gm8_src = gmap;
  if (Pw) {
    PD_REQUIRE(m8 != nullptr && gPw != nullptr, "global_bias_map_bwd: m8/gPw required with projection");
    launch_gpw(gmap, m8, gPw, Cin, Co, P, st);
    // gm8[c,p] = sum_o Pw[o,c] gmap[o,p]
    if (Cin <= 16) {
      launch_gm8(Pw, gmap, gm8, Cin, Co, P, st);
    } else {
      hipLaunchKernelGGL(small_mix_kernel, dim3((unsigned)((P + 255) / 256), Cin), dim3(256), 0, st, Pw, 1,
                         Cin, gmap, gm8, Cin, Co, P);
    }
    gm8_src = gm8;
  }
  // (T1, T2 and the finish in ONE kernel - everything is local to a rank index r: R workgroups walking gm8 once, row dot
  //  products by wave sums, column sums in registers - was built in round 5: 31.5 us per call in the 32x64 step against
  //  9.1 + 10.5 + 9.1 us for the three wide kernels, 3.2 against 1.56 ms at 721x1440; removed)
  const int64_t nwaves = (int64_t)Cin * R * H;
  hipLaunchKernelGGL(gbias_t1_kernel, dim3((unsigned)((nwaves * 64 + 255) / 256)), dim3(256), 0, st,
                     gm8_src, V, T1, Cin, R, H, W);
  hipLaunchKernelGGL(gbias_t2_kernel, dim3(stream_blocks((int64_t)Cin * R * W)), dim3(256), 0, st, gm8_src,
                     U, T2, Cin, R, H, W);
  const int nfin = (Cin * R + 3) / 4 + (R * H + R * W + 255) / 256;      // gA waves, then gU / gV threads
  hipLaunchKernelGGL(gbias_finish_kernel, dim3(nfin), dim3(256), 0, st, T1, T2, A, U, gA, gU,
                     gV, Cin, R, H, W);
  PD_CHECK_LAUNCH("global_bias_map_bwd");
  return 0;
}

// ---- GlobalBias in two stages (lets the GEMM epilogue apply the projection on the fly) ----
// stage 1: m8[Cin,H,W] = sum_r A[c,r] U[r,h] V[r,w]
extern "C" int paradis_global_bias_m8_fwd(const float* A, const float* U, const float* V, float* m8,
                                          int Cin, int R, int H, int W, void* stream) {
  return paradis_global_bias_map_fwd(A, U, V, nullptr, nullptr, m8, Cin, Cin, R, H, W, stream);
}
// adjoint of stage 1: (gA, gU, gV) from gm8; workspace >= paradis_global_bias_map_bwd_ws_bytes
extern "C" int paradis_global_bias_m8_bwd(const float* gm8, const float* A, const float* U,
                                          const float* V, float* gA, float* gU, float* gV, int Cin,
                                          int R, int H, int W, void* workspace, void* stream) {
  return paradis_global_bias_map_bwd(gm8, A, U, V, nullptr, nullptr, gA, gU, gV, nullptr, Cin, Cin, R, H,
                                     W, workspace, stream);
}
// adjoint of the projection map[o,p] = sum_c Pw[o,c] m8[c,p]:  gPw[o,c] = sum_p gmap[o,p] m8[c,p],
// gm8[c,p] = sum_o Pw[o,c] gmap[o,p]
extern "C" int paradis_global_bias_proj_bwd(const float* gmap, const float* m8, const float* Pw,
                                            float* gPw, float* gm8, int Cin, int Co, int64_t P,
                                            void* stream) {
  PD_REQUIRE(Cin >= 1 && Cin <= 16 && Co >= 1 && P >= 1, "global_bias_proj_bwd: bad shape (Cin <= 16)");
  hipStream_t st = (hipStream_t)stream;
  launch_gpw(gmap, m8, gPw, Cin, Co, P, st);
  launch_gm8(Pw, gmap, gm8, Cin, Co, P, st);
  PD_CHECK_LAUNCH("global_bias_proj_bwd");
  return 0;
}
