// Depthwise stencil, one 32x64 tile per workgroup: every k in 1..11 on every grid (what the whole-plane and staged-tiles
// families do not take); forward, data gradient, weight gradient and their launchers.
#include "stencil_common.h"

namespace {

template <int K, bool Y16 = false>
__global__ void __launch_bounds__(256)
dwconv_geo_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                      const float* __restrict__ bias, float* __restrict__ y, int C, int H, int W,
                      int tiles_x, int tiles, int whole_vec4) {
  __shared__ float tile[(TH + K - 1) * (TW + K - 1)];
  const int64_t plane = blockIdx.x / tiles;
  const int t = blockIdx.x - plane * tiles;
  const int ty0 = (t / tiles_x) * TH, tx0 = (t % tiles_x) * TW;
  const int c = plane % C;
  stage_any<K>(tile, x + plane * (int64_t)H * W, H, W, ty0, tx0, whole_vec4);
  __syncthreads();
  float acc[RPT];
  tile_stencil<K, false>(tile, w + (int64_t)c * K * K, acc);
  const float bv = bias ? bias[c] : 0.f;
  const int xx = tx0 + (threadIdx.x & 63), r0 = ty0 + (threadIdx.x >> 6) * RPT;
  if (xx < W) {
    float* yp = y + plane * (int64_t)H * W;
    uint16_t* yp16 = reinterpret_cast<uint16_t*>(y) + plane * (int64_t)H * W;
#pragma unroll
    for (int o = 0; o < RPT; ++o)
      if (r0 + o < H) {
        const float v = acc[o] + bv;
        if constexpr (Y16) yp16[(int64_t)(r0 + o) * W + xx] = bf16_bits(v);
        else yp[(int64_t)(r0 + o) * W + xx] = v;
      }
  }
}

// Data gradient.  With the halo virtual, gx = PadAdjoint(ConvTranspose(gy)).  Folding the halo
// aliases back analytically gives a stencil on the *geocyclic extension* E of gy itself:
//   rows of E inside the image : transposed taps        w[p-dr][p-dc]
//   rows of E beyond a pole    : row index NOT flipped   w[p+dr][p-dc]  (the over-the-pole glide
//                                reflection reverses the row direction), and they only feed source
//                                rows 1..p (south) / H-1-p..H-2 (north);
//   the pole row itself seen through the mirror (dr = -y resp. H-1-y) needs the W/2-shifted pole
//   row, which differs from E's unshifted row: K extra taps read from global memory.
// Longitude wrap is implied by E's periodic columns.
// `addend` (nullable): gx = dgrad + addend - the other gradient of the stencil's input (a consumer around the block:
// the gated blend's share of the advection input), added here instead of by a separate pass of the autograd engine.
template <int K>
__global__ void __launch_bounds__(256)
dwconv_geo_dgrad_kernel(const float* __restrict__ gy, const float* __restrict__ w, const float* __restrict__ addend,
                        float* __restrict__ gx, int C, int H, int W, int tiles_x, int tiles,
                        int whole_vec4) {
  constexpr int P = (K - 1) / 2, LW = TW + K - 1;
  __shared__ float tile[(TH + K - 1) * (TW + K - 1)];
  const int64_t plane = blockIdx.x / tiles;
  const int t = blockIdx.x - plane * tiles;
  const int ty0 = (t / tiles_x) * TH, tx0 = (t % tiles_x) * TW;
  const int c = plane % C;
  const float* g = gy + plane * (int64_t)H * W;
  const float* wc = w + (int64_t)c * K * K;
  stage_any<K>(tile, g, H, W, ty0, tx0, whole_vec4);
  __syncthreads();
  const int xl = threadIdx.x & 63, r0 = (threadIdx.x >> 6) * RPT;
  float wr[K * K];
#pragma unroll
  for (int i = 0; i < K * K; ++i) wr[i] = wc[i];
  float acc[RPT];
#pragma unroll
  for (int o = 0; o < RPT; ++o) acc[o] = 0.f;
#pragma unroll
  for (int rr = 0; rr < RPT + K - 1; ++rr) {
    const int ii = ty0 + r0 + rr - P;   // image row of this tile row (wave-uniform)
    float val[K];
#pragma unroll
    for (int b = 0; b < K; ++b) val[b] = tile[(r0 + rr) * LW + xl + b];
    if (ii >= 0 && ii < H) {
#pragma unroll
      for (int a = 0; a < K; ++a) {       // a = tile row offset of output o: rr = o + a, dr = a - P
        const int o = rr - a;
        if (o >= 0 && o < RPT) {
#pragma unroll
          for (int b = 0; b < K; ++b) acc[o] += wr[(K - 1 - a) * K + (K - 1 - b)] * val[b];
        }
      }
    } else {
#pragma unroll
      for (int a = 0; a < K; ++a) {
        const int o = rr - a;
        if (o >= 0 && o < RPT) {
          const int yy = ty0 + r0 + o;
          const bool feeds = (ii < 0) ? (yy >= 1) : (yy <= H - 2);
          if (feeds) {
#pragma unroll
            for (int b = 0; b < K; ++b) acc[o] += wr[a * K + (K - 1 - b)] * val[b];
          }
        }
      }
    }
  }
  const int xx = tx0 + xl;
  if (xx >= W) return;
  const int half = W >> 1;
#pragma unroll
  for (int o = 0; o < RPT; ++o) {
    const int yy = ty0 + r0 + o;
    if (yy >= H) break;
    float extra = 0.f;
    // mirrored pole rows: E'[0][jj] = gy[0][jj + W/2], E'[H-1][jj] = gy[H-1][jj + W/2].  When the
    // plane is a single tile both pole rows are in LDS (tile rows P and H-1+P, column + P).
    const bool south = yy >= 1 && yy <= P, north = yy >= H - 1 - P && yy <= H - 2;
    if (south || north) {
      const int a = south ? P - yy : P + (H - 1 - yy);   // dr = -yy  resp.  H-1-yy
      const int prow = south ? 0 : H - 1;
#pragma unroll
      for (int b = 0; b < K; ++b) {     // dc = P - b
        int col = xx + P - b + half;
        if (col >= W) col -= W;          // xx + P - b + W/2 lies in [-P+W/2, W + P + W/2)
        if (col >= W) col -= W;
        const float pv = tiles == 1 ? tile[(prow + P) * LW + col + P] : g[(int64_t)prow * W + col];
        extra += wc[a * K + b] * pv;   // (wc, not the register copy: a is not a compile-time index)
      }
    }
    const int64_t at = plane * (int64_t)H * W + (int64_t)yy * W + xx;
    gx[at] = acc[o] + extra + (addend ? addend[at] : 0.f);
  }
}

// partial[c][chunk][K*K (+1 for bias)] ; items of a channel = (batch n, tile t)
template <int K>
__global__ void __launch_bounds__(256)
dwconv_geo_wgrad_kernel(const float* __restrict__ gy, const float* __restrict__ x,
                        float* __restrict__ partial, int B, int C, int H, int W, int tiles_x,
                        int tiles, int chunks, int whole_vec4) {
  constexpr int LW = TW + K - 1, NW = K * K + 1;
  __shared__ float tile[(TH + K - 1) * (TW + K - 1)];
  __shared__ float red[4][NW];
  const int c = blockIdx.x / chunks, chunk = blockIdx.x - c * chunks;
  const int items = B * tiles;
  const int xl = threadIdx.x & 63, wave = threadIdx.x >> 6, r0l = wave * RPT;
  float acc[K * K];
#pragma unroll
  for (int i = 0; i < K * K; ++i) acc[i] = 0.f;
  float gsum = 0.f;
  // (tile cells no staging path writes meet zero cotangents: keep 0 x NaN out, see dwconv_geo_wgrad_planes_kernel, stencil_planes.hip)
  for (int i = threadIdx.x; i < (TH + K - 1) * (TW + K - 1); i += 256) tile[i] = 0.f;
  for (int item = chunk; item < items; item += chunks) {
    const int n = item / tiles, t = item - n * tiles;
    const int ty0 = (t / tiles_x) * TH, tx0 = (t % tiles_x) * TW;
    const int64_t plane = (int64_t)n * C + c;
    __syncthreads();
    stage_any<K>(tile, x + plane * (int64_t)H * W, H, W, ty0, tx0, whole_vec4);
    __syncthreads();
    float g[RPT];
    const int xx = tx0 + xl;
#pragma unroll
    for (int o = 0; o < RPT; ++o) {
      const int yy = ty0 + r0l + o;
      g[o] = (xx < W && yy < H) ? gy[plane * (int64_t)H * W + (int64_t)yy * W + xx] : 0.f;
      gsum += g[o];
    }
#pragma unroll
    for (int rr = 0; rr < RPT + K - 1; ++rr) {
      float val[K];
#pragma unroll
      for (int b = 0; b < K; ++b) val[b] = tile[(r0l + rr) * LW + xl + b];
#pragma unroll
      for (int a = 0; a < K; ++a) {
        const int o = rr - a;
        if (o >= 0 && o < RPT) {
#pragma unroll
          for (int b = 0; b < K; ++b) acc[a * K + b] += g[o] * val[b];
        }
      }
    }
  }
#pragma unroll
  for (int i = 0; i < K * K; ++i) {
    float s = wave_sum_dpp(acc[i]);
    if (xl == 0) red[wave][i] = s;
  }
  {
    float s = wave_sum_dpp(gsum);
    if (xl == 0) red[wave][K * K] = s;
  }
  __syncthreads();
  if (threadIdx.x < NW) {
    float s = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
    partial[((int64_t)c * chunks + chunk) * NW + threadIdx.x] = s;
  }
}

#define DISPATCH_K(k, CALL)          \
  switch (k) {                       \
    case 1: { constexpr int KK = 1; CALL; } break; \
    case 3: { constexpr int KK = 3; CALL; } break; \
    case 5: { constexpr int KK = 5; CALL; } break; \
    case 7: { constexpr int KK = 7; CALL; } break; \
    case 9: { constexpr int KK = 9; CALL; } break; \
    default: { constexpr int KK = 11; CALL; } break; \
  }

// forward kernel of a size, indexed by the boolean template parameter
using FwdKernel = decltype(&dwconv_geo_fwd_kernel<5, false>);
template <int K>
constexpr FwdKernel FWD[2] = {&dwconv_geo_fwd_kernel<K, false>, &dwconv_geo_fwd_kernel<K, true>};   // [Y16]

}  // namespace

void pd_dw_fwd_generic(const DwArgs& a, bool y16, int whole_vec4) {
  const unsigned grid = (unsigned)dw_fwd_geom(DwSched::Generic, a).grid;
  DISPATCH_K(a.k, hipLaunchKernelGGL(FWD<KK>[y16], dim3(grid), dim3(256), 0, a.st, a.x, a.w, a.bias, a.y, a.C, a.H, a.W,
                                     dw_tiles_x(a.W), dw_tiles(a.H, a.W), whole_vec4));
}

void pd_dw_dgrad_generic(const DwArgs& a, int whole_vec4) {
  const unsigned grid = (unsigned)dw_dgrad_geom(DwSched::Generic, a).grid;
  DISPATCH_K(a.k, hipLaunchKernelGGL(dwconv_geo_dgrad_kernel<KK>, dim3(grid), dim3(256), 0, a.st, a.gy, a.w, a.addend,
                                     a.gx, a.C, a.H, a.W, dw_tiles_x(a.W), dw_tiles(a.H, a.W), whole_vec4));
}

int pd_dw_wgrad_generic(const DwArgs& a, int whole_vec4) {
  const DwGeom g = dw_wgrad_geom(DwSched::Generic, a);
  DISPATCH_K(a.k, hipLaunchKernelGGL(dwconv_geo_wgrad_kernel<KK>, dim3((unsigned)g.grid), dim3(256), 0, a.st, a.gy, a.x,
                                     a.partial, a.B, a.C, a.H, a.W, dw_tiles_x(a.W), dw_tiles(a.H, a.W), g.chunks,
                                     whole_vec4));
  return g.chunks;
}
