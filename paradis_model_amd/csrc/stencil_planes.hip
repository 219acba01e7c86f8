// Depthwise stencil, the two k = 5 families that keep the next item's loads in flight under the current item's arithmetic:
// whole planes (W = 64, H <= 32: the reference grids at 5.625 degrees; PLANE_CHUNK planes per workgroup, both directions
// and the one-pass backward) and staged full tiles of the larger grids (forward, and the backward kernel that computes
// either gradient or both); their launchers.  One unit for both: alone in a unit the whole-plane kernels are the only
// callers of geo_src, the compiler propagates W = 64 into it and all nine get different (equivalent) instructions.
#include "stencil_common.h"

namespace {

// The whole-plane case again (W == TW, H <= TH, k = 5: stage_plane_vec4's conditions), split into LOAD and STORE so
// that a workgroup walking several planes can have the next plane's loads in flight while it computes the current one:
// with one plane per workgroup a CU has loads outstanding only about half of the time (4.6 TB/s; Little's law with
// eight 8-KB planes per CU).  The per-thread cells - two float4 of the interior, two halo cells (destination in the
// tile, source in the plane) - do not depend on the plane and are computed once.
template <int K>
struct PlaneStager {
  static constexpr int P = (K - 1) / 2, LW = TW + K - 1;
  unsigned vsrc[2], hsrc[2];
  int vdst[2], hdst[2];
  __device__ __forceinline__ void init(int H) {
    constexpr int W = TW, w4 = W / 4, hc = 2 * P;
    const int nvec = H * w4, nhalo_rows = 2 * P * LW, nhalo = nhalo_rows + H * hc, Hp = H + 2 * P;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int v = threadIdx.x + 256 * j, vc = min(v, nvec - 1);
      const int y = vc / w4, x4 = vc - y * w4;
      vsrc[j] = (unsigned)vc * 16u;                     // byte offsets
      vdst[j] = v < nvec ? (y + P) * LW + P + 4 * x4 : -1;
      const int kk = threadIdx.x + 256 * j, k = min(kk, nhalo - 1);
      int lr, lc;
      if (k < nhalo_rows) {
        const int rr = k / LW;
        lc = k - rr * LW;
        lr = rr < P ? rr : Hp - 2 * P + rr;
      } else {
        const int e = k - nhalo_rows, rr = e / hc, cc = e - rr * hc;
        lr = rr + P;
        lc = cc < P ? cc : W + cc;
      }
      int sr, sc;
      geo_src(lr - P, lc - P, H, W, sr, sc);
      hsrc[j] = (unsigned)(sr * W + sc) * 4u;
      hdst[j] = kk < nhalo ? lr * LW + lc : -1;
    }
  }
  __device__ __forceinline__ void load(const float* __restrict__ F, f32x4 (&q)[2], float (&hv)[2]) const {
    const ubase_t b = uniform_base(F);
#pragma unroll
    for (int j = 0; j < 2; ++j) { q[j] = load_at<f32x4>(b, vsrc[j]); hv[j] = load_at<float>(b, hsrc[j]); }
  }
  // the same plane stored as bf16 (round 6: the cotangent of a bf16-stored output): half the byte offsets.  load16 keeps the
  // RAW words (q.x, q.y = four bf16; hv = one, zero-extended by the load) so that nothing waits for the data at the fetch
  // site - the prefetch stays in flight under the previous plane's arithmetic - and store16 widens them on the way to LDS.
  __device__ __forceinline__ void load16(const uint16_t* __restrict__ F, f32x4 (&q)[2], float (&hv)[2]) const {
    const ubase_t b = uniform_base(F);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const u32x2 r = load_at<u32x2>(b, vsrc[j] >> 1);
      q[j].x = __uint_as_float(r.x); q[j].y = __uint_as_float(r.y);
      hv[j] = __uint_as_float((uint32_t)load_at<uint16_t>(b, hsrc[j] >> 1));
    }
  }
  __device__ __forceinline__ void store16(float* tile, const f32x4 (&q)[2], const float (&hv)[2]) const {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      if (vdst[j] >= 0) {
        const uint32_t lo = __float_as_uint(q[j].x), hi = __float_as_uint(q[j].y);
        float2* d = reinterpret_cast<float2*>(tile + vdst[j]);
        d[0] = make_float2(__uint_as_float(lo << 16), __uint_as_float(lo & 0xffff0000u));
        d[1] = make_float2(__uint_as_float(hi << 16), __uint_as_float(hi & 0xffff0000u));
      }
      if (hdst[j] >= 0) tile[hdst[j]] = __uint_as_float(__float_as_uint(hv[j]) << 16);
    }
  }
  __device__ __forceinline__ void store(float* tile, const f32x4 (&q)[2], const float (&hv)[2]) const {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      if (vdst[j] >= 0) {
        float2* d = reinterpret_cast<float2*>(tile + vdst[j]);      // 8-byte aligned (P, LW even)
        d[0] = make_float2(q[j].x, q[j].y);
        d[1] = make_float2(q[j].z, q[j].w);
      }
      if (hdst[j] >= 0) tile[hdst[j]] = hv[j];
    }
  }
};

// whole-plane path: PLANE_CHUNK planes per workgroup, the next plane's loads in flight during the stencil
template <int K, bool Y16 = false>
__global__ void __launch_bounds__(256, 5)   // (8 waves per SIMD = 64 registers spill the prefetched plane: 235 us instead of 99)
dwconv_geo_fwd_planes_kernel(const float* __restrict__ x, const float* __restrict__ w,
                             const float* __restrict__ bias, float* __restrict__ y, int C, int H, int64_t planes) {
  constexpr int W = TW;
  __shared__ float tile[(TH + K - 1) * (TW + K - 1)];
  const int xl = threadIdx.x & 63, r0l = (threadIdx.x >> 6) * RPT;
  const int64_t first = (int64_t)blockIdx.x * PLANE_CHUNK;
  const int n = (int)min((int64_t)PLANE_CHUNK, planes - first);
  PlaneStager<K> sg;
  sg.init(H);
  f32x4 q[2];
  float hv[2];
  sg.load(x + first * (int64_t)H * W, q, hv);
  for (int i = 0; i < n; ++i) {
    const int64_t plane = first + i;
    const int c = (int)(plane % C);
    sg.store(tile, q, hv);
    __syncthreads();
    if (i + 1 < n) sg.load(x + (plane + 1) * (int64_t)H * W, q, hv);
    float acc[RPT];
    tile_stencil<K, false>(tile, w + (int64_t)c * K * K, acc);
    const float bv = bias ? bias[c] : 0.f;
    constexpr int ES = Y16 ? 2 : 4;
    const ubase_t yp = uniform_base(reinterpret_cast<const char*>(y) + plane * (int64_t)H * W * ES);
    const unsigned o0 = (unsigned)(r0l * W + xl) * (unsigned)ES;
#pragma unroll
    for (int o = 0; o < RPT; ++o)
      if (r0l + o < H) {      // (the row step is on the scalar base)
        if constexpr (Y16) store_at<uint16_t>(yp + o * W * ES, o0, bf16_bits(acc[o] + bv));
        else store_at<float>(yp + o * W * ES, o0, acc[o] + bv);
      }
    __syncthreads();
  }
}

// whole-plane path of the data gradient: PLANE_CHUNK planes per workgroup, next plane's loads in flight (see
// dwconv_geo_fwd_planes_kernel); the mirrored pole rows come from the tile
template <int K, bool ADD>
__global__ void __launch_bounds__(256, 5)
dwconv_geo_dgrad_planes_kernel(const float* __restrict__ gy, const float* __restrict__ w,
                               const float* __restrict__ addend, float* __restrict__ gx,
                               int C, int H, int64_t planes) {
  constexpr int P = (K - 1) / 2, LW = TW + K - 1, W = TW;
  __shared__ float tile[(TH + K - 1) * (TW + K - 1)];
  const int xl = threadIdx.x & 63, r0 = (threadIdx.x >> 6) * RPT;
  const int64_t first = (int64_t)blockIdx.x * PLANE_CHUNK;
  const int n = (int)min((int64_t)PLANE_CHUNK, planes - first);
  PlaneStager<K> sg;
  sg.init(H);
  f32x4 q[2];
  float hv[2];
  sg.load(gy + first * (int64_t)H * W, q, hv);
  for (int i = 0; i < n; ++i) {
    const int64_t plane = first + i;
    const float* wc = w + (int64_t)(plane % C) * K * K;
    sg.store(tile, q, hv);
    __syncthreads();
    if (i + 1 < n) sg.load(gy + (plane + 1) * (int64_t)H * W, q, hv);
    const unsigned o0 = (unsigned)(r0 * W + xl) * 4u;
    float av[RPT];                  // this plane's addend values: in flight under the stencil arithmetic
    if (ADD) {
      const ubase_t ab = uniform_base(addend + plane * (int64_t)H * W);
#pragma unroll
      for (int o = 0; o < RPT; ++o) av[o] = (r0 + o < H) ? load_at<float>(ab + o * W * 4, o0) : 0.f;
    }
    float wr[K * K];
#pragma unroll
    for (int j = 0; j < K * K; ++j) wr[j] = wc[j];
    float acc[RPT];
#pragma unroll
    for (int o = 0; o < RPT; ++o) acc[o] = 0.f;
#pragma unroll
    for (int rr = 0; rr < RPT + K - 1; ++rr) {
      const int ii = r0 + rr - P;   // image row of this tile row (wave-uniform)
      float val[K];
#pragma unroll
      for (int b = 0; b < K; ++b) val[b] = tile[(r0 + rr) * LW + xl + b];
      if (ii >= 0 && ii < H) {
#pragma unroll
        for (int a = 0; a < K; ++a) {
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
            const int yy = r0 + o;
            const bool feeds = (ii < 0) ? (yy >= 1) : (yy <= H - 2);
            if (feeds) {
#pragma unroll
              for (int b = 0; b < K; ++b) acc[o] += wr[a * K + (K - 1 - b)] * val[b];
            }
          }
        }
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    const ubase_t gp = uniform_base(gx + plane * (int64_t)H * W);
    constexpr int half = W >> 1;
#pragma unroll
    for (int o = 0; o < RPT; ++o) {
      const int yy = r0 + o;
      if (yy < H) {
        float extra = 0.f;
        const bool south = yy >= 1 && yy <= P, north = yy >= H - 1 - P && yy <= H - 2;
        if (south || north) {
          const int a = south ? P - yy : P + (H - 1 - yy);   // dr = -yy  resp.  H-1-yy
          const int prow = south ? 0 : H - 1;
#pragma unroll
          for (int b = 0; b < K; ++b) {     // dc = P - b
            int col = xl + P - b + half;
            if (col >= W) col -= W;
            if (col >= W) col -= W;
            extra += wc[a * K + b] * tile[(prow + P) * LW + col + P];
          }
        }
        store_at<float>(gp + o * W * 4, o0, ADD ? (acc[o] + extra) + av[o] : acc[o] + extra);   // (= the two-pass sum, bit for bit)
      }
    }
    __syncthreads();
  }
}

// whole-plane path of the weight gradient: the items of a chunk are whole planes (sample n, channel c); the next
// item's x plane and gy rows are loaded while the current one is accumulated
template <int K>
__global__ void __launch_bounds__(256, 5)
dwconv_geo_wgrad_planes_kernel(const float* __restrict__ gy, const float* __restrict__ x,
                               float* __restrict__ partial, int B, int C, int H, int chunks) {
  constexpr int LW = TW + K - 1, NW = K * K + 1, W = TW;
  __shared__ float tile[(TH + K - 1) * (TW + K - 1)];
  __shared__ float red[4][NW];
  const int c = blockIdx.x / chunks, chunk = blockIdx.x - c * chunks;
  const int xl = threadIdx.x & 63, wave = threadIdx.x >> 6, r0l = wave * RPT;
  float acc[K * K];
#pragma unroll
  for (int i = 0; i < K * K; ++i) acc[i] = 0.f;
  float gsum = 0.f;
  PlaneStager<K> sg;
  sg.init(H);
  f32x4 q[2];
  float hv[2], gn[RPT];
  const unsigned g0 = (unsigned)(r0l * W + xl) * 4u;
  auto fetch = [&](int item) __attribute__((always_inline)) {
    const int64_t off = ((int64_t)item * C + c) * (int64_t)H * W;
    sg.load(x + off, q, hv);
    const ubase_t gb = uniform_base(gy + off);
#pragma unroll
    for (int o = 0; o < RPT; ++o) gn[o] = (r0l + o < H) ? load_at<float>(gb + o * W * 4, g0) : 0.f;
  };
  // rows of the tile beyond the padded plane (H < 32: a wave's strip may overshoot) are never staged: they meet
  // cotangent rows that are zero, and 0 x uninitialised LDS could be 0 x NaN - define them once
  for (int i = threadIdx.x; i < (TH + K - 1) * (TW + K - 1); i += 256) tile[i] = 0.f;
  __syncthreads();
  if (chunk < B) fetch(chunk);
  for (int item = chunk; item < B; item += chunks) {
    sg.store(tile, q, hv);
    float g[RPT];
#pragma unroll
    for (int o = 0; o < RPT; ++o) { g[o] = gn[o]; gsum += g[o]; }
    __syncthreads();
    if (item + chunks < B) fetch(item + chunks);
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
    __syncthreads();
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

// Data gradient AND weight gradient of the whole-plane path in one pass (round 4): both read the cotangent plane; run
// apart they move gy twice (812 MB per 32x64 B=32 layer at C = 1024), together once (603 MB).  The workgroup is the
// weight-gradient kernel's - one channel, the samples of a chunk, the 26 sums in registers across planes - and stages
// TWO tiles per plane: gy with its geocyclic extension (what the data gradient convolves) and x with its halo; the
// cotangent values the weight gradient multiplies are the centre of the gy tile.  Same arithmetic in the same order as
// dwconv_geo_dgrad_planes_kernel and dwconv_geo_wgrad_planes_kernel: bit-identical results.
// GY16 (round 6, bf16-mixed mode): gy is a bf16 tensor - the data gradient of the SepConv's pointwise GEMM, which consumed
// the stencil's bf16-stored output (bf16-valued in the reference's autocast backward too).
template <int K, bool ADD, bool GY16 = false>
__global__ void __launch_bounds__(256, 4)
dwconv_geo_bwd_planes_kernel(const float* __restrict__ gy, const float* __restrict__ x, const float* __restrict__ w,
                             const float* __restrict__ addend, float* __restrict__ gx, float* __restrict__ partial,
                             int B, int C, int H, int chunks) {
  constexpr int P = (K - 1) / 2, LW = TW + K - 1, NW = K * K + 1, W = TW, TN = (TH + K - 1) * (TW + K - 1);
  __shared__ float tg[TN], tx[TN];
  __shared__ float red[4][NW];
  const int c = blockIdx.x / chunks, chunk = blockIdx.x - c * chunks;
  const int xl = threadIdx.x & 63, wave = threadIdx.x >> 6, r0 = wave * RPT;
  const float* wc = w + (int64_t)c * K * K;
  float accw[K * K];
#pragma unroll
  for (int i = 0; i < K * K; ++i) accw[i] = 0.f;
  float gsum = 0.f;
  PlaneStager<K> sg;
  sg.init(H);
  f32x4 qg[2], qx[2];
  float hg[2], hx[2];
  const unsigned o0 = (unsigned)(r0 * W + xl) * 4u;
  auto fetch = [&](int item) __attribute__((always_inline)) {
    const int64_t off = ((int64_t)item * C + c) * (int64_t)H * W;
    if constexpr (GY16) sg.load16(reinterpret_cast<const uint16_t*>(gy) + off, qg, hg);
    else sg.load(gy + off, qg, hg);
    sg.load(x + off, qx, hx);
  };
  // (rows of the tiles beyond the padded plane are never staged: define them once - see the weight-gradient kernel)
  for (int i = threadIdx.x; i < TN; i += 256) { tg[i] = 0.f; tx[i] = 0.f; }
  __syncthreads();
  if (chunk < B) fetch(chunk);
  for (int item = chunk; item < B; item += chunks) {
    const int64_t off = ((int64_t)item * C + c) * (int64_t)H * W;
    if constexpr (GY16) sg.store16(tg, qg, hg); else sg.store(tg, qg, hg);
    sg.store(tx, qx, hx);
    __syncthreads();
    if (item + chunks < B) fetch(item + chunks);
    float av[RPT];
    if (ADD) {
      const ubase_t ab = uniform_base(addend + off);
#pragma unroll
      for (int o = 0; o < RPT; ++o) av[o] = (r0 + o < H) ? load_at<float>(ab + o * W * 4, o0) : 0.f;
    }
    // ---- data gradient of this plane (dwconv_geo_dgrad_planes_kernel)
    {
      float wr[K * K];
#pragma unroll
      for (int j = 0; j < K * K; ++j) wr[j] = wc[j];
      float acc[RPT];
#pragma unroll
      for (int o = 0; o < RPT; ++o) acc[o] = 0.f;
#pragma unroll
      for (int rr = 0; rr < RPT + K - 1; ++rr) {
        const int ii = r0 + rr - P;   // image row of this tile row (wave-uniform)
        float val[K];
#pragma unroll
        for (int b = 0; b < K; ++b) val[b] = tg[(r0 + rr) * LW + xl + b];
        if (ii >= 0 && ii < H) {
#pragma unroll
          for (int a = 0; a < K; ++a) {
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
              const int yy = r0 + o;
              const bool feeds = (ii < 0) ? (yy >= 1) : (yy <= H - 2);
              if (feeds) {
#pragma unroll
                for (int b = 0; b < K; ++b) acc[o] += wr[a * K + (K - 1 - b)] * val[b];
              }
            }
          }
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      const ubase_t gp = uniform_base(gx + off);
      constexpr int half = W >> 1;
#pragma unroll
      for (int o = 0; o < RPT; ++o) {
        const int yy = r0 + o;
        if (yy < H) {
          float extra = 0.f;
          const bool south = yy >= 1 && yy <= P, north = yy >= H - 1 - P && yy <= H - 2;
          if (south || north) {
            const int a = south ? P - yy : P + (H - 1 - yy);
            const int prow = south ? 0 : H - 1;
#pragma unroll
            for (int b = 0; b < K; ++b) {
              int col = xl + P - b + half;
              if (col >= W) col -= W;
              if (col >= W) col -= W;
              extra += wc[a * K + b] * tg[(prow + P) * LW + col + P];
            }
          }
          store_at<float>(gp + o * W * 4, o0, ADD ? (acc[o] + extra) + av[o] : acc[o] + extra);
        }
      }
    }
    // ---- weight gradient: this plane's share of the channel's sums (dwconv_geo_wgrad_planes_kernel)
    {
      float g[RPT];
#pragma unroll
      for (int o = 0; o < RPT; ++o) {
        g[o] = (r0 + o < H) ? tg[(r0 + o + P) * LW + xl + P] : 0.f;
        gsum += g[o];
      }
#pragma unroll
      for (int rr = 0; rr < RPT + K - 1; ++rr) {
        float val[K];
#pragma unroll
        for (int b = 0; b < K; ++b) val[b] = tx[(r0 + rr) * LW + xl + b];
#pragma unroll
        for (int a = 0; a < K; ++a) {
          const int o = rr - a;
          if (o >= 0 && o < RPT) {
#pragma unroll
            for (int b = 0; b < K; ++b) accw[a * K + b] += g[o] * val[b];
          }
        }
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < K * K; ++i) {
    float s = wave_sum_dpp(accw[i]);
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

// ---------------------------------------------------------------------------- staged tiles of the larger grids
// Grids of more than one tile (128x256, 721x1440, ...; k = 5): the whole-plane kernels' structure - 16-byte loads from
// per-thread offsets computed once, the next item's loads in flight under the current item's arithmetic - on 32x64
// tiles that are always FULL: the last tile row / column starts at H - 32 / W - 64, overlapping its neighbour, and
// owns (stores, and counts in the weight gradient) only the rows / columns its neighbour does not.  A full tile has
// one fixed shape: 512 aligned float4 of interior and a 400-cell halo ring through the index map, two of each per
// thread, whatever the position.
template <int K>
struct TileStager {
  static constexpr int P = (K - 1) / 2, LW = TW + K - 1;
  unsigned vsrc[2], hsrc[2];
  int vdst[2], hdst[2];
  __device__ __forceinline__ void init(int H, int W, int ty0, int tx0) {
    constexpr int w4 = TW / 4, hc = 2 * P, nhalo_rows = 2 * P * LW, nhalo = nhalo_rows + TH * hc;
    static_assert(TH * w4 == 512 && nhalo <= 512, "two interior vectors and two halo cells per thread");
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int v = threadIdx.x + 256 * j;
      const int y = v / w4, x4 = v - y * w4;
      vsrc[j] = (unsigned)((ty0 + y) * W + tx0 + 4 * x4) * 4u;          // byte offsets in the plane
      vdst[j] = (y + P) * LW + P + 4 * x4;
      const int kk = threadIdx.x + 256 * j, k = min(kk, nhalo - 1);
      int lr, lc;
      if (k < nhalo_rows) {
        const int rr = k / LW;
        lc = k - rr * LW;
        lr = rr < P ? rr : TH + rr;
      } else {
        const int e = k - nhalo_rows, rr = e / hc, cc = e - rr * hc;
        lr = rr + P;
        lc = cc < P ? cc : TW + cc;
      }
      int sr, sc;
      geo_src(ty0 + lr - P, tx0 + lc - P, H, W, sr, sc);
      hsrc[j] = (unsigned)(sr * W + sc) * 4u;
      hdst[j] = kk < nhalo ? lr * LW + lc : -1;
    }
  }
  __device__ __forceinline__ void load(const float* __restrict__ F, f32x4 (&q)[2], float (&hv)[2]) const {
    const ubase_t b = uniform_base(F);
#pragma unroll
    for (int j = 0; j < 2; ++j) { q[j] = load_at<f32x4>(b, vsrc[j]); hv[j] = load_at<float>(b, hsrc[j]); }
  }
  __device__ __forceinline__ void store(float* tile, const f32x4 (&q)[2], const float (&hv)[2]) const {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      float2* d = reinterpret_cast<float2*>(tile + vdst[j]);      // 8-byte aligned (P, LW even)
      d[0] = make_float2(q[j].x, q[j].y);
      d[1] = make_float2(q[j].z, q[j].w);
      if (hdst[j] >= 0) tile[hdst[j]] = hv[j];
    }
  }
};

// position of tile t: (ty0, tx0) = where it is staged from, (ny0, nx0) = the first row / column it owns
struct TilePos { int ty0, tx0, ny0, nx0; };
__device__ __forceinline__ TilePos tile_pos(int t, int tiles_x, int H, int W) {
  const int tyi = t / tiles_x, txi = t - tyi * tiles_x;
  TilePos p;
  p.ny0 = tyi * TH; p.nx0 = txi * TW;
  p.ty0 = min(p.ny0, H - TH); p.tx0 = min(p.nx0, W - TW);
  return p;
}

// forward: a workgroup walks PLANE_CHUNK planes at one tile position
template <int K, bool Y16 = false>
__global__ void __launch_bounds__(256, 5)
dwconv_geo_fwd_tiles_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                            float* __restrict__ y, int C, int H, int W, int tiles_x, int tiles, int64_t planes) {
  __shared__ float tile[(TH + K - 1) * (TW + K - 1)];
  const int L = xcd_contiguous((int)blockIdx.x, (int)gridDim.x);
  const int chunk = L / tiles, t = L - chunk * tiles;
  const TilePos tp = tile_pos(t, tiles_x, H, W);
  const int xl = threadIdx.x & 63, r0l = (threadIdx.x >> 6) * RPT;
  const int64_t first = (int64_t)chunk * PLANE_CHUNK, PS = (int64_t)H * W;
  const int n = (int)min((int64_t)PLANE_CHUNK, planes - first);
  TileStager<K> sg;
  sg.init(H, W, tp.ty0, tp.tx0);
  f32x4 q[2];
  float hv[2];
  sg.load(x + first * PS, q, hv);
  constexpr int ES = Y16 ? 2 : 4;
  const unsigned o0 = (unsigned)((tp.ty0 + r0l) * W + tp.tx0 + xl) * (unsigned)ES;
  const bool col_owned = tp.tx0 + xl >= tp.nx0;
  const int own0 = tp.ny0 - tp.ty0 - r0l;           // rows o >= own0 of this thread's strip are owned
  for (int i = 0; i < n; ++i) {
    const int64_t plane = first + i;
    const int c = (int)(plane % C);
    sg.store(tile, q, hv);
    __syncthreads();
    if (i + 1 < n) sg.load(x + (plane + 1) * PS, q, hv);
    float acc[RPT];
    tile_stencil<K, false>(tile, w + (int64_t)c * K * K, acc);
    const float bv = bias ? bias[c] : 0.f;
    const ubase_t yp = uniform_base(reinterpret_cast<const char*>(y) + plane * PS * ES);
#pragma unroll
    for (int o = 0; o < RPT; ++o)
      if (col_owned && o >= own0) {
        if constexpr (Y16) store_at<uint16_t>(yp + (int64_t)o * W * ES, o0, bf16_bits(acc[o] + bv));
        else store_at<float>(yp + (int64_t)o * W * ES, o0, acc[o] + bv);
      }
    __syncthreads();
  }
}

// item -> (tile, sample) of a channel's B x tiles items.  Tile fastest: a workgroup's contiguous range of items walks
// the tiles of one plane in row-major order, so the halo cells a tile shares with its left neighbour were read by the
// same CU one item earlier (L2 hits); sample fastest would keep the stager's offsets across items instead.
__device__ __forceinline__ void item_of(int item, int B, int tiles, int& t, int& n) {
  if (DWCONV_BWD_TFAST) { n = item / tiles; t = item - n * tiles; }
  else { t = item / B; n = item - t * B; }
}

// both gradients in one pass (dwconv_geo_bwd_planes_kernel's arithmetic on tiles): workgroup (channel c, chunk) walks a
// contiguous range of the channel's B x tiles items (item_of); the 26 sums stay in registers across items.  The
// standalone entry points run the same kernel with one half compiled out: whichever way the gradients are asked for,
// the bits are the same.  (The data gradient is also the one-tile-per-workgroup kernel's sum in the same order; the
// weight gradient partitions its sum differently from dwconv_geo_wgrad_kernel: same terms, another fixed order.)
template <int K, bool ADD, bool DG, bool WG>   // DG: data gradient, WG: weight gradient (either alone = the standalone entry points)
__global__ void __launch_bounds__(256, 4)
dwconv_geo_bwd_tiles_kernel(const float* __restrict__ gy, const float* __restrict__ x, const float* __restrict__ w,
                            const float* __restrict__ addend, float* __restrict__ gx, float* __restrict__ partial,
                            int B, int C, int H, int W, int tiles_x, int tiles, int chunks, int per) {
  constexpr int P = (K - 1) / 2, LW = TW + K - 1, NW = K * K + 1, TN = (TH + K - 1) * (TW + K - 1);
  __shared__ float tg[TN], tx[TN];
  __shared__ float red[4][NW];
  const int c = blockIdx.x / chunks, chunk = blockIdx.x - c * chunks;
  const int items = B * tiles, i0 = chunk * per, i1 = min(items, i0 + per);
  const int xl = threadIdx.x & 63, wave = threadIdx.x >> 6, r0 = wave * RPT;
  const float* wc = w + (int64_t)c * K * K;
  const int64_t PS = (int64_t)H * W;
  const int half = W >> 1;
  float accw[K * K];
#pragma unroll
  for (int i = 0; i < K * K; ++i) accw[i] = 0.f;
  float gsum = 0.f;
  TileStager<K> sg;
  f32x4 qg[2], qx[2];
  float hg[2], hx[2];
  int staged_t = -1;
  auto fetch = [&](int item) __attribute__((always_inline)) {
    int t, n;
    item_of(item, B, tiles, t, n);
    if (t != staged_t) {                                       // (wave-uniform)
      const TilePos np = tile_pos(t, tiles_x, H, W);
      sg.init(H, W, np.ty0, np.tx0);
      staged_t = t;
    }
    const int64_t off = ((int64_t)n * C + c) * PS;
    sg.load(gy + off, qg, hg);
    if (WG) sg.load(x + off, qx, hx);
  };
  if (i0 < i1) fetch(i0);
  for (int item = i0; item < i1; ++item) {
    int t, n;
    item_of(item, B, tiles, t, n);
    const TilePos tp = tile_pos(t, tiles_x, H, W);
    const int64_t off = ((int64_t)n * C + c) * PS;
    const float* gpl = gy + off;
    sg.store(tg, qg, hg);
    if (WG) sg.store(tx, qx, hx);
    __syncthreads();
    if (item + 1 < i1) fetch(item + 1);
    const unsigned o0 = (unsigned)((tp.ty0 + r0) * W + tp.tx0 + xl) * 4u;
    const int xx = tp.tx0 + xl;
    const bool col_owned = xx >= tp.nx0;
    const int own0 = tp.ny0 - tp.ty0 - r0;
    float av[RPT];
    if (ADD) {
      const ubase_t ab = uniform_base(addend + off);
#pragma unroll
      for (int o = 0; o < RPT; ++o) av[o] = load_at<float>(ab + (int64_t)o * W * 4, o0);
    }
    // ---- data gradient of this tile (dwconv_geo_dgrad_kernel)
    if constexpr (DG) {
      float wr[K * K];
#pragma unroll
      for (int j = 0; j < K * K; ++j) wr[j] = wc[j];
      float acc[RPT];
#pragma unroll
      for (int o = 0; o < RPT; ++o) acc[o] = 0.f;
#pragma unroll
      for (int rr = 0; rr < RPT + K - 1; ++rr) {
        const int ii = tp.ty0 + r0 + rr - P;   // image row of this tile row (wave-uniform)
        float val[K];
#pragma unroll
        for (int b = 0; b < K; ++b) val[b] = tg[(r0 + rr) * LW + xl + b];
        if (ii >= 0 && ii < H) {
#pragma unroll
          for (int a = 0; a < K; ++a) {
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
              const int yy = tp.ty0 + r0 + o;
              const bool feeds = (ii < 0) ? (yy >= 1) : (yy <= H - 2);
              if (feeds) {
#pragma unroll
                for (int b = 0; b < K; ++b) acc[o] += wr[a * K + (K - 1 - b)] * val[b];
              }
            }
          }
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      const ubase_t gp = uniform_base(gx + off);
#pragma unroll
      for (int o = 0; o < RPT; ++o) {
        const int yy = tp.ty0 + r0 + o;
        float extra = 0.f;
        const bool south = yy >= 1 && yy <= P, north = yy >= H - 1 - P && yy <= H - 2;
        if (south || north) {                   // (wave-uniform; the W/2-shifted pole row comes from memory)
          const int a = south ? P - yy : P + (H - 1 - yy);
          const int prow = south ? 0 : H - 1;
#pragma unroll
          for (int b = 0; b < K; ++b) {
            int col = xx + P - b + half;
            if (col >= W) col -= W;
            if (col >= W) col -= W;
            extra += wc[a * K + b] * gpl[(int64_t)prow * W + col];
          }
        }
        if (col_owned && o >= own0)
          store_at<float>(gp + (int64_t)o * W * 4, o0, ADD ? (acc[o] + extra) + av[o] : acc[o] + extra);
      }
    }
    // ---- weight gradient: the owned points' share of the channel's sums
    if constexpr (WG) {
      float g[RPT];
#pragma unroll
      for (int o = 0; o < RPT; ++o) {
        g[o] = (col_owned && o >= own0) ? tg[(r0 + o + P) * LW + xl + P] : 0.f;
        gsum += g[o];
      }
#pragma unroll
      for (int rr = 0; rr < RPT + K - 1; ++rr) {
        float val[K];
#pragma unroll
        for (int b = 0; b < K; ++b) val[b] = tx[(r0 + rr) * LW + xl + b];
#pragma unroll
        for (int a = 0; a < K; ++a) {
          const int o = rr - a;
          if (o >= 0 && o < RPT) {
#pragma unroll
            for (int b = 0; b < K; ++b) accw[a * K + b] += g[o] * val[b];
          }
        }
      }
    }
    __syncthreads();
  }
  if (!WG) return;
#pragma unroll
  for (int i = 0; i < K * K; ++i) {
    float s = wave_sum_dpp(accw[i]);
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

// ---- kernel tables, indexed by the boolean template parameters --------------------------------------------------------
using FwdPlanesKernel = decltype(&dwconv_geo_fwd_planes_kernel<5, false>);
constexpr FwdPlanesKernel FWD_PLANES[2] = {&dwconv_geo_fwd_planes_kernel<5, false>, &dwconv_geo_fwd_planes_kernel<5, true>};   // [Y16]
using DgradPlanesKernel = decltype(&dwconv_geo_dgrad_planes_kernel<5, false>);
constexpr DgradPlanesKernel DGRAD_PLANES[2] = {&dwconv_geo_dgrad_planes_kernel<5, false>, &dwconv_geo_dgrad_planes_kernel<5, true>};   // [ADD]
using BwdPlanesKernel = decltype(&dwconv_geo_bwd_planes_kernel<5, false, false>);
constexpr BwdPlanesKernel BWD_PLANES[2][2] = {      // [ADD][GY16]
    {&dwconv_geo_bwd_planes_kernel<5, false, false>, &dwconv_geo_bwd_planes_kernel<5, false, true>},
    {&dwconv_geo_bwd_planes_kernel<5, true, false>, &dwconv_geo_bwd_planes_kernel<5, true, true>}};

using FwdTilesKernel = decltype(&dwconv_geo_fwd_tiles_kernel<5, false>);
constexpr FwdTilesKernel FWD_TILES[2] = {&dwconv_geo_fwd_tiles_kernel<5, false>, &dwconv_geo_fwd_tiles_kernel<5, true>};   // [Y16]
using BwdTilesKernel = decltype(&dwconv_geo_bwd_tiles_kernel<5, false, true, true>);
enum BwdHalf { DGRAD, WGRAD, BOTH };      // <DG, WG> = <true, false>, <false, true>, <true, true>
constexpr BwdTilesKernel BWD_TILES[3][2] = {         // [BwdHalf][ADD]; the weight gradient alone has no addend
    {&dwconv_geo_bwd_tiles_kernel<5, false, true, false>, &dwconv_geo_bwd_tiles_kernel<5, true, true, false>},
    {&dwconv_geo_bwd_tiles_kernel<5, false, false, true>, &dwconv_geo_bwd_tiles_kernel<5, false, false, true>},
    {&dwconv_geo_bwd_tiles_kernel<5, false, true, true>, &dwconv_geo_bwd_tiles_kernel<5, true, true, true>}};

// the tensors of the half that is compiled out are not passed on
int launch_bwd_tiles(const DwArgs& a, BwdHalf half) {
  const DwGeom g = dw_bwd_tiles_geom(a);
  const int tiles = dw_tiles(a.H, a.W);
  const bool dg = half != WGRAD, wg = half != DGRAD;
  const float* none = nullptr;
  float* nowhere = nullptr;
  hipLaunchKernelGGL(BWD_TILES[half][dg && a.addend != nullptr], dim3((unsigned)g.grid), dim3(256), 0, a.st, a.gy,
                     wg ? a.x : none, dg ? a.w : none, dg ? a.addend : none, dg ? a.gx : nowhere,
                     wg ? a.partial : nowhere, a.B, a.C, a.H, a.W, dw_tiles_x(a.W), tiles, g.chunks, g.per);
  return g.chunks;
}

}  // namespace

void pd_dw_fwd_planes(const DwArgs& a, bool y16) {
  hipLaunchKernelGGL(FWD_PLANES[y16], dim3((unsigned)dw_fwd_geom(DwSched::Planes, a).grid), dim3(256), 0, a.st, a.x, a.w,
                     a.bias, a.y, a.C, a.H, (int64_t)a.B * a.C);
}

void pd_dw_dgrad_planes(const DwArgs& a) {
  hipLaunchKernelGGL(DGRAD_PLANES[a.addend != nullptr], dim3((unsigned)dw_dgrad_geom(DwSched::Planes, a).grid), dim3(256), 0,
                     a.st, a.gy, a.w, a.addend, a.gx, a.C, a.H, (int64_t)a.B * a.C);
}

int pd_dw_wgrad_planes(const DwArgs& a) {
  const DwGeom g = dw_wgrad_geom(DwSched::Planes, a);
  hipLaunchKernelGGL(dwconv_geo_wgrad_planes_kernel<5>, dim3((unsigned)g.grid), dim3(256), 0, a.st, a.gy, a.x, a.partial,
                     a.B, a.C, a.H, g.chunks);
  return g.chunks;
}

int pd_dw_bwd_planes(const DwArgs& a, bool gy16) {
  const DwGeom g = dw_wgrad_geom(DwSched::Planes, a);
  hipLaunchKernelGGL(BWD_PLANES[a.addend != nullptr][gy16], dim3((unsigned)g.grid), dim3(256), 0, a.st, a.gy, a.x, a.w,
                     a.addend, a.gx, a.partial, a.B, a.C, a.H, g.chunks);
  return g.chunks;
}

void pd_dw_fwd_tiles(const DwArgs& a, bool y16) {
  hipLaunchKernelGGL(FWD_TILES[y16], dim3((unsigned)dw_fwd_geom(DwSched::Tiles, a).grid), dim3(256), 0, a.st, a.x, a.w,
                     a.bias, a.y, a.C, a.H, a.W, dw_tiles_x(a.W), dw_tiles(a.H, a.W), (int64_t)a.B * a.C);
}

void pd_dw_dgrad_tiles(const DwArgs& a) { launch_bwd_tiles(a, DGRAD); }   // the one-pass kernel's data-gradient half
int pd_dw_wgrad_tiles(const DwArgs& a) { return launch_bwd_tiles(a, WGRAD); }   // its weight-gradient half
int pd_dw_bwd_tiles(const DwArgs& a) { return launch_bwd_tiles(a, BOTH); }
