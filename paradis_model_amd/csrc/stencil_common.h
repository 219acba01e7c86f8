// What the translation units of the depthwise stencil on the virtual geocyclic halo share: stencil.hip (the C ABI,
// check_dw, the schedule choice, dwconv_wgrad_finish), stencil_planes.hip (the two k = 5 families: whole planes - W = 64,
// H <= 32 - and staged full tiles of the larger grids) and stencil_generic.hip (one tile per workgroup, every k in
// 1..11), each family with both directions and its launchers.  The call's arguments, the tile constants and A/B knobs,
// tile staging and the forward stencil, the scalar-base accessors, the chunk formulas of the weight gradient and the
// schedule choice (host only: tools/stencil_sched_check.hip includes this header).  Everything below the declarations
// sits in an anonymous namespace.
#pragma once
#include <algorithm>
#include <initializer_list>
#include "common.h"

// One call of paradis_dwconv_geo_*; a tensor the entry point does not have is nullptr
struct DwArgs {
  const float* gy; const float* x; const float* w; const float* bias; const float* addend;
  float* y; float* gx; float* gw; float* gbias;
  float* partial;           // the workspace (paradis_dwconv_geo_wgrad_ws_bytes): partial[c][chunk][k*k + 1]
  int B, C, H, W, k;
  hipStream_t st;
};

// Launchers, one per family and direction (stencil.hip picks: dw_schedule); the caller checks the launch
// (PD_CHECK_LAUNCH).  y16: y is a bf16 tensor; gy16: gy is.  The weight-gradient and one-pass launchers fill a.partial
// and return the chunks per channel that dwconv_wgrad_finish (stencil.hip) then sums.
void pd_dw_fwd_planes(const DwArgs& a, bool y16);       // stencil_planes.hip
void pd_dw_dgrad_planes(const DwArgs& a);
int pd_dw_wgrad_planes(const DwArgs& a);
int pd_dw_bwd_planes(const DwArgs& a, bool gy16);
void pd_dw_fwd_tiles(const DwArgs& a, bool y16);
void pd_dw_dgrad_tiles(const DwArgs& a);
int pd_dw_wgrad_tiles(const DwArgs& a);
int pd_dw_bwd_tiles(const DwArgs& a);
void pd_dw_fwd_generic(const DwArgs& a, bool y16, int whole_vec4);      // stencil_generic.hip
void pd_dw_dgrad_generic(const DwArgs& a, int whole_vec4);
int pd_dw_wgrad_generic(const DwArgs& a, int whole_vec4);

namespace {

constexpr int TH = 32, TW = 64;  // output tile; 256 threads: lane -> column, wave -> 8-row strip
constexpr int RPT = 8;           // rows per thread

// Stage a (TH+K-1) x (TW+K-1) tile, flat over the 256 threads (a row-per-wave variant measured
// 25-30 % slower: the 68-wide rows leave most lanes of the second pass idle).  Loads are issued in
// batches from clamped, always-valid addresses and selected afterwards: a load under a per-lane
// condition makes the compiler wait for each one separately (one memory round trip per element).
template <int K, bool GEO>
__device__ __forceinline__ void stage_tile(float* tile, const float* __restrict__ src, int H, int W,
                                           int ty0, int tx0) {
  constexpr int P = (K - 1) / 2, LW = TW + K - 1, LH = TH + K - 1, N = LH * LW, BATCH = 5;
  for (int i0 = threadIdx.x; i0 < N; i0 += 256 * BATCH) {
    float val[BATCH];
#pragma unroll
    for (int j = 0; j < BATCH; ++j) {
      const int i = min(i0 + 256 * j, N - 1);
      const int lr = i / LW, lc = i - lr * LW;
      const int ii = ty0 + lr - P, jj = tx0 + lc - P;
      bool valid;
      int r, c;
      if (GEO) {
        valid = ii < H + P && jj < W + P;
        geo_src(min(ii, H + P - 1), min(jj, W + P - 1), H, W, r, c);
      } else {
        valid = ii >= 0 && ii < H && jj >= 0 && jj < W;
        r = min(max(ii, 0), H - 1); c = min(max(jj, 0), W - 1);
      }
      const float v = src[(int64_t)r * W + c];
      val[j] = valid ? v : 0.f;
    }
#pragma unroll
    for (int j = 0; j < BATCH; ++j)
      if (i0 + 256 * j < N) tile[i0 + 256 * j] = val[j];
  }
}

// the tile is the whole padded plane (W == TW, H <= TH, 16-byte aligned plane, even halo): plain
// 16-byte copy of the interior, only the halo ring through the index map (common.h)
template <int K>
__device__ __forceinline__ void stage_any(float* tile, const float* __restrict__ src, int H, int W, int ty0,
                                          int tx0, bool whole_vec4) {
  if (whole_vec4) stage_plane_vec4(tile, src, H, W, (K - 1) / 2);
  else stage_tile<K, true>(tile, src, H, W, ty0, tx0);
}

// a wave-uniform base address pinned to scalar registers plus an unsigned 32-bit BYTE offset per lane: the access is
// `global_load/store v, v_off, s[base:base+1]` - no 64-bit address arithmetic, no 64-bit addresses kept in registers
// (with typed indexing the compiler only finds this form for 4-byte elements)
typedef __attribute__((address_space(1))) char* ubase_t;
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));   // (HIP's float4 struct cannot be read through an address-space pointer on the host pass)
__device__ __forceinline__ ubase_t uniform_base(const void* p) {
  const uint64_t a = (uint64_t)p;
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)a), hi = __builtin_amdgcn_readfirstlane((uint32_t)(a >> 32));
  return (ubase_t)(((uint64_t)hi << 32) | lo);
}
// (the empty asm keeps the 32-bit offset opaque at the access: otherwise the loop optimiser widens it once to a 64-bit
//  per-thread address, carries that through the plane loop - two registers per access - and adds the base on the
//  vector unit)
template <typename T>
__device__ __forceinline__ T load_at(ubase_t b, unsigned off) {
  asm volatile("" : "+v"(off));
  return *(const __attribute__((address_space(1))) T*)(b + off);
}
template <typename T>
__device__ __forceinline__ void store_at(ubase_t b, unsigned off, T v) {
  asm volatile("" : "+v"(off));
  *(__attribute__((address_space(1))) T*)(b + off) = v;
}

#ifndef DWCONV_PLANE_CHUNK       // (A/B builds)
#define DWCONV_PLANE_CHUNK 4
#endif
constexpr int PLANE_CHUNK = DWCONV_PLANE_CHUNK;   // planes per workgroup on the whole-plane path (and per tile position on the staged-tiles forward)
#ifndef DWCONV_PLANES            // (A/B builds: 0 = one plane per workgroup)
#define DWCONV_PLANES 1
#endif
#ifndef DWCONV_BWD_FUSED         // (A/B builds: 0 = paradis_dwconv_geo_bwd runs the two separate kernels)
#define DWCONV_BWD_FUSED 1
#endif
#ifndef DWCONV_BWD_TFAST         // (A/B builds: item order of the staged-tiles backward: item_of)
#define DWCONV_BWD_TFAST 1
#endif
#ifndef DWCONV_TILES             // (A/B builds: 0 = the one-tile-per-workgroup kernels on every larger grid)
#define DWCONV_TILES 1
#endif

// FLIP=false: y = w (*) geo-padded x  (+bias).   FLIP=true: self-alias part of the data gradient.
template <int K, bool FLIP>
__device__ __forceinline__ void tile_stencil(const float* tile, const float* __restrict__ wc,
                                             float (&acc)[RPT]) {
  constexpr int LW = TW + K - 1;
  const int x = threadIdx.x & 63, r0 = (threadIdx.x >> 6) * RPT;
  float w[K * K];
#pragma unroll
  for (int i = 0; i < K * K; ++i) w[i] = wc[FLIP ? (K * K - 1 - i) : i];
#pragma unroll
  for (int o = 0; o < RPT; ++o) acc[o] = 0.f;
#pragma unroll
  for (int rr = 0; rr < RPT + K - 1; ++rr) {
    float val[K];
#pragma unroll
    for (int b = 0; b < K; ++b) val[b] = tile[(r0 + rr) * LW + x + b];
#pragma unroll
    for (int a = 0; a < K; ++a) {
      const int o = rr - a;
      if (o >= 0 && o < RPT) {
#pragma unroll
        for (int b = 0; b < K; ++b) acc[o] += w[a * K + b] * val[b];
      }
    }
    // (row by row: left alone the scheduler hoists the LDS reads of many rows and the kernel sits at exactly 64
    //  registers with no room for the prefetched plane)
    __builtin_amdgcn_sched_barrier(0);
  }
}

// Y16 (round 6, bf16-mixed mode): y written as bf16 (round to nearest even) for a consumer that is the pointwise GEMM of
// the same SepConv - the value that GEMM rounds its operand to (reference model/blocks.py:107-110 under autocast).
__device__ __forceinline__ uint16_t bf16_bits(float v) { return __builtin_bit_cast(uint16_t, (__bf16)v); }

// consecutive workgroup ids go round the eight XCDs; hand every XCD a contiguous range of logical ids instead: the
// tiles of a plane chunk - neighbours that share halo cells - then run behind one L2
__device__ __forceinline__ int xcd_contiguous(int id, int nwg) {
  const int q = nwg >> 3, r = nwg & 7, xcd = id & 7;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (id >> 3);
}

// ======================================================================================
// host side
// ======================================================================================
inline int dw_tiles_x(int W) { return (W + TW - 1) / TW; }
inline int dw_tiles(int H, int W) { return dw_tiles_x(W) * ((H + TH - 1) / TH); }
inline int64_t dw_plane_chunks(int64_t planes) { return (planes + PLANE_CHUNK - 1) / PLANE_CHUNK; }

// workgroups per channel of the one-tile-per-workgroup and whole-plane weight gradients (items = B x tiles)
int wgrad_chunks(int B, int C, int tiles) {
  int items = B * tiles;
  int chunks = (2048 + C - 1) / C;
  return std::max(1, std::min(chunks, items));
}

// staged-tiles backward: items per workgroup and workgroups per channel (~8192 workgroups: 8 resident sets of the chip)
int bwd_tiles_per(int B, int C, int tiles) {
  const int items = std::max(1, B * tiles);
  const int chunks = std::max(1, std::min((8192 + C - 1) / C, items));
  return (items + chunks - 1) / chunks;
}
int bwd_tiles_chunks(int B, int C, int tiles) {
  const int items = std::max(1, B * tiles), per = bwd_tiles_per(B, C, tiles);
  return (items + per - 1) / per;
}

// ---- the schedule choice ---------------------------------------------------------------------------------------------
enum class DwSched { Planes, Tiles, Generic };

// whole padded plane == one tile and the 16-byte staging path applies (even halo: k = 5)
inline bool dw_planes_shape(int H, int W, int k) { return k == 5 && W == TW && H <= TH && ((int64_t)H * W) % 4 == 0; }
// more than one tile, and the staged full-tile kernels apply: k = 5, at least one full tile each way, rows of whole
// float4, byte offsets in a plane fit 32 bits
inline bool dw_tiles_shape(int H, int W, int k) {
  return k == 5 && H >= TH && W >= TW && (H > TH || W > TW) && W % 4 == 0 && (int64_t)H * W * 4 < (1ll << 32);
}
// every pointer (nullptr: absent) a multiple of `bytes`; a tensor aligned, every plane of it is on both paths
inline bool dw_aligned(std::initializer_list<const void*> ps, uintptr_t bytes) {
  uintptr_t bits = 0;
  for (const void* p : ps) bits |= reinterpret_cast<uintptr_t>(p);
  return (bits & (bytes - 1)) == 0;
}
// `whole_vec4` of the generic kernels (stage_any): the plane they stage is one tile and 16-byte aligned
inline int dw_whole_vec4(int H, int W, int k, const void* staged) {
  return dw_planes_shape(H, W, k) && dw_aligned({staged}, 16);
}

// The family that runs a call.  `staged`: the tensor the call stages into LDS (x forward and in the weight gradient, gy
// in the data gradient); `rest`: the other [B,C,H,W] tensors it reads or writes, nullptr where absent.  The whole-plane
// kernels read `staged` in 16-byte vectors and the rest by element (`elem` bytes: no tensor that is valid at all fails
// that test - the forward, which used to ask nothing of y there, passes the size of y's elements); the staged-tiles
// kernels want 16 bytes of every tensor.  The two shapes exclude each other.
inline DwSched dw_schedule(int H, int W, int k, const void* staged, std::initializer_list<const void*> rest,
                           uintptr_t elem = 4) {
  if (DWCONV_PLANES && dw_whole_vec4(H, W, k, staged) && dw_aligned(rest, elem)) return DwSched::Planes;
  if (DWCONV_TILES && dw_tiles_shape(H, W, k) && dw_aligned({staged}, 16) && dw_aligned(rest, 16)) return DwSched::Tiles;
  return DwSched::Generic;
}

// The schedule of each direction.  Every entry point asks once; paradis_dwconv_geo_bwd asks for both halves.
inline DwSched dw_fwd_schedule(const DwArgs& a, bool y16) { return dw_schedule(a.H, a.W, a.k, a.x, {a.y}, y16 ? 2 : 4); }
inline DwSched dw_dgrad_schedule(const DwArgs& a) { return dw_schedule(a.H, a.W, a.k, a.gy, {a.gx, a.addend}); }
// (an empty batch still writes zero gradients: by the kernels that run with B = 0)
inline DwSched dw_wgrad_schedule(const DwArgs& a) {
  const DwSched s = dw_schedule(a.H, a.W, a.k, a.x, {a.gy});
  return a.B == 0 && s == DwSched::Tiles ? DwSched::Generic : s;
}
// both gradients from one kernel that reads gy once: where the two halves agree on a family that has such a kernel
inline bool dw_one_pass(DwSched dgrad, DwSched wgrad, int B) {
  return B > 0 && dgrad == wgrad && (dgrad == DwSched::Tiles || (dgrad == DwSched::Planes && DWCONV_BWD_FUSED));
}
// Launch geometry of a family, by direction: workgroups, and the chunks per channel / items per workgroup the weight
// gradient and staged-tiles kernels are told.  The launchers take it from here, and so does
// tools/stencil_sched_check.hip.
struct DwGeom { int64_t grid; int chunks, per; };
inline DwGeom dw_bwd_tiles_geom(const DwArgs& a) {       // either half of the staged-tiles backward, or both
  const int tiles = dw_tiles(a.H, a.W), chunks = bwd_tiles_chunks(a.B, a.C, tiles);
  return {(int64_t)a.C * chunks, chunks, bwd_tiles_per(a.B, a.C, tiles)};
}
inline DwGeom dw_fwd_geom(DwSched s, const DwArgs& a) {
  const int64_t planes = (int64_t)a.B * a.C;
  if (s == DwSched::Planes) return {dw_plane_chunks(planes), 0, 0};
  if (s == DwSched::Tiles) return {dw_plane_chunks(planes) * dw_tiles(a.H, a.W), 0, 0};
  return {planes * dw_tiles(a.H, a.W), 0, 0};
}
inline DwGeom dw_dgrad_geom(DwSched s, const DwArgs& a) {
  if (s == DwSched::Tiles) return dw_bwd_tiles_geom(a);
  return dw_fwd_geom(s, a);
}
inline DwGeom dw_wgrad_geom(DwSched s, const DwArgs& a) {      // also the one-pass kernels'
  if (s == DwSched::Tiles) return dw_bwd_tiles_geom(a);
  const int chunks = wgrad_chunks(a.B, a.C, s == DwSched::Planes ? 1 : dw_tiles(a.H, a.W));
  return {(int64_t)a.C * chunks, chunks, 0};
}

// chunks per channel the workspace has room for.  Sizes are asked before the pointers, and with them the schedule, are
// known: the larger of the two counts
inline int dw_ws_chunks(int B, int C, int tiles) { return std::max(wgrad_chunks(B, C, tiles), bwd_tiles_chunks(B, C, tiles)); }

}  // namespace
