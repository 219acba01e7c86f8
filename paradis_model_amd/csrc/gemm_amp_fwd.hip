// Forward / data-gradient kernels of the bf16-mixed scheme (PARADIS_GEMM_BF16) and their launcher pd_amp_launch_fwd,
// called from gemm.hip; shared definitions: gemm_common.h.
#include <cstdlib>
#include "gemm_common.h"

namespace {


// PARADIS_GEMM_BF16 forward / dgrad (the reference's bf16-mixed mode): operands rounded to bf16, ONE
// product.  The 128 x 256 workgroup tile of pw_gemm_split_wide_kernel (two 128-column halves sharing one weight tile),
// but with 32-deep k-tiles: with one product per k the k16 structure leaves four MFMAs per wave between two barriers and
// 32 KB of fp32 activations in flight per workgroup - the kernel then waits on its own per-tile chain, not on the
// matrix pipe or on bytes.  Here a tile is two k16 SLICES: eight MFMAs per wave and barrier, sixteen loads per thread and
// tile in flight two tiles ahead.  Images: weights [m-tile][k32-tile][slice][k-half][128 rows] chunks of 8 bf16
// (= two consecutive k16 tiles of the one-plane layout, K padded to a multiple of 32 with zeros), activations the same
// per stage in LDS.  48 KiB of LDS, <= 128 VGPRs: two 8-wave workgroups per CU.  Rows of the activation tile beyond K
// re-read row K - 1 against the zero padding of the weight image.
constexpr int BK32_SL = 2;                       // k16 slices per tile
template <bool C16 = false, bool ZM16 = false>       // bf16-stored output (and zout) / zmul: see gemm_epilogue
__global__ void __launch_bounds__(512, 4)
pw_gemm_bf16_k32_kernel(GemmArgs g) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int SIMG = simg(BK32_SL), SA = 2, KT = SBK * BK32_SL;
  u32x4* img = reinterpret_cast<u32x4*>(lds);        // [2 subs][2 activation stages][SIMG] | [SA weight stages][SIMG]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int sub = __builtin_amdgcn_readfirstlane(wave >> 2), lw = wave & 3, ltid = tid & 255;
  const int wm = lw >> 1, wn = lw & 1;
  const int li = lane & 31, lh = lane >> 5;

  const int MT = (g.M + BM - 1) / BM, NT = (g.N + BN - 1) / BN, NT2 = (NT + 1) / 2;
  int L;
  {
    const int nwg = gridDim.x, id = blockIdx.x;
    const int q = nwg >> 3, r = nwg & 7, xcd = id & 7;
    L = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (id >> 3);
  }
  const int mt = L % MT, nt2 = (L / MT) % NT2, bz = L / (MT * NT2);
  const bool live = 2 * nt2 + sub < NT;              // wave-uniform
  const int nt = min(2 * nt2 + sub, NT - 1);
  const int m0 = mt * BM, n0 = nt * BN;
  const int T = (g.K + KT - 1) / KT;

  // the weight tile (SIMG = 512 chunks of 16 bytes) goes by LDS-DMA, one chunk per thread
  const u32x4* Ag = reinterpret_cast<const u32x4*>(g.A) + (int64_t)bz * g.a_bs + (int64_t)mt * T * SIMG + tid;
  const int bh = __builtin_amdgcn_readfirstlane(ltid >> 7);      // k-half staged by this wave
  const float* Bb;
  {
    const uint64_t a = reinterpret_cast<uint64_t>(g.B + (int64_t)bz * g.b_bs);
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)a), hi = __builtin_amdgcn_readfirstlane((uint32_t)(a >> 32));
    Bb = reinterpret_cast<const float*>(((uint64_t)hi << 32) | lo);
  }
  const int bn = min(n0 + (ltid & 127), g.N - 1);
  const uint32_t flip = split_flip_mask(ltid & 127);
  // ONE register set for the activations of the next tile (two sets of 2 x 8 next to 64 accumulators spilled 228 bytes
  // per lane at the 128 registers two workgroups per CU allow): tile t + 1 is loaded at the top of step t, converted
  // and stored behind the eight MFMAs of tile t - ~1,000 cycles at four waves per SIMD, the latency of an L2 hit
  float xb[BK32_SL][8] = {};
  auto issueA = [&](int t) __attribute__((always_inline)) {
    __builtin_amdgcn_global_load_lds((gbl_ptr_t)(Ag + (int64_t)t * SIMG), (lds_ptr_t)(img + (4 + t % SA) * SIMG + wave * 64), 16, 0, 0);
  };
  auto round_store = [&](const float (&x)[BK32_SL][8], u32x4* o) __attribute__((always_inline)) {
#pragma unroll
    for (int sl = 0; sl < BK32_SL; ++sl) {
      float xs[8];
      flip8(xs, x[sl], flip);       // sign checkerboard: odd 64-column blocks are staged negated
      o[sl * 2 * SCH] = round8(xs);
    }
  };
  const uint32_t boff = (uint32_t)bn * 4u;
  auto fetchB = [&](int t, float (&x)[BK32_SL][8]) __attribute__((always_inline)) {
#pragma unroll
    for (int sl = 0; sl < BK32_SL; ++sl) {
      const int k0 = t * KT + sl * SBK + bh * 8;
      const float* p = Bb + (int64_t)min(k0, g.K - 1) * g.ldb;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        asm volatile("global_load_dword %0, %1, %2" : "=&v"(x[sl][j]) : "v"(boff), "s"(p) : "memory");
        p += (k0 + j + 1 < g.K) ? g.ldb : 0;
      }
    }
  };
#define USE_X16(x, N) do { asm volatile("s_waitcnt vmcnt(" #N ")" :: "v"(x[0][0]), "v"(x[0][1]), "v"(x[0][2]), "v"(x[0][3]), \
                                        "v"(x[0][4]), "v"(x[0][5]), "v"(x[0][6]), "v"(x[0][7]), "v"(x[1][0]), "v"(x[1][1]),     \
                                        "v"(x[1][2]), "v"(x[1][3]), "v"(x[1][4]), "v"(x[1][5]), "v"(x[1][6]), "v"(x[1][7])      \
                                        : "memory");                                                                           \
                           __builtin_amdgcn_sched_barrier(0); } while (0)
  u32x4* const Bst = img + sub * 2 * SIMG + bh * SCH + (ltid & 127);   // this thread's chunk in its sub's stage 0

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  issueA(0);
  fetchB(0, xb);
  USE_X16(xb, 0);
  round_store(xb, Bst);
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
  for (int t = 0; t < T; ++t) {
    const int cur = t & 1;
    const u32x4* As = img + (4 + cur) * SIMG + lh * SCH + wm * 64 + li;
    const u32x4* Bs = img + (sub * 2 + cur) * SIMG + lh * SCH + wn * 64 + li;
    const bool more = t + 1 < T;                      // workgroup-uniform
    if (more) { issueA(t + 1); fetchB(t + 1, xb); }
#pragma unroll
    for (int sl = 0; sl < BK32_SL; ++sl) {          // one slice's fragments at a time: 16 registers
      const u32x4 a0 = As[sl * 2 * SCH], a1 = As[sl * 2 * SCH + 32], b0 = Bs[sl * 2 * SCH], b1 = Bs[sl * 2 * SCH + 32];
      SPLIT_MFMA(a0, b0, acc[0][0]); SPLIT_MFMA(a0, b1, acc[0][1]);
      SPLIT_MFMA(a1, b0, acc[1][0]); SPLIT_MFMA(a1, b1, acc[1][1]);
    }
    if (more) {
      USE_X16(xb, 0);                                 // (the DMA piece of this step is older than the loads: landed too)
      round_store(xb, Bst + (cur ^ 1) * SIMG);
    }
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
  }
#undef USE_X16
  if (live) {
    split_unflip(acc, wn);
    gemm_epilogue<true, C16, ZM16>(g, acc, bz, m0, n0, wm, wn, li, lh);
  }
}

// The same kernel in 256 x 256 x 64 steps on sixteen waves (round 6; the structure of pw_gemm_b16_quad_kernel below, for an
// fp32-STORED activation operand): 1024 threads = two copies (msub 0 / 1 = m-tiles 2 mt2, 2 mt2 + 1) of the 8-wave arrangement
// sharing the ROUNDED activation tiles in LDS.  Per step each thread fetches the sixteen fp32 values it fetched per k32 tile
// above - copy msub stages the k-rows [32 msub, 32 msub + 32) of the 64 - so the rounding work and the activation bytes from
// L2 per MFMA halve, and a wave runs SIXTEEN MFMAs between two barriers.  Weight tiles: two k32 image tiles per copy and
// step by LDS-DMA.  Two stages of 64 KB.  An odd number of k32 image tiles: the last step runs two of its four slices.
constexpr int Q32_BCH = 4 * 2 * SCH;                      // chunks of one sub's activation image per stage: [4 slices][2 k-halves][128 columns]
constexpr int Q32_STAGE = 2 * (2 * simg(2)) + 2 * Q32_BCH;  // [copy 0: 2 k32 weight tiles | copy 1 | sub 0 | sub 1]
constexpr size_t q32_lds_bytes() { return (size_t)2 * Q32_STAGE * 16; }
template <bool C16, bool ZM16>
__global__ void __launch_bounds__(1024, 4)
pw_gemm_bf16_quad32_kernel(GemmArgs g) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int ACH = simg(2);                      // 512 chunks: one k32 weight-image tile
  u32x4* img = reinterpret_cast<u32x4*>(lds);
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int msub = wave >> 3, w8 = wave & 7, sub = w8 >> 2, lw = w8 & 3, ltid = tid & 255;
  const int wm = lw >> 1, wn = lw & 1;
  const int li = lane & 31, lh = lane >> 5;

  const int MT = (g.M + BM - 1) / BM, MT2 = (MT + 1) / 2, NT = (g.N + BN - 1) / BN, NT2 = (NT + 1) / 2;
  int L;
  {
    const int nwg = gridDim.x, id = blockIdx.x;
    const int q = nwg >> 3, r = nwg & 7, xcd = id & 7;
    L = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (id >> 3);
  }
  const int mt2 = L % MT2, nt2 = (L / MT2) % NT2, bz = L / (MT2 * NT2);
  const bool live = 2 * nt2 + sub < NT && 2 * mt2 + msub < MT;       // wave-uniform
  const int nt = min(2 * nt2 + sub, NT - 1), mt = min(2 * mt2 + msub, MT - 1);
  const int m0 = mt * BM, n0 = nt * BN;
  const int T32 = (g.K + 31) / 32, T = (T32 + 1) / 2;

  const u32x4* Ag = reinterpret_cast<const u32x4*>(g.A) + (int64_t)bz * g.a_bs + (int64_t)mt * T32 * ACH + (tid & 511);
  const int bh = __builtin_amdgcn_readfirstlane(ltid >> 7);      // k-half staged by this wave
  const float* Bb;
  {
    const uint64_t a = reinterpret_cast<uint64_t>(g.B + (int64_t)bz * g.b_bs);
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)a), hi = __builtin_amdgcn_readfirstlane((uint32_t)(a >> 32));
    Bb = reinterpret_cast<const float*>(((uint64_t)hi << 32) | lo);
  }
  const int bn = min(n0 + (ltid & 127), g.N - 1);
  const uint32_t flip = split_flip_mask(ltid & 127);
  float xb[2][8] = {};
  auto issueA = [&](int t) __attribute__((always_inline)) {
    u32x4* st = img + (t & 1) * Q32_STAGE + 2 * msub * ACH;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int t32 = min(2 * t + h, T32 - 1);
      __builtin_amdgcn_global_load_lds((gbl_ptr_t)(Ag + (int64_t)t32 * ACH), (lds_ptr_t)(st + h * ACH + w8 * 64), 16, 0, 0);
    }
  };
  const uint32_t boff = (uint32_t)bn * 4u;
  auto fetchB = [&](int t, float (&x)[2][8]) __attribute__((always_inline)) {      // this copy's 32 k-rows of step t
#pragma unroll
    for (int sl = 0; sl < 2; ++sl) {
      const int k0 = t * 64 + msub * 32 + sl * SBK + bh * 8;
      const float* p = Bb + (int64_t)min(k0, g.K - 1) * g.ldb;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        asm volatile("global_load_dword %0, %1, %2" : "=&v"(x[sl][j]) : "v"(boff), "s"(p) : "memory");
        p += (k0 + j + 1 < g.K) ? g.ldb : 0;
      }
    }
  };
#define USE_XQ16(x) do { asm volatile("s_waitcnt vmcnt(0)" :: "v"(x[0][0]), "v"(x[0][1]), "v"(x[0][2]), "v"(x[0][3]), \
                                      "v"(x[0][4]), "v"(x[0][5]), "v"(x[0][6]), "v"(x[0][7]), "v"(x[1][0]), "v"(x[1][1]),     \
                                      "v"(x[1][2]), "v"(x[1][3]), "v"(x[1][4]), "v"(x[1][5]), "v"(x[1][6]), "v"(x[1][7])      \
                                      : "memory");                                                                           \
                         __builtin_amdgcn_sched_barrier(0); } while (0)
  // this thread's chunk in its sub's image of stage 0: slices 2 msub, 2 msub + 1
  u32x4* const Bst = img + 4 * ACH + sub * Q32_BCH + (2 * msub) * 2 * SCH + bh * SCH + (ltid & 127);
  auto round_store = [&](const float (&x)[2][8], u32x4* o) __attribute__((always_inline)) {
#pragma unroll
    for (int sl = 0; sl < 2; ++sl) {
      float xs[8];
      flip8(xs, x[sl], flip);
      o[sl * 2 * SCH] = round8(xs);
    }
  };

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  issueA(0);
  fetchB(0, xb);
  USE_XQ16(xb);
  round_store(xb, Bst);
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
  for (int t = 0; t < T; ++t) {
    const int cur = t & 1;
    const u32x4* As = img + cur * Q32_STAGE + 2 * msub * ACH + lh * SCH + wm * 64 + li;
    const u32x4* Bs = img + cur * Q32_STAGE + 4 * ACH + sub * Q32_BCH + lh * SCH + wn * 64 + li;
    const bool more = t + 1 < T;                      // workgroup-uniform
    if (more) { issueA(t + 1); fetchB(t + 1, xb); }
    const int nsl = (2 * t + 1 < T32) ? 4 : 2;       // workgroup-uniform
#pragma unroll
    for (int sl = 0; sl < 4; ++sl) {
      if (sl < nsl) {
        const u32x4 a0 = As[sl * 2 * SCH], a1 = As[sl * 2 * SCH + 32], b0 = Bs[sl * 2 * SCH], b1 = Bs[sl * 2 * SCH + 32];
        SPLIT_MFMA(a0, b0, acc[0][0]); SPLIT_MFMA(a0, b1, acc[0][1]);
        SPLIT_MFMA(a1, b0, acc[1][0]); SPLIT_MFMA(a1, b1, acc[1][1]);
      }
    }
    if (more) {
      USE_XQ16(xb);                                   // (this step's DMAs are older than the loads: landed too)
      round_store(xb, Bst + (cur ^ 1) * Q32_STAGE);
    }
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
  }
#undef USE_XQ16
  if (live) {
    split_unflip(acc, wn);
    gemm_epilogue<true, C16, ZM16>(g, acc, bz, m0, n0, wm, wn, li, lh);
  }
}

// PARADIS_GEMM_BF16 forward / dgrad with the activation operand STORED as bf16 (round 6; GemmArgs::io16 & IO_B16).
// B is [K rows][N columns] of bf16, n-contiguous (a [C, H W] plane stack as it sits in HBM).  Nothing of it passes through
// the vector ALU: a 32 x 256 tile (16 KB) goes HBM -> LDS by LDS-DMA, sixteen bytes per lane, and the MFMA's B fragment -
// eight consecutive k of one column per lane - comes out of the row-major image through the hardware transpose read
// ds_read_b64_tr_b16 (four k per read).  The weight tile is the [m-tile][k32-tile][slice][k-half][128 rows] image of
// pw_gemm_bf16_k32_kernel, by LDS-DMA as there.  Same 128 x 256 workgroup tile, accumulator layout and epilogue.
//   LDS: three stages of (8 KB weights + 16 KB activations) = 72 KB: two 8-wave workgroups per CU; tile t + 2 is in
//   flight while tile t is multiplied; one barrier per k-tile.
//   Image of the activation tile: row r (k) = 512 bytes, 16-byte chunk cc of the row stored at slot cc ^ ((r & 3) << 2):
//   the DMA writes lane-linearly (the permutation sits in the SOURCE address of a lane), and the four rows a transposed
//   read gathers per 16-lane group fall into the four bank quarters (conflict-free: rows 512 bytes apart would share one).
//   Requires N % 8 == 0, ldb % 8 == 0 and 16-byte aligned planes (host-checked).  Rows of a tile beyond K re-read row
//   K - 1 against the zero padding of the weight image; columns beyond N re-read the last eight and are never stored.
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) s16x4* lds_s16x4_ptr_t;
constexpr int B16_KT = 32, B16_ST = 3;
constexpr int B16_ACH = simg(2);                  // 512 chunks: the weight tile of one k32 step
constexpr int B16_BCH = B16_KT * 32;              // 1024 chunks: 32 k-rows x 256 columns of bf16
constexpr int B16_STAGE = B16_ACH + B16_BCH;      // chunks per stage (24 KB)
constexpr size_t b16_lds_bytes() { return (size_t)B16_ST * B16_STAGE * 16; }
template <bool C16, bool ZM16>
__global__ void __launch_bounds__(512, 4)
pw_gemm_b16_kernel(GemmArgs g) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  u32x4* img = reinterpret_cast<u32x4*>(lds);
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int sub = wave >> 2, lw = wave & 3;
  const int wm = lw >> 1, wn = lw & 1;
  const int li = lane & 31, lh = lane >> 5;

  const int MT = (g.M + BM - 1) / BM, NT = (g.N + BN - 1) / BN, NT2 = (NT + 1) / 2;
  int L;
  {
    const int nwg = gridDim.x, id = blockIdx.x;
    const int q = nwg >> 3, r = nwg & 7, xcd = id & 7;
    L = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (id >> 3);
  }
  const int mt = L % MT, nt2 = (L / MT) % NT2, bz = L / (MT * NT2);
  const bool live = 2 * nt2 + sub < NT;              // wave-uniform
  const int nt = min(2 * nt2 + sub, NT - 1);
  const int m0 = mt * BM, n0 = nt * BN;
  const int T = (g.K + B16_KT - 1) / B16_KT;

  const u32x4* Ag = reinterpret_cast<const u32x4*>(g.A) + (int64_t)bz * g.a_bs + (int64_t)mt * T * B16_ACH + tid;
  const uint16_t* Bb = reinterpret_cast<const uint16_t*>(g.B) + (int64_t)bz * g.b_bs;
  // this lane's two source chunks of a tile: LDS chunk c = (2 wave + j) 64 + lane -> row c >> 5, slot c & 31
  int brow[2], bcol[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int c = (2 * wave + j) * 64 + lane, r = c >> 5, slot = c & 31;
    brow[j] = r;
    bcol[j] = min(nt2 * 2 * BN + 8 * (slot ^ ((r & 3) << 2)), g.N - 8);
  }
  auto issue = [&](int t) __attribute__((always_inline)) {
    u32x4* st = img + (t % B16_ST) * B16_STAGE;
    __builtin_amdgcn_global_load_lds((gbl_ptr_t)(Ag + (int64_t)t * B16_ACH), (lds_ptr_t)(st + wave * 64), 16, 0, 0);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int k = min(t * B16_KT + brow[j], g.K - 1);
      __builtin_amdgcn_global_load_lds((gbl_ptr_t)(Bb + (int64_t)k * g.ldb + bcol[j]),
                                       (lds_ptr_t)(st + B16_ACH + (2 * wave + j) * 64), 16, 0, 0);
    }
  };
  // transposed reads: lane 4q + p of 16-lane group gq supplies (row 8 lh + q [+ 16 slice + 4 e], columns 4p .. 4p + 3 of the
  // group's 16): byte offset of this lane inside a stage's activation image, one per 32-column block tn of the wave
  const int gq = lane >> 4, q4 = (lane >> 2) & 3, p4 = lane & 3;
  uint32_t boff[2];
#pragma unroll
  for (int tn = 0; tn < 2; ++tn) {
    const int nbi = sub * 4 + wn * 2 + tn;                               // 32-column block inside the 256 columns
    boff[tn] = (uint32_t)((8 * lh + q4) * 512 + (4 * (nbi ^ q4) + 2 * (gq & 1) + (p4 >> 1)) * 16 + 8 * (p4 & 1));
  }

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  issue(0);
  if (T > 1) issue(1);
  for (int t = 0; t < T; ++t) {
    // tile t has landed (three DMAs per tile and lane; the next tile's may stay in flight) and every wave is past tile t - 1
    if (t + 1 < T) asm volatile("s_waitcnt vmcnt(3)\n\ts_barrier" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
    if (t + 2 < T) issue(t + 2);
    const u32x4* st = img + (t % B16_ST) * B16_STAGE;
    const u32x4* As = st + lh * SCH + wm * 64 + li;
    const char* Bs = reinterpret_cast<const char*>(st + B16_ACH);
#pragma unroll
    for (int sl = 0; sl < 2; ++sl) {
      const u32x4 a0 = As[sl * 2 * SCH], a1 = As[sl * 2 * SCH + 32];
      u32x4 b[2];
#pragma unroll
      for (int tn = 0; tn < 2; ++tn) {
        const char* pb = Bs + boff[tn] + sl * 16 * 512;
        const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr_t)(pb));
        const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr_t)(pb + 4 * 512));
        const uint64_t l64 = __builtin_bit_cast(uint64_t, lo), h64 = __builtin_bit_cast(uint64_t, hi);
        b[tn] = (u32x4){(uint32_t)l64, (uint32_t)(l64 >> 32), (uint32_t)h64, (uint32_t)(h64 >> 32)};
      }
      SPLIT_MFMA(a0, b[0], acc[0][0]); SPLIT_MFMA(a0, b[1], acc[0][1]);
      SPLIT_MFMA(a1, b[0], acc[1][0]); SPLIT_MFMA(a1, b[1], acc[1][1]);
    }
  }
  if (live) {
    // the weight image holds the rows of odd 32-row blocks negated (sign checkerboard of the register-staged kernels; the
    // activations come straight from memory here, un-negated): block tm = 1 of every wave accumulated -C
    if (SPLIT_SIGNED) {
#pragma unroll
      for (int tn = 0; tn < 2; ++tn)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[1][tn][r] = -acc[1][tn][r];
    }
    gemm_epilogue<true, C16, ZM16>(g, acc, bz, m0, n0, wm, wn, li, lh);
  }
}

// 256 x 256 x 64 steps with sixteen waves (round 6): 1024 threads = two copies (msub 0 / 1 = m-tiles 2 mt2, 2 mt2 + 1) of the
// 8-wave arrangement above sharing the activation tile in LDS, and k-steps of 64: SIXTEEN MFMAs per wave between two
// barriers instead of eight - the 128 x 256 x 32 kernel waits on its per-step chain (DMA landing, barrier, fragment reads;
// matrix pipe 19 % busy at 2.4 GHz), not on bytes.  Every wave keeps its 64 x 64 accumulators and its epilogue; sixteen waves
// per CU as with two 512-thread workgroups.  Two stages of 64 KB (32 KB of weight tiles - two k32 image tiles per copy - and
// 32 KB of activations); a thread issues four LDS-DMAs per step.  An odd number of k32 image tiles: the last step runs
// two of its four k16 slices.
constexpr int B16Q_KT = 64;
constexpr int B16Q_STAGE = 2 * (2 * B16_ACH) + 2 * B16_BCH;          // chunks per stage: [copy 0: 2 k32 weight tiles | copy 1 | 64 rows of activations]
constexpr size_t b16q_lds_bytes() { return (size_t)2 * B16Q_STAGE * 16; }
template <bool C16, bool ZM16>
__global__ void __launch_bounds__(1024, 4)
pw_gemm_b16_quad_kernel(GemmArgs g) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  u32x4* img = reinterpret_cast<u32x4*>(lds);
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int msub = wave >> 3, w8 = wave & 7, sub = w8 >> 2, lw = w8 & 3;
  const int wm = lw >> 1, wn = lw & 1;
  const int li = lane & 31, lh = lane >> 5;

  const int MT = (g.M + BM - 1) / BM, MT2 = (MT + 1) / 2, NT = (g.N + BN - 1) / BN, NT2 = (NT + 1) / 2;
  int L;
  {
    const int nwg = gridDim.x, id = blockIdx.x;
    const int q = nwg >> 3, r = nwg & 7, xcd = id & 7;
    L = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (id >> 3);
  }
  const int mt2 = L % MT2, nt2 = (L / MT2) % NT2, bz = L / (MT2 * NT2);
  const bool live = 2 * nt2 + sub < NT && 2 * mt2 + msub < MT;       // wave-uniform
  const int nt = min(2 * nt2 + sub, NT - 1), mt = min(2 * mt2 + msub, MT - 1);
  const int m0 = mt * BM, n0 = nt * BN;
  const int T32 = (g.K + B16_KT - 1) / B16_KT, T = (T32 + 1) / 2;     // k32 image tiles, k64 steps

  const u32x4* Ag = reinterpret_cast<const u32x4*>(g.A) + (int64_t)bz * g.a_bs + (int64_t)mt * T32 * B16_ACH + (tid & 511);
  const uint16_t* Bb = reinterpret_cast<const uint16_t*>(g.B) + (int64_t)bz * g.b_bs;
  // this lane's two source chunks of the activation tile: LDS chunk c = (2 wave + j) 64 + lane -> row c >> 5 (0..63), slot c & 31
  int brow[2], bcol[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int c = (2 * wave + j) * 64 + lane, r = c >> 5, slot = c & 31;
    brow[j] = r;
    bcol[j] = min(nt2 * 2 * BN + 8 * (slot ^ ((r & 3) << 2)), g.N - 8);
  }
  auto issue = [&](int t) __attribute__((always_inline)) {
    u32x4* st = img + (t & 1) * B16Q_STAGE;
#pragma unroll
    for (int h = 0; h < 2; ++h) {        // the two k32 image tiles of the step (an odd T32: the last one twice, second use skipped)
      const int t32 = min(2 * t + h, T32 - 1);
      __builtin_amdgcn_global_load_lds((gbl_ptr_t)(Ag + (int64_t)t32 * B16_ACH),
                                       (lds_ptr_t)(st + (2 * msub + h) * B16_ACH + w8 * 64), 16, 0, 0);
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int k = min(t * B16Q_KT + brow[j], g.K - 1);
      __builtin_amdgcn_global_load_lds((gbl_ptr_t)(Bb + (int64_t)k * g.ldb + bcol[j]),
                                       (lds_ptr_t)(st + 4 * B16_ACH + (2 * wave + j) * 64), 16, 0, 0);
    }
  };
  const int gq = lane >> 4, q4 = (lane >> 2) & 3, p4 = lane & 3;
  uint32_t boff[2];
#pragma unroll
  for (int tn = 0; tn < 2; ++tn) {
    const int nbi = sub * 4 + wn * 2 + tn;
    boff[tn] = (uint32_t)((8 * lh + q4) * 512 + (4 * (nbi ^ q4) + 2 * (gq & 1) + (p4 >> 1)) * 16 + 8 * (p4 & 1));
  }

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  issue(0);
  for (int t = 0; t < T; ++t) {
    // step t has landed (the only DMAs in flight) and every wave is past step t - 1: refill that stage at once
    asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
    if (t + 1 < T) issue(t + 1);
    const u32x4* st = img + (t & 1) * B16Q_STAGE;
    const u32x4* As = st + 2 * msub * B16_ACH + lh * SCH + wm * 64 + li;
    const char* Bs = reinterpret_cast<const char*>(st + 4 * B16_ACH);
    const int nsl = (2 * t + 1 < T32) ? 4 : 2;       // workgroup-uniform
#pragma unroll
    for (int sl = 0; sl < 4; ++sl) {
      if (sl < nsl) {
        const u32x4 a0 = As[sl * 2 * SCH], a1 = As[sl * 2 * SCH + 32];     // (slice sl of the two k32 image tiles: 2 SCH chunks apart)
        u32x4 b[2];
#pragma unroll
        for (int tn = 0; tn < 2; ++tn) {
          const char* pb = Bs + boff[tn] + sl * 16 * 512;
          const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr_t)(pb));
          const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr_t)(pb + 4 * 512));
          const uint64_t l64 = __builtin_bit_cast(uint64_t, lo), h64 = __builtin_bit_cast(uint64_t, hi);
          b[tn] = (u32x4){(uint32_t)l64, (uint32_t)(l64 >> 32), (uint32_t)h64, (uint32_t)(h64 >> 32)};
        }
        SPLIT_MFMA(a0, b[0], acc[0][0]); SPLIT_MFMA(a0, b[1], acc[0][1]);
        SPLIT_MFMA(a1, b[0], acc[1][0]); SPLIT_MFMA(a1, b[1], acc[1][1]);
      }
    }
  }
  if (live) {
    if (SPLIT_SIGNED) {
#pragma unroll
      for (int tn = 0; tn < 2; ++tn)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[1][tn][r] = -acc[1][tn][r];
    }
    gemm_epilogue<true, C16, ZM16>(g, acc, bz, m0, n0, wm, wn, li, lh);
  }
}

// (A 256 x 256 workgroup tile for this kernel - 2 x 4 waves of 128 x 64, 200-219 registers, one workgroup per CU, four
//  32 KB stages - halves the activation bytes pulled from L2 and was built and measured in round 6: 309 against 218 us at
//  896 x 896, the bf16-mixed step 83.8 against 77.6 ms.  At two waves per SIMD the store-bound epilogue doubles - a K = 32
//  launch 161 against 78 us - and takes back more than the k-loop gains; the weight gradient, whose epilogue writes one
//  fp32 tile per slab, does gain from that tile: pw_gemm_wgrad_square_kernel.  Removed; profiles/r06_amp_gemm_tiles.txt.
//  The same 256 x 256 tile with SIXTEEN waves - 1024 threads, two copies of the arrangement above sharing the activation tile
//  in LDS, every wave keeping its 64 x 64 accumulators and epilogue, 0.47 instead of 0.94 GB of activations per launch - was
//  parity-green and changed nothing: 183 / 210 against 180 / 222 us at 896^2 / 1024^2, the step 78.7 against 77.8 ms.  With
//  8 MFMAs per wave between two barriers the kernel waits on its per-tile chain (DMA landing, barrier, fragment reads), not on
//  L2 bytes - which is why the weight gradient, whose taller tiles also DOUBLE the MFMAs per barrier, gained and this did not.
//  With k-steps of 64 on top - sixteen MFMAs per barrier - it does pay: pw_gemm_b16_quad_kernel above.)

// the kernel families above by their two I/O-type flags (C16, ZM16)
constexpr GemmKernel BF16_K32[4] = IO2_KERNELS(pw_gemm_bf16_k32_kernel), BF16_QUAD32[4] = IO2_KERNELS(pw_gemm_bf16_quad32_kernel);
constexpr GemmKernel B16[4] = IO2_KERNELS(pw_gemm_b16_kernel), B16_QUAD[4] = IO2_KERNELS(pw_gemm_b16_quad_kernel);

}  // namespace

// ---- launcher of the bf16-mixed forward / data-gradient kernels (called from gemm.hip) ---------------------------------
int pd_amp_launch_fwd(const GemmArgs& d, hipStream_t st) {
  const int NT = (d.N + BN - 1) / BN;
  // (round 5: the k16 kernels with one plane ran the bf16-mixed step at 91.6 ms; a 256 x 128 tile - two M-tiles
  //  sharing one fp32 activation tile, 16 instead of 20 KB through L2 per tile pair - at 95.9 ms: with four MFMAs per
  //  wave and barrier the kernel is bound by its per-tile latency chain, not by bytes.  Hence 32-deep tiles.)
  const size_t lds = (size_t)(2 * 2 + 2) * simg(BK32_SL) * 16;
  const int MT = (d.M + BM - 1) / BM;
  const dim3 grid(MT * ((NT + 1) / 2) * d.nbatch), bl(512);
  const dim3 gq(((MT + 1) / 2) * ((NT + 1) / 2) * d.nbatch), bq(1024);     // the quad kernels' 256 x 256 tiles
  const bool quad_shape = MT >= 2 && ((MT + 1) / 2) * 2 * 7 <= MT * 8;     // (an odd MT repeats its last m-tile: at most 1/8)
  const bool c16 = (d.io16 & IO_C16) != 0, zm16 = (d.io16 & IO_ZM16) != 0 && d.zmul != nullptr;
  if (d.io16 & IO_B16) {     // activations stored as bf16: LDS-DMA + transposed reads (layout checked by the caller)
    static PerDeviceOnce once;      // (reserved before the quad kernel is considered, as ever)
    if (int e = reserve_lds(once, IO2_KERNELS(pw_gemm_b16_kernel), b16_lds_bytes(), "pw_gemm(b16)")) return e;
    static const bool quad_on = [] { const char* e = getenv("PARADIS_GEMM_B16_QUAD"); return !(e && e[0] == '0'); }();   // (=0: A/B)
    if (quad_on && quad_shape) return launch_io2<B16_QUAD>(c16, zm16, gq, bq, b16q_lds_bytes(), "pw_gemm(b16 quad)", st, d);
    return launch_io2<B16>(c16, zm16, grid, bl, b16_lds_bytes(), nullptr, st, d);
  }
  static const bool q32_on = [] { const char* e = getenv("PARADIS_GEMM_K32_QUAD"); return !(e && e[0] == '0'); }();   // (=0: A/B)
  if (q32_on && quad_shape) return launch_io2<BF16_QUAD32>(c16, zm16, gq, bq, q32_lds_bytes(), "pw_gemm(k32 quad)", st, d);
  return launch_io2<BF16_K32>(c16, zm16, grid, bl, lds, nullptr, st, d);
}
