// The split-operand family: the same fp32 GEMMs on the bf16 / f16 matrix pipe (gemm_common.h, "Split-bf16 kernels").  The
// operands' amax, the weight images (amax_partials_kernel, split_weights*_kernel and their entry points), the forward /
// data-gradient kernels on a 128 x 128 and a 128 x 256 tile, and the launch of the shared weight-gradient kernel with
// three and two planes.  gemm.hip calls in through pd_split_* (declared in gemm_common.h).
#include <cstring>
#include <type_traits>
#include "gemm_common.h"

namespace {

constexpr int SIMG = simg(3);            // chunks of a bf16x3 image tile (the split kernels shadow it with simg(NP))

// max |x| over B blocks of `inner` contiguous floats (block stride bs) -> PARADIS_AMAX_PARTIALS words, one
// per workgroup (bits of a non-negative float order like unsigned integers; a NaN is larger than Inf and
// so survives).  The consumers take the maximum of the words: no atomics, no zero-fill, deterministic.
__global__ void __launch_bounds__(256)
amax_partials_kernel(const float* __restrict__ x, int B, int64_t inner, int64_t bs, int vec, uint32_t* __restrict__ out) {
  uint32_t m = 0;
  if (vec) {
    const int64_t n4 = inner >> 2, total = n4 * B;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
      const int64_t b = i / n4, j = i - b * n4;
      const uint4 q = *reinterpret_cast<const uint4*>(x + b * bs + 4 * j);
      m = max(max(m, q.x & 0x7fffffffu), max(q.y & 0x7fffffffu, max(q.z & 0x7fffffffu, q.w & 0x7fffffffu)));
    }
  } else {
    const int64_t total = inner * B;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
      const int64_t b = i / inner, j = i - b * inner;
      m = max(m, __float_as_uint(x[b * bs + j]) & 0x7fffffffu);
    }
  }
  m = wave_umax_lane63(m);
  __shared__ uint32_t red[4];
  if ((threadIdx.x & 63) == 63) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) out[blockIdx.x] = max(max(red[0], red[1]), max(red[2], red[3]));
}


// Image of A[m,k] = W[m*rs + k*cs] (rs/cs select W or W^T), zero padded to [MT*128, KT*16]:
// out[((mt*KT + kt)*3 + s)*256 + half*128 + row] ; one thread per (mt, kt, half, row).
template <int NP = 3>
__device__ __forceinline__ void split_weights_body(const float* __restrict__ Wb, int64_t rs, int64_t cs, int M, int K,
                                                   int KT, int64_t units, u32x4* __restrict__ ob) {
  for (int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x; u < units; u += (int64_t)gridDim.x * 256) {
    const int row = (int)(u & 127), half = (int)((u >> 7) & 1);
    const int64_t tile = u >> 8;
    const int kt = (int)(tile % KT), mt = (int)(tile / KT);
    const int m = mt * BM + row;
    float x[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int k = kt * SBK + half * 8 + j;
      x[j] = (m < M && k < K) ? Wb[(int64_t)m * rs + (int64_t)k * cs] : 0.f;
      if (SPLIT_SIGNED && (row & 32)) x[j] = -x[j];      // sign checkerboard: odd 32-row blocks hold -W
    }
    if constexpr (NP == 3) {
      u32x4 h, mm, l;
      split8(x, h, mm, l);
      u32x4* o = ob + tile * SIMG + half * SCH + row;
      o[0] = h; o[2 * SCH] = mm; o[4 * SCH] = l;
    } else {
      ob[tile * simg(1) + half * SCH + row] = round8(x);
    }
  }
}

template <int NP>
__global__ void __launch_bounds__(256)
split_weights_kernel(const float* __restrict__ W, int64_t rs, int64_t cs, int M, int K, int KT, int64_t units,
                     int64_t w_bs, int64_t out_bs, u32x4* __restrict__ out) {
  split_weights_body<NP>(W + (int64_t)blockIdx.y * w_bs, rs, cs, M, K, KT, units, out + (int64_t)blockIdx.y * out_bs);
}

// both images of one row-major W[M,K] in ONE launch (a training step needs W for the forward GEMM and W^T for the
// data gradient: 78 launches of a few microseconds per step instead of 155): blockIdx.y = 0 -> W, 1 -> W^T
template <int NP>
__global__ void __launch_bounds__(256)
split_weights_pair_kernel(const float* __restrict__ W, int M, int K, int KT, int KTt, int64_t units, int64_t units_t,
                          u32x4* __restrict__ out, u32x4* __restrict__ out_t) {
  if (blockIdx.y == 0) split_weights_body<NP>(W, K, 1, M, K, KT, units, out);
  else split_weights_body<NP>(W, 1, K, K, M, KTt, units_t, out_t);
}

// f16x2 image: out[((mt*KT + kt)*2 + s)*256 + half*128 + row]; `tail` = the words behind the image:
// [0] = bits of max |W| (written here, read by the GEMMs), [4 ..) = the amax partials of W (input)
__global__ void __launch_bounds__(256)
split_weights_f16_kernel(const float* __restrict__ W, int64_t rs, int64_t cs, int M, int K, int KT, int64_t units,
                         u32x4* __restrict__ out, uint32_t* __restrict__ tail) {
  const uint32_t amax = reduce_amax_partials(tail + 4);
  if (blockIdx.x == 0 && threadIdx.x == 0) tail[0] = amax;
  float sc, inv;
  scale_from_amax(amax, sc, inv);
  for (int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x; u < units; u += (int64_t)gridDim.x * 256) {
    const int row = (int)(u & 127), half = (int)((u >> 7) & 1);
    const int64_t tile = u >> 8;
    const int kt = (int)(tile % KT), mt = (int)(tile / KT);
    const int m = mt * BM + row;
    float x[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int k = kt * SBK + half * 8 + j;
      x[j] = (m < M && k < K) ? W[(int64_t)m * rs + (int64_t)k * cs] : 0.f;
    }
    u32x4 h, l;
    split8_f16(x, (SPLIT_SIGNED && (row & 32)) ? -sc : sc, h, l);      // sign checkerboard
    u32x4* o = out + tile * simg(2) + half * SCH + row;
    o[0] = h; o[2 * SCH] = l;
  }
}

// fwd / dgrad:  C_b = epi( A . B_b ),  A = split weight image (g.A, batch stride g.a_bs chunks),
// B_b[K,N] fp32 with n contiguous.
//
// Pipeline per k-tile t (one barrier per tile, two LDS stages):
//   fragment reads of t  ->  weight DMA of t+1, activation loads of t+2 (registers, two sets used
//   alternately: the loop is unrolled by two so that each set is a fixed register range)  ->
//   the 24 MFMAs of t with the bf16 split of t+1's activations interleaved between them
//   (sched_group_barrier: the VALU work issues in the shadow of the MFMAs of the same wave)  ->
//   ds_write of t+1  ->  s_waitcnt vmcnt(8): the DMA has landed, the loads of t+2 stay in flight.
//
// weight-image ring depth per scheme (stages; the DMA runs stages - 1 tiles ahead).  bf16x3: 2 (48 KiB,
// 3 WGs/CU; 4 stages = 72 KiB, 2 WGs/CU measured -2 %).  f16x2: its 8 KiB stages make a deeper ring free.
#ifndef SPLIT_ASTAGES_F16
#define SPLIT_ASTAGES_F16 2
#endif
constexpr int split_astages(int np) { return np == 2 ? SPLIT_ASTAGES_F16 : 2; }
template <int NP>
__global__ void __launch_bounds__(256, 3)
pw_gemm_split_kernel(GemmArgs g) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int SIMG = simg(NP);                     // (shadows the bf16 constant)
  u32x4* img = reinterpret_cast<u32x4*>(lds);        // [2 activation stages][SIMG] | [SA weight stages][SIMG]
  constexpr int SA = split_astages(NP), DA = SA - 1;     // weight ring depth, DMA distance in tiles
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int li = lane & 31, lh = lane >> 5;

  const int MT = (g.M + BM - 1) / BM, NT = (g.N + BN - 1) / BN;
  int L;
  {
    const int nwg = gridDim.x, id = blockIdx.x;
    const int q = nwg >> 3, r = nwg & 7, xcd = id & 7;
    L = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (id >> 3);
  }
  const int mt = L % MT, nt = (L / MT) % NT, bz = L / (MT * NT);
  const int m0 = mt * BM, n0 = nt * BN;
  const int T = (g.K + SBK - 1) / SBK;

  const u32x4* Ag = reinterpret_cast<const u32x4*>(g.A) + (int64_t)bz * g.a_bs + (int64_t)mt * T * SIMG + tid;
  // k-half staged by this thread's wave (waves 0,1 -> 0; 2,3 -> 1): row addresses stay scalar
  const int bh = __builtin_amdgcn_readfirstlane(tid >> 7);
  // (uniform, but derived from integer divisions done on the vector unit: pin it to scalar registers)
  const float* Bb;
  {
    const uint64_t a = reinterpret_cast<uint64_t>(g.B + (int64_t)bz * g.b_bs);
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)a), hi = __builtin_amdgcn_readfirstlane((uint32_t)(a >> 32));
    Bb = reinterpret_cast<const float*>(((uint64_t)hi << 32) | lo);
  }
  const int bn = min(n0 + (tid & 127), g.N - 1);

  float sc_b = 1.f, inv_a = 1.f, inv_b = 1.f;       // f16x2: activation scale, inverse scales of both operands
  if constexpr (NP == 2) {
    float sc_a;
    scale_from_amax(reduce_amax_partials(g.b_amax), sc_b, inv_b);
    scale_from_amax(g.a_amax[0], sc_a, inv_a);
  }

  const uint32_t flip = split_flip_mask(tid & 127);
  if constexpr (NP == 2) sc_b = __uint_as_float(__float_as_uint(sc_b) ^ flip);
  float xb[2][8] = {};     // defined values: the surplus split of the last tile reads a set that was never loaded
  auto issueA = [&](int t) __attribute__((always_inline)) {
    const u32x4* a = Ag + (int64_t)t * SIMG;
    u32x4* la = img + (2 + t % SA) * SIMG + wave * 64;
#pragma unroll
    for (int i = 0; i < NP; ++i)
      __builtin_amdgcn_global_load_lds((gbl_ptr_t)(a + i * 256), (lds_ptr_t)(la + i * 256), 16, 0, 0);
  };
  auto split_store = [&](const float (&x)[8], u32x4* o) __attribute__((always_inline)) {
    if constexpr (NP == 3) {
      u32x4 h, m, l;
      float xs[8];
      flip8(xs, x, flip);          // sign checkerboard: odd 64-column blocks are staged negated
      split8(xs, h, m, l);
      o[0] = h; o[2 * SCH] = m; o[4 * SCH] = l;
    } else {
      u32x4 h, l;
      split8_f16(x, sc_b, h, l);   // (the column's sign rides on the scale)
      o[0] = h; o[2 * SCH] = l;
    }
  };
  // Activation loads are issued from inline asm (saddr form: scalar row base + 32-bit lane offset, no
  // vector address arithmetic) so that the compiler does not account for them: on this loop its own
  // bookkeeping degrades to s_waitcnt vmcnt(0) in front of the first use, which would also wait for the
  // loads of the tile after and for the weight DMA just issued.  The waits are counted by hand (use_x).
  // Rows beyond K re-read row K-1: they meet the zero padding of the weight image, and finite x 0 = 0
  // (a non-finite row K-1 poisons every output anyway), so no zero-fill is needed.
  const uint32_t boff = (uint32_t)bn * 4u;
  auto fetchB = [&](int t, float (&x)[8]) __attribute__((always_inline)) {
    const int k0 = t * SBK + bh * 8;
    const float* p = Bb + (int64_t)min(k0, g.K - 1) * g.ldb;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      asm volatile("global_load_dword %0, %1, %2" : "=&v"(x[j]) : "v"(boff), "s"(p) : "memory");
      p += (k0 + j + 1 < g.K) ? g.ldb : 0;
    }
  };
  // Wait until at most N vector-memory operations issued after x's loads are outstanding.  x is an INPUT
  // of the asm (an in/out operand lets the compiler copy the not-yet-landed registers in front of the
  // wait), and a sched_barrier behind it keeps every read of x below.
#define USE_X(x, N) do { asm volatile("s_waitcnt vmcnt(" #N ")" :: "v"(x[0]), "v"(x[1]), "v"(x[2]), "v"(x[3]), \
                                      "v"(x[4]), "v"(x[5]), "v"(x[6]), "v"(x[7]) : "memory");                  \
                         __builtin_amdgcn_sched_barrier(0); } while (0)
  u32x4* const Bst = img + bh * SCH + (tid & 127);   // this thread's chunk in the activation image of stage 0

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  // prologue (once per 64-tile range: waited for in full)
  for (int u = 0; u < DA && u < T; ++u) issueA(u);
  fetchB(0, xb[0]);
  USE_X(xb[0], 0);
  if (T > 1) fetchB(1, xb[1]);
  split_store(xb[0], Bst);
  // raw barriers with counted waits: __syncthreads() is s_waitcnt vmcnt(0) lgkmcnt(0) + s_barrier and
  // would make every barrier wait for the activation loads that are meant to stay in flight
  if (T > 1) asm volatile("s_waitcnt vmcnt(8) lgkmcnt(0)\n\ts_barrier" ::: "memory");
  else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
  auto step = [&](int t, int cur, float (&xload)[8], float (&xsplit)[8]) __attribute__((always_inline)) {
    const u32x4* As = img + (2 + t % SA) * SIMG + lh * SCH + wm * 64 + li;
    const u32x4* Bs = img + cur * SIMG + lh * SCH + wn * 64 + li;
    const bool dmaA = t + DA < T, ldB = t + 2 < T;
    if (dmaA) issueA(t + DA);
    if (ldB) fetchB(t + 2, xload);
    // xsplit (tile t+1) was loaded a step ago; younger operations: this step's NP DMA and 8 loads
    if (dmaA && ldB) { if constexpr (NP == 3) USE_X(xsplit, 11); else USE_X(xsplit, 10); }
    else if (ldB) USE_X(xsplit, 8);
    else USE_X(xsplit, 0);
    // The fragment reads sit in the block of the MFMAs (behind the branches above the compiler's lgkmcnt
    // bookkeeping falls back to lgkmcnt(0) in front of the first MFMA; inside one block the waits are
    // counted and the first MFMA starts after two of the twelve reads).
    SplitFrags<NP> f;
    split_tile_read<NP, 2 * SCH, 2 * SCH>(As, Bs, f);
    // One basic block for every tile, the last included (its split writes a stage that nobody reads any
    // more): a second copy of the MFMA block behind a branch costs 32 accumulator moves per tile.
    split_tile_mfma<NP>(f, acc);
    split_store(xsplit, Bst + (cur ^ 1) * SIMG);
    // without this pinning, the training step 0.9 % slower (tools/ab_step.sh, same box, 3 of 3 rounds).
    __builtin_amdgcn_sched_group_barrier(0x100, 4 * NP, 0);   // all fragment reads first, in first-use order
#pragma unroll
    for (int i = 0; i < (NP == 3 ? 24 : 12); ++i) {
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
      __builtin_amdgcn_sched_group_barrier(0x002, NP == 3 ? 3 : 2, 0);
    }
    // weight tile t+1 landed (its DMA is DA steps old: 8 loads of that step + 8 + NP operations per step since
    // are younger), own ds_writes done, the loads of t+2 and the younger DMAs still in flight
    if (dmaA && ldB) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" :: "n"(8 + (8 + NP) * (DA - 1)) : "memory");
    else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
  };
  for (int t = 0; t < T; t += 2) {
    step(t, 0, xb[0], xb[1]);
    if (t + 1 < T) step(t + 1, 1, xb[1], xb[0]);
  }
  split_unflip(acc, wn);
  if constexpr (NP == 2) split_unscale(acc, inv_a, inv_b);
  gemm_epilogue(g, acc, bz, m0, n0, wm, wn, li, lh);
}

// f16x2 forward / dgrad with a 128 x 256 workgroup tile: 8 waves = two 128-column halves (sub 0 / 1 = n-tiles
// 2 nt2, 2 nt2 + 1, each staging its own activation tile exactly like pw_gemm_split_kernel<2>) that share ONE
// weight tile and its DMA ring.  The k-loop of this GEMM is bound by the bytes it pulls out of L2 (DESIGN.md
// 4.1c): 24 KiB per two 128 x 128 x 16 tiles here instead of 32.  48 KiB of LDS, <= 128 VGPRs: two workgroups =
// 16 waves per CU.  An odd last n-tile leaves sub 1 without work: it runs along on the clamped last tile and
// skips the epilogue.
#ifndef SPLIT_STAGGER         // (-DSPLIT_STAGGER=1: A/B build of the staggered 128 x 256 kernel)
#define SPLIT_STAGGER 0
#endif
// EPI: 0 = gemm_epilogue for every tile; an option set (EP_ON | ...) = split_epilogue_interior<EPI> for the interior tiles of
// a launch whose options ARE that set (the host's choice: split_epilogue_flags), gemm_epilogue for its ragged tiles.
template <int NSUB, int NP = 2, int EPI = 0>
__global__ void __launch_bounds__(256 * NSUB, 4)      // (second argument: waves per SIMD)
pw_gemm_split_wide_kernel(GemmArgs g) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int SIMG = simg(NP), SA = 2, DA = SA - 1;
  u32x4* img = reinterpret_cast<u32x4*>(lds);        // [NSUB][2 activation stages][SIMG] | [SA weight stages][SIMG]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int sub = __builtin_amdgcn_readfirstlane(wave >> 2), lw = wave & 3, ltid = tid & 255;
  const int wm = lw >> 1, wn = lw & 1;
  const int li = lane & 31, lh = lane >> 5;

  const int MT = (g.M + BM - 1) / BM, NT = (g.N + BN - 1) / BN, NT2 = (NT + NSUB - 1) / NSUB;
  int L;
  {
    const int nwg = gridDim.x, id = blockIdx.x;
    const int q = nwg >> 3, r = nwg & 7, xcd = id & 7;
    L = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (id >> 3);
  }
  int mt = L % MT, nt2 = (L / MT) % NT2, bz = L / (MT * NT2);
  if constexpr (NP == 3 && SPLIT_SIGN_LOOPS_FWD && SPLIT_SIGNED) {
    // (uniform, but divided on the vector unit: with two loop copies the epilogue's copies of these no longer fit into
    //  the 128 vector registers beside the loops - they belong in scalar registers)
    mt = __builtin_amdgcn_readfirstlane(mt); nt2 = __builtin_amdgcn_readfirstlane(nt2); bz = __builtin_amdgcn_readfirstlane(bz);
  }
  const bool live = NSUB * nt2 + sub < NT;           // wave-uniform
  const int nt = min(NSUB * nt2 + sub, NT - 1);
  const int m0 = mt * BM, n0 = nt * BN;
  const int T = (g.K + SBK - 1) / SBK;

  // the weight tile (SIMG = 256 NP chunks of 16 bytes) goes by LDS-DMA, one chunk per thread and piece: f16x2 one
  // piece of 512 chunks (the first 512 threads), bf16x3 a piece of 512 and a piece of 256 (waves 0-3)
  const bool doA = NSUB == 2 || wave < 8;            // wave-uniform
  const bool doA2 = NP == 3 && wave < 4;             // wave-uniform: second piece
  const u32x4* Ag = reinterpret_cast<const u32x4*>(g.A) + (int64_t)bz * g.a_bs + (int64_t)mt * T * SIMG + (tid & 511);
  const int bh = __builtin_amdgcn_readfirstlane(ltid >> 7);      // k-half staged by this wave
  const float* Bb;
  {
    const uint64_t a = reinterpret_cast<uint64_t>(g.B + (int64_t)bz * g.b_bs);
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)a), hi = __builtin_amdgcn_readfirstlane((uint32_t)(a >> 32));
    Bb = reinterpret_cast<const float*>(((uint64_t)hi << 32) | lo);
  }
  const int bn = min(n0 + (ltid & 127), g.N - 1);

  float sc_b = 1.f, inv_a = 1.f, inv_b = 1.f;
  if constexpr (NP == 2) {
    float sc_a;
    __shared__ uint32_t red[4 * NSUB];
    const uint32_t* pp = g.b_amax;
    uint32_t m = NSUB == 2 ? max(pp[tid], pp[tid + 512]) : pp[tid];
    m = wave_umax_lane63(m);
    if (lane == 63) red[wave] = m;
    __syncthreads();
    m = red[0];
#pragma unroll
    for (int i = 1; i < 4 * NSUB; ++i) m = max(m, red[i]);
    scale_from_amax(m, sc_b, inv_b);
    scale_from_amax(g.a_amax[0], sc_a, inv_a);
  }

  const uint32_t flip = split_flip_mask(ltid & 127);
  if constexpr (NP == 2) sc_b = __uint_as_float(__float_as_uint(sc_b) ^ flip);
  auto issueA = [&](int t) __attribute__((always_inline)) {
    if (doA)
      __builtin_amdgcn_global_load_lds((gbl_ptr_t)(Ag + (int64_t)t * SIMG), (lds_ptr_t)(img + (2 * NSUB + t % SA) * SIMG + wave * 64), 16, 0, 0);
    if (doA2)
      __builtin_amdgcn_global_load_lds((gbl_ptr_t)(Ag + (int64_t)t * SIMG + 512), (lds_ptr_t)(img + (2 * NSUB + t % SA) * SIMG + 512 + wave * 64), 16, 0, 0);
  };
  // SG: the sign mode of the loop copy that calls - 0 / 1 = plain / negated at compile time, 2 = the run-time mask
  auto split_store = [&](auto SG, const float (&x)[8], u32x4* o) __attribute__((always_inline)) {
    constexpr int sg = decltype(SG)::value;
    if constexpr (NP == 3) {
      u32x4 h, m, l;
      // sign checkerboard: odd 64-column blocks are staged negated.  (Two code paths behind a wave-uniform branch INSIDE
      // the step, with the sign folded into source modifiers - no v_xor - measured SLOWER, 154.8 against 153.0 ms per
      // step: the branch takes the split out of the MFMA block's schedule.  Two copies of the WHOLE loop keep one block per
      // step and measured 1.3 ms faster per step than the v_xor loop: profiles/r08_gemm_sign_loops.txt.)
      if constexpr (sg == 2) {
        float xs[8];
        flip8(xs, x, flip);
        split8(xs, h, m, l);
      } else {
        split8s<sg == 1>(x, h, m, l);
      }
      o[0] = h; o[2 * SCH] = m; o[4 * SCH] = l;
    } else {
      u32x4 h, l;
      split8_f16(x, sc_b, h, l);   // (the column's sign rides on the scale)
      o[0] = h; o[2 * SCH] = l;
    }
  };
  // inline-asm loads with hand-counted waits: see pw_gemm_split_kernel
  const uint32_t boff = (uint32_t)bn * 4u;
  auto fetchB = [&](int t, float (&x)[8]) __attribute__((always_inline)) {
    const int k0 = t * SBK + bh * 8;
    const float* p = Bb + (int64_t)min(k0, g.K - 1) * g.ldb;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      asm volatile("global_load_dword %0, %1, %2" : "=&v"(x[j]) : "v"(boff), "s"(p) : "memory");
      p += (k0 + j + 1 < g.K) ? g.ldb : 0;
    }
  };
#define USE_X(x, N) do { asm volatile("s_waitcnt vmcnt(" #N ")" :: "v"(x[0]), "v"(x[1]), "v"(x[2]), "v"(x[3]), \
                                      "v"(x[4]), "v"(x[5]), "v"(x[6]), "v"(x[7]) : "memory");                  \
                         __builtin_amdgcn_sched_barrier(0); } while (0)
  u32x4* const Bst = img + sub * 2 * SIMG + bh * SCH + (ltid & 127);   // this thread's chunk in its sub's stage 0

  f32x16 acc[2][2];

  // the prologue and the k-loop: one copy per sign mode (the activation registers belong to the copy: nothing but acc is
  // live where the copies meet)
  auto run = [&](auto SG) __attribute__((always_inline)) {
    // (a zero of the copy's own: one shared block of sixteen zeros ahead of the branch reaches the second copy through scratch)
    float zero = 0.f;
    if constexpr (decltype(SG)::value != 2) asm volatile("" : "+v"(zero));
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][j][r] = zero;
    float xb[2][8] = {};     // defined values: the surplus split of the last tile reads a set that was never loaded
    for (int u = 0; u < DA && u < T; ++u) issueA(u);
    fetchB(0, xb[0]);
    USE_X(xb[0], 0);
    if (T > 1) fetchB(1, xb[1]);
    split_store(SG, xb[0], Bst);
    if (T > 1) asm volatile("s_waitcnt vmcnt(8) lgkmcnt(0)\n\ts_barrier" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
    auto step = [&](int t, int cur, float (&xload)[8], float (&xsplit)[8]) __attribute__((always_inline)) {
      const u32x4* As = img + (2 * NSUB + t % SA) * SIMG + lh * SCH + wm * 64 + li;
      const u32x4* Bs = img + (sub * 2 + cur) * SIMG + lh * SCH + wn * 64 + li;
      const bool dmaA = t + DA < T, ldB = t + 2 < T;
      if (dmaA) issueA(t + DA);
      if (ldB) fetchB(t + 2, xload);
      // xsplit (tile t+1) was loaded a step ago; younger operations: this step's DMA piece(s) and 8 loads
      if (dmaA && ldB && doA2) USE_X(xsplit, 10);
      else if (dmaA && ldB && doA) USE_X(xsplit, 9);
      else if (ldB) USE_X(xsplit, 8);
      else USE_X(xsplit, 0);
      if constexpr (NP == 3) {
        // three planes at 128 registers: the B fragments of ONE plane at a time (8 registers instead of 24), planes
        // in the order l, m, h so that the products still arrive roughly smallest first:
        //   ah.bl | am.bm, ah.bm | al.bh, am.bh, ah.bh
        auto mfma_block = [&]() __attribute__((always_inline)) {
          u32x4 a[3][2], b[2];
#pragma unroll
          for (int pl = 0; pl < 3; ++pl) { a[pl][0] = As[pl * 2 * SCH]; a[pl][1] = As[pl * 2 * SCH + 32]; }
#pragma unroll
          for (int pb = 2; pb >= 0; --pb) {
            b[0] = Bs[pb * 2 * SCH]; b[1] = Bs[pb * 2 * SCH + 32];
#pragma unroll
            for (int pa = 2 - pb; pa >= 0; --pa)
#pragma unroll
              for (int tm = 0; tm < 2; ++tm)
#pragma unroll
                for (int tn = 0; tn < 2; ++tn) SPLIT_MFMA(a[pa][tm], b[tn], acc[tm][tn]);
          }
        };
#if SPLIT_STAGGER
        // SIMD partners out of phase (MI355X_MICROARCH.md, two waves per SIMD, item 9): waves 4-7 (sub 1) split and store
        // tile t+1 FIRST and multiply afterwards, waves 0-3 the other way round - one half of a SIMD's waves is on the
        // vector unit and the LDS store path while the other half feeds the matrix pipe
        // (ONE copy of the MFMA block: a second copy behind the branch spills the accumulators)
        if (sub == 1) split_store(SG, xsplit, Bst + (cur ^ 1) * SIMG);
        __builtin_amdgcn_sched_barrier(0);
        mfma_block();
        __builtin_amdgcn_sched_barrier(0);
        if (sub == 0) split_store(SG, xsplit, Bst + (cur ^ 1) * SIMG);
#else
        mfma_block();
        split_store(SG, xsplit, Bst + (cur ^ 1) * SIMG);
#endif
        // (no sched_group_barrier pinning here: the 1 MFMA : 3 VALU pattern of the 128 x 128 kernel measured 0.7 % slower
        //  on the step than the compiler's own order, three rounds on one box)
      } else {
        SplitFrags<NP> f;
        split_tile_read<NP, 2 * SCH, 2 * SCH>(As, Bs, f);
        split_tile_mfma<NP>(f, acc);
        split_store(SG, xsplit, Bst + (cur ^ 1) * SIMG);
        __builtin_amdgcn_sched_group_barrier(0x100, 4 * NP, 0);   // all fragment reads first, in first-use order
#pragma unroll
        for (int i = 0; i < 12; ++i) {
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
          __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);
        }
      }
      // weight tile t+1 landed (8 loads of this step are younger), own ds_writes done, the loads of t+2 in flight
      if (dmaA && ldB) asm volatile("s_waitcnt vmcnt(8) lgkmcnt(0)\n\ts_barrier" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
    };
    for (int t = 0; t < T; t += 2) {
      step(t, 0, xb[0], xb[1]);
      if (t + 1 < T) step(t + 1, 1, xb[1], xb[0]);
    }
  };
  if constexpr (NP == 3 && SPLIT_SIGN_LOOPS_FWD && SPLIT_SIGNED) {
    // the wave's column-block bit (= wn), chosen once: both copies issue the same barriers per step
    if (__builtin_amdgcn_readfirstlane((ltid >> 6) & 1)) run(std::integral_constant<int, 1>{});
    else run(std::integral_constant<int, 0>{});
  } else {
    run(std::integral_constant<int, 2>{});
  }
#undef USE_X
  if (live) {
    if constexpr (EPI != 0) {
      // The epilogue's lane values are derived afresh from ONE register (the thread index, opaque to the compiler from
      // here on): values of theirs that the compiler computes ahead of the k-loop stay live through it, and one register
      // more at the 128 this kernel has turns the k-loop's schedule into a pressure-driven one.
      int t = tid;
      asm volatile("" : "+v"(t));
      const int ew = __builtin_amdgcn_readfirstlane((t >> 6) & 3), ewm = ew >> 1, ewn = ew & 1, eli = t & 31, elh = (t >> 5) & 1;
      split_unflip(acc, ewn);
      if constexpr (NP == 2) split_unscale(acc, inv_a, inv_b);
      if (m0 + BM <= g.M && n0 + BN <= g.N) split_epilogue_interior<EPI>(g, acc, bz, m0, n0, ewm, ewn, eli, elh);
      else gemm_epilogue(g, acc, bz, m0, n0, ewm, ewn, eli, elh);
    } else {
      split_unflip(acc, wn);
      if constexpr (NP == 2) split_unscale(acc, inv_a, inv_b);
      gemm_epilogue(g, acc, bz, m0, n0, wm, wn, li, lh);
    }
  }
}

// (A 256 x 256 workgroup tile for the six-product kernel - sixteen waves, TWO copies of the arrangement above sharing the
//  STAGED activation tiles, so that a 16 x 256 fp32 tile is fetched from L2 and split into its bf16 planes once per 256 output
//  rows: 40 instead of 56 KB through L2 per 256 x 256 x 16 and half the split arithmetic per MFMA; the copies take turns
//  fetching / splitting; 96 KB of LDS, one 1024-thread workgroup per CU; bit-identical results - was built in round 6
//  (`pw_gemm_split_quad_kernel`; the structure is all that is recorded) and measured on the training step: 156.2 / 157.0 against 154.8 / 155.0 ms,
//  same box.  Fewer L2 bytes and fewer VALU operations per MFMA buy nothing: what bounds these kernels is the matrix pipe
//  under the chip's power budget (busy x clock), as the yardstick of DESIGN.md 4.1 says.  Removed; profiles/r06_gemm_quad.txt.)

// ---- host side ----------------------------------------------------------------------------------------------------------
constexpr size_t split_lds(int np) { return (size_t)(2 + split_astages(np)) * simg(np) * 16; }
constexpr int AMAX_WORDS = PARADIS_AMAX_PARTIALS;
// f16x2 weight image: the planes, then 16 bytes ([0] = bits of max |W|), then the amax partials of W
constexpr size_t F16_TAIL_BYTES = 16 + (size_t)AMAX_WORDS * 4;

// k16 tiles of an image: the one-plane (bf16) layout is read in pairs of tiles (pw_gemm_bf16_k32_kernel): an even count
int split_image_ktiles(int K, int np) {
  const int kt = (K + SBK - 1) / SBK;
  return np == 1 ? (kt + 1) & ~1 : kt;
}
int64_t split_image_chunks(int M, int K, int np = 3) {
  return (int64_t)((M + BM - 1) / BM) * split_image_ktiles(K, np) * simg(np);
}

int launch_amax(const float* x, int B, int64_t inner, int64_t bs, uint32_t* out, hipStream_t st) {
  const int vec = (inner % 4 == 0) && (bs % 4 == 0) && aligned16(x);
  hipLaunchKernelGGL(amax_partials_kernel, dim3(AMAX_WORDS), dim3(256), 0, st, x, B, inner, bs, vec, out);
  return 0;
}

constexpr size_t split_wide_lds(int nsub, int np = 2) { return (size_t)(2 * nsub + 2) * simg(np) * 16; }   // f16x2: 48 KiB, bf16x3: 72 KiB
// n-tiles per workgroup: 2 (two 8-wave workgroups per CU).  4 - one 16-wave workgroup per CU, another 17 % fewer
// bytes - measured 2.5 % SLOWER: a single workgroup's waves all stop at the same barriers.
constexpr int SPLIT_WIDE_NSUB = 2;
// bf16x3 on the 128 x 256 tile (round 3).  With all twelve fragments of a k-tile live (the 128 x 128 kernel's way) the
// kernel needs ~150 registers and hipcc spills 1.2 KB per lane at the 128 that two 8-wave workgroups per CU allow;
// reading the B fragments one PLANE at a time (8 instead of 24 registers, planes in the order l, m, h) brings it to
// 128 registers and 12 bytes of scratch.  Training step 160.0 -> 156.3 ms, GEMMs 188 -> 194 TF (same box, two rounds).
#ifndef SPLIT_WIDE_BF16X3      // (0: the 128 x 128 kernel for every shape; A/B builds)
#define SPLIT_WIDE_BF16X3 1
#endif
// the kernel tables, all [NP - 2]: 128 x 128 tile, 128 x (128 NSUB) tile, weight gradient
constexpr GemmKernelEntry SPLIT[2] = {{&pw_gemm_split_kernel<2>, split_lds(2)}, {&pw_gemm_split_kernel<3>, split_lds(3)}};
constexpr GemmKernelEntry SPLIT_WIDE[2] = {{&pw_gemm_split_wide_kernel<SPLIT_WIDE_NSUB, 2>, split_wide_lds(SPLIT_WIDE_NSUB, 2)},
                                           {&pw_gemm_split_wide_kernel<SPLIT_WIDE_NSUB, 3>, split_wide_lds(SPLIT_WIDE_NSUB, 3)}};
// ([2]: bf16x3 with scalar-base loads, split_wgrad_a32)
constexpr GemmKernelEntry SPLIT_WGRAD[3] = {{&pw_gemm_wgrad_split_kernel<2>, split_lds_wgrad(2)},
                                            {&pw_gemm_wgrad_split_kernel<3>, split_lds_wgrad(3)},
                                            {&pw_gemm_wgrad_split_kernel<3, 1>, split_lds_wgrad(3)}};
// bf16x3 on the 128 x 256 tile with a compile-time epilogue: the option sets the default model's training step launches
// (DESIGN.md 4.1), SPLIT_WIDE_EPI_SETS[i] = the set of SPLIT_WIDE_EPI[i].  Any other set runs SPLIT_WIDE.
#define EPI_SETS(X)                                                                                                       \
  X(EP_ON) X(EP_ON | EP_ZMUL)                                                              /* data gradient */           \
  X(EP_ON | EP_BIAS) X(EP_ON | EP_BIAS | EP_RES) X(EP_ON | EP_BIAS | EP_RES | EP_GATE)     /* forward */                 \
  X(EP_ON | EP_BIAS | EP_SILU | EP_ZOUT) X(EP_ON | EP_BIAS | EP_MAP | EP_RES)                                            \
  X(EP_ON | EP_BIAS | EP_MAP | EP_SILU | EP_ZOUT)
#define EPI_SET(E) (E),
#define EPI_ENTRY(E) {&pw_gemm_split_wide_kernel<SPLIT_WIDE_NSUB, 3, (E)>, split_wide_lds(SPLIT_WIDE_NSUB, 3)},
constexpr int SPLIT_WIDE_EPI_SETS[] = {EPI_SETS(EPI_SET)};
constexpr GemmKernelEntry SPLIT_WIDE_EPI[] = {EPI_SETS(EPI_ENTRY)};
#undef EPI_ENTRY
#undef EPI_SET
#undef EPI_SETS

// the option set of a launch as split_epilogue_interior spells it; 0: a set it does not cover (the projected GlobalBias,
// GELU, an activation gradient without an activation, a lane offset beyond 32 bits).  PARADIS_GEMM_EPILOGUE=generic
// (read at every launch: an A/B, or a test of one path against the other, needs one process) answers 0 for every launch.
int split_epilogue_flags(const GemmArgs& d) {
  const char* e = getenv("PARADIS_GEMM_EPILOGUE");
  if (e && strcmp(e, "generic") == 0) return 0;
  if (d.pw || d.io16 || d.ldc >= (1 << 26) || (d.gate && !d.res)) return 0;
  if (d.zmul ? d.act != PARADIS_ACT_SILU : (d.act != 0 && d.act != PARADIS_ACT_SILU)) return 0;
  return EP_ON | (d.bias ? EP_BIAS : 0) | (d.map ? EP_MAP : 0) | (d.zout ? EP_ZOUT : 0) | (d.zmul ? EP_ZMUL : 0) |
         (!d.zmul && d.act ? EP_SILU : 0) | (d.res ? EP_RES : 0) | (d.gate ? EP_GATE : 0);
}

}  // namespace

extern "C" size_t paradis_pw_gemm_split_bytes(int M, int K, int scheme) {
  if (M < 1 || K < 1) return 0;
  if (scheme == PARADIS_GEMM_F16X2) return (size_t)split_image_chunks(M, K, 2) * 16 + F16_TAIL_BYTES;
  if (scheme == PARADIS_GEMM_BF16) return (size_t)split_image_chunks(M, K, 1) * 16;
  return scheme == PARADIS_GEMM_BF16X3 ? (size_t)split_image_chunks(M, K, 3) * 16 : 0;
}

extern "C" int paradis_amax_partials(const float* x, int B, int64_t inner, int64_t bs, uint32_t* partials,
                                     void* stream) {
  PD_REQUIRE(partials != nullptr && B >= 0 && inner >= 0 && (x != nullptr || B == 0 || inner == 0),
             "amax_partials: bad arguments");
  launch_amax(x, B, inner, bs, partials, (hipStream_t)stream);
  PD_CHECK_LAUNCH("amax_partials");
  return 0;
}

// Split image (tile order) of A = W[M,K] (transpose = 0) or of A = W^T[K,M] (transpose = 1, from the same
// row-major W[M,K]); out holds split_bytes(M,K,scheme) resp. split_bytes(K,M,scheme).  BF16X3: h/m/l bf16
// planes.  F16X2: h/l f16 planes of W 2^e and, behind them, the bits of max |W|.
extern "C" int paradis_pw_gemm_split_weights(const float* W, int M, int K, int transpose, int scheme, void* out,
                                             void* stream) {
  PD_REQUIRE(W != nullptr && out != nullptr && M >= 1 && K >= 1, "pw_gemm_split_weights: bad arguments");
  PD_REQUIRE(scheme == PARADIS_GEMM_BF16X3 || scheme == PARADIS_GEMM_F16X2 || scheme == PARADIS_GEMM_BF16,
             "pw_gemm_split_weights: unknown scheme %d", scheme);
  const int AM = transpose ? K : M, AK = transpose ? M : K;
  const int KT = split_image_ktiles(AK, scheme == PARADIS_GEMM_BF16 ? 1 : 3);
  const int64_t units = (int64_t)((AM + BM - 1) / BM) * KT * 256;
  const int blocks = (int)std::min<int64_t>((units + 255) / 256, 4096);
  if (scheme == PARADIS_GEMM_F16X2) {
    uint32_t* tail = reinterpret_cast<uint32_t*>((char*)out + (size_t)split_image_chunks(AM, AK, 2) * 16);
    launch_amax(W, 1, (int64_t)M * K, 0, tail + 4, (hipStream_t)stream);
    hipLaunchKernelGGL(split_weights_f16_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, W,
                       (int64_t)(transpose ? 1 : K), (int64_t)(transpose ? K : 1), AM, AK, KT, units, (u32x4*)out, tail);
  } else if (scheme == PARADIS_GEMM_BF16) {
    hipLaunchKernelGGL(split_weights_kernel<1>, dim3(blocks, 1), dim3(256), 0, (hipStream_t)stream, W,
                       (int64_t)(transpose ? 1 : K), (int64_t)(transpose ? K : 1), AM, AK, KT, units,
                       (int64_t)0, (int64_t)0, (u32x4*)out);
  } else {
    hipLaunchKernelGGL(split_weights_kernel<3>, dim3(blocks, 1), dim3(256), 0, (hipStream_t)stream, W,
                       (int64_t)(transpose ? 1 : K), (int64_t)(transpose ? K : 1), AM, AK, KT, units,
                       (int64_t)0, (int64_t)0, (u32x4*)out);
  }
  PD_CHECK_LAUNCH("pw_gemm_split_weights");
  return 0;
}

// images of W[M,K] (-> out, split_bytes(M,K,scheme)) and of W^T (-> out_t, split_bytes(K,M,scheme)) in one launch:
// PARADIS_GEMM_BF16X3 or PARADIS_GEMM_BF16 (the f16x2 image needs the amax of W first: paradis_pw_gemm_split_weights)
extern "C" int paradis_pw_gemm_split_weights_pair_scheme(const float* W, int M, int K, int scheme, void* out, void* out_t,
                                                         void* stream) {
  PD_REQUIRE(W != nullptr && out != nullptr && out_t != nullptr && out != out_t && M >= 1 && K >= 1,
             "pw_gemm_split_weights_pair: bad arguments");
  PD_REQUIRE(scheme == PARADIS_GEMM_BF16X3 || scheme == PARADIS_GEMM_BF16,
             "pw_gemm_split_weights_pair: scheme %d has no paired images", scheme);
  const int np = scheme == PARADIS_GEMM_BF16 ? 1 : 3;
  const int KT = split_image_ktiles(K, np), KTt = split_image_ktiles(M, np);      // (bf16-mixed images: an even count of k16 tiles)
  const int64_t units = (int64_t)((M + BM - 1) / BM) * KT * 256, units_t = (int64_t)((K + BM - 1) / BM) * KTt * 256;
  const int blocks = (int)std::min<int64_t>((std::max(units, units_t) + 255) / 256, 4096);
  if (scheme == PARADIS_GEMM_BF16X3)
    hipLaunchKernelGGL(split_weights_pair_kernel<3>, dim3(blocks, 2), dim3(256), 0, (hipStream_t)stream, W, M, K, KT, KTt,
                       units, units_t, (u32x4*)out, (u32x4*)out_t);
  else
    hipLaunchKernelGGL(split_weights_pair_kernel<1>, dim3(blocks, 2), dim3(256), 0, (hipStream_t)stream, W, M, K, KT, KTt,
                       units, units_t, (u32x4*)out, (u32x4*)out_t);
  PD_CHECK_LAUNCH("pw_gemm_split_weights_pair");
  return 0;
}
// (ABI 7's spelling: the bf16x3 pair)
extern "C" int paradis_pw_gemm_split_weights_pair(const float* W, int M, int K, void* out, void* out_t, void* stream) {
  return paradis_pw_gemm_split_weights_pair_scheme(W, M, K, PARADIS_GEMM_BF16X3, out, out_t, stream);
}


// ---- what gemm.hip calls --------------------------------------------------------------------------------------------------
int pd_split_launch(const GemmArgs& d, int scheme, hipStream_t st) {
  static PerDeviceOnce once, once_wide, once_epi;
  const int np = scheme == PARADIS_GEMM_F16X2 ? 2 : 3;
  const int MT = (d.M + BM - 1) / BM, NT = (d.N + BN - 1) / BN;
  if (NT >= 2 && np == 3 && SPLIT_WIDE_BF16X3) {      // ... with the launch's option set compiled in, where one is built
    constexpr int NE = sizeof(SPLIT_WIDE_EPI_SETS) / sizeof(int);
    const int set = split_epilogue_flags(d);
    for (int i = 0; set != 0 && i < NE; ++i)
      if (SPLIT_WIDE_EPI_SETS[i] == set)
        return launch_entry(SPLIT_WIDE_EPI, i, once_epi, "pw_gemm(split)", MT * ((NT + SPLIT_WIDE_NSUB - 1) / SPLIT_WIDE_NSUB) * d.nbatch,
                            256 * SPLIT_WIDE_NSUB, st, d);
  }
  if (NT >= 2 && (np == 2 || SPLIT_WIDE_BF16X3))      // 128 x (128 NSUB) tiles
    return launch_entry(SPLIT_WIDE, np - 2, once_wide, "pw_gemm(split)", MT * ((NT + SPLIT_WIDE_NSUB - 1) / SPLIT_WIDE_NSUB) * d.nbatch,
                        256 * SPLIT_WIDE_NSUB, st, d);
  return launch_entry(SPLIT, np - 2, once, "pw_gemm(split)", MT * NT * d.nbatch, 256, st, d);
}

// pw_gemm_wgrad_split_kernel<3, 1> adds an unsigned 32-bit BYTE offset to the pointer of a tile's first row: the last
// access of a tile ends (127 ld + 16) x 4 bytes behind it, below 2^31 for ld < 2^22.  Leading dimensions from 2^22 floats
// on (16 MiB rows) take <3, 0>, today's 64-bit vector addresses; neither that fallback nor the ldc >= 2^26 generic
// epilogue is reached by a test - an operand of such rows is tens of GiB.
bool split_wgrad_a32(const GemmArgs& g) {
  constexpr int64_t LIM = (int64_t)1 << 22;
  return SPLIT_WGRAD_SADDR && g.lda >= 0 && g.lda < LIM && g.ldb >= 0 && g.ldb < LIM;
}

int pd_split_launch_wgrad(const GemmArgs& g, const WgradPlan& p, hipStream_t st) {
  static PerDeviceOnce once;
  if (p.kind == WgradKind::F16x2) return launch_entry(SPLIT_WGRAD, 0, once, "pw_gemm_wgrad(split)", p.grid, p.block, st, g, p.lds);
  GemmArgs d = g;
  const char* e = getenv("PARADIS_GEMM_EPILOGUE");      // (read at every launch, as split_epilogue_flags does)
  d.generic_epilogue = (e && strcmp(e, "generic") == 0) || d.ldc >= (1 << 26);
  return launch_entry(SPLIT_WGRAD, split_wgrad_a32(d) ? 2 : 1, once, "pw_gemm_wgrad(split)", p.grid, p.block, st, d, p.lds);
}

int64_t pd_split_image_chunks(int M, int K, int np) { return split_image_chunks(M, K, np); }

void pd_split_launch_images(const float* A, int nbatch, int M, int K, int64_t a_bs, void* out, hipStream_t st) {
  const int KT = (K + SBK - 1) / SBK;
  const int64_t units = (int64_t)((M + BM - 1) / BM) * KT * 256;
  const int blocks = (int)std::min<int64_t>((units + 255) / 256, 1024);
  hipLaunchKernelGGL(split_weights_kernel<3>, dim3(blocks, nbatch), dim3(256), 0, st, A, (int64_t)K, (int64_t)1, M, K, KT, units,
                     a_bs, split_image_chunks(M, K), (u32x4*)out);
}
