// Weight-gradient kernels of the bf16-mixed scheme (PARADIS_GEMM_BF16) and their launcher pd_amp_launch_wgrad, called from
// gemm.hip with the plan (WgradKind::Amp128 / Tall / Square); the 128 x 128 kernel for fp32 operands is
// pw_gemm_wgrad_split_kernel<1> of gemm_common.h.
#include "gemm_common.h"

namespace {

// the registers r of a fetch are complete once at most S younger loads of this wave are in flight
#define USE_RN(r, S) do { asm volatile("s_waitcnt vmcnt(" S ")" :: "v"(r.a0), "v"(r.a1), "v"(r.b0), "v"(r.b1) : "memory"); \
                          __builtin_amdgcn_sched_barrier(0); } while (0)

// PARADIS_GEMM_BF16 weight gradient with bf16-STORED operands (round 6): pw_gemm_wgrad_split_kernel<1> with the staging
// of a bf16 operand reduced to one 16-byte load per thread and k-tile - the eight values ARE the LDS chunk (no rounding,
// no packing; the slab's sign alternation is an XOR on the packed sign bits) - while an fp32 operand is rounded in
// registers as before.  A16: dY is bf16 (GemmArgs::io16 & IO_A16), B16: X is bf16 (IO_B16).  Same tiles, slabs, row sums
// and epilogue; rows need 16-byte alignment in their own element size (host-checked).
template <bool A16, bool B16>
__global__ void __launch_bounds__(256, 3)
pw_gemm_wgrad_b16_kernel(GemmArgs g) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int SIMGP = simgp(1);
  u32x4* img = reinterpret_cast<u32x4*>(lds);        // [2 stages][A|B][SIMGP]
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
  const int KT = g.K / SBK;
  const int64_t total = (int64_t)g.inner * KT;
  const int t_begin = (int)(total * bz / g.nbatch);
  const int T = (int)(total * (bz + 1) / g.nbatch) - t_begin;

  const int srow = tid >> 1, sh = tid & 1;
  // byte addresses: element size 2 or 4 per operand
  constexpr int EA = A16 ? 2 : 4, EB = B16 ? 2 : 4;
  const char* Ag = reinterpret_cast<const char*>(g.A) + ((int64_t)min(m0 + srow, g.M - 1) * g.lda + sh * 8) * EA;
  const char* Bg = reinterpret_cast<const char*>(g.B) + ((int64_t)min(n0 + srow, g.N - 1) * g.ldb + sh * 8) * EB;

  int f_ib = t_begin / KT, f_kt = t_begin - f_ib * KT;
  struct Regs { f32x4 a0, a1, b0, b1; };
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  Regs r0{zero4, zero4, zero4, zero4}, r1 = r0;
  auto fetch = [&](Regs& r) __attribute__((always_inline)) {
    const char* a = Ag + ((int64_t)f_ib * g.a_is + (int64_t)f_kt * SBK) * EA;
    const char* b = Bg + ((int64_t)f_ib * g.b_is + (int64_t)f_kt * SBK) * EB;
    asm volatile("global_load_dwordx4 %0, %1, off" : "=&v"(r.a0) : "v"(a) : "memory");
    if constexpr (!A16) asm volatile("global_load_dwordx4 %0, %1, off offset:16" : "=&v"(r.a1) : "v"(a) : "memory");
    asm volatile("global_load_dwordx4 %0, %1, off" : "=&v"(r.b0) : "v"(b) : "memory");
    if constexpr (!B16) asm volatile("global_load_dwordx4 %0, %1, off offset:16" : "=&v"(r.b1) : "v"(b) : "memory");
    if (++f_kt == KT) { f_kt = 0; ++f_ib; }
  };
  constexpr int NL = (A16 ? 1 : 2) + (B16 ? 1 : 2);      // loads per fetch
  auto wait_keep_one = [&](Regs& r) __attribute__((always_inline)) {      // the younger fetch may stay in flight
    if constexpr (NL == 4) USE_RN(r, "4"); else if constexpr (NL == 3) USE_RN(r, "3"); else USE_RN(r, "2");
  };
  const bool do_rowsum = g.rowsum != nullptr && nt == 0;
  float rs = 0.f;
  const uint32_t slab_flip = (SPLIT_SIGNED_WGRAD && (bz & 1)) ? 0x80000000u : 0u;      // workgroup-uniform
  const uint32_t slab_flip16 = slab_flip | (slab_flip >> 16);
  auto split_store = [&](const Regs& r, int st, bool keep) __attribute__((always_inline)) {
    u32x4* o = img + st * 2 * SIMGP + sh * SCHP + srow;
    if constexpr (A16) {
      const u32x4 c = __builtin_bit_cast(u32x4, r.a0);
      if (do_rowsum) {       // (workgroup-uniform) bias gradient: row sums of the staged dY values
        float add = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) add += __uint_as_float(c[i] << 16) + __uint_as_float(c[i] & 0xffff0000u);
        rs += keep ? add : 0.f;
      }
      o[0] = (u32x4){c[0] ^ slab_flip16, c[1] ^ slab_flip16, c[2] ^ slab_flip16, c[3] ^ slab_flip16};
    } else {
      const float xa[8] = {r.a0.x, r.a0.y, r.a0.z, r.a0.w, r.a1.x, r.a1.y, r.a1.z, r.a1.w};
      const float add = ((xa[0] + xa[1]) + (xa[2] + xa[3])) + ((xa[4] + xa[5]) + (xa[6] + xa[7]));
      rs += keep ? add : 0.f;
      float xs[8];
      flip8(xs, xa, slab_flip);
      o[0] = round8(xs);
    }
    if constexpr (B16) {
      o[SIMGP] = __builtin_bit_cast(u32x4, r.b0);
    } else {
      const float xb[8] = {r.b0.x, r.b0.y, r.b0.z, r.b0.w, r.b1.x, r.b1.y, r.b1.z, r.b1.w};
      o[SIMGP] = round8(xb);
    }
  };

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  if (T > 0) {
    fetch(r0);
    if (T > 1) { fetch(r1); wait_keep_one(r0); } else { USE_RN(r0, "0"); }
    split_store(r0, 0, do_rowsum);
  }
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");

  auto step = [&](int t, int cur, Regs& rload, Regs& rsplit) __attribute__((always_inline)) {
    const u32x4* As = img + cur * 2 * SIMGP + lh * SCHP + wm * 64 + li;
    const u32x4* Bs = img + (cur * 2 + 1) * SIMGP + lh * SCHP + wn * 64 + li;
    SplitFrags<1> f;
    split_tile_read<1, 2 * SCHP, 2 * SCHP>(As, Bs, f);
    __builtin_amdgcn_sched_barrier(0);
    if (t + 2 < T) { fetch(rload); wait_keep_one(rsplit); }
    else USE_RN(rsplit, "0");
    split_tile_mfma<1>(f, acc);
    split_store(rsplit, cur ^ 1, do_rowsum && t + 1 < T);
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
  };
  for (int t = 0; t < T; t += 2) {
    step(t, 0, r0, r1);
    if (t + 1 < T) step(t + 1, 1, r1, r0);
  }
  if (do_rowsum) {
    rs += __shfl_xor(rs, 1, 64);
    const int m = m0 + srow;
    if (sh == 0 && m < g.M) g.rowsum[(int64_t)bz * g.M + m] = rs;
  }
  if (slab_flip) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][j][r] = -acc[i][j][r];
  }
  gemm_epilogue(g, acc, bz, m0, n0, wm, wn, li, lh);
}

// PARADIS_GEMM_BF16 weight gradient on a 256 x 128 output tile (round 6).  With ONE product per k the 128 x 128 kernels
// above are bound by the bytes their workgroups pull from L2, not by the matrix pipe: every 128-row block of dY is read
// once per 128-column block of X and vice versa (1024 x 1024 at N = 65,536, bf16 operands: 2.1 GB per launch = the 250 us
// they take at the ~10 TB/s the L2 delivers to the CUs).  A tile twice as tall halves the re-reads of X: 1.6 GB.
// 512 threads = 4 (M) x 2 (N) waves of 64 x 64; thread t stages chunk (row t >> 1, k-half t & 1) of dY and, waves 0-3
// only, of X; A16 / B16 = the operand is stored as bf16 (one 16-byte load is the LDS chunk) or as fp32 (two loads,
// rounded in registers); otherwise the pipeline of pw_gemm_wgrad_b16_kernel: loads two tiles ahead, one barrier per tile,
// K-range slabs with alternating sign, fused row sums.
// (row pitches TALL_PA / TALL_PB, TALL_STAGE chunks per stage and tall_lds_bytes(): gemm_common.h, beside the plan)
template <bool A16, bool B16>
__global__ void __launch_bounds__(512, 4)
pw_gemm_wgrad_tall_kernel(GemmArgs g) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  u32x4* img = reinterpret_cast<u32x4*>(lds);        // [2 stages][A: 2 x TALL_PA | B: 2 x TALL_PB]
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int li = lane & 31, lh = lane >> 5;
  const bool stB = wave < 4;                          // wave-uniform: these waves also stage X

  const int MT = (g.M + 255) / 256, NT = (g.N + BN - 1) / BN;
  int L;
  {
    const int nwg = gridDim.x, id = blockIdx.x;
    const int q = nwg >> 3, r = nwg & 7, xcd = id & 7;
    L = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (id >> 3);
  }
  const int mt = L % MT, nt = (L / MT) % NT, bz = L / (MT * NT);
  const int m0 = mt * 256, n0 = nt * BN;
  const int KT = g.K / SBK;
  const int64_t total = (int64_t)g.inner * KT;
  const int t_begin = (int)(total * bz / g.nbatch);
  const int T = (int)(total * (bz + 1) / g.nbatch) - t_begin;

  const int srow = tid >> 1, sh = tid & 1;
  constexpr int EA = A16 ? 2 : 4, EB = B16 ? 2 : 4;
  const char* Ag = reinterpret_cast<const char*>(g.A) + ((int64_t)min(m0 + srow, g.M - 1) * g.lda + sh * 8) * EA;
  const char* Bg = reinterpret_cast<const char*>(g.B) + ((int64_t)min(n0 + (srow & 127), g.N - 1) * g.ldb + sh * 8) * EB;

  int f_ib = t_begin / KT, f_kt = t_begin - f_ib * KT;
  struct Regs { f32x4 a0, a1, b0, b1; };
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  Regs r0{zero4, zero4, zero4, zero4}, r1 = r0;
  auto fetch = [&](Regs& r) __attribute__((always_inline)) {
    const char* a = Ag + ((int64_t)f_ib * g.a_is + (int64_t)f_kt * SBK) * EA;
    asm volatile("global_load_dwordx4 %0, %1, off" : "=&v"(r.a0) : "v"(a) : "memory");
    if constexpr (!A16) asm volatile("global_load_dwordx4 %0, %1, off offset:16" : "=&v"(r.a1) : "v"(a) : "memory");
    if (stB) {
      const char* b = Bg + ((int64_t)f_ib * g.b_is + (int64_t)f_kt * SBK) * EB;
      asm volatile("global_load_dwordx4 %0, %1, off" : "=&v"(r.b0) : "v"(b) : "memory");
      if constexpr (!B16) asm volatile("global_load_dwordx4 %0, %1, off offset:16" : "=&v"(r.b1) : "v"(b) : "memory");
    }
    if (++f_kt == KT) { f_kt = 0; ++f_ib; }
  };
  constexpr int NLA = A16 ? 1 : 2, NLB = B16 ? 1 : 2;
  // the registers of the older fetch are complete; the younger fetch (NLA or NLA + NLB loads of this wave) stays in flight
  auto wait_keep_one = [&](Regs& r) __attribute__((always_inline)) {
    if (stB) {
      if constexpr (NLA + NLB == 4) USE_RN(r, "4"); else if constexpr (NLA + NLB == 3) USE_RN(r, "3"); else USE_RN(r, "2");
    } else {
      if constexpr (NLA == 2) USE_RN(r, "2"); else USE_RN(r, "1");
    }
  };
  const bool do_rowsum = g.rowsum != nullptr && nt == 0;
  float rs = 0.f;
  const uint32_t slab_flip = (SPLIT_SIGNED_WGRAD && (bz & 1)) ? 0x80000000u : 0u;      // workgroup-uniform
  const uint32_t slab_flip16 = slab_flip | (slab_flip >> 16);
  auto split_store = [&](const Regs& r, int st, bool keep) __attribute__((always_inline)) {
    u32x4* o = img + st * TALL_STAGE + sh * TALL_PA + srow;
    if constexpr (A16) {
      const u32x4 c = __builtin_bit_cast(u32x4, r.a0);
      if (do_rowsum) {
        float add = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) add += __uint_as_float(c[i] << 16) + __uint_as_float(c[i] & 0xffff0000u);
        rs += keep ? add : 0.f;
      }
      o[0] = (u32x4){c[0] ^ slab_flip16, c[1] ^ slab_flip16, c[2] ^ slab_flip16, c[3] ^ slab_flip16};
    } else {
      const float xa[8] = {r.a0.x, r.a0.y, r.a0.z, r.a0.w, r.a1.x, r.a1.y, r.a1.z, r.a1.w};
      const float add = ((xa[0] + xa[1]) + (xa[2] + xa[3])) + ((xa[4] + xa[5]) + (xa[6] + xa[7]));
      rs += keep ? add : 0.f;
      float xs[8];
      flip8(xs, xa, slab_flip);
      o[0] = round8(xs);
    }
    if (stB) {
      u32x4* ob = img + st * TALL_STAGE + 2 * TALL_PA + sh * TALL_PB + srow;      // (srow < 128 in these waves)
      if constexpr (B16) {
        ob[0] = __builtin_bit_cast(u32x4, r.b0);
      } else {
        const float xb[8] = {r.b0.x, r.b0.y, r.b0.z, r.b0.w, r.b1.x, r.b1.y, r.b1.z, r.b1.w};
        ob[0] = round8(xb);
      }
    }
  };

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  if (T > 0) {
    fetch(r0);
    if (T > 1) { fetch(r1); wait_keep_one(r0); } else { USE_RN(r0, "0"); }
    split_store(r0, 0, do_rowsum);
  }
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");

  auto step = [&](int t, int cur, Regs& rload, Regs& rsplit) __attribute__((always_inline)) {
    const u32x4* As = img + cur * TALL_STAGE + lh * TALL_PA + wm * 64 + li;
    const u32x4* Bs = img + cur * TALL_STAGE + 2 * TALL_PA + lh * TALL_PB + wn * 64 + li;
    SplitFrags<1> f;
    split_tile_read<1, 0, 0>(As, Bs, f);
    __builtin_amdgcn_sched_barrier(0);
    if (t + 2 < T) { fetch(rload); wait_keep_one(rsplit); }
    else USE_RN(rsplit, "0");
    split_tile_mfma<1>(f, acc);
    split_store(rsplit, cur ^ 1, do_rowsum && t + 1 < T);
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
  };
  for (int t = 0; t < T; t += 2) {
    step(t, 0, r0, r1);
    if (t + 1 < T) step(t + 1, 1, r1, r0);
  }
  if (do_rowsum) {
    rs += __shfl_xor(rs, 1, 64);
    const int m = m0 + srow;
    if (sh == 0 && m < g.M) g.rowsum[(int64_t)bz * g.M + m] = rs;
  }
  if (slab_flip) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][j][r] = -acc[i][j][r];
  }
  // the wave's 64 rows as rows of the 128-row tile at m0 + 128 (wm >> 1)
  if (m0 + (wm >> 1) * 128 < g.M) gemm_epilogue(g, acc, bz, m0 + (wm >> 1) * 128, n0, wm & 1, wn, li, lh);
}

// (The bf16x3 - fp32-width - weight gradient on this 256 x 128 tile, three planes per operand image and 24 MFMAs per wave
//  and k-tile in the 128 registers that two 8-wave workgroups per CU leave, was tried in round 6: the step went from 150 to
//  308 ms - the twelve operand fragments next to 64 accumulators spill - and it failed the accuracy test; removed.  The
//  six-product kernels are bound by the matrix pipe's power budget, not by L2 bytes: DESIGN.md section 4.1.)
// ... and on a 256 x 256 tile (1.07 GB): 4 x 2 waves of 64 x 128, 128 accumulator registers per lane, ONE workgroup per CU
// (two waves per SIMD: enough for a kernel that waits on L2 bytes, not on the matrix pipe); every thread stages one chunk of
// each operand.  1024 x 1024, bf16 operands: 296 us (128 x 128) -> 250 (256 x 128) -> 221 (256 x 256).  PARADIS_WGRAD_SQUARE=0 /
// PARADIS_WGRAD_TALL=0 select the smaller tiles (A/B runs).
// (row pitch SQ_P, SQ_STAGE chunks per stage and sq_lds_bytes(): gemm_common.h)
template <bool A16, bool B16>
__global__ void __launch_bounds__(512, 2)
pw_gemm_wgrad_square_kernel(GemmArgs g) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  u32x4* img = reinterpret_cast<u32x4*>(lds);        // [4 stages][A: 2 x SQ_P | B: 2 x SQ_P]
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int li = lane & 31, lh = lane >> 5;
  constexpr bool stB = true;

  const int MT = (g.M + 255) / 256, NT = (g.N + 255) / 256;
  int L;
  {
    const int nwg = gridDim.x, id = blockIdx.x;
    const int q = nwg >> 3, r = nwg & 7, xcd = id & 7;
    L = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (id >> 3);
  }
  const int mt = L % MT, nt = (L / MT) % NT, bz = L / (MT * NT);
  const int m0 = mt * 256, n0 = nt * 256;
  const int KT = g.K / SBK;
  const int64_t total = (int64_t)g.inner * KT;
  const int t_begin = (int)(total * bz / g.nbatch);
  const int T = (int)(total * (bz + 1) / g.nbatch) - t_begin;

  const int srow = tid >> 1, sh = tid & 1;
  constexpr int EA = A16 ? 2 : 4, EB = B16 ? 2 : 4;
  const char* Ag = reinterpret_cast<const char*>(g.A) + ((int64_t)min(m0 + srow, g.M - 1) * g.lda + sh * 8) * EA;
  const char* Bg = reinterpret_cast<const char*>(g.B) + ((int64_t)min(n0 + srow, g.N - 1) * g.ldb + sh * 8) * EB;

  int f_ib = t_begin / KT, f_kt = t_begin - f_ib * KT;
  struct Regs { f32x4 a0, a1, b0, b1; };
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  Regs r0{zero4, zero4, zero4, zero4}, r1 = r0;
  auto fetch = [&](Regs& r) __attribute__((always_inline)) {
    const char* a = Ag + ((int64_t)f_ib * g.a_is + (int64_t)f_kt * SBK) * EA;
    asm volatile("global_load_dwordx4 %0, %1, off" : "=&v"(r.a0) : "v"(a) : "memory");
    if constexpr (!A16) asm volatile("global_load_dwordx4 %0, %1, off offset:16" : "=&v"(r.a1) : "v"(a) : "memory");
    if (stB) {
      const char* b = Bg + ((int64_t)f_ib * g.b_is + (int64_t)f_kt * SBK) * EB;
      asm volatile("global_load_dwordx4 %0, %1, off" : "=&v"(r.b0) : "v"(b) : "memory");
      if constexpr (!B16) asm volatile("global_load_dwordx4 %0, %1, off offset:16" : "=&v"(r.b1) : "v"(b) : "memory");
    }
    if (++f_kt == KT) { f_kt = 0; ++f_ib; }
  };
  constexpr int NLA = A16 ? 1 : 2, NLB = B16 ? 1 : 2;
  // the registers of the older fetch are complete; the younger fetch (NLA or NLA + NLB loads of this wave) stays in flight
  auto wait_keep_one = [&](Regs& r) __attribute__((always_inline)) {
    if (stB) {
      if constexpr (NLA + NLB == 4) USE_RN(r, "4"); else if constexpr (NLA + NLB == 3) USE_RN(r, "3"); else USE_RN(r, "2");
    } else {
      if constexpr (NLA == 2) USE_RN(r, "2"); else USE_RN(r, "1");
    }
  };
  const bool do_rowsum = g.rowsum != nullptr && nt == 0;
  float rs = 0.f;
  const uint32_t slab_flip = (SPLIT_SIGNED_WGRAD && (bz & 1)) ? 0x80000000u : 0u;      // workgroup-uniform
  const uint32_t slab_flip16 = slab_flip | (slab_flip >> 16);
  auto split_store = [&](const Regs& r, int st, bool keep) __attribute__((always_inline)) {
    u32x4* o = img + st * SQ_STAGE + sh * SQ_P + srow;
    if constexpr (A16) {
      const u32x4 c = __builtin_bit_cast(u32x4, r.a0);
      if (do_rowsum) {
        float add = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) add += __uint_as_float(c[i] << 16) + __uint_as_float(c[i] & 0xffff0000u);
        rs += keep ? add : 0.f;
      }
      o[0] = (u32x4){c[0] ^ slab_flip16, c[1] ^ slab_flip16, c[2] ^ slab_flip16, c[3] ^ slab_flip16};
    } else {
      const float xa[8] = {r.a0.x, r.a0.y, r.a0.z, r.a0.w, r.a1.x, r.a1.y, r.a1.z, r.a1.w};
      const float add = ((xa[0] + xa[1]) + (xa[2] + xa[3])) + ((xa[4] + xa[5]) + (xa[6] + xa[7]));
      rs += keep ? add : 0.f;
      float xs[8];
      flip8(xs, xa, slab_flip);
      o[0] = round8(xs);
    }
    if (stB) {
      u32x4* ob = img + st * SQ_STAGE + 2 * SQ_P + sh * SQ_P + srow;      // (srow < 128 in these waves)
      if constexpr (B16) {
        ob[0] = __builtin_bit_cast(u32x4, r.b0);
      } else {
        const float xb[8] = {r.b0.x, r.b0.y, r.b0.z, r.b0.w, r.b1.x, r.b1.y, r.b1.z, r.b1.w};
        ob[0] = round8(xb);
      }
    }
  };

  f32x16 acc[2][2], acc2[2][2];     // columns wn 128 + [0, 64) and + [64, 128)
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) { acc[i][j][r] = 0.f; acc2[i][j][r] = 0.f; }

  {
    // Two k-tiles per barrier (sixteen MFMAs per wave between two barriers instead of eight): a ring of FOUR stages, tile t in
    // stage t & 3.  Entering a pair (t, t + 1) both tiles are staged and the loads of t + 2 / t + 3 sit in r0 / r1; inside the
    // pair tile t + 2 is stored behind the MFMAs of t and tile t + 3 behind those of t + 1 (their stages were last read a pair
    // ago: every wave is past that pair's barrier), each followed by the fetch of the tile four ahead.
    auto stage_tile = [&](int t, Regs& r, bool younger_in_flight) __attribute__((always_inline)) {
      if (younger_in_flight) wait_keep_one(r); else USE_RN(r, "0");
      split_store(r, t & 3, do_rowsum);
    };
    if (T > 0) { fetch(r0); }
    if (T > 1) { fetch(r1); }
    if (T > 0) { stage_tile(0, r0, T > 1); asm volatile("" : "+v"(rs)); if (T > 2) fetch(r0); }      // (the pin: see half())
    if (T > 1) { stage_tile(1, r1, T > 2); asm volatile("" : "+v"(rs)); if (T > 3) fetch(r1); }
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    auto half = [&](int t, Regs& r) __attribute__((always_inline)) {      // tile t is staged; r holds the loads of tile t + 2
      const u32x4* As = img + (t & 3) * SQ_STAGE + lh * SQ_P + wm * 64 + li;
      const u32x4* Bs = img + (t & 3) * SQ_STAGE + 2 * SQ_P + lh * SQ_P + wn * 128 + li;
      SplitFrags<1> f, f2;
      split_tile_read<1, 0, 0>(As, Bs, f);
      f2.a[0][0] = f.a[0][0]; f2.a[0][1] = f.a[0][1];
      f2.b[0][0] = Bs[64]; f2.b[0][1] = Bs[96];
      __builtin_amdgcn_sched_barrier(0);
      split_tile_mfma<1>(f, acc);
      split_tile_mfma<1>(f2, acc2);
      if (t + 2 < T) {
        stage_tile(t + 2, r, t + 3 < T);       // (the fetch of tile t + 3, issued after this one's, may stay in flight)
        // The row sum must be COMPLETE before the next fetch is issued.  Left alone, the compiler sinks the add chain of an
        // fp32 dY below the (volatile, but register-only) load statements: the old value of r then lives across them, the new
        // loads get other registers and a copy "new -> old registers" follows the load at once - it reads registers whose data
        // has not arrived, and the data lands later in registers that hold addresses by then (NaNs, memory faults on long
        // slabs: this schedule's first version; tools/async_load_check.py finds such copies in the ISA).
        asm volatile("" : "+v"(rs));
        if (t + 4 < T) fetch(r);
      }
    };
    for (int t = 0; t < T; t += 2) {
      half(t, r0);
      if (t + 1 < T) half(t + 1, r1);
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    }
  }
  if (do_rowsum) {
    rs += __shfl_xor(rs, 1, 64);
    const int m = m0 + srow;
    if (sh == 0 && m < g.M) g.rowsum[(int64_t)bz * g.M + m] = rs;
  }
  if (slab_flip) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) { acc[i][j][r] = -acc[i][j][r]; acc2[i][j][r] = -acc2[i][j][r]; }
  }
  // the wave's 64 rows as rows of the 128-row tile at m0 + 128 (wm >> 1)
  if (m0 + (wm >> 1) * 128 < g.M) {
    const int mm = m0 + (wm >> 1) * 128, nn = n0 + wn * 128;           // 64-column halves as "wn" 0 / 1 of a 128-column tile
    if (nn < g.N) {
      gemm_epilogue(g, acc, bz, mm, nn, wm & 1, 0, li, lh);
      gemm_epilogue(g, acc2, bz, mm, nn, wm & 1, 1, li, lh);
    }
  }
}

// the kernel families above by their two I/O-type flags (A16, B16); the 128 x 128 tile with both operands stored as
// fp32 is the shared weight-gradient kernel with one plane
constexpr GemmKernel WGRAD_SQUARE[4] = IO2_KERNELS(pw_gemm_wgrad_square_kernel), WGRAD_TALL[4] = IO2_KERNELS(pw_gemm_wgrad_tall_kernel);
constexpr GemmKernel WGRAD_128[4] = {&pw_gemm_wgrad_split_kernel<1>, &pw_gemm_wgrad_b16_kernel<true, false>,
                                     &pw_gemm_wgrad_b16_kernel<false, true>, &pw_gemm_wgrad_b16_kernel<true, true>};

}  // namespace

// ---- launcher of the bf16-mixed weight-gradient kernels (called from gemm.hip) ------------------------------------------
int pd_amp_launch_wgrad(const GemmArgs& g0, int io16, const WgradPlan& p, hipStream_t st) {
  GemmArgs g = g0;
  g.io16 = io16;
  const bool a16 = (io16 & IO_A16) != 0, b16 = (io16 & IO_B16) != 0;
  const dim3 grid(p.grid), block(p.block);
  if (p.kind == WgradKind::Square) return launch_io2<WGRAD_SQUARE>(a16, b16, grid, block, p.lds, "pw_gemm_wgrad(square)", st, g);
  if (p.kind == WgradKind::Tall) return launch_io2<WGRAD_TALL>(a16, b16, grid, block, p.lds, nullptr, st, g);
  return launch_io2<WGRAD_128>(a16, b16, grid, block, p.lds, nullptr, st, g);      // Amp128
}
