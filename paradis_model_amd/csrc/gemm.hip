// a6: pointwise (1x1) channel mixing as a batched GEMM on FP32 MFMA (v_mfma_f32_32x32x2_f32).
// Reference call sites: model/blocks.py:86 (CLinear), :110 (SepConv pointwise).
//
//   fwd   : Y[b][Co,P] = epi( W[Co,Ci] . X[b][Ci,P] )      A = W  (k-contiguous), B = X  (n-contiguous)
//   dgrad : dX[b][Ci,P] = epi( W^T . dY[b][Co,P] )         A = W^T(m-contiguous), B = dY (n-contiguous)
//   wgrad : dW[Co,Ci]   = sum_b dY[b] . X[b]^T             A = dY (k-contiguous), B = X^T(k-contiguous)
//
// Exact fp32: the f32 MFMA is a k-ordered fmaf chain (no TF32/xf32 on gfx950), so results differ
// from the CPU's blocked SGEMM only by summation order.
//
// Tile: 128x128x32 per 256-thread workgroup; wave (wm,wn) owns 64x64 = 2x2 MFMA 32x32 tiles
// (64 accumulator VGPRs).  Both operands are staged through registers into LDS as [k][m|n] images
// (row pitch 129 for transposing stores, 132 for vector stores: both conflict-free) so that
// fragment reads are conflict-free ds_read_b32; two LDS stages (66 KiB => exactly 2 workgroups per
// CU, which makes every shape of this model an integral number of rounds over the 256 CUs), one
// barrier per k-tile, global loads for tile t+1 in flight during the 64 MFMAs of tile t, fragment
// reads for k-step kk+1 issued before the MFMAs of kk.  Work-group ids are remapped so that the
// M-tiles that share one X tile run on the same XCD (L2 reuse of X).
#include <algorithm>
#include <cstdlib>
#include "gemm_common.h"

// The bf16-mixed scheme (PARADIS_GEMM_BF16) has its kernels and launchers in gemm_amp_fwd.hip (forward / data gradient)
// and gemm_amp_wgrad.hip (weight gradient); what the three units share is in gemm_common.h.

namespace {

constexpr int ld_of(bool kc) { return kc ? BM + 1 : BM + 4; }  // floats per k-row of the LDS image
constexpr int stage_floats(int bk) { return bk * (BM + 4); }   // per operand per stage (upper bound)
constexpr size_t lds_bytes(int bk) { return (size_t)4 * stage_floats(bk) * sizeof(float); }
constexpr int nv_of(int bk) { return BM * bk / (256 * 4); }    // float4 loads per thread per operand

// Tunables (debug setters below; defaults chosen from tools/gemm_bench.py measurements)
int g_bk = 16;            // k-tile depth: 16 or 32
int g_wg_per_cu = 4;      // resident workgroups per CU enforced through the dynamic-LDS request
int g_stagger = 0;        // see GemmArgs::stagger
int g_dma_stages = 3;     // LDS-DMA ring depth for row-contiguous operands (0 = never use the DMA kernel)
int g_wgrad_dma_stages = 2;  // LDS-DMA ring depth of the weight-gradient kernel (0 = register-staged)


// ---- staging: 128 x 16 operand slab -> registers -> LDS image [k][m] -------------------------
// KC: element (row=m|n, k) at base[row*ld + k]   (k contiguous)
// MC: element (row=m|n, k) at base[k*ld + row]   (row contiguous)
template <bool KC, int BK>
__device__ __forceinline__ void slab_load(const float* __restrict__ base, int64_t ld, int row0,
                                          int k0, int rows, int K, bool vec_ok,
                                          float4 (&r)[nv_of(BK)]) {
  constexpr int NV = nv_of(BK);
  constexpr int TPR = BK / 4;       // threads per row (k-contiguous layout)
  constexpr int RPP = 256 / TPR;    // rows per pass
  const int tid = threadIdx.x;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    if (KC) {
      const int row = row0 + (tid / TPR) + RPP * i, k = k0 + (tid % TPR) * 4;
      const float* p = base + (int64_t)row * ld + k;
      if (vec_ok && row < rows && k + 3 < K) {
        r[i] = *reinterpret_cast<const float4*>(p);
      } else {
        float t[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) t[j] = (row < rows && k + j < K) ? p[j] : 0.f;
        r[i] = make_float4(t[0], t[1], t[2], t[3]);
      }
    } else {
      const int k = k0 + (tid >> 5) + 8 * i, row = row0 + (tid & 31) * 4;
      const float* p = base + (int64_t)k * ld + row;
      if (vec_ok && k < K && row + 3 < rows) {
        r[i] = *reinterpret_cast<const float4*>(p);
      } else {
        float t[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) t[j] = (k < K && row + j < rows) ? p[j] : 0.f;
        r[i] = make_float4(t[0], t[1], t[2], t[3]);
      }
    }
  }
}

template <bool KC, int BK>
__device__ __forceinline__ void slab_store(float* __restrict__ img, const float4 (&r)[nv_of(BK)]) {
  constexpr int LD = ld_of(KC), NV = nv_of(BK);
  constexpr int TPR = BK / 4, RPP = 256 / TPR;
  const int tid = threadIdx.x;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    if (KC) {
      const int m = (tid / TPR) + RPP * i, k = (tid % TPR) * 4;
      img[(k + 0) * LD + m] = r[i].x;
      img[(k + 1) * LD + m] = r[i].y;
      img[(k + 2) * LD + m] = r[i].z;
      img[(k + 3) * LD + m] = r[i].w;
    } else {
      const int k = (tid >> 5) + 8 * i, m = (tid & 31) * 4;
      *reinterpret_cast<float4*>(img + k * LD + m) = r[i];
    }
  }
}

template <bool A_KC, bool B_KC, int BK>
__global__ void __launch_bounds__(256, (BK == 16 ? 4 : 2))
pw_gemm_kernel(GemmArgs g) {
  extern __shared__ __attribute__((aligned(16))) float lds[];  // [stage][A|B][STAGE_FLOATS]
  constexpr int LDA = ld_of(A_KC), LDB = ld_of(B_KC);
  constexpr int NV = nv_of(BK), STAGE_FLOATS = stage_floats(BK);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int li = lane & 31, lh = lane >> 5;

  // ---- XCD-aware decode: consecutive logical ids (same X tile, different M tiles) share an XCD
  const int MT = (g.M + BM - 1) / BM, NT = (g.N + BN - 1) / BN;
  int L;
  {
    const int nwg = gridDim.x, id = blockIdx.x;
    const int q = nwg >> 3, r = nwg & 7, xcd = id & 7;
    L = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (id >> 3);
  }
  const int mt = L % MT, nt = (L / MT) % NT, bz = L / (MT * NT);
  const int m0 = mt * BM, n0 = nt * BN;

  // k-tile range of this workgroup.  fwd/dgrad: all KT tiles of sample bz.  wgrad: the flattened
  // (sample, k-tile) sequence of inner*KT tiles is cut into nbatch equal contiguous ranges.
  const int KT = (g.K + BK - 1) / BK;
  int t_begin = 0, T = KT;
  if (g.inner > 0) {
    const int64_t total = (int64_t)g.inner * KT;
    t_begin = (int)(total * bz / g.nbatch);
    T = (int)(total * (bz + 1) / g.nbatch) - t_begin;
  }
  const float* Ab = g.A + (g.inner > 0 ? 0 : (int64_t)bz * g.a_bs);
  const float* Bb = g.B + (g.inner > 0 ? 0 : (int64_t)bz * g.b_bs);

  const bool a_vec = ((g.lda & 3) == 0) && ((reinterpret_cast<uintptr_t>(g.A) & 15) == 0) &&
                     ((g.a_bs & 3) == 0) && ((g.a_is & 3) == 0);
  const bool b_vec = ((g.ldb & 3) == 0) && ((reinterpret_cast<uintptr_t>(g.B) & 15) == 0) &&
                     ((g.b_bs & 3) == 0) && ((g.b_is & 3) == 0);

  // Co-resident workgroups of one CU (dispatch ids 256 apart) run the same program with one
  // barrier per k-tile and drift into lockstep: their non-MFMA phases (LDS store, barrier, global
  // issue) then coincide and the matrix pipe idles.  Skew their start by a fraction of a k-tile.
  if (g.stagger > 0) {
    const int lag = (blockIdx.x >> 8) & 3;
    for (int i = 0; i < lag * g.stagger; ++i) __builtin_amdgcn_s_sleep(8);
  }

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  float4 ra[NV], rb[NV];
  auto fetch = [&](int t) {
    const int tt = t_begin + t;
    const int ib = tt / KT, kt = tt - ib * KT;
    const float* Ap = Ab + (g.inner > 0 ? (int64_t)ib * g.a_is : 0);
    const float* Bp = Bb + (g.inner > 0 ? (int64_t)ib * g.b_is : 0);
    slab_load<A_KC, BK>(Ap, g.lda, m0, kt * BK, g.M, g.K, a_vec, ra);
    slab_load<B_KC, BK>(Bp, g.ldb, n0, kt * BK, g.N, g.K, b_vec, rb);
  };
  auto stageA = [&](int st) { return lds + (st * 2 + 0) * STAGE_FLOATS; };
  auto stageB = [&](int st) { return lds + (st * 2 + 1) * STAGE_FLOATS; };

  if (T > 0) {
    fetch(0);
    slab_store<A_KC, BK>(stageA(0), ra);
    slab_store<B_KC, BK>(stageB(0), rb);
  }
  __syncthreads();

  for (int t = 0; t < T; ++t) {
    const int cur = t & 1;
    if (t + 1 < T) fetch(t + 1);
    const float* As = stageA(cur) + wm * 64 + li + lh * LDA;
    const float* Bs = stageB(cur) + wn * 64 + li + lh * LDB;
    float a0 = As[0], a1 = As[32], b0 = Bs[0], b1 = Bs[32];
#pragma unroll
    for (int kk = 0; kk < BK / 2; ++kk) {
      float na0 = 0.f, na1 = 0.f, nb0 = 0.f, nb1 = 0.f;
      if (kk + 1 < BK / 2) {
        na0 = As[(2 * kk + 2) * LDA]; na1 = As[(2 * kk + 2) * LDA + 32];
        nb0 = Bs[(2 * kk + 2) * LDB]; nb1 = Bs[(2 * kk + 2) * LDB + 32];
      }
      acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
      a0 = na0; a1 = na1; b0 = nb0; b1 = nb1;
    }
    if (t + 1 < T) {
      slab_store<A_KC, BK>(stageA(cur ^ 1), ra);
      slab_store<B_KC, BK>(stageB(cur ^ 1), rb);
    }
    __syncthreads();
  }

  gemm_epilogue(g, acc, bz, m0, n0, wm, wn, li, lh);
}

// ======================================================================================
// LDS-DMA variant for row-contiguous operands (A(m,k) at A[k*lda+m], B(k,n) at B[k*ldb+n]):
// fwd with pre-transposed weights, dgrad.  Tiles go global -> LDS with global_load_lds_dwordx4
// (no VGPR staging, no ds_write), an S-deep LDS ring, counted vmcnt and a raw barrier per k-tile,
// so that S-1 tiles of loads stay in flight behind the MFMAs (measured on the register-staged
// kernel: exposed global-load latency costs ~25 % of the matrix pipe).
// Requirements (checked by the host, else the register-staged kernel is used):
//   K % 16 == 0, lda/ldb/batch strides multiples of 4 floats, 16-B aligned bases, M % 4 == N % 4 == 0.
// Out-of-range rows/cols of edge tiles are clamped to valid addresses; they only feed outputs
// that the epilogue discards.
// ======================================================================================
constexpr int DBK = 16;                 // k-tile depth of the DMA kernel
constexpr int DTILE = DBK * BM;         // floats per operand per stage (pitch 128, unpadded)


template <int S, int MINW>
__global__ void __launch_bounds__(256, MINW)
pw_gemm_dma_kernel(GemmArgs g) {
  extern __shared__ __attribute__((aligned(16))) float lds[];  // [S][A|B][DTILE]
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
  const int T = g.K / DBK;

  // this lane's source column inside a 2-row piece, clamped to stay inside the matrix
  const int pr = lane >> 5, pc = (lane & 31) * 4;
  const int acol = min(m0 + pc, g.M - 4), bcol = min(n0 + pc, g.N - 4);
  const float* Ap = g.A + (int64_t)bz * g.a_bs + (int64_t)(2 * (2 * wave) + pr) * g.lda + acol;
  const float* Bp = g.B + (int64_t)bz * g.b_bs + (int64_t)(2 * (2 * wave) + pr) * g.ldb + bcol;
  const int64_t a_piece = 2 * g.lda, b_piece = 2 * g.ldb;      // next 2-row piece
  const int64_t a_tile = (int64_t)DBK * g.lda, b_tile = (int64_t)DBK * g.ldb;

  auto issue = [&](int t) {
    float* st = lds + (t % S) * (2 * DTILE);
    const float* a = Ap + (int64_t)t * a_tile;
    const float* b = Bp + (int64_t)t * b_tile;
    // wave w owns pieces 2w, 2w+1 (k-rows 4w..4w+3) of both operands
    float* la = st + (2 * wave) * 256;
    float* lb = st + DTILE + (2 * wave) * 256;
    __builtin_amdgcn_global_load_lds((gbl_ptr_t)a, (lds_ptr_t)la, 16, 0, 0);
    __builtin_amdgcn_global_load_lds((gbl_ptr_t)(a + a_piece), (lds_ptr_t)(la + 256), 16, 0, 0);
    __builtin_amdgcn_global_load_lds((gbl_ptr_t)b, (lds_ptr_t)lb, 16, 0, 0);
    __builtin_amdgcn_global_load_lds((gbl_ptr_t)(b + b_piece), (lds_ptr_t)(lb + 256), 16, 0, 0);
  };

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

#pragma unroll
  for (int t = 0; t < S - 1; ++t)
    if (t < T) issue(t);

  for (int t = 0; t < T; ++t) {
    // tile t must have landed; up to S-2 younger tiles (4 DMAs each per wave) stay in flight
    const int pending = min(S - 2, T - 1 - t);
    if (pending >= 2) asm volatile("s_waitcnt vmcnt(8)\n\ts_barrier" ::: "memory");
    else if (pending == 1) asm volatile("s_waitcnt vmcnt(4)\n\ts_barrier" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
    // the stage of tile t-1 is free now (every wave has passed its MFMAs): refill it
    if (t + S - 1 < T) issue(t + S - 1);
    const float* As = lds + (t % S) * (2 * DTILE) + wm * 64 + li + lh * BM;
    const float* Bs = As - wm * 64 + DTILE + wn * 64;
    float a0 = As[0], a1 = As[32], b0 = Bs[0], b1 = Bs[32];
#pragma unroll
    for (int kk = 0; kk < DBK / 2; ++kk) {
      float na0 = 0.f, na1 = 0.f, nb0 = 0.f, nb1 = 0.f;
      if (kk + 1 < DBK / 2) {
        na0 = As[(2 * kk + 2) * BM]; na1 = As[(2 * kk + 2) * BM + 32];
        nb0 = Bs[(2 * kk + 2) * BN]; nb1 = Bs[(2 * kk + 2) * BN + 32];
      }
      acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
      a0 = na0; a1 = na1; b0 = nb0; b1 = nb1;
    }
  }
  gemm_epilogue(g, acc, bz, m0, n0, wm, wn, li, lh);
}

// ======================================================================================
// LDS-DMA weight-gradient kernel: dW[M,N'] = sum over (sample, p) of A[m][p] * B[n][p] with BOTH
// operands k(=p)-contiguous.  A 128x16 slab is DMA'd as 8 pieces of 16 rows x 64 B into a
// [row][16 k] LDS image whose 16-B chunks are XOR-swizzled on the SOURCE side
// (slot = chunk ^ ((row>>2)&3)) so that ds_read_b128 of one chunk per lane is bank-conflict free.
// MFMA k-permutation: lanes 0-31 read chunk 2g, lanes 32-63 chunk 2g+1 of their row; MFMA e of
// group g then contracts k = {8g+e, 8g+4+e}; both operands use the same convention, so any
// permutation of k is legal.  8 ds_read_b128 per wave per k-tile instead of 32 ds_read_b32.
// ======================================================================================
template <int S>
__global__ void __launch_bounds__(256, 4)
pw_gemm_wgrad_dma_kernel(GemmArgs g) {
  extern __shared__ __attribute__((aligned(16))) float lds[];  // [S][A|B][128*16]
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
  const int KT = g.K / DBK;
  const int64_t total = (int64_t)g.inner * KT;
  const int t_begin = (int)(total * bz / g.nbatch);
  const int T = (int)(total * (bz + 1) / g.nbatch) - t_begin;

  // DMA lane mapping inside a 16-row piece: row = lane>>2, LDS slot = lane&3, source chunk swizzled
  const int prow = lane >> 2, pslot = lane & 3;
  const int chunk = pslot ^ ((prow >> 2) & 3);
  const int ra0 = min(m0 + 16 * (2 * wave) + prow, g.M - 1), ra1 = min(m0 + 16 * (2 * wave + 1) + prow, g.M - 1);
  const int rb0 = min(n0 + 16 * (2 * wave) + prow, g.N - 1), rb1 = min(n0 + 16 * (2 * wave + 1) + prow, g.N - 1);
  const float* pa0 = g.A + (int64_t)ra0 * g.lda + 4 * chunk;
  const float* pa1 = g.A + (int64_t)ra1 * g.lda + 4 * chunk;
  const float* pb0 = g.B + (int64_t)rb0 * g.ldb + 4 * chunk;
  const float* pb1 = g.B + (int64_t)rb1 * g.ldb + 4 * chunk;

  auto issue = [&](int t) {
    const int tt = t_begin + t;
    const int ib = tt / KT, kt = tt - ib * KT;
    const int64_t oa = (int64_t)ib * g.a_is + (int64_t)kt * DBK, ob = (int64_t)ib * g.b_is + (int64_t)kt * DBK;
    float* st = lds + (t % S) * (2 * DTILE);
    float* la = st + (2 * wave) * 256;
    float* lb = st + DTILE + (2 * wave) * 256;
    __builtin_amdgcn_global_load_lds((gbl_ptr_t)(pa0 + oa), (lds_ptr_t)la, 16, 0, 0);
    __builtin_amdgcn_global_load_lds((gbl_ptr_t)(pa1 + oa), (lds_ptr_t)(la + 256), 16, 0, 0);
    __builtin_amdgcn_global_load_lds((gbl_ptr_t)(pb0 + ob), (lds_ptr_t)lb, 16, 0, 0);
    __builtin_amdgcn_global_load_lds((gbl_ptr_t)(pb1 + ob), (lds_ptr_t)(lb + 256), 16, 0, 0);
  };

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

#pragma unroll
  for (int t = 0; t < S - 1; ++t)
    if (t < T) issue(t);

  // bias gradient for free: the n-tile-0 workgroups also sum their A rows (dZ) over k.
  // thread t covers row t>>1, 16-B slots 2*(t&1), 2*(t&1)+1 (any chunk order: it is a plain sum)
  const bool do_rowsum = g.rowsum != nullptr && nt == 0;
  float rs = 0.f;
  const int rs_off = (tid >> 1) * DBK + (tid & 1) * 8;

  // fragment addressing: row r = w?*64 + t?*32 + li, slot = (2g+lh) ^ ((li>>2)&3)
  const int sw = (li >> 2) & 3;
  const int offA = (wm * 64 + li) * DBK, offB = DTILE + (wn * 64 + li) * DBK;
  const int s0 = ((0 + lh) ^ sw) * 4, s1 = ((2 + lh) ^ sw) * 4;

  for (int t = 0; t < T; ++t) {
    const int pending = min(S - 2, T - 1 - t);
    if (pending >= 2) asm volatile("s_waitcnt vmcnt(8)\n\ts_barrier" ::: "memory");
    else if (pending == 1) asm volatile("s_waitcnt vmcnt(4)\n\ts_barrier" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
    if (t + S - 1 < T) issue(t + S - 1);
    const float* st = lds + (t % S) * (2 * DTILE);
    if (do_rowsum) {
      const float4 q0 = *reinterpret_cast<const float4*>(st + rs_off);
      const float4 q1 = *reinterpret_cast<const float4*>(st + rs_off + 4);
      rs += ((q0.x + q0.y) + (q0.z + q0.w)) + ((q1.x + q1.y) + (q1.z + q1.w));
    }
    const float4 a00 = *reinterpret_cast<const float4*>(st + offA + s0);
    const float4 a10 = *reinterpret_cast<const float4*>(st + offA + 32 * DBK + s0);
    const float4 b00 = *reinterpret_cast<const float4*>(st + offB + s0);
    const float4 b10 = *reinterpret_cast<const float4*>(st + offB + 32 * DBK + s0);
    const float4 a01 = *reinterpret_cast<const float4*>(st + offA + s1);
    const float4 a11 = *reinterpret_cast<const float4*>(st + offA + 32 * DBK + s1);
    const float4 b01 = *reinterpret_cast<const float4*>(st + offB + s1);
    const float4 b11 = *reinterpret_cast<const float4*>(st + offB + 32 * DBK + s1);
#define MFMA4(A0, A1, B0, B1)                                                       \
    acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(A0, B0, acc[0][0], 0, 0, 0);   \
    acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(A0, B1, acc[0][1], 0, 0, 0);   \
    acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(A1, B0, acc[1][0], 0, 0, 0);   \
    acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(A1, B1, acc[1][1], 0, 0, 0);
    MFMA4(a00.x, a10.x, b00.x, b10.x)
    MFMA4(a00.y, a10.y, b00.y, b10.y)
    MFMA4(a00.z, a10.z, b00.z, b10.z)
    MFMA4(a00.w, a10.w, b00.w, b10.w)
    MFMA4(a01.x, a11.x, b01.x, b11.x)
    MFMA4(a01.y, a11.y, b01.y, b11.y)
    MFMA4(a01.z, a11.z, b01.z, b11.z)
    MFMA4(a01.w, a11.w, b01.w, b11.w)
#undef MFMA4
  }
  if (do_rowsum) {
    rs += __shfl_xor(rs, 1, 64);
    const int m = m0 + (tid >> 1);
    if ((tid & 1) == 0 && m < g.M) g.rowsum[(int64_t)bz * g.M + m] = rs;
  }
  gemm_epilogue(g, acc, bz, m0, n0, wm, wn, li, lh);
}

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
template <int NSUB, int NP = 2>
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
  const int mt = L % MT, nt2 = (L / MT) % NT2, bz = L / (MT * NT2);
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
  float xb[2][8] = {};     // defined values: the surplus split of the last tile reads a set that was never loaded
  auto issueA = [&](int t) __attribute__((always_inline)) {
    if (doA)
      __builtin_amdgcn_global_load_lds((gbl_ptr_t)(Ag + (int64_t)t * SIMG), (lds_ptr_t)(img + (2 * NSUB + t % SA) * SIMG + wave * 64), 16, 0, 0);
    if (doA2)
      __builtin_amdgcn_global_load_lds((gbl_ptr_t)(Ag + (int64_t)t * SIMG + 512), (lds_ptr_t)(img + (2 * NSUB + t % SA) * SIMG + 512 + wave * 64), 16, 0, 0);
  };
  auto split_store = [&](const float (&x)[8], u32x4* o) __attribute__((always_inline)) {
    if constexpr (NP == 3) {
      u32x4 h, m, l;
      // sign checkerboard: odd 64-column blocks are staged negated.  (Two code paths behind a wave-uniform branch
      // with the sign folded into source modifiers - no v_xor - measured SLOWER, 154.8 against 153.0 ms per step: the
      // branch takes the split out of the MFMA block's schedule.)
      float xs[8];
      flip8(xs, x, flip);
      split8(xs, h, m, l);
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
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  for (int u = 0; u < DA && u < T; ++u) issueA(u);
  fetchB(0, xb[0]);
  USE_X(xb[0], 0);
  if (T > 1) fetchB(1, xb[1]);
  split_store(xb[0], Bst);
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
      if (sub == 1) split_store(xsplit, Bst + (cur ^ 1) * SIMG);
      __builtin_amdgcn_sched_barrier(0);
      mfma_block();
      __builtin_amdgcn_sched_barrier(0);
      if (sub == 0) split_store(xsplit, Bst + (cur ^ 1) * SIMG);
#else
      mfma_block();
      split_store(xsplit, Bst + (cur ^ 1) * SIMG);
#endif
      // (no sched_group_barrier pinning here: the 1 MFMA : 3 VALU pattern of the 128 x 128 kernel measured 0.7 % slower
      //  on the step than the compiler's own order, three rounds on one box)
    } else {
      SplitFrags<NP> f;
      split_tile_read<NP, 2 * SCH, 2 * SCH>(As, Bs, f);
      split_tile_mfma<NP>(f, acc);
      split_store(xsplit, Bst + (cur ^ 1) * SIMG);
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
#undef USE_X
  if (live) {
    split_unflip(acc, wn);
    if constexpr (NP == 2) split_unscale(acc, inv_a, inv_b);
    gemm_epilogue(g, acc, bz, m0, n0, wm, wn, li, lh);
  }
}

// (A 256 x 256 workgroup tile for the six-product kernel - sixteen waves, TWO copies of the arrangement above sharing the
//  STAGED activation tiles, so that a 16 x 256 fp32 tile is fetched from L2 and split into its bf16 planes once per 256 output
//  rows: 40 instead of 56 KB through L2 per 256 x 256 x 16 and half the split arithmetic per MFMA; the copies take turns
//  fetching / splitting; 96 KB of LDS, one 1024-thread workgroup per CU; bit-identical results - was built in round 6
//  (`pw_gemm_split_quad_kernel`; the structure is all that is recorded) and measured on the training step: 156.2 / 157.0 against 154.8 / 155.0 ms,
//  same box.  Fewer L2 bytes and fewer VALU operations per MFMA buy nothing: what bounds these kernels is the matrix pipe
//  under the chip's power budget (busy x clock), as the yardstick of DESIGN.md 4.1 says.  Removed; profiles/r06_gemm_quad.txt.)

// out[i] = slabs[0][i] + slabs[1][i] + ... in that order; vec: n % 4 == 0 and 16-byte aligned pointers (four
// elements per thread, four slabs' loads in flight)
__global__ void __launch_bounds__(256)
slab_reduce_kernel(const float* __restrict__ slabs, float* __restrict__ out, int64_t n, int S, int vec,
                   const float* __restrict__ slabs2, float* __restrict__ out2, int n2, int blocks1) {
  // second, small reduction riding in the same launch (the bias gradient's row sums next to the weight gradient's
  // slabs: 131 launches per training step less): blocks [blocks1, gridDim.x)
  if ((int)blockIdx.x >= blocks1) {
    const int i = ((int)blockIdx.x - blocks1) * 256 + threadIdx.x;
    if (i < n2) {
      float t = 0.f;
      for (int k = 0; k < S; ++k) t += slabs2[(int64_t)k * n2 + i];
      out2[i] = t;
    }
    return;
  }
  const int nblk = blocks1;      // (the grid-stride loops below run over the first `blocks1` blocks)
  if (vec) {
    const int64_t n4 = n >> 2;
    const float4* sl = reinterpret_cast<const float4*>(slabs);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)nblk * 256) {
      float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
      int k = 0;
      for (; k + 4 <= S; k += 4) {
        float4 q[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) q[j] = sl[(int64_t)(k + j) * n4 + i];
#pragma unroll
        for (int j = 0; j < 4; ++j) { s.x += q[j].x; s.y += q[j].y; s.z += q[j].z; s.w += q[j].w; }
      }
      for (; k < S; ++k) {
        const float4 q = sl[(int64_t)k * n4 + i];
        s.x += q.x; s.y += q.y; s.z += q.z; s.w += q.w;
      }
      reinterpret_cast<float4*>(out)[i] = s;
    }
    return;
  }
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)nblk * 256) {
    float s = 0.f;
    for (int k = 0; k < S; ++k) s += slabs[(int64_t)k * n + i];
    out[i] = s;
  }
}

int slots() { return 256 * g_wg_per_cu; }

// both operands p-contiguous with whole, 16-B aligned 16-float chunks (LDS-DMA and split kernels)
bool wgrad_vec_layout(int N, int64_t dy_bs, int64_t x_bs, const void* a, const void* b) {
  auto a16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
  return N % DBK == 0 && (dy_bs & 3) == 0 && (x_bs & 3) == 0 && a16(a) && a16(b);
}
bool wgrad_dma_ok(int N, int64_t dy_bs, int64_t x_bs, const void* a, const void* b) {
  return g_wgrad_dma_stages >= 2 && wgrad_vec_layout(N, dy_bs, x_bs, a, b);
}

// number of k-range splits: one round of resident workgroups over the CUs
int wgrad_splits(int B, int M, int K, int N, int bk, int wg_per_cu) {
  const int tiles = ((M + BM - 1) / BM) * ((K + BN - 1) / BN);
  const int64_t total_kt = (int64_t)B * ((N + bk - 1) / bk);
  int s = (int)std::max<int64_t>(1, std::min<int64_t>(256 * wg_per_cu / tiles, total_kt));
  // the split kernels accumulate alternate slabs with opposite sign so that the bf16 MFMA's alignment offset cancels
  // in the slab sum ("sign checkerboard"): that takes an even number of slabs (1536 x 384: 21 -> 20; round 5)
  if (s > 1) s &= ~1;
  return s;
}
int wgrad_dma_wgs() { return g_wgrad_dma_stages == 2 ? 4 : 3; }
// bf16-mixed scheme: the 256 x 128 kernel where the taller tile wastes at most ~1/7 of its rows (PARADIS_WGRAD_TALL=0: off)
bool wgrad_tall_ok(int M) {
  static const bool on = [] { const char* e = getenv("PARADIS_WGRAD_TALL"); return !(e && e[0] == '0'); }();
  return on && M >= 256 && ((M + 255) / 256) * 256 * 7 <= M * 8;
}
bool wgrad_square_on() {
  static const bool on = [] { const char* e = getenv("PARADIS_WGRAD_SQUARE"); return !(e && e[0] == '0'); }();
  return on;
}
int wgrad_splits_square(int B, int M, int K, int N) {
  const int tiles = ((M + 255) / 256) * ((K + 255) / 256);
  const int64_t total_kt = (int64_t)B * ((N + SBK - 1) / SBK);
  int s = (int)std::max<int64_t>(1, std::min<int64_t>(256 / tiles, total_kt));
  if (s > 1) s &= ~1;
  return s;
}
int wgrad_splits_tall(int B, int M, int K, int N) {
  const int tiles = ((M + 255) / 256) * ((K + BN - 1) / BN);
  const int64_t total_kt = (int64_t)B * ((N + SBK - 1) / SBK);
  int s = (int)std::max<int64_t>(1, std::min<int64_t>(512 / tiles, total_kt));
  if (s > 1) s &= ~1;
  return s;
}

template <bool A_KC, bool B_KC, int BK>
int launch_gemm_bk(const GemmArgs& g, int grid, hipStream_t st) {
  // the dynamic-LDS request doubles as the occupancy control: 160 KiB / request = workgroups per CU
  size_t request = std::max(lds_bytes(BK), (size_t)(160 * 1024 / g_wg_per_cu) & ~(size_t)255);
  request = std::min(request, (size_t)160 * 1024);
  static PerDeviceOnce once;
  if (int e = reserve_lds(once, {&pw_gemm_kernel<A_KC, B_KC, BK>}, 160 * 1024, "pw_gemm")) return e;
  hipLaunchKernelGGL((pw_gemm_kernel<A_KC, B_KC, BK>), dim3(grid), dim3(256), request, st, g);
  return 0;
}

bool dma_eligible(const GemmArgs& g) {
  auto a16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
  return g_dma_stages >= 2 && g.inner == 0 && g.K % DBK == 0 && g.M % 4 == 0 && g.N % 4 == 0 &&
         g.M >= 4 && g.N >= 4 && (g.lda & 3) == 0 && (g.ldb & 3) == 0 && (g.a_bs & 3) == 0 &&
         (g.b_bs & 3) == 0 && a16(g.A) && a16(g.B);
}

int launch_gemm_dma(const GemmArgs& g, int grid, hipStream_t st) {
  const size_t bytes = (size_t)g_dma_stages * 2 * DTILE * sizeof(float);
  switch (g_dma_stages) {
    case 2: hipLaunchKernelGGL((pw_gemm_dma_kernel<2, 4>), dim3(grid), dim3(256), bytes, st, g); break;
    case 3: hipLaunchKernelGGL((pw_gemm_dma_kernel<3, 3>), dim3(grid), dim3(256), bytes, st, g); break;
    default: hipLaunchKernelGGL((pw_gemm_dma_kernel<4, 2>), dim3(grid), dim3(256), (size_t)4 * 2 * DTILE * sizeof(float), st, g); break;
  }
  return 0;
}

template <bool A_KC, bool B_KC>
int launch_gemm(const GemmArgs& g, int grid, hipStream_t st) {
  return g_bk == 32 ? launch_gemm_bk<A_KC, B_KC, 32>(g, grid, st)
                    : launch_gemm_bk<A_KC, B_KC, 16>(g, grid, st);
}

constexpr size_t split_lds(int np) { return (size_t)(2 + split_astages(np)) * simg(np) * 16; }
constexpr size_t split_lds_wgrad(int np) { return (size_t)2 * 2 * simgp(np) * 16; }
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

bool known_scheme(int scheme) {
  return scheme == PARADIS_GEMM_EXACT || scheme == PARADIS_GEMM_BF16X3 || scheme == PARADIS_GEMM_F16X2 ||
         scheme == PARADIS_GEMM_BF16;
}

int launch_amax(const float* x, int B, int64_t inner, int64_t bs, uint32_t* out, hipStream_t st) {
  const int vec = (inner % 4 == 0) && (bs % 4 == 0) && ((reinterpret_cast<uintptr_t>(x) & 15) == 0);
  hipLaunchKernelGGL(amax_partials_kernel, dim3(AMAX_WORDS), dim3(256), 0, st, x, B, inner, bs, vec, out);
  return 0;
}

template <int NP>
int launch_split_np(const GemmArgs& d, hipStream_t st) {
  const int grid = ((d.M + BM - 1) / BM) * ((d.N + BN - 1) / BN) * d.nbatch;
  static PerDeviceOnce once;
  if (split_lds(NP) > 64 * 1024)
    if (int e = reserve_lds(once, {&pw_gemm_split_kernel<NP>}, split_lds(NP), "pw_gemm(split)")) return e;
  hipLaunchKernelGGL(pw_gemm_split_kernel<NP>, dim3(grid), dim3(256), split_lds(NP), st, d);
  return 0;
}
constexpr size_t split_wide_lds(int nsub, int np = 2) { return (size_t)(2 * nsub + 2) * simg(np) * 16; }   // f16x2: 48 KiB, bf16x3: 72 KiB
// n-tiles per workgroup: 2 (two 8-wave workgroups per CU).  4 - one 16-wave workgroup per CU, another 17 % fewer
// bytes - measured 2.5 % SLOWER: a single workgroup's waves all stop at the same barriers.
constexpr int SPLIT_WIDE_NSUB = 2;
// scheme: PARADIS_GEMM_BF16X3 or PARADIS_GEMM_F16X2 (the latter with d.a_amax / d.b_amax set)
// bf16x3 on the 128 x 256 tile (round 3).  With all twelve fragments of a k-tile live (the 128 x 128 kernel's way) the
// kernel needs ~150 registers and hipcc spills 1.2 KB per lane at the 128 that two 8-wave workgroups per CU allow;
// reading the B fragments one PLANE at a time (8 instead of 24 registers, planes in the order l, m, h) brings it to
// 128 registers and 12 bytes of scratch.  Training step 160.0 -> 156.3 ms, GEMMs 188 -> 194 TF (same box, two rounds).
#ifndef SPLIT_WIDE_BF16X3      // (0: the 128 x 128 kernel for every shape; A/B builds)
#define SPLIT_WIDE_BF16X3 1
#endif
template <int NP>
int launch_split_wide(const GemmArgs& d, int NT, hipStream_t st) {
  constexpr int NSUB = SPLIT_WIDE_NSUB;
  static PerDeviceOnce once;
  if (split_wide_lds(NSUB, NP) > 64 * 1024)
    if (int e = reserve_lds(once, {&pw_gemm_split_wide_kernel<NSUB, NP>}, split_wide_lds(NSUB, NP), "pw_gemm(split)")) return e;
  const int grid = ((d.M + BM - 1) / BM) * ((NT + NSUB - 1) / NSUB) * d.nbatch;     // 128 x (128 NSUB) tiles
  hipLaunchKernelGGL((pw_gemm_split_wide_kernel<NSUB, NP>), dim3(grid), dim3(256 * NSUB), split_wide_lds(NSUB, NP), st, d);
  return 0;
}
int launch_split(const GemmArgs& d, int scheme, hipStream_t st) {
  const int NT = (d.N + BN - 1) / BN;
  if (scheme == PARADIS_GEMM_BF16) return pd_amp_launch_fwd(d, st);      // (gemm_amp_fwd.hip)
  if (scheme != PARADIS_GEMM_F16X2) {
#if SPLIT_WIDE_BF16X3
    if (NT >= 2) return launch_split_wide<3>(d, NT, st);
#endif
    return launch_split_np<3>(d, st);
  }
  if (NT < 2) return launch_split_np<2>(d, st);
  return launch_split_wide<2>(d, NT, st);
}

int check_gemm(const char* name, int B, int M, int K, int N) {
  PD_REQUIRE(B >= 0 && M >= 1 && K >= 1 && N >= 1, "%s: bad shape B=%d M=%d K=%d N=%d", name, B, M, K, N);
  const int64_t tiles = (int64_t)((M + BM - 1) / BM) * ((N + BN - 1) / BN) * std::max(B, 1);
  PD_REQUIRE(tiles < (1ll << 31), "%s: too many tiles", name);
  return 0;
}

}  // namespace

#ifdef PARADIS_DEV_KNOBS
// diagnostic knobs of the development build only (`make dev`, tools/gemm_bench.py); the shipped
// library exports none of them.  bk in {16,32}, wg_per_cu in 1..4
extern "C" void paradis_debug_set_gemm(int bk, int wg_per_cu) {
  if (bk == 16 || bk == 32) g_bk = bk;
  if (wg_per_cu >= 1 && wg_per_cu <= 4) g_wg_per_cu = wg_per_cu;
}
extern "C" void paradis_debug_set_gemm_stagger(int units) { g_stagger = units < 0 ? 0 : units; }
extern "C" void paradis_debug_set_gemm_dma(int stages) { g_dma_stages = stages < 2 ? 0 : (stages > 4 ? 4 : stages); }
extern "C" void paradis_debug_set_wgrad_dma(int stages) { g_wgrad_dma_stages = stages < 2 ? 0 : (stages > 3 ? 3 : stages); }
#endif

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

namespace {
// A = split image at `img` of an [AM, AK] matrix; F16X2 needs the activations' amax partials
int run_split(GemmArgs d, const void* img, int AM, int AK, int scheme, const uint32_t* b_amax, const char* what,
              hipStream_t st) {
  d.A = (const float*)img; d.a_bs = 0;
  if (scheme == PARADIS_GEMM_F16X2) {
    if (b_amax == nullptr) { paradis_set_error(what); return 1; }
    d.a_amax = reinterpret_cast<const uint32_t*>((const char*)img + (size_t)split_image_chunks(AM, AK, 2) * 16);
    d.b_amax = b_amax;
  }
  return launch_split(d, scheme, st);
}
// bf16-stored tensors exist in the bf16-mixed scheme only; the DMA'd activation operand needs whole 16-byte chunks
int check_io16(const char* name, int io16, int scheme, const void* Bop, int64_t b_bs, int N, bool has_res) {
  if (io16 == 0) return 0;
  PD_REQUIRE(scheme == PARADIS_GEMM_BF16, "%s: bf16-stored tensors need the PARADIS_GEMM_BF16 scheme", name);
  PD_REQUIRE((io16 & ~(IO_B16 | IO_C16 | IO_ZM16 | IO_A16)) == 0, "%s: unknown io16 bits %d", name, io16);
  PD_REQUIRE(!(io16 & IO_C16) || !has_res, "%s: a bf16 output cannot carry the fp32 residual", name);
  if (io16 & IO_B16)
    PD_REQUIRE(N % 8 == 0 && N >= 8 && b_bs % 8 == 0 && (reinterpret_cast<uintptr_t>(Bop) & 15) == 0,
               "%s: a bf16 activation operand needs N %% 8 == 0 and 16-byte aligned planes", name);
  return 0;
}
}  // namespace

static int pw_gemm_fwd_impl(const float* Wt, const float* WtT, const void* Wsplit, int scheme,
                            const uint32_t* x_amax, const float* X,
                            const float* bias, const float* map, const float* m8,
                            const float* pwT, int cin, const float* res, const float* gate, float* Y, float* zpre,
                            int B, int M, int K, int N, int64_t x_bs, int64_t res_bs,
                            int64_t y_bs, int act, void* stream, int io16 = 0) {
  if (int e = check_gemm("pw_gemm_fwd", B, M, K, N)) return e;
  if (int e = check_io16("pw_gemm_fwd", io16, scheme, X, x_bs, N, res != nullptr)) return e;
  PD_REQUIRE(gate == nullptr || res != nullptr || B == 0, "pw_gemm_fwd: a gate needs the tensor it blends with (res)");
  PD_REQUIRE(act >= 0 && act <= 2, "pw_gemm_fwd: unknown activation code %d", act);
  PD_REQUIRE(known_scheme(scheme) && (Wsplit != nullptr) == (scheme != PARADIS_GEMM_EXACT),
             "pw_gemm_fwd: scheme %d needs %s weight image", scheme, scheme ? "a" : "no");
  PD_REQUIRE((m8 == nullptr) == (pwT == nullptr) && (pwT == nullptr || (cin >= 1 && M % 4 == 0)),
             "pw_gemm_fwd: projected bias needs m8, pwT, cin >= 1 and M %% 4 == 0");
  if (B == 0) return 0;
  GemmArgs g{};
  g.m8 = m8; g.pw = pwT; g.cin = cin;
  g.A = Wt; g.B = X; g.C = Y; g.M = M; g.N = N; g.K = K;
  g.lda = K; g.ldb = N; g.ldc = N;
  g.a_bs = 0; g.b_bs = x_bs; g.c_bs = y_bs; g.nbatch = B; g.inner = 0;
  g.bias = bias; g.map = map; g.res = res; g.res_bs = res_bs; g.zmul = nullptr; g.zout = zpre;
  g.zout_bs = (int64_t)M * N; g.act = act; g.gate = gate;
  g.stagger = g_stagger;
  g.io16 = io16;
  const int grid = ((M + BM - 1) / BM) * ((N + BN - 1) / BN) * B;
  if (Wsplit != nullptr) {   // split image of the weights: split kernel (any shape)
    if (int e = run_split(g, Wsplit, M, K, scheme, x_amax, "pw_gemm_fwd: the f16x2 scheme needs x_amax",
                          (hipStream_t)stream)) return e;
    PD_CHECK_LAUNCH("pw_gemm_fwd(split)");
    return 0;
  }
  if (WtT != nullptr) {   // weights also supplied as [K,M]: row-contiguous A operand -> LDS-DMA kernel
    GemmArgs d = g;
    d.A = WtT; d.lda = M;
    if (dma_eligible(d)) {
      launch_gemm_dma(d, grid, (hipStream_t)stream);
      PD_CHECK_LAUNCH("pw_gemm_fwd(dma)");
      return 0;
    }
  }
  if (int e = launch_gemm<true, false>(g, grid, (hipStream_t)stream)) return e;
  PD_CHECK_LAUNCH("pw_gemm_fwd");
  return 0;
}

extern "C" int paradis_pw_gemm_fwd(const float* Wt, const float* WtT, const void* Wsplit, int scheme,
                                   const uint32_t* x_amax, const float* X,
                                   const float* bias, const float* map, const float* m8,
                                   const float* pwT, int cin, const float* res, float* Y, float* zpre,
                                   int B, int M, int K, int N, int64_t x_bs, int64_t res_bs,
                                   int64_t y_bs, int act, void* stream) {
  return pw_gemm_fwd_impl(Wt, WtT, Wsplit, scheme, x_amax, X, bias, map, m8, pwT, cin, res, nullptr, Y, zpre, B, M, K, N,
                          x_bs, res_bs, y_bs, act, stream);
}

// Y = res + sigmoid(gate[m]) (act(W X + ...) - res): the gated blend of the advected field with the field it was
// advected from (reference model/paradis.py:239-243) inside the epilogue of the up-projection's last layer - the
// advected tensor is never written.  Same bits as paradis_pw_gemm_fwd followed by paradis_gated_blend_fwd.
extern "C" int paradis_pw_gemm_fwd_gated(const float* Wt, const float* WtT, const void* Wsplit, int scheme,
                                         const uint32_t* x_amax, const float* X,
                                         const float* bias, const float* map, const float* m8,
                                         const float* pwT, int cin, const float* res, const float* gate, float* Y,
                                         float* zpre, int B, int M, int K, int N, int64_t x_bs, int64_t res_bs,
                                         int64_t y_bs, int act, void* stream) {
  PD_REQUIRE(gate != nullptr && (res != nullptr || B == 0), "pw_gemm_fwd_gated: gate [M] and res required");
  return pw_gemm_fwd_impl(Wt, WtT, Wsplit, scheme, x_amax, X, bias, map, m8, pwT, cin, res, gate, Y, zpre, B, M, K, N,
                          x_bs, res_bs, y_bs, act, stream);
}

// PARADIS_GEMM_BF16 with bf16-STORED tensors (round 6): io16 = PARADIS_IO_X16 (X is bf16 [B][K,N]) | PARADIS_IO_Y16 (Y and
// zpre are written as bf16; no residual then).  Everything else as paradis_pw_gemm_fwd / _gated (gate may be NULL).
extern "C" int paradis_pw_gemm_fwd16(const void* Wsplit, const void* X, const float* bias, const float* map,
                                     const float* m8, const float* pwT, int cin, const float* res, const float* gate,
                                     void* Y, void* zpre, int B, int M, int K, int N, int64_t x_bs, int64_t res_bs,
                                     int64_t y_bs, int act, int io16, void* stream) {
  PD_REQUIRE((io16 & ~(IO_B16 | IO_C16)) == 0, "pw_gemm_fwd16: io16 may name X (1) and Y (2)");
  PD_REQUIRE(Wsplit != nullptr, "pw_gemm_fwd16: weight image required");
  return pw_gemm_fwd_impl(nullptr, nullptr, Wsplit, PARADIS_GEMM_BF16, nullptr, (const float*)X, bias, map, m8, pwT, cin,
                          res, gate, (float*)Y, (float*)zpre, B, M, K, N, x_bs, res_bs, y_bs, act, stream, io16);
}

// Plain batched GEMM  C_b[M,N] = A_b[M,K] B_b[K,N]  (row-major, batch strides in elements) on the same
// kernels; AT (optional) = the [K,M] transposes of A_b with batch stride at_bs, which lets the LDS-DMA
// kernel run; split_ws (optional, nbatch * paradis_pw_gemm_split_bytes(M,K) bytes) selects the bf16-split
// arithmetic instead (the A matrices are split into it first).  Used by the Newton-Schulz iteration of the Muon step (muon.hip): same-shape weight
// matrices are stacked so that one launch fills the chip (a single 896^3 product is 49 tiles).
extern "C" int paradis_bgemm(const float* A, const float* AT, const float* Bm, float* C, int nbatch, int M,
                             int K, int N, int64_t a_bs, int64_t at_bs, int64_t b_bs, int64_t c_bs,
                             void* split_ws, void* stream) {
  PD_REQUIRE(nbatch >= 0 && M >= 1 && K >= 1 && N >= 1, "bgemm: bad shape");
  if (nbatch == 0) return 0;
  GemmArgs g{};
  g.A = A; g.B = Bm; g.C = C; g.M = M; g.N = N; g.K = K;
  g.lda = K; g.ldb = N; g.ldc = N;
  g.a_bs = a_bs; g.b_bs = b_bs; g.c_bs = c_bs; g.nbatch = nbatch; g.inner = 0;
  g.stagger = g_stagger;
  const int64_t tiles = (int64_t)((M + BM - 1) / BM) * ((N + BN - 1) / BN) * nbatch;
  PD_REQUIRE(tiles < (1ll << 31), "bgemm: too many tiles");
  const int grid = (int)tiles;
  if (split_ws != nullptr) {   // bf16-split path: images of the nbatch A matrices in split_ws
    PD_REQUIRE(nbatch <= 65535, "bgemm: too many batches for the split path");
    const int KT = (K + SBK - 1) / SBK;
    const int64_t chunks = split_image_chunks(M, K), units = (int64_t)((M + BM - 1) / BM) * KT * 256;
    const int blocks = (int)std::min<int64_t>((units + 255) / 256, 1024);
    hipLaunchKernelGGL(split_weights_kernel<3>, dim3(blocks, nbatch), dim3(256), 0, (hipStream_t)stream, A,
                       (int64_t)K, (int64_t)1, M, K, KT, units, a_bs, chunks, (u32x4*)split_ws);
    GemmArgs d = g;
    d.A = (const float*)split_ws; d.a_bs = chunks;
    if (int e = launch_split(d, PARADIS_GEMM_BF16X3, (hipStream_t)stream)) return e;
    PD_CHECK_LAUNCH("bgemm(split)");
    return 0;
  }
  if (AT != nullptr) {
    GemmArgs d = g;
    d.A = AT; d.lda = M; d.a_bs = at_bs;
    if (dma_eligible(d)) {
      launch_gemm_dma(d, grid, (hipStream_t)stream);
      PD_CHECK_LAUNCH("bgemm(dma)");
      return 0;
    }
  }
  if (int e = launch_gemm<true, false>(g, grid, (hipStream_t)stream)) return e;
  PD_CHECK_LAUNCH("bgemm");
  return 0;
}

static int pw_gemm_dgrad_impl(const float* Wt, const void* WTsplit, int scheme, const uint32_t* dy_amax,
                              const float* dY, const float* zpre,
                              const float* addend, float* dX, int B, int M, int K, int N,
                              int64_t dy_bs, int64_t z_bs, int64_t add_bs, int64_t dx_bs,
                              int act, void* stream, int io16) {
  // W is [M,K] (M = Co, K = Ci); result dX is [K,N] per sample: GEMM with M' = K, K' = M.
  if (int e = check_gemm("pw_gemm_dgrad", B, K, M, N)) return e;
  if (int e = check_io16("pw_gemm_dgrad", io16, scheme, dY, dy_bs, N, addend != nullptr)) return e;
  PD_REQUIRE(act >= 0 && act <= 2, "pw_gemm_dgrad: unknown activation code %d", act);
  PD_REQUIRE(known_scheme(scheme) && (WTsplit != nullptr) == (scheme != PARADIS_GEMM_EXACT),
             "pw_gemm_dgrad: scheme %d needs %s weight image", scheme, scheme ? "a" : "no");
  if (B == 0) return 0;
  GemmArgs g{};
  g.A = Wt; g.B = dY; g.C = dX; g.M = K; g.N = N; g.K = M;
  g.lda = K; g.ldb = N; g.ldc = N;
  g.a_bs = 0; g.b_bs = dy_bs; g.c_bs = dx_bs; g.nbatch = B; g.inner = 0;
  g.res = addend; g.res_bs = add_bs; g.zmul = zpre; g.zmul_bs = z_bs; g.act = zpre ? act : 0;
  g.stagger = g_stagger;
  g.io16 = io16;
  const int grid = ((K + BM - 1) / BM) * ((N + BN - 1) / BN) * B;
  if (WTsplit != nullptr) {   // split image of W^T
    if (int e = run_split(g, WTsplit, K, M, scheme, dy_amax, "pw_gemm_dgrad: the f16x2 scheme needs dy_amax",
                          (hipStream_t)stream)) return e;
    PD_CHECK_LAUNCH("pw_gemm_dgrad(split)");
    return 0;
  }
  if (dma_eligible(g)) {
    launch_gemm_dma(g, grid, (hipStream_t)stream);
    PD_CHECK_LAUNCH("pw_gemm_dgrad(dma)");
    return 0;
  }
  if (int e = launch_gemm<false, false>(g, grid, (hipStream_t)stream)) return e;
  PD_CHECK_LAUNCH("pw_gemm_dgrad");
  return 0;
}

extern "C" int paradis_pw_gemm_dgrad(const float* Wt, const void* WTsplit, int scheme, const uint32_t* dy_amax,
                                     const float* dY, const float* zpre,
                                     const float* addend, float* dX, int B, int M, int K, int N,
                                     int64_t dy_bs, int64_t z_bs, int64_t add_bs, int64_t dx_bs,
                                     int act, void* stream) {
  return pw_gemm_dgrad_impl(Wt, WTsplit, scheme, dy_amax, dY, zpre, addend, dX, B, M, K, N, dy_bs, z_bs, add_bs, dx_bs,
                            act, stream, 0);
}

// PARADIS_GEMM_BF16 with bf16-STORED tensors: io16 = PARADIS_IO_X16 (dY is bf16) | PARADIS_IO_Y16 (dX is written as bf16)
// | PARADIS_IO_Z16 (zpre is bf16).
extern "C" int paradis_pw_gemm_dgrad16(const void* WTsplit, const void* dY, const void* zpre, void* dX, int B, int M,
                                       int K, int N, int64_t dy_bs, int64_t z_bs, int64_t dx_bs, int act, int io16,
                                       void* stream) {
  PD_REQUIRE((io16 & ~(IO_B16 | IO_C16 | IO_ZM16)) == 0, "pw_gemm_dgrad16: io16 may name dY (1), dX (2) and zpre (4)");
  PD_REQUIRE(WTsplit != nullptr, "pw_gemm_dgrad16: weight image required");
  return pw_gemm_dgrad_impl(nullptr, WTsplit, PARADIS_GEMM_BF16, nullptr, (const float*)dY, (const float*)zpre, nullptr,
                            (float*)dX, B, M, K, N, dy_bs, z_bs, 0, dx_bs, act, stream, io16);
}

extern "C" size_t paradis_pw_gemm_wgrad_ws_bytes(int B, int M, int K, int N) {
  const int b = std::max(B, 1);
  const int S = std::max({wgrad_splits(b, M, K, N, DBK, wgrad_dma_wgs()), wgrad_splits(b, M, K, N, g_bk, g_wg_per_cu),
                          wgrad_splits(b, M, K, N, SBK, 3), wgrad_splits_tall(b, M, K, N),
                          wgrad_splits_square(b, M, K, N)});
  return (size_t)S * M * ((size_t)K + 1) * sizeof(float) + 256;   // slabs + row-sum partials
}

// K-range slabs the split weight-gradient kernel runs for this shape (1, or an even number: see wgrad_splits)
extern "C" int paradis_pw_gemm_wgrad_slabs(int B, int M, int K, int N) {
  if (M < 1 || K < 1 || N < 1) return 0;
  return wgrad_splits(std::max(B, 1), M, K, N, SBK, 3);
}

extern "C" int paradis_bias_grads(const float* dz, float* gmap, float* gbias, int B, int C, int P,
                                  int64_t dz_bs, void* stream);

static int pw_gemm_wgrad_impl(const float* dY, const float* X, float* dW, float* gbias, int B,
                              int M, int K, int N, int64_t dy_bs, int64_t x_bs, int scheme,
                              const uint32_t* dy_amax, const uint32_t* x_amax, void* workspace,
                              void* stream, int io16) {
  // dW[M,K] = sum_b dY[b][M,N] . X[b][K,N]^T : GEMM with M'=M, N'=K, K'=N, reduced over samples.
  if (int e = check_gemm("pw_gemm_wgrad", 1, M, N, K)) return e;
  if (io16) {
    PD_REQUIRE(scheme == PARADIS_GEMM_BF16 && (io16 & ~(IO_A16 | IO_B16)) == 0,
               "pw_gemm_wgrad: bf16-stored operands need the PARADIS_GEMM_BF16 scheme (io16 = dY 8 | X 1)");
    auto a16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
    PD_REQUIRE(N % SBK == 0 && a16(dY) && a16(X) && dy_bs % ((io16 & IO_A16) ? 8 : 4) == 0 &&
               x_bs % ((io16 & IO_B16) ? 8 : 4) == 0,
               "pw_gemm_wgrad: bf16-stored operands need N %% 16 == 0 and 16-byte aligned rows");
  }
  PD_REQUIRE(known_scheme(scheme), "pw_gemm_wgrad: unknown scheme %d", scheme);
  PD_REQUIRE(scheme != PARADIS_GEMM_F16X2 || (dy_amax != nullptr && x_amax != nullptr),
             "pw_gemm_wgrad: the f16x2 scheme needs dy_amax and x_amax");
  hipStream_t st = (hipStream_t)stream;
  if (B == 0) {
    if (pd_zero_async(dW, (size_t)M * K * sizeof(float), st) != hipSuccess) return 2;
    if (gbias && pd_zero_async(gbias, (size_t)M * sizeof(float), st) != hipSuccess) return 2;
    return 0;
  }
  // a split scheme: both operands are split in registers (same layout requirements as the LDS-DMA kernel)
  const bool use_split = io16 != 0 || (scheme != PARADIS_GEMM_EXACT && wgrad_vec_layout(N, dy_bs, x_bs, dY, X));
  const bool dma = use_split || wgrad_dma_ok(N, dy_bs, x_bs, dY, X);   // "dma" = kernels with fused row sums
  const bool tall = use_split && scheme == PARADIS_GEMM_BF16 && wgrad_tall_ok(M);
  const bool square = tall && wgrad_square_on() && ((K + 255) / 256) * 256 * 7 <= K * 8;
  const int S = square ? wgrad_splits_square(B, M, K, N) : tall ? wgrad_splits_tall(B, M, K, N)
              : use_split ? wgrad_splits(B, M, K, N, SBK, 3)
                          : dma ? wgrad_splits(B, M, K, N, DBK, wgrad_dma_wgs())
                                : wgrad_splits(B, M, K, N, g_bk, g_wg_per_cu);
  PD_REQUIRE(workspace != nullptr, "pw_gemm_wgrad: workspace required");
  float* rowsum_ws = (float*)workspace + (size_t)S * M * K;   // [S][M], behind the slabs
  if (gbias && !dma) {   // register-staged kernel has no fused row sums: separate reduction pass
    if (int e = paradis_bias_grads(dY, nullptr, gbias, B, M, N, dy_bs, stream)) return e;
  }
  GemmArgs g{};
  g.A = dY; g.B = X; g.C = S > 1 ? (float*)workspace : dW;
  g.M = M; g.N = K; g.K = N;
  g.lda = N; g.ldb = N; g.ldc = K;
  g.a_bs = 0; g.b_bs = 0; g.c_bs = (int64_t)M * K; g.nbatch = S;
  g.inner = B; g.a_is = dy_bs; g.b_is = x_bs;
  g.stagger = g_stagger;
  g.rowsum = (gbias && dma) ? rowsum_ws : nullptr;
  const int grid = (tall ? (M + 255) / 256 : (M + BM - 1) / BM) * ((K + BN - 1) / BN) * S;
  if (square || tall) {
    const int g2 = square ? ((M + 255) / 256) * ((K + 255) / 256) * S : grid;
    if (int e = pd_amp_launch_wgrad(g, io16, square ? 3 : 2, g2, st)) return e;
  } else if (use_split && scheme == PARADIS_GEMM_F16X2) {
    g.a_amax = dy_amax; g.b_amax = x_amax;
    hipLaunchKernelGGL(pw_gemm_wgrad_split_kernel<2>, dim3(grid), dim3(256), split_lds_wgrad(2), st, g);
  } else if (use_split && scheme == PARADIS_GEMM_BF16) {
    if (int e = pd_amp_launch_wgrad(g, io16, io16 ? 1 : 0, grid, st)) return e;
  } else if (use_split) {
    hipLaunchKernelGGL(pw_gemm_wgrad_split_kernel<3>, dim3(grid), dim3(256), split_lds_wgrad(3), st, g);
  } else if (dma) {
    const size_t bytes = (size_t)g_wgrad_dma_stages * 2 * DTILE * sizeof(float);
    if (g_wgrad_dma_stages == 2)
      hipLaunchKernelGGL(pw_gemm_wgrad_dma_kernel<2>, dim3(grid), dim3(256), bytes, st, g);
    else
      hipLaunchKernelGGL(pw_gemm_wgrad_dma_kernel<3>, dim3(grid), dim3(256), (size_t)3 * 2 * DTILE * sizeof(float), st, g);
  } else if (int e = launch_gemm<true, true>(g, grid, st)) return e;
  {
    // slab sums in a fixed order; with one slab the GEMM wrote dW itself and only the row sums (if any) remain
    const int64_t n = S > 1 ? (int64_t)M * K : 0;
    const int vec = n % 4 == 0 && ((reinterpret_cast<uintptr_t>(workspace) | reinterpret_cast<uintptr_t>(dW)) & 15) == 0;
    const int blocks1 = n ? (int)std::min<int64_t>(((vec ? n / 4 : n) + 255) / 256, 2048) : 0;
    const int n2 = g.rowsum ? M : 0, blocks2 = (n2 + 255) / 256;
    if (blocks1 + blocks2 > 0)
      hipLaunchKernelGGL(slab_reduce_kernel, dim3(blocks1 + blocks2), dim3(256), 0, st, (const float*)workspace, dW, n, S,
                         vec, (const float*)rowsum_ws, gbias, n2, blocks1);
  }
  PD_CHECK_LAUNCH("pw_gemm_wgrad");
  return 0;
}

extern "C" int paradis_pw_gemm_wgrad(const float* dY, const float* X, float* dW, float* gbias, int B,
                                     int M, int K, int N, int64_t dy_bs, int64_t x_bs, int scheme,
                                     const uint32_t* dy_amax, const uint32_t* x_amax, void* workspace,
                                     void* stream) {
  return pw_gemm_wgrad_impl(dY, X, dW, gbias, B, M, K, N, dy_bs, x_bs, scheme, dy_amax, x_amax, workspace, stream, 0);
}

// PARADIS_GEMM_BF16 with bf16-STORED operands: io16 = PARADIS_IO_DY16 (dY is bf16) | PARADIS_IO_X16 (X is bf16); dW and the
// bias gradient stay fp32.  Workspace: paradis_pw_gemm_wgrad_ws_bytes.
extern "C" int paradis_pw_gemm_wgrad16(const void* dY, const void* X, float* dW, float* gbias, int B, int M, int K, int N,
                                       int64_t dy_bs, int64_t x_bs, int io16, void* workspace, void* stream) {
  return pw_gemm_wgrad_impl((const float*)dY, (const float*)X, dW, gbias, B, M, K, N, dy_bs, x_bs, PARADIS_GEMM_BF16,
                            nullptr, nullptr, workspace, stream, io16);
}
