// The f32-MFMA family of the pointwise GEMMs (v_mfma_f32_32x32x2_f32; entry points and operand layouts: gemm.hip): the
// register-staged kernel, the LDS-DMA kernels of fwd / dgrad and of the weight gradient, their tunables and their launchers
// (pd_exact_*, declared in gemm_common.h and called from gemm.hip).
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
#include "gemm_common.h"

namespace {

constexpr int ld_of(bool kc) { return kc ? BM + 1 : BM + 4; }  // floats per k-row of the LDS image
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

  const bool a_vec = ((g.lda & 3) == 0) && aligned16(g.A) && ((g.a_bs & 3) == 0) && ((g.a_is & 3) == 0);
  const bool b_vec = ((g.ldb & 3) == 0) && aligned16(g.B) && ((g.b_bs & 3) == 0) && ((g.b_is & 3) == 0);

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
// (DBK = 16, the k-tile depth, and DTILE = DBK * BM floats per operand and stage: gemm_common.h, beside the LDS sizes)


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

// ---- host side: one table per kernel, indexed by its template parameters ------------------------------------------------
#define STAGED_BK(A_KC, B_KC) {&pw_gemm_kernel<A_KC, B_KC, 16>, STAGED_LDS_MAX}, {&pw_gemm_kernel<A_KC, B_KC, 32>, STAGED_LDS_MAX}
// [staged_index(A_KC, B_KC, BK)]; nobody has a row-contiguous A beside a k-contiguous B
constexpr int staged_index(bool a_kc, bool b_kc, int bk) { return (a_kc * 2 + b_kc) * 2 + (bk == 32); }
constexpr GemmKernelEntry STAGED[8] = {STAGED_BK(false, false), {nullptr, 0}, {nullptr, 0}, STAGED_BK(true, false), STAGED_BK(true, true)};
#undef STAGED_BK
// [S - 2], S = ring depth; the second parameter: workgroups per CU that S stages leave room for
constexpr GemmKernelEntry DMA[3] = {{&pw_gemm_dma_kernel<2, 4>, dma_lds_bytes(2)}, {&pw_gemm_dma_kernel<3, 3>, dma_lds_bytes(3)},
                                    {&pw_gemm_dma_kernel<4, 2>, dma_lds_bytes(4)}};
constexpr GemmKernelEntry WGRAD_DMA[2] = {{&pw_gemm_wgrad_dma_kernel<2>, dma_lds_bytes(2)},
                                          {&pw_gemm_wgrad_dma_kernel<3>, dma_lds_bytes(3)}};

}  // namespace

GemmTunables pd_exact_tunables() { return {g_bk, g_wg_per_cu, g_stagger, g_dma_stages, g_wgrad_dma_stages}; }

int pd_exact_launch(bool a_kc, bool b_kc, const GemmArgs& g, int grid, hipStream_t st) {
  static PerDeviceOnce once;
  return launch_entry(STAGED, staged_index(a_kc, b_kc, g_bk), once, "pw_gemm", grid, 256, st, g,
                      staged_lds_request(g_bk, g_wg_per_cu));
}

bool pd_exact_dma_eligible(const GemmArgs& g) {
  return g_dma_stages >= 2 && g.inner == 0 && g.K % DBK == 0 && g.M % 4 == 0 && g.N % 4 == 0 &&
         g.M >= 4 && g.N >= 4 && (g.lda & 3) == 0 && (g.ldb & 3) == 0 && (g.a_bs & 3) == 0 &&
         (g.b_bs & 3) == 0 && aligned16(g.A) && aligned16(g.B);
}

int pd_exact_launch_dma(const GemmArgs& g, int grid, hipStream_t st) {
  static PerDeviceOnce once;
  return launch_entry(DMA, g_dma_stages - 2, once, "pw_gemm(dma)", grid, 256, st, g);
}

int pd_exact_launch_wgrad(const GemmArgs& g, const WgradPlan& p, hipStream_t st) {
  static PerDeviceOnce once;
  if (p.kind == WgradKind::Staged) return pd_exact_launch(true, true, g, p.grid, st);
  return launch_entry(WGRAD_DMA, g_wgrad_dma_stages - 2, once, "pw_gemm_wgrad(dma)", p.grid, p.block, st, g, p.lds);
}

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
