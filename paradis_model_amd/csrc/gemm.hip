// a6: pointwise (1x1) channel mixing as a batched GEMM.
// Reference call sites: model/blocks.py:86 (CLinear), :110 (SepConv pointwise).
//
//   fwd   : Y[b][Co,P] = epi( W[Co,Ci] . X[b][Ci,P] )      A = W  (k-contiguous), B = X  (n-contiguous)
//   dgrad : dX[b][Ci,P] = epi( W^T . dY[b][Co,P] )         A = W^T(m-contiguous), B = dY (n-contiguous)
//   wgrad : dW[Co,Ci]   = sum_b dY[b] . X[b]^T             A = dY (k-contiguous), B = X^T(k-contiguous)
//
// This unit is the C ABI of those three and of paradis_bgemm: argument checks, GemmArgs, the choice of a kernel family and
// the weight gradient's slab reduction.  The kernels and their launchers live in gemm_exact.hip (f32 MFMA: exact fp32),
// gemm_split.hip (bf16x3 / f16x2 split operands, weight images), gemm_amp_fwd.hip and gemm_amp_wgrad.hip (the bf16-mixed
// scheme, PARADIS_GEMM_BF16); what the five share, the weight gradient's plan included, is in gemm_common.h.
#include "gemm_common.h"

namespace {

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

bool known_scheme(int scheme) {
  return scheme == PARADIS_GEMM_EXACT || scheme == PARADIS_GEMM_BF16X3 || scheme == PARADIS_GEMM_F16X2 ||
         scheme == PARADIS_GEMM_BF16;
}

int check_gemm(const char* name, int B, int M, int K, int N) {
  PD_REQUIRE(B >= 0 && M >= 1 && K >= 1 && N >= 1, "%s: bad shape B=%d M=%d K=%d N=%d", name, B, M, K, N);
  const int64_t tiles = (int64_t)((M + BM - 1) / BM) * ((N + BN - 1) / BN) * std::max(B, 1);
  PD_REQUIRE(tiles < (1ll << 31), "%s: too many tiles", name);
  return 0;
}

// A = split image at `img` of an [AM, AK] matrix; F16X2 needs the activations' amax partials
int run_split(GemmArgs d, const void* img, int AM, int AK, int scheme, const uint32_t* b_amax, const char* what,
              hipStream_t st) {
  d.A = (const float*)img; d.a_bs = 0;
  if (scheme == PARADIS_GEMM_F16X2) {
    if (b_amax == nullptr) { paradis_set_error(what); return 1; }
    d.a_amax = reinterpret_cast<const uint32_t*>((const char*)img + (size_t)pd_split_image_chunks(AM, AK, 2) * 16);
    d.b_amax = b_amax;
  }
  return scheme == PARADIS_GEMM_BF16 ? pd_amp_launch_fwd(d, st) : pd_split_launch(d, scheme, st);
}
// The f32-MFMA tail of fwd / dgrad / bgemm: the LDS-DMA kernel on `rows` - the arguments with a row-contiguous A operand,
// nullptr if the caller has none - where it is eligible, else the register-staged kernel on g (a_kc: A is k-contiguous)
int run_exact(const char* name, const GemmArgs& g, const GemmArgs* rows, bool a_kc, int grid, hipStream_t st) {
  const bool dma = rows != nullptr && pd_exact_dma_eligible(*rows);
  if (int e = dma ? pd_exact_launch_dma(*rows, grid, st) : pd_exact_launch(a_kc, false, g, grid, st)) return e;
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    paradis_set_error("%s%s: launch failed: %s", name, dma ? "(dma)" : "", hipGetErrorString(e));
    return 2;
  }
  return 0;
}
// bf16-stored tensors exist in the bf16-mixed scheme only; the DMA'd activation operand needs whole 16-byte chunks
int check_io16(const char* name, int io16, int scheme, const void* Bop, int64_t b_bs, int N, bool has_res) {
  if (io16 == 0) return 0;
  PD_REQUIRE(scheme == PARADIS_GEMM_BF16, "%s: bf16-stored tensors need the PARADIS_GEMM_BF16 scheme", name);
  PD_REQUIRE((io16 & ~(IO_B16 | IO_C16 | IO_ZM16 | IO_A16)) == 0, "%s: unknown io16 bits %d", name, io16);
  PD_REQUIRE(!(io16 & IO_C16) || !has_res, "%s: a bf16 output cannot carry the fp32 residual", name);
  if (io16 & IO_B16)
    PD_REQUIRE(N % 8 == 0 && N >= 8 && b_bs % 8 == 0 && aligned16(Bop),
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
  g.stagger = pd_exact_tunables().stagger;
  g.io16 = io16;
  const int grid = ((M + BM - 1) / BM) * ((N + BN - 1) / BN) * B;
  if (Wsplit != nullptr) {   // split image of the weights: split kernel (any shape)
    if (int e = run_split(g, Wsplit, M, K, scheme, x_amax, "pw_gemm_fwd: the f16x2 scheme needs x_amax",
                          (hipStream_t)stream)) return e;
    PD_CHECK_LAUNCH("pw_gemm_fwd(split)");
    return 0;
  }
  GemmArgs d = g;         // weights also supplied as [K,M]: row-contiguous A operand -> LDS-DMA kernel
  d.A = WtT; d.lda = M;
  return run_exact("pw_gemm_fwd", g, WtT ? &d : nullptr, true, grid, (hipStream_t)stream);
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
  g.stagger = pd_exact_tunables().stagger;
  const int64_t tiles = (int64_t)((M + BM - 1) / BM) * ((N + BN - 1) / BN) * nbatch;
  PD_REQUIRE(tiles < (1ll << 31), "bgemm: too many tiles");
  const int grid = (int)tiles;
  if (split_ws != nullptr) {   // bf16-split path: images of the nbatch A matrices in split_ws
    PD_REQUIRE(nbatch <= 65535, "bgemm: too many batches for the split path");
    pd_split_launch_images(A, nbatch, M, K, a_bs, split_ws, (hipStream_t)stream);
    GemmArgs d = g;
    d.A = (const float*)split_ws; d.a_bs = pd_split_image_chunks(M, K, 3);
    if (int e = pd_split_launch(d, PARADIS_GEMM_BF16X3, (hipStream_t)stream)) return e;
    PD_CHECK_LAUNCH("bgemm(split)");
    return 0;
  }
  GemmArgs d = g;
  d.A = AT; d.lda = M; d.a_bs = at_bs;
  return run_exact("bgemm", g, AT ? &d : nullptr, true, grid, (hipStream_t)stream);
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
  g.stagger = pd_exact_tunables().stagger;
  g.io16 = io16;
  const int grid = ((K + BM - 1) / BM) * ((N + BN - 1) / BN) * B;
  if (WTsplit != nullptr) {   // split image of W^T
    if (int e = run_split(g, WTsplit, K, M, scheme, dy_amax, "pw_gemm_dgrad: the f16x2 scheme needs dy_amax",
                          (hipStream_t)stream)) return e;
    PD_CHECK_LAUNCH("pw_gemm_dgrad(split)");
    return 0;
  }
  return run_exact("pw_gemm_dgrad", g, &g, false, grid, (hipStream_t)stream);
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

// slabs + row-sum partials of whichever kernel the call turns out to take (wgrad_ws_bytes, gemm_common.h)
extern "C" size_t paradis_pw_gemm_wgrad_ws_bytes(int B, int M, int K, int N) {
  return wgrad_ws_bytes(B, M, K, N, pd_exact_tunables());
}

// K-range slabs the split weight-gradient kernel runs for this shape (1, or an even number: see wgrad_splits)
extern "C" int paradis_pw_gemm_wgrad_slabs(int B, int M, int K, int N) {
  if (M < 1 || K < 1 || N < 1) return 0;
  return wgrad_plan_of(WgradKind::Bf16x3, std::max(B, 1), M, K, N, pd_exact_tunables()).S;
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
    PD_REQUIRE(N % SBK == 0 && aligned16(dY) && aligned16(X) && dy_bs % ((io16 & IO_A16) ? 8 : 4) == 0 &&
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
  PD_REQUIRE(workspace != nullptr, "pw_gemm_wgrad: workspace required");
  const GemmTunables tun = pd_exact_tunables();
  const WgradPlan p = wgrad_plan(B, M, K, N, dy_bs, x_bs, dY, X, scheme, io16, tun, wgrad_env());
  const bool rowsums = gbias && p.fused_rowsums;
  if (gbias && !rowsums) {   // the register-staged kernel has no fused row sums: separate reduction pass
    if (int e = paradis_bias_grads(dY, nullptr, gbias, B, M, N, dy_bs, stream)) return e;
  }
  GemmArgs g{};
  g.A = dY; g.B = X; g.C = p.to_slabs ? (float*)workspace : dW;
  g.M = M; g.N = K; g.K = N;
  g.lda = N; g.ldb = N; g.ldc = K;
  g.a_bs = 0; g.b_bs = 0; g.c_bs = (int64_t)M * K; g.nbatch = p.S;
  g.inner = B; g.a_is = dy_bs; g.b_is = x_bs;
  g.stagger = tun.stagger;
  g.rowsum = rowsums ? p.ws.rowsums(workspace) : nullptr;
  int e = 0;
  switch (p.kind) {
    case WgradKind::Staged: case WgradKind::Dma: e = pd_exact_launch_wgrad(g, p, st); break;
    case WgradKind::F16x2: g.a_amax = dy_amax; g.b_amax = x_amax; [[fallthrough]];
    case WgradKind::Bf16x3: e = pd_split_launch_wgrad(g, p, st); break;
    case WgradKind::Amp128: case WgradKind::Tall: case WgradKind::Square: e = pd_amp_launch_wgrad(g, io16, p, st); break;
  }
  if (e) return e;
  const SlabReduce r = wgrad_reduce(p, workspace, dW, rowsums);
  if (r.blocks1 + r.blocks2 > 0)
    hipLaunchKernelGGL(slab_reduce_kernel, dim3(r.blocks1 + r.blocks2), dim3(256), 0, st, (const float*)workspace, dW, r.n, p.S,
                       r.vec, (const float*)p.ws.rowsums(workspace), gbias, r.n2, r.blocks1);
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
