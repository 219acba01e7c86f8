/*
 * paradis_hip.h -- C ABI of libparadis_hip.so (gfx950 / MI355X).
 *
 * Drop-in boundary for the PARADIS advection-diffusion-reaction hot path.
 * The reference has no FFI layer (it is pure Python on ATen); each entry point
 * below replaces the ATen call sequence of the cited reference lines and is
 * what a ctypes binding in the reference's model/ package would call (see
 * INTEGRATION.md).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to fp32 (unless noted), NCHW, planes
 *     (H*W) contiguous; `*_bs` arguments are batch strides in ELEMENTS so that
 *     channel slices of a larger tensor can be read/written without copies;
 *   - inputs are borrowed, outputs are caller-allocated, no global mutable
 *     state, no host synchronisation; kernels are enqueued on `stream`
 *     (a hipStream_t passed as void*), so calls are graph-capturable;
 *   - return 0 on success; non-zero = rejected arguments (1) or HIP launch
 *     failure (2); paradis_last_error() returns a thread-local message;
 *   - `act`: 0 none, 1 SiLU, 2 GELU(erf).  `mode`: 1 bilinear, 2 bicubic.
 */
#ifndef PARADIS_HIP_H
#define PARADIS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PARADIS_ACT_NONE 0
#define PARADIS_ACT_SILU 1
#define PARADIS_ACT_GELU 2
#define PARADIS_INTERP_BILINEAR 1
#define PARADIS_INTERP_BICUBIC 2
/* `flags` of paradis_sl_advect_{fwd,bwd}.  0 = automatic schedule: the whole padded plane in LDS when it
 * fits 64 KiB (one wave per latitude row when W == 64 and PARADIS_ADVECT_SEPARABLE is set), otherwise
 * a windowed schedule with an L2 path for taps outside the window: with PARADIS_ADVECT_SEPARABLE 128-column strips
 * walked top to bottom through a ring of padded rows in LDS (round 4), otherwise 128-column tiles with a halo.
 *   bit 0  PARADIS_ADVECT_GENERIC   whole-plane schedule with per-point table loads even when W == 64
 *   bit 1  PARADIS_ADVECT_TILED     windowed schedule regardless of the plane size
 *   bit 2  PARADIS_ADVECT_SEPARABLE the caller vouches that sin_lat/cos_lat are constant along a row and
 *                                   lon along a column (every regular lat-lon grid)
 *   bit 3  PARADIS_ADVECT_TILES     diagnostic: the 64 x 128 / 16 x 128 tile schedule of rounds 2-3 instead of strips
 *   bit 4  PARADIS_ADVECT_STRIPS    backward: 128-column strips even where the full-circle ring (W <= 256) would run
 *   bits 8-15  window halo in longitude of the windowed schedules (0 = built-in default, else halo + 1)
 *   bits 16-23 the same for the backward kernel only */
#define PARADIS_ADVECT_AUTO 0
#define PARADIS_ADVECT_GENERIC 1
#define PARADIS_ADVECT_TILED 2
#define PARADIS_ADVECT_SEPARABLE 4
#define PARADIS_ADVECT_TILES 8
#define PARADIS_ADVECT_STRIPS 16
#define PARADIS_ADVECT_HALO_SHIFT 8
#define PARADIS_ADVECT_HALO_BWD_SHIFT 16
#define PARADIS_ADVECT_HALO(h) (((h) + 1) << PARADIS_ADVECT_HALO_SHIFT)

int paradis_abi_version(void);   /* 10: paradis_adamw_step_d / paradis_adamw_multi_d (hyper-parameters in double): additions only; 9: bf16-stored tensors of the bf16-mixed mode (paradis_pw_gemm_fwd16 / _dgrad16 / _wgrad16, paradis_bias_grads16, paradis_channel_norm_fwd16 / _bwd16, paradis_dwconv_geo_fwd16 / _bwd16, paradis_act_bwd16): additions only; 8: PARADIS_GEMM_BF16 scheme, paradis_pw_gemm_wgrad_slabs (query); no signature changed; 7: paradis_dwconv_geo_dgrad_add, paradis_dwconv_geo_bwd, paradis_pw_gemm_split_weights_pair, paradis_pw_gemm_fwd_gated, paradis_gated_blend_bwd_out; 6: paradis_sl_advect_ws_bytes takes the call's flags (strip schedule); 5: no amax side outputs, lat_cells table of sl_advect_* (4: GEMM `scheme` arguments, paradis_amax_partials; 3: `flags` of sl_advect_*) */
const char* paradis_last_error(void);

/* ---- a1: GeoCyclicPadding.forward (reference model/padding.py:11-39) and its adjoint.
 * x [planes,H,W] -> y [planes,H+2p,W+2p];  gx[src(i,j)] += gy[i,j]. Integer index map, bit-exact. */
int paradis_geocyclic_pad_fwd(const float* x, float* y, int64_t planes, int H, int W, int p, void* stream);
int paradis_geocyclic_pad_bwd(const float* gy, float* gx, int64_t planes, int H, int W, int p, void* stream);

/* ---- a3-a5: fused core of NeuralSemiLagrangian.forward (reference model/advection.py:129-169):
 * pole mean -> departure point (advection.py:74-98) -> virtual geocyclic index map ->
 * bilinear/bicubic gather (ATen grid_sampler_2d semantics, align_corners, zeros) -> pole mean.
 * field/out [B,K,H,W]; u,v [B,K,H,W] with batch stride uv_bs; sin_lat/cos_lat/lon tables [H*W].
 * lat_cells [H*W] (optional, NULL allowed): the arrival latitude in PADDED cells,
 *   p + (lat - min_lat) (H-1)/d_lat   with p = 2 (bicubic) | 1 (bilinear), evaluated in double and rounded once.
 *   The separable schedules (PARADIS_ADVECT_SEPARABLE) need it: they take the departure latitude relative to the
 *   arrival latitude at small displacements (no asin half-angle chain, no 1/cos(lat) amplification of the rounding
 *   of sin(lat_d) next to the poles); without the table the per-point kernels run. */
int paradis_sl_advect_fwd(const float* field, const float* u, const float* v, float* out,
                          const float* sin_lat, const float* cos_lat, const float* lat_cells, const float* lon,
                          int B, int K, int H, int W, int64_t f_bs, int64_t uv_bs, int64_t o_bs,
                          float dt, float min_lat, float min_lon, float d_lat, float d_lon,
                          int mode, int flags, void* workspace, void* stream);
/* gfield [B,K,H,W] (batch stride gf_bs), gu/gv with batch stride guv_bs.
 * workspace (fwd and bwd): >= paradis_sl_advect_ws_bytes(B,K,H,W,flags) bytes for the `flags` of the call (with
 * PARADIS_DETERMINISTIC=1 this includes the 64-bit integer plane the windowed backward accumulates into: 8 bytes per
 * gather point; for the strip schedule it includes the lists of points whose taps leave the window: 12 bytes per gather
 * point). */
size_t paradis_sl_advect_ws_bytes(int B, int K, int H, int W, int flags);
int paradis_sl_advect_bwd(const float* gout, const float* field, const float* u, const float* v,
                          float* gfield, float* gu, float* gv,
                          const float* sin_lat, const float* cos_lat, const float* lat_cells, const float* lon,
                          int B, int K, int H, int W, int64_t go_bs, int64_t f_bs, int64_t uv_bs,
                          int64_t gf_bs, int64_t guv_bs,
                          float dt, float min_lat, float min_lon, float d_lat, float d_lon,
                          int mode, int flags, void* workspace, void* stream);

/* ---- a7 (depthwise half of SepConv, reference model/blocks.py:101-113) and the static
 * encoder's GeoCyclicPadding(3)+Conv2d(groups=C) (reference model/paradis.py:189-190):
 * k x k per-channel stencil on the virtual geocyclic halo. w [C,k,k]; bias [C] or NULL; k odd, 1..11. */
int paradis_dwconv_geo_fwd(const float* x, const float* w, const float* bias, float* y,
                           int B, int C, int H, int W, int k, void* stream);
int paradis_dwconv_geo_dgrad(const float* gy, const float* w, float* gx,
                             int B, int C, int H, int W, int k, void* stream);
/* gx = dgrad(gy) + addend: the stencil's input has a second consumer (the block input that the gated blend of
 * reference model/paradis.py:239-240 reads next to the advection's down-projection); its gradient enters here
 * instead of through an accumulation pass.  addend [B,C,H,W], must not alias gx.  (ABI 7) */
int paradis_dwconv_geo_dgrad_add(const float* gy, const float* w, const float* addend, float* gx,
                                 int B, int C, int H, int W, int k, void* stream);
/* Both gradients from one call (autograd of the same module): gx = dgrad(gy) (+ addend, nullable), gw [C,k,k],
 * gbias [C] or NULL.  k = 5 with 16-byte aligned tensors and W = 64, H <= 32 (one tile) or H >= 32, W >= 64, W % 4 == 0
 * (several tiles): one kernel that reads gy once; otherwise the two kernels above.  Bit-identical to them.
 * workspace: paradis_dwconv_geo_wgrad_ws_bytes.  (ABI 7) */
int paradis_dwconv_geo_bwd(const float* gy, const float* x, const float* w, const float* addend, float* gx,
                           float* gw, float* gbias, int B, int C, int H, int W, int k, void* workspace, void* stream);
size_t paradis_dwconv_geo_wgrad_ws_bytes(int B, int C, int H, int W, int k);
int paradis_dwconv_geo_wgrad(const float* gy, const float* x, float* gw, float* gbias,
                             int B, int C, int H, int W, int k, void* workspace, void* stream);

/* ---- a11: PhysicalDownsample (reference model/blocks.py:57-71): geocyclic 5x5 box mean, stride s >= 1;
 * y [planes, (H-1)/s + 1, (W-1)/s + 1].  Restriction: H >= 4 and W >= 4, W even (rc 1 otherwise).  The reference module
 * also runs at H = 3 (its halo rows then mirror through the opposite pole row) and at W = 2 (the wrap repeats the
 * plane); neither is a grid the model is built on, and the index map of a1 (pad <= H - 2) does not cover them. */
int paradis_avgpool_geo_fwd(const float* x, float* y, int64_t planes, int H, int W, int stride, void* stream);
int paradis_avgpool_geo_bwd(const float* gy, float* gx, int64_t planes, int H, int W, int stride, void* stream);

/* ---- a14: Paradis.upsample (reference model/paradis.py:208-220): lon-periodic bilinear, align_corners */
int paradis_upsample_lonp_fwd(const float* x, float* y, int64_t planes, int Hc, int Wc, int H, int W, void* stream);
int paradis_upsample_lonp_bwd(const float* gy, float* gx, int64_t planes, int Hc, int Wc, int H, int W, void* stream);

/* ---- a6: CLinear / pointwise half of SepConv (reference model/blocks.py:86,110): per-sample GEMM.
 * Y[b] = epi( W[M,K] * X[b][K,N] ),  epi(v) = res + act(v + bias[m] + map[m,n]).
 * bias/map/res/zpre may be NULL.  zpre (if given) receives the pre-activation value.
 *
 * Three arithmetic schemes, all fp32 in / fp32 accumulate / fp32 out (`scheme` arguments):
 *   - PARADIS_GEMM_EXACT:  v_mfma_f32_32x32x2_f32 (an fmaf chain over k);
 *   - PARADIS_GEMM_BF16X3: each fp32 operand is decomposed exactly into three bf16 terms and the product is
 *     accumulated from the six partial products >= 2^-16 on v_mfma_f32_32x32x16_bf16 (relative
 *     truncation 2^-23 per product, fewer accumulation roundings: error vs fp64 not above the exact path's);
 *   - PARADIS_GEMM_F16X2 (opt-in; a block-exponent format, NOT the reference's per-element fp32 arithmetic):
 *     each operand TENSOR is scaled by a power of two that puts its largest magnitude
 *     into [2^14, 2^15) and every value is written as two f16 terms (22 significand bits; values more than
 *     ~2^17 below the tensor's maximum keep an absolute accuracy of 2^-39 max|x|); three partial products on
 *     v_mfma_f32_32x32x16_f16, result unscaled in the epilogue.  Error vs fp64 of a K = 1024 product: that of
 *     an fp32 SGEMM.  Needs the tensors' largest magnitudes: paradis_amax_partials for activations, the
 *     weight image carries its own.
 * fwd / dgrad take the split image of their weight operand (NULL with PARADIS_GEMM_EXACT).
 *
 * A fourth scheme is NOT fp32 arithmetic and exists for one purpose - the reference's shipped training mode
 * `use_amp: true` (config/paradis_settings.yaml:75 -> precision="bf16-mixed", train.py:56), in which torch.autocast runs
 * every conv2d with bf16 operands and a bf16 result:
 *   - PARADIS_GEMM_BF16 (ABI 8): operands rounded to bf16, ONE product on v_mfma_f32_32x32x16_bf16, fp32 accumulate;
 *     the pre-activation, the activated value and (dgrad) the activation-gradient product are rounded to bf16 where
 *     autocast's conv2d / activation round them, the residual / blend and the weight gradient stay fp32; tensors are
 *     stored as fp32.  The Python layer selects it only under torch.autocast(dtype=bfloat16). */
#define PARADIS_GEMM_EXACT 0
#define PARADIS_GEMM_BF16 1     /* ABI 8: the reference's bf16-mixed (AMP) mode, never the fp32 path: see below */
#define PARADIS_GEMM_F16X2 2
#define PARADIS_GEMM_BF16X3 3
#define PARADIS_AMAX_PARTIALS 1024
/* partials[PARADIS_AMAX_PARTIALS] <- bit patterns of partial maxima of |x| over B blocks of `inner`
 * contiguous floats (block stride bs); the tensor's maximum is the (unsigned) maximum of the words, a NaN
 * anywhere makes it a NaN pattern.  One read pass, no atomics, no pre-zeroing. */
int paradis_amax_partials(const float* x, int B, int64_t inner, int64_t bs, uint32_t* partials, void* stream);
size_t paradis_pw_gemm_split_bytes(int M, int K, int scheme);   /* bytes of the split image of an [M,K] A operand */
/* split image of A = W[M,K] (transpose 0; out: split_bytes(M,K,scheme)) or of A = W^T (transpose 1; out:
 * split_bytes(K,M,scheme)) from row-major W[M,K]; scheme = PARADIS_GEMM_BF16X3 or PARADIS_GEMM_F16X2 */
int paradis_pw_gemm_split_weights(const float* W, int M, int K, int transpose, int scheme, void* out, void* stream);
/* PARADIS_GEMM_BF16X3 images of W (-> out) and of W^T (-> out_t) in one launch: a training step needs both (ABI 7) */
int paradis_pw_gemm_split_weights_pair(const float* W, int M, int K, void* out, void* out_t, void* stream);
/* the same for PARADIS_GEMM_BF16X3 or PARADIS_GEMM_BF16 (ABI 9) */
int paradis_pw_gemm_split_weights_pair_scheme(const float* W, int M, int K, int scheme, void* out, void* out_t, void* stream);
int paradis_pw_gemm_fwd(const float* Wt, const float* WtT /* optional [K,M] copy of Wt, or NULL */,
                        const void* Wsplit /* split image of Wt for `scheme`, NULL for PARADIS_GEMM_EXACT */,
                        int scheme, const uint32_t* x_amax /* amax partials of X: PARADIS_GEMM_F16X2 only */,
                        const float* X, const float* bias, const float* map,
                        const float* m8 /* [cin,N] */, const float* pwT /* [cin,M] */, int cin,
                        /* ^ optional low-rank bias applied on the fly: + sum_c pwT[c,m]*m8[c,n] (GlobalBias
                         *   with projection, reference model/blocks.py:190-196), M % 4 == 0, or NULL/NULL/0 */
                        const float* res, float* Y, float* zpre,
                        int B, int M, int K, int N, int64_t x_bs, int64_t res_bs, int64_t y_bs,
                        int act, void* stream);
/* The same with the gated blend of reference model/paradis.py:239-243 in the epilogue:
 * Y = res + sigmoid(gate[m]) (act(...) - res); gate [M] = alpha_adv, res = the field the advection started from.
 * Bit-identical to paradis_pw_gemm_fwd (res = NULL) followed by paradis_gated_blend_fwd.  (ABI 7) */
int paradis_pw_gemm_fwd_gated(const float* Wt, const float* WtT, const void* Wsplit, int scheme, const uint32_t* x_amax,
                              const float* X, const float* bias, const float* map, const float* m8, const float* pwT,
                              int cin, const float* res, const float* gate, float* Y, float* zpre,
                              int B, int M, int K, int N, int64_t x_bs, int64_t res_bs, int64_t y_bs,
                              int act, void* stream);
/* dX[b][K,N] = (W^T[K,M] * dY[b][M,N]) (* act'(zpre[b][K,N]) if zpre) (+ addend[b][K,N] if addend);
 * WTsplit: split image of W^T (paradis_pw_gemm_split_weights(..., transpose=1)), NULL for PARADIS_GEMM_EXACT */
int paradis_pw_gemm_dgrad(const float* Wt, const void* WTsplit, int scheme,
                          const uint32_t* dy_amax /* amax partials of dY: PARADIS_GEMM_F16X2 only */,
                          const float* dY, const float* zpre,
                          const float* addend, float* dX, int B, int M, int K, int N, int64_t dy_bs,
                          int64_t z_bs, int64_t add_bs, int64_t dx_bs, int act, void* stream);
/* dW[M,K] = sum_b dY[b][M,N] * X[b][K,N]^T ; gbias[M] = sum_{b,n} dY (optional, NULL to skip; fused
 * into the GEMM as row sums of its A operand); workspace >= paradis_pw_gemm_wgrad_ws_bytes;
 * a split scheme is used when N % 16 == 0 and the rows are 16-B aligned (the exact kernels run otherwise) */
size_t paradis_pw_gemm_wgrad_ws_bytes(int B, int M, int K, int N);
/* number of K-range slabs of the split weight-gradient kernel for this shape: 1 or an even number (alternate slabs
 * accumulate with opposite sign; the bf16 MFMA's accumulator-alignment offset cancels in the slab sum).  (ABI 8) */
int paradis_pw_gemm_wgrad_slabs(int B, int M, int K, int N);
int paradis_pw_gemm_wgrad(const float* dY, const float* X, float* dW, float* gbias,
                          int B, int M, int K, int N, int64_t dy_bs, int64_t x_bs, int scheme,
                          const uint32_t* dy_amax, const uint32_t* x_amax /* PARADIS_GEMM_F16X2 only */,
                          void* workspace, void* stream);

/* ---- bf16-STORED tensors of the bf16-mixed mode (ABI 9; PARADIS_GEMM_BF16 only).  Under torch.autocast(bfloat16) the
 * reference's nn.Conv2d calls (model/blocks.py:86,110) produce bf16 TENSORS (config/paradis_settings.yaml:75 ->
 * train.py:56); these entry points take / write such tensors in place of the fp32 words holding bf16 values that the
 * fp32-pointer entry points above use in this scheme: same values bit for bit, half the bytes.  `io16` says which
 * tensors are bf16 (2 bytes per element; all strides stay in ELEMENTS); everything not named is fp32.
 *   fwd16  : PARADIS_IO_X16 = X,  PARADIS_IO_Y16 = Y and zpre (no residual then)
 *   dgrad16: PARADIS_IO_X16 = dY, PARADIS_IO_Y16 = dX, PARADIS_IO_Z16 = zpre
 *   wgrad16: PARADIS_IO_X16 = X,  PARADIS_IO_DY16 = dY (dW, gbias fp32)
 * A bf16 activation operand needs N % 8 == 0 (wgrad: N % 16 == 0) and 16-byte aligned planes: it is staged HBM -> LDS by
 * LDS-DMA and transposed by ds_read_b64_tr_b16 (fwd / dgrad), never touching the vector ALU.  Wsplit / WTsplit: the
 * PARADIS_GEMM_BF16 weight images of paradis_pw_gemm_split_weights. */
#define PARADIS_IO_X16 1
#define PARADIS_IO_Y16 2
#define PARADIS_IO_Z16 4
#define PARADIS_IO_DY16 8
int paradis_pw_gemm_fwd16(const void* Wsplit, const void* X, const float* bias, const float* map, const float* m8,
                          const float* pwT, int cin, const float* res, const float* gate /* or NULL */, void* Y,
                          void* zpre, int B, int M, int K, int N, int64_t x_bs, int64_t res_bs, int64_t y_bs, int act,
                          int io16, void* stream);
int paradis_pw_gemm_dgrad16(const void* WTsplit, const void* dY, const void* zpre, void* dX, int B, int M, int K, int N,
                            int64_t dy_bs, int64_t z_bs, int64_t dx_bs, int act, int io16, void* stream);
int paradis_pw_gemm_wgrad16(const void* dY, const void* X, float* dW, float* gbias, int B, int M, int K, int N,
                            int64_t dy_bs, int64_t x_bs, int io16, void* workspace, void* stream);
/* the producers of a pointwise layer's input writing it as bf16 (round to nearest even: the value the GEMM rounds its
 * operand to): ChannelNorm (model/blocks.py:118-134) and the depthwise stencil of a SepConv (:101-113) */
int paradis_channel_norm_fwd16(const float* x1, const float* x2, const float* w, const float* b, void* y /* bf16 */,
                               float* mean, float* rstd, int B, int C1, int C2, int P, int64_t x1_bs, int64_t x2_bs,
                               float eps, void* stream);
int paradis_dwconv_geo_fwd16(const float* x, const float* w, const float* bias, void* y /* bf16 */, int B, int C, int H,
                             int W, int k, void* stream);
/* ... and their backward reading the cotangent of that bf16 output as a bf16 tensor - the consumer's data gradient, bf16-valued in
 * the reference's autocast backward as well.  Same arguments as paradis_channel_norm_bwd / paradis_dwconv_geo_bwd otherwise; every
 * result fp32 and bit-identical to the fp32 entry point on the widened cotangent.  Supported where the *_ok query returns 1
 * (ChannelNorm: exactly the shapes paradis_channel_norm_bwd accepts; the whole-plane stencil kernel: k = 5, W = 64, H <= 32);
 * elsewhere the call fails with rc 1 (a stencil caller widens gy; a ChannelNorm shape has no other route). */
int paradis_channel_norm_bwd16_ok(int B, int C, int P);
int paradis_channel_norm_bwd16(const void* gy /* bf16 */, const float* x1, const float* x2, const float* w, const float* mean,
                               const float* rstd, float* gx1, float* gx2, float* gw, float* gb, int B, int C1, int C2, int P,
                               int64_t x1_bs, int64_t x2_bs, int64_t gx1_bs, int64_t gx2_bs, const float* addend1,
                               int64_t add1_bs, void* workspace, void* stream);
int paradis_dwconv_geo_bwd16_ok(int H, int W, int k);
int paradis_dwconv_geo_bwd16(const void* gy /* bf16 */, const float* x, const float* w, const float* addend, float* gx, float* gw,
                             float* gbias, int B, int C, int H, int W, int k, void* workspace, void* stream);
/* paradis_act_bwd writing gx = gy * act'(x) as a bf16 tensor (to nearest even): d(pre-activation) of a pointwise layer, which both
 * of its gradient GEMMs would round to bf16 on load.  n % 4 == 0, 16-byte aligned gy / x. */
int paradis_act_bwd16(const float* gy, const float* x, void* gx /* bf16 */, int64_t n, int act, void* stream);
/* paradis_bias_grads on a bf16-stored dz (P % 8 == 0, 16-byte aligned rows); outputs fp32 */
int paradis_bias_grads16(const void* dz, float* gmap, float* gbias, int B, int C, int P, int64_t dz_bs, void* stream);

/* ---- a8: ChannelNorm (reference model/blocks.py:118-134): per-pixel, unbiased variance.
 * x may be the virtual concatenation [x1 (C1 ch, batch stride x1_bs) ; x2 (C2 ch)] (paradis.py:249). */
int paradis_channel_norm_fwd(const float* x1, const float* x2, const float* w, const float* b,
                             float* y, float* mean, float* rstd,
                             int B, int C1, int C2, int P, int64_t x1_bs, int64_t x2_bs,
                             float eps, void* stream);
size_t paradis_channel_norm_bwd_ws_bytes(int B, int C, int P);
/* gx1/gx2 receive the slices of the input gradient (gx2 may be NULL); gw,gb [C].
 * addend1 (optional, [B,C1,P] with batch stride add1_bs) is added to gx1: the gradient that reaches
 * x1 through the residual connection around the block (paradis.py:246,253), so autograd's separate
 * accumulation pass disappears.
 * One schedule (two streaming kernels, fixed-order finish) whose apply grid is B * (C1 + C2) * ceil(P / 8192) workgroups:
 * a shape at which that product reaches 2^31 - a cotangent of 8 GiB or more - is refused with rc 1 ("too large").
 * workspace: paradis_channel_norm_bwd_ws_bytes(B, C1 + C2, P) bytes, 16-byte aligned for the 16-byte path. */
int paradis_channel_norm_bwd(const float* gy, const float* x1, const float* x2, const float* w,
                             const float* mean, const float* rstd, float* gx1, float* gx2,
                             float* gw, float* gb, int B, int C1, int C2, int P,
                             int64_t x1_bs, int64_t x2_bs, int64_t gx1_bs, int64_t gx2_bs,
                             const float* addend1, int64_t add1_bs, void* workspace, void* stream);

/* ---- a9: GlobalBias map (reference model/blocks.py:188-196).
 * m8[Cin,H,W] = sum_r A[c,r] U[r,h] V[r,w];  map[Co,H,W] = Pw[Co,Cin] m8 (or map = m8 if Pw NULL). */
int paradis_global_bias_map_fwd(const float* A, const float* U, const float* V, const float* Pw,
                                float* m8, float* map, int Cin, int Co, int R, int H, int W, void* stream);
size_t paradis_global_bias_map_bwd_ws_bytes(int Cin, int Co, int R, int H, int W);
int paradis_global_bias_map_bwd(const float* gmap, const float* A, const float* U, const float* V,
                                const float* Pw, const float* m8, float* gA, float* gU, float* gV,
                                float* gPw, int Cin, int Co, int R, int H, int W,
                                void* workspace, void* stream);

/* GlobalBias in two stages, used when the projection is fused into the GEMM epilogue */
int paradis_global_bias_m8_fwd(const float* A, const float* U, const float* V, float* m8,
                               int Cin, int R, int H, int W, void* stream);
int paradis_global_bias_m8_bwd(const float* gm8, const float* A, const float* U, const float* V,
                               float* gA, float* gU, float* gV, int Cin, int R, int H, int W,
                               void* workspace, void* stream);
int paradis_global_bias_proj_bwd(const float* gmap, const float* m8, const float* Pw, float* gPw,
                                 float* gm8, int Cin, int Co, int64_t P, void* stream);

/* ---- elementwise / reductions used by the blocks */
int paradis_act_fwd(const float* x, float* y, int64_t n, int act, void* stream);
int paradis_act_bwd(const float* gy, const float* x, float* gx, int64_t n, int act, void* stream);
/* out = h + sigmoid(alpha[c]) * (adv - h)          (reference model/paradis.py:239,243) */
int paradis_gated_blend_fwd(const float* h, const float* adv, const float* alpha, float* out,
                            int B, int C, int P, void* stream);
size_t paradis_gated_blend_bwd_ws_bytes(int B, int C, int P);
int paradis_gated_blend_bwd(const float* gout, const float* h, const float* adv, const float* alpha,
                            float* gh, float* gadv, float* galpha, int B, int C, int P,
                            void* workspace, void* stream);
/* the same gradients from the blended OUTPUT instead of adv (the gated GEMM epilogue never writes adv):
 * galpha = (1 - sigmoid) sum gout (out - h)  (ABI 7) */
int paradis_gated_blend_bwd_out(const float* gout, const float* h, const float* out, const float* alpha,
                                float* gh, float* gadv, float* galpha, int B, int C, int P,
                                void* workspace, void* stream);
/* gmap[C,P] = sum_b dz[b,C,P] (NULL to skip), gbias[C] = sum_{b,p} dz (NULL to skip) */
int paradis_bias_grads(const float* dz, float* gmap, float* gbias, int B, int C, int P,
                       int64_t dz_bs, void* stream);
/* y = a + b (n elements) */
int paradis_add(const float* a, const float* b, float* y, int64_t n, void* stream);
/* out[cols,rows] = in[rows,cols]^T (weights for the LDS-DMA forward GEMM) */
int paradis_transpose(const float* in, float* out, int rows, int cols, void* stream);
/* y[b,i] = x[b,i] + m[i], i < per_sample  (standalone GlobalBias.forward, reference model/blocks.py:196) */
int paradis_add_bcast(const float* x, const float* m, float* y, int64_t per_sample, int B, void* stream);

/* ---- rows f1-f3 (callers around the model in the training step)
 * f1: ParadisLoss forward + gradient (reference utils/loss.py:233-282): loss[0] = mean(wf[c]*wl[h]*l(pred-target)),
 *     grad = d loss / d pred (for upstream gradient 1).  kind: 0 mse, 1 smooth reversed Huber.
 *     wl may be NULL; partial needs paradis_loss_blocks(total) floats. */
int paradis_loss_blocks(int64_t total);
int paradis_loss_fwd_bwd(const float* pred, const float* target, const float* wf, const float* wl,
                         float* loss, float* grad, float* partial, int B, int C, int H, int W,
                         int kind, float delta, void* stream);
/* y = x * scalar[0] (device scalar) */
int paradis_scale(const float* x, const float* scalar, float* y, int64_t n, void* stream);
/* f2: dst[b, 0:per_sample] = src[b, 0:per_sample] with different batch strides (channel-block copy used
 *     to assemble cat([input, forcings, constants]) and the next autoregressive input,
 *     reference trainer.py:534-538, 710-729) */
int paradis_copy_channels(const float* src, int64_t src_bs, float* dst, int64_t dst_bs, int B,
                          int64_t per_sample, void* stream);
/* f3: AdamW update of one tensor, torch.optim.AdamW operation order (reference trainer.py:327-335) */
int paradis_adamw_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1,
                       float beta2, float eps, float weight_decay, int step, void* stream);
/* The same update for a whole parameter group in one launch.  Device tables: ptrs[4][n_tensors]
 * (addresses of p, g, m, v as int64), numel[n_tensors], and one entry per chunk of
 * paradis_adamw_chunk() elements: chunk_tensor[n_chunks], chunk_off[n_chunks].
 * dev_state (optional, NULL = use `step` and `lr`): int32[2] on the device, [0] = step count, [1] = the bits of
 * the fp32 learning rate.  With it the bias corrections are formed on the device, so a HIP graph captured around
 * the training step (harness.GraphedTrainStep) stays valid from replay to replay; paradis_adamw_tick advances the
 * count on the stream (once per optimiser step, before the groups' updates). */
int paradis_adamw_chunk(void);
int paradis_adamw_multi(const int64_t* ptrs, const int64_t* numel, const int* chunk_tensor,
                        const int64_t* chunk_off, int n_tensors, int n_chunks, float lr, float beta1,
                        float beta2, float eps, float weight_decay, int step, const int* dev_state, void* stream);
int paradis_adamw_tick(int* dev_state, void* stream);
/* The same two updates with the hyper-parameters in double, as torch.optim.AdamW holds them (ABI 10): the coefficients
 * 1 - lr*weight_decay, 1 - beta1, 1 - beta2, lr / (1 - beta1^step) and sqrt(1 - beta2^step) are formed in double and
 * rounded to fp32 once - the scalars torch hands its fp32 kernels.  The float entry points above widen their arguments
 * and call these: with beta1 = 0.9f they update with 1 - beta1 = 0.10000002, 2.4e-7 off torch's 0.1f in m (and v). */
int paradis_adamw_step_d(float* p, const float* g, float* m, float* v, int64_t n, double lr, double beta1,
                         double beta2, double eps, double weight_decay, int step, void* stream);
int paradis_adamw_multi_d(const int64_t* ptrs, const int64_t* numel, const int* chunk_tensor,
                          const int64_t* chunk_off, int n_tensors, int n_chunks, double lr, double beta1,
                          double beta2, double eps, double weight_decay, int step, const int* dev_state, void* stream);
/* Learning-rate schedule on the device, one launch of one wavefront per optimiser step, behind the groups' ticks:
 * states = DEVICE table of n_groups addresses (int64; 0 = skip the group) of the int32[2] states above, table = DEVICE
 * fp32 [n_groups][n_steps].  With s = the group's already-ticked, 1-based step count:
 * state_g[1] = bits(table[g][min(s - 1, n_steps - 1)]) - past the end of the table its last entry holds.  A plain kernel
 * on `stream` (no host synchronisation, no copy or fill node): a captured training step walks the schedule by itself. */
int paradis_lr_schedule(const int64_t* states, const float* table, int n_groups, int n_steps, void* stream);

/* ---- f1 (AMSE): the spectral loss of reference utils/amse_loss.py on the equiangular grid H x W, W = 2(H-1), poles
 * included; row j of a plane is colatitude pi*j/(H-1) (RealSHT's order).  M = H-1 degrees / orders are used.
 * Tables (built once per grid and device): leg = paradis_amse_table_floats(H) floats, the quadrature-weighted
 * orthonormal Legendre functions times sqrt(4 pi) (fp64 recurrence, stored fp32) for l >= m, l < M; twiddle = W*2*(H-1)
 * floats; ws = paradis_amse_tables_ws_bytes(H) bytes of scratch. */
size_t paradis_amse_table_floats(int H);
size_t paradis_amse_tables_ws_bytes(int H);
int paradis_amse_tables(float* leg, float* twiddle, double* ws, int H, int W, void* stream);
/* loss[0] = AMSE(pred, target) over N = B*C planes [N,H,W] (mean over scales k < H-1, then over the planes); a NaN
 * result becomes 1e6 on the device.  grad (NULL to skip) = d loss / d pred for upstream gradient 1, all zero when the
 * value was NaN.  ws: paradis_amse_ws_bytes(N, H) bytes.  Fixed-order reductions: bit-reproducible. */
size_t paradis_amse_ws_bytes(int N, int H);
int paradis_amse_loss(const float* pred, const float* target, const float* leg, const float* twiddle, float* loss,
                      float* grad, void* ws, int N, int H, int W, void* stream);

/* ---- f3 (second half): Muon / NorMuon step on T same-shaped weight matrices w_t[rows, cols] (conv
 * weights flattened to [out, in*kh*kw]), the reference's default optimiser for Conv/Linear weights
 * (trainer.py:24-64,337-364; `dion` package, un-vendored and un-pinned: restated from its published
 * algorithm - momentum, Frobenius normalisation, 5 quintic Newton-Schulz iterations on the wide
 * orientation, NorMuon's per-neuron second-moment normalisation, decoupled weight decay).
 * ptrs: DEVICE table [4][table_stride] of addresses (int64) of w, g, m (momentum [rows*cols]) and
 * v (NorMuon per-row state [rows]); lr_adj: the shape-adjusted learning rate. */
size_t paradis_muon_ws_bytes(int T, int rows, int cols);
int paradis_muon_step(const int64_t* ptrs, int table_stride, int T, int rows, int cols, float lr,
                      float lr_adj, float mu, float beta2, float weight_decay, float eps, int nesterov,
                      int normuon, int split /* Newton-Schulz products on the bf16-split GEMM */,
                      void* workspace, void* stream);
/* The same step with the learning rate on the device.  dev_state (NULL = exactly paradis_muon_step, `lr_scale` unused):
 * the int32[2] state of paradis_adamw_multi_d, [1] = the bits of the fp32 learning rate.  The one kernel of the step
 * that uses the learning rate then reads lr = dev_state[1] and forms 1 - lr*weight_decay (fp32) and
 * lr_adj = (float)((double)lr * lr_scale) itself; `lr` and `lr_adj` are ignored, and nothing about the learning rate is
 * a launch constant (harness.GraphedTrainStep).  lr_scale: the shape factor of the adjusted learning rate - 1,
 * sqrt(fan_out / fan_in) or 0.2 sqrt(max(fan_out, fan_in)).  Agrees with the host-scalar entry to 1 ulp of the two
 * coefficients. */
int paradis_muon_step_d(const int64_t* ptrs, int table_stride, int T, int rows, int cols, float lr,
                        float lr_adj, float mu, float beta2, float weight_decay, float eps, int nesterov,
                        int normuon, int split, void* workspace, const int* dev_state, double lr_scale,
                        void* stream);
/* Plain batched GEMM C_b[M,N] = A_b[M,K] B_b[K,N] (row-major; AT = optional [K,M] transposes of A_b,
 * enabling the LDS-DMA kernel; split_ws = optional nbatch * paradis_pw_gemm_split_bytes(M,K,PARADIS_GEMM_BF16X3) bytes of
 * scratch selecting the bf16-split arithmetic) used by the Newton-Schulz iteration. */
int paradis_bgemm(const float* A, const float* AT, const float* B, float* C, int nbatch, int M, int K, int N,
                  int64_t a_bs, int64_t at_bs, int64_t b_bs, int64_t c_bs, void* split_ws, void* stream);

/* ---- f4: data feed on the device --------------------------------------------------------------
 * Forcings of B series of T consecutive timestamps each, every series as the dataset assembles one
 * sample (reference data/era5_dataset.py:587-621; data/forcings/time_vars.py:6-40;
 * data/forcings/toa_radiation.py:38-199):
 * out[B, T-n+1, H, W, n_vars*n] float32, out[b,s,y,x, v*n+k] = forcing v at time s+k of series b.
 * times_us: int64 microseconds since 1970-01-01 (numpy datetime64[us]); lat/lon in degrees (float64
 * storage; lat_is_f32 != 0 reproduces the float32 arithmetic numpy uses when the latitude array is
 * float32).  var_codes (HOST array): 0 toa_incident_solar_radiation (z-scored with toa_mean/std),
 * 1 sin_time_of_day, 2 cos_time_of_day, 3 sin_year_progress, 4 cos_year_progress. */
size_t paradis_forcings_ws_bytes(int B, int T);
int paradis_forcings(const int64_t* times_us /* [B,T] */, const double* lat_deg, const double* lon_deg,
                     int lat_is_f32, int B, int T, int H, int W, int n_time_inputs, const int* var_codes, int n_vars,
                     double toa_mean, double toa_std, float* out, void* workspace, void* stream);
/* Channels-last feature (de)normalisation in place (reference utils/normalization.py:6-80 as applied by
 * data/era5_dataset.py:547-584): data[rows, C]; kind[c]: 0 none, 1 z-score (p0 mean, p1 std),
 * 2 specific humidity (p0 q_min, p1 q_max, eps_q), 3 precipitation (shift 10, eps 1e-6). */
int paradis_normalize_features(float* data, const int* kind, const float* p0, const float* p1,
                               int64_t rows, int C, float eps_q, int inverse, void* stream);

/* Batch assembly from a device-resident store (reference data/era5_dataset.py:337-423 with the store held in HBM): ONE
 * launch writes the input and the target of B samples from store[T, F, H, W] (channels first, float32),
 *   input [b, 0, k*Fin + j] = norm(store[t_in(b) + k, feature(j)]),   k < n_time_inputs, j < Fin
 *   target[b, s, j]         = norm(store[t_in(b) + dt(s, j), feature(j)]),   s < S, j < Fout
 * with t_in(b) = base + idx[b] * interval_steps.  planes: DEVICE table of n_time_inputs*Fin + S*Fout entries, one per
 * output plane of a sample (the input's channels, then the target's, step-major): source feature, time offset from
 * t_in, and the kind / p0 / p1 of paradis_normalize_features, whose arithmetic the launch shares bit for bit.
 * idx: DEVICE int64 [B] (no host sync: the launch can be captured).  target == NULL: input only (the prediction-stage
 * item; the table's first n_time_inputs*Fin entries are used).  A time row or a feature outside the store is clamped
 * - nothing outside the store is ever read - and *flag (DEVICE int, owned by the caller, never cleared here) is set to
 * 1.  Float4 accesses when H*W % 4 == 0 and the three bases are 16-byte aligned, scalar otherwise.  Arguments are
 * checked before any HIP call; B == 0 does nothing.  paradis_assemble_batch_chunk(): values per workgroup. */
typedef struct {
  int32_t feature; /* row of the store's feature axis */
  int32_t dt;      /* time rows after t_in */
  int32_t kind;    /* 0 none, 1 z-score, 2 specific humidity, 3 precipitation */
  float p0, p1;    /* mean, std | q_min, q_max */
} paradis_plane_t;
int paradis_assemble_batch_chunk(void);
int paradis_assemble_batch(const float* store, int64_t T, int F, int H, int W, const int64_t* idx, int B, int64_t base,
                           int64_t interval_steps, const paradis_plane_t* planes, int n_time_inputs, int Fin, int S,
                           int Fout, float* input, float* target, float eps_q, int* flag, void* stream);

/* ---- The 16-bit packed store (ABI 10, additive), csrc/feed.hip: GRIB simple packing per plane.  A plane is one
 * (time, feature) field of P = H*W values.  domain [F] DEVICE int: 0 linear (y = x), 1 log (y = log(x + 1e-6), the
 * precipitation normalisation's shift; log and exp evaluated in double and rounded to float32 once).  lo, hi: minimum
 * and maximum of the plane's finite y; s = (hi - lo) / 65534 in float32.  Code 65535 is "missing": NaN and +-Inf are
 * stored so and decode to NaN (the float32 store passes Inf through).  Otherwise code = rint((y - lo) / s) clamped to
 * [0, 65534], 0 when s == 0; a plane without a finite value has lo = s = 0; a lo of -0 is stored as +0.  Decode:
 * y' = lo + s * (float)code, two fp32 roundings and no FMA; log domain: x' = max((float)exp(y') - 1e-6f, 0).
 * params: DEVICE float [T, F, 2] = (lo, s);  codes: DEVICE uint16 [T, F, H, W].
 *
 * paradis_pack_planes: slab [n, F, H, W] fp32 (dense) -> rows [row0, row0 + n) of codes and params.  Two launches: the
 * minimum / maximum of pieces of paradis_pack_planes_piece() values into ws (paradis_pack_planes_ws_bytes(n, F, H, W)
 * bytes, 4-byte aligned), then every workgroup folds its plane's partials and quantises its piece.  No atomics:
 * bit-identical run to run, and a slab packed in pieces equals the slab packed whole.  n == 0 does nothing.
 * Algorithmic HBM bytes: 10 per value (the slab is read twice).
 * paradis_unpack_planes: rows [a, b) decoded to out [b - a, F, H, W] fp32.  a == b does nothing.  6 B per value.
 * paradis_assemble_batch_packed: paradis_assemble_batch over a packed store - the same kernel over another element
 * reader, the same plane table, clamping, flag, B == 0 and target == NULL; the decode is the one of
 * paradis_unpack_planes, so its batch equals, bit for bit, paradis_assemble_batch over the unpacked rows.  6 B per value.
 * 16-byte stores fed by 8-byte loads of four codes when H*W % 4 == 0, codes are 8-byte and the outputs (pack: the
 * slab) 16-byte aligned; scalar otherwise, the same bits.  Every entry returns 1 before any HIP call for a bad shape,
 * rows outside [0, T], a missing pointer or a grid above the launch limit. */
int paradis_pack_planes_piece(void);
size_t paradis_pack_planes_ws_bytes(int n, int F, int H, int W);
int paradis_pack_planes(const float* slab, int n, int F, int H, int W, const int* domain, int64_t row0, int64_t T,
                        uint16_t* codes, float* params, void* ws, void* stream);
int paradis_unpack_planes(const uint16_t* codes, const float* params, const int* domain, int64_t T, int F, int H, int W,
                          int64_t a, int64_t b, float* out, void* stream);
int paradis_assemble_batch_packed(const uint16_t* codes, const float* params, const int* domain, int64_t T, int F,
                                  int H, int W, const int64_t* idx, int B, int64_t base, int64_t interval_steps,
                                  const paradis_plane_t* planes, int n_time_inputs, int Fin, int S, int Fout,
                                  float* input, float* target, float eps_q, int* flag, void* stream);

/* ---- f5: forecast post-processing (reference trainer.py:772-778 = utils/postprocessing.py:190-215 de-normalisation
 * + utils/postprocessing.py:74-122,143-187 Cartesian -> spherical winds, and the dew-point depression of
 * utils/mhuaes.py:33-96 that utils/file_output.py:165-173 derives - all on the CPU there).  One pass: reads the
 * normalised model output [B, C, H, W] (batch stride out_bs elements; never written) and writes the physical-unit
 * state to chunk + chunk_off with batch stride chunk_bs (slot t of a [B, T, C, H, W] chunk: chunk_off = t*C*H*W),
 * optionally the dew-point depression to dew + dew_off ([B, T, L, H, W]: dew_off = t*L*H*W; NULL to skip).
 * DEVICE tables: kind / p0 / p1 [C] with the codes of the feature normalisation below; units [n_units][8] int =
 * {type, q, T, x, y, z, level, 0}: type 0 one channel (its index in the q field), 1 a pressure level (channel indices
 * of specific humidity - or -1 -, temperature, wind_x / wind_y / wind_z - x = -1: no wind conversion - and the level's
 * index into plev), 2 the 10 m wind triple (x, y, z); every channel belongs to exactly one unit.  plev [n_levels]
 * double, hPa.  trig: double sin(lat)[H], cos(lat)[H], sin(lon)[W], cos(lon)[W].  fp32 de-normalisation in the
 * reference's operation order; winds and dew point in fp64, rounded once.  W % 4 == 0 and 16-byte aligned planes take
 * the 16-byte path, anything else a scalar one with the same arithmetic.
 * Algorithmic HBM bytes: 8*B*C*H*W (+ 4*B*L*H*W with the dew point). */
int paradis_forecast_post(const float* output, int64_t out_bs, float* chunk, int64_t chunk_bs, int64_t chunk_off,
                          float* dew, int64_t dew_bs, int64_t dew_off, const int* kind, const float* p0,
                          const float* p1, float eps_q, const int* units, int n_units, const double* plev,
                          int n_levels, const double* trig, int B, int C, int H, int W, void* stream);

/* ---- f5, the writer's layout (ABI 10, additive): a flushed chunk [B, n, C, H, W] (batch / time strides chunk_bs /
 * chunk_ts in elements, dense [C, H, W] states: a trailing partial chunk is a dense view of a larger buffer) and its
 * dew-point chunk [B, n, L, H, W] (dew_bs / dew_ts; NULL: none) regrouped into the named variables the reference's
 * writer builds (utils/file_output.py:66-175) and passed through BitRound(keepbits) (utils/file_output.py:18-24), in
 * ONE launch on `stream`: no host synchronisation, no memset or copy nodes; neither source is written.
 *   out: one buffer of out_elems floats.  Variable v owns the contiguous block [B, n_td, L_v, H, W]; the blocks follow
 *   one another in table order.  The launch writes time slots [td_off, td_off + n) of every block and nothing else.
 *   planes: DEVICE table, one row per output plane of a (sample, time slot); planes_host: the same rows in host memory,
 *   checked against C, L and out_elems before any HIP call.  A row's plane lands at element
 *     (first * B * n_td + (b * n_td + td_off + t) * levels + level) * H * W.
 *   keepbits 1 .. 23 on the float32 bit pattern, in 32-bit unsigned arithmetic, for any input (NaN, infinities):
 *     m = 23 - keepbits;  bits += ((bits >> m) & 1) + ((1 << (m - 1)) - 1);  bits &= 0xFFFFFFFF << m
 *   (numcodecs' published BitRound.encode restated; not pinned against the package).  keepbits 23, or 0 (the filter
 *   off), copies the bits unchanged.
 * rc 1 before any HIP call for: keepbits outside 0 .. 23, td_off + n > n_td, strides shorter than a state (or than the
 * n states of a sample), a NULL table, a row outside the sources or the buffer.  B == 0 does nothing.
 * 16-byte accesses when H*W % 4 == 0 and every base and stride keeps 16-byte alignment, scalar ones otherwise: the
 * same bits either way.  Algorithmic HBM bytes: 8 * B * n * n_planes * H * W. */
typedef struct {
  int32_t src;    /* >= 0: channel of the chunk; < 0: level (-1 - src) of the dew-point chunk */
  int32_t first;  /* planes per (sample, time slot) of the variables in front of this plane's variable */
  int32_t levels; /* L_v: the levels of this plane's variable (1 for a surface variable) */
  int32_t level;  /* this plane's level within its variable */
} paradis_encode_plane_t;
int paradis_forecast_encode(const float* chunk, int64_t chunk_bs, int64_t chunk_ts, const float* dew, int64_t dew_bs,
                            int64_t dew_ts, const paradis_encode_plane_t* planes,
                            const paradis_encode_plane_t* planes_host, int n_planes, float* out, int64_t out_elems,
                            int B, int n, int C, int L, int H, int W, int n_td, int td_off, int keepbits, void* stream);

/* ---- validation scores (reference trainer.py:652-708, _get_report_rmse trainer.py:291-315, per-channel loss
 * utils/loss.py:105-127).  One pass over pred and target [B, C, H, W] fp32 (batch strides pred_bs / target_bs in
 * elements, dense states; neither is written) and a finishing kernel that combines the per-workgroup partials in
 * double, in a fixed order (no atomics: bit-identical run to run), into the fp32 row out[1 + 2C + R]:
 *   out[0]           mean_c(wf[c] * s[c] / N), s = sum wl[h] l(e) with wl, else sum l(e); e = pred - target; N = B*H*W
 *   out[1 .. C]      wf[c] * s[c] / N                        out[1+C .. 2C]   sum l(e) / N   (unweighted)
 *   out[1+2C+r]      sqrt(sum lat_w[h] d^2 / N) of channel rep_chan[r], d in physical units by rep_class[r]:
 *                    1 z-score (target - pred) * p1, 2 specific humidity and 3 precipitation the difference of the two
 *                    de-normalised values (codes, p0 = q_min, p1 = std | q_max as paradis_normalize_features;
 *                    eps 1e-12 and shift 10 / eps 1e-6 as the reference's defaults)
 * kind: 0 mse, 1 smooth reversed Huber (threshold delta) as paradis_loss_fwd_bwd, 2 none: out[0 .. 2C] are zeros and
 * only report channels are read.  DEVICE tables: wf [C]; wl [H] or NULL; lat_w [H] (NULL allowed when R == 0);
 * per channel rflag [C] (>= 0 a report channel, -1 none), rcls / rp0 / rp1 [C] (read where rflag >= 0); rchan [R].
 * HOST arrays rep_chan / rep_class [R]: the same report list, checked here before anything is launched.
 * workspace: paradis_val_score_ws_bytes(B, C, H, W) bytes.  B == 0 does nothing.
 * W % 4 == 0 with 16-byte aligned planes takes 16-byte loads, anything else scalar loads: the same bits either way.
 * Algorithmic HBM bytes: 8*B*C*H*W. */
size_t paradis_val_score_ws_bytes(int B, int C, int H, int W);
int paradis_val_score(const float* pred, int64_t pred_bs, const float* target, int64_t target_bs, const float* wf,
                      const float* wl, const float* lat_w, int kind, float delta, const int* rep_chan,
                      const int* rep_class, int R, const int* rflag, const int* rcls, const float* rp0,
                      const float* rp1, const int* rchan, float* out, void* workspace, int B, int C, int H, int W,
                      void* stream);

/* ---- training diagnostics: per-group parameter / gradient / first-moment statistics (reference
 * on_before_optimizer_step, trainer.py:844-923).  Two launches on `stream`, no host synchronisation, no atomics
 * (bit-identical run to run).  Tables as paradis_adamw_multi_d: workgroup c reads at most paradis_param_stats_chunk()
 * elements of tensor chunk_tensor[c] from element chunk_off[c]; ptrs [3][n_tensors] holds the fp32 parameter, gradient
 * and first-moment addresses, a gradient or moment address of 0 means absent (a moment without a gradient is not read).
 * The chunk table is sorted by group: the chunks of group g are group_first_chunk[g] .. group_first_chunk[g + 1] - 1
 * (int32 [n_groups + 1], DEVICE; all other tables DEVICE too).  Sums are accumulated in double.
 *   out [(n_groups + 1) * 8] fp32, row g = {sum p^2, sum g^2, sum g.m, sum m^2, grad norm sqrt(sum g^2),
 *       gradratio = grad norm / pnorm, pnorm = max(sqrt(sum p^2), 1e-12),
 *       alignment = sum g.m / (sqrt(sum g^2) sqrt(sum m^2) + 1e-12), 0 where sum m^2 = 0};
 *   g.m and m^2 only over tensors with both a gradient and a moment; row n_groups: the same from the sums over all groups.
 * workspace: paradis_param_stats_ws_bytes(n_chunks) bytes (four doubles per chunk), 8-byte aligned.
 * n_chunks == 0 still writes out (zero sums, pnorm 1e-12); n_groups == 0 does nothing; at most 1024 groups.
 * 16-byte loads where every present tensor's chunk start is 16-byte aligned, scalar loads otherwise: the same bits.
 * Algorithmic HBM bytes: 12 per element with all three tensors present. */
int paradis_param_stats_chunk(void);
size_t paradis_param_stats_ws_bytes(int n_chunks);
int paradis_param_stats(const int64_t* ptrs, const int64_t* numel, const int* chunk_tensor, const int64_t* chunk_off,
                        const int* group_first_chunk, int n_tensors, int n_chunks, int n_groups, void* workspace,
                        float* out, void* stream);

/* ---- global-norm gradient clipping over many tensors (ABI 10, additive): torch.nn.utils.clip_grad_norm_(params,
 * max_norm, norm_type=2.0, error_if_nonfinite=False) - the reference's training.gradient_clip_val, train.py:52-53 - with
 * fewer roundings.  At most three launches on `stream` (chunk partials, one finishing workgroup, scale), no host
 * synchronisation, no memset or copy nodes, no atomics (bit-identical run to run).  Tables as paradis_adamw_multi_d:
 * workgroup c works on at most paradis_clip_grad_chunk() elements of tensor chunk_tensor[c] from element chunk_off[c];
 * grads [n_tensors] holds the addresses of the fp32 gradients, 0 = absent (neither read nor written); a table entry out
 * of range reads nothing.  All tables DEVICE.
 *   S = sum of g^2 over all present tensors, accumulated in double (an fp32 x fp32 product is exact in fp64);
 *   out[0] = (float)sqrt(S);  c = max_norm / (sqrt(S) + 1e-6) in double;  out[1] = (float)(c < 1 ? c : (c is NaN ? c : 1));
 *   every present gradient becomes g * out[1] in place, one fp32 multiply (skipped where out[1] is exactly 1.0f).
 * A NaN gradient element gives out = {NaN, NaN} and all-NaN gradients, as torch does.
 * max_norm must be finite and > 0 (rc 1 before any HIP call otherwise).  out: DEVICE fp32 [2].
 * workspace: paradis_clip_grad_ws_bytes(n_chunks) bytes (one double per chunk), 8-byte aligned.
 * n_chunks == 0 still writes out = {0, 1}.
 * 16-byte loads and stores where a chunk start is 16-byte aligned, scalar otherwise: the same bits either way.
 * Algorithmic HBM bytes: 4 per element (norm pass) + 8 per element (scale pass, when it clips). */
int paradis_clip_grad_chunk(void);
size_t paradis_clip_grad_ws_bytes(int n_chunks);
int paradis_clip_grad_norm(const int64_t* grads, const int64_t* numel, const int* chunk_tensor, const int64_t* chunk_off,
                           int n_tensors, int n_chunks, double max_norm, void* workspace, float* out, void* stream);

/* ---- forecast verification (ABI 10, additive): latitude-weighted RMSE, bias, MAE, anomaly correlation and activity
 * per (lead, channel), WeatherBench-2's conventions.  One launch pair on `stream`, no host synchronisation, no memset or
 * copy nodes, no atomics (bit-identical run to run); neither input is written.
 *   fc, truth [B, C, H, W] fp32 in physical units, dense [C, H, W] states, batch strides fc_bs / truth_bs in elements;
 *   lat_w [H] fp32 >= 0 (DEVICE);  Z = W * sum_h lat_w[h], formed in double by the caller;
 *   clim [K, C, H, W] fp32 dense and clim_index [B] int32 (DEVICE, 0 <= k < K: the slot of sample b; a slot out of
 *   range is not read and turns the sums of its sample into NaN), or both NULL.
 * Per sample b and channel c over the plane, w = lat_w[h], fa = f - clim[k[b]], ta = t - clim[k[b]]:
 *   se = sum w (f-t)^2 / Z,  e = sum w (f-t) / Z,  ae = sum w |f-t| / Z,
 *   ff = sum w fa^2,  tt = sum w ta^2,  ft = sum w fa ta,  acc_b = ft / sqrt(ff tt)
 *   acc[c][0..7] += {1, se, e, ae, acc_b, 1, ff, tt}     (acc_b and its 1 are left out when ff tt == 0)
 * acc: DEVICE double [C][8], the row of this lead, read and written by an ordinary read-modify-write (calls on one
 * stream are ordered); without a climatology entries 4 .. 7 are not touched.  Non-finite inputs are not masked.
 * Sums: fp32 per thread over at most paradis_verify_piece() / 256 cells, double from there on, in a fixed order.
 * ws: paradis_verify_ws_bytes(B, C, H, W, with_clim) bytes, 8-byte aligned: double [6 with a climatology, else 3]
 * [B*C][ceil(H*W / paradis_verify_piece())].  B == 0 does nothing.  rc 1 before any HIP call for: clim without
 * clim_index or the reverse, C / H / W < 1, K < 1 with a climatology, Z <= 0 or non-finite, a NULL acc or ws, a grid
 * above the launch limit.
 * W % 4 == 0 with 16-byte aligned planes takes 16-byte loads, anything else scalar loads: the same bits either way.
 * Algorithmic HBM bytes: 12*B*C*H*W with a climatology, 8*B*C*H*W without. */
int paradis_verify_piece(void);
size_t paradis_verify_ws_bytes(int B, int C, int H, int W, int with_clim);
int paradis_verify_update(const float* fc, int64_t fc_bs, const float* truth, int64_t truth_bs, const float* clim,
                          const int* clim_index, int K, const float* lat_w, double Z, double* acc, void* ws, int B,
                          int C, int H, int W, void* stream);

/* ---- Store preparation (reference scripts/preprocess_dataset.py: compute_statistics :409-479,
 * compute_tendency_statistics :482-590, compute_cartesian_wind :42-105), csrc/prepare.hip.
 *
 * paradis_store_stats: one pass over a slab x [T, F, H, W] fp32 (dense) that merges into a running accumulator, per
 * feature and over every non-NaN value (skipna=True: NaN is skipped, nothing else),
 *   {n, sum (x - pivot), sum (x - pivot)^2, min, max}                               into set field_set (>= 0), and / or
 *   the same five of d = x[t] - x[t - stride] (float32 difference, pivot 0, NaN d skipped) into set tend_set (>= 0);
 * -1 leaves a set out.  A pair is counted with its later row, t = 0 .. T - 1; rows t - stride < 0 are the LAST rows of
 * prev [n_prev, F, H, W] (the rows seen before x; NULL / 0: none), pairs reaching further back are not counted.
 *   acc: DEVICE double [F][n_sets + 1][5].  Sets 0 .. n_sets - 1 hold the five quantities; the caller initialises them
 *   to {0, 0, 0, +inf, -inf}.  Row n_sets of a feature is {pivot, pivot_is_set, 0, 0, 0}, initialised to zeros: the
 *   first call with a field set stores the first non-NaN cell (index order) of plane f of row 0 there, 0 if it has
 *   none, and every later call uses that value.  Read and written by ordinary accesses (calls on one stream are ordered).
 * Everything after the fp32 load / difference is double; sums in a fixed order (csrc/stream_common.h), no atomics:
 * bit-identical run to run for a given partition into slabs.  Three launches whatever T and F are; the workgroup
 * count stays near 4096 + F * ceil(H*W / paradis_store_stats_piece()).
 * ws: paradis_store_stats_ws_bytes(T, F, H, W) bytes, 8-byte aligned.  T == 0 does nothing.  rc 1 before any HIP call
 * for: F / H / W < 1, a set outside [-1, n_sets), both sets -1 or equal, stride < 1 with a tendency, n_prev > 0 without
 * prev, a NULL x / acc / ws, a grid above the launch limit.
 * H*W % 4 == 0 with 16-byte aligned x and prev takes 16-byte loads, anything else scalar loads: the same bits.
 * Algorithmic HBM bytes: 4*T*F*H*W for the field alone or with the tendency of stride 1 (the row just read stays in
 * registers), 8*T*F*H*W with a longer stride or for a tendency alone.
 *
 * paradis_cartesian_winds: dst[t, row.dst_x / y / z] = Cartesian wind of src[t, row.src_u / v / w / t] for every table
 * row and t < T in one launch; src [T, Fs, H, W], dst [T, Fd, H, W] fp32 dense, possibly the same tensor provided no
 * row's destination is another row's source.  src_w = src_t = -1: a surface row (dr/dt = 0).  With k = (float32)(omega *
 * 287.05 * T) / (level_hpa * 100 * 9.80616):
 *   x = -u sin(lon) - v sin(lat) cos(lon) - k cos(lat) cos(lon)
 *   y =  u cos(lon) - v sin(lat) sin(lon) - k cos(lat) sin(lon)
 *   z =  v cos(lat) - k sin(lat)
 * in double from the fp32 fields and trig = double [sin(lat)[H], cos(lat)[H], sin(lon)[W], cos(lon)[W]] (DEVICE, built
 * on the host), rounded to fp32 once: what numpy gives the reference for float32 fields and float64 grids.  rows: DEVICE
 * table; rows_host: the same table in host memory, checked (columns inside [0, Fs) / [0, Fd), level > 0) before any
 * HIP call.  W % 4 == 0 with 16-byte aligned bases takes 16-byte accesses.  T == 0 or n_rows == 0 does nothing.
 * Algorithmic HBM bytes per cell: 28 for a level row, 20 for a surface row. */
typedef struct {
  int32_t src_u, src_v, src_w, src_t; /* columns of src: u, v, omega (Pa/s), temperature; src_w = src_t = -1: surface */
  int32_t dst_x, dst_y, dst_z;        /* columns of dst */
  float level_hpa;                    /* pressure level in hPa (unused for a surface row) */
} paradis_wind_row_t;
int paradis_store_stats_piece(void);
size_t paradis_store_stats_ws_bytes(int T, int F, int H, int W);
int paradis_store_stats(const float* x, int T, const float* prev, int n_prev, int F, int H, int W, int field_set,
                        int tend_set, int stride, double* acc, int n_sets, void* ws, void* stream);
int paradis_cartesian_winds(const float* src, int Fs, float* dst, int Fd, const paradis_wind_row_t* rows,
                            const paradis_wind_row_t* rows_host, int n_rows, const double* trig, int T, int H, int W,
                            void* stream);

/* ---- The verification climatology of a device-resident store (ABI 10, additive), csrc/climatology.hip: the slot means
 * that paradis_verify_update reads as clim [K, C, H, W].  The project's own windowed day-of-year x hour definition
 * (climatology.ClimPlan builds the lists on the host); not pinned against WeatherBench-2.
 *
 * paradis_clim_mean / paradis_clim_mean_packed: the store [T, F, H, W] as paradis_assemble_batch /
 * paradis_assemble_batch_packed take it (never written).  CSR lists, all DEVICE: ptr int64 [K + 1], rows int64 [N],
 * w double [N]; cols int32 [C]: the store feature column of output channel c.  For slot k, channel c and pixel p, over
 * the entries j in [ptr[k], ptr[k + 1]) whose value x[rows[j], cols[c], p] is finite (NaN and +-Inf are skipped per
 * pixel; a packed store decodes "missing" to NaN):
 *   S = sum_j w[j] * x,  Wt = sum_j w[j],  out[k, c, p] = (float)(S / Wt), NaN when Wt == 0
 * S and Wt in double, in list order: no atomics, no zero fill, bit-identical run to run.  A row outside [0, T), a column
 * outside [0, F) or a list bound outside [0, N] is CLAMPED (never read outside) and reported through *flag (DEVICE int,
 * set to 1, never cleared).  One workgroup owns paradis_clim_mean_chunk() values of one (slot, channel) plane; when K * C
 * * chunks exceeds the launch limit the slots are split over several launches.  K == 0 or C == 0 does nothing.
 * rc 1 before any HIP call for a bad shape, a missing pointer, N < 0, or C * chunks above the launch limit.
 * H*W % 4 == 0 with a 16-byte aligned out and a 16-byte (float32) / 8-byte (packed) aligned store takes 16 B / 8 B
 * loads, anything else scalar loads with the same arithmetic per cell: the same bits either way.
 * Algorithmic HBM bytes: N*C*H*W*(4 | 2) read + 4*K*C*H*W written.
 *
 * paradis_spherical_winds_inplace: the (x, y, z) planes of every wind triple of data [K, C, H, W] (fp32, dense) become
 * (u, v, w), in place, by the expression of paradis_forecast_post (csrc/winds.h: one copy, the same bits).  units
 * [n_units][8] int, plev and trig as paradis_forecast_post takes them; units_host: the same rows in host memory, checked
 * (channels inside [0, C), levels inside [0, n_levels)) before any HIP call.  Rows of type 0 and level rows with x = -1
 * are skipped; a level row reads its temperature channel (w = dr/dt * p g / (R T)).  A NaN in any of the three
 * components gives NaN in all three.  K == 0 or n_units == 0 does nothing.
 * Algorithmic HBM bytes per cell: 28 for a level row, 24 for the 10 m row. */
int paradis_clim_mean_chunk(void);
int paradis_clim_mean(const float* store, int64_t T, int F, int H, int W, const int64_t* ptr, const int64_t* rows,
                      const double* w, int64_t N, int K, const int* cols, int C, float* out, int* flag, void* stream);
int paradis_clim_mean_packed(const uint16_t* codes, const float* params, const int* domain, int64_t T, int F, int H,
                             int W, const int64_t* ptr, const int64_t* rows, const double* w, int64_t N, int K,
                             const int* cols, int C, float* out, int* flag, void* stream);
int paradis_spherical_winds_inplace(float* data, const int* units, const int* units_host, int n_units,
                                    const double* plev, int n_levels, const double* trig, int K, int C, int H, int W,
                                    void* stream);

/* ---- The quantile climatology of a device-resident store (ABI 10, additive), csrc/quantile.hip: per slot, channel and
 * cell the quantiles of the rows that a slot's list names - per-cell thresholds for the event tables (an anomaly source
 * against a quantile field at threshold 0 decides x >= q).  The project's own definition; not pinned against any package.
 *
 * Store, ptr, rows, cols and flag as paradis_clim_mean takes them (no weights: quantiles are unweighted).  For slot k,
 * channel c and cell p: the values x[rows[j], cols[c], p], j in [ptr[k], ptr[k + 1]), -0.0 read as +0.0, NaN and +-Inf
 * skipped; m of them are kept, v[0] <= .. <= v[m-1] ascending.  For each of the Q levels q_host[i] in [0, 1] (HOST
 * doubles, Q <= 8, checked on the host and passed as kernel arguments):
 *   pos = q * (m - 1),  lo = floor(pos),  hi = min(lo + 1, m - 1),  frac = pos - lo
 *   out[i, k, c, p] = (float)(v[lo] + (v[hi] - v[lo]) * frac)     in double, uncontracted, one rounding
 *   out[i, k, c, p] = NaN when m < min_count (min_count >= 1)
 * numpy's method="linear" position rule with the plain lerp.  out is [Q, K, C, H*W].
 * max_entries: the longest list (0 .. paradis_clim_quantile_max_entries() = 4096); it fixes the tile: one workgroup
 * owns paradis_clim_quantile_cells(max_entries) adjacent cells of one (slot, channel) plane, their keys in LDS, sorted
 * there.  A list longer than max_entries is CLAMPED to its first max_entries entries and reported through *flag, as a
 * row, column or list bound outside the store is.  No atomics, no zero fill: bit-identical run to run.  K == 0, C == 0
 * or Q == 0 does nothing.  rc 1 before any HIP call for a bad shape, a missing pointer, N < 0, Q > 8, a level outside
 * [0, 1], max_entries outside its range, min_count < 1, or C * tiles above the launch limit.
 * H*W % 4 == 0 with a 16-byte (float32) / 8-byte (packed) aligned store takes 16 B / 8 B loads, anything else scalar
 * loads: the same bits either way.
 * Algorithmic HBM bytes: N*C*H*W*(4 | 2) read + 4*Q*K*C*H*W written. */
int paradis_clim_quantile_max_entries(void);
int paradis_clim_quantile_cells(int max_entries);
int paradis_clim_quantile(const float* store, int64_t T, int F, int H, int W, const int64_t* ptr, const int64_t* rows,
                          int64_t N, int K, int max_entries, const int* cols, int C, const double* q_host, int Q,
                          int min_count, float* out, int* flag, void* stream);
int paradis_clim_quantile_packed(const uint16_t* codes, const float* params, const int* domain, int64_t T, int F, int H,
                                 int W, const int64_t* ptr, const int64_t* rows, int64_t N, int K, int max_entries,
                                 const int* cols, int C, const double* q_host, int Q, int min_count, float* out,
                                 int* flag, void* stream);

/* ---- The SEEPS climatology (ABI 10, additive), csrc/quantile.hip: the same store, lists, tile, clamp flag and sort as
 * paradis_clim_quantile, with another stage behind the sort.  The project's own restatement of the climatology of
 * Rodwell et al. (2010); not pinned against any package.  With the m kept values v[0] <= .. <= v[m-1] of a cell, dry a
 * finite float32 and wet_level a double in [0, 1] (both HOST values):
 *   n_dry = #{ v[i] < dry }   (strict; -0.0 is +0.0 on both sides),   n_wet = m - n_dry
 *   p1  = (float)((double)n_dry / (double)m)                                       NaN when m < min_count
 *   pos = wet_level * (n_wet - 1),  lo = floor(pos),  hi = min(lo + 1, n_wet - 1),  frac = pos - lo
 *   thr = (float)(v[n_dry + lo] + (v[n_dry + hi] - v[n_dry + lo]) * frac)          in double, uncontracted, one rounding;
 *                                                                                  NaN when n_wet < 1 or m < min_count
 * out is [2, K, C, H*W]: plane 0 p1, plane 1 thr.  K == 0 or C == 0 does nothing.  rc 1 before any HIP call for what
 * paradis_clim_quantile refuses, a dry that is not finite and a wet_level outside [0, 1].
 * Algorithmic HBM bytes: N*C*H*W*(4 | 2) read + 8*K*C*H*W written. */
int paradis_clim_seeps(const float* store, int64_t T, int F, int H, int W, const int64_t* ptr, const int64_t* rows,
                       int64_t N, int K, int max_entries, const int* cols, int C, float dry, double wet_level,
                       int min_count, float* out, int* flag, void* stream);
int paradis_clim_seeps_packed(const uint16_t* codes, const float* params, const int* domain, int64_t T, int F, int H,
                              int W, const int64_t* ptr, const int64_t* rows, int64_t N, int K, int max_entries,
                              const int* cols, int C, float dry, double wet_level, int min_count, float* out, int* flag,
                              void* stream);

/* ---- Zonal power spectra of forecast and truth (ABI 10, additive), csrc/spectrum.hip: at which scales a forecast has
 * gone wrong.  The project's own definition, in the spirit of WeatherBench-2's ZonalEnergySpectrum; not pinned against it.
 * One launch pair on `stream`, no host synchronisation, no memset or copy nodes, no atomics (bit-identical run to run);
 * neither input is written.
 *   fc, truth [B, C, H, W] fp32 in physical units, dense [C, H, W] states, batch strides fc_bs / truth_bs in elements;
 *   channels int32 [Cs] (DEVICE): the plane of output channel cs (only these planes are read; an entry outside [0, C)
 *   is not read and turns its sums into NaN), or NULL with Cs == C;
 *   band_w double [R][H] >= 0 (DEVICE), band_wsum double [R] = sum_h band_w[r][h] > 0 (DEVICE, formed by the caller);
 *   twiddle float [W][2] (DEVICE) = exp(-2 pi i j / W), j < W, computed in double by the caller and rounded once.
 * Per row h, W even, K = W / 2, k = 0 .. K, m_k = 1 for k in {0, K}, else 2:
 *   X[h,k] = (1/W) sum_i x[h,i] exp(-2 pi i k i / W),  pf = m_k |F|^2,  pt = m_k |T|^2,  co = m_k Re(F conj T)
 *   S[r,k] = sum_h band_w[r][h] p[h,k] / band_wsum[r] over the rows with band_w[r][h] != 0 (a row of weight 0 is left
 *   out, not multiplied in; a row of weight 0 in every band is neither read nor transformed)
 *   acc[cs][r][k][0..2] += {S_ff, S_tt, S_ft} per sample in b order, the row groups of a sample in index order;
 *   count[0] += B.  Two calls of B samples give the bits of one call of the 2B batch.
 * acc: DEVICE double [Cs][R][K + 1][3] and count: DEVICE double [1], the rows of this lead, ordinary read-modify-write
 * (calls on one stream are ordered).  Non-finite inputs are not masked.
 * Forecast and truth rows go through ONE complex fp32 transform of z = (f - p) + i (t - p), p = truth[h][0] (restored
 * at k = 0 in double); everything after the transform is double.  paradis_spectrum_schedule(W): 1 = fft (W even, a
 * product of 2, 3 and 5, W <= paradis_spectrum_fft_max_w(): Stockham mixed radix in LDS), 2 = direct (any other even
 * W <= paradis_spectrum_direct_max_w(): an O(W^2) row DFT out of LDS, summed in double), 0 = refused.  A workgroup owns
 * paradis_spectrum_rows() rows of one plane.
 * ws: paradis_spectrum_ws_bytes(B, Cs, H, W, R) bytes, 8-byte aligned: double [B*Cs][ceil(H / paradis_spectrum_rows())]
 * [R][3][K + 1].  B == 0 does nothing.  rc 1 before any HIP call for: B < 0 or C / Cs / H / W < 1, a refused W, R outside
 * [1, 64] or more bands than the LDS holds at this W (24 * R * (K + 1) bytes beside the transform's buffers), channels
 * NULL with Cs != C, a NULL acc / count / ws / input, batch strides shorter than a state, a grid above the launch limit.
 * Algorithmic HBM bytes: 8 * B * Cs * H * W (less the rows of weight 0 in every band). */
int paradis_spectrum_rows(void);
int paradis_spectrum_fft_max_w(void);
int paradis_spectrum_direct_max_w(void);
int paradis_spectrum_schedule(int W);
size_t paradis_spectrum_ws_bytes(int B, int Cs, int H, int W, int R);
int paradis_spectrum_update(const float* fc, int64_t fc_bs, const float* truth, int64_t truth_bs, const int* channels,
                            int Cs, const double* band_w, const double* band_wsum, const float* twiddle, double* acc,
                            double* count, void* ws, int B, int C, int H, int W, int R, void* stream);

/* ---- Event verification (ABI 10, additive), csrc/events.hip: per lead, event source and latitude row the integer 2x2
 * contingency counts of "value beyond a threshold" in forecast against truth.  One launch pair on `stream`, no host
 * synchronisation, no memset or copy nodes, no atomics, no float arithmetic after the decision: the counts are exact.
 *   fc, truth [B, C, H, W] fp32 in physical units, dense [C, H, W] states, batch strides fc_bs / truth_bs in elements;
 *   clim [K, C, H, W] fp32 dense and clim_index [B] int32 (DEVICE), or both NULL;
 *   src_table HOST int32 [S][4] = {kind, c0, c1, nthr}: kind 0 plain x = v[c0]; 1 speed x = sqrtf(v[c0]^2 + v[c1]^2)
 *   (fp32: mul, mul, add, sqrt, uncontracted); 2 anomaly x = v[c0] - clim[clim_index[b]][c0] (one fp32 subtraction);
 *   thr_table HOST float [S][1 + paradis_events_max_thresholds()] = {sign, thr'[0 .. nthr)}: the event is
 *   sign * x >= thr'[j], sign = +1 or -1 ("x <= thr" is sign = -1, thr' = -thr).  Both tables are read on the host and
 *   travel as kernel arguments (a captured launch keeps their values); S <= paradis_events_max_sources().
 * A cell is valid for a source iff every value it reads is finite (forecast and truth, both components of a speed, the
 * climatology cell of an anomaly); a sample whose clim_index is outside [0, K) has no valid cell for anomaly sources
 * and nothing of that slot is read.  Invalid cells are counted in no class.
 *   acc_lead: DEVICE int64 [S][H][1 + 3 TMAX], the row of this lead: {nV, nF[TMAX], nO[TMAX], nFO[TMAX]} += the counts of
 *   valid cells, forecast events, truth events and joint events (entries past nthr stay as they are: += 0);
 *   n_samples_lead: DEVICE int64 [1] += B.  Ordinary read-modify-writes (calls on one stream are ordered).
 * A workgroup owns paradis_events_rows(W) ~ 8192 / W (>= 1) whole rows of one (sample, source); only the planes of the
 * sources are read.  ws: paradis_events_ws_bytes(B, S, H, W) bytes, 4-byte aligned: uint32 [B][S][H][1 + 3 TMAX].
 * B == 0 does nothing.  rc 1 before any HIP call for: B < 0, C / S / H / W < 1, S above the limit, H W >= 2^31 - 8192,
 * a grid above the launch limit, batch strides shorter than a state, clim without clim_index or the reverse, K < 1
 * with a climatology, an anomaly source without a climatology, a kind outside 0 .. 2, channels outside [0, C), nthr
 * outside [1, TMAX], a sign that is not +-1, a NULL acc_lead, n_samples_lead, ws or table.
 * W % 4 == 0 with 16-byte aligned bases and strides takes 16-byte loads, anything else scalar loads: the same counts.
 * Algorithmic HBM bytes per cell of a source: 8 plain, 16 speed, 12 anomaly. */
int paradis_events_max_thresholds(void);
int paradis_events_max_sources(void);
int paradis_events_rows(int W);
size_t paradis_events_ws_bytes(int B, int S, int H, int W);
int paradis_events_update(const float* fc, int64_t fc_bs, const float* truth, int64_t truth_bs, const float* clim,
                          const int* clim_index, int K, const int* src_table, const float* thr_table,
                          int64_t* acc_lead, int64_t* n_samples_lead, void* ws, int B, int C, int S, int H, int W,
                          void* stream);

/* ---- Neighbourhood verification (ABI 10, additive), csrc/fss.hip: the integer sums of the fractions skill score per
 * lead, event source, latitude row, scale and threshold.  Three launches on `stream` (the decision and the row counts;
 * the windows; the finish), no host synchronisation, no memset or copy nodes, no atomics, no float arithmetic after the
 * decision: the sums are exact.
 *   fc, truth, fc_bs, truth_bs, clim, clim_index, K_clim, src_table, thr_table: as paradis_events_update (K there),
 *   with its limits (paradis_events_max_sources(), paradis_events_max_thresholds() = TMAX) and its checks; the decided
 *   bits F[j], O[j] are those of events.hip, and an INVALID CELL IS A NON-EVENT in both fields;
 *   half_y HOST int32 [K]: the latitude half-width ny[k] of scale k in rows, 0 .. paradis_fss_max_half_y() (read on the
 *   host, travels as a kernel argument); K in 1 .. paradis_fss_max_scales() (K_MAX);
 *   half_x DEVICE int32 [K][H]: the longitude half-width nx[k][h] of the windows centred in row h, in cells.  It cannot
 *   be checked on the host: THE KERNEL CLAMPS every entry into [0, min(paradis_fss_max_half_x(), (W - 1) / 2)].
 * The window of centre cell (h, w) at scale k: rows max(0, h - ny) .. min(H - 1, h + ny) (clipped at the grid edge, no
 * over-the-pole wrap), columns w - nx .. w + nx modulo W; cF / cO: the F / O bits in it.
 *   acc_lead: DEVICE int64 [S][H][1 + 2 TMAX + 3 K_MAX TMAX], the row of this lead:
 *     [0] nV   [1 + j] nF[j]   [1 + TMAX + j] nO[j]                              (paradis_events_update's counts)
 *     [1 + 2 TMAX + 3 (k TMAX + j) + q]   q = 0: sum_w cF^2, 1: sum_w cO^2, 2: sum_w cF cO
 *   each += the sums of this call (entries past nthr or K: += 0 or untouched); n_samples_lead: DEVICE int64 [1] += B.
 * ws: paradis_fss_ws_bytes(B, S, H, W, K) bytes, 16-byte aligned: the decided bits uint16 [B][S][H][W], then uint64
 * partials [B][S][H][1 + 2 TMAX + 3 K TMAX].  A workgroup of the window kernel owns paradis_fss_rows(W, ny_max) centre
 * rows of one (sample, source, scale) (0 for a W or ny_max outside the limits) and reads 2 ny[k] halo rows of bits.
 * B == 0 does nothing.  rc 1 before any HIP call for everything paradis_events_update refuses, W above
 * paradis_fss_max_w(), K outside [1, K_MAX], a half_y entry outside its range, a NULL table, half_y or half_x, a ws that
 * is not 16-byte aligned.  W % 4 == 0 with 16-byte aligned bases and strides takes 16-byte loads, anything else scalar
 * loads: the same integers.  Algorithmic HBM bytes per cell of a source: 8 plain, 16 speed, 12 anomaly. */
int paradis_fss_max_scales(void);
int paradis_fss_max_half_y(void);
int paradis_fss_max_half_x(void);
int paradis_fss_max_w(void);
int paradis_fss_rows(int W, int ny_max);
size_t paradis_fss_ws_bytes(int B, int S, int H, int W, int K);
int paradis_fss_update(const float* fc, int64_t fc_bs, const float* truth, int64_t truth_bs, const float* clim,
                       const int* clim_index, int K_clim, const int* src_table, const float* thr_table,
                       const int* half_y, const int* half_x, int64_t* acc_lead, int64_t* n_samples_lead, void* ws,
                       int B, int C, int S, int H, int W, int K, void* stream);

/* ---- Ensemble verification (ABI 10, additive), csrc/ensemble.hip: per lead, chosen channel and latitude row the row
 * sums of the CRPS and spread / skill terms of M-member ensembles and the histogram of the truth's rank.  The project's
 * own textbook definitions in the spirit of WeatherBench-2's probabilistic metrics; not pinned against any package.  One
 * launch pair on `stream`, no host synchronisation, no memset or copy nodes, no atomics, no sort; neither input is
 * written.
 *   fc [G * M, C, H, W] fp32 in physical units, member-minor (member i of ensemble g is batch entry g M + i), dense
 *   [C, H, W] states, fc_bs the stride between members in elements; truth [G, C, H, W], truth_bs the stride between
 *   ensembles; 2 <= M <= paradis_ens_max_members();
 *   chan int32 [Cs] (DEVICE): the state channel of output channel cs - only these planes are read; an entry outside
 *   [0, C) is not read, adds 0 to its counters and turns its four sums into NaN;
 *   rM = 1.0f / M formed by the caller; salt: uint32, the caller's seed + lead.
 * A cell is valid iff its truth y and all M member values x_i are finite; an invalid cell adds nothing anywhere.  Per
 * valid cell, in fp32, uncontracted, in exactly this order:
 *   A = sum_i |x_i - y| (i ascending, from 0.0f)      P = sum_{i<j} |x_i - x_j| (i ascending, then j ascending)
 *   m = (sum_i x_i) * rM      E2 = (m - y) * (m - y)      V = sum_i (x_i - m) * (x_i - m)
 *   lo = #{x_i < y}   eq = #{x_i == y}   r = lo + hash32(key) % (eq + 1), the truth's rank in 0 .. M
 *   key = uint32(((n C + c) H + h) W + w) + salt * 0x9E3779B9 (mod 2^32), c = chan[cs], n = n_samples_lead[0] as the
 *   call finds it + g;  hash32(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16.
 *   acc_real_lead: DEVICE double [Cs][H][4], the rows of this lead: {sum A, sum P, sum E2, sum V} over the row's valid
 *   cells, each cell term widened to double before it meets another, summed in a fixed order; the ensembles are folded
 *   in g order, (acc + s_0) + s_1 ..: two calls give the bits of one call of the concatenated ensembles;
 *   acc_int_lead: DEVICE int64 [Cs][H][2 + M]: {nV, hist[0 .. M]} += the valid cells and the histogram of r (exact);
 *   n_samples_lead: DEVICE int64 [1] += G, read by the counting kernel before the finishing kernel adds to it.
 *   Ordinary read-modify-writes (calls on one stream are ordered).
 * A workgroup owns paradis_ens_rows(W, M) (>= 4; 0 for W < 1 or M outside its range) whole rows of one (ensemble,
 * channel).  ws: paradis_ens_ws_bytes(G, Cs, H, W, M) bytes, 8-byte aligned: double [G][Cs][H][4], then uint32
 * [G][Cs][H][2 + M].  G == 0 does nothing.  rc 1 before any HIP call for: G < 0, C / Cs / H / W < 1, M outside its range,
 * a NULL accumulator, ws or input, H W >= 2^31 - 8192, batch strides shorter than a state, a grid above the launch limit.
 * W % 4 == 0 with 16-byte aligned bases and strides takes one 16-byte load per plane and quad of cells (8-byte loads of
 * cell pairs above 16 members), anything else scalar loads: the same bits.
 * Algorithmic HBM bytes per cell of a channel: 4 (M + 1). */
int paradis_ens_max_members(void);
int paradis_ens_rows(int W, int M);
size_t paradis_ens_ws_bytes(int G, int Cs, int H, int W, int M);
int paradis_ens_update(const float* fc, int64_t fc_bs, const float* truth, int64_t truth_bs, const int* chan, float rM,
                       unsigned salt, double* acc_real_lead, int64_t* acc_int_lead, int64_t* n_samples_lead, void* ws,
                       int G, int M, int C, int Cs, int H, int W, void* stream);

/* ---- Probabilistic event verification (ABI 10, additive), csrc/probability.hip: per lead, event source, latitude row
 * and threshold the joint integer histogram of (the truth has the event, the number of members that have it) of M-member
 * ensembles - what the Brier score and its decomposition, the reliability diagram and the ROC curve are made of.  The
 * project's own textbook definitions; not pinned against any package.  One launch pair on `stream`, no host
 * synchronisation, no memset or copy nodes, no global atomics, no float arithmetic after the decision: the counts are
 * exact; neither input is written.
 *   fc [G * M, C, H, W] fp32 in physical units, member-minor (member i of ensemble g is batch entry g M + i), dense
 *   [C, H, W] states, fc_bs the stride between members in elements; truth [G, C, H, W], truth_bs the stride between
 *   ensembles; 2 <= M <= paradis_prob_max_members();
 *   clim [K, C, H, W] fp32 dense and clim_index [G] int32 (DEVICE), one slot per ensemble, or both NULL;
 *   src_table, thr_table: HOST tables as paradis_events_update's, with its limits (paradis_events_max_sources(),
 *   paradis_events_max_thresholds() = TMAX) and its checks; T in 1 .. TMAX: the thresholds an accumulator row has room
 *   for, at least every source's nthr.  The value of a source and the decision sign * x >= thr'[j] are those of
 *   paradis_events_update (csrc/event_source.h), for the truth and for each member.
 * A cell is valid for a source iff every value it reads is finite (the truth's channel or channels, the climatology cell
 * of an anomaly, the channel or channels of all M members); an ensemble whose clim_index is outside [0, K) has no valid
 * cell for anomaly sources and nothing of that slot is read.  Invalid cells are counted nowhere.  Per valid cell and
 * threshold j < nthr, o = the truth has the event (0 / 1), k = the members that have it (0 .. M).
 *   acc_lead: DEVICE int64 [S][H][paradis_prob_counters(M, T)], the row of this lead, counters = 1 + 2 T (M + 1):
 *     [0] nV      [1 + (2 j + o) (M + 1) + k] joint[j][o][k]
 *   each += the counts of this call (entries of j >= nthr: += 0); sum_{o,k} joint[j][o][k] == nV for every j < nthr;
 *   n_samples_lead: DEVICE int64 [1] += G.  Ordinary read-modify-writes (calls on one stream are ordered); the ensembles
 *   are folded in g order.
 * A workgroup owns paradis_prob_rows(W) ~ 1024 / W (a multiple of 4, >= 4; 0 for W < 1) whole rows of one (ensemble,
 * source) and a wave whole rows; the members are streamed with a runtime bound (one compiled kernel for every M), a row's counts are kept
 * in a per-wave LDS histogram.  ws: paradis_prob_ws_bytes(G, S, H, W, M, T) bytes, 4-byte aligned: uint32
 * [G][S][H][counters]; 0, like paradis_prob_counters, for an M or T outside its range or an empty shape.
 * G == 0 does nothing.  rc 1 before any HIP call for everything paradis_events_update refuses (B there is G), M or T
 * outside its range, a source with more than T thresholds, a NULL acc_lead, n_samples_lead, ws, input or table.
 * W % 4 == 0 with 16-byte aligned bases and strides takes 16-byte loads, anything else scalar loads: the same counts.
 * Algorithmic HBM bytes per cell of a source: 4 (M + 1) plain, 8 (M + 1) speed, 4 (M + 1) + 4 anomaly. */
int paradis_prob_max_members(void);
int paradis_prob_rows(int W);
int paradis_prob_counters(int M, int T);
size_t paradis_prob_ws_bytes(int G, int S, int H, int W, int M, int T);
int paradis_prob_update(const float* fc, int64_t fc_bs, const float* truth, int64_t truth_bs, const float* clim,
                        const int* clim_index, int K, const int* src_table, const float* thr_table, int64_t* acc_lead,
                        int64_t* n_samples_lead, void* ws, int G, int M, int T, int C, int S, int H, int W,
                        void* stream);

/* ---- SEEPS, the three-category precipitation score (ABI 10, additive), csrc/seeps.hip: per lead, chosen channel and
 * latitude row the 3x3 table of (forecast category, truth category), the masked cells and the row sums of the score
 * split by the truth's category.  The project's own restatement of Rodwell et al. (2010), in the spirit of
 * WeatherBench-2; not pinned against any package.  Three launches on `stream`, no host synchronisation, no memset or copy
 * nodes, no atomics; no input is written.
 *   fc / truth [B, C, H, W] fp32 in physical units, dense [C, H, W] states, fc_bs / truth_bs the batch strides in elements;
 *   p1 / thr: the two planes of a SEEPS climatology (paradis_clim_seeps), cell p of slot k and output channel cs at
 *   [k * clim_ks + cs * clim_cs + p] (strides in elements); clim_index int32 [B] (DEVICE): the slot of every sample;
 *   chan_host int32 [Cs] (HOST, Cs <= paradis_seeps_max_channels() = 8): the state channel of output channel cs, checked
 *   here and handed to the kernel as arguments - only these planes are read;
 *   dry: the dry threshold; 0 < p_lo <= p_hi < 1: the bounds of p1 (all fp32, compared in fp32).
 * cat(x) = 0 if x < dry, else 2 if x >= thr, else 1.  A cell is valid iff f, o, p1 and thr are finite, p_lo <= p1 <= p_hi
 * and the sample's slot is in [0, K); masked iff all four are finite and the slot is in range but p1 is outside the
 * bounds; anything else is counted nowhere, and nothing of an out-of-range slot is read.  Per valid cell, in double,
 * uncontracted, p = (double)p1:
 *   a = 1.0 / (1.0 - p),  b = 1.0 / p,  c = 3.0 / (2.0 + p)
 *   M[cf][co] = {{0, a, 4.0 * a}, {b, 0, 3.0 * a}, {b + c, c, 0}},   s = 0.5 * M[cat(f)][cat(o)]
 *   acc_real_lead: DEVICE double [Cs][H][3]: the sums of s over the row's valid cells whose truth is dry, light, heavy,
 *   summed in a fixed order; the samples are folded in b order, (acc + s_0) + s_1 ..: two calls give the bits of one
 *   call of the concatenated batch;
 *   acc_int_lead: DEVICE int64 [Cs][H][10]: {n[cf][co] (cf-major), n_masked} += the counts (exact);
 *   n_samples_lead: DEVICE int64 [1] += B.  Ordinary read-modify-writes (calls on one stream are ordered).
 * A workgroup owns paradis_seeps_rows(W) (0 for W < 1) whole rows of one (sample, channel).  ws:
 * paradis_seeps_ws_bytes(B, Cs, H, W) bytes, 8-byte aligned: double [B][Cs][H][3], then uint32 [B][Cs][H][10].  B == 0 or
 * K == 0 does nothing.  rc 1 before any HIP call for: B or K < 0, C / Cs / H / W < 1, Cs above the maximum, a dry that is
 * not finite, bounds that are not 0 < p_lo <= p_hi < 1, a NULL accumulator, ws or input, a channel outside [0, C),
 * H W >= 2^31 - 8192, strides shorter than a state / a plane, a grid above the launch limit.
 * W % 4 == 0 with 16-byte aligned bases and strides takes one 16-byte load per plane and quad of cells, anything else
 * scalar loads: the same bits.  Algorithmic HBM bytes per cell of a channel: 16. */
int paradis_seeps_max_channels(void);
int paradis_seeps_rows(int W);
size_t paradis_seeps_ws_bytes(int B, int Cs, int H, int W);
int paradis_seeps_update(const float* fc, int64_t fc_bs, const float* truth, int64_t truth_bs, const float* p1,
                         const float* thr, int64_t clim_ks, int64_t clim_cs, const int* clim_index, int K,
                         const int* chan_host, int Cs, float dry, float p_lo, float p_hi, double* acc_real_lead,
                         int64_t* acc_int_lead, int64_t* n_samples_lead, void* ws, int B, int C, int H, int W,
                         void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PARADIS_HIP_H */
