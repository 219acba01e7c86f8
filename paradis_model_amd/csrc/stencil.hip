// a7: depthwise k x k stencil on the virtual geocyclic halo (no padded tensor is materialised; reference
// model/blocks.py:101-113, model/paradis.py:189-190): the C ABI, the schedule choice and the last step of the weight
// gradient.  The kernels sit in stencil_planes.hip (whole planes and staged full tiles, k = 5) and stencil_generic.hip
// (one tile per workgroup, every k) over stencil_common.h.
//
// HBM-bound: the stencil reads 4 B + writes 4 B per (channel, point) (+ halo re-reads served by L2); tiles of 32x64
// outputs are staged once in LDS including the halo.
#include "stencil_common.h"

namespace {

__global__ void __launch_bounds__(256)
dwconv_wgrad_finish(const float* __restrict__ partial, float* __restrict__ gw,
                    float* __restrict__ gbias, int C, int KK, int chunks) {
  const int NW = KK + 1;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= C * NW) return;
  const int c = idx / NW, i = idx - c * NW;
  float s = 0.f;
  for (int ch = 0; ch < chunks; ++ch) s += partial[((int64_t)c * chunks + ch) * NW + i];
  if (i < KK) gw[(int64_t)c * KK + i] = s;
  else if (gbias) gbias[c] = s;
}

int check_dw(const char* name, int B, int C, int H, int W, int k) {
  PD_REQUIRE(B >= 0 && C >= 1 && H >= 2 && W >= 2, "%s: bad shape", name);
  PD_REQUIRE(k >= 1 && k <= 11 && (k & 1), "%s: kernel size %d not supported (odd sizes 1..11)", name, k);
  PD_REQUIRE(W % 2 == 0, "%s: Number of longitude points must be even", name);
  PD_REQUIRE((k - 1) / 2 <= H - 2 && (k - 1) <= W, "%s: grid %dx%d too small for k=%d", name, H, W, k);
  // the analytic halo folding of the data gradient is verified for halos that do not overlap themselves
  PD_REQUIRE(k <= 7 || (H >= 2 * k && W >= 2 * k), "%s: k=%d needs a grid of at least %dx%d", name, k, 2 * k, 2 * k);
  PD_REQUIRE((int64_t)B * C * (((H + TH - 1) / TH) * ((W + TW - 1) / TW)) < (1ll << 31), "%s: too large", name);
  return 0;
}

// The two halves of the backward.  The standalone entry points and the two-kernel path of paradis_dwconv_geo_bwd both
// come through here with the same schedules (stencil_common.h), and its one-pass kernels are these families' kernels
// with both halves compiled in: paradis_dwconv_geo_bwd has the bits of paradis_dwconv_geo_dgrad(_add) +
// paradis_dwconv_geo_wgrad by construction.
int dgrad_half(DwSched s, const DwArgs& a) {
  if (a.B == 0) return 0;
  switch (s) {
    case DwSched::Planes: pd_dw_dgrad_planes(a); break;
    case DwSched::Tiles: pd_dw_dgrad_tiles(a); break;
    case DwSched::Generic: pd_dw_dgrad_generic(a, dw_whole_vec4(a.H, a.W, a.k, a.gy)); break;
  }
  PD_CHECK_LAUNCH("dwconv_geo_dgrad");
  return 0;
}

void wgrad_finish(const DwArgs& a, int chunks) {
  const int n = a.C * (a.k * a.k + 1);
  hipLaunchKernelGGL(dwconv_wgrad_finish, dim3((n + 255) / 256), dim3(256), 0, a.st, a.partial, a.gw, a.gbias, a.C,
                     a.k * a.k, chunks);
}

int wgrad_half(DwSched s, const DwArgs& a) {
  int chunks = 1;
  switch (s) {
    case DwSched::Planes: chunks = pd_dw_wgrad_planes(a); break;
    case DwSched::Tiles: chunks = pd_dw_wgrad_tiles(a); break;
    case DwSched::Generic: chunks = pd_dw_wgrad_generic(a, dw_whole_vec4(a.H, a.W, a.k, a.x)); break;
  }
  wgrad_finish(a, chunks);
  PD_CHECK_LAUNCH("dwconv_geo_wgrad");
  return 0;
}

int dwconv_geo_fwd_impl(const float* x, const float* w, const float* bias, float* y, int B, int C, int H, int W, int k,
                        void* stream, bool y16) {
  if (int e = check_dw("dwconv_geo_fwd", B, C, H, W, k)) return e;
  if (B == 0) return 0;
  DwArgs a{};
  a.x = x; a.w = w; a.bias = bias; a.y = y;
  a.B = B; a.C = C; a.H = H; a.W = W; a.k = k; a.st = (hipStream_t)stream;
  switch (dw_fwd_schedule(a, y16)) {
    case DwSched::Planes: pd_dw_fwd_planes(a, y16); break;
    case DwSched::Tiles: pd_dw_fwd_tiles(a, y16); break;
    case DwSched::Generic: pd_dw_fwd_generic(a, y16, dw_whole_vec4(H, W, k, x)); break;
  }
  PD_CHECK_LAUNCH("dwconv_geo_fwd");
  return 0;
}

DwArgs bwd_args(const float* gy, const float* x, const float* w, const float* addend, float* gx, float* gw, float* gbias,
                int B, int C, int H, int W, int k, void* workspace, void* stream) {
  DwArgs a{};
  a.gy = gy; a.x = x; a.w = w; a.addend = addend; a.gx = gx; a.gw = gw; a.gbias = gbias;
  a.partial = (float*)workspace;
  a.B = B; a.C = C; a.H = H; a.W = W; a.k = k; a.st = (hipStream_t)stream;
  return a;
}

int dwconv_geo_dgrad_launch(const float* gy, const float* w, const float* addend, float* gx, int B, int C, int H, int W,
                            int k, void* stream) {
  if (int e = check_dw("dwconv_geo_dgrad", B, C, H, W, k)) return e;
  const DwArgs a = bwd_args(gy, nullptr, w, addend, gx, nullptr, nullptr, B, C, H, W, k, nullptr, stream);
  return dgrad_half(dw_dgrad_schedule(a), a);
}

}  // namespace

extern "C" int paradis_dwconv_geo_fwd(const float* x, const float* w, const float* bias, float* y,
                                      int B, int C, int H, int W, int k, void* stream) {
  return dwconv_geo_fwd_impl(x, w, bias, y, B, C, H, W, k, stream, false);
}

// y written as bf16 (ABI 9; bf16-mixed mode: the consumer is the SepConv's pointwise GEMM)
extern "C" int paradis_dwconv_geo_fwd16(const float* x, const float* w, const float* bias, void* y,
                                        int B, int C, int H, int W, int k, void* stream) {
  return dwconv_geo_fwd_impl(x, w, bias, (float*)y, B, C, H, W, k, stream, true);
}

extern "C" int paradis_dwconv_geo_dgrad(const float* gy, const float* w, float* gx, int B, int C,
                                        int H, int W, int k, void* stream) {
  return dwconv_geo_dgrad_launch(gy, w, nullptr, gx, B, C, H, W, k, stream);
}

// gx = dgrad(gy) + addend (addend [B,C,H,W], not aliasing gx)
extern "C" int paradis_dwconv_geo_dgrad_add(const float* gy, const float* w, const float* addend, float* gx, int B,
                                            int C, int H, int W, int k, void* stream) {
  PD_REQUIRE(B == 0 || (addend != nullptr && addend != gx), "dwconv_geo_dgrad_add: addend must be a tensor other than gx");
  return dwconv_geo_dgrad_launch(gy, w, addend, gx, B, C, H, W, k, stream);
}

// (the pointers, and with them the schedule, are not known when sizes are asked: room for either chunk count, dw_ws_chunks)
extern "C" size_t paradis_dwconv_geo_wgrad_ws_bytes(int B, int C, int H, int W, int k) {
  return (size_t)C * dw_ws_chunks(B, C, dw_tiles(H, W)) * (k * k + 1) * sizeof(float) + 256;
}

extern "C" int paradis_dwconv_geo_wgrad(const float* gy, const float* x, float* gw, float* gbias,
                                        int B, int C, int H, int W, int k, void* workspace,
                                        void* stream) {
  if (int e = check_dw("dwconv_geo_wgrad", B, C, H, W, k)) return e;
  PD_REQUIRE(workspace != nullptr, "dwconv_geo_wgrad: workspace required");
  const DwArgs a = bwd_args(gy, x, nullptr, nullptr, nullptr, gw, gbias, B, C, H, W, k, workspace, stream);
  return wgrad_half(dw_wgrad_schedule(a), a);
}

// Both gradients of the stencil from one call: gx = dgrad(gy) (+ addend), gw / gbias.  Where the two halves agree on the
// whole-plane schedule (k = 5, W = 64, H <= 32, aligned tensors: the reference grids at 5.625 degrees) or on the
// staged-tiles schedule (k = 5, larger grids with W % 4 == 0) ONE kernel reads gy once; elsewhere the two halves run one
// after the other, as from paradis_dwconv_geo_dgrad / _wgrad.  Bit-identical to paradis_dwconv_geo_dgrad(_add) and
// paradis_dwconv_geo_wgrad on every path.  workspace: paradis_dwconv_geo_wgrad_ws_bytes.  addend, gbias: nullable.
extern "C" int paradis_dwconv_geo_bwd(const float* gy, const float* x, const float* w, const float* addend, float* gx,
                                      float* gw, float* gbias, int B, int C, int H, int W, int k, void* workspace,
                                      void* stream) {
  if (int e = check_dw("dwconv_geo_bwd", B, C, H, W, k)) return e;
  PD_REQUIRE(workspace != nullptr, "dwconv_geo_bwd: workspace required");
  PD_REQUIRE(addend == nullptr || addend != gx, "dwconv_geo_bwd: addend must not alias gx");
  const DwArgs a = bwd_args(gy, x, w, addend, gx, gw, gbias, B, C, H, W, k, workspace, stream);
  const DwSched sd = dw_dgrad_schedule(a), sw = dw_wgrad_schedule(a);
  if (dw_one_pass(sd, sw, B)) {
    wgrad_finish(a, sd == DwSched::Tiles ? pd_dw_bwd_tiles(a) : pd_dw_bwd_planes(a, false));
    PD_CHECK_LAUNCH("dwconv_geo_bwd");
    return 0;
  }
  // (what is left here: k != 5, rows that are not whole float4, grids smaller than a tile one way, misaligned tensors.  A
  //  first one-pass kernel for the larger grids - one channel per workgroup, (sample, tile) items strided over two
  //  workgroups, both tiles staged synchronously per item - measured 1004 us per call at 128 x 256, B = 8, C = 1024
  //  against 628 + 483 us for these two kernels; dwconv_geo_bwd_tiles_kernel - next item's loads in flight, tile-fastest
  //  item order, ~8192 workgroups - takes 822 us)
  if (int e = dgrad_half(sd, a)) return e;
  return wgrad_half(sw, a);
}

// gy as a bf16 tensor (ABI 9; bf16-mixed mode), everything else as paradis_dwconv_geo_bwd.  Whole-plane grids only
// (paradis_dwconv_geo_bwd16_ok: k = 5, W = 64, H <= 32 - the 5.625-degree grid); the caller widens gy elsewhere.
extern "C" int paradis_dwconv_geo_bwd16_ok(int H, int W, int k) {
  return (DWCONV_BWD_FUSED && DWCONV_PLANES && dw_planes_shape(H, W, k)) ? 1 : 0;
}
extern "C" int paradis_dwconv_geo_bwd16(const void* gy, const float* x, const float* w, const float* addend, float* gx,
                                        float* gw, float* gbias, int B, int C, int H, int W, int k, void* workspace,
                                        void* stream) {
  if (int e = check_dw("dwconv_geo_bwd16", B, C, H, W, k)) return e;
  PD_REQUIRE(workspace != nullptr, "dwconv_geo_bwd16: workspace required");
  PD_REQUIRE(addend == nullptr || addend != gx, "dwconv_geo_bwd16: addend must not alias gx");
  PD_REQUIRE(paradis_dwconv_geo_bwd16_ok(H, W, k), "dwconv_geo_bwd16: whole-plane grids only (%dx%d, k = %d)", H, W, k);
  const DwArgs a = bwd_args((const float*)gy, x, w, addend, gx, gw, gbias, B, C, H, W, k, workspace, stream);
  PD_REQUIRE(dw_dgrad_schedule(a) == DwSched::Planes && dw_wgrad_schedule(a) == DwSched::Planes,
             "dwconv_geo_bwd16: misaligned tensor");
  if (B == 0) return paradis_dwconv_geo_bwd(nullptr, x, w, addend, gx, gw, gbias, B, C, H, W, k, workspace, stream);
  wgrad_finish(a, pd_dw_bwd_planes(a, true));
  PD_CHECK_LAUNCH("dwconv_geo_bwd");
  return 0;
}
