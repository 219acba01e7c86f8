// a3-a5: fused semi-Lagrangian advection core (reference model/advection.py:129-169).
//
//   F~  = F with rows 0, H-1 replaced by their longitudinal mean       (advection.py:100-114)
//   (phi, lam) departure point in the rotated frame                     (advection.py:74-98)
//   sample coordinates on the geocyclic-padded plane                    (advection.py:139-150 +
//       ATen grid_sampler unnormalise, align_corners=True)
//   bilinear / bicubic (Keys A=-0.75) gather, rows 0, H-1 of the result replaced by their mean
//
// Saved-for-backward state is (F, u, v) only; everything else is recomputed.
// Algorithmic HBM traffic: 16 B/point forward, 28 B/point backward.
//
// The kernels are VALU-issue bound, not HBM bound (round 1: 264 issue units per point; on gfx950
// only fp32 add/mul/fma, v_mov, v_and and v_add_u32 issue at 2 cycles per wave, every compare, select,
// min/max/med3, conversion, shift, integer multiply-add and DPP move costs 4, transcendentals 8:
// tools/valu_rate_bench.hip).  Round 2 therefore restates the coordinate arithmetic:
//
//   * Sample coordinates.  The reference forms  lon_d = remainder(lon_a + atan2(n,d) + 2pi, 2pi),
//     pix = (lon_d - min)/d_lon (W-1), normalises to [-1,1] and ATen un-normalises again: ten fp32
//     roundings per axis.  Here  ix = wrap(lon_a cx + c0x + atan2(n,d) cx, [c0x, c0x + period))  and
//     iy = asin(s) cy + c0y  with cx = (W-1)/d_lon, cy = (H-1)/d_lat, period = 2 pi cx and the offsets
//     evaluated in double on the host (two FMAs and a floor per axis).  Same mathematical function;
//     its distance to the fp64 evaluation is HALF the CPU-fp32 reference's own (x: 1.4e-6 vs 3.4e-6
//     cells rms at 32x64), and its distance to the CPU-fp32 result is that reference's own rounding
//     noise (6.5e-6 rms at 32x64, tests/test_hip_pad_advect.py).
//   * asin / atan2 / sincos: polynomial kernels with wave-uniform range specialisation (a wave is one
//     latitude row: all its lanes sit in the same asin branch; displacements below 45 degrees need
//     neither range reduction nor octant fix-ups).  <= 2.3 ulp like the host libm.
//   * Cubic weights from A t (1-t)^2 and A t^2 (1-t) (5 instead of 8 operations for the outer taps).
//   * Tap origin: v_fract / v_med3 in float, one conversion for the LDS index.
//
// A workgroup stages a WINDOW of the geocyclic-PADDED plane in LDS through the a1 index map (pole rows
// already replaced by their means); the 4x4 / 2x2 taps of a point are plain 2-D indexing from one
// base address.  The first three schedules of the same arithmetic (the strips: advect_strips.hip):
//   row64 : W == 64, separable grid (the 5.625 degree configuration): window = the whole padded plane,
//           one workgroup per plane, one wave per latitude row: sin/cos(lat) are scalar loads, the
//           longitude column is a per-thread constant, pole-row means are wave reductions;
//   whole : any plane that fits LDS, per-point table loads;
//   tiled : 64x128 (forward) / 16x128 (backward) arrival tiles with a halo of D padded cells; taps
//           outside the window fall back to global loads through the index map / global float atomics.
// Backward scatters into 64-bit fixed-point window accumulators with integer LDS atomics
// (ds_add_f32 is ~30x slower than ds_add_u64 on gfx950, tools/lds_atomic_bench.hip), scaled by an
// exact power of two from the tile's max |cotangent| (resolution max|g| 2^-41; integer adds are
// associative: bitwise reproducible), then folds the halo back (whole) or flushes the window once
// with global atomics (tiled).
//
// This unit: the C ABI, the workspace layout, the schedule choice and the prologue / epilogue kernels (pole-row means,
// the deterministic mode's per-plane maximum and fixed-point conversion).  The schedules: advect_planes.hip,
// advect_tilerow.hip, advect_strips.hip; what they share: advect_common.h.
#include <assert.h>
#include "advect_common.h"

namespace {

// ---- pole-row helpers of the tiled schedule ---------------------------------------------
__global__ void __launch_bounds__(256)
pole_row_means(const float* __restrict__ src, float* __restrict__ means, int planes, int K, int H,
               int W, int64_t bs) {
  const int w = (blockIdx.x * 256 + threadIdx.x) >> 6;  // one wave per (plane,row)
  if (w >= planes * 2) return;
  const int plane = w >> 1, which = w & 1;
  const int b = plane / K, k = plane - b * K;
  const float* row = src + (int64_t)b * bs + (int64_t)k * H * W + (which ? (int64_t)(H - 1) * W : 0);
  const float m = wave_row_mean(row, W);
  if ((threadIdx.x & 63) == 0) means[w] = m;
}

// ---- deterministic tiled backward (PARADIS_DETERMINISTIC=1): per-plane max |cotangent| and the conversion of the
// integer accumulators; integer global atomics are associative, so the field gradient no longer depends on the order
// in which the tiles flush
__global__ void __launch_bounds__(256)
plane_absmax_kernel(const float* __restrict__ src, unsigned* __restrict__ pmax, int K, int P, int64_t bs) {
  __shared__ unsigned red[4];
  const int plane = blockIdx.x, b = plane / K, k = plane - b * K;
  const float* s = src + (int64_t)b * bs + (int64_t)k * P;
  unsigned m = 0;
  for (int i = threadIdx.x; i < P; i += 256) m = max(m, abs_bits(s[i]));
  m = wave_umax_lane63(m);
  if ((threadIdx.x & 63) == 63) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) pmax[plane] = max(max(red[0], red[1]), max(red[2], red[3]));
}

__global__ void __launch_bounds__(256)
fixed_to_float_kernel(const unsigned long long* __restrict__ gacc, const unsigned* __restrict__ pmax,
                      float* __restrict__ dst, int P, int64_t total) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    float scale, inv;
    fixed_point_scale(__uint_as_float(pmax[i / P]), scale, inv);
    dst[i] = (float)((double)(long long)gacc[i] * (double)inv);
  }
}

__global__ void __launch_bounds__(256)
pole_rows_to_mean(float* __restrict__ dst, int planes, int K, int H, int W, int64_t bs) {
  const int w = (blockIdx.x * 256 + threadIdx.x) >> 6;
  if (w >= planes * 2) return;
  const int plane = w >> 1, which = w & 1;
  const int b = plane / K, k = plane - b * K;
  float* row = dst + (int64_t)b * bs + (int64_t)k * H * W + (which ? (int64_t)(H - 1) * W : 0);
  const float m = wave_row_mean(row, W);
  for (int x = threadIdx.x & 63; x < W; x += 64) row[x] = m;
}

int check_adv(const char* name, int B, int K, int H, int W, int mode) {
  PD_REQUIRE(B >= 0 && K >= 1 && H >= 4 && W >= 4, "%s: bad shape B=%d K=%d H=%d W=%d", name, B, K, H, W);
  PD_REQUIRE(W % 2 == 0, "%s: Number of longitude points must be even", name);
  PD_REQUIRE(mode == PARADIS_INTERP_BILINEAR || mode == PARADIS_INTERP_BICUBIC,
             "%s: interpolation mode must be 1 (bilinear) or 2 (bicubic)", name);
  PD_REQUIRE((int64_t)B * K < (1 << 30) && (int64_t)H * W < (1ll << 24), "%s: too large", name);
  return 0;
}

// 16-byte staging path: aligned planes, p even (bicubic), padded width even
int adv_vec4(const float* field, int H, int W, int64_t f_bs, int p) {
  return (W % 4 == 0) && (f_bs % 4 == 0) && (((int64_t)H * W) % 4 == 0) && (p % 2 == 0) && aligned16(field);
}

// ---- the schedule of a call ----------------------------------------------------------------------------------------
// row64  : W == 64, separable grid, the padded plane fits LDS: one wave per latitude row (advect_planes.hip)
// whole  : any other plane that fits LDS (advect_planes.hip)
// strips : larger planes on a separable grid: ring strips of 128 columns (advect_strips.hip)
// circle : backward of such planes of at most 256 longitudes: the ring spans the whole circle (advect_strips.hip)
// tilerow: PARADIS_ADVECT_TILES on a separable grid: the row-wave tiles, a diagnostic A/B (advect_tilerow.hip)
// tiled  : larger planes on any other grid: arrival tiles with a halo (advect_planes.hip)
enum class AdvSchedule { ROW64, WHOLE, STRIPS, CIRCLE, TILEROW, TILED };

constexpr size_t WHOLE_LDS_LIMIT = 64 * 1024;
// `separable`: a grid whose latitude depends on the row only and whose longitude depends on the column only - the caller
// vouches for it through `flags` and passes the latitude table; `deterministic`: paradis_deterministic()
AdvSchedule adv_schedule(bool backward, int H, int W, int mode, int flags, bool has_lat_cells, bool deterministic) {
  const int p = adv_pad(mode), NT = 2 * p;
  const bool separable = (flags & PARADIS_ADVECT_SEPARABLE) && !(flags & PARADIS_ADVECT_GENERIC) && has_lat_cells;
  // the whole-plane footprints of the two directions differ: a plane may run whole forward and tiled backward
  const size_t whole = backward ? bwd_whole_lds(H, W, p) : fwd_whole_lds(H, W, p);
  if (!(flags & PARADIS_ADVECT_TILED) && whole <= WHOLE_LDS_LIMIT) return W == 64 && separable ? AdvSchedule::ROW64 : AdvSchedule::WHOLE;
  if (!separable) return AdvSchedule::TILED;
  // strips: packed 16-bit source columns
  if (!(W < 32768) || (flags & PARADIS_ADVECT_TILES)) return AdvSchedule::TILEROW;
  // full-circle ring only where both of its variants fit LDS (H > 160 takes the 64-row ring: W beyond ~200 columns then
  // does not fit and the 128-column strips run instead, with their zero fill); the deterministic mode's
  // integer plane is the strips'
  const bool circle = backward && W <= 256 && !deterministic && !(flags & PARADIS_ADVECT_STRIPS) &&
                      circle_lds(H, W, NT) <= (size_t)STRIP_LDS_MAX && circle_lds_wide(W, NT) <= (size_t)STRIP_LDS_MAX;
  return circle ? AdvSchedule::CIRCLE : AdvSchedule::STRIPS;
}

// ---- the workspace of a call ---------------------------------------------------------------------------------------
//   [pole-row means of field, then of cotangent: 2 + 2 floats per plane | padding to 256 bytes + 256]          base
//   [deterministic mode: per-plane max |cotangent|, one word per plane | 64-bit integer plane, 16-byte aligned]  det
//   [strip schedules, 256-byte aligned: counts, one word per list | class words, one per plane | padding to 256 bytes |
//    deferred-point lists, 3 x H x 128 words per strip]
// The deterministic region BEGINS where the means end - inside the padding of the base region - but is counted as if it
// began behind it: base_bytes() + det_bytes() is therefore an upper bound of its end, and that is where the strip region
// starts.  (The paddings and alignments are those of the ABI-6 layout, kept byte for byte.)
struct AdvWorkspace {
  size_t planes, H, P;
  size_t strips;      // deferred-point lists: planes x strips of 128 columns
  bool strip_region;  // false: no call of this shape and these flags takes a strip schedule
  bool deterministic;
  // sized for either direction and either padding width: the caller allocates once per shape and flags
  AdvWorkspace(int B, int K, int H_, int W, int flags, bool det)
      : planes((size_t)B * K), H((size_t)H_), P((size_t)H_ * W), strips(planes * (size_t)((W + STRIP_W - 1) / STRIP_W)),
        strip_region(false), deterministic(det) {
    for (int backward = 0; backward < 2; ++backward)
      for (int mode : {PARADIS_INTERP_BILINEAR, PARADIS_INTERP_BICUBIC}) {
        const AdvSchedule s = adv_schedule(backward != 0, H_, W, mode, flags, true, det);
        if (s == AdvSchedule::STRIPS || s == AdvSchedule::CIRCLE) strip_region = true;
      }
    assert(means_bytes() <= base_bytes());      // the invariant above
  }
  size_t means_bytes() const { return planes * 4 * sizeof(float); }
  size_t base_bytes() const { return ((means_bytes() + 255) & ~(size_t)255) + 256; }
  size_t det_bytes() const { return deterministic ? planes * sizeof(unsigned) + 16 + planes * P * 8 + 16 : 0; }
  size_t count_bytes() const { return ((strips + planes) * sizeof(unsigned) + 255) & ~(size_t)255; }   // counts and class words
  size_t list_bytes() const { return 3 * strips * H * STRIP_W * sizeof(unsigned); }
  size_t total() const { return base_bytes() + det_bytes() + 256 + (strip_region ? list_bytes() + count_bytes() + 256 : 0); }

  // the regions in the caller's allocation (alignments are of the address, as ever)
  static char* align_up(void* q, uintptr_t a) { return (char*)(((uintptr_t)q + a - 1) & ~(a - 1)); }
  float* fmeans(void* ws) const { return (float*)ws; }
  float* gmeans(void* ws) const { return fmeans(ws) + planes * 2; }
  unsigned* pmax(void* ws) const { return (unsigned*)((char*)ws + means_bytes()); }
  unsigned long long* gacc(void* ws) const { return (unsigned long long*)align_up(pmax(ws) + planes, 16); }
  unsigned* counts(void* ws) const { return (unsigned*)align_up((char*)ws + base_bytes() + det_bytes(), 256); }
  unsigned* wide(void* ws) const { return counts(ws) + strips; }
  unsigned* queue(void* ws) const { return (unsigned*)((char*)counts(ws) + count_bytes()); }
};

inline int stream_blocks_adv(int64_t n) { return (int)std::min<int64_t>((n + 255) / 256, 256 * 32); }

}  // namespace

extern "C" size_t paradis_sl_advect_ws_bytes(int B, int K, int H, int W, int flags) {
  return AdvWorkspace(B, K, H, W, flags, paradis_deterministic()).total();
}

extern "C" int paradis_sl_advect_fwd(const float* field, const float* u, const float* v, float* out,
                                     const float* sin_lat, const float* cos_lat, const float* lat_cells,
                                     const float* lon,
                                     int B, int K, int H, int W, int64_t f_bs, int64_t uv_bs,
                                     int64_t o_bs, float dt, float min_lat, float min_lon,
                                     float d_lat, float d_lon, int mode, int flags, void* workspace,
                                     void* stream) {
  if (int e = check_adv("sl_advect_fwd", B, K, H, W, mode)) return e;
  if (B == 0) return 0;
  const int p = adv_pad(mode), planes = B * K;
  hipStream_t st = (hipStream_t)stream;
  AdvArgs a = {};
  a.field = field; a.u = u; a.v = v; a.out = out;
  a.sin_lat = sin_lat; a.cos_lat = cos_lat; a.lat_cells = lat_cells; a.lon = lon;
  a.B = B; a.K = K; a.H = H; a.W = W;
  a.f_bs = f_bs; a.uv_bs = uv_bs; a.o_bs = o_bs;
  a.dt = dt; a.min_lat = min_lat; a.min_lon = min_lon; a.d_lat = d_lat; a.d_lon = d_lon;
  a.mode = mode; a.flags = flags; a.st = st;
  a.vec4 = adv_vec4(field, H, W, f_bs, p);
  const AdvSchedule s = adv_schedule(false, H, W, mode, flags, lat_cells != nullptr, paradis_deterministic());
  if (s == AdvSchedule::ROW64 || s == AdvSchedule::WHOLE) {
    if (int e = s == AdvSchedule::ROW64 ? pd_adv_fwd_row64(a) : pd_adv_fwd_whole(a)) return e;
    PD_CHECK_LAUNCH("sl_advect_fwd");
    return 0;
  }
  PD_REQUIRE(workspace != nullptr, "sl_advect_fwd: workspace required for the tiled schedule");
  const AdvWorkspace ws(B, K, H, W, flags, paradis_deterministic());
  a.fmeans = ws.fmeans(workspace);
  const int mean_blocks = (planes * 2 * 64 + 255) / 256;
  hipLaunchKernelGGL(pole_row_means, dim3(mean_blocks), dim3(256), 0, st, field, a.fmeans, planes, K, H, W, f_bs);
  const AdvTiles t = adv_tiles(H, W, 2 * p, flags, false);      // (checked for every schedule of this branch, as ever)
  PD_REQUIRE((int64_t)planes * t.tiles < (1ll << 31), "sl_advect_fwd: too many tiles");
  PD_REQUIRE(t.lds <= 160 * 1024, "sl_advect_fwd: window does not fit LDS");
  int e;
#ifdef PARADIS_DEV_KNOBS
  static const int direct = [] { const char* e = getenv("PARADIS_ADVECT_DIRECT"); return e ? atoi(e) : 0; }();   // (A/B: 4 or 8 rows per workgroup)
  if (direct > 0 && s != AdvSchedule::TILED) e = pd_adv_fwd_direct(a, direct);     // (any separable grid)
  else
#endif
  if (s == AdvSchedule::STRIPS) {
    a.counts = ws.counts(workspace); a.queue = ws.queue(workspace);
    e = pd_adv_fwd_strips(a);
  } else {
    e = s == AdvSchedule::TILEROW ? pd_adv_fwd_tilerow(a) : pd_adv_fwd_tiled(a);
  }
  if (e) return e;
  hipLaunchKernelGGL(pole_rows_to_mean, dim3(mean_blocks), dim3(256), 0, st, out, planes, K, H, W, o_bs);
  PD_CHECK_LAUNCH("sl_advect_fwd(tiled)");
  return 0;
}

extern "C" int paradis_sl_advect_bwd(const float* gout, const float* field, const float* u,
                                     const float* v, float* gfield, float* gu, float* gv,
                                     const float* sin_lat, const float* cos_lat, const float* lat_cells,
                                     const float* lon,
                                     int B, int K, int H, int W, int64_t go_bs, int64_t f_bs,
                                     int64_t uv_bs, int64_t gf_bs, int64_t guv_bs, float dt,
                                     float min_lat, float min_lon, float d_lat, float d_lon, int mode,
                                     int flags, void* workspace, void* stream) {
  if (int e = check_adv("sl_advect_bwd", B, K, H, W, mode)) return e;
  if (B == 0) return 0;
  const int p = adv_pad(mode), planes = B * K, P = H * W;
  hipStream_t st = (hipStream_t)stream;
  AdvArgs a = {};
  a.gout = gout; a.field = field; a.u = u; a.v = v; a.gfield = gfield; a.gu = gu; a.gv = gv;
  a.sin_lat = sin_lat; a.cos_lat = cos_lat; a.lat_cells = lat_cells; a.lon = lon;
  a.B = B; a.K = K; a.H = H; a.W = W;
  a.go_bs = go_bs; a.f_bs = f_bs; a.uv_bs = uv_bs; a.gf_bs = gf_bs; a.guv_bs = guv_bs;
  a.dt = dt; a.min_lat = min_lat; a.min_lon = min_lon; a.d_lat = d_lat; a.d_lon = d_lon;
  a.mode = mode; a.flags = flags; a.st = st;
  a.vec4 = adv_vec4(field, H, W, f_bs, p);
  const bool det = paradis_deterministic();
  const AdvSchedule s = adv_schedule(true, H, W, mode, flags, lat_cells != nullptr, det);
  if (s == AdvSchedule::ROW64 || s == AdvSchedule::WHOLE) {
    if (int e = s == AdvSchedule::ROW64 ? pd_adv_bwd_row64(a) : pd_adv_bwd_whole(a)) return e;
    PD_CHECK_LAUNCH("sl_advect_bwd");
    return 0;
  }
  PD_REQUIRE(workspace != nullptr, "sl_advect_bwd: workspace required for the tiled schedule");
  PD_REQUIRE(gf_bs == (int64_t)K * P, "sl_advect_bwd: tiled schedule needs a contiguous gfield");
  const AdvWorkspace ws(B, K, H, W, flags, det);
  a.fmeans = ws.fmeans(workspace); a.gmeans = ws.gmeans(workspace);
  const int mean_blocks = (planes * 2 * 64 + 255) / 256;
  hipLaunchKernelGGL(pole_row_means, dim3(mean_blocks), dim3(256), 0, st, field, a.fmeans, planes, K, H, W, f_bs);
  hipLaunchKernelGGL(pole_row_means, dim3(mean_blocks), dim3(256), 0, st, gout, a.gmeans, planes, K, H, W, go_bs);
  // PARADIS_DETERMINISTIC=1: the tiles add 64-bit fixed-point values (one power-of-two scale per plane) into an integer
  // plane in the workspace, converted once at the end - no float atomics on the field gradient
  if (det) {
    a.pmax = ws.pmax(workspace); a.gacc = ws.gacc(workspace);
    hipLaunchKernelGGL(plane_absmax_kernel, dim3(planes), dim3(256), 0, st, gout, a.pmax, K, P, go_bs);
  }
  // (the full circle stores every cell of gfield: no zero fill)
  if (s != AdvSchedule::CIRCLE &&
      pd_zero_async(det ? (void*)a.gacc : (void*)gfield, (size_t)planes * P * (det ? 8 : 4), st) != hipSuccess) {
    paradis_set_error("sl_advect_bwd: memset failed");
    return 2;
  }
  const AdvTiles t = adv_tiles(H, W, 2 * p, flags, true);       // (checked for every schedule of this branch, as ever)
  PD_REQUIRE((int64_t)planes * t.tiles < (1ll << 31), "sl_advect_bwd: too many tiles");
  PD_REQUIRE(t.lds <= 160 * 1024, "sl_advect_bwd: window does not fit LDS");
  int e;
  if (s == AdvSchedule::CIRCLE || s == AdvSchedule::STRIPS) {
    a.counts = ws.counts(workspace); a.wide = ws.wide(workspace); a.queue = ws.queue(workspace);
    e = s == AdvSchedule::CIRCLE ? pd_adv_bwd_circle(a) : pd_adv_bwd_strips(a);
  } else {
    e = s == AdvSchedule::TILEROW ? pd_adv_bwd_tilerow(a) : pd_adv_bwd_tiled(a);
  }
  if (e) return e;
  if (det)
    hipLaunchKernelGGL(fixed_to_float_kernel, dim3(stream_blocks_adv((int64_t)planes * P)), dim3(256), 0, st,
                       (const unsigned long long*)a.gacc, (const unsigned*)a.pmax, gfield, P, (int64_t)planes * P);
  hipLaunchKernelGGL(pole_rows_to_mean, dim3(mean_blocks), dim3(256), 0, st, gfield, planes, K, H, W, gf_bs);
  PD_CHECK_LAUNCH("sl_advect_bwd(tiled)");
  return 0;
}
