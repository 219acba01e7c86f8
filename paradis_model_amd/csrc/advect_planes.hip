// Schedules whose kernels share the whole-plane helpers: W == 64 planes on a separable grid (the 5.625 degree
// configuration; one wave per latitude row, the window is the whole padded plane) and the generic kernels of any
// grid - the whole padded plane in LDS where it fits, 64x128 (forward) / 16x128 (backward) arrival tiles with a halo
// where it does not.  Both directions and their launchers (called from advect.hip); shared: advect_common.h.
// (One unit on purpose: alone in a unit, the W == 64 kernels are the only callers of stage_window, geo_src and the
//  pole-row helpers, the compiler propagates W = 64 into those before inlining them and emits other - equivalent -
//  instructions than it does beside the generic kernels.)
#include "advect_common.h"

namespace {

// Value of one arrival point from a whole-plane window that is XR = 1 column wider than the padded plane
// (column Wp repeats the wrap): for finite inputs the tap block then always lies inside the window -
// ix is in [p - eps, W + p + eps], iy within half a cell of the grid's latitude range - so the forward
// needs neither clamps nor the edge path.  A non-finite coordinate makes every weight NaN and a garbage
// index, and LDS reads beyond the allocation return 0: the result is NaN, as it should be.
constexpr int ROW64_XR = 1;
// velocities and output are touched once per launch: non-temporal
#define ADV_LD(p) __builtin_nontemporal_load(p)
#define ADV_ST(v, p) __builtin_nontemporal_store(v, p)
template <int MODE>
__device__ __forceinline__ float sample_wide(const float* win, float ix, float iy, int WS, float WSf) {
  constexpr int NT = Interp<MODE>::NT, OFF0 = Interp<MODE>::OFF0;
  const float tx = __builtin_amdgcn_fractf(ix), ty = __builtin_amdgcn_fractf(iy);
  float wx[NT], wy[NT];
  Interp<MODE>::weights(tx, wx);
  Interp<MODE>::weights(ty, wy);
  const int cell = (int)fmaf(iy - ty, WSf, ix - tx);
  const float* base = win + OFF0 * (WS + 1) + cell;
  float acc = 0.f;
#pragma unroll
  for (int a = 0; a < NT; ++a) {
    float rowacc = 0.f;
#pragma unroll
    for (int bb = 0; bb < NT; ++bb) rowacc = fmaf(base[a * WS + bb], wx[bb], rowacc);
    acc = fmaf(rowacc, wy[a], acc);
  }
  return acc;
}

// W == 64, separable grid: a workgroup (4 waves) walks ROW64_CHUNK consecutive planes, wave w owns rows
// w, w+4, ... of each.  The planes are software pipelined through two LDS windows:
//   - the interior of plane n+1 goes global -> LDS by DMA (one 256-byte row per global_load_lds_dword)
//     while plane n is computed: no staging registers, no staging latency on the critical path;
//   - halo columns and the mirrored rows beyond the poles are copies of interior cells, filled LDS -> LDS;
//   - the velocity prefetch runs ADV_PF rows ahead ACROSS plane boundaries.
// XR = ROW64_XR: global grid (the host checked the coordinate range), wide window, unclamped taps;
// XR = 0: any other grid, taps outside the padded plane count as zero like ATen's grid_sample.
#ifndef ADV_ROW64_CHUNK     // (A/B builds)
#define ADV_ROW64_CHUNK 4
#endif
constexpr int ROW64_CHUNK = ADV_ROW64_CHUNK;   // 1 and 12 (one workgroup per resident slot) measured 3-6 % slower
typedef __attribute__((address_space(3))) void* adv_lds_ptr_t;
typedef const __attribute__((address_space(1))) void* adv_gbl_ptr_t;

// velocity prefetch cursor of a wave: ADV_PF rows ahead of the row being computed, across plane boundaries.
// Element offsets, not pointers: the loads must stay `global` with a scalar base (srow).
struct VelCursor {
  int64_t off, uv_bs;      // offset of the cursor's plane in u and in v
  int plane, last, b, k, K, y, wave, H, P;
  int yend;                // wave + 4 * (row slots per plane): ceil(H / 4) rounded up to a multiple of 2 ADV_PF
  __device__ __forceinline__ void load(const float* __restrict__ u, const float* __restrict__ v, unsigned lane,
                                       float& a, float& c) {
    const int64_t j = off + min(y, H - 1) * 64;
    a = ADV_LD(&srow(u + j)[lane]);
    c = ADV_LD(&srow(v + j)[lane]);
    y += 4;
    if (y >= yend && plane + 1 < last) {   // (past the last plane: keeps reloading its last row)
      ++plane; y = wave;
      if (++k == K) { k = 0; ++b; }
      off = (int64_t)b * uv_bs + (int64_t)k * P;
    }
  }
};

// One 256-byte row global -> LDS by DMA (M0 = LDS row start, lane -> +4 bytes), both addresses wave-uniform.
// Inline assembly on purpose: with the builtin the compiler's wait-count pass treats the vector memory
// counter as unordered while a DMA is pending and turns every wait for a prefetched velocity into vmcnt(0).
// Hidden from it, its counted waits only become stricter (they count fewer newer operations than there are).
__device__ __forceinline__ void dma_row_to_lds(const float* grow, unsigned lane_bytes, float* lds_row) {
  const uint64_t a = (uint64_t)grow;
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)a);
  const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(a >> 32));
  const uint64_t base = ((uint64_t)hi << 32) | lo;
  const uint32_t m = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)(adv_lds_ptr_t)lds_row);
  asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dword %1, %2"
               :: "s"(m), "v"(lane_bytes), "s"(base) : "memory");   // (M0 is reserved: the compiler keeps nothing in it across statements)
}

// Halo cells of the W = 64 window: the 2p mirrored rows beyond the poles, then p + (p + XR) columns per row.  Cell q of
// that list as (destination << 16 | source) offsets into the window, 0xffff0000 for the cells of the two pole rows
// (written whole by pole_rows_to_mean_lds).  The list does not depend on the plane: each thread keeps its ROW64_HMAP
// pairs in registers for the whole launch instead of redoing the index arithmetic (~50 vector instructions) per plane.
constexpr int ROW64_HMAP = 3;
constexpr unsigned ROW64_NO_CELL = 0xffff0000u;   // (its source half reads cell 0)
template <int MODE, int XR>
__device__ __forceinline__ int row64_halo_cells(int H) {
  constexpr int p = Interp<MODE>::NT / 2, WS = 64 + 2 * p + XR;
  return 2 * p * WS + H * (2 * p + XR);
}
template <int MODE, int XR>
__device__ __forceinline__ unsigned row64_halo_pair(int q, int H) {
  constexpr int W = 64, p = Interp<MODE>::NT / 2, WS = W + 2 * p + XR, hc = 2 * p + XR, nrow_cells = 2 * p * WS;
  int lr, lc;
  if (q < nrow_cells) {
    const int rr = q / WS;
    lc = q - rr * WS;
    lr = rr < p ? rr : H + rr;
  } else {
    const int e = q - nrow_cells, rr = e / hc, cc = e - rr * hc;
    lr = rr + p;
    lc = cc < p ? cc : W + cc;
  }
  if (lr == p || lr == H - 1 + p) return ROW64_NO_CELL;
  int sr, sc;
  geo_src(lr - p, lc - p, H, W, sr, sc);
  return ((unsigned)(lr * WS + lc) << 16) | (unsigned)((sr + p) * WS + sc + p);
}

// One plane of the pipeline.  The interior of the NEXT plane goes global -> LDS by DMA, one row per row
// iteration, while this plane is computed.  That the DMA INTO cur - issued one plane earlier - has landed
// is the caller's counted wait.
template <int MODE, int XR>
__device__ __forceinline__ void row64_plane(float* __restrict__ cur, float* __restrict__ nxt,
                                            const float* __restrict__ field, int64_t next_off, bool has_next,
                                            float* __restrict__ O, const float* __restrict__ u,
                                            const float* __restrict__ v, VelCursor& vc, float (&qu)[ADV_PF],
                                            float (&qv)[ADV_PF], const float* __restrict__ sin_lat,
                                            const float* __restrict__ cos_lat, const float* __restrict__ lat_cells,
                                            float lonc, const AdvGeom& g, int wave, unsigned lane, bool fill_halo,
                                            const unsigned (&hmap)[ROW64_HMAP]) {
  constexpr int W = 64, p = Interp<MODE>::NT / 2, WS = W + 2 * p + XR;
  const int H = g.H, Hp = H + 2 * p, tid = threadIdx.x;
  // halo columns (p left, p + XR right) and the p mirrored rows beyond each pole are copies of interior
  // cells; the two pole rows are written whole by pole_rows_to_mean_lds
  if (fill_halo) {
    if (row64_halo_cells<MODE, XR>(H) <= 256 * ROW64_HMAP) {   // the (destination, source) cells of this thread: row64_halo_map
      float t[ROW64_HMAP];
#pragma unroll
      for (int k = 0; k < ROW64_HMAP; ++k) t[k] = cur[hmap[k] & 0xffffu];
#pragma unroll
      for (int k = 0; k < ROW64_HMAP; ++k)
        if (hmap[k] != ROW64_NO_CELL) cur[hmap[k] >> 16] = t[k];
    } else {
      for (int q = tid; q < row64_halo_cells<MODE, XR>(H); q += 256) {
        const unsigned m = row64_halo_pair<MODE, XR>(q, H);
        if (m != ROW64_NO_CELL) cur[m >> 16] = cur[m & 0xffffu];
      }
    }
  }
  pole_rows_to_mean_lds(cur, H, W, p, WS);
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");   // (no vmcnt: loads stay in flight)
  const float Hpf = (float)Hp, WSf = (float)WS;
  // one row: consume the velocities in (cu, cv), refill the slot (nu, nv) from the cursor
  auto do_row = [&](int y, float cu, float cv, float& nu, float& nv) {
    if (has_next && y < H) dma_row_to_lds(field + next_off + y * W, 4 * lane, nxt + (y + p) * WS + p);
    vc.load(u, v, lane, nu, nv);
    if (y < H) {
      const float sa = sin_lat[y * W], ca = cos_lat[y * W];   // uniform address: scalar loads
      float ix, iy;
      departure_row(cu, cv, sa, ca, lonc, lat_cells[y * W], g, ix, iy, nullptr);
      float acc = XR ? sample_wide<MODE>(cur, ix, iy, WS, WSf) : sample_whole<MODE>(cur, ix, iy, Hp, WS, Hpf, WSf);
      if (y == 0 || y == H - 1) acc = wave_sum_dpp(acc) * (1.0f / 64.0f);   // pole rows <- their mean
      ADV_ST(acc, &srow(O + y * W)[lane]);
    }
  };
  // Two register sets that swap roles (qu/qv -> ru/rv -> qu/qv): a load never targets a register whose old
  // value is still needed, so there is no copy of a just-loaded register - and no vmcnt(0) - at the back edge.
  float ru[ADV_PF], rv[ADV_PF];
  for (int y0 = wave; y0 < vc.yend; y0 += 8 * ADV_PF) {   // the cursor's slot count: the same for every wave
#pragma unroll
    for (int d = 0; d < ADV_PF; ++d) do_row(y0 + 4 * d, qu[d], qv[d], ru[d], rv[d]);
#pragma unroll
    for (int d = 0; d < ADV_PF; ++d) do_row(y0 + 4 * (ADV_PF + d), ru[d], rv[d], qu[d], qv[d]);
  }
}

// Scalar-register cap of the forward kernel.  The compiler's own choice (106 SGPRs: row pointers, table values and the
// constants of five code paths) admits 6 workgroups per CU (800 SGPRs per SIMD / (112 + 16)); at <= 80 the
// hardware admits 8, which is also what the 59 VGPRs and the 19.9 KB of LDS allow.  27 values then live in VGPR
// lanes (v_readlane / v_writelane around the rare paths): 178 -> 173 us per launch, same box (round 3).
#ifndef ADV_FWD_SGPRS      // (0 = the compiler's choice)
#define ADV_FWD_SGPRS 80
#endif
#if ADV_FWD_SGPRS
#define ADV_FWD_SGPR_ATTR __attribute__((amdgpu_num_sgpr(ADV_FWD_SGPRS)))
#else
#define ADV_FWD_SGPR_ATTR
#endif
template <int MODE, int XR>
__global__ void __launch_bounds__(256) ADV_FWD_SGPR_ATTR
sl_advect_fwd_row64(const float* __restrict__ field, const float* __restrict__ u,
                    const float* __restrict__ v, float* __restrict__ out,
                    const float* __restrict__ sin_lat, const float* __restrict__ cos_lat,
                    const float* __restrict__ lat_cells, const float* __restrict__ lon, int K, AdvGeom g, int64_t f_bs, int64_t uv_bs,
                    int64_t o_bs, int planes, int chunk) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int W = 64, p = Interp<MODE>::NT / 2, WS = W + 2 * p + XR;   // WS: window row stride
  const int H = g.H, P = H * W, Hp = H + 2 * p;
  const int tid = threadIdx.x;
  const unsigned lane = tid & 63;   // unsigned: row pointer (scalar) + 32-bit lane offset addressing
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int first = blockIdx.x * chunk, last = min(first + chunk, planes);
  int b = first / K, k = first - b * K;

  VelCursor vc;
  vc.uv_bs = uv_bs; vc.plane = first; vc.last = last; vc.b = b; vc.k = k; vc.K = K;
  vc.y = wave; vc.wave = wave; vc.H = H; vc.P = P;
  vc.yend = wave + 4 * (((H + 3) / 4 + 2 * ADV_PF - 1) / (2 * ADV_PF) * (2 * ADV_PF));
  vc.off = (int64_t)b * uv_bs + (int64_t)k * P;
  float qu[ADV_PF], qv[ADV_PF];
#pragma unroll
  for (int d = 0; d < ADV_PF; ++d) vc.load(u, v, lane, qu[d], qv[d]);
  const float lonc = lon_cells(lon[lane], g);
  unsigned hmap[ROW64_HMAP];
#pragma unroll
  for (int k = 0; k < ROW64_HMAP; ++k) {
    const int q = tid + 256 * k;
    hmap[k] = q < row64_halo_cells<MODE, XR>(H) ? row64_halo_pair<MODE, XR>(q, H) : ROW64_NO_CELL;
  }
  float* cur = smem;
  float* nxt = smem + Hp * WS;
  {   // the first plane of the chunk is staged through registers, halo included
    Window w{0, 0, Hp, WS};
    stage_window(cur, field + (int64_t)b * f_bs + (int64_t)k * P, w, H, W, p, false, 0.f, 0.f, 256);
  }
  for (int plane = first; plane < last; ++plane) {
    // `cur` has landed and every wave is done reading `nxt`.  A wave issues its last DMA at the top of its
    // last row; two loads and one store (at least) follow.  Loads complete in issue order, so with at most
    // 2 operations outstanding the DMA - older than both loads - is in LDS whatever the store did; the
    // barrier covers the other waves' rows.
    if (plane != first) asm volatile("s_waitcnt vmcnt(2)\n\ts_barrier" ::: "memory");
    else asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    int nb = b, nk = k + 1;
    if (nk == K) { nk = 0; ++nb; }
    const bool has_next = plane + 1 < last;
    const int64_t next_off = has_next ? (int64_t)nb * f_bs + (int64_t)nk * P : 0;
    row64_plane<MODE, XR>(cur, nxt, field, next_off, has_next, out + (int64_t)b * o_bs + (int64_t)k * P, u, v, vc,
                          qu, qv, sin_lat, cos_lat, lat_cells, lonc, g, wave, lane, plane != first, hmap);
    float* t = cur; cur = nxt; nxt = t;
    b = nb; k = nk;
  }
}

// W == 64, separable grid: one workgroup per plane, wave w owns rows w, w+4, ...
// (five workgroups per CU: 29 KB of LDS each; the second launch-bound keeps the registers at 96)
#ifndef ADV_BWD_WAVES
#define ADV_BWD_WAVES 5
#endif
template <int MODE>
__global__ void __launch_bounds__(256, ADV_BWD_WAVES)
sl_advect_bwd_row64(const float* __restrict__ gout, const float* __restrict__ field,
                    const float* __restrict__ u, const float* __restrict__ v,
                    float* __restrict__ gfield, float* __restrict__ gu, float* __restrict__ gv,
                    const float* __restrict__ sin_lat, const float* __restrict__ cos_lat,
                    const float* __restrict__ lat_cells, const float* __restrict__ lon, int K, AdvGeom g, int64_t go_bs, int64_t f_bs,
                    int64_t uv_bs, int64_t gf_bs, int64_t guv_bs, int vec4) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int NT = Interp<MODE>::NT, OFF0 = Interp<MODE>::OFF0, W = 64;
  const int H = g.H, p = g.p, P = H * W, Hp = H + 2 * p, Wp = W + 2 * p;
  const int tid = threadIdx.x;
  const unsigned lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int plane = blockIdx.x;
  const int b = plane / K, k = plane - b * K;
  const float* F = field + (int64_t)b * f_bs + (int64_t)k * P;
  const float* U = u + (int64_t)b * uv_bs + (int64_t)k * P;
  const float* V = v + (int64_t)b * uv_bs + (int64_t)k * P;
  const float* GO = gout + (int64_t)b * go_bs + (int64_t)k * P;
  float* GF = gfield + (int64_t)b * gf_bs + (int64_t)k * P;
  float* GU = gu + (int64_t)b * guv_bs + (int64_t)k * P;
  float* GV = gv + (int64_t)b * guv_bs + (int64_t)k * P;

  const int wn = Hp * Wp, wn2 = (wn + 1) & ~1;
  unsigned long long* acc = reinterpret_cast<unsigned long long*>(smem);  // [wn] fixed-point sums
  float* win = smem + 2 * wn2;                                             // [wn]  F~ window
  float* misc = win + wn2;   // [0..1] pole means of gout, [2..6) per-wave max |cotangent|

  // first rows' operands while the window is staged
  float qu[ADV_PF], qv[ADV_PF], qg[ADV_PF];
#pragma unroll
  for (int d = 0; d < ADV_PF; ++d) {
    const int j = min(wave + 4 * d, H - 1) * W;
    qu[d] = srow(U + j)[lane]; qv[d] = srow(V + j)[lane]; qg[d] = srow(GO + j)[lane];
  }
  const float lonc = lon_cells(lon[lane], g);
  if (vec4) stage_plane_vec4(win, F, H, W, p);
  else {
    Window w{0, 0, Hp, Wp};
    stage_window(win, F, w, H, W, p, false, 0.f, 0.f, 256);
  }
  for (int i = tid; i < wn; i += 256) acc[i] = 0ull;
  unsigned gmaxb = 0;
  for (int y = wave; y < H; y += 4) {
    const float gval = srow(GO + y * W)[lane];
    gmaxb = max(gmaxb, abs_bits(gval));
    if (y == 0 || y == H - 1) {   // adjoint of the final pole mean: the cotangent of a pole row is its row mean
      const float m = wave_sum_dpp(gval) * (1.0f / 64.0f);
      if (lane == 0) misc[y == 0 ? 0 : 1] = m;
    }
  }
  const float mxall = reduce_gmax(gmaxb, misc, 4);    // its barrier also closes the staging
  pole_rows_to_mean_lds(win, H, W, p, Wp);
  __syncthreads();
  const float gm0 = misc[0], gm1 = misc[1];
  float scale, inv_scale;   // every thread derives the same power-of-two scale
  fixed_point_scale(mxall, scale, inv_scale);

  const float Hpf = (float)Hp, Wpf = (float)Wp;
  for (int y0 = wave; y0 < H; y0 += 4 * ADV_PF) {
#pragma unroll
    for (int d = 0; d < ADV_PF; ++d) {
      const int y = y0 + 4 * d;                 // wave-uniform
      const float cu = qu[d], cv = qv[d], cgo = qg[d];
      {
        const int j = min(y + 4 * ADV_PF, H - 1) * W;
        qu[d] = srow(U + j)[lane]; qv[d] = srow(V + j)[lane]; qg[d] = srow(GO + j)[lane];
      }
      if (y < H) {
        const float sa = sin_lat[y * W], ca = cos_lat[y * W];
        float ix, iy, tx, ty, wx[NT], wy[NT], dwx[NT], dwy[NT];
        DepState st;
        departure_row(cu, cv, sa, ca, lonc, lat_cells[y * W], g, ix, iy, &st);
        int cell;
        const bool edge = tap_block_whole<MODE>(ix, iy, Hpf, Wpf, tx, ty, cell);
        int base = cell + OFF0 * (Wp + 1);
        if (__any(edge)) {
          int bx, by, sx, sy;
          tap_origin<MODE>(ix, iy, Hp, Wp, bx, by, sx, sy, tx, ty);
          Interp<MODE>::weights(tx, wx); Interp<MODE>::weights(ty, wy);
          Interp<MODE>::dweights(tx, dwx); Interp<MODE>::dweights(ty, dwy);
          shift_weights<NT>(wx, sx); shift_weights<NT>(dwx, sx);
          shift_weights<NT>(wy, sy); shift_weights<NT>(dwy, sy);
          base = by * Wp + bx;
        } else {
          Interp<MODE>::weights(tx, wx); Interp<MODE>::weights(ty, wy);
          Interp<MODE>::dweights(tx, dwx); Interp<MODE>::dweights(ty, dwy);
        }
        const float gval = (y == 0) ? gm0 : ((y == H - 1) ? gm1 : cgo);
        float gix, giy;
        scatter_gather<MODE>(acc, win, base, Wp, wx, wy, dwx, dwy, gval * scale, gix, giy);
        float guv, gvv;
        departure_backward(st, sa, ca, gix * gval, giy * gval, g, guv, gvv);
        srow(GU + y * W)[lane] = guv;
        srow(GV + y * W)[lane] = gvv;
      }
    }
  }
  __syncthreads();
  // fold the halo back: every source cell sums its aliases (adjoint of the a1 map: its own cell, the
  // lon-wrap copies of the p edge columns, and for rows next to a pole the mirrored row shifted by
  // W/2), then the adjoint of the first pole mean (rows 0, H-1 <- their mean)
  const double inv = (double)inv_scale;
  const bool lo_edge = lane < p, hi_edge = lane >= W - p;
  const unsigned xm = lane ^ 32u;                     // (x + W/2) mod W
  const bool mlo = xm < p, mhi = xm >= W - p;
  for (int y = wave; y < H; y += 4) {
    int mr = -1;                                 // padded row of the over-the-pole alias (wave-uniform)
    if (y >= 1 && y <= p) mr = p - y;
    else if (y >= H - 1 - p && y <= H - 2) mr = 2 * (H - 1) - y + p;
    const unsigned long long* row = acc + (y + p) * Wp + p;
    long long s = (long long)row[lane];
    if (lo_edge) s += (long long)row[lane + W];
    if (hi_edge) s += (long long)row[lane - W];
    if (mr >= 0) {
      const unsigned long long* mrow = acc + mr * Wp + p;
      s += (long long)mrow[xm];
      if (mlo) s += (long long)mrow[xm + W];
      if (mhi) s += (long long)mrow[xm - W];
    }
    float val = (float)((double)s * inv);
    if (y == 0 || y == H - 1) val = wave_sum_dpp(val) * (1.0f / 64.0f);
    srow(GF + y * W)[lane] = val;
  }
}

template <int MODE, bool WHOLE, int NTH>
__global__ void __launch_bounds__(NTH)
sl_advect_fwd_kernel(const float* __restrict__ field, const float* __restrict__ u,
                     const float* __restrict__ v, float* __restrict__ out,
                     const float* __restrict__ sin_lat, const float* __restrict__ cos_lat,
                     const float* __restrict__ lon, const float* __restrict__ fmeans, int K,
                     AdvGeom g, int64_t f_bs, int64_t uv_bs, int64_t o_bs, int halo, int tiles_x,
                     int tiles, int vec4) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int NT = Interp<MODE>::NT;
  const int H = g.H, W = g.W, p = g.p, P = H * W, Hp = H + 2 * p, Wp = W + 2 * p;
  const int tid = threadIdx.x, wave = tid >> 6;
  const int plane = WHOLE ? blockIdx.x : blockIdx.x / tiles;
  const int tile = WHOLE ? 0 : blockIdx.x - plane * tiles;
  const int b = plane / K, k = plane - b * K;
  const float* F = field + (int64_t)b * f_bs + (int64_t)k * P;
  const float* U = u + (int64_t)b * uv_bs + (int64_t)k * P;
  const float* V = v + (int64_t)b * uv_bs + (int64_t)k * P;
  float* O = out + (int64_t)b * o_bs + (int64_t)k * P;

  const int ty0 = WHOLE ? 0 : (tile / tiles_x) * TILE_HF, tx0 = WHOLE ? 0 : (tile % tiles_x) * TILE_W;
  const int th = WHOLE ? H : min(TILE_HF, H - ty0), tw = WHOLE ? W : min(TILE_W, W - tx0);
  Window w;
  if (WHOLE) { w.wy0 = 0; w.wx0 = 0; w.WH = Hp; w.WW = Wp; }
  else { w.wy0 = ty0 + p - halo; w.wx0 = tx0 + p - halo; w.WH = TILE_HF + 2 * halo + NT; w.WW = TILE_W + 2 * halo + NT; }
  float* win = smem;                           // [WH*WW]
  float* pole_out = win + w.WH * w.WW;         // [2*W]  (WHOLE only)

  float m0 = 0.f, m1 = 0.f;
  if (!WHOLE) { m0 = fmeans[2 * plane]; m1 = fmeans[2 * plane + 1]; }
  if (WHOLE && vec4) stage_plane_vec4(win, F, H, W, p);
  else stage_window(win, F, w, H, W, p, !WHOLE, m0, m1, NTH);
  __syncthreads();
  if (WHOLE) {
    pole_rows_to_mean_lds(win, H, W, p, Wp);
    __syncthreads();
  }
  const float Hpf = (float)Hp, Wpf = (float)Wp;
  const int npts = th * tw;
  // one arrival point of the tiled schedule: departure -> tap block -> window gather or L2 fallback
  auto point_tiled = [&](float uu, float vv, float sa, float ca, float lo) -> float {
    float ix, iy, tx, ty, wx[NT], wy[NT];
    int bx, by, sx, sy;
    departure(uu, vv, sa, ca, lon_cells(lo, g), g, ix, iy, nullptr);
    tap_origin<MODE>(ix, iy, Hp, Wp, bx, by, sx, sy, tx, ty);
    Interp<MODE>::weights(tx, wx);
    Interp<MODE>::weights(ty, wy);
    if (sx | sy) {   // only when a coordinate rounds onto the plane edge (or is not finite)
      shift_weights<NT>(wx, sx);
      shift_weights<NT>(wy, sy);
    }
    int ry = by - w.wy0, rx = bx - w.wx0;
    if (rx < 0) rx += W; else if (rx > w.WW - NT) rx -= W;
    const bool inwin = ry >= 0 && ry <= w.WH - NT && rx >= 0 && rx <= w.WW - NT;
    float acc = 0.f;
    if (inwin) {
      const float* base = win + ry * w.WW + rx;
#pragma unroll
      for (int a = 0; a < NT; ++a) {
        float rowacc = 0.f;
#pragma unroll
        for (int bb = 0; bb < NT; ++bb) rowacc = fmaf(base[a * w.WW + bb], wx[bb], rowacc);
        acc = fmaf(rowacc, wy[a], acc);
      }
    } else {  // taps served by L2 through the index map
      const int lastrow = H - 1;
#pragma unroll
      for (int a = 0; a < NT; ++a) {
        float rowacc = 0.f;
#pragma unroll
        for (int bb = 0; bb < NT; ++bb) {
          int r, c;
          geo_src(by + a - p, bx + bb - p, H, W, r, c);
          float val = F[(int64_t)r * W + c];
          if (r == 0) val = m0; else if (r == lastrow) val = m1;
          rowacc = fmaf(val, wx[bb], rowacc);
        }
        acc = fmaf(rowacc, wy[a], acc);
      }
    }
    return acc;
  };
  if constexpr (WHOLE) {
    // Whole plane: the arrival index is the flat index.  Operands are prefetched ADV_PF points ahead
    // into a queue whose slots are fixed registers (the loop is unrolled ADV_PF times) with
    // unconditional, clamped loads: straight-line code lets the compiler count vmcnt exactly.
    const int last = npts - 1;
    float qu[ADV_PF], qv[ADV_PF], qs[ADV_PF], qc[ADV_PF], ql[ADV_PF];
#pragma unroll
    for (int d = 0; d < ADV_PF; ++d) {
      const int j = min(tid + NTH * d, last);
      qu[d] = U[j]; qv[d] = V[j]; qs[d] = sin_lat[j]; qc[d] = cos_lat[j]; ql[d] = lon[j];
    }
    const int lastrow0 = (H - 1) * W;
    for (int i0 = tid; i0 < npts; i0 += NTH * ADV_PF) {
#pragma unroll
      for (int d = 0; d < ADV_PF; ++d) {
        const int i = i0 + NTH * d;
        const float cu = qu[d], cv = qv[d], csa = qs[d], cca = qc[d], clo = ql[d];
        {
          const int j = min(i + NTH * ADV_PF, last);
          qu[d] = U[j]; qv[d] = V[j]; qs[d] = sin_lat[j]; qc[d] = cos_lat[j]; ql[d] = lon[j];
        }
        float ix, iy;
        departure(cu, cv, csa, cca, lon_cells(clo, g), g, ix, iy, nullptr);
        const float acc = sample_whole<MODE>(win, ix, iy, Hp, Wp, Hpf, Wpf);
        if (i < npts) {
          if (i < W || i >= lastrow0) pole_out[i < W ? i : W + i - lastrow0] = acc;
          else O[i] = acc;
        }
      }
    }
    __syncthreads();
    if (wave < 2) {
      const float* row = pole_out + (wave == 0 ? 0 : W);
      const float m = wave_row_mean(row, W);
      float* orow = O + (wave == 0 ? 0 : (int64_t)(H - 1) * W);
      for (int x = tid & 63; x < W; x += 64) orow[x] = m;
    }
  } else {
    // tiled schedule: operands of point i+1 are loaded before point i is computed
    TileIter it(tid, tw, NTH);
    float nu = 0.f, nv = 0.f, nsa = 0.f, nca = 0.f, nlo = 0.f;
    if (tid < npts) {
      const int idx = (ty0 + it.yl) * W + tx0 + it.xl;
      nu = U[idx]; nv = V[idx]; nsa = sin_lat[idx]; nca = cos_lat[idx]; nlo = lon[idx];
    }
    for (int i = tid; i < npts; i += NTH) {
      const int idx = (ty0 + it.yl) * W + tx0 + it.xl;
      const float cu = nu, cv = nv, csa = nsa, cca = nca, clo = nlo;
      it.next();
      if (i + NTH < npts) {
        const int nidx = (ty0 + it.yl) * W + tx0 + it.xl;
        nu = U[nidx]; nv = V[nidx]; nsa = sin_lat[nidx]; nca = cos_lat[nidx]; nlo = lon[nidx];
      }
      const float acc = point_tiled(cu, cv, csa, cca, clo);
      O[idx] = acc;
    }
  }
}

template <int MODE, bool WHOLE, int NTH, bool DET = false>   // DET: integer global accumulators (deterministic tiled mode)
__global__ void __launch_bounds__(NTH)
sl_advect_bwd_kernel(const float* __restrict__ gout, const float* __restrict__ field,
                     const float* __restrict__ u, const float* __restrict__ v,
                     float* __restrict__ gfield, float* __restrict__ gu, float* __restrict__ gv,
                     const float* __restrict__ sin_lat, const float* __restrict__ cos_lat,
                     const float* __restrict__ lon, const float* __restrict__ fmeans,
                     const float* __restrict__ gmeans, int K, AdvGeom g, int64_t go_bs, int64_t f_bs,
                     int64_t uv_bs, int64_t gf_bs, int64_t guv_bs, int halo, int tiles_x, int tiles,
                     int vec4, unsigned long long* __restrict__ gacc, const unsigned* __restrict__ pmax) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int NT = Interp<MODE>::NT;
  const int H = g.H, W = g.W, p = g.p, P = H * W, Hp = H + 2 * p, Wp = W + 2 * p;
  const int tid = threadIdx.x, wave = tid >> 6;
  const int plane = WHOLE ? blockIdx.x : blockIdx.x / tiles;
  const int tile = WHOLE ? 0 : blockIdx.x - plane * tiles;
  const int b = plane / K, k = plane - b * K;
  const float* F = field + (int64_t)b * f_bs + (int64_t)k * P;
  const float* U = u + (int64_t)b * uv_bs + (int64_t)k * P;
  const float* V = v + (int64_t)b * uv_bs + (int64_t)k * P;
  const float* GO = gout + (int64_t)b * go_bs + (int64_t)k * P;
  float* GF = gfield + (int64_t)b * gf_bs + (int64_t)k * P;
  float* GU = gu + (int64_t)b * guv_bs + (int64_t)k * P;
  float* GV = gv + (int64_t)b * guv_bs + (int64_t)k * P;

  const int ty0 = WHOLE ? 0 : (tile / tiles_x) * TILE_H, tx0 = WHOLE ? 0 : (tile % tiles_x) * TILE_W;
  const int th = WHOLE ? H : min(TILE_H, H - ty0), tw = WHOLE ? W : min(TILE_W, W - tx0);
  Window w;
  if (WHOLE) { w.wy0 = 0; w.wx0 = 0; w.WH = Hp; w.WW = Wp; }
  else { w.wy0 = ty0 + p - halo; w.wx0 = tx0 + p - halo; w.WH = TILE_H + 2 * halo + NT; w.WW = TILE_W + 2 * halo + NT; }
  const int wn = w.WH * w.WW, wn2 = (wn + 1) & ~1;
  unsigned long long* acc = reinterpret_cast<unsigned long long*>(smem);  // [wn] fixed-point sums
  float* win = smem + 2 * wn2;                                             // [wn]  F~ window
  float* misc = win + wn2;   // [0..1] pole means of gout, [2..2+NTH/64) per-wave max |cotangent|

  float m0 = 0.f, m1 = 0.f, gm0 = 0.f, gm1 = 0.f;
  if (!WHOLE) {
    m0 = fmeans[2 * plane]; m1 = fmeans[2 * plane + 1];
    gm0 = gmeans[2 * plane]; gm1 = gmeans[2 * plane + 1];
  }
  if (WHOLE && vec4) stage_plane_vec4(win, F, H, W, p);
  else stage_window(win, F, w, H, W, p, !WHOLE, m0, m1, NTH);
  for (int i = tid; i < wn; i += NTH) acc[i] = 0ull;
  // max |cotangent| over this workgroup's arrival points -> fixed-point scale
  const int npts = th * tw;
  unsigned gmaxb = WHOLE ? 0u : max(abs_bits(gm0), abs_bits(gm1));
  {
    TileIter itg(tid, tw, NTH);
    for (int i = tid; i < npts; i += NTH, itg.next())
      gmaxb = max(gmaxb, abs_bits(GO[(ty0 + itg.yl) * W + tx0 + itg.xl]));
  }
  float mxall = reduce_gmax(gmaxb, misc, NTH / 64);
  // deterministic tiled mode: integer global accumulators need ONE scale per plane (its max |cotangent|, a pre-pass)
  unsigned long long* GA = nullptr;
  if constexpr (DET) { GA = gacc + (int64_t)plane * P; mxall = __uint_as_float(pmax[plane]); }
  if (WHOLE) {
    if (wave < 2) {
      float* row = win + (wave == 0 ? p : H - 1 + p) * Wp;
      const float m = wave_row_mean(row + p, W);
      for (int x = tid & 63; x < Wp; x += 64) row[x] = m;
    } else if (wave < 4) {
      // adjoint of the final pole mean: the cotangent of a pole row is its own row mean
      const float* row = GO + (wave == 2 ? 0 : (int64_t)(H - 1) * W);
      const float m = wave_row_mean(row, W);
      if ((tid & 63) == 0) misc[wave - 2] = m;
    }
    __syncthreads();
    gm0 = misc[0]; gm1 = misc[1];
  }
  float scale, inv_scale;   // every thread derives the same power-of-two scale
  fixed_point_scale(mxall, scale, inv_scale);

  TileIter it(tid, tw, NTH);
  // operands of point i+1 are in flight while point i is computed (see the forward kernel)
  float nu = 0.f, nv = 0.f, nsa = 0.f, nca = 0.f, nlo = 0.f, ngo = 0.f;
  if (tid < npts) {
    const int idx = (ty0 + it.yl) * W + tx0 + it.xl;
    nu = U[idx]; nv = V[idx]; nsa = sin_lat[idx]; nca = cos_lat[idx]; nlo = lon[idx]; ngo = GO[idx];
  }
  for (int i = tid; i < npts; i += NTH) {
    const int y = ty0 + it.yl, x = tx0 + it.xl, idx = y * W + x;
    const float cu = nu, cv = nv, sa = nsa, ca = nca, clo = nlo, cgo = ngo;
    it.next();
    if (i + NTH < npts) {
      const int nidx = (ty0 + it.yl) * W + tx0 + it.xl;
      nu = U[nidx]; nv = V[nidx]; nsa = sin_lat[nidx]; nca = cos_lat[nidx]; nlo = lon[nidx]; ngo = GO[nidx];
    }
    float ix, iy, tx, ty, wx[NT], wy[NT], dwx[NT], dwy[NT];
    int bx, by, sx, sy;
    DepState st;
    departure(cu, cv, sa, ca, lon_cells(clo, g), g, ix, iy, &st);
    tap_origin<MODE>(ix, iy, Hp, Wp, bx, by, sx, sy, tx, ty);
    Interp<MODE>::weights(tx, wx);
    Interp<MODE>::weights(ty, wy);
    Interp<MODE>::dweights(tx, dwx);
    Interp<MODE>::dweights(ty, dwy);
    if (sx | sy) {
      shift_weights<NT>(wx, sx);
      shift_weights<NT>(dwx, sx);
      shift_weights<NT>(wy, sy);
      shift_weights<NT>(dwy, sy);
    }
    const float gval = (y == 0) ? gm0 : ((y == H - 1) ? gm1 : cgo);
    int ry = by - w.wy0, rx = bx - w.wx0;
    bool inwin = true;
    if (!WHOLE) {
      if (rx < 0) rx += W; else if (rx > w.WW - NT) rx -= W;
      inwin = ry >= 0 && ry <= w.WH - NT && rx >= 0 && rx <= w.WW - NT;
    }
    float gix = 0.f, giy = 0.f;
    if (inwin) {
      scatter_gather<MODE>(acc, win, ry * w.WW + rx, w.WW, wx, wy, dwx, dwy, gval * scale, gix, giy);
    } else {  // tiled schedule only
      const int lastrow = H - 1;
#pragma unroll
      for (int a = 0; a < NT; ++a) {
        float sxv = 0.f, sdx = 0.f;
#pragma unroll
        for (int bb = 0; bb < NT; ++bb) {
          int r, c;
          geo_src(by + a - p, bx + bb - p, H, W, r, c);
          float val = F[(int64_t)r * W + c];
          if (r == 0) val = m0; else if (r == lastrow) val = m1;
          if constexpr (DET) atomicAdd(&GA[(int64_t)r * W + c], fixed_from_product((double)(gval * scale * wy[a]), (double)wx[bb]));
          else atomicAdd(&GF[(int64_t)r * W + c], gval * wy[a] * wx[bb]);
          sxv = fmaf(val, wx[bb], sxv);
          sdx = fmaf(val, dwx[bb], sdx);
        }
        gix = fmaf(wy[a], sdx, gix);
        giy = fmaf(dwy[a], sxv, giy);
      }
    }
    float guv, gvv;
    departure_backward(st, sa, ca, gix * gval, giy * gval, g, guv, gvv);
    GU[idx] = guv;
    GV[idx] = gvv;
  }
  __syncthreads();
  const double inv = (double)inv_scale;
  if (WHOLE) {
    // fold the halo back: every source cell sums its aliases (adjoint of the a1 map), then the
    // adjoint of the first pole mean (rows 0, H-1 <- their mean)
    for (int i = tid; i < P; i += NTH) {
      const int y = i / W, x = i - y * W;
      long long s = 0;
      geo_for_each_alias(y, x, H, W, p, [&](int ii, int jj) { s += (long long)acc[(ii + p) * Wp + jj + p]; });
      win[i] = (float)((double)s * inv);   // the float plane reuses the window storage
    }
    __syncthreads();
    if (wave < 2) {
      float* row = win + (wave == 0 ? 0 : (H - 1) * W);
      const float m = wave_row_mean(row, W);
      for (int x = tid & 63; x < W; x += 64) row[x] = m;
    }
    __syncthreads();
    for (int i = tid; i < P; i += NTH) {
      GF[i] = win[i];
    }
  } else {
    // flush the window once: one global float atomic per touched cell instead of 16 per point
    // (consecutive lanes -> consecutive cells: the 16 atomics per 64-byte line of one wave-instruction
    //  are combined by the memory pipeline; spreading them over 64 lines measured 2x slower)
    for (int i = tid; i < wn; i += NTH) {
      const long long s = (long long)acc[i];
      if (s == 0) continue;
      const int lr = i / w.WW, lc = i - lr * w.WW;
      const int r = w.wy0 + lr;
      if (r < 0 || r >= Hp) continue;
      int jj = (w.wx0 + lc - p) % W;
      if (jj < 0) jj += W;
      int sr, sc;
      geo_src(r - p, jj, H, W, sr, sc);
      if constexpr (DET) atomicAdd(&GA[(int64_t)sr * W + sc], (unsigned long long)s);   // integer: order-independent
      else atomicAdd(&GF[(int64_t)sr * W + sc], (float)((double)s * inv));
    }
  }
}

// Does every tap block of a finite departure point lie inside a whole-plane window with `xr` extra
// columns?  ix = [0, period] + c0x, iy = [-pi/2, pi/2] cy + c0y, each with a margin for rounding; true for
// the global grids of the reference (period = W cells, latitudes from pole to pole).
bool taps_stay_inside(const AdvGeom& g, int NT, int xr) {
  const int off0 = NT == 4 ? -1 : 0;
  const double eps = 1e-2, hpi = 1.5707963267948966;
  const double x_lo = std::floor((double)g.c0x - eps) + off0, x_hi = std::floor((double)g.per + g.c0x + eps) + off0 + NT - 1;
  const double y_lo = std::floor(-hpi * g.cy + g.c0y - eps) + off0, y_hi = std::floor(hpi * g.cy + g.c0y + eps) + off0 + NT - 1;
  return x_lo >= 0 && x_hi <= g.W + 2 * g.p + xr - 1 && y_lo >= 0 && y_hi <= g.H + 2 * g.p - 1;
}

// ---- kernel tables: the reservation iterates them, the launch indexes them; first index adv_mode_index(mode) ----------
using Row64FwdKernel = decltype(&sl_advect_fwd_row64<PARADIS_INTERP_BILINEAR, 0>);
constexpr Row64FwdKernel ROW64_FWD[2][2] = {      // [mode][wide window: taps_stay_inside]
    {&sl_advect_fwd_row64<PARADIS_INTERP_BILINEAR, 0>, &sl_advect_fwd_row64<PARADIS_INTERP_BILINEAR, ROW64_XR>},
    {&sl_advect_fwd_row64<PARADIS_INTERP_BICUBIC, 0>, &sl_advect_fwd_row64<PARADIS_INTERP_BICUBIC, ROW64_XR>}};
using Row64BwdKernel = decltype(&sl_advect_bwd_row64<PARADIS_INTERP_BILINEAR>);
constexpr Row64BwdKernel ROW64_BWD[2] = {&sl_advect_bwd_row64<PARADIS_INTERP_BILINEAR>, &sl_advect_bwd_row64<PARADIS_INTERP_BICUBIC>};
using GenericFwdKernel = decltype(&sl_advect_fwd_kernel<PARADIS_INTERP_BILINEAR, true, 256>);
constexpr GenericFwdKernel WHOLE_FWD[2] = {&sl_advect_fwd_kernel<PARADIS_INTERP_BILINEAR, true, 256>,
                                           &sl_advect_fwd_kernel<PARADIS_INTERP_BICUBIC, true, 256>};
constexpr GenericFwdKernel TILED_FWD[2] = {&sl_advect_fwd_kernel<PARADIS_INTERP_BILINEAR, false, TILED_THREADS_FWD>,
                                           &sl_advect_fwd_kernel<PARADIS_INTERP_BICUBIC, false, TILED_THREADS_FWD>};
using GenericBwdKernel = decltype(&sl_advect_bwd_kernel<PARADIS_INTERP_BILINEAR, true, 256>);
constexpr GenericBwdKernel WHOLE_BWD[2] = {&sl_advect_bwd_kernel<PARADIS_INTERP_BILINEAR, true, 256>,
                                           &sl_advect_bwd_kernel<PARADIS_INTERP_BICUBIC, true, 256>};
constexpr GenericBwdKernel TILED_BWD[2][2] = {    // [mode][deterministic]
    {&sl_advect_bwd_kernel<PARADIS_INTERP_BILINEAR, false, TILED_THREADS_BWD, false>,
     &sl_advect_bwd_kernel<PARADIS_INTERP_BILINEAR, false, TILED_THREADS_BWD, true>},
    {&sl_advect_bwd_kernel<PARADIS_INTERP_BICUBIC, false, TILED_THREADS_BWD, false>,
     &sl_advect_bwd_kernel<PARADIS_INTERP_BICUBIC, false, TILED_THREADS_BWD, true>}};

}  // namespace

int pd_adv_fwd_row64(const AdvArgs& a) {
  const AdvGeom g = make_geom(a);
  const int p = g.p, planes = a.B * a.K;
  const bool wide = taps_stay_inside(g, 2 * p, ROW64_XR);
  const size_t lds = 2 * (size_t)(a.H + 2 * p) * (a.W + 2 * p + (wide ? ROW64_XR : 0)) * sizeof(float);
  static PerDeviceOnce once;
  if (int e = reserve_lds(once, ROW64_FWD, "sl_advect_fwd")) return e;
  const int chunk = ROW64_CHUNK, groups = (planes + chunk - 1) / chunk;
  hipLaunchKernelGGL(ROW64_FWD[adv_mode_index(a.mode)][wide], dim3(groups), dim3(256), lds, a.st, a.field, a.u, a.v, a.out,
                     a.sin_lat, a.cos_lat, a.lat_cells, a.lon, a.K, g, a.f_bs, a.uv_bs, a.o_bs, planes, chunk);
  return 0;
}

int pd_adv_bwd_row64(const AdvArgs& a) {
  const AdvGeom g = make_geom(a);
  hipLaunchKernelGGL(ROW64_BWD[adv_mode_index(a.mode)], dim3(a.B * a.K), dim3(256), bwd_whole_lds(a.H, a.W, g.p), a.st,
                     a.gout, a.field, a.u, a.v, a.gfield, a.gu, a.gv, a.sin_lat, a.cos_lat, a.lat_cells, a.lon, a.K, g,
                     a.go_bs, a.f_bs, a.uv_bs, a.gf_bs, a.guv_bs, a.vec4);
  return 0;
}

// the generic kernels: `tiled` picks the table and the tile geometry (whole plane: one "tile" per plane, no halo, no means)
static void launch_generic_fwd(const AdvArgs& a, bool tiled) {
  const AdvGeom g = make_geom(a);
  const int planes = a.B * a.K, m = adv_mode_index(a.mode);
  AdvTiles t = {0, 1, 1, fwd_whole_lds(a.H, a.W, g.p)};
  if (tiled) t = adv_tiles(a.H, a.W, 2 * g.p, a.flags, false);
  const GenericFwdKernel kernel = tiled ? TILED_FWD[m] : WHOLE_FWD[m];
  hipLaunchKernelGGL(kernel, dim3((unsigned)(planes * t.tiles)),
                     dim3(tiled ? TILED_THREADS_FWD : 256), t.lds, a.st, a.field, a.u, a.v, a.out, a.sin_lat, a.cos_lat, a.lon,
                     tiled ? a.fmeans : nullptr, a.K, g, a.f_bs, a.uv_bs, a.o_bs, t.halo, t.tx, t.tiles, a.vec4);
}
static void launch_generic_bwd(const AdvArgs& a, bool tiled) {
  const AdvGeom g = make_geom(a);
  const int planes = a.B * a.K, m = adv_mode_index(a.mode);
  AdvTiles t = {0, 1, 1, bwd_whole_lds(a.H, a.W, g.p)};
  if (tiled) t = adv_tiles(a.H, a.W, 2 * g.p, a.flags, true);
  const GenericBwdKernel kernel = tiled ? TILED_BWD[m][a.gacc != nullptr] : WHOLE_BWD[m];
  hipLaunchKernelGGL(kernel, dim3((unsigned)(planes * t.tiles)),
                     dim3(tiled ? TILED_THREADS_BWD : 256), t.lds, a.st, a.gout, a.field, a.u, a.v, a.gfield, a.gu, a.gv,
                     a.sin_lat, a.cos_lat, a.lon, tiled ? a.fmeans : nullptr, tiled ? a.gmeans : nullptr, a.K, g, a.go_bs,
                     a.f_bs, a.uv_bs, a.gf_bs, a.guv_bs, t.halo, t.tx, t.tiles, a.vec4, tiled ? a.gacc : nullptr,
                     tiled ? a.pmax : nullptr);
}

int pd_adv_fwd_whole(const AdvArgs& a) { launch_generic_fwd(a, false); return 0; }
int pd_adv_bwd_whole(const AdvArgs& a) { launch_generic_bwd(a, false); return 0; }
int pd_adv_fwd_tiled(const AdvArgs& a) {
  static PerDeviceOnce once;
  if (int e = reserve_lds(once, TILED_FWD, "sl_advect_fwd")) return e;
  launch_generic_fwd(a, true);
  return 0;
}
int pd_adv_bwd_tiled(const AdvArgs& a) {
  static PerDeviceOnce once;
  if (int e = reserve_lds(once, TILED_BWD, "sl_advect_bwd")) return e;
  launch_generic_bwd(a, true);
  return 0;
}
