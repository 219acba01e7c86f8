// Strip schedules of the advection (round 4): large planes on a separable grid (configs[3], configs[4]).  Ring strips
// of both directions, the full-circle backward, the displacement classes, the fix-ups of the deferred points and the
// development-only direct gather; their launchers (called from advect.hip); shared definitions: advect_common.h.
//
// A workgroup owns a STRIP of 128 arrival columns of one plane and walks down ALL its rows, eight per step.  The window
// of the padded plane it samples from is a RING of R padded rows x (128 + 2 hx + NT) columns in LDS: while the eight
// arrival rows of step s are computed against rows [lo(s), lo(s) + R - 8), the eight rows that enter the window at step
// s + 1 are written into the ring slots of the eight rows that left it at step s - 1 (their global loads were issued a
// step earlier and sit in registers), so one barrier per step separates readers and writers and staging overlaps with
// the arithmetic.  What this buys over the 64 x 128 / 16 x 128 tiles of rounds 1-3:
//   * a window cell is staged once per strip, not once per tile row band: 1.19 (hx = 10) to 1.5 (hx = 32) cells per
//     arrival point instead of 1.5-3.0 - the latitude halo costs LDS rows, not HBM bytes - and the halos can be
//     asymmetric: displacements are a few rows in latitude but tens of columns in longitude next to the poles
//     (tools/adv_disp_stats.py: in the default model at 721 x 1440 |dy| stays below 22 rows for 99 % of the points
//     while 30 % of them move more than 16 columns);
//   * backward: the accumulator rows leave the ring complete - one float atomic per window cell of the strip,
//     1.19 per point instead of 3.0 - and the power-of-two scale of the 64-bit fixed-point sums follows the running
//     maximum of the cotangent (a rescale of the ring when a step raises it) instead of a pre-pass over the cotangent;
//   * taps that leave the window go to L2 with the row / column maps of the tap block evaluated once per point
//     (4 + 4 index computations instead of 16).
#include "advect_common.h"

namespace {

// lane's source columns of the window columns lane, lane + 64, ...: image column in the low half, the column of the
// over-the-pole rows (shifted by W / 2) in the high half
struct StripCols { unsigned pk[STRIP_CH]; };
__device__ __forceinline__ StripCols strip_cols(int wx0, int WS, int W, int p, unsigned lane, int cfirst = 0) {
  StripCols c;
#pragma unroll
  for (int i = 0; i < STRIP_CH; ++i) {
    const int lc = min((int)lane + 64 * (cfirst + i), WS - 1);
    int jj = (wx0 + lc - p) % W;
    if (jj < 0) jj += W;
    int jm = jj + (W >> 1);
    if (jm >= W) jm -= W;
    c.pk[i] = (unsigned)jj | ((unsigned)jm << 16);
  }
  return c;
}

// source row of padded row pr (wave-uniform): valid = inside the padded plane, mir = beyond a pole
struct StripRow { int sr; bool valid, mir; };
__device__ __forceinline__ StripRow strip_row(int pr, int H, int p) {
  const int Hp = H + 2 * p;
  StripRow r;
  r.valid = pr >= 0 && pr < Hp;
  const int ii = min(max(pr, 0), Hp - 1) - p;
  r.mir = ii < 0 || ii >= H;
  r.sr = ii < 0 ? -ii : (ii >= H ? 2 * (H - 1) - ii : ii);
  return r;
}

__device__ __forceinline__ void strip_load_row(const float* __restrict__ F, int pr, int H, int W, int p, const StripCols& cs,
                                               int nch, float (&pre)[STRIP_CH]) {
  const StripRow r = strip_row(pr, H, p);
  const global_ptr<const float> row = srow(F + (int64_t)r.sr * W);
#pragma unroll
  for (int i = 0; i < STRIP_CH; ++i)
    if (i < nch) pre[i] = row[r.mir ? (cs.pk[i] >> 16) : (cs.pk[i] & 0xffffu)];
}

__device__ __forceinline__ void strip_store_row(float* __restrict__ ring, int pr, int RMASK, int WS, int H, int p, float m0,
                                                float m1, unsigned lane, int nch, const float (&pre)[STRIP_CH],
                                                int cfirst = 0) {
  const StripRow r = strip_row(pr, H, p);
  float* dst = ring + (pr & RMASK) * WS;
#pragma unroll
  for (int i = 0; i < STRIP_CH; ++i)
    if (i < nch) {
      float v = pre[i];
      if (r.sr == 0) v = m0;                 // rows 0 and H-1 enter as their longitudinal means (advection.py:100-114)
      if (r.sr == H - 1) v = m1;
      if (!r.valid) v = 0.f;
      const int lc = (int)lane + 64 * (cfirst + i);
      if (lc < WS) dst[lc] = v;
    }
}

// lanes of a wave inside a 128-column strip: waves 2r, 2r+1 own the two 64-column halves of a row
struct StripLane {
  int cbase; unsigned lx; bool active;
  __device__ __forceinline__ StripLane(int half, unsigned lane, int x0, int tw, int W) {
    const int first = half * 64;
    active = first + (int)lane < tw;
    cbase = min(x0 + first, W - 1);
    lx = min(lane, (unsigned)max(tw - 1 - first, 0));
  }
};

// column maps of a tap block at clamped origin column bx (padded coordinates): col[b] / colm[b] = source column of a
// plain / over-the-pole row
template <int NT>
struct TapCols { int col[NT], colm[NT]; };
template <int NT>
__device__ __forceinline__ void tap_cols(int bx, int W, int p, TapCols<NT>& m) {
#pragma unroll
  for (int b = 0; b < NT; ++b) {
    int j = bx + b - p;
    j += j < 0 ? W : 0;
    j -= j >= W ? W : 0;
    int jm = j + (W >> 1);
    jm -= jm >= W ? W : 0;
    m.col[b] = j; m.colm[b] = jm;
  }
}
// source row of padded tap row pr: returns the row offset sr * W; mir = beyond a pole, pole = 1 / 2 for rows 0 / H-1
__device__ __forceinline__ int tap_row(int pr, int H, int W, int p, bool& mir, int& pole) {
  const int ii = pr - p;
  mir = ii < 0 || ii >= H;
  const int sr = ii < 0 ? -ii : (ii >= H ? 2 * (H - 1) - ii : ii);
  pole = sr == 0 ? 1 : (sr == H - 1 ? 2 : 0);
  return sr * W;
}

// value of a point whose tap block leaves the window: all taps from global memory (L2) through the a1 map, two tap
// rows in flight at a time (the registers of this path set the occupancy of the whole kernel)
template <int MODE>
__device__ __forceinline__ float gather_global(const float* __restrict__ F, float ix, float iy, int H, int W, int p,
                                               float m0, float m1) {
  constexpr int NT = Interp<MODE>::NT;
  float tx, ty, wx[NT], wy[NT];
  int bx, by, sx, sy;
  tap_origin<MODE>(ix, iy, H + 2 * p, W + 2 * p, bx, by, sx, sy, tx, ty);
  Interp<MODE>::weights(tx, wx);
  Interp<MODE>::weights(ty, wy);
  shift_weights<NT>(wx, sx);
  shift_weights<NT>(wy, sy);
  TapCols<NT> m;
  tap_cols<NT>(bx, W, p, m);
  float acc = 0.f;
#pragma unroll
  for (int a0 = 0; a0 < NT; a0 += 2) {
    float val[2][NT];
    int pole[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      bool mir;
      const int ro = tap_row(by + a0 + q, H, W, p, mir, pole[q]);
#pragma unroll
      for (int b = 0; b < NT; ++b) val[q][b] = F[ro + (mir ? m.colm[b] : m.col[b])];
    }
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      float rowacc = 0.f;
#pragma unroll
      for (int b = 0; b < NT; ++b) {
        const float t = pole[q] == 1 ? m0 : (pole[q] == 2 ? m1 : val[q][b]);
        rowacc = fmaf(t, wx[b], rowacc);
      }
      acc = fmaf(rowacc, wy[a0 + q], acc);
    }
    asm volatile("" ::: "memory");      // keeps the next pair's loads behind this pair's use
  }
  return acc;
}

// tap block of a point against the ring window: fraction, plane clamp, window-relative column (the window may
// straddle the date line), padded row of tap row 0.  Returns true when the NT x NT block lies inside the resident
// rows [rlo, rhi] x the window columns and the plane clamp did not move it.  All values are integers below 2^24 held
// in floats; r0 / c0 = padded row / window column of tap (0, 0).
template <int MODE>
__device__ __forceinline__ bool tap_block_ring(float ix, float iy, float Hpf, float Wpf, float Wf, float wx0f, float WSf,
                                               float rlof, float rhif, float& tx, float& ty, int& r0, int& c0) {
  constexpr int NT = Interp<MODE>::NT, OFF0 = Interp<MODE>::OFF0;
  tx = __builtin_amdgcn_fractf(ix);
  ty = __builtin_amdgcn_fractf(iy);
  const float x0f = ix - tx, y0f = iy - ty;
  const float xc = __builtin_amdgcn_fmed3f(x0f, (float)(-OFF0), Wpf - (float)(NT + OFF0));
  const float yc = __builtin_amdgcn_fmed3f(y0f, (float)(-OFF0), Hpf - (float)(NT + OFF0));
  float rx = (xc + (float)OFF0) - wx0f;
  const float ry = yc + (float)OFF0;
  rx = rx < 0.f ? rx + Wf : (rx > WSf - (float)NT ? rx - Wf : rx);
  const float rxc = __builtin_amdgcn_fmed3f(rx, 0.f, WSf - (float)NT);
  const float ryc = __builtin_amdgcn_fmed3f(ry, rlof, rhif - (float)(NT - 1));
  r0 = (int)ryc;
  c0 = (int)rxc;
  return xc == x0f && yc == y0f && rxc == rx && ryc == ry;
}

// append this lane's point to the strip's list of deferred points: one LDS atomic per wave that holds any
// (forward: the sample coordinates ride along in two more lists of the same length behind the first, cap entries each)
__device__ __forceinline__ void strip_defer(bool defer, unsigned idx, unsigned* __restrict__ q, unsigned* qcount,
                                            unsigned lane, size_t cap = 0, float ix = 0.f, float iy = 0.f) {
  const unsigned long long m = __ballot(defer);
  if (m == 0ull) return;                                  // wave-uniform
  const int leader = __ffsll((long long)m) - 1;
  unsigned base = 0;
  if ((int)lane == leader) base = atomicAdd(qcount, (unsigned)__popcll(m));
  base = __shfl((int)base, leader, 64);
  if (defer) {
    const unsigned slot = base + __popcll(m & ((1ull << lane) - 1ull));
    q[slot] = idx;
    if (cap) {
      reinterpret_cast<float*>(q)[cap + slot] = ix;
      reinterpret_cast<float*>(q)[2 * cap + slot] = iy;
    }
  }
}

// geometry of the ring: rows resident while the arrival rows [8 s, 8 s + 8) are computed
template <int MODE, int R>
struct StripRing {
  static constexpr int NT = Interp<MODE>::NT, OFF0 = Interp<MODE>::OFF0;
  static constexpr int RW = R - STRIP_ROWS;                      // resident rows
  static constexpr int HYL = (RW - (STRIP_ROWS - 1 + NT)) / 2;     // latitude halo below (rows); above: the rest
  static __device__ __forceinline__ int lo(int s, int p) { return STRIP_ROWS * s + p + OFF0 - HYL; }
};

// waves per SIMD the strip kernels are compiled for: the forward's 19 KB ring of the 128-row grids admits four
// 8-wave workgroups per CU (64 registers, no scratch), its 50 KB ring of the large grids three (74 registers)
#ifndef STRIP_FWD_WAVES
#define STRIP_FWD_WAVES (R == 32 ? 8 : 6)
#endif
#ifndef STRIP_BWD_WAVES
#define STRIP_BWD_WAVES 4
#endif
#ifndef STRIP_FWD_INLINE_FIXUP     // 1: a strip's workgroup processes its own deferred points; 0: a second launch does
#define STRIP_FWD_INLINE_FIXUP 1
#endif
template <int MODE, int R>
__global__ void __launch_bounds__(STRIP_THREADS, STRIP_FWD_WAVES)
sl_advect_fwd_strip(const float* __restrict__ field, const float* __restrict__ u, const float* __restrict__ v,
                    float* __restrict__ out, const float* __restrict__ sin_lat, const float* __restrict__ cos_lat,
                    const float* __restrict__ lat_cells, const float* __restrict__ lon, const float* __restrict__ fmeans,
                    int K, AdvGeom g, int64_t f_bs, int64_t uv_bs, int64_t o_bs, int hx, int strips,
                    unsigned* __restrict__ queue, unsigned* __restrict__ counts) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  __shared__ unsigned qcount;
  using Ring = StripRing<MODE, R>;
  constexpr int NT = Interp<MODE>::NT, RW = Ring::RW, RMASK = R - 1;
  const int H = g.H, W = g.W, p = g.p, P = H * W, Hp = H + 2 * p, Wp = W + 2 * p;
  const int tid = threadIdx.x;
  const unsigned lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int plane = blockIdx.x / strips, strip = blockIdx.x - plane * strips;
  const int b = plane / K, k = plane - b * K;
  const float* F = field + (int64_t)b * f_bs + (int64_t)k * P;
  const float* U = u + (int64_t)b * uv_bs + (int64_t)k * P;
  const float* V = v + (int64_t)b * uv_bs + (int64_t)k * P;
  float* O = out + (int64_t)b * o_bs + (int64_t)k * P;
  const int x0 = strip * STRIP_W, tw = min(STRIP_W, W - x0);
  const int WS = STRIP_W + 2 * hx + NT, wx0 = x0 + p - hx, nch = (WS + 63) >> 6;
  float* ring = smem;
  const float m0 = fmeans[2 * plane], m1 = fmeans[2 * plane + 1];
  const StripLane tl(wave & 1, lane, x0, tw, W);
  const int rw = wave >> 1;                          // this wave's arrival rows of a step: rw and rw + 4
  const int nsteps = (H + STRIP_ROWS - 1) / STRIP_ROWS;
  const StripCols cs = strip_cols(wx0, WS, W, p, lane);
  const size_t qcap = (size_t)H * STRIP_W;
  unsigned* const q = queue + (size_t)blockIdx.x * 3 * qcap;    // this strip's lists of deferred points: index, ix, iy
  if (tid == 0) qcount = 0u;

  float qu[2], qv[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int idx = min(rw + 4 * j, H - 1) * W + tl.cbase;
    qu[j] = srow(U + idx)[tl.lx]; qv[j] = srow(V + idx)[tl.lx];
  }
  const float lonc = lon_cells(srow(lon + tl.cbase)[tl.lx], g);

  // initial window: rows [lo(0), lo(0) + RW), two rounds of eight rows in flight
  float pre[STRIP_CH], pre2[STRIP_CH];
  const int lo0 = Ring::lo(0, p);
  for (int r8 = 0; r8 < RW; r8 += 2 * STRIP_ROWS) {
    strip_load_row(F, lo0 + r8 + wave, H, W, p, cs, nch, pre);
    if (r8 + STRIP_ROWS < RW) strip_load_row(F, lo0 + r8 + STRIP_ROWS + wave, H, W, p, cs, nch, pre2);
    strip_store_row(ring, lo0 + r8 + wave, RMASK, WS, H, p, m0, m1, lane, nch, pre);
    if (r8 + STRIP_ROWS < RW) strip_store_row(ring, lo0 + r8 + STRIP_ROWS + wave, RMASK, WS, H, p, m0, m1, lane, nch, pre2);
  }
  strip_load_row(F, lo0 + RW + wave, H, W, p, cs, nch, pre);      // the rows that enter at step 1
  __syncthreads();

  const float Hpf = (float)Hp, Wpf = (float)Wp, Wf = (float)W, wx0f = (float)wx0, WSf = (float)WS;
  for (int s = 0; s < nsteps; ++s) {
    const int lo = Ring::lo(s, p);
    // rows [lo + RW, lo + R): ring slots nobody reads during this step
    strip_store_row(ring, lo + RW + wave, RMASK, WS, H, p, m0, m1, lane, nch, pre);
    if (s + 1 < nsteps) strip_load_row(F, lo + R + wave, H, W, p, cs, nch, pre);
    const float rlof = (float)lo, rhif = (float)(lo + RW - 1);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int y = STRIP_ROWS * s + rw + 4 * j;          // wave-uniform
      const float cu = qu[j], cv = qv[j];
      {
        const int idx = min(y + STRIP_ROWS, H - 1) * W + tl.cbase;
        qu[j] = srow(U + idx)[tl.lx]; qv[j] = srow(V + idx)[tl.lx];
      }
      if (y < H) {
        const float sa = sin_lat[y * W], ca = cos_lat[y * W];
        float ix, iy, tx, ty;
        departure_row(cu, cv, sa, ca, lonc, lat_cells[y * W], g, ix, iy, nullptr);
        int r0, c0;
        const bool fast = tap_block_ring<MODE>(ix, iy, Hpf, Wpf, Wf, wx0f, WSf, rlof, rhif, tx, ty, r0, c0);
        // (a tap block outside the window reads a clamped, valid address; its value is dropped)
        float wx[NT], wy[NT];
        Interp<MODE>::weights(tx, wx);
        Interp<MODE>::weights(ty, wy);
        float acc = 0.f;
#pragma unroll
        for (int a = 0; a < NT; ++a) {
          const float* base = ring + ((r0 + a) & RMASK) * WS + c0;
          float rowacc = 0.f;
#pragma unroll
          for (int bb = 0; bb < NT; ++bb) rowacc = fmaf(base[bb], wx[bb], rowacc);
          acc = fmaf(rowacc, wy[a], acc);
        }
        if (tl.active && fast) srow(O + y * W + tl.cbase)[tl.lx] = acc;
        strip_defer(!fast && tl.active, (unsigned)(y * W + tl.cbase) + tl.lx, q, &qcount, lane, qcap, ix, iy);
      }
    }
    // raw barrier: __syncthreads() would also wait for this step's stores and the prefetches (s_waitcnt vmcnt(0))
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
  }
  if constexpr (STRIP_FWD_INLINE_FIXUP && R == 64) {
  // (large grids only: with the 32-row ring the extra code costs the kernel its 64-register fit, and the few deferred
  //  points of the 128-row grids are cheap in the second launch: 0.93 vs 0.96 ms per launch in the model)
  // The deferred points of this strip, densely, by the workgroup that listed them: while the other workgroups of the CU
  // are still in their row loops the scattered 4-byte loads of this phase overlap with their arithmetic, and the rows
  // it touches were streamed through the caches moments ago.  (The lists were written by this workgroup's own waves:
  // __syncthreads() drains the stores; no line of a list has been read before, so no stale L1 copy exists.)
  __syncthreads();
  {
    const unsigned n = qcount;
    const float* qx = reinterpret_cast<const float*>(q) + qcap;
    const float* qy = qx + qcap;
    for (unsigned i = tid; i < n; i += STRIP_THREADS)
      O[q[i]] = gather_global<MODE>(F, qx[i], qy[i], H, W, p, m0, m1);
  }
  if (tid == 0) counts[blockIdx.x] = 0u;
  } else {
    if (tid == 0) counts[blockIdx.x] = qcount;
  }
}

// Deferred points of the strips (tap block outside the ring window: the polar rows, and whatever moved further than the
// halos): every lane takes one point - the divergent slow path of rounds 1-3 ran the sixteen global loads of a point
// for every WAVE that held one; here the points of a strip are processed densely, in a launch of their own.
template <int MODE>
__global__ void __launch_bounds__(256)
sl_advect_fwd_strip_fixup(const float* __restrict__ field, const float* __restrict__ u, const float* __restrict__ v,
                          float* __restrict__ out, const float* __restrict__ sin_lat, const float* __restrict__ cos_lat,
                          const float* __restrict__ lon, const float* __restrict__ fmeans, int K, AdvGeom g, int64_t f_bs,
                          int64_t uv_bs, int64_t o_bs, int strips, const unsigned* __restrict__ queue,
                          const unsigned* __restrict__ counts) {
  const int H = g.H, W = g.W, p = g.p, P = H * W;
  const unsigned n = counts[blockIdx.x];
  if (n == 0) return;
  const int plane = blockIdx.x / strips;
  const int b = plane / K, k = plane - b * K;
  const float* F = field + (int64_t)b * f_bs + (int64_t)k * P;
  float* O = out + (int64_t)b * o_bs + (int64_t)k * P;
  const size_t qcap = (size_t)H * STRIP_W;
  const unsigned* q = queue + (size_t)blockIdx.x * 3 * qcap;
  const float* qx = reinterpret_cast<const float*>(q) + qcap;
  const float* qy = qx + qcap;
  const float m0 = fmeans[2 * plane], m1 = fmeans[2 * plane + 1];
  for (unsigned i = threadIdx.x; i < n; i += 256)
    O[q[i]] = gather_global<MODE>(F, qx[i], qy[i], H, W, p, m0, m1);
}

#ifdef PARADIS_DEV_KNOBS
// Diagnostic (round 6, verdict r5 item 5; development library only, PARADIS_ADVECT_DIRECT=4|8): the forward gather with NO LDS window - every tap a
// global load served by L2.  All workgroups of a plane run on ONE XCD (blockIdx % 8 = XCD; a 721 x 1440 plane is 4.15 MB,
// that XCD's L2 holds the band of rows in flight), a wave takes 64 points of one latitude row (scalar sa / ca as in the
// strips), a workgroup DROWS consecutive rows so that its waves share tap rows through the CU's L1.  Same departure
// point and tap arithmetic as the strips' deferred points (gather_global).  A/B (profiles/r06_advect_direct.txt, tools/advect_direct_ab.py):
// 2-3x slower than the strips with bicubic taps, 1.5x with bilinear, outputs identical.
template <int MODE, int DROWS>
__global__ void __launch_bounds__(64 * DROWS)
sl_advect_fwd_direct(const float* __restrict__ field, const float* __restrict__ u, const float* __restrict__ v,
                     float* __restrict__ out, const float* __restrict__ sin_lat, const float* __restrict__ cos_lat,
                     const float* __restrict__ lat_cells, const float* __restrict__ lon, const float* __restrict__ fmeans,
                     int K, AdvGeom g, int64_t f_bs, int64_t uv_bs, int64_t o_bs, int planes, int rgroups, int cblocks) {
  const int H = g.H, W = g.W, p = g.p, P = H * W;
  const int per_plane = rgroups * cblocks;
  const unsigned j = blockIdx.x >> 3;
  const int plane = (int)(j / per_plane) * 8 + (int)(blockIdx.x & 7);
  if (plane >= planes) return;
  const int t = (int)(j % per_plane), rg = t / cblocks, cb = t - rg * cblocks;
  const unsigned lane = threadIdx.x & 63;
  const int y = rg * DROWS + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (y >= H) return;
  const int b = plane / K, k = plane - b * K;
  const float* F = field + (int64_t)b * f_bs + (int64_t)k * P;
  const float* U = u + (int64_t)b * uv_bs + (int64_t)k * P;
  const float* V = v + (int64_t)b * uv_bs + (int64_t)k * P;
  float* O = out + (int64_t)b * o_bs + (int64_t)k * P;
  const int x = cb * 64 + (int)lane;
  const bool active = x < W;
  const unsigned xc = (unsigned)min(x, W - 1);
  const float cu = srow(U + y * W)[xc], cv = srow(V + y * W)[xc];
  const float lonc = lon_cells(srow(lon)[xc], g);
  const float sa = sin_lat[y * W], ca = cos_lat[y * W];
  float ix, iy;
  departure_row(cu, cv, sa, ca, lonc, lat_cells[y * W], g, ix, iy, nullptr);
  const float r = gather_global<MODE>(F, ix, iy, H, W, p, fmeans[2 * plane], fmeans[2 * plane + 1]);
  if (active) srow(O + y * W)[xc] = r;
}
#endif

// field gradient and coordinate gradients of a point whose tap block leaves the window: global atomics on the field
// gradient (float, or the integer plane of the deterministic mode), taps from global memory, one tap row at a time
template <int MODE, bool DET>
__device__ __forceinline__ void scatter_global(const float* __restrict__ F, float* __restrict__ GF,
                                               unsigned long long* __restrict__ GA, float ix, float iy, int H, int W,
                                               int p, float m0, float m1, float gval, float scale, float& gix, float& giy) {
  constexpr int NT = Interp<MODE>::NT;
  float tx, ty, wx[NT], wy[NT], dwx[NT], dwy[NT];
  int bx, by, sx, sy;
  tap_origin<MODE>(ix, iy, H + 2 * p, W + 2 * p, bx, by, sx, sy, tx, ty);
  Interp<MODE>::weights(tx, wx); Interp<MODE>::weights(ty, wy);
  Interp<MODE>::dweights(tx, dwx); Interp<MODE>::dweights(ty, dwy);
  shift_weights<NT>(wx, sx); shift_weights<NT>(dwx, sx);
  shift_weights<NT>(wy, sy); shift_weights<NT>(dwy, sy);
  TapCols<NT> m;
  tap_cols<NT>(bx, W, p, m);
  gix = 0.f; giy = 0.f;
#pragma unroll
  for (int a = 0; a < NT; ++a) {
    bool mir;
    int pole;
    const int ro = tap_row(by + a, H, W, p, mir, pole);
    float val[NT];
#pragma unroll
    for (int b = 0; b < NT; ++b) val[b] = F[ro + (mir ? m.colm[b] : m.col[b])];
    float sxv = 0.f, sdx = 0.f;
    const float gwy = gval * wy[a];
#pragma unroll
    for (int b = 0; b < NT; ++b) {
      const int cell = ro + (mir ? m.colm[b] : m.col[b]);
      const float t = pole == 1 ? m0 : (pole == 2 ? m1 : val[b]);
      if constexpr (DET) atomicAdd(&GA[cell], fixed_from_product((double)(gwy * scale), (double)wx[b]));
      else atomicAdd(&GF[cell], gwy * wx[b]);
      sxv = fmaf(t, wx[b], sxv);
      sdx = fmaf(t, dwx[b], sdx);
    }
    gix = fmaf(wy[a], sdx, gix);
    giy = fmaf(dwy[a], sxv, giy);
    asm volatile("" ::: "memory");
  }
}

// exponent e of the fixed-point scale 2^(40 - e) for a bound with bit pattern `bits` on |cotangent|: |g| < 2^e;
// 255 = a non-finite cotangent (every sum becomes NaN), -128 = all zero so far
__device__ __forceinline__ int fixed_exponent(unsigned bits) {
  if (bits >= 0x7f800000u) return 255;
  if (bits == 0) return -128;
  int e = (int)(bits >> 23) - 126;                  // 2^(e-1) <= |g| < 2^e for normal numbers
  return e < -80 ? -80 : (e > 80 ? 80 : e);
}

template <int MODE, int R, bool DET>
__global__ void __launch_bounds__(STRIP_THREADS, STRIP_BWD_WAVES)
sl_advect_bwd_strip(const float* __restrict__ gout, const float* __restrict__ field, const float* __restrict__ u,
                    const float* __restrict__ v, float* __restrict__ gfield, float* __restrict__ gu,
                    float* __restrict__ gv, const float* __restrict__ sin_lat, const float* __restrict__ cos_lat,
                    const float* __restrict__ lat_cells, const float* __restrict__ lon, const float* __restrict__ fmeans,
                    const float* __restrict__ gmeans, int K, AdvGeom g, int64_t go_bs, int64_t f_bs, int64_t uv_bs,
                    int64_t gf_bs, int64_t guv_bs, int hx, int strips, unsigned long long* __restrict__ gacc,
                    const unsigned* __restrict__ pmax, unsigned* __restrict__ queue, unsigned* __restrict__ counts,
                    const unsigned* __restrict__ wide) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  __shared__ unsigned qcount;
  // tall grids (round 5): the 32-row ring (63 KB: two workgroups per CU) for planes whose latitude displacements it
  // covers, the 64-row ring (126 KB: one) for the others - two launches back to back, a plane runs in the one its class
  // word names (adv_dy_class_kernel), the other returns at once; NULL = this launch takes every plane
  if (wide != nullptr && (wide[blockIdx.x / strips] != 0u) != (R == 64)) return;
  using Ring = StripRing<MODE, R>;
  constexpr int NT = Interp<MODE>::NT, RW = Ring::RW, RMASK = R - 1;
  const int H = g.H, W = g.W, p = g.p, P = H * W, Hp = H + 2 * p, Wp = W + 2 * p;
  const int tid = threadIdx.x;
  const unsigned lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int plane = blockIdx.x / strips, strip = blockIdx.x - plane * strips;
  const int b = plane / K, k = plane - b * K;
  const float* F = field + (int64_t)b * f_bs + (int64_t)k * P;
  const float* U = u + (int64_t)b * uv_bs + (int64_t)k * P;
  const float* V = v + (int64_t)b * uv_bs + (int64_t)k * P;
  const float* GO = gout + (int64_t)b * go_bs + (int64_t)k * P;
  float* GF = gfield + (int64_t)b * gf_bs + (int64_t)k * P;
  float* GU = gu + (int64_t)b * guv_bs + (int64_t)k * P;
  float* GV = gv + (int64_t)b * guv_bs + (int64_t)k * P;
  unsigned long long* GA = DET ? gacc + (int64_t)plane * P : nullptr;
  const int x0 = strip * STRIP_W, tw = min(STRIP_W, W - x0);
  const int WS = STRIP_W + 2 * hx + NT, wx0 = x0 + p - hx, nch = (WS + 63) >> 6;
  const int wn = R * WS;
  unsigned long long* acc = reinterpret_cast<unsigned long long*>(smem);    // [R][WS] fixed-point sums
  float* ring = smem + 2 * wn;                                               // [R][WS] field window
  unsigned* stepmax = reinterpret_cast<unsigned*>(ring + wn);                // [3] max |cotangent| bits of a step
  const float m0 = fmeans[2 * plane], m1 = fmeans[2 * plane + 1];
  const float gm0 = gmeans[2 * plane], gm1 = gmeans[2 * plane + 1];
  const StripLane tl(wave & 1, lane, x0, tw, W);
  const int rw = wave >> 1;
  const int nsteps = (H + STRIP_ROWS - 1) / STRIP_ROWS;
  const StripCols cs = strip_cols(wx0, WS, W, p, lane);
  unsigned* const q = queue + (size_t)blockIdx.x * 3 * (size_t)(H * STRIP_W);    // deferred points (see the forward)
  if (tid == 0) qcount = 0u;

  float qu[2], qv[2], qg[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int idx = min(rw + 4 * j, H - 1) * W + tl.cbase;
    qu[j] = srow(U + idx)[tl.lx]; qv[j] = srow(V + idx)[tl.lx]; qg[j] = srow(GO + idx)[tl.lx];
  }
  const float lonc = lon_cells(srow(lon + tl.cbase)[tl.lx], g);

  for (int i = tid; i < wn; i += STRIP_THREADS) acc[i] = 0ull;
  if (tid < 3) stepmax[tid] = 0u;
  float pre[STRIP_CH], pre2[STRIP_CH];
  const int lo0 = Ring::lo(0, p);
  for (int r8 = 0; r8 < RW; r8 += 2 * STRIP_ROWS) {
    strip_load_row(F, lo0 + r8 + wave, H, W, p, cs, nch, pre);
    if (r8 + STRIP_ROWS < RW) strip_load_row(F, lo0 + r8 + STRIP_ROWS + wave, H, W, p, cs, nch, pre2);
    strip_store_row(ring, lo0 + r8 + wave, RMASK, WS, H, p, m0, m1, lane, nch, pre);
    if (r8 + STRIP_ROWS < RW) strip_store_row(ring, lo0 + r8 + STRIP_ROWS + wave, RMASK, WS, H, p, m0, m1, lane, nch, pre2);
  }
  strip_load_row(F, lo0 + RW + wave, H, W, p, cs, nch, pre);
  __syncthreads();
  // bound on |cotangent| of step 0 (the pole rows' means ride along: they are what pole rows scatter)
  {
    unsigned mb = max(abs_bits(gm0), abs_bits(gm1));
#pragma unroll
    for (int j = 0; j < 2; ++j) mb = max(mb, abs_bits(qg[j]));
    mb = wave_umax_lane63(mb);
    if (lane == 63) atomicMax(&stepmax[0], mb);
  }
  __syncthreads();

  int ecur = DET ? fixed_exponent(pmax[plane]) : -128;      // exponent of the ring's accumulators (wave-uniform)
  float scale = 0.f, inv_scale = 0.f;
  auto set_scale = [&](int e) {
    ecur = e;
    if (e == 255) { scale = 0.f; inv_scale = NAN; }
    else if (e == -128) { scale = 0.f; inv_scale = 0.f; }
    else { scale = ldexpf(1.0f, 40 - e); inv_scale = ldexpf(1.0f, e - 40); }
  };
  set_scale(ecur);

  // flush padded row pr of the ring (complete: no later arrival row reaches it) and clear its accumulators
  auto flush_row = [&](int pr) {
    const StripRow r = strip_row(pr, H, p);
    unsigned long long* arow = acc + (pr & RMASK) * WS;
    const double inv = (double)inv_scale;
#pragma unroll
    for (int i = 0; i < STRIP_CH; ++i)
      if (i < nch) {
        const int lc = (int)lane + 64 * i;
        if (lc < WS) {
          const long long sv = (long long)arow[lc];
          if (sv != 0) {
            arow[lc] = 0ull;
            if (r.valid) {
              const int cell = r.sr * W + (int)(r.mir ? (cs.pk[i] >> 16) : (cs.pk[i] & 0xffffu));
              if constexpr (DET) atomicAdd(&GA[cell], (unsigned long long)sv);
              else atomicAdd(&GF[cell], (float)((double)sv * inv));
            }
          }
        }
      }
  };

  const float Hpf = (float)Hp, Wpf = (float)Wp, Wf = (float)W, wx0f = (float)wx0, WSf = (float)WS;
  for (int s = 0; s < nsteps; ++s) {
    const int lo = Ring::lo(s, p);
    if constexpr (!DET) {
      // the scale follows the running maximum of |cotangent|: a step that raises it shifts every accumulator of the
      // ring down to the new exponent (rare: once per strip on smooth cotangents)
      const int e = fixed_exponent(stepmax[s % 3]);
      if (e > ecur) {
        if (ecur != -128 && e != 255) {
          const int sh = min(e - ecur, 63);
          for (int i = tid; i < wn; i += STRIP_THREADS) acc[i] = (unsigned long long)((long long)acc[i] >> sh);
        }
        set_scale(e);
        __syncthreads();
      }
      if (tid == 0) stepmax[(s + 2) % 3] = 0u;
    }
    // rows that left the window after step s - 1 go out; the rows entering at step s + 1 take their slots
    if (s > 0) flush_row(lo - STRIP_ROWS + wave);
    strip_store_row(ring, lo + RW + wave, RMASK, WS, H, p, m0, m1, lane, nch, pre);
    if (s + 1 < nsteps) strip_load_row(F, lo + R + wave, H, W, p, cs, nch, pre);
    const float rlof = (float)lo, rhif = (float)(lo + RW - 1);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int y = STRIP_ROWS * s + rw + 4 * j;          // wave-uniform
      const float cu = qu[j], cv = qv[j], cgo = qg[j];
      {
        const int idx = min(y + STRIP_ROWS, H - 1) * W + tl.cbase;
        qu[j] = srow(U + idx)[tl.lx]; qv[j] = srow(V + idx)[tl.lx]; qg[j] = srow(GO + idx)[tl.lx];
      }
      if (y < H) {
        const float sa = sin_lat[y * W], ca = cos_lat[y * W];
        float ix, iy, tx, ty;
        DepState st;
        departure_row(cu, cv, sa, ca, lonc, lat_cells[y * W], g, ix, iy, &st);
        int r0, c0;
        const bool fast = tap_block_ring<MODE>(ix, iy, Hpf, Wpf, Wf, wx0f, WSf, rlof, rhif, tx, ty, r0, c0);
        const float gval = (y == 0) ? gm0 : ((y == H - 1) ? gm1 : cgo);
        float gix = 0.f, giy = 0.f;
        // (the sample coordinates ride along, as in the forward: the fix-up evaluates the gradient where the forward sampled)
        strip_defer(!fast && tl.active, (unsigned)(y * W + tl.cbase) + tl.lx, q, &qcount, lane, (size_t)H * STRIP_W, ix, iy);
        if (tl.active && fast) {
          {
            float wx[NT], wy[NT], dwx[NT], dwy[NT];
            Interp<MODE>::weights(tx, wx); Interp<MODE>::weights(ty, wy);
            Interp<MODE>::dweights(tx, dwx); Interp<MODE>::dweights(ty, dwy);
            const float gs_ = gval * scale;
            double wxd[NT];
#pragma unroll
            for (int bb = 0; bb < NT; ++bb) wxd[bb] = (double)wx[bb];
#pragma unroll
            for (int a = 0; a < NT; ++a) {
              const int rb = ((r0 + a) & RMASK) * WS + c0;
              float sxv = 0.f, sdx = 0.f;
              const double gwy = (double)(gs_ * wy[a]);
#pragma unroll
              for (int bb = 0; bb < NT; ++bb) {
                const float val = ring[rb + bb];
                atomicAdd(&acc[rb + bb], fixed_from_product(gwy, wxd[bb]));
                sxv = fmaf(val, wx[bb], sxv);
                sdx = fmaf(val, dwx[bb], sdx);
              }
              gix = fmaf(wy[a], sdx, gix);
              giy = fmaf(dwy[a], sxv, giy);
            }
          }
          float guv, gvv;
          departure_backward(st, sa, ca, gix * gval, giy * gval, g, guv, gvv);
          srow(GU + y * W + tl.cbase)[tl.lx] = guv;
          srow(GV + y * W + tl.cbase)[tl.lx] = gvv;
        }
      }
    }
    if constexpr (!DET) {
      // |cotangent| of the next step (prefetched above), published by the barrier
      unsigned mb = max(abs_bits(qg[0]), abs_bits(qg[1]));
      mb = wave_umax_lane63(mb);
      if (lane == 63 && s + 1 < nsteps) atomicMax(&stepmax[(s + 1) % 3], mb);
    }
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");     // (raw: the stores and atomics stay in flight)
  }
  // what is still resident: the window of the last step
  const int lo_last = Ring::lo(nsteps - 1, p);
  for (int r8 = 0; r8 < RW; r8 += STRIP_ROWS) flush_row(lo_last + r8 + wave);
  if (tid == 0) counts[blockIdx.x] = qcount;
}

// Backward on grids of at most 256 longitudes (configs[3]): the ring spans the WHOLE latitude circle (window column lc
// holds image column lc mod W, the first NT columns repeated behind the last), one workgroup per plane.  No tap leaves
// the window in longitude - the polar rows, whose departure points lie anywhere on their circle, stay on the LDS path -
// and no other workgroup writes this plane: the rows leaving the ring are folded onto their source cells IN LDS (the
// wrap columns onto columns 0..NT-1, the rows beyond a pole onto their mirror rows, half a circle away) and go out as
// plain 256-byte stores.  Against the 128-column strips: no float atomics (the strips' flush ran at the chip's
// 1.3 TB/s atomic rate), no zero fill of the gradient, 1.02 instead of 1.19 window cells per point.
// 4 WPR waves: WPR 64-column segments per row, two rows per wave and step.
template <int MODE, int R, int WPR, bool FLDS>
__global__ void __launch_bounds__(256 * WPR)
sl_advect_bwd_circle(const float* __restrict__ gout, const float* __restrict__ field, const float* __restrict__ u,
                     const float* __restrict__ v, float* __restrict__ gfield, float* __restrict__ gu,
                     float* __restrict__ gv, const float* __restrict__ sin_lat, const float* __restrict__ cos_lat,
                     const float* __restrict__ lat_cells, const float* __restrict__ lon, const float* __restrict__ fmeans,
                     const float* __restrict__ gmeans, int K, AdvGeom g, int64_t go_bs, int64_t f_bs, int64_t uv_bs,
                     int64_t gf_bs, int64_t guv_bs, int strips, unsigned* __restrict__ queue, unsigned* __restrict__ counts,
                     const unsigned* __restrict__ wide) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  __shared__ unsigned qcount;
  using Ring = StripRing<MODE, R>;
  constexpr int NT = Interp<MODE>::NT, RW = Ring::RW, RMASK = R - 1, NTHREADS = 256 * WPR, SUBS = WPR / 2;
  const int H = g.H, W = g.W, p = g.p, P = H * W, Hp = H + 2 * p, Wp = W + 2 * p;
  const int tid = threadIdx.x;
  const unsigned lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int plane = blockIdx.x;
  // two variants of this kernel are launched back to back; a plane runs in the one its displacement class names
  // (adv_dy_class_kernel: sampled max |v dt| in rows), the other one returns at once
  if ((wide[plane] != 0u) == FLDS) return;
  const int b = plane / K, k = plane - b * K;
  const float* F = field + (int64_t)b * f_bs + (int64_t)k * P;
  const float* U = u + (int64_t)b * uv_bs + (int64_t)k * P;
  const float* V = v + (int64_t)b * uv_bs + (int64_t)k * P;
  const float* GO = gout + (int64_t)b * go_bs + (int64_t)k * P;
  float* GF = gfield + (int64_t)b * gf_bs + (int64_t)k * P;
  float* GU = gu + (int64_t)b * guv_bs + (int64_t)k * P;
  float* GV = gv + (int64_t)b * guv_bs + (int64_t)k * P;
  const int WS = W + NT, wx0 = p;
  const int wn = R * WS;
  unsigned long long* acc = reinterpret_cast<unsigned long long*>(smem);    // [R][WS] fixed-point sums
  float* ring = smem + 2 * wn;                                               // [R][WS] field window (FLDS only)
  unsigned* stepmax = reinterpret_cast<unsigned*>(ring + (FLDS ? wn : 0));   // [3] max |cotangent| bits of a step
  const float m0 = fmeans[2 * plane], m1 = fmeans[2 * plane + 1];
  const float gm0 = gmeans[2 * plane], gm1 = gmeans[2 * plane + 1];
  const StripLane tl(wave % WPR, lane, 0, W, W);
  const int rw = wave / WPR;                         // rows rw and rw + 4 of a step
  const int nsteps = (H + STRIP_ROWS - 1) / STRIP_ROWS;
  // staging / flushing: wave -> ring row (wave & 7), 64-column chunks [cfirst, cfirst + nch) of the window row
  const int srw = wave & 7, sub = wave >> 3;
  const int nch_all = (WS + 63) >> 6, per = (nch_all + SUBS - 1) / SUBS;
  const int cfirst = sub * per, nch = max(0, min(per, nch_all - cfirst));
  const StripCols cs = strip_cols(wx0, WS, W, p, lane, cfirst);
  unsigned* const q = queue + (size_t)plane * strips * 3 * (size_t)(H * STRIP_W);   // deferred points: |dy| beyond the ring
  if (tid == 0) qcount = 0u;

  float qu[2], qv[2], qg[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int idx = min(rw + 4 * j, H - 1) * W + tl.cbase;
    qu[j] = srow(U + idx)[tl.lx]; qv[j] = srow(V + idx)[tl.lx]; qg[j] = srow(GO + idx)[tl.lx];
  }
  const float lonc = lon_cells(srow(lon + tl.cbase)[tl.lx], g);

  for (int i = tid; i < wn; i += NTHREADS) acc[i] = 0ull;
  if (tid < 3) stepmax[tid] = 0u;
  float pre[STRIP_CH];
  const int lo0 = Ring::lo(0, p);
  if constexpr (FLDS) {
    for (int r8 = 0; r8 < RW; r8 += STRIP_ROWS) {
      strip_load_row(F, lo0 + r8 + srw, H, W, p, cs, nch, pre);
      strip_store_row(ring, lo0 + r8 + srw, RMASK, WS, H, p, m0, m1, lane, nch, pre, cfirst);
    }
    strip_load_row(F, lo0 + RW + srw, H, W, p, cs, nch, pre);
  }
  __syncthreads();
  {
    unsigned mb = max(abs_bits(gm0), abs_bits(gm1));
#pragma unroll
    for (int j = 0; j < 2; ++j) mb = max(mb, abs_bits(qg[j]));
    mb = wave_umax_lane63(mb);
    if (lane == 63) atomicMax(&stepmax[0], mb);
  }
  __syncthreads();

  int ecur = -128;
  float scale = 0.f, inv_scale = 0.f;
  auto set_scale = [&](int e) {
    ecur = e;
    if (e == 255) { scale = 0.f; inv_scale = NAN; }
    else if (e == -128) { scale = 0.f; inv_scale = 0.f; }
    else { scale = ldexpf(1.0f, 40 - e); inv_scale = ldexpf(1.0f, e - 40); }
  };

  // a row beyond a pole: its sums belong to the mirror row, half a circle away, which is still in the ring
  auto fold_row = [&](int pr) {
    const StripRow r = strip_row(pr, H, p);
    if (!(r.valid && r.mir)) return;                       // wave-uniform
    unsigned long long* arow = acc + (pr & RMASK) * WS;
    unsigned long long* trow = acc + ((r.sr + p) & RMASK) * WS;
#pragma unroll
    for (int i = 0; i < STRIP_CH; ++i)
      if (i < nch) {
        const int lc = (int)lane + 64 * (cfirst + i);
        if (lc < WS) {
          const unsigned long long sv = arow[lc];
          if (sv != 0ull) {
            arow[lc] = 0ull;
            atomicAdd(&trow[cs.pk[i] >> 16], sv);
          }
        }
      }
  };
  // a source row leaves complete: wrap columns folded in, plain stores (every cell of the plane is written once)
  auto flush_row = [&](int pr) {
    const StripRow r = strip_row(pr, H, p);
    if (!r.valid || r.mir) return;                          // wave-uniform
    unsigned long long* arow = acc + (pr & RMASK) * WS;
    const double inv = (double)inv_scale;
    const global_ptr<float> dst = srow(GF + (int64_t)r.sr * W);
#pragma unroll
    for (int i = 0; i < STRIP_CH; ++i)
      if (i < nch) {
        const int j = (int)lane + 64 * (cfirst + i);
        if (j < W) {
          long long sv = (long long)arow[j];
          arow[j] = 0ull;
          if (j < NT) { sv += (long long)arow[j + W]; arow[j + W] = 0ull; }
          dst[j] = (float)((double)sv * inv);
        }
      }
  };

  const float Hpf = (float)Hp, Wpf = (float)Wp, Wf = (float)W, wx0f = (float)wx0, WSf = (float)WS;
  for (int s = 0; s < nsteps; ++s) {
    const int lo = Ring::lo(s, p);
    {
      const int e = fixed_exponent(stepmax[s % 3]);
      if (e > ecur) {
        if (ecur != -128 && e != 255) {
          const int sh = min(e - ecur, 63);
          for (int i = tid; i < wn; i += NTHREADS) acc[i] = (unsigned long long)((long long)acc[i] >> sh);
        }
        set_scale(e);
        __syncthreads();
      }
      if (tid == 0) stepmax[(s + 2) % 3] = 0u;
    }
    if (s > 0) {
      // (a row beyond the south pole and its mirror row never leave in the same group of eight: lo(s) = -5 mod 8)
      fold_row(lo - STRIP_ROWS + srw);
      flush_row(lo - STRIP_ROWS + srw);
    }
    if constexpr (FLDS) {
      strip_store_row(ring, lo + RW + srw, RMASK, WS, H, p, m0, m1, lane, nch, pre, cfirst);
      if (s + 1 < nsteps) strip_load_row(F, lo + R + srw, H, W, p, cs, nch, pre);
    }
    const float rlof = (float)lo, rhif = (float)(lo + RW - 1);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int y = STRIP_ROWS * s + rw + 4 * j;          // wave-uniform
      const float cu = qu[j], cv = qv[j], cgo = qg[j];
      {
        const int idx = min(y + STRIP_ROWS, H - 1) * W + tl.cbase;
        qu[j] = srow(U + idx)[tl.lx]; qv[j] = srow(V + idx)[tl.lx]; qg[j] = srow(GO + idx)[tl.lx];
      }
      if (y < H) {
        const float sa = sin_lat[y * W], ca = cos_lat[y * W];
        float ix, iy, tx, ty;
        DepState st;
        departure_row(cu, cv, sa, ca, lonc, lat_cells[y * W], g, ix, iy, &st);
        int r0, c0;
        const bool fast = tap_block_ring<MODE>(ix, iy, Hpf, Wpf, Wf, wx0f, WSf, rlof, rhif, tx, ty, r0, c0);
        const float gval = (y == 0) ? gm0 : ((y == H - 1) ? gm1 : cgo);
        float gix = 0.f, giy = 0.f;
        // (the sample coordinates ride along, as in the forward: the fix-up evaluates the gradient where the forward sampled)
        strip_defer(!fast && tl.active, (unsigned)(y * W + tl.cbase) + tl.lx, q, &qcount, lane, (size_t)strips * H * STRIP_W, ix, iy);   // (one list per plane: three lists of strips x H x 128 entries)
        if (tl.active && fast) {
          float wx[NT], wy[NT], dwx[NT], dwy[NT];
          Interp<MODE>::weights(tx, wx); Interp<MODE>::weights(ty, wy);
          Interp<MODE>::dweights(tx, dwx); Interp<MODE>::dweights(ty, dwy);
          const float gs_ = gval * scale;
          double wxd[NT];
#pragma unroll
          for (int bb = 0; bb < NT; ++bb) wxd[bb] = (double)wx[bb];
          int fcol[NT], fcolm[NT];           // !FLDS: the field taps come from global memory (L1 / L2)
          if constexpr (!FLDS) {
#pragma unroll
            for (int bb = 0; bb < NT; ++bb) {
              int j = c0 + bb;                // window column = image column (wx0 = p), wrap columns behind W
              j -= j >= W ? W : 0;
              int jm = j + (W >> 1);
              jm -= jm >= W ? W : 0;
              fcol[bb] = j; fcolm[bb] = jm;
            }
          }
#pragma unroll
          for (int a = 0; a < NT; ++a) {
            const int rb = ((r0 + a) & RMASK) * WS + c0;
            float sxv = 0.f, sdx = 0.f;
            const double gwy = (double)(gs_ * wy[a]);
            float fval[NT];
            if constexpr (!FLDS) {
              bool mir;
              int pole;
              const int ro = tap_row(r0 + a, H, W, p, mir, pole);
#pragma unroll
              for (int bb = 0; bb < NT; ++bb) fval[bb] = F[ro + (mir ? fcolm[bb] : fcol[bb])];
#pragma unroll
              for (int bb = 0; bb < NT; ++bb) fval[bb] = pole == 1 ? m0 : (pole == 2 ? m1 : fval[bb]);
            }
#pragma unroll
            for (int bb = 0; bb < NT; ++bb) {
              const float val = FLDS ? ring[rb + bb] : fval[bb];
              atomicAdd(&acc[rb + bb], fixed_from_product(gwy, wxd[bb]));
              sxv = fmaf(val, wx[bb], sxv);
              sdx = fmaf(val, dwx[bb], sdx);
            }
            gix = fmaf(wy[a], sdx, gix);
            giy = fmaf(dwy[a], sxv, giy);
          }
          float guv, gvv;
          departure_backward(st, sa, ca, gix * gval, giy * gval, g, guv, gvv);
          srow(GU + y * W + tl.cbase)[tl.lx] = guv;
          srow(GV + y * W + tl.cbase)[tl.lx] = gvv;
        }
      }
    }
    {
      unsigned mb = max(abs_bits(qg[0]), abs_bits(qg[1]));
      mb = wave_umax_lane63(mb);
      if (lane == 63 && s + 1 < nsteps) atomicMax(&stepmax[(s + 1) % 3], mb);
    }
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
  }
  // what is still resident: first the rows beyond the poles onto their mirror rows, then the source rows
  const int lo_last = Ring::lo(nsteps - 1, p);
  for (int r8 = 0; r8 < RW; r8 += STRIP_ROWS) fold_row(lo_last + r8 + srw);
  __syncthreads();
  for (int r8 = 0; r8 < RW; r8 += STRIP_ROWS) flush_row(lo_last + r8 + srw);
  if (tid < strips) counts[(size_t)plane * strips + tid] = tid == 0 ? qcount : 0u;
}

// displacement class of a plane for the full-circle backward: 1 when more than 1/16 of the sampled points (every fourth
// row) move further in latitude than the ring of the field-in-LDS variant covers.  Such points are deferred to sixteen
// global float atomics each (~60 ps per point against ~14 in the ring): beyond ~9 % of them the 64-row variant, 35 %
// slower per point, wins.  A heuristic that only selects between two correct kernels.
__global__ void __launch_bounds__(256)
adv_dy_class_kernel(const float* __restrict__ v, unsigned* __restrict__ wide, int K, int H, int W, int64_t bs,
                    float thresh) {
  __shared__ unsigned red[4];
  const int plane = blockIdx.x, b = plane / K, k = plane - b * K;
  const float* V = v + (int64_t)b * bs + (int64_t)k * H * W;
  unsigned far = 0;
  for (int y = 0; y < H; y += 4)
    for (int x = threadIdx.x; x < W; x += 256) far += !(fabsf(V[y * W + x]) <= thresh) ? 1u : 0u;   // (a NaN counts as far)
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) far += (unsigned)__shfl_xor((int)far, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = far;
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned f = red[0] + red[1] + red[2] + red[3];
    const unsigned t = (unsigned)((H + 3) / 4) * (unsigned)W;      // points sampled
    wide[plane] = 16ull * f > t ? 1u : 0u;
  }
}

// the deferred points of the backward strips, one per lane: field gradient by global atomics, velocity gradients
template <int MODE, bool DET>
__global__ void __launch_bounds__(256)
sl_advect_bwd_strip_fixup(const float* __restrict__ gout, const float* __restrict__ field, const float* __restrict__ u,
                          const float* __restrict__ v, float* __restrict__ gfield, float* __restrict__ gu,
                          float* __restrict__ gv, const float* __restrict__ sin_lat, const float* __restrict__ cos_lat,
                          const float* __restrict__ lon, const float* __restrict__ fmeans, const float* __restrict__ gmeans,
                          int K, AdvGeom g, int64_t go_bs, int64_t f_bs, int64_t uv_bs, int64_t gf_bs, int64_t guv_bs,
                          int strips, unsigned long long* __restrict__ gacc, const unsigned* __restrict__ pmax,
                          const unsigned* __restrict__ queue, const unsigned* __restrict__ counts, int lists_per_plane) {
  // lists_per_plane: `strips` (one list per strip, capacity H x 128) or 1 (the full-circle kernel: one list per plane
  // at the plane's first strip, capacity strips x H x 128)
  const int H = g.H, W = g.W, p = g.p, P = H * W;
  const unsigned n = counts[blockIdx.x];
  if (n == 0) return;
  const int plane = blockIdx.x / strips;
  const int b = plane / K, k = plane - b * K;
  const float* F = field + (int64_t)b * f_bs + (int64_t)k * P;
  const float* U = u + (int64_t)b * uv_bs + (int64_t)k * P;
  const float* V = v + (int64_t)b * uv_bs + (int64_t)k * P;
  const float* GO = gout + (int64_t)b * go_bs + (int64_t)k * P;
  float* GF = gfield + (int64_t)b * gf_bs + (int64_t)k * P;
  float* GU = gu + (int64_t)b * guv_bs + (int64_t)k * P;
  float* GV = gv + (int64_t)b * guv_bs + (int64_t)k * P;
  unsigned long long* GA = DET ? gacc + (int64_t)plane * P : nullptr;
  const size_t qcap1 = (size_t)H * STRIP_W, qcap = lists_per_plane == 1 ? qcap1 * strips : qcap1;
  const unsigned* q = queue + (size_t)blockIdx.x * 3 * qcap1;
  const float* qx = reinterpret_cast<const float*>(q) + qcap;
  const float* qy = qx + qcap;
  const float m0 = fmeans[2 * plane], m1 = fmeans[2 * plane + 1];
  const float gm0 = gmeans[2 * plane], gm1 = gmeans[2 * plane + 1];
  float scale = 0.f;
  if constexpr (DET) {
    float inv;
    fixed_point_scale(__uint_as_float(pmax[plane]), scale, inv);
  }
  const unsigned last = (unsigned)(H - 1) * (unsigned)W;
  for (unsigned i = threadIdx.x; i < n; i += 256) {
    const unsigned idx = q[i];
    const float sa = sin_lat[idx], ca = cos_lat[idx];
    float ix_l, iy_l, gix, giy;
    DepState st;
    // the chain-rule state of the departure map, per lane (no wave-uniform branches: a list's order, and with it a
    // point's wave mates, varies from run to run).  The tap block and the weights are those of the coordinates the
    // strip kernel computed, decided on and stored - the ones the forward sampled at (departure_lane's own
    // coordinates differ from them in the last bits, which a polar point amplified to 2e-4 of its velocity gradient)
    departure_lane(U[idx], V[idx], sa, ca, lon_cells(lon[idx], g), g, ix_l, iy_l, &st);
    const float ix = qx[i], iy = qy[i];
    const float gval = idx < (unsigned)W ? gm0 : (idx >= last ? gm1 : GO[idx]);
    scatter_global<MODE, DET>(F, GF, GA, ix, iy, H, W, p, m0, m1, gval, scale, gix, giy);
    float guv, gvv;
    departure_backward(st, sa, ca, gix * gval, giy * gval, g, guv, gvv);
    GU[idx] = guv;
    GV[idx] = gvv;
  }
}

// ---- kernel tables: the reservation iterates them, the launch indexes them; first index adv_mode_index(mode) ----------
constexpr int BL = PARADIS_INTERP_BILINEAR, BC = PARADIS_INTERP_BICUBIC;
using StripFwdKernel = decltype(&sl_advect_fwd_strip<BL, 32>);
constexpr StripFwdKernel STRIP_FWD[2][2] = {      // [mode][ring rows: 32, 64]
    {&sl_advect_fwd_strip<BL, 32>, &sl_advect_fwd_strip<BL, 64>}, {&sl_advect_fwd_strip<BC, 32>, &sl_advect_fwd_strip<BC, 64>}};
using StripFwdFixupKernel = decltype(&sl_advect_fwd_strip_fixup<BL>);
constexpr StripFwdFixupKernel STRIP_FWD_FIXUP[2] = {&sl_advect_fwd_strip_fixup<BL>, &sl_advect_fwd_strip_fixup<BC>};
using StripBwdKernel = decltype(&sl_advect_bwd_strip<BL, 32, false>);
constexpr StripBwdKernel STRIP_BWD[2][2][2] = {   // [mode][ring rows: 32, 64][deterministic]
    {{&sl_advect_bwd_strip<BL, 32, false>, &sl_advect_bwd_strip<BL, 32, true>},
     {&sl_advect_bwd_strip<BL, 64, false>, &sl_advect_bwd_strip<BL, 64, true>}},
    {{&sl_advect_bwd_strip<BC, 32, false>, &sl_advect_bwd_strip<BC, 32, true>},
     {&sl_advect_bwd_strip<BC, 64, false>, &sl_advect_bwd_strip<BC, 64, true>}}};
using StripBwdFixupKernel = decltype(&sl_advect_bwd_strip_fixup<BL, false>);
constexpr StripBwdFixupKernel STRIP_BWD_FIXUP[2][2] = {   // [mode][deterministic]
    {&sl_advect_bwd_strip_fixup<BL, false>, &sl_advect_bwd_strip_fixup<BL, true>},
    {&sl_advect_bwd_strip_fixup<BC, false>, &sl_advect_bwd_strip_fixup<BC, true>}};
using CircleKernel = decltype(&sl_advect_bwd_circle<BL, 32, 2, true>);
enum { CIRCLE_R32 = 0, CIRCLE_R64 = 1, CIRCLE_R64_SUMS = 2 };   // field and sums in a ring of 32 / 64 rows; the sums alone in 64 rows
constexpr CircleKernel CIRCLE_BWD[2][2][3] = {    // [mode][waves per row: 2, 4][variant]
    {{&sl_advect_bwd_circle<BL, 32, 2, true>, &sl_advect_bwd_circle<BL, 64, 2, true>, &sl_advect_bwd_circle<BL, 64, 2, false>},
     {&sl_advect_bwd_circle<BL, 32, 4, true>, &sl_advect_bwd_circle<BL, 64, 4, true>, &sl_advect_bwd_circle<BL, 64, 4, false>}},
    {{&sl_advect_bwd_circle<BC, 32, 2, true>, &sl_advect_bwd_circle<BC, 64, 2, true>, &sl_advect_bwd_circle<BC, 64, 2, false>},
     {&sl_advect_bwd_circle<BC, 32, 4, true>, &sl_advect_bwd_circle<BC, 64, 4, true>, &sl_advect_bwd_circle<BC, 64, 4, false>}}};
#ifdef PARADIS_DEV_KNOBS
using DirectKernel = decltype(&sl_advect_fwd_direct<BL, 4>);
constexpr DirectKernel DIRECT_FWD[2][2] = {       // [mode][rows per workgroup: 4, 8]
    {&sl_advect_fwd_direct<BL, 4>, &sl_advect_fwd_direct<BL, 8>}, {&sl_advect_fwd_direct<BC, 4>, &sl_advect_fwd_direct<BC, 8>}};
#endif

}  // namespace

int pd_adv_fwd_strips(const AdvArgs& a) {
  const AdvGeom g = make_geom(a);
  const int NT = 2 * g.p, planes = a.B * a.K, m = adv_mode_index(a.mode);
  // ring of R padded rows, longitude halo hx (flags: PARADIS_ADVECT_HALO)
  const int ring = strip_ring_rows(a.H), hx = halo_of(a.flags, strip_halo_fwd(a.W), false);
  const int strips = (a.W + STRIP_W - 1) / STRIP_W;
  const size_t slds = (size_t)ring * (STRIP_W + 2 * hx + NT) * sizeof(float);
  PD_REQUIRE((int64_t)planes * strips < (1ll << 31), "sl_advect_fwd: too many strips");
  PD_REQUIRE(STRIP_W + 2 * hx + NT <= STRIP_MAX_WS, "sl_advect_fwd: halo too wide");
  static PerDeviceOnce once;
  if (int e = reserve_lds(once, STRIP_FWD, "sl_advect_fwd", STRIP_LDS_MAX)) return e;
  const dim3 grid((unsigned)(planes * strips));
  hipLaunchKernelGGL(STRIP_FWD[m][ring == 64], grid, dim3(STRIP_THREADS), slds, a.st, a.field, a.u, a.v, a.out, a.sin_lat,
                     a.cos_lat, a.lat_cells, a.lon, a.fmeans, a.K, g, a.f_bs, a.uv_bs, a.o_bs, hx, strips, a.queue, a.counts);
  // the points whose tap block left the window, densely
  hipLaunchKernelGGL(STRIP_FWD_FIXUP[m], grid, dim3(256), 0, a.st, a.field, a.u, a.v, a.out, a.sin_lat, a.cos_lat, a.lon,
                     a.fmeans, a.K, g, a.f_bs, a.uv_bs, a.o_bs, strips, a.queue, a.counts);
  return 0;
}

#ifdef PARADIS_DEV_KNOBS
int pd_adv_fwd_direct(const AdvArgs& a, int rows) {
  const AdvGeom g = make_geom(a);
  const int planes = a.B * a.K;
  const int drows = rows >= 8 ? 8 : 4, rgroups = (a.H + drows - 1) / drows, cblocks = (a.W + 63) / 64;
  const int64_t nwg = (int64_t)((planes + 7) / 8) * 8 * rgroups * cblocks;
  PD_REQUIRE(nwg < (1ll << 31), "sl_advect_fwd(direct): too many workgroups");
  hipLaunchKernelGGL(DIRECT_FWD[adv_mode_index(a.mode)][drows == 8], dim3((unsigned)nwg), dim3(64 * drows), 0, a.st, a.field,
                     a.u, a.v, a.out, a.sin_lat, a.cos_lat, a.lat_cells, a.lon, a.fmeans, a.K, g, a.f_bs, a.uv_bs, a.o_bs,
                     planes, rgroups, cblocks);
  return 0;
}
#endif

// Full-circle ring, one workgroup per plane: plain stores (gfield needs no zero fill).  Two variants, chosen per plane on
// the device (adv_dy_class_kernel): field + sums in a ring of strip_ring_rows(H) rows, or - displacements of many rows -
// the sums alone in a ring of 64 rows with the field taps from L2.
int pd_adv_bwd_circle(const AdvArgs& a) {
  const AdvGeom g = make_geom(a);
  const int NT = 2 * g.p, planes = a.B * a.K, m = adv_mode_index(a.mode);
  const bool cubic = a.mode == PARADIS_INTERP_BICUBIC;
  const int ring = strip_ring_rows(a.H), strips = (a.W + STRIP_W - 1) / STRIP_W;
  static PerDeviceOnce once;
  if (int e = reserve_lds(once, CIRCLE_BWD, "sl_advect_bwd", STRIP_LDS_MAX)) return e;
  {
    // rows the field-in-LDS ring covers below an arrival row, in radians of v dt
    const int hyl = ring == 32 ? (cubic ? 6 : 7) : (cubic ? 22 : 23);
    const float thresh = ring == 64 ? INFINITY : (float)hyl / (g.cy * fabsf(a.dt));
    hipLaunchKernelGGL(adv_dy_class_kernel, dim3(planes), dim3(256), 0, a.st, a.v, a.wide, a.K, a.H, a.W, a.uv_bs, thresh);
  }
  const int wpr = a.W <= 128 ? 2 : 4;
  auto launch = [&](int variant, size_t lds) {
    hipLaunchKernelGGL(CIRCLE_BWD[m][wpr == 4][variant], dim3((unsigned)planes), dim3(256 * wpr), lds, a.st, a.gout, a.field,
                       a.u, a.v, a.gfield, a.gu, a.gv, a.sin_lat, a.cos_lat, a.lat_cells, a.lon, a.fmeans, a.gmeans, a.K, g,
                       a.go_bs, a.f_bs, a.uv_bs, a.gf_bs, a.guv_bs, strips, a.queue, a.counts, a.wide);
  };
  launch(ring == 32 ? CIRCLE_R32 : CIRCLE_R64, circle_lds(a.H, a.W, NT));
  if (ring == 32) launch(CIRCLE_R64_SUMS, circle_lds_wide(a.W, NT));
  // one list per plane (lists_per_plane = 1); never deterministic: adv_schedule
  hipLaunchKernelGGL(STRIP_BWD_FIXUP[m][0], dim3((unsigned)(planes * strips)), dim3(256), 0, a.st, a.gout, a.field, a.u, a.v,
                     a.gfield, a.gu, a.gv, a.sin_lat, a.cos_lat, a.lon, a.fmeans, a.gmeans, a.K, g, a.go_bs, a.f_bs, a.uv_bs,
                     a.gf_bs, a.guv_bs, strips, nullptr, nullptr, a.queue, a.counts, 1);
  return 0;
}

int pd_adv_bwd_strips(const AdvArgs& a) {
  const AdvGeom g = make_geom(a);
  const int NT = 2 * g.p, planes = a.B * a.K, m = adv_mode_index(a.mode);
  const bool cubic = a.mode == PARADIS_INTERP_BICUBIC, det = a.gacc != nullptr;
  const int ring = strip_ring_rows(a.H), hx = halo_of(a.flags, strip_halo_bwd(a.W), true);
  const int strips = (a.W + STRIP_W - 1) / STRIP_W;
  auto slds_of = [&](int r) { return ((size_t)r * (STRIP_W + 2 * hx + NT) * 3 + 8) * sizeof(float); };
  PD_REQUIRE(slds_of(ring) <= (size_t)STRIP_LDS_MAX, "sl_advect_bwd: window does not fit LDS");
  PD_REQUIRE((int64_t)planes * strips < (1ll << 31), "sl_advect_bwd: too many strips");
  PD_REQUIRE(STRIP_W + 2 * hx + NT <= STRIP_MAX_WS, "sl_advect_bwd: halo too wide");
  static PerDeviceOnce once;
  if (int e = reserve_lds(once, STRIP_BWD, "sl_advect_bwd", STRIP_LDS_MAX)) return e;
  const unsigned* wide = nullptr;       // class word per plane on tall grids (64-row ring), see sl_advect_bwd_strip
  if (ring == 64) {
    // planes whose sampled |v dt| stays inside the 32-row ring's latitude halo (more than 15/16 of the points) run in
    // it at two workgroups per CU: 721 x 1440 backward 20.7 -> 13.4 ms at small velocities (tools/advect_bench.py)
    wide = a.wide;
    const int hyl = cubic ? 6 : 7;     // rows the 32-row ring covers below an arrival row
    hipLaunchKernelGGL(adv_dy_class_kernel, dim3(planes), dim3(256), 0, a.st, a.v, a.wide, a.K, a.H, a.W, a.uv_bs,
                       (float)hyl / (g.cy * fabsf(a.dt)));
  }
  const dim3 grid((unsigned)(planes * strips));
  auto launch = [&](int r) {
    hipLaunchKernelGGL(STRIP_BWD[m][r == 64][det], grid, dim3(STRIP_THREADS), slds_of(r), a.st, a.gout, a.field, a.u, a.v,
                       a.gfield, a.gu, a.gv, a.sin_lat, a.cos_lat, a.lat_cells, a.lon, a.fmeans, a.gmeans, a.K, g, a.go_bs,
                       a.f_bs, a.uv_bs, a.gf_bs, a.guv_bs, hx, strips, a.gacc, a.pmax, a.queue, a.counts, wide);
  };
  launch(32);
  if (ring == 64) launch(64);
  hipLaunchKernelGGL(STRIP_BWD_FIXUP[m][det], grid, dim3(256), 0, a.st, a.gout, a.field, a.u, a.v, a.gfield, a.gu, a.gv,
                     a.sin_lat, a.cos_lat, a.lon, a.fmeans, a.gmeans, a.K, g, a.go_bs, a.f_bs, a.uv_bs, a.gf_bs, a.guv_bs,
                     strips, a.gacc, a.pmax, a.queue, a.counts, strips);
  return 0;
}
