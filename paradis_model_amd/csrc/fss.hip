// Neighbourhood verification - the integer sums of the fractions skill score.  Per sample b, event source s (the
// sources, thresholds, directions and validity of events.hip; event_source.h), latitude row h: nV, nF[j], nO[j] as
// events.hip counts them, and per scale k and threshold j the sums over the row's cells of cF^2, cO^2 and cF cO, cF /
// cO being the number of forecast / truth event cells in the window of the cell: rows max(0, h - ny[k]) ..
// min(H - 1, h + ny[k]) (clipped, no over-the-pole wrap), columns w - nx[k][h] .. w + nx[k][h] modulo W.  An invalid
// cell is a non-event in both fields.  Everything after the decision is integer: the result is exact.
//
// Three launches on the stream.
//   1. fss_decide_kernel: the pass over the planes.  The layout of events.hip: a workgroup of 256 threads owns
//      PLANE_PIECE / W whole rows of one (sample, source), wave v the rows v, v + 4, ..; a row is walked 256 cells at a
//      time, lane l at the quad 4 l .. 4 l + 3 (one 16-byte load per plane where VEC, scalar loads otherwise: the same
//      bits).  Per cell it packs the decided bits into 16 bits - bit j: F[j], bit 8 + j: O[j] - and stores them to the
//      mask plane [B][S][H][W] (uint16) of the workspace; nV, nF, nO are counted by wave ballots and go to the partials.
//   2. fss_window_kernel: the stencil over the decided bits.  A workgroup of 256 threads owns FSS rows (R) centre
//      rows of one (sample, source, SCALE): the halo a workgroup reads is its own scale's, 2 ny[k] mask rows of two
//      bytes a cell (from L2: the mask planes of a 721x1440 state are 2 MB a source), and K times as many workgroups
//      fill the device at B = 1.  Thread t owns the columns t, t + 256, ..; per column it keeps the vertical counts of
//      the 2 T bits as byte lanes packed in dwords (a count is at most 2 * 16 + 1 = 33): the rows of the first centre
//      row's window are added up, then the count slides - add the mask row entering, subtract the one leaving.  Per
//      centre row the column counts go to LDS; for the window sums thread t takes the ceil(W / 256) consecutive columns
//      from t ceil(W / 256): it sums the 2 nx + 1 columns (modulo W) of its first window in 16-bit lanes (at most
//      33 * 129 = 4257) and slides that sum to its next columns, squares and multiplies per threshold into 32-bit
//      sums of its at most 6 columns (6 * 4257^2 = 1.1e8); those are summed over the 16 lanes of a DPP row in 32 bits
//      (1.7e9 < 2^32) and from there on in 64 bits through LDS: a row's sum reaches 1440 * 4257^2 = 2.6e10.
//   3. lead_finish_kernel (event_source.h): acc += sum_b partials, n_samples += B, ordinary read-modify-writes; a partial
//      row is the prefix of an acc row of FSS_CNT entries.
// event_source.h also holds the entry point's checks behind its B == 0 return (event_launch_prologue, which checks the
// window kernel's grid too); this unit keeps its two kernels written out.
// No atomics, no host synchronisation, no memset or copy nodes; the inputs are only read, and only the sources' planes.
// Workspace: the mask planes, then the partials uint64 [B][S][H][1 + 2 TMAX + 3 K TMAX], a prefix of an acc row.
#include "common.h"
#include "stream_common.h"
#include "event_source.h"

#include <cmath>

#pragma clang fp contract(off)

namespace {

constexpr int FSS_KMAX = 8;                        // scales per launch
constexpr int FSS_MAX_HY = 16;                     // latitude half-width, rows
constexpr int FSS_MAX_HX = 64;                     // longitude half-width, cells
constexpr int FSS_NC = 6;                          // columns per thread of the window kernel
constexpr int FSS_MAX_W = 1440;                    // longitudes
constexpr int FSS_HEAD = 1 + 2 * EVSRC_TMAX;       // nV, nF[TMAX], nO[TMAX]
constexpr int FSS_CNT = FSS_HEAD + 3 * FSS_KMAX * EVSRC_TMAX;      // int64 per (source, row) of acc
static_assert(FSS_MAX_W <= 256 * FSS_NC, "a thread of the window kernel owns at most FSS_NC columns");
static_assert(2 * FSS_MAX_HY + 1 <= 255, "a vertical count fits a byte lane");
static_assert((2 * FSS_MAX_HY + 1) * (2 * FSS_MAX_HX + 1) <= 65535, "a window count fits a 16-bit lane");
static_assert(16ull * FSS_NC * ((2 * FSS_MAX_HY + 1) * (2 * FSS_MAX_HX + 1)) * ((2 * FSS_MAX_HY + 1) * (2 * FSS_MAX_HX + 1)) <
                  (1ull << 32), "the sum over a DPP row of the threads' sums fits 32 bits");

// centre rows per workgroup of the window kernel: few, so that one 721x1440 state gives every CU several workgroups
// of every scale (the halo is two-byte bits out of L2, cheap beside the window sums)
inline int fss_rows() { return 8; }
inline size_t mask_bytes(int B, int S, int H, int W) {
  return ((size_t)B * S * H * W * sizeof(uint16_t) + 15) / 16 * 16;
}
inline int row_counters(int K) { return FSS_HEAD + 3 * K * EVSRC_TMAX; }

// ---------------------------------------------------------------------------------------------- 1. the decision
struct DecideArgs {
  SourceInputs in;
  uint16_t* mask;           // [B][S][H][W]
  unsigned long long* partial;   // [B][S][H][n_row]
  int n_row;
};

// rows h0 + wave, h0 + wave + 4, .. < h1 of one (sample, source)
template <int KIND, bool VEC>
__device__ __forceinline__ void decide_rows_of_wave(const SourcePlanes& p, const float* __restrict__ tab, int nthr, int W,
                                                    int h0, int h1, uint16_t* __restrict__ mask,
                                                    unsigned long long* __restrict__ out, int n_row) {
  const int lane = (int)(threadIdx.x & 63);
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  float th[EVSRC_TMAX];
  const float sign = source_thresholds(tab, nthr, th);
  const int wpr = (W + 255) / 256;                                              // walks per row
  for (int h = h0 + wave; h < h1; h += 4) {
    const int64_t row = (int64_t)h * W;
    unsigned nV = 0, nF[EVSRC_TMAX], nO[EVSRC_TMAX];
#pragma unroll
    for (int j = 0; j < EVSRC_TMAX; ++j) nF[j] = nO[j] = 0;
#pragma clang loop vectorize(disable) interleave(disable)
    for (int wk = 0; wk < wpr; ++wk) {
      // (source_load_walk's loads spelt out into local arrays: with the quads in a SourceQuads this loop's schedule came
      // out 6-7 % slower for speed sources)
      const int w0 = 256 * wk + 4 * lane;
      const int at = VEC ? min(w0, W - 4) : w0;           // (VEC: W % 4 == 0, a lane past the end reloads the last quad)
      float fa[4], ta[4], fb[4], tb[4], cv[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) fb[k] = tb[k] = cv[k] = 0.f;
      load_quad<VEC>(p.f0 + row, at, W, fa);
      load_quad<VEC>(p.t0 + row, at, W, ta);
      if (KIND == EVSRC_SPEED) {
        load_quad<VEC>(p.f1 + row, at, W, fb);
        load_quad<VEC>(p.t1 + row, at, W, tb);
      }
      if (KIND == EVSRC_ANOMALY) load_quad<VEC>(p.cl + row, at, W, cv);
      unsigned mk[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float sf, st;
        const bool ok = event_cell<KIND>((VEC ? w0 : w0 + k) < W, fa[k], ta[k], fb[k], tb[k], cv[k], sign, sf, st);
        nV += count_lanes(ok);
        unsigned bits = 0;
#pragma unroll
        for (int j = 0; j < EVSRC_TMAX; ++j) {
          const bool F = ok && sf >= th[j], O = ok && st >= th[j];
          nF[j] += count_lanes(F);
          nO[j] += count_lanes(O);
          bits |= (F ? 1u << j : 0u) | (O ? 256u << j : 0u);
        }
        mk[k] = bits;
      }
      if (VEC) {
        if (w0 < W) *reinterpret_cast<uint2*>(mask + row + w0) = make_uint2(mk[0] | (mk[1] << 16), mk[2] | (mk[3] << 16));
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (w0 + k < W) mask[row + w0 + k] = (uint16_t)mk[k];
      }
    }
    unsigned mine = lane == 0 ? nV : 0u;
#pragma unroll
    for (int j = 0; j < EVSRC_TMAX; ++j) {
      mine = lane == 1 + j ? nF[j] : mine;
      mine = lane == 1 + EVSRC_TMAX + j ? nO[j] : mine;
    }
    if (lane < FSS_HEAD) out[(int64_t)h * n_row + lane] = mine;
  }
}

template <bool VEC>
__global__ void __launch_bounds__(256) fss_decide_kernel(DecideArgs a) {
  const SourceInputs& in = a.in;
  const int64_t pair = blockIdx.x / in.ngroups;                      // b S + s
  const int g = (int)(blockIdx.x - pair * in.ngroups);
  const int b = (int)(pair / in.S), s = (int)(pair - (int64_t)b * in.S);
  const int kind = in.src[s][0], nthr = in.src[s][3];
  const int h0 = g * in.rows, h1 = min(in.H, h0 + in.rows);
  unsigned long long* out = a.partial + pair * in.H * a.n_row;
  uint16_t* mask = a.mask + pair * in.P;
  SourcePlanes p = source_planes(in, b, s);
  const float* tab = in.thr[s];
  if (kind == EVSRC_ANOMALY) {
    const int slot = in.clim_index[b];
    if (slot < 0 || slot >= in.K) {                  // (workgroup-uniform) no valid cell; nothing of such a slot is read
      for (int64_t i = (int64_t)h0 * in.W + threadIdx.x; i < (int64_t)h1 * in.W; i += 256) mask[i] = 0;
      const int lane = (int)(threadIdx.x & 63);
      for (int h = h0 + (int)(threadIdx.x >> 6); h < h1; h += 4)
        if (lane < FSS_HEAD) out[(int64_t)h * a.n_row + lane] = 0ull;
      return;
    }
    p.cl = in.clim + ((int64_t)slot * in.C + in.src[s][1]) * in.P;
    decide_rows_of_wave<EVSRC_ANOMALY, VEC>(p, tab, nthr, in.W, h0, h1, mask, out, a.n_row);
  } else if (kind == EVSRC_SPEED) {
    decide_rows_of_wave<EVSRC_SPEED, VEC>(p, tab, nthr, in.W, h0, h1, mask, out, a.n_row);
  } else {
    decide_rows_of_wave<EVSRC_PLAIN, VEC>(p, tab, nthr, in.W, h0, h1, mask, out, a.n_row);
  }
}

// ---------------------------------------------------------------------------------------------- 2. the windows
struct WindowArgs {
  const uint16_t* mask;          // [B][S][H][W]
  const int* half_x;             // DEVICE [K][H]
  unsigned long long* partial;   // [B][S][H][n_row]
  int H, W, K, rows, ngroups, n_row, nx_cap;
  int hy[FSS_KMAX];
};

// bits 0 .. 3 of x to the low bits of the four bytes of a dword
__device__ __forceinline__ unsigned spread4(unsigned x) { return ((x & 0xfu) * 0x00204081u) & 0x01010101u; }

// sum over the 16 lanes of a DPP row, in its lane 15 (row_shr 1 / 2 / 4 / 8; lanes a shift has no source for add 0)
__device__ __forceinline__ unsigned row16_sum_lane15(unsigned v) {
#define PD_DPP_UADD(ctrl) v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, ctrl, 0xf, 0xf, true)
  PD_DPP_UADD(0x111); PD_DPP_UADD(0x112); PD_DPP_UADD(0x114); PD_DPP_UADD(0x118);
#undef PD_DPP_UADD
  return v;
}

// NC: columns per thread (W <= 256 NC); NW: dwords of byte lanes per field (4 NW thresholds are carried)
template <int NC, int NW>
__global__ void __launch_bounds__(256) fss_window_kernel(WindowArgs a) {
  constexpr int NV = 2 * NW;                     // dwords per column: F words, then O words
  constexpr int NT = 4 * NW;
  __shared__ __attribute__((aligned(16))) unsigned vs[256 * NC * NV];       // the column counts of the centre row
  __shared__ unsigned red[3 * NT][16];                                       // the sums of the 16 DPP rows
  const int t = (int)threadIdx.x, lane = t & 63;
  int bid = (int)blockIdx.x;
  const int g = bid % a.ngroups;
  bid /= a.ngroups;
  const int k = bid % a.K;
  const int64_t pair = bid / a.K;
  const int H = a.H, W = a.W;
  int ny = 0;
#pragma unroll
  for (int i = 0; i < FSS_KMAX; ++i) ny = i == k ? a.hy[i] : ny;
  const int h0 = g * a.rows, h1 = min(H, h0 + a.rows);
  const int ncw = (W + 255) / 256;               // columns of a thread's segment in the window sums (<= NC)
  const uint16_t* __restrict__ m = a.mask + pair * (int64_t)H * W;
  unsigned long long* out = a.partial + pair * (int64_t)H * a.n_row + FSS_HEAD + 3 * EVSRC_TMAX * k;

  unsigned V[NC][NV];
#pragma unroll
  for (int i = 0; i < NC; ++i)
#pragma unroll
    for (int w = 0; w < NV; ++w) V[i][w] = 0u;
  // V +- the bits of mask row `row` (workgroup-uniform, inside the grid)
  auto slide = [&](int row, bool add) {
    const uint16_t* __restrict__ mr = m + (int64_t)row * W;
#pragma unroll
    for (int i = 0; i < NC; ++i) {
      const int c = t + 256 * i;
      const unsigned mk = c < W ? (unsigned)mr[c] : 0u;
#pragma unroll
      for (int w = 0; w < NW; ++w) {
        const unsigned f = spread4(mk >> (4 * w)), o = spread4(mk >> (8 + 4 * w));
        V[i][w] = add ? V[i][w] + f : V[i][w] - f;
        V[i][NW + w] = add ? V[i][NW + w] + o : V[i][NW + w] - o;
      }
    }
  };
  for (int row = max(0, h0 - ny); row <= min(H - 1, h0 + ny); ++row) slide(row, true);

  for (int h = h0; h < h1; ++h) {
    if (h > h0) {
      if (h + ny < H) slide(h + ny, true);
      if (h - ny - 1 >= 0) slide(h - ny - 1, false);
    }
    // (the previous row's window reads ended before its second barrier)
#pragma unroll
    for (int i = 0; i < NC; ++i) {
      const int c = t + 256 * i;
      if (c < W) {
#pragma unroll
        for (int w = 0; w < NV; ++w) vs[c * NV + w] = V[i][w];
      }
    }
    __syncthreads();
    const int nx = min(max(a.half_x[(int64_t)k * H + h], 0), a.nx_cap);     // the clamp of the entry point's contract
    unsigned ff[NT], oo[NT], fo[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) ff[j] = oo[j] = fo[j] = 0u;
    // the thread's segment of ncw consecutive columns: the window of the first is summed column by column, the window
    // of each next one slides - subtract the column leaving, add the one entering (a lane never goes below 0: what
    // leaves was added before); 2 nx + 1 == W: the column leaving is the one entering
    const int c0 = t * ncw, c1 = min(W, c0 + ncw);
    if (c0 < W) {
      unsigned s16[2 * NV];                       // per dword of byte lanes: its even bytes, its odd bytes, 16 bits each
#pragma unroll
      for (int w = 0; w < 2 * NV; ++w) s16[w] = 0u;
      int lo = c0 - nx;
      lo = lo < 0 ? lo + W : lo;                  // (2 nx + 1 <= W: one wrap) the column that leaves next
      int hi = lo;                                // the column that enters next
      for (int d = 0; d <= 2 * nx; ++d) {
#pragma unroll
        for (int w = 0; w < NV; ++w) {
          const unsigned v = vs[hi * NV + w];
          s16[2 * w] += v & 0x00ff00ffu;
          s16[2 * w + 1] += (v >> 8) & 0x00ff00ffu;
        }
        hi = hi + 1 == W ? 0 : hi + 1;
      }
      for (int c = c0;;) {
#pragma unroll
        for (int j = 0; j < NT; ++j) {            // threshold j: byte j % 4 of dword j / 4 (F) and NW + j / 4 (O)
          const int by = j & 3, sh = 16 * (by >> 1);
          const unsigned cF = (s16[2 * (j >> 2) + (by & 1)] >> sh) & 0xffffu;
          const unsigned cO = (s16[2 * (NW + (j >> 2)) + (by & 1)] >> sh) & 0xffffu;
          ff[j] += cF * cF;
          oo[j] += cO * cO;
          fo[j] += cF * cO;
        }
        if (++c >= c1) break;
#pragma unroll
        for (int w = 0; w < NV; ++w) {
          const unsigned vo = vs[lo * NV + w], vi = vs[hi * NV + w];
          s16[2 * w] = s16[2 * w] - (vo & 0x00ff00ffu) + (vi & 0x00ff00ffu);
          s16[2 * w + 1] = s16[2 * w + 1] - ((vo >> 8) & 0x00ff00ffu) + ((vi >> 8) & 0x00ff00ffu);
        }
        lo = lo + 1 == W ? 0 : lo + 1;
        hi = hi + 1 == W ? 0 : hi + 1;
      }
    }
    // (all 256 threads: the DPP sums need the whole wave)
    const int slot = (t >> 6) * 4 + (lane >> 4);
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const unsigned r0 = row16_sum_lane15(ff[j]), r1 = row16_sum_lane15(oo[j]), r2 = row16_sum_lane15(fo[j]);
      if ((lane & 15) == 15) {
        red[3 * j][slot] = r0;
        red[3 * j + 1][slot] = r1;
        red[3 * j + 2][slot] = r2;
      }
    }
    __syncthreads();
    if (t < 3 * EVSRC_TMAX) {                       // entry 3 j + q of this scale: FF, OO, FO of threshold j
      unsigned long long s = 0ull;
      if (t < 3 * NT) {
#pragma unroll
        for (int i = 0; i < 16; ++i) s += (unsigned long long)red[t][i];
      }
      out[(int64_t)h * a.n_row + t] = s;
    }
  }
}

}  // namespace

extern "C" int paradis_fss_max_scales(void) { return FSS_KMAX; }

extern "C" int paradis_fss_max_half_y(void) { return FSS_MAX_HY; }

extern "C" int paradis_fss_max_half_x(void) { return FSS_MAX_HX; }

extern "C" int paradis_fss_max_w(void) { return FSS_MAX_W; }

extern "C" int paradis_fss_rows(int W, int ny_max) {
  return (W < 1 || W > FSS_MAX_W || ny_max < 0 || ny_max > FSS_MAX_HY) ? 0 : fss_rows();
}

extern "C" size_t paradis_fss_ws_bytes(int B, int S, int H, int W, int K) {
  if (B < 1 || S < 1 || H < 1 || W < 1 || K < 1 || K > FSS_KMAX) return 0;
  return mask_bytes(B, S, H, W) + (size_t)B * S * H * row_counters(K) * sizeof(unsigned long long);
}

extern "C" int paradis_fss_update(const float* fc, int64_t fc_bs, const float* truth, int64_t truth_bs, const float* clim,
                                  const int* clim_index, int K_clim, const int* src_table, const float* thr_table,
                                  const int* half_y, const int* half_x, int64_t* acc_lead, int64_t* n_samples_lead,
                                  void* ws, int B, int C, int S, int H, int W, int K, void* stream) {
  int rc = event_shape_check("fss_update", "K_clim", clim, clim_index, K_clim, B, C, S, H, W);
  if (rc != 0) return rc;
  PD_REQUIRE(W <= FSS_MAX_W, "fss_update: W=%d, at most %d longitudes", W, FSS_MAX_W);
  PD_REQUIRE(K >= 1 && K <= FSS_KMAX, "fss_update: K=%d scales, 1 to %d are allowed", K, FSS_KMAX);
  if (B == 0) return 0;
  PD_REQUIRE(src_table && thr_table && half_y, "fss_update: null table (src_table, thr_table, half_y)");
  WindowArgs wa;
  int ny_max = 0;
  for (int k = 0; k < FSS_KMAX; ++k) {
    wa.hy[k] = k < K ? half_y[k] : 0;
    PD_REQUIRE(wa.hy[k] >= 0 && wa.hy[k] <= FSS_MAX_HY, "fss_update: half_y[%d] = %d is outside [0, %d]", k, wa.hy[k],
               FSS_MAX_HY);
    ny_max = std::max(ny_max, wa.hy[k]);
  }
  const int R = fss_rows(), n_row = row_counters(K);
  const int64_t wgroups = ceil_div64(H, R), wgrid_n = (int64_t)B * S * K * wgroups;
  DecideArgs a;
  EventLaunch L;
  const EventUnit u{"fss_update", ws != nullptr && aligned16(ws), " or not 16-byte aligned", fc && truth && half_x,
                    " (fc, truth, half_x)", plane_rows(W), n_row, EVSRC_TMAX, wgrid_n};
  rc = event_launch_prologue(u, a.in, L, acc_lead, n_samples_lead, fc, fc_bs, truth, truth_bs, clim, clim_index, K_clim,
                             src_table, thr_table, B, C, S, H, W);
  if (rc != 0) return rc;
  int nthr_max = 0;
  for (int s = 0; s < S; ++s) nthr_max = std::max(nthr_max, a.in.src[s][3]);
  a.mask = static_cast<uint16_t*>(ws);
  a.partial = reinterpret_cast<unsigned long long*>(static_cast<char*>(ws) + mask_bytes(B, S, H, W));
  a.n_row = n_row;
  wa.mask = a.mask; wa.half_x = half_x; wa.partial = a.partial;
  wa.H = H; wa.W = W; wa.K = K; wa.rows = R; wa.ngroups = (int)wgroups; wa.n_row = n_row;
  wa.nx_cap = std::min(FSS_MAX_HX, (W - 1) / 2);
  hipStream_t st = (hipStream_t)stream;
  const dim3 dgrid(L.grid), wgrid((unsigned)wgrid_n);
  if (L.vec) hipLaunchKernelGGL(fss_decide_kernel<true>, dgrid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL(fss_decide_kernel<false>, dgrid, dim3(256), 0, st, a);
  const bool narrow = W <= 256, few = nthr_max <= 4;
  if (narrow && few) hipLaunchKernelGGL((fss_window_kernel<1, 1>), wgrid, dim3(256), 0, st, wa);
  else if (narrow) hipLaunchKernelGGL((fss_window_kernel<1, 2>), wgrid, dim3(256), 0, st, wa);
  else if (few) hipLaunchKernelGGL((fss_window_kernel<FSS_NC, 1>), wgrid, dim3(256), 0, st, wa);
  else hipLaunchKernelGGL((fss_window_kernel<FSS_NC, 2>), wgrid, dim3(256), 0, st, wa);
  launch_lead_finish(L, a.partial, acc_lead, n_samples_lead, B, n_row, FSS_CNT, st);
  PD_CHECK_LAUNCH("fss_update");
  return 0;
}
