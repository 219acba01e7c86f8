// SEEPS (stable equitable error in probability space, Rodwell et al. 2010) - one pass over a forecast state and its truth
// [B, C, H, W] (physical units, fp32, each with its own batch stride) and the two planes of a SEEPS climatology (p1: the
// climatological probability of a dry cell, thr: the light / heavy edge; climatology.build_seeps, quantile.hip) that
// forms, per sample b, chosen channel cs and latitude row h, the 3x3 table of (forecast category, truth category), the
// number of masked cells and the row sums of the score split by the truth's category, and finishing kernels that fold
// the samples, in b order, into the rows of one lead.  The project's own restatement of the published formulas, in the
// spirit of WeatherBench-2; not pinned against any package (tests/seeps_oracle.py restates it in numpy).
//
// Per cell, f / o the forecast / truth value, p1 / thr the climatology's of slot clim_index[b]:
//   cat(x) = 0 (dry) if x < dry, else 2 (heavy) if x >= thr, else 1 (light)       exact fp32 comparisons of loaded values
//   valid   iff f, o, p1, thr are finite, p_lo <= p1 <= p_hi (fp32) and the slot is in [0, K)
//   masked  iff all four are finite and the slot is in range, but p1 is outside the bounds
//   anything else is counted nowhere
// Per valid cell, in double, uncontracted, p = (double)p1:
//   a = 1.0 / (1.0 - p),  b = 1.0 / p,  c = 3.0 / (2.0 + p)
//   M[cf][co] = {{0, a, 4.0 * a}, {b, 0, 3.0 * a}, {b + c, c, 0}}                 (row: forecast, column: truth)
//   s = 0.5 * M[cat(f)][cat(o)]
// Per row: SP_CNT = 10 counters {n[cf][co] (cf-major), n_masked} and SP_REAL = 3 doubles: the sum of s over the valid cells
// whose truth is dry, light, heavy.  The integers are exact; the doubles are summed in a fixed order.
//
// Work layout (events.hip's): a workgroup of 256 threads owns plane_rows(W) whole rows of one (sample, channel) pair.
// Wave v owns the rows v, v + 4, .. of the group: a row's sums never cross waves.  A row is walked 256 cells at a time,
// lane l at the quad of cells 4 l .. 4 l + 3: four planes per walk (f, o, p1, thr), one 16-byte load each where VEC,
// four scalar loads otherwise - the same bits, and the same lane has the same cells; the quads of the wave's next walk
// are loaded before the current walk is counted.  The counters are __popcll(__ballot(..)) into scalar registers; a lane
// adds its cells' s into three doubles in walk order, selecting ok ? s : 0.0 behind the arithmetic (an invalid cell's
// divisions may give Inf or NaN and add exactly nothing); the wave folds the lanes by the xor tree of stream_common.h.
// No LDS, no atomics, no zero fill: bit-identical run to run.
// Algorithmic HBM bytes per cell of a channel: 16.
#include "common.h"
#include "stream_common.h"
#include "event_source.h"

#include <cmath>

#pragma clang fp contract(off)

namespace {

constexpr int SP_CMAX = 8;          // channels per launch: their state indices travel as kernel arguments
constexpr int SP_CNT = 10;          // {n[3][3], n_masked}
constexpr int SP_REAL = 3;          // the sums of s by truth category

struct SeepsArgs {
  const float* fc;
  const float* truth;
  const float* p1;                // [K][..][P]: slot stride clim_ks, channel stride clim_cs
  const float* thr;
  const int* clim_index;          // [B]
  double* real;                   // [B][Cs][H][SP_REAL]
  unsigned* cnt;                  // [B][Cs][H][SP_CNT]
  int64_t fc_bs, truth_bs, clim_ks, clim_cs, P;
  float dry, p_lo, p_hi;
  int K, Cs, H, W, rows, ngroups;
  int chan[SP_CMAX];              // the state channel of output channel cs, checked on the host
};

// the planes of one (sample, channel)
struct SeepsPlanes {
  const float* f;
  const float* o;
  const float* p;
  const float* t;
};

// the quads of one lane for one walk (256 cells of one row); w0: the first cell of the lane's quad
struct SeepsQuads {
  float f[4], o[4], p[4], t[4];
  int w0;
};

// walk `wk` of row h (source_load_walk's rule: VEC, a lane past the row's end loads the row's last quad instead - no
// branch around the loads - and its cells are not counted)
template <bool VEC>
__device__ __forceinline__ void seeps_load_walk(const SeepsPlanes& pl, int W, int h, int wk, int lane, SeepsQuads& q) {
  const int64_t row = (int64_t)h * W;
  q.w0 = 256 * wk + 4 * lane;
  const int at = VEC ? min(q.w0, W - 4) : q.w0;
  load_quad<VEC>(pl.f + row, at, W, q.f);
  load_quad<VEC>(pl.o + row, at, W, q.o);
  load_quad<VEC>(pl.p + row, at, W, q.p);
  load_quad<VEC>(pl.t + row, at, W, q.t);
}

__device__ __forceinline__ int seeps_cat(float x, float dry, float thr) { return x < dry ? 0 : (x >= thr ? 2 : 1); }

// rows h0 + wave, h0 + wave + 4, .. < h1 of one (sample, channel).  The wave's walks (row after row, ceil(W / 256) per
// row) form one sequence; the quads of walk i + 1 are loaded before walk i is counted
template <bool VEC>
__device__ __forceinline__ void seeps_rows_walk(const SeepsPlanes& pl, float dry, float p_lo, float p_hi, int W, int h0,
                                                int h1, double* __restrict__ real, unsigned* __restrict__ cnt) {
  const int lane = (int)(threadIdx.x & 63);
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int first = h0 + wave;
  if (first >= h1) return;
  const int wpr = (W + 255) / 256;                                  // walks per row
  const int nwalks = ((h1 - first + 3) / 4) * wpr;
  unsigned n[3][3], nM = 0;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) n[i][j] = 0;
  double sum[SP_REAL] = {0.0, 0.0, 0.0};
  SeepsQuads q;
  seeps_load_walk<VEC>(pl, W, first, 0, lane, q);
  int h = first, wk = 0;                                            // the walk held in q
  // (the loop vectorizer would interleave two iterations and break the 16-byte accesses into 4-byte ones)
#pragma clang loop vectorize(disable) interleave(disable)
  for (int it = 0; it < nwalks; ++it) {
    const bool last_of_row = wk == wpr - 1, more = it + 1 < nwalks;
    // (after the last walk the same walk is loaded once more, unused: no branch around the loads)
    const int h_next = more && last_of_row ? h + 4 : h, wk_next = !more ? wk : last_of_row ? 0 : wk + 1;
    SeepsQuads nx;
    seeps_load_walk<VEC>(pl, W, h_next, wk_next, lane, nx);
    __builtin_amdgcn_sched_barrier(0);            // (the scheduler would sink the loads to the end of the counting)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float f = q.f[k], o = q.o[k], p1 = q.p[k], th = q.t[k];
      const bool fin = ((VEC ? q.w0 : q.w0 + k) < W) && __builtin_isfinite(f) && __builtin_isfinite(o) &&
                       __builtin_isfinite(p1) && __builtin_isfinite(th);
      const bool ok = fin && p1 >= p_lo && p1 <= p_hi;
      nM += count_lanes(fin && !ok);
      const int cf = seeps_cat(f, dry, th), co = seeps_cat(o, dry, th);
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) n[i][j] += count_lanes(ok && cf == i && co == j);
      const double p = (double)p1;
      const double a = 1.0 / (1.0 - p), b = 1.0 / p, c = 3.0 / (2.0 + p);
      const double m0 = co == 0 ? 0.0 : co == 1 ? a : 4.0 * a;        // the forecast is dry
      const double m1 = co == 0 ? b : co == 1 ? 0.0 : 3.0 * a;        //              light
      const double m2 = co == 0 ? b + c : co == 1 ? c : 0.0;          //              heavy
      const double s = 0.5 * (cf == 0 ? m0 : cf == 1 ? m1 : m2);
#pragma unroll
      for (int j = 0; j < SP_REAL; ++j) sum[j] += (ok && co == j) ? s : 0.0;   // (from +0, terms >= 0: a +0 changes no bit)
    }
    if (last_of_row) {                                              // (wave-uniform)
#pragma unroll
      for (int j = 0; j < SP_REAL; ++j) sum[j] = wave_sum_f64(sum[j]);
      if (lane < SP_REAL) real[(int64_t)h * SP_REAL + lane] = lane == 0 ? sum[0] : lane == 1 ? sum[1] : sum[2];
      unsigned mine = lane == 9 ? nM : 0u;
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) mine = lane == 3 * i + j ? n[i][j] : mine;
      if (lane < SP_CNT) cnt[(int64_t)h * SP_CNT + lane] = mine;
      nM = 0;
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) n[i][j] = 0;
#pragma unroll
      for (int j = 0; j < SP_REAL; ++j) sum[j] = 0.0;
    }
    q = nx;
    h = h_next;
    wk = wk_next;
  }
}

template <bool VEC>
__global__ void __launch_bounds__(256) seeps_kernel(SeepsArgs a) {
  const int64_t pair = blockIdx.x / a.ngroups;                        // b Cs + cs
  const int g = (int)(blockIdx.x - pair * a.ngroups);
  const int b = (int)(pair / a.Cs), cs = (int)(pair - (int64_t)b * a.Cs);
  const int h0 = g * a.rows, h1 = min(a.H, h0 + a.rows);
  double* real = a.real + pair * a.H * SP_REAL;
  unsigned* cnt = a.cnt + pair * a.H * SP_CNT;
  const int slot = a.clim_index[b];
  if (slot < 0 || slot >= a.K) {                  // (workgroup-uniform) nothing of such a slot is read: zero rows
    const int lane = (int)(threadIdx.x & 63);
    for (int h = h0 + (int)(threadIdx.x >> 6); h < h1; h += 4) {
      if (lane < SP_REAL) real[(int64_t)h * SP_REAL + lane] = 0.0;
      if (lane < SP_CNT) cnt[(int64_t)h * SP_CNT + lane] = 0u;
    }
    return;
  }
  int c = a.chan[0];
#pragma unroll
  for (int j = 1; j < SP_CMAX; ++j) c = cs == j ? a.chan[j] : c;
  SeepsPlanes pl;
  pl.f = a.fc + (int64_t)b * a.fc_bs + (int64_t)c * a.P;
  pl.o = a.truth + (int64_t)b * a.truth_bs + (int64_t)c * a.P;
  pl.p = a.p1 + (int64_t)slot * a.clim_ks + (int64_t)cs * a.clim_cs;
  pl.t = a.thr + (int64_t)slot * a.clim_ks + (int64_t)cs * a.clim_cs;
  seeps_rows_walk<VEC>(pl, a.dry, a.p_lo, a.p_hi, a.W, h0, h1, real, cnt);
}

// one thread per double of the lead's rows: (acc + s_0) + s_1 .., b ascending (ens_finish_kernel's rule for its doubles);
// an ordinary read-modify-write (launches of one stream are ordered)
__global__ void __launch_bounds__(256) seeps_finish_real_kernel(const double* __restrict__ real, double* __restrict__ acc_real,
                                                                int B, int64_t nreal) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= nreal) return;
  double s = acc_real[i];
  for (int b = 0; b < B; ++b) s += real[(int64_t)b * nreal + i];
  acc_real[i] = s;
}

}  // namespace

extern "C" int paradis_seeps_max_channels(void) { return SP_CMAX; }

extern "C" int paradis_seeps_rows(int W) { return W < 1 ? 0 : plane_rows(W); }

extern "C" size_t paradis_seeps_ws_bytes(int B, int Cs, int H, int W) {
  if (B < 1 || Cs < 1 || H < 1 || W < 1) return 0;
  return (size_t)B * (size_t)Cs * (size_t)H * (SP_REAL * sizeof(double) + SP_CNT * sizeof(unsigned));
}

extern "C" int paradis_seeps_update(const float* fc, int64_t fc_bs, const float* truth, int64_t truth_bs, const float* p1,
                                    const float* thr, int64_t clim_ks, int64_t clim_cs, const int* clim_index, int K,
                                    const int* chan_host, int Cs, float dry, float p_lo, float p_hi,
                                    double* acc_real_lead, int64_t* acc_int_lead, int64_t* n_samples_lead, void* ws,
                                    int B, int C, int H, int W, void* stream) {
  PD_REQUIRE(B >= 0 && C >= 1 && Cs >= 1 && Cs <= SP_CMAX && H >= 1 && W >= 1 && K >= 0,
             "seeps_update: bad shape B=%d C=%d Cs=%d (at most %d) H=%d W=%d K=%d", B, C, Cs, SP_CMAX, H, W, K);
  PD_REQUIRE(std::isfinite(dry), "seeps_update: the dry threshold is %g, not finite", (double)dry);
  PD_REQUIRE(p_lo > 0.f && p_hi < 1.f && p_lo <= p_hi, "seeps_update: p1 bounds (%g, %g) must satisfy 0 < p_lo <= p_hi < 1",
             (double)p_lo, (double)p_hi);
  if (B == 0 || K == 0) return 0;
  PD_REQUIRE(acc_real_lead != nullptr && acc_int_lead != nullptr && n_samples_lead != nullptr,
             "seeps_update: acc_real_lead / acc_int_lead / n_samples_lead missing");
  PD_REQUIRE(ws != nullptr, "seeps_update: ws (workspace) missing");
  PD_REQUIRE(fc && truth && p1 && thr && clim_index && chan_host, "seeps_update: null input pointer");
  const int64_t P = (int64_t)H * W;
  PD_REQUIRE(P < (1ll << 31) - PLANE_PIECE, "seeps_update: a plane of %d x %d cells is too large", H, W);
  PD_REQUIRE(fc_bs >= P * C && truth_bs >= P * C, "seeps_update: batch strides shorter than one state");
  PD_REQUIRE(clim_cs >= P && clim_ks >= P, "seeps_update: climatology strides shorter than one plane");
  SeepsArgs a;
  for (int j = 0; j < SP_CMAX; ++j) a.chan[j] = 0;
  for (int j = 0; j < Cs; ++j) {
    PD_REQUIRE(chan_host[j] >= 0 && chan_host[j] < C, "seeps_update: channel %d reads state channel %d outside [0, %d)", j,
               chan_host[j], C);
    a.chan[j] = chan_host[j];
  }
  a.rows = plane_rows(W);
  a.ngroups = (int)ceil_div64(H, a.rows);
  const int64_t pairs = (int64_t)B * Cs, groups = pairs * a.ngroups;
  PD_REQUIRE(groups < (1ll << 31), "seeps_update: %lld workgroups exceed the grid limit", (long long)groups);
  const int64_t nreal = (int64_t)Cs * H * SP_REAL;
  EventLaunch L;
  L.n = (int64_t)Cs * H * SP_CNT;
  PD_REQUIRE(ceil_div64(L.n, 256) < (1ll << 31), "seeps_update: %lld counters exceed the grid limit", (long long)L.n);
  L.grid = (unsigned)groups;
  L.finish_grid = (unsigned)ceil_div64(L.n, 256);
  L.vec = (W % 4 == 0) && aligned16(fc) && aligned16(truth) && aligned16(p1) && aligned16(thr) && (fc_bs % 4 == 0) &&
          (truth_bs % 4 == 0) && (clim_ks % 4 == 0) && (clim_cs % 4 == 0);
  a.fc = fc; a.truth = truth; a.p1 = p1; a.thr = thr; a.clim_index = clim_index;
  a.real = static_cast<double*>(ws);
  a.cnt = reinterpret_cast<unsigned*>(a.real + (int64_t)B * nreal);
  a.fc_bs = fc_bs; a.truth_bs = truth_bs; a.clim_ks = clim_ks; a.clim_cs = clim_cs; a.P = P;
  a.dry = dry; a.p_lo = p_lo; a.p_hi = p_hi;
  a.K = K; a.Cs = Cs; a.H = H; a.W = W;
  hipStream_t st = (hipStream_t)stream;
  if (L.vec) hipLaunchKernelGGL(seeps_kernel<true>, dim3(L.grid), dim3(256), 0, st, a);
  else hipLaunchKernelGGL(seeps_kernel<false>, dim3(L.grid), dim3(256), 0, st, a);
  hipLaunchKernelGGL(seeps_finish_real_kernel, dim3((unsigned)ceil_div64(nreal, 256)), dim3(256), 0, st, a.real,
                     acc_real_lead, B, nreal);
  launch_lead_finish(L, a.cnt, acc_int_lead, n_samples_lead, B, SP_CNT, SP_CNT, st);
  PD_CHECK_LAUNCH("seeps_update");
  return 0;
}
