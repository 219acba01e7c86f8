// Event verification - one pass over a forecast state and its truth [B, C, H, W] (physical units, fp32, each with its own
// batch stride) that counts, per sample b, event source s and latitude row h, the cells of the 2x2 contingency table of
// "value beyond a threshold" in forecast against truth, and a finishing kernel that adds the counts to the int64 row of
// one lead.  A source yields one fp32 value x per cell (src_table [S][4] = {kind, c0, c1, nthr}):
//   plain    x = v[c0]
//   speed    x = sqrtf(v[c0] * v[c0] + v[c1] * v[c1])        (mul, mul, add, sqrt: the unit is built uncontracted)
//   anomaly  x = v[c0] - clim[clim_index[b]][c0]
// (both tables are HOST memory, checked by the entry point and handed to the kernel as arguments: no copy node, and a
// captured launch keeps them) and thr_table [S][1 + TMAX] = {sign, thr'...} holds its direction and thresholds: the event
// is sign * x >= thr'[j]
// ("le" is sign = -1, thr' = -thr on the host: exact, so there is one code path).  A cell is valid iff every value it
// reads is finite; a sample whose clim_index is outside [0, K) has no valid cell for an anomaly source and nothing of
// that slot is read.  Per valid cell, F: the forecast is beyond thr'[j], O: the truth is.  Per row, EV_CNT counters:
//   [0] nV    [1 + j] nF[j]    [1 + TMAX + j] nO[j]    [1 + 2 TMAX + j] nFO[j]         (0 for j >= nthr)
// Everything after the decision is integer: the result is exact and the same whichever path produced it.
//
// Work layout (stream_common.h): a workgroup of 256 threads owns a group of events_rows(W) ~ PLANE_PIECE / W whole rows of
// one (sample, source) pair, so clim_index[b], the source's table row and every plane base are workgroup-uniform.  Wave
// v owns the rows v, v + 4, .. of the group: a row's counts never cross waves.  A row is walked 256 cells at a time,
// lane l at the quad of cells 4 l .. 4 l + 3 (one 16-byte load per plane where VEC, four scalar loads otherwise: the
// same bits); the quads of the wave's next walk - of this row or of its next row - are loaded before the current walk
// is counted.  Counting is __popcll(__ballot(pred)) into scalar registers - no per-lane counters, no shuffle tree, no
// LDS, no atomics; the dominant class (no event in either field) costs what every class costs.  At the end of a row
// lane i < EV_CNT picks counter i and the wave stores them with one vector store to partial [B][S][H][EV_CNT] (uint32).
// The number of thresholds is rounded up to 1, 2, 4 or 8 compiled variants; thresholds past nthr are NaN, which nothing
// reaches.
// Algorithmic HBM bytes per cell of a source: 8 plain, 16 speed, 12 anomaly.
#include "common.h"
#include "stream_common.h"

#include <cmath>

#pragma clang fp contract(off)

namespace {

constexpr int EV_TMAX = 8;                        // thresholds per source
constexpr int EV_CNT = 1 + 3 * EV_TMAX;           // counters per (source, row)
constexpr int EV_SMAX = 16;                       // sources per launch: their tables travel as kernel arguments
constexpr int EV_PLAIN = 0, EV_SPEED = 1, EV_ANOMALY = 2;

struct EventsArgs {
  const float* fc;
  const float* truth;
  const float* clim;        // [K][C][P] or null
  const int* clim_index;    // [B] or null
  unsigned* partial;        // [B][S][H][EV_CNT]
  int64_t fc_bs, truth_bs, P;
  int C, S, H, W, K, rows, ngroups;
  int src[EV_SMAX][4];                // {kind, c0, c1, nthr}, checked on the host
  float thr[EV_SMAX][1 + EV_TMAX];    // {sign, thr'...}
};

inline int events_rows(int W) { return W >= PLANE_PIECE ? 1 : PLANE_PIECE / (W < 1 ? 1 : W); }

__device__ __forceinline__ unsigned count_lanes(bool p) { return (unsigned)__popcll(__ballot(p)); }

// the planes of one source for one sample; f1 / t1: the second component of a speed source; cl: the climatology plane
struct EventPlanes {
  const float* f0;
  const float* t0;
  const float* f1;
  const float* t1;
  const float* cl;
};

// the quads of one lane for one walk (256 cells of one row); w0: the first cell of the lane's quad
struct EventQuads {
  float fa[4], ta[4], fb[4], tb[4], cv[4];
  int w0;
};

// walk `wk` of row h: 256 cells from cell 256 wk, this lane's quad at w0 = 256 wk + 4 lane.  VEC (W % 4 == 0: a quad
// that starts inside the row is whole): a lane past the row's end loads the row's last quad instead - no branch around
// the loads, so that they can stay in flight while the previous walk is counted - and its cells are not counted
template <int KIND, bool VEC>
__device__ __forceinline__ void events_load_walk(const EventPlanes& p, int W, int h, int wk, int lane, EventQuads& q) {
  const int64_t row = (int64_t)h * W;
  q.w0 = 256 * wk + 4 * lane;
  const int at = VEC ? min(q.w0, W - 4) : q.w0;
#pragma unroll
  for (int k = 0; k < 4; ++k) q.fb[k] = q.tb[k] = q.cv[k] = 0.f;
  load_quad<VEC>(p.f0 + row, at, W, q.fa);
  load_quad<VEC>(p.t0 + row, at, W, q.ta);
  if (KIND == EV_SPEED) {
    load_quad<VEC>(p.f1 + row, at, W, q.fb);
    load_quad<VEC>(p.t1 + row, at, W, q.tb);
  }
  if (KIND == EV_ANOMALY) load_quad<VEC>(p.cl + row, at, W, q.cv);
}

// rows h0 + wave, h0 + wave + 4, .. < h1 of one (sample, source): NT compiled thresholds th[0 .. NT).  The wave's walks
// (row after row, ceil(W / 256) per row) form one sequence; the quads of walk i + 1 are loaded before walk i is counted
template <int KIND, int NT, bool VEC>
__device__ __forceinline__ void events_count_rows(const EventPlanes& p, float sign, const float (&th)[NT], int W, int h0,
                                                  int h1, unsigned* __restrict__ out) {
  const int lane = (int)(threadIdx.x & 63);
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int first = h0 + wave;
  if (first >= h1) return;
  const int wpr = (W + 255) / 256;                                  // walks per row
  const int nwalks = ((h1 - first + 3) / 4) * wpr;
  unsigned nV = 0, nF[NT], nO[NT], nFO[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) nF[j] = nO[j] = nFO[j] = 0;
  EventQuads q;
  events_load_walk<KIND, VEC>(p, W, first, 0, lane, q);
  int h = first, wk = 0;                                            // the walk held in q
  // (the loop vectorizer would interleave two iterations and break the 16-byte accesses into 4-byte ones)
#pragma clang loop vectorize(disable) interleave(disable)
  for (int i = 0; i < nwalks; ++i) {
    const bool last_of_row = wk == wpr - 1, more = i + 1 < nwalks;
    // (after the last walk the same walk is loaded once more, unused: no branch around the loads)
    const int h_next = more && last_of_row ? h + 4 : h, wk_next = !more ? wk : last_of_row ? 0 : wk + 1;
    EventQuads n;
    events_load_walk<KIND, VEC>(p, W, h_next, wk_next, lane, n);
    __builtin_amdgcn_sched_barrier(0);            // (the scheduler would sink the loads to the end of the counting)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      bool ok = (VEC ? q.w0 : q.w0 + k) < W;
      ok = ok && __builtin_isfinite(q.fa[k]) && __builtin_isfinite(q.ta[k]);
      float xf = q.fa[k], xt = q.ta[k];
      if (KIND == EV_SPEED) {
        ok = ok && __builtin_isfinite(q.fb[k]) && __builtin_isfinite(q.tb[k]);
        xf = sqrtf(q.fa[k] * q.fa[k] + q.fb[k] * q.fb[k]);
        xt = sqrtf(q.ta[k] * q.ta[k] + q.tb[k] * q.tb[k]);
      }
      if (KIND == EV_ANOMALY) {
        ok = ok && __builtin_isfinite(q.cv[k]);
        xf = q.fa[k] - q.cv[k];
        xt = q.ta[k] - q.cv[k];
      }
      const float sf = sign * xf, st = sign * xt;          // (sign = +-1: exact)
      nV += count_lanes(ok);
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        const bool F = ok && sf >= th[j], O = ok && st >= th[j];
        nF[j] += count_lanes(F);
        nO[j] += count_lanes(O);
        nFO[j] += count_lanes(F && O);
      }
    }
    if (last_of_row) {                                              // (wave-uniform)
      unsigned mine = lane == 0 ? nV : 0u;
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        mine = lane == 1 + j ? nF[j] : mine;
        mine = lane == 1 + EV_TMAX + j ? nO[j] : mine;
        mine = lane == 1 + 2 * EV_TMAX + j ? nFO[j] : mine;
      }
      if (lane < EV_CNT) out[(int64_t)h * EV_CNT + lane] = mine;
      nV = 0;
#pragma unroll
      for (int j = 0; j < NT; ++j) nF[j] = nO[j] = nFO[j] = 0;
    }
    q = n;
    h = h_next;
    wk = wk_next;
  }
}

template <int KIND, bool VEC>
__device__ __forceinline__ void events_count_kind(const EventPlanes& p, const float* __restrict__ tab, int nthr, int W,
                                                  int h0, int h1, unsigned* __restrict__ out) {
  const float sign = tab[0];
  float th[EV_TMAX];
#pragma unroll
  for (int j = 0; j < EV_TMAX; ++j) th[j] = j < nthr ? tab[1 + j] : NAN;       // (x >= NaN is never an event)
  if (nthr <= 1) {
    const float t1[1] = {th[0]};
    events_count_rows<KIND, 1, VEC>(p, sign, t1, W, h0, h1, out);
  } else if (nthr <= 2) {
    const float t2[2] = {th[0], th[1]};
    events_count_rows<KIND, 2, VEC>(p, sign, t2, W, h0, h1, out);
  } else if (nthr <= 4) {
    const float t4[4] = {th[0], th[1], th[2], th[3]};
    events_count_rows<KIND, 4, VEC>(p, sign, t4, W, h0, h1, out);
  } else {
    events_count_rows<KIND, 8, VEC>(p, sign, th, W, h0, h1, out);
  }
}

template <bool VEC>
__global__ void __launch_bounds__(256) events_kernel(EventsArgs a) {
  const int64_t pair = blockIdx.x / a.ngroups;                       // b S + s
  const int g = (int)(blockIdx.x - pair * a.ngroups);
  const int b = (int)(pair / a.S), s = (int)(pair - (int64_t)b * a.S);
  const int kind = a.src[s][0], c0 = a.src[s][1], c1 = a.src[s][2], nthr = a.src[s][3];
  const int h0 = g * a.rows, h1 = min(a.H, h0 + a.rows);
  unsigned* out = a.partial + pair * a.H * EV_CNT;
  EventPlanes p;
  p.f0 = a.fc + (int64_t)b * a.fc_bs + (int64_t)c0 * a.P;
  p.t0 = a.truth + (int64_t)b * a.truth_bs + (int64_t)c0 * a.P;
  p.f1 = a.fc + (int64_t)b * a.fc_bs + (int64_t)c1 * a.P;
  p.t1 = a.truth + (int64_t)b * a.truth_bs + (int64_t)c1 * a.P;
  p.cl = nullptr;
  const float* tab = a.thr[s];
  if (kind == EV_ANOMALY) {
    const int k = a.clim_index[b];
    if (k < 0 || k >= a.K) {                                         // (workgroup-uniform) nothing of such a slot is read
      const int lane = (int)(threadIdx.x & 63);
      for (int h = h0 + (int)(threadIdx.x >> 6); h < h1; h += 4)
        if (lane < EV_CNT) out[(int64_t)h * EV_CNT + lane] = 0u;
      return;
    }
    p.cl = a.clim + ((int64_t)k * a.C + c0) * a.P;
    events_count_kind<EV_ANOMALY, VEC>(p, tab, nthr, a.W, h0, h1, out);
  } else if (kind == EV_SPEED) {
    events_count_kind<EV_SPEED, VEC>(p, tab, nthr, a.W, h0, h1, out);
  } else {
    events_count_kind<EV_PLAIN, VEC>(p, tab, nthr, a.W, h0, h1, out);
  }
}

// one thread per (source, row, counter): acc += sum_b partial, an ordinary read-modify-write (launches of one stream
// are ordered); thread 0 adds B to the lead's sample count
__global__ void __launch_bounds__(256) events_finish_kernel(const unsigned* __restrict__ partial,
                                                            int64_t* __restrict__ acc,
                                                            int64_t* __restrict__ n_samples, int B, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i == 0) n_samples[0] += B;
  if (i >= n) return;
  int64_t s = 0;
  for (int b = 0; b < B; ++b) s += (int64_t)partial[(int64_t)b * n + i];
  acc[i] += s;
}

}  // namespace

extern "C" int paradis_events_max_thresholds(void) { return EV_TMAX; }

extern "C" int paradis_events_max_sources(void) { return EV_SMAX; }

extern "C" int paradis_events_rows(int W) { return W < 1 ? 0 : events_rows(W); }

extern "C" size_t paradis_events_ws_bytes(int B, int S, int H, int W) {
  if (B < 1 || S < 1 || H < 1 || W < 1) return 0;
  return (size_t)B * (size_t)S * (size_t)H * EV_CNT * sizeof(unsigned);
}

extern "C" int paradis_events_update(const float* fc, int64_t fc_bs, const float* truth, int64_t truth_bs,
                                     const float* clim, const int* clim_index, int K, const int* src_table,
                                     const float* thr_table, int64_t* acc_lead, int64_t* n_samples_lead, void* ws,
                                     int B, int C, int S, int H, int W, void* stream) {
  PD_REQUIRE(B >= 0 && C >= 1 && S >= 1 && S <= EV_SMAX && H >= 1 && W >= 1,
             "events_update: bad shape B=%d C=%d S=%d (at most %d) H=%d W=%d", B, C, S, EV_SMAX, H, W);
  PD_REQUIRE((clim != nullptr) == (clim_index != nullptr),
             "events_update: clim and clim_index go together (a climatology needs the slot of every sample)");
  PD_REQUIRE(clim == nullptr || K >= 1, "events_update: K must be >= 1 with a climatology, got %d", K);
  if (B == 0) return 0;
  PD_REQUIRE(acc_lead != nullptr && n_samples_lead != nullptr, "events_update: acc_lead / n_samples_lead missing");
  PD_REQUIRE(ws != nullptr, "events_update: ws (workspace) missing");
  PD_REQUIRE(fc && truth && src_table && thr_table, "events_update: null input pointer");
  const int64_t P = (int64_t)H * W;
  PD_REQUIRE(P < (1ll << 31) - PLANE_PIECE, "events_update: a plane of %d x %d cells is too large", H, W);
  const int rows = events_rows(W);
  const int64_t ngroups = ceil_div64(H, rows), pairs = (int64_t)B * S;
  PD_REQUIRE(pairs * ngroups < (1ll << 31), "events_update: %lld workgroups exceed the grid limit",
             (long long)(pairs * ngroups));
  const int64_t n = (int64_t)S * H * EV_CNT;
  PD_REQUIRE(ceil_div64(n, 256) < (1ll << 31), "events_update: %lld counters exceed the grid limit", (long long)n);
  PD_REQUIRE(fc_bs >= P * C && truth_bs >= P * C, "events_update: batch strides shorter than one state");
  EventsArgs a;
  for (int s = 0; s < S; ++s) {
    const int kind = src_table[4 * s], c0 = src_table[4 * s + 1], c1 = src_table[4 * s + 2], nthr = src_table[4 * s + 3];
    PD_REQUIRE(kind == EV_PLAIN || kind == EV_SPEED || kind == EV_ANOMALY, "events_update: source %d has kind %d", s, kind);
    PD_REQUIRE(kind != EV_ANOMALY || clim != nullptr, "events_update: source %d is an anomaly, but there is no climatology",
               s);
    PD_REQUIRE(c0 >= 0 && c0 < C && (kind != EV_SPEED || (c1 >= 0 && c1 < C)),
               "events_update: source %d reads channels %d, %d outside [0, %d)", s, c0, c1, C);
    PD_REQUIRE(nthr >= 1 && nthr <= EV_TMAX, "events_update: source %d has %d thresholds, outside [1, %d]", s, nthr,
               EV_TMAX);
    const float sign = thr_table[s * (1 + EV_TMAX)];
    PD_REQUIRE(sign == 1.f || sign == -1.f, "events_update: source %d has sign %g, not +-1", s, (double)sign);
    a.src[s][0] = kind; a.src[s][1] = c0; a.src[s][2] = kind == EV_SPEED ? c1 : c0; a.src[s][3] = nthr;
    for (int j = 0; j <= EV_TMAX; ++j) a.thr[s][j] = thr_table[s * (1 + EV_TMAX) + j];
  }
  for (int s = S; s < EV_SMAX; ++s) {
    for (int j = 0; j < 4; ++j) a.src[s][j] = 0;
    for (int j = 0; j <= EV_TMAX; ++j) a.thr[s][j] = 0.f;
  }
  a.fc = fc; a.truth = truth; a.clim = clim; a.clim_index = clim_index;
  a.partial = static_cast<unsigned*>(ws);
  a.fc_bs = fc_bs; a.truth_bs = truth_bs; a.P = P;
  a.C = C; a.S = S; a.H = H; a.W = W; a.K = K; a.rows = rows; a.ngroups = (int)ngroups;
  const bool vec = (W % 4 == 0) && aligned16(fc) && aligned16(truth) && (fc_bs % 4 == 0) && (truth_bs % 4 == 0) &&
                   (clim == nullptr || aligned16(clim));
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)(pairs * ngroups));
  if (vec) hipLaunchKernelGGL(events_kernel<true>, grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL(events_kernel<false>, grid, dim3(256), 0, st, a);
  hipLaunchKernelGGL(events_finish_kernel, dim3((unsigned)ceil_div64(n, 256)), dim3(256), 0, st, a.partial, acc_lead,
                     n_samples_lead, B, n);
  PD_CHECK_LAUNCH("events_update");
  return 0;
}
