// Event sources - the one definition of what events.hip (contingency tables), fss.hip (fractions skill score) and
// probability.hip (joint histogram of an ensemble) decide per cell, and the one frame around their per-cell loops.
// Include in a unit built with -ffp-contract=off.
//   plain    x = v[c0]
//   speed    x = sqrtf(v[c0] * v[c0] + v[c1] * v[c1])        (mul, mul, add, sqrt: uncontracted)
//   anomaly  x = v[c0] - clim[clim_index[b]][c0]
// A cell is valid iff every value it reads is finite.  The event is sign * x >= thr' (sign = +-1: the product is exact;
// "le" is sign = -1, thr' = -thr on the host).  src_table [S][4] = {kind, c0, c1, nthr} and thr_table [S][1 + TMAX] =
// {sign, thr'...} are HOST memory, checked here and handed to the kernel as arguments: no copy node, and a captured launch
// keeps them.
// Work layout of the decision kernels: a workgroup of 256 threads owns `rows` whole rows of one (sample, source) pair -
// plane_rows(W) ~ PLANE_PIECE / W of them, or the unit's own number; block = pair * ngroups + group -, so clim_index[b],
// the source's table row and every plane base are workgroup-uniform.
// Once for the three units:
//   host    event_shape_check (in front of a unit's B == 0 return), event_launch_prologue (every check behind it,
//           event_sources_fill, the two grids), launch_lead_finish
//   device  source_planes, source_thresholds, event_source_value / event_cell (the decision), lead_finish_kernel
//           (acc += sum_b partial)
// Not here, on purpose: the decision kernels themselves - the blockIdx decode, the climatology-slot test, the KIND and
// threshold dispatch - and their per-cell loops.  The kernels sit at the scalar-register limit (SourceInputs carries 832
// bytes of tables as kernel arguments; scalars spill to vector lanes), and written over shared helpers (a decode struct,
// dispatch over lambdas) they compiled to other register counts and other spill placement than written out, and two
// units measured slower.  Each unit keeps its kernel, written out.
#pragma once
#include "common.h"
#include "stream_common.h"

#include <cmath>

#pragma clang fp contract(off)

constexpr int EVSRC_PLAIN = 0, EVSRC_SPEED = 1, EVSRC_ANOMALY = 2;
constexpr int EVSRC_TMAX = 8;                     // thresholds per source
constexpr int EVSRC_SMAX = 16;                    // sources per launch: their tables travel as kernel arguments

// what a decision kernel reads; filled by event_sources_fill
struct SourceInputs {
  const float* fc;
  const float* truth;
  const float* clim;        // [K][C][P] or null
  const int* clim_index;    // [B] or null
  int64_t fc_bs, truth_bs, P;
  int C, S, H, W, K, rows, ngroups;
  int src[EVSRC_SMAX][4];                 // {kind, c0, c1, nthr}, checked on the host
  float thr[EVSRC_SMAX][1 + EVSRC_TMAX];  // {sign, thr'...}
};

inline int plane_rows(int W) { return W >= PLANE_PIECE ? 1 : PLANE_PIECE / (W < 1 ? 1 : W); }

// the first checks of an entry point `who`, in front of its B == 0 return; kname: how it calls the climatology slots
inline int event_shape_check(const char* who, const char* kname, const float* clim, const int* clim_index, int K, int B,
                             int C, int S, int H, int W) {
  PD_REQUIRE(B >= 0 && C >= 1 && S >= 1 && S <= EVSRC_SMAX && H >= 1 && W >= 1,
             "%s: bad shape B=%d C=%d S=%d (at most %d) H=%d W=%d", who, B, C, S, EVSRC_SMAX, H, W);
  PD_REQUIRE((clim != nullptr) == (clim_index != nullptr),
             "%s: clim and clim_index go together (a climatology needs the slot of every sample)", who);
  PD_REQUIRE(clim == nullptr || K >= 1, "%s: %s must be >= 1 with a climatology, got %d", who, kname, K);
  return 0;
}

// checks the planes, the strides and the two host tables (non-null: the caller's check) and fills `in`; rows: the rows
// of a workgroup; vec: every plane quad is one aligned 16-byte load.  Returns the entry point's rc
inline int event_sources_fill(const char* who, SourceInputs& in, bool& vec, const float* fc, int64_t fc_bs,
                              const float* truth, int64_t truth_bs, const float* clim, const int* clim_index, int K,
                              const int* src_table, const float* thr_table, int C, int S, int H, int W, int rows) {
  const int64_t P = (int64_t)H * W;
  PD_REQUIRE(P < (1ll << 31) - PLANE_PIECE, "%s: a plane of %d x %d cells is too large", who, H, W);
  PD_REQUIRE(fc_bs >= P * C && truth_bs >= P * C, "%s: batch strides shorter than one state", who);
  for (int s = 0; s < EVSRC_SMAX; ++s) {
    for (int j = 0; j < 4; ++j) in.src[s][j] = 0;
    for (int j = 0; j <= EVSRC_TMAX; ++j) in.thr[s][j] = 0.f;
  }
  for (int s = 0; s < S; ++s) {
    const int kind = src_table[4 * s], c0 = src_table[4 * s + 1], c1 = src_table[4 * s + 2], nthr = src_table[4 * s + 3];
    PD_REQUIRE(kind == EVSRC_PLAIN || kind == EVSRC_SPEED || kind == EVSRC_ANOMALY, "%s: source %d has kind %d", who, s,
               kind);
    PD_REQUIRE(kind != EVSRC_ANOMALY || clim != nullptr, "%s: source %d is an anomaly, but there is no climatology", who,
               s);
    PD_REQUIRE(c0 >= 0 && c0 < C && (kind != EVSRC_SPEED || (c1 >= 0 && c1 < C)),
               "%s: source %d reads channels %d, %d outside [0, %d)", who, s, c0, c1, C);
    PD_REQUIRE(nthr >= 1 && nthr <= EVSRC_TMAX, "%s: source %d has %d thresholds, outside [1, %d]", who, s, nthr,
               EVSRC_TMAX);
    const float sign = thr_table[s * (1 + EVSRC_TMAX)];
    PD_REQUIRE(sign == 1.f || sign == -1.f, "%s: source %d has sign %g, not +-1", who, s, (double)sign);
    in.src[s][0] = kind; in.src[s][1] = c0; in.src[s][2] = kind == EVSRC_SPEED ? c1 : c0; in.src[s][3] = nthr;
    for (int j = 0; j <= EVSRC_TMAX; ++j) in.thr[s][j] = thr_table[s * (1 + EVSRC_TMAX) + j];
  }
  in.fc = fc; in.truth = truth; in.clim = clim; in.clim_index = clim_index;
  in.fc_bs = fc_bs; in.truth_bs = truth_bs; in.P = P;
  in.C = C; in.S = S; in.H = H; in.W = W; in.K = K;
  in.rows = rows;
  in.ngroups = (int)ceil_div64(H, in.rows);         // (<= H)
  vec = (W % 4 == 0) && aligned16(fc) && aligned16(truth) && (fc_bs % 4 == 0) && (truth_bs % 4 == 0) &&
        (clim == nullptr || aligned16(clim));
  return 0;
}

// what event_launch_prologue hands back beside the filled SourceInputs
struct EventLaunch {
  bool vec;
  unsigned grid, finish_grid;   // the decision kernel's workgroups, lead_finish_kernel's blocks: both checked
  int64_t n;                    // S H n_row, the counters of one sample's partials
};

// what differs between the units in event_launch_prologue
struct EventUnit {
  const char* who;
  bool ws_ok;                 // the unit's condition on its workspace, and the tail of the message
  const char* ws_also;
  bool inputs_ok;             // the same for its input pointers
  const char* inputs_which;
  int rows;                   // rows of a decision workgroup
  int n_row;                  // counters of a partial row
  int row_thr = EVSRC_TMAX;   // thresholds an accumulator row holds (probability.hip: its T)
  int64_t other_grid = 0;     // workgroups of the unit's second kernel (fss.hip: the windows)
};

// What the three entry points check behind their B == 0 return, in the order the messages fire, then the grids.  What
// stands in front of that return differs - events_update: event_shape_check; fss_update: also W and K (and, behind the
// return, its tables and half_y); prob_update: also M and T - and stays with each entry point, in its own order
inline int event_launch_prologue(const EventUnit& u, SourceInputs& in, EventLaunch& L, const void* acc_lead,
                                 const void* n_samples_lead, const float* fc, int64_t fc_bs, const float* truth,
                                 int64_t truth_bs, const float* clim, const int* clim_index, int K,
                                 const int* src_table, const float* thr_table, int B, int C, int S, int H, int W) {
  const char* who = u.who;
  PD_REQUIRE(acc_lead != nullptr && n_samples_lead != nullptr, "%s: acc_lead / n_samples_lead missing", who);
  PD_REQUIRE(u.ws_ok, "%s: ws (workspace) missing%s", who, u.ws_also);
  PD_REQUIRE(u.inputs_ok, "%s: null input pointer%s", who, u.inputs_which);
  const int rc = event_sources_fill(who, in, L.vec, fc, fc_bs, truth, truth_bs, clim, clim_index, K, src_table,
                                    thr_table, C, S, H, W, u.rows);
  if (rc != 0) return rc;
  for (int s = 0; s < S; ++s)
    PD_REQUIRE(in.src[s][3] <= u.row_thr, "%s: source %d has %d thresholds, the accumulator row holds T = %d", who, s,
               in.src[s][3], u.row_thr);
  const int64_t groups = (int64_t)B * S * in.ngroups;
  PD_REQUIRE(groups < (1ll << 31) && u.other_grid < (1ll << 31), "%s: %lld workgroups exceed the grid limit", who,
             (long long)std::max(groups, u.other_grid));
  L.n = (int64_t)S * H * u.n_row;
  PD_REQUIRE(ceil_div64(L.n, 256) < (1ll << 31), "%s: %lld counters exceed the grid limit", who, (long long)L.n);
  L.grid = (unsigned)groups;
  L.finish_grid = (unsigned)ceil_div64(L.n, 256);
  return 0;
}

// the planes of one source for one sample; f1 / t1: the second component of a speed source; cl: the climatology plane,
// which the caller sets once it has tested the sample's slot
struct SourcePlanes {
  const float* f0;
  const float* t0;
  const float* f1;
  const float* t1;
  const float* cl;
};

__device__ __forceinline__ SourcePlanes source_planes(const SourceInputs& in, int b, int s) {
  const int c0 = in.src[s][1], c1 = in.src[s][2];
  SourcePlanes p;
  p.f0 = in.fc + (int64_t)b * in.fc_bs + (int64_t)c0 * in.P;
  p.t0 = in.truth + (int64_t)b * in.truth_bs + (int64_t)c0 * in.P;
  p.f1 = in.fc + (int64_t)b * in.fc_bs + (int64_t)c1 * in.P;
  p.t1 = in.truth + (int64_t)b * in.truth_bs + (int64_t)c1 * in.P;
  p.cl = nullptr;
  return p;
}

// the quads of one lane for one walk (256 cells of one row); w0: the first cell of the lane's quad
struct SourceQuads {
  float fa[4], ta[4], fb[4], tb[4], cv[4];
  int w0;
};

// walk `wk` of row h: 256 cells from cell 256 wk, this lane's quad at w0 = 256 wk + 4 lane.  VEC (W % 4 == 0: a quad
// that starts inside the row is whole): a lane past the row's end loads the row's last quad instead - no branch around
// the loads, so that they can stay in flight - and its cells are not counted
template <int KIND, bool VEC>
__device__ __forceinline__ void source_load_walk(const SourcePlanes& p, int W, int h, int wk, int lane, SourceQuads& q) {
  const int64_t row = (int64_t)h * W;
  q.w0 = 256 * wk + 4 * lane;
  const int at = VEC ? min(q.w0, W - 4) : q.w0;
#pragma unroll
  for (int k = 0; k < 4; ++k) q.fb[k] = q.tb[k] = q.cv[k] = 0.f;
  load_quad<VEC>(p.f0 + row, at, W, q.fa);
  load_quad<VEC>(p.t0 + row, at, W, q.ta);
  if (KIND == EVSRC_SPEED) {
    load_quad<VEC>(p.f1 + row, at, W, q.fb);
    load_quad<VEC>(p.t1 + row, at, W, q.tb);
  }
  if (KIND == EVSRC_ANOMALY) load_quad<VEC>(p.cl + row, at, W, q.cv);
}

// the sign and the thresholds of table row `tab`; entries past nthr are NaN (x >= NaN is never an event)
__device__ __forceinline__ float source_thresholds(const float* __restrict__ tab, int nthr, float (&th)[EVSRC_TMAX]) {
  const float sign = tab[0];           // (read first: the order of the loads decides how many scalars the kernels spill)
#pragma unroll
  for (int j = 0; j < EVSRC_TMAX; ++j) th[j] = j < nthr ? tab[1 + j] : NAN;
  return sign;
}

// a: the value of channel c0, b: of channel c1 (speed only), cv: the climatology cell (anomaly only); returns whether the
// field's own values are finite and sets sx = sign x
template <int KIND>
__device__ __forceinline__ bool event_source_value(float a, float b, float cv, float sign, float& sx) {
  bool ok = __builtin_isfinite(a);
  float x = a;
  if (KIND == EVSRC_SPEED) {
    ok = ok && __builtin_isfinite(b);
    x = sqrtf(a * a + b * b);
  }
  if (KIND == EVSRC_ANOMALY) x = a - cv;
  sx = sign * x;
  return ok;
}

// one cell of both fields: sf / st = sign x of forecast / truth; returns whether the cell is valid (inside: it is a cell
// of the row at all)
template <int KIND>
__device__ __forceinline__ bool event_cell(bool inside, float fa, float ta, float fb, float tb, float cv, float sign,
                                           float& sf, float& st) {
  bool ok = event_source_value<KIND>(fa, fb, cv, sign, sf) && inside;
  ok = event_source_value<KIND>(ta, tb, cv, sign, st) && ok;
  if (KIND == EVSRC_ANOMALY) ok = ok && __builtin_isfinite(cv);
  return ok;
}

namespace {

// one thread per (source, row, counter of a partial row), n = S H n_row of them: acc += sum_b partial, b ascending, an
// ordinary read-modify-write (launches of one stream are ordered); thread 0 adds B to the lead's sample count.  T:
// unsigned or unsigned long long; an accumulator row has acc_row >= n_row entries, the partial row is its prefix
template <class T>
__global__ void __launch_bounds__(256) lead_finish_kernel(const T* __restrict__ partial, int64_t* __restrict__ acc,
                                                          int64_t* __restrict__ n_samples, int B, int64_t n, int n_row,
                                                          int acc_row) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i == 0) n_samples[0] += B;
  if (i >= n) return;
  int64_t s = 0;
  for (int b = 0; b < B; ++b) s += (int64_t)partial[(int64_t)b * n + i];
  int64_t at = i;
  if (acc_row != n_row) {              // (uniform: events.hip and probability.hip never pay the 64-bit division)
    const int64_t r = i / n_row;
    at = r * acc_row + (i - r * n_row);
  }
  acc[at] += s;
}

template <class T>
inline void launch_lead_finish(const EventLaunch& L, const T* partial, int64_t* acc_lead, int64_t* n_samples_lead, int B,
                               int n_row, int acc_row, hipStream_t st) {
  hipLaunchKernelGGL(lead_finish_kernel<T>, dim3(L.finish_grid), dim3(256), 0, st, partial, acc_lead, n_samples_lead, B,
                     L.n, n_row, acc_row);
}

}  // namespace
