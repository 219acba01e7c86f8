// Event verification - one pass over a forecast state and its truth [B, C, H, W] (physical units, fp32, each with its own
// batch stride) that counts, per sample b, event source s and latitude row h, the cells of the 2x2 contingency table of
// "value beyond a threshold" in forecast against truth, and a finishing kernel that adds the counts to the int64 row of
// one lead.  The sources, their host tables, validity and the event decision are event_source.h's (fss.hip and
// probability.hip decide the same events through the same header), and so are the entry point's checks behind its
// B == 0 return (event_launch_prologue) and the finishing kernel (lead_finish_kernel).  This unit keeps its decision
// kernel written out, its counters and its workspace.  The event is sign * x >= thr'[j],
// a cell is valid iff every value it reads is finite, and a sample whose clim_index is outside [0, K) has no valid cell
// for an anomaly source - nothing of that slot is read.  Per valid cell, F: the forecast is beyond thr'[j], O: the truth
// is.  Per row, EV_CNT counters:
//   [0] nV    [1 + j] nF[j]    [1 + TMAX + j] nO[j]    [1 + 2 TMAX + j] nFO[j]         (0 for j >= nthr)
// Everything after the decision is integer: the result is exact and the same whichever path produced it.
//
// Work layout (event_source.h): a workgroup of 256 threads owns a group of plane_rows(W) ~ PLANE_PIECE / W whole rows of
// one (sample, source) pair.  Wave v owns the rows v, v + 4, .. of the group: a row's counts never cross waves.  A row is
// walked 256 cells at a time,
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
#include "event_source.h"

#include <cmath>

#pragma clang fp contract(off)

namespace {

constexpr int EV_CNT = 1 + 3 * EVSRC_TMAX;        // counters per (source, row)

struct EventsArgs {
  SourceInputs in;
  unsigned* partial;        // [B][S][H][EV_CNT]
};

// rows h0 + wave, h0 + wave + 4, .. < h1 of one (sample, source): NT compiled thresholds th[0 .. NT).  The wave's walks
// (row after row, ceil(W / 256) per row) form one sequence; the quads of walk i + 1 are loaded before walk i is counted
template <int KIND, int NT, bool VEC>
__device__ __forceinline__ void events_count_rows(const SourcePlanes& p, float sign, const float (&th)[NT], int W, int h0,
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
  SourceQuads q;
  source_load_walk<KIND, VEC>(p, W, first, 0, lane, q);
  int h = first, wk = 0;                                            // the walk held in q
  // (the loop vectorizer would interleave two iterations and break the 16-byte accesses into 4-byte ones)
#pragma clang loop vectorize(disable) interleave(disable)
  for (int i = 0; i < nwalks; ++i) {
    const bool last_of_row = wk == wpr - 1, more = i + 1 < nwalks;
    // (after the last walk the same walk is loaded once more, unused: no branch around the loads)
    const int h_next = more && last_of_row ? h + 4 : h, wk_next = !more ? wk : last_of_row ? 0 : wk + 1;
    SourceQuads n;
    source_load_walk<KIND, VEC>(p, W, h_next, wk_next, lane, n);
    __builtin_amdgcn_sched_barrier(0);            // (the scheduler would sink the loads to the end of the counting)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float sf, st;
      const bool ok = event_cell<KIND>((VEC ? q.w0 : q.w0 + k) < W, q.fa[k], q.ta[k], q.fb[k], q.tb[k], q.cv[k], sign, sf,
                                       st);
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
        mine = lane == 1 + EVSRC_TMAX + j ? nO[j] : mine;
        mine = lane == 1 + 2 * EVSRC_TMAX + j ? nFO[j] : mine;
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
__device__ __forceinline__ void events_count_kind(const SourcePlanes& p, const float* __restrict__ tab, int nthr, int W,
                                                  int h0, int h1, unsigned* __restrict__ out) {
  float th[EVSRC_TMAX];
  const float sign = source_thresholds(tab, nthr, th);
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
  const SourceInputs& in = a.in;
  const int64_t pair = blockIdx.x / in.ngroups;                      // b S + s
  const int g = (int)(blockIdx.x - pair * in.ngroups);
  const int b = (int)(pair / in.S), s = (int)(pair - (int64_t)b * in.S);
  const int kind = in.src[s][0], nthr = in.src[s][3];
  const int h0 = g * in.rows, h1 = min(in.H, h0 + in.rows);
  unsigned* out = a.partial + pair * in.H * EV_CNT;
  SourcePlanes p = source_planes(in, b, s);
  const float* tab = in.thr[s];
  if (kind == EVSRC_ANOMALY) {
    const int slot = in.clim_index[b];
    if (slot < 0 || slot >= in.K) {                                         // (workgroup-uniform) nothing of such a slot is read
      const int lane = (int)(threadIdx.x & 63);
      for (int h = h0 + (int)(threadIdx.x >> 6); h < h1; h += 4)
        if (lane < EV_CNT) out[(int64_t)h * EV_CNT + lane] = 0u;
      return;
    }
    p.cl = in.clim + ((int64_t)slot * in.C + in.src[s][1]) * in.P;
    events_count_kind<EVSRC_ANOMALY, VEC>(p, tab, nthr, in.W, h0, h1, out);
  } else if (kind == EVSRC_SPEED) {
    events_count_kind<EVSRC_SPEED, VEC>(p, tab, nthr, in.W, h0, h1, out);
  } else {
    events_count_kind<EVSRC_PLAIN, VEC>(p, tab, nthr, in.W, h0, h1, out);
  }
}

}  // namespace

extern "C" int paradis_events_max_thresholds(void) { return EVSRC_TMAX; }

extern "C" int paradis_events_max_sources(void) { return EVSRC_SMAX; }

extern "C" int paradis_events_rows(int W) { return W < 1 ? 0 : plane_rows(W); }

extern "C" size_t paradis_events_ws_bytes(int B, int S, int H, int W) {
  if (B < 1 || S < 1 || H < 1 || W < 1) return 0;
  return (size_t)B * (size_t)S * (size_t)H * EV_CNT * sizeof(unsigned);
}

extern "C" int paradis_events_update(const float* fc, int64_t fc_bs, const float* truth, int64_t truth_bs,
                                     const float* clim, const int* clim_index, int K, const int* src_table,
                                     const float* thr_table, int64_t* acc_lead, int64_t* n_samples_lead, void* ws,
                                     int B, int C, int S, int H, int W, void* stream) {
  int rc = event_shape_check("events_update", "K", clim, clim_index, K, B, C, S, H, W);
  if (rc != 0 || B == 0) return rc;
  EventsArgs a;
  EventLaunch L;
  const EventUnit u{"events_update", ws != nullptr, "", fc && truth && src_table && thr_table, "", plane_rows(W), EV_CNT};
  rc = event_launch_prologue(u, a.in, L, acc_lead, n_samples_lead, fc, fc_bs, truth, truth_bs, clim, clim_index, K,
                             src_table, thr_table, B, C, S, H, W);
  if (rc != 0) return rc;
  a.partial = static_cast<unsigned*>(ws);
  hipStream_t st = (hipStream_t)stream;
  if (L.vec) hipLaunchKernelGGL(events_kernel<true>, dim3(L.grid), dim3(256), 0, st, a);
  else hipLaunchKernelGGL(events_kernel<false>, dim3(L.grid), dim3(256), 0, st, a);
  launch_lead_finish(L, a.partial, acc_lead, n_samples_lead, B, EV_CNT, EV_CNT, st);
  PD_CHECK_LAUNCH("events_update");
  return 0;
}
