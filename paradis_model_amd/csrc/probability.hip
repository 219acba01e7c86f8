// Probabilistic event verification - one pass over the M members of G ensembles [G * M, C, H, W] (member-minor: member i
// of ensemble g is batch entry g M + i; physical units, fp32, one batch stride) and their truths [G, C, H, W] that
// counts, per ensemble g, event source s, latitude row h and threshold j, the valid cells by (o, k) - o: the truth has
// the event, k: the number of members that have it, 0 .. M - and a finishing kernel that folds the ensembles, in g
// order, into the int64 row of one lead.  The sources, their host tables, validity and the event decision are
// event_source.h's (events.hip and fss.hip decide the same events through the same header), and so are the entry
// point's checks behind its G == 0 return (event_launch_prologue, which hands prob_rows(W) to event_sources_fill) and
// the finishing kernel (lead_finish_kernel); this unit keeps its decision kernel written out.  The event is
// sign * x >= thr'[j]; a cell is valid iff every value it reads is finite - the truth's, the climatology cell of an
// anomaly, all M members' -; an ensemble whose clim_index is outside [0, K) has no valid cell for an anomaly source and
// nothing of that slot is read.  Per row, NC = 1 + 2 T (M + 1) counters (T: the table's longest threshold list):
//   [0] nV      [1 + (j 2 + o) (M + 1) + k] joint[j][o][k]                                (0 for j >= nthr)
// Everything after the decision is integer: the result is exact and the same whichever path produced it.
//
// Work layout (event_source.h's, with fewer rows per workgroup): a workgroup of 256 threads owns a group of
// prob_rows(W) ~ PR_PIECE / W whole rows of one (ensemble, source) pair - a multiple of four, so that the four waves of
// a group have equal work, and M + 1 times the bytes of an events.hip row each: a 1440-cell row is a wave's whole work.
// Wave v owns the rows v, v + 4, .. of the group: a row's counters never cross waves.  A row is walked 256
// cells at a time, lane l at the quad of cells 4 l .. 4 l + 3 (one 16-byte load per plane where VEC, four scalar loads
// otherwise: the same bits).  The truth quad (and the climatology quad) and the first DEPTH member quads of a walk
// are loaded together (DEPTH = 8, 4 for a speed, whose members are two quads: 32 VGPRs either way); then the members
// are streamed, i = 0 .. M - 1, a runtime bound: member i is decided and counted
// into the lane's k[j][cell], and the load of member i + DEPTH goes into the registers it leaves (past the last
// member: the last member once more, unused - no branch around a load, so the waits stay counted).  No variant per M.
//
// Counting.  A wave keeps the histogram of its current row, [T][2][M + 1] uint32, in LDS (at most 2112 bytes per
// wave).  Per cell of the quad and threshold, the bin of the wave's first valid lane is broadcast, the lanes in the same
// bin are counted by a ballot and that first lane adds their number; the lanes in other bins add 1 each to their own -
// one LDS integer add instruction for both.  A dry field (every cell in one bin) therefore costs one add of one lane,
// a field spread over many bins one add per lane, and integer sums do not depend on their order.  nV is
// __popcll(__ballot(ok)) into a scalar register.  At the end of a row the wave copies the histogram to
// partial [G][S][H][NC] (uint32) with ordinary vector stores and clears it.  No global atomics, no float atomics.
// The number of thresholds is rounded up to 1, 2, 4 or 8 compiled variants, as in events.hip.
// Algorithmic HBM bytes per cell of a source: 4 (M + 1) plain, 8 (M + 1) speed, 4 (M + 1) + 4 anomaly.
#include "common.h"
#include "stream_common.h"
#include "event_source.h"

#include <cmath>

#pragma clang fp contract(off)

namespace {

constexpr int PR_MMAX = 32;                         // members per ensemble (ensemble.hip's limit)
constexpr int PR_PIECE = 1024;                      // cells of one plane per workgroup (about): 4 rows from W = 256 on
constexpr int pr_depth(int kind) { return kind == EVSRC_SPEED ? 4 : 8; }      // member quads in flight per lane
constexpr int PR_BINS_MAX = 2 * EVSRC_TMAX * (PR_MMAX + 1);

inline int prob_counters(int M, int T) { return 1 + 2 * T * (M + 1); }
inline int prob_rows(int W) {
  const int r = (PR_PIECE / (W < 1 ? 1 : W)) & ~3;
  return r < 4 ? 4 : r;
}

struct ProbArgs {
  SourceInputs in;          // fc: member 0 of ensemble 0, fc_bs: the stride between members; clim_index: [G]
  unsigned* partial;        // [G][S][H][NC]
  int M, T, NC;
};

// the quad(s) of one member for one lane
struct MemberQuad {
  float a[4], b[4];
};

template <int KIND, bool VEC>
__device__ __forceinline__ void load_member(const float* __restrict__ f0, const float* __restrict__ f1, int64_t off,
                                            int at, int W, MemberQuad& q) {
  load_quad<VEC>(f0 + off, at, W, q.a);
  if (KIND == EVSRC_SPEED) load_quad<VEC>(f1 + off, at, W, q.b);
}

// rows h0 + wave, h0 + wave + 4, .. < h1 of one (ensemble, source): NT compiled thresholds th[0 .. NT), of which the
// first nthr are the source's; p.f0 / p.f1: the planes of member 0; hist: this wave's LDS histogram, all zero
template <int KIND, int NT, bool VEC>
__device__ __forceinline__ void prob_count_rows(const ProbArgs& a, const SourcePlanes& p, float sign,
                                                const float (&th)[NT], int nthr, int h0, int h1,
                                                unsigned* __restrict__ out, unsigned* hist) {
  const int lane = (int)(threadIdx.x & 63);
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int M = a.M, W = a.in.W, M1 = M + 1, NC = a.NC, NB = NC - 1;
  const int64_t bs = a.in.fc_bs;
  const int wpr = (W + 255) / 256;                                  // walks per row
  constexpr int DEPTH = pr_depth(KIND);
  for (int h = h0 + wave; h < h1; h += 4) {
    const int64_t row = (int64_t)h * W;
    unsigned nV = 0;
    // (the loop vectorizer would interleave two iterations and break the 16-byte accesses into 4-byte ones)
#pragma clang loop vectorize(disable) interleave(disable)
    for (int wk = 0; wk < wpr; ++wk) {
      const int w0 = 256 * wk + 4 * lane;
      // VEC (W % 4 == 0: a quad that starts inside the row is whole): a lane past the row's end loads the row's last
      // quad instead - no branch around the loads - and its cells are not counted
      const int at = VEC ? min(w0, W - 4) : w0;
      float ta[4], tb[4], cv[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) tb[k] = cv[k] = 0.f;
      load_quad<VEC>(p.t0 + row, at, W, ta);
      if (KIND == EVSRC_SPEED) load_quad<VEC>(p.t1 + row, at, W, tb);
      if (KIND == EVSRC_ANOMALY) load_quad<VEC>(p.cl + row, at, W, cv);
      // (member loads carry no branch - a load under a wave-uniform branch makes every later wait a wait for all
      // loads -: a slot past the last member loads the last member again, a hit in the cache, and is not consumed)
      MemberQuad buf[DEPTH];
#pragma unroll
      for (int d = 0; d < DEPTH; ++d)
        load_member<KIND, VEC>(p.f0, p.f1, (int64_t)min(d, M - 1) * bs + row, at, W, buf[d]);
      __builtin_amdgcn_sched_barrier(0);            // (the loads of the walk's head are issued before any arithmetic)
      float st[4];
      bool ok[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        ok[k] = event_source_value<KIND>(ta[k], tb[k], cv[k], sign, st[k]) && ((VEC ? w0 : w0 + k) < W);
        if (KIND == EVSRC_ANOMALY) ok[k] = ok[k] && __builtin_isfinite(cv[k]);
      }
      // o (M + 1) + k per threshold and cell: it starts at the truth's o (M + 1) and counts the members with the event
      unsigned kc[NT][4];
#pragma unroll
      for (int j = 0; j < NT; ++j) {
#pragma unroll
        for (int k = 0; k < 4; ++k) kc[j][k] = st[k] >= th[j] ? (unsigned)M1 : 0u;
      }
      for (int i = 0; i < M; i += DEPTH) {
#pragma unroll
        for (int d = 0; d < DEPTH; ++d) {
          if (i + d < M) {                                            // (wave-uniform)
#pragma unroll
            for (int k = 0; k < 4; ++k) {
              float sx;
              ok[k] = event_source_value<KIND>(buf[d].a[k], buf[d].b[k], cv[k], sign, sx) && ok[k];
#pragma unroll
              for (int j = 0; j < NT; ++j) kc[j][k] += sx >= th[j] ? 1u : 0u;
            }
          }
          load_member<KIND, VEC>(p.f0, p.f1, (int64_t)min(i + d + DEPTH, M - 1) * bs + row, at, W, buf[d]);
          __builtin_amdgcn_sched_barrier(0);        // (the next member's load stays where it was written)
        }
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const unsigned long long act = __ballot(ok[k]);
        nV += (unsigned)__popcll(act);
        if (act == 0ull) continue;                                    // (wave-uniform)
        const int leader = __builtin_amdgcn_readfirstlane((int)__builtin_ctzll(act));
#pragma unroll
        for (int j = 0; j < NT; ++j) {
          if (j < nthr) {                                             // (wave-uniform)
            const int bin = 2 * j * M1 + (int)kc[j][k];
            const int first = __builtin_amdgcn_readlane(bin, leader);
            const bool same = ok[k] && bin == first;
            const unsigned n = count_lanes(same);
            const unsigned add = !ok[k] ? 0u : !same ? 1u : lane == leader ? n : 0u;
            if (add != 0u)
              __hip_atomic_fetch_add(&hist[bin], add, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          }
        }
      }
    }
    // the row leaves the wave: its histogram to the partial row, then cleared for the next row
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    unsigned* o = out + (int64_t)h * NC;
    if (lane == 0) o[0] = nV;
    for (int i = lane; i < NB; i += 64) {
      o[1 + i] = hist[i];
      hist[i] = 0u;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
  }
}

template <int KIND, bool VEC>
__device__ __forceinline__ void prob_count_kind(const ProbArgs& a, const SourcePlanes& p, const float* __restrict__ tab,
                                                int nthr, int h0, int h1, unsigned* __restrict__ out, unsigned* hist) {
  float th[EVSRC_TMAX];
  const float sign = source_thresholds(tab, nthr, th);
  if (nthr <= 1) {
    const float t1[1] = {th[0]};
    prob_count_rows<KIND, 1, VEC>(a, p, sign, t1, nthr, h0, h1, out, hist);
  } else if (nthr <= 2) {
    const float t2[2] = {th[0], th[1]};
    prob_count_rows<KIND, 2, VEC>(a, p, sign, t2, nthr, h0, h1, out, hist);
  } else if (nthr <= 4) {
    const float t4[4] = {th[0], th[1], th[2], th[3]};
    prob_count_rows<KIND, 4, VEC>(a, p, sign, t4, nthr, h0, h1, out, hist);
  } else {
    prob_count_rows<KIND, 8, VEC>(a, p, sign, th, nthr, h0, h1, out, hist);
  }
}

template <bool VEC>
__global__ void __launch_bounds__(256) prob_kernel(ProbArgs a) {
  __shared__ unsigned hist_all[4][PR_BINS_MAX];
  const SourceInputs& in = a.in;
  const int64_t pair = blockIdx.x / in.ngroups;                      // g S + s
  const int grp = (int)(blockIdx.x - pair * in.ngroups);
  const int g = (int)(pair / in.S), s = (int)(pair - (int64_t)g * in.S);
  const int kind = in.src[s][0], nthr = in.src[s][3];
  const int h0 = grp * in.rows, h1 = min(in.H, h0 + in.rows);
  const int lane = (int)(threadIdx.x & 63);
  unsigned* out = a.partial + pair * in.H * a.NC;
  unsigned* hist = hist_all[threadIdx.x >> 6];
  for (int i = lane; i < a.NC - 1; i += 64) hist[i] = 0u;            // (each wave its own: no workgroup barrier)
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
  // member 0 of ensemble g is batch entry g M; the truth of ensemble g is entry g
  SourcePlanes p = source_planes(in, g, s);
  const int64_t lead = (int64_t)g * (a.M - 1) * in.fc_bs;            // (source_planes went g strides: M g in all)
  p.f0 += lead;
  p.f1 += lead;
  const float* tab = in.thr[s];
  if (kind == EVSRC_ANOMALY) {
    const int slot = in.clim_index[g];
    if (slot < 0 || slot >= in.K) {                                  // (workgroup-uniform) nothing of such a slot is read
      for (int h = h0 + (int)(threadIdx.x >> 6); h < h1; h += 4)
        for (int i = lane; i < a.NC; i += 64) out[(int64_t)h * a.NC + i] = 0u;
      return;
    }
    p.cl = in.clim + ((int64_t)slot * in.C + in.src[s][1]) * in.P;
    prob_count_kind<EVSRC_ANOMALY, VEC>(a, p, tab, nthr, h0, h1, out, hist);
  } else if (kind == EVSRC_SPEED) {
    prob_count_kind<EVSRC_SPEED, VEC>(a, p, tab, nthr, h0, h1, out, hist);
  } else {
    prob_count_kind<EVSRC_PLAIN, VEC>(a, p, tab, nthr, h0, h1, out, hist);
  }
}

inline bool prob_members_ok(int M) { return M >= 2 && M <= PR_MMAX; }
inline bool prob_thresholds_ok(int T) { return T >= 1 && T <= EVSRC_TMAX; }

}  // namespace

extern "C" int paradis_prob_max_members(void) { return PR_MMAX; }

extern "C" int paradis_prob_rows(int W) { return W < 1 ? 0 : prob_rows(W); }

extern "C" int paradis_prob_counters(int M, int T) {
  return (prob_members_ok(M) && prob_thresholds_ok(T)) ? prob_counters(M, T) : 0;
}

extern "C" size_t paradis_prob_ws_bytes(int G, int S, int H, int W, int M, int T) {
  if (G < 1 || S < 1 || H < 1 || W < 1 || !prob_members_ok(M) || !prob_thresholds_ok(T)) return 0;
  return (size_t)G * (size_t)S * (size_t)H * (size_t)prob_counters(M, T) * sizeof(unsigned);
}

extern "C" int paradis_prob_update(const float* fc, int64_t fc_bs, const float* truth, int64_t truth_bs,
                                   const float* clim, const int* clim_index, int K, const int* src_table,
                                   const float* thr_table, int64_t* acc_lead, int64_t* n_samples_lead, void* ws, int G,
                                   int M, int T, int C, int S, int H, int W, void* stream) {
  int rc = event_shape_check("prob_update", "K", clim, clim_index, K, G, C, S, H, W);
  if (rc != 0) return rc;
  PD_REQUIRE(prob_members_ok(M), "prob_update: %d members, outside [2, %d]", M, PR_MMAX);
  PD_REQUIRE(prob_thresholds_ok(T), "prob_update: T = %d thresholds per source, outside [1, %d]", T, EVSRC_TMAX);
  if (G == 0) return 0;
  ProbArgs a;
  EventLaunch L;
  a.M = M; a.T = T; a.NC = prob_counters(M, T);
  const EventUnit u{"prob_update", ws != nullptr, "", fc && truth && src_table && thr_table, "", prob_rows(W), a.NC, T};
  rc = event_launch_prologue(u, a.in, L, acc_lead, n_samples_lead, fc, fc_bs, truth, truth_bs, clim, clim_index, K,
                             src_table, thr_table, G, C, S, H, W);
  if (rc != 0) return rc;
  a.partial = static_cast<unsigned*>(ws);
  hipStream_t st = (hipStream_t)stream;
  if (L.vec) hipLaunchKernelGGL(prob_kernel<true>, dim3(L.grid), dim3(256), 0, st, a);
  else hipLaunchKernelGGL(prob_kernel<false>, dim3(L.grid), dim3(256), 0, st, a);
  launch_lead_finish(L, a.partial, acc_lead, n_samples_lead, G, a.NC, a.NC, st);
  PD_CHECK_LAUNCH("prob_update");
  return 0;
}
