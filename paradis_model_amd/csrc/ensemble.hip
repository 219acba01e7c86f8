// Ensemble verification - one pass over the M members of G ensembles [G * M, C, H, W] (member-minor: member i of ensemble
// g is batch entry g M + i; physical units, fp32, one batch stride) and their truths [G, C, H, W] that forms, per
// ensemble g, chosen channel cs and latitude row h, the row sums of the CRPS and spread / skill terms and the histogram
// of the truth's rank, and a finishing kernel that folds the ensembles, in g order, into the rows of one lead.
// A cell is valid iff its truth y and all M member values x_i are finite; an invalid cell adds nothing anywhere.  Per
// valid cell, all in fp32, uncontracted, in exactly this order (rM = 1.0f / M from the host):
//   A  = sum_i |x_i - y|             i ascending, from 0.0f            P = sum_{i<j} |x_i - x_j|     i, then j ascending
//   m  = (sum_i x_i) * rM            E2 = (m - y) * (m - y)            V = sum_i (x_i - m) * (x_i - m)
//   lo = #{x_i < y}   eq = #{x_i == y}   r = lo + hash32(key) % (eq + 1)            (no sort: P is the CRPS's spread term)
//   key = uint32(((n C + c) H + h) W + w) + salt * 0x9E3779B9,  n = n_samples (as this call found it) + g
// Per row: four doubles {sum A, sum P, sum E2, sum V} - every cell term is widened before it meets another cell's - and
// EN_CNT(M) = 2 + M counters {nV, hist[0 .. M]}.  The integers are exact; the doubles are summed in a fixed order.
//
// Work layout (events.hip's): a workgroup of 256 threads owns ens_rows(W, M) whole rows of one (ensemble, channel) pair.
// Wave v owns the rows v, v + 4, .. of the group: a row's sums never cross waves.  A row is walked 64 Q cells at a time,
// lane l at the cells Q l .. Q l + Q - 1 of the walk (Q = 4; 2 in the 32-member variant, whose 33 planes would otherwise
// hold 132 values per lane): one 16-byte (8-byte) load per plane where VEC, scalar loads otherwise - the same bits, and
// the same lane has the same cells, so the lane's sums are the same too.  The M + 1 loads of a walk are issued before any
// arithmetic on them; the member values sit in registers indexed at compile time.  The member count is rounded up to a
// compiled variant MP of 4, 8, 16 or 32; members past M are neither loaded nor used (wave-uniform i < M guards; an
// ensemble of exactly MP members takes the FULL variant, compiled without them).  A lane
// adds its cells' terms in double in walk order, the wave folds the lanes by the xor tree of stream_common.h; the
// histogram is __popcll(__ballot(rank == r)) into scalar registers.  No LDS, no atomics: bit-identical run to run.
// Algorithmic HBM bytes per cell of a channel: 4 (M + 1).
#include "common.h"
#include "stream_common.h"

#include <cmath>

#pragma clang fp contract(off)

namespace {

constexpr int EN_MMAX = 32;                         // members per ensemble
constexpr int EN_BUDGET = 32768;                    // member values of one plane row group per workgroup (about)

constexpr int en_pad(int M) { return M <= 4 ? 4 : M <= 8 ? 8 : M <= 16 ? 16 : 32; }
inline int ens_rows(int W, int M) {
  const int r = (EN_BUDGET / en_pad(M) / (W < 1 ? 1 : W)) & ~3;
  return r < 4 ? 4 : r;
}

struct EnsArgs {
  const float* fc;
  const float* truth;
  const int* chan;                // [Cs] DEVICE
  const int64_t* n_samples;       // [1]: read, not written, by the counting kernel
  double* real;                   // [G][Cs][H][4]
  unsigned* cnt;                  // [G][Cs][H][2 + M]
  int64_t fc_bs, truth_bs, P;
  float rM;
  unsigned salt;
  int M, C, Cs, H, W, rows, ngroups;
};

__device__ __forceinline__ unsigned hash32(unsigned x) {
  x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
  return x;
}

// Q cells of row x from cell `at` (VEC: one aligned 8- or 16-byte load, the cells are whole) or from w0 with +0 past W
template <int Q, bool VEC>
__device__ __forceinline__ void load_cells(const float* __restrict__ x, int at, int w0, int W, float (&v)[Q]) {
  static_assert(Q == 4 || Q == 2, "a lane takes a quad or a pair of cells");
  if constexpr (VEC && Q == 4) {
    const float4 q = *reinterpret_cast<const float4*>(x + at);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else if constexpr (VEC) {
    const float2 q = *reinterpret_cast<const float2*>(x + at);
    v[0] = q.x; v[1] = q.y;
  } else {
#pragma unroll
    for (int k = 0; k < Q; ++k) v[k] = w0 + k < W ? x[w0 + k] : 0.f;
  }
}

// rows h0 + wave, h0 + wave + 4, .. < h1 of one (ensemble, channel): f0 the plane of member 0, t0 the truth's; key0 the
// hash key of cell (h = 0, w = 0) of this plane
template <int MP, int Q, bool VEC, bool FULL>
__device__ __forceinline__ void ens_rows_walk(const EnsArgs& a, const float* __restrict__ f0, const float* __restrict__ t0,
                                              unsigned key0, int h0, int h1, double* __restrict__ real,
                                              unsigned* __restrict__ cnt) {
  constexpr int WALK = 64 * Q;
  const int lane = (int)(threadIdx.x & 63);
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int M = FULL ? MP : a.M, W = a.W, NC = 2 + M;           // (FULL: M == MP, every guard below folds away)
  const float rM = a.rM;
  const int nwalk = (W + WALK - 1) / WALK;
  for (int h = h0 + wave; h < h1; h += 4) {
    const int64_t row = (int64_t)h * W;
    const unsigned keyh = key0 + (unsigned)h * (unsigned)W;
    double sA = 0.0, sP = 0.0, sE = 0.0, sV = 0.0;
    unsigned bins[MP + 1];
#pragma unroll
    for (int r = 0; r <= MP; ++r) bins[r] = 0u;
    // (the loop vectorizer would interleave two iterations and break the wide accesses into 4-byte ones)
#pragma clang loop vectorize(disable) interleave(disable)
    for (int wk = 0; wk < nwalk; ++wk) {
      const int w0 = WALK * wk + Q * lane;
      // VEC (W % 4 == 0: cells that start inside the row are whole): a lane past the row's end loads the row's last
      // cells instead - no branch around the loads - and they are not counted
      const int at = VEC ? min(w0, W - Q) : w0;
      float y[Q], x[MP][Q];
      load_cells<Q, VEC>(t0 + row, at, w0, W, y);
#pragma unroll
      for (int i = 0; i < MP; ++i) {
        if (i < M) {                                                  // (wave-uniform)
          load_cells<Q, VEC>(f0 + (int64_t)i * a.fc_bs + row, at, w0, W, x[i]);
        } else {
#pragma unroll
          for (int k = 0; k < Q; ++k) x[i][k] = 0.f;
        }
      }
      __builtin_amdgcn_sched_barrier(0);              // (every load of the walk is issued before the arithmetic)
      float A[Q], S[Q], Pp[Q], V[Q];
      unsigned lo[Q], eq[Q];
      bool ok[Q];
#pragma unroll
      for (int k = 0; k < Q; ++k) {
        A[k] = S[k] = Pp[k] = V[k] = 0.f;
        lo[k] = eq[k] = 0u;
        ok[k] = ((VEC ? w0 : w0 + k) < W) && __builtin_isfinite(y[k]);
      }
#pragma unroll
      for (int i = 0; i < MP; ++i) {
        if (i < M) {
#pragma unroll
          for (int k = 0; k < Q; ++k) {
            A[k] += fabsf(x[i][k] - y[k]);
            S[k] += x[i][k];
            lo[k] += x[i][k] < y[k] ? 1u : 0u;
            eq[k] += x[i][k] == y[k] ? 1u : 0u;
            ok[k] = ok[k] && __builtin_isfinite(x[i][k]);
          }
        }
      }
#pragma unroll
      for (int i = 0; i < MP; ++i) {
#pragma unroll
        for (int j = i + 1; j < MP; ++j) {
          if (j < M) {
#pragma unroll
            for (int k = 0; k < Q; ++k) Pp[k] += fabsf(x[i][k] - x[j][k]);
          }
        }
      }
      float E2[Q];
#pragma unroll
      for (int k = 0; k < Q; ++k) {
        S[k] = S[k] * rM;                                             // the ensemble mean
        const float d = S[k] - y[k];
        E2[k] = d * d;
      }
#pragma unroll
      for (int i = 0; i < MP; ++i) {
        if (i < M) {
#pragma unroll
          for (int k = 0; k < Q; ++k) {
            const float d = x[i][k] - S[k];
            V[k] += d * d;
          }
        }
      }
#pragma unroll
      for (int k = 0; k < Q; ++k) {
        sA += ok[k] ? (double)A[k] : 0.0;             // (sums of non-negative terms from +0: a +0 changes no bit)
        sP += ok[k] ? (double)Pp[k] : 0.0;
        sE += ok[k] ? (double)E2[k] : 0.0;
        sV += ok[k] ? (double)V[k] : 0.0;
        unsigned r = lo[k];
        if (ok[k] && eq[k] > 0u) r += hash32(keyh + (unsigned)(w0 + k)) % (eq[k] + 1u);
#pragma unroll
        for (int b = 0; b <= MP; ++b) {
          if (b <= M) bins[b] += count_lanes(ok[k] && r == (unsigned)b);
        }
      }
    }
    sA = wave_sum_f64(sA);
    sP = wave_sum_f64(sP);
    sE = wave_sum_f64(sE);
    sV = wave_sum_f64(sV);
    if (lane < 4) real[(int64_t)h * 4 + lane] = lane == 0 ? sA : lane == 1 ? sP : lane == 2 ? sE : sV;
    unsigned nV = 0u, mine = 0u;
#pragma unroll
    for (int b = 0; b <= MP; ++b) {
      nV += bins[b];                                                  // (bins past M are 0)
      mine = lane == 1 + b ? bins[b] : mine;
    }
    mine = lane == 0 ? nV : mine;
    if (lane < NC) cnt[(int64_t)h * NC + lane] = mine;
  }
}

template <int MP, int Q, bool VEC, bool FULL>
__global__ void __launch_bounds__(256) ens_kernel(EnsArgs a) {
  const int64_t pair = blockIdx.x / a.ngroups;                        // g Cs + cs
  const int grp = (int)(blockIdx.x - pair * a.ngroups);
  const int g = (int)(pair / a.Cs), cs = (int)(pair - (int64_t)g * a.Cs);
  const int h0 = grp * a.rows, h1 = min(a.H, h0 + a.rows);
  const int NC = 2 + a.M;
  double* real = a.real + pair * a.H * 4;
  unsigned* cnt = a.cnt + pair * a.H * NC;
  const int c = a.chan[cs];
  if (c < 0 || c >= a.C) {                          // (workgroup-uniform) no such plane: nothing is read, the sums say so
    const int lane = (int)(threadIdx.x & 63);
    for (int h = h0 + (int)(threadIdx.x >> 6); h < h1; h += 4) {
      if (lane < 4) real[(int64_t)h * 4 + lane] = NAN;
      if (lane < NC) cnt[(int64_t)h * NC + lane] = 0u;
    }
    return;
  }
  const float* f0 = a.fc + (int64_t)g * a.M * a.fc_bs + (int64_t)c * a.P;
  const float* t0 = a.truth + (int64_t)g * a.truth_bs + (int64_t)c * a.P;
  const unsigned n = (unsigned)a.n_samples[0] + (unsigned)g;
  const unsigned key0 = (n * (unsigned)a.C + (unsigned)c) * (unsigned)a.H * (unsigned)a.W + a.salt * 0x9E3779B9u;
  ens_rows_walk<MP, Q, VEC, FULL>(a, f0, t0, key0, h0, h1, real, cnt);
}

// one thread per accumulator entry of the lead: the doubles first ((acc + s_0) + s_1 .., g ascending), then the
// counters; ordinary read-modify-writes (launches of one stream are ordered); thread 0 adds G to the lead's ensemble count
__global__ void __launch_bounds__(256) ens_finish_kernel(const double* __restrict__ real, const unsigned* __restrict__ cnt,
                                                         double* __restrict__ acc_real, int64_t* __restrict__ acc_int,
                                                         int64_t* __restrict__ n_samples, int G, int64_t nreal,
                                                         int64_t nint) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i == 0) n_samples[0] += G;
  if (i < nreal) {
    double s = acc_real[i];
    for (int g = 0; g < G; ++g) s += real[(int64_t)g * nreal + i];
    acc_real[i] = s;
  } else if (i - nreal < nint) {
    const int64_t j = i - nreal;
    int64_t s = 0;
    for (int g = 0; g < G; ++g) s += (int64_t)cnt[(int64_t)g * nint + j];
    acc_int[j] += s;
  }
}

template <int MP, int Q>
void ens_launch(bool vec, dim3 grid, hipStream_t st, const EnsArgs& a) {
  const bool full = a.M == MP;
  if (vec && full) hipLaunchKernelGGL((ens_kernel<MP, Q, true, true>), grid, dim3(256), 0, st, a);
  else if (vec) hipLaunchKernelGGL((ens_kernel<MP, Q, true, false>), grid, dim3(256), 0, st, a);
  else if (full) hipLaunchKernelGGL((ens_kernel<MP, Q, false, true>), grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL((ens_kernel<MP, Q, false, false>), grid, dim3(256), 0, st, a);
}

}  // namespace

extern "C" int paradis_ens_max_members(void) { return EN_MMAX; }

extern "C" int paradis_ens_rows(int W, int M) { return (W < 1 || M < 2 || M > EN_MMAX) ? 0 : ens_rows(W, M); }

extern "C" size_t paradis_ens_ws_bytes(int G, int Cs, int H, int W, int M) {
  if (G < 1 || Cs < 1 || H < 1 || W < 1 || M < 2 || M > EN_MMAX) return 0;
  return (size_t)G * (size_t)Cs * (size_t)H * (4 * sizeof(double) + (size_t)(2 + M) * sizeof(unsigned));
}

extern "C" int paradis_ens_update(const float* fc, int64_t fc_bs, const float* truth, int64_t truth_bs, const int* chan,
                                  float rM, unsigned salt, double* acc_real_lead, int64_t* acc_int_lead,
                                  int64_t* n_samples_lead, void* ws, int G, int M, int C, int Cs, int H, int W,
                                  void* stream) {
  PD_REQUIRE(G >= 0 && C >= 1 && Cs >= 1 && H >= 1 && W >= 1, "ens_update: bad shape G=%d C=%d Cs=%d H=%d W=%d", G, C, Cs,
             H, W);
  PD_REQUIRE(M >= 2 && M <= EN_MMAX, "ens_update: %d members, outside [2, %d]", M, EN_MMAX);
  if (G == 0) return 0;
  PD_REQUIRE(acc_real_lead != nullptr && acc_int_lead != nullptr && n_samples_lead != nullptr,
             "ens_update: acc_real_lead / acc_int_lead / n_samples_lead missing");
  PD_REQUIRE(ws != nullptr, "ens_update: ws (workspace) missing");
  PD_REQUIRE(fc && truth && chan, "ens_update: null input pointer");
  const int64_t P = (int64_t)H * W;
  PD_REQUIRE(P < (1ll << 31) - PLANE_PIECE, "ens_update: a plane of %d x %d cells is too large", H, W);
  PD_REQUIRE(fc_bs >= P * C && truth_bs >= P * C, "ens_update: batch strides shorter than one state");
  EnsArgs a;
  a.rows = ens_rows(W, M);
  a.ngroups = (int)ceil_div64(H, a.rows);
  const int64_t pairs = (int64_t)G * Cs;
  PD_REQUIRE(pairs * a.ngroups < (1ll << 31), "ens_update: %lld workgroups exceed the grid limit",
             (long long)(pairs * a.ngroups));
  const int64_t nreal = (int64_t)Cs * H * 4, nint = (int64_t)Cs * H * (2 + M);
  PD_REQUIRE(ceil_div64(nreal + nint, 256) < (1ll << 31), "ens_update: %lld accumulator entries exceed the grid limit",
             (long long)(nreal + nint));
  a.fc = fc; a.truth = truth; a.chan = chan; a.n_samples = n_samples_lead;
  a.real = static_cast<double*>(ws);
  a.cnt = reinterpret_cast<unsigned*>(a.real + (int64_t)G * nreal);
  a.fc_bs = fc_bs; a.truth_bs = truth_bs; a.P = P;
  a.rM = rM; a.salt = salt;
  a.M = M; a.C = C; a.Cs = Cs; a.H = H; a.W = W;
  const bool vec = (W % 4 == 0) && aligned16(fc) && aligned16(truth) && (fc_bs % 4 == 0) && (truth_bs % 4 == 0);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)(pairs * a.ngroups));
  if (M <= 4) ens_launch<4, 4>(vec, grid, st, a);
  else if (M <= 8) ens_launch<8, 4>(vec, grid, st, a);
  else if (M <= 16) ens_launch<16, 4>(vec, grid, st, a);
  else ens_launch<32, 2>(vec, grid, st, a);
  hipLaunchKernelGGL(ens_finish_kernel, dim3((unsigned)ceil_div64(nreal + nint, 256)), dim3(256), 0, st, a.real, a.cnt,
                     acc_real_lead, acc_int_lead, n_samples_lead, G, nreal, nint);
  PD_CHECK_LAUNCH("ens_update");
  return 0;
}
