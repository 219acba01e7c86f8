// Forecast verification - one pass over a forecast state and its truth [B, C, H, W] (physical units, fp32, each with its
// own batch stride: chunk[:, slot] and truth[:, k] are consumed in place) and, optionally, the climatology slot
// clim[clim_index[b]] of each sample, that yields per sample b and channel c the latitude-weighted sums of
// WeatherBench-2's deterministic scores (w = lat_w[h], fa = f - clim, ta = t - clim):
//   s0 = sum w (f-t)^2    s1 = sum w (f-t)    s2 = sum w |f-t|    s3 = sum w fa^2    s4 = sum w ta^2    s5 = sum w fa ta
// and a finishing kernel that folds them, in double and in a fixed order, into the eight accumulators of (lead, c):
//   se = s0 / Z, e = s1 / Z, ae = s2 / Z, acc_b = s5 / sqrt(s3 s4) (the sample is left out of the ACC mean when s3 s4 == 0)
//   acc[c] += {1, se, e, ae, acc_b, 1 (0 when left out), s3, s4}      = {n, sum se, sum e, sum ae, sum acc_b, n_acc, sum ff, sum tt}
// Without a climatology only s0 .. s2 exist, no third tensor is read and acc[c][4 .. 7] are not touched.
// Non-finite values are not masked: they propagate into every sum of their plane.
//
// Work layout (stream_common.h; the piece loop is written out here): a workgroup sees ONE plane - piece j of plane
// (b, c) - so clim_index[b] and the three plane bases are workgroup-uniform.  The thread's sums are fp32 over its at most
// PLANE_PIECE / 256 = 32 cells; they are widened to double before the wave shuffles, the LDS step across the four waves
// and the store (partial [6 or 3][B C][npieces]).
// Algorithmic HBM bytes: 12*B*C*H*W with a climatology, 8*B*C*H*W without.
#include "common.h"
#include "stream_common.h"

#include <cmath>

#pragma clang fp contract(off)

namespace {

constexpr int VERIFY_ACC = 8;                     // doubles per (lead, channel)

constexpr int verify_sums(bool clim) { return clim ? 6 : 3; }

struct VerifyArgs {
  const float* fc;
  const float* truth;
  const float* clim;        // [K][C][P] or null
  const int* clim_index;    // [B] or null
  const float* lat_w;       // [H]
  double* partial;          // [6 or 3][B C][npieces]
  int64_t fc_bs, truth_bs;
  int64_t P;
  int C, W, K, npieces, vec;
  int64_t planes;           // B C
};

// cells [start, end) of one plane; VEC: every quad is whole, 16-byte aligned and inside one row
template <bool CLIM, bool VEC>
__device__ __forceinline__ void verify_piece_sums(const float* __restrict__ f, const float* __restrict__ t,
                                                  const float* __restrict__ cl, const float* __restrict__ lat_w, int W,
                                                  int start, int end, float (&s)[6]) {
  // (the loop vectorizer would interleave two iterations and break the 16-byte accesses into 4-byte ones)
#pragma clang loop vectorize(disable) interleave(disable) unroll(full)
  for (int i = 0; i < PLANE_ITERS; ++i) {
    const int q0 = start + 4 * (256 * i + (int)threadIdx.x);
    if (q0 >= end) break;
    float fv[4], tv[4], cv[4] = {0.f, 0.f, 0.f, 0.f}, wv[4];
    const int h0 = q0 / W;
    if (VEC) {
      load_quad<true>(f, q0, end, fv);
      load_quad<true>(t, q0, end, tv);
      if (CLIM) load_quad<true>(cl, q0, end, cv);
      wv[0] = wv[1] = wv[2] = wv[3] = lat_w[h0];
    } else {
      const int w0 = q0 - h0 * W;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const bool in = q0 + k < end;
        fv[k] = in ? f[q0 + k] : 0.f;
        tv[k] = in ? t[q0 + k] : 0.f;
        if (CLIM) cv[k] = in ? cl[q0 + k] : 0.f;
        wv[k] = in ? lat_w[h0 + (w0 + k) / W] : 0.f;
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (!VEC && !(q0 + k < end)) continue;        // cells past the end add nothing, not even a +0
      const float w = wv[k];
      const float d = fv[k] - tv[k];
      s[0] += w * (d * d);
      s[1] += w * d;
      s[2] += w * fabsf(d);
      if (CLIM) {
        const float fa = fv[k] - cv[k], ta = tv[k] - cv[k];
        s[3] += w * (fa * fa);
        s[4] += w * (ta * ta);
        s[5] += w * (fa * ta);
      }
    }
  }
}

template <bool CLIM>
__global__ void __launch_bounds__(256) verify_kernel(VerifyArgs a) {
  constexpr int NS = verify_sums(CLIM);
  const int64_t plane = blockIdx.x / a.npieces;                      // b C + c
  const int piece = (int)(blockIdx.x - plane * a.npieces);
  const int b = (int)(plane / a.C), c = (int)(plane - (int64_t)b * a.C);
  const float* f = a.fc + (int64_t)b * a.fc_bs + (int64_t)c * a.P;
  const float* t = a.truth + (int64_t)b * a.truth_bs + (int64_t)c * a.P;
  const float* cl = nullptr;
  bool bad_slot = false;                                             // (workgroup-uniform)
  if (CLIM) {
    const int k = a.clim_index[b];
    bad_slot = k < 0 || k >= a.K;                                    // nothing of such a slot is read: its sums are NaN
    if (!bad_slot) cl = a.clim + ((int64_t)k * a.C + c) * a.P;
  }
  float s[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (!bad_slot) {
    const int start = piece * PLANE_PIECE;                           // P < 2^31
    const int end = (int)min(a.P, (int64_t)start + PLANE_PIECE);
    if (a.vec) verify_piece_sums<CLIM, true>(f, t, cl, a.lat_w, a.W, start, end, s);
    else verify_piece_sums<CLIM, false>(f, t, cl, a.lat_w, a.W, start, end, s);
  }
  double sd[NS];
#pragma unroll
  for (int i = 0; i < NS; ++i) sd[i] = wave_sum_f64((double)s[i]);
  block_fold4(sd, [&](int i, double v) {
    a.partial[((int64_t)i * a.planes + plane) * a.npieces + piece] = bad_slot ? (double)NAN : v;
  });
}

// one workgroup (one wave) per channel; for b = 0 .. B - 1 in order: lane i < NS folds the pieces of sum i of plane
// (b, c) in index order, lane 0 forms the sample's scores and adds them to its copy of the channel's accumulators,
// which it read at the start and stores at the end (launches of one stream are ordered: an ordinary read-modify-write)
template <bool CLIM>
__global__ void __launch_bounds__(64) verify_finish_kernel(const double* __restrict__ partial, double* __restrict__ acc,
                                                           int B, int C, int npieces, double Z) {
  constexpr int NS = verify_sums(CLIM);
  __shared__ double tot[NS];
  const int c = blockIdx.x;
  const int64_t planes = (int64_t)B * C;
  double a[VERIFY_ACC] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (threadIdx.x == 0) {
#pragma unroll
    for (int i = 0; i < VERIFY_ACC; ++i) a[i] = acc[(int64_t)c * VERIFY_ACC + i];
  }
  for (int b = 0; b < B; ++b) {
    if (threadIdx.x < NS) {
      const double* p = partial + ((int64_t)threadIdx.x * planes + ((int64_t)b * C + c)) * npieces;
      double s = 0.0;
      for (int k = 0; k < npieces; ++k) s += p[k];
      tot[threadIdx.x] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      a[0] += 1.0;
      a[1] += tot[0] / Z;
      a[2] += tot[1] / Z;
      a[3] += tot[2] / Z;
      if (CLIM) {
        const double ff = tot[3], tt = tot[4], ft = tot[5];
        if (ff * tt != 0.0) {                    // (a NaN product is not zero: the sample counts and its NaN propagates)
          a[4] += ft / sqrt(ff * tt);
          a[5] += 1.0;
        }
        a[6] += ff;
        a[7] += tt;
      }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
#pragma unroll
    for (int i = 0; i < (CLIM ? VERIFY_ACC : 4); ++i) acc[(int64_t)c * VERIFY_ACC + i] = a[i];
  }
}

inline int64_t verify_pieces(int H, int W) { return ceil_div64((int64_t)H * W, PLANE_PIECE); }

}  // namespace

extern "C" int paradis_verify_piece(void) { return PLANE_PIECE; }

extern "C" size_t paradis_verify_ws_bytes(int B, int C, int H, int W, int with_clim) {
  if (B < 1 || C < 1 || H < 1 || W < 1) return 0;
  return (size_t)verify_sums(with_clim != 0) * (size_t)B * (size_t)C * (size_t)verify_pieces(H, W) * sizeof(double);
}

extern "C" int paradis_verify_update(const float* fc, int64_t fc_bs, const float* truth, int64_t truth_bs,
                                     const float* clim, const int* clim_index, int K, const float* lat_w, double Z,
                                     double* acc, void* ws, int B, int C, int H, int W, void* stream) {
  PD_REQUIRE(B >= 0 && C >= 1 && H >= 1 && W >= 1, "verify_update: bad shape B=%d C=%d H=%d W=%d", B, C, H, W);
  PD_REQUIRE((clim != nullptr) == (clim_index != nullptr),
             "verify_update: clim and clim_index go together (a climatology needs the slot of every sample)");
  PD_REQUIRE(clim == nullptr || K >= 1, "verify_update: K must be >= 1 with a climatology, got %d", K);
  PD_REQUIRE(std::isfinite(Z) && Z > 0.0, "verify_update: Z must be finite and > 0, got %g", Z);
  if (B == 0) return 0;
  PD_REQUIRE(acc != nullptr, "verify_update: acc missing");
  PD_REQUIRE(ws != nullptr, "verify_update: ws (workspace) missing");
  PD_REQUIRE(fc && truth && lat_w, "verify_update: null input pointer");
  const int64_t P = (int64_t)H * W;
  PD_REQUIRE(P < (1ll << 31) - PLANE_PIECE, "verify_update: a plane of %d x %d cells is too large", H, W);
  const int64_t npieces = verify_pieces(H, W), planes = (int64_t)B * C;
  PD_REQUIRE(planes * npieces < (1ll << 31), "verify_update: %lld workgroups exceed the grid limit",
             (long long)(planes * npieces));
  PD_REQUIRE(fc_bs >= P * C && truth_bs >= P * C, "verify_update: batch strides shorter than one state");
  VerifyArgs a;
  a.fc = fc; a.truth = truth; a.clim = clim; a.clim_index = clim_index; a.lat_w = lat_w;
  a.partial = static_cast<double*>(ws);
  a.fc_bs = fc_bs; a.truth_bs = truth_bs; a.P = P;
  a.C = C; a.W = W; a.K = K; a.npieces = (int)npieces; a.planes = planes;
  a.vec = (W % 4 == 0) && aligned16(fc) && aligned16(truth) && (fc_bs % 4 == 0) && (truth_bs % 4 == 0) &&
          (clim == nullptr || aligned16(clim));
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)(planes * npieces));
  if (clim != nullptr) {
    hipLaunchKernelGGL(verify_kernel<true>, grid, dim3(256), 0, st, a);
    hipLaunchKernelGGL(verify_finish_kernel<true>, dim3(C), dim3(64), 0, st, a.partial, acc, B, C, (int)npieces, Z);
  } else {
    hipLaunchKernelGGL(verify_kernel<false>, grid, dim3(256), 0, st, a);
    hipLaunchKernelGGL(verify_finish_kernel<false>, dim3(C), dim3(64), 0, st, a.partial, acc, B, C, (int)npieces, Z);
  }
  PD_CHECK_LAUNCH("verify_update");
  return 0;
}
