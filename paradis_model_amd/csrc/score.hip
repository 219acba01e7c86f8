// Validation scores - one pass over a model output and its target [B, C, H, W] (normalised, fp32, each with its own
// batch stride: the target is true_data[:, step], consumed in place) that yields every number a validation or logging
// step needs (reference trainer.py:652-708 with _get_report_rmse, trainer.py:291-315, and utils/loss.py:105-127):
//   s0[c] = sum l(e)            e = pred - target, l as paradis_loss_kernel (train.hip): 0 mse, 1 smooth reversed Huber
//   s1[c] = sum wl[h] l(e)      only with the loss's latitude weights
//   s2[c] = sum lat_w[h] d^2    report channels only; d in physical units by the channel's normalisation class:
//                               z-score (target - pred) * std, humidity / precipitation the difference of the two
//                               de-normalised values (utils/normalization.py:39-52,69-80), fp32 in the reference's order
// and a finishing kernel that combines the partials in double, in a fixed order, into one fp32 row
//   out[0]            mean_c(wf[c] (s1 or s0)[c] / N)                  = ParadisLoss.forward
//   out[1 .. C]       wf[c] (s1 or s0)[c] / N                          = per_channel_loss(weighted=True)
//   out[1+C .. 2C]    s0[c] / N                                        = per_channel_loss(weighted=False)
//   out[1+2C+r]       sqrt(s2[chan(r)] / N),  N = B H W                = _get_report_rmse
// kind 2 ("none": the AMSE validation loss, whose value comes from paradis_amse_loss) skips s0 / s1 and writes zeros;
// workgroups of channels without a report then read nothing.
//
// Work layout (stream_common.h; the piece loop is written out here): a workgroup sees ONE channel - piece k of plane
// (b, c) - so weights, class and de-normalisation constants are workgroup-uniform.  The thread's and the workgroup's sums
// stay fp32 (three ordinary stores per workgroup); the finishing kernel folds them in double.
// Algorithmic HBM bytes: 8*B*C*H*W (the training loss kernel with its gradient store: 12).
#include "common.h"
#include "normalize.h"
#include "stream_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int KIND_NONE = 2;   // the loss kind "none"; the normalisation classes of the reports are normalize.h's NORM_*

struct ScoreArgs {
  const float* pred;
  const float* target;
  const float* wl;      // [H] or null
  const float* lat_w;   // [H] (null when there are no reports)
  const int* rflag;     // [C] >= 0: a report channel, -1: none (null when there are no reports)
  const int* rcls;      // [C]
  const float* rp0;     // [C] q_min
  const float* rp1;     // [C] std | q_max
  float* partial;       // [3][C][nb]
  int64_t pred_bs, target_bs;
  int64_t P;
  int C, W, npieces, nb, kind;
  float delta;
};

__device__ __forceinline__ float loss_term(float e, int kind, float delta) {
  if (kind == 0) return e * e;
  const float a = fabsf(e);
  const float s = 1.0f / (1.0f + expf(-2.0f * (a - delta)));
  const float small = delta * a;
  const float large = (e * e + delta * delta) / (2.0f * delta);
  return (1.0f - s) * small + s * large;
}

template <bool VEC>
__global__ void __launch_bounds__(256) val_score_kernel(ScoreArgs a) {
  const int c = blockIdx.x / a.nb;
  const int j = blockIdx.x - c * a.nb;
  const int b = j / a.npieces;
  const int64_t start = (int64_t)(j - b * a.npieces) * PLANE_PIECE;
  const int cls = (a.rflag != nullptr && a.rflag[c] >= 0) ? a.rcls[c] : 0;      // 0: not a report channel
  const bool with_loss = a.kind != KIND_NONE;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f;
  if (with_loss || cls != 0) {       // (workgroup-uniform)
    const float* p = a.pred + (int64_t)b * a.pred_bs + (int64_t)c * a.P;
    const float* t = a.target + (int64_t)b * a.target_bs + (int64_t)c * a.P;
    const float std_r = cls == NORM_ZSCORE ? a.rp1[c] : 1.0f;
    float lmin = 0.f, lspan = 0.f, qmax = 0.f;
    if (cls == NORM_HUMIDITY) {
      qmax = a.rp1[c];
      lmin = logf(a.rp0[c]);
      lspan = logf(qmax) - lmin;
    }
    const int64_t end = min(a.P, start + PLANE_PIECE);
#pragma unroll
    for (int i = 0; i < PLANE_ITERS; ++i) {
      const int64_t q0 = start + 4 * (int64_t)(256 * i + (int)threadIdx.x);
      if (q0 >= end) break;
      float pv[4], tv[4];
      int hv[4];
      const int h0 = (int)(q0 / a.W);
      if (VEC) {     // W % 4 == 0, P % 4 == 0: the four cells exist and share a row
        load_quad<true>(p, q0, end, pv);
        load_quad<true>(t, q0, end, tv);
        hv[0] = hv[1] = hv[2] = hv[3] = h0;
      } else {
        const int w0 = (int)(q0 - (int64_t)h0 * a.W);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const bool in = q0 + k < end;
          pv[k] = in ? p[q0 + k] : 0.f;
          tv[k] = in ? t[q0 + k] : 0.f;
          hv[k] = in ? h0 + (w0 + k) / a.W : 0;       // cells past the end: e = 0, d = 0, every term +0
        }
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (!VEC && !(q0 + k < end)) continue;
        if (with_loss) {
          const float l = loss_term(pv[k] - tv[k], a.kind, a.delta);
          s0 += l;
          if (a.wl != nullptr) s1 += a.wl[hv[k]] * l;
        }
        if (cls != 0) {
          float d;
          if (cls == NORM_ZSCORE) d = (tv[k] - pv[k]) * std_r;
          else if (cls == NORM_HUMIDITY) d = denorm_humidity(tv[k], lmin, lspan, qmax, NORM_HUMIDITY_EPS) -
                                            denorm_humidity(pv[k], lmin, lspan, qmax, NORM_HUMIDITY_EPS);
          else d = denorm_precip(tv[k]) - denorm_precip(pv[k]);
          s2 += (d * d) * a.lat_w[hv[k]];
        }
      }
    }
  }
  const float s[3] = {wave_sum(s0), wave_sum(s1), wave_sum(s2)};
  block_fold4(s, [&](int i, float v) { a.partial[((int64_t)i * a.C + c) * a.nb + j] = v; });
}

// one workgroup of 16 waves; wave w owns channels w, w + 16, ..: its lanes sum the channel's nb partials in double
// (lane-strided, then the shuffle tree), lane 0 writes the channel's entries; the loss is the sum of the waves' own
// channel sums, taken in wave order.  Reports: wave w owns reports w, w + 16, .. and sums the s2 partials of chan(r)
// the same way (a channel reported twice is summed twice, to the same bits).
constexpr int FIN_THREADS = 1024, FIN_WAVES = FIN_THREADS / 64;

__global__ void __launch_bounds__(FIN_THREADS)
val_score_finish_kernel(const float* __restrict__ partial, const float* __restrict__ wf, const int* __restrict__ rchan,
                        float* __restrict__ out, int C, int nb, int R, int use_s1, int kind, double inv_n) {
  __shared__ double wsum[FIN_WAVES];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const float* p0 = partial;
  const float* p1 = partial + (int64_t)C * nb;
  const float* p2 = partial + 2 * (int64_t)C * nb;
  double mine = 0.0;
  for (int c = wave; c < C; c += FIN_WAVES) {
    double a0 = 0.0, a1 = 0.0;
    if (kind != KIND_NONE) {
      for (int i = lane; i < nb; i += 64) {
        a0 += (double)p0[(int64_t)c * nb + i];
        if (use_s1) a1 += (double)p1[(int64_t)c * nb + i];
      }
      a0 = wave_sum_f64(a0);
      a1 = use_s1 ? wave_sum_f64(a1) : a0;
    }
    const double weighted = (double)wf[c] * a1 * inv_n;
    mine += weighted;
    if (lane == 0) {
      out[1 + c] = (float)weighted;
      out[1 + C + c] = (float)(a0 * inv_n);
    }
  }
  if (lane == 0) wsum[wave] = mine;
  __syncthreads();
  if (threadIdx.x == 0) {
    double tot = 0.0;
    for (int w = 0; w < FIN_WAVES; ++w) tot += wsum[w];
    out[0] = (float)(tot / (double)C);
  }
  for (int r = wave; r < R; r += FIN_WAVES) {
    const int c = rchan[r];
    double a2 = 0.0;
    for (int i = lane; i < nb; i += 64) a2 += (double)p2[(int64_t)c * nb + i];
    a2 = wave_sum_f64(a2);
    if (lane == 0) out[1 + 2 * C + r] = (float)sqrt(a2 * inv_n);
  }
}

inline int64_t score_pieces(int H, int W) { return ceil_div64((int64_t)H * W, PLANE_PIECE); }

}  // namespace

extern "C" size_t paradis_val_score_ws_bytes(int B, int C, int H, int W) {
  if (B < 1 || C < 1 || H < 1 || W < 1) return 0;
  return (size_t)3 * (size_t)C * (size_t)B * (size_t)score_pieces(H, W) * sizeof(float);
}

extern "C" int paradis_val_score(const float* pred, int64_t pred_bs, const float* target, int64_t target_bs,
                                 const float* wf, const float* wl, const float* lat_w, int kind, float delta,
                                 const int* rep_chan_host, const int* rep_class_host, int R, const int* rflag,
                                 const int* rcls, const float* rp0, const float* rp1, const int* rchan, float* out,
                                 void* workspace, int B, int C, int H, int W, void* stream) {
  PD_REQUIRE(B >= 0 && C >= 1 && H >= 1 && W >= 1 && R >= 0, "val_score: bad shape B=%d C=%d H=%d W=%d R=%d", B, C, H, W, R);
  PD_REQUIRE(kind == 0 || kind == 1 || kind == KIND_NONE,
             "val_score: kind must be 0 (mse), 1 (reversed_huber) or 2 (none), got %d", kind);
  PD_REQUIRE(R == 0 || (rep_chan_host != nullptr && rep_class_host != nullptr), "val_score: report lists missing");
  for (int r = 0; r < R; ++r) {
    PD_REQUIRE(rep_chan_host[r] >= 0 && rep_chan_host[r] < C, "val_score: report %d names channel %d of %d", r,
               rep_chan_host[r], C);
    PD_REQUIRE(rep_class_host[r] >= NORM_ZSCORE && rep_class_host[r] <= NORM_PRECIP,
               "val_score: report %d has unknown normalisation class %d", r, rep_class_host[r]);
  }
  PD_REQUIRE(R == 0 || lat_w != nullptr, "val_score: reports need the latitude weight table");
  PD_REQUIRE(R == 0 || (rflag && rcls && rp0 && rp1 && rchan), "val_score: device report tables missing");
  const int64_t P = (int64_t)H * W;
  PD_REQUIRE(P < (1ll << 31), "val_score: a plane of %d x %d cells is too large", H, W);
  PD_REQUIRE(pred_bs >= P * C && target_bs >= P * C, "val_score: batch strides shorter than one state");
  if (B == 0) return 0;
  const int64_t npieces = score_pieces(H, W), nb = (int64_t)B * npieces;
  PD_REQUIRE(nb * C < (1ll << 31), "val_score: %lld workgroups exceed the grid", (long long)(nb * C));
  PD_REQUIRE(pred && target && wf && out && workspace, "val_score: null pointer");
  ScoreArgs a;
  a.pred = pred; a.target = target; a.wl = wl; a.lat_w = lat_w;
  a.rflag = R > 0 ? rflag : nullptr;
  a.rcls = rcls; a.rp0 = rp0; a.rp1 = rp1;
  a.partial = static_cast<float*>(workspace);
  a.pred_bs = pred_bs; a.target_bs = target_bs; a.P = P;
  a.C = C; a.W = W; a.npieces = (int)npieces; a.nb = (int)nb; a.kind = kind; a.delta = delta;
  const bool vec = (W % 4 == 0) && aligned16(pred) && aligned16(target) && (pred_bs % 4 == 0) && (target_bs % 4 == 0);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)(nb * C));
  if (vec) hipLaunchKernelGGL(val_score_kernel<true>, grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL(val_score_kernel<false>, grid, dim3(256), 0, st, a);
  hipLaunchKernelGGL(val_score_finish_kernel, dim3(1), dim3(FIN_THREADS), 0, st, a.partial, wf, rchan, out, C, (int)nb,
                     R, wl != nullptr ? 1 : 0, kind, 1.0 / ((double)B * (double)P));
  PD_CHECK_LAUNCH("val_score");
  return 0;
}
