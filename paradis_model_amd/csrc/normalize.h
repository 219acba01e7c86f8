// The feature normalisation classes (reference utils/normalization.py:6-80 as data/era5_dataset.py:463-584 applies them)
// and their inverses, written once for feed.hip (batch assembly, paradis_normalize_features), post.hip (forecast
// post-processing) and score.hip (report RMSE).  The codes are those of feed.py (KIND_*), the per-channel tables of
// paradis_plane_t, PostSpec and ReportSpec.
//
// fp32 in the reference's operation order; every including unit is compiled with -ffp-contract=off, so the three give
// the same bits.  The forward direction has one user and stays there (feed.hip::normalize_value).
#pragma once

constexpr int NORM_NONE = 0, NORM_ZSCORE = 1, NORM_HUMIDITY = 2, NORM_PRECIP = 3;

// precipitation: y = log(x + NORM_PRECIP_EPS) + NORM_PRECIP_SHIFT
constexpr float NORM_PRECIP_EPS = 1e-6f, NORM_PRECIP_SHIFT = 10.0f;
// the humidity epsilon of the reference's datamodule (data/era5_dataset.py:58), for an entry point that has no eps_q
// argument (paradis_val_score)
constexpr float NORM_HUMIDITY_EPS = 1e-12f;

// x * std + mean
__device__ __forceinline__ float denorm_zscore(float x, float mean, float std) { return x * std + mean; }

// clip(exp(x * (log qmax - log qmin) + log qmin) - eps, 0, qmax); lmin = logf(qmin), lspan = logf(qmax) - logf(qmin)
__device__ __forceinline__ float denorm_humidity(float x, float lmin, float lspan, float qmax, float eps) {
  const float q = expf(x * lspan + lmin) - eps;
  return fminf(fmaxf(q, 0.f), qmax);
}

// max(exp(x - 10) - 1e-6, 0)
__device__ __forceinline__ float denorm_precip(float x) {
  return fmaxf(expf(x - NORM_PRECIP_SHIFT) - NORM_PRECIP_EPS, 0.f);
}
