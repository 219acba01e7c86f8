// f4: the data feed on the device - temporal + top-of-atmosphere-radiation forcings
// (reference data/forcings/time_vars.py:6-40, data/forcings/toa_radiation.py:38-199, assembled as
// data/era5_dataset.py:587-621) and the feature normalisations (utils/normalization.py:6-80 as applied
// by data/era5_dataset.py:547-584).  The reference does this per sample with numpy in dataloader
// workers; here one launch per batch of timestamps.
//
// Arithmetic types follow the reference: solar geometry per instant in float64, the grid part in
// float32 with a float64 weight and float32 accumulation (numpy >= 2 promotion), compiled with
// -ffp-contract=off.  HBM traffic: 4 B per output value (write only); the kernel is bound by the
// 15 cosines per (time, cell).
#include "common.h"
#include "normalize.h"
#include "store_reader.h"

#pragma clang fp contract(off)

namespace {

constexpr int NQ = 15;
constexpr double JULIAN_REF_US = 946728000000000.0;  // 2000-01-01T12:00 in microseconds since 1970
// numpy.polynomial.legendre.leggauss(15)
__constant__ double QNODE[NQ] = {-0x1.f9da27c32e6d0p-1, -0x1.dfe24c4f8b448p-1, -0x1.b248221fffd63p-1, -0x1.72e6e181ab3c4p-1,
                                 -0x1.245676f08f3a4p-1, -0x1.939c69257d6b6p-2, -0x1.9c0ba62ef04b5p-3, 0x0.0p+0,
                                 0x1.9c0ba62ef04b5p-3,  0x1.939c69257d6b6p-2,  0x1.245676f08f3a4p-1,  0x1.72e6e181ab3c4p-1,
                                 0x1.b248221fffd63p-1,  0x1.dfe24c4f8b448p-1,  0x1.f9da27c32e6d0p-1};
__constant__ double QWEIGHT[NQ] = {0x1.f7dc7227a2aa8p-6, 0x1.2038260b5d022p-4, 0x1.b6ec9635f113ap-4, 0x1.1dd73b4963152p-3,
                                   0x1.5484f30a86eccp-3, 0x1.7d41fa76dc25bp-3, 0x1.96633f1fd02c2p-3, 0x1.9ee1575f9c972p-3,
                                   0x1.96633f1fd02c2p-3, 0x1.7d41fa76dc25bp-3, 0x1.5484f30a86eccp-3, 0x1.1dd73b4963152p-3,
                                   0x1.b6ec9635f113ap-4, 0x1.2038260b5d022p-4, 0x1.f7dc7227a2aa8p-6};

// numpy.mod for a positive divisor
__device__ __forceinline__ double pymod(double x, double d) {
  double r = fmod(x, d);
  if (r != 0.0 && r < 0.0) r += d;
  return r;
}

__device__ __forceinline__ int64_t floor_div(int64_t a, int64_t b) {
  int64_t q = a / b;
  if ((a % b != 0) && ((a < 0) != (b < 0))) --q;
  return q;
}

// days since 1970-01-01 of January 1st of the civil year containing day z (proleptic Gregorian)
__device__ int64_t year_start_days(int64_t z) {
  z += 719468;
  const int64_t era = floor_div(z, 146097);
  const int64_t doe = z - era * 146097;
  const int64_t yoe = (doe - doe / 1460 + doe / 36524 - doe / 146096) / 365;
  int64_t y = yoe + era * 400;
  const int64_t doy = doe - (365 * yoe + yoe / 4 - yoe / 100);
  const int64_t mp = (5 * doy + 2) / 153;
  const int64_t m = mp < 10 ? mp + 3 : mp - 9;
  if (m <= 2) ++y;
  // days_from_civil(y, 1, 1)
  const int64_t yy = y - 1;   // January: year shifted by one in the March-based calendar
  const int64_t era2 = floor_div(yy, 400);
  const int64_t yoe2 = yy - era2 * 400;
  const int64_t doy2 = (153 * (1 + 9) + 2) / 5;   // Jan 1 -> month index 10 in the March-based year
  const int64_t doe2 = yoe2 * 365 + yoe2 / 4 - yoe2 / 100 + doy2;
  return era2 * 146097 + doe2 - 719468;
}

// per-instant scalars.  thread (t, q): q < 15 quadrature node of the hour ending at times[t];
// q == 15: the four temporal forcings of times[t].
//   sc_f[(t*15+q)*3 + {0,1,2}] = sin(decl), cos(decl), mod_day (float32);  sc_w[t*15+q] = weight (float64)
//   tf[t*4 + {0..3}] = sin/cos time of day, sin/cos year progress
__global__ void forcing_scalars_kernel(const int64_t* __restrict__ times_us, int T, float* __restrict__ tf,
                                       float* __restrict__ sc_f, double* __restrict__ sc_w) {
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  const int t = gid >> 4, q = gid & 15;
  if (t >= T) return;
  const int64_t us = times_us[t];
  if (q == NQ) {
    const int64_t hours = floor_div(us, 3600000000ll);          // astype("datetime64[h]")
    const int64_t days = floor_div(hours, 24);
    const double hour_of_day = (double)(hours - days * 24);
    const double tod = hour_of_day / 24.0;
    const double doy = (double)(hours - year_start_days(days) * 24) / 24.0;
    const double yp = doy / 365.25;
    const double two_pi = 2.0 * 3.141592653589793;
    tf[t * 4 + 0] = (float)sin(two_pi * tod);
    tf[t * 4 + 1] = (float)cos(two_pi * tod);
    tf[t * 4 + 2] = (float)sin(two_pi * yp);
    tf[t * 4 + 3] = (float)cos(two_pi * yp);
    return;
  }
  const double pi = 3.141592653589793;
  const double tq = (double)us - 3600e6 * (1.0 + QNODE[q]) / 2.0;
  const double mjd = (tq - JULIAN_REF_US) / 86400e6;
  const double anomaly = pymod(357.529 + 0.98560028 * mjd, 360.0) * pi / 180.0;
  const double mean_lon = pymod(280.459 + 0.98564736 * mjd, 360.0) * pi / 180.0;
  const double app_lon = mean_lon + (1.915 * sin(anomaly) + 0.020 * sin(2.0 * anomaly)) * pi / 180.0;
  const double dist = 1.00014 - 0.01671 * cos(anomaly) - 0.00014 * cos(2.0 * anomaly);
  const double obliq = (23.439 - 0.00000036 * mjd) * pi / 180.0;
  const double asc = atan2(cos(obliq) * sin(app_lon), cos(app_lon));
  const double decl = asin(sin(obliq) * sin(app_lon));
  const double eot = (pymod(mean_lon - asc + pi, 2.0 * pi) - pi) / (2.0 * pi);
  const float mod_day = (float)(pymod(mjd + eot, 1.0) * 2.0 * pi);
  const float decl32 = (float)decl;
  const int o = t * NQ + q;
  sc_f[o * 3 + 0] = sinf(decl32);
  sc_f[o * 3 + 1] = cosf(decl32);
  sc_f[o * 3 + 2] = mod_day;
  sc_w[o] = (1360.56 / (dist * dist)) * (3600.0 * QWEIGHT[q] / 2.0);
}

struct ForcingVars {
  int n;         // number of forcing variables
  int code[8];   // 0 = toa radiation, 1..4 = sin/cos time of day, sin/cos year progress
};

// thread (b, t, y, x): TOA radiation of one cell at one time of series b, scattered (with the temporal
// forcings of that time) to every window (s, k) with s + k = t:  out[b, s, y, x, v*n + k]
__global__ void __launch_bounds__(256)
forcings_kernel(const double* __restrict__ lat_deg, const double* __restrict__ lon_deg, int lat_f32, int B,
                int T, int H, int W, int n, ForcingVars fv, float toa_mean, float toa_std,
                const float* __restrict__ tf, const float* __restrict__ sc_f, const double* __restrict__ sc_w,
                float* __restrict__ out) {
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t P = (int64_t)H * W;
  if (gid >= (int64_t)B * T * P) return;
  const int t = (int)(gid / P);            // flat (series, time) index
  const int64_t cell = gid - (int64_t)t * P;
  const int b = t / T, tl = t - b * T;     // windows never straddle two series
  const int y = (int)(cell / W), x = (int)(cell - (int64_t)y * W);
  bool need_toa = false;
  for (int v = 0; v < fv.n; ++v) need_toa |= fv.code[v] == 0;
  float toa = 0.f;
  if (need_toa) {
    // toa_radiation.py:135-136: lat*pi/180 in the latitude array's own dtype, then float32
    float lat_rad;
    if (lat_f32) lat_rad = ((float)lat_deg[y] * 3.14159274f) / 180.0f;
    else lat_rad = (float)(lat_deg[y] * 3.141592653589793 / 180.0);
    const float lon32 = (float)lon_deg[x];
    const float slat = sinf(lat_rad), clat = cosf(lat_rad);
    const float lon_rad = (lon32 * 3.14159274f) / 180.0f;
    float acc = 0.f;
    for (int q = 0; q < NQ; ++q) {
      const int o = t * NQ + q;
      const float sdec = sc_f[o * 3], cdec = sc_f[o * 3 + 1], mod_day = sc_f[o * 3 + 2];
      const float clst = cosf(lon_rad + mod_day);
      const float cz = fmaxf(0.f, slat * sdec + clat * cdec * clst);
      acc = (float)((double)acc + (double)cz * sc_w[o]);
    }
    toa = (acc - toa_mean) / toa_std;
  }
  const int steps = T - n + 1, C = fv.n * n;
  for (int k = 0; k < n; ++k) {
    const int s = tl - k;
    if (s < 0 || s >= steps) continue;
    float* o = out + (((int64_t)b * steps + s) * P + cell) * C;
    for (int v = 0; v < fv.n; ++v) o[v * n + k] = fv.code[v] == 0 ? toa : tf[t * 4 + fv.code[v] - 1];
  }
}

// one value through one feature normalisation (reference utils/normalization.py:6-80): k in {0 none, 1 z-score (a mean,
// b std), 2 humidity (a q_min, b q_max), 3 precipitation}.  The ONE expression of the unit: normalize_kernel and
// assemble_batch_kernel both call it, so a plane assembled by the second equals the first applied to a gathered copy.
__device__ __forceinline__ float normalize_value(float x, int k, float a, float b, float eps_q, int inverse) {
  float r = x;
  if (k == NORM_ZSCORE) {
    r = inverse ? denorm_zscore(x, a, b) : (x - a) / b;
  } else if (k == NORM_HUMIDITY) {
    const float lmin = logf(a), lmax = logf(b);
    if (!inverse) {
      r = (logf(fminf(fmaxf(x, 0.f), b) + eps_q) - lmin) / (lmax - lmin);
    } else {
      r = denorm_humidity(x, lmin, lmax - lmin, b, eps_q);
    }
  } else if (k == NORM_PRECIP) {
    r = inverse ? denorm_precip(x) : logf(x + NORM_PRECIP_EPS) + NORM_PRECIP_SHIFT;
  }
  return r;
}

// channels-last feature (de)normalisation, in place: data[i, c], kind[c] in {0 none, 1 z-score (p0 mean,
// p1 std), 2 humidity (p0 q_min, p1 q_max), 3 precipitation}
__global__ void __launch_bounds__(256)
normalize_kernel(float* __restrict__ data, const int* __restrict__ kind, const float* __restrict__ p0,
                 const float* __restrict__ p1, int64_t n, int C, float eps_q, int inverse) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int c = (int)(i % C);
  const int k = kind[c];
  if (k == NORM_NONE) return;
  data[i] = normalize_value(data[i], k, p0[c], p1[c], eps_q, inverse);
}

// Packing (the store format, its constants, the ONE decode and the element readers: store_reader.h).
__device__ __forceinline__ float pack_domain_value(float x, int domain) {
  return domain == 1 ? (float)log((double)(x + PACK_LOG_EPS)) : x;
}

// the code of one packed-domain value; s == 0: a constant plane
__device__ __forceinline__ uint32_t pack_code(float y, float lo, float s) {
  if (!isfinite(y)) return PACK_MISSING;
  const float c = s == 0.f ? 0.f : rintf((y - lo) / s);
  return (uint32_t)fminf(fmaxf(c, 0.f), PACK_TOP);
}

// Batch assembly from a device-resident channels-first store [T, F, P] (P = H*W): one workgroup copies one chunk of
// AB_CHUNK = AB_THREADS * 4 * AB_UNROLL values of ONE output plane through that plane's normalisation, so the table
// entry, the sample's time row and both plane addresses are wave-uniform (scalar loads, no divergence in the kind
// switch).  Planes [0, n_in) of a sample are the input's channels, [n_in, n_in + n_out) the target's (step-major).
// 8 B of HBM traffic per value from a float32 store, 6 B from a packed one (whose plane's lo / s / domain are
// wave-uniform too).  Rows and features outside the store are CLAMPED (never read outside) and reported
// through *flag; a negative or enormous idx[b] is limited first so that base + idx * interval cannot wrap.
constexpr int AB_THREADS = 256, AB_UNROLL = 2, AB_CHUNK = AB_THREADS * 4 * AB_UNROLL;

// values [lo, hi) of one plane through normalisation k (0: none).  vec: lo, hi and both plane bases are multiples of
// four values, the destination 16-byte and the source Quad aligned.
template <class Reader>
__device__ __forceinline__ void copy_plane_chunk(const typename Reader::Plane& pl, float* __restrict__ dst, int64_t lo,
                                                 int64_t hi, int k, float a, float c, float eps_q, int vec) {
  if (vec) {
    typename Reader::Quad q[AB_UNROLL];
#pragma unroll
    for (int u = 0; u < AB_UNROLL; ++u) {
      const int64_t i = lo + (int64_t)(u * AB_THREADS + threadIdx.x) * 4;
      if (i < hi) q[u] = Reader::load_quad(pl, i);
    }
#pragma unroll
    for (int u = 0; u < AB_UNROLL; ++u) {
      const int64_t i = lo + (int64_t)(u * AB_THREADS + threadIdx.x) * 4;
      if (i < hi) {
        const float4 v = Reader::quad_values(pl, q[u]);
        float4 o;
        o.x = normalize_value(v.x, k, a, c, eps_q, 0);
        o.y = normalize_value(v.y, k, a, c, eps_q, 0);
        o.z = normalize_value(v.z, k, a, c, eps_q, 0);
        o.w = normalize_value(v.w, k, a, c, eps_q, 0);
        *reinterpret_cast<float4*>(dst + i) = o;
      }
    }
  } else {
    for (int64_t i = lo + threadIdx.x; i < hi; i += AB_THREADS)
      dst[i] = normalize_value(Reader::value(pl, i), k, a, c, eps_q, 0);
  }
}

template <class Reader>
__global__ void __launch_bounds__(AB_THREADS)
assemble_batch_kernel(const Reader store, int64_t T, int F, int64_t P, const int64_t* __restrict__ idx,
                      int64_t base, int64_t interval, const paradis_plane_t* __restrict__ planes, int n_in, int n_out,
                      int chunks, float* __restrict__ input, float* __restrict__ target, float eps_q,
                      int* __restrict__ flag, int vec) {
  const uint32_t blk = blockIdx.x, r = blk / (uint32_t)chunks;     // the grid is below 2^31: 32-bit divisions
  const int chunk = (int)(blk - r * (uint32_t)chunks);
  const uint32_t np = (uint32_t)(n_in + n_out);
  const int64_t b = r / np;
  const int plane = (int)(r - (uint32_t)b * np);
  const paradis_plane_t e = planes[plane];
  constexpr int64_t IDX_LIMIT = 1ll << 40;
  const int64_t i_raw = idx[b];
  const int64_t i_ok = i_raw < -IDX_LIMIT ? -IDX_LIMIT : (i_raw > IDX_LIMIT ? IDX_LIMIT : i_raw);
  const int64_t row_raw = base + i_ok * interval + e.dt;
  const int64_t row = row_raw < 0 ? 0 : (row_raw >= T ? T - 1 : row_raw);
  const int f = e.feature < 0 ? 0 : (e.feature >= F ? F - 1 : e.feature);
  if ((row != row_raw || f != e.feature) && threadIdx.x == 0) *flag = 1;
  const typename Reader::Plane src = store.plane(row * F + f, f, P);
  float* __restrict__ dst = plane < n_in ? input + (b * n_in + plane) * P : target + (b * n_out + (plane - n_in)) * P;
  const int64_t lo = (int64_t)chunk * AB_CHUNK;
  const int64_t hi = lo + AB_CHUNK < P ? lo + AB_CHUNK : P;
  copy_plane_chunk<Reader>(src, dst, lo, hi, e.kind, e.p0, e.p1, eps_q, vec);
}

// rows [a, b) of a packed store as float32: workgroup (plane, chunk) decodes one chunk of one plane
__global__ void __launch_bounds__(AB_THREADS)
unpack_planes_kernel(const PackedPlanes store, int F, int64_t P, int64_t first_plane, int chunks,
                     float* __restrict__ out, int vec) {
  const uint32_t blk = blockIdx.x, r = blk / (uint32_t)chunks;
  const int chunk = (int)(blk - r * (uint32_t)chunks);
  const int64_t index = first_plane + r;
  const PackedPlanes::Plane src = store.plane(index, (int)(index % F), P);
  const int64_t lo = (int64_t)chunk * AB_CHUNK;
  const int64_t hi = lo + AB_CHUNK < P ? lo + AB_CHUNK : P;
  copy_plane_chunk<PackedPlanes>(src, out + (int64_t)r * P, lo, hi, 0, 0.f, 0.f, 0.f, vec);
}

// Packing.  Workgroup (plane, piece) owns PACK_PIECE cells of one plane of the slab.  Pass 1 writes the minimum and the
// maximum of the piece's finite packed-domain values to ws[(plane * pieces + piece) * 2]; pass 2 folds the plane's
// partials again (every workgroup of the plane, the same values: a minimum does not depend on the order, and no
// atomics take part), writes the plane's (lo, s) once and the codes of its piece.  8 + 2 B of HBM traffic per value.
constexpr int PACK_THREADS = 256, PACK_PIECE = 8192;

// minimum and maximum over the workgroup, in every thread
__device__ __forceinline__ void block_min_max(float& mn, float& mx) {
  __shared__ float red[2][PACK_THREADS / WAVE];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    mn = fminf(mn, __shfl_xor(mn, o, 64));
    mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  }
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = mn;
    red[1][threadIdx.x >> 6] = mx;
  }
  __syncthreads();
  mn = fminf(fminf(red[0][0], red[0][1]), fminf(red[0][2], red[0][3]));
  mx = fmaxf(fmaxf(red[1][0], red[1][1]), fmaxf(red[1][2], red[1][3]));
}

template <bool VEC>
__global__ void __launch_bounds__(PACK_THREADS)
pack_min_max_kernel(const float* __restrict__ slab, int F, int64_t P, const int* __restrict__ domain, int pieces,
                    float* __restrict__ ws) {
  const uint32_t blk = blockIdx.x, plane = blk / (uint32_t)pieces;
  const int piece = (int)(blk - plane * (uint32_t)pieces);
  const int dom = domain[plane % (uint32_t)F];
  const float* __restrict__ x = slab + (int64_t)plane * P;
  const int64_t lo = (int64_t)piece * PACK_PIECE;
  const int64_t hi = lo + PACK_PIECE < P ? lo + PACK_PIECE : P;
  float mn = INFINITY, mx = -INFINITY;
  if (VEC) {      // P % 4 == 0 and a 16-byte aligned slab: every quad below hi is whole
    for (int64_t i = lo + 4 * (int64_t)threadIdx.x; i < hi; i += 4 * PACK_THREADS) {
      const float4 q = *reinterpret_cast<const float4*>(x + i);
      const float v[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float y = pack_domain_value(v[k], dom);
        if (isfinite(y)) mn = fminf(mn, y), mx = fmaxf(mx, y);
      }
    }
  } else {
    for (int64_t i = lo + threadIdx.x; i < hi; i += PACK_THREADS) {
      const float y = pack_domain_value(x[i], dom);
      if (isfinite(y)) mn = fminf(mn, y), mx = fmaxf(mx, y);
    }
  }
  block_min_max(mn, mx);
  if (threadIdx.x == 0) {
    ws[2 * (int64_t)blk] = mn;
    ws[2 * (int64_t)blk + 1] = mx;
  }
}

template <bool VEC>
__global__ void __launch_bounds__(PACK_THREADS)
pack_quantize_kernel(const float* __restrict__ slab, int F, int64_t P, const int* __restrict__ domain, int pieces,
                     const float* __restrict__ ws, uint16_t* __restrict__ codes, float* __restrict__ params) {
  const uint32_t blk = blockIdx.x, plane = blk / (uint32_t)pieces;
  const int piece = (int)(blk - plane * (uint32_t)pieces);
  const int dom = domain[plane % (uint32_t)F];
  float mn = INFINITY, mx = -INFINITY;
  for (int j = threadIdx.x; j < pieces; j += PACK_THREADS) {
    mn = fminf(mn, ws[2 * ((int64_t)plane * pieces + j)]);
    mx = fmaxf(mx, ws[2 * ((int64_t)plane * pieces + j) + 1]);
  }
  block_min_max(mn, mx);
  // no finite value: lo = s = 0, every code missing.  lo == 0 is stored as +0 whichever zero the minimum met.
  float lo_y = 0.f, s = 0.f;
  if (mn <= mx) {
    lo_y = mn == 0.f ? 0.f : mn;
    s = (mx - mn) / PACK_TOP;
  }
  if (piece == 0 && threadIdx.x == 0) {
    params[2 * (int64_t)plane] = lo_y;
    params[2 * (int64_t)plane + 1] = s;
  }
  const float* __restrict__ x = slab + (int64_t)plane * P;
  uint16_t* __restrict__ out = codes + (int64_t)plane * P;
  const int64_t lo = (int64_t)piece * PACK_PIECE;
  const int64_t hi = lo + PACK_PIECE < P ? lo + PACK_PIECE : P;
  if (VEC) {      // as above, and 8-byte aligned codes
    for (int64_t i = lo + 4 * (int64_t)threadIdx.x; i < hi; i += 4 * PACK_THREADS) {
      const float4 q = *reinterpret_cast<const float4*>(x + i);
      uint2 o;
      o.x = pack_code(pack_domain_value(q.x, dom), lo_y, s) | (pack_code(pack_domain_value(q.y, dom), lo_y, s) << 16);
      o.y = pack_code(pack_domain_value(q.z, dom), lo_y, s) | (pack_code(pack_domain_value(q.w, dom), lo_y, s) << 16);
      *reinterpret_cast<uint2*>(out + i) = o;
    }
  } else {
    for (int64_t i = lo + threadIdx.x; i < hi; i += PACK_THREADS)
      out[i] = (uint16_t)pack_code(pack_domain_value(x[i], dom), lo_y, s);
  }
}

// the argument checks and the launch of both assembly entry points
template <class Reader>
int assemble_batch_launch(const char* name, const Reader& store, bool store_ok, bool store_vec, int64_t T, int F, int H,
                          int W, const int64_t* idx, int B, int64_t base, int64_t interval_steps,
                          const paradis_plane_t* planes, int n_time_inputs, int Fin, int S, int Fout, float* input,
                          float* target, float eps_q, int* flag, void* stream) {
  PD_REQUIRE(T >= 1 && F >= 1 && H >= 1 && W >= 1 && B >= 0, "%s: bad shape T=%lld F=%d H=%d W=%d B=%d", name,
             (long long)T, F, H, W, B);
  PD_REQUIRE(n_time_inputs >= 1, "%s: n_time_inputs=%d must be >= 1", name, n_time_inputs);
  PD_REQUIRE(S >= 0, "%s: forecast steps S=%d must be >= 0", name, S);
  PD_REQUIRE(Fin >= 1 && Fout >= 0, "%s: bad feature counts Fin=%d Fout=%d", name, Fin, Fout);
  PD_REQUIRE(interval_steps >= 1, "%s: interval_steps=%lld must be >= 1", name, (long long)interval_steps);
  PD_REQUIRE((int64_t)n_time_inputs * Fin < (1 << 24) && (int64_t)S * Fout < (1 << 24),
             "%s: too many planes per sample", name);
  PD_REQUIRE(planes != nullptr, "%s: plane table required", name);
  if (B == 0) return 0;
  PD_REQUIRE(store_ok && idx != nullptr && input != nullptr && flag != nullptr,
             "%s: store, idx, input and flag pointers required", name);
  const int n_in = n_time_inputs * Fin;
  const int n_out = target != nullptr ? S * Fout : 0;     // no target: the prediction-stage item
  const int64_t P = (int64_t)H * W;
  const int64_t chunks = ceil_div64(P, AB_CHUNK);
  PD_REQUIRE(chunks < (1ll << 31), "%s: grid too large", name);
  const int64_t blocks = (int64_t)B * (n_in + n_out) * chunks;
  PD_REQUIRE(blocks < (1ll << 31), "%s: too large (%lld workgroups)", name, (long long)blocks);
  const int vec = P % 4 == 0 && store_vec && aligned16(input) && (target == nullptr || aligned16(target));
  hipLaunchKernelGGL(assemble_batch_kernel<Reader>, dim3((unsigned)blocks), dim3(AB_THREADS), 0, (hipStream_t)stream,
                     store, T, F, P, idx, base, interval_steps, planes, n_in, n_out, (int)chunks, input, target, eps_q,
                     flag, vec);
  PD_CHECK_LAUNCH(name);
  return 0;
}

}  // namespace

extern "C" size_t paradis_forcings_ws_bytes(int B, int T) {
  // per timestamp: [15] double weights, [15*3] float scalars, [4] float temporal forcings
  const size_t n = (size_t)(B < 0 ? 0 : B) * (size_t)(T < 0 ? 0 : T);
  return n * 15 * sizeof(double) + n * (15 * 3 + 4) * sizeof(float) + 256;
}

extern "C" int paradis_forcings(const int64_t* times_us, const double* lat_deg, const double* lon_deg,
                                int lat_is_f32, int B, int T, int H, int W, int n_time_inputs,
                                const int* var_codes, int n_vars, double toa_mean, double toa_std,
                                float* out, void* workspace, void* stream) {
  PD_REQUIRE(B >= 0 && T >= 1 && H >= 1 && W >= 1 && n_time_inputs >= 1 && n_time_inputs <= T,
             "forcings: bad shape B=%d T=%d H=%d W=%d n_time_inputs=%d", B, T, H, W, n_time_inputs);
  PD_REQUIRE((int64_t)B * T < (1 << 26), "forcings: too many timestamps");
  PD_REQUIRE(n_vars >= 1 && n_vars <= 8 && var_codes != nullptr, "forcings: 1..8 forcing variables");
  PD_REQUIRE(workspace != nullptr, "forcings: workspace required");
  ForcingVars fv{};
  fv.n = n_vars;
  for (int v = 0; v < n_vars; ++v) {
    PD_REQUIRE(var_codes[v] >= 0 && var_codes[v] <= 4, "forcings: unknown variable code %d", var_codes[v]);
    fv.code[v] = var_codes[v];
  }
  if (B == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  const int TT = B * T;
  double* sc_w = (double*)workspace;
  float* sc_f = (float*)(sc_w + (size_t)TT * 15);
  float* tf = sc_f + (size_t)TT * 15 * 3;
  hipLaunchKernelGGL(forcing_scalars_kernel, dim3((TT * 16 + 63) / 64), dim3(64), 0, st, times_us, TT, tf, sc_f, sc_w);
  const int64_t total = (int64_t)TT * H * W;
  PD_REQUIRE((total + 255) / 256 < (1ll << 31), "forcings: too large");
  hipLaunchKernelGGL(forcings_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, lat_deg, lon_deg,
                     lat_is_f32, B, T, H, W, n_time_inputs, fv, (float)toa_mean, (float)toa_std, (const float*)tf,
                     (const float*)sc_f, (const double*)sc_w, out);
  PD_CHECK_LAUNCH("forcings");
  return 0;
}

extern "C" int paradis_normalize_features(float* data, const int* kind, const float* p0, const float* p1,
                                          int64_t rows, int C, float eps_q, int inverse, void* stream) {
  PD_REQUIRE(rows >= 0 && C >= 1, "normalize_features: bad shape");
  if (rows == 0) return 0;
  const int64_t n = rows * C;
  PD_REQUIRE((n + 255) / 256 < (1ll << 31), "normalize_features: too large");
  hipLaunchKernelGGL(normalize_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, data,
                     kind, p0, p1, n, C, eps_q, inverse);
  PD_CHECK_LAUNCH("normalize_features");
  return 0;
}

extern "C" int paradis_assemble_batch_chunk(void) { return AB_CHUNK; }

extern "C" int paradis_assemble_batch(const float* store, int64_t T, int F, int H, int W, const int64_t* idx, int B,
                                      int64_t base, int64_t interval_steps, const paradis_plane_t* planes,
                                      int n_time_inputs, int Fin, int S, int Fout, float* input, float* target,
                                      float eps_q, int* flag, void* stream) {
  return assemble_batch_launch("assemble_batch", FloatPlanes{store}, store != nullptr, aligned16(store), T, F, H, W, idx,
                               B, base, interval_steps, planes, n_time_inputs, Fin, S, Fout, input, target, eps_q, flag,
                               stream);
}

extern "C" int paradis_assemble_batch_packed(const uint16_t* codes, const float* params, const int* domain, int64_t T,
                                             int F, int H, int W, const int64_t* idx, int B, int64_t base,
                                             int64_t interval_steps, const paradis_plane_t* planes, int n_time_inputs,
                                             int Fin, int S, int Fout, float* input, float* target, float eps_q,
                                             int* flag, void* stream) {
  return assemble_batch_launch("assemble_batch_packed", PackedPlanes{codes, params, domain},
                               codes != nullptr && params != nullptr && domain != nullptr, aligned8(codes), T, F, H, W,
                               idx, B, base, interval_steps, planes, n_time_inputs, Fin, S, Fout, input, target, eps_q,
                               flag, stream);
}

extern "C" int paradis_pack_planes_piece(void) { return PACK_PIECE; }

extern "C" size_t paradis_pack_planes_ws_bytes(int n, int F, int H, int W) {
  if (n < 1 || F < 1 || H < 1 || W < 1) return 0;
  return (size_t)n * (size_t)F * (size_t)ceil_div64((int64_t)H * W, PACK_PIECE) * 2 * sizeof(float);
}

extern "C" int paradis_pack_planes(const float* slab, int n, int F, int H, int W, const int* domain, int64_t row0,
                                   int64_t T, uint16_t* codes, float* params, void* ws, void* stream) {
  PD_REQUIRE(n >= 0 && F >= 1 && H >= 1 && W >= 1, "pack_planes: bad shape n=%d F=%d H=%d W=%d", n, F, H, W);
  PD_REQUIRE(row0 >= 0 && T >= 1 && row0 <= T && (int64_t)n <= T - row0,
             "pack_planes: rows [%lld, %lld) outside a store of %lld", (long long)row0, (long long)row0 + n,
             (long long)T);
  if (n == 0) return 0;
  PD_REQUIRE(slab != nullptr && domain != nullptr && codes != nullptr && params != nullptr && ws != nullptr,
             "pack_planes: slab, domain, codes, params and workspace pointers required");
  const int64_t P = (int64_t)H * W;
  const int64_t pieces = ceil_div64(P, PACK_PIECE);
  const int64_t blocks = (int64_t)n * F * pieces;
  PD_REQUIRE(pieces < (1ll << 31) && blocks < (1ll << 31), "pack_planes: too large (%lld workgroups)",
             (long long)blocks);
  uint16_t* out = codes + row0 * F * P;
  float* par = params + row0 * F * 2;
  hipStream_t st = (hipStream_t)stream;
  const bool vec = P % 4 == 0 && aligned16(slab);
  const dim3 grid((unsigned)blocks), block(PACK_THREADS);
  if (vec) hipLaunchKernelGGL(pack_min_max_kernel<true>, grid, block, 0, st, slab, F, P, domain, (int)pieces, (float*)ws);
  else hipLaunchKernelGGL(pack_min_max_kernel<false>, grid, block, 0, st, slab, F, P, domain, (int)pieces, (float*)ws);
  if (vec && aligned8(out))
    hipLaunchKernelGGL(pack_quantize_kernel<true>, grid, block, 0, st, slab, F, P, domain, (int)pieces,
                       (const float*)ws, out, par);
  else
    hipLaunchKernelGGL(pack_quantize_kernel<false>, grid, block, 0, st, slab, F, P, domain, (int)pieces,
                       (const float*)ws, out, par);
  PD_CHECK_LAUNCH("pack_planes");
  return 0;
}

extern "C" int paradis_unpack_planes(const uint16_t* codes, const float* params, const int* domain, int64_t T, int F,
                                     int H, int W, int64_t a, int64_t b, float* out, void* stream) {
  PD_REQUIRE(T >= 1 && F >= 1 && H >= 1 && W >= 1, "unpack_planes: bad shape T=%lld F=%d H=%d W=%d", (long long)T, F, H,
             W);
  PD_REQUIRE(a >= 0 && a <= b && b <= T, "unpack_planes: rows [%lld, %lld) outside a store of %lld", (long long)a,
             (long long)b, (long long)T);
  if (a == b) return 0;
  PD_REQUIRE(codes != nullptr && params != nullptr && domain != nullptr && out != nullptr,
             "unpack_planes: codes, params, domain and out pointers required");
  const int64_t P = (int64_t)H * W;
  const int64_t chunks = ceil_div64(P, AB_CHUNK);
  const int64_t blocks = (b - a) * F * chunks;
  PD_REQUIRE(chunks < (1ll << 31) && blocks < (1ll << 31), "unpack_planes: too large (%lld workgroups)",
             (long long)blocks);
  const int vec = P % 4 == 0 && aligned8(codes) && aligned16(out);
  hipLaunchKernelGGL(unpack_planes_kernel, dim3((unsigned)blocks), dim3(AB_THREADS), 0, (hipStream_t)stream,
                     PackedPlanes{codes, params, domain}, F, P, a * F, (int)chunks, out, vec);
  PD_CHECK_LAUNCH("unpack_planes");
  return 0;
}
