// The verification climatology of a device-resident store: the slot means clim [K, C, H, W] that verify.hip reads for
// the anomaly correlation and the activity, built from the store's own rows (float32 or 16-bit packed) by CSR lists the
// host plans (climatology.ClimPlan: the project's own windowed day-of-year x hour definition, in the spirit of
// WeatherBench-2's climatology but not pinned against it), and the Cartesian -> spherical winds of the finished means.
//
// Arithmetic: every value is widened to double as it is read; S = sum w x and Wt = sum w are double, in list order, with
// NaN / +-Inf skipped per pixel (skipna, the rule of the store statistics); one division and one rounding to fp32.
// -ffp-contract=off: a packed value is decoded to the bits paradis_unpack_planes gives (store_reader.h), the winds are
// the expression of post.hip (winds.h).
//
// Memory-bound: N*C*P*(4 | 2) B read, K*C*P*4 B written.  No atomics, no zero fill: bit-identical run to run.
#include "common.h"
#include "store_reader.h"
#include "winds.h"

#pragma clang fp contract(off)

namespace {

// One workgroup owns CM_CHUNK = CM_THREADS * 4 values of ONE (slot, channel) plane and walks the slot's list, so the
// list entry, its weight, the plane address and a packed plane's (lo, s, domain) are wave-uniform (scalar loads).  A
// thread keeps four cells' (S, Wt) in registers - 16 VGPRs of double - and CM_ROWS rows' loads in flight in front of the
// dependent adds: at 32x64 there are only K * C * 2 workgroups and a 61-day window's list has ~900 entries, so the
// latency of one load per row would be the whole run time.
constexpr int CM_THREADS = 256, CM_CHUNK = CM_THREADS * 4, CM_ROWS = 8;

__device__ __forceinline__ void clim_add(double& S, double& Wt, float v, double w) {
  if (isfinite(v)) {
    S += w * (double)v;
    Wt += w;
  }
}

// VEC: P % 4 == 0, out 16-byte and the store Quad-aligned - a thread owns the four adjacent cells lo + 4 * tid ..;
// otherwise the four cells lo + tid + {0, 1, 2, 3} * CM_THREADS, scalar loads, the same arithmetic per cell.
template <class Reader, bool VEC>
__global__ void __launch_bounds__(CM_THREADS)
clim_mean_kernel(const Reader store, int64_t T, int F, int64_t P, const int64_t* __restrict__ ptr,
                 const int64_t* __restrict__ rows, const double* __restrict__ wts, int64_t N, int k0,
                 const int* __restrict__ cols, int C, int chunks, float* __restrict__ out, int* __restrict__ flag) {
  const uint32_t blk = blockIdx.x, r = blk / (uint32_t)chunks;     // the grid is below 2^31: 32-bit divisions
  const int chunk = (int)(blk - r * (uint32_t)chunks);
  const uint32_t kk = r / (uint32_t)C;
  const int c = (int)(r - kk * (uint32_t)C);
  const int64_t k = (int64_t)k0 + kk;
  const int f_raw = cols[c];
  const int f = f_raw < 0 ? 0 : (f_raw >= F ? F - 1 : f_raw);
  const int64_t b_raw = ptr[k], e_raw = ptr[k + 1];
  const int64_t jb = b_raw < 0 ? 0 : (b_raw > N ? N : b_raw);
  const int64_t je = e_raw < jb ? jb : (e_raw > N ? N : e_raw);
  bool clamped = f != f_raw || jb != b_raw || je != e_raw;
  const int64_t lo = (int64_t)chunk * CM_CHUNK;
  const int64_t hi = lo + CM_CHUNK < P ? lo + CM_CHUNK : P;
  const int tid = threadIdx.x;
  // cell m of this thread, and whether it lies in the plane (VEC: quads are whole, m = 0 decides)
  int64_t cell[4];
  bool in[4];
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    cell[m] = VEC ? lo + 4 * (int64_t)tid + m : lo + tid + (int64_t)m * CM_THREADS;
    in[m] = cell[m] < hi;
  }
  double S[4] = {0.0, 0.0, 0.0, 0.0}, Wt[4] = {0.0, 0.0, 0.0, 0.0};
  for (int64_t j = jb; j < je; j += CM_ROWS) {
    typename Reader::Plane pl[CM_ROWS];
    typename Reader::Quad q[CM_ROWS];
    float sv[CM_ROWS][4];
    double w[CM_ROWS];
#pragma unroll
    for (int u = 0; u < CM_ROWS; ++u) {
      if (j + u < je) {                                     // wave-uniform
        const int64_t row_raw = rows[j + u];
        const int64_t row = row_raw < 0 ? 0 : (row_raw >= T ? T - 1 : row_raw);
        clamped |= row != row_raw;
        w[u] = wts[j + u];
        pl[u] = store.plane(row * F + f, f, P);
        if (VEC) {
          if (in[0]) q[u] = Reader::load_quad(pl[u], cell[0]);
        } else {
#pragma unroll
          for (int m = 0; m < 4; ++m)
            if (in[m]) sv[u][m] = Reader::value(pl[u], cell[m]);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < CM_ROWS; ++u) {
      if (j + u < je) {
        if (VEC) {
          if (in[0]) {
            const float4 v = Reader::quad_values(pl[u], q[u]);
            clim_add(S[0], Wt[0], v.x, w[u]);
            clim_add(S[1], Wt[1], v.y, w[u]);
            clim_add(S[2], Wt[2], v.z, w[u]);
            clim_add(S[3], Wt[3], v.w, w[u]);
          }
        } else {
#pragma unroll
          for (int m = 0; m < 4; ++m)
            if (in[m]) clim_add(S[m], Wt[m], sv[u][m], w[u]);
        }
      }
    }
  }
  if (clamped && tid == 0) *flag = 1;
  float* __restrict__ dst = out + (k * C + c) * P;
  float o[4];
#pragma unroll
  for (int m = 0; m < 4; ++m) o[m] = Wt[m] == 0.0 ? __builtin_nanf("") : (float)(S[m] / Wt[m]);
  if (VEC) {
    if (in[0]) *reinterpret_cast<float4*>(dst + cell[0]) = make_float4(o[0], o[1], o[2], o[3]);
  } else {
#pragma unroll
    for (int m = 0; m < 4; ++m)
      if (in[m]) dst[cell[m]] = o[m];
  }
}

// the argument checks and the launches of both entry points
template <class Reader>
int clim_mean_launch(const char* name, const Reader& store, bool store_ok, bool store_vec, int64_t T, int F, int H,
                     int W, const int64_t* ptr, const int64_t* rows, const double* w, int64_t N, int K,
                     const int* cols, int C, float* out, int* flag, void* stream) {
  PD_REQUIRE(T >= 1 && F >= 1 && H >= 1 && W >= 1 && K >= 0 && C >= 0, "%s: bad shape T=%lld F=%d H=%d W=%d K=%d C=%d",
             name, (long long)T, F, H, W, K, C);
  PD_REQUIRE(N >= 0, "%s: N=%lld list entries", name, (long long)N);
  if (K == 0 || C == 0) return 0;
  PD_REQUIRE(store_ok && ptr != nullptr && cols != nullptr && out != nullptr && flag != nullptr,
             "%s: store, ptr, cols, out and flag pointers required", name);
  PD_REQUIRE(N == 0 || (rows != nullptr && w != nullptr), "%s: rows and w required for %lld entries", name,
             (long long)N);
  const int64_t P = (int64_t)H * W;
  const int64_t chunks = ceil_div64(P, CM_CHUNK);
  const int64_t per_slot = (int64_t)C * chunks;
  constexpr int64_t GRID_LIMIT = (1ll << 31) - 1;
  PD_REQUIRE(chunks <= GRID_LIMIT && per_slot <= GRID_LIMIT, "%s: too large (%lld workgroups per slot)", name,
             (long long)per_slot);
  const bool vec = P % 4 == 0 && store_vec && aligned16(out);
  const int64_t slots_per_launch = GRID_LIMIT / per_slot;
  for (int64_t k0 = 0; k0 < K; k0 += slots_per_launch) {
    const int64_t nk = K - k0 < slots_per_launch ? K - k0 : slots_per_launch;
    const dim3 grid((unsigned)(nk * per_slot)), block(CM_THREADS);
    if (vec)
      hipLaunchKernelGGL((clim_mean_kernel<Reader, true>), grid, block, 0, (hipStream_t)stream, store, T, F, P, ptr,
                         rows, w, N, (int)k0, cols, C, (int)chunks, out, flag);
    else
      hipLaunchKernelGGL((clim_mean_kernel<Reader, false>), grid, block, 0, (hipStream_t)stream, store, T, F, P, ptr,
                         rows, w, N, (int)k0, cols, C, (int)chunks, out, flag);
    PD_CHECK_LAUNCH(name);
  }
  return 0;
}

constexpr int UNIT_INTS = 8;   // type, q, T, x, y, z, level, pad: the unit rows of paradis_forecast_post
constexpr int U_SINGLE = 0, U_LEVEL = 1, U_SURFACE = 2;

// thread (k, unit, cell): one cell of one wind triple of slot k.  Units without winds end at once (a handful of rows).
__global__ void __launch_bounds__(256)
spherical_winds_kernel(float* __restrict__ data, const int* __restrict__ units, int n_units,
                       const double* __restrict__ plev, const double* __restrict__ trig, int K, int C, int H, int W) {
  const int64_t P = (int64_t)H * W, per_slot = P * n_units, total = per_slot * K;
  const double* slat_t = trig;
  const double* clat_t = trig + H;
  const double* slon_t = trig + 2 * H;
  const double* clon_t = slon_t + W;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t k = i / per_slot, r = i - k * per_slot;
    const int u = (int)(r / P);
    const int64_t cell = r - (int64_t)u * P;
    const int* un = units + u * UNIT_INTS;
    const int type = un[0], ct = un[2], cx = un[3], cy = un[4], cz = un[5];
    if (type == U_SINGLE || cx < 0) continue;
    const int y = (int)(cell / W), x = (int)(cell - (int64_t)y * W);
    float* base = data + k * C * P + cell;
    const float X = base[cx * P], Y = base[cy * P], Z = base[cz * P];
    const bool level = type == U_LEVEL;
    const float T = level ? base[ct * P] : 0.f;
    const double pg = level ? plev[un[6]] * 100.0 * 9.80616 : 0.0;
    float ou, ov, ow;
    spherical_wind(X, Y, Z, T, level, pg, slat_t[y], clat_t[y], slon_t[x], clon_t[x], ou, ov, ow);
    if (isnan(X) || isnan(Y) || isnan(Z)) ou = ov = ow = __builtin_nanf("");
    base[cx * P] = ou;
    base[cy * P] = ov;
    base[cz * P] = ow;
  }
}

}  // namespace

extern "C" int paradis_clim_mean_chunk(void) { return CM_CHUNK; }

extern "C" int paradis_clim_mean(const float* store, int64_t T, int F, int H, int W, const int64_t* ptr,
                                 const int64_t* rows, const double* w, int64_t N, int K, const int* cols, int C,
                                 float* out, int* flag, void* stream) {
  return clim_mean_launch("clim_mean", FloatPlanes{store}, store != nullptr, aligned16(store), T, F, H, W, ptr, rows, w,
                          N, K, cols, C, out, flag, stream);
}

extern "C" int paradis_clim_mean_packed(const uint16_t* codes, const float* params, const int* domain, int64_t T, int F,
                                        int H, int W, const int64_t* ptr, const int64_t* rows, const double* w,
                                        int64_t N, int K, const int* cols, int C, float* out, int* flag, void* stream) {
  return clim_mean_launch("clim_mean_packed", PackedPlanes{codes, params, domain},
                          codes != nullptr && params != nullptr && domain != nullptr, aligned8(codes), T, F, H, W, ptr,
                          rows, w, N, K, cols, C, out, flag, stream);
}

extern "C" int paradis_spherical_winds_inplace(float* data, const int* units, const int* units_host, int n_units,
                                               const double* plev, int n_levels, const double* trig, int K, int C,
                                               int H, int W, void* stream) {
  PD_REQUIRE(K >= 0 && C >= 1 && H >= 1 && W >= 1, "spherical_winds_inplace: bad shape K=%d C=%d H=%d W=%d", K, C, H, W);
  PD_REQUIRE(n_units >= 0 && n_units <= C && n_levels >= 0 && n_levels <= C,
             "spherical_winds_inplace: %d units / %d levels for %d channels", n_units, n_levels, C);
  if (K == 0 || n_units == 0) return 0;
  PD_REQUIRE(data && units && units_host && trig && (n_levels == 0 || plev), "spherical_winds_inplace: null pointer");
  bool any = false;
  for (int u = 0; u < n_units; ++u) {
    const int* un = units_host + u * UNIT_INTS;
    PD_REQUIRE(un[0] >= U_SINGLE && un[0] <= U_SURFACE, "spherical_winds_inplace: unit %d has type %d", u, un[0]);
    if (un[0] == U_SINGLE || un[3] < 0) continue;
    any = true;
    PD_REQUIRE(un[3] < C && un[4] >= 0 && un[4] < C && un[5] >= 0 && un[5] < C,
               "spherical_winds_inplace: unit %d names a wind channel outside [0, %d)", u, C);
    PD_REQUIRE(un[3] != un[4] && un[3] != un[5] && un[4] != un[5],
               "spherical_winds_inplace: unit %d names one channel twice", u);
    if (un[0] == U_LEVEL)
      PD_REQUIRE(un[2] >= 0 && un[2] < C && un[6] >= 0 && un[6] < n_levels,
                 "spherical_winds_inplace: unit %d names a temperature channel or level outside the tensor", u);
  }
  if (!any) return 0;
  const int64_t total = (int64_t)K * n_units * H * W;
  const unsigned blocks = (unsigned)(ceil_div64(total, 256) < 4096 ? ceil_div64(total, 256) : 4096);
  hipLaunchKernelGGL(spherical_winds_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, data, units, n_units, plev,
                     trig, K, C, H, W);
  PD_CHECK_LAUNCH("spherical_winds_inplace");
  return 0;
}
