// Store preparation on the device: what the reference's scripts/preprocess_dataset.py does between raw ERA5 fields and
// the store that dataset.DeviceStore serves - compute_cartesian_wind (:42-105) and the per-feature statistics of
// compute_statistics (:409-479) and compute_tendency_statistics (:482-590) - as two entry points.
//
// a. paradis_store_stats: one pass over a slab x[T, F, H, W] (fp32) that accumulates per feature f, over every
//    non-NaN value (the reference's skipna=True: NaN is skipped, nothing else is),
//      {n, sum (x - pivot_f), sum (x - pivot_f)^2, min, max}
//    and, optionally in the same pass, the same five of the tendency d = x[t] - x[t - stride] (float32 subtraction, as
//    the reference's float32 arrays give it; a d that is NaN is skipped; its pivot is 0: a tendency is centred on
//    (x[last] - x[first]) / n).  Everything after the fp32 load (or the fp32 difference) is double.  pivot_f is the
//    first non-NaN cell, in index order, of plane f of the first row the accumulator ever sees (0 when that plane has
//    none): with plain sum x, sum x^2 a feature of mean 1e5 and standard deviation 0.5 loses 5 - 46 float32 ulps of its
//    std even in double; about a pivot the sums carry the spread only.  It is kept beside the sums, so every later slab
//    subtracts the same one.
//
//    Work layout (stream_common.h; the piece loop is written out here): a workgroup of 256 threads owns piece j of
//    PLANE_PIECE cells of the plane of ONE feature over a block of consecutive time rows, which it walks in order; thread
//    t handles the quads at cells 4 (256 i + t) of the piece, i = 0, 1, .., and in a quad the cells k = 0 .. 3: a
//    thread's additions are strictly sequential (rows, then quads, then cells).  The number of time blocks is chosen on
//    the host so that the grid stays near STATS_TARGET_WG workgroups whatever T x F is: the launch count (three), the
//    workgroup count and the partials do not grow with the length of the store.  Wave: xor tree; the four waves through
//    LDS, (r0 + r1) + (r2 + r3) (min / max alike); one ordinary store per quantity (partial [F][blocks][sets][5]).  A
//    finishing kernel folds the blocks of a feature in index order and merges them into the running accumulator by an
//    ordinary read-modify-write.  No atomics: bit-identical run to run for a given partition into slabs.
//    A tendency pair is counted with its LATER row; the earlier row may lie in `prev`, the rows that came before the
//    slab (StoreStats keeps the last max(strides) of them), so a pair that straddles two slabs is counted once.
//    16-byte loads when H W % 4 == 0 and both bases are 16-byte aligned (every quad of every plane is then whole and
//    aligned), four scalar loads otherwise (an odd H W leaves every second plane 4-byte aligned only); a cell past the
//    end of the piece is left out of every quantity, so both give the same bits.
//    With the field and stride 1 the row just read stays in registers as the next row's earlier operand
//    (stats_walk_carry: 4 B per value instead of 8; 6 % faster at 721x1440, 0.5 % at 32x64).
//    Algorithmic HBM bytes per value: 4 (field alone, field + stride 1), 8 (field + a longer stride, a tendency alone).
//
// b. paradis_cartesian_winds: every pressure level and the 10 m winds of T time rows in one launch, driven by a table
//    of rows {src u, src v, src omega, src T, dst x, dst y, dst z, level hPa}.  numpy multiplies the float32 fields by
//    float64 trigonometry of latitude and longitude, so the reference's result is the float64 expression rounded to
//    float32 once; so is this one: four host-built double tables (no device trigonometry), double arithmetic per cell in
//    the reference's order of operations, one rounding at the store.  The one place where numpy stays in float32 inside
//    the expression - omega * R * T, a float32 array times a Python scalar times a float32 array - is float32 here too
//    (as R * T is in post.hip, the inverse transform).
//    Algorithmic HBM bytes per cell: 28 for a level (four loads, three stores), 20 for the surface row.
#include "common.h"
#include "stream_common.h"

#include <cmath>

#pragma clang fp contract(off)

namespace {

constexpr int STATS_Q = 5;               // n, sum, sum of squares, min, max
constexpr int STATS_TARGET_WG = 4096;    // 16 workgroups per CU: the grid the time blocks are sized for

struct StatsArgs {
  const float* x;        // [T, F, P]
  const float* prev;     // [n_prev, F, P]: the rows before x, or null
  const double* acc;     // [F][n_sets + 1][5]; row n_sets = {pivot, pivot set, 0, 0, 0}
  double* partial;       // [F][nblocks][sets of this launch][5]
  int64_t P;
  int T, n_prev, F, stride, n_sets;
  int npieces, ntb, rows_per, vec;
};

struct Five {
  int n = 0;
  double s1 = 0.0, s2 = 0.0;
  float mn = INFINITY, mx = -INFINITY;
  __device__ __forceinline__ void add(float v, bool in, double pivot) {
    const bool ok = in && v == v;
    const double d = ok ? (double)v - pivot : 0.0;      // (a sum that starts at +0 is never -0: + 0.0 changes no bit)
    s1 += d;
    s2 += d * d;
    n += ok ? 1 : 0;
    mn = ok ? fminf(mn, v) : mn;
    mx = ok ? fmaxf(mx, v) : mx;
  }
};

// row r of the slab, r in [-n_prev, T): negative rows are the last rows of prev
__device__ __forceinline__ const float* stats_row(const StatsArgs& a, int r, int f) {
  const float* base = r >= 0 ? a.x : a.prev;
  const int64_t row = r >= 0 ? r : a.n_prev + r;
  return base + (row * a.F + f) * a.P;
}

template <bool FIELD, bool TEND, bool VEC>
__device__ __forceinline__ void stats_walk(const StatsArgs& a, int f, int r0, int r1, int start, int end, double pivot,
                                           Five& fs, Five& ts) {
  for (int r = r0; r < r1; ++r) {
    const float* cur = stats_row(a, r, f);
    const bool pair = TEND && r - a.stride >= -a.n_prev;               // (workgroup-uniform)
    if (!FIELD && !pair) continue;
    const float* old = pair ? stats_row(a, r - a.stride, f) : cur;
    // (the loop vectorizer would interleave two iterations and break the 16-byte accesses into 4-byte ones)
#pragma clang loop vectorize(disable) interleave(disable) unroll(full)
    for (int i = 0; i < PLANE_ITERS; ++i) {
      const int q0 = start + 4 * (256 * i + (int)threadIdx.x);
      if (q0 >= end) break;
      float c[4], o[4] = {0.f, 0.f, 0.f, 0.f};
      load_quad<VEC>(cur, q0, end, c);
      if (pair) load_quad<VEC>(old, q0, end, o);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const bool in = VEC || q0 + k < end;
        if (FIELD) fs.add(c[k], in, pivot);
        if (TEND) ts.add(c[k] - o[k], in && pair, 0.0);
      }
    }
  }
}

// stride 1 with the field: the row just read is the next row's earlier operand, kept in registers (the thread's quads
// of the piece: PLANE_ITERS x 4 floats) instead of being read again - 4 B per value and one more row per time block.
// The same values in the same order as stats_walk: the same bits.
template <bool VEC>
__device__ __forceinline__ void stats_walk_carry(const StatsArgs& a, int f, int r0, int r1, int start, int end,
                                                 double pivot, Five& fs, Five& ts) {
  float o[PLANE_ITERS][4];
  bool pair = r0 - 1 >= -a.n_prev;                                      // (workgroup-uniform)
  if (pair) {
    const float* old = stats_row(a, r0 - 1, f);
#pragma clang loop vectorize(disable) interleave(disable) unroll(full)
    for (int i = 0; i < PLANE_ITERS; ++i) {
      const int q0 = start + 4 * (256 * i + (int)threadIdx.x);
      if (q0 < end) load_quad<VEC>(old, q0, end, o[i]);
    }
  }
  for (int r = r0; r < r1; ++r) {
    const float* cur = stats_row(a, r, f);
#pragma clang loop vectorize(disable) interleave(disable) unroll(full)
    for (int i = 0; i < PLANE_ITERS; ++i) {
      const int q0 = start + 4 * (256 * i + (int)threadIdx.x);
      if (q0 >= end) break;
      float c[4];
      load_quad<VEC>(cur, q0, end, c);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const bool in = VEC || q0 + k < end;
        fs.add(c[k], in, pivot);
        ts.add(c[k] - (pair ? o[i][k] : 0.f), in && pair, 0.0);
        o[i][k] = c[k];
      }
    }
    pair = true;
  }
}

__device__ __forceinline__ double wave_min_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ double wave_max_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}

// the thread's five of one set -> the workgroup's, stored by threads 0 .. 4 at out[0 .. 4]
__device__ __forceinline__ void stats_store(const Five& s, double (*red)[4], double* out) {
  double w[STATS_Q];
  w[0] = wave_sum_f64((double)s.n);
  w[1] = wave_sum_f64(s.s1);
  w[2] = wave_sum_f64(s.s2);
  w[3] = wave_min_f64((double)s.mn);
  w[4] = wave_max_f64((double)s.mx);
  __syncthreads();                                       // (red is used once per set)
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int j = 0; j < STATS_Q; ++j) red[j][threadIdx.x >> 6] = w[j];
  }
  __syncthreads();
  if (threadIdx.x < STATS_Q) {
    const double* r = red[threadIdx.x];
    double v;
    if (threadIdx.x == 3) v = fmin(fmin(r[0], r[1]), fmin(r[2], r[3]));
    else if (threadIdx.x == 4) v = fmax(fmax(r[0], r[1]), fmax(r[2], r[3]));
    else v = (r[0] + r[1]) + (r[2] + r[3]);
    out[threadIdx.x] = v;
  }
}

template <bool FIELD, bool TEND, bool CARRY = false>
__global__ void __launch_bounds__(256) store_stats_kernel(StatsArgs a) {
  constexpr int NS = (FIELD ? 1 : 0) + (TEND ? 1 : 0);
  __shared__ double red[STATS_Q][4];
  const int nblocks = a.npieces * a.ntb;
  const int f = blockIdx.x / nblocks;
  const int blk = blockIdx.x - f * nblocks;
  const int piece = blk / a.ntb, tb = blk - piece * a.ntb;
  const int r0 = tb * a.rows_per, r1 = min(a.T, r0 + a.rows_per);
  const int start = piece * PLANE_PIECE;                               // P < 2^31
  const int end = (int)min(a.P, (int64_t)start + PLANE_PIECE);
  const double pivot = FIELD ? a.acc[((int64_t)f * (a.n_sets + 1) + a.n_sets) * STATS_Q] : 0.0;
  Five fs, ts;
  if (CARRY) {
    if (a.vec) stats_walk_carry<true>(a, f, r0, r1, start, end, pivot, fs, ts);
    else stats_walk_carry<false>(a, f, r0, r1, start, end, pivot, fs, ts);
  } else {
    if (a.vec) stats_walk<FIELD, TEND, true>(a, f, r0, r1, start, end, pivot, fs, ts);
    else stats_walk<FIELD, TEND, false>(a, f, r0, r1, start, end, pivot, fs, ts);
  }
  double* out = a.partial + ((int64_t)f * nblocks + blk) * (NS * STATS_Q);
  if (FIELD) stats_store(fs, red, out);
  if (TEND) stats_store(ts, red, out + (FIELD ? STATS_Q : 0));
}

// one wave per feature, before the first slab's sums: the pivot is the first non-NaN cell of plane f of row 0, found
// 64 cells at a time (the lowest lane of the first group that has one), else 0; set once per accumulator
__global__ void __launch_bounds__(64) store_stats_pivot_kernel(const float* __restrict__ x, double* __restrict__ acc,
                                                               int n_sets, int64_t P) {
  const int f = blockIdx.x;
  double* row = acc + ((int64_t)f * (n_sets + 1) + n_sets) * STATS_Q;
  if (row[1] != 0.0) return;                                           // (uniform: every lane reads the same word)
  const float* p = x + (int64_t)f * P;
  double pivot = 0.0;
  for (int64_t c0 = 0; c0 < P; c0 += 64) {
    const int64_t c = c0 + threadIdx.x;
    const float v = c < P ? p[c] : NAN;
    const unsigned long long m = __ballot(v == v);
    if (m != 0ull) {
      pivot = (double)__shfl(v, __ffsll((long long)m) - 1, 64);
      break;
    }
  }
  if (threadIdx.x == 0) {
    row[0] = pivot;
    row[1] = 1.0;
  }
}

// one wave per feature: lane j < NS * 5 folds quantity j % 5 of launch set j / 5 over the feature's blocks in index
// order and merges it into the accumulator's set (launches of one stream are ordered: an ordinary read-modify-write)
__global__ void __launch_bounds__(64) store_stats_finish_kernel(const double* __restrict__ partial,
                                                                double* __restrict__ acc, int nblocks, int ns,
                                                                int set0, int set1, int n_sets) {
  const int f = blockIdx.x, j = threadIdx.x;
  if (j >= ns * STATS_Q) return;
  const int s = j / STATS_Q, q = j - s * STATS_Q;
  const double* p = partial + (int64_t)f * nblocks * (ns * STATS_Q) + j;
  double* dst = acc + ((int64_t)f * (n_sets + 1) + (s == 0 ? set0 : set1)) * STATS_Q + q;
  double v = *dst;
  for (int b = 0; b < nblocks; ++b) {
    const double w = p[(int64_t)b * (ns * STATS_Q)];
    v = q == 3 ? fmin(v, w) : (q == 4 ? fmax(v, w) : v + w);
  }
  *dst = v;
}

struct StatsPlan {
  int npieces, ntb, rows_per;
};
inline StatsPlan stats_plan(int T, int F, int H, int W) {
  StatsPlan p;
  p.npieces = (int)ceil_div64((int64_t)H * W, PLANE_PIECE);
  const int64_t want = std::max<int64_t>(1, ceil_div64(STATS_TARGET_WG, (int64_t)F * p.npieces));
  p.rows_per = (int)ceil_div64(T, std::min<int64_t>(want, T));
  p.ntb = (int)ceil_div64(T, p.rows_per);
  return p;
}

// ---------------------------------------------------------------------------------------------- Cartesian winds

struct WindArgs {
  const float* src;
  float* dst;
  const paradis_wind_row_t* rows;
  const double* trig;      // sin(lat)[H], cos(lat)[H], sin(lon)[W], cos(lon)[W]
  int64_t src_ts, dst_ts;  // elements per time row: Fs P, Fd P
  int n_rows, T, H, W;
};

// V = 4: W % 4 == 0 and every plane 16-byte aligned; V = 1: the scalar path, the same arithmetic per cell.  A thread
// reads its cells of u, v, omega, T before it writes them of x, y, z: src may be dst as long as no row's destination is
// another row's source (prepare.WindPlan checks)
template <int V>
__global__ void __launch_bounds__(256) cartesian_winds_kernel(WindArgs a) {
  const int WV = a.W / V;
  const int64_t P = (int64_t)a.H * a.W;
  const int64_t per_row = (int64_t)a.H * WV, per_time = per_row * a.n_rows, total = per_time * a.T;
  const double* slat_t = a.trig;
  const double* clat_t = a.trig + a.H;
  const double* slon_t = a.trig + 2 * a.H;
  const double* clon_t = slon_t + a.W;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int t = (int)(i / per_time);
    const int64_t r = i - (int64_t)t * per_time;
    const int u_ = (int)(r / per_row);
    const int cell = (int)(r - (int64_t)u_ * per_row);
    const int y = cell / WV, x0 = (cell - y * WV) * V;
    const paradis_wind_row_t row = a.rows[u_];
    const int64_t pix = (int64_t)y * a.W + x0;
    const float* src = a.src + (int64_t)t * a.src_ts + pix;
    float* dst = a.dst + (int64_t)t * a.dst_ts + pix;
    const bool level = row.src_w >= 0;
    float u[V], v[V], w[V], T[V];
    if constexpr (V == 4) {
      load_quad<true>(src + row.src_u * P, 0, 4, u);
      load_quad<true>(src + row.src_v * P, 0, 4, v);
      if (level) {
        load_quad<true>(src + row.src_w * P, 0, 4, w);
        load_quad<true>(src + row.src_t * P, 0, 4, T);
      }
    } else {
      u[0] = src[row.src_u * P];
      v[0] = src[row.src_v * P];
      if (level) {
        w[0] = src[row.src_w * P];
        T[0] = src[row.src_t * P];
      }
    }
    const double sla = slat_t[y], cla = clat_t[y];
    const double pg = (double)row.level_hpa * 100.0 * 9.80616;          // plev * 100 * g, in that order
    float ox[V], oy[V], oz[V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const double slo = slon_t[x0 + j], clo = clon_t[x0 + j];
      const double U = (double)u[j], Vv = (double)v[j];
      double X = -U * slo - (Vv * sla) * clo;
      double Y = U * clo - (Vv * sla) * slo;
      double Z = Vv * cla;
      if (level) {
        const float wrt = (w[j] * 287.05f) * T[j];                        // numpy: omega * R * T stays float32
        const double k = (double)wrt / pg;
        X = X - (k * cla) * clo;
        Y = Y - (k * cla) * slo;
        Z = Z - k * sla;
      }
      ox[j] = (float)X;
      oy[j] = (float)Y;
      oz[j] = (float)Z;
    }
    if constexpr (V == 4) {
      *reinterpret_cast<float4*>(dst + row.dst_x * P) = make_float4(ox[0], ox[1], ox[2], ox[3]);
      *reinterpret_cast<float4*>(dst + row.dst_y * P) = make_float4(oy[0], oy[1], oy[2], oy[3]);
      *reinterpret_cast<float4*>(dst + row.dst_z * P) = make_float4(oz[0], oz[1], oz[2], oz[3]);
    } else {
      dst[row.dst_x * P] = ox[0];
      dst[row.dst_y * P] = oy[0];
      dst[row.dst_z * P] = oz[0];
    }
  }
}

}  // namespace

extern "C" int paradis_store_stats_piece(void) { return PLANE_PIECE; }

extern "C" size_t paradis_store_stats_ws_bytes(int T, int F, int H, int W) {
  if (T < 1 || F < 1 || H < 1 || W < 1) return 0;
  const StatsPlan p = stats_plan(T, F, H, W);
  return (size_t)F * (size_t)p.npieces * (size_t)p.ntb * 2 * STATS_Q * sizeof(double);
}

extern "C" int paradis_store_stats(const float* x, int T, const float* prev, int n_prev, int F, int H, int W,
                                   int field_set, int tend_set, int stride, double* acc, int n_sets, void* ws,
                                   void* stream) {
  PD_REQUIRE(T >= 0 && F >= 1 && H >= 1 && W >= 1, "store_stats: bad shape T=%d F=%d H=%d W=%d", T, F, H, W);
  PD_REQUIRE(n_sets >= 1 && field_set < n_sets && tend_set < n_sets && field_set >= -1 && tend_set >= -1,
             "store_stats: sets %d / %d outside the accumulator's %d", field_set, tend_set, n_sets);
  PD_REQUIRE(field_set >= 0 || tend_set >= 0, "store_stats: nothing to accumulate (both sets are -1)");
  PD_REQUIRE(field_set != tend_set, "store_stats: the field and the tendency need different sets");
  PD_REQUIRE(tend_set < 0 || stride >= 1, "store_stats: stride must be >= 1, got %d", stride);
  PD_REQUIRE(n_prev >= 0 && (n_prev == 0 || prev != nullptr), "store_stats: %d previous rows without their tensor",
             n_prev);
  if (T == 0) return 0;
  PD_REQUIRE(x && acc && ws, "store_stats: null pointer");
  const int64_t P = (int64_t)H * W;
  PD_REQUIRE(P < (1ll << 31) - PLANE_PIECE, "store_stats: a plane of %d x %d cells is too large", H, W);
  const StatsPlan p = stats_plan(T, F, H, W);
  const int64_t grid = (int64_t)F * p.npieces * p.ntb;
  PD_REQUIRE(grid < (1ll << 31), "store_stats: %lld workgroups exceed the grid limit", (long long)grid);
  StatsArgs a;
  a.x = x; a.prev = n_prev > 0 ? prev : nullptr; a.acc = acc; a.partial = static_cast<double*>(ws);
  a.P = P; a.T = T; a.n_prev = n_prev; a.F = F; a.stride = tend_set >= 0 ? stride : 1; a.n_sets = n_sets;
  a.npieces = p.npieces; a.ntb = p.ntb; a.rows_per = p.rows_per;
  a.vec = (P % 4 == 0) && aligned16(x) && (a.prev == nullptr || aligned16(a.prev));
  hipStream_t st = (hipStream_t)stream;
  const dim3 g((unsigned)grid), wg(256);
  const int nblocks = p.npieces * p.ntb;
  if (field_set >= 0) {
    hipLaunchKernelGGL(store_stats_pivot_kernel, dim3(F), dim3(64), 0, st, x, acc, n_sets, P);
    if (tend_set >= 0 && stride == 1) hipLaunchKernelGGL((store_stats_kernel<true, true, true>), g, wg, 0, st, a);
    else if (tend_set >= 0) hipLaunchKernelGGL((store_stats_kernel<true, true>), g, wg, 0, st, a);
    else hipLaunchKernelGGL((store_stats_kernel<true, false>), g, wg, 0, st, a);
  } else {
    hipLaunchKernelGGL((store_stats_kernel<false, true>), g, wg, 0, st, a);
  }
  const int ns = (field_set >= 0 ? 1 : 0) + (tend_set >= 0 ? 1 : 0);
  hipLaunchKernelGGL(store_stats_finish_kernel, dim3(F), dim3(64), 0, st, a.partial, acc, nblocks, ns,
                     field_set >= 0 ? field_set : tend_set, tend_set, n_sets);
  PD_CHECK_LAUNCH("store_stats");
  return 0;
}

extern "C" int paradis_cartesian_winds(const float* src, int Fs, float* dst, int Fd, const paradis_wind_row_t* rows,
                                       const paradis_wind_row_t* rows_host, int n_rows, const double* trig, int T,
                                       int H, int W, void* stream) {
  PD_REQUIRE(T >= 0 && Fs >= 1 && Fd >= 1 && H >= 1 && W >= 1, "cartesian_winds: bad shape T=%d Fs=%d Fd=%d H=%d W=%d",
             T, Fs, Fd, H, W);
  PD_REQUIRE(n_rows >= 0, "cartesian_winds: %d table rows", n_rows);
  if (T == 0 || n_rows == 0) return 0;
  PD_REQUIRE(src && dst && rows && rows_host && trig, "cartesian_winds: null pointer");
  const int64_t P = (int64_t)H * W;
  PD_REQUIRE(P * std::max(Fs, Fd) < (1ll << 31), "cartesian_winds: a time row of %d x %d x %d cells is too large",
             std::max(Fs, Fd), H, W);
  for (int i = 0; i < n_rows; ++i) {                   // the host copy of the table: nothing outside the tensors is touched
    const paradis_wind_row_t& r = rows_host[i];
    const bool level = r.src_w >= 0 || r.src_t >= 0;
    PD_REQUIRE(r.src_u >= 0 && r.src_u < Fs && r.src_v >= 0 && r.src_v < Fs, "cartesian_winds: row %d: u / v column outside [0, %d)", i, Fs);
    PD_REQUIRE(!level || (r.src_w >= 0 && r.src_w < Fs && r.src_t >= 0 && r.src_t < Fs),
               "cartesian_winds: row %d: a level needs omega and T columns inside [0, %d)", i, Fs);
    PD_REQUIRE(!level || (std::isfinite(r.level_hpa) && r.level_hpa > 0.f), "cartesian_winds: row %d: level %g hPa", i,
               (double)r.level_hpa);
    PD_REQUIRE(r.dst_x >= 0 && r.dst_x < Fd && r.dst_y >= 0 && r.dst_y < Fd && r.dst_z >= 0 && r.dst_z < Fd,
               "cartesian_winds: row %d: destination column outside [0, %d)", i, Fd);
  }
  WindArgs a;
  a.src = src; a.dst = dst; a.rows = rows; a.trig = trig;
  a.src_ts = (int64_t)Fs * P; a.dst_ts = (int64_t)Fd * P;
  a.n_rows = n_rows; a.T = T; a.H = H; a.W = W;
  const bool vec = (W % 4 == 0) && aligned16(src) && aligned16(dst);
  const int64_t total = (int64_t)T * n_rows * H * (vec ? W / 4 : W);
  const unsigned blocks = (unsigned)std::min<int64_t>(ceil_div64(total, 256), 256 * 32);
  if (vec) hipLaunchKernelGGL(cartesian_winds_kernel<4>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(cartesian_winds_kernel<1>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, a);
  PD_CHECK_LAUNCH("cartesian_winds");
  return 0;
}
