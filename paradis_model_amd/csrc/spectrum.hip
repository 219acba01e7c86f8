// Zonal power spectra of a forecast state and its truth [B, C, H, W] (physical units, fp32, each with its own batch
// stride: chunk[:, slot] and truth[:, k] are consumed in place).  The project's own definition, in the spirit of
// WeatherBench-2's ZonalEnergySpectrum and not pinned against it.  Per row h of a plane, W even, K = W / 2, k = 0 .. K:
//   X[h,k] = (1/W) sum_i x[h,i] exp(-2 pi i k i / W)          m_k = 1 for k in {0, K}, else 2
//   pf = m_k |F|^2      pt = m_k |T|^2      co = m_k Re(F conj T)
// and per band r with row weights wb[r,h] >= 0:  S[r,k] = sum_h wb[r,h] p[h,k] / sum_h wb[r,h]  over the rows with
// wb[r,h] != 0 (a row of weight 0 is left out of the band, not multiplied in: its NaN never reaches the band; a row of
// weight 0 in every band is neither read nor transformed).  Otherwise non-finite values propagate.
//   acc[cs][r][k][0..2] += {S_ff, S_tt, S_ft}  per sample, in b order;   count += B
//
// One transform per row pair.  z = (f - p) + i (t - p) with the pivot p = t[h,0] (fp32 differences of neighbouring
// magnitudes: the mean of a 1e5-offset field does not eat the mantissa of the transform); Z = sum_i z_i w^(k i) is ONE
// complex length-W transform, and with Zc = Z[(W - k) mod W]
//   F = (Z_k + conj Zc) / 2W        T = (Z_k - conj Zc) / 2iW        k = 0:  F += p, T += p
// formed in double from the fp32 Z.  Everything after the transform is double.
//
// Two schedules, chosen on the host from W (spectrum_plan):
//   fft     W = product of radices out of {4, 2, 3, 5} (at most one 2): Stockham autosort, decimation in frequency.  A
//           pass of radix r at length n (stride s = W / n, m = n / r) takes butterfly t = p s + q (p < m, q < s), reads
//           a_j = x[t + j W / r], forms b = DFT_r(a) and writes y[q + s (r p + j)] = b_j w_n^(p j), w_n^(p j) =
//           table[p j s] (p j s < W: no reduction).  The last pass leaves Z in natural order.
//   direct  any other even W <= SPECTRUM_DIRECT_MAX_W: Z_k = sum_j z_j table[(j k) mod W], the index kept by add and
//           conditional subtract, the sum in double (254 sequential fp32 additions would cost the bound of the tests).
// The table exp(-2 pi i j / W), j < W, comes from the host (double, rounded to fp32 once); no device sincos.
//
// LDS.  Real and imaginary parts are separate float arrays, two buffers of each (ping-pong), for NR rows in flight; the
// element of logical index i lives at i + (i >> 5): one pad word per 32.  Reads of a pass are unit-stride across the lanes
// (t + j W / r): conflict-free.  Writes have lane stride r at s = 1 (and r s / gcd patterns later): without the pad a
// radix-4 pass puts 32 lanes on 8 banks (4-way; ds_write banks are dword % 32), with it lanes l and l + 8 land one bank
// apart and the first pass is conflict-free; later passes write runs of s consecutive words per p, which the pad leaves
// conflict-free for s >= 32 and at worst 2-way in between.  A power-of-two stride never meets a power-of-two row.
// The per-band sums live in LDS as doubles [R][3][K + 1]; slot (r, k) is owned by ONE thread (k = tid + 256 j) that adds
// the rows in index order: no synchronisation, no atomics, a fixed order.  The twiddle table, the weights of the run's
// rows and the pivots of the rows in flight are in LDS too (see the prefetch in the kernel).
//
// Work layout.  A workgroup owns rows [g ROWS, g ROWS + ROWS) of plane (b, cs): it lists the rows with a non-zero
// weight, transforms them NR at a time (NR W <= SPECTRUM_FLIGHT cells in flight), and stores its band sums as partial
// [B Cs][G][R][3][K + 1] double.  The finishing kernel (one thread per (cs, r, k)) folds, per sample in b order, the row
// groups in index order, divides by the band's weight sum and adds to acc: two updates of B samples are one update of
// the 2B batch bit for bit.  Thread 0 adds B to count.
// Algorithmic HBM bytes: 8 * B * Cs * (rows of non-zero weight) * W.
#include "common.h"

#include <cmath>

// The stated formulas are the arithmetic: F, T and the three products are written out in double, and the butterflies
// are additions and explicit products whose rounding the CPU yardsticks (tests/spectrum_oracle.py) are compared with.
#pragma clang fp contract(off)

namespace {

constexpr int SPECTRUM_THREADS = 256;
constexpr int SPECTRUM_ROWS = 32;              // rows of one plane per workgroup
constexpr int SPECTRUM_FFT_MAX_W = 2048;       // fft schedule: one row is at most the cells in flight (SPECTRUM_FLIGHT)
constexpr int SPECTRUM_DIRECT_MAX_W = 254;     // direct schedule: W^2 / 256 double complex multiply-adds per thread and row
constexpr int SPECTRUM_FLIGHT = 2048;          // cells in flight: NR = clamp(SPECTRUM_FLIGHT / W, 1, SPECTRUM_ROWS)
constexpr int SPECTRUM_PF = SPECTRUM_FLIGHT / SPECTRUM_THREADS;      // cells of a batch per thread (the prefetch registers)
constexpr int SPECTRUM_MAX_PASSES = 8;         // 2 * 3^6 = 1458 has 7 factors; 2 * 3^7 > 2048
static_assert(SPECTRUM_FFT_MAX_W <= SPECTRUM_FLIGHT && SPECTRUM_DIRECT_MAX_W <= SPECTRUM_FLIGHT, "a row must fit a batch");
constexpr int SPECTRUM_MAX_BANDS = 64;
constexpr size_t SPECTRUM_LDS = 160 * 1024;    // per workgroup (one CU's LDS)
constexpr size_t SPECTRUM_LDS_STATIC = 512;    // of it for the kernel's static arrays

enum { SCHED_NONE = 0, SCHED_FFT = 1, SCHED_DIRECT = 2 };

struct SpectrumPlan {
  int schedule;
  int npass;
  int radix[SPECTRUM_MAX_PASSES];
};

// the one schedule choice: W even; {2,3,5}-smooth up to the fft limit -> fft, else up to the direct limit -> direct
inline SpectrumPlan spectrum_plan(int W) {
  SpectrumPlan p;
  p.schedule = SCHED_NONE;
  p.npass = 0;
  if (W < 2 || (W & 1)) return p;
  if (W <= SPECTRUM_FFT_MAX_W) {
    int n = W;
    const int order[4] = {4, 2, 3, 5};
    for (int r : order) {
      while (n % r == 0 && !(r == 2 && n % 4 == 0) && p.npass < SPECTRUM_MAX_PASSES) {
        p.radix[p.npass++] = r;
        n /= r;
      }
    }
    if (n == 1) {
      p.schedule = SCHED_FFT;
      return p;
    }
    p.npass = 0;
  }
  if (W <= SPECTRUM_DIRECT_MAX_W) p.schedule = SCHED_DIRECT;
  return p;
}

inline int spectrum_flight_rows(int W) { return std::max(1, std::min(SPECTRUM_ROWS, SPECTRUM_FLIGHT / W)); }
inline int spectrum_groups(int H) { return (H + SPECTRUM_ROWS - 1) / SPECTRUM_ROWS; }
__host__ __device__ inline int spectrum_pad(int i) { return i + (i >> 5); }
// dynamic LDS: the band sums and the weights of the run's rows (double, first: 8-byte aligned), then the twiddle table
// (tw_lds) and 4 float arrays of NR padded rows
inline size_t spectrum_lds_bytes(int W, int R, bool tw_lds) {
  const size_t dbl = ((size_t)R * 3 * (W / 2 + 1) + (size_t)R * SPECTRUM_ROWS) * sizeof(double);
  const size_t row = (size_t)spectrum_pad(W) + 1;
  return dbl + ((tw_lds ? 2 * (size_t)W : 0) + 4 * (size_t)spectrum_flight_rows(W) * row) * sizeof(float);
}
// the twiddle table goes to LDS unless that alone costs a CU its second workgroup (721 x 1440 with three bands)
inline bool spectrum_tw_lds(int W, int R) {
  const size_t half = SPECTRUM_LDS / 2 - SPECTRUM_LDS_STATIC;
  return !(spectrum_lds_bytes(W, R, true) > half && spectrum_lds_bytes(W, R, false) <= half);
}
// n / d for 0 <= n < 2^16 with inv = 1.0f / d: (n + 0.5) / d is at least 0.5 / d away from an integer, the float
// product is off by less than 2^-22 n / d
__device__ __forceinline__ int spectrum_div(int n, float inv) { return (int)(((float)n + 0.5f) * inv); }

struct SpectrumArgs {
  const float* fc;
  const float* truth;
  const int* chan;          // [Cs] or null (cs -> cs)
  const double* wb;         // [R][H]
  const float* tw;          // [W][2]
  double* partial;          // [B Cs][G][R][3][K + 1]
  int64_t fc_bs, truth_bs;
  int C, Cs, H, W, R, G, NR;
  SpectrumPlan plan;
};

// b = DFT_R(a): b_j = sum_k a_k exp(-2 pi i j k / R)
template <int R>
__device__ __forceinline__ void dft_small(const float (&ar)[5], const float (&ai)[5], float (&br)[5], float (&bi)[5]) {
  if (R == 2) {
    br[0] = ar[0] + ar[1]; bi[0] = ai[0] + ai[1];
    br[1] = ar[0] - ar[1]; bi[1] = ai[0] - ai[1];
  } else if (R == 4) {
    const float sr = ar[0] + ar[2], si = ai[0] + ai[2], dr = ar[0] - ar[2], di = ai[0] - ai[2];
    const float tr = ar[1] + ar[3], ti = ai[1] + ai[3], er = ar[1] - ar[3], ei = ai[1] - ai[3];
    br[0] = sr + tr; bi[0] = si + ti;
    br[2] = sr - tr; bi[2] = si - ti;
    br[1] = dr + ei; bi[1] = di - er;        // d - i e
    br[3] = dr - ei; bi[3] = di + er;        // d + i e
  } else if (R == 3) {
    constexpr float C1 = -0.5f, S1 = 0.86602540378443864676f;        // cos, sin of 2 pi / 3
    const float sr = ar[1] + ar[2], si = ai[1] + ai[2], dr = ar[1] - ar[2], di = ai[1] - ai[2];
    br[0] = ar[0] + sr; bi[0] = ai[0] + si;
    const float mr = ar[0] + C1 * sr, mi = ai[0] + C1 * si;
    br[1] = mr + S1 * di; bi[1] = mi - S1 * dr;                      // m - i S1 d
    br[2] = mr - S1 * di; bi[2] = mi + S1 * dr;
  } else {                                                           // R == 5
    constexpr float C1 = 0.30901699437494742410f, S1 = 0.95105651629515357212f;     // 2 pi / 5
    constexpr float C2 = -0.80901699437494742410f, S2 = 0.58778525229247312917f;    // 4 pi / 5
    const float s1r = ar[1] + ar[4], s1i = ai[1] + ai[4], d1r = ar[1] - ar[4], d1i = ai[1] - ai[4];
    const float s2r = ar[2] + ar[3], s2i = ai[2] + ai[3], d2r = ar[2] - ar[3], d2i = ai[2] - ai[3];
    br[0] = ar[0] + (s1r + s2r); bi[0] = ai[0] + (s1i + s2i);
    const float m1r = ar[0] + (C1 * s1r + C2 * s2r), m1i = ai[0] + (C1 * s1i + C2 * s2i);
    const float m2r = ar[0] + (C2 * s1r + C1 * s2r), m2i = ai[0] + (C2 * s1i + C1 * s2i);
    const float n1r = S1 * d1r + S2 * d2r, n1i = S1 * d1i + S2 * d2i;
    const float n2r = S2 * d1r - S1 * d2r, n2i = S2 * d1i - S1 * d2i;
    br[1] = m1r + n1i; bi[1] = m1i - n1r;                            // m1 - i n1
    br[4] = m1r - n1i; bi[4] = m1i + n1r;
    br[2] = m2r + n2i; bi[2] = m2i - n2r;                            // m2 - i n2
    br[3] = m2r - n2i; bi[3] = m2i + n2r;
  }
}

// one Stockham pass of radix R over nb rows: butterflies t < W / R of row j at flat item j (W / R) + t
template <int R>
__device__ __forceinline__ void fft_pass(const float* __restrict__ xr, const float* __restrict__ xi, float* __restrict__ yr,
                                         float* __restrict__ yi, const float* __restrict__ tw, int W, int s, int nb,
                                         int rowlen) {
  const int per = W / R;
  const float inv_per = 1.0f / (float)per, inv_s = 1.0f / (float)s;
  for (int it = threadIdx.x; it < nb * per; it += SPECTRUM_THREADS) {
    const int row = nb == 1 ? 0 : spectrum_div(it, inv_per), t = it - row * per;
    const int p = spectrum_div(t, inv_s), q = t - p * s;
    const int base = row * rowlen;
    float ar[5], ai[5], br[5], bi[5];
#pragma unroll
    for (int j = 0; j < R; ++j) {
      const int i = spectrum_pad(t + j * per);
      ar[j] = xr[base + i];
      ai[j] = xi[base + i];
    }
    dft_small<R>(ar, ai, br, bi);
    const int o = q + s * R * p;
    const int step = p * s;                                   // index of w_n^p in the table; j-th power at j * step < W
    {
      const int i = spectrum_pad(o);
      yr[base + i] = br[0];
      yi[base + i] = bi[0];
    }
#pragma unroll
    for (int j = 1; j < R; ++j) {
      const float wr = tw[2 * (j * step)], wi = tw[2 * (j * step) + 1];
      const int i = spectrum_pad(o + j * s);
      yr[base + i] = br[j] * wr - bi[j] * wi;
      yi[base + i] = br[j] * wi + bi[j] * wr;
    }
  }
}

// TWL: the twiddle table is copied to LDS (spectrum_tw_lds)
template <bool TWL>
__global__ void __launch_bounds__(SPECTRUM_THREADS) spectrum_kernel(SpectrumArgs a) {
  extern __shared__ double lds_d[];
  __shared__ int rows[SPECTRUM_ROWS];            // the rows of this run with a non-zero weight, in index order
  __shared__ int nrows_s;
  __shared__ float piv[SPECTRUM_ROWS];           // the pivots of the rows in flight
  const int W = a.W, K = W >> 1, K1 = K + 1, R = a.R, H = a.H;
  const int rowlen = spectrum_pad(W) + 1;
  double* band = lds_d;                                                   // [R][3][K1]
  double* wrow = band + (size_t)R * 3 * K1;                               // [R][ROWS]: the weights of the listed rows
  float* twl = reinterpret_cast<float*>(wrow + (size_t)R * SPECTRUM_ROWS);   // [W][2]: the twiddle table
  float* buf = twl + (TWL ? 2 * W : 0);                                   // re0, im0, re1, im1: [NR][rowlen] each
  const float* tw = TWL ? twl : a.tw;
  const int bufsz = a.NR * rowlen;
  const int plane = blockIdx.x / a.G, g = blockIdx.x - plane * a.G;       // plane = b Cs + cs
  const int b = plane / a.Cs, cs = plane - b * a.Cs;
  const int c = a.chan ? a.chan[cs] : cs;
  const bool bad = c < 0 || c >= a.C;                                     // (workgroup-uniform) nothing of it is read
  const int h0 = g * SPECTRUM_ROWS, h1 = min(H, h0 + SPECTRUM_ROWS);
  double* out = a.partial + ((int64_t)plane * a.G + g) * ((int64_t)R * 3 * K1);

  for (int i = threadIdx.x; i < R * 3 * K1; i += SPECTRUM_THREADS) band[i] = 0.0;
  if (threadIdx.x == 0) {
    int n = 0;
    for (int h = h0; h < h1; ++h) {
      bool any = false;
      for (int r = 0; r < R; ++r) any = any || a.wb[(int64_t)r * H + h] != 0.0;
      if (any) rows[n++] = h;
    }
    nrows_s = bad ? 0 : n;
  }
  if (TWL)
    for (int i = threadIdx.x; i < 2 * W; i += SPECTRUM_THREADS) twl[i] = a.tw[i];
  __syncthreads();
  const int nrows = nrows_s;
  for (int i = threadIdx.x; i < R * nrows; i += SPECTRUM_THREADS) {       // (read after the first barrier of the loop)
    const int r = i / nrows, j = i - r * nrows;
    wrow[r * SPECTRUM_ROWS + j] = a.wb[(int64_t)r * H + rows[j]];
  }
  const int64_t P = (int64_t)H * W;
  const float* f = a.fc + (int64_t)b * a.fc_bs + (int64_t)(bad ? 0 : c) * P;
  const float* t = a.truth + (int64_t)b * a.truth_bs + (int64_t)(bad ? 0 : c) * P;

  // The global loads of a batch are issued one batch ahead, into registers, and land in LDS when the batch starts: with
  // the twiddles, the weights and the pivots in LDS nothing else is loaded from memory in between, so no wait on a later
  // load drains them early and their latency hides behind the passes of the batch in front.  Cell j of this thread is
  // cell tid + THREADS j of the batch: (row in the batch, column), the same for every batch.
  int cell[SPECTRUM_PF];
  float rf[SPECTRUM_PF], rt[SPECTRUM_PF], rp[SPECTRUM_PF];
#pragma unroll
  for (int j = 0; j < SPECTRUM_PF; ++j) {
    const int it = (int)threadIdx.x + SPECTRUM_THREADS * j, row = it / W;
    cell[j] = (row << 16) | (it - row * W);                               // W <= 2048, row < 32
  }
  auto prefetch = [&](int r0, int nb) {
#pragma unroll
    for (int j = 0; j < SPECTRUM_PF; ++j) {
      const int row = cell[j] >> 16, col = cell[j] & 0xffff;
      if (row < nb) {
        const int64_t o = (int64_t)rows[r0 + row] * W;
        rf[j] = f[o + col];
        rt[j] = t[o + col];
        rp[j] = t[o];
      }
    }
  };
  if (nrows > 0) prefetch(0, min(a.NR, nrows));
  for (int r0 = 0; r0 < nrows; r0 += a.NR) {
    const int nb = min(a.NR, nrows - r0);
    float* xr = buf;
    float* xi = buf + bufsz;
    float* yr = buf + 2 * bufsz;
    float* yi = buf + 3 * bufsz;
    // z = (f - p) + i (t - p), p = t[h, 0]
#pragma unroll
    for (int j = 0; j < SPECTRUM_PF; ++j) {
      const int row = cell[j] >> 16, col = cell[j] & 0xffff;
      if (row < nb) {
        const int d = row * rowlen + spectrum_pad(col);
        xr[d] = rf[j] - rp[j];
        xi[d] = rt[j] - rp[j];
        if (col == 0) piv[row] = rp[j];
      }
    }
    __syncthreads();
    if (r0 + a.NR < nrows) prefetch(r0 + a.NR, min(a.NR, nrows - r0 - a.NR));
    if (a.plan.schedule == SCHED_FFT) {
      int s = 1;
      for (int ps = 0; ps < a.plan.npass; ++ps) {
        const int r = a.plan.radix[ps];
        if (r == 4) fft_pass<4>(xr, xi, yr, yi, tw, W, s, nb, rowlen);
        else if (r == 2) fft_pass<2>(xr, xi, yr, yi, tw, W, s, nb, rowlen);
        else if (r == 3) fft_pass<3>(xr, xi, yr, yi, tw, W, s, nb, rowlen);
        else fft_pass<5>(xr, xi, yr, yi, tw, W, s, nb, rowlen);
        s *= r;
        float* sw = xr; xr = yr; yr = sw;
        sw = xi; xi = yi; yi = sw;
        __syncthreads();
      }
    } else {
      for (int it = threadIdx.x; it < nb * W; it += SPECTRUM_THREADS) {
        const int row = it / W, k = it - row * W;
        const int base = row * rowlen;
        double sr = 0.0, si = 0.0;
        int idx = 0;                                            // (j k) mod W
        for (int j = 0; j < W; ++j) {
          const double zr = (double)xr[base + spectrum_pad(j)], zi = (double)xi[base + spectrum_pad(j)];
          const double wr = (double)tw[2 * idx], wi = (double)tw[2 * idx + 1];
          sr += zr * wr - zi * wi;
          si += zr * wi + zi * wr;
          idx += k;
          if (idx >= W) idx -= W;
        }
        yr[base + spectrum_pad(k)] = (float)sr;
        yi[base + spectrum_pad(k)] = (float)si;
      }
      float* sw = xr; xr = yr; yr = sw;
      sw = xi; xi = yi; yi = sw;
      __syncthreads();
    }
    // Z is in (xr, xi), natural order.  Thread-owned k: the rows of the batch in index order.
    const double inv = 0.5 / (double)W;
    for (int k = threadIdx.x; k < K1; k += SPECTRUM_THREADS) {
      const int kc = k == 0 ? 0 : W - k;
      const double m = (k == 0 || k == K) ? 1.0 : 2.0;
      for (int row = 0; row < nb; ++row) {
        const int base = row * rowlen;
        const double zr = (double)xr[base + spectrum_pad(k)], zi = (double)xi[base + spectrum_pad(k)];
        const double cr = (double)xr[base + spectrum_pad(kc)], ci = (double)xi[base + spectrum_pad(kc)];
        double Fr = (zr + cr) * inv, Fi = (zi - ci) * inv;     // (Z_k + conj Zc) / 2W
        double Tr = (zi + ci) * inv, Ti = (cr - zr) * inv;     // (Z_k - conj Zc) / 2iW
        if (k == 0) {
          const double p = (double)piv[row];
          Fr += p;
          Tr += p;
        }
        const double pf = m * (Fr * Fr + Fi * Fi);
        const double pt = m * (Tr * Tr + Ti * Ti);
        const double co = m * (Fr * Tr + Fi * Ti);
        for (int r = 0; r < R; ++r) {
          const double w = wrow[r * SPECTRUM_ROWS + r0 + row];
          if (w != 0.0) {
            double* s3 = band + (size_t)r * 3 * K1 + k;
            s3[0] += w * pf;
            s3[K1] += w * pt;
            s3[2 * K1] += w * co;
          }
        }
      }
    }
    __syncthreads();                                            // the next batch overwrites the buffers
  }
  // every slot was written by the thread that stores it, except the zero fill (in front of a barrier above)
  for (int k = threadIdx.x; k < K1; k += SPECTRUM_THREADS)
    for (int j = 0; j < R * 3; ++j) out[(size_t)j * K1 + k] = bad ? (double)NAN : band[(size_t)j * K1 + k];
}

// one thread per (cs, r, k); for b = 0 .. B - 1 in order: the row groups of plane (b, cs) in index order, divided by the
// band's weight sum, added to the thread's copy of the three accumulators (launches of one stream are ordered: an
// ordinary read-modify-write)
__global__ void __launch_bounds__(256) spectrum_finish_kernel(const double* __restrict__ partial,
                                                              const double* __restrict__ wsum, double* __restrict__ acc,
                                                              double* __restrict__ count, int B, int Cs, int G, int R,
                                                              int K1) {
  const int64_t n = (int64_t)Cs * R * K1;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i == 0) count[0] += (double)B;
  if (i >= n) return;
  const int k = (int)(i % K1);
  const int r = (int)((i / K1) % R);
  const int cs = (int)(i / ((int64_t)K1 * R));
  const double z = wsum[r];
  double s[3] = {acc[3 * i], acc[3 * i + 1], acc[3 * i + 2]};
  const int64_t block = (int64_t)R * 3 * K1;
  for (int b = 0; b < B; ++b) {
    const double* p = partial + ((int64_t)b * Cs + cs) * G * block + ((int64_t)r * 3) * K1 + k;
    double v[3] = {0.0, 0.0, 0.0};
    for (int g = 0; g < G; ++g) {
#pragma unroll
      for (int j = 0; j < 3; ++j) v[j] += p[(int64_t)g * block + (int64_t)j * K1];
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) s[j] += v[j] / z;
  }
#pragma unroll
  for (int j = 0; j < 3; ++j) acc[3 * i + j] = s[j];
}

PerDeviceOnce spectrum_lds_once;

}  // namespace

extern "C" int paradis_spectrum_rows(void) { return SPECTRUM_ROWS; }
extern "C" int paradis_spectrum_fft_max_w(void) { return SPECTRUM_FFT_MAX_W; }
extern "C" int paradis_spectrum_direct_max_w(void) { return SPECTRUM_DIRECT_MAX_W; }
extern "C" int paradis_spectrum_schedule(int W) { return spectrum_plan(W).schedule; }

extern "C" size_t paradis_spectrum_ws_bytes(int B, int Cs, int H, int W, int R) {
  if (B < 1 || Cs < 1 || H < 1 || W < 2 || R < 1) return 0;
  return (size_t)B * (size_t)Cs * (size_t)spectrum_groups(H) * (size_t)R * 3 * (size_t)(W / 2 + 1) * sizeof(double);
}

extern "C" int paradis_spectrum_update(const float* fc, int64_t fc_bs, const float* truth, int64_t truth_bs,
                                       const int* channels, int Cs, const double* band_w, const double* band_wsum,
                                       const float* twiddle, double* acc, double* count, void* ws, int B, int C, int H,
                                       int W, int R, void* stream) {
  PD_REQUIRE(B >= 0 && C >= 1 && H >= 1 && W >= 1 && Cs >= 1, "spectrum_update: bad shape B=%d C=%d Cs=%d H=%d W=%d", B,
             C, Cs, H, W);
  const SpectrumPlan plan = spectrum_plan(W);
  PD_REQUIRE(plan.schedule != SCHED_NONE,
             "spectrum_update: W = %d is refused: W must be even and either a product of 2, 3 and 5 up to %d (fft) or at "
             "most %d (direct)", W, SPECTRUM_FFT_MAX_W, SPECTRUM_DIRECT_MAX_W);
  PD_REQUIRE(R >= 1 && R <= SPECTRUM_MAX_BANDS, "spectrum_update: R (bands) must be in [1, %d], got %d", SPECTRUM_MAX_BANDS,
             R);
  const bool tw_lds = spectrum_tw_lds(W, R);
  const size_t lds = spectrum_lds_bytes(W, R, tw_lds);
  PD_REQUIRE(lds + SPECTRUM_LDS_STATIC <= SPECTRUM_LDS, "spectrum_update: R = %d bands at W = %d need %zu bytes of LDS, a workgroup has %zu", R,
             W, lds, SPECTRUM_LDS);
  PD_REQUIRE(channels != nullptr || Cs == C, "spectrum_update: without a channel table Cs must equal C (%d != %d)", Cs, C);
  if (B == 0) return 0;
  PD_REQUIRE(acc != nullptr && count != nullptr, "spectrum_update: acc or count missing");
  PD_REQUIRE(ws != nullptr, "spectrum_update: ws (workspace) missing");
  PD_REQUIRE(fc && truth && band_w && band_wsum && twiddle, "spectrum_update: null input pointer");
  const int64_t P = (int64_t)H * W;
  PD_REQUIRE(P < (1ll << 31), "spectrum_update: a plane of %d x %d cells is too large", H, W);
  PD_REQUIRE(fc_bs >= P * C && truth_bs >= P * C, "spectrum_update: batch strides shorter than one state");
  const int G = spectrum_groups(H);
  const int64_t blocks = (int64_t)B * Cs * G;
  PD_REQUIRE(blocks < (1ll << 31) && (int64_t)Cs * R * (W / 2 + 1) < (1ll << 31) * 256,
             "spectrum_update: %lld workgroups exceed the grid limit", (long long)blocks);
  SpectrumArgs a;
  a.fc = fc; a.truth = truth; a.chan = channels; a.wb = band_w; a.tw = twiddle;
  a.partial = static_cast<double*>(ws);
  a.fc_bs = fc_bs; a.truth_bs = truth_bs;
  a.C = C; a.Cs = Cs; a.H = H; a.W = W; a.R = R; a.G = G; a.NR = spectrum_flight_rows(W);
  a.plan = plan;
  hipStream_t st = (hipStream_t)stream;
  if (lds > 64 * 1024 && spectrum_lds_once.first()) {
    for (const void* k : {reinterpret_cast<const void*>(spectrum_kernel<true>),
                          reinterpret_cast<const void*>(spectrum_kernel<false>)}) {
      const hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize,
                                               (int)(SPECTRUM_LDS - SPECTRUM_LDS_STATIC));
      if (e != hipSuccess) {
        paradis_set_error("spectrum_update: cannot raise the LDS limit: %s", hipGetErrorString(e));
        return 2;
      }
    }
  }
  if (tw_lds) hipLaunchKernelGGL(spectrum_kernel<true>, dim3((unsigned)blocks), dim3(SPECTRUM_THREADS), lds, st, a);
  else hipLaunchKernelGGL(spectrum_kernel<false>, dim3((unsigned)blocks), dim3(SPECTRUM_THREADS), lds, st, a);
  const int K1 = W / 2 + 1;
  const int64_t n = (int64_t)Cs * R * K1;
  hipLaunchKernelGGL(spectrum_finish_kernel, dim3((unsigned)ceil_div64(n, 256)), dim3(256), 0, st, a.partial, band_wsum,
                     acc, count, B, Cs, G, R, K1);
  PD_CHECK_LAUNCH("spectrum_update");
  return 0;
}
