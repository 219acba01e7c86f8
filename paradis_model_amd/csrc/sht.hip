// AMSE spectral loss (reference utils/amse_loss.py, Subich et al. 2025) on the equiangular grid H x W, W = 2(H-1):
//   1. longitude DFT       x[n, j, i] -> X[m][j][(s, re/im, n)]       GEMM on the f32 MFMA against a twiddle table
//   2. Legendre analysis   X[m] -> c[m][l >= m][(s, re/im, n)]         one GEMM per m over latitude, triangle only
//   3. spectral AMSE       PSDs, cross-spectra, coherence, per-scale terms (fp64), d loss / d c_pred in the same pass
//   4. finish              fixed-order mean over (k, n), NaN -> 1e6 with a zero-gradient flag
//   5. adjoint Legendre + adjoint DFT (want_grad): d loss / d pred
// s = 0 pred, 1 target; n = b * C + c; M = H - 1 = the number of degrees / orders AMSE reads (l, m < H - 1).
// Rows are taken as RealSHT takes them: row j of the tensor is colatitude pi * j / (H - 1).  Every reduction runs in a
// fixed order (no float atomics): the result is bit-reproducible.
#include <math.h>
#include "common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// sqrt(4 pi) / sqrt(4 pi) = 1 for the "backward" normalisation: orthonormal Legendre functions times sqrt(4 pi).  The
// global factor (every PSD and the loss scale by 4 pi) is restated, not pinned against torch_harmonics.
constexpr double SHT_NORM_FACTOR = 3.5449077018110320546;   // sqrt(4 pi)
constexpr double AMSE_EPS = 1e-7;

__host__ __device__ inline int64_t tri_rows(int64_t m, int64_t M) { return m * M - m * (m - 1) / 2; }

// ---- generic fp32 GEMM on v_mfma_f32_16x16x4_f32: C[z] (rows x cols) = A[z] (rows x depth) * B[z] (depth x cols) -----
// 64 x 64 tile per 256-thread workgroup (four waves of 32 x 32 = 2 x 2 MFMA blocks), depth step 16 through LDS.  The
// problem type P maps (z, i, k) / (z, k, j) to loads and (z, i, j) to the store; A_KF / B_KF choose which index runs
// fastest across the threads that stage a tile (the one that is contiguous in memory).
constexpr int TM = 64, TN = 64, TK = 16;

template <class P, bool A_KF, bool B_KF>
__global__ void __launch_bounds__(256) sht_gemm_kernel(P p) {
  const int z = blockIdx.z;
  const int rows = p.rows(z), cols = p.cols(z), depth = p.depth(z);
  const int i0 = blockIdx.y * TM, j0 = blockIdx.x * TN;
  if (i0 >= rows || j0 >= cols) return;     // (workgroup-uniform: the triangle's empty tiles)
  __shared__ float As[TK][TM + 4];
  __shared__ float Bs[TK][TN + 4];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int wi = (wv >> 1) * 32, wj = (wv & 1) * 32;
  f32x4 acc[2][2];
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int t = 0; t < 2; ++t) acc[s][t] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < depth; k0 += TK) {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int e = tid + 256 * t;
      const int ii = A_KF ? (e >> 4) : (e & 63), kk = A_KF ? (e & 15) : (e >> 6);
      const int gi = i0 + ii, gk = k0 + kk;
      As[kk][ii] = (gi < rows && gk < depth) ? p.a(z, gi, gk) : 0.f;
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int e = tid + 256 * t;
      const int jj = B_KF ? (e >> 4) : (e & 63), kk = B_KF ? (e & 15) : (e >> 6);
      const int gj = j0 + jj, gk = k0 + kk;
      Bs[kk][jj] = (gj < cols && gk < depth) ? p.b(z, gk, gj) : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < TK; kk += 4) {
      const int kq = kk + (lane >> 4);
      float av[2], bv[2];
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        av[s] = As[kq][wi + 16 * s + (lane & 15)];
        bv[s] = Bs[kq][wj + 16 * s + (lane & 15)];
      }
#pragma unroll
      for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int t = 0; t < 2; ++t) acc[s][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s], bv[t], acc[s][t], 0, 0, 0);
    }
    __syncthreads();
  }
  // D of a 16x16x4 block: column lane & 15, row 4 * (lane >> 4) + r
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int gi = i0 + wi + 16 * s + 4 * (lane >> 4) + r, gj = j0 + wj + 16 * t + (lane & 15);
        if (gi < rows && gj < cols) p.store(z, gi, gj, acc[s][t][r]);
      }
}

// 1. forward DFT, z = s: rows (c, m) [2M], cols (j, n) [H N], depth i [W].  X[m][j][(2 s + c) N + n]
struct DftFwd {
  const float* x[2];
  const float* tw;      // [W][2M]
  float* X;
  int N, H, W, M;
  __device__ int rows(int) const { return 2 * M; }
  __device__ int cols(int) const { return H * N; }
  __device__ int depth(int) const { return W; }
  __device__ float a(int, int i, int k) const { return tw[(int64_t)k * (2 * M) + i]; }
  __device__ float b(int z, int k, int col) const {
    const int j = col / N, n = col - j * N;
    return x[z][((int64_t)n * H + j) * W + k];
  }
  __device__ void store(int z, int i, int col, float v) const {
    const int c = i >= M, m = i - c * M, j = col / N, n = col - j * N;
    X[((int64_t)m * H + j) * (4 * N) + (2 * z + c) * N + n] = v;
  }
};

// 2. Legendre analysis, z = m: rows l - m [M - m], cols q [4N], depth j [H].  c[tri(m) + l - m][q]
struct LegFwd {
  const float* tab;     // [tri(M)][H]
  const float* X;
  float* coef;
  int N, H, M;
  __device__ int rows(int m) const { return M - m; }
  __device__ int cols(int) const { return 4 * N; }
  __device__ int depth(int) const { return H; }
  __device__ float a(int m, int l, int j) const { return tab[(tri_rows(m, M) + l) * H + j]; }
  __device__ float b(int m, int j, int q) const { return X[((int64_t)m * H + j) * (4 * N) + q]; }
  __device__ void store(int m, int l, int q, float v) const { coef[(tri_rows(m, M) + l) * (4 * N) + q] = v; }
};

// 4. adjoint Legendre, z = m: rows j [H], cols q [2N], depth l - m [M - m].  gX[m][j][q]
struct LegAdj {
  const float* tab;
  const float* gcoef;
  float* gX;
  int N, H, M;
  __device__ int rows(int) const { return H; }
  __device__ int cols(int) const { return 2 * N; }
  __device__ int depth(int m) const { return M - m; }
  __device__ float a(int m, int j, int l) const { return tab[(tri_rows(m, M) + l) * H + j]; }
  __device__ float b(int m, int l, int q) const { return gcoef[(tri_rows(m, M) + l) * (2 * N) + q]; }
  __device__ void store(int m, int j, int q, float v) const { gX[((int64_t)m * H + j) * (2 * N) + q] = v; }
};

// 5. adjoint DFT: rows (j, n) [H N], cols i [W], depth (c, m) [2M].  grad[n][j][i], zero where the loss was NaN
struct DftAdj {
  const float* gX;
  const float* tw;
  const float* flag;
  float* grad;
  int N, H, W, M;
  __device__ int rows(int) const { return H * N; }
  __device__ int cols(int) const { return W; }
  __device__ int depth(int) const { return 2 * M; }
  __device__ float a(int, int r, int kk) const {
    const int j = r / N, n = r - j * N, c = kk >= M, m = kk - c * M;
    return gX[((int64_t)m * H + j) * (2 * N) + c * N + n];
  }
  __device__ float b(int, int kk, int i) const { return tw[(int64_t)i * (2 * M) + kk]; }
  __device__ void store(int, int r, int i, float v) const {
    const int j = r / N, n = r - j * N;
    grad[((int64_t)n * H + j) * W + i] = flag[0] != 0.f ? v : 0.f;
  }
};

template <bool A_KF, bool B_KF, class P>
void launch_gemm(const P& p, int max_rows, int max_cols, int batches, hipStream_t st) {
  const dim3 grid((unsigned)((max_cols + TN - 1) / TN), (unsigned)((max_rows + TM - 1) / TM), (unsigned)batches);
  hipLaunchKernelGGL((sht_gemm_kernel<P, A_KF, B_KF>), grid, dim3(256), 0, st, p);
}

// ---- tables ----------------------------------------------------------------------------------------------------------
// colatitude cosines and Clenshaw-Curtis weights (Waldvogel's rule in its closed cosine form; the weights sum to 2)
__global__ void __launch_bounds__(256) cc_nodes_kernel(double* __restrict__ xw, int H) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= H) return;
  const int n1 = H - 1;
  const double th = M_PI * (double)j / (double)n1;
  double s = 0.0;
  for (int k = 1; k <= n1 / 2; ++k) {
    const double bk = (2 * k == n1) ? 1.0 : 2.0;
    s += bk * cos(2.0 * k * th) / (4.0 * k * k - 1.0);
  }
  const double cj = (j == 0 || j == n1) ? 1.0 : 2.0;
  xw[j] = cos(th);
  xw[H + j] = cj / n1 * (1.0 - s);
}

// one thread per (m, j): the three-term recurrence of torch_harmonics' legpoly in fp64 up the column l = m .. M-1,
// Condon-Shortley phase, times the quadrature weight; stored fp32 (values below fp32's range flush, as in the reference)
__global__ void __launch_bounds__(256) legendre_table_kernel(const double* __restrict__ xw, float* __restrict__ tab,
                                                             int H, int M) {
  const int j = blockIdx.x * 256 + threadIdx.x, m = blockIdx.y;
  if (j >= H) return;
  const double x = xw[j], w = xw[H + j] * ((m & 1) ? -1.0 : 1.0);
  const int64_t base = tri_rows(m, M);
  double pmm = SHT_NORM_FACTOR / sqrt(4.0 * M_PI);
  for (int l = 1; l <= m; ++l) pmm = sqrt((2.0 * l + 1) * (1 + x) * (1 - x) / 2 / l) * pmm;
  tab[base * H + j] = (float)(pmm * w);
  if (m + 1 >= M) return;
  double p0 = pmm, p1 = sqrt(2.0 * (m + 1) + 1) * x * pmm;
  tab[(base + 1) * H + j] = (float)(p1 * w);
  for (int l = m + 2; l < M; ++l) {
    const double a = x * sqrt((2.0 * l - 1) / (l - m) * (2.0 * l + 1) / (l + m));
    const double b = sqrt((double)(l + m - 1) / (l - m) * (2.0 * l + 1) / (2.0 * l - 3) * (double)(l - m - 1) / (l + m));
    const double p = a * p1 - b * p0;
    tab[(base + (l - m)) * H + j] = (float)(p * w);
    p0 = p1;
    p1 = p;
  }
}

// tw[i][(c, m)] = 2 pi / W * (cos, -sin)(2 pi m i / W), the phase reduced exactly (m i mod W) before the fp64 sincos
__global__ void __launch_bounds__(256) twiddle_kernel(float* __restrict__ tw, int W, int M) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)W * 2 * M) return;
  const int i = (int)(e / (2 * M)), col = (int)(e - (int64_t)i * 2 * M);
  const int c = col >= M, m = col - c * M;
  const double ang = 2.0 * M_PI * (double)(((int64_t)m * i) % W) / W;
  const double sc = 2.0 * M_PI / W;
  tw[e] = (float)(c ? -sc * sin(ang) : sc * cos(ang));
}

// ---- 3. spectral AMSE: one thread per (k, n), fp64 sums over m = 0 .. k --------------------------------------------
// psd = |c_k0|^2 + 2 sum_{m>=1} |c_km|^2 + eps ; X = conj(P_k0) T_k0 + 2 sum_{m>=1} conj(P_km) T_km
// coh = clamp(|X| / (sqrt(psdP psdT + eps) + eps), 0, 1) ; amse_k = (sqrt psdP - sqrt psdT)^2 + 2 max(psdP, psdT)(1 - coh)
// gradient (torch's conventions: a tie in max splits 1/2 - 1/2, clamp passes at both bounds, d|z| = 0 at z = 0) times
// gscale = 1 / (K N) into gcoef[tri(m) + k - m][(re/im, n)]
__global__ void __launch_bounds__(256)
amse_spectral_kernel(const float* __restrict__ coef, float* __restrict__ gcoef, double* __restrict__ amse_kn, int N,
                     int M, double gscale) {
  const int k = blockIdx.y, n = blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  const int64_t Q = 4 * (int64_t)N;
  double a = 0.0, b = 0.0, xr = 0.0, xi = 0.0;
  for (int m = 0; m <= k; ++m) {
    const float* c = coef + (tri_rows(m, M) + (k - m)) * Q + n;
    const double pr = c[0], pi = c[N], tr = c[2 * N], ti = c[3 * N], wt = m ? 2.0 : 1.0;
    a += wt * (pr * pr + pi * pi);
    b += wt * (tr * tr + ti * ti);
    xr += wt * (pr * tr + pi * ti);
    xi += wt * (pr * ti - pi * tr);
  }
  a += AMSE_EPS;
  b += AMSE_EPS;
  const double sa = sqrt(a), sb = sqrt(b), mx = a > b ? a : b;
  const double ax = sqrt(xr * xr + xi * xi), rt = sqrt(a * b + AMSE_EPS), den = rt + AMSE_EPS;
  const double rho = ax / den, coh = rho < 0.0 ? 0.0 : (rho > 1.0 ? 1.0 : rho);
  amse_kn[(int64_t)k * N + n] = (sa - sb) * (sa - sb) + 2.0 * mx * (1.0 - coh);
  if (gcoef == nullptr) return;
  const double dmax = a > b ? 1.0 : (a == b ? 0.5 : 0.0);
  const double grho = (rho >= 0.0 && rho <= 1.0) ? -2.0 * mx : 0.0;
  const double gax = grho / den, gden = -grho * ax / (den * den);
  const double ga = ((sa - sb) / sa + 2.0 * (1.0 - coh) * dmax + gden * b / (2.0 * rt)) * gscale;
  const double gxr = ax > 0.0 ? gax * xr / ax * gscale : 0.0, gxi = ax > 0.0 ? gax * xi / ax * gscale : 0.0;
  const int64_t G = 2 * (int64_t)N;
  for (int m = 0; m <= k; ++m) {
    const int64_t row = tri_rows(m, M) + (k - m);
    const float* c = coef + row * Q + n;
    const double pr = c[0], pi = c[N], tr = c[2 * N], ti = c[3 * N], wt = m ? 2.0 : 1.0;
    gcoef[row * G + n] = (float)(wt * (2.0 * ga * pr + gxr * tr + gxi * ti));
    gcoef[row * G + N + n] = (float)(wt * (2.0 * ga * pi + gxr * ti - gxi * tr));
  }
}

// ---- 4. the scalar: thread t sums n = t, t + 256, ... over k in order, then a fixed tree --------------------------
__global__ void __launch_bounds__(256)
amse_finish_kernel(const double* __restrict__ amse_kn, float* __restrict__ loss, float* __restrict__ flag, int N, int K) {
  __shared__ double red[256];
  double acc = 0.0;
  for (int n = threadIdx.x; n < N; n += 256) {
    double s = 0.0;
    for (int k = 0; k < K; ++k) s += amse_kn[(int64_t)k * N + n];
    acc += s;
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float v = (float)(red[0] / ((double)K * (double)N));   // N = 0: 0 / 0 = NaN, as torch.mean of nothing
    const bool bad = isnan(v);
    loss[0] = bad ? 1e6f : v;                                     // the reference's fallback value
    flag[0] = bad ? 0.f : 1.f;                                    // ... with a zero gradient
  }
}

struct Ws {
  float* X;        // [M][H][4N]; reused as gX [M][H][2N]
  float* coef;     // [tri(M)][4N]
  float* gcoef;    // [tri(M)][2N]
  double* amse;    // [K][N]
  float* flag;
};

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

size_t ws_layout(int N, int H, char* base, Ws* w) {
  const int64_t M = H - 1;
  const size_t bx = align256(sizeof(float) * (size_t)M * H * 4 * N);
  const size_t bc = align256(sizeof(float) * (size_t)tri_rows(M, M) * 4 * N);
  const size_t bg = align256(sizeof(float) * (size_t)tri_rows(M, M) * 2 * N);
  const size_t ba = align256(sizeof(double) * (size_t)M * N);
  if (w) {
    w->X = reinterpret_cast<float*>(base);
    w->coef = reinterpret_cast<float*>(base + bx);
    w->gcoef = reinterpret_cast<float*>(base + bx + bc);
    w->amse = reinterpret_cast<double*>(base + bx + bc + bg);
    w->flag = reinterpret_cast<float*>(base + bx + bc + bg + ba);
  }
  return bx + bc + bg + ba + 256;
}

bool grid_ok(int H, int W) { return H >= 3 && W == 2 * (H - 1) && H <= 4097; }

}  // namespace

extern "C" size_t paradis_amse_table_floats(int H) {
  if (H < 3) return 0;
  const int64_t M = H - 1;
  return (size_t)tri_rows(M, M) * H;
}

extern "C" size_t paradis_amse_tables_ws_bytes(int H) { return sizeof(double) * 2 * (size_t)(H > 0 ? H : 0); }

extern "C" int paradis_amse_tables(float* leg, float* twiddle, double* ws, int H, int W, void* stream) {
  PD_REQUIRE(grid_ok(H, W), "amse_tables: the equiangular transform needs W = 2*(H-1) and 3 <= H <= 4097 (got %dx%d)",
             H, W);
  PD_REQUIRE(leg && twiddle && ws, "amse_tables: buffers missing");
  const int M = H - 1;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(cc_nodes_kernel, dim3((H + 255) / 256), dim3(256), 0, st, ws, H);
  hipLaunchKernelGGL(legendre_table_kernel, dim3((H + 255) / 256, M), dim3(256), 0, st, ws, leg, H, M);
  const int64_t nt = (int64_t)W * 2 * M;
  hipLaunchKernelGGL(twiddle_kernel, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, st, twiddle, W, M);
  PD_CHECK_LAUNCH("amse_tables");
  return 0;
}

extern "C" size_t paradis_amse_ws_bytes(int N, int H) {
  if (N < 0 || H < 3) return 0;
  return ws_layout(N, H, nullptr, nullptr);
}

extern "C" int paradis_amse_loss(const float* pred, const float* target, const float* leg, const float* twiddle,
                                 float* loss, float* grad, void* ws, int N, int H, int W, void* stream) {
  PD_REQUIRE(grid_ok(H, W), "amse_loss: the equiangular transform needs W = 2*(H-1) and 3 <= H <= 4097 (got %dx%d)",
             H, W);
  PD_REQUIRE(N >= 0, "amse_loss: bad batch");
  PD_REQUIRE((int64_t)H * N <= (int64_t)65535 * TM, "amse_loss: B*C*H too large for one launch (%d x %d)", N, H);
  PD_REQUIRE(loss && ws && leg && twiddle, "amse_loss: buffers missing");
  PD_REQUIRE(N == 0 || (pred && target), "amse_loss: inputs missing");
  const int M = H - 1, K = M;
  hipStream_t st = (hipStream_t)stream;
  Ws w;
  ws_layout(N, H, static_cast<char*>(ws), &w);
  if (N > 0) {
    DftFwd d{{pred, target}, twiddle, w.X, N, H, W, M};
    launch_gemm<false, true>(d, 2 * M, H * N, 2, st);
    LegFwd f{leg, w.X, w.coef, N, H, M};
    launch_gemm<true, false>(f, M, 4 * N, M, st);
    hipLaunchKernelGGL(amse_spectral_kernel, dim3((N + 255) / 256, K), dim3(256), 0, st, w.coef,
                       grad ? w.gcoef : nullptr, w.amse, N, M, 1.0 / ((double)K * N));
  }
  hipLaunchKernelGGL(amse_finish_kernel, dim3(1), dim3(256), 0, st, w.amse, loss, w.flag, N, K);
  if (N > 0 && grad) {
    LegAdj g{leg, w.gcoef, w.X, N, H, M};
    launch_gemm<false, false>(g, H, 2 * N, M, st);
    DftAdj h{w.X, twiddle, w.flag, grad, N, H, W, M};
    launch_gemm<false, true>(h, H * N, W, 1, st);
  }
  PD_CHECK_LAUNCH("amse_loss");
  return 0;
}
