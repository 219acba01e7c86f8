// The quantile climatology of a device-resident store: per slot, channel and grid cell the quantiles of the store rows
// that climatology.ClimPlan assigns to the slot - the per-cell thresholds of the event tables (an anomaly source against
// a quantile field at threshold 0 decides x >= q).  The lists are clim_mean's CSR lists, without the weights.
//
// Definition (the project's own; numpy's method="linear" position rule with the plain lerp).  The values x[rows[j],
// cols[c], p] of the slot's entries, -0.0 read as +0.0, NaN / +-Inf skipped (the rule of clim_mean); m of them are kept,
// v[0] <= .. <= v[m-1] ascending.  For a level q in [0, 1]:
//   pos = q * (m - 1),  lo = floor(pos),  hi = min(lo + 1, m - 1),  frac = pos - lo
//   out = (float)(v[lo] + (v[hi] - v[lo]) * frac)      all in double, one rounding;  NaN when m < min_count
// -ffp-contract=off: a packed value is decoded to the bits paradis_unpack_planes gives (store_reader.h), and the
// interpolation is mul, sub, mul, add as the numpy restatement (tests/quantile_oracle.py) writes it.
//
// N*C*P*(4 | 2) B read, Q*K*C*P*4 B written; the work is the sort in LDS.  No atomics, no zero fill: bit-identical run
// to run.
//
// The SEEPS climatology (paradis_clim_seeps[_packed]) is the same fill and the same sort with another stage behind them
// (QT_SELECT_SEEPS, a compile-time choice of the one kernel).  With dry a finite float32 and wet_level in [0, 1]:
//   n_dry = #{ v[i] < dry }  (strict: the lower bound of key(dry) among the sorted keys),  n_wet = m - n_dry
//   p1  = (float)((double)n_dry / (double)m)                                      NaN when m < min_count
//   pos = wet_level * (n_wet - 1),  lo = floor(pos),  hi = min(lo + 1, n_wet - 1),  frac = pos - lo
//   thr = (float)(v[n_dry + lo] + (v[n_dry + hi] - v[n_dry + lo]) * frac)         NaN when n_wet < 1 or m < min_count
// out is [2, K, C, P]: plane 0 p1, plane 1 thr.  tests/seeps_oracle.py restates it.
#include "common.h"
#include "store_reader.h"

#include <cmath>

#pragma clang fp contract(off)

namespace {

// One workgroup owns `cells` adjacent cells of ONE (slot, channel) plane and holds their keys in LDS as
// key[entry][cell]: lanes of consecutive cells hit consecutive banks when the tile is filled, in every compare-exchange
// and in the selection.  npad = the power of two at or above the longest list; cells = the largest power of two whose
// cells * npad keys fit QT_LDS_BYTES, at most QT_MAX_CELLS - 64 cells from 129 to 512 entries, 8 at 4096 - or, for
// short lists, QT_WIDE_BYTES, at most QT_WIDE_CELLS: 1024 cells up to 16 entries, 512 at 32, 128 at 128.  (A 64-cell tile of a
// four-entry list is 1 KiB of work, and a launch of such workgroups is bound by the rate at which they start.)  A
// list's own length (workgroup-uniform) decides how far the tile is filled and sorted: npk = the power of two at or
// above it.
constexpr int QT_THREADS = 256, QT_ROWS = 4, QT_MAX_CELLS = 64, QT_MAX_ENTRIES = 4096, QT_MAX_LEVELS = 8;
constexpr int QT_LDS_BYTES = 128 * 1024, QT_WIDE_CELLS = 1024, QT_WIDE_BYTES = 64 * 1024;
constexpr uint32_t QT_MISSING = 0xffffffffu;   // the image of a NaN pattern: above every finite value's key

// what the stage behind the sort computes; its parameters travel in QtLevels either way
constexpr int QT_SELECT_LEVELS = 0;   // lv.q[0 .. Q): the levels; out [Q, K, C, P]
constexpr int QT_SELECT_SEEPS = 1;    // lv.q[0] = wet_level, lv.q[1] = (double)dry (exact); Q = 2 planes: out [2, K, C, P]

struct QtLevels {
  double q[QT_MAX_LEVELS];
};

int qt_npad(int max_entries) {
  int n = 1;
  while (n < max_entries) n <<= 1;
  return n;
}
int qt_cells_log2(int npad) {
  int lg = 0;
  while ((2 << lg) <= QT_MAX_CELLS && (int64_t)(2 << lg) * npad * 4 <= QT_LDS_BYTES) ++lg;
  while ((2 << lg) <= QT_WIDE_CELLS && (int64_t)(2 << lg) * npad * 4 <= QT_WIDE_BYTES) ++lg;
  return lg;
}

// order-preserving key of a finite value (unsigned compare == float compare, -0.0 as +0.0); QT_MISSING otherwise
__device__ __forceinline__ uint32_t qt_key(float v) {
  const uint32_t b = __float_as_uint(v);
  if ((b & 0x7f800000u) == 0x7f800000u) return QT_MISSING;
  if ((b << 1) == 0u) return 0x80000000u;
  return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ __forceinline__ double qt_value(uint32_t k) {
  return (double)__uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xffffffffu));
}

constexpr int QT_BLOCK = 16, QT_PAIRS = 4;

__device__ __forceinline__ void qt_cx(uint32_t& a, uint32_t& b, bool up) {
  const uint32_t lo = a < b ? a : b, hi = a < b ? b : a;
  a = up ? lo : hi;
  b = up ? hi : lo;
}

// One step (span, j) of the network over the whole tile: compare-exchange i = (pair, cell), cell-minor.  A thread reads
// QT_PAIRS of its pairs before it writes the first (the pairs of a step are disjoint).
__device__ __forceinline__ void qt_pair_step(uint32_t* __restrict__ key, int cells_log2, int npk, int span, int j,
                                             int tid) {
  const int cells = 1 << cells_log2, n_cx = (npk >> 1) << cells_log2, dj = j << cells_log2;
  for (int i0 = tid; i0 < n_cx; i0 += QT_THREADS * QT_PAIRS) {
    uint32_t x[QT_PAIRS], y[QT_PAIRS];
    int ia[QT_PAIRS];
#pragma unroll
    for (int u = 0; u < QT_PAIRS; ++u) {
      const int i = i0 + u * QT_THREADS;
      if (i < n_cx) {
        const int cell = i & (cells - 1), p = i >> cells_log2;
        const int a = ((p & ~(j - 1)) << 1) | (p & (j - 1));
        ia[u] = (a << cells_log2) + cell;
        x[u] = key[ia[u]];
        y[u] = key[ia[u] + dj];
      }
    }
#pragma unroll
    for (int u = 0; u < QT_PAIRS; ++u) {
      if (i0 + u * QT_THREADS < n_cx) {
        const bool up = ((ia[u] >> cells_log2) & span) == 0;
        if (up ? x[u] > y[u] : x[u] < y[u]) {
          key[ia[u]] = y[u];
          key[ia[u] + dj] = x[u];
        }
      }
    }
  }
}

// The steps of distance j < QT_BLOCK of `span`, in registers: a thread owns the QT_BLOCK adjacent entries `base ..` of
// one cell.  WHOLE (span == QT_BLOCK): every span up to QT_BLOCK, i.e. the block comes out sorted, upwards where
// (base & QT_BLOCK) == 0.  Needs npk >= QT_BLOCK.
template <bool WHOLE>
__device__ __forceinline__ void qt_block_steps(uint32_t* __restrict__ key, int cells_log2, int npk, int span, int tid) {
  const int cells = 1 << cells_log2, n_blocks = (npk / QT_BLOCK) << cells_log2;
  for (int i = tid; i < n_blocks; i += QT_THREADS) {
    const int cell = i & (cells - 1), base = (i >> cells_log2) * QT_BLOCK;
    uint32_t* col = key + ((size_t)base << cells_log2) + cell;
    uint32_t v[QT_BLOCK];
#pragma unroll
    for (int r = 0; r < QT_BLOCK; ++r) v[r] = col[(size_t)r << cells_log2];
    if (WHOLE) {
#pragma unroll
      for (int s = 2; s < QT_BLOCK; s <<= 1)
#pragma unroll
        for (int j = s >> 1; j > 0; j >>= 1)
#pragma unroll
          for (int r = 0; r < QT_BLOCK; ++r)
            if ((r & j) == 0) qt_cx(v[r], v[r | j], (r & s) == 0);
    }
    const bool up = (base & span) == 0;
#pragma unroll
    for (int j = QT_BLOCK >> 1; j > 0; j >>= 1)
#pragma unroll
      for (int r = 0; r < QT_BLOCK; ++r)
        if ((r & j) == 0) qt_cx(v[r], v[r | j], up);
#pragma unroll
    for (int r = 0; r < QT_BLOCK; ++r) col[(size_t)r << cells_log2] = v[r];
  }
}

// VEC: P % 4 == 0, cells % 4 == 0 and the store Quad-aligned - a thread fills four adjacent cells of an entry with one
// 16 B / 8 B load and one 16 B LDS write; otherwise one cell, scalar.  The same keys either way.
// Fill: the items (entry, unit) of the tile, unit-minor (a unit is a quad or a cell), are dealt to the threads in turn;
// QT_ROWS of a thread's items are in flight in front of the LDS writes.  (Entry-uniform waves, as in clim_mean, would
// leave a 64-cell tile one row per wave-load; here a wave's load covers 64 / units rows, and rows[] and a packed
// plane's (lo, s) are same-address loads.)
template <class Reader, bool VEC, int SELECT>
__global__ void __launch_bounds__(QT_THREADS)
clim_quantile_kernel(const Reader store, int64_t T, int F, int64_t P, const int64_t* __restrict__ ptr,
                     const int64_t* __restrict__ rows, int64_t N, int k0, int K, const int* __restrict__ cols, int C,
                     int tiles, int cells_log2, int max_entries, const QtLevels lv, int Q, int min_count,
                     float* __restrict__ out, int* __restrict__ flag) {
  extern __shared__ uint32_t qt_keys[];
  uint32_t* __restrict__ key = qt_keys;
  const uint32_t blk = blockIdx.x, r = blk / (uint32_t)tiles;     // the grid is below 2^31: 32-bit divisions
  const int tile = (int)(blk - r * (uint32_t)tiles);
  const uint32_t kk = r / (uint32_t)C;
  const int c = (int)(r - kk * (uint32_t)C);
  const int64_t k = (int64_t)k0 + kk;
  const int f_raw = cols[c];
  const int f = f_raw < 0 ? 0 : (f_raw >= F ? F - 1 : f_raw);
  const int64_t b_raw = ptr[k], e_raw = ptr[k + 1];
  const int64_t jb = b_raw < 0 ? 0 : (b_raw > N ? N : b_raw);
  const int64_t je = e_raw < jb ? jb : (e_raw > N ? N : e_raw);
  bool clamped = f != f_raw || jb != b_raw || je != e_raw;
  int len = max_entries;
  if (je - jb <= (int64_t)max_entries) len = (int)(je - jb);
  else clamped = true;                                            // a list longer than the tile: its first max_entries
  int npk = 1;
  while (npk < len) npk <<= 1;                                    // <= npad: len <= max_entries <= npad
  const int cells = 1 << cells_log2, tid = threadIdx.x;
  const int64_t lo = (int64_t)tile << cells_log2;

  // ---- fill: item i = (entry, unit), unit-minor; a unit is a quad of cells (VEC) or one cell
  const int ulog = VEC ? cells_log2 - 2 : cells_log2;
  const int n_items = npk << ulog;
  for (int i0 = tid; i0 < n_items; i0 += QT_THREADS * QT_ROWS) {
    typename Reader::Plane pl[QT_ROWS];
    typename Reader::Quad qd[QT_ROWS];
    float sv[QT_ROWS];
#pragma unroll
    for (int i = 0; i < QT_ROWS; ++i) {
      const int it = i0 + i * QT_THREADS, idx = it >> ulog, u = it & ((1 << ulog) - 1);
      const int64_t cell0 = lo + (VEC ? 4 * u : u);               // (VEC: P % 4 == 0, quads are whole)
      if (idx < len && cell0 < P) {
        const int64_t row_raw = rows[jb + idx];
        const int64_t row = row_raw < 0 ? 0 : (row_raw >= T ? T - 1 : row_raw);
        clamped |= row != row_raw;
        pl[i] = store.plane(row * F + f, f, P);
        if (VEC) qd[i] = Reader::load_quad(pl[i], cell0);
        else sv[i] = Reader::value(pl[i], cell0);
      }
    }
#pragma unroll
    for (int i = 0; i < QT_ROWS; ++i) {
      const int it = i0 + i * QT_THREADS, idx = it >> ulog, u = it & ((1 << ulog) - 1);
      if (it < n_items) {
        const int cu = VEC ? 4 * u : u;
        const bool have = idx < len && lo + cu < P;               // cells past the plane and entries past the list
        uint32_t* d = key + ((size_t)idx << cells_log2) + cu;
        if (VEC) {
          uint4 kq = make_uint4(QT_MISSING, QT_MISSING, QT_MISSING, QT_MISSING);
          if (have) {
            const float4 v = Reader::quad_values(pl[i], qd[i]);
            kq = make_uint4(qt_key(v.x), qt_key(v.y), qt_key(v.z), qt_key(v.w));
          }
          *reinterpret_cast<uint4*>(d) = kq;                      // 16-byte aligned: cells % 4 == 0, cu % 4 == 0
        } else {
          *d = have ? qt_key(sv[i]) : QT_MISSING;
        }
      }
    }
  }
  if (clamped) *flag = 1;                                         // (every writer writes 1)
  __syncthreads();

  // ---- bitonic sort of the npk keys of every cell, ascending.  The steps of distance j < QT_BLOCK touch only the
  // QT_BLOCK adjacent entries of one cell: a thread takes such a block into registers and runs them all (qt_block_steps)
  // - the whole network up to span QT_BLOCK at first, then the last log2(QT_BLOCK) steps of every longer span -, so a
  // 256-entry tile is read and written 15 times instead of 36.  The steps of distance j >= QT_BLOCK go pair by pair.
  if (npk >= QT_BLOCK) {
    qt_block_steps<true>(key, cells_log2, npk, QT_BLOCK, tid);
    __syncthreads();
    for (int span = 2 * QT_BLOCK; span <= npk; span <<= 1) {
      for (int j = span >> 1; j >= QT_BLOCK; j >>= 1) {
        qt_pair_step(key, cells_log2, npk, span, j, tid);
        __syncthreads();
      }
      qt_block_steps<false>(key, cells_log2, npk, span, tid);
      __syncthreads();
    }
  } else {
    for (int span = 2; span <= npk; span <<= 1)
      for (int j = span >> 1; j > 0; j >>= 1) {
        qt_pair_step(key, cells_log2, npk, span, j, tid);
        __syncthreads();
      }
  }

  // ---- select: m = the position of the first missing key
  if constexpr (SELECT == QT_SELECT_LEVELS) {
    // thread (level, cell)
    const int n_sel = Q << cells_log2;
    for (int i = tid; i < n_sel; i += QT_THREADS) {
      const int cell = i & (cells - 1), qi = i >> cells_log2;
      if (lo + cell >= P) continue;
      const uint32_t* col = key + cell;
      int a = 0, b = npk;
      while (a < b) {
        const int mid = (a + b) >> 1;
        if (col[(size_t)mid << cells_log2] == QT_MISSING) b = mid;
        else a = mid + 1;
      }
      const int m = a;
      double q = lv.q[0];
#pragma unroll
      for (int j = 1; j < QT_MAX_LEVELS; ++j)
        if (qi == j) q = lv.q[j];
      float o = __builtin_nanf("");
      if (m >= min_count) {                                         // min_count >= 1: m >= 1
        const double pos = q * (double)(m - 1), fl = floor(pos), frac = pos - fl;
        const int il = (int)fl, ih = il + 1 < m - 1 ? il + 1 : m - 1;
        const double vl = qt_value(col[(size_t)il << cells_log2]), vh = qt_value(col[(size_t)ih << cells_log2]);
        o = (float)(vl + (vh - vl) * frac);
      }
      out[(((int64_t)qi * K + k) * C + c) * P + lo + cell] = o;
    }
  } else {
    // thread cell: both planes.  n_dry = the position of the first key >= key(dry) among the m kept (a missing key is
    // above every finite value's, so the search needs no m)
    const double wet_level = lv.q[0];
    const uint32_t kdry = qt_key((float)lv.q[1]);
    for (int cell = tid; cell < cells; cell += QT_THREADS) {
      if (lo + cell >= P) continue;
      const uint32_t* col = key + cell;
      int a = 0, b = npk;
      while (a < b) {
        const int mid = (a + b) >> 1;
        if (col[(size_t)mid << cells_log2] == QT_MISSING) b = mid;
        else a = mid + 1;
      }
      const int m = a;
      a = 0, b = m;
      while (a < b) {
        const int mid = (a + b) >> 1;
        if (col[(size_t)mid << cells_log2] >= kdry) b = mid;
        else a = mid + 1;
      }
      const int n_dry = a, n_wet = m - n_dry;
      float p1 = __builtin_nanf(""), thr = __builtin_nanf("");
      if (m >= min_count) {                                         // min_count >= 1: m >= 1
        p1 = (float)((double)n_dry / (double)m);
        if (n_wet >= 1) {
          const double pos = wet_level * (double)(n_wet - 1), fl = floor(pos), frac = pos - fl;
          const int il = (int)fl, ih = il + 1 < n_wet - 1 ? il + 1 : n_wet - 1;
          const double vl = qt_value(col[(size_t)(n_dry + il) << cells_log2]);
          const double vh = qt_value(col[(size_t)(n_dry + ih) << cells_log2]);
          thr = (float)(vl + (vh - vl) * frac);
        }
      }
      const int64_t at = ((int64_t)k * C + c) * P + lo + cell;
      out[at] = p1;
      out[(int64_t)K * C * P + at] = thr;
    }
  }
}

PerDeviceOnce qt_lds_once;

// the argument checks and the launches of the four entry points.  set_select(lv): the checks of the stage's own
// parameters, behind the shared ones, and the fill of lv; Q: the planes of out
template <int SELECT, class Reader, class SetSelect>
int clim_quantile_launch(const char* name, const Reader& store, bool store_ok, bool store_vec, int64_t T, int F, int H,
                         int W, const int64_t* ptr, const int64_t* rows, int64_t N, int K, int max_entries,
                         const int* cols, int C, bool select_ok, int Q, SetSelect&& set_select, int min_count,
                         float* out, int* flag, void* stream) {
  PD_REQUIRE(T >= 1 && F >= 1 && H >= 1 && W >= 1 && K >= 0 && C >= 0, "%s: bad shape T=%lld F=%d H=%d W=%d K=%d C=%d",
             name, (long long)T, F, H, W, K, C);
  PD_REQUIRE(N >= 0, "%s: N=%lld list entries", name, (long long)N);
  PD_REQUIRE(Q >= 0 && Q <= QT_MAX_LEVELS, "%s: %d levels, at most %d go into one launch", name, Q, QT_MAX_LEVELS);
  PD_REQUIRE(max_entries >= 0 && max_entries <= QT_MAX_ENTRIES, "%s: max_entries=%d outside [0, %d]", name, max_entries,
             QT_MAX_ENTRIES);
  PD_REQUIRE(min_count >= 1, "%s: min_count=%d, at least 1", name, min_count);
  if (K == 0 || C == 0 || Q == 0) return 0;
  PD_REQUIRE(store_ok && ptr != nullptr && cols != nullptr && select_ok && out != nullptr && flag != nullptr,
             "%s: store, ptr, cols, %sout and flag pointers required", name, SELECT == QT_SELECT_LEVELS ? "q, " : "");
  PD_REQUIRE(N == 0 || rows != nullptr, "%s: rows required for %lld entries", name, (long long)N);
  QtLevels lv;
  for (int i = 0; i < QT_MAX_LEVELS; ++i) lv.q[i] = 0.0;
  const int rc = set_select(lv);
  if (rc != 0) return rc;
  const int64_t P = (int64_t)H * W;
  const int npad = qt_npad(max_entries), cells_log2 = qt_cells_log2(npad), cells = 1 << cells_log2;
  const int64_t tiles = ceil_div64(P, cells);
  const int64_t per_slot = (int64_t)C * tiles;
  constexpr int64_t GRID_LIMIT = (1ll << 31) - 1;
  PD_REQUIRE(tiles <= GRID_LIMIT && per_slot <= GRID_LIMIT, "%s: too large (%lld workgroups per slot)", name,
             (long long)per_slot);
  const size_t lds = (size_t)cells * npad * sizeof(uint32_t);
  const bool vec = P % 4 == 0 && cells % 4 == 0 && store_vec;
  if (lds > 64 * 1024 && qt_lds_once.first()) {                     // every instantiation, whichever asks first
#define QT_KERNELS_OF(R, V) reinterpret_cast<const void*>(clim_quantile_kernel<R, V, QT_SELECT_LEVELS>), \
                            reinterpret_cast<const void*>(clim_quantile_kernel<R, V, QT_SELECT_SEEPS>)
    const void* kernels[8] = {QT_KERNELS_OF(FloatPlanes, true), QT_KERNELS_OF(FloatPlanes, false),
                              QT_KERNELS_OF(PackedPlanes, true), QT_KERNELS_OF(PackedPlanes, false)};
#undef QT_KERNELS_OF
    for (const void* kn : kernels)
      if (hipFuncSetAttribute(kn, hipFuncAttributeMaxDynamicSharedMemorySize, QT_LDS_BYTES) != hipSuccess) {
        paradis_set_error("%s: cannot reserve LDS", name);
        return 2;
      }
  }
  const int64_t slots_per_launch = GRID_LIMIT / per_slot;
  for (int64_t k0 = 0; k0 < K; k0 += slots_per_launch) {
    const int64_t nk = K - k0 < slots_per_launch ? K - k0 : slots_per_launch;
    const dim3 grid((unsigned)(nk * per_slot)), block(QT_THREADS);
    if (vec)
      hipLaunchKernelGGL((clim_quantile_kernel<Reader, true, SELECT>), grid, block, lds, (hipStream_t)stream, store, T, F,
                         P, ptr, rows, N, (int)k0, K, cols, C, (int)tiles, cells_log2, max_entries, lv, Q, min_count, out,
                         flag);
    else
      hipLaunchKernelGGL((clim_quantile_kernel<Reader, false, SELECT>), grid, block, lds, (hipStream_t)stream, store, T,
                         F, P, ptr, rows, N, (int)k0, K, cols, C, (int)tiles, cells_log2, max_entries, lv, Q, min_count,
                         out, flag);
    PD_CHECK_LAUNCH(name);
  }
  return 0;
}

// the levels of paradis_clim_quantile[_packed]
auto qt_set_levels(const char* name, const double* q_host, int Q) {
  return [=](QtLevels& lv) -> int {
    for (int i = 0; i < Q; ++i) {
      PD_REQUIRE(q_host[i] >= 0.0 && q_host[i] <= 1.0, "%s: level %d is %g, outside [0, 1]", name, i, q_host[i]);
      lv.q[i] = q_host[i];
    }
    return 0;
  };
}

// the parameters of paradis_clim_seeps[_packed]
auto qt_set_seeps(const char* name, float dry, double wet_level) {
  return [=](QtLevels& lv) -> int {
    PD_REQUIRE(std::isfinite(dry), "%s: the dry threshold is %g, not finite", name, (double)dry);
    PD_REQUIRE(wet_level >= 0.0 && wet_level <= 1.0, "%s: wet_level is %g, outside [0, 1]", name, wet_level);
    lv.q[0] = wet_level;
    lv.q[1] = (double)dry;
    return 0;
  };
}

}  // namespace

extern "C" int paradis_clim_quantile_max_entries(void) { return QT_MAX_ENTRIES; }

extern "C" int paradis_clim_quantile_cells(int max_entries) {
  const int n = max_entries < 1 ? 1 : (max_entries > QT_MAX_ENTRIES ? QT_MAX_ENTRIES : max_entries);
  return 1 << qt_cells_log2(qt_npad(n));
}

extern "C" int paradis_clim_quantile(const float* store, int64_t T, int F, int H, int W, const int64_t* ptr,
                                     const int64_t* rows, int64_t N, int K, int max_entries, const int* cols, int C,
                                     const double* q_host, int Q, int min_count, float* out, int* flag, void* stream) {
  return clim_quantile_launch<QT_SELECT_LEVELS>("clim_quantile", FloatPlanes{store}, store != nullptr, aligned16(store),
                                                T, F, H, W, ptr, rows, N, K, max_entries, cols, C, q_host != nullptr, Q,
                                                qt_set_levels("clim_quantile", q_host, Q), min_count, out, flag, stream);
}

extern "C" int paradis_clim_quantile_packed(const uint16_t* codes, const float* params, const int* domain, int64_t T,
                                            int F, int H, int W, const int64_t* ptr, const int64_t* rows, int64_t N,
                                            int K, int max_entries, const int* cols, int C, const double* q_host, int Q,
                                            int min_count, float* out, int* flag, void* stream) {
  return clim_quantile_launch<QT_SELECT_LEVELS>("clim_quantile_packed", PackedPlanes{codes, params, domain},
                                                codes != nullptr && params != nullptr && domain != nullptr,
                                                aligned8(codes), T, F, H, W, ptr, rows, N, K, max_entries, cols, C,
                                                q_host != nullptr, Q, qt_set_levels("clim_quantile_packed", q_host, Q),
                                                min_count, out, flag, stream);
}

extern "C" int paradis_clim_seeps(const float* store, int64_t T, int F, int H, int W, const int64_t* ptr,
                                  const int64_t* rows, int64_t N, int K, int max_entries, const int* cols, int C,
                                  float dry, double wet_level, int min_count, float* out, int* flag, void* stream) {
  return clim_quantile_launch<QT_SELECT_SEEPS>("clim_seeps", FloatPlanes{store}, store != nullptr, aligned16(store), T,
                                               F, H, W, ptr, rows, N, K, max_entries, cols, C, true, 2,
                                               qt_set_seeps("clim_seeps", dry, wet_level), min_count, out, flag, stream);
}

extern "C" int paradis_clim_seeps_packed(const uint16_t* codes, const float* params, const int* domain, int64_t T, int F,
                                         int H, int W, const int64_t* ptr, const int64_t* rows, int64_t N, int K,
                                         int max_entries, const int* cols, int C, float dry, double wet_level,
                                         int min_count, float* out, int* flag, void* stream) {
  return clim_quantile_launch<QT_SELECT_SEEPS>("clim_seeps_packed", PackedPlanes{codes, params, domain},
                                               codes != nullptr && params != nullptr && domain != nullptr,
                                               aligned8(codes), T, F, H, W, ptr, rows, N, K, max_entries, cols, C, true,
                                               2, qt_set_seeps("clim_seeps_packed", dry, wet_level), min_count, out, flag,
                                               stream);
}
