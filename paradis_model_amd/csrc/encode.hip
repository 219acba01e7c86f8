// f5, the writer's side: one pass over a flushed forecast chunk [B, n, C, H, W] (physical units, model channel order)
// and its dew-point chunk [B, n, L, H, W] that writes the layout the reference's writer hands to its region write -
// named variables [B, n_td, L_v, H, W], the model's channels regrouped by fancy indexing, the dropped channels left
// out (reference utils/file_output.py:66-175) - with every value already through the BitRound filter of its encoding
// (utils/file_output.py:18-24,262-263).  The reference does all of this on the CPU in numpy, several passes per state.
//
// BitRound is a bit operation on the float32 pattern, in 32-bit unsigned arithmetic, for any input (NaN, infinities
// and denormals included; a carry out of the mantissa rounds the exponent up, out of the exponent into the sign):
//   maskbits = 23 - keepbits;  b += ((b >> maskbits) & 1) + ((1 << (maskbits - 1)) - 1);  b &= 0xFFFFFFFF << maskbits
// - round to nearest, ties to the even kept bit.  This restates numcodecs' published BitRound.encode; numcodecs is not
// a dependency of this project and the restatement is NOT pinned against the package (no golden file holds its
// output).  keepbits = 23 keeps every mantissa bit: the bits are copied unchanged, as with the filter off.
//
// Memory-bound streaming, no reductions, no LDS: 8 B of HBM traffic per value.  A workgroup walks segments of
// EN_CHUNK = EN_THREADS * 4 * EN_UNROLL values of ONE output plane in a grid-stride loop, so the table row, the sample,
// the time slot and both plane addresses are wave-uniform (one table lookup per segment, scalar loads) and a lane has
// EN_UNROLL 16-byte loads in flight.  The source is never written; nothing outside the addressed time slots is written.
#include "common.h"

namespace {

constexpr int EN_THREADS = 256, EN_UNROLL = 2, EN_CHUNK = EN_THREADS * 4 * EN_UNROLL;

struct EncodeArgs {
  const uint32_t* chunk;
  const uint32_t* dew;
  uint32_t* out;
  const paradis_encode_plane_t* planes;
  int64_t chunk_bs, chunk_ts, dew_bs, dew_ts, P;
  uint32_t segs, chunks, n_planes, n;   // segs = B * n * n_planes * chunks < 2^31
  int B, n_td, td_off;
  uint32_t maskbits;                    // 0: copy
};

__device__ __forceinline__ uint32_t bitround(uint32_t b, uint32_t maskbits) {
  if (maskbits == 0) return b;
  b += ((b >> maskbits) & 1u) + ((1u << (maskbits - 1)) - 1u);
  return b & (0xFFFFFFFFu << maskbits);
}

// V = 4: P % 4 == 0, 16-byte aligned bases and strides that are multiples of four floats; V = 1: the scalar path, the
// same arithmetic per value
template <int V>
__global__ void __launch_bounds__(EN_THREADS) forecast_encode_kernel(EncodeArgs a) {
  for (uint32_t seg = blockIdx.x; seg < a.segs; seg += gridDim.x) {
    const uint32_t r = seg / a.chunks, chunk = seg - r * a.chunks;
    const uint32_t s = r / a.n_planes, plane = r - s * a.n_planes;    // s = b * n + t
    const uint32_t b = s / a.n, t = s - b * a.n;
    const paradis_encode_plane_t e = a.planes[plane];
    const uint32_t* __restrict__ src =
        e.src >= 0 ? a.chunk + (int64_t)b * a.chunk_bs + (int64_t)t * a.chunk_ts + (int64_t)e.src * a.P
                   : a.dew + (int64_t)b * a.dew_bs + (int64_t)t * a.dew_ts + (int64_t)(-1 - e.src) * a.P;
    // variable block [B, n_td, levels, P] behind the blocks of the `first` planes per (sample, slot) in front of it
    const int64_t row = (int64_t)e.first * a.B * a.n_td + ((int64_t)b * a.n_td + a.td_off + t) * e.levels + e.level;
    uint32_t* __restrict__ dst = a.out + row * a.P;
    const int64_t lo = (int64_t)chunk * EN_CHUNK;
    const int64_t hi = lo + EN_CHUNK < a.P ? lo + EN_CHUNK : a.P;
    if (V == 4) {
      uint4 q[EN_UNROLL];
#pragma unroll
      for (int u = 0; u < EN_UNROLL; ++u) {
        const int64_t i = lo + (int64_t)(u * EN_THREADS + threadIdx.x) * 4;
        if (i < hi) q[u] = *reinterpret_cast<const uint4*>(src + i);
      }
#pragma unroll
      for (int u = 0; u < EN_UNROLL; ++u) {
        const int64_t i = lo + (int64_t)(u * EN_THREADS + threadIdx.x) * 4;
        if (i < hi) {
          uint4 o;
          o.x = bitround(q[u].x, a.maskbits);
          o.y = bitround(q[u].y, a.maskbits);
          o.z = bitround(q[u].z, a.maskbits);
          o.w = bitround(q[u].w, a.maskbits);
          *reinterpret_cast<uint4*>(dst + i) = o;
        }
      }
    } else {
      for (int64_t i = lo + threadIdx.x; i < hi; i += EN_THREADS) dst[i] = bitround(src[i], a.maskbits);
    }
  }
}

}  // namespace

extern "C" int paradis_forecast_encode(const float* chunk, int64_t chunk_bs, int64_t chunk_ts, const float* dew,
                                       int64_t dew_bs, int64_t dew_ts, const paradis_encode_plane_t* planes,
                                       const paradis_encode_plane_t* planes_host, int n_planes, float* out,
                                       int64_t out_elems, int B, int n, int C, int L, int H, int W, int n_td,
                                       int td_off, int keepbits, void* stream) {
  PD_REQUIRE(B >= 0 && n >= 1 && C >= 1 && L >= 0 && H >= 1 && W >= 1,
             "forecast_encode: bad shape B=%d n=%d C=%d L=%d H=%d W=%d", B, n, C, L, H, W);
  PD_REQUIRE(keepbits >= 0 && keepbits <= 23, "forecast_encode: keepbits=%d must be 1..23, or 0 for no rounding",
             keepbits);
  PD_REQUIRE(td_off >= 0 && n_td >= 1 && (int64_t)td_off + n <= n_td,
             "forecast_encode: time slots [%d, %d + %d) do not fit the %d slots of a block", td_off, td_off, n, n_td);
  const int64_t P = (int64_t)H * W;
  PD_REQUIRE(P * C < (1ll << 31) && P * (L > 0 ? L : 1) < (1ll << 31),
             "forecast_encode: a state of %d x %d x %d cells is too large", C, H, W);
  PD_REQUIRE(chunk_ts >= P * C && chunk_bs >= (int64_t)(n - 1) * chunk_ts + P * C,
             "forecast_encode: chunk strides shorter than a state (time %lld, batch %lld, state %lld)",
             (long long)chunk_ts, (long long)chunk_bs, (long long)(P * C));
  PD_REQUIRE(dew == nullptr || (L >= 1 && dew_ts >= P * L && dew_bs >= (int64_t)(n - 1) * dew_ts + P * L),
             "forecast_encode: dew strides shorter than a state of %d levels (time %lld, batch %lld)", L,
             (long long)dew_ts, (long long)dew_bs);
  PD_REQUIRE(planes != nullptr && planes_host != nullptr && n_planes >= 1 && n_planes < (1 << 20),
             "forecast_encode: plane table required (device and host copy, 1 .. 2^20 - 1 rows)");
  int64_t slot_planes = 0;      // planes of all variables per (sample, time slot)
  for (int i = 0; i < n_planes; ++i) {
    const paradis_encode_plane_t& e = planes_host[i];
    PD_REQUIRE(e.src >= 0 ? e.src < C : (dew != nullptr && -1 - (int64_t)e.src < L),
               "forecast_encode: table row %d reads %s %lld, outside the source", i,
               e.src >= 0 ? "channel" : "dew level", (long long)(e.src >= 0 ? e.src : -1 - (int64_t)e.src));
    PD_REQUIRE(e.first >= 0 && e.levels >= 1 && e.level >= 0 && e.level < e.levels,
               "forecast_encode: table row %d has a bad destination (first %d, level %d of %d)", i, e.first, e.level,
               e.levels);
    slot_planes = std::max<int64_t>(slot_planes, (int64_t)e.first + e.levels);
  }
  PD_REQUIRE(out_elems >= (int64_t)B * n_td * slot_planes * P,
             "forecast_encode: the encoded buffer has %lld elements, B * n_td * %lld planes * H * W = %lld are addressed",
             (long long)out_elems, (long long)slot_planes, (long long)((int64_t)B * n_td * slot_planes * P));
  if (B == 0) return 0;
  PD_REQUIRE(chunk != nullptr && out != nullptr, "forecast_encode: null pointer");
  const int64_t chunks = ceil_div64(P, EN_CHUNK);
  const int64_t segs = (int64_t)B * n * n_planes * chunks;
  PD_REQUIRE(segs < (1ll << 31), "forecast_encode: too large (%lld segments)", (long long)segs);
  EncodeArgs a;
  a.chunk = reinterpret_cast<const uint32_t*>(chunk);
  a.dew = reinterpret_cast<const uint32_t*>(dew);
  a.out = reinterpret_cast<uint32_t*>(out);
  a.planes = planes;
  a.chunk_bs = chunk_bs; a.chunk_ts = chunk_ts; a.dew_bs = dew_bs; a.dew_ts = dew_ts; a.P = P;
  a.segs = (uint32_t)segs; a.chunks = (uint32_t)chunks; a.n_planes = (uint32_t)n_planes; a.n = (uint32_t)n;
  a.B = B; a.n_td = n_td; a.td_off = td_off;
  a.maskbits = keepbits == 0 ? 0u : (uint32_t)(23 - keepbits);
  const bool vec = P % 4 == 0 && aligned16(chunk) && aligned16(out) && chunk_bs % 4 == 0 && chunk_ts % 4 == 0 &&
                   (dew == nullptr || (aligned16(dew) && dew_bs % 4 == 0 && dew_ts % 4 == 0));
  const unsigned blocks = (unsigned)std::min<int64_t>(segs, 8192);
  if (vec) hipLaunchKernelGGL(forecast_encode_kernel<4>, dim3(blocks), dim3(EN_THREADS), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(forecast_encode_kernel<1>, dim3(blocks), dim3(EN_THREADS), 0, (hipStream_t)stream, a);
  PD_CHECK_LAUNCH("forecast_encode");
  return 0;
}
