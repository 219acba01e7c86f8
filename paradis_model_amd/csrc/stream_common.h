// Streaming reductions: one layout ("Streaming reductions: one layout").  Included after common.h by
// the memory-bound "read once, reduce in a fixed order" units: score.hip, stats.hip, clip.hip, verify.hip, and by
// train.hip for the chunk table and the wave sum.  It holds the constants, the wave sum, the four-wave fold, the chunk
// table decoder, the quad loader and the chunk walk of clip.hip.
//
// The layout.  A workgroup of 256 threads owns one piece of one tensor: a chunk (tensor, offset) of a chunk table - at
// most TABLE_CHUNK elements, many tensors per launch - or piece j of PLANE_PIECE cells of one [H, W] plane.  Thread t
// handles the quads at cells 4 (256 i + t) .. + 3 of its piece, i = 0, 1, .., in that order, and inside a quad the cells
// k = 0 .. 3 in that order: a thread's additions are strictly sequential.  A quad is one 16-byte load where it is whole
// and 16-byte aligned (VEC) and four scalar loads that give +0 past the end otherwise; both give the same bits, so the
// choice (per workgroup for chunks, whose starts DDP's bucket views leave only 4-byte aligned; per launch, on the host,
// for planes) never shows in a result.  The unit says where fp32 ends and fp64 begins; from there on everything is
// double.  A wave is summed by the xor tree o = 32, 16, .., 1 (v += v[lane ^ o]), lane 0 of each of the four waves
// writes to LDS, and the workgroup's sum is (r0 + r1) + (r2 + r3), written by one ordinary store per sum.  A finishing
// kernel of the unit folds these partials in a fixed order.  No atomics anywhere: bit-identical run to run.
//
// The chunk table.  chunk_tensor[b], chunk_off[b]: workgroup b works on elements [off, off + n) of tensor t, n =
// min(TABLE_CHUNK, numel[t] - off); the tensors' addresses come in rows of T int64 (row r of tensor t at ptrs[r T + t]),
// which the host rewrites before every launch through a pinned staging row (paradis_model_amd/_tables.py), an
// address of 0 meaning "absent" where the unit allows it.
#pragma once
#include <type_traits>

constexpr int TABLE_CHUNK = 32768;                       // elements of one tensor per workgroup: 32 quads per thread
constexpr int TABLE_ITERS = TABLE_CHUNK / (256 * 4);
constexpr int PLANE_PIECE = 8192;                        // cells of one plane per workgroup: 8 quads per thread, tensor
constexpr int PLANE_ITERS = PLANE_PIECE / (256 * 4);

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// the lanes of the wave for which p holds: the integer counting of events.hip, fss.hip and ensemble.hip
__device__ __forceinline__ unsigned count_lanes(bool p) { return (unsigned)__popcll(__ballot(p)); }

// the four waves of a 256-thread workgroup: s[j] is this wave's sum j (after the xor tree); thread j < NS gets the
// workgroup's sum j handed to store(j, sum)
template <class T, int NS, class Store>
__device__ __forceinline__ void block_fold4(const T (&s)[NS], Store&& store) {
  __shared__ T red[NS][4];
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int j = 0; j < NS; ++j) red[j][threadIdx.x >> 6] = s[j];
  }
  __syncthreads();
  if (threadIdx.x < NS) {
    const T* r = red[threadIdx.x];
    store((int)threadIdx.x, (r[0] + r[1]) + (r[2] + r[3]));
  }
}

// entry blockIdx.x of a chunk table: tensor t, offset off, length n; a bad entry gives n = 0 (workgroup-uniform)
struct TableChunk {
  int t;
  int64_t off;
  int n;
};
__device__ __forceinline__ TableChunk table_chunk(const int64_t* __restrict__ numel, const int* __restrict__ chunk_tensor,
                                                  const int64_t* __restrict__ chunk_off, int T) {
  TableChunk c;
  c.t = chunk_tensor[blockIdx.x];
  c.off = chunk_off[blockIdx.x];
  const int64_t left = (c.t >= 0 && c.t < T && c.off >= 0) ? numel[c.t] - c.off : 0;
  c.n = (int)(left < (int64_t)TABLE_CHUNK ? (left > 0 ? left : 0) : (int64_t)TABLE_CHUNK);
  return c;
}

// four cells of x starting at q0, +0 past n; VEC: the quad is whole and 16-byte aligned.  (A sum that starts at +0 is
// never -0, so adding the +0 cells changes no bit.)
template <bool VEC, class Idx>
__device__ __forceinline__ void load_quad(const float* __restrict__ x, Idx q0, Idx n, float (&v)[4]) {
  if (VEC) {
    const float4 q = *reinterpret_cast<const float4*>(x + q0);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = q0 + k < n ? x[q0 + k] : 0.f;
  }
}

// The chunk walk of clip.hip's two passes.  It hands the thread's running sum through the body BY VALUE
// (s = body(s, q0)): with a sum captured by reference LLVM unrolls the loop without its remainder loop and one 16-byte
// load is lost.  After touching it, compile clip.hip to assembly and compare with the previous build: the same
// instructions, 18 / 10 VGPRs, 5 + 4 flat_load_dwordx4 and 4 flat_store_dwordx4.  NoSums is the state of a pass that sums
// nothing.
struct NoSums {};

// iterations [first, last) of a chunk of n elements: s = body(s, q0) for this thread's quad of each
template <class S, class Body>
__device__ __forceinline__ S walk_chunk_iters(int first, int last, int n, S s, Body&& body) {
  // (the loop vectorizer would interleave two iterations and break the 16-byte accesses into 4-byte ones)
#pragma clang loop vectorize(disable) interleave(disable) unroll_count(4)
  for (int i = first; i < last; ++i) {
    const int q0 = 4 * (256 * i + (int)threadIdx.x);
    if (q0 >= n) break;
    s = body(s, q0);
  }
  return s;
}
// a whole chunk: s = body(std::true_type, s, q0) over the iterations whose 256 quads are all whole (1024 cells each)
// when `aligned`, then s = body(std::false_type, s, q0) over the rest
template <class S, class Body>
__device__ __forceinline__ S walk_chunk(bool aligned, int n, S s, Body&& body) {
  const int whole = aligned ? n / 1024 : 0;
  s = walk_chunk_iters(0, whole, n, s, [&](S a, int q0) { return body(std::true_type{}, a, q0); });
  return walk_chunk_iters(whole, TABLE_ITERS, n, s, [&](S a, int q0) { return body(std::false_type{}, a, q0); });
}

// Not here, on purpose: the loops of stats.hip (three tensors per quad), score.hip and verify.hip (plane pieces).
// Written over a shared walk with the per-quad or per-cell body passed in, hipcc compiled them to other code than the
// loops written out - stats.hip to half the registers and other loads under the pragmas above, the plane kernels with
// the division by W repeated in every unrolled iteration, 1 - 1.5 % slower at 721x1440 - so each keeps its loop, in the
// thread order stated at the top, over load_quad and the constants.
