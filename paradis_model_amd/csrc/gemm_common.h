// What the five translation units of the pointwise GEMMs share: gemm.hip (the C ABI's GEMM entry points, the weight
// gradient's slab reduction), gemm_exact.hip (the f32-MFMA kernels and their tunables), gemm_split.hip (the split-operand
// kernels and the weight images' entry points), gemm_amp_fwd.hip and gemm_amp_wgrad.hip (the bf16-mixed scheme's forward /
// data-gradient and weight-gradient kernels).
// Arguments, tile constants, the epilogue, the split / round helpers, the one kernel template that two units instantiate
// (pw_gemm_wgrad_split_kernel), the launch helpers and - host only, at the end - the weight gradient's plan (wgrad_plan).
// Everything below the declarations sits in an anonymous namespace.
#pragma once
#include <algorithm>
#include <cstdlib>
#include <initializer_list>
#include <type_traits>
#include "common.h"

struct GemmArgs {
  const float* A; const float* B; float* C;
  int M, N, K;
  int64_t lda, ldb, ldc;
  int64_t a_bs, b_bs, c_bs;   // stride between grid batches (fwd/dgrad: sample; wgrad: split slab)
  int nbatch;                 // grid batches (fwd/dgrad: samples; wgrad: k-range splits)
  int inner;                  // wgrad: number of samples reduced (0 for fwd/dgrad)
  int64_t a_is, b_is;         // wgrad: strides between samples
  // epilogue:  v = acc (+bias[m]) (+map[m,n]); zout = v; v = zmul ? v*act'(zmul) : act(v);
  //            v = gate ? res + sigmoid(gate[m]) (v - res) : v + res
  const float* bias; const float* map; const float* res; const float* zmul; float* zout;
  const float* gate;          // [M] or NULL: the residual is blended in per output channel (gated blend of the advection)
  int64_t res_bs, zmul_bs, zout_bs;
  int act;
  int stagger;                // start-up skew between co-resident workgroups, in units of 512 cycles
  float* rowsum;              // wgrad only: [nbatch][M] partial row sums of A (= bias gradient), or NULL
  int generic_epilogue;       // split wgrad only: every tile ends in gemm_epilogue (PARADIS_GEMM_EPILOGUE=generic)
  // low-rank bias map applied on the fly: acc[m,n] += sum_c pw[c*M + m] * m8[c*N + n]  (M % 4 == 0)
  const float* m8; const float* pw; int cin;
  // f16x2 scheme: where the operands' max |value| comes from.  a_amax: one word (bits of max |A|, weight
  // image tail) for fwd/dgrad, PARADIS_AMAX_PARTIALS words for wgrad; b_amax: PARADIS_AMAX_PARTIALS words.
  const uint32_t* a_amax; const uint32_t* b_amax;
  // PARADIS_GEMM_BF16 only (round 6): which tensors are STORED as bf16 (2 bytes per element; strides stay in elements).
  // IO_B16: the activation operand B (fwd: X, dgrad: dY) - pw_gemm_b16_kernel stages it by LDS-DMA and reads it with
  // ds_read_b64_tr_b16; IO_C16: the output C (and zout); IO_ZM16: zmul.  Residual, bias and maps are always fp32.
  int io16;
  // (PARADIS_GEMM_BF16, the reference's bf16-mixed mode: the result is rounded to bf16 where the reference's autocast
  //  conv2d rounds it - the pre-activation and the activated value (fwd), the activation-gradient product (dgrad) -
  //  before the fp32 residual / blend; a compile-time property of pw_gemm_bf16_k32_kernel's epilogue.  Stored as fp32.)
};

// The weight-gradient kernels, one per schedule (wgrad_plan below picks one):
//   Staged  pw_gemm_kernel<true, true, BK>      f32 MFMA, operands staged through registers; any shape, no fused row sums
//   Dma     pw_gemm_wgrad_dma_kernel            f32 MFMA, LDS-DMA
//   Bf16x3  pw_gemm_wgrad_split_kernel<3>       six bf16 products          F16x2  pw_gemm_wgrad_split_kernel<2>
//   Amp128 / Tall / Square                      bf16-mixed scheme on a 128 x 128, 256 x 128, 256 x 256 tile
enum class WgradKind { Staged, Dma, Bf16x3, F16x2, Amp128, Tall, Square };
// the workspace: [S][M,K] slabs, then [S][M] row-sum partials (S = 1: the slab area is unused, the GEMM writes dW)
struct WgradWorkspace {
  int S, M, K;
  size_t rowsum_offset() const { return (size_t)S * M * K; }      // floats
  size_t bytes() const { return (size_t)S * M * ((size_t)K + 1) * sizeof(float) + 256; }
  float* rowsums(void* ws) const { return (float*)ws + rowsum_offset(); }
};

struct WgradPlan {
  WgradKind kind;
  int S;                  // K-range slabs = grid batches
  int grid, block;
  size_t lds;
  bool fused_rowsums;     // the kernel also sums the rows of dY per slab (else: a separate paradis_bias_grads pass)
  bool to_slabs;          // the GEMM writes S slabs for slab_reduce_kernel (else: dW itself)
  WgradWorkspace ws;
};

// gemm_exact.hip: its tunables by value, and its launchers (a_kc / b_kc: the operand is k-contiguous)
struct GemmTunables { int bk, wg_per_cu, stagger, dma_stages, wgrad_dma_stages; };
GemmTunables pd_exact_tunables();
int pd_exact_launch(bool a_kc, bool b_kc, const GemmArgs& g, int grid, hipStream_t st);
bool pd_exact_dma_eligible(const GemmArgs& g);
int pd_exact_launch_dma(const GemmArgs& g, int grid, hipStream_t st);
int pd_exact_launch_wgrad(const GemmArgs& g, const WgradPlan& p, hipStream_t st);      // Staged, Dma
// gemm_split.hip.  scheme: PARADIS_GEMM_BF16X3 or PARADIS_GEMM_F16X2 (the latter with d.a_amax / d.b_amax set)
int pd_split_launch(const GemmArgs& d, int scheme, hipStream_t st);
int pd_split_launch_wgrad(const GemmArgs& g, const WgradPlan& p, hipStream_t st);      // Bf16x3, F16x2
int64_t pd_split_image_chunks(int M, int K, int np);
// bf16x3 images of nbatch row-major [M,K] matrices (stride a_bs) into out, pd_split_image_chunks(M, K, 3) chunks each
void pd_split_launch_images(const float* A, int nbatch, int M, int K, int64_t a_bs, void* out, hipStream_t st);
// launchers of the bf16-mixed kernels (gemm_amp_fwd.hip, gemm_amp_wgrad.hip)
int pd_amp_launch_fwd(const GemmArgs& d, hipStream_t st);
int pd_amp_launch_wgrad(const GemmArgs& g, int io16, const WgradPlan& p, hipStream_t st);      // Amp128, Tall, Square

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int BM = 128, BN = 128;

// ---- low-rank bias (GlobalBias with projection) accumulated straight into the MFMA accumulators:
//   acc[m,n] += sum_c pwT[c,m] * m8[c,n].  pwT is the transposed projection weight so that the four
//   consecutive rows (r&3) of an accumulator group come from one 16-byte load (needs M % 4 == 0).
//   One channel at a time keeps the live set at acc + 8 registers.
__device__ __forceinline__ void gemm_add_projection(const GemmArgs& g, f32x16 (&acc)[2][2], int m0, int n0,
                                                    int wm, int wn, int li, int lh) {
  const int nc0 = min(n0 + wn * 64 + li, g.N - 1), nc1 = min(n0 + wn * 64 + 32 + li, g.N - 1);
#pragma unroll 1
  for (int c = 0; c < g.cin; ++c) {
    const float mb0 = g.m8[(int64_t)c * g.N + nc0], mb1 = g.m8[(int64_t)c * g.N + nc1];
    const float* pc = g.pw + (int64_t)c * g.M;
#pragma unroll
    for (int tm = 0; tm < 2; ++tm) {
      const int mrow = m0 + wm * 64 + tm * 32 + 4 * lh;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int mr = mrow + 8 * j;
        const float4 p4 = (mr < g.M) ? *reinterpret_cast<const float4*>(pc + mr) : make_float4(0.f, 0.f, 0.f, 0.f);
        acc[tm][0][4 * j + 0] += p4.x * mb0; acc[tm][1][4 * j + 0] += p4.x * mb1;
        acc[tm][0][4 * j + 1] += p4.y * mb0; acc[tm][1][4 * j + 1] += p4.y * mb1;
        acc[tm][0][4 * j + 2] += p4.z * mb0; acc[tm][1][4 * j + 2] += p4.z * mb1;
        acc[tm][0][4 * j + 3] += p4.w * mb0; acc[tm][1][4 * j + 3] += p4.w * mb1;
      }
    }
  }
}

__device__ __forceinline__ float gate_sigmoid(float a) { return 1.0f / (1.0f + expf(-a)); }
// value of x rounded to bf16 (round to nearest even; a NaN stays a NaN: v_cvt_pk_bf16_f32)
__device__ __forceinline__ float round_bf16(float x) { return (float)(__bf16)x; }
// Activations of the bf16-mixed epilogue (R16): the value is rounded to bf16 - 8 significant bits - in the next instruction, so
// the hardware's 1-ulp exp2 / reciprocal stand in for expf and the IEEE division of act_apply / act_grad (common.h): about 9
// instead of about 29 vector instructions per element in an epilogue that was bound by exactly those (sixteen waves x 64 elements
// per lane and tensor).  SiLU only; GELU keeps the library functions.  The fp32-width schemes never call these.
__device__ __forceinline__ float sigmoid_r16(float z) {
  return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.44269504088896340736f * z));
}
__device__ __forceinline__ float act_apply_r16(float z, int act) {
  return act == PARADIS_ACT_SILU ? z * sigmoid_r16(z) : act_apply(z, act);
}
__device__ __forceinline__ float act_grad_r16(float z, int act) {
  if (act == PARADIS_ACT_SILU) {
    const float s = sigmoid_r16(z);
    return s * (1.0f + z * (1.0f - s));
  }
  return act_grad(z, act);
}
// (An epilogue / k-loop stagger - the second workgroup of every CU of the first round starting late by 64-256 x 512 cycles,
//  so that one workgroup's store-bound epilogue runs under the other's MFMA-bound k-loop - was measured on the bf16-mixed
//  and the bf16x3 kernels and lost 0-10 % at every setting: profiles/r06_stagger_sweep.txt.  Not kept.)
[[maybe_unused]] constexpr int IO_B16 = 1, IO_C16 = 2, IO_ZM16 = 4, IO_A16 = 8;     // GemmArgs::io16 (IO_A16: wgrad's dY operand)
// bf16 storage: element i of a bf16 array as a float / a bf16-VALUED float (already rounded) into a bf16 array
__device__ __forceinline__ float ld_bf16(const void* p, int64_t i) {
  return __uint_as_float((uint32_t)reinterpret_cast<const uint16_t*>(p)[i] << 16);
}
__device__ __forceinline__ void st_bf16(void* p, int64_t i, float v) {
  reinterpret_cast<uint16_t*>(p)[i] = (uint16_t)(__float_as_uint(v) >> 16);
}

// ---- epilogue: C/D layout of v_mfma_f32_32x32x2_f32: col = lane&31, row = (r&3) + 8*(r>>2) + 4*(lane>>5)
//   v = acc (+bias[m]) (+map[m,n]); zout = v; v = zmul ? v*act'(zmul) : act(v);
//   v = gate ? res + sigmoid(gate[m]) (v - res) : v + res; C = v
// Interior tiles take a path without per-element guards in which all loads of one 32-row group are
// issued back to back (the guarded form serialises every load behind an s_waitcnt vmcnt(0)).
// R16 (compile time: only the bf16-mixed kernel instantiates it, the fp32 schemes' epilogue is the round-4 code): round
// the pre-activation and the activated / activation-gradient value to bf16 (see the note in GemmArgs)
template <bool R16 = false, bool C16 = false, bool ZM16 = false>
__device__ __forceinline__ void gemm_epilogue(const GemmArgs& g, f32x16 (&acc)[2][2], int bz, int m0,
                                              int n0, int wm, int wn, int li, int lh) {
  float* Cb = g.C + (int64_t)bz * g.c_bs;
  const float* resb = g.res ? g.res + (int64_t)bz * g.res_bs : nullptr;
  const float* zmulb = g.zmul ? g.zmul + (int64_t)bz * g.zmul_bs : nullptr;
  float* zoutb = g.zout ? g.zout + (int64_t)bz * g.zout_bs : nullptr;
  // bf16-stored tensors (compile-time properties of the bf16-mixed kernels' instantiations - as run-time branches they
  // cost the 128-register kernels 256 bytes of scratch and 100 us per launch): the same element offsets on 2-byte elements
  static_assert(R16 || !(C16 || ZM16), "bf16-stored tensors exist in the bf16-mixed scheme only");
  (void)sizeof(char[C16 + ZM16 + 1]);
  const int64_t cb16 = (int64_t)bz * g.c_bs, zmb16 = (int64_t)bz * g.zmul_bs, zob16 = (int64_t)bz * g.zout_bs;
  if (g.pw) gemm_add_projection(g, acc, m0, n0, wm, wn, li, lh);
  if constexpr (C16 || ZM16) {
    // bf16-stored tensors of an interior tile move as PACKED PAIRS: a lane holds pixel li of the wave's two 32-column MFMA
    // tiles (columns li and 32 + li of one row) - as 2-byte accesses a row of a tile is a 64-byte segment per instruction.
    // Adjacent lanes swap one value each (even lane: its tile-1 value for the odd lane's tile-0 value), after which the even
    // lane holds columns (li, li + 1) of tile 0 and the odd lane columns (31 + li, 32 + li): one dword per lane, 128 contiguous
    // bytes per row and instruction, half the instructions.  Loads of a bf16 zmul run the same exchange backwards.
    if (m0 + BM <= g.M && n0 + BN <= g.N && ((g.ldc | g.c_bs | g.zout_bs | g.zmul_bs) & 1) == 0) {
      const bool odd = (li & 1) != 0;
      const uint32_t sel = odd ? 0x07060302u : 0x03020706u;       // v_perm_b32(keep, recv): {lo, hi} halves of the dword
      const int pcol = odd ? 31 + li : li;                         // first column of this lane's pair (even)
      auto swap1 = [](float v) __attribute__((always_inline)) {   // the neighbour's value (lanes 2u <-> 2u + 1)
        return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xf, 0xf, false));
      };
      auto pack = [&](float a0, float a1) __attribute__((always_inline)) {      // a0 / a1: this lane's tile-0 / tile-1 value (bf16-valued)
        const float keep = odd ? a1 : a0, recv = swap1(odd ? a0 : a1);
        return __builtin_amdgcn_perm(__float_as_uint(keep), __float_as_uint(recv), sel);
      };
      auto unpack = [&](uint32_t w, float& t0, float& t1) __attribute__((always_inline)) {
        const float wlo = __uint_as_float(w << 16), whi = __uint_as_float(w & 0xffff0000u);
        const float recv = swap1(odd ? wlo : whi);
        t0 = odd ? recv : wlo;
        t1 = odd ? whi : recv;
      };
#pragma unroll
      for (int tm = 0; tm < 2; ++tm) {
        const int mrow = m0 + wm * 64 + tm * 32 + 4 * lh;
        const int64_t base = (int64_t)mrow * g.ldc + n0 + wn * 64 + li;          // tile 0; tile 1: + 32
        const int64_t pbase = (int64_t)mrow * g.ldc + n0 + wn * 64 + pcol;       // this lane's pair
#pragma unroll
        for (int h = 0; h < 4; ++h) {   // 4 accumulator registers of each tile at a time
          float v[2][4], t[2][4];
          // register r = 4h + q  ->  row offset q + 8h
#define ROWOFF(q) ((int64_t)((q) + 8 * h) * g.ldc)
#pragma unroll
          for (int tn = 0; tn < 2; ++tn)
#pragma unroll
            for (int q = 0; q < 4; ++q) v[tn][q] = acc[tm][tn][4 * h + q];
          if (g.bias) {
#pragma unroll
            for (int q = 0; q < 4; ++q) t[0][q] = g.bias[mrow + q + 8 * h];
#pragma unroll
            for (int q = 0; q < 4; ++q) { v[0][q] += t[0][q]; v[1][q] += t[0][q]; }
          }
          if (g.map) {
#pragma unroll
            for (int tn = 0; tn < 2; ++tn)
#pragma unroll
              for (int q = 0; q < 4; ++q) t[tn][q] = g.map[base + 32 * tn + ROWOFF(q)];
#pragma unroll
            for (int tn = 0; tn < 2; ++tn)
#pragma unroll
              for (int q = 0; q < 4; ++q) v[tn][q] += t[tn][q];
          }
#pragma unroll
          for (int tn = 0; tn < 2; ++tn)
#pragma unroll
            for (int q = 0; q < 4; ++q) v[tn][q] = round_bf16(v[tn][q]);
          if (zoutb) {
            if constexpr (C16) {
#pragma unroll
              for (int q = 0; q < 4; ++q)
                reinterpret_cast<uint32_t*>(g.zout)[(zob16 + pbase + ROWOFF(q)) >> 1] = pack(v[0][q], v[1][q]);
            } else {
#pragma unroll
              for (int tn = 0; tn < 2; ++tn)
#pragma unroll
                for (int q = 0; q < 4; ++q) zoutb[base + 32 * tn + ROWOFF(q)] = v[tn][q];
            }
          }
          if (zmulb) {
            if constexpr (ZM16) {
              uint32_t w[4];
#pragma unroll
              for (int q = 0; q < 4; ++q) w[q] = reinterpret_cast<const uint32_t*>(g.zmul)[(zmb16 + pbase + ROWOFF(q)) >> 1];
#pragma unroll
              for (int q = 0; q < 4; ++q) unpack(w[q], t[0][q], t[1][q]);
            } else {
#pragma unroll
              for (int tn = 0; tn < 2; ++tn)
#pragma unroll
                for (int q = 0; q < 4; ++q) t[tn][q] = zmulb[base + 32 * tn + ROWOFF(q)];
            }
#pragma unroll
            for (int tn = 0; tn < 2; ++tn)
#pragma unroll
              for (int q = 0; q < 4; ++q) v[tn][q] *= act_grad_r16(t[tn][q], g.act);
          } else if (g.act) {
#pragma unroll
            for (int tn = 0; tn < 2; ++tn)
#pragma unroll
              for (int q = 0; q < 4; ++q) v[tn][q] = act_apply_r16(v[tn][q], g.act);
          }
          if (zmulb || g.act) {
#pragma unroll
            for (int tn = 0; tn < 2; ++tn)
#pragma unroll
              for (int q = 0; q < 4; ++q) v[tn][q] = round_bf16(v[tn][q]);
          }
          if (resb) {
#pragma unroll
            for (int tn = 0; tn < 2; ++tn)
#pragma unroll
              for (int q = 0; q < 4; ++q) t[tn][q] = resb[base + 32 * tn + ROWOFF(q)];
            if (g.gate) {
#pragma unroll
              for (int q = 0; q < 4; ++q) {
                const float gm = gate_sigmoid(g.gate[mrow + q + 8 * h]);
                v[0][q] = fmaf(gm, v[0][q] - t[0][q], t[0][q]);
                v[1][q] = fmaf(gm, v[1][q] - t[1][q], t[1][q]);
              }
            } else {
#pragma unroll
              for (int tn = 0; tn < 2; ++tn)
#pragma unroll
                for (int q = 0; q < 4; ++q) v[tn][q] += t[tn][q];
            }
          }
          if constexpr (C16) {
#pragma unroll
            for (int q = 0; q < 4; ++q)
              reinterpret_cast<uint32_t*>(g.C)[(cb16 + pbase + ROWOFF(q)) >> 1] = pack(v[0][q], v[1][q]);
          } else {
#pragma unroll
            for (int tn = 0; tn < 2; ++tn)
#pragma unroll
              for (int q = 0; q < 4; ++q) Cb[base + 32 * tn + ROWOFF(q)] = v[tn][q];
          }
          asm volatile("" ::: "memory");
          __builtin_amdgcn_sched_barrier(0);
#undef ROWOFF
        }
      }
      return;
    }
  }
  if (m0 + BM <= g.M && n0 + BN <= g.N) {
#pragma unroll
    for (int tm = 0; tm < 2; ++tm) {
      const int mrow = m0 + wm * 64 + tm * 32 + 4 * lh;
#pragma unroll
      for (int tn = 0; tn < 2; ++tn) {
        const int64_t base = (int64_t)mrow * g.ldc + n0 + wn * 64 + tn * 32 + li;
#pragma unroll
        for (int h = 0; h < 2; ++h) {   // 8 accumulator registers at a time keeps the kernel <= 128 VGPRs
          float v[8], t[8];
          // register r = 8h + q  ->  row offset (q&3) + 8*(2h + (q>>2))
#define ROWOFF(q) ((int64_t)(((q) & 3) + 8 * (2 * h + ((q) >> 2))) * g.ldc)
#pragma unroll
          for (int q = 0; q < 8; ++q) v[q] = acc[tm][tn][8 * h + q];
          if (g.bias) {
#pragma unroll
            for (int q = 0; q < 8; ++q) t[q] = g.bias[mrow + (q & 3) + 8 * (2 * h + (q >> 2))];
#pragma unroll
            for (int q = 0; q < 8; ++q) v[q] += t[q];
          }
          if (g.map) {
#pragma unroll
            for (int q = 0; q < 8; ++q) t[q] = g.map[base + ROWOFF(q)];
#pragma unroll
            for (int q = 0; q < 8; ++q) v[q] += t[q];
          }
          if constexpr (R16) {
#pragma unroll
            for (int q = 0; q < 8; ++q) v[q] = round_bf16(v[q]);
          }
          if (zoutb) {
            if constexpr (C16) {
#pragma unroll
              for (int q = 0; q < 8; ++q) st_bf16(g.zout, zob16 + base + ROWOFF(q), v[q]);
            } else {
#pragma unroll
              for (int q = 0; q < 8; ++q) zoutb[base + ROWOFF(q)] = v[q];
            }
          }
          if (zmulb) {
            if constexpr (ZM16) {
#pragma unroll
              for (int q = 0; q < 8; ++q) t[q] = ld_bf16(g.zmul, zmb16 + base + ROWOFF(q));
            } else {
#pragma unroll
              for (int q = 0; q < 8; ++q) t[q] = zmulb[base + ROWOFF(q)];
            }
#pragma unroll
            for (int q = 0; q < 8; ++q) v[q] *= R16 ? act_grad_r16(t[q], g.act) : act_grad(t[q], g.act);
          } else if (g.act) {
#pragma unroll
            for (int q = 0; q < 8; ++q) v[q] = R16 ? act_apply_r16(v[q], g.act) : act_apply(v[q], g.act);
          }
          if constexpr (R16) {
            if (zmulb || g.act) {
#pragma unroll
              for (int q = 0; q < 8; ++q) v[q] = round_bf16(v[q]);
            }
          }
          if (resb) {
#pragma unroll
            for (int q = 0; q < 8; ++q) t[q] = resb[base + ROWOFF(q)];
            if (g.gate) {   // h + sigmoid(alpha) (adv - h): the arithmetic of gated_blend_fwd_kernel (elementwise.hip), bit for bit
#pragma unroll
              for (int q = 0; q < 8; ++q) {
                const float gm = gate_sigmoid(g.gate[mrow + (q & 3) + 8 * (2 * h + (q >> 2))]);
                v[q] = fmaf(gm, v[q] - t[q], t[q]);
              }
            } else {
#pragma unroll
              for (int q = 0; q < 8; ++q) v[q] += t[q];
            }
          }
          if constexpr (C16) {
#pragma unroll
            for (int q = 0; q < 8; ++q) st_bf16(g.C, cb16 + base + ROWOFF(q), v[q]);
          } else {
#pragma unroll
            for (int q = 0; q < 8; ++q) Cb[base + ROWOFF(q)] = v[q];
          }
          // keep the scheduler from hoisting the next chunk's loads (register pressure)
          asm volatile("" ::: "memory");
          __builtin_amdgcn_sched_barrier(0);
#undef ROWOFF
        }
      }
    }
    return;
  }
#pragma unroll
  for (int tm = 0; tm < 2; ++tm) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int m = m0 + wm * 64 + tm * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
      if (m >= g.M) continue;
      const float bv = g.bias ? g.bias[m] : 0.f;
#pragma unroll
      for (int tn = 0; tn < 2; ++tn) {
        const int n = n0 + wn * 64 + tn * 32 + li;
        if (n >= g.N) continue;
        const int64_t off = (int64_t)m * g.ldc + n;
        float v = acc[tm][tn][r] + bv;
        if (g.map) v += g.map[off];
        if constexpr (R16) v = round_bf16(v);
        if (zoutb) { if constexpr (C16) st_bf16(g.zout, zob16 + off, v); else zoutb[off] = v; }
        if (zmulb) {
          const float zm = ZM16 ? ld_bf16(g.zmul, zmb16 + off) : zmulb[off];
          v *= R16 ? act_grad_r16(zm, g.act) : act_grad(zm, g.act);
        } else if (g.act) {
          v = R16 ? act_apply_r16(v, g.act) : act_apply(v, g.act);
        }
        if constexpr (R16) { if (zmulb || g.act) v = round_bf16(v); }
        if (resb) {
          const float r = resb[off];
          v = g.gate ? fmaf(gate_sigmoid(g.gate[m]), v - r, r) : v + r;
        }
        if constexpr (C16) st_bf16(g.C, cb16 + off, v); else Cb[off] = v;
      }
    }
  }
}

typedef __attribute__((address_space(3))) void* lds_ptr_t;
typedef const __attribute__((address_space(1))) void* gbl_ptr_t;

// ======================================================================================
// Split-bf16 kernels: the same fp32 GEMMs on the bf16 matrix pipe (16x the f32 MFMA rate).
// Every fp32 operand value x is written as h + m + l with h = bf16(x), m = bf16(x - h),
// l = bf16(x - h - m): three bf16 numbers carry 3 x 8 = 24 significand bits, so the split is exact.
// a*b is accumulated in fp32 from the six partial products of weight >= 2^-16,
//     ah*bh + ah*bm + am*bh + ah*bl + al*bh + am*bm        (dropped: am*bl, al*bm, al*bl <= 2^-23 |ab|)
// v_mfma_f32_32x32x16_bf16 forms the 8x8-bit products exactly and accumulates in fp32, 6/16 roundings
// per k instead of the f32 MFMA's 1: the measured error against fp64 is below the f32 kernels'
// (tests/test_hip_gemm_split.py).  Non-finite inputs come out as NaN (Inf - Inf in the split).
//
// LDS image of a 128 x 16 operand tile: [split 3][k-half 2][row 128] chunks of 16 B = 8 bf16
// (k = 8*half + 0..7), so that one ds_read_b128 per lane (row = lane&31, half = lane>>5) is the
// MFMA operand.  Weights are split once per call into that image in global memory
// (split_weights_kernel) and move by LDS-DMA; activations are split in registers while staged.
// 2 stages x 24 KiB => 3 workgroups per CU.
// ======================================================================================
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
// LDS images are accessed through a clang vector type, not HIP's u32x4 struct: behind a struct-typed
// ds_read the compiler inserts an s_waitcnt vmcnt for every LDS-DMA still in flight (alias rule),
// which would serialise the DMA rings; vector-typed reads do not get that wait.
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int SBK = 16;                  // k depth of a tile = one bf16 / f16 MFMA
constexpr int SCH = 128;                 // chunks per k-half row of an unpadded image
constexpr int SCHP = 128 + 8;            // padded variant (wgrad: lane pairs write both k-halves of a row)
// NP = number of planes of an operand image = terms of the split: 3 = bf16 h/m/l (exact, six products),
// 2 = f16 h/l of the scaled value (22 significand bits, three products), 1 = the value rounded to bf16 (ONE product:
// PARADIS_GEMM_BF16, the arithmetic of the reference's bf16-mixed training mode - train.py:56 - never the fp32 path's)
constexpr int simg(int np) { return np * 2 * SCH; }      // chunks per operand per stage (12 / 8 KiB)
constexpr int simgp(int np) { return np * 2 * SCHP; }

// ---- sign checkerboard (round 4) ---------------------------------------------------------------------------------
// What the bf16 / f16 MFMA does with its accumulator input (tools/mfma_round_probe.hip, gfx950): the sixteen products
// are summed first; the smaller of {C, product sum} is then aligned to the larger one's exponent, and when the smaller
// one is C its low bits are dropped by a two's-complement FLOOR (C = -2^-26 against a product sum of 1 - 1 comes out as
// -2^-24).  Whenever a k-tile's product sum outweighs the running accumulator - the first tiles, and every later zero
// crossing: ~5 times per K = 1024 dot product of zero-mean data - the result moves half a granule towards -infinity.
// The f32 MFMA (an fma chain, round to nearest) has no such term.  Measured (tools/gemm_bias_check.py, N(0,1) data,
// unit u = 2^-24 rms(C)): every output of the six-product GEMM carried the SAME offset, -0.9 u on top of 8.2 u of
// zero-mean noise (f32 MFMA: +0.002 u on 9.6 u), -8 u on the weight gradient's 32,768-term sums.  Harmless per element,
// but sums over pixels or channels of a GEMM output (bias / ChannelNorm parameter gradients over 32,768 points, the
// per-pixel channel statistics) add the offset coherently where noise averages out: 0.9 u x 32,768 against 8.2 u x 181.
// Remedy without a second accumulator set or VALU work per tile: run alternate 32-row x 64-column blocks of the output
// in the NEGATED space.  The weight image holds the rows of odd 32-row blocks with the opposite sign (free: written once
// by split_weights_kernel), the activation columns of odd 64-column blocks - the columns ONE wave stages - are negated
// while they are split in registers (-x splits exactly into -h, -m, -l; in the 128 x 256 kernel the sign is a
// compile-time property of the code path a staging wave takes, so it rides on source modifiers), so block (tm) of
// compute wave (wm, wn) accumulates (-1)^(tm+wn) C: there the floor acts on -C, the offset of C is +0.9 u, and the
// epilogue flips those blocks back.  The offset is still there per element; it alternates in sign every 32 rows and
// 64 columns and cancels in every sum over more than a block.  The weight gradient alternates by K-range slab instead (odd slabs negate dY): there the offsets of an
// element's slabs cancel in the slab sum.
#ifndef SPLIT_SIGNED          // (-DSPLIT_SIGNED=0: the unsigned accumulation of rounds 1-3, for A/B runs)
#define SPLIT_SIGNED 1
#endif
#ifndef SPLIT_SIGNED_WGRAD    // (the slab alternation of the weight gradient alone)
#define SPLIT_SIGNED_WGRAD SPLIT_SIGNED
#endif
// The sign as a compile-time property of the k-loop (bf16x3 kernels): the sign of a staging wave (forward / data gradient:
// bit 6 of its column) or workgroup (weight gradient: the slab's parity) never changes during a launch, so the wave picks
// ONE of two complete copies of prologue and k-loop ahead of the loop; the negated copy splits -x through source modifiers
// (split8s<true>) where the single loop spends eight v_xor per thread and k-tile (flip8).  Each copy keeps one basic block
// per step.  The weight gradient likewise keeps its fused row sums to a loop copy of the workgroups that store them, forms
// its load addresses from a scalar base and one 32-bit lane offset, and stores interior tiles through
// split_epilogue_interior.  -DSPLIT_SIGN_LOOPS=0 restores the v_xor loops and everything else of the single-loop kernels
// (A/B builds); the parts can be switched one at a time.
#ifndef SPLIT_SIGN_LOOPS
#define SPLIT_SIGN_LOOPS 1
#endif
#ifndef SPLIT_SIGN_LOOPS_FWD         // forward / data gradient: sign copies of pw_gemm_split_wide_kernel<2, 3, EPI>
#define SPLIT_SIGN_LOOPS_FWD SPLIT_SIGN_LOOPS
#endif
#ifndef SPLIT_SIGN_LOOPS_WGRAD       // weight gradient: sign copies
#define SPLIT_SIGN_LOOPS_WGRAD SPLIT_SIGN_LOOPS
#endif
#ifndef SPLIT_WGRAD_ROWSUM_LOOP      // weight gradient: row-sum adds only in the copy of the workgroups that store them
#define SPLIT_WGRAD_ROWSUM_LOOP SPLIT_SIGN_LOOPS
#endif
#ifndef SPLIT_WGRAD_SADDR            // weight gradient: scalar base + 32-bit lane offset
#define SPLIT_WGRAD_SADDR SPLIT_SIGN_LOOPS
#endif
#ifndef SPLIT_WGRAD_EPILOGUE         // weight gradient: interior tiles through split_epilogue_interior<EP_ON>
#define SPLIT_WGRAD_EPILOGUE SPLIT_SIGN_LOOPS
#endif
// sign bit of the staging thread's activation column (column = tid & 127 of a 128-column tile)
__device__ __forceinline__ uint32_t split_flip_mask(int col) { return SPLIT_SIGNED && (col & 64) ? 0x80000000u : 0u; }
__device__ __forceinline__ void flip8(float (&y)[8], const float (&x)[8], uint32_t mask) {
#pragma unroll
  for (int j = 0; j < 8; ++j) y[j] = __uint_as_float(__float_as_uint(x[j]) ^ mask);
}
// the row blocks tm with (tm + wn) odd hold -C (wn = the wave's 64-column half: the sign of its activation columns)
__device__ __forceinline__ void split_unflip(f32x16 (&acc)[2][2], int wn) {
  if (!SPLIT_SIGNED) return;
  const float s0 = wn ? -1.f : 1.f, s1 = -s0;          // wave-uniform
#pragma unroll
  for (int tn = 0; tn < 2; ++tn)
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc[0][tn][r] *= s0; acc[1][tn][r] *= s1; }
}

// ---- f16x2 scheme ------------------------------------------------------------------------------
// x' = x 2^e with e chosen per TENSOR so that max |x'| lies in [2^14, 2^15) (fp16 holds 65504);
// h = f16(x'), l = f16(x' - h): x' = h + l up to 2^-23 |x'|, and - fp16 being a fixed-point format below
// 2^-14 - up to 2^-25 absolutely, i.e. 2^-39 of the tensor's largest magnitude.  a b is accumulated in
// fp32 from  al bh + ah bl + ah bh  (dropped: al bl <= 2^-22 |ab|); the f16 MFMA forms the 11x11-bit
// products exactly.  The result is unscaled by 2^-(ea+eb) in the epilogue (two exact multiplications).
// Error against fp64 of a K = 1024 product of N(0,1) operands: 5.1e-7 of max |C| (SGEMM: 5.8e-7); what
// it gives up against the bf16x3 scheme is elements more than ~2^17 below their tensor's maximum, which
// keep an ABSOLUTE accuracy of 2^-39 max|x| instead of a relative one.
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

// scale 2^e and its inverse from the bits of max |x| (biased exponent E: e = 14 - (E - 127)); a zero or
// tiny maximum takes the largest scale.  A non-finite maximum (an Inf or NaN somewhere in the tensor) has no
// meaningful scale: the scale becomes NaN and with it the whole product - loudly wrong, never silently rescaled.
__device__ __forceinline__ void scale_from_amax(uint32_t amax_bits, float& s, float& inv) {
  int E = (int)((amax_bits >> 23) & 0xffu);
  const bool finite = E != 255;
  E = E < 15 ? 15 : E;
  s = finite ? __uint_as_float((uint32_t)(268 - E) << 23) : __uint_as_float(0x7fc00000u);
  inv = __uint_as_float((uint32_t)(E - 14) << 23);
}

// max of PARADIS_AMAX_PARTIALS (= 1024) words, by a 256-thread workgroup; every thread gets the result
__device__ __forceinline__ uint32_t reduce_amax_partials(const uint32_t* __restrict__ p) {
  __shared__ uint32_t red[4];
  const int tid = threadIdx.x;
  uint32_t m = max(max(p[tid], p[tid + 256]), max(p[tid + 512], p[tid + 768]));
  m = wave_umax_lane63(m);
  if ((tid & 63) == 63) red[tid >> 6] = m;
  __syncthreads();
  m = max(max(red[0], red[1]), max(red[2], red[3]));
  __syncthreads();
  return m;
}

// (x0, x1) 2^e -> packed halves h, l.  v_fma_mix*: fp32 FMA, result rounded once to f16; x s and
// x s - h are exact in fp32, so h and l are the correctly rounded values.
__device__ __forceinline__ void split2_pair(float x0, float x1, float s, uint32_t& h, uint32_t& l) {
  uint32_t hh, ll;
  asm("v_fma_mixlo_f16 %0, %1, %2, 0" : "=v"(hh) : "v"(x0), "v"(s));
  asm("v_fma_mixhi_f16 %0, %1, %2, 0" : "+v"(hh) : "v"(x1), "v"(s));
  asm("v_fma_mixlo_f16 %0, %1, %2, -%3 op_sel:[0,0,0] op_sel_hi:[0,0,1]" : "=v"(ll) : "v"(x0), "v"(s), "v"(hh));
  asm("v_fma_mixhi_f16 %0, %1, %2, -%3 op_sel:[0,0,1] op_sel_hi:[0,0,1]" : "+v"(ll) : "v"(x1), "v"(s), "v"(hh));
  h = hh; l = ll;
}

__device__ __forceinline__ uint32_t pack_bf16(float a, float b) {
  const f32x2 v = {a, b};
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2));   // v_cvt_pk_bf16_f32, a in the low half
}

__device__ __forceinline__ void split_pair(float x0, float x1, uint32_t& h, uint32_t& m, uint32_t& l) {
  h = pack_bf16(x0, x1);
  const float r0 = x0 - __uint_as_float(h << 16), r1 = x1 - __uint_as_float(h & 0xffff0000u);
  m = pack_bf16(r0, r1);
  l = pack_bf16(r0 - __uint_as_float(m << 16), r1 - __uint_as_float(m & 0xffff0000u));
}

__device__ __forceinline__ void split8(const float (&x)[8], u32x4& h, u32x4& m, u32x4& l) {
  uint32_t hh[4], mm[4], ll[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) split_pair(x[2 * i], x[2 * i + 1], hh[i], mm[i], ll[i]);
  h = (u32x4){hh[0], hh[1], hh[2], hh[3]};
  m = (u32x4){mm[0], mm[1], mm[2], mm[3]};
  l = (u32x4){ll[0], ll[1], ll[2], ll[3]};
}

// the planes of x (FLIP = false) or of -x (true): -x splits exactly into (-h, -m, -l); the negations are written in the
// expressions, where they fold into the source modifiers of v_cvt_pk_bf16_f32 and v_sub_f32
template <bool FLIP>
__device__ __forceinline__ void split8s(const float (&x)[8], u32x4& h, u32x4& m, u32x4& l) {
  if constexpr (!FLIP) {
    split8(x, h, m, l);
  } else {
    uint32_t hh[4], mm[4], ll[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float x0 = x[2 * i], x1 = x[2 * i + 1];
      // (hipcc folds the negation into v_sub_f32 but not into the conversion: spelled out, or it costs the v_xor again)
      asm("v_cvt_pk_bf16_f32 %0, -%1, -%2" : "=v"(hh[i]) : "v"(x0), "v"(x1));
      const float r0 = (-x0) - __uint_as_float(hh[i] << 16), r1 = (-x1) - __uint_as_float(hh[i] & 0xffff0000u);
      mm[i] = pack_bf16(r0, r1);
      ll[i] = pack_bf16(r0 - __uint_as_float(mm[i] << 16), r1 - __uint_as_float(mm[i] & 0xffff0000u));
    }
    h = (u32x4){hh[0], hh[1], hh[2], hh[3]};
    m = (u32x4){mm[0], mm[1], mm[2], mm[3]};
    l = (u32x4){ll[0], ll[1], ll[2], ll[3]};
  }
}

// eight values rounded to bf16 (the one plane of PARADIS_GEMM_BF16)
__device__ __forceinline__ u32x4 round8(const float (&x)[8]) {
  return (u32x4){pack_bf16(x[0], x[1]), pack_bf16(x[2], x[3]), pack_bf16(x[4], x[5]), pack_bf16(x[6], x[7])};
}

__device__ __forceinline__ void split8_f16(const float (&x)[8], float s, u32x4& h, u32x4& l) {
  uint32_t hh[4], ll[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) split2_pair(x[2 * i], x[2 * i + 1], s, hh[i], ll[i]);
  h = (u32x4){hh[0], hh[1], hh[2], hh[3]};
  l = (u32x4){ll[0], ll[1], ll[2], ll[3]};
}

#define SPLIT_MFMA(A, B, C) C = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, A), __builtin_bit_cast(bf16x8, B), C, 0, 0, 0)
// The six partial products of one 32x32 block, smallest first.  (An order in which consecutive MFMAs
// share an operand register, snaking over the four blocks of a wave tile, measured +0.5 % - nothing -
// once the A/B alternated the variants: a fixed order of variants shows 3-5 % in favour of whichever
// runs later.)
#define SPLIT_BLOCK(AH, AM, AL, BH, BM_, BL, C) \
  SPLIT_MFMA(AM, BM_, C); SPLIT_MFMA(AL, BH, C); SPLIT_MFMA(AH, BL, C); \
  SPLIT_MFMA(AM, BH, C);  SPLIT_MFMA(AH, BM_, C); SPLIT_MFMA(AH, BH, C)
#define SPLIT_MFMA16(A, B, C) C = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, A), __builtin_bit_cast(f16x8, B), C, 0, 0, 0)

// one k-tile: fragments of both operands from the images at As/Bs (chunk pointers at this lane's
// row of block 0, k-half lh), plane stride PA/PB chunks ...
template <int NP> struct SplitFrags { u32x4 a[NP][2], b[NP][2]; };
template <int NP, int PA, int PB>
__device__ __forceinline__ void split_tile_read(const u32x4* As, const u32x4* Bs, SplitFrags<NP>& f) {
  // in the order of first use by split_tile_mfma (block (0,0): m.m, l.h, h.l first; l.h, h.l for two
  // planes), so that the counted lgkmcnt waits let the first MFMAs start after two reads
  if constexpr (NP == 3) {
    f.a[1][0] = As[PA];          f.b[1][0] = Bs[PB];
    f.a[2][0] = As[2 * PA];      f.b[0][0] = Bs[0];
    f.a[0][0] = As[0];           f.b[2][0] = Bs[2 * PB];
    f.b[1][1] = Bs[PB + 32];     f.b[0][1] = Bs[32];          f.b[2][1] = Bs[2 * PB + 32];
    f.a[1][1] = As[PA + 32];     f.a[2][1] = As[2 * PA + 32]; f.a[0][1] = As[32];
  } else if constexpr (NP == 2) {
    f.a[1][0] = As[PA];          f.b[0][0] = Bs[0];
    f.a[0][0] = As[0];           f.b[1][0] = Bs[PB];
    f.b[0][1] = Bs[32];          f.b[1][1] = Bs[PB + 32];
    f.a[1][1] = As[PA + 32];     f.a[0][1] = As[32];
  } else {
    f.a[0][0] = As[0];  f.b[0][0] = Bs[0];
    f.b[0][1] = Bs[32]; f.a[0][1] = As[32];
  }
}
// ... then the 24 (12) MFMAs, smallest products first
template <int NP>
__device__ __forceinline__ void split_tile_mfma(const SplitFrags<NP>& f, f32x16 (&acc)[2][2]) {
#pragma unroll
  for (int tm = 0; tm < 2; ++tm)
#pragma unroll
    for (int tn = 0; tn < 2; ++tn) {
      if constexpr (NP == 3) {
        SPLIT_BLOCK(f.a[0][tm], f.a[1][tm], f.a[2][tm], f.b[0][tn], f.b[1][tn], f.b[2][tn], acc[tm][tn]);
      } else if constexpr (NP == 2) {
        SPLIT_MFMA16(f.a[1][tm], f.b[0][tn], acc[tm][tn]);
        SPLIT_MFMA16(f.a[0][tm], f.b[1][tn], acc[tm][tn]);
        SPLIT_MFMA16(f.a[0][tm], f.b[0][tn], acc[tm][tn]);
      } else {
        SPLIT_MFMA(f.a[0][tm], f.b[0][tn], acc[tm][tn]);
      }
    }
}

// f16x2: C = 2^-(ea+eb) acc, two exact multiplications (their product may lie outside the fp32 range)
__device__ __forceinline__ void split_unscale(f32x16 (&acc)[2][2], float inv_a, float inv_b) {
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = (acc[i][j][r] * inv_a) * inv_b;
}

// ---- the interior-tile epilogue of the six-product (bf16x3) kernels, one instantiation per option set ------------------------
// gemm_epilogue (above) decides every option at run time and waits for each operand tensor of each group of eight values
// on its own.  Here the option set EPI is a compile-time bit set, and per element the operations, their order and their
// contraction are gemm_epilogue's, so the results are the same bits.  Two kernels use it: the 128 x 256 forward /
// data-gradient kernel with the sets a training step launches (SPLIT_WIDE_EPI in gemm_split.hip), and the weight-gradient
// kernel below with EP_ON alone - a slab or dW tile is a plain store.  Everything else, ragged tiles included, keeps
// gemm_epilogue.
//   * a wave walks its 64 x 64 block as eight groups (tm, h, tn) of eight rows x 64 lanes; all operand loads of group
//     g + 1 (map, zmul, res) are issued before the arithmetic and the stores of group g, into the registers the k-loop
//     has released, and waited for by count (the stores count as well: vmcnt retires in order);
//   * loads and stores take the saddr form - a scalar row pointer plus ONE 32-bit lane offset ((4 lh ldc + li) x 4 bytes;
//     the second 32-column tile sits in the instruction's immediate offset) - instead of a 64-bit vector address each;
//   * bias[m] and sigmoid(gate[m]) are per-row values: lane l of a wave fetches row l of the wave's 64 rows once (one
//     expf and one division per lane and tile instead of 64), and a pair of groups picks its eight rows with ds_bpermute.
enum : int { EP_ON = 1, EP_BIAS = 2, EP_MAP = 4, EP_ZOUT = 8, EP_SILU = 16, EP_ZMUL = 32, EP_RES = 64, EP_GATE = 128 };

template <int OFF>
__device__ __forceinline__ void ep_load(float& x, uint32_t voff, const float* p) {
  asm volatile("global_load_dword %0, %1, %2 offset:%3" : "=&v"(x) : "v"(voff), "s"(p), "n"(OFF) : "memory");
}
template <int OFF>
__device__ __forceinline__ void ep_store(float x, uint32_t voff, float* p) {
  asm volatile("global_store_dword %0, %1, %2 offset:%3" :: "v"(voff), "v"(x), "s"(p), "n"(OFF) : "memory");
}
// at most N younger vector-memory operations outstanding; the registers waited for are INPUTS (see USE_X in gemm_split.hip)
template <int N>
__device__ __forceinline__ void ep_wait(const float (&a)[8]) {
  asm volatile("s_waitcnt vmcnt(%0)" :: "n"(N), "v"(a[0]), "v"(a[1]), "v"(a[2]), "v"(a[3]), "v"(a[4]), "v"(a[5]), "v"(a[6]),
               "v"(a[7]) : "memory");
  __builtin_amdgcn_sched_barrier(0);
}
template <int N>
__device__ __forceinline__ void ep_wait(const float (&a)[8], const float (&b)[8]) {
  asm volatile("s_waitcnt vmcnt(%0)" :: "n"(N), "v"(a[0]), "v"(a[1]), "v"(a[2]), "v"(a[3]), "v"(a[4]), "v"(a[5]), "v"(a[6]),
               "v"(a[7]), "v"(b[0]), "v"(b[1]), "v"(b[2]), "v"(b[3]), "v"(b[4]), "v"(b[5]), "v"(b[6]), "v"(b[7]) : "memory");
  __builtin_amdgcn_sched_barrier(0);
}
template <int N>
__device__ __forceinline__ void ep_wait(float a, float b) {
  asm volatile("s_waitcnt vmcnt(%0)" :: "n"(N), "v"(a), "v"(b) : "memory");
  __builtin_amdgcn_sched_barrier(0);
}
__device__ __forceinline__ float ep_row(float rowvec, int addr) {      // rowvec of lane addr / 4
  return __int_as_float(__builtin_amdgcn_ds_bpermute(addr, __float_as_int(rowvec)));
}
template <class T>
__device__ __forceinline__ T* ep_uniform(T* p) {      // wave-uniform by construction: pin it to scalar registers
  const uint64_t a = reinterpret_cast<uint64_t>(p);
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)a), hi = __builtin_amdgcn_readfirstlane((uint32_t)(a >> 32));
  return reinterpret_cast<T*>(((uint64_t)hi << 32) | lo);
}

template <int EPI>
__device__ __forceinline__ void split_epilogue_interior(const GemmArgs& g, f32x16 (&acc)[2][2], int bz, int m0, int n0,
                                                        int wm, int wn, int li, int lh) {
  constexpr bool BIAS = EPI & EP_BIAS, MAP = EPI & EP_MAP, ZOUT = EPI & EP_ZOUT, SILU = EPI & EP_SILU, ZMUL = EPI & EP_ZMUL,
                 RES = EPI & EP_RES, GATE = EPI & EP_GATE;
  static_assert(!(GATE && !RES) && !(ZMUL && (SILU || ZOUT)), "no such epilogue");
  // operand tensors of a group, their slots in the load buffers, loads / stores per group
  constexpr int NT = MAP + ZMUL + RES, I_MAP = 0, I_ZM = MAP, I_RES = MAP + ZMUL;
  static_assert(NT <= 2, "a third operand tensor needs a third ep_wait");
  constexpr int L = 8 * NT, S = 8 * (1 + ZOUT);
  const int wrow = __builtin_amdgcn_readfirstlane(m0 + wm * 64), wcol = __builtin_amdgcn_readfirstlane(n0 + wn * 64);
  const int64_t ld = g.ldc, tile = (int64_t)wrow * ld + wcol;
  float* const Cs = ep_uniform(g.C + (int64_t)bz * g.c_bs + tile);
  float* const zos = ZOUT ? ep_uniform(g.zout + (int64_t)bz * g.zout_bs + tile) : nullptr;
  const float* const mps = MAP ? ep_uniform(g.map + tile) : nullptr;
  const float* const zms = ZMUL ? ep_uniform(g.zmul + (int64_t)bz * g.zmul_bs + tile) : nullptr;
  const float* const rss = RES ? ep_uniform(g.res + (int64_t)bz * g.res_bs + tile) : nullptr;
  const uint32_t voff = ((uint32_t)(4 * lh) * (uint32_t)ld + (uint32_t)li) * 4u;      // (host: ldc < 2^26)
  const int radr = 16 * lh;                                   // ds_bpermute address of row 4 lh of the wave's 64
  // group gi = (tm, h, tn); element q sits in row tm 32 + (q & 3) + 8 (2 h + (q >> 2)) (+ 4 lh) of the wave's block
  auto rowof = [](int gi, int q) constexpr { return (gi >> 2) * 32 + (q & 3) + 8 * (2 * ((gi >> 1) & 1) + (q >> 2)); };

  float bv = 0.f, gv = 0.f;             // lane l: bias / gate of row wrow + l
  float buf[2][NT ? NT : 1][8];
  auto issue = [&](auto G) __attribute__((always_inline)) {
    constexpr int gi = decltype(G)::value, OFF = (gi & 1) * 128;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int64_t ro = (int64_t)rowof(gi, q) * ld;
      if constexpr (MAP) ep_load<OFF>(buf[gi & 1][I_MAP][q], voff, mps + ro);
      if constexpr (ZMUL) ep_load<OFF>(buf[gi & 1][I_ZM][q], voff, zms + ro);
      if constexpr (RES) ep_load<OFF>(buf[gi & 1][I_RES][q], voff, rss + ro);
    }
  };
  float br[8], gr[8];                   // the rows of the current (tm, h): picked at tn = 0, used by both column tiles
  if constexpr (BIAS) ep_load<0>(bv, (uint32_t)(32 * lh + li) * 4u, ep_uniform(g.bias + wrow));
  if constexpr (GATE) ep_load<0>(gv, (uint32_t)(32 * lh + li) * 4u, ep_uniform(g.gate + wrow));
  if constexpr (NT > 0) issue(std::integral_constant<int, 0>{});
  __builtin_amdgcn_sched_barrier(0);

  auto group = [&](auto G) __attribute__((always_inline)) {
    constexpr int gi = decltype(G)::value, tm = gi >> 2, h = (gi >> 1) & 1, tn = gi & 1, OFF = tn * 128, b = gi & 1;
    if constexpr (NT > 0 && gi < 7) {
      issue(std::integral_constant<int, gi + 1>{});
      __builtin_amdgcn_sched_barrier(0);
    }
    if constexpr (gi == 0 && (BIAS || GATE)) {
      ep_wait<NT ? 2 * L : 0>(bv, gv);       // younger: the loads of groups 0 and 1
      if constexpr (GATE) gv = gate_sigmoid(gv);
    }
    if constexpr (tn == 0 && (BIAS || GATE)) {      // eight (sixteen) picks back to back, one counted LDS wait each
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        if constexpr (BIAS) br[q] = ep_row(bv, radr + 4 * rowof(gi, q));
        if constexpr (GATE) gr[q] = ep_row(gv, radr + 4 * rowof(gi, q));
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    // younger than this group's loads: the stores of the group before, the loads of the group after
    constexpr int YOUNGER = (gi < 7 ? L : 0) + (gi > 0 ? S : 0);
    if constexpr (NT == 1) ep_wait<YOUNGER>(buf[b][0]);
    if constexpr (NT == 2) ep_wait<YOUNGER>(buf[b][0], buf[b][1]);
    float v[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) v[q] = acc[tm][tn][8 * h + q];
    if constexpr (BIAS) {
#pragma unroll
      for (int q = 0; q < 8; ++q) v[q] += br[q];
    }
    if constexpr (MAP) {
#pragma unroll
      for (int q = 0; q < 8; ++q) v[q] += buf[b][I_MAP][q];
    }
    if constexpr (ZOUT) {
#pragma unroll
      for (int q = 0; q < 8; ++q) ep_store<OFF>(v[q], voff, zos + (int64_t)rowof(gi, q) * ld);
    }
    if constexpr (ZMUL) {
#pragma unroll
      for (int q = 0; q < 8; ++q) v[q] *= act_grad(buf[b][I_ZM][q], PARADIS_ACT_SILU);
    } else if constexpr (SILU) {
#pragma unroll
      for (int q = 0; q < 8; ++q) v[q] = act_apply(v[q], PARADIS_ACT_SILU);
    }
    if constexpr (RES) {
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const float r = buf[b][I_RES][q];
        if constexpr (GATE) v[q] = fmaf(gr[q], v[q] - r, r);
        else v[q] += r;
      }
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) ep_store<OFF>(v[q], voff, Cs + (int64_t)rowof(gi, q) * ld);
    __builtin_amdgcn_sched_barrier(0);      // (a group's arithmetic stays behind the stores of the group before)
  };
  group(std::integral_constant<int, 0>{}); group(std::integral_constant<int, 1>{});
  group(std::integral_constant<int, 2>{}); group(std::integral_constant<int, 3>{});
  group(std::integral_constant<int, 4>{}); group(std::integral_constant<int, 5>{});
  group(std::integral_constant<int, 6>{}); group(std::integral_constant<int, 7>{});
}

// ---- the weight-gradient kernel of the split schemes: gemm_split.hip launches NP = 3 and 2, gemm_amp_wgrad.hip NP = 1 ---
// wgrad: dW[M,N'] = sum over (sample, p) A[m][p] B[n][p], both operands p-contiguous fp32, both split
// in registers.  Thread t stages 8 consecutive p of row t>>1 (k-half t&1) of each operand.
// Needs K % 16 == 0 and 16-B aligned rows (host-checked; otherwise the f32 kernels run).
// Same pipeline as the fwd/dgrad kernel: loads two tiles ahead into alternating register sets (inline asm,
// counted waits), the two splits of tile t+1 between the MFMAs of tile t, raw barriers, one MFMA block
// per tile.
typedef float f32x4 __attribute__((ext_vector_type(4)));
// (A soft rendezvous of a K-range slab's tiles - round 5: FETCH_SIZE 8.48 -> 4.06 GB per launch at 128 x 256, kernel 13 %
//  slower - was measured and removed: DESIGN_HISTORY.md section 4.1d, profiles/r05_wgrad_rendezvous.txt.)
// A32 (bf16x3 only; the host's choice, split_wgrad_a32): both operands' tile rows lie within 2^31 bytes of the tile's first
// row, so a load address is a scalar pointer (tile row 0 of the current sample and k-tile, advanced on the scalar unit)
// plus one constant 32-bit lane offset - no 64-bit vector address arithmetic in the loop.
template <int NP, int A32 = 0>
__global__ void __launch_bounds__(256, 3)
pw_gemm_wgrad_split_kernel(GemmArgs g) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  static_assert(A32 == 0 || NP == 3, "the scalar-base loads exist in the bf16x3 instantiation only");
  constexpr bool SADDR = A32 != 0 && SPLIT_WGRAD_SADDR;
  // loop copies (bf16x3): sign 0 / 1 = plain / negated at compile time, row sums 0 / 1 = absent / present; 2 = decided
  // by run-time values inside the one loop, as in the two-plane and one-plane instantiations
  constexpr bool SIGN_COPIES = NP == 3 && SPLIT_SIGN_LOOPS_WGRAD && SPLIT_SIGNED_WGRAD;
  constexpr bool ROWSUM_COPIES = NP == 3 && SPLIT_WGRAD_ROWSUM_LOOP;
  constexpr int SIMGP = simgp(NP);
  u32x4* img = reinterpret_cast<u32x4*>(lds);        // [2 stages][A|B][SIMGP]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int li = lane & 31, lh = lane >> 5;

  const int MT = (g.M + BM - 1) / BM, NT = (g.N + BN - 1) / BN;
  int L;
  {
    const int nwg = gridDim.x, id = blockIdx.x;
    const int q = nwg >> 3, r = nwg & 7, xcd = id & 7;
    L = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (id >> 3);
  }
  int mt = L % MT, nt = (L / MT) % NT, bz = L / (MT * NT);
  if constexpr (SIGN_COPIES || ROWSUM_COPIES || SADDR) {
    // (uniform, but divided on the vector unit: what the loop copies are chosen by, and what the epilogue keeps through
    //  them, belongs in scalar registers)
    mt = __builtin_amdgcn_readfirstlane(mt); nt = __builtin_amdgcn_readfirstlane(nt); bz = __builtin_amdgcn_readfirstlane(bz);
  }
  const int m0 = mt * BM, n0 = nt * BN;
  const int KT = g.K / SBK;
  const int64_t total = (int64_t)g.inner * KT;
  int t_begin = (int)(total * bz / g.nbatch);
  int T = (int)(total * (bz + 1) / g.nbatch) - t_begin;
  if constexpr (SADDR) {      // (uniform, but divided on the vector unit: the loop's tile counters belong in scalar registers)
    t_begin = __builtin_amdgcn_readfirstlane(t_begin);
    T = __builtin_amdgcn_readfirstlane(T);
  }

  // (sample, k-tile) of the next tile to fetch, advanced incrementally
  int f_ib0 = t_begin / KT, f_kt0 = t_begin - f_ib0 * KT;
  // SADDR: row 0 of the tile at (sample, k-tile); a thread adds the byte offset of its row (run below)
  const float* sa0 = nullptr;
  const float* sb0 = nullptr;
  int64_t wrap_a = 0, wrap_b = 0;       // what a step to the next sample's first k-tile adds on top of SBK
  if constexpr (SADDR) {
    f_ib0 = __builtin_amdgcn_readfirstlane(f_ib0);
    f_kt0 = __builtin_amdgcn_readfirstlane(f_kt0);
    sa0 = ep_uniform(g.A + (int64_t)m0 * g.lda + (int64_t)f_ib0 * g.a_is + (int64_t)f_kt0 * SBK);
    sb0 = ep_uniform(g.B + (int64_t)n0 * g.ldb + (int64_t)f_ib0 * g.b_is + (int64_t)f_kt0 * SBK);
    wrap_a = g.a_is - (int64_t)KT * SBK;
    wrap_b = g.b_is - (int64_t)KT * SBK;
  }
  struct Regs { f32x4 a0, a1, b0, b1; };
  // at most N younger vector-memory operations outstanding; registers as asm inputs (see USE_X)
#define USE_R(r, N) do { asm volatile("s_waitcnt vmcnt(" #N ")" :: "v"(r.a0), "v"(r.a1), "v"(r.b0), "v"(r.b1) : "memory"); \
                         __builtin_amdgcn_sched_barrier(0); } while (0)
  const bool do_rowsum = g.rowsum != nullptr && nt == 0;
  float rs = 0.f;
  float sc_a = 1.f, sc_b = 1.f, inv_a = 1.f, inv_b = 1.f;
  if constexpr (NP == 2) {
    scale_from_amax(reduce_amax_partials(g.a_amax), sc_a, inv_a);
    scale_from_amax(reduce_amax_partials(g.b_amax), sc_b, inv_b);
  }
  // the offset of the MFMA's accumulator alignment (see "sign checkerboard") cancels between an element's slabs
  const uint32_t slab_flip = (SPLIT_SIGNED_WGRAD && (bz & 1)) ? 0x80000000u : 0u;      // workgroup-uniform
  if constexpr (NP == 2) sc_a = __uint_as_float(__float_as_uint(sc_a) ^ slab_flip);
  // SG / RS: the loop copy's sign and row-sum modes (see above)
  // (o0: the thread's chunk in the A image of stage 0)
  auto split_store = [&](auto SG, auto RS, const Regs& r, u32x4* o0, int st, bool keep) __attribute__((always_inline)) {
    constexpr int sg = decltype(SG)::value, rsm = decltype(RS)::value;
    const float xa[8] = {r.a0.x, r.a0.y, r.a0.z, r.a0.w, r.a1.x, r.a1.y, r.a1.z, r.a1.w};
    const float xb[8] = {r.b0.x, r.b0.y, r.b0.z, r.b0.w, r.b1.x, r.b1.y, r.b1.z, r.b1.w};
    // bias gradient: row sums of the staged dY values (a select, not a product: the surplus split of the
    // last tile works on stale registers that may hold NaNs)
    if constexpr (rsm != 0) {
      const float add = ((xa[0] + xa[1]) + (xa[2] + xa[3])) + ((xa[4] + xa[5]) + (xa[6] + xa[7]));
      rs += keep ? add : 0.f;
    }
    u32x4* o = o0 + st * 2 * SIMGP;
    if constexpr (NP == 3) {
      u32x4 ha, ma, la, hb, mb, lb;
      // sign alternation by slab: odd K-ranges accumulate -dW
      if constexpr (sg == 2) {
        float xs[8];
        flip8(xs, xa, slab_flip);
        split8(xs, ha, ma, la);
      } else {
        split8s<sg == 1>(xa, ha, ma, la);
      }
      split8(xb, hb, mb, lb);
      o[0] = ha; o[2 * SCHP] = ma; o[4 * SCHP] = la;
      o += SIMGP;
      o[0] = hb; o[2 * SCHP] = mb; o[4 * SCHP] = lb;
    } else if constexpr (NP == 1) {
      float xs[8];
      flip8(xs, xa, slab_flip);
      o[0] = round8(xs);
      o[SIMGP] = round8(xb);
    } else {
      u32x4 ha, la, hb, lb;
      split8_f16(xa, sc_a, ha, la);
      split8_f16(xb, sc_b, hb, lb);
      o[0] = ha; o[2 * SCHP] = la;
      o += SIMGP;
      o[0] = hb; o[2 * SCHP] = lb;
    }
  };

  f32x16 acc[2][2];
  // the prologue, the k-loop and the closing negation of a negated slab: one copy per (sign, row sums)
  auto run = [&](auto SG, auto RS) __attribute__((always_inline)) {
    constexpr int sg = decltype(SG)::value, rsm = decltype(RS)::value;
    const bool rsum = rsm == 2 ? do_rowsum : true;        // (rsm = 0: unused)
    // (a zero of the copy's own: one shared block of sixteen zeros ahead of the branch reaches later copies through scratch)
    float zero = 0.f;
    if constexpr (sg != 2 || rsm != 2) asm volatile("" : "+v"(zero));
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][j][r] = zero;
    // (with several copies, each derives its lane values afresh from the thread index, as the epilogue does: values
    //  shared between the copies stay live through all of them, beside 168 registers of loop)
    int ot = tid;
    if constexpr (sg != 2 || rsm != 2) asm volatile("" : "+v"(ot));
    const int lwm = (ot >> 7) & 1, lwn = (ot >> 6) & 1, lli = ot & 31, llh = (ot >> 5) & 1;
    const int srow = ot >> 1, sh = ot & 1;      // the staged row (clamped to the matrix) and k-half
    u32x4* const o0 = img + sh * SCHP + srow;
    const float* const Ag = SADDR ? nullptr : g.A + (int64_t)min(m0 + srow, g.M - 1) * g.lda + sh * 8;
    const float* const Bg = SADDR ? nullptr : g.B + (int64_t)min(n0 + srow, g.N - 1) * g.ldb + sh * 8;
    const uint32_t voa = ((uint32_t)min(srow, g.M - 1 - m0) * (uint32_t)g.lda + (uint32_t)(sh * 8)) * 4u;      // (host: 128 lda < 2^29)
    const uint32_t vob = ((uint32_t)min(srow, g.N - 1 - n0) * (uint32_t)g.ldb + (uint32_t)(sh * 8)) * 4u;
    // (the loads' state and registers belong to the copy: nothing but acc and rs is live where the copies meet)
    int f_ib = f_ib0, f_kt = f_kt0;
    const float* sa = sa0;
    const float* sb = sb0;
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    Regs r0{zero4, zero4, zero4, zero4}, r1 = r0;   // defined values: the surplus split of a one-tile range reads r1
    auto fetch = [&](Regs& r) __attribute__((always_inline)) {
      if constexpr (SADDR) {
        asm volatile("global_load_dwordx4 %0, %1, %2" : "=&v"(r.a0) : "v"(voa), "s"(sa) : "memory");
        asm volatile("global_load_dwordx4 %0, %1, %2 offset:16" : "=&v"(r.a1) : "v"(voa), "s"(sa) : "memory");
        asm volatile("global_load_dwordx4 %0, %1, %2" : "=&v"(r.b0) : "v"(vob), "s"(sb) : "memory");
        asm volatile("global_load_dwordx4 %0, %1, %2 offset:16" : "=&v"(r.b1) : "v"(vob), "s"(sb) : "memory");
        sa += SBK; sb += SBK;
        if (++f_kt == KT) { f_kt = 0; sa += wrap_a; sb += wrap_b; }
      } else {
        const float* a = Ag + (int64_t)f_ib * g.a_is + (int64_t)f_kt * SBK;
        const float* b = Bg + (int64_t)f_ib * g.b_is + (int64_t)f_kt * SBK;
        asm volatile("global_load_dwordx4 %0, %1, off" : "=&v"(r.a0) : "v"(a) : "memory");
        asm volatile("global_load_dwordx4 %0, %1, off offset:16" : "=&v"(r.a1) : "v"(a) : "memory");
        asm volatile("global_load_dwordx4 %0, %1, off" : "=&v"(r.b0) : "v"(b) : "memory");
        asm volatile("global_load_dwordx4 %0, %1, off offset:16" : "=&v"(r.b1) : "v"(b) : "memory");
        if (++f_kt == KT) { f_kt = 0; ++f_ib; }
      }
    };
    if (T > 0) {
      fetch(r0);
      if (T > 1) { fetch(r1); USE_R(r0, 4); } else { USE_R(r0, 0); }
      split_store(SG, RS, r0, o0, 0, rsum);
    }
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");

    auto step = [&](int t, int cur, Regs& rload, Regs& rsplit) __attribute__((always_inline)) {
      const u32x4* As = img + cur * 2 * SIMGP + llh * SCHP + lwm * 64 + lli;
      const u32x4* Bs = img + (cur * 2 + 1) * SIMGP + llh * SCHP + lwn * 64 + lli;
      SplitFrags<NP> f;
      split_tile_read<NP, 2 * SCHP, 2 * SCHP>(As, Bs, f);
      __builtin_amdgcn_sched_barrier(0);
      if (t + 2 < T) { fetch(rload); USE_R(rsplit, 4); }
      else USE_R(rsplit, 0);
      // one basic block for every tile; the last tile's split is surplus (stage nobody reads, keep = 0)
      split_tile_mfma<NP>(f, acc);
      split_store(SG, RS, rsplit, o0, cur ^ 1, rsum && t + 1 < T);
      if constexpr (NP > 1) {
#pragma unroll
        for (int i = 0; i < (NP == 3 ? 24 : 12); ++i) {
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);   // one MFMA
          __builtin_amdgcn_sched_group_barrier(0x002, 5, 0);   // five VALU of the two splits
        }
      }
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    };
    for (int t = 0; t < T; t += 2) {
      step(t, 0, r0, r1);
      if (t + 1 < T) step(t + 1, 1, r1, r0);
    }
    if (sg == 1 || (sg == 2 && slab_flip)) {
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[i][j][r] = -acc[i][j][r];
    }
  };
  {
    using std::integral_constant;
    constexpr integral_constant<int, SIGN_COPIES ? 0 : 2> plain;
    constexpr integral_constant<int, SIGN_COPIES ? 1 : 2> negated;
    constexpr integral_constant<int, ROWSUM_COPIES ? 0 : 2> no_sums;
    constexpr integral_constant<int, ROWSUM_COPIES ? 1 : 2> sums;
    const bool neg = SIGN_COPIES && slab_flip != 0, with_sums = ROWSUM_COPIES && do_rowsum;      // workgroup-uniform
    if (with_sums) {
      if (neg) run(negated, sums); else run(plain, sums);
    } else {
      if (neg) run(negated, no_sums); else run(plain, no_sums);
    }
  }
#undef USE_R
  if (do_rowsum) {
    int t = tid;
    if constexpr (SIGN_COPIES || ROWSUM_COPIES) asm volatile("" : "+v"(t));
    rs += __shfl_xor(rs, 1, 64);
    const int m = m0 + (t >> 1);
    if ((t & 1) == 0 && m < g.M) g.rowsum[(int64_t)bz * g.M + m] = rs;
  }
  if constexpr (NP == 2) split_unscale(acc, inv_a, inv_b);
  if constexpr (SIGN_COPIES || ROWSUM_COPIES || (NP == 3 && SPLIT_WGRAD_EPILOGUE)) {
    int t = tid;      // (the epilogue's lane values, derived afresh: see pw_gemm_split_wide_kernel)
    asm volatile("" : "+v"(t));
    const int ew = __builtin_amdgcn_readfirstlane((t >> 6) & 3), ewm = ew >> 1, ewn = ew & 1, eli = t & 31, elh = (t >> 5) & 1;
    // an interior tile of a slab or of dW is a plain store: the straight-line epilogue of the forward kernel, no options
    if (NP == 3 && SPLIT_WGRAD_EPILOGUE && !g.generic_epilogue && m0 + BM <= g.M && n0 + BN <= g.N)
      split_epilogue_interior<EP_ON>(g, acc, bz, m0, n0, ewm, ewn, eli, elh);
    else
      gemm_epilogue(g, acc, bz, m0, n0, ewm, ewn, eli, elh);
  } else {
    gemm_epilogue(g, acc, bz, m0, n0, wm, wn, li, lh);
  }
}

// ---- host side: reserve LDS once per device, pick the instantiation, launch -------------------------------------------
typedef void (*GemmKernel)(GemmArgs);
// the four instantiations of a kernel template over two I/O-type flags, indexed a + 2 * b
#define IO2_KERNELS(K) {&K<false, false>, &K<true, false>, &K<false, true>, &K<true, true>}

// a dynamic-LDS request above 64 KiB has to be granted per kernel and device
inline int reserve_lds(GemmKernel k, size_t bytes, const char* what) {
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) == hipSuccess) return 0;
  paradis_set_error("%s: cannot reserve LDS", what);
  return 2;
}
// ... `bytes` on every kernel of `ks`, once per device (`once`: one per kernel family)
inline int reserve_lds(PerDeviceOnce& once, std::initializer_list<GemmKernel> ks, size_t bytes, const char* what) {
  if (!once.first()) return 0;
  for (GemmKernel k : ks)
    if (int e = reserve_lds(k, bytes, what)) return e;
  return 0;
}

// KS = IO2_KERNELS(family): launch the instantiation that (a, b) selects; reserve_for: the name for the error message
// if the family's `lds` bytes need reserving (on all four), nullptr if they fit the 64 KiB a kernel gets unasked
template <const GemmKernel (&KS)[4]>
int launch_io2(bool a, bool b, dim3 grid, dim3 block, size_t lds, const char* reserve_for, hipStream_t st, const GemmArgs& g) {
  static PerDeviceOnce once;
  if (reserve_for)
    if (int e = reserve_lds(once, {KS[0], KS[1], KS[2], KS[3]}, lds, reserve_for)) return e;
  hipLaunchKernelGGL(KS[a + 2 * b], grid, block, lds, st, g);
  return 0;
}

// A kernel family as ONE constexpr table indexed by its template parameters: the launch indexes it, the reservation walks
// it (`once`: one per table).  lds: the dynamic LDS the entry's launches may ask for, reserved if above 64 KiB; k == nullptr:
// a combination of parameters that nobody instantiates.
struct GemmKernelEntry { GemmKernel k; size_t lds; };
template <int N>
int reserve_lds(PerDeviceOnce& once, const GemmKernelEntry (&tab)[N], const char* what) {
  bool any = false;
  for (const GemmKernelEntry& e : tab) any = any || (e.k && e.lds > 64 * 1024);
  if (!any || !once.first()) return 0;
  for (const GemmKernelEntry& e : tab)
    if (e.k && e.lds > 64 * 1024)
      if (int err = reserve_lds(e.k, e.lds, what)) return err;
  return 0;
}
// launch entry i with the entry's LDS bytes, or with `lds` of them if given (a request that varies at run time)
template <int N>
int launch_entry(const GemmKernelEntry (&tab)[N], int i, PerDeviceOnce& once, const char* what, int grid, int block,
                 hipStream_t st, const GemmArgs& g, size_t lds = 0) {
  if (i < 0 || i >= N || tab[i].k == nullptr) { paradis_set_error("%s: no kernel for index %d", what, i); return 1; }
  if (int e = reserve_lds(once, tab, what)) return e;
  hipLaunchKernelGGL(tab[i].k, dim3(grid), dim3(block), lds ? lds : tab[i].lds, st, g);
  return 0;
}

// ---- host side: LDS bytes of the weight-gradient kernels (their launchers and the plan below) --------------------------------
constexpr int DBK = 16;                 // k-tile depth of the LDS-DMA f32 kernels (gemm_exact.hip)
constexpr int DTILE = DBK * BM;         // floats per operand per stage (pitch 128, unpadded)
constexpr size_t dma_lds_bytes(int stages) { return (size_t)stages * 2 * DTILE * sizeof(float); }
// register-staged f32 kernel: floats per operand per stage (upper bound), bytes of its two stages, and what a launch asks
// for - the dynamic-LDS request doubles as the occupancy control: 160 KiB / request = workgroups per CU
constexpr int stage_floats(int bk) { return bk * (BM + 4); }
constexpr size_t lds_bytes(int bk) { return (size_t)4 * stage_floats(bk) * sizeof(float); }
constexpr size_t STAGED_LDS_MAX = 160 * 1024;
inline size_t staged_lds_request(int bk, int wg_per_cu) {
  return std::min(std::max(lds_bytes(bk), (size_t)(160 * 1024 / wg_per_cu) & ~(size_t)255), STAGED_LDS_MAX);
}
constexpr size_t split_lds_wgrad(int np) { return (size_t)2 * 2 * simgp(np) * 16; }
// bf16-mixed 256 x 128 and 256 x 256 tiles (gemm_amp_wgrad.hip): row pitches and stage sizes in chunks
constexpr int TALL_PA = 256 + 8, TALL_PB = 128 + 8, TALL_STAGE = 2 * TALL_PA + 2 * TALL_PB;
constexpr size_t tall_lds_bytes() { return (size_t)2 * TALL_STAGE * 16; }
constexpr int SQ_P = 256 + 8, SQ_STAGE = 4 * SQ_P;
constexpr size_t sq_lds_bytes() { return (size_t)4 * SQ_STAGE * 16; }

// ---- the weight gradient's plan: dW[M,K] = sum_b dY[b][M,N] . X[b][K,N]^T ---------------------------------------------------
// ONE place decides which kernel runs, how many K-range slabs it writes, its launch geometry, whether it fuses the bias
// gradient's row sums and where slabs and row sums live in the workspace.  paradis_pw_gemm_wgrad launches from it,
// paradis_pw_gemm_wgrad_ws_bytes / _slabs ask it, tools/gemm_plan_check.hip holds it against the rules it replaced.
// Host only: nothing here touches the device.

// PARADIS_WGRAD_TALL=0 / PARADIS_WGRAD_SQUARE=0 switch the bf16-mixed scheme's larger tiles off (A/B runs); read once
struct WgradEnv { bool tall, square; };
inline WgradEnv wgrad_env() {
  static const WgradEnv env = [] {
    const char *t = getenv("PARADIS_WGRAD_TALL"), *s = getenv("PARADIS_WGRAD_SQUARE");
    return WgradEnv{!(t && t[0] == '0'), !(s && s[0] == '0')};
  }();
  return env;
}

// output tile, k depth, resident workgroups per CU, threads and dynamic LDS of a kind's kernel
struct WgradTile { int th, tw, kd, wg_per_cu, block; size_t lds; };
inline WgradTile wgrad_tile(WgradKind kind, const GemmTunables& t) {
  switch (kind) {
    case WgradKind::Staged: return {BM, BN, t.bk, t.wg_per_cu, 256, staged_lds_request(t.bk, t.wg_per_cu)};
    case WgradKind::Dma:    return {BM, BN, DBK, t.wgrad_dma_stages == 2 ? 4 : 3, 256, dma_lds_bytes(t.wgrad_dma_stages)};
    case WgradKind::Bf16x3: return {BM, BN, SBK, 3, 256, split_lds_wgrad(3)};
    case WgradKind::F16x2:  return {BM, BN, SBK, 3, 256, split_lds_wgrad(2)};
    case WgradKind::Amp128: return {BM, BN, SBK, 3, 256, split_lds_wgrad(1)};
    case WgradKind::Tall:   return {256, BN, SBK, 2, 512, tall_lds_bytes()};
    case WgradKind::Square: return {256, 256, SBK, 1, 512, sq_lds_bytes()};
  }
  return {};
}
constexpr WgradKind WGRAD_KINDS[] = {WgradKind::Staged, WgradKind::Dma,  WgradKind::Bf16x3, WgradKind::F16x2,
                                     WgradKind::Amp128, WgradKind::Tall, WgradKind::Square};

// number of K-range slabs: one round of resident workgroups over the 256 CUs
inline int wgrad_splits(int B, int M, int K, int N, const WgradTile& tl) {
  const int tiles = ((M + tl.th - 1) / tl.th) * ((K + tl.tw - 1) / tl.tw);
  const int64_t total_kt = (int64_t)B * ((N + tl.kd - 1) / tl.kd);
  int s = (int)std::max<int64_t>(1, std::min<int64_t>(256 * tl.wg_per_cu / tiles, total_kt));
  // the split kernels accumulate alternate slabs with opposite sign so that the bf16 MFMA's alignment offset cancels
  // in the slab sum ("sign checkerboard"): that takes an even number of slabs (1536 x 384: 21 -> 20; round 5)
  if (s > 1) s &= ~1;
  return s;
}

// the tile wastes at most ~1/7 of its 256 rows / columns
inline bool wgrad_fills_256(int n) { return ((n + 255) / 256) * 256 * 7 <= n * 8; }

// dy_bs / x_bs: sample strides in elements; dY / X: alignment only
inline WgradKind wgrad_kind(int M, int K, int N, int64_t dy_bs, int64_t x_bs, const void* dY, const void* X, int scheme,
                            int io16, const GemmTunables& t, WgradEnv env) {
  // both operands p-contiguous with whole, 16-B aligned 16-float chunks (LDS-DMA and split kernels)
  const bool vec = N % DBK == 0 && (dy_bs & 3) == 0 && (x_bs & 3) == 0 && aligned16(dY) && aligned16(X);
  // a split scheme: both operands are split in registers; bf16-stored operands (io16) were checked by the caller
  if (io16 != 0 || (scheme != PARADIS_GEMM_EXACT && vec)) {
    if (scheme == PARADIS_GEMM_BF16) {
      const bool tall = env.tall && M >= 256 && wgrad_fills_256(M);
      return tall && env.square && wgrad_fills_256(K) ? WgradKind::Square : tall ? WgradKind::Tall : WgradKind::Amp128;
    }
    return scheme == PARADIS_GEMM_F16X2 ? WgradKind::F16x2 : WgradKind::Bf16x3;
  }
  return t.wgrad_dma_stages >= 2 && vec ? WgradKind::Dma : WgradKind::Staged;
}

inline WgradPlan wgrad_plan_of(WgradKind kind, int B, int M, int K, int N, const GemmTunables& t) {
  const WgradTile tl = wgrad_tile(kind, t);
  const int S = wgrad_splits(B, M, K, N, tl), grid = ((M + tl.th - 1) / tl.th) * ((K + tl.tw - 1) / tl.tw) * S;
  return {kind, S, grid, tl.block, tl.lds, kind != WgradKind::Staged, S > 1, {S, M, K}};
}

inline WgradPlan wgrad_plan(int B, int M, int K, int N, int64_t dy_bs, int64_t x_bs, const void* dY, const void* X, int scheme,
                            int io16, const GemmTunables& t, WgradEnv env) {
  return wgrad_plan_of(wgrad_kind(M, K, N, dy_bs, x_bs, dY, X, scheme, io16, t, env), B, M, K, N, t);
}

// Workspace bytes for a shape: the largest over EVERY kind.  The query sees neither pointers, strides, scheme nor the
// switches, and the value is part of what callers (ops.py, muon.hip) size buffers from: it stays what it always was.
inline size_t wgrad_ws_bytes(int B, int M, int K, int N, const GemmTunables& t) {
  size_t bytes = 0;
  for (WgradKind kind : WGRAD_KINDS) bytes = std::max(bytes, wgrad_plan_of(kind, std::max(B, 1), M, K, N, t).ws.bytes());
  return bytes;
}

// slab_reduce_kernel's launch: slab sums in a fixed order over blocks1 workgroups (n = 0: one slab, the GEMM wrote dW itself),
// the row sums' reduction riding along in blocks2 more
struct SlabReduce { int64_t n; int vec, blocks1, n2, blocks2; };
inline SlabReduce wgrad_reduce(const WgradPlan& p, const void* workspace, const void* dW, bool rowsums) {
  const int64_t n = p.to_slabs ? (int64_t)p.ws.M * p.ws.K : 0;
  const int vec = n % 4 == 0 && aligned16(workspace) && aligned16(dW);
  const int n2 = rowsums ? p.ws.M : 0;
  return {n, vec, n ? (int)std::min<int64_t>(((vec ? n / 4 : n) + 255) / 256, 2048) : 0, n2, (n2 + 255) / 256};
}
}  // namespace
