// Host-only check of the weight gradient's plan (runs without a GPU; nothing is launched, no pointer is dereferenced):
// what pw_gemm_wgrad_impl, paradis_pw_gemm_wgrad_ws_bytes and paradis_pw_gemm_wgrad_slabs of csrc/gemm.hip decided
// before the split into gemm.hip / gemm_exact.hip / gemm_split.hip - the predicates and the wgrad_splits* functions below
// are that file's, copied, with its tunables as a struct - against wgrad_plan, wgrad_ws_bytes and wgrad_reduce of
// gemm_common.h.  Kernel, slab count, grid, block, LDS bytes, fused or separate row sums, output target, row-sum offset,
// the slab reduction's geometry and the two queries have to agree for every shape, alignment, stride, scheme, io16 and
// setting of the tunables.  The two environment switches are read once per process: one run per setting, with the
// sanitizers on the host side:
//   hipcc --cuda-host-only -O1 -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -I paradis_model_amd/csrc tools/gemm_plan_check.hip -o build/gemm_plan_check
//   for t in 1 0; do for s in 1 0; do PARADIS_WGRAD_TALL=$t PARADIS_WGRAD_SQUARE=$s build/gemm_plan_check; done; done
// It also prints the kernel chosen for each shape of test_wgrad_every_kind_exact (tests/test_hip_kernel_edges.py) and
// fails unless all seven kinds occur among them (with both switches on).
#include <stdio.h>
#include <utility>
#include <vector>
#include "gemm_common.h"

namespace before {   // ---- the single unit's tunables, predicates and slab rules --------------------------------------------

int g_bk = 16, g_wg_per_cu = 4, g_wgrad_dma_stages = 2;
constexpr int DBK = 16, SBK = 16, BM = 128, BN = 128;
constexpr int DTILE = DBK * BM;
constexpr int stage_floats(int bk) { return bk * (BM + 4); }
constexpr size_t lds_bytes(int bk) { return (size_t)4 * stage_floats(bk) * sizeof(float); }
constexpr int simgp(int np) { return np * 2 * (128 + 8); }
constexpr size_t split_lds_wgrad(int np) { return (size_t)2 * 2 * simgp(np) * 16; }
constexpr int TALL_PA = 256 + 8, TALL_PB = 128 + 8, TALL_STAGE = 2 * TALL_PA + 2 * TALL_PB;
constexpr size_t tall_lds_bytes() { return (size_t)2 * TALL_STAGE * 16; }
constexpr int SQ_P = 256 + 8, SQ_STAGE = 4 * SQ_P;
constexpr size_t sq_lds_bytes() { return (size_t)4 * SQ_STAGE * 16; }

bool wgrad_vec_layout(int N, int64_t dy_bs, int64_t x_bs, const void* a, const void* b) {
  auto a16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
  return N % DBK == 0 && (dy_bs & 3) == 0 && (x_bs & 3) == 0 && a16(a) && a16(b);
}
bool wgrad_dma_ok(int N, int64_t dy_bs, int64_t x_bs, const void* a, const void* b) {
  return g_wgrad_dma_stages >= 2 && wgrad_vec_layout(N, dy_bs, x_bs, a, b);
}
int wgrad_splits(int B, int M, int K, int N, int bk, int wg_per_cu) {
  const int tiles = ((M + BM - 1) / BM) * ((K + BN - 1) / BN);
  const int64_t total_kt = (int64_t)B * ((N + bk - 1) / bk);
  int s = (int)std::max<int64_t>(1, std::min<int64_t>(256 * wg_per_cu / tiles, total_kt));
  if (s > 1) s &= ~1;
  return s;
}
int wgrad_dma_wgs() { return g_wgrad_dma_stages == 2 ? 4 : 3; }
bool wgrad_tall_ok(int M) {
  static const bool on = [] { const char* e = getenv("PARADIS_WGRAD_TALL"); return !(e && e[0] == '0'); }();
  return on && M >= 256 && ((M + 255) / 256) * 256 * 7 <= M * 8;
}
bool wgrad_square_on() {
  static const bool on = [] { const char* e = getenv("PARADIS_WGRAD_SQUARE"); return !(e && e[0] == '0'); }();
  return on;
}
int wgrad_splits_square(int B, int M, int K, int N) {
  const int tiles = ((M + 255) / 256) * ((K + 255) / 256);
  const int64_t total_kt = (int64_t)B * ((N + SBK - 1) / SBK);
  int s = (int)std::max<int64_t>(1, std::min<int64_t>(256 / tiles, total_kt));
  if (s > 1) s &= ~1;
  return s;
}
int wgrad_splits_tall(int B, int M, int K, int N) {
  const int tiles = ((M + 255) / 256) * ((K + BN - 1) / BN);
  const int64_t total_kt = (int64_t)B * ((N + SBK - 1) / SBK);
  int s = (int)std::max<int64_t>(1, std::min<int64_t>(512 / tiles, total_kt));
  if (s > 1) s &= ~1;
  return s;
}

size_t ws_bytes(int B, int M, int K, int N) {
  const int b = std::max(B, 1);
  const int S = std::max({wgrad_splits(b, M, K, N, DBK, wgrad_dma_wgs()), wgrad_splits(b, M, K, N, g_bk, g_wg_per_cu),
                          wgrad_splits(b, M, K, N, SBK, 3), wgrad_splits_tall(b, M, K, N),
                          wgrad_splits_square(b, M, K, N)});
  return (size_t)S * M * ((size_t)K + 1) * sizeof(float) + 256;
}
int slabs(int B, int M, int K, int N) {
  if (M < 1 || K < 1 || N < 1) return 0;
  return wgrad_splits(std::max(B, 1), M, K, N, SBK, 3);
}

}  // namespace before

// everything one call of paradis_pw_gemm_wgrad (B >= 1) does on the host side
struct Call {
  int kind = -1, S = 0, grid = 0, block = 0;
  size_t lds = 0, rowsum_offset = 0;      // offset in floats
  bool bias_pass = false, fused = false, to_slabs = false;
  int64_t n = 0;
  int vec = 0, blocks1 = 0, n2 = 0, blocks2 = 0;
  bool operator==(const Call& o) const {
    return kind == o.kind && S == o.S && grid == o.grid && block == o.block && lds == o.lds && rowsum_offset == o.rowsum_offset &&
           bias_pass == o.bias_pass && fused == o.fused && to_slabs == o.to_slabs && n == o.n && vec == o.vec &&
           blocks1 == o.blocks1 && n2 == o.n2 && blocks2 == o.blocks2;
  }
};
struct Case {
  int B, M, K, N, scheme, io16;
  int64_t dy_bs, x_bs;
  const void *dY, *X, *ws, *dW;
  bool gbias;
};

namespace before {
// pw_gemm_wgrad_impl from "a split scheme" on, with each launch recorded instead of made
Call wgrad(const Case& c) {
  using namespace before;
  const int B = c.B, M = c.M, K = c.K, N = c.N, scheme = c.scheme, io16 = c.io16;
  Call r;
  const bool use_split = io16 != 0 || (scheme != PARADIS_GEMM_EXACT && wgrad_vec_layout(N, c.dy_bs, c.x_bs, c.dY, c.X));
  const bool dma = use_split || wgrad_dma_ok(N, c.dy_bs, c.x_bs, c.dY, c.X);
  const bool tall = use_split && scheme == PARADIS_GEMM_BF16 && wgrad_tall_ok(M);
  const bool square = tall && wgrad_square_on() && ((K + 255) / 256) * 256 * 7 <= K * 8;
  const int S = square ? wgrad_splits_square(B, M, K, N) : tall ? wgrad_splits_tall(B, M, K, N)
              : use_split ? wgrad_splits(B, M, K, N, SBK, 3)
                          : dma ? wgrad_splits(B, M, K, N, DBK, wgrad_dma_wgs())
                                : wgrad_splits(B, M, K, N, g_bk, g_wg_per_cu);
  r.S = S;
  r.rowsum_offset = (size_t)S * M * K;
  r.bias_pass = c.gbias && !dma;
  r.to_slabs = S > 1;
  r.fused = c.gbias && dma;
  const int grid = (tall ? (M + 255) / 256 : (M + BM - 1) / BM) * ((K + BN - 1) / BN) * S;
  r.grid = grid; r.block = 256;
  if (square || tall) {
    r.grid = square ? ((M + 255) / 256) * ((K + 255) / 256) * S : grid;
    r.kind = square ? (int)WgradKind::Square : (int)WgradKind::Tall;
    r.block = 512; r.lds = square ? sq_lds_bytes() : tall_lds_bytes();
  } else if (use_split && scheme == PARADIS_GEMM_F16X2) {
    r.kind = (int)WgradKind::F16x2; r.lds = split_lds_wgrad(2);
  } else if (use_split && scheme == PARADIS_GEMM_BF16) {
    r.kind = (int)WgradKind::Amp128; r.lds = (size_t)2 * 2 * simgp(1) * 16;
  } else if (use_split) {
    r.kind = (int)WgradKind::Bf16x3; r.lds = split_lds_wgrad(3);
  } else if (dma) {
    r.kind = (int)WgradKind::Dma;
    r.lds = g_wgrad_dma_stages == 2 ? (size_t)g_wgrad_dma_stages * 2 * DTILE * sizeof(float) : (size_t)3 * 2 * DTILE * sizeof(float);
  } else {
    r.kind = (int)WgradKind::Staged;
    size_t request = std::max(lds_bytes(g_bk), (size_t)(160 * 1024 / g_wg_per_cu) & ~(size_t)255);
    r.lds = std::min(request, (size_t)160 * 1024);
  }
  r.n = S > 1 ? (int64_t)M * K : 0;
  r.vec = r.n % 4 == 0 && ((reinterpret_cast<uintptr_t>(c.ws) | reinterpret_cast<uintptr_t>(c.dW)) & 15) == 0;
  r.blocks1 = r.n ? (int)std::min<int64_t>(((r.vec ? r.n / 4 : r.n) + 255) / 256, 2048) : 0;
  r.n2 = r.fused ? M : 0;
  r.blocks2 = (r.n2 + 255) / 256;
  return r;
}
}  // namespace before

namespace after {   // ---- pw_gemm_wgrad_impl over wgrad_plan ------------------------------------------------------------------
Call wgrad(const Case& c, const GemmTunables& t) {
  const WgradPlan p = wgrad_plan(c.B, c.M, c.K, c.N, c.dy_bs, c.x_bs, c.dY, c.X, c.scheme, c.io16, t, wgrad_env());
  const bool rowsums = c.gbias && p.fused_rowsums;
  const SlabReduce s = wgrad_reduce(p, c.ws, c.dW, rowsums);
  Call r;
  r.kind = (int)p.kind; r.S = p.S; r.grid = p.grid; r.block = p.block; r.lds = p.lds;
  r.rowsum_offset = p.ws.rowsum_offset();
  r.bias_pass = c.gbias && !rowsums; r.fused = rowsums; r.to_slabs = p.to_slabs;
  r.n = s.n; r.vec = s.vec; r.blocks1 = s.blocks1; r.n2 = s.n2; r.blocks2 = s.blocks2;
  return r;
}
}  // namespace after

static long long cases = 0, failures = 0;
static void expect(bool ok, const char* what, const Case& c, const GemmTunables& t) {
  ++cases;
  if (ok) return;
  if (++failures <= 20)
    fprintf(stderr, "MISMATCH %s: B=%d M=%d K=%d N=%d scheme=%d io16=%d dy_bs=%lld x_bs=%lld dY=%p X=%p bk=%d wg=%d wdma=%d\n", what,
            c.B, c.M, c.K, c.N, c.scheme, c.io16, (long long)c.dy_bs, (long long)c.x_bs, c.dY, c.X, t.bk, t.wg_per_cu,
            t.wgrad_dma_stages);
}

static const char* KIND_NAME[] = {"register-staged", "f32 DMA", "bf16x3 split", "f16x2 split", "bf16-mixed 128x128", "tall", "square"};

int main() {
  const uintptr_t base = (uintptr_t)1 << 40;      // never dereferenced
  auto at = [&](int tensor, int off) { return reinterpret_cast<const void*>(base + ((uintptr_t)tensor << 36) + (uintptr_t)off); };
  // what a call with bf16-stored operands has to satisfy (pw_gemm_wgrad_impl's PD_REQUIRE)
  auto io16_legal = [](const Case& c) {
    return c.scheme == PARADIS_GEMM_BF16 && c.N % 16 == 0 && aligned16(c.dY) && aligned16(c.X) &&
           c.dy_bs % ((c.io16 & IO_A16) ? 8 : 4) == 0 && c.x_bs % ((c.io16 & IO_B16) ? 8 : 4) == 0;
  };
  const int SCHEME_IO[][2] = {{PARADIS_GEMM_EXACT, 0}, {PARADIS_GEMM_BF16X3, 0}, {PARADIS_GEMM_F16X2, 0}, {PARADIS_GEMM_BF16, 0},
                              {PARADIS_GEMM_BF16, IO_B16}, {PARADIS_GEMM_BF16, IO_A16}, {PARADIS_GEMM_BF16, IO_A16 | IO_B16}};
  // shapes (M, K): the model's layers (tests/test_abi_and_host.py), ragged ones, and a sweep around the tile edges
  std::vector<std::pair<int, int>> MK = {{1024, 186}, {384, 1024}, {1536, 384}, {768, 1024}, {1024, 768}, {1024, 1024}, {896, 1152},
                                         {896, 896}, {1024, 896}, {768, 768}, {97, 768}, {2048, 1536}, {128, 128}, {640, 640},
                                         {5, 3}, {1, 1}, {97, 13}, {333, 7}, {2500, 2500}, {4096, 3000}, {256, 8}, {256, 224}};
  const int EDGE[] = {127, 128, 129, 224, 255, 256, 257, 447, 448, 449, 511, 512, 513};
  for (int m : EDGE)
    for (int k : EDGE) MK.push_back({m, k});
  const int NS[] = {1, 15, 16, 17, 31, 32, 33, 48, 60, 64, 2048, 32768, 721 * 1440};
  const int BS[] = {0, 1, 2, 4, 32};
  const int PTR[] = {0, 4, 8};          // mod 16
  const int STR[] = {0, 2, 4};          // added to the dense batch stride: mod 8 for N % 8 == 0

  for (int bk : {16, 32})
    for (int wg = 1; wg <= 4; ++wg)
      for (int wdma : {0, 2, 3}) {
        const GemmTunables t{bk, wg, 0, 3, wdma};
        before::g_bk = bk; before::g_wg_per_cu = wg; before::g_wgrad_dma_stages = wdma;
        for (const auto& mk : MK)
          for (int N : NS)
            for (int B : BS) {
              Case c{};
              c.B = B; c.M = mk.first; c.K = mk.second; c.N = N;
              expect(before::ws_bytes(B, c.M, c.K, N) == wgrad_ws_bytes(B, c.M, c.K, N, t), "ws_bytes", c, t);
              expect(before::slabs(B, c.M, c.K, N) == wgrad_plan_of(WgradKind::Bf16x3, std::max(B, 1), c.M, c.K, N, t).S, "slabs", c, t);
              if (B == 0) continue;      // the entry point zero-fills and returns before it plans
              for (const auto& si : SCHEME_IO)
                for (int pa : PTR)
                  for (int pb : PTR)
                    for (int sa : STR)
                      for (int sb : STR) {
                        c.scheme = si[0]; c.io16 = si[1];
                        c.dY = at(1, pa); c.X = at(2, pb);
                        c.dy_bs = (int64_t)c.M * N + sa; c.x_bs = (int64_t)c.K * N + sb;
                        if (c.io16 && !io16_legal(c)) continue;
                        // workspace / dW alignment and the bias gradient only reach the slab reduction: vary them along
                        c.ws = at(3, (pa + sb) & 4 ? 4 : 0); c.dW = at(4, (pb + sa) & 8 ? 8 : 0);
                        c.gbias = ((pa >> 2) + (sa >> 1) + B) & 1;
                        const Call b0 = before::wgrad(c), b1 = after::wgrad(c, t);
                        expect(b0 == b1, "wgrad", c, t);
                        expect((size_t)(b1.rowsum_offset + (size_t)b1.S * c.M) * sizeof(float) <= wgrad_ws_bytes(B, c.M, c.K, N, t),
                               "workspace holds slabs and row sums", c, t);
                      }
            }
      }

  // the shapes of test_wgrad_every_kind_exact: (scheme, io16, B, Co, Ci, P), dense and 16-byte aligned, default tunables
  const GemmTunables def{16, 4, 0, 3, 2};
  const int T5[][6] = {{PARADIS_GEMM_EXACT, 0, 2, 5, 3, 60},  {PARADIS_GEMM_EXACT, 0, 2, 5, 3, 64},  {PARADIS_GEMM_EXACT, 0, 1, 5, 3, 16},
                       {PARADIS_GEMM_BF16X3, 0, 2, 5, 3, 64}, {PARADIS_GEMM_BF16X3, 0, 1, 5, 3, 16}, {PARADIS_GEMM_F16X2, 0, 2, 5, 3, 64},
                       {PARADIS_GEMM_F16X2, 0, 1, 5, 3, 16},  {PARADIS_GEMM_BF16, 0, 2, 5, 3, 64},   {PARADIS_GEMM_BF16, IO_A16, 2, 5, 3, 64},
                       {PARADIS_GEMM_BF16, IO_B16, 2, 5, 3, 64}, {PARADIS_GEMM_BF16, IO_A16 | IO_B16, 2, 5, 3, 64},
                       {PARADIS_GEMM_BF16, 0, 2, 256, 8, 32}, {PARADIS_GEMM_BF16, 0, 2, 448, 8, 32}, {PARADIS_GEMM_BF16, 0, 2, 256, 224, 32},
                       {PARADIS_GEMM_BF16X3, 0, 2, 5, 3, 60}};
  unsigned seen = 0;
  for (const auto& s : T5) {
    const WgradPlan p = wgrad_plan(s[2], s[3], s[4], s[5], (int64_t)s[3] * s[5], (int64_t)s[4] * s[5], at(1, 0), at(2, 0), s[0], s[1],
                                   def, wgrad_env());
    seen |= 1u << (int)p.kind;
    printf("  scheme %d io16 %d B=%d Co=%d Ci=%d P=%d -> %s, %d slab%s, grid %d x %d, %zu B LDS, %s\n", s[0], s[1], s[2], s[3], s[4],
           s[5], KIND_NAME[(int)p.kind], p.S, p.S == 1 ? "" : "s", p.grid, p.block, p.lds, p.to_slabs ? "slabs" : "writes dW");
  }
  const WgradEnv env = wgrad_env();
  if (env.tall && env.square && seen != 0x7fu) {
    fprintf(stderr, "the test shapes reach kinds %#x, not all seven\n", seen);
    ++failures;
  }
  printf("gemm_plan_check: %lld cases, %lld mismatches (PARADIS_WGRAD_TALL=%d PARADIS_WGRAD_SQUARE=%d)\n", cases, failures, env.tall,
         env.square);
  return failures ? 1 : 0;
}
