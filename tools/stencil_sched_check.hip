// Host-only check of the depthwise stencil's schedule choice (runs without a GPU; nothing is launched, no pointer is
// dereferenced): the decision every entry point of csrc/stencil.hip took before the split into family units - the
// predicates below are that file's, copied - against dw_schedule and the per-direction functions of stencil_common.h.
// Family, one-pass decision, the generic kernels' whole_vec4 flag, grid size, chunks / per and the workspace size have
// to agree for every k, every grid, every alignment of every tensor, with and without an addend.  Build once per
// setting of the A/B switches that change host code, with the sanitizers on the host side:
//   for d in "" -DDWCONV_PLANE_CHUNK=2 -DDWCONV_PLANES=0 -DDWCONV_BWD_FUSED=0 -DDWCONV_TILES=0; do
//     hipcc --cuda-host-only -O1 -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined $d \
//         -I paradis_model_amd/csrc tools/stencil_sched_check.hip -o build/stencil_sched_check && build/stencil_sched_check
//   done
#include <stdio.h>
#include "stencil_common.h"

namespace before {   // ---- the single unit's predicates and the order its entry points tested them in --------------------

int whole_plane_vec4(const float* src, int H, int W, int k) {
  return k == 5 && W == TW && H <= TH && ((int64_t)H * W) % 4 == 0 && (reinterpret_cast<uintptr_t>(src) & 15) == 0;
}
bool staged_tiles(const void* a, const void* b, int H, int W, int k) {
  return DWCONV_TILES && k == 5 && H >= TH && W >= TW && (H > TH || W > TW) && W % 4 == 0 &&
         (int64_t)H * W * 4 < (1ll << 32) && (reinterpret_cast<uintptr_t>(a) & 15) == 0 &&
         (reinterpret_cast<uintptr_t>(b) & 15) == 0;
}
int wgrad_chunks(int B, int C, int tiles) {
  int items = B * tiles;
  int chunks = (2048 + C - 1) / C;
  return std::max(1, std::min(chunks, items));
}
int bwd_tiles_per(int B, int C, int tiles) {
  const int items = std::max(1, B * tiles);
  const int chunks = std::max(1, std::min((8192 + C - 1) / C, items));
  return (items + chunks - 1) / chunks;
}
int bwd_tiles_chunks(int B, int C, int tiles) {
  const int items = std::max(1, B * tiles), per = bwd_tiles_per(B, C, tiles);
  return (items + per - 1) / per;
}

}  // namespace before

// one launch: family (DwSched), workgroups, and what the kernel is told
struct Launch {
  int family = -1, whole_vec4 = 0, chunks = 0, per = 0;
  int64_t grid = 0;
  bool operator==(const Launch& o) const {
    return family == o.family && whole_vec4 == o.whole_vec4 && chunks == o.chunks && per == o.per && grid == o.grid;
  }
};
// a backward call: one pass (then `dgrad` is that launch) or the two halves
struct Bwd {
  bool one_pass = false;
  Launch dgrad, wgrad;
  bool operator==(const Bwd& o) const { return one_pass == o.one_pass && dgrad == o.dgrad && wgrad == o.wgrad; }
};
constexpr int PLANES = (int)DwSched::Planes, TILES = (int)DwSched::Tiles, GENERIC = (int)DwSched::Generic;

namespace before {

Launch fwd(const DwArgs& a) {
  Launch l;
  const int tiles = ((a.W + TW - 1) / TW) * ((a.H + TH - 1) / TH);
  const int64_t planes = (int64_t)a.B * a.C;
  if (DWCONV_PLANES && whole_plane_vec4(a.x, a.H, a.W, a.k)) {
    l.family = PLANES; l.grid = (planes + PLANE_CHUNK - 1) / PLANE_CHUNK;
  } else if (staged_tiles(a.x, a.y, a.H, a.W, a.k)) {
    l.family = TILES; l.grid = (planes + PLANE_CHUNK - 1) / PLANE_CHUNK * tiles;
  } else {
    l.family = GENERIC; l.grid = planes * tiles; l.whole_vec4 = whole_plane_vec4(a.x, a.H, a.W, a.k);
  }
  return l;
}

Launch dgrad(const DwArgs& a) {
  Launch l;
  if (a.B == 0) return l;
  const int tiles = ((a.W + TW - 1) / TW) * ((a.H + TH - 1) / TH);
  if (DWCONV_PLANES && whole_plane_vec4(a.gy, a.H, a.W, a.k) && (reinterpret_cast<uintptr_t>(a.gx) & 3) == 0 &&
      (reinterpret_cast<uintptr_t>(a.addend) & 3) == 0) {
    l.family = PLANES; l.grid = ((int64_t)a.B * a.C + PLANE_CHUNK - 1) / PLANE_CHUNK;
  } else if (staged_tiles(a.gy, a.gx, a.H, a.W, a.k) && staged_tiles(a.gy, a.addend, a.H, a.W, a.k)) {
    l.family = TILES; l.per = bwd_tiles_per(a.B, a.C, tiles); l.chunks = bwd_tiles_chunks(a.B, a.C, tiles);
    l.grid = (int64_t)a.C * l.chunks;
  } else {
    l.family = GENERIC; l.grid = (int64_t)a.B * a.C * tiles; l.whole_vec4 = whole_plane_vec4(a.gy, a.H, a.W, a.k);
  }
  return l;
}

Launch wgrad(const DwArgs& a) {
  Launch l;
  const int tiles = ((a.W + TW - 1) / TW) * ((a.H + TH - 1) / TH);
  const bool staged = a.B > 0 && staged_tiles(a.gy, a.x, a.H, a.W, a.k);
  l.chunks = a.B == 0 ? 1 : (staged ? bwd_tiles_chunks(a.B, a.C, tiles) : wgrad_chunks(a.B, a.C, tiles));
  l.grid = (int64_t)a.C * l.chunks;
  if (staged) {
    l.family = TILES; l.per = bwd_tiles_per(a.B, a.C, tiles);
  } else if (DWCONV_PLANES && whole_plane_vec4(a.x, a.H, a.W, a.k) && (reinterpret_cast<uintptr_t>(a.gy) & 3) == 0) {
    l.family = PLANES;
  } else {
    l.family = GENERIC; l.whole_vec4 = whole_plane_vec4(a.x, a.H, a.W, a.k);
  }
  return l;
}

Bwd bwd(const DwArgs& a) {
  Bwd r;
  const bool fused = DWCONV_BWD_FUSED && DWCONV_PLANES && a.B > 0 && whole_plane_vec4(a.gy, a.H, a.W, a.k) &&
                     whole_plane_vec4(a.x, a.H, a.W, a.k) && (reinterpret_cast<uintptr_t>(a.gx) & 3) == 0 &&
                     (reinterpret_cast<uintptr_t>(a.addend) & 3) == 0;
  if (a.B > 0 && staged_tiles(a.gy, a.x, a.H, a.W, a.k) && staged_tiles(a.gx, a.addend, a.H, a.W, a.k)) {
    const int tiles = ((a.W + TW - 1) / TW) * ((a.H + TH - 1) / TH);
    r.one_pass = true;
    r.dgrad.family = TILES; r.dgrad.per = bwd_tiles_per(a.B, a.C, tiles); r.dgrad.chunks = bwd_tiles_chunks(a.B, a.C, tiles);
    r.dgrad.grid = (int64_t)a.C * r.dgrad.chunks;
  } else if (!fused) {
    r.dgrad = dgrad(a); r.wgrad = wgrad(a);
  } else {
    r.one_pass = true;
    r.dgrad.family = PLANES; r.dgrad.chunks = wgrad_chunks(a.B, a.C, 1); r.dgrad.grid = (int64_t)a.C * r.dgrad.chunks;
  }
  return r;
}

int bwd16_ok(int H, int W, int k) {
  return (DWCONV_BWD_FUSED && DWCONV_PLANES && k == 5 && W == TW && H <= TH && ((int64_t)H * W) % 4 == 0) ? 1 : 0;
}
// the alignment paradis_dwconv_geo_bwd16 requires on top of bwd16_ok
bool bwd16_aligned(const DwArgs& a) {
  return ((reinterpret_cast<uintptr_t>(a.gy) | reinterpret_cast<uintptr_t>(a.x)) & 15) == 0 &&
         ((reinterpret_cast<uintptr_t>(a.gx) | reinterpret_cast<uintptr_t>(a.addend)) & 3) == 0;
}
size_t ws_bytes(int B, int C, int H, int W, int k) {
  const int tiles = ((W + TW - 1) / TW) * ((H + TH - 1) / TH);
  const int chunks = std::max(wgrad_chunks(B, C, tiles), bwd_tiles_chunks(B, C, tiles));
  return (size_t)C * chunks * (k * k + 1) * sizeof(float) + 256;
}

}  // namespace before

namespace after {   // ---- stencil.hip's entry points over stencil_common.h; dw_*_geom is what the launchers launch ----------

Launch launch_of(DwSched s, const DwGeom& g, int whole_vec4) {
  Launch l;
  l.family = (int)s; l.grid = g.grid; l.chunks = g.chunks; l.per = g.per;
  l.whole_vec4 = s == DwSched::Generic ? whole_vec4 : 0;
  return l;
}

Launch fwd(const DwArgs& a, bool y16) {
  const DwSched s = dw_fwd_schedule(a, y16);
  return launch_of(s, dw_fwd_geom(s, a), dw_whole_vec4(a.H, a.W, a.k, a.x));
}

Launch dgrad_half(DwSched s, const DwArgs& a) {
  if (a.B == 0) return Launch();
  return launch_of(s, dw_dgrad_geom(s, a), dw_whole_vec4(a.H, a.W, a.k, a.gy));
}

Launch wgrad_half(DwSched s, const DwArgs& a) {
  return launch_of(s, dw_wgrad_geom(s, a), dw_whole_vec4(a.H, a.W, a.k, a.x));
}

Bwd bwd(const DwArgs& a) {
  Bwd r;
  const DwSched sd = dw_dgrad_schedule(a), sw = dw_wgrad_schedule(a);
  if (dw_one_pass(sd, sw, a.B)) {
    r.one_pass = true;
    r.dgrad = wgrad_half(sd, a);       // the one-pass launchers take the weight gradient's chunks
  } else {
    r.dgrad = dgrad_half(sd, a); r.wgrad = wgrad_half(sw, a);
  }
  return r;
}

int bwd16_ok(int H, int W, int k) { return (DWCONV_BWD_FUSED && DWCONV_PLANES && dw_planes_shape(H, W, k)) ? 1 : 0; }
bool bwd16_aligned(const DwArgs& a) {
  return dw_dgrad_schedule(a) == DwSched::Planes && dw_wgrad_schedule(a) == DwSched::Planes;
}
size_t ws_bytes(int B, int C, int H, int W, int k) {
  return (size_t)C * dw_ws_chunks(B, C, dw_tiles(H, W)) * (k * k + 1) * sizeof(float) + 256;
}

}  // namespace after

static long long cases = 0, failures = 0;
static void expect(bool ok, const char* what, const DwArgs& a) {
  ++cases;
  if (ok) return;
  if (++failures <= 20)
    fprintf(stderr, "MISMATCH %s: B=%d C=%d H=%d W=%d k=%d gy=%p x=%p gx=%p addend=%p y=%p\n", what, a.B, a.C, a.H, a.W, a.k,
            (const void*)a.gy, (const void*)a.x, (const void*)a.gx, (const void*)a.addend, (const void*)a.y);
}

int main() {
  const int BC[][2] = {{0, 4}, {2, 6}, {3, 1030}, {8, 1024}};
  const int OFF[] = {0, 4, 8, 16};
  const uintptr_t base = (uintptr_t)1 << 40;      // never dereferenced
  auto at = [&](int tensor, int off) { return reinterpret_cast<float*>(base + ((uintptr_t)tensor << 32) + (uintptr_t)off); };
  for (int k = 1; k <= 11; k += 2)
    for (int hi = 2; hi <= 132; ++hi)
      for (int wi = 2; wi <= 266; wi += 2) {
        int H = hi, W = wi;
        if (hi > 130 || wi > 264) {               // the two reference grids beyond the sweep, once each
          if (hi == 131 && wi == 266) { H = 721; W = 1440; }
          else if (hi == 132 && wi == 266) { H = 181; W = 360; }
          else continue;
        }
        for (const auto& bc : BC) {
          DwArgs a{};
          a.B = bc[0]; a.C = bc[1]; a.H = H; a.W = W; a.k = k;
          expect(before::ws_bytes(a.B, a.C, H, W, k) == after::ws_bytes(a.B, a.C, H, W, k), "ws_bytes", a);
          expect(before::bwd16_ok(H, W, k) == after::bwd16_ok(H, W, k), "bwd16_ok", a);
          const int ws_chunks = dw_ws_chunks(a.B, a.C, dw_tiles(H, W));
          for (int ox : OFF)
            for (int oy : OFF) {                 // forward: x, y
              a.x = at(1, ox); a.y = at(2, oy);
              for (int y16 = 0; y16 < 2; ++y16) expect(before::fwd(a) == after::fwd(a, y16), "fwd", a);
            }
          a.y = nullptr;
          for (int og : OFF)
            for (int ox : OFF)
              for (int oo : OFF)
                for (int oa = -1; oa < 4; ++oa) {   // backward: gy, x, gx, addend (-1: none)
                  a.gy = at(3, og); a.x = at(1, ox); a.gx = at(4, oo); a.addend = oa < 0 ? nullptr : at(5, OFF[oa]);
                  if (ox == 0) expect(before::dgrad(a) == after::dgrad_half(dw_dgrad_schedule(a), a), "dgrad", a);
                  if (oo == 0 && oa < 0) expect(before::wgrad(a) == after::wgrad_half(dw_wgrad_schedule(a), a), "wgrad", a);
                  const Bwd b0 = before::bwd(a), b1 = after::bwd(a);
                  expect(b0 == b1, "bwd", a);
                  expect(std::max(b1.dgrad.chunks, b1.wgrad.chunks) <= ws_chunks, "workspace holds the chunks", a);
                  if (before::bwd16_ok(H, W, k)) expect(before::bwd16_aligned(a) == after::bwd16_aligned(a), "bwd16 alignment", a);
                }
        }
      }
  printf("stencil_sched_check: %lld cases, %lld mismatches (PLANE_CHUNK=%d PLANES=%d BWD_FUSED=%d TILES=%d)\n", cases,
         failures, DWCONV_PLANE_CHUNK, DWCONV_PLANES, DWCONV_BWD_FUSED, DWCONV_TILES);
  return failures ? 1 : 0;
}
