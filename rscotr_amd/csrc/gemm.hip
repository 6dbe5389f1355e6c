// fp32 GEMM on the CDNA4 matrix cores (v_mfma_f32_32x32x2_f32: f32 in, f32 accumulate, exact
// fp32 = an fmaf chain; gfx950 has no TF32/xf32) with fused epilogues.
//
// This is the substrate under every dense contraction of the co-training step: what the
// reference reaches as nn.Linear / F.linear / 1x1 and patchify Conv2d through mmcv, mmdet, mmcls
// and torch (QKV/proj/MLP of mmdet SwinTransformer — configs/multi/MTL_slvlcls_...potsdam.py:9-25;
// FFN 256->2048->256 and the MSDeformAttn projections of the shared encoder — :34-50; the DINO and
// Mask2Former decoder/branch Linears — models/multi/bbox_head/dino_head.py:40-47,
// models/multi/seg_head/mask2former_head.py:60-83; ChannelMapper 1x1 convs — :26-33), together with
// the two backward contractions autograd derives from each of them.
//
//   C[m,n] = epilogue( sum_k Aop[m,k] * Bop[n,k] )
//   Aop[m,k] = a_kmajor ? A[k*lda + m] : A[m*lda + k]     (same for B with ldb, over n)
// so that   y  = x W^T + b      is (A=x,  B=W,  a_kmajor=0, b_kmajor=0)   [F.linear]
//           dx = dy W           is (A=dy, B=W,  a_kmajor=0, b_kmajor=1)
//           dW = dy^T x         is (A=dy, B=x,  a_kmajor=1, b_kmajor=1)
// epilogue(v): v += bias[n]; if (pre) pre[m,n] = v; v = act(v) or v *= act'(aux[m,n]);
//              v += resid[m,n]; if (accumulate) v += C[m,n].
//
// Files: this one holds no kernel — the mode switches, the route planner (plan_gemm), validation and the C entry points of the
// planned products.  The kernels live one family per file behind the launch_* functions of gemm_plan.h; the kernel-shape notes
// are in front of the bodies (gemm_tiled_body.h, gemm_split_body.h).
#include "gemm_plan.h"
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <atomic>

using namespace rscotr;

constexpr int GEMM_PREC_DEFAULT = 3;
// 0: fp32 matrix pipe (v_mfma_f32_32x32x2_f32) everywhere; 3: the split product (three bf16 planes, six MFMAs: fp32-accurate —
// or, with the operands' value ranges, two fp16 planes and three MFMAs) where it pays, fp32 pipe elsewhere.
// RSCOTR_GEMM_PREC=fp32|bf16x6 sets the start value, rscotr_gemm_set_precision() changes it (tests, A/B runs).  (Modes 1 / 2,
// round 1's two-plane bf16 product at 4-6e-6, lost their A/B in rounds 2 and 3 and left the library in round 5.)
static std::atomic<int> g_gemm_prec{[] {
  const char* e = getenv("RSCOTR_GEMM_PREC");
  if (e && (!strcmp(e, "fp32") || !strcmp(e, "0"))) return 0;
  if (e && (!strcmp(e, "bf16x6") || !strcmp(e, "3"))) return 3;
  return GEMM_PREC_DEFAULT;
}()};

static std::atomic<int> g_h3_on{[] {
  const char* e = getenv("RSCOTR_GEMM_H3");
  return e ? atoi(e) : 1;
}()};

// k-slices through slabs, shared by the split-product planner and the workspace bound: aim at kSliceWgs workgroups, with at
// least kSliceMinK of the reduction per slice; weight gradients are sliced from K = kSliceFromK on
constexpr long kSliceWgs = 512, kSliceMinK = 256, kSliceFromK = 1024;

// Tile / slice choice of the bf16x6 kernel for one problem; bm == 0: not its domain (the fp32 pipe takes it).
struct Split6Cfg {
  int bm, splits, klen;
};

static Split6Cfg choose_split6(const GemmParams& p, int a_kmajor, int b_kmajor, int64_t ws_bytes) {
  Split6Cfg c{0, 1, p.K};
  constexpr long t128_min = 512;
  constexpr long t64_min = 256;  // (round 4: 256 measures -0.3 ms per round on mtl512 against 512 — Swin stage-2 / -4 products move to the split product, flop share 0.85 -> 0.90; 384: -0.2; 192 and 128 lose 0.7.  It also re-routes the 2500-row stage-4 products of the 800 x 800 det step: that parity run passes with its tensors outside the 1e-3 tier explained by the fp64 anchor)
  constexpr long dw_t128_min = 24;
  constexpr int k_min = 192;
  constexpr long mid_t64 = 96;  // (round 4: 96 takes the 512-row Swin stage-4 products with K >= 2304 (96 tiles, 6 k-slices): -0.25 ms per round against 128)
  constexpr int mid_k = 1024;
  // Measured on the step (profiles/r2_gemm_census.txt against profiles/history/r1_s7_gemm_census_fp32.txt): the split
  // product wins where the MFMA work dominates — the encoder FFN products (117 -> 85 us, 125 -> 100 us), their weight
  // gradients (124 -> 75 us), the 10880- / 2048-row products with K >= 256 (5-15 %) — and loses on small outputs (256 x 256
  // weight gradients: 22.6 -> 32.5 us: too few tiles to hide the staging), on K < 192 (conversion not amortised) and where
  // the epilogue's memory traffic bounds the launch anyway.
  if (!p.vecA || !p.vecB || p.K % 4 || p.K < k_min || p.M < 64 || p.N < 64) return c;
  // ragged shapes (M = 4 x 13 294 rows at 800 x 800, N = 96 / 288 columns of Swin stage 1, K = 53 176 of the 800 x 800 weight
  // gradients) take the EDGE instantiations (split_ragged): clamped loads, zeros past K, guarded stores; a k-major operand is
  // read four rows at a time, so its row count must be a multiple of 4 (which every interior shape satisfies anyway)
  if ((a_kmajor && p.M % 4) || (b_kmajor && p.N % 4)) return c;
  const long t64 = (long)((p.M + 63) / 64) * ((p.N + 63) / 64);
  const long t128 = (long)((p.M + 127) / 128) * ((p.N + 127) / 128);
  // (a 128-wide tile on a ragged edge wastes up to half a tile per row / column of tiles: only where that is < 1/8 of the work)
  const bool fit128 = (p.M % 128 == 0 || p.M >= 1024) && (p.N % 128 == 0 || p.N >= 1024);
  if (a_kmajor && b_kmajor) {  // weight gradients: small outputs, long reductions -> k-slices through slabs
    if (p.rowscale || p.K < kSliceFromK || p.M % 128 || p.N % 128 || t128 < dw_t128_min) return c;
    const int bm = 128;
    const long tiles = t128;
    if (tiles > 2048) return c;
    long sp = std::max<long>(1, std::min<long>((kSliceWgs + tiles - 1) / tiles, p.K / kSliceMinK));
    const int64_t per = ((int64_t)p.M * p.N + p.M) * 4;
    if (sp > 1) sp = std::min<long>(sp, ws_bytes / per);
    if (sp < 1) sp = 1;
    int klen = (int)((p.K + sp - 1) / sp);
    klen = (klen + X6_BK0 - 1) / X6_BK0 * X6_BK0;
    c.bm = bm; c.klen = klen; c.splits = (p.K + klen - 1) / klen;
    if (c.splits == 1) c.klen = p.K;
    return c;
  }
  if (p.kscale) return c;
  if (fit128 && t128 >= t128_min) c.bm = 128;
  else if (t64 >= t64_min && p.K <= 4096) c.bm = 64;
  else if (t64 >= mid_t64 && p.K >= mid_k) {
    // mid-size outputs with a long reduction (Swin stage 3: 2048 x 384 x 1536): too few 64 x 64 tiles for the chip, so the
    // reduction is cut into k-slices whose slabs the combine launch sums and runs the epilogue on
    long sp = std::min<long>((kSliceWgs + t64 - 1) / t64, p.K / kSliceMinK);
    const int64_t per = ((int64_t)p.M * p.N + p.M) * 4;
    sp = std::min<long>(sp, ws_bytes / per);
    if (sp >= 2) {
      int klen = (int)((p.K + sp - 1) / sp);
      const int kq = p.K % 32 == 0 ? 32 : 16;  // (k-slices of whole 32-k stages for the pipelined 64 x 64 kernel)
      klen = (klen + kq - 1) / kq * kq;
      c.bm = 64; c.klen = klen; c.splits = (p.K + klen - 1) / klen;
      if (c.splits == 1) c.klen = p.K;
    }
  }
  return c;
}

// The EDGE instantiations of the split product: the tile does not divide M or N, or the k-step of its loop does not divide K
// (X6_BK0 = 32 for the one-stage 128 x 128 loop, 16 for the 64 x 64 loops).  The one definition.  The two predictions used to
// test K % 16 for both tiles; never observable: split_route used it for 64-wide tiles only, and choose_split6 only to demand
// row counts % 4 of k-major operands, which M % 64 == N % 64 == 0 implies (profiles/README.md).
static bool split_ragged(const GemmParams& p, int bm) { return p.M % bm || p.N % bm || p.K % (bm == 128 ? X6_BK0 : 16); }

// Wavefront groups per workgroup for a launch of `wgs` workgroups with `nk` k-tiles each: short grids leave
// most CUs idle, so the k loop of each tile is spread over 2 or 4 groups.
static int choose_kgroups(long wgs, long nk) {
  constexpr long kg4_max = 256, kg2_max = 768;
  if (wgs <= kg4_max && nk >= 8) return 4;
  if (wgs <= kg2_max && nk >= 4) return 2;
  return 1;
}

// The low-latency kernel's domain: small outputs, short reductions, no per-sample scaling (those are Swin products).
static bool small_gemm_ok(const GemmParams& p, int a_kmajor, int b_kmajor, long nbatch) {
  constexpr long max_tiles = 512;
  constexpr int max_k = 512;
  if (p.K % 8 || p.K < 32 || p.rowscale || p.kscale) return false;
  if ((!a_kmajor && !p.vecA) || (!b_kmajor && !p.vecB)) return false;
  const long tiles = (long)((p.M + 31) / 32) * ((p.N + 31) / 32);
  // a handful of output tiles with a longer reduction (the classifier's fc: 2 x 45 x 768) ran as ONE workgroup of the tiled
  // kernel walking 48 dependent k-tiles (26 us); here 16 wavefronts split K
  if (p.K > max_k) return p.K <= 4096 && tiles * nbatch <= 8;
  return tiles * nbatch <= max_tiles;
}

// Wave-tile and split choice of the direct weight-gradient kernel; splits == 0: not its domain.
struct DwCfg {
  int TM, TN, tiles;
  long splits;
  int klen;
};

static DwCfg choose_dw_direct(int M, int N, int K) {
  // Measured on the step (profiles/README.md, trip 37): wins where the 64x64 tiling pads badly and the reduction is
  // very long (Swin stage 1: 288x96, 96x384, 384x96 over 32768 tokens: 104 / 80 / 77 us -> 67 / 68 / 69 us); loses on
  // the 256-wide and stage 2-3 gradients (one 24-load block in flight per wavefront is latency-bound below ~K = 16k).
  constexpr int max_tiles = 4, min_k = 16384;
  constexpr long target = 256;
  DwCfg c{0, 0, 0, 0, 0};
  if (K < min_k || M < 8 || N < 8) return c;
  // least padded of 96x96, 64x128, 128x64 wave tiles
  const int cand[3][2] = {{3, 3}, {2, 4}, {4, 2}};
  long best = -1;
  for (const auto& t : cand) {
    const long tm = (M + 32 * t[0] - 1) / (32 * t[0]), tn = (N + 32 * t[1] - 1) / (32 * t[1]);
    const long area = tm * 32 * t[0] * tn * 32 * t[1];
    if (best < 0 || area < best) { best = area; c.TM = t[0]; c.TN = t[1]; c.tiles = (int)(tm * tn); }
  }
  if (c.tiles > max_tiles || c.tiles < 3) return c;
  // ~`target` workgroups of 4 wavefronts (one per SIMD of a CU), >= 128 k per workgroup, <= 128 slabs
  long sp = std::min<long>({(target + c.tiles - 1) / c.tiles, (long)K / 128, 128L});
  if (sp < 2) return c;
  int klen = (int)((K + sp - 1) / sp);
  klen = (klen + 7) / 8 * 8;
  c.klen = klen;
  c.splits = (K + klen - 1) / klen;
  if (c.splits < 2) c.splits = 0;
  return c;
}

struct GemmCfg {
  int BM, BN;
  long splits;
};

// Tile / split choice.  The grid must cover 256 CUs a few times over (3 workgroups per CU are
// resident): prefer the largest tile that still gives >= 512 tiles, then smaller tiles, then split K
// (>= 16 k-tiles per split) through caller-provided slabs.
static GemmCfg choose_cfg(int M, int N, int K) {
  GemmCfg c;
  // Measured on MI355X over the step's shapes (a tile sweep of round 1, scripts/lab/gemm_lab.hip,
  // profiles/history/r1_gemm_tuning.md): 64x64 tiles (8 resident workgroups per CU) win on nearly every shape;
  // 128x64 wins on the wide, tall products of the encoder FFN (N >= 1024, >= 1360 tiles of 128x64).
  c.BM = 64; c.BN = 64;
  if (N <= 32) { c.BM = 128; c.BN = 32; }
  else if (N >= 1024 && M >= 4096 && M % 128 == 0) { c.BM = 128; c.BN = 64; }
  const long t = (long)((M + c.BM - 1) / c.BM) * ((N + c.BN - 1) / c.BN);
  // Split only long reductions on short grids: a 64x64 tile costs ~0.2 us per k-tile, so K < 1024
  // finishes in a few microseconds on however few CUs, cheaper than a second (combine) launch; longer
  // K is cut (>= 256 elements per slice) until the grid holds ~2 workgroups per CU (each then runs 2 k-groups:
  // 512 workgroups x 2 groups measured equal to 1024 x 1 with half the slab traffic).
  c.splits = 1;
  constexpr long split_target = 512;
  if (t < 512 && K >= 1024) {
    long sp = (split_target + t - 1) / t;
    sp = std::min<long>(sp, K / 256);
    c.splits = std::max<long>(1, std::min<long>(sp, 64));
  }
  return c;
}

// The one walk of the cascade: small -> direct dW -> split product -> fp32 tiles.  p carries the shape, vecA / vecB and the
// rowscale / kscale pointers (null or not); ws_bytes = bytes of workspace the call may use (0: none); ranges / planes: both
// operand ranges / the pre-split planes of B are at hand.
static GemmPlan plan_gemm(const GemmParams& p, int a_kmajor, int b_kmajor, int64_t ws_bytes, bool ranges, bool planes) {
  const int M = p.M, N = p.N, K = p.K;
  GemmPlan pl{};
  pl.a_kmajor = a_kmajor; pl.b_kmajor = b_kmajor;
  pl.splits = 1; pl.klen = K; pl.kgroups = 1; pl.nbatch = 1;
  const int64_t per = ((int64_t)M * N + M) * 4;  // one slab + its row-sum partials
  auto grid = [&] {  // split-K: every XCD owns a run of tiles with all their slices (gemm_f32_body)
    pl.nwg = pl.splits > 1 ? (unsigned)(8 * ((pl.tiles >> 3) + ((pl.tiles & 7) ? 1 : 0)) * pl.splits) : (unsigned)pl.tiles;
  };
  if (small_gemm_ok(p, a_kmajor, b_kmajor, 1)) {
    pl.route = ROUTE_SMALL; pl.bm = pl.bn = 32;
    pl.nwg = (unsigned)(((M + 31) / 32) * ((N + 31) / 32));
    pl.nw = K / 8 > 32 ? 16 : K / 8 > 16 ? 8 : 4;  // <= 4 octets of k (one pass) per wavefront where 16 wavefronts allow it
    return pl;
  }
  if (a_kmajor && b_kmajor && !p.rowscale) {
    const DwCfg d = choose_dw_direct(M, N, K);
    if (d.splits >= 2 && ws_bytes >= d.splits * per) {
      pl.route = ROUTE_DW_DIRECT; pl.tm = d.TM; pl.tn = d.TN;
      pl.klen = d.klen; pl.splits = (int)d.splits; pl.tiles = d.tiles;
      pl.nwg = (unsigned)(d.tiles * d.splits);
      return pl;
    }
  }
  if (g_gemm_prec.load(std::memory_order_relaxed) == 3) {
    const Split6Cfg sc = choose_split6(p, a_kmajor, b_kmajor, ws_bytes);
    if (sc.bm) {
      pl.route = ROUTE_SPLIT; pl.bm = pl.bn = sc.bm;
      pl.splits = sc.splits; pl.klen = sc.klen;
      pl.tiles = ((M + sc.bm - 1) / sc.bm) * ((N + sc.bm - 1) / sc.bm);
      pl.edge = split_ragged(p, sc.bm);
      // the pipelined loop on 64 x 64 tiles measured -0.45 ms / round; it stages 32 k per step
      pl.pipe = sc.bm == 128 ? 0 : (sc.klen % 32 == 0 && (pl.edge || K % 32 == 0)) ? 2 : 1;
      pl.h3 = ranges && g_h3_on.load(std::memory_order_relaxed);
      // B from its pre-split planes (rscotr_gemm_f32_rb; row-major by construction): the interior pipelined 64 x 64 fp16 kernel only
      pl.b_from_planes = pl.h3 && planes && !a_kmajor && !pl.edge && sc.bm == 64 && pl.pipe == 2;
      if (pl.b_from_planes) pl.b_kmajor = 0;
      grid();
      return pl;
    }
  }
  const GemmCfg cfg = choose_cfg(M, N, K);
  pl.route = ROUTE_TILED; pl.bm = cfg.BM; pl.bn = cfg.BN;
  pl.tiles = (int)((long)((M + cfg.BM - 1) / cfg.BM) * ((N + cfg.BN - 1) / cfg.BN));
  const long splits = std::max<long>(1, std::min<long>(cfg.splits, ws_bytes / per));
  if (splits > 1) {
    pl.klen = (int)((K + splits - 1) / splits);
    pl.klen = (pl.klen + GEMM_BK - 1) / GEMM_BK * GEMM_BK;
    pl.splits = (K + pl.klen - 1) / pl.klen;
  }
  grid();
  if (cfg.BM != 128 || cfg.BN != 64) pl.kgroups = choose_kgroups((long)pl.nwg, (pl.klen + GEMM_BK - 1) / GEMM_BK);
  return pl;
}

// Name of a launch for the launch-site profiler: the kernel, or with RSCOTR_PROF_SHAPES the shape (a per-shape census instead of
// a per-kernel one; bench.py and scripts/gemm_shapes.py parse these strings).
static void plan_name(const GemmParams& p, const GemmPlan& pl, char (&name)[112]) {
  static const bool shapes = getenv("RSCOTR_PROF_SHAPES") != nullptr;
  const char* tf[2] = {"false", "true"};
  const char *ak = tf[pl.a_kmajor != 0], *bk = tf[pl.b_kmajor != 0], *fam = pl.h3 ? "h3" : "bf16x6";
  const int n = (int)sizeof(name), r = pl.route;
  if (shapes) {  // "M= N= K= <layouts> [<family>-<tile>] splits=<k-slices: 0 small, negative direct dW>"
    char mid[40];
    if (r == ROUTE_SPLIT) snprintf(mid, sizeof(mid), "%d%d %s-%d", pl.a_kmajor, pl.b_kmajor, fam, pl.bm);
    else if (r == ROUTE_WPLANES) snprintf(mid, sizeof(mid), "0p wplanes-%d", pl.bn);
    else snprintf(mid, sizeof(mid), "%d%d", pl.a_kmajor, pl.b_kmajor);
    snprintf(name, n, "M=%d N=%d K=%d %s splits=%d", p.M, p.N, p.K, mid, r == ROUTE_SMALL ? 0 : r == ROUTE_DW_DIRECT ? -pl.splits : pl.splits);
  } else if (r == ROUTE_SMALL) snprintf(name, n, "rscotr::gemm_small_kernel<%s, %s, *>", ak, bk);
  else if (r == ROUTE_DW_DIRECT) snprintf(name, n, "rscotr::gemm_dw_direct_kernel<%d, %d>", pl.tm, pl.tn);
  else if (r == ROUTE_SPLIT) snprintf(name, n, "rscotr::gemm_%s_kernel<%d, %d, %s, %s, *>", fam, pl.bm, pl.bm, ak, bk);
  else if (r == ROUTE_WPLANES) snprintf(name, n, "rscotr::gemm_wplanes_kernel<%d>", pl.bn);
  else snprintf(name, n, "rscotr::gemm_f32_kernel<%d, %d, %d, %d, %s, %s, *>", pl.bm, pl.bn, pl.bn == 32 ? 4 : 2, pl.bn == 32 ? 1 : 2, ak, bk);
}

// Deferred combine (rscotr_gemm_f32_dw_slabs): the split-K launch stops after writing its slabs and reports the split
// count; rscotr_splitk_flush later combines every pending problem of a backward pass in ONE launch.
static thread_local int tl_defer = 0;
static thread_local int tl_last_splits = 1;

extern "C" int rscotr_gemm_set_precision(int prec) {
  if (prec != 0 && prec != 3) return fail(RSCOTR_E_ARG, "rscotr_gemm_set_precision: 0 (fp32 matrix pipe everywhere) or 3 (the fp32-accurate split product where it pays)");
  g_gemm_prec.store(prec);
  return RSCOTR_OK;
}

extern "C" int rscotr_gemm_get_precision(void) { return g_gemm_prec.load(); }

// Workspace the split-K path wants for this problem (bytes; 0 = never splits): slabs + row-sum partials.  A bound of its own that
// feeds back into the plan (ws_bytes / per), so its values stay: 128-wide tiles from 16 of them (choose_split6: dw_t128_min = 24),
// mid-size slices from 128 tiles of 64 (there: mid_t64 = 96).  Reconciling them would change launches.
extern "C" int64_t rscotr_gemm_f32_workspace(int M, int N, int K) {
  if (M <= 0 || N <= 0 || K <= 0) return 0;
  const GemmCfg c = choose_cfg(M, N, K);
  const DwCfg d = choose_dw_direct(M, N, K);
  int64_t sp = std::max<int64_t>(c.splits > 1 ? c.splits : 0, d.splits);
  if (g_gemm_prec.load(std::memory_order_relaxed) == 3 && M >= 64 && N >= 64 && K % 4 == 0 && K >= kSliceFromK) {
    const long t128 = (M % 128 == 0 && N % 128 == 0) ? (long)(M / 128) * (N / 128) : 0;
    const long tiles = t128 >= 16 ? t128 : (long)((M + 63) / 64) * ((N + 63) / 64);
    sp = std::max<int64_t>(sp, std::max<long>(1, std::min<long>((kSliceWgs + tiles - 1) / tiles, K / kSliceMinK)));  // as a weight gradient
    const long t64 = (long)((M + 63) / 64) * ((N + 63) / 64);
    if (t64 >= 128 && t64 < 512) sp = std::max<int64_t>(sp, std::min<long>((kSliceWgs + t64 - 1) / t64, K / kSliceMinK));  // mid-size k-slices
  }
  return sp * ((int64_t)M * N + M) * 4;
}

extern "C" int rscotr_gemm_set_h3(int on) { return g_h3_on.exchange(on ? 1 : 0); }

// The plan of rscotr_gemm_f32 for a product described without pointers (16-byte aligned operands assumed)
static GemmPlan plan_of_shape(int M, int N, int K, int lda, int ldb, int a_kmajor, int b_kmajor, int has_rowscale, int has_kscale,
                              int64_t workspace_bytes) {
  static float dummy;
  GemmParams p{};
  p.M = M; p.N = N; p.K = K; p.lda = lda; p.ldb = ldb; p.ldc = N;
  p.vecA = lda % 4 == 0; p.vecB = ldb % 4 == 0;
  p.rowscale = has_rowscale ? &dummy : nullptr; p.kscale = has_kscale ? &dummy : nullptr;
  return plan_gemm(p, a_kmajor, b_kmajor, workspace_bytes, true, true);
}

// 1 if rscotr_gemm_f32 with these arguments (16-byte aligned operands, precision mode 3) runs on the interior 128 x 128
// split-product tiles with one k-slice: the products that may carry the ReLU gate as bits (ACT_RELU_BITS / ACT_RELU_GRAD_BITS)
extern "C" int rscotr_gemm_relu_bits_ok(int M, int N, int K, int lda, int ldb, int a_kmajor, int b_kmajor) {
  if (M <= 0 || N <= 0 || K <= 0 || a_kmajor || g_gemm_prec.load(std::memory_order_relaxed) != 3) return 0;
  const GemmPlan pl = plan_of_shape(M, N, K, lda, ldb, a_kmajor, b_kmajor, 0, 0, 0);
  return pl.route == ROUTE_SPLIT && pl.bm == 128 && !pl.edge && pl.splits == 1;
}

// rscotr_gemm_f32_r with the B operand ALSO given as pre-split fp16 planes (rscotr_gemm_split_weights_h3: the planes of B for a
// row-major B, of its transpose for a k-major one; b_rpad = their padded row count).  Taken where rscotr_gemm_f32_split_route
// answers 2 (the interior pipelined 64 x 64 fp16 kernel); everywhere else the call is rscotr_gemm_f32_r on B itself, which lands here too.
extern "C" int rscotr_gemm_f32_rb(const float* A, const float* B, float* C, int M, int N, int K, int lda, int ldb, int ldc, int a_kmajor, int b_kmajor,
                                  const float* bias, int act, const float* aux, float* pre, const float* resid, int accumulate, float* rowsum, int rowsum_accumulate,
                                  const float* rowscale, int rows_per_scale, const float* kscale, int krows_per_scale, float* out2, float* workspace,
                                  int64_t workspace_bytes, const uint32_t* amax_a, const uint32_t* amax_b, uint32_t* amax_out, const void* b_planes, int b_rpad,
                                  void* stream) {
  if (b_planes && (b_rpad < N || b_rpad % 64 || ((uintptr_t)b_planes & 15)))
    return fail(RSCOTR_E_ARG, "rscotr_gemm_f32_rb: the plane set has %d rows for N = %d (a multiple of 64 >= N, 16-byte aligned)", b_rpad, N);
  if (M < 0 || N < 0 || K < 0) return fail(RSCOTR_E_SHAPE, "rscotr_gemm_f32: negative dimension");
  if ((rowscale && rows_per_scale <= 0) || (kscale && (krows_per_scale <= 0 || !a_kmajor)))
    return fail(RSCOTR_E_ARG, "rscotr_gemm_f32: rowscale needs rows_per_scale > 0; kscale needs a k-major A and krows_per_scale > 0");
  if (M == 0 || N == 0) return RSCOTR_OK;
  if (!A || !B || !C) return fail(RSCOTR_E_ARG, "rscotr_gemm_f32: null pointer");
  if (act < ACT_NONE || act > ACT_RELU_GRAD_BITS) return fail(RSCOTR_E_ARG, "rscotr_gemm_f32: unknown act %d", act);
  if ((act == ACT_RELU_GRAD || act == ACT_GELU_GRAD || act == ACT_RELU_GRAD_BITS) && !aux)
    return fail(RSCOTR_E_ARG, "rscotr_gemm_f32: act %d needs aux", act);
  const bool relu_bits = act == ACT_RELU_BITS || act == ACT_RELU_GRAD_BITS;
  if (relu_bits) {
    // the one-bit ReLU gate lives in the interior 128 x 128 split-product tiles only (callers ask rscotr_gemm_relu_bits_ok first)
    if (act == ACT_RELU_BITS ? (!pre || ((uintptr_t)pre & 7)) : ((uintptr_t)aux & 7))
      return fail(RSCOTR_E_ARG, "rscotr_gemm_f32: act %d moves the gate bits through %s (8-byte aligned, M * N / 8 bytes)", act,
                  act == ACT_RELU_BITS ? "pre" : "aux");
    if ((act == ACT_RELU_GRAD_BITS && pre) || resid || accumulate || rowscale || out2 || rowsum || kscale)
      return fail(RSCOTR_E_ARG, "rscotr_gemm_f32: act %d takes bias only (no pre / resid / accumulate / rowscale / out2 / rowsum)", act);
    if (!rscotr_gemm_relu_bits_ok(M, N, K, lda, ldb, a_kmajor, b_kmajor))
      return fail(RSCOTR_E_SHAPE, "rscotr_gemm_f32: act %d on a product that does not take the interior 128 x 128 split-product tiles "
                  "(M = %d N = %d K = %d): rscotr_gemm_relu_bits_ok", act, M, N, K);
  }
  if (lda < (a_kmajor ? M : K) || ldb < (b_kmajor ? N : K) || ldc < N)
    return fail(RSCOTR_E_SHAPE, "rscotr_gemm_f32: leading dimension too small");
  if (rowsum && !a_kmajor) return fail(RSCOTR_E_ARG, "rscotr_gemm_f32: rowsum needs a k-major A");
  GemmParams p;
  p.A = A; p.B = B; p.C = C; p.bias = bias; p.aux = aux; p.pre = pre; p.resid = resid; p.C2 = out2;
  p.M = M; p.N = N; p.K = K; p.lda = lda; p.ldb = ldb; p.ldc = ldc;
  p.act = act; p.accumulate = accumulate;
  p.vecA = aligned16(A) && (lda % 4 == 0);
  p.vecB = aligned16(B) && (ldb % 4 == 0);
  p.vecC = (ldc % 4 == 0) && aligned16(C) && aligned16(bias) && aligned16(aux) && aligned16(pre) && aligned16(resid) && aligned16(out2);
  p.rowsum = rowsum; p.rowsum_acc = rowsum_accumulate;
  p.nb1 = 0; p.nb2 = 1;
  p.rowscale = rowscale; p.rows_per = rows_per_scale; p.kscale = kscale; p.krows_per = krows_per_scale;
  p.amax_out = amax_out;
  hipStream_t s = (hipStream_t)stream;

  const GemmPlan pl = plan_gemm(p, a_kmajor, b_kmajor, workspace ? workspace_bytes : 0, amax_a && amax_b, b_planes != nullptr);
  p.ksplit_len = pl.klen; p.splits = pl.splits; p.tiles = pl.tiles;
  p.slabs = pl.splits > 1 ? workspace : nullptr;
  p.rs_slabs = pl.splits > 1 ? workspace + pl.splits * (int64_t)M * N : nullptr;
  if (pl.route == ROUTE_SPLIT) {
    p.amax_a = amax_a; p.amax_b = amax_b;
    if (pl.b_from_planes) {
      p.B = reinterpret_cast<const float*>(b_planes);
      p.ldb = b_rpad;
    }
  }
  static_assert(ROUTE_SMALL == 0 && ROUTE_DW_DIRECT == 1 && ROUTE_SPLIT == 2 && ROUTE_TILED == 3, "order of what[]");
  static const char* const what[4][2] = {{"rscotr_gemm_f32 (small)", ""}, {"rscotr_gemm_f32 (dw direct)", "rscotr_gemm_f32 (dw direct reduce)"},
                                         {"rscotr_gemm_f32 (bf16x6)", "rscotr_gemm_f32 (bf16x6, split-K reduce)"}, {"rscotr_gemm_f32", "rscotr_gemm_f32 (split-K reduce)"}};
  char name[112];
  plan_name(p, pl, name);
  ProfScope prof(PROF_GEMM, 2.0 * M * N * K, s, "%s", name);
  if (pl.route == ROUTE_SMALL) launch_small(p, pl, s);
  else if (pl.route == ROUTE_DW_DIRECT) launch_dw_direct(p, pl, s);
  else if (pl.route == ROUTE_TILED) launch_tiled(p, pl, s);
  else if (pl.h3) launch_h3(p, pl, s);  // the fp16 split product: same tiles, same loops
  else launch_bf16x6(p, pl, s);
  if (int e = check_launch(what[pl.route][0])) return e;
  if (pl.splits > 1) {
    if (tl_defer) { tl_last_splits = pl.splits; return RSCOTR_OK; }
    splitk_reduce_launch(p, workspace, s);
    return check_launch(what[pl.route][1]);
  }
  return RSCOTR_OK;
}

extern "C" int rscotr_gemm_f32(const float* A, const float* B, float* C, int M, int N, int K, int lda, int ldb, int ldc, int a_kmajor, int b_kmajor, const float* bias,
                               int act, const float* aux, float* pre, const float* resid, int accumulate, float* rowsum, int rowsum_accumulate, const float* rowscale,
                               int rows_per_scale, const float* kscale, int krows_per_scale, float* out2, float* workspace, int64_t workspace_bytes, void* stream) {
  return rscotr_gemm_f32_rb(A, B, C, M, N, K, lda, ldb, ldc, a_kmajor, b_kmajor, bias, act, aux, pre, resid, accumulate, rowsum, rowsum_accumulate,
                            rowscale, rows_per_scale, kscale, krows_per_scale, out2, workspace, workspace_bytes, nullptr, nullptr, nullptr, nullptr, 0, stream);
}

extern "C" int rscotr_gemm_f32_r(const float* A, const float* B, float* C, int M, int N, int K, int lda, int ldb, int ldc, int a_kmajor, int b_kmajor,
                                 const float* bias, int act, const float* aux, float* pre, const float* resid, int accumulate, float* rowsum, int rowsum_accumulate,
                                 const float* rowscale, int rows_per_scale, const float* kscale, int krows_per_scale, float* out2, float* workspace,
                                 int64_t workspace_bytes, const uint32_t* amax_a, const uint32_t* amax_b, uint32_t* amax_out, void* stream) {
  return rscotr_gemm_f32_rb(A, B, C, M, N, K, lda, ldb, ldc, a_kmajor, b_kmajor, bias, act, aux, pre, resid, accumulate, rowsum, rowsum_accumulate,
                            rowscale, rows_per_scale, kscale, krows_per_scale, out2, workspace, workspace_bytes, amax_a, amax_b, amax_out, nullptr, 0, stream);
}

// dW = A^T B into slabs only (both operands k-major, result to be ACCUMULATED into C / rowsum later): the launch of
// rscotr_gemm_f32(a_kmajor = b_kmajor = 1, accumulate = 1, rowsum_accumulate = 1) without its combine.  *splits_out = the
// number of slabs written ([splits][M][N] floats at slab_region, then [splits][M] row-sum partials); 1 = the problem
// was not split and C / rowsum already hold the final result.
extern "C" int rscotr_gemm_f32_dw_slabs_r(const float* A, const float* B, float* C, int M, int N, int K, int lda, int ldb, int ldc, float* rowsum, const float* kscale,
                                          int krows_per_scale, float* slab_region, int64_t slab_bytes, int32_t* splits_out, const uint32_t* amax_a,
                                          const uint32_t* amax_b, void* stream) {
  if (!splits_out) return fail(RSCOTR_E_ARG, "rscotr_gemm_f32_dw_slabs: splits_out required");
  tl_defer = 1;
  tl_last_splits = 1;
  const int e = rscotr_gemm_f32_rb(A, B, C, M, N, K, lda, ldb, ldc, 1, 1, nullptr, ACT_NONE, nullptr, nullptr, nullptr, 1, rowsum,
                                   1, nullptr, 0, kscale, krows_per_scale, nullptr, slab_region, slab_bytes, amax_a, amax_b, nullptr,
                                   nullptr, 0, stream);
  tl_defer = 0;
  *splits_out = tl_last_splits;
  return e;
}

extern "C" int rscotr_gemm_f32_dw_slabs(const float* A, const float* B, float* C, int M, int N, int K, int lda, int ldb, int ldc, float* rowsum, const float* kscale,
                                        int krows_per_scale, float* slab_region, int64_t slab_bytes, int32_t* splits_out, void* stream) {
  return rscotr_gemm_f32_dw_slabs_r(A, B, C, M, N, K, lda, ldb, ldc, rowsum, kscale, krows_per_scale, slab_region, slab_bytes,
                                    splits_out, nullptr, nullptr, stream);
}

// 1 if rscotr_gemm_f32 with these arguments (16-byte aligned operands assumed) runs on the split-product kernels, i.e. as the
// fp16 split product when the value ranges of both operands are supplied (rscotr_gemm_f32_r): callers ask before they
// go looking for ranges.
extern "C" int rscotr_gemm_f32_split_route(int M, int N, int K, int lda, int ldb, int a_kmajor, int b_kmajor, int act, int has_pre, int has_rowscale, int has_kscale,
                                           int64_t workspace_bytes) {
  if (M <= 0 || N <= 0 || K <= 0 || g_gemm_prec.load(std::memory_order_relaxed) != 3 || !g_h3_on.load(std::memory_order_relaxed)) return 0;
  const GemmPlan pl = plan_of_shape(M, N, K, lda, ldb, a_kmajor, b_kmajor, has_rowscale, has_kscale, workspace_bytes);
  // (act and has_pre: no route depends on them)  2: the interior pipelined 64 x 64 kernel, which can take its B operand from pre-split planes (rscotr_gemm_f32_rb)
  return pl.route == ROUTE_SPLIT ? (pl.b_from_planes ? 2 : 1) : 0;
}

// Tile width and k-slices of the pre-split product: one 128 x 256 workgroup is resident per CU (86 KB of LDS), two 128 x 128
// ones; the grid should be a whole number of such rounds over the 256 CUs (340 workgroups take as long as 512).
static void wplanes_cfg(int M, int N, int K, int* bn_out, int* splits_out) {
  const long tm = (M + 127) / 128;
  const long smax = std::max<long>(1, std::min<long>(8, K / 256));
  double best = -1.0;
  int bbn = 128, bsp = 1;
  for (int bn = 256; bn >= 128; bn -= 128) {
    if (bn == 256 && N <= 128) continue;
    const long t = tm * ((N + bn - 1) / bn), cap = bn == 256 ? 256 : 512;
    for (long sp = 1; sp <= smax; ++sp) {
      const long wgs = t * sp, rounds = (wgs + cap - 1) / cap;
      // time model: rounds x (k-steps per slice + prologue / epilogue worth ~4 steps) x tile area, plus the slab pass
      const double steps = (double)K / 16 / sp + 4.0;
      // (a round of 512 half-width workgroups covers the area of a round of 256 full-width ones, ~1.2x slower: lab)
      double cost = rounds * steps * (bn == 256 ? 1.0 : 1.22);
      if (sp > 1) cost += 2.0 * sp * M * N * 4.0 * 1.9e-7;  // slabs written and read at ~4 TB/s, in k-steps of 1.3 us
      const double score = 1.0 / cost;
      if (score > best) { best = score; bbn = bn; bsp = (int)sp; }
    }
  }
  *bn_out = bbn; *splits_out = bsp;
}

// Where the weight-plane kernel above wins: long reductions over many rows (the encoder's FFN2 / its dX).  (Round 4's tiled
// split-product kernels with their B operand from planes gained 15-28 % per dispatch and lost the round to the per-iteration
// re-split of every weight — profiles/r4_planes_b_tiled.txt — and left the library in round 5.)
static bool wplanes_classic(int M, int K) {
  constexpr int min_m = 4096, min_k = 1024;
  return M >= min_m && K >= min_k;
}

/* 1: rscotr_gemm_f32_wplanes is worth calling for (M, N, K); 0: the caller multiplies with the fp32 weight (rscotr_gemm_f32) */
extern "C" int rscotr_gemm_f32_wplanes_ok(int M, int N, int K, int act_is_gelu) {
  if (M <= 0 || N <= 0 || K < 16 || K % 16) return 0;
  (void)act_is_gelu;
  return wplanes_classic(M, K) && N >= 64;
}

extern "C" int64_t rscotr_gemm_f32_wplanes_workspace(int M, int N, int K) {
  int bn, splits;
  wplanes_cfg(M, N, K, &bn, &splits);
  return splits > 1 ? (int64_t)splits * M * N * 4 : 0;
}

// C = epilogue(A x Bplanes): A (M, K) fp32 row-major (lda), planes = the pre-split B of rscotr_gemm_split_weights (N rows,
// npad >= N rounded up to 256, reduction K, K % 16 == 0); epilogue arguments as rscotr_gemm_f32.
extern "C" int rscotr_gemm_f32_wplanes(const float* A, const void* planes, int npad, float* C, int M, int N, int K, int lda, int ldc, const float* bias, int act,
                                       const float* aux, float* pre, const float* resid, int accumulate, const float* rowscale, int rows_per_scale, float* out2,
                                       float* workspace, int64_t workspace_bytes, void* stream) {
  if (M < 0 || N < 0 || K < 0) return fail(RSCOTR_E_SHAPE, "rscotr_gemm_f32_wplanes: negative dimension");
  if (M == 0 || N == 0) return RSCOTR_OK;
  if (!A || !planes || !C) return fail(RSCOTR_E_ARG, "rscotr_gemm_f32_wplanes: null pointer");
  if (K % 16 || K < 16 || npad % 256 || npad < N || lda < K || ldc < N || lda % 4 || !aligned16(A) || !aligned16(planes))
    return fail(RSCOTR_E_SHAPE, "rscotr_gemm_f32_wplanes: K %% 16, npad %% 256, 16-byte aligned A rows required (M=%d N=%d K=%d npad=%d lda=%d)",
                M, N, K, npad, lda);
  if (act < ACT_NONE || act > ACT_GELU_GRAD) return fail(RSCOTR_E_ARG, "rscotr_gemm_f32_wplanes: unknown act %d", act);
  if ((act == ACT_RELU_GRAD || act == ACT_GELU_GRAD) && !aux) return fail(RSCOTR_E_ARG, "rscotr_gemm_f32_wplanes: act %d needs aux", act);
  if (rowscale && rows_per_scale <= 0) return fail(RSCOTR_E_ARG, "rscotr_gemm_f32_wplanes: rowscale needs rows_per_scale > 0");
  GemmParams p;
  p.A = A; p.B = nullptr; p.C = C; p.bias = bias; p.aux = aux; p.pre = pre; p.resid = resid; p.C2 = out2;
  p.M = M; p.N = N; p.K = K; p.lda = lda; p.ldb = K; p.ldc = ldc;
  p.act = act; p.accumulate = accumulate;
  p.vecA = 1; p.vecB = 1;
  p.vecC = (ldc % 4 == 0) && aligned16(C) && aligned16(bias) && aligned16(aux) && aligned16(pre) && aligned16(resid) && aligned16(out2);
  p.rowsum = nullptr; p.rowsum_acc = 0; p.rs_slabs = nullptr;
  p.nb1 = 0; p.nb2 = 1;
  p.rowscale = rowscale; p.rows_per = rows_per_scale; p.kscale = nullptr; p.krows_per = 0;
  hipStream_t s = (hipStream_t)stream;
  int bn, splits;
  wplanes_cfg(M, N, K, &bn, &splits);
  if (splits > 1 && (!workspace || workspace_bytes < (int64_t)splits * M * N * 4))
    splits = (int)std::max<int64_t>(1, workspace ? workspace_bytes / ((int64_t)M * N * 4) : 1);
  p.tiles = (int)((long)((M + 127) / 128) * ((N + bn - 1) / bn));
  p.splits = splits; p.ksplit_len = K;
  p.slabs = splits > 1 ? workspace : nullptr;
  GemmPlan pl{};
  pl.route = ROUTE_WPLANES; pl.bm = 128; pl.bn = bn; pl.splits = splits; pl.klen = K; pl.tiles = p.tiles;
  pl.nwg = (unsigned)p.tiles * (unsigned)splits;
  char name[112];
  plan_name(p, pl, name);
  ProfScope prof(PROF_GEMM, 2.0 * M * N * K, s, "%s", name);
  launch_wplanes(p, pl, reinterpret_cast<const unsigned short*>(planes), npad, s);
  if (int e = check_launch("rscotr_gemm_f32_wplanes")) return e;
  if (splits > 1) {
    splitk_reduce_launch(p, workspace, s);
    return check_launch("rscotr_gemm_f32_wplanes (split-K reduce)");
  }
  return RSCOTR_OK;
}

// Batched form: nb0 * nb1 independent problems of one shape, problem (b0, b1) at element offsets
// b0*s?0 + b1*s?1 of A, B, C (e.g. b0 = image, b1 = head: the per-head slices of (B, L, heads*32) tensors are
// addressed in place, no permute copies).  No bias / activation; accumulate adds into C.
// ksplits > 1 (row-major A = a_kmajor 0, k-major B = b_kmajor 1 only; K % ksplits == 0): the reduction is cut
// into ksplits slices, slice s of every problem writes slab s = workspace + s * c_elems (laid out like C,
// c_elems = elements of the whole C tensor), and the slabs are summed into C by a second kernel — for the
// attention products with few output tiles and thousands of keys (P v and dS k of the seg decoder's
// cross-attention: 100 queries x 4096 keys per head).
extern "C" int rscotr_gemm_f32_batched(const float* A, const float* B, float* C, int M, int N, int K, int lda, int ldb, int ldc, int a_kmajor, int b_kmajor, int nb0,
                                       int nb1, int64_t sA0, int64_t sA1, int64_t sB0, int64_t sB1, int64_t sC0, int64_t sC1, int accumulate, int ksplits,
                                       float* workspace, int64_t c_elems, void* stream) {
  if (M < 0 || N < 0 || K < 0 || nb0 < 0 || nb1 < 0) return fail(RSCOTR_E_SHAPE, "rscotr_gemm_f32_batched: negative dimension");
  if (M == 0 || N == 0 || nb0 == 0 || nb1 == 0) return RSCOTR_OK;
  if (!A || !B || !C) return fail(RSCOTR_E_ARG, "rscotr_gemm_f32_batched: null pointer");
  if (ksplits < 1) ksplits = 1;
  if ((long)nb0 * nb1 * ksplits > 65535) return fail(RSCOTR_E_SHAPE, "rscotr_gemm_f32_batched: more than 65535 problems");
  if (lda < (a_kmajor ? M : K) || ldb < (b_kmajor ? N : K) || ldc < N)
    return fail(RSCOTR_E_SHAPE, "rscotr_gemm_f32_batched: leading dimension too small");
  if (ksplits > 1 && (a_kmajor || !b_kmajor || K % ksplits || accumulate || !workspace || c_elems % 4 || !aligned16(C) ||
                      !aligned16(workspace)))
    return fail(RSCOTR_E_ARG, "rscotr_gemm_f32_batched: ksplits needs row-major A, k-major B, K %% ksplits == 0, a workspace");
  GemmParams p;
  p.A = A; p.B = B; p.C = ksplits > 1 ? workspace : C; p.C2 = nullptr; p.bias = nullptr; p.aux = nullptr; p.pre = nullptr; p.resid = nullptr;
  p.M = M; p.N = N; p.K = K / ksplits; p.lda = lda; p.ldb = ldb; p.ldc = ldc;
  p.act = ACT_NONE; p.accumulate = accumulate;
  const long kl = K / ksplits;
  p.vecC = 0;
  p.vecA = aligned16(A) && (lda % 4 == 0) && (sA0 % 4 == 0) && (sA1 % 4 == 0) && (kl % 4 == 0);
  p.vecB = aligned16(B) && (ldb % 4 == 0) && (sB0 % 4 == 0) && (sB1 % 4 == 0);
  p.rowsum = nullptr; p.rowsum_acc = 0;
  p.rowscale = nullptr; p.kscale = nullptr; p.rows_per = p.krows_per = 1;
  p.nb1 = nb1; p.nb2 = ksplits;
  p.sA0 = sA0; p.sA1 = sA1; p.sB0 = sB0; p.sB1 = sB1; p.sC0 = sC0; p.sC1 = sC1;
  p.sA2 = kl; p.sB2 = kl * ldb; p.sC2 = c_elems;
  p.ksplit_len = p.K; p.splits = 1; p.slabs = nullptr; p.rs_slabs = nullptr;
  int BM = 64, BN = 64;
  if (N <= 32) { BM = 128; BN = 32; }
  const long tiles = (long)((M + BM - 1) / BM) * ((N + BN - 1) / BN);
  p.tiles = (int)tiles;
  GemmPlan pl{};
  pl.route = ROUTE_TILED; pl.bm = BM; pl.bn = BN; pl.a_kmajor = a_kmajor; pl.b_kmajor = b_kmajor;
  pl.splits = 1; pl.klen = p.K; pl.tiles = p.tiles;
  pl.nwg = (unsigned)tiles; pl.nbatch = (unsigned)(nb0 * nb1 * ksplits);
  hipStream_t s = (hipStream_t)stream;
  pl.kgroups = choose_kgroups((long)pl.nwg * pl.nbatch, (p.K + GEMM_BK - 1) / GEMM_BK);
  launch_tiled(p, pl, s);
  if (int e = check_launch("rscotr_gemm_f32_batched")) return e;
  if (ksplits > 1) {
    launch_slab_sum(workspace, C, c_elems / 4, ksplits, s);
    return check_launch("rscotr_gemm_f32_batched (slab sum)");
  }
  return RSCOTR_OK;
}
