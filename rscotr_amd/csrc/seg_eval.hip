// Segmentation evaluation on the device (include/rscotr.h: rscotr_seg_predict_u8, rscotr_seg_predict_slide_u8,
// rscotr_seg_predict_tta_u8, rscotr_seg_areas_u8).
//
// seg_predict: MTL.whole_inference_seg + the test-time flip + arg-max over channels in one launch.  The head's logits
// (B, C, h, w) are a few MB and stay in L2; every output pixel composes the two bilinear resamplings of the torch chain
// (logits -> canvas, canvas[:hs, :ws] -> ori_shape) per channel in registers, so no up-sampled tensor is ever written.
// One thread per output pixel, a wavefront along x: neighbouring lanes share or neighbour their 16 source taps, which the
// vector L1 serves.  The tap indices and weights do not depend on the channel and are computed once per thread.
//
// seg_predict_tta: mmseg aug_test (multi-scale / flip testing, mode 'whole') of a batch in one launch.  Each thread owns one
// output pixel and walks the V views in order: the composed two-stage value of every channel as above, softmax over the
// channels, and the probabilities added into the pixel's C accumulators, which live in dynamic LDS laid out [c][pixel of the
// tile]: a wavefront's 64 lanes touch 64 consecutive words (no bank conflict), every lane owns its column (no barrier, no
// cross-lane traffic).  A workgroup is one wavefront row of 64 pixels along x times T rows, T chosen by the host from C so that
// the accumulators take at most 64 KB (at least two workgroups per CU).  The softmax needs the channel maximum and the sum
// before the first probability, so the channels are walked three times per view (max, sum, accumulate) and the 16-tap value
// is RECOMPUTED in each pass instead of being stashed in a second LDS column: the stash would double the LDS per pixel, and
// LDS per pixel (C words) is already what bounds the occupancy (six wavefronts per CU at C = 100); halving it again to
// save 32 L1 / L2 hits per channel starves the latency hiding that those very loads need.  The view table rides in the kernel
// arguments (scalar loads, no device table).
//
// seg_predict_slide: mmseg slide_inference (test mode 'slide') + rescale + flip + arg-max in one launch over the logits of ALL
// windows, (Gy Gx B, C, h, w) in visiting order.  The grid is regular, so the kernel derives it from (H, W, crop, stride): the
// windows covering a canvas coordinate are a contiguous index range per axis (only the last window of an axis is shifted back).
// Thread layout as seg_predict.  Per channel, in registers: the in-order sum over the covering windows of the window's 4-tap
// value, divided by their number, at the one canvas position (no rescale) or at the four positions of the outer taps, then the
// running arg-max; no canvas-sized tensor, no atomics.  The number of covering windows is dynamic (crop / stride is the user's),
// so the per-axis taps of (canvas coordinate, window), which do not depend on the channel, cannot sit in registers: each thread
// computes them once into a private column of dynamic LDS laid out [slot][pixel of the tile] (conflict-free, no barrier, as
// the TTA accumulators), 3 words per tap, 2 (Ky + Kx) taps with rescale.  That is 36 KB per 256 pixels at crop 512 / stride
// 341 (at most 3 windows per axis), against C words per pixel in the TTA kernel: four workgroups per CU still fit, so here the
// stash is the cheaper side of the trade-off, and the host shrinks the tile (T rows of 64) to keep it under 64 KB.  Where even
// one row does not fit (more than 42 windows over a pixel's two axes), the same kernel recomputes the taps in the loop.  A
// pixel under one window without rescale takes the body of seg_predict's plain path.
//
// seg_areas: mmseg intersect_and_union of a batch.  Per-workgroup LDS histograms over all 256 byte values, then 64-bit
// integer adds of the first C bins into the caller-zeroed output: exact in any order.
#include <algorithm>

#include "common.h"

namespace rscotr {
namespace {

// One axis of ATen's upsample_bilinear2d (align_corners = False): destination index -> lower / upper tap and their weights.
struct Tap {
  int i0, i1;
  float l0, l1;
};

__device__ __forceinline__ Tap bilinear_tap(int dst, float scale, int in) {
  float src = __fsub_rn(__fmul_rn(scale, (float)dst + 0.5f), 0.5f);  // (product and difference rounded separately)
  src = src < 0.f ? 0.f : src;
  Tap t;
  t.i0 = min((int)src, in - 1);
  t.i1 = min(t.i0 + 1, in - 1);
  t.l1 = src - (float)t.i0;
  t.l0 = 1.f - t.l1;
  return t;
}

// the lambda-weighted four-tap value as ATen writes it: rows outside, columns inside
__device__ __forceinline__ float blend(float hl0, float hl1, float wl0, float wl1, float v00, float v01, float v10, float v11) {
  return hl0 * (wl0 * v00 + wl1 * v01) + hl1 * (wl0 * v10 + wl1 * v11);
}

// torch.argmax over an ascending channel loop: first index on ties, a NaN wins, the first NaN wins among several
__device__ __forceinline__ void argmax_step(float v, int c, float& best, int& idx) {
  if (best == best && !(v <= best)) {
    best = v;
    idx = c;
  }
}

template <bool kRescale>
__global__ __launch_bounds__(256) void seg_predict_kernel(const float* __restrict__ logit, uint8_t* __restrict__ out, int C, int h,
                                                          int w, int H, int W, int hs, int ws, int Ho, int Wo, int flip) {
  const int x = blockIdx.x * 64 + threadIdx.x;
  const int y = blockIdx.y * 4 + threadIdx.y;
  if (x >= Wo || y >= Ho) return;
  // the flip acts on the finished map: output (y, x) holds the prediction at the mirrored coordinate
  const int px = flip == 1 ? Wo - 1 - x : x;
  const int py = flip == 2 ? Ho - 1 - y : y;
  const float s1y = (float)h / (float)H, s1x = (float)w / (float)W;
  const long plane = (long)h * w;
  const float* __restrict__ base = logit + (long)blockIdx.z * C * plane;
  uint8_t* __restrict__ dst = out + ((long)blockIdx.z * Ho + y) * Wo + x;

  if constexpr (!kRescale) {
    const Tap ty = bilinear_tap(py, s1y, h), tx = bilinear_tap(px, s1x, w);
    const int o00 = ty.i0 * w + tx.i0, o01 = ty.i0 * w + tx.i1, o10 = ty.i1 * w + tx.i0, o11 = ty.i1 * w + tx.i1;
    float best = blend(ty.l0, ty.l1, tx.l0, tx.l1, base[o00], base[o01], base[o10], base[o11]);
    int idx = 0;
#pragma unroll 4
    for (int c = 1; c < C; ++c) {
      const float* __restrict__ p = base + c * plane;
      argmax_step(blend(ty.l0, ty.l1, tx.l0, tx.l1, p[o00], p[o01], p[o10], p[o11]), c, best, idx);
    }
    *dst = (uint8_t)idx;
    return;
  }

  // stage 2: four taps on the (hs, ws) crop of the canvas grid; stage 1: each of them is a four-tap value on (h, w)
  const Tap t2y = bilinear_tap(py, (float)hs / (float)Ho, hs), t2x = bilinear_tap(px, (float)ws / (float)Wo, ws);
  const Tap ya = bilinear_tap(t2y.i0, s1y, h), yb = bilinear_tap(t2y.i1, s1y, h);
  const Tap xa = bilinear_tap(t2x.i0, s1x, w), xb = bilinear_tap(t2x.i1, s1x, w);
  const int ra0 = ya.i0 * w, ra1 = ya.i1 * w, rb0 = yb.i0 * w, rb1 = yb.i1 * w;
  float best = 0.f;
  int idx = 0;
#pragma unroll 2
  for (int c = 0; c < C; ++c) {
    const float* __restrict__ p = base + c * plane;
    const float a00 = p[ra0 + xa.i0], a01 = p[ra0 + xa.i1], a02 = p[ra0 + xb.i0], a03 = p[ra0 + xb.i1];
    const float a10 = p[ra1 + xa.i0], a11 = p[ra1 + xa.i1], a12 = p[ra1 + xb.i0], a13 = p[ra1 + xb.i1];
    const float b00 = p[rb0 + xa.i0], b01 = p[rb0 + xa.i1], b02 = p[rb0 + xb.i0], b03 = p[rb0 + xb.i1];
    const float b10 = p[rb1 + xa.i0], b11 = p[rb1 + xa.i1], b12 = p[rb1 + xb.i0], b13 = p[rb1 + xb.i1];
    const float v00 = blend(ya.l0, ya.l1, xa.l0, xa.l1, a00, a01, a10, a11);  // canvas (t2y.i0, t2x.i0)
    const float v01 = blend(ya.l0, ya.l1, xb.l0, xb.l1, a02, a03, a12, a13);  // canvas (t2y.i0, t2x.i1)
    const float v10 = blend(yb.l0, yb.l1, xa.l0, xa.l1, b00, b01, b10, b11);  // canvas (t2y.i1, t2x.i0)
    const float v11 = blend(yb.l0, yb.l1, xb.l0, xb.l1, b02, b03, b12, b13);  // canvas (t2y.i1, t2x.i1)
    const float v = blend(t2y.l0, t2y.l1, t2x.l0, t2x.l1, v00, v01, v10, v11);
    if (c == 0) best = v;
    else argmax_step(v, c, best, idx);
  }
  *dst = (uint8_t)idx;
}

// ---- test-time augmentation: V views, softmax, mean, arg-max ----------------------------------------------------------------
constexpr int kTtaViewsMax = 16;

struct TtaView {
  const float* logit;  // (B, C, h, w)
  int h, w, H, W, hs, ws, flip;
};
struct TtaViews {
  TtaView v[kTtaViewsMax];
};

// the taps of one output pixel in one view: the kRescale body of seg_predict_kernel, channel-independent
struct TtaTaps {
  Tap t2y, t2x, ya, yb, xa, xb;
  int ra0, ra1, rb0, rb1;
};

__device__ __forceinline__ float tta_value(const float* __restrict__ p, const TtaTaps& k) {
  const float a00 = p[k.ra0 + k.xa.i0], a01 = p[k.ra0 + k.xa.i1], a02 = p[k.ra0 + k.xb.i0], a03 = p[k.ra0 + k.xb.i1];
  const float a10 = p[k.ra1 + k.xa.i0], a11 = p[k.ra1 + k.xa.i1], a12 = p[k.ra1 + k.xb.i0], a13 = p[k.ra1 + k.xb.i1];
  const float b00 = p[k.rb0 + k.xa.i0], b01 = p[k.rb0 + k.xa.i1], b02 = p[k.rb0 + k.xb.i0], b03 = p[k.rb0 + k.xb.i1];
  const float b10 = p[k.rb1 + k.xa.i0], b11 = p[k.rb1 + k.xa.i1], b12 = p[k.rb1 + k.xb.i0], b13 = p[k.rb1 + k.xb.i1];
  const float v00 = blend(k.ya.l0, k.ya.l1, k.xa.l0, k.xa.l1, a00, a01, a10, a11);
  const float v01 = blend(k.ya.l0, k.ya.l1, k.xb.l0, k.xb.l1, a02, a03, a12, a13);
  const float v10 = blend(k.yb.l0, k.yb.l1, k.xa.l0, k.xa.l1, b00, b01, b10, b11);
  const float v11 = blend(k.yb.l0, k.yb.l1, k.xb.l0, k.xb.l1, b02, b03, b12, b13);
  return blend(k.t2y.l0, k.t2y.l1, k.t2x.l0, k.t2x.l1, v00, v01, v10, v11);
}

// block (64, T): acc[c * 64 T + threadIdx.y * 64 + threadIdx.x], C * 64 T floats of dynamic LDS.  No barrier anywhere: a
// thread outside the map leaves at once, every other thread reads and writes its own column only.
__global__ __launch_bounds__(256) void seg_predict_tta_kernel(const TtaViews views, uint8_t* __restrict__ out, int V, int C, int Ho,
                                                              int Wo) {
  extern __shared__ __attribute__((aligned(16))) float tta_acc[];
  const int x = blockIdx.x * 64 + threadIdx.x;
  const int y = blockIdx.y * blockDim.y + threadIdx.y;
  if (x >= Wo || y >= Ho) return;
  const int cols = 64 * blockDim.y;
  float* __restrict__ acc = tta_acc + threadIdx.y * 64 + threadIdx.x;

  for (int v = 0; v < V; ++v) {
    const TtaView vw = views.v[v];
    const int h = vw.h, w = vw.w;
    const int px = vw.flip == 1 ? Wo - 1 - x : x;
    const int py = vw.flip == 2 ? Ho - 1 - y : y;
    const float s1y = (float)h / (float)vw.H, s1x = (float)w / (float)vw.W;
    TtaTaps k;
    k.t2y = bilinear_tap(py, (float)vw.hs / (float)Ho, vw.hs);
    k.t2x = bilinear_tap(px, (float)vw.ws / (float)Wo, vw.ws);
    k.ya = bilinear_tap(k.t2y.i0, s1y, h);
    k.yb = bilinear_tap(k.t2y.i1, s1y, h);
    k.xa = bilinear_tap(k.t2x.i0, s1x, w);
    k.xb = bilinear_tap(k.t2x.i1, s1x, w);
    k.ra0 = k.ya.i0 * w, k.ra1 = k.ya.i1 * w, k.rb0 = k.yb.i0 * w, k.rb1 = k.yb.i1 * w;
    const int plane = h * w;
    const float* __restrict__ base = vw.logit + (long)blockIdx.z * C * plane;

    // torch.softmax: the maximum propagates a NaN (every probability of the pixel is then NaN)
    float mx = tta_value(base, k);
#pragma unroll 4
    for (int c = 1; c < C; ++c) {
      const float t = tta_value(base + c * plane, k);
      mx = (t > mx || t != t) ? t : mx;
    }
    float sum = 0.f;
#pragma unroll 4
    for (int c = 0; c < C; ++c) sum += expf(tta_value(base + c * plane, k) - mx);
    if (v == 0) {
#pragma unroll 4
      for (int c = 0; c < C; ++c) acc[c * cols] = __fdiv_rn(expf(tta_value(base + c * plane, k) - mx), sum);
    } else {
#pragma unroll 4
      for (int c = 0; c < C; ++c) acc[c * cols] += __fdiv_rn(expf(tta_value(base + c * plane, k) - mx), sum);
    }
  }

  const float nv = (float)V;
  float best = __fdiv_rn(acc[0], nv);
  int idx = 0;
  for (int c = 1; c < C; ++c) argmax_step(__fdiv_rn(acc[c * cols], nv), c, best, idx);
  out[((long)blockIdx.z * Ho + y) * Wo + x] = (uint8_t)idx;
}

// ---- test mode 'slide': the windows' logits merged, rescaled and arg-maxed -------------------------------------------------
// One axis of the window grid (mmseg slide_inference): g windows of `crop` (already min(crop, n)) every `stride`, the last one
// shifted back inside [0, n).
struct SlideAxis {
  int n, crop, stride, g, in;  // in: the logits' extent on this axis
  float scale;                 // in / crop: every window is resampled to the common window size
};

// the windows covering canvas coordinate pos: lo .. lo + cnt - 1 (stride <= crop wherever n > crop: cnt >= 1)
__device__ __forceinline__ void slide_cover(int pos, const SlideAxis& a, int& lo, int& cnt) {
  lo = pos >= a.crop ? (pos - a.crop) / a.stride + 1 : 0;
  lo = min(lo, a.g - 1);
  int hi = min(pos / a.stride, a.g - 2);
  if (pos >= a.n - a.crop) hi = a.g - 1;  // the shifted last window
  cnt = hi - lo + 1;
}

// the tap of canvas coordinate pos in window i: offsets in elements (mul = the axis's element stride) and the upper weight
struct SlideTap {
  int o0, o1;
  float l1;
};

__device__ __forceinline__ SlideTap slide_tap(int pos, int i, const SlideAxis& a, int mul) {
  const int start = max(min(i * a.stride + a.crop, a.n) - a.crop, 0);
  const Tap t = bilinear_tap(pos - start, a.scale, a.in);
  return SlideTap{t.i0 * mul, t.i1 * mul, t.l1};
}

// a thread's stash column: word `slot` of the thread lives at stash[slot * cols]
__device__ __forceinline__ void stash_put(int* __restrict__ stash, int cols, int slot, const SlideTap& t) {
  stash[(3 * slot) * cols] = t.o0;
  stash[(3 * slot + 1) * cols] = t.o1;
  stash[(3 * slot + 2) * cols] = __float_as_int(t.l1);
}

__device__ __forceinline__ SlideTap stash_get(const int* __restrict__ stash, int cols, int slot) {
  return SlideTap{stash[(3 * slot) * cols], stash[(3 * slot + 1) * cols], __int_as_float(stash[(3 * slot + 2) * cols])};
}

// One canvas position of one channel: preds (zeros) += the window's resampled logits, in window order (y outer), / count.
// p: channel c of window 0 of this image; wstride: elements between consecutive windows (B C h w).  ys / xs: first stash slot
// of this position's y / x taps (kStash), else the taps are recomputed from (Y, X).
template <bool kStash>
__device__ __forceinline__ float slide_canvas(const float* __restrict__ p, long wstride, int Gx, int Y, int X, int ylo, int ny,
                                              int xlo, int nx, const SlideAxis& ay, const SlideAxis& ax, const int* __restrict__ stash,
                                              int cols, int ys, int xs) {
  float sum = 0.f;
  for (int iy = 0; iy < ny; ++iy) {
    const SlideTap ty = kStash ? stash_get(stash, cols, ys + iy) : slide_tap(Y, ylo + iy, ay, ax.in);
    const float hl0 = 1.f - ty.l1;
    const float* __restrict__ q = p + ((long)(ylo + iy) * Gx + xlo) * wstride;
    for (int ix = 0; ix < nx; ++ix, q += wstride) {
      const SlideTap tx = kStash ? stash_get(stash, cols, xs + ix) : slide_tap(X, xlo + ix, ax, 1);
      sum += blend(hl0, ty.l1, 1.f - tx.l1, tx.l1, q[ty.o0 + tx.o0], q[ty.o0 + tx.o1], q[ty.o1 + tx.o0], q[ty.o1 + tx.o1]);
    }
  }
  return __fdiv_rn(sum, (float)(ny * nx));
}

// block (64, T).  kStash: 3 * kP * (KY + KX) * 64 T words of dynamic LDS, kP = 2 canvas coordinates per axis with rescale, else 1;
// KY / KX: the host's bound on the windows covering one coordinate.  Thread-private columns: no barrier.
template <bool kRescale, bool kStash>
__global__ __launch_bounds__(256) void seg_predict_slide_kernel(const float* __restrict__ logit, uint8_t* __restrict__ out, int B, int C,
                                                                SlideAxis ay, SlideAxis ax, int KY, int KX, int hs, int ws, int Ho,
                                                                int Wo, int flip) {
  extern __shared__ __attribute__((aligned(16))) int slide_stash[];
  const int x = blockIdx.x * 64 + threadIdx.x;
  const int y = blockIdx.y * blockDim.y + threadIdx.y;
  if (x >= Wo || y >= Ho) return;
  const int px = flip == 1 ? Wo - 1 - x : x;
  const int py = flip == 2 ? Ho - 1 - y : y;
  const int cols = 64 * blockDim.y;
  const int* __restrict__ stash = slide_stash + threadIdx.y * 64 + threadIdx.x;
  const long plane = (long)ay.in * ax.in;
  const long wstride = (long)B * C * plane;
  const float* __restrict__ base = logit + (long)blockIdx.z * C * plane;  // image b of window 0
  uint8_t* __restrict__ dst = out + ((long)blockIdx.z * Ho + y) * Wo + x;
  constexpr int kP = kRescale ? 2 : 1;

  Tap t2y, t2x;
  int Ys[kP], Xs[kP], ylo[kP], ny[kP], xlo[kP], nx[kP];
  if constexpr (kRescale) {
    t2y = bilinear_tap(py, (float)hs / (float)Ho, hs);
    t2x = bilinear_tap(px, (float)ws / (float)Wo, ws);
    Ys[0] = t2y.i0, Ys[1] = t2y.i1, Xs[0] = t2x.i0, Xs[1] = t2x.i1;
  } else {
    Ys[0] = py, Xs[0] = px;
  }
#pragma unroll
  for (int j = 0; j < kP; ++j) {
    slide_cover(Ys[j], ay, ylo[j], ny[j]);
    slide_cover(Xs[j], ax, xlo[j], nx[j]);
    ny[j] = min(ny[j], KY);  // (never binds: KY, KX bound the cover; keeps the stash column in its slots)
    nx[j] = min(nx[j], KX);
  }

  if constexpr (!kRescale) {
    if (ny[0] == 1 && nx[0] == 1) {  // one window, no division: seg_predict's plain path on that window's logits
      const SlideTap ty = slide_tap(py, ylo[0], ay, ax.in), tx = slide_tap(px, xlo[0], ax, 1);
      const float hl0 = 1.f - ty.l1, wl0 = 1.f - tx.l1;
      const int o00 = ty.o0 + tx.o0, o01 = ty.o0 + tx.o1, o10 = ty.o1 + tx.o0, o11 = ty.o1 + tx.o1;
      const float* __restrict__ p = base + ((long)ylo[0] * ax.g + xlo[0]) * wstride;
      float best = blend(hl0, ty.l1, wl0, tx.l1, p[o00], p[o01], p[o10], p[o11]);
      int idx = 0;
#pragma unroll 4
      for (int c = 1; c < C; ++c) {
        p += plane;
        argmax_step(blend(hl0, ty.l1, wl0, tx.l1, p[o00], p[o01], p[o10], p[o11]), c, best, idx);
      }
      *dst = (uint8_t)idx;
      return;
    }
  }

  if constexpr (kStash) {
    int* __restrict__ mine = slide_stash + threadIdx.y * 64 + threadIdx.x;
#pragma unroll
    for (int j = 0; j < kP; ++j) {
      for (int i = 0; i < ny[j]; ++i) stash_put(mine, cols, j * KY + i, slide_tap(Ys[j], ylo[j] + i, ay, ax.in));
      for (int i = 0; i < nx[j]; ++i) stash_put(mine, cols, kP * KY + j * KX + i, slide_tap(Xs[j], xlo[j] + i, ax, 1));
    }
  }

  float best = 0.f;
  int idx = 0;
  for (int c = 0; c < C; ++c) {
    const float* __restrict__ p = base + c * plane;
    float v;
    if constexpr (kRescale) {
      float q[2][2];
#pragma unroll
      for (int jy = 0; jy < 2; ++jy)
#pragma unroll
        for (int jx = 0; jx < 2; ++jx)
          q[jy][jx] = slide_canvas<kStash>(p, wstride, ax.g, Ys[jy], Xs[jx], ylo[jy], ny[jy], xlo[jx], nx[jx], ay, ax, stash, cols,
                                           jy * KY, kP * KY + jx * KX);
      v = blend(t2y.l0, t2y.l1, t2x.l0, t2x.l1, q[0][0], q[0][1], q[1][0], q[1][1]);
    } else {
      v = slide_canvas<kStash>(p, wstride, ax.g, Ys[0], Xs[0], ylo[0], ny[0], xlo[0], nx[0], ay, ax, stash, cols, 0, kP * KY);
    }
    if (c == 0) best = v;
    else argmax_step(v, c, best, idx);
  }
  *dst = (uint8_t)idx;
}

constexpr int kAreaThreads = 256;
constexpr int kAreaBlocksMax = 64;    // workgroups per image
constexpr int kAreaPixPerBlock = 4096;

__global__ __launch_bounds__(kAreaThreads) void seg_areas_kernel(const uint8_t* __restrict__ pred, const uint8_t* __restrict__ gt,
                                                                 unsigned long long* __restrict__ out, long n, int C,
                                                                 int ignore_index, int reduce_zero_label) {
  __shared__ unsigned hist[3][256];  // intersect, pred, label: indexed by the byte value, so no index can leave a row
  for (int i = threadIdx.x; i < 3 * 256; i += kAreaThreads) (&hist[0][0])[i] = 0u;
  __syncthreads();
  const uint8_t* __restrict__ p = pred + (long)blockIdx.y * n;
  const uint8_t* __restrict__ g = gt + (long)blockIdx.y * n;
  for (long i = (long)blockIdx.x * kAreaThreads + threadIdx.x; i < n; i += (long)gridDim.x * kAreaThreads) {
    int l = g[i];
    const int q = p[i];
    if (reduce_zero_label) {  // mmseg LoadAnnotations order, as metrics.confusion_matrix
      if (l == 0) l = 255;
      if (l != 255) l -= 1;
      if (l == 254) l = 255;
    }
    if (l == ignore_index) continue;
    atomicAdd(&hist[1][q], 1u);
    atomicAdd(&hist[2][l], 1u);
    if (q == l) atomicAdd(&hist[0][q], 1u);
  }
  __syncthreads();
  // bins >= C fall out of their own histogram only (torch.histc in mmseg); union = pred + label - intersect is linear
  unsigned long long* __restrict__ o = out + (long)blockIdx.y * 4 * C;
  for (int c = threadIdx.x; c < C; c += kAreaThreads) {
    const unsigned long long ni = hist[0][c], np = hist[1][c], nl = hist[2][c];
    if (ni) atomicAdd(o + c, ni);
    if (np + nl - ni) atomicAdd(o + C + c, np + nl - ni);
    if (np) atomicAdd(o + 2 * C + c, np);
    if (nl) atomicAdd(o + 3 * C + c, nl);
  }
}

}  // namespace
}  // namespace rscotr

using namespace rscotr;

extern "C" int rscotr_seg_predict_u8(const float* logit, uint8_t* out, int B, int C, int h, int w, int H, int W, int rescale,
                                     int hs, int ws, int Ho, int Wo, int flip, void* stream) {
  const char* fn = "rscotr_seg_predict_u8";
  if (B <= 0 || C <= 0 || h <= 0 || w <= 0 || H <= 0 || W <= 0) return fail(RSCOTR_E_SHAPE, "%s: non-positive size", fn);
  if (C > 255) return fail(RSCOTR_E_SHAPE, "%s: C = %d does not fit a uint8 label map (C <= 255)", fn, C);
  if (flip < 0 || flip > 2) return fail(RSCOTR_E_ARG, "%s: flip must be 0 (none), 1 (horizontal) or 2 (vertical)", fn);
  if (rescale) {
    if (hs <= 0 || ws <= 0 || Ho <= 0 || Wo <= 0) return fail(RSCOTR_E_SHAPE, "%s: non-positive size", fn);
    if (hs > H || ws > W) return fail(RSCOTR_E_SHAPE, "%s: crop %d x %d larger than the canvas %d x %d", fn, hs, ws, H, W);
  } else {
    Ho = H;
    Wo = W;
  }
  if (B > 65535 || (Ho + 3) / 4 > 65535) return fail(RSCOTR_E_SHAPE, "%s: B <= 65535 and Ho <= 262140", fn);
  if ((int64_t)C * h * w > INT32_MAX) return fail(RSCOTR_E_SHAPE, "%s: C * h * w must fit 31 bits", fn);
  if (!logit || !out) return fail(RSCOTR_E_ARG, "%s: null pointer", fn);
  const dim3 grid((Wo + 63) / 64, (Ho + 3) / 4, B), block(64, 4);
  if (rescale)
    seg_predict_kernel<true><<<grid, block, 0, (hipStream_t)stream>>>(logit, out, C, h, w, H, W, hs, ws, Ho, Wo, flip);
  else
    seg_predict_kernel<false><<<grid, block, 0, (hipStream_t)stream>>>(logit, out, C, h, w, H, W, H, W, Ho, Wo, flip);
  return check_launch(fn);
}

extern "C" int rscotr_seg_predict_slide_u8(const float* logit, uint8_t* out, int B, int C, int h, int w, int H, int W, int ch, int cw,
                                           int sy, int sx, int rescale, int hs, int ws, int Ho, int Wo, int flip, void* stream) {
  const char* fn = "rscotr_seg_predict_slide_u8";
  if (B <= 0 || C <= 0 || h <= 0 || w <= 0 || H <= 0 || W <= 0 || ch <= 0 || cw <= 0 || sy <= 0 || sx <= 0)
    return fail(RSCOTR_E_SHAPE, "%s: non-positive size", fn);
  if (C > 255) return fail(RSCOTR_E_SHAPE, "%s: C = %d does not fit a uint8 label map (C <= 255)", fn, C);
  if (flip < 0 || flip > 2) return fail(RSCOTR_E_ARG, "%s: flip must be 0 (none), 1 (horizontal) or 2 (vertical)", fn);
  if ((H > ch && sy > ch) || (W > cw && sx > cw))
    return fail(RSCOTR_E_SHAPE, "%s: stride %d x %d larger than the crop %d x %d leaves pixels of the %d x %d canvas uncovered", fn, sy,
                sx, ch, cw, H, W);
  if (rescale) {
    if (hs <= 0 || ws <= 0 || Ho <= 0 || Wo <= 0) return fail(RSCOTR_E_SHAPE, "%s: non-positive size", fn);
    if (hs > H || ws > W) return fail(RSCOTR_E_SHAPE, "%s: crop %d x %d larger than the canvas %d x %d", fn, hs, ws, H, W);
  } else {
    hs = Ho = H;
    ws = Wo = W;
  }
  if ((int64_t)C * h * w > INT32_MAX) return fail(RSCOTR_E_SHAPE, "%s: C * h * w must fit 31 bits", fn);
  // the window grid of mmseg slide_inference; every window has the size min(crop, image)
  const int gy = (int)(std::max((int64_t)H - ch + sy - 1, (int64_t)0) / sy) + 1;
  const int gx = (int)(std::max((int64_t)W - cw + sx - 1, (int64_t)0) / sx) + 1;
  if ((int64_t)gy * gx * B > INT32_MAX) return fail(RSCOTR_E_SHAPE, "%s: windows * B must fit 31 bits", fn);
  if (!logit || !out) return fail(RSCOTR_E_ARG, "%s: null pointer", fn);
  const int wh = std::min(ch, H), ww = std::min(cw, W);
  const SlideAxis ay{H, wh, sy, gy, h, (float)h / (float)wh}, ax{W, ww, sx, gx, w, (float)w / (float)ww};
  // at most ceil(crop / stride) unshifted windows and the shifted last one cover a coordinate
  const int KY = (int)std::min((int64_t)gy, ((int64_t)wh + sy - 1) / sy + 1), KX = (int)std::min((int64_t)gx, ((int64_t)ww + sx - 1) / sx + 1);
  const int64_t per_row = (int64_t)3 * (rescale ? 2 : 1) * ((int64_t)KY + KX) * 64 * sizeof(int);  // stash bytes of 64 pixels
  const bool stash = per_row <= 65536;  // (the 64 KB a launch may ask for without opting in)
  const int T = !stash || 4 * per_row <= 65536 ? 4 : 2 * per_row <= 65536 ? 2 : 1;
  if (B > 65535 || (Ho + T - 1) / T > 65535) return fail(RSCOTR_E_SHAPE, "%s: B <= 65535 and Ho <= %d", fn, 65535 * T);
  const dim3 grid((Wo + 63) / 64, (Ho + T - 1) / T, B), block(64, T);
  const size_t shm = stash ? (size_t)per_row * T : 0;
  hipStream_t st = (hipStream_t)stream;
  if (rescale) {
    if (stash) seg_predict_slide_kernel<true, true><<<grid, block, shm, st>>>(logit, out, B, C, ay, ax, KY, KX, hs, ws, Ho, Wo, flip);
    else seg_predict_slide_kernel<true, false><<<grid, block, 0, st>>>(logit, out, B, C, ay, ax, KY, KX, hs, ws, Ho, Wo, flip);
  } else {
    if (stash) seg_predict_slide_kernel<false, true><<<grid, block, shm, st>>>(logit, out, B, C, ay, ax, KY, KX, hs, ws, Ho, Wo, flip);
    else seg_predict_slide_kernel<false, false><<<grid, block, 0, st>>>(logit, out, B, C, ay, ax, KY, KX, hs, ws, Ho, Wo, flip);
  }
  return check_launch(fn);
}

extern "C" int rscotr_seg_predict_tta_u8(const int64_t* views, uint8_t* out, int V, int B, int C, int Ho, int Wo, void* stream) {
  const char* fn = "rscotr_seg_predict_tta_u8";
  if (V < 1 || V > kTtaViewsMax) return fail(RSCOTR_E_SHAPE, "%s: V = %d views (1 <= V <= %d)", fn, V, kTtaViewsMax);
  if (B <= 0 || C <= 0 || Ho <= 0 || Wo <= 0) return fail(RSCOTR_E_SHAPE, "%s: non-positive size", fn);
  if (C > 255) return fail(RSCOTR_E_SHAPE, "%s: C = %d does not fit a uint8 label map (C <= 255)", fn, C);
  if (!views || !out) return fail(RSCOTR_E_ARG, "%s: null pointer", fn);
  const int T = C <= 64 ? 4 : C <= 128 ? 2 : 1;  // rows of 64 pixels per workgroup: C * 64 T floats <= 64 KB (65 280 B at C = 255)
  if (B > 65535 || (Ho + T - 1) / T > 65535) return fail(RSCOTR_E_SHAPE, "%s: B <= 65535 and Ho <= %d", fn, 65535 * T);
  TtaViews tv;
  const int64_t lim = INT32_MAX;
  for (int v = 0; v < kTtaViewsMax; ++v) {
    const int64_t* r = views + 8 * (v < V ? v : 0);  // (the unused rows repeat row 0: never read, never garbage)
    if (v < V) {
      for (int i = 1; i < 7; ++i)
        if (r[i] <= 0 || r[i] > lim) return fail(RSCOTR_E_SHAPE, "%s: view %d: non-positive size (or one past 31 bits)", fn, v);
      if (r[5] > r[3] || r[6] > r[4])
        return fail(RSCOTR_E_SHAPE, "%s: view %d: crop %lld x %lld larger than the canvas %lld x %lld", fn, v, (long long)r[5],
                    (long long)r[6], (long long)r[3], (long long)r[4]);
      if (r[7] < 0 || r[7] > 2) return fail(RSCOTR_E_ARG, "%s: view %d: flip must be 0 (none), 1 (horizontal) or 2 (vertical)", fn, v);
      if ((int64_t)C * r[1] * r[2] > lim) return fail(RSCOTR_E_SHAPE, "%s: view %d: C * h * w must fit 31 bits", fn, v);
      if (r[0] == 0) return fail(RSCOTR_E_ARG, "%s: view %d: null logit address", fn, v);
    }
    tv.v[v] = TtaView{reinterpret_cast<const float*>((uintptr_t)r[0]), (int)r[1], (int)r[2], (int)r[3], (int)r[4], (int)r[5], (int)r[6],
                      (int)r[7]};
  }
  const dim3 grid((Wo + 63) / 64, (Ho + T - 1) / T, B), block(64, T);
  // at most 65 280 B (C = 255, T = 1), 65 536 B at C = 64: within the 64 KB a launch may ask for without opting in, so no
  // hipFuncSetAttribute (the MSDA launches set it only above 64 KB)
  const size_t shm = (size_t)C * 64 * T * sizeof(float);
  seg_predict_tta_kernel<<<grid, block, shm, (hipStream_t)stream>>>(tv, out, V, C, Ho, Wo);
  return check_launch(fn);
}

extern "C" int rscotr_seg_areas_u8(const uint8_t* pred, const uint8_t* gt, int64_t* out, int B, int Hp, int Wp, int C,
                                   int ignore_index, int reduce_zero_label, void* stream) {
  const char* fn = "rscotr_seg_areas_u8";
  if (B <= 0 || Hp <= 0 || Wp <= 0 || C <= 0) return fail(RSCOTR_E_SHAPE, "%s: non-positive size", fn);
  if (C > 256) return fail(RSCOTR_E_SHAPE, "%s: C = %d exceeds the 256 values of a uint8 map", fn, C);
  if (B > 65535) return fail(RSCOTR_E_SHAPE, "%s: B <= 65535", fn);
  const int64_t n = (int64_t)Hp * Wp;
  if (n > INT32_MAX) return fail(RSCOTR_E_SHAPE, "%s: Hp * Wp must fit 31 bits", fn);
  if (!pred || !gt || !out) return fail(RSCOTR_E_ARG, "%s: null pointer", fn);
  int blocks = (int)((n + kAreaPixPerBlock - 1) / kAreaPixPerBlock);
  blocks = blocks > kAreaBlocksMax ? kAreaBlocksMax : blocks;
  seg_areas_kernel<<<dim3(blocks, B), kAreaThreads, 0, (hipStream_t)stream>>>(
      pred, gt, reinterpret_cast<unsigned long long*>(out), (long)n, C, ignore_index, reduce_zero_label ? 1 : 0);
  return check_launch(fn);
}
