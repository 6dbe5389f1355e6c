// Segmentation evaluation on the device (include/rscotr.h: rscotr_seg_predict_u8, rscotr_seg_predict_tta_u8,
// rscotr_seg_areas_u8).
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
// seg_areas: mmseg intersect_and_union of a batch.  Per-workgroup LDS histograms over all 256 byte values, then 64-bit
// integer adds of the first C bins into the caller-zeroed output: exact in any order.
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
