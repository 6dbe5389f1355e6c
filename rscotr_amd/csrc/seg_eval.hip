// Segmentation evaluation on the device (include/rscotr.h: rscotr_seg_predict_u8, rscotr_seg_areas_u8).
//
// seg_predict: MTL.whole_inference_seg + the test-time flip + arg-max over channels in one launch.  The head's logits
// (B, C, h, w) are a few MB and stay in L2; every output pixel composes the two bilinear resamplings of the torch chain
// (logits -> canvas, canvas[:hs, :ws] -> ori_shape) per channel in registers, so no up-sampled tensor is ever written.
// One thread per output pixel, a wavefront along x: neighbouring lanes share or neighbour their 16 source taps, which the
// vector L1 serves.  The tap indices and weights do not depend on the channel and are computed once per thread.
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
