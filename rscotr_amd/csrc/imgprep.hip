// Device-side input pipeline for gfx950: crop window -> flip (x, y or both) -> BGR->RGB + (x - mean) / std -> pad ->
// HWC uint8 to CHW float32 -> collate, one launch for a whole batch of ragged decoded images.
//
// Replaces, per sample on a CPU worker and then `collate`, the pipeline tail of the reference's dataset configs
//   cls  configs/_base_/cls/resisc_swin_224.py:14,36-38   RandomFlip, Normalize, ImageToTensor, Collect
//   det  configs/_base_/det/dior.py:15-19                 RandomFlip, Normalize, Pad(size_divisor=32), DefaultFormatBundle
//   seg  configs/_base_/seg/potsdam_IRRG_all.py:12-19     RandomCrop (window), RandomFlip, Normalize, Pad(size, pad_val=0,
//                                                         seg_pad_val), DefaultFormatBundle; LoadAnnotations(reduce_zero_label)
// (mmcv.imflip / imnormalize / impad, mmseg LoadAnnotations; the un-vendored mm* pipelines run these in NumPy/OpenCV
// on float32 copies of the image: ~6 passes over the pixels per sample plus the collate copy).  Resizing, the
// photometric and the erasing steps are the second pair of entries below (rscotr_img_aug_u8 / rscotr_seg_label_aug_u8);
// RandAugment is rscotr_img_frames_u8 below + randaug.hip; mmseg RandomRotate is the last pair (rscotr_img_aug_rot_u8 /
// rscotr_seg_label_rot_u8); decoding stays on the host.
// The flip word of every meta row is a bit set (mmcv imflip): bit 0 mirrors x ('horizontal'), bit 1 mirrors y ('vertical'),
// 3 = both ('diagonal').
//
// HBM-bound: reads 3 B and writes 12 B per output pixel; one thread per output pixel x position, the three channel
// planes written as coalesced float rows; source rows are read as bytes (3 consecutive bytes per thread: consecutive
// lanes read consecutive pixels, reversed under flip).
#include "common.h"

namespace rscotr {

// int64 per sample: byte offset, H, W, row stride (bytes), x0, y0, crop w, crop h, flip (bit 0: x, bit 1: y), -
constexpr int IMGPREP_META = 10;

struct PrepNorm {
  float mean[3], inv_std[3];
};

__global__ __launch_bounds__(256) void img_prep_kernel(const uint8_t* __restrict__ src, const int64_t* __restrict__ meta,
                                                       float* __restrict__ out, int Hout, int Wout, PrepNorm nm,
                                                       int to_rgb) {
  const int b = blockIdx.z, y = blockIdx.y;
  const int x = blockIdx.x * 256 + threadIdx.x;
  if (x >= Wout) return;
  const int64_t* m = meta + (long)b * IMGPREP_META;
  const long off = m[0], stride = m[3];
  const int x0 = (int)m[4], y0 = (int)m[5], cw = (int)m[6], ch = (int)m[7], flip = (int)m[8];
  float v[3] = {0.f, 0.f, 0.f};  // mmcv Pad runs after Normalize with pad_val = 0
  if (y < ch && x < cw) {
    const int sx = (flip & 1) ? cw - 1 - x : x, sy = (flip & 2) ? ch - 1 - y : y;
    const uint8_t* p = src + off + (long)(y0 + sy) * stride + (long)(x0 + sx) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float u = (float)p[to_rgb ? 2 - c : c];
      v[c] = (u - nm.mean[c]) * nm.inv_std[c];
    }
  }
  const long plane = (long)Hout * Wout;
  float* o = out + (long)b * 3 * plane + (long)y * Wout + x;
  o[0] = v[0];
  o[plane] = v[1];
  o[2 * plane] = v[2];
}

__global__ __launch_bounds__(256) void seg_label_prep_kernel(const uint8_t* __restrict__ src,
                                                             const int64_t* __restrict__ meta, int64_t* __restrict__ out,
                                                             int Hout, int Wout, int reduce_zero_label, int pad_val) {
  const int b = blockIdx.z, y = blockIdx.y;
  const int x = blockIdx.x * 256 + threadIdx.x;
  if (x >= Wout) return;
  const int64_t* m = meta + (long)b * IMGPREP_META;
  const long off = m[0], stride = m[3];
  const int x0 = (int)m[4], y0 = (int)m[5], cw = (int)m[6], ch = (int)m[7], flip = (int)m[8];
  int64_t v = pad_val;
  if (y < ch && x < cw) {
    const int sx = (flip & 1) ? cw - 1 - x : x, sy = (flip & 2) ? ch - 1 - y : y;
    int l = src[off + (long)(y0 + sy) * stride + (x0 + sx)];
    if (reduce_zero_label) {  // mmseg LoadAnnotations: 0 -> 255, l -> l - 1, 254 -> 255
      l = (l == 0) ? 255 : l - 1;
      if (l == 254) l = 255;
    }
    v = l;
  }
  out[((long)b * Hout + y) * Wout + x] = v;
}

}  // namespace rscotr

using namespace rscotr;

static int check_prep(const char* fn, const void* src, const void* meta, const void* out, int B, int Hout, int Wout) {
  if (B < 0 || Hout < 0 || Wout < 0) return fail(RSCOTR_E_SHAPE, "%s: negative dimension", fn);
  if (B > 65535 || Hout > 65535) return fail(RSCOTR_E_SHAPE, "%s: B and Hout must be <= 65535", fn);
  if (B && Hout && Wout && (!src || !meta || !out)) return fail(RSCOTR_E_ARG, "%s: null pointer", fn);
  return RSCOTR_OK;
}

extern "C" int rscotr_img_prep_u8(const uint8_t* src, const int64_t* meta, float* out, int B, int Hout, int Wout,
                                  const float* mean3, const float* std3, int to_rgb, void* stream) {
  if (int e = check_prep("rscotr_img_prep_u8", src, meta, out, B, Hout, Wout)) return e;
  if (!mean3 || !std3) return fail(RSCOTR_E_ARG, "rscotr_img_prep_u8: mean / std (3 host floats each) required");
  if (B == 0 || Hout == 0 || Wout == 0) return RSCOTR_OK;
  PrepNorm nm;
  for (int c = 0; c < 3; ++c) {
    if (!(std3[c] > 0.f)) return fail(RSCOTR_E_ARG, "rscotr_img_prep_u8: std[%d] must be positive", c);
    nm.mean[c] = mean3[c];
    nm.inv_std[c] = (float)(1.0 / (double)std3[c]);  // mmcv.imnormalize: stdinv = 1 / np.float64(std)
  }
  img_prep_kernel<<<dim3((Wout + 255) / 256, Hout, B), 256, 0, (hipStream_t)stream>>>(src, meta, out, Hout, Wout, nm,
                                                                                    to_rgb ? 1 : 0);
  return check_launch("rscotr_img_prep_u8");
}

extern "C" int rscotr_seg_label_prep_u8(const uint8_t* src, const int64_t* meta, int64_t* out, int B, int Hout, int Wout,
                                        int reduce_zero_label, int pad_val, void* stream) {
  if (int e = check_prep("rscotr_seg_label_prep_u8", src, meta, out, B, Hout, Wout)) return e;
  if (B == 0 || Hout == 0 || Wout == 0) return RSCOTR_OK;
  seg_label_prep_kernel<<<dim3((Wout + 255) / 256, Hout, B), 256, 0, (hipStream_t)stream>>>(src, meta, out, Hout, Wout,
                                                                                          reduce_zero_label, pad_val);
  return check_launch("rscotr_seg_label_prep_u8");
}

// ---- resample + photometric + erasing (rscotr_img_aug_u8 / rscotr_seg_label_aug_u8) ---------------------------------
// The same output geometry as img_prep_kernel (pad test, flip of the output index, window into a frame), but the frame is
// a RESIZED image: every output coordinate reads its source through a per-sample, per-axis table the host built
// (rscotr_amd/pipeline.py), so the kernel does integer work only and the result is exact and deterministic:
//   table entry (int32, stride K + 2): {first source index, tap count n <= K, w_0 .. w_{K-1}}; the crop window's offset
//   into the resized frame is folded into the entries (entry j describes resized coordinate x0 + j).
//   RESAMPLE_NEAREST  one tap, weights unused (mmcv imresize / imrescale 'nearest'; also the identity when no resize)
//   RESAMPLE_LINEAR   11-bit weights, (sum_y wy * sum_x wx * p + 2^21) >> 22 clamped to [0, 255]: the scalar fixed-point form
//                     of OpenCV's uint8 INTER_LINEAR (mmcv 'bilinear').  Parity with cv2 is unpinned (+-1 LSB expected).
//   RESAMPLE_PIL      Pillow ImagingResample, 22-bit weights: horizontal pass with its uint8-clipped intermediate, recomputed
//                     per output pixel for every vertical tap, then the vertical pass (mmcv imresize backend='pillow').
// Then the per-pixel PhotoMetricDistortion chain of mmseg 0.28 on the uint8 BGR triplet, the RandomErasing patch (uint8 in
// `src`, drawn on the host) and Normalize as in img_prep_kernel.  Reads <= n_y * n_x * 3 B and writes 12 B per output pixel.

enum { RESAMPLE_NEAREST = 0, RESAMPLE_LINEAR = 1, RESAMPLE_PIL = 2 };
// int64 per sample: byte offset, H, W, row stride (bytes), out w, out h, flip (bit 0: the output x index is mirrored, bit 1:
// the output y index), x-table offset, y-table offset (int32 units),
// x taps K, y taps K, resample mode, photometric flags, hue delta, erase x0, y0, w, h, patch byte offset, -
constexpr int IMGAUG_META = 20;
// photometric flags (bit set = step applied; mmseg PhotoMetricDistortion draws randint(2) per step and the mode)
enum { PM_BRIGHT = 1, PM_CONTRAST = 2, PM_CONTRAST_FIRST = 4, PM_SAT = 8, PM_HUE = 16 };
constexpr int IMGAUG_PARAMS = 4;  // float per sample: brightness beta, contrast alpha, saturation alpha, -

// OpenCV RGB2HSV_b tables (hsv_shift = 12, hrange = 180): sdiv[i] = saturate_cast<int>((255 << 12) / (1. * i)),
// hdiv180[i] = saturate_cast<int>((180 << 12) / (6. * i)); saturate_cast rounds half to even.
struct HsvTables {
  int sdiv[256], hdiv[256];
};
constexpr int round_half_even(double v) {
  const long i = (long)v;  // v >= 0 here
  const double f = v - (double)i;
  return (int)(f > 0.5 ? i + 1 : f < 0.5 ? i : (i % 2 ? i + 1 : i));
}
constexpr HsvTables make_hsv_tables() {
  HsvTables t{};
  for (int i = 1; i < 256; ++i) {
    t.sdiv[i] = round_half_even((double)(255 << 12) / (1.0 * i));
    t.hdiv[i] = round_half_even((double)(180 << 12) / (6.0 * i));
  }
  return t;
}
__constant__ HsvTables kHsv = make_hsv_tables();

__device__ __forceinline__ int clip8_pil(int v) {  // Pillow clip8: v >> 22 clamped to [0, 255]
  v >>= 22;
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// mmseg PhotoMetricDistortion.convert: float32(v) * alpha + beta (two rounded fp32 operations), clip, truncate
__device__ __forceinline__ int pm_convert(int v, float alpha, float beta) {
  float f = __fadd_rn(__fmul_rn((float)v, alpha), beta);
  f = fminf(fmaxf(f, 0.f), 255.f);
  return (int)f;
}

// cv2.cvtColor(COLOR_BGR2HSV), uint8 (RGB2HSV_b, scalar form)
__device__ __forceinline__ void bgr2hsv_u8(const int bgr[3], int hsv[3]) {
  const int b = bgr[0], g = bgr[1], r = bgr[2];
  const int v = max(b, max(g, r)), vmin = min(b, min(g, r));
  const int diff = v - vmin;
  const int vr = v == r ? -1 : 0, vg = v == g ? -1 : 0;
  const int s = (diff * kHsv.sdiv[v] + (1 << 11)) >> 12;
  int h = (vr & (g - b)) + (~vr & ((vg & (b - r + 2 * diff)) + ((~vg) & (r - g + 4 * diff))));
  h = (h * kHsv.hdiv[diff] + (1 << 11)) >> 12;
  h += h < 0 ? 180 : 0;
  hsv[0] = h;
  hsv[1] = s;
  hsv[2] = v;
}

__device__ __forceinline__ int sat_cast_u8(float f) {  // saturate_cast<uchar>(float): round half to even, clamp
  const int i = __float2int_rn(f);
  return i < 0 ? 0 : (i > 255 ? 255 : i);
}

// cv2.cvtColor(COLOR_HSV2BGR), uint8 (HSV2RGB_b: s scaled by 1/255 in float, HSV2RGB_native's sector form)
__device__ __forceinline__ void hsv2bgr_u8(const int hsv[3], int bgr[3]) {
#pragma clang fp contract(off)
  const float s = (float)hsv[1] * (1.0f / 255.0f), v = (float)hsv[2];
  float b, g, r;
  if (s == 0.f) {
    b = g = r = v;
  } else {
    const int sector_data[6][3] = {{1, 3, 0}, {1, 0, 2}, {3, 0, 1}, {0, 2, 1}, {0, 1, 3}, {2, 1, 0}};
    float h = (float)hsv[0] * (6.0f / 180.0f);
    h = fmodf(h, 6.f);
    int sector = (int)floorf(h);
    h -= (float)sector;
    if ((unsigned)sector >= 6u) {
      sector = 0;
      h = 0.f;
    }
    float tab[4];
    tab[0] = v;
    tab[1] = v * (1.f - s);
    tab[2] = v * (1.f - s * h);
    tab[3] = v * (1.f - s * (1.f - h));
    b = tab[sector_data[sector][0]];
    g = tab[sector_data[sector][1]];
    r = tab[sector_data[sector][2]];
  }
  bgr[0] = sat_cast_u8(b);
  bgr[1] = sat_cast_u8(g);
  bgr[2] = sat_cast_u8(r);
}

__device__ __forceinline__ void photometric(int u[3], int flags, int hue_delta, const float* prm) {
  if (flags & PM_BRIGHT)
    for (int c = 0; c < 3; ++c) u[c] = pm_convert(u[c], 1.f, prm[0]);
  if ((flags & PM_CONTRAST_FIRST) && (flags & PM_CONTRAST))
    for (int c = 0; c < 3; ++c) u[c] = pm_convert(u[c], prm[1], 0.f);
  if (flags & PM_SAT) {
    int hsv[3];
    bgr2hsv_u8(u, hsv);
    hsv[1] = pm_convert(hsv[1], prm[2], 0.f);
    hsv2bgr_u8(hsv, u);
  }
  if (flags & PM_HUE) {
    int hsv[3];
    bgr2hsv_u8(u, hsv);
    hsv[0] = ((hsv[0] + hue_delta) % 180 + 180) % 180;
    hsv2bgr_u8(hsv, u);
  }
  if (!(flags & PM_CONTRAST_FIRST) && (flags & PM_CONTRAST))
    for (int c = 0; c < 3; ++c) u[c] = pm_convert(u[c], prm[1], 0.f);
}

// One pixel of the resized, flipped frame: output coordinate (x, y) of sample row `m` -> the uint8 BGR triplet, through
// the host's per-axis tables.  Shared by img_aug_kernel and img_frames_kernel (the RandAugment path's first step).
__device__ __forceinline__ void resample_u8(const uint8_t* __restrict__ src, const int64_t* __restrict__ m,
                                            const int32_t* __restrict__ tables, int x, int y, int u[3]) {
  const int cw = (int)m[4], ch = (int)m[5], flip = (int)m[6];
  const long off = m[0], stride = m[3];
  const int j = (flip & 1) ? cw - 1 - x : x, i = (flip & 2) ? ch - 1 - y : y;
  const int kx = (int)m[9], ky = (int)m[10], mode = (int)m[11];
  const int32_t* tx = tables + m[7] + (long)j * (kx + 2);
  const int32_t* ty = tables + m[8] + (long)i * (ky + 2);
  const uint8_t* base = src + off;
  if (mode == RESAMPLE_NEAREST) {
    const uint8_t* p = base + (long)ty[0] * stride + (long)tx[0] * 3;
    u[0] = p[0];
    u[1] = p[1];
    u[2] = p[2];
  } else {
    const int nx = tx[1], ny = ty[1];
    const uint8_t* col = base + (long)tx[0] * 3;
    int acc[3] = {0, 0, 0};
    for (int a = 0; a < ny; ++a) {
      const uint8_t* row = col + (long)(ty[0] + a) * stride;
      int hs[3] = {0, 0, 0};
      if (mode == RESAMPLE_PIL) hs[0] = hs[1] = hs[2] = 1 << 21;
      for (int t = 0; t < nx; ++t) {
        const int w = tx[2 + t];
#pragma unroll
        for (int c = 0; c < 3; ++c) hs[c] += w * (int)row[t * 3 + c];
      }
      const int wy = ty[2 + a];
#pragma unroll
      for (int c = 0; c < 3; ++c) acc[c] += wy * (mode == RESAMPLE_PIL ? clip8_pil(hs[c]) : hs[c]);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) u[c] = mode == RESAMPLE_PIL ? clip8_pil(acc[c] + (1 << 21)) : min(max((acc[c] + (1 << 21)) >> 22, 0), 255);
  }
}

__global__ __launch_bounds__(256) void img_aug_kernel(const uint8_t* __restrict__ src, const int64_t* __restrict__ meta,
                                                      const int32_t* __restrict__ tables,
                                                      const float* __restrict__ params, float* __restrict__ out,
                                                      int Hout, int Wout, PrepNorm nm, int to_rgb) {
  const int b = blockIdx.z, y = blockIdx.y;
  const int x = blockIdx.x * 256 + threadIdx.x;
  if (x >= Wout) return;
  const int64_t* m = meta + (long)b * IMGAUG_META;
  const int cw = (int)m[4], ch = (int)m[5];
  float v[3] = {0.f, 0.f, 0.f};  // mmcv Pad runs after Normalize with pad_val = 0
  if (y < ch && x < cw) {
    int u[3];
    resample_u8(src, m, tables, x, y, u);
    if (m[12]) photometric(u, (int)m[12], (int)m[13], params + (long)b * IMGAUG_PARAMS);
    const int ex = x - (int)m[14], ey = y - (int)m[15];
    if (ex >= 0 && ey >= 0 && ex < (int)m[16] && ey < (int)m[17]) {  // mmcls RandomErasing: patch overwrite
      const uint8_t* p = src + m[18] + ((long)ey * m[16] + ex) * 3;
      u[0] = p[0];
      u[1] = p[1];
      u[2] = p[2];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = ((float)u[to_rgb ? 2 - c : c] - nm.mean[c]) * nm.inv_std[c];
  }
  const long plane = (long)Hout * Wout;
  float* o = out + (long)b * 3 * plane + (long)y * Wout + x;
  o[0] = v[0];
  o[plane] = v[1];
  o[2 * plane] = v[2];
}

__global__ __launch_bounds__(256) void seg_label_aug_kernel(const uint8_t* __restrict__ src,
                                                            const int64_t* __restrict__ meta,
                                                            const int32_t* __restrict__ tables,
                                                            int64_t* __restrict__ out, int Hout, int Wout,
                                                            int reduce_zero_label, int pad_val) {
  const int b = blockIdx.z, y = blockIdx.y;
  const int x = blockIdx.x * 256 + threadIdx.x;
  if (x >= Wout) return;
  const int64_t* m = meta + (long)b * IMGAUG_META;
  const int cw = (int)m[4], ch = (int)m[5];
  int64_t v = pad_val;
  if (y < ch && x < cw) {
    const int j = (m[6] & 1) ? cw - 1 - x : x, i = (m[6] & 2) ? ch - 1 - y : y;
    const int sx = tables[m[7] + (long)j * (m[9] + 2)], sy = tables[m[8] + (long)i * (m[10] + 2)];
    int l = src[m[0] + (long)sy * m[3] + sx];
    if (reduce_zero_label) {  // mmseg LoadAnnotations: 0 -> 255, l -> l - 1, 254 -> 255
      l = (l == 0) ? 255 : l - 1;
      if (l == 254) l = 255;
    }
    v = l;
  }
  out[((long)b * Hout + y) * Wout + x] = v;
}

// Step 1 of the RandAugment path (rscotr_img_frames_u8): the resample + flip half of img_aug_kernel, written as uint8 HWC BGR
// frames (B, H, W, 3) for the in-place operations of randaug.hip; no colour stage, no erasing, no normalize.  Pixels outside
// a sample's (out h, out w) are written 0.
__global__ __launch_bounds__(256) void img_frames_kernel(const uint8_t* __restrict__ src, const int64_t* __restrict__ meta,
                                                         const int32_t* __restrict__ tables, uint8_t* __restrict__ frames,
                                                         int H, int W) {
  const int b = blockIdx.z, y = blockIdx.y;
  const int x = blockIdx.x * 256 + threadIdx.x;
  if (x >= W) return;
  const int64_t* m = meta + (long)b * IMGAUG_META;
  int u[3] = {0, 0, 0};
  if (y < (int)m[5] && x < (int)m[4]) resample_u8(src, m, tables, x, y, u);
  uint8_t* o = frames + (((long)b * H + y) * W + x) * 3;
  o[0] = (uint8_t)u[0];
  o[1] = (uint8_t)u[1];
  o[2] = (uint8_t)u[2];
}

// ---- flip -> resize -> crop -> resize in one launch (rscotr_img_aug_chain_u8) ------------------------------------------------------
// mmdet's AutoAugment policy of the DETR recipe (Resize, RandomCrop, Resize(override)): the frame between the two resizes is a
// uint8 image on the CPU path; here it is never stored.  An output pixel reads its <= 2 x 2 pixels of frame 1 through the
// stage-2 entries (cv2 bilinear; coordinates of the crop window of frame 1), and each of them is made by resample_u8 through
// the stage-1 entries, rounded and clamped to uint8 as the stored frame would be; the stage-2 blend is the same fixed-point
// form.  So the result is bit-equal to the two passes, at <= 16 byte-triplet reads and 12 B written per output pixel.  The meta
// row is rscotr_img_aug_u8's: words 0 .. 11 describe stage 1 (out w / h = the crop window of frame 1, flip 0: an early flip is
// in the x entries, and in the y entries when it is vertical or diagonal), words 12 .. 15 = stage-2 x-table offset, y-table offset (entries of 4 words), final out w, out h.  A
// sample with one stage carries identity stage-2 entries (one tap of weight 2048).
__global__ __launch_bounds__(256) void img_aug_chain_kernel(const uint8_t* __restrict__ src, const int64_t* __restrict__ meta,
                                                            const int32_t* __restrict__ tables, float* __restrict__ out,
                                                            int Hout, int Wout, PrepNorm nm, int to_rgb) {
  const int b = blockIdx.z, y = blockIdx.y;
  const int x = blockIdx.x * 256 + threadIdx.x;
  if (x >= Wout) return;
  const int64_t* m = meta + (long)b * IMGAUG_META;
  float v[3] = {0.f, 0.f, 0.f};  // mmcv Pad runs after Normalize with pad_val = 0
  if (y < (int)m[15] && x < (int)m[14]) {
    const int32_t* tx = tables + m[12] + (long)x * 4;
    const int32_t* ty = tables + m[13] + (long)y * 4;
    const int nx = tx[1], ny = ty[1];
    int acc[3] = {0, 0, 0};
    for (int a = 0; a < ny; ++a) {
      int hs[3] = {0, 0, 0};
      for (int t = 0; t < nx; ++t) {
        int u[3];
        resample_u8(src, m, tables, tx[0] + t, ty[0] + a, u);
        const int w = tx[2 + t];
#pragma unroll
        for (int c = 0; c < 3; ++c) hs[c] += w * u[c];
      }
      const int wy = ty[2 + a];
#pragma unroll
      for (int c = 0; c < 3; ++c) acc[c] += wy * hs[c];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int u = min(max((acc[to_rgb ? 2 - c : c] + (1 << 21)) >> 22, 0), 255);
      v[c] = ((float)u - nm.mean[c]) * nm.inv_std[c];
    }
  }
  const long plane = (long)Hout * Wout;
  float* o = out + (long)b * 3 * plane + (long)y * Wout + x;
  o[0] = v[0];
  o[plane] = v[1];
  o[2 * plane] = v[2];
}

// ---- mmseg RandomRotate between the flipped window and the colour stages (rscotr_img_aug_rot_u8 / rscotr_seg_label_rot_u8) ---------
// mmcv.imrotate = cv2.warpAffine(INTER_LINEAR, borderValue=pad_val) of the cropped, flipped uint8 window (cw, ch); the CPU path
// stores that window and warps it, here it is never stored.  An output pixel takes its fixed-point source coordinate in WINDOW
// space from the sample's warp table {adelta[cw], bdelta[cw], X0[ch], Y0[ch]} (rscotr_randaug_u8's layout: AB_SCALE 1024, the
// float64 inverse matrix and round_delta folded in by the host): X = (X0[y] + adelta[x]) >> 5, sx = X >> 5, ax = X & 31, and the
// same in y.  Each of the taps (sy .. sy + 1) x (sx .. sx + 1) that lies inside the window is the uint8 pixel img_aug_kernel
// makes there (resample_u8: un-flipped and resampled from the raw source through the window's entries); a tap outside is the
// pad colour (BGR).  The weights are (32 - ay | ay) * (32 - ax | ax) * 32: exact, they sum to 32768, no table; out =
// (sum w * p + 2^14) >> 15.  A zero-weight tap is not read (ax = ay = 0: the pixel itself).  Then photometric, erasing,
// normalize and pad as in img_aug_kernel.  rot: int32 rows of 4 {warp table offset (0 = the sample is not rotated and takes
// img_aug_kernel's path: bit-equal to rscotr_img_aug_u8), pad B, pad G, pad R}.  Gathers are per lane and rely on L2 (a
// wavefront's lanes walk consecutive output x, so its taps lie along one line of the window); <= 4 x the reads of img_aug_kernel.
constexpr int IMGROT_ROW = 4;

__global__ __launch_bounds__(256) void img_aug_rot_kernel(const uint8_t* __restrict__ src, const int64_t* __restrict__ meta,
                                                          const int32_t* __restrict__ tables,
                                                          const float* __restrict__ params, const int32_t* __restrict__ rot,
                                                          const int32_t* __restrict__ warp, float* __restrict__ out,
                                                          int Hout, int Wout, PrepNorm nm, int to_rgb) {
  const int b = blockIdx.z, y = blockIdx.y;
  const int x = blockIdx.x * 256 + threadIdx.x;
  if (x >= Wout) return;
  const int64_t* m = meta + (long)b * IMGAUG_META;
  const int32_t* r = rot + (long)b * IMGROT_ROW;
  const int cw = (int)m[4], ch = (int)m[5];
  float v[3] = {0.f, 0.f, 0.f};  // mmcv Pad runs after Normalize with pad_val = 0
  if (y < ch && x < cw) {
    int u[3];
    if (r[0] == 0) {
      resample_u8(src, m, tables, x, y, u);
    } else {
      const int32_t* wt = warp + r[0];
      const int X = (wt[2 * cw + y] + wt[x]) >> 5, Y = (wt[2 * cw + ch + y] + wt[cw + x]) >> 5;
      const int sx = X >> 5, sy = Y >> 5, ax = X & 31, ay = Y & 31;
      int acc[3] = {0, 0, 0};
#pragma unroll
      for (int a = 0; a < 2; ++a) {
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          const int w = (a ? ay : 32 - ay) * (t ? ax : 32 - ax) * 32;
          if (w == 0) continue;
          const int px = sx + t, py = sy + a;
          int p[3] = {r[1], r[2], r[3]};
          if (px >= 0 && px < cw && py >= 0 && py < ch) resample_u8(src, m, tables, px, py, p);
#pragma unroll
          for (int c = 0; c < 3; ++c) acc[c] += w * p[c];
        }
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) u[c] = (acc[c] + (1 << 14)) >> 15;  // (weights >= 0 that sum to 2^15: within [0, 255])
    }
    if (m[12]) photometric(u, (int)m[12], (int)m[13], params + (long)b * IMGAUG_PARAMS);
    const int ex = x - (int)m[14], ey = y - (int)m[15];
    if (ex >= 0 && ey >= 0 && ex < (int)m[16] && ey < (int)m[17]) {  // mmcls RandomErasing: patch overwrite
      const uint8_t* p = src + m[18] + ((long)ey * m[16] + ex) * 3;
      u[0] = p[0];
      u[1] = p[1];
      u[2] = p[2];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = ((float)u[to_rgb ? 2 - c : c] - nm.mean[c]) * nm.inv_std[c];
  }
  const long plane = (long)Hout * Wout;
  float* o = out + (long)b * 3 * plane + (long)y * Wout + x;
  o[0] = v[0];
  o[plane] = v[1];
  o[2 * plane] = v[2];
}

// The label companion: the same matrix, cv2 INTER_NEAREST (round_delta 512 folded in, sx = X >> 10).  Inside the window the raw
// label is read through the nearest entries (un-flipped) and reduce_zero_label applies; outside it the value is the rot row's
// seg_pad_val AS GIVEN (mmseg reduces at load time, before RandomRotate fills).  rot: int32 rows of 4 {warp table offset (0 =
// not rotated: seg_label_aug_kernel's path), seg_pad_val, -, -}.  The canvas outside the window is pad_val (Pad's).
__global__ __launch_bounds__(256) void seg_label_rot_kernel(const uint8_t* __restrict__ src,
                                                            const int64_t* __restrict__ meta,
                                                            const int32_t* __restrict__ tables,
                                                            const int32_t* __restrict__ rot,
                                                            const int32_t* __restrict__ warp, int64_t* __restrict__ out,
                                                            int Hout, int Wout, int reduce_zero_label, int pad_val) {
  const int b = blockIdx.z, y = blockIdx.y;
  const int x = blockIdx.x * 256 + threadIdx.x;
  if (x >= Wout) return;
  const int64_t* m = meta + (long)b * IMGAUG_META;
  const int32_t* r = rot + (long)b * IMGROT_ROW;
  const int cw = (int)m[4], ch = (int)m[5];
  int64_t v = pad_val;
  if (y < ch && x < cw) {
    int px = x, py = y;
    if (r[0] != 0) {
      const int32_t* wt = warp + r[0];
      px = (wt[2 * cw + y] + wt[x]) >> 10;
      py = (wt[2 * cw + ch + y] + wt[cw + x]) >> 10;
    }
    if (px >= 0 && px < cw && py >= 0 && py < ch) {
      const int j = (m[6] & 1) ? cw - 1 - px : px, i = (m[6] & 2) ? ch - 1 - py : py;
      const int sx = tables[m[7] + (long)j * (m[9] + 2)], sy = tables[m[8] + (long)i * (m[10] + 2)];
      int l = src[m[0] + (long)sy * m[3] + sx];
      if (reduce_zero_label) {  // mmseg LoadAnnotations: 0 -> 255, l -> l - 1, 254 -> 255
        l = (l == 0) ? 255 : l - 1;
        if (l == 254) l = 255;
      }
      v = l;
    } else {
      v = r[1];
    }
  }
  out[((long)b * Hout + y) * Wout + x] = v;
}

extern "C" int rscotr_img_aug_rot_u8(const uint8_t* src, const int64_t* meta, const int32_t* tables, const float* params,
                                     const int32_t* rot, const int32_t* warp, float* out, int B, int Hout, int Wout,
                                     const float* mean3, const float* std3, int to_rgb, void* stream) {
  if (int e = check_prep("rscotr_img_aug_rot_u8", src, meta, out, B, Hout, Wout)) return e;
  if (B && Hout && Wout && (!tables || !params || !rot || !warp)) return fail(RSCOTR_E_ARG, "rscotr_img_aug_rot_u8: null pointer");
  if (!mean3 || !std3) return fail(RSCOTR_E_ARG, "rscotr_img_aug_rot_u8: mean / std (3 host floats each) required");
  PrepNorm nm;
  for (int c = 0; c < 3; ++c) {
    if (!(std3[c] > 0.f)) return fail(RSCOTR_E_ARG, "rscotr_img_aug_rot_u8: std[%d] must be positive", c);
    nm.mean[c] = mean3[c];
    nm.inv_std[c] = (float)(1.0 / (double)std3[c]);  // as rscotr_img_prep_u8
  }
  if (B == 0 || Hout == 0 || Wout == 0) return RSCOTR_OK;
  img_aug_rot_kernel<<<dim3((Wout + 255) / 256, Hout, B), 256, 0, (hipStream_t)stream>>>(src, meta, tables, params, rot, warp,
                                                                                       out, Hout, Wout, nm, to_rgb ? 1 : 0);
  return check_launch("rscotr_img_aug_rot_u8");
}

extern "C" int rscotr_seg_label_rot_u8(const uint8_t* src, const int64_t* meta, const int32_t* tables, const int32_t* rot,
                                       const int32_t* warp, int64_t* out, int B, int Hout, int Wout, int reduce_zero_label,
                                       int pad_val, void* stream) {
  if (int e = check_prep("rscotr_seg_label_rot_u8", src, meta, out, B, Hout, Wout)) return e;
  if (B && Hout && Wout && (!tables || !rot || !warp)) return fail(RSCOTR_E_ARG, "rscotr_seg_label_rot_u8: null pointer");
  if (B == 0 || Hout == 0 || Wout == 0) return RSCOTR_OK;
  seg_label_rot_kernel<<<dim3((Wout + 255) / 256, Hout, B), 256, 0, (hipStream_t)stream>>>(src, meta, tables, rot, warp, out,
                                                                                         Hout, Wout, reduce_zero_label, pad_val);
  return check_launch("rscotr_seg_label_rot_u8");
}

extern "C" int rscotr_img_aug_u8(const uint8_t* src, const int64_t* meta, const int32_t* tables, const float* params,
                                 float* out, int B, int Hout, int Wout, const float* mean3, const float* std3, int to_rgb,
                                 void* stream) {
  if (int e = check_prep("rscotr_img_aug_u8", src, meta, out, B, Hout, Wout)) return e;
  if (B && Hout && Wout && (!tables || !params)) return fail(RSCOTR_E_ARG, "rscotr_img_aug_u8: null pointer");
  if (!mean3 || !std3) return fail(RSCOTR_E_ARG, "rscotr_img_aug_u8: mean / std (3 host floats each) required");
  PrepNorm nm;
  for (int c = 0; c < 3; ++c) {
    if (!(std3[c] > 0.f)) return fail(RSCOTR_E_ARG, "rscotr_img_aug_u8: std[%d] must be positive", c);
    nm.mean[c] = mean3[c];
    nm.inv_std[c] = (float)(1.0 / (double)std3[c]);  // as rscotr_img_prep_u8
  }
  if (B == 0 || Hout == 0 || Wout == 0) return RSCOTR_OK;
  img_aug_kernel<<<dim3((Wout + 255) / 256, Hout, B), 256, 0, (hipStream_t)stream>>>(src, meta, tables, params, out, Hout,
                                                                                   Wout, nm, to_rgb ? 1 : 0);
  return check_launch("rscotr_img_aug_u8");
}

extern "C" int rscotr_img_aug_chain_u8(const uint8_t* src, const int64_t* meta, const int32_t* tables, float* out, int B,
                                       int Hout, int Wout, const float* mean3, const float* std3, int to_rgb, void* stream) {
  if (int e = check_prep("rscotr_img_aug_chain_u8", src, meta, out, B, Hout, Wout)) return e;
  if (B && Hout && Wout && !tables) return fail(RSCOTR_E_ARG, "rscotr_img_aug_chain_u8: null pointer");
  if (!mean3 || !std3) return fail(RSCOTR_E_ARG, "rscotr_img_aug_chain_u8: mean / std (3 host floats each) required");
  PrepNorm nm;
  for (int c = 0; c < 3; ++c) {
    if (!(std3[c] > 0.f)) return fail(RSCOTR_E_ARG, "rscotr_img_aug_chain_u8: std[%d] must be positive", c);
    nm.mean[c] = mean3[c];
    nm.inv_std[c] = (float)(1.0 / (double)std3[c]);  // as rscotr_img_prep_u8
  }
  if (B == 0 || Hout == 0 || Wout == 0) return RSCOTR_OK;
  img_aug_chain_kernel<<<dim3((Wout + 255) / 256, Hout, B), 256, 0, (hipStream_t)stream>>>(src, meta, tables, out, Hout, Wout,
                                                                                         nm, to_rgb ? 1 : 0);
  return check_launch("rscotr_img_aug_chain_u8");
}

extern "C" int rscotr_seg_label_aug_u8(const uint8_t* src, const int64_t* meta, const int32_t* tables, int64_t* out, int B,
                                       int Hout, int Wout, int reduce_zero_label, int pad_val, void* stream) {
  if (int e = check_prep("rscotr_seg_label_aug_u8", src, meta, out, B, Hout, Wout)) return e;
  if (B && Hout && Wout && !tables) return fail(RSCOTR_E_ARG, "rscotr_seg_label_aug_u8: null pointer");
  if (B == 0 || Hout == 0 || Wout == 0) return RSCOTR_OK;
  seg_label_aug_kernel<<<dim3((Wout + 255) / 256, Hout, B), 256, 0, (hipStream_t)stream>>>(src, meta, tables, out, Hout,
                                                                                         Wout, reduce_zero_label, pad_val);
  return check_launch("rscotr_seg_label_aug_u8");
}

extern "C" int rscotr_img_frames_u8(const uint8_t* src, const int64_t* meta, const int32_t* tables, uint8_t* frames, int B,
                                    int H, int W, void* stream) {
  if (int e = check_prep("rscotr_img_frames_u8", src, meta, frames, B, H, W)) return e;
  if (B && H && W && !tables) return fail(RSCOTR_E_ARG, "rscotr_img_frames_u8: null pointer");
  if (B && H && W && frames == src) return fail(RSCOTR_E_ARG, "rscotr_img_frames_u8: frames must not alias src");
  if (B == 0 || H == 0 || W == 0) return RSCOTR_OK;
  img_frames_kernel<<<dim3((W + 255) / 256, H, B), 256, 0, (hipStream_t)stream>>>(src, meta, tables, frames, H, W);
  return check_launch("rscotr_img_frames_u8");
}
