// RandAugment on the device for gfx950 (rscotr_randaug_u8): ONE SLOT of mmcls RandAugment over a batch of uint8 HWC BGR
// frames, every sample applying its own operation (or none) from a ping frame to a pong frame.
//
// Replaces, per sample on a CPU worker, mmcls RandAugment(policies=rand_increasing_policies, num_policies=2, ...) of
// configs/_base_/cls/resisc_swin_224.py:15-27 with the policies of configs/_base_/cls/rand_aug.py:2-42, i.e. the mmcv
// functions auto_contrast, imequalize, iminvert, posterize, solarize, adjust_color, adjust_contrast, adjust_brightness,
// adjust_sharpness, imrotate, imshear, imtranslate (cv2.warpAffine / filter2D / addWeighted / cvtColor underneath).
//
// Two launches per slot, chosen over one-workgroup-per-image-in-LDS because the batch is small (16 frames would occupy 16
// of 256 CUs) while the frames are 150 KB each (a 256-thread workgroup per 4096 pixels gives 13 x B workgroups per launch):
//   stats   per sample whose operation needs it (AutoContrast, Equalize, Contrast): 3 x 256 channel histograms in LDS
//           (integer LDS atomics), merged into the sample's global table with integer atomics, and the sum of the cv2
//           grey value as a 64-bit integer.  Integer sums are order-independent: the step is bit-reproducible.  The table
//           is zeroed by a memset node in front of the launch.  Skipped when the host says no sample needs it.
//   apply   grid (tile of 4096 pixels, sample); the operation code and parameters come from the sample's meta row.  Point
//           operations go through a 3 x 256 byte LUT the workgroup builds in LDS: from the histogram (256-bin prefix sum
//           for Equalize, min / max for AutoContrast) or from the parameters.  ColorTransform / Contrast blend with the grey
//           value / grey mean, Sharpness reads 3 x 3 with reflect-101 borders, the warps gather through the inverse
//           affine map in OpenCV's fixed point: the per-sample coordinate tables and the 1024 x 16 int16 bicubic weight
//           table are built by the host, so the device arithmetic is integer.  Float steps are float32, unfused.
// Every read of a frame is bounds-checked here against the sample's (w, h); the table offsets are the caller's.
#include "common.h"

// every float / double step below restates a fixed sequence of rounded operations (cv2 / NumPy): no fused multiply-add
#pragma clang fp contract(off)

namespace rscotr {

enum {
  RA_NONE = 0, RA_AUTOCONTRAST = 1, RA_EQUALIZE = 2, RA_INVERT = 3, RA_POSTERIZE = 4, RA_SOLARIZE = 5, RA_SOLARIZE_ADD = 6,
  RA_COLOR = 7, RA_CONTRAST = 8, RA_BRIGHTNESS = 9, RA_SHARPNESS = 10, RA_ROTATE = 11, RA_SHEAR = 12, RA_TRANSLATE = 13
};
// int32 per sample: op, w, h, integer parameter, float a (bits), float b (bits), warp table offset (int32 elements),
// warp interpolation (0 nearest, 1 bicubic), pad B, pad G, pad R, reserved x 5
constexpr int RA_META = 16;
constexpr int RA_STATS = 770;  // uint32 per sample: 3 x 256 histogram bins, then the grey sum (uint64, two words)
constexpr int RA_TILE = 4096;  // pixels per workgroup

__device__ __forceinline__ int grey_u8(int b, int g, int r) {  // cv2 BGR2GRAY, uint8
  return (b * 3735 + g * 19235 + r * 9798 + (1 << 14)) >> 15;
}

__device__ __forceinline__ int trunc_u8(float f) {  // np.clip(f, 0, 255).astype(uint8)
  return (int)fminf(fmaxf(f, 0.f), 255.f);
}

__device__ __forceinline__ int round_u8(float f) {  // saturate_cast<uchar>(float): round half to even, clamp
  const int i = __float2int_rn(f);
  return i < 0 ? 0 : (i > 255 ? 255 : i);
}

__device__ __forceinline__ float blend(float p, float a, float q, float b) {  // p * a + q * b, two products and a sum
  return p * a + q * b;  // (unfused: the pragma above; the __f*_rn wrappers of the HIP headers may be contracted)
}

__device__ __forceinline__ int reflect101(int i, int n) {  // cv2 BORDER_REFLECT_101 for i in [-1, n]
  if (n == 1) return 0;
  return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i);
}

__device__ __forceinline__ bool needs_stats(int op) {
  return op == RA_AUTOCONTRAST || op == RA_EQUALIZE || op == RA_CONTRAST;
}

__global__ __launch_bounds__(256) void randaug_stats_kernel(const uint8_t* __restrict__ in, const int32_t* __restrict__ meta,
                                                            uint32_t* __restrict__ stats, int H, int W) {
  const int b = blockIdx.y, tid = threadIdx.x;
  const int32_t* m = meta + (long)b * RA_META;
  if (!needs_stats(m[0])) return;
  const int w = m[1], h = m[2], n = w * h;
  const int p0 = blockIdx.x * RA_TILE;
  if (p0 >= n) return;
  __shared__ uint32_t hist[768];
  __shared__ unsigned long long gsum;
  for (int i = tid; i < 768; i += 256) hist[i] = 0u;
  if (tid == 0) gsum = 0ull;
  __syncthreads();
  const uint8_t* f = in + (long)b * H * W * 3;
  const int p1 = min(n, p0 + RA_TILE);
  uint32_t g = 0u;
  for (int p = p0 + tid; p < p1; p += 256) {
    const int y = p / w, x = p - y * w;
    const uint8_t* px = f + ((long)y * W + x) * 3;
    const int c0 = px[0], c1 = px[1], c2 = px[2];
    atomicAdd(&hist[c0], 1u);
    atomicAdd(&hist[256 + c1], 1u);
    atomicAdd(&hist[512 + c2], 1u);
    g += (uint32_t)grey_u8(c0, c1, c2);
  }
  atomicAdd(&gsum, (unsigned long long)g);
  __syncthreads();
  uint32_t* st = stats + (long)b * RA_STATS;
  for (int i = tid; i < 768; i += 256)
    if (hist[i]) atomicAdd(st + i, hist[i]);
  if (tid == 0) atomicAdd(reinterpret_cast<unsigned long long*>(st + 768), gsum);
}

// lowest / highest non-empty bin of one channel's histogram (256 threads, thread i = bin i)
__device__ __forceinline__ void bin_range(const uint32_t* hc, int tid, int* lohi, int& lo, int& hi) {
  __syncthreads();
  if (tid == 0) {
    lohi[0] = 256;
    lohi[1] = -1;
  }
  __syncthreads();
  if (hc[tid]) {
    atomicMin(&lohi[0], tid);
    atomicMax(&lohi[1], tid);
  }
  __syncthreads();
  lo = lohi[0];
  hi = lohi[1];
}

__global__ __launch_bounds__(256) void randaug_apply_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out,
                                                            const int32_t* __restrict__ meta,
                                                            const int32_t* __restrict__ warp,
                                                            const int16_t* __restrict__ wtab,
                                                            const uint32_t* __restrict__ stats, int H, int W) {
  const int b = blockIdx.y, tid = threadIdx.x;
  const int32_t* m = meta + (long)b * RA_META;
  const int op = (needs_stats(m[0]) && !stats) ? RA_NONE : m[0];  // (no table: the entry was told no sample needs one)
  const int w = m[1], h = m[2], n = w * h;
  const int p0 = blockIdx.x * RA_TILE;
  if (p0 >= n) return;
  const int ip = m[3];
  const float fa = __int_as_float(m[4]), fb = __int_as_float(m[5]);
  __shared__ uint8_t lut[768];
  __shared__ uint32_t scan[256];
  __shared__ int lohi[2];
  const bool lut_op = (op >= RA_AUTOCONTRAST && op <= RA_SOLARIZE_ADD) || op == RA_BRIGHTNESS;
  float mean = 0.f;
  if (op == RA_AUTOCONTRAST) {  // mmcv auto_contrast, cutoff 0: lut = clip(i * s - lo * s, 0, 255) in float64, truncated
    for (int c = 0; c < 3; ++c) {
      int lo, hi;
      bin_range(stats + (long)b * RA_STATS + c * 256, tid, lohi, lo, hi);
      int v = tid;
      if (hi > lo) {
        const double s = 255.0 / (double)(hi - lo);
        double t = (double)tid * s + -((double)lo * s);
        t = t < 0.0 ? 0.0 : (t > 255.0 ? 255.0 : t);
        v = (int)t;
      }
      lut[c * 256 + tid] = (uint8_t)v;
    }
  } else if (op == RA_EQUALIZE) {  // mmcv imequalize: step = (n - last non-empty bin) / 255, lut = (exclusive cumsum + step / 2) / step
    for (int c = 0; c < 3; ++c) {
      const uint32_t* hc = stats + (long)b * RA_STATS + c * 256;
      int lo, hi;
      bin_range(hc, tid, lohi, lo, hi);
      const uint32_t mine = hc[tid];
      scan[tid] = mine;
      __syncthreads();
      for (int d = 1; d < 256; d <<= 1) {
        const uint32_t t = tid >= d ? scan[tid - d] : 0u;
        __syncthreads();
        scan[tid] += t;
        __syncthreads();
      }
      const uint32_t total = scan[255], step = (total - (hi < 0 ? 0u : hc[hi])) / 255u;
      int v = tid;
      if (step) v = (int)min((scan[tid] - mine + step / 2u) / step, 255u);
      lut[c * 256 + tid] = (uint8_t)v;
      __syncthreads();
    }
  } else if (lut_op) {
    int v = tid;
    if (op == RA_INVERT) v = 255 - tid;
    else if (op == RA_POSTERIZE) v = ip >= 8 ? 0 : (tid >> ip) << ip;          // ip = 8 - bits
    else if (op == RA_SOLARIZE) v = tid < ip ? tid : 255 - tid;               // ip = ceil(thr)
    else if (op == RA_SOLARIZE_ADD) v = tid < 128 ? min(tid + ip, 255) : tid;  // ip = floor(magnitude)
    else v = trunc_u8((float)tid * fa);                              // Brightness
    lut[tid] = lut[256 + tid] = lut[512 + tid] = (uint8_t)v;
  } else if (op == RA_CONTRAST) {  // mean = round(sum(grey) / n), Python round of the float64 quotient
    const unsigned long long gs = *reinterpret_cast<const unsigned long long*>(stats + (long)b * RA_STATS + 768);
    mean = (float)rint((double)gs / (double)n);
  }
  __syncthreads();
  const uint8_t* fin = in + (long)b * H * W * 3;
  uint8_t* fout = out + (long)b * H * W * 3;
  const int pad[3] = {m[8], m[9], m[10]};
  const float k1 = (float)(1.0 / 13.0), k5 = (float)(5.0 / 13.0);
  const int p1 = min(n, p0 + RA_TILE);
  for (int p = p0 + tid; p < p1; p += 256) {
    const int y = p / w, x = p - y * w;
    const uint8_t* px = fin + ((long)y * W + x) * 3;
    int u[3] = {px[0], px[1], px[2]};
    if (lut_op) {
#pragma unroll
      for (int c = 0; c < 3; ++c) u[c] = lut[c * 256 + u[c]];
    } else if (op == RA_COLOR) {  // cv2.addWeighted(img, a, grey, b, 0) on uint8: float32, rounded, saturated
      const float g = (float)grey_u8(u[0], u[1], u[2]);
#pragma unroll
      for (int c = 0; c < 3; ++c) u[c] = round_u8(blend((float)u[c], fa, g, fb));
    } else if (op == RA_CONTRAST) {
#pragma unroll
      for (int c = 0; c < 3; ++c) u[c] = trunc_u8(blend((float)u[c], fa, mean, fb));
    } else if (op == RA_SHARPNESS) {  // filter2D([[1,1,1],[1,5,1],[1,1,1]] / 13), float32 taps in row-major order
      float acc[3] = {0.f, 0.f, 0.f};
      for (int dy = -1; dy <= 1; ++dy) {
        const uint8_t* row = fin + (long)reflect101(y + dy, h) * W * 3;
        for (int dx = -1; dx <= 1; ++dx) {
          const uint8_t* q = row + reflect101(x + dx, w) * 3;
          const float k = (dy == 0 && dx == 0) ? k5 : k1;
#pragma unroll
          for (int c = 0; c < 3; ++c) acc[c] = acc[c] + k * (float)q[c];
        }
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) u[c] = trunc_u8(blend((float)u[c], fa, (float)round_u8(acc[c]), fb));
    } else if (op >= RA_ROTATE) {  // cv2.warpAffine, fixed point; the tables hold adelta | bdelta | X0 | Y0 (round_delta added)
      const int32_t* wt = warp + m[6];
      const int X = wt[2 * w + y] + wt[x], Y = wt[2 * w + h + y] + wt[w + x];
      if (m[7] == 0) {
        const int sx = X >> 10, sy = Y >> 10;
        const bool inb = (unsigned)sx < (unsigned)w && (unsigned)sy < (unsigned)h;
        const uint8_t* q = fin + ((long)(inb ? sy : 0) * W + (inb ? sx : 0)) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) u[c] = inb ? q[c] : pad[c];
      } else {
        const int X5 = X >> 5, Y5 = Y >> 5;
        const int sx = X5 >> 5, sy = Y5 >> 5;
        const int16_t* wv = wtab + ((Y5 & 31) * 32 + (X5 & 31)) * 16;
        int acc[3] = {0, 0, 0};
        for (int a = 0; a < 4; ++a) {
          const int yy = sy - 1 + a;
          const bool yin = (unsigned)yy < (unsigned)h;
          for (int t = 0; t < 4; ++t) {
            const int xx = sx - 1 + t;
            const bool inb = yin && (unsigned)xx < (unsigned)w;
            const uint8_t* q = fin + ((long)(inb ? yy : 0) * W + (inb ? xx : 0)) * 3;
            const int wgt = wv[a * 4 + t];
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[c] += wgt * (inb ? (int)q[c] : pad[c]);
          }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) u[c] = min(max((acc[c] + (1 << 14)) >> 15, 0), 255);
      }
    }
    uint8_t* o = fout + ((long)y * W + x) * 3;
    o[0] = (uint8_t)u[0];
    o[1] = (uint8_t)u[1];
    o[2] = (uint8_t)u[2];
  }
}

}  // namespace rscotr

using namespace rscotr;

extern "C" int rscotr_randaug_u8(const uint8_t* in, uint8_t* out, const int32_t* meta, const int32_t* warp,
                                 const int16_t* wtab, uint32_t* stats, int need_stats, int B, int H, int W, void* stream) {
  const char* fn = "rscotr_randaug_u8";
  if (B < 0 || H < 0 || W < 0) return fail(RSCOTR_E_SHAPE, "%s: negative dimension", fn);
  if (B > 65535) return fail(RSCOTR_E_SHAPE, "%s: B must be <= 65535", fn);
  if ((long)H * W > (1L << 30)) return fail(RSCOTR_E_SHAPE, "%s: H * W must be <= 2^30", fn);
  if (B == 0 || H == 0 || W == 0) return RSCOTR_OK;
  if (!in || !out || !meta || !warp || !wtab) return fail(RSCOTR_E_ARG, "%s: null pointer", fn);
  if (in == out) return fail(RSCOTR_E_ARG, "%s: in and out must be different frames (warps and Sharpness read neighbours)", fn);
  if (need_stats && !stats) return fail(RSCOTR_E_ARG, "%s: need_stats without a stats table (B x 770 uint32)", fn);
  if (need_stats && (reinterpret_cast<uintptr_t>(stats) & 7u)) return fail(RSCOTR_E_ALIGN, "%s: stats must be 8-byte aligned", fn);
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)(((long)H * W + RA_TILE - 1) / RA_TILE), B);
  if (need_stats) {
    if (hipMemsetAsync(stats, 0, (size_t)B * RA_STATS * sizeof(uint32_t), s) != hipSuccess)
      return fail(RSCOTR_E_LAUNCH, "%s: hipMemsetAsync failed", fn);
    randaug_stats_kernel<<<grid, 256, 0, s>>>(in, meta, stats, H, W);
    if (int e = check_launch(fn)) return e;
  }
  randaug_apply_kernel<<<grid, 256, 0, s>>>(in, out, meta, warp, wtab, stats, H, W);
  return check_launch(fn);
}
