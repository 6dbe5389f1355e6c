// Fused bilinear-upsample + softmax + set-overlap losses for the seg head (gfx950): mmseg 0.28 DiceLoss and TverskyLoss as
// BaseDecodeHead.losses reaches them.  One set of kernel bodies, templated on the loss (TV: Tversky), instantiated twice.
//
//   u = resize(seg_logit (B,C,h,w), size=label.shape, mode='bilinear', align_corners=False);  p = softmax(u, dim=1)
//   t[b,c,.] = [clamp(label, 0, C-1) == c]     (an ignored 255 lands in channel C-1)       v[b,.] = [label != ignore_index]
// Dice:
//   num[b,c] = 2 * sum_pix p t v + smooth      den[b,c] = sum_pix (p^2 + t) + smooth       (den is NOT masked: mmseg's quirk)
//   loss = loss_weight / C * sum_{c != ignore_index} class_weight[c] * mean_b (1 - num / den)
// Tversky:
//   TP = sum_pix p t v     FP = sum_pix p (1 - t) v     FN = sum_pix (1 - p) t v            (all three masked)
//   num[b,c] = TP + smooth                     den[b,c] = TP + alpha FP + beta FN + smooth
//   loss as above
//
// As in seg_loss.hip, neither the up-sampled logits nor the probabilities exist in memory: a pixel's interpolated logits
// live in registers.  Unlike the cross-entropy, a pixel's gradient depends on sums over its whole image, so:
//   forward   upsample_{dice,tversky}_fwd_kernel   one thread per pixel, a workgroup stays inside one image: log-sum-exp per
//                                        pixel (saved), then the classes once more, DICE_CT at a time in registers, for
//                                        sum p t v, sum p^2 and sum t (Tversky: sum p t v, sum p v and sum t v, from which
//                                        FP = sum p v - TP and FN = sum t v - TP); one partial row per workgroup and class pass
//             upsample_{dice,tversky}_coef_kernel  folds the rows in fixed order, forms num / den, the loss, and the two backward
//                                        coefficients of every (image, class), k = loss_weight * class_weight[c] / (C * B)
//                                        (0 for the skipped channel):
//                                          Dice     a = -2k / den,  bcoef = 2k num / den^2        g_c = a t v + bcoef p_c
//                                          Tversky  a = k (num (1 - alpha - beta) / den^2 - 1 / den),  bcoef = k alpha num / den^2
//                                                                                                  g_c = v (a t + bcoef)
//   backward  upsample_{dice,tversky}_s_kernel     S(pix) = sum_c g_c p_c, one thread per pixel
//             upsample_{dice,tversky}_bwd_kernel   the blocked gather of seg_upsample.h (the cross-entropy's as well) with the
//                                        term p (g_c - S); Dice does NOT skip an ignored pixel (it acts through p^2 in den),
//                                        Tversky does (every sum is masked: it contributes nothing)
// No float atomics, every sum in a fixed order: two runs are bit-equal.  Nothing synchronises with the host.
#include <algorithm>

#include "seg_upsample.h"

namespace rscotr {

constexpr int DICE_CT = 16;       // classes of one register pass of the forward kernel
constexpr int DICE_CHUNKS = 128;  // workgroups per image at most (8 pixels per thread at 512 x 512)

template <bool TV>
__device__ __forceinline__ void upsample_dice_fwd_body(const float* __restrict__ logit, const int64_t* __restrict__ label,
                                                       float* lse, float* __restrict__ part, int C, int h, int w, int H, int W,
                                                       int ignore, int nchunk) {
  const int b = blockIdx.x / nchunk, k = blockIdx.x % nchunk;
  const int HW = H * W, tid = threadIdx.x;
  const float sy = (float)h / (float)H, sx = (float)w / (float)W;
  const float* base = logit + (long)b * C * h * w;
  const int64_t* lab_b = label + (long)b * HW;
  float* lse_b = lse + (long)b * HW;
  const int step = nchunk * 256;
  // every pixel of this workgroup: online log-sum-exp over the classes (as upsample_ce_fwd_kernel)
  for (int i = k * 256 + tid; i < HW; i += step) {
    const Taps taps(i / W, i % W, sy, sx, h, w);
    float m = -3.0e38f, s = 0.f;
    for (int c = 0; c < C; ++c) {
      const float v = taps.at(base + (long)c * h * w);
      if (v > m) { s = s * __expf(m - v) + 1.f; m = v; }
      else s += __expf(v - m);
    }
    lse_b[i] = m + __logf(s);
  }
  // the three per-class sums, DICE_CT classes at a time (each thread re-reads the log-sum-exps it wrote itself)
  __shared__ float red[4][3 * DICE_CT];
  const int lane = tid & 63, wv = tid >> 6;
  for (int c0 = 0; c0 < C; c0 += DICE_CT) {
    float aI[DICE_CT], aP[DICE_CT], aT[DICE_CT];
#pragma unroll
    for (int j = 0; j < DICE_CT; ++j) aI[j] = aP[j] = aT[j] = 0.f;
    for (int i = k * 256 + tid; i < HW; i += step) {
      const Taps taps(i / W, i % W, sy, sx, h, w);
      const long lab = lab_b[i];
      const int lc = (int)std::min<long>(std::max<long>(lab, 0), C - 1);  // the CLAMPED label: never an index
      const float valid = lab != ignore ? 1.f : 0.f;
      const float l = lse_b[i];
#pragma unroll
      for (int j = 0; j < DICE_CT; ++j) {
        const int c = c0 + j;
        if (c < C) {  // (uniform)
          const float p = __expf(taps.at(base + (long)c * h * w) - l);
          if constexpr (TV) {
            aP[j] = fmaf(p, valid, aP[j]);
            if (c == lc) { aI[j] = fmaf(p, valid, aI[j]); aT[j] += valid; }
          } else {
            aP[j] = fmaf(p, p, aP[j]);
            if (c == lc) { aI[j] = fmaf(p, valid, aI[j]); aT[j] += 1.f; }
          }
        }
      }
    }
#pragma unroll
    for (int j = 0; j < DICE_CT; ++j) { aI[j] = wave_sum(aI[j]); aP[j] = wave_sum(aP[j]); aT[j] = wave_sum(aT[j]); }
    __syncthreads();  // (the previous pass's read of red)
    if (lane == 0) {
#pragma unroll
      for (int j = 0; j < DICE_CT; ++j) { red[wv][j] = aI[j]; red[wv][DICE_CT + j] = aP[j]; red[wv][2 * DICE_CT + j] = aT[j]; }
    }
    __syncthreads();
    if (tid < 3 * DICE_CT) {  // partial row [b][k][{p t v, p^2 | p v, t | t v}][C], folded in fixed order by the coef kernel
      const int q = tid / DICE_CT, c = c0 + tid % DICE_CT;
      if (c < C) part[(((long)b * nchunk + k) * 3 + q) * C + c] = red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
    }
  }
}

__global__ __launch_bounds__(256) void upsample_dice_fwd_kernel(const float* __restrict__ logit,
                                                                const int64_t* __restrict__ label, float* lse,
                                                                float* __restrict__ part, int C, int h, int w, int H, int W,
                                                                int ignore, int nchunk) {
  upsample_dice_fwd_body<false>(logit, label, lse, part, C, h, w, H, W, ignore, nchunk);
}

__global__ __launch_bounds__(256) void upsample_tversky_fwd_kernel(const float* __restrict__ logit,
                                                                   const int64_t* __restrict__ label, float* lse,
                                                                   float* __restrict__ part, int C, int h, int w, int H, int W,
                                                                   int ignore, int nchunk) {
  upsample_dice_fwd_body<true>(logit, label, lse, part, C, h, w, H, W, ignore, nchunk);
}

// one workgroup: fold, num / den, the backward coefficients (without the upstream gradient) and the loss
template <bool TV>
__device__ __forceinline__ void upsample_dice_coef_body(const float* __restrict__ part, const float* __restrict__ cw,
                                                        float* __restrict__ coef, float* __restrict__ loss, int B, int C,
                                                        int nchunk, int ignore, float smooth, float loss_weight, float alpha,
                                                        float beta) {
  double acc = 0.0;
  for (int i = threadIdx.x; i < B * C; i += 256) {
    const int b = i / C, c = i % C;
    float s[3] = {0.f, 0.f, 0.f};
    for (int k = 0; k < nchunk; ++k)
#pragma unroll
      for (int q = 0; q < 3; ++q) s[q] += part[(((long)b * nchunk + k) * 3 + q) * C + c];
    const double kk = c == ignore ? 0.0 : (double)(cw ? cw[c] : 1.f) * (double)loss_weight / ((double)C * (double)B);
    if constexpr (TV) {
      const double tp = (double)s[0], fp = (double)s[1] - tp, fn = (double)s[2] - tp;
      const double num = tp + (double)smooth, den = tp + (double)alpha * fp + (double)beta * fn + (double)smooth;
      coef[2 * i] = (float)(kk * (num * (1.0 - (double)alpha - (double)beta) / (den * den) - 1.0 / den));
      coef[2 * i + 1] = (float)(kk * (double)alpha * num / (den * den));
      acc += kk * ((den - num) / den);
    } else {
      const double num = 2.0 * (double)s[0] + (double)smooth, den = (double)s[1] + (double)s[2] + (double)smooth;
      coef[2 * i] = (float)(-2.0 * kk / den);
      coef[2 * i + 1] = (float)(2.0 * kk * num / (den * den));
      acc += kk * ((den - num) / den);
    }
  }
  __shared__ double red[256];
  red[threadIdx.x] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int i = 0; i < 256; ++i) t += red[i];
    loss[0] = (float)t;
  }
}

__global__ __launch_bounds__(256) void upsample_dice_coef_kernel(const float* __restrict__ part, const float* __restrict__ cw,
                                                                 float* __restrict__ coef, float* __restrict__ loss, int B, int C,
                                                                 int nchunk, int ignore, float smooth, float loss_weight) {
  upsample_dice_coef_body<false>(part, cw, coef, loss, B, C, nchunk, ignore, smooth, loss_weight, 0.f, 0.f);
}

__global__ __launch_bounds__(256) void upsample_tversky_coef_kernel(const float* __restrict__ part, const float* __restrict__ cw,
                                                                    float* __restrict__ coef, float* __restrict__ loss, int B,
                                                                    int C, int nchunk, int ignore, float smooth, float loss_weight,
                                                                    float alpha, float beta) {
  upsample_dice_coef_body<true>(part, cw, coef, loss, B, C, nchunk, ignore, smooth, loss_weight, alpha, beta);
}

// S(pix) = sum_c g_c p_c: one thread per pixel, the classes streamed once more
//   Dice     a[b, label] v p_label + sum_c bcoef[b, c] p_c^2
//   Tversky  v (a[b, label] p_label + sum_c bcoef[b, c] p_c)
template <bool TV>
__device__ __forceinline__ void upsample_dice_s_body(const float* __restrict__ logit, const int64_t* __restrict__ label,
                                                     const float* __restrict__ lse, const float* __restrict__ coef,
                                                     float* __restrict__ pix_s, int B, int C, int h, int w, int H, int W,
                                                     int ignore) {
  const long npix = (long)B * H * W;
  const float sy = (float)h / (float)H, sx = (float)w / (float)W;
  for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < npix; p += (long)gridDim.x * 256) {
    const long lab = label[p];
    if (TV && lab == ignore) {  // (the gather skips this pixel)
      pix_s[p] = 0.f;
      continue;
    }
    const int x = (int)(p % W), y = (int)((p / W) % H), b = (int)(p / ((long)W * H));
    const Taps taps(y, x, sy, sx, h, w);
    const float* base = logit + (long)b * C * h * w;
    const float2* cf = reinterpret_cast<const float2*>(coef) + (long)b * C;
    const int lc = (int)std::min<long>(std::max<long>(lab, 0), C - 1);
    const float valid = lab != ignore ? 1.f : 0.f;
    const float l = lse[p];
    float s = 0.f;
    for (int c = 0; c < C; ++c) {
      const float q = __expf(taps.at(base + (long)c * h * w) - l);
      const float2 ab = cf[c];
      if constexpr (TV) s = fmaf((c == lc ? ab.x : 0.f) + ab.y, q, s);
      else s = fmaf(fmaf(ab.y, q, c == lc ? ab.x * valid : 0.f), q, s);
    }
    pix_s[p] = s;
  }
}

__global__ __launch_bounds__(256) void upsample_dice_s_kernel(const float* __restrict__ logit, const int64_t* __restrict__ label,
                                                              const float* __restrict__ lse, const float* __restrict__ coef,
                                                              float* __restrict__ pix_s, int B, int C, int h, int w, int H, int W,
                                                              int ignore) {
  upsample_dice_s_body<false>(logit, label, lse, coef, pix_s, B, C, h, w, H, W, ignore);
}

__global__ __launch_bounds__(256) void upsample_tversky_s_kernel(const float* __restrict__ logit, const int64_t* __restrict__ label,
                                                                 const float* __restrict__ lse, const float* __restrict__ coef,
                                                                 float* __restrict__ pix_s, int B, int C, int h, int w, int H,
                                                                 int W, int ignore) {
  upsample_dice_s_body<true>(logit, label, lse, coef, pix_s, B, C, h, w, H, W, ignore);
}

// dlogit[b,c,cy,cx] = scale * sum over output pixels p touching the cell of  wt(p->cell) * p_c (g_c - S(p)): the blocked gather
// of seg_upsample.h.  A lane holds its class's two coefficients in registers, a pixel is staged with its clamped label (-1 where
// ignored: no class) and S as the gather's plane.  Dice skips no pixel (g_c = a t v + bcoef p_c); Tversky skips the ignored ones
// (g_c = v (a t + bcoef)).
template <bool TV>
struct DiceTerm {
  static constexpr bool PLANE = true;
  static constexpr bool RAW = false;
  const int64_t* __restrict__ label;
  const float* __restrict__ coef;
  const float* __restrict__ pix_s;
  int C, ignore;
  float ca, cb;  // this lane's class: a and bcoef of (b, c)
  __device__ __forceinline__ void load_class(int b, int c) {
    ca = 0.f; cb = 0.f;
    if (c < C) { ca = coef[((long)b * C + c) * 2]; cb = coef[((long)b * C + c) * 2 + 1]; }
  }
  __device__ __forceinline__ int stage(long p, float& plane) const {
    const long lab = label[p];
    plane = pix_s[p];
    return lab != ignore ? (int)std::min<long>(std::max<long>(lab, 0), C - 1) : -1;
  }
  __device__ __forceinline__ bool skip(int lab) const { return TV && lab < 0; }
  __device__ __forceinline__ float term(float prob, int c, int lab, float plane) const {
    if constexpr (TV) return prob * ((c == lab ? ca : 0.f) + cb - plane);
    else return prob * (fmaf(cb, prob, c == lab ? ca : 0.f) - plane);
  }
};

__global__ __launch_bounds__(512) void upsample_dice_bwd_kernel(const float* __restrict__ logit, const int64_t* __restrict__ label,
                                                                const float* __restrict__ lse, const float* __restrict__ coef,
                                                                const float* __restrict__ pix_s, const float* __restrict__ gscale,
                                                                float* __restrict__ dlogit, int B, int C, int h, int w, int H,
                                                                int W, int ignore) {
  upsample_gather(DiceTerm<false>{label, coef, pix_s, C, ignore, 0.f, 0.f}, logit, lse, gscale, dlogit, C, h, w, H, W);
}

__global__ __launch_bounds__(512) void upsample_tversky_bwd_kernel(const float* __restrict__ logit,
                                                                   const int64_t* __restrict__ label, const float* __restrict__ lse,
                                                                   const float* __restrict__ coef, const float* __restrict__ pix_s,
                                                                   const float* __restrict__ gscale, float* __restrict__ dlogit,
                                                                   int B, int C, int h, int w, int H, int W, int ignore) {
  upsample_gather(DiceTerm<true>{label, coef, pix_s, C, ignore, 0.f, 0.f}, logit, lse, gscale, dlogit, C, h, w, H, W);
}

static int dice_chunks(int H, int W) { return (int)std::min<long>(((long)H * W + 255) / 256, DICE_CHUNKS); }

// the forward partial rows: [B][chunks <= DICE_CHUNKS][3][C] floats
static int64_t dice_workspace(int B, int C) { return (int64_t)std::max(B, 0) * DICE_CHUNKS * 3 * std::max(C, 0) * 4; }

// Host side of the two forward entries (alpha / beta: Tversky only)
template <bool TV>
static int dice_fwd(const char* entry, const float* logit, const int64_t* label, const float* class_weight, float* lse,
                    float* coef, float* loss, int B, int C, int h, int w, int H, int W, int ignore_index, float smooth,
                    float loss_weight, float alpha, float beta, float* workspace, int64_t workspace_bytes, void* stream) {
  if (int e = upsample_check_shape(entry, B, C, h, w, H, W)) return e;
  if ((long)H * W > (1L << 24))  // the label counts are float sums: exact below 2^24
    return fail(RSCOTR_E_SHAPE, "%s: more than 2^24 pixels per image", entry);
  if ((long)B * C > 0x3fffffffL || (long)C * h * w > 0x7fffffffL) return fail(RSCOTR_E_SHAPE, "%s: shape too large", entry);
  if (!loss) return fail(RSCOTR_E_ARG, "%s: null pointer", entry);
  hipStream_t s = (hipStream_t)stream;
  if (B == 0) {
    (void)hipMemsetAsync(loss, 0, sizeof(float), s);
    return RSCOTR_OK;
  }
  if (!logit || !label || !lse || !coef) return fail(RSCOTR_E_ARG, "%s: null pointer", entry);
  if (!workspace || workspace_bytes < dice_workspace(B, C))
    return fail(RSCOTR_E_ARG, "%s: workspace of rscotr_upsample_%s_workspace(B, C) bytes required", entry, TV ? "tversky" : "dice");
  const int nchunk = dice_chunks(H, W);
  if ((long)B * nchunk > 0x7fffffffL) return fail(RSCOTR_E_SHAPE, "%s: batch too large", entry);
  if constexpr (TV) {
    upsample_tversky_fwd_kernel<<<B * nchunk, 256, 0, s>>>(logit, label, lse, workspace, C, h, w, H, W, ignore_index, nchunk);
    upsample_tversky_coef_kernel<<<1, 256, 0, s>>>(workspace, class_weight, coef, loss, B, C, nchunk, ignore_index, smooth,
                                                   loss_weight, alpha, beta);
  } else {
    upsample_dice_fwd_kernel<<<B * nchunk, 256, 0, s>>>(logit, label, lse, workspace, C, h, w, H, W, ignore_index, nchunk);
    upsample_dice_coef_kernel<<<1, 256, 0, s>>>(workspace, class_weight, coef, loss, B, C, nchunk, ignore_index, smooth,
                                                loss_weight);
  }
  return check_launch(entry);
}

template <bool TV>
static int dice_bwd(const char* entry, const float* logit, const int64_t* label, const float* lse, const float* coef,
                    const float* grad_scale, float* pix_s, float* dlogit, int B, int C, int h, int w, int H, int W,
                    int ignore_index, void* stream) {
  if (int e = upsample_check_shape(entry, B, C, h, w, H, W)) return e;
  if (B == 0) return RSCOTR_OK;
  if (!logit || !label || !lse || !coef || !grad_scale || !pix_s || !dlogit) return fail(RSCOTR_E_ARG, "%s: null pointer", entry);
  hipStream_t s = (hipStream_t)stream;
  const long npix = (long)B * H * W;
  const int nwg = (int)std::min<long>((npix + 255) / 256, 4096);
  if constexpr (TV) {
    upsample_tversky_s_kernel<<<nwg, 256, 0, s>>>(logit, label, lse, coef, pix_s, B, C, h, w, H, W, ignore_index);
    launch_upsample_gather<upsample_tversky_bwd_kernel, true>(s, B, h, w, logit, label, lse, coef, pix_s, grad_scale, dlogit, B, C,
                                                              h, w, H, W, ignore_index);
  } else {
    upsample_dice_s_kernel<<<nwg, 256, 0, s>>>(logit, label, lse, coef, pix_s, B, C, h, w, H, W, ignore_index);
    launch_upsample_gather<upsample_dice_bwd_kernel, true>(s, B, h, w, logit, label, lse, coef, pix_s, grad_scale, dlogit, B, C, h,
                                                           w, H, W, ignore_index);
  }
  return check_launch(entry);
}

}  // namespace rscotr

using namespace rscotr;

extern "C" int64_t rscotr_upsample_dice_workspace(int B, int C) { return dice_workspace(B, C); }

extern "C" int rscotr_upsample_dice_fwd(const float* logit, const int64_t* label, const float* class_weight, float* lse,
                                        float* coef, float* loss, int B, int C, int h, int w, int H, int W, int ignore_index,
                                        float smooth, float loss_weight, float* workspace, int64_t workspace_bytes,
                                        void* stream) {
  return dice_fwd<false>("rscotr_upsample_dice_fwd", logit, label, class_weight, lse, coef, loss, B, C, h, w, H, W, ignore_index,
                         smooth, loss_weight, 0.f, 0.f, workspace, workspace_bytes, stream);
}

// dlogit (B,C,h,w) = grad_scale[0] * d(loss)/d(logit); grad_scale is a DEVICE scalar (the upstream gradient); pix_s (B,H,W) is
// the caller's scratch plane for S
extern "C" int rscotr_upsample_dice_bwd(const float* logit, const int64_t* label, const float* lse, const float* coef,
                                        const float* grad_scale, float* pix_s, float* dlogit, int B, int C, int h, int w,
                                        int H, int W, int ignore_index, void* stream) {
  return dice_bwd<false>("rscotr_upsample_dice_bwd", logit, label, lse, coef, grad_scale, pix_s, dlogit, B, C, h, w, H, W,
                         ignore_index, stream);
}

// ---- Tversky: the same buffers and launches (additive entries; the three above are untouched) -----------------------------------
extern "C" int64_t rscotr_upsample_tversky_workspace(int B, int C) { return dice_workspace(B, C); }

extern "C" int rscotr_upsample_tversky_fwd(const float* logit, const int64_t* label, const float* class_weight, float* lse,
                                           float* coef, float* loss, int B, int C, int h, int w, int H, int W, int ignore_index,
                                           float alpha, float beta, float smooth, float loss_weight, float* workspace,
                                           int64_t workspace_bytes, void* stream) {
  if (!(smooth > 0.f)) return fail(RSCOTR_E_ARG, "rscotr_upsample_tversky_fwd: smooth > 0 required");
  return dice_fwd<true>("rscotr_upsample_tversky_fwd", logit, label, class_weight, lse, coef, loss, B, C, h, w, H, W, ignore_index,
                        smooth, loss_weight, alpha, beta, workspace, workspace_bytes, stream);
}

extern "C" int rscotr_upsample_tversky_bwd(const float* logit, const int64_t* label, const float* lse, const float* coef,
                                           const float* grad_scale, float* pix_s, float* dlogit, int B, int C, int h, int w,
                                           int H, int W, int ignore_index, void* stream) {
  return dice_bwd<true>("rscotr_upsample_tversky_bwd", logit, label, lse, coef, grad_scale, pix_s, dlogit, B, C, h, w, H, W,
                        ignore_index, stream);
}
