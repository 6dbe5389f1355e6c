// Detection loss arithmetic of the DINO head as three kernels (each replaces a few dozen element-wise launches):
//   match_cost_kernel   mmdet FocalLossCost + BBoxL1Cost(xywh) + IoUCost(giou | iou) of HungarianAssigner.assign
//                       (cfg ...potsdam.py:169-174; reached from models/multi/bbox_head/mmdet_detr_head/detr_head.py:513-515)
//   focal_sum_kernel    mmcv sigmoid_focal_loss summed per prediction set (detr_head.py:384-385, dino_head.py:272-273)
//   qfl_sum_kernel      mmdet QualityFocalLoss in its place (loss_cls=dict(type='QualityFocalLoss'))
//   box_loss_kernel     L1 (cxcywh, normalised) and GIoU | IoU | DIoU | CIoU (xyxy, pixels) sums per set (detr_head.py:392-415)
// The two loss kernels also write the gradient of their sums with respect to the predictions (the upstream
// gradient of a set's sum is one scalar, applied afterwards), so backward needs no second pass over the formulas.
// One workgroup per prediction set and a fixed reduction order: deterministic sums.
#include "common.h"

namespace rscotr {

__device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + expf(-x)); }
__device__ __forceinline__ float powg(float x, float gamma) { return gamma == 2.f ? x * x : powf(x, gamma); }

// deterministic block sum (256 threads): returns the total in every thread
__device__ __forceinline__ float block_sum256(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// the IoU measures of mmdet's box losses / match costs; IoULoss's `mode`
enum { KIND_GIOU = 0, KIND_IOU = 1, KIND_DIOU = 2, KIND_CIOU = 3, KIND_COUNT = 4 };
enum { IOU_LINEAR = 0, IOU_SQUARE = 1, IOU_LOG = 2 };

struct BoxIou {
  float v;     // the measure: a loss is 1 - v (IoULoss: its mode applied to v)
  float d[4];  // d v / d (x1, y1, x2, y2) of the first box
};

// The IoU measure KIND of p against t (both xyxy); optionally its gradient with respect to p.  The 1-D max / min and the
// clamps take strict comparisons: a tie gives p no gradient.
//   GIOU  ov / u - (ea - u) / ea, u and ea clamped at eps as mmdet bbox_overlaps
//   IOU   ov / max(u, eps)                                          (bbox_overlaps mode 'iou'; IoULoss, IoUCost, QFL's score)
//   DIOU  ov / (u + eps) - rho2 / c2, c2 = ew^2 + eh^2 + eps, rho2 = squared centre distance            (mmdet diou_loss)
//   CIOU  clamp(DIOU - alpha v, -1, 1), v = 4 / pi^2 (atan(w2 / h2) - atan(w1 / h1))^2 with h + eps,
//         alpha = [iou > 0.5] v / (1 - iou + v) held constant                                           (mmdet ciou_loss)
template <int KIND, bool GRAD>
__device__ __forceinline__ BoxIou box_iou(const float* p, const float* t, float eps) {
  BoxIou r;
  const float pw = p[2] - p[0], ph = p[3] - p[1];
  const float a1 = pw * ph, a2 = (t[2] - t[0]) * (t[3] - t[1]);
  const float ix1 = fmaxf(p[0], t[0]), iy1 = fmaxf(p[1], t[1]), ix2 = fminf(p[2], t[2]), iy2 = fminf(p[3], t[3]);
  const float iw = fmaxf(ix2 - ix1, 0.f), ih = fmaxf(iy2 - iy1, 0.f);
  const float ov = iw * ih;
  const float uraw = a1 + a2 - ov;
  // d(ov), d(a1) with respect to (x1, y1, x2, y2)
  const float wpos = ix2 - ix1 > 0.f ? 1.f : 0.f, hpos = iy2 - iy1 > 0.f ? 1.f : 0.f;
  const float diw[4] = {p[0] > t[0] ? -wpos : 0.f, 0.f, p[2] < t[2] ? wpos : 0.f, 0.f};
  const float dih[4] = {0.f, p[1] > t[1] ? -hpos : 0.f, 0.f, p[3] < t[3] ? hpos : 0.f};
  const float da1[4] = {-ph, -pw, ph, pw};
  if constexpr (KIND == KIND_IOU) {
    const float u = fmaxf(uraw, eps);
    r.v = ov / u;
    if (GRAD) {
      const float ulive = uraw > eps ? 1.f : 0.f;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float dov = diw[k] * ih + iw * dih[k];
        const float du = ulive * (da1[k] - dov);
        r.d[k] = (dov * u - ov * du) / (u * u);
      }
    }
    return r;
  }
  const float ex1 = fminf(p[0], t[0]), ey1 = fminf(p[1], t[1]), ex2 = fmaxf(p[2], t[2]), ey2 = fmaxf(p[3], t[3]);
  const float ew = fmaxf(ex2 - ex1, 0.f), eh = fmaxf(ey2 - ey1, 0.f);
  const float ewpos = ex2 - ex1 > 0.f ? 1.f : 0.f, ehpos = ey2 - ey1 > 0.f ? 1.f : 0.f;
  const float dew[4] = {p[0] < t[0] ? -ewpos : 0.f, 0.f, p[2] > t[2] ? ewpos : 0.f, 0.f};
  const float deh[4] = {0.f, p[1] < t[1] ? -ehpos : 0.f, 0.f, p[3] > t[3] ? ehpos : 0.f};
  if constexpr (KIND == KIND_GIOU) {
    const float u = fmaxf(uraw, eps);
    const float earaw = ew * eh;
    const float ea = fmaxf(earaw, eps);
    r.v = ov / u - (ea - u) / ea;
    if (GRAD) {
      const float ulive = uraw > eps ? 1.f : 0.f, elive = earaw > eps ? 1.f : 0.f;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float dov = diw[k] * ih + iw * dih[k];
        const float du = ulive * (da1[k] - dov);
        const float dea = elive * (dew[k] * eh + ew * deh[k]);
        // giou = ov/u - 1 + u/ea
        r.d[k] = (dov * u - ov * du) / (u * u) + (du * ea - u * dea) / (ea * ea);
      }
    }
    return r;
  }
  // DIOU / CIOU
  const float u = uraw + eps;
  const float iou = ov / u;
  const float c2 = ew * ew + eh * eh + eps;
  const float dx = (t[0] + t[2]) - (p[0] + p[2]), dy = (t[1] + t[3]) - (p[1] + p[3]);
  const float rho2 = 0.25f * (dx * dx) + 0.25f * (dy * dy);
  float raw = iou - rho2 / c2;
  float alpha = 0.f, ang = 0.f, w1 = 0.f, h1 = 0.f;
  if constexpr (KIND == KIND_CIOU) {
    w1 = pw;
    h1 = ph + eps;
    const float w2 = t[2] - t[0], h2 = t[3] - t[1] + eps;
    ang = atanf(w2 / h2) - atanf(w1 / h1);
    const float v = 0.405284734569351f * (ang * ang);  // 4 / pi^2
    alpha = iou > 0.5f ? v / (1.f - iou + v) : 0.f;
    raw = iou - (rho2 / c2 + alpha * v);
    r.v = fminf(fmaxf(raw, -1.f), 1.f);
  } else {
    r.v = raw;
  }
  if (GRAD) {
    const float live = (KIND == KIND_CIOU && !(raw > -1.f && raw < 1.f)) ? 0.f : 1.f;
    // d rho2 / d (x1, y1, x2, y2) = -(dx, dy, dx, dy) / 2; CIOU: d v = 8 / pi^2 ang d ang, d ang = (h1, -w1, -h1, w1) / (w1^2 + h1^2)
    const float drho[4] = {-0.5f * dx, -0.5f * dy, -0.5f * dx, -0.5f * dy};
    const float den = w1 * w1 + h1 * h1;
    const float dang[4] = {h1, -w1, -h1, w1};
    const float vs = KIND == KIND_CIOU ? alpha * 0.810569469138702f * ang / den : 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float dov = diw[k] * ih + iw * dih[k];
      const float du = da1[k] - dov;
      const float dc2 = 2.f * (ew * dew[k] + eh * deh[k]);
      float d = (dov * u - ov * du) / (u * u) - (drho[k] * c2 - rho2 * dc2) / (c2 * c2);
      if constexpr (KIND == KIND_CIOU) d -= vs * dang[k];
      r.d[k] = live * d;
    }
  }
  return r;
}

// IoU of two normalised cxcywh boxes (QualityFocalLoss's score)
__device__ __forceinline__ float iou_cxcywh(const float* a, const float* b) {
  const float pa[4] = {a[0] - 0.5f * a[2], a[1] - 0.5f * a[3], a[0] + 0.5f * a[2], a[1] + 0.5f * a[3]};
  const float pb[4] = {b[0] - 0.5f * b[2], b[1] - 0.5f * b[3], b[0] + 0.5f * b[2], b[1] + 0.5f * b[3]};
  return box_iou<KIND_IOU, false>(pa, pb, 1e-6f).v;
}

// one thread per (s, b, q, g); KIND = IoUCost's iou_mode (GIOU or IOU)
template <int KIND>
__global__ __launch_bounds__(256) void match_cost_kernel(const float* __restrict__ cls, const float* __restrict__ box,
                                                         const float* __restrict__ gt_box, const long* __restrict__ gt_lab,
                                                         const float* __restrict__ factors, float* __restrict__ cost,
                                                         int S, int B, int Q, int C, int G, float w_cls, float w_l1,
                                                         float w_iou, float alpha, float gamma, float eps) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const long total = (long)S * B * Q * G;
  if (i >= total) return;
  const int g = (int)(i % G);
  const long sbq = i / G;
  const int b = (int)((sbq / Q) % B);
  const float* f = factors + b * 4;
  const float* gb = gt_box + ((long)b * G + g) * 4;
  const long lab = gt_lab[(long)b * G + g];
  const float p = sigmoidf_(cls[sbq * C + lab]);
  const float neg = -logf(1.f - p + eps) * (1.f - alpha) * powg(p, gamma);
  const float pos = -logf(p + eps) * alpha * powg(1.f - p, gamma);
  const float c_cls = (pos - neg) * w_cls;
  const float* pb = box + sbq * 4;
  const float n0 = gb[0] / f[0], n1 = gb[1] / f[1], n2 = gb[2] / f[2], n3 = gb[3] / f[3];
  const float gc[4] = {(n0 + n2) / 2.f, (n1 + n3) / 2.f, n2 - n0, n3 - n1};
  const float c_l1 = (fabsf(pb[0] - gc[0]) + fabsf(pb[1] - gc[1]) + fabsf(pb[2] - gc[2]) + fabsf(pb[3] - gc[3])) * w_l1;
  const float px[4] = {(pb[0] - 0.5f * pb[2]) * f[0], (pb[1] - 0.5f * pb[3]) * f[1], (pb[0] + 0.5f * pb[2]) * f[2],
                       (pb[1] + 0.5f * pb[3]) * f[3]};
  const float c_iou = -box_iou<KIND, false>(px, gb, 1e-6f).v * w_iou;
  cost[i] = c_cls + c_l1 + c_iou;
}

// grid = S sets; sums[s] = sum over (n, c) of weight[s,n] * focal(pred[s,n,c], target[s,n]); dpred = d sums / d pred
// (1024 threads per set: a set is 36 000 logits with an exp and a log each — 256 threads took 51 us for the 7 sets of a det
// iteration, a launch that runs alone on 7 CUs; the 16 wavefront sums meet in fixed order)
constexpr int FOCAL_THREADS = 1024;
__global__ __launch_bounds__(FOCAL_THREADS) void focal_sum_kernel(const float* __restrict__ pred, const long* __restrict__ target,
                                                                  const float* __restrict__ weight, float* __restrict__ sums,
                                                                  float* __restrict__ dpred, int N, int C, float gamma, float alpha) {
  __shared__ float red[FOCAL_THREADS / 64];
  const int s = blockIdx.x;
  const float tiny = 1.17549435e-38f;
  float acc = 0.f;
  const long base = (long)s * N * C;
  for (long e = threadIdx.x; e < (long)N * C; e += FOCAL_THREADS) {
    const long n = e / C;
    const int c = (int)(e - n * C);
    const float w = weight ? weight[(long)s * N + n] : 1.f;
    const float x = pred[base + e];
    const float p = sigmoidf_(x);
    const bool is_pos = target[(long)s * N + n] == c;
    float l, d;
    if (is_pos) {
      const float lp = logf(fmaxf(p, tiny)), q = powg(1.f - p, gamma);
      l = -alpha * q * lp;
      d = alpha * q * (gamma * p * lp - (1.f - p));
    } else {
      const float lq = logf(fmaxf(1.f - p, tiny)), q = powg(p, gamma);
      l = -(1.f - alpha) * q * lq;
      d = (1.f - alpha) * q * (p - gamma * (1.f - p) * lq);
    }
    acc += w * l;
    dpred[base + e] = w * d;
  }
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = 0.f;
#pragma unroll
    for (int w = 0; w < FOCAL_THREADS / 64; ++w) t += red[w];
    sums[s] = t;
  }
}

// mmdet QualityFocalLoss (DETR / DINO heads of mmdet 3.x) summed per set, the layout and reduction of focal_sum_kernel:
// off the target class BCE(x, 0) sigma^beta; at the target class BCE(x, s) |s - sigma|^beta with the quality s = IoU of the
// query's (detached) predicted box and its target box, both normalised cxcywh.  BCE in its stable form
// max(x, 0) - x s + log1p(exp(-|x|)).  dpred = d sums / d pred; s is a constant, the boxes get no gradient.
__global__ __launch_bounds__(FOCAL_THREADS) void qfl_sum_kernel(const float* __restrict__ pred, const long* __restrict__ target,
                                                                const float* __restrict__ weight, const float* __restrict__ box,
                                                                const float* __restrict__ box_t, float* __restrict__ sums,
                                                                float* __restrict__ dpred, int N, int C, float beta) {
  __shared__ float red[FOCAL_THREADS / 64];
  const int s = blockIdx.x;
  float acc = 0.f;
  const long base = (long)s * N * C;
  for (long e = threadIdx.x; e < (long)N * C; e += FOCAL_THREADS) {
    const long n = e / C;
    const int c = (int)(e - n * C);
    const long row = (long)s * N + n;
    const float w = weight ? weight[row] : 1.f;
    const float x = pred[base + e];
    // one exp feeds the sigmoid, its complement and BCE(x, 0): ex = exp(-|x|) <= 1
    const float ex = expf(-fabsf(x)), r1 = 1.f / (1.f + ex);
    const float p = x >= 0.f ? r1 : ex * r1, omp = x >= 0.f ? ex * r1 : r1;  // sigma, 1 - sigma
    const float soft = fmaxf(x, 0.f) + log1pf(ex);                           // BCE(x, 0)
    float l, d;
    if (target[row] == c) {
      const float q = iou_cxcywh(box + row * 4, box_t + row * 4);
      const float bce = soft - x * q, df = p - q, ad = fabsf(df);
      // |df|^beta and d |df|^beta / d df = beta |df|^(beta - 1) sign(df)
      const float m = powg(ad, beta);
      const float dm = beta == 2.f ? 2.f * df : (ad > 0.f ? beta * powf(ad, beta - 1.f) * (df > 0.f ? 1.f : -1.f) : 0.f);
      l = bce * m;
      d = df * m + bce * dm * p * omp;
    } else {
      const float m = powg(p, beta);
      l = soft * m;
      d = m * (p + beta * omp * soft);
    }
    acc += w * l;
    dpred[base + e] = w * d;
  }
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = 0.f;
#pragma unroll
    for (int w = 0; w < FOCAL_THREADS / 64; ++w) t += red[w];
    sums[s] = t;
  }
}

// grid = S sets over the B*Q boxes of a set: sums[0][s] = sum |pred - target| * weight (cxcywh, normalised);
// sums[1][s] = sum loss_KIND(pred_xyxy * f, target_xyxy * f) * mean(weight), loss = 1 - box_iou<KIND> (KIND_IOU: IoULoss's
// `mode` of max(iou, eps), the union clamped at 1e-6); d_l1 / d_giou = their gradients wrt pred.  Kinds other than GIOU give a
// row of zero weight an exact 0 and a zero gradient whatever its boxes hold (CIOU's alpha is 0 / 0 for identical boxes).
template <int KIND>
__global__ __launch_bounds__(256) void box_loss_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                       const float* __restrict__ weight, const float* __restrict__ factors,
                                                       float* __restrict__ sums, float* __restrict__ d_l1,
                                                       float* __restrict__ d_giou, int S, int B, int Q, float eps, int mode) {
  __shared__ float red[4];
  const int s = blockIdx.x;
  float a_l1 = 0.f, a_gi = 0.f;
  for (int e = threadIdx.x; e < B * Q; e += 256) {
    const int b = e / Q;
    const long o = ((long)s * B * Q + e) * 4;
    const float* f = factors + b * 4;
    const float* p = pred + o;
    const float* t = target + o;
    const float* w = weight + o;
    float dl[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float df = p[k] - t[k];
      a_l1 += fabsf(df) * w[k];
      dl[k] = (df > 0.f ? 1.f : (df < 0.f ? -1.f : 0.f)) * w[k];
    }
    const float px[4] = {(p[0] - 0.5f * p[2]) * f[0], (p[1] - 0.5f * p[3]) * f[1], (p[0] + 0.5f * p[2]) * f[2],
                         (p[1] + 0.5f * p[3]) * f[3]};
    const float tx[4] = {(t[0] - 0.5f * t[2]) * f[0], (t[1] - 0.5f * t[3]) * f[1], (t[0] + 0.5f * t[2]) * f[2],
                         (t[1] + 0.5f * t[3]) * f[3]};
    const float wm = (w[0] + w[1] + w[2] + w[3]) * 0.25f;
    BoxIou g = box_iou<KIND, true>(px, tx, KIND == KIND_IOU ? 1e-6f : eps);
    float loss = 1.f - g.v;
    if constexpr (KIND == KIND_IOU) {
      // IoULoss: iou floored at eps (no gradient below it), then 1 - iou | 1 - iou^2 | -log(iou); g.d becomes -d loss
      const float iou = fmaxf(g.v, eps);
      const float live = g.v > eps ? 1.f : 0.f;
      const float sc = live * (mode == IOU_LINEAR ? 1.f : (mode == IOU_SQUARE ? 2.f * iou : 1.f / iou));
      loss = mode == IOU_LINEAR ? 1.f - iou : (mode == IOU_SQUARE ? 1.f - iou * iou : -logf(iou));
#pragma unroll
      for (int k = 0; k < 4; ++k) g.d[k] *= sc;
    }
    if constexpr (KIND != KIND_GIOU) {
      if (wm == 0.f) {
        loss = 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) g.d[k] = 0.f;
      }
    }
    a_gi += loss * wm;
    // d loss/d(cx, cy, w, h) through x1 = (cx - w/2) f0, y1 = (cy - h/2) f1, x2 = (cx + w/2) f2, y2 = (cy + h/2) f3
    const float gx1 = -g.d[0] * wm * f[0], gy1 = -g.d[1] * wm * f[1], gx2 = -g.d[2] * wm * f[2], gy2 = -g.d[3] * wm * f[3];
    float4 dg = make_float4(gx1 + gx2, gy1 + gy2, 0.5f * (gx2 - gx1), 0.5f * (gy2 - gy1));
    *reinterpret_cast<float4*>(d_l1 + o) = make_float4(dl[0], dl[1], dl[2], dl[3]);
    *reinterpret_cast<float4*>(d_giou + o) = dg;
  }
  const float t1 = block_sum256(a_l1, red);
  const float t2 = block_sum256(a_gi, red);
  if (threadIdx.x == 0) {
    sums[s] = t1;
    sums[S + s] = t2;
  }
}

// Iterative box refinement of Deformable-DETR / DINO: out = sigmoid(delta + inverse_sigmoid(ref, eps))
// (models/multi/bbox_head/transformer.py:112-118 in the decoder, dino_head.py:133-137 in the head), with
// inverse_sigmoid(x) = log(max(clamp(x,0,1), eps) / max(1 - clamp(x,0,1), eps)).  One launch instead of eight.
__global__ __launch_bounds__(256) void refine_box_fwd_kernel(const float* __restrict__ delta, const float* __restrict__ ref,
                                                             float* __restrict__ out, long n, float eps) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float x = fminf(fmaxf(ref[i], 0.f), 1.f);
  const float inv = logf(fmaxf(x, eps) / fmaxf(1.f - x, eps));
  out[i] = sigmoidf_(delta[i] + inv);
}

// d_delta = g * out * (1 - out); d_ref = d_delta * d inverse_sigmoid / d ref (zero where a clamp is active)
__global__ __launch_bounds__(256) void refine_box_bwd_kernel(const float* __restrict__ g, const float* __restrict__ out,
                                                             const float* __restrict__ ref, float* __restrict__ d_delta,
                                                             float* __restrict__ d_ref, long n, float eps) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float o = out[i];
  const float d = g[i] * o * (1.f - o);
  if (d_delta) d_delta[i] = d;
  if (d_ref) {
    const float r = ref[i];
    float di = 0.f;
    if (r >= 0.f && r <= 1.f) {  // inside the outer clamp
      if (r >= eps) di += 1.f / r;                 // d log(max(x, eps))
      if (1.f - r >= eps) di += 1.f / (1.f - r);   // -d log(max(1 - x, eps))
    }
    d_ref[i] = d * di;
  }
}

}  // namespace rscotr

using namespace rscotr;

extern "C" int rscotr_refine_box_fwd(const float* delta, const float* ref, float* out, int64_t n, float eps, void* stream) {
  if (n < 0) return fail(RSCOTR_E_SHAPE, "rscotr_refine_box_fwd: negative size");
  if (n == 0) return RSCOTR_OK;
  if (!delta || !ref || !out) return fail(RSCOTR_E_ARG, "rscotr_refine_box_fwd: null pointer");
  refine_box_fwd_kernel<<<(unsigned)((n + 255) / 256), 256, 0, (hipStream_t)stream>>>(delta, ref, out, n, eps);
  return check_launch("rscotr_refine_box_fwd");
}

extern "C" int rscotr_refine_box_bwd(const float* grad_out, const float* out, const float* ref, float* d_delta, float* d_ref,
                                     int64_t n, float eps, void* stream) {
  if (n < 0) return fail(RSCOTR_E_SHAPE, "rscotr_refine_box_bwd: negative size");
  if (n == 0) return RSCOTR_OK;
  if (!grad_out || !out || !ref) return fail(RSCOTR_E_ARG, "rscotr_refine_box_bwd: null pointer");
  refine_box_bwd_kernel<<<(unsigned)((n + 255) / 256), 256, 0, (hipStream_t)stream>>>(grad_out, out, ref, d_delta, d_ref, n, eps);
  return check_launch("rscotr_refine_box_bwd");
}

// `who` names the exported entry in error messages: the three fixed-recipe entries forward to the kind-parameterised ones
static int match_cost_launch(const char* who, const float* cls, const float* box, const float* gt_box, const int64_t* gt_lab,
                             const float* factors, float* cost, int S, int B, int Q, int C, int G, float w_cls, float w_l1,
                             float w_iou, float alpha, float gamma, float eps, int iou_mode, void* stream) {
  if (S < 0 || B < 0 || Q < 0 || C <= 0 || G < 0) return fail(RSCOTR_E_SHAPE, "%s: bad shape", who);
  if (iou_mode != KIND_GIOU && iou_mode != KIND_IOU) return fail(RSCOTR_E_ARG, "%s: iou_mode must be 0 (giou) or 1 (iou)", who);
  const long total = (long)S * B * Q * G;
  if (total == 0) return RSCOTR_OK;
  if (!cls || !box || !gt_box || !gt_lab || !factors || !cost) return fail(RSCOTR_E_ARG, "%s: null pointer", who);
  const unsigned grid = (unsigned)((total + 255) / 256);
  if (iou_mode == KIND_GIOU)
    match_cost_kernel<KIND_GIOU><<<grid, 256, 0, (hipStream_t)stream>>>(cls, box, gt_box, (const long*)gt_lab, factors, cost, S, B, Q,
                                                                        C, G, w_cls, w_l1, w_iou, alpha, gamma, eps);
  else
    match_cost_kernel<KIND_IOU><<<grid, 256, 0, (hipStream_t)stream>>>(cls, box, gt_box, (const long*)gt_lab, factors, cost, S, B, Q,
                                                                       C, G, w_cls, w_l1, w_iou, alpha, gamma, eps);
  return check_launch(who);
}

extern "C" int rscotr_match_cost(const float* cls, const float* box, const float* gt_box, const int64_t* gt_lab,
                                 const float* factors, float* cost, int S, int B, int Q, int C, int G, float w_cls,
                                 float w_l1, float w_iou, float alpha, float gamma, float eps, void* stream) {
  return match_cost_launch("rscotr_match_cost", cls, box, gt_box, gt_lab, factors, cost, S, B, Q, C, G, w_cls, w_l1, w_iou, alpha,
                           gamma, eps, KIND_GIOU, stream);
}

extern "C" int rscotr_match_cost_kind(const float* cls, const float* box, const float* gt_box, const int64_t* gt_lab,
                                      const float* factors, float* cost, int S, int B, int Q, int C, int G, float w_cls,
                                      float w_l1, float w_iou, float alpha, float gamma, float eps, int iou_mode, void* stream) {
  return match_cost_launch("rscotr_match_cost_kind", cls, box, gt_box, gt_lab, factors, cost, S, B, Q, C, G, w_cls, w_l1, w_iou,
                           alpha, gamma, eps, iou_mode, stream);
}

extern "C" int rscotr_focal_sum(const float* pred, const int64_t* target, const float* weight, float* sums, float* dpred,
                                int S, int N, int C, float gamma, float alpha, void* stream) {
  if (S < 0 || N < 0 || C <= 0) return fail(RSCOTR_E_SHAPE, "rscotr_focal_sum: bad shape");
  if (S == 0) return RSCOTR_OK;
  if (!pred || !target || !sums || !dpred) return fail(RSCOTR_E_ARG, "rscotr_focal_sum: null pointer");
  focal_sum_kernel<<<S, FOCAL_THREADS, 0, (hipStream_t)stream>>>(pred, (const long*)target, weight, sums, dpred, N, C, gamma, alpha);
  return check_launch("rscotr_focal_sum");
}

extern "C" int rscotr_qfl_sum(const float* pred, const int64_t* target, const float* weight, const float* box, const float* box_target,
                              float* sums, float* dpred, int S, int N, int C, float beta, void* stream) {
  if (S < 0 || N < 0 || C <= 0) return fail(RSCOTR_E_SHAPE, "rscotr_qfl_sum: bad shape");
  if (!(beta >= 0.f)) return fail(RSCOTR_E_ARG, "rscotr_qfl_sum: beta must be >= 0");
  if (S == 0) return RSCOTR_OK;
  if (!pred || !target || !box || !box_target || !sums || !dpred) return fail(RSCOTR_E_ARG, "rscotr_qfl_sum: null pointer");
  qfl_sum_kernel<<<S, FOCAL_THREADS, 0, (hipStream_t)stream>>>(pred, (const long*)target, weight, box, box_target, sums, dpred, N, C,
                                                               beta);
  return check_launch("rscotr_qfl_sum");
}

static int box_loss_launch(const char* who, const float* pred, const float* target, const float* weight, const float* factors,
                           float* sums, float* d_l1, float* d_iou, int S, int B, int Q, float eps, int kind, int mode,
                           void* stream) {
  if (S < 0 || B < 0 || Q < 0) return fail(RSCOTR_E_SHAPE, "%s: bad shape", who);
  if (kind < 0 || kind >= KIND_COUNT) return fail(RSCOTR_E_ARG, "%s: kind must be 0 (giou), 1 (iou), 2 (diou) or 3 (ciou)", who);
  if (kind == KIND_IOU && (mode < IOU_LINEAR || mode > IOU_LOG))
    return fail(RSCOTR_E_ARG, "%s: mode must be 0 (linear), 1 (square) or 2 (log)", who);
  if (S == 0) return RSCOTR_OK;
  if (!pred || !target || !weight || !factors || !sums || !d_l1 || !d_iou) return fail(RSCOTR_E_ARG, "%s: null pointer", who);
  if (!aligned16(d_l1) || !aligned16(d_iou)) return fail(RSCOTR_E_ALIGN, "%s: gradient buffers must be 16-byte aligned", who);
  const hipStream_t st = (hipStream_t)stream;
  switch (kind) {
    case KIND_GIOU: box_loss_kernel<KIND_GIOU><<<S, 256, 0, st>>>(pred, target, weight, factors, sums, d_l1, d_iou, S, B, Q, eps, mode); break;
    case KIND_IOU: box_loss_kernel<KIND_IOU><<<S, 256, 0, st>>>(pred, target, weight, factors, sums, d_l1, d_iou, S, B, Q, eps, mode); break;
    case KIND_DIOU: box_loss_kernel<KIND_DIOU><<<S, 256, 0, st>>>(pred, target, weight, factors, sums, d_l1, d_iou, S, B, Q, eps, mode); break;
    default: box_loss_kernel<KIND_CIOU><<<S, 256, 0, st>>>(pred, target, weight, factors, sums, d_l1, d_iou, S, B, Q, eps, mode); break;
  }
  return check_launch(who);
}

extern "C" int rscotr_box_loss(const float* pred, const float* target, const float* weight, const float* factors,
                               float* sums, float* d_l1, float* d_giou, int S, int B, int Q, float eps, void* stream) {
  return box_loss_launch("rscotr_box_loss", pred, target, weight, factors, sums, d_l1, d_giou, S, B, Q, eps, KIND_GIOU, 0, stream);
}

extern "C" int rscotr_box_loss_kind(const float* pred, const float* target, const float* weight, const float* factors,
                                    float* sums, float* d_l1, float* d_iou, int S, int B, int Q, float eps, int kind, int mode,
                                    void* stream) {
  return box_loss_launch("rscotr_box_loss_kind", pred, target, weight, factors, sums, d_l1, d_iou, S, B, Q, eps, kind, mode, stream);
}
