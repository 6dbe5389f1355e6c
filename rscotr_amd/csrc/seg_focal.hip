// Fused bilinear-upsample + sigmoid focal loss for the seg head (gfx950): mmseg 0.28 FocalLoss (py_sigmoid_focal_loss) as
// BaseDecodeHead.losses reaches it, with the head's ignore_index.
//
//   u = resize(seg_logit (B,C,h,w), size=label.shape, mode='bilinear', align_corners=False)
//   t[b,c,.] = [label == c]      (an ignored pixel, or any label outside [0, C), has no positive class)
//   v[b,.]   = [label != ignore_index]
//   s = sigmoid(u);  q = (1 - s) t + s (1 - t)
//   e = BCE_with_logits(u, t) * (alpha_c t + (1 - alpha_c) (1 - t)) * q^gamma * class_weight[c] * v
//   loss = loss_scale * sum e        (loss_scale = loss_weight / (B*H*W*C) for reduction='mean': ignored pixels count in the divisor)
//
// With x = -u for the positive class and u for a negative one, q = sigmoid(x) and BCE = softplus(x), so one element is
// k softplus(x) sigmoid(x)^gamma and d e / d x = k q^gamma (q + gamma softplus(x) (1 - q)).  Everything is formed from
// E = exp(-|x|) in (0, 1]: softplus(x) = max(x, 0) + log1p(E), q = {1, E} / (1 + E), q^gamma = exp(-gamma softplus(-x)); no
// exp(u), no inf / inf, and gamma = 0 gives q^0 = 1 with a finite gradient.
//
// As in seg_loss.hip, the up-sampled logits never exist in memory: a pixel's interpolated logits live in registers.  Focal is
// per element: no log-sum-exp, and nothing per pixel is saved for backward.
//   forward   upsample_focal_fwd_kernel   one thread per pixel walks the classes; one partial sum per workgroup
//             upsample_focal_fold_kernel  folds the partial sums in fixed order (fp64) and applies loss_scale
//   backward  upsample_focal_bwd_kernel   the blocked gather of seg_upsample.h with a RAW term (the interpolated logit itself
//                                         reaches term(): no lse array is read); an ignored pixel is skipped
// No float atomics, every sum in a fixed order: two runs are bit-equal.  Nothing synchronises with the host.
#include <algorithm>

#include "seg_upsample.h"

namespace rscotr {

constexpr int FOCAL_MAX_WG = 4096;  // grid cap of the forward launch = partial sums in the workspace

// one element from x (see above): softplus(x), q = sigmoid(x), 1 - q, q^gamma.  GRAD (the backward term): log1p(E) as log(1 + E)
// and the reciprocal as v_rcp_f32 — an absolute error of 1e-7 on softplus, which the gradient multiplies by gamma (1 - q) <= gamma;
// the forward sum keeps log1pf (small terms would lose their relative accuracy).
template <bool GRAD>
struct FocalElem {
  float sp, q, omq, qg;
  __device__ __forceinline__ FocalElem(float x, float gamma) {
    const float E = __expf(-fabsf(x));
    const float L = GRAD ? __logf(1.f + E) : log1pf(E);
    const float r = GRAD ? __builtin_amdgcn_rcpf(1.f + E) : 1.f / (1.f + E);
    sp = fmaxf(x, 0.f) + L;
    q = x >= 0.f ? r : E * r;
    omq = x >= 0.f ? E * r : r;
    qg = __expf(-gamma * (fmaxf(-x, 0.f) + L));
  }
};

// alpha_c t + (1 - alpha_c) (1 - t), times the class weight
__device__ __forceinline__ float focal_class_k(const float* __restrict__ alpha_c, const float* __restrict__ cw, float alpha, int c,
                                               bool positive) {
  const float a = alpha_c ? alpha_c[c] : alpha;
  return (positive ? a : 1.f - a) * (cw ? cw[c] : 1.f);
}

__global__ __launch_bounds__(256) void upsample_focal_fwd_kernel(const float* __restrict__ logit, const int64_t* __restrict__ label,
                                                                 const float* __restrict__ alpha_c, const float* __restrict__ cw,
                                                                 float* __restrict__ part, int B, int C, int h, int w, int H, int W,
                                                                 int ignore, float gamma, float alpha) {
  const long npix = (long)B * H * W;
  const float sy = (float)h / (float)H, sx = (float)w / (float)W;
  float loss = 0.f;
  for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < npix; p += (long)gridDim.x * 256) {
    const long lab = label[p];
    if (lab == ignore) continue;
    const int x = (int)(p % W), y = (int)((p / W) % H), b = (int)(p / ((long)W * H));
    const Taps taps(y, x, sy, sx, h, w);
    const float* base = logit + (long)b * C * h * w;
    float e = 0.f;
    for (int c = 0; c < C; ++c) {
      const float u = taps.at(base + (long)c * h * w);
      const bool pos = c == lab;
      const FocalElem<false> f(pos ? -u : u, gamma);
      e = fmaf(focal_class_k(alpha_c, cw, alpha, c, pos), f.sp * f.qg, e);
    }
    loss += e;
  }
  loss = wave_sum(loss);
  __shared__ float red[4];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = loss;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

// one workgroup: the partial sums in fixed order
__global__ __launch_bounds__(256) void upsample_focal_fold_kernel(const float* __restrict__ part, float* __restrict__ loss,
                                                                  int nparts, float loss_scale) {
  double acc = 0.0;
  for (int i = threadIdx.x; i < nparts; i += 256) acc += (double)part[i];
  __shared__ double red[256];
  red[threadIdx.x] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int i = 0; i < 256; ++i) t += red[i];
    loss[0] = (float)(t * (double)loss_scale);
  }
}

// dlogit[b,c,cy,cx] = scale * sum over output pixels p touching the cell of  wt(p->cell) * d e_c(p) / d u_c(p): the blocked
// gather of seg_upsample.h on the interpolated logit itself.  A lane holds its class's two weights (positive, negative) in
// registers; a pixel is staged with its label where that is a channel, -1 where it is none (all-negative), -2 where ignored.
struct FocalTerm {
  static constexpr bool PLANE = false;
  static constexpr bool RAW = true;
  const int64_t* __restrict__ label;
  const float* __restrict__ alpha_c;
  const float* __restrict__ cw;
  int C, ignore;
  float gamma, alpha;
  float kp, kn;  // this lane's class
  __device__ __forceinline__ void load_class(int, int c) {
    kp = 0.f; kn = 0.f;
    if (c < C) { kp = focal_class_k(alpha_c, cw, alpha, c, true); kn = focal_class_k(alpha_c, cw, alpha, c, false); }
  }
  __device__ __forceinline__ int stage(long p, float&) const {
    const long lab = label[p];
    return lab == ignore ? -2 : (lab >= 0 && lab < C ? (int)lab : -1);
  }
  __device__ __forceinline__ bool skip(int lab) const { return lab == -2; }
  __device__ __forceinline__ float term(float u, int c, int lab, float) const {
    const bool pos = c == lab;
    const FocalElem<true> f(pos ? -u : u, gamma);
    const float dx = f.qg * fmaf(gamma * f.sp, f.omq, f.q);
    return pos ? -kp * dx : kn * dx;
  }
};

__global__ __launch_bounds__(512) void upsample_focal_bwd_kernel(const float* __restrict__ logit, const int64_t* __restrict__ label,
                                                                 const float* __restrict__ alpha_c, const float* __restrict__ cw,
                                                                 const float* __restrict__ gscale, float* __restrict__ dlogit, int B,
                                                                 int C, int h, int w, int H, int W, int ignore, float gamma,
                                                                 float alpha) {
  upsample_gather(FocalTerm{label, alpha_c, cw, C, ignore, gamma, alpha, 0.f, 0.f}, logit, nullptr, gscale, dlogit, C, h, w, H, W);
}

static int focal_check(const char* entry, int B, int C, int h, int w, int H, int W, float gamma) {
  if (int e = upsample_check_shape(entry, B, C, h, w, H, W)) return e;
  if ((long)C * h * w > 0x7fffffffL || (long)H * W > 0x7fffffffL) return fail(RSCOTR_E_SHAPE, "%s: shape too large", entry);
  if (!(gamma >= 0.f)) return fail(RSCOTR_E_ARG, "%s: gamma >= 0 required", entry);
  return RSCOTR_OK;
}

}  // namespace rscotr

using namespace rscotr;

// the forward partial sums: one float per workgroup
extern "C" int64_t rscotr_upsample_focal_workspace(void) { return (int64_t)FOCAL_MAX_WG * 4; }

extern "C" int rscotr_upsample_focal_fwd(const float* logit, const int64_t* label, const float* alpha_per_class,
                                         const float* class_weight, float* loss, int B, int C, int h, int w, int H, int W,
                                         int ignore_index, float gamma, float alpha, float loss_scale, float* workspace,
                                         int64_t workspace_bytes, void* stream) {
  if (int e = focal_check("rscotr_upsample_focal_fwd", B, C, h, w, H, W, gamma)) return e;
  if (!loss) return fail(RSCOTR_E_ARG, "rscotr_upsample_focal_fwd: null pointer");
  hipStream_t s = (hipStream_t)stream;
  if (B == 0) {
    (void)hipMemsetAsync(loss, 0, sizeof(float), s);
    return RSCOTR_OK;
  }
  if (!logit || !label) return fail(RSCOTR_E_ARG, "rscotr_upsample_focal_fwd: null pointer");
  if (!workspace || workspace_bytes < rscotr_upsample_focal_workspace())
    return fail(RSCOTR_E_ARG, "rscotr_upsample_focal_fwd: workspace of rscotr_upsample_focal_workspace() bytes required");
  const long npix = (long)B * H * W;
  const int nwg = (int)std::min<long>((npix + 255) / 256, FOCAL_MAX_WG);
  upsample_focal_fwd_kernel<<<nwg, 256, 0, s>>>(logit, label, alpha_per_class, class_weight, workspace, B, C, h, w, H, W,
                                                ignore_index, gamma, alpha);
  upsample_focal_fold_kernel<<<1, 256, 0, s>>>(workspace, loss, nwg, loss_scale);
  return check_launch("rscotr_upsample_focal_fwd");
}

// dlogit (B,C,h,w) = grad_scale[0] * d(sum e)/d(logit); grad_scale is a DEVICE scalar (upstream gradient * loss_scale)
extern "C" int rscotr_upsample_focal_bwd(const float* logit, const int64_t* label, const float* alpha_per_class,
                                         const float* class_weight, const float* grad_scale, float* dlogit, int B, int C, int h,
                                         int w, int H, int W, int ignore_index, float gamma, float alpha, void* stream) {
  if (int e = focal_check("rscotr_upsample_focal_bwd", B, C, h, w, H, W, gamma)) return e;
  if (B == 0) return RSCOTR_OK;
  if ((long)B * ((h + UCE_TB - 1) / UCE_TB) * ((w + UCE_TB - 1) / UCE_TB) > 0x7fffffffL)
    return fail(RSCOTR_E_SHAPE, "rscotr_upsample_focal_bwd: batch too large");
  if (!logit || !label || !grad_scale || !dlogit) return fail(RSCOTR_E_ARG, "rscotr_upsample_focal_bwd: null pointer");
  launch_upsample_gather<upsample_focal_bwd_kernel, false>((hipStream_t)stream, B, h, w, logit, label, alpha_per_class, class_weight,
                                                           grad_scale, dlogit, B, C, h, w, H, W, ignore_index, gamma, alpha);
  return check_launch("rscotr_upsample_focal_bwd");
}
