// Fused bilinear-upsample + cross-entropy (+ top-1 accuracy) for the seg head (gfx950).
//
// Replaces mmseg BaseDecodeHead.losses as reached from models/multi/seg_head/mask2former_head.py:204:
//   seg_logit = resize(seg_logit (B,C,h,w), size=label.shape, mode='bilinear', align_corners=False)
//   loss_ce   = F.cross_entropy(seg_logit, label, ignore_index=255, reduction='none').mean()   (all pixels)
//   acc_seg   = accuracy(seg_logit, label)   (top-1 over the non-ignored pixels, in percent)
// The reference materialises the upsampled logits — (2,100,512,512) fp32 = 210 MB written, read by
// log-softmax, NLL, arg-max, and again in backward.  Here a pixel's C interpolated logits only ever
// exist in registers: forward reads the (B,C,h,w) logits (3.3 MB) and the labels, writes one
// log-sum-exp per pixel (for backward) and three scalars; backward is a GATHER per block of low-resolution cells (no atomics).
// The resize's source index (src_index), a pixel's 2 x 2 taps and the body of that gather are in seg_upsample.h, shared with
// csrc/seg_dice.hip and csrc/seg_focal.hip; this file supplies the cross-entropy's gradient term (CeTerm).
#include "seg_upsample.h"

namespace rscotr {

// one thread per output pixel; classes streamed (online log-sum-exp + running arg-max)
// WT (class weights / pixel sampling, rscotr_upsample_ce_w_fwd): the pixel's CE is also written to `nll` (0 for an ignored pixel)
// and its weight cw[label] (1 without class weights, 0 for an ignored pixel) to `pixw`; sums[0] is the WEIGHTED sum.  The
// unweighted instantiation never touches the three extra pointers.
template <bool WT>
__global__ __launch_bounds__(256) void upsample_ce_fwd_kernel(const float* __restrict__ logit,
                                                              const int64_t* __restrict__ label,
                                                              float* __restrict__ lse, float* __restrict__ sums, int B,
                                                              int C, int h, int w, int H, int W, int ignore,
                                                              const float* __restrict__ cw, float* __restrict__ nll,
                                                              float* __restrict__ pixw) {
  const long npix = (long)B * H * W;
  const float sy = (float)h / (float)H, sx = (float)w / (float)W;
  float loss = 0.f, correct = 0.f, valid = 0.f;
  for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < npix; p += (long)gridDim.x * 256) {
    const int x = (int)(p % W), y = (int)((p / W) % H), b = (int)(p / ((long)W * H));
    const Taps taps(y, x, sy, sx, h, w);
    const float* base = logit + (long)b * C * h * w;
    const long lab = label[p];
    float m = -3.0e38f, s = 0.f, best = -3.0e38f, at_label = 0.f;
    int arg = 0;
    for (int c = 0; c < C; ++c) {
      const float v = taps.at(base + (long)c * h * w);
      if (v > best) { best = v; arg = c; }
      if (c == lab) at_label = v;
      if (v > m) { s = s * __expf(m - v) + 1.f; m = v; }
      else s += __expf(v - m);
    }
    const float l = m + __logf(s);
    lse[p] = l;
    if constexpr (WT) {
      float nl = 0.f, pw = 0.f;
      if (lab != ignore) {
        nl = l - at_label;
        pw = (cw && lab >= 0 && lab < C) ? cw[lab] : 1.f;
        loss = fmaf(pw, nl, loss);
        valid += 1.f;
        correct += (arg == (int)lab) ? 1.f : 0.f;
      }
      nll[p] = nl;
      pixw[p] = pw;
    } else if (lab != ignore) {
      loss += l - at_label;
      valid += 1.f;
      correct += (arg == (int)lab) ? 1.f : 0.f;
    }
  }
  loss = wave_sum(loss);
  correct = wave_sum(correct);
  valid = wave_sum(valid);
  __shared__ float red[4][3];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) { red[wv][0] = loss; red[wv][1] = correct; red[wv][2] = valid; }
  __syncthreads();
  if (threadIdx.x < 3)  // one partial row per workgroup, folded in fixed order by upsample_ce_sums_kernel (no atomics)
    sums[(long)blockIdx.x * 3 + threadIdx.x] = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
}

__global__ __launch_bounds__(256) void upsample_ce_sums_kernel(const float* __restrict__ part, float* __restrict__ sums,
                                                               int nparts) {
  float a[3] = {0.f, 0.f, 0.f};
  for (int i = threadIdx.x; i < nparts; i += 256)
#pragma unroll
    for (int k = 0; k < 3; ++k) a[k] += part[(long)i * 3 + k];
  __shared__ float red[4][3];
#pragma unroll
  for (int k = 0; k < 3; ++k) a[k] = wave_sum(a[k]);
  if ((threadIdx.x & 63) == 0)
#pragma unroll
    for (int k = 0; k < 3; ++k) red[threadIdx.x >> 6][k] = a[k];
  __syncthreads();
  if (threadIdx.x < 3) sums[threadIdx.x] = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
}

// Backward: the blocked gather of seg_upsample.h with softmax_c(p) - [c == label_p] as the term; an ignored pixel is skipped.
// WT (rscotr_upsample_ce_w_bwd): every pixel's softmax - one-hot is multiplied by pixw[p] (class weight x sampling mask), staged
// as the gather's plane (UCE_FP^2 more floats of LDS, 80 KB in all: still two workgroups per CU); a pixel of weight 0 is staged
// as ignored.
template <bool WT>
struct CeTerm {
  static constexpr bool PLANE = WT;
  static constexpr bool RAW = false;
  const int64_t* __restrict__ label;
  const float* __restrict__ pixw;  // WT only
  int ignore;
  __device__ __forceinline__ void load_class(int, int) {}
  __device__ __forceinline__ int stage(long p, float& plane) const {
    if constexpr (WT) plane = pixw[p];
    return WT && plane == 0.f ? ignore : (int)label[p];
  }
  __device__ __forceinline__ bool skip(int lab) const { return lab == ignore; }
  __device__ __forceinline__ float term(float prob, int c, int lab, float plane) const {
    const float gq = prob - (c == lab ? 1.f : 0.f);
    return WT ? gq * plane : gq;
  }
};

template <bool WT>
__global__ __launch_bounds__(512) void upsample_ce_bwd_kernel(const float* __restrict__ logit, const int64_t* __restrict__ label,
                                                              const float* __restrict__ lse, const float* __restrict__ gscale,
                                                              float* __restrict__ dlogit, int B, int C, int h, int w, int H, int W,
                                                              int ignore, const float* __restrict__ pixw) {
  upsample_gather(CeTerm<WT>{label, pixw, ignore}, logit, lse, gscale, dlogit, C, h, w, H, W);
}

// ---- online hard example mining (mmseg OHEMPixelSampler with a probability threshold) ---------------------------------------
// A valid pixel is kept when prob_p < max(kth, thresh), kth = the min(kept, N_valid - 1)-th smallest prob_p = exp(-nll_p) over
// the valid pixels.  exp is monotone, so the selection is made on the CE plane itself: nll_p > min(k-th LARGEST nll, -log thresh).
// The order statistic is a radix select over the order-preserving 32-bit keys of the floats, most significant byte first: a
// histogram launch (LDS bins, then integer atomics on 256 global bins: order-independent) and a one-workgroup pick launch per
// byte.  N_valid is the first histogram's total: it never leaves the device.  Any number of equal values lands in one bin.
constexpr int UCE_SEL_WG = 256;  // grid cap of the histogram and mask launches (one workgroup per CU)
constexpr int UCE_SEL_WORDS = 4 * 256 + 8;  // four histograms + {prefix, rank, N_valid, bits of the CE threshold}

__device__ __forceinline__ unsigned uce_key(float v) {  // a < b  <=>  key(a) < key(b) (as unsigned; -0 < +0)
  const unsigned b = __float_as_uint(v);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float uce_unkey(unsigned k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// pass j counts byte (3 - j) of the keys whose higher bytes equal the prefix picked so far
__global__ __launch_bounds__(256) void uce_ohem_hist_kernel(const int64_t* __restrict__ label, const float* __restrict__ nll,
                                                            unsigned* __restrict__ hist, const unsigned* __restrict__ st,
                                                            long npix, int ignore, int pass) {
  __shared__ unsigned sh[256];
  sh[threadIdx.x] = 0u;
  __syncthreads();
  const int shift = 24 - 8 * pass;
  const unsigned prefix = pass ? st[0] : 0u;
  for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < npix; p += (long)gridDim.x * 256) {
    if (label[p] == ignore) continue;
    const unsigned key = uce_key(nll[p]);
    if (pass == 0 || (key >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&sh[(key >> shift) & 255u], 1u);
  }
  __syncthreads();
  if (sh[threadIdx.x]) atomicAdd(&hist[threadIdx.x], sh[threadIdx.x]);
}

// one workgroup: the bin that holds the wanted rank extends the prefix; the last pass leaves the CE threshold
__global__ __launch_bounds__(256) void uce_ohem_pick_kernel(const unsigned* __restrict__ hist, unsigned* __restrict__ st,
                                                            long long kept, float nl_thresh, int pass) {
  __shared__ unsigned sh[256];
  sh[threadIdx.x] = hist[threadIdx.x];
  __syncthreads();
  if (threadIdx.x != 0) return;
  unsigned prefix = 0u, rank = 0u;
  if (pass == 0) {
    unsigned n = 0u;
    for (int i = 0; i < 256; ++i) n += sh[i];
    st[2] = n;
    // ascending rank of the min(kept, n - 1)-th largest value
    if (n) rank = (unsigned)((long long)n - 1 - (kept < (long long)n - 1 ? kept : (long long)n - 1));
  } else {
    prefix = st[0];
    rank = st[1];
  }
  unsigned cum = 0u;
  int b = 0;
  for (; b < 255; ++b) {
    if (rank < cum + sh[b]) break;
    cum += sh[b];
  }
  prefix |= (unsigned)b << (24 - 8 * pass);
  st[0] = prefix;
  st[1] = rank - cum;
  if (pass == 3)  // no valid pixel: nothing is greater than +inf
    st[3] = __float_as_uint(st[2] ? fminf(uce_unkey(prefix), nl_thresh) : __builtin_inff());
}

// pix_weight = [valid and nll > threshold] * cw[label], and sum pix_weight * nll.  The sum is formed as the forward kernel forms
// its own — "virtual" workgroup v of nvwg (the forward launch's grid) owns pixels v * 256 + t, + nvwg * 256, ... and leaves
// partial row v — so a sampler that keeps every valid pixel reproduces the unsampled sum bit for bit, at any grid size here.
__global__ __launch_bounds__(256) void uce_ohem_mask_kernel(const int64_t* __restrict__ label, const float* __restrict__ cw,
                                                            const float* __restrict__ nll, const unsigned* __restrict__ st,
                                                            float* __restrict__ pixw, float* __restrict__ part, long npix,
                                                            int C, int ignore, int nvwg) {
  __shared__ float red[4];
  const float thr = __uint_as_float(st[3]);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int v = blockIdx.x; v < nvwg; v += gridDim.x) {
    float loss = 0.f;
    for (long p = (long)v * 256 + threadIdx.x; p < npix; p += (long)nvwg * 256) {
      const long lab = label[p];
      const float nl = nll[p];
      float pw = 0.f;
      if (lab != ignore && nl > thr) pw = (cw && lab >= 0 && lab < C) ? cw[lab] : 1.f;
      pixw[p] = pw;
      loss = fmaf(pw, nl, loss);
    }
    loss = wave_sum(loss);
    __syncthreads();  // (the previous round's read of red)
    if (lane == 0) red[wv] = loss;
    __syncthreads();
    if (threadIdx.x == 0) part[(long)v * 3] = red[0] + red[1] + red[2] + red[3];
  }
}

// column 0 of upsample_ce_sums_kernel, in its order
__global__ __launch_bounds__(256) void uce_fold1_kernel(const float* __restrict__ part, float* __restrict__ out, int nparts) {
  float a = 0.f;
  for (int i = threadIdx.x; i < nparts; i += 256) a += part[(long)i * 3];
  __shared__ float red[4];
  a = wave_sum(a);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
  __syncthreads();
  if (threadIdx.x == 0) out[0] = red[0] + red[1] + red[2] + red[3];
}

// Masked-attention mask of the Mask2Former-style decoder (models/multi/seg_head/mask2former_head.py:126-136 and
// :177-178): mask logits (rows, h, w) -> bilinear resize to (th, tw) (align_corners=False) -> sigmoid < 0.5 ->
// rows that came out all-True are reset to all-False -> bool (rows, th*tw).  One workgroup per (image, query) row;
// replaces interpolate + sigmoid + compare + all + and-not (5 launches, 10 times per seg step).
__global__ __launch_bounds__(256) void seg_attn_mask_kernel(const float* __restrict__ pred, unsigned char* __restrict__ out,
                                                            int h, int w, int th, int tw) {
  __shared__ int s_any_false;
  const float* src = pred + (long)blockIdx.x * h * w;
  unsigned char* dst = out + (long)blockIdx.x * th * tw;
  const float sy = (float)h / (float)th, sx = (float)w / (float)tw;
  if (threadIdx.x == 0) s_any_false = 0;
  __syncthreads();
  bool any_false = false;
  for (int i = threadIdx.x; i < th * tw; i += 256) {
    const Interp iy = src_index(i / tw, sy, h), ix = src_index(i % tw, sx, w);
    const float v = iy.l0 * (ix.l0 * src[iy.i0 * w + ix.i0] + ix.l1 * src[iy.i0 * w + ix.i1]) +
                    iy.l1 * (ix.l0 * src[iy.i1 * w + ix.i0] + ix.l1 * src[iy.i1 * w + ix.i1]);
    const bool blocked = 1.f / (1.f + expf(-v)) < 0.5f;
    dst[i] = blocked ? 1 : 0;
    any_false |= !blocked;
  }
  if (any_false) s_any_false = 1;  // benign race: every writer stores 1
  __syncthreads();
  if (!s_any_false)
    for (int i = threadIdx.x; i < th * tw; i += 256) dst[i] = 0;
}

}  // namespace rscotr

using namespace rscotr;

extern "C" int rscotr_seg_attn_mask(const float* mask_pred, unsigned char* out, int rows, int h, int w, int th, int tw,
                                    void* stream) {
  if (rows < 0 || h <= 0 || w <= 0 || th <= 0 || tw <= 0) return fail(RSCOTR_E_SHAPE, "rscotr_seg_attn_mask: bad shape");
  if (rows == 0) return RSCOTR_OK;
  if (!mask_pred || !out) return fail(RSCOTR_E_ARG, "rscotr_seg_attn_mask: null pointer");
  seg_attn_mask_kernel<<<rows, 256, 0, (hipStream_t)stream>>>(mask_pred, out, h, w, th, tw);
  return check_launch("rscotr_seg_attn_mask");
}


// sums[3] = {sum of per-pixel CE over non-ignored pixels, #correct, #non-ignored}; lse (B,H,W) saved.
constexpr int UCE_MAX_WG = 4096;
extern "C" int64_t rscotr_upsample_ce_workspace(void) { return (int64_t)UCE_MAX_WG * 3 * 4; }

extern "C" int rscotr_upsample_ce_fwd(const float* logit, const int64_t* label, float* lse, float* sums, int B,
                                      int C, int h, int w, int H, int W, int ignore_index, float* workspace,
                                      int64_t workspace_bytes, void* stream) {
  if (int e = upsample_check_shape("rscotr_upsample_ce_fwd", B, C, h, w, H, W)) return e;
  if (!sums) return fail(RSCOTR_E_ARG, "rscotr_upsample_ce_fwd: null pointer");
  hipStream_t s = (hipStream_t)stream;
  if (B == 0) {
    hipMemsetAsync(sums, 0, 3 * sizeof(float), s);
    return RSCOTR_OK;
  }
  if (!logit || !label || !lse) return fail(RSCOTR_E_ARG, "rscotr_upsample_ce_fwd: null pointer");
  if (!workspace || workspace_bytes < rscotr_upsample_ce_workspace())
    return fail(RSCOTR_E_ARG, "rscotr_upsample_ce_fwd: workspace of rscotr_upsample_ce_workspace() bytes required");
  const long npix = (long)B * H * W;
  const int nwg = (int)std::min<long>((npix + 255) / 256, UCE_MAX_WG);
  upsample_ce_fwd_kernel<false><<<nwg, 256, 0, s>>>(logit, label, lse, workspace, B, C, h, w, H, W, ignore_index, nullptr, nullptr,
                                                    nullptr);
  upsample_ce_sums_kernel<<<1, 256, 0, s>>>(workspace, sums, nwg);
  return check_launch("rscotr_upsample_ce_fwd");
}

// dlogit (B,C,h,w) = grad_scale[0] * d(sum of per-pixel CE)/d(logit); grad_scale is a DEVICE scalar
// (upstream gradient / number of pixels), so no host sync is needed.
extern "C" int rscotr_upsample_ce_bwd(const float* logit, const int64_t* label, const float* lse,
                                      const float* grad_scale, float* dlogit, int B, int C, int h, int w, int H,
                                      int W, int ignore_index, void* stream) {
  if (int e = upsample_check_shape("rscotr_upsample_ce_bwd", B, C, h, w, H, W)) return e;
  if (B == 0) return RSCOTR_OK;
  if (!logit || !label || !lse || !grad_scale || !dlogit) return fail(RSCOTR_E_ARG, "rscotr_upsample_ce_bwd: null pointer");
  launch_upsample_gather<upsample_ce_bwd_kernel<false>, false>((hipStream_t)stream, B, h, w, logit, label, lse, grad_scale, dlogit, B,
                                                               C, h, w, H, W, ignore_index, nullptr);
  return check_launch("rscotr_upsample_ce_bwd");
}

// ---- class weights / avg_non_ignore / OHEM (additive entries; the two above are untouched) -------------------------------------
// workspace: the forward partial rows, then the select's histograms and state
extern "C" int64_t rscotr_upsample_ce_w_workspace(void) { return (int64_t)(UCE_MAX_WG * 3 + UCE_SEL_WORDS) * 4; }

extern "C" int rscotr_upsample_ce_w_fwd(const float* logit, const int64_t* label, const float* class_weight, float* lse,
                                        float* nll, float* pix_weight, float* sums, int B, int C, int h, int w, int H, int W,
                                        int ignore_index, float* workspace, int64_t workspace_bytes, void* stream) {
  if (int e = upsample_check_shape("rscotr_upsample_ce_w_fwd", B, C, h, w, H, W)) return e;
  if (!sums) return fail(RSCOTR_E_ARG, "rscotr_upsample_ce_w_fwd: null pointer");
  hipStream_t s = (hipStream_t)stream;
  if (B == 0) {
    hipMemsetAsync(sums, 0, 4 * sizeof(float), s);
    return RSCOTR_OK;
  }
  if (!logit || !label || !lse || !nll || !pix_weight) return fail(RSCOTR_E_ARG, "rscotr_upsample_ce_w_fwd: null pointer");
  if (!workspace || workspace_bytes < rscotr_upsample_ce_w_workspace())
    return fail(RSCOTR_E_ARG, "rscotr_upsample_ce_w_fwd: workspace of rscotr_upsample_ce_w_workspace() bytes required");
  const long npix = (long)B * H * W;
  const int nwg = (int)std::min<long>((npix + 255) / 256, UCE_MAX_WG);  // (the unweighted launch's grid: same summation order)
  upsample_ce_fwd_kernel<true><<<nwg, 256, 0, s>>>(logit, label, lse, workspace, B, C, h, w, H, W, ignore_index, class_weight, nll,
                                                   pix_weight);
  upsample_ce_sums_kernel<<<1, 256, 0, s>>>(workspace, sums, nwg);
  return check_launch("rscotr_upsample_ce_w_fwd");
}

extern "C" int rscotr_upsample_ce_ohem(const int64_t* label, const float* class_weight, const float* nll, float* pix_weight,
                                       float* sum_out, int64_t npix, int C, int ignore_index, int64_t kept, float nll_thresh,
                                       float* workspace, int64_t workspace_bytes, void* stream) {
  if (npix < 0 || npix > 0x7fffffffLL || C <= 0) return fail(RSCOTR_E_SHAPE, "rscotr_upsample_ce_ohem: bad shape");
  if (kept < 0 || nll_thresh != nll_thresh) return fail(RSCOTR_E_ARG, "rscotr_upsample_ce_ohem: kept >= 0 and a threshold required");
  if (!sum_out) return fail(RSCOTR_E_ARG, "rscotr_upsample_ce_ohem: null pointer");
  hipStream_t s = (hipStream_t)stream;
  if (npix == 0) {
    hipMemsetAsync(sum_out, 0, sizeof(float), s);
    return RSCOTR_OK;
  }
  if (!label || !nll || !pix_weight) return fail(RSCOTR_E_ARG, "rscotr_upsample_ce_ohem: null pointer");
  if (!workspace || workspace_bytes < rscotr_upsample_ce_w_workspace())
    return fail(RSCOTR_E_ARG, "rscotr_upsample_ce_ohem: workspace of rscotr_upsample_ce_w_workspace() bytes required");
  unsigned* hist = reinterpret_cast<unsigned*>(workspace) + UCE_MAX_WG * 3;
  unsigned* st = hist + 4 * 256;
  hipMemsetAsync(hist, 0, UCE_SEL_WORDS * sizeof(unsigned), s);
  const int nsel = (int)std::min<long>((npix + 255) / 256, UCE_SEL_WG);
  for (int pass = 0; pass < 4; ++pass) {
    uce_ohem_hist_kernel<<<nsel, 256, 0, s>>>(label, nll, hist + pass * 256, st, npix, ignore_index, pass);
    uce_ohem_pick_kernel<<<1, 256, 0, s>>>(hist + pass * 256, st, (long long)kept, nll_thresh, pass);
  }
  const int nvwg = (int)std::min<long>((npix + 255) / 256, UCE_MAX_WG);
  uce_ohem_mask_kernel<<<nsel, 256, 0, s>>>(label, class_weight, nll, st, pix_weight, workspace, npix, C, ignore_index, nvwg);
  uce_fold1_kernel<<<1, 256, 0, s>>>(workspace, sum_out, nvwg);
  return check_launch("rscotr_upsample_ce_ohem");
}

extern "C" int rscotr_upsample_ce_w_bwd(const float* logit, const int64_t* label, const float* lse, const float* pix_weight,
                                        const float* grad_scale, float* dlogit, int B, int C, int h, int w, int H, int W,
                                        int ignore_index, void* stream) {
  if (int e = upsample_check_shape("rscotr_upsample_ce_w_bwd", B, C, h, w, H, W)) return e;
  if (B == 0) return RSCOTR_OK;
  if (!logit || !label || !lse || !pix_weight || !grad_scale || !dlogit)
    return fail(RSCOTR_E_ARG, "rscotr_upsample_ce_w_bwd: null pointer");
  launch_upsample_gather<upsample_ce_bwd_kernel<true>, true>((hipStream_t)stream, B, h, w, logit, label, lse, grad_scale, dlogit, B, C,
                                                             h, w, H, W, ignore_index, pix_weight);
  return check_launch("rscotr_upsample_ce_w_bwd");
}
