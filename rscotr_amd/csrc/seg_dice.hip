// Fused bilinear-upsample + softmax + Dice loss for the seg head (gfx950): mmseg 0.28 DiceLoss as BaseDecodeHead.losses reaches it.
//
//   u = resize(seg_logit (B,C,h,w), size=label.shape, mode='bilinear', align_corners=False);  p = softmax(u, dim=1)
//   t[b,c,.] = [clamp(label, 0, C-1) == c]     (an ignored 255 lands in channel C-1)       v[b,.] = [label != ignore_index]
//   num[b,c] = 2 * sum_pix p t v + smooth      den[b,c] = sum_pix (p^2 + t) + smooth       (den is NOT masked: mmseg's quirk)
//   loss = loss_weight / C * sum_{c != ignore_index} class_weight[c] * mean_b (1 - num / den)
//
// As in seg_loss.hip, neither the up-sampled logits nor the probabilities exist in memory: a pixel's interpolated logits
// live in registers.  Unlike the cross-entropy, a pixel's gradient depends on sums over its whole image, so:
//   forward   upsample_dice_fwd_kernel   one thread per pixel, a workgroup stays inside one image: log-sum-exp per pixel
//                                        (saved), then the classes once more, DICE_CT at a time in registers, for
//                                        sum p t v, sum p^2 and sum t; one partial row per workgroup and class pass
//             upsample_dice_coef_kernel  folds the rows in fixed order, forms num / den, the loss, and the two backward
//                                        coefficients of every (image, class):  a = -2k / den,  bcoef = 2k num / den^2,
//                                        k = loss_weight * class_weight[c] / (C * B)  (0 for the skipped channel)
//   backward  upsample_dice_s_kernel     S(pix) = sum_c g_c p_c with g_c = a t v + bcoef p_c, one thread per pixel
//             upsample_dice_bwd_kernel   the blocked gather of upsample_ce_bwd_kernel with p (g_c - S) in place of
//                                        softmax - one-hot; an ignored pixel is NOT skipped (it acts through p^2 in den)
// No float atomics, every sum in a fixed order: two runs are bit-equal.  Nothing synchronises with the host.
#include <algorithm>

#include "seg_upsample.h"

namespace rscotr {

constexpr int DICE_CT = 16;       // classes of one register pass of the forward kernel
constexpr int DICE_CHUNKS = 128;  // workgroups per image at most (8 pixels per thread at 512 x 512)

__global__ __launch_bounds__(256) void upsample_dice_fwd_kernel(const float* __restrict__ logit,
                                                                const int64_t* __restrict__ label, float* lse,
                                                                float* __restrict__ part, int C, int h, int w, int H, int W,
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
    const Interp iy = src_index(i / W, sy, h), ix = src_index(i % W, sx, w);
    const float w00 = iy.l0 * ix.l0, w01 = iy.l0 * ix.l1, w10 = iy.l1 * ix.l0, w11 = iy.l1 * ix.l1;
    const int o00 = iy.i0 * w + ix.i0, o01 = iy.i0 * w + ix.i1, o10 = iy.i1 * w + ix.i0, o11 = iy.i1 * w + ix.i1;
    float m = -3.0e38f, s = 0.f;
    for (int c = 0; c < C; ++c) {
      const float* pc = base + (long)c * h * w;
      const float v = w00 * pc[o00] + w01 * pc[o01] + w10 * pc[o10] + w11 * pc[o11];
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
      const Interp iy = src_index(i / W, sy, h), ix = src_index(i % W, sx, w);
      const float w00 = iy.l0 * ix.l0, w01 = iy.l0 * ix.l1, w10 = iy.l1 * ix.l0, w11 = iy.l1 * ix.l1;
      const int o00 = iy.i0 * w + ix.i0, o01 = iy.i0 * w + ix.i1, o10 = iy.i1 * w + ix.i0, o11 = iy.i1 * w + ix.i1;
      const long lab = lab_b[i];
      const int lc = (int)std::min<long>(std::max<long>(lab, 0), C - 1);  // the CLAMPED label: never an index
      const float valid = lab != ignore ? 1.f : 0.f;
      const float l = lse_b[i];
#pragma unroll
      for (int j = 0; j < DICE_CT; ++j) {
        const int c = c0 + j;
        if (c < C) {  // (uniform)
          const float* pc = base + (long)c * h * w;
          const float p = __expf(w00 * pc[o00] + w01 * pc[o01] + w10 * pc[o10] + w11 * pc[o11] - l);
          aP[j] = fmaf(p, p, aP[j]);
          if (c == lc) { aI[j] = fmaf(p, valid, aI[j]); aT[j] += 1.f; }
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
    if (tid < 3 * DICE_CT) {  // partial row [b][k][{p t v, p^2, t}][C], folded in fixed order by upsample_dice_coef_kernel
      const int q = tid / DICE_CT, c = c0 + tid % DICE_CT;
      if (c < C) part[(((long)b * nchunk + k) * 3 + q) * C + c] = red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
    }
  }
}

// one workgroup: fold, num / den, the backward coefficients (without the upstream gradient) and the loss
__global__ __launch_bounds__(256) void upsample_dice_coef_kernel(const float* __restrict__ part, const float* __restrict__ cw,
                                                                 float* __restrict__ coef, float* __restrict__ loss, int B, int C,
                                                                 int nchunk, int ignore, float smooth, float loss_weight) {
  double acc = 0.0;
  for (int i = threadIdx.x; i < B * C; i += 256) {
    const int b = i / C, c = i % C;
    float s[3] = {0.f, 0.f, 0.f};
    for (int k = 0; k < nchunk; ++k)
#pragma unroll
      for (int q = 0; q < 3; ++q) s[q] += part[(((long)b * nchunk + k) * 3 + q) * C + c];
    const double num = 2.0 * (double)s[0] + (double)smooth, den = (double)s[1] + (double)s[2] + (double)smooth;
    const double kk = c == ignore ? 0.0 : (double)(cw ? cw[c] : 1.f) * (double)loss_weight / ((double)C * (double)B);
    coef[2 * i] = (float)(-2.0 * kk / den);
    coef[2 * i + 1] = (float)(2.0 * kk * num / (den * den));
    acc += kk * ((den - num) / den);
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

// S(pix) = a[b, label] v p_label + sum_c bcoef[b, c] p_c^2: one thread per pixel, the classes streamed once more
__global__ __launch_bounds__(256) void upsample_dice_s_kernel(const float* __restrict__ logit, const int64_t* __restrict__ label,
                                                              const float* __restrict__ lse, const float* __restrict__ coef,
                                                              float* __restrict__ pix_s, int B, int C, int h, int w, int H, int W,
                                                              int ignore) {
  const long npix = (long)B * H * W;
  const float sy = (float)h / (float)H, sx = (float)w / (float)W;
  for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < npix; p += (long)gridDim.x * 256) {
    const int x = (int)(p % W), y = (int)((p / W) % H), b = (int)(p / ((long)W * H));
    const Interp iy = src_index(y, sy, h), ix = src_index(x, sx, w);
    const float w00 = iy.l0 * ix.l0, w01 = iy.l0 * ix.l1, w10 = iy.l1 * ix.l0, w11 = iy.l1 * ix.l1;
    const float* base = logit + (long)b * C * h * w;
    const float2* cf = reinterpret_cast<const float2*>(coef) + (long)b * C;
    const int o00 = iy.i0 * w + ix.i0, o01 = iy.i0 * w + ix.i1, o10 = iy.i1 * w + ix.i0, o11 = iy.i1 * w + ix.i1;
    const long lab = label[p];
    const int lc = (int)std::min<long>(std::max<long>(lab, 0), C - 1);
    const float valid = lab != ignore ? 1.f : 0.f;
    const float l = lse[p];
    float s = 0.f;
    for (int c = 0; c < C; ++c) {
      const float* pc = base + (long)c * h * w;
      const float q = __expf(w00 * pc[o00] + w01 * pc[o01] + w10 * pc[o10] + w11 * pc[o11] - l);
      const float2 ab = cf[c];
      s = fmaf(fmaf(ab.y, q, c == lc ? ab.x * valid : 0.f), q, s);
    }
    pix_s[p] = s;
  }
}

// dlogit[b,c,cy,cx] = scale * sum over output pixels p touching the cell of  wt(p->cell) * p_c (a t v + bcoef p_c - S(p)).
// The structure, the LDS layout and the staging are upsample_ce_bwd_kernel<true>'s (seg_loss.hip: 512 threads = 4 row
// groups x 128 class lanes over a UCE_TB x UCE_TB block of cells); what differs: a lane holds its class's two coefficients
// in registers, the staged pixel record is {clamped label, or -1 where ignored; log-sum-exp * log2 e} plus S in the weight
// plane's place, and no pixel is skipped.
__global__ __launch_bounds__(512) void upsample_dice_bwd_kernel(const float* __restrict__ logit,
                                                                const int64_t* __restrict__ label,
                                                                const float* __restrict__ lse,
                                                                const float* __restrict__ coef,
                                                                const float* __restrict__ pix_s,
                                                                const float* __restrict__ gscale, float* __restrict__ dlogit,
                                                                int B, int C, int h, int w, int H, int W, int ignore) {
  extern __shared__ __attribute__((aligned(16))) float dice_smem[];
  float* sN = dice_smem;                                 // [UCE_NB * UCE_NB][128]   neighbourhood logits of the 128 classes of a pass
  float* sAcc = sN + UCE_NB * UCE_NB * 128;              // [4 groups][UCE_TB * UCE_TB][128]
  int2* sLL = reinterpret_cast<int2*>(sAcc + 4 * UCE_TB * UCE_TB * 128);  // [UCE_FP * UCE_FP] {label or -1, bits of lse * log2 e}
  float* sYl = reinterpret_cast<float*>(sLL + UCE_FP * UCE_FP);    // [UCE_FP][2]  l0, l1 of a footprint row
  int* sYi = reinterpret_cast<int*>(sYl + 2 * UCE_FP);   // [UCE_FP][2]  i0, i1 relative to the block's first cell - 1
  int4* sXT = reinterpret_cast<int4*>(sYi + 2 * UCE_FP);  // [UCE_FP] {i0, i1 (same origin), bits of l0, l1} of a footprint column
  float* sS = reinterpret_cast<float*>(sXT + UCE_FP);    // [UCE_FP * UCE_FP] S of a footprint pixel
  const int bw = (w + UCE_TB - 1) / UCE_TB, bh = (h + UCE_TB - 1) / UCE_TB;
  const int blk = blockIdx.x;
  const int cx0 = (blk % bw) * UCE_TB, cy0 = ((blk / bw) % bh) * UCE_TB, b = blk / (bw * bh);
  const float sy = (float)h / (float)H, sx = (float)w / (float)W;
  // output rows / columns whose taps can include a cell of the block: source coordinate in (c0 - 1, c0 + TB)
  const int y_lo = max(0, (int)floorf(((float)cy0 - 1.f + 0.5f) / sy - 0.5f));
  const int y_hi = min(H - 1, (int)ceilf(((float)(cy0 + UCE_TB) + 0.5f) / sy - 0.5f));
  const int x_lo = max(0, (int)floorf(((float)cx0 - 1.f + 0.5f) / sx - 0.5f));
  const int x_hi = min(W - 1, (int)ceilf(((float)(cx0 + UCE_TB) + 0.5f) / sx - 0.5f));
  const int ny = y_hi - y_lo + 1, nx = x_hi - x_lo + 1;
  const bool staged = ny <= UCE_FP && nx <= UCE_FP;  // uniform
  const int tid = threadIdx.x, lane = tid & 127, grp = tid >> 7;
  const float* base = logit + (long)b * C * h * w;
  const float scale = gscale[0];
  if (staged) {
    for (int i = tid; i < ny * nx; i += 512) {
      const long p = ((long)b * H + y_lo + i / nx) * W + x_lo + i % nx;
      const long lab = label[p];
      const int lc = lab != ignore ? (int)std::min<long>(std::max<long>(lab, 0), C - 1) : -1;
      sS[i] = pix_s[p];
      sLL[i] = make_int2(lc, __float_as_int(lse[p] * 1.4426950408889634f));  // (the staged path works in the log2 domain)
    }
  }
  for (int i = tid; i < min(ny, UCE_FP); i += 512) {
    const Interp iy = src_index(y_lo + i, sy, h);
    sYl[2 * i] = iy.l0; sYl[2 * i + 1] = iy.l1;
    sYi[2 * i] = iy.i0 - cy0 + 1; sYi[2 * i + 1] = iy.i1 - cy0 + 1;
  }
  for (int i = tid; i < min(nx, UCE_FP); i += 512) {
    const Interp ix = src_index(x_lo + i, sx, w);
    sXT[i] = make_int4(ix.i0 - cx0 + 1, ix.i1 - cx0 + 1, __float_as_int(ix.l0), __float_as_int(ix.l1));
  }
  for (int c0 = 0; c0 < C; c0 += 128) {
    const int c = c0 + lane;
    __syncthreads();
    // neighbourhood (cells cy0 - 1 .. cy0 + TB, cx0 - 1 .. cx0 + TB; zeros outside the map: never weighted) of this pass's classes
    for (int k = grp; k < UCE_NB * UCE_NB; k += 4) {
      const int ny_ = cy0 + k / UCE_NB - 1, nx_ = cx0 + k % UCE_NB - 1;
      sN[k * 128 + lane] = (c < C && ny_ >= 0 && ny_ < h && nx_ >= 0 && nx_ < w) ? base[(long)c * h * w + ny_ * w + nx_] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < UCE_TB * UCE_TB; ++k) sAcc[(grp * UCE_TB * UCE_TB + k) * 128 + lane] = 0.f;
    float ca = 0.f, cb = 0.f;  // this lane's class: a and bcoef of (b, c)
    if (c < C) { ca = coef[((long)b * C + c) * 2]; cb = coef[((long)b * C + c) * 2 + 1]; }
    __syncthreads();
    if (c < C && staged) {
      // Staged footprints (the step's shapes): the pixel-only quantities are wave-uniform and read to scalar registers; the
      // footprint columns are walked one column pair at a time (see upsample_ce_bwd_kernel)
      float* acc = sAcc + grp * UCE_TB * UCE_TB * 128 + lane;
      auto sc = [](int v) { return __builtin_amdgcn_readfirstlane(v); };
      auto scf = [](float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); };
      int xs[UCE_TB + 2];  // xs[k] = first footprint column whose first tap is block column >= k - 1 (columns ascend with xx)
#pragma unroll
      for (int k = 0; k < UCE_TB + 2; ++k) xs[k] = 0;
      for (int xx = 0; xx < nx; ++xx) {
        const int kx0 = sc(sXT[xx].x);
#pragma unroll
        for (int k = 0; k < UCE_TB + 2; ++k) xs[k] += kx0 < k ? 1 : 0;
      }
      for (int r = grp; r < ny; r += 4) {
        const int ky0 = sc(sYi[2 * r]), ky1 = sc(sYi[2 * r + 1]);
        const float yl0 = scf(sYl[2 * r]), yl1 = scf(sYl[2 * r + 1]);
        const bool in0 = ky0 >= 1 && ky0 <= UCE_TB && cy0 + ky0 - 1 < h, in1 = ky1 >= 1 && ky1 <= UCE_TB && cy0 + ky1 - 1 < h;
        if (!in0 && !in1) continue;
        const int b0 = min(max(ky0, 0), UCE_NB - 1), b1 = min(max(ky1, 0), UCE_NB - 1);
        const int2* llr = sLL + r * nx;
        const float* ssr = sS + r * nx;
        float cs[UCE_TB + 2];  // column sums of this row by block column + 1 (0 and TB + 1: the halo, dropped)
#pragma unroll
        for (int k = 0; k < UCE_TB + 2; ++k) cs[k] = 0.f;
#pragma unroll
        for (int k = 0; k <= UCE_TB; ++k) {  // pairs (k, k + 1); at the far edge of the map (k, k)
          const int x0 = xs[k], x1 = xs[k + 1];
          if (x0 == x1) continue;  // (uniform)
          const int kx1 = sc(sXT[x0].y);
          const int a1 = min(max(kx1, 0), UCE_NB - 1);
          const float n00 = sN[(b0 * UCE_NB + k) * 128 + lane], n01 = sN[(b0 * UCE_NB + a1) * 128 + lane];
          const float n10 = sN[(b1 * UCE_NB + k) * 128 + lane], n11 = sN[(b1 * UCE_NB + a1) * 128 + lane];
          const float A0 = (yl0 * n00 + yl1 * n10) * 1.4426950408889634f;
          const float A1 = (yl0 * n01 + yl1 * n11) * 1.4426950408889634f;
          float s0 = 0.f, s1 = 0.f;
          int4 xt_n = sXT[x0];
          int2 ll_n = llr[x0];
          float ss_n = ssr[x0];
          for (int xx = x0; xx < x1; ++xx) {
            const int4 xt = xt_n;
            const int2 ll = ll_n;
            const float ss = ss_n;
            const int xn = min(xx + 1, nx - 1);
            xt_n = sXT[xn];
            ll_n = llr[xn];
            ss_n = ssr[xn];
            const int lab = sc(ll.x);
            const float xl0 = __int_as_float(sc(xt.z)), xl1 = __int_as_float(sc(xt.w));
            const float ls = __int_as_float(sc(ll.y));
            const float p = __builtin_amdgcn_exp2f(fmaf(xl1, A1, fmaf(xl0, A0, -ls)));
            const float gq = p * (fmaf(cb, p, c == lab ? ca : 0.f) - scf(ss));
            s0 = fmaf(xl0, gq, s0);
            s1 = fmaf(xl1, gq, s1);
          }
          cs[k] += s0;
          if (kx1 == k) cs[k] += s1; else cs[k + 1] += s1;  // (uniform)
        }
#pragma unroll
        for (int k = 1; k <= UCE_TB; ++k) {
          if (cx0 + k - 1 < w) {
            if (in0) acc[((ky0 - 1) * UCE_TB + k - 1) * 128] += yl0 * cs[k];
            if (in1) acc[((ky1 - 1) * UCE_TB + k - 1) * 128] += yl1 * cs[k];
          }
        }
      }
    } else if (c < C) {
      float* acc = sAcc + grp * UCE_TB * UCE_TB * 128 + lane;
      for (int r = grp; r < ny; r += 4) {
        int ky0, ky1;
        float yl0, yl1;
        if (r < UCE_FP) { ky0 = sYi[2 * r]; ky1 = sYi[2 * r + 1]; yl0 = sYl[2 * r]; yl1 = sYl[2 * r + 1]; }
        else { const Interp iy = src_index(y_lo + r, sy, h); ky0 = iy.i0 - cy0 + 1; ky1 = iy.i1 - cy0 + 1; yl0 = iy.l0; yl1 = iy.l1; }
        // (a row whose both taps lie outside the block contributes nothing; the footprint bounds are conservative)
        const bool in0 = ky0 >= 1 && ky0 <= UCE_TB && cy0 + ky0 - 1 < h, in1 = ky1 >= 1 && ky1 <= UCE_TB && cy0 + ky1 - 1 < h;
        if (!in0 && !in1) continue;
        float t00 = 0.f, t01 = 0.f, t10 = 0.f, t11 = 0.f;
        int cur0 = -100, cur1 = -100;
        auto flush = [&]() {
          if (cur0 == -100) return;
          const bool jx0 = cur0 >= 1 && cur0 <= UCE_TB && cx0 + cur0 - 1 < w, jx1 = cur1 >= 1 && cur1 <= UCE_TB && cx0 + cur1 - 1 < w;
          if (in0 && jx0) acc[((ky0 - 1) * UCE_TB + cur0 - 1) * 128] += t00;
          if (in0 && jx1) acc[((ky0 - 1) * UCE_TB + cur1 - 1) * 128] += t01;
          if (in1 && jx0) acc[((ky1 - 1) * UCE_TB + cur0 - 1) * 128] += t10;
          if (in1 && jx1) acc[((ky1 - 1) * UCE_TB + cur1 - 1) * 128] += t11;
          t00 = t01 = t10 = t11 = 0.f;
        };
        float n00 = 0.f, n01 = 0.f, n10 = 0.f, n11 = 0.f;
        for (int xx = 0; xx < nx; ++xx) {
          int kx0, kx1;
          float xl0, xl1;
          if (xx < UCE_FP) { const int4 xt = sXT[xx]; kx0 = xt.x; kx1 = xt.y; xl0 = __int_as_float(xt.z); xl1 = __int_as_float(xt.w); }
          else { const Interp ix = src_index(x_lo + xx, sx, w); kx0 = ix.i0 - cx0 + 1; kx1 = ix.i1 - cx0 + 1; xl0 = ix.l0; xl1 = ix.l1; }
          if (kx0 != cur0 || kx1 != cur1) {  // a new column pair: fold the finished one, fetch this one's four cell logits
            flush();
            cur0 = kx0; cur1 = kx1;
            const int a0 = min(max(kx0, 0), UCE_NB - 1), a1 = min(max(kx1, 0), UCE_NB - 1);
            const int b0 = min(max(ky0, 0), UCE_NB - 1), b1 = min(max(ky1, 0), UCE_NB - 1);
            n00 = sN[(b0 * UCE_NB + a0) * 128 + lane]; n01 = sN[(b0 * UCE_NB + a1) * 128 + lane];
            n10 = sN[(b1 * UCE_NB + a0) * 128 + lane]; n11 = sN[(b1 * UCE_NB + a1) * 128 + lane];
          }
          const long p = ((long)b * H + y_lo + r) * W + x_lo + xx;  // (footprints past the staged size)
          const long lab = label[p];
          const bool hit = lab != ignore && (long)c == std::min<long>(std::max<long>(lab, 0), C - 1);
          const float v = yl0 * (xl0 * n00 + xl1 * n01) + yl1 * (xl0 * n10 + xl1 * n11);
          const float q = __expf(v - lse[p]);
          const float gq = q * (fmaf(cb, q, hit ? ca : 0.f) - pix_s[p]);
          t00 += yl0 * xl0 * gq; t01 += yl0 * xl1 * gq; t10 += yl1 * xl0 * gq; t11 += yl1 * xl1 * gq;
        }
        flush();
      }
    }
    __syncthreads();
    // the four row groups meet in fixed order; thread (grp, lane) writes block rows grp of class lane
    if (c < C && cy0 + grp < h) {
      float* drow = dlogit + ((long)b * C + c) * h * w + (long)(cy0 + grp) * w + cx0;
#pragma unroll
      for (int k = 0; k < UCE_TB; ++k) {
        if (cx0 + k < w) {
          float v = 0.f;
#pragma unroll
          for (int g2 = 0; g2 < 4; ++g2) v += sAcc[((g2 * UCE_TB + grp) * UCE_TB + k) * 128 + lane];
          drow[k] = v * scale;
        }
      }
    }
  }
}

constexpr size_t dice_bwd_lds_bytes() {
  return (size_t)(UCE_NB * UCE_NB * 128 + 4 * UCE_TB * UCE_TB * 128 + 3 * UCE_FP * UCE_FP + 8 * UCE_FP) * 4;
}
static_assert(2 * dice_bwd_lds_bytes() <= 160 * 1024, "two backward workgroups per CU");

static int dice_chunks(int H, int W) { return (int)std::min<long>(((long)H * W + 255) / 256, DICE_CHUNKS); }

}  // namespace rscotr

using namespace rscotr;

// the forward partial rows: [B][chunks <= DICE_CHUNKS][3][C] floats
extern "C" int64_t rscotr_upsample_dice_workspace(int B, int C) {
  return (int64_t)std::max(B, 0) * DICE_CHUNKS * 3 * std::max(C, 0) * 4;
}

extern "C" int rscotr_upsample_dice_fwd(const float* logit, const int64_t* label, const float* class_weight, float* lse,
                                        float* coef, float* loss, int B, int C, int h, int w, int H, int W, int ignore_index,
                                        float smooth, float loss_weight, float* workspace, int64_t workspace_bytes,
                                        void* stream) {
  if (B < 0 || C <= 0 || h <= 0 || w <= 0 || H <= 0 || W <= 0)
    return fail(RSCOTR_E_SHAPE, "rscotr_upsample_dice_fwd: bad shape");
  if ((long)H * W > (1L << 24))  // the label counts are float sums: exact below 2^24
    return fail(RSCOTR_E_SHAPE, "rscotr_upsample_dice_fwd: more than 2^24 pixels per image");
  if ((long)B * C > 0x3fffffffL || (long)C * h * w > 0x7fffffffL)
    return fail(RSCOTR_E_SHAPE, "rscotr_upsample_dice_fwd: shape too large");
  if (!loss) return fail(RSCOTR_E_ARG, "rscotr_upsample_dice_fwd: null pointer");
  hipStream_t s = (hipStream_t)stream;
  if (B == 0) {
    (void)hipMemsetAsync(loss, 0, sizeof(float), s);
    return RSCOTR_OK;
  }
  if (!logit || !label || !lse || !coef) return fail(RSCOTR_E_ARG, "rscotr_upsample_dice_fwd: null pointer");
  if (!workspace || workspace_bytes < rscotr_upsample_dice_workspace(B, C))
    return fail(RSCOTR_E_ARG, "rscotr_upsample_dice_fwd: workspace of rscotr_upsample_dice_workspace(B, C) bytes required");
  const int nchunk = dice_chunks(H, W);
  if ((long)B * nchunk > 0x7fffffffL) return fail(RSCOTR_E_SHAPE, "rscotr_upsample_dice_fwd: batch too large");
  upsample_dice_fwd_kernel<<<B * nchunk, 256, 0, s>>>(logit, label, lse, workspace, C, h, w, H, W, ignore_index, nchunk);
  upsample_dice_coef_kernel<<<1, 256, 0, s>>>(workspace, class_weight, coef, loss, B, C, nchunk, ignore_index, smooth,
                                              loss_weight);
  return check_launch("rscotr_upsample_dice_fwd");
}

// dlogit (B,C,h,w) = grad_scale[0] * d(loss)/d(logit); grad_scale is a DEVICE scalar (the upstream gradient); pix_s (B,H,W) is
// the caller's scratch plane for S
extern "C" int rscotr_upsample_dice_bwd(const float* logit, const int64_t* label, const float* lse, const float* coef,
                                        const float* grad_scale, float* pix_s, float* dlogit, int B, int C, int h, int w,
                                        int H, int W, int ignore_index, void* stream) {
  if (B < 0 || C <= 0 || h <= 0 || w <= 0 || H <= 0 || W <= 0)
    return fail(RSCOTR_E_SHAPE, "rscotr_upsample_dice_bwd: bad shape");
  if (B == 0) return RSCOTR_OK;
  if (!logit || !label || !lse || !coef || !grad_scale || !pix_s || !dlogit)
    return fail(RSCOTR_E_ARG, "rscotr_upsample_dice_bwd: null pointer");
  static_assert(UCE_TB == 4, "four row groups write the four cell rows of a block");
  static const bool attr_set = [] {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(upsample_dice_bwd_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                        (int)dice_bwd_lds_bytes());
    return true;
  }();
  (void)attr_set;
  hipStream_t s = (hipStream_t)stream;
  const long npix = (long)B * H * W;
  const int nwg = (int)std::min<long>((npix + 255) / 256, 4096);
  upsample_dice_s_kernel<<<nwg, 256, 0, s>>>(logit, label, lse, coef, pix_s, B, C, h, w, H, W, ignore_index);
  const int nblk = B * ((h + UCE_TB - 1) / UCE_TB) * ((w + UCE_TB - 1) / UCE_TB);
  upsample_dice_bwd_kernel<<<nblk, 512, dice_bwd_lds_bytes(), s>>>(logit, label, lse, coef, pix_s, grad_scale, dlogit, B, C, h, w,
                                                                  H, W, ignore_index);
  return check_launch("rscotr_upsample_dice_bwd");
}
