// Bilinear resize (align_corners=False) for the fused seg losses (csrc/seg_loss.hip: cross-entropy, csrc/seg_dice.hip: Dice
// and Tversky, csrc/seg_focal.hip: sigmoid focal, csrc/seg_lovasz.hip: Lovasz-softmax) and the masked-attention mask: the source index, the 2 x 2 taps of an output
// pixel, the blocked backward gather that every loss instantiates with its own gradient term, and the host helpers of their
// entries.
//
// PyTorch's upsample_bilinear2d (align_corners=False) source index: s = max((d + 0.5) * in/out - 0.5, 0),
// i0 = floor(s), i1 = min(i0 + 1, in - 1), lambda1 = s - i0.
#pragma once
#include <type_traits>

#include "common.h"

namespace rscotr {

struct Interp {
  int i0, i1;
  float l0, l1;
};

__device__ __forceinline__ Interp src_index(int d, float scale, int in) {
  Interp r;
  const float s = fmaxf(((float)d + 0.5f) * scale - 0.5f, 0.f);
  r.i0 = min((int)s, in - 1);
  r.i1 = min(r.i0 + 1, in - 1);
  r.l1 = s - (float)r.i0;
  r.l0 = 1.f - r.l1;
  return r;
}

// The four taps of output pixel (y, x) on an h x w plane: weights and offsets, and the interpolated value of a plane.
struct Taps {
  float w00, w01, w10, w11;
  int o00, o01, o10, o11;
  __device__ __forceinline__ Taps(int y, int x, float sy, float sx, int h, int w) {
    const Interp iy = src_index(y, sy, h), ix = src_index(x, sx, w);
    w00 = iy.l0 * ix.l0; w01 = iy.l0 * ix.l1; w10 = iy.l1 * ix.l0; w11 = iy.l1 * ix.l1;
    o00 = iy.i0 * w + ix.i0; o01 = iy.i0 * w + ix.i1; o10 = iy.i1 * w + ix.i0; o11 = iy.i1 * w + ix.i1;
  }
  __device__ __forceinline__ float at(const float* __restrict__ pc) const {
    return w00 * pc[o00] + w01 * pc[o01] + w10 * pc[o10] + w11 * pc[o11];
  }
};

// dlogit[b,c,cy,cx] = scale * sum over output pixels p touching the cell of  wt(p->cell) * term_c(p), term_c(p) the loss's
// d(loss)/d(interpolated logit c of p): softmax_c(p) - [c == label_p] for the cross-entropy.
// Round 5: one workgroup per BLOCK of UCE_TB x UCE_TB low-resolution cells instead of one per cell.  The output pixels whose
// 2 x 2 tap footprint meets the block — (UCE_TB + 1) * 8 = 40 per axis at the step's x8 resize, 1.56 x the pixels the block
// owns — are visited ONCE per class (the per-cell kernel visited every pixel from each of the four cells it touches and
// re-interpolated its logits each time: 245 us at 2 x 100 x 64 x 64 -> 512^2).  512 threads = 4 row groups x 128 class lanes:
// group g takes the footprint rows y_lo + g, + 4, ...; a lane keeps the four cell sums of the current (row pair, column
// pair) in registers and folds them into its private LDS column when the column pair changes (every ~8 pixels); the
// (UCE_TB + 2)^2 cell neighbourhood of all classes, the labels and log-sum-exps of the footprint and the row / column
// interpolation tables are staged in LDS once.  The four groups meet in fixed order: no atomics, bit-reproducible.
constexpr int UCE_TB = 4;    // cells per block edge
constexpr int UCE_NB = UCE_TB + 2;
constexpr int UCE_FP = 48;   // staged footprint rows / columns (40 at x8); larger footprints read labels / lse from global memory
static_assert(UCE_TB == 4, "four row groups write the four cell rows of a block");

// dynamic LDS of a gather workgroup; plane: the loss stages a float per footprint pixel next to {label, lse} (Term::PLANE)
constexpr size_t upsample_gather_lds_bytes(bool plane) {
  return (size_t)(UCE_NB * UCE_NB * 128 + 4 * UCE_TB * UCE_TB * 128 + 2 * UCE_FP * UCE_FP + 8 * UCE_FP +
                  (plane ? UCE_FP * UCE_FP : 0)) * 4;
}
static_assert(2 * upsample_gather_lds_bytes(true) <= 160 * 1024, "two backward workgroups per CU");

// The body of a __launch_bounds__(512) kernel with upsample_gather_lds_bytes(Term::PLANE) bytes of dynamic LDS, one workgroup
// per block of cells.  Term is what a loss supplies:
//   static constexpr bool PLANE           a per-pixel float is staged with the label (a weight, a per-pixel sum)
//   static constexpr bool RAW             term() takes the interpolated logit u_c(p) itself instead of softmax_c(p) (a per-element
//                                         loss: the sigmoid focal, where exp(u) overflows and a sigmoid does not); `lse` is then
//                                         never read and may be null
//   void  load_class(b, c)                this lane's class constants of image b (c may be >= C)
//   int   stage(p, float& plane)          the label output pixel p is staged with, and its plane value (PLANE only)
//   bool  skip(lab)                       a pixel staged with this label contributes nothing
//   float term(prob, c, lab, plane)       the gradient term of class c from prob = softmax_c(p) (RAW: from u_c(p))
//   static constexpr bool PIXEL           (optional, absent = false) term() takes the flat output-pixel index (b * H + y) * W + x
//                                         as a fifth argument: a loss whose gradient reads a per-(class, pixel) plane (Lovasz)
// Both implementations below — the staged walk and the one for footprints past UCE_FP — call the same stage / skip / term.
template <class T, class = void>
struct term_sees_pixel : std::false_type {};
template <class T>
struct term_sees_pixel<T, std::void_t<decltype(T::PIXEL)>> : std::bool_constant<T::PIXEL> {};

template <class Term>
__device__ __forceinline__ void upsample_gather(Term term, const float* __restrict__ logit, const float* __restrict__ lse,
                                                const float* __restrict__ gscale, float* __restrict__ dlogit, int C, int h, int w,
                                                int H, int W) {
  extern __shared__ __attribute__((aligned(16))) float uce_smem[];
  float* sN = uce_smem;                                  // [UCE_NB * UCE_NB][128]   neighbourhood logits of the 128 classes of a pass
  float* sAcc = sN + UCE_NB * UCE_NB * 128;              // [4 groups][UCE_TB * UCE_TB][128]
  int2* sLL = reinterpret_cast<int2*>(sAcc + 4 * UCE_TB * UCE_TB * 128);  // [UCE_FP * UCE_FP] {staged label, bits of lse * log2 e} of a footprint pixel
  float* sYl = reinterpret_cast<float*>(sLL + UCE_FP * UCE_FP);    // [UCE_FP][2]  l0, l1 of a footprint row
  int* sYi = reinterpret_cast<int*>(sYl + 2 * UCE_FP);   // [UCE_FP][2]  i0, i1 relative to the block's first cell - 1
  int4* sXT = reinterpret_cast<int4*>(sYi + 2 * UCE_FP);  // [UCE_FP] {i0, i1 (same origin), bits of l0, l1} of a footprint column
  float* sPl = reinterpret_cast<float*>(sXT + UCE_FP);   // PLANE only: [UCE_FP * UCE_FP] plane value of a footprint pixel
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
      float plane = 0.f;
      const int lab = term.stage(p, plane);
      if constexpr (Term::PLANE) sPl[i] = plane;
      if constexpr (Term::RAW) sLL[i] = make_int2(lab, 0);
      else sLL[i] = make_int2(lab, __float_as_int(lse[p] * 1.4426950408889634f));  // (the staged path works in the log2 domain: one v_exp_f32 per pixel and class)
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
    term.load_class(b, c);
    __syncthreads();
    if (c < C && staged) {
      // Staged footprints (the step's shapes).  Everything that depends on the pixel alone — tap indices and weights, label,
      // log-sum-exp — is the same for the 64 lanes of a wavefront (a row group is two whole wavefronts): read to scalar
      // registers.  The footprint columns are walked one COLUMN PAIR (first tap on block column k - 1, k = 0 .. TB) at a time,
      // the pair loop unrolled: the vector work per pixel and class is the interpolation (2 FMAs on the row-combined cell
      // logits A0 / A1 of the pair), one exp2, the loss's term and two FMAs into the pair's sums s0 / s1, which land in the row's
      // column sums cs[] by static register index; the row weights multiply cs once per row and only then touch the thread's
      // LDS cells (8 read-add-writes per footprint row; the first cut folded 4 per column pair: 151 -> 118 us at
      // 2 x 100 x 64 x 64 -> 512^2, this form: see profiles/README.md)
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
        const float* plr = sPl + r * nx;  // (PLANE only)
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
          constexpr float dom = Term::RAW ? 1.f : 1.4426950408889634f;  // (RAW: the logit itself, no log2 domain)
          const float A0 = (yl0 * n00 + yl1 * n10) * dom;
          const float A1 = (yl0 * n01 + yl1 * n11) * dom;
          float s0 = 0.f, s1 = 0.f;
          // one 16-byte column record + one 8-byte pixel record per step, the next step's pair requested before this one is used
          int4 xt_n = sXT[x0];
          int2 ll_n = llr[x0];
          float pl_n = Term::PLANE ? plr[x0] : 0.f;
          for (int xx = x0; xx < x1; ++xx) {
            const int4 xt = xt_n;
            const int2 ll = ll_n;
            const float pl = pl_n;
            const int xn = min(xx + 1, nx - 1);
            xt_n = sXT[xn];
            ll_n = llr[xn];
            if constexpr (Term::PLANE) pl_n = plr[xn];
            const int lab = sc(ll.x);
            if (term.skip(lab)) continue;
            const float xl0 = __int_as_float(sc(xt.z)), xl1 = __int_as_float(sc(xt.w));
            float prob;
            if constexpr (Term::RAW) prob = fmaf(xl1, A1, xl0 * A0);
            else {
              const float ls = __int_as_float(sc(ll.y));
              prob = __builtin_amdgcn_exp2f(fmaf(xl1, A1, fmaf(xl0, A0, -ls)));
            }
            float gq;
            if constexpr (term_sees_pixel<Term>::value)
              gq = term.term(prob, c, lab, Term::PLANE ? scf(pl) : 0.f, ((long)b * H + y_lo + r) * W + x_lo + xx);
            else gq = term.term(prob, c, lab, Term::PLANE ? scf(pl) : 0.f);
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
          const long p = ((long)b * H + y_lo + r) * W + x_lo + xx;  // (footprints past the staged size: nothing of the pixel is in LDS)
          float plane = 0.f;
          const int lab = term.stage(p, plane);
          if (term.skip(lab)) continue;
          const float v = yl0 * (xl0 * n00 + xl1 * n01) + yl1 * (xl0 * n10 + xl1 * n11);
          float prob;
          if constexpr (Term::RAW) prob = v;
          else prob = __expf(v - lse[p]);
          float gq;
          if constexpr (term_sees_pixel<Term>::value) gq = term.term(prob, c, lab, plane, p);
          else gq = term.term(prob, c, lab, plane);
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

// Host side of the rscotr_upsample_* entries.
inline int upsample_check_shape(const char* entry, int B, int C, int h, int w, int H, int W) {
  if (B < 0 || C <= 0 || h <= 0 || w <= 0 || H <= 0 || W <= 0) return fail(RSCOTR_E_SHAPE, "%s: bad shape", entry);
  return RSCOTR_OK;
}

// One gather launch: a workgroup of 512 per block of cells.  The dynamic-LDS attribute is set once per kernel (the static
// belongs to this instantiation).
template <auto Kernel, bool PLANE, class... Args>
inline void launch_upsample_gather(hipStream_t s, int B, int h, int w, Args... args) {
  static const bool attr_set = [] {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)upsample_gather_lds_bytes(PLANE));
    return true;
  }();
  (void)attr_set;
  const int nblk = B * ((h + UCE_TB - 1) / UCE_TB) * ((w + UCE_TB - 1) / UCE_TB);
  Kernel<<<nblk, 512, upsample_gather_lds_bytes(PLANE), s>>>(args...);
}

}  // namespace rscotr
