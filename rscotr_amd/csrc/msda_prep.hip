// The element-wise prologue of mmcv MultiScaleDeformableAttention.forward as launches of its own (rscotr_msda_prep_fwd /
// rscotr_msda_prep_bwd).  msda_fwd_kernel<.., PREP = true> (msda_fwd.hip) repeats the forward arithmetic bit for bit on the
// geometries rscotr_msda_fused_ok takes; both use msda_location, group_max and group_sum of common.h.
#include "common.h"
#include <stdlib.h>

namespace rscotr {

// ---- sampling locations + attention weights of mmcv MultiScaleDeformableAttention.forward in one pass -----------
// (models reach it at seg_head/pixel_decoder.py:134-146, bbox_head/transformer.py:211-221,258-269)
//   attn = softmax over the L*P logits of a (query, head);
//   loc  = ref_xy + off / (W_l, H_l)                      (2-d reference points)
//   loc  = ref_xy + off / P * ref_wh * 0.5                (4-d reference points)
// 16 consecutive lanes own one (image, query, head) when L*P == 16 (the configs' 4 levels x 4 points); general
// L*P <= 64 uses one wavefront slice of LP lanes rounded up to a power of two.
template <int G>
__global__ __launch_bounds__(256) void msda_prep_fwd_kernel(const float* __restrict__ off, const float* __restrict__ logit,
                                                            const float* __restrict__ ref, const float* __restrict__ norm,
                                                            float* __restrict__ loc, float* __restrict__ attn, long groups,
                                                            int Nq, int H, int L, int P, int refdim, int ld_off,
                                                            int ld_logit, int ref_levels) {
  const long gid = ((long)blockIdx.x * 256 + threadIdx.x) / G;
  const int s = threadIdx.x % G, LP = L * P;
  const bool in = gid < groups && s < LP;
  const long e = gid * LP + s;
  float lg = -3.0e38f;
  if (in) {
    const long bq = gid / H;                // b * Nq + q
    const int h = (int)(gid - bq * H);
    lg = logit[bq * ld_logit + h * LP + s];
    const int l = s / P;
    const float* r = ref + (bq * ref_levels + (ref_levels > 1 ? l : 0)) * refdim;
    const float2 o = *reinterpret_cast<const float2*>(off + bq * ld_off + (h * LP + s) * 2);
    reinterpret_cast<float2*>(loc)[e] = msda_location(r, o, norm, l, P, refdim);
  }
  const float m = group_max<G>(lg);
  const float ex = in ? expf(lg - m) : 0.f;
  const float sum = group_sum<G>(ex);
  if (in) attn[e] = ex / sum;
}

// grad_off = grad_loc * d(loc)/d(off); grad_logit = attn * (grad_attn - sum attn * grad_attn)
template <int G>
__global__ __launch_bounds__(256) void msda_prep_bwd_kernel(const float* __restrict__ gloc, const float* __restrict__ gattn,
                                                            const float* __restrict__ attn, const float* __restrict__ ref,
                                                            const float* __restrict__ norm, float* __restrict__ goff,
                                                            float* __restrict__ glogit, long groups, int Nq, int H, int L,
                                                            int P, int refdim, int ld_off, int ld_logit, int ref_levels,
                                                            unsigned* __restrict__ amax_out) {
  const long gid = ((long)blockIdx.x * 256 + threadIdx.x) / G;
  const int s = threadIdx.x % G, LP = L * P;
  const bool in = gid < groups && s < LP;
  float amx = 0.f;  // max |grad_off|, |grad_logit| -> the range word of the gradient (common.h: amax_commit)
  const long e = gid * LP + s;
  const long bq = gid / H;
  const int h = (int)(gid - bq * H);
  float p = 0.f, ga = 0.f;
  if (in) {
    p = attn[e];
    ga = gattn[e];
    const int l = s / P;
    const float2 g = reinterpret_cast<const float2*>(gloc)[e];
    float2 out;
    if (refdim == 2) {
      out.x = g.x / norm[2 * l];
      out.y = g.y / norm[2 * l + 1];
    } else {
      const float* r = ref + (bq * ref_levels + (ref_levels > 1 ? l : 0)) * refdim;
      out.x = g.x * (r[2] * 0.5f) / (float)P;
      out.y = g.y * (r[3] * 0.5f) / (float)P;
    }
    *reinterpret_cast<float2*>(goff + bq * ld_off + (h * LP + s) * 2) = out;
    amx = fmaxf(fabsf(out.x), fabsf(out.y));
  }
  const float dot = group_sum<G>(p * ga);
  if (in) {
    const float gl = p * (ga - dot);
    glogit[bq * ld_logit + h * LP + s] = gl;
    amx = fmaxf(amx, fabsf(gl));
  }
  amax_commit(amax_out, amx);
}

}  // namespace rscotr

using namespace rscotr;

static int msda_prep_check(const char* fn, int B, int Nq, int H, int L, int P, int refdim, int ld_off, int ld_logit,
                           int ref_levels) {
  if (B < 0 || Nq < 0 || H <= 0 || L <= 0 || P <= 0) return fail(RSCOTR_E_SHAPE, "%s: bad shape", fn);
  if (ld_off < H * L * P * 2 || (ld_off & 1) || ld_logit < H * L * P)
    return fail(RSCOTR_E_SHAPE, "%s: row strides must cover a row (offsets: even)", fn);
  if (ref_levels != L && ref_levels != 1) return fail(RSCOTR_E_SHAPE, "%s: ref_levels must be L or 1", fn);
  if (L * P > 64) return fail(RSCOTR_E_SHAPE, "%s: L*P = %d > 64", fn, L * P);
  if (refdim != 2 && refdim != 4) return fail(RSCOTR_E_SHAPE, "%s: reference points must be 2- or 4-d", fn);
  return RSCOTR_OK;
}

#define MSDA_PREP_DISPATCH(LP, CALL) \
  do {                               \
    if ((LP) <= 8) { CALL(8); }      \
    else if ((LP) <= 16) { CALL(16); } \
    else if ((LP) <= 32) { CALL(32); } \
    else { CALL(64); }               \
  } while (0)

extern "C" int rscotr_msda_prep_fwd(const float* off, const float* logit, const float* ref, const float* norm, float* loc,
                                    float* attn, int B, int Nq, int H, int L, int P, int refdim, int ld_off, int ld_logit,
                                    int ref_levels, void* stream) {
  if (int e = msda_prep_check("rscotr_msda_prep_fwd", B, Nq, H, L, P, refdim, ld_off, ld_logit, ref_levels)) return e;
  const long groups = (long)B * Nq * H;
  if (groups == 0) return RSCOTR_OK;
  if (!off || !logit || !ref || !loc || !attn || (refdim == 2 && !norm))
    return fail(RSCOTR_E_ARG, "rscotr_msda_prep_fwd: null pointer");
#define CALL(G) \
  msda_prep_fwd_kernel<G><<<(unsigned)((groups * G + 255) / 256), 256, 0, (hipStream_t)stream>>>(off, logit, ref, norm, loc, attn, groups, Nq, H, L, P, refdim, ld_off, ld_logit, ref_levels)
  MSDA_PREP_DISPATCH(L * P, CALL);
#undef CALL
  return check_launch("rscotr_msda_prep_fwd");
}

extern "C" int rscotr_msda_prep_bwd(const float* grad_loc, const float* grad_attn, const float* attn, const float* ref,
                                    const float* norm, float* grad_off, float* grad_logit, int B, int Nq, int H, int L,
                                    int P, int refdim, int ld_off, int ld_logit, int ref_levels, uint32_t* amax_out, void* stream) {
  if (int e = msda_prep_check("rscotr_msda_prep_bwd", B, Nq, H, L, P, refdim, ld_off, ld_logit, ref_levels)) return e;
  const long groups = (long)B * Nq * H;
  if (groups == 0) return RSCOTR_OK;
  if (!grad_loc || !grad_attn || !attn || !ref || !grad_off || !grad_logit || (refdim == 2 && !norm))
    return fail(RSCOTR_E_ARG, "rscotr_msda_prep_bwd: null pointer");
#define CALL(G) \
  msda_prep_bwd_kernel<G><<<(unsigned)((groups * G + 255) / 256), 256, 0, (hipStream_t)stream>>>(grad_loc, grad_attn, attn, ref, norm, grad_off, grad_logit, groups, Nq, H, L, P, refdim, ld_off, ld_logit, ref_levels, amax_out)
  MSDA_PREP_DISPATCH(L * P, CALL);
#undef CALL
  return check_launch("rscotr_msda_prep_bwd");
}
