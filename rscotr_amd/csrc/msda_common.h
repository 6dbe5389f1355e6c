// What the multi-scale deformable attention (MSDA) files share: the bilinear set-up of one sample, the per-sample records the
// forward and the backward sample kernel stage in LDS, the level limits, the shape check and the (D, P) dispatch.
//
// The operator replaces what the reference reaches through mmcv's
//   MultiScaleDeformableAttnFunction.apply(value, spatial_shapes, level_start_index,
//                                          sampling_locations, attention_weights, im2col_step)
// (ext_module.ms_deform_attn_forward / _backward), called from
//   models/multi/seg_head/pixel_decoder.py:134-146   (shared encoder, seg)
//   models/multi/bbox_head/transformer.py:211-221    (shared encoder, det)
//   models/multi/bbox_head/transformer.py:258-269    (DINO decoder cross-attn)
//
//   out[b,q,h,:] = sum_{l<L} sum_{p<P} A[b,q,h,l,p] * bilinear(V_l[b,:,h,:], loc[b,q,h,l,p,:])
// with pixel coords x = loc_x*W_l - 0.5, y = loc_y*H_l - 0.5, zero padding outside the map
// (== F.grid_sample(bilinear, zeros, align_corners=False)).
//
// Files: msda_fwd.hip (forward, with the fused prologue), msda_prep.hip (the stand-alone prologue), msda_bwd_sample.hip
// (grad_loc / grad_attn by sample, and the atomic scatter of grad_value), msda_bwd_sorted.hip and msda_bwd_tiled.hip (grad_value
// without atomics), msda.hip (host only: which of them serves a backward call).
#pragma once
#include <cstdlib>
#include <cstring>

#include "common.h"
#include "rscotr.h"

namespace rscotr {

constexpr int MSDA_MAXL = 16;   // levels the sorted backward handles (LevelGeom); the forward and the scatter take any L with L P <= 64
constexpr int MSDA_T_MAXL = 8;  // levels the tiled backward handles (MsdaTiles, MsdaMaskGeom)

// queries per 256-thread workgroup of the forward and the backward sample kernel: D / 4 lanes hold the D channels of one query
constexpr int msda_qb(int D) { return 4 * (kWave / (D / 4)); }

struct Bilinear {
  int i1, i2, i3, i4;      // token offsets inside the level (valid only if ok*)
  bool ok1, ok2, ok3, ok4;  // tap inside the map
  bool in;                  // sample inside (-1, size) on both axes
  float hh, hw, lh, lw;
  int h_low, w_low;         // top-left tap (-1 .. size - 1 when `in`)
};

// Pixel coordinate of a normalised sampling location: loc * extent - 0.5 as ONE explicitly fused multiply-add.  Every kernel that
// derives a bin (floor) or a fractional weight from a location calls this: the bin written by the sample kernel and the
// weights re-derived by the tile kernel must come from the same float, whatever the compiler would contract on its own (a
// sample within one ulp of an integer coordinate would otherwise land in bin n with a weight of ~0 instead of ~1: ADVICE r3)
__device__ __forceinline__ float msda_pix(float loc, int extent) { return __fmaf_rn(loc, (float)extent, -0.5f); }

__device__ __forceinline__ Bilinear bilinear_setup(float lx, float ly, int Hl, int Wl) {
  Bilinear t;
  const float h_im = msda_pix(ly, Hl);
  const float w_im = msda_pix(lx, Wl);
  t.in = (h_im > -1.f) && (w_im > -1.f) && (h_im < (float)Hl) && (w_im < (float)Wl);
  const float hf = floorf(h_im), wf = floorf(w_im);
  const int h_low = t.in ? (int)hf : 0, w_low = t.in ? (int)wf : 0;
  const int h_high = h_low + 1, w_high = w_low + 1;
  t.h_low = h_low;
  t.w_low = w_low;
  t.lh = h_im - hf;
  t.lw = w_im - wf;
  t.hh = 1.f - t.lh;
  t.hw = 1.f - t.lw;
  if (!t.in) t.lh = t.lw = t.hh = t.hw = 0.f;  // sample skipped entirely (also NaN/inf locations)
  t.ok1 = t.in && h_low >= 0 && w_low >= 0;
  t.ok2 = t.in && h_low >= 0 && w_high <= Wl - 1;
  t.ok3 = t.in && h_high <= Hl - 1 && w_low >= 0;
  t.ok4 = t.in && h_high <= Hl - 1 && w_high <= Wl - 1;
  t.i1 = h_low * Wl + w_low;
  t.i2 = t.i1 + 1;
  t.i3 = t.i1 + Wl;
  t.i4 = t.i3 + 1;
  return t;
}

__device__ __forceinline__ float4 ld4(const float* p, bool ok) {
  return ok ? *reinterpret_cast<const float4*>(p) : make_float4(0.f, 0.f, 0.f, 0.f);
}

// One sample of a (query, head) as the forward's gather loop wants it: the bilinear set-up is done ONCE per sample by the thread that
// stages it — the G = D / 4 lanes that share a (query, head) used to repeat it, ~50 of the ~85 instructions a lane issued per
// sample, and the launch was bound by instruction issue (22 us of issue on the whole chip for the 1.39 M samples of an
// encoder call), not by the L2.  Same arithmetic on the same inputs: results are bit-identical.
struct alignas(16) MsdaSample {
  float aw, w1, w2, w3;  // attention weight; bilinear weights of the four taps
  float w4;
  int e1;                // element offset of the top-left tap's channel row from the (image, head) base (level start included)
  int ok;                // bit t: tap t lies inside the map
  int pad;
};

// the backward sample kernel's record: the fractional weights themselves (its derivative terms want them)
struct alignas(16) MsdaSampleB {
  float aw, hh, hw, lh;
  float lw;
  int e1;   // element offset of the top-left tap's channel row from the LEVEL's first token
  int ok;   // bits 0-3: tap inside the map; bit 4: the sample counts (inside (-1, size) on both axes)
  int pad;
};

__device__ __forceinline__ float dot4(float4 a, float4 b) {
  return a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w;
}

__device__ __forceinline__ float4 scale4(float4 a, float s) {
  return make_float4(a.x * s, a.y * s, a.z * s, a.w * s);
}

inline int check_shape(const char* fn, int B, int Nk, int Nq, int H, int D, int L, int P) {
  if (B < 0 || Nk < 0 || Nq < 0 || H <= 0 || L <= 0)
    return fail(RSCOTR_E_SHAPE, "%s: negative/zero dimension (B=%d Nk=%d Nq=%d H=%d L=%d)", fn, B,
                Nk, Nq, H, L);
  if (!(D == 16 || D == 32 || D == 64))
    return fail(RSCOTR_E_SHAPE, "%s: channels per head D=%d not in {16,32,64}", fn, D);
  if (!(P == 1 || P == 2 || P == 4 || P == 8))
    return fail(RSCOTR_E_SHAPE, "%s: num_points P=%d not in {1,2,4,8}", fn, P);
  if ((long)L * P > 64) return fail(RSCOTR_E_SHAPE, "%s: L*P=%d exceeds 64", fn, L * P);
  return RSCOTR_OK;
}

#define RSCOTR_DISPATCH_DP(D, P, CALL)                         \
  switch ((D) * 16 + (P)) {                                    \
    case 16 * 16 + 1: { CALL(16, 1); } break;                  \
    case 16 * 16 + 2: { CALL(16, 2); } break;                  \
    case 16 * 16 + 4: { CALL(16, 4); } break;                  \
    case 16 * 16 + 8: { CALL(16, 8); } break;                  \
    case 32 * 16 + 1: { CALL(32, 1); } break;                  \
    case 32 * 16 + 2: { CALL(32, 2); } break;                  \
    case 32 * 16 + 4: { CALL(32, 4); } break;                  \
    case 32 * 16 + 8: { CALL(32, 8); } break;                  \
    case 64 * 16 + 1: { CALL(64, 1); } break;                  \
    case 64 * 16 + 2: { CALL(64, 2); } break;                  \
    case 64 * 16 + 4: { CALL(64, 4); } break;                  \
    case 64 * 16 + 8: { CALL(64, 8); } break;                  \
  }

}  // namespace rscotr
