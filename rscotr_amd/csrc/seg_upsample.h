// Bilinear resize (align_corners=False) source index and the geometry of the blocked backward gather, shared by the fused seg
// losses (csrc/seg_loss.hip: cross-entropy, csrc/seg_dice.hip: Dice) and the masked-attention mask.
//
// PyTorch's upsample_bilinear2d (align_corners=False) source index: s = max((d + 0.5) * in/out - 0.5, 0),
// i0 = floor(s), i1 = min(i0 + 1, in - 1), lambda1 = s - i0.
#pragma once
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

// The backward gathers: one workgroup per UCE_TB x UCE_TB block of low-resolution cells (see upsample_ce_bwd_kernel).
constexpr int UCE_TB = 4;    // cells per block edge
constexpr int UCE_NB = UCE_TB + 2;
constexpr int UCE_FP = 48;   // staged footprint rows / columns (40 at x8); larger footprints read labels / lse from global memory

}  // namespace rscotr
