// The MSDA backward between its files: what one rscotr_msda_bwd call carries (MsdaBwdArgs), the one launcher of the sample
// kernel, and per grad_value strategy its workspace arithmetic and its launch function.  msda.hip decides which runs.
#pragma once
#include "msda_common.h"

namespace rscotr {

// the tensors and sizes of one rscotr_msda_bwd call (include/rscotr.h)
struct MsdaBwdArgs {
  const float *value;
  const int64_t *shapes, *lsi;  // device
  const float *loc, *attn, *go;
  float *gv, *gl, *ga;
  int B, Nk, Nq, H, D, L, P;
  hipStream_t s;
};

// ---- tiled strategy (msda_bwd_tiled.hip) ----
struct MsdaTiles {
  int L, NW;                                       // levels, workgroups (= partial tiles) per (b, h)
  int Hl[MSDA_T_MAXL], Wl[MSDA_T_MAXL], lsi[MSDA_T_MAXL];
  int tsx[MSDA_T_MAXL], tsy[MSDA_T_MAXL];          // bins per tile along x / y (<= 16)
  int ntx[MSDA_T_MAXL], nty[MSDA_T_MAXL];          // tiles along x / y
  int nch[MSDA_T_MAXL];                            // sample chunks
  int wbase[MSDA_T_MAXL];                          // first workgroup of the level
};

// Tile geometry the sample kernel needs for the BLOCK MASKS of the tile-accumulation backward: per level,
// reciprocal tile edges (in bins) and tiles per row.  mask[(b h, level, query tile of the sample kernel)] has bit
// (tile & 63) set iff one of the block's samples has its bin in that tile: the tile workgroups skip the other blocks.
struct MsdaMaskGeom {
  float itx[MSDA_T_MAXL], ity[MSDA_T_MAXL];
  int ntx[MSDA_T_MAXL];
};

// false: the strategy does not take this pyramid (L > MSDA_T_MAXL, an extent above 32 766, more than 2^20 workgroups, token sum != Nk)
bool msda_tiles_build(MsdaTiles* T, const int64_t* shapes_host, int L, int Nk, long SP, int D);
int64_t msda_tiled_ws_bytes(const MsdaTiles& T, int BH, int Nq, int P, int D);
// sample kernel (bin words + block masks) + tile kernel + combine kernel; grad_value fully overwritten, its range word folded
// into *amax_gv by the combine kernel
void launch_msda_bwd_tiled(const MsdaBwdArgs& a, const MsdaTiles& T, char* ws, unsigned* amax_gv);

// ---- sorted strategy (msda_bwd_sorted.hip) ----
int64_t msda_sorted_ws_bytes(int BH, int Nk, int Nq, int L, int P);
// true: the host's bound on the extended bins exceeds the LDS histogram, so only the kernels know (from the level shapes on
// the device) whether the strategy runs or stands down for the sample kernel's atomic scatter
bool msda_sorted_may_stand_down(int Nk, int L);
// histogram, sample kernel, bin sums, plan, fill, pull, chunk combine; with may_stand_down grad_value is zeroed here first
void launch_msda_bwd_sorted(const MsdaBwdArgs& a, int* ws, bool may_stand_down);

// ---- the sample kernel (msda_bwd_sample.hip): grad_loc / grad_attn, and per mode what grad_value needs ----
enum MsdaSampleMode {
  MSDA_SAMPLE_GRADS = 0,      // grad_loc / grad_attn only (grad_value comes from the pull kernel)
  MSDA_SAMPLE_SCATTER = 1,    // also scatter grad_value with fp32 atomics (into a zeroed tensor)
  MSDA_SAMPLE_SCATTER_IF = 2, // scatter iff the pyramid has more than bins_cap extended bins (the sorted strategy stood down)
  MSDA_SAMPLE_TILE = 3,       // grad_loc / grad_attn + one bin word per sample + the block masks of the tiled strategy
};
constexpr size_t MSDA_CU_LDS = 160 * 1024;  // LDS of a gfx950 compute unit: what one workgroup can be given at most
// dynamic LDS of msda_bwd_kernel: per sample a 32-byte record, grad_attn, grad_loc (2), one bin word; + the level masks
inline size_t msda_bwd_lds(int D, int L, int P) { return (size_t)msda_qb(D) * L * P * 12 * sizeof(float) + 64; }
// THE launch of msda_bwd_kernel: grid, LDS bytes and the opt-in to dynamic LDS above 64 KB for the instantiation launched.
// binw / mask / MG: MSDA_SAMPLE_TILE only (else null); bins_cap: MSDA_SAMPLE_SCATTER_IF only.
void launch_msda_bwd_sample(const MsdaBwdArgs& a, MsdaSampleMode mode, int* binw, unsigned long long* mask,
                            const MsdaMaskGeom* MG, int bins_cap);

}  // namespace rscotr
