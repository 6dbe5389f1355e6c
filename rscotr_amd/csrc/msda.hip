// MSDA backward, host side only: which grad_value strategy serves a rscotr_msda_bwd call (plan_msda_bwd), the two workspace
// queries, and the entry itself — validate, plan, launch.  The kernels live in msda_bwd_sample.hip, msda_bwd_tiled.hip and
// msda_bwd_sorted.hip (msda_bwd.h); the forward in msda_fwd.hip; the operator and the reference's call sites in msda_common.h.
//
// All three strategies are live:
//   tiled    the default of rscotr_amd.ops: 3 launches, bit-reproducible, grad_value fully overwritten;
//   sorted   what a tiled request gets when msda_tiles_build refuses the pyramid (L > 8, an extent above 32 766, more than 2^20
//            workgroups, a token sum other than Nk): 8 launches, bit-reproducible, grad_value fully overwritten;
//   scatter  what is left when the sorted strategy has no workspace either (none given, too small, L > 16), and what the
//            sample kernel decides ON THE DEVICE when the sorted strategy's extended bins do not fit its LDS histogram:
//            fp32 atomics into a zeroed grad_value, order-dependent.
#include "msda_bwd.h"

namespace rscotr {

enum MsdaBwdStrategy {
  MSDA_BWD_TILED,
  MSDA_BWD_SORTED,
  MSDA_BWD_SORTED_OR_SCATTER,  // sorted, but only the device knows whether the bins fit: the launcher zeroes grad_value itself
  MSDA_BWD_SCATTER,
};

struct MsdaBwdPlan {
  MsdaBwdStrategy strategy;
  MsdaTiles tiles;          // MSDA_BWD_TILED only: the geometry, built once
  int64_t workspace_bytes;  // what the strategy uses of the caller's workspace (0: none)
  // The caller must pass grad_value ZEROED: MSDA_BWD_SCATTER only.  rscotr_amd/ops/deform.py serves this from the same two
  // queries the planner uses: it zeroes exactly when both answer 0 (or 'scatter' is forced and it passes no workspace)
  bool zeroed_grad_value;
  bool amax_by_combine;     // grad_value's range word comes out of msda_tile_combine_kernel; else rscotr_amax_f32 after the launches
  size_t sample_lds;        // dynamic LDS of the sample kernel (msda_bwd_lds)
};

// bytes of the tiled strategy's workspace, 0 where it does not take the geometry; *T: the geometry it runs on
static int64_t tiled_workspace(MsdaTiles* T, const int64_t* shapes_host, int B, int Nk, int Nq, int H, int D, int L, int P) {
  if (B <= 0 || Nq <= 0 || H <= 0 || P <= 0 || Nq >= (1 << 20) || !msda_tiles_build(T, shapes_host, L, Nk, (long)Nq * P, D)) return 0;
  return msda_tiled_ws_bytes(*T, B * H, Nq, P, D);
}

// bytes of the sorted strategy's workspace, 0 where it does not take the geometry
static int64_t sorted_workspace(int B, int Nk, int Nq, int H, int L, int P) {
  if (B <= 0 || Nk <= 0 || Nq <= 0 || H <= 0 || L <= 0 || P <= 0 || L > MSDA_MAXL) return 0;
  return msda_sorted_ws_bytes(B * H, Nk, Nq, L, P);
}

// The one place that decides how grad_value is computed, from what the caller passed (include/rscotr.h).  The cascade is the
// one rscotr_msda_bwd always ran; three of its conditions are accidents of its order and are kept because callers may lean
// on them:
//   * `Nk > 0` is tested on both workspace branches although both queries already answer 0 for Nk == 0 (the tiled one through
//     the token sum of msda_tiles_build): redundant, never observable;
//   * the workspace's alignment is tested only on a branch that uses the workspace: a misaligned workspace that is too small
//     for both strategies is not an error, the call scatters;
//   * a workspace too small for the tiled strategy is not an error either: the request falls through to the sorted
//     strategy, and from there to the scatter — into a grad_value the caller may not have zeroed (ops/deform.py always sizes
//     the workspace from the queries, so it cannot get there).
static int plan_msda_bwd(MsdaBwdPlan* plan, int B, int Nk, int Nq, int H, int D, int L, int P, const int64_t* shapes_host,
                         const void* workspace, int64_t workspace_bytes) {
  plan->sample_lds = msda_bwd_lds(D, L, P);
  if (plan->sample_lds > MSDA_CU_LDS)  // (D = 16 with L P > 53; all three strategies launch the sample kernel)
    return fail(RSCOTR_E_SHAPE, "rscotr_msda_bwd: the sample kernel needs %zu bytes of LDS for D=%d, L*P=%d; a compute unit has %zu",
                plan->sample_lds, D, L * P, MSDA_CU_LDS);
  plan->workspace_bytes = 0;
  plan->zeroed_grad_value = plan->amax_by_combine = false;
  if (workspace && shapes_host && Nk > 0) {
    const int64_t need = tiled_workspace(&plan->tiles, shapes_host, B, Nk, Nq, H, D, L, P);
    if (need > 0 && workspace_bytes >= need) {
      if (!aligned16(workspace)) return fail(RSCOTR_E_ALIGN, "rscotr_msda_bwd: workspace must be 16-byte aligned");
      plan->strategy = MSDA_BWD_TILED;
      plan->workspace_bytes = need;
      plan->amax_by_combine = true;
      return RSCOTR_OK;
    }
  }
  const int64_t need = sorted_workspace(B, Nk, Nq, H, L, P);
  if (workspace && need > 0 && workspace_bytes >= need && Nk > 0) {
    if (!aligned16(workspace)) return fail(RSCOTR_E_ALIGN, "rscotr_msda_bwd: workspace must be 16-byte aligned");
    plan->strategy = msda_sorted_may_stand_down(Nk, L) ? MSDA_BWD_SORTED_OR_SCATTER : MSDA_BWD_SORTED;
    plan->workspace_bytes = need;
    return RSCOTR_OK;
  }
  plan->strategy = MSDA_BWD_SCATTER;
  plan->zeroed_grad_value = true;
  return RSCOTR_OK;
}

}  // namespace rscotr

using namespace rscotr;

extern "C" int64_t rscotr_msda_bwd_workspace(int B, int Nk, int Nq, int H, int L, int P) {
  return sorted_workspace(B, Nk, Nq, H, L, P);
}

extern "C" int64_t rscotr_msda_bwd_tiled_workspace(const int64_t* shapes_host, int B, int Nk, int Nq, int H, int D, int L,
                                                   int P) {
  MsdaTiles T;
  return tiled_workspace(&T, shapes_host, B, Nk, Nq, H, D, L, P);
}

extern "C" int rscotr_msda_bwd(const float* value, const int64_t* spatial_shapes,
                               const int64_t* level_start_index, const float* loc,
                               const float* attn, const float* grad_out, float* grad_value,
                               float* grad_loc, float* grad_attn, int B, int Nk, int Nq, int H,
                               int D, int L, int P, const int64_t* shapes_host, void* workspace,
                               int64_t workspace_bytes, uint32_t* amax_grad_value, void* stream) {
  if (int e = check_shape("rscotr_msda_bwd", B, Nk, Nq, H, D, L, P)) return e;
  if (B == 0 || Nq == 0) return RSCOTR_OK;  // grad_value stays as zeroed by the caller
  if (!value || !spatial_shapes || !level_start_index || !loc || !attn || !grad_out ||
      !grad_value || !grad_loc || !grad_attn)
    return fail(RSCOTR_E_ARG, "rscotr_msda_bwd: null pointer");
  if (!aligned16(value) || !aligned16(grad_out) || !aligned16(grad_value))
    return fail(RSCOTR_E_ALIGN, "rscotr_msda_bwd: value/grad_out/grad_value must be 16-byte aligned");
  MsdaBwdPlan plan;
  if (int e = plan_msda_bwd(&plan, B, Nk, Nq, H, D, L, P, shapes_host, workspace, workspace_bytes)) return e;
  hipStream_t s = (hipStream_t)stream;
  // algorithmic bytes: read value, read-modify-write grad_value, read loc/attn/grad_out, write grad_loc/grad_attn
  ProfScope prof(PROF_MSDA_BWD, 4.0 * B * (3.0 * Nk * H * D + (double)Nq * H * L * P * 6 + (double)Nq * H * D), s,
                 "rscotr_msda_bwd<%d, %d> (sample + tile + combine kernels)", D, P);
  const MsdaBwdArgs a{value, spatial_shapes, level_start_index, loc, attn, grad_out, grad_value, grad_loc, grad_attn,
                      B, Nk, Nq, H, D, L, P, s};
  const char* what = "rscotr_msda_bwd";
  switch (plan.strategy) {
    case MSDA_BWD_TILED:
      launch_msda_bwd_tiled(a, plan.tiles, (char*)workspace, amax_grad_value);
      what = "rscotr_msda_bwd (tiled)";
      break;
    case MSDA_BWD_SORTED:
    case MSDA_BWD_SORTED_OR_SCATTER:
      launch_msda_bwd_sorted(a, (int*)workspace, plan.strategy == MSDA_BWD_SORTED_OR_SCATTER);
      what = "rscotr_msda_bwd (sorted)";
      break;
    case MSDA_BWD_SCATTER:
      launch_msda_bwd_sample(a, MSDA_SAMPLE_SCATTER, nullptr, nullptr, nullptr, 0);
      break;
  }
  if (int e = check_launch(what)) return e;
  if (plan.amax_by_combine || !amax_grad_value) return RSCOTR_OK;
  return rscotr_amax_f32(grad_value, (int64_t)B * Nk, H * D, H * D, amax_grad_value, stream);
}
