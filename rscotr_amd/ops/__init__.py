"""Operator layer of the product path: torch.autograd.Function wrappers over the C ABI.

Each op launches hand-written gfx950 kernels from librscotr.so on the current torch stream with raw device pointers
(PyTorch only provides memory, streams and autograd bookkeeping).  There is NO CPU / eager fallback: a missing library, a
CPU tensor, or a non-zero return code raises.

    state      STATE: strategy switches and hooks (gradient sink, profiling, side stream) — the only mutable globals
    core       stream handle, workspace, profiling context, tensor checks
    ranges     RANGES: value ranges (amax slots) of GEMM operands for the fp16 split product
    deferred   DEFER: split-K slabs, LayerNorm / window-attention partials and grouped weight gradients folded by flush_deferred
    planes     WPLANES / HPLANES / FPLANES: pre-split planes of the weight operands, one life cycle
    fused      RELU_BITS, FFN_FUSED, LIN_FUSED: the fused-launch gates and callers of the Linear / MLP node
    matmul     gemm / gemm_batched / colsum, linear / mlp
    norm       layer_norm, layer_norm_fork, group_norm_tokens
    deform     msda, msda_prep, msda_attention (mmcv MultiScaleDeformableAttention)
    attention  swin_window_attention, mha (nn.MultiheadAttention), mask_logits, seg_class_logits, seg_attn_mask
    glue       level_embed_add, fan_out, cdn_queries, sine_embed4, neck im2col, layout helpers, cls pooling / loss
    losses     box utilities, match_cost_batched(_kind), lsap_*, focal / quality focal / box loss sums (box_loss_sums_kind), upsample_ce, upsample_ce_weighted, upsample_dice,
               upsample_tversky, upsample_focal, upsample_lovasz
    distutil   packed scalar all-reduces
    seg_eval   seg_predict (resample + flip + arg-max of the seg logits), seg_predict_tta (the same over V views: softmax, mean,
               arg-max), slide_windows / seg_predict_slide (test mode 'slide': the windows' logits merged, rescaled and arg-maxed),
               seg_areas (mmseg pre_eval areas)
    det_eval   det_decode (sigmoid + top-k + box decoding of a batch), det_match (COCOeval's per-image matching)

Callers use `from rscotr_amd import ops; ops.linear(...)`: every public (and test-visible) name of the submodules is
re-exported here (submodule names differ from every op name: `ops.gemm` and `ops.msda` are the functions)."""
from . import attention, core, deferred, deform, det_eval, distutil, fused, glue, losses, matmul, norm, planes, ranges, seg_eval, state
from .state import STATE

for _m in (core, ranges, deferred, planes, fused, matmul, norm, deform, attention, glue, losses, distutil, seg_eval, det_eval):
    for _k, _v in vars(_m).items():
        if not _k.startswith('__') and _k not in ('STATE',):
            globals().setdefault(_k, _v)
del _m, _k, _v
