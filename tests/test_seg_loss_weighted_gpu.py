"""The fused seg loss with class weights, avg_non_ignore, reduction='sum' and OHEM pixel sampling
(ops.upsample_ce_weighted: rscotr_upsample_ce_w_fwd / _ohem / _w_bwd) against the fp64 restatement of the contract in
tests/test_seg_loss_weighted_cpu.py, on every path of the backward kernel the unweighted tests name.

Tolerances are those of tests/test_seg_loss_gpu.py: loss within 1e-5 relative, d(1.7 loss)/d logit within 1e-4 of the largest
reference gradient, cells with an exactly zero reference gradient exactly zero, counts exact, arg-max ambiguity as there."""
import functools
import math

import pytest
import torch

from test_seg_loss_gpu import UCE_MAX_WG, _REACHES, _uce_blocks
from test_seg_loss_weighted_cpu import EPS, contract_loss, uce_inputs

pytestmark = pytest.mark.gpu

UCE_SEL_WG = 256  # csrc/seg_loss.hip: grid cap of the OHEM histogram and mask launches

_SHAPES = [
    ('staged', 2, 7, 8, 8, 64, 64),                                   # x8 as in the step
    ('fallback_both_axes_one_block', 1, 3, 4, 4, 64, 64),
    ('fallback_two_class_passes', 1, 130, 5, 6, 70, 30),
    ('staged_interior_two_class_passes', 2, 130, 9, 10, 23, 61),
    ('staged_interior_blocks', 1, 2, 13, 11, 50, 37),                 # non-integer ratios
    ('staged', 2, 7, 8, 8, 8, 8),                                     # identity
    ('staged_downsample', 1, 2, 13, 9, 5, 4),                         # untouched cells
    ('fallback_rows_only_mixed_launch', 1, 2, 5, 6, 70, 30),
    ('fallback_cols_only', 1, 2, 6, 5, 30, 70),
    ('fallback_records_recomputed', 1, 2, 3, 3, 150, 150),
]
_MODES = [('cw', False, 'mean'), ('cw', True, 'mean'), ('cw', False, 'sum')]
_NO_SAMPLER = [s + m for s in _SHAPES for m in _MODES[:2]] + [_SHAPES[0] + _MODES[2]]


@functools.lru_cache(maxsize=None)
def _inputs(B, C, h, w, H, W, ignore=255):
    return uce_inputs(B, C, h, w, H, W, ignore)


@functools.lru_cache(maxsize=None)
def _forward_facts(B, C, h, w, H, W, ignore=255):
    """(#non-ignored, #correct, #non-ignored pixels whose two largest interpolated logits are closer than 1e-4), fp64."""
    logit, label, _ = _inputs(B, C, h, w, H, W, ignore)
    r = contract_loss(logit, label, ignore)
    up, valid = r['up'], r['valid']
    correct = int(((up.argmax(1) == label) & valid).sum())
    n_near = 0
    if C > 1:
        top2 = up.topk(2, dim=1).values
        n_near = int((((top2[:, 0] - top2[:, 1]) < 1e-4) & valid).sum())
    return r['n_valid'], correct, n_near


def _reference(logit, label, ignore, cw, avg, reduction, mask=None):
    r = contract_loss(logit, label, ignore, cw, avg, reduction, mask=mask)
    (r['loss'] * 1.7).backward()
    return float(r['loss'].detach()), r['logit'].grad


def _check_loss_and_grad(tag, loss, ld, loss_r, grad_r):
    loss_v = float(loss.detach())
    (loss * 1.7).backward()
    grad = ld.grad.cpu()
    err = float((grad.double() - grad_r).abs().max() / (grad_r.abs().max() + 1e-30))
    print(f'{tag}: loss {loss_v:.8f} ref {loss_r:.8f}  gradient max error {err:.3e} of the largest reference gradient')
    assert abs(loss_v - loss_r) <= 1e-5 * max(abs(loss_r), 1e-3), (loss_v, loss_r)
    assert err < 1e-4, err
    untouched = grad_r == 0
    assert bool((grad[untouched] == 0).all()), int((grad[untouched] != 0).sum())
    return int(untouched.sum())


def _run_no_sampler(cuda, reaches, B, C, h, w, H, W, use_cw, avg, reduction, ignore=255):
    from rscotr_amd import ops
    assert _REACHES[reaches](h, w, H, W, C), (reaches, _uce_blocks(h, w, H, W))
    logit, label, cw = _inputs(B, C, h, w, H, W, ignore)
    valid, correct, n_near = _forward_facts(B, C, h, w, H, W, ignore)
    assert n_near <= 0.001 * valid, (n_near, valid)
    loss_r, grad_r = _reference(logit, label, ignore, cw, avg, reduction)
    ld, label_d, cw_d = logit.to(cuda).requires_grad_(True), label.to(cuda), cw.to(cuda)
    loss, acc, pixw = ops.upsample_ce_weighted(ld, label_d, ignore, class_weight=cw_d, avg_non_ignore=avg, reduction=reduction)
    assert not pixw.requires_grad
    with torch.no_grad():
        sums = ops.losses._UpsampleCEWeighted.apply(ld.detach(), label_d, ignore, cw_d, 'sum', None)[1].cpu()
    print(f'sums {sums[:3].tolist()} valid {valid} correct {correct} n_near {n_near}')
    assert valid < 2 ** 24 and float(sums[2]) == valid
    assert abs(float(sums[1]) - correct) <= n_near, (float(sums[1]), correct, n_near)
    assert abs(float(acc) - float(sums[1]) * 100.0 / max(valid, 1)) <= 1e-4
    # the weight plane kept for backward: the class weight of the label, 0 where ignored — exactly
    want = torch.where(label != ignore, cw[label.clamp(0, C - 1)], torch.zeros(()))
    assert torch.equal(pixw.cpu(), want)
    return _check_loss_and_grad('upsample_ce_weighted', loss, ld, loss_r, grad_r)


@pytest.mark.parametrize('reaches,B,C,h,w,H,W,use_cw,avg,reduction', _NO_SAMPLER)
def test_weighted_no_sampler(cuda, reaches, B, C, h, w, H, W, use_cw, avg, reduction):
    untouched = _run_no_sampler(cuda, reaches, B, C, h, w, H, W, use_cw, avg, reduction)
    if reaches == 'staged_downsample':
        assert untouched >= 59 * C


def test_weighted_other_ignore_index(cuda):
    _run_no_sampler(cuda, *_SHAPES[4], 'cw', True, 'mean', ignore=-100)


def test_weighted_forward_grid_stride(cuda):
    """More pixels than one trip of the capped forward grid, and the device select over a million values (forward only: the
    backward grid is one workgroup per block of cells and never strides)."""
    from rscotr_amd import ops
    B, C, h, w, H, W = 1, 2, 8, 8, 1056, 1000
    assert B * H * W > UCE_MAX_WG * 256
    logit, label, cw = _inputs(B, C, h, w, H, W)
    r = contract_loss(logit, label, 255, cw, True)
    loss, _, pixw = ops.upsample_ce_weighted(logit.to(cuda), label.to(cuda), 255, class_weight=cw.to(cuda), avg_non_ignore=True)
    loss_r = float(r['loss'].detach())
    assert abs(float(loss) - loss_r) <= 1e-5 * max(abs(loss_r), 1e-3), (float(loss), loss_r)
    assert torch.equal(pixw.cpu(), torch.where(label != 255, cw[label.clamp(0, C - 1)], torch.zeros(())))
    _check_ohem_mask(cuda, B, C, h, w, H, W, 0.1, 300000)


# ---- exact metamorphic checks ------------------------------------------------------------------------------------------------
_EXACT = [_SHAPES[0][1:], _SHAPES[1][1:]]


def _call(ops, logit, label_d, ignore=255, **kw):
    ld = logit.detach().clone().requires_grad_(True)
    loss, acc, pixw = ops.upsample_ce_weighted(ld, label_d, ignore, **kw)
    (loss * 1.7).backward()
    return loss.detach(), ld.grad, pixw


@pytest.mark.parametrize('B,C,h,w,H,W', _EXACT)
def test_unit_and_doubled_weights_are_exact(cuda, B, C, h, w, H, W):
    from rscotr_amd import ops
    logit, label, _ = _inputs(B, C, h, w, H, W)
    ld, label_d = logit.to(cuda), label.to(cuda)
    l0 = ld.clone().requires_grad_(True)
    loss0, _ = ops.upsample_ce(l0, label_d, 255)
    (loss0 * 1.7).backward()
    loss1, g1, pw1 = _call(ops, ld, label_d, class_weight=torch.ones(C, device=cuda))
    assert torch.equal(loss1, loss0.detach()) and torch.equal(g1, l0.grad)
    loss_n, g_n, _ = _call(ops, ld, label_d)  # no class weights at all: the same
    assert torch.equal(loss_n, loss0.detach()) and torch.equal(g_n, l0.grad)
    loss2, g2, pw2 = _call(ops, ld, label_d, class_weight=torch.full((C,), 2.0, device=cuda))
    assert torch.equal(loss2, 2 * loss0.detach()) and torch.equal(g2, 2 * l0.grad) and torch.equal(pw2, 2 * pw1)


@pytest.mark.parametrize('B,C,h,w,H,W', _EXACT)
def test_all_ignored_with_avg_non_ignore_is_zero(cuda, B, C, h, w, H, W):
    from rscotr_amd import ops
    logit, label, cw = _inputs(B, C, h, w, H, W)
    label_d = torch.full_like(label, 255).to(cuda)
    for kw in (dict(), dict(ohem=(0.7, 100))):
        loss, grad, pixw = _call(ops, logit.to(cuda), label_d, class_weight=cw.to(cuda), avg_non_ignore=True, **kw)
        assert float(loss) == 0.0 and not bool(torch.isnan(grad).any())
        assert float(grad.abs().max()) == 0.0 and float(pixw.abs().max()) == 0.0


@pytest.mark.parametrize('B,C,h,w,H,W', _EXACT)
def test_two_calls_are_bit_equal(cuda, B, C, h, w, H, W):
    from rscotr_amd import ops
    logit, label, cw = _inputs(B, C, h, w, H, W)
    ld, label_d, cw_d = logit.to(cuda), label.to(cuda), cw.to(cuda)
    for kw in (dict(), dict(ohem=(0.1, 1000))):
        a = _call(ops, ld, label_d, class_weight=cw_d, avg_non_ignore=True, **kw)
        b = _call(ops, ld, label_d, class_weight=cw_d, avg_non_ignore=True, **kw)
        assert all(torch.equal(x, y) for x, y in zip(a, b)), kw


# ---- OHEM ------------------------------------------------------------------------------------------------------------------------
_OHEM = [
    (2, 7, 8, 8, 64, 64, 0.7, 100),          # decided by thresh
    (2, 7, 8, 8, 64, 64, 0.7, 10 ** 6),      # decided by kth, clamped to N_valid - 1
    (2, 7, 8, 8, 64, 64, 0.999, 10 ** 6),    # thresh: every valid pixel
    (1, 3, 4, 4, 64, 64, 0.1, 1000),         # thresh, fallback path
    (2, 130, 9, 10, 23, 61, 0.0005, 600),    # kth
    (1, 2, 13, 11, 50, 37, 0.05, 800),       # kth
    (2, 7, 8, 8, 8, 8, 0.001, 20),           # kth
    (1, 2, 8, 8, 300, 300, 0.1, 30000),      # kth, select over 81010 values
]


def _check_ohem_mask(cuda, B, C, h, w, H, W, thresh, min_kept):
    """pix_weight != 0 against the reference mask.  A valid pixel is ambiguous when |nll_p - (-log T_ref)| <= 1e-4 in fp64:
    the fp32 interpolation error at these logit magnitudes is about 4e-6 (tests/test_seg_loss_gpu.py), order statistics are
    1-Lipschitz in the sup norm, so the kernel's threshold moves by no more than its values do; 1e-4 is more than ten times
    that.  Such pixels must be rare: n_ambiguous <= 1 + 0.002 N_valid, asserted before the GPU is touched."""
    from rscotr_amd import ops
    logit, label, _ = _inputs(B, C, h, w, H, W)
    r = contract_loss(logit, label, 255, ohem=(thresh, min_kept))
    valid, ref = r['valid'], r['mask']
    amb = valid & ((r['nll'] - r['nll_T']).abs() <= 1e-4)
    print(f'ohem {(B, C, h, w, H, W)} thresh {thresh} min_kept {min_kept}: selected {int(ref.sum())} ambiguous {int(amb.sum())} '
          f'valid {r["n_valid"]}')
    assert int(amb.sum()) <= 1 + 0.002 * r['n_valid']
    _, _, pixw = ops.upsample_ce_weighted(logit.to(cuda), label.to(cuda), 255, ohem=(thresh, min_kept))
    got = pixw.cpu() != 0
    assert not bool((got & ~valid).any())
    assert bool(((got == ref) | amb).all()), int(((got != ref) & ~amb).sum())
    assert bool(((pixw.cpu() == 1) | (pixw.cpu() == 0)).all())


@pytest.mark.parametrize('B,C,h,w,H,W,thresh,min_kept', _OHEM)
def test_ohem_mask(cuda, B, C, h, w, H, W, thresh, min_kept):
    if H == 300:
        # more than one trip of the histogram and mask launches' grids, and more partial rows than the mask launch has workgroups
        assert B * H * W > UCE_SEL_WG * 256 and (B * H * W + 255) // 256 > UCE_SEL_WG
    _check_ohem_mask(cuda, B, C, h, w, H, W, thresh, min_kept)


@pytest.mark.parametrize('use_cw,avg', [(False, False), (True, True)])
@pytest.mark.parametrize('B,C,h,w,H,W,thresh,min_kept', [_OHEM[0], _OHEM[3], _OHEM[4], _OHEM[5]])
def test_ohem_loss_and_gradient(cuda, B, C, h, w, H, W, thresh, min_kept, use_cw, avg):
    """Against the reference evaluated with the kernel's OWN mask (read back); the mask has its own test."""
    from rscotr_amd import ops
    logit, label, cw = _inputs(B, C, h, w, H, W)
    cw = cw if use_cw else None
    ld = logit.to(cuda).requires_grad_(True)
    loss, _, pixw = ops.upsample_ce_weighted(ld, label.to(cuda), 255, class_weight=None if cw is None else cw.to(cuda),
                                             avg_non_ignore=avg, ohem=(thresh, min_kept))
    mask = pixw.cpu() != 0
    assert 0 < int(mask.sum())
    want = torch.where(mask, torch.ones(()) if cw is None else cw[label.clamp(0, C - 1)], torch.zeros(()))
    assert torch.equal(pixw.cpu(), want)
    loss_r, grad_r = _reference(logit, label, 255, cw, avg, 'mean', mask=mask)
    _check_loss_and_grad('ohem', loss, ld, loss_r, grad_r)


def test_ohem_ties_are_exact(cuda):
    """All-zero logits: every probability is the same value.  The strict `<` keeps nothing when the k-th value decides, and
    everything when the threshold lies above — then bit-equal to the call without a sampler."""
    from rscotr_amd import ops
    B, C, h, w, H, W = 2, 7, 8, 8, 64, 64
    _, label, cw = _inputs(B, C, h, w, H, W)
    zeros, label_d, cw_d = torch.zeros(B, C, h, w, device=cuda), label.to(cuda), cw.to(cuda)
    loss, grad, pixw = _call(ops, zeros, label_d, class_weight=cw_d, ohem=(0.001, 10))
    assert float(loss) == 0.0 and float(grad.abs().max()) == 0.0 and float(pixw.abs().max()) == 0.0
    a = _call(ops, zeros, label_d, class_weight=cw_d, ohem=(0.7, 10))
    b = _call(ops, zeros, label_d, class_weight=cw_d)
    assert float(b[0]) > 0 and all(torch.equal(x, y) for x, y in zip(a, b))


# ---- graph capture and the model ---------------------------------------------------------------------------------------------------
def test_op_captured_in_a_graph_replays_bit_equal(cuda):
    """Forward and backward captured on a side stream as the runner captures an iteration (warm-up on the same stream, then
    torch.cuda.graph), replayed on fresh inputs copied into the static tensors: bit-equal to the eager call."""
    from rscotr_amd import ops
    B, C, h, w, H, W = 2, 7, 8, 8, 64, 64
    logit, label, cw = _inputs(B, C, h, w, H, W)
    cw_d = cw.to(cuda)
    kw = dict(class_weight=cw_d, avg_non_ignore=True, ohem=(0.7, 100))
    s_logit = torch.zeros(B, C, h, w, device=cuda, requires_grad=True)
    s_label = torch.zeros(B, H, W, dtype=torch.long, device=cuda)

    def body():
        loss, acc, pixw = ops.upsample_ce_weighted(s_logit, s_label, 255, **kw)
        (grad,) = torch.autograd.grad(loss * 1.7, s_logit)
        return loss.detach(), grad, pixw, acc

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            body()
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            outs = body()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.Generator().manual_seed(5)
    for trial in range(2):
        lg = (torch.randn(B, C, h, w, generator=g) * 3).to(cuda)
        lb = torch.randint(0, C, (B, H, W), generator=g)
        lb[torch.rand(B, H, W, generator=g) < 0.1] = 255
        lb = lb.to(cuda)
        with torch.no_grad():
            s_logit.copy_(lg)
            s_label.copy_(lb)
        graph.replay()
        torch.cuda.synchronize()
        eager = _call(ops, lg, lb, **kw)
        assert float(outs[0]) > 0 and 0 < int((outs[2] != 0).sum()) < B * H * W
        assert all(torch.equal(x, y) for x, y in zip(outs[:3], eager)), trial


def test_seg_iterations_with_options_graph_equals_eager(cuda):
    """The tiny model with class weights, avg_non_ignore and OHEM on its seg head: two seg iterations (the second one is the
    captured and replayed one when graphs are on) from identical weights on identical batches.  Losses and the seg head's
    parameter gradients are finite and bit-equal between the graphed and the eager runner.  (DropPath off: its draws differ
    between captured and eager RNG streams; a seg-only loader: the two iterations are consecutive.)"""
    import copy
    import numpy as np
    from util import build_model, load_model_cfg
    from rscotr_amd.data import build_synthetic_multidataloader
    from rscotr_amd.runner import build_runner
    cfg, mcfg = load_model_cfg(tiny=True)
    mcfg = copy.deepcopy(mcfg)
    mcfg['backbone']['drop_path_rate'] = 0.0
    g = torch.Generator().manual_seed(11)
    mcfg['seg_head']['loss_decode'] = dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=1.0, avg_non_ignore=True,
                                           class_weight=(0.25 + 4 * torch.rand(mcfg['seg_head']['num_queries'], generator=g)).tolist())
    mcfg['seg_head']['sampler'] = dict(type='OHEMPixelSampler', thresh=0.7, min_kept=500)
    runs = []
    for graphs in (True, False):
        torch.manual_seed(0)
        np.random.seed(2022)
        model = build_model(mcfg).to(cuda)
        loader = build_synthetic_multidataloader(cfg, cuda, size=64, batch_size=2, tasks=('seg',))
        runner = build_runner(model, cfg, loader, graph_tasks=('seg',) if graphs else ())
        logs = [dict(runner.train_iter()['log_vars']) for _ in range(2)]
        torch.cuda.synchronize()
        assert set(runner.graphed) == ({'seg'} if graphs else set())
        grads = {n: p.grad.detach().clone() for n, p in model.seg_head.named_parameters()}
        runner.optimizer.close()
        assert all(math.isfinite(v) for lg in logs for v in lg.values()), logs
        assert grads and all(bool(torch.isfinite(v).all()) for v in grads.values())
        assert any(float(v.abs().max()) > 0 for v in grads.values())
        runs.append((logs, grads))
    (lg, gg), (le, ge) = runs
    print('graphed', lg, '\neager  ', le)
    assert [list(d) for d in lg] == [list(d) for d in le] and any('seg' in k and 'loss' in k for k in lg[0])
    for a, b in zip(lg, le):
        for k in a:
            if 'loss' in k:
                assert a[k] == b[k], (k, a[k], b[k])
    worst = {n: float((gg[n] - ge[n]).abs().max()) for n in gg if not torch.equal(gg[n], ge[n])}
    assert not worst, worst
