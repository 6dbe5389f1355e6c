"""The fused bilinear upsample + softmax + Dice loss (ops.upsample_dice: rscotr_upsample_dice_fwd / _bwd) against the fp64
restatement of the contract in tests/seg_dice_oracle.py, on every path of its kernels, then through `Mask2FormerHead.losses`
and the training step.

Gates are those of the cross-entropy tests (tests/test_seg_loss_gpu.py): loss within 1e-5 relative, d(1.7 loss)/d logit within
1e-4 of the largest reference gradient, cells with an exactly zero reference gradient exactly zero."""
import copy
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from seg_dice_oracle import dice_inputs, dice_reference
from test_seg_loss_gpu import _REACHES, _uce_blocks

pytestmark = pytest.mark.gpu

# csrc/seg_dice.hip: workgroups per image of the forward launch at most (256 pixels each per trip) and the classes of one
# register pass; the backward gather has the block geometry of the cross-entropy one (csrc/seg_upsample.h), so the reach
# predicates of tests/test_seg_loss_gpu.py apply as they stand
DICE_CHUNKS = 128
DICE_CT = 16

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
_BASE = _SHAPES[0][1:]


@functools.lru_cache(maxsize=None)
def _inputs(B, C, h, w, H, W, ignore=255):
    return dice_inputs(B, C, h, w, H, W, ignore)


def _check(cuda, logit, label, ignore=255, smooth=1.0, cw=None, loss_weight=1.0, tag='upsample_dice'):
    from rscotr_amd import ops
    loss_r, grad_r = dice_reference(logit, label, ignore, smooth, cw, loss_weight)
    ld = logit.to(cuda).requires_grad_(True)
    loss = ops.upsample_dice(ld, label.to(cuda), ignore, smooth=smooth, class_weight=None if cw is None else cw.to(cuda),
                             loss_weight=loss_weight)
    assert loss.dim() == 0 and loss.dtype == torch.float32
    loss_v = float(loss.detach())
    (loss * 1.7).backward()
    grad = ld.grad.cpu()
    assert bool(torch.isfinite(grad).all()) and math.isfinite(loss_v)
    err = float((grad.double() - grad_r).abs().max() / (grad_r.abs().max() + 1e-30))
    print(f'{tag}: loss {loss_v:.8f} ref {loss_r:.8f} rel {abs(loss_v - loss_r) / max(abs(loss_r), 1e-3):.2e}  '
          f'gradient max error {err:.3e} of the largest reference gradient {float(grad_r.abs().max()):.3e}')
    assert abs(loss_v - loss_r) <= 1e-5 * max(abs(loss_r), 1e-3), (loss_v, loss_r)
    assert err < 1e-4, err
    untouched = grad_r == 0
    assert bool((grad[untouched] == 0).all()), int((grad[untouched] != 0).sum())
    return int(untouched.sum())


@pytest.mark.parametrize('use_cw', [False, True])
@pytest.mark.parametrize('reaches,B,C,h,w,H,W', _SHAPES)
def test_dice_backward_paths(cuda, reaches, B, C, h, w, H, W, use_cw):
    assert _REACHES[reaches](h, w, H, W, C), (reaches, _uce_blocks(h, w, H, W))
    if C > 128:
        assert C % DICE_CT != 0  # a partial register pass of the forward kernel as well
    logit, label, cw = _inputs(B, C, h, w, H, W)
    untouched = _check(cuda, logit, label, cw=cw if use_cw else None, tag=reaches)
    if reaches == 'staged_downsample':
        # cells no output pixel touches (13 x 9 cells, 5 x 4 pixels of 2 x 2 taps: at least 117 - 80 = 37 per channel) have
        # an exactly zero reference gradient, so _check has required exact zeros of the kernel there
        ones = torch.ones(1, 1, h, w, dtype=torch.float64, requires_grad=True)
        F.interpolate(ones, size=(H, W), mode='bilinear', align_corners=False).sum().backward()
        no_pixel = int((ones.grad == 0).sum())
        assert no_pixel >= 37 and untouched >= no_pixel * B * C, (no_pixel, untouched)


def test_dice_forward_grid_stride(cuda):
    """More pixels per image than one trip of the capped forward grid covers (DICE_CHUNKS workgroups of 256 per image)."""
    B, C, h, w, H, W = 2, 2, 8, 8, 192, 184
    assert H * W > DICE_CHUNKS * 256
    logit, label, cw = _inputs(B, C, h, w, H, W)
    _check(cuda, logit, label, cw=cw, tag='grid_stride')


@pytest.mark.parametrize('smooth,loss_weight,ignore', [
    (1e-3, 1.0, 255), (1.0, 3.0, 255), (1.0, 1.0, 5), (1e-3, 3.0, 5), (1.0, 1.0, -100)])
def test_dice_options(cuda, smooth, loss_weight, ignore):
    """smooth, loss_weight, and DiceLoss's own ignore_index: 5 of C = 7 is a channel (skipped; the divisor stays 7) AND the
    value that masks the numerator."""
    logit, label, cw = _inputs(*_BASE, ignore)
    assert int((label == ignore).sum()) > 0
    _check(cuda, logit, label, ignore, smooth, cw, loss_weight, tag=f'smooth {smooth} lw {loss_weight} ignore {ignore}')


def test_dice_labels_past_the_last_channel_are_clamped(cuda):
    logit, label, cw = _inputs(*_BASE)
    label = label.clone()
    label[0, 8:24, 8:40] = 9          # >= C = 7, not ignored: counts for channel 6
    label[1, 40:48, :16] = 1000
    label[1, :8, 48:] = -3            # below 0: channel 0
    _check(cuda, logit, label, cw=cw, tag='clamped')


def test_dice_one_image_all_ignored_and_an_absent_class(cuda):
    logit, label, cw = _inputs(*_BASE)
    label = label.clone()
    label[0] = 255                    # every pixel of image 0 ignored: finite, num = smooth, den keeps p^2 and t of channel 6
    label[1][label[1] == 3] = 2       # class 3 absent from image 1
    assert not bool((label[1] == 3).any())
    for smooth in (1.0, 1e-3):
        _check(cuda, logit, label, smooth=smooth, cw=cw, tag=f'all-ignored image, smooth {smooth}')


def test_dice_closed_forms(cuda):
    from rscotr_amd import ops
    # a perfect prediction with nothing ignored: loss 0
    label = torch.randint(0, 5, (2, 16, 16), generator=torch.Generator().manual_seed(3))
    logit = 200.0 * F.one_hot(label, 5).permute(0, 3, 1, 2).float()
    loss = ops.upsample_dice(logit.to(cuda), label.to(cuda))
    print('perfect prediction:', float(loss))
    assert abs(float(loss)) <= 1e-6
    # all-zero logits (1,4,2,2), all-zero label (1,8,8)
    loss = ops.upsample_dice(torch.zeros(1, 4, 2, 2, device=cuda), torch.zeros(1, 8, 8, dtype=torch.long, device=cuda))
    want = ((1 - 33 / 69) + 3 * (1 - 1 / 5)) / 4
    print('uniform:', float(loss), want)
    assert abs(float(loss) - want) <= 1e-5 * want


def _call(ops, logit, label_d, **kw):
    ld = logit.detach().clone().requires_grad_(True)
    loss = ops.upsample_dice(ld, label_d, **kw)
    (loss * 1.7).backward()
    return loss.detach(), ld.grad


@pytest.mark.parametrize('B,C,h,w,H,W', [_SHAPES[0][1:], _SHAPES[1][1:]])
def test_dice_two_calls_are_bit_equal(cuda, B, C, h, w, H, W):
    from rscotr_amd import ops
    logit, label, cw = _inputs(B, C, h, w, H, W)
    ld, label_d, cw_d = logit.to(cuda), label.to(cuda), cw.to(cuda)
    a = _call(ops, ld, label_d, class_weight=cw_d, loss_weight=3.0)
    b = _call(ops, ld, label_d, class_weight=cw_d, loss_weight=3.0)
    assert float(a[0]) > 0 and float(a[1].abs().max()) > 0
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_dice_op_captured_in_a_graph_replays_bit_equal(cuda):
    """Forward and backward captured on a side stream as the runner captures an iteration (warm-up on the same stream, then
    torch.cuda.graph), replayed on fresh inputs copied into the static tensors: bit-equal to the eager call."""
    from rscotr_amd import ops
    B, C, h, w, H, W = _BASE
    _, _, cw = _inputs(B, C, h, w, H, W)
    kw = dict(class_weight=cw.to(cuda), smooth=1.0, loss_weight=3.0)
    s_logit = torch.zeros(B, C, h, w, device=cuda, requires_grad=True)
    s_label = torch.zeros(B, H, W, dtype=torch.long, device=cuda)

    def body():
        loss = ops.upsample_dice(s_logit, s_label, **kw)
        (grad,) = torch.autograd.grad(loss * 1.7, s_logit)
        return loss.detach(), grad

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
        assert float(outs[0]) > 0 and float(outs[1].abs().max()) > 0
        assert all(torch.equal(x, y) for x, y in zip(outs, eager)), trial


# ---- the head and the step -----------------------------------------------------------------------------------------------------
def test_head_losses_with_ce_and_dice(cuda):
    """`Mask2FormerHead.losses` with [CE(class_weight), Dice]: loss_ce and acc_seg are the CE-only head's bits, the logit gradient
    is the sum of the two ops' gradients, and a configured OHEM sampler does not reach the Dice entry."""
    from rscotr_amd import ops
    from test_seg_loss_weighted_cpu import _CW100, _head
    B, C, h, w, H, W = 2, 100, 8, 8, 64, 64
    logit, label, _ = _inputs(B, C, h, w, H, W)
    ld, seg_label = logit.to(cuda), label.to(cuda).unsqueeze(1)
    ce = dict(type='CrossEntropyLoss', loss_name='loss_ce', class_weight=_CW100, loss_weight=1.0)
    dice = dict(type='DiceLoss', loss_name='loss_dice', loss_weight=3.0)

    def run(**over):
        head, _ = _head(**over)
        x = ld.clone().requires_grad_(True)
        out = head.losses(x, seg_label)
        sum(v for k, v in out.items() if 'loss' in k).backward()
        return out, x.grad

    both, g_both = run(loss_decode=[ce, dice])
    only, g_ce = run(loss_decode=[ce])
    assert list(both) == ['loss_ce', 'loss_dice', 'acc_seg'] and list(only) == ['loss_ce', 'acc_seg']
    assert torch.equal(both['loss_ce'], only['loss_ce']) and torch.equal(both['acc_seg'], only['acc_seg'])
    x = ld.clone().requires_grad_(True)
    loss_d = ops.upsample_dice(x, seg_label.squeeze(1), loss_weight=3.0)
    (g_dice,) = torch.autograd.grad(loss_d, x)
    assert torch.equal(both['loss_dice'], loss_d) and float(loss_d.detach()) > 0
    assert torch.equal(g_both, g_ce + g_dice)
    sampler = dict(type='OHEMPixelSampler', thresh=0.7, min_kept=100)
    ohem, _ = run(loss_decode=[ce, dice], sampler=sampler)
    ohem_ce, _ = run(loss_decode=[ce], sampler=sampler)
    assert torch.equal(ohem['loss_dice'], both['loss_dice'])
    assert torch.equal(ohem['loss_ce'], ohem_ce['loss_ce']) and torch.equal(ohem['acc_seg'], both['acc_seg'])
    # no CE entry: the accuracy comes from one unweighted forward without a graph
    alone, g_alone = run(loss_decode=[dice])
    assert list(alone) == ['loss_dice', 'acc_seg'] and not alone['acc_seg'].requires_grad
    assert torch.equal(alone['acc_seg'], only['acc_seg']) and torch.equal(g_alone, g_dice)


def test_seg_iterations_with_ce_and_dice_graph_equals_eager(cuda):
    """The tiny model with [CE, Dice(loss_weight=3)] on its seg head: two seg iterations (the second one is the captured and
    replayed one when graphs are on) from identical weights on identical batches.  Losses and the seg head's parameter gradients
    are finite and bit-equal between the graphed and the eager runner; log_vars holds seg.*.loss_dice and loss is
    task_weight * (loss_ce + loss_dice).  A third, eager runner with the default CE-only head on the same weights and batch gives
    the same loss_ce and acc_seg bits in its first iteration: the CE entry of the list takes the default path.  (DropPath off:
    its draws differ between captured and eager RNG streams; a seg-only loader: the two iterations are consecutive.)"""
    from util import build_model, load_model_cfg
    from rscotr_amd.data import build_synthetic_multidataloader
    from rscotr_amd.runner import build_runner
    cfg, mcfg = load_model_cfg(tiny=True)
    mcfg = copy.deepcopy(mcfg)
    mcfg['backbone']['drop_path_rate'] = 0.0
    mcfg['task_weight'] = dict(cls=1, det=1, seg=2)  # (a power of two: the scaled log values stay exact)
    default_loss = copy.deepcopy(mcfg['seg_head']['loss_decode'])
    ce_dice = [dict(type='CrossEntropyLoss', loss_name='loss_ce', loss_weight=1.0),
               dict(type='DiceLoss', loss_name='loss_dice', loss_weight=3.0)]
    runs = []
    for graphs, loss_decode, iters in ((True, ce_dice, 2), (False, ce_dice, 2), (False, default_loss, 1)):
        mcfg['seg_head']['loss_decode'] = loss_decode
        torch.manual_seed(0)
        np.random.seed(2022)
        model = build_model(mcfg).to(cuda)
        loader = build_synthetic_multidataloader(cfg, cuda, size=64, batch_size=2, tasks=('seg',))
        runner = build_runner(model, cfg, loader, graph_tasks=('seg',) if graphs else ())
        logs = [dict(runner.train_iter()['log_vars']) for _ in range(iters)]
        torch.cuda.synchronize()
        assert set(runner.graphed) == ({'seg'} if graphs else set())
        grads = {n: p.grad.detach().clone() for n, p in model.seg_head.named_parameters()}
        runner.optimizer.close()
        assert all(math.isfinite(v) for lg in logs for v in lg.values()), logs
        assert grads and all(bool(torch.isfinite(v).all()) for v in grads.values())
        assert any(float(v.abs().max()) > 0 for v in grads.values())
        runs.append((logs, grads))
    (lg, gg), (le, ge), (ld, _) = runs
    print('graphed', lg, '\neager  ', le, '\ndefault', ld)
    assert [list(d) for d in lg] == [list(d) for d in le]
    for a, b in zip(lg, le):
        for k in a:
            if 'loss' in k:
                assert a[k] == b[k], (k, a[k], b[k])
    worst = {n: float((gg[n] - ge[n]).abs().max()) for n in gg if not torch.equal(gg[n], ge[n])}
    assert not worst, worst
    for d in lg:
        (k_dice,) = [k for k in d if k.startswith('seg.') and k.endswith('.loss_dice')]
        k_ce = k_dice[:-len('loss_dice')] + 'loss_ce'
        (k_loss,) = [k for k in d if k.startswith('seg.') and k.endswith('.loss')]
        assert d[k_dice] > 0 and d[k_ce] > 0
        assert d[k_loss] == float(np.float32(d[k_ce]) + np.float32(d[k_dice])), d
    # the default head on the same weights and batch
    k_ce = [k for k in ld[0] if k.endswith('.loss_ce')][0]
    assert not any(k.endswith('loss_dice') for k in ld[0])
    assert ld[0][k_ce] == le[0][k_ce] and ld[0][k_ce.replace('loss_ce', 'acc_seg')] == le[0][k_ce.replace('loss_ce', 'acc_seg')]
