"""The fused bilinear upsample + sigmoid focal loss (ops.upsample_focal: rscotr_upsample_focal_fwd / _bwd) and the fused
bilinear upsample + softmax + Tversky loss (ops.upsample_tversky: rscotr_upsample_tversky_fwd / _bwd) against the fp64
restatements of their contracts in tests/seg_focal_tversky_oracle.py, on every path of their kernels, then through
`Mask2FormerHead.losses` and the training step.  Mirrors tests/test_seg_dice_gpu.py.

Gates are those of the family (tests/test_seg_loss_gpu.py): loss within 1e-5 relative (floor 1e-3), d(1.7 loss)/d logit within
1e-4 of the largest reference gradient, cells with an exactly zero reference gradient exactly zero."""
import copy
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from seg_focal_tversky_oracle import dice_inputs, focal_reference, tversky_contract, tversky_reference
from test_seg_dice_gpu import _BASE, _SHAPES, DICE_CHUNKS, DICE_CT
from test_seg_loss_gpu import _REACHES, _uce_blocks

pytestmark = pytest.mark.gpu

_LOSSES = ('focal', 'tversky')


@functools.lru_cache(maxsize=None)
def _inputs(B, C, h, w, H, W, ignore=255):
    return dice_inputs(B, C, h, w, H, W, ignore)


def _dev(v, cuda):
    return v.to(cuda) if torch.is_tensor(v) else v


def _check(cuda, which, logit, label, tag, **kw):
    """One op against its oracle under the family's gates; kw are the op's keyword arguments (tensors on the CPU).
    -> the number of cells whose reference gradient is exactly zero."""
    from rscotr_amd import ops
    op, ref = (ops.upsample_focal, focal_reference) if which == 'focal' else (ops.upsample_tversky, tversky_reference)
    loss_r, grad_r = ref(logit, label, **kw)
    ld = logit.to(cuda).requires_grad_(True)
    loss = op(ld, label.to(cuda), **{k: _dev(v, cuda) for k, v in kw.items()})
    assert loss.dim() == 0 and loss.dtype == torch.float32
    loss_v = float(loss.detach())
    (loss * 1.7).backward()
    grad = ld.grad.cpu()
    assert bool(torch.isfinite(grad).all()) and math.isfinite(loss_v)
    err = float((grad.double() - grad_r).abs().max() / (grad_r.abs().max() + 1e-30))
    print(f'{which} {tag}: loss {loss_v:.8f} ref {loss_r:.8f} rel {abs(loss_v - loss_r) / max(abs(loss_r), 1e-3):.2e}  '
          f'gradient max error {err:.3e} of the largest reference gradient {float(grad_r.abs().max()):.3e}')
    assert abs(loss_v - loss_r) <= 1e-5 * max(abs(loss_r), 1e-3), (loss_v, loss_r)
    assert err < 1e-4, err
    untouched = grad_r == 0
    assert bool((grad[untouched] == 0).all()), int((grad[untouched] != 0).sum())
    return int(untouched.sum())


@pytest.mark.parametrize('use_cw', [False, True])
@pytest.mark.parametrize('which', _LOSSES)
@pytest.mark.parametrize('reaches,B,C,h,w,H,W', _SHAPES)
def test_backward_paths(cuda, reaches, B, C, h, w, H, W, which, use_cw):
    assert _REACHES[reaches](h, w, H, W, C), (reaches, _uce_blocks(h, w, H, W))
    if C > 128:
        assert C % DICE_CT != 0  # a partial register pass of the Tversky forward kernel as well
    logit, label, cw = _inputs(B, C, h, w, H, W)
    untouched = _check(cuda, which, logit, label, reaches, class_weight=cw if use_cw else None)
    if reaches == 'staged_downsample':
        # cells no output pixel touches have an exactly zero reference gradient: _check has required exact zeros there
        ones = torch.ones(1, 1, h, w, dtype=torch.float64, requires_grad=True)
        F.interpolate(ones, size=(H, W), mode='bilinear', align_corners=False).sum().backward()
        no_pixel = int((ones.grad == 0).sum())
        assert no_pixel >= 37 and untouched >= no_pixel * B * C, (no_pixel, untouched)


@pytest.mark.parametrize('which', _LOSSES)
def test_forward_grid_stride(cuda, which):
    """More pixels per image than one trip of the capped Tversky forward grid covers (DICE_CHUNKS workgroups of 256 per image)."""
    B, C, h, w, H, W = 2, 2, 8, 8, 192, 184
    assert H * W > DICE_CHUNKS * 256
    logit, label, cw = _inputs(B, C, h, w, H, W)
    _check(cuda, which, logit, label, 'grid_stride', class_weight=cw)


# ---- focal ---------------------------------------------------------------------------------------------------------------------
_ALPHA7 = [0.1, 0.25, 0.4, 0.5, 0.6, 0.75, 0.9]


@pytest.mark.parametrize('gamma,alpha,reduction,loss_weight,ignore', [
    (0.0, 0.5, 'mean', 1.0, 255), (1.5, 0.25, 'mean', 3.0, 255), (2.0, _ALPHA7, 'sum', 1.0, 255), (2.0, 0.25, 'mean', 1.0, 5),
    (1.5, _ALPHA7, 'sum', 3.0, 5), (0.0, _ALPHA7, 'mean', 3.0, -100)])
def test_focal_options(cuda, gamma, alpha, reduction, loss_weight, ignore):
    """gamma (0: q^0 = 1 with a finite gradient), alpha as a scalar and per class, both reductions, loss_weight, and an
    ignore_index that is a channel (5 of C = 7: the pixels are masked, the channel still counts as a negative) or negative."""
    logit, label, cw = _inputs(*_BASE, ignore)
    assert int((label == ignore).sum()) > 0
    alpha = torch.tensor(alpha) if isinstance(alpha, list) else alpha
    _check(cuda, 'focal', logit, label, f'gamma {gamma} reduction {reduction} lw {loss_weight} ignore {ignore}', ignore_index=ignore,
           gamma=gamma, alpha=alpha, class_weight=cw, reduction=reduction, loss_weight=loss_weight)


def test_focal_labels_outside_the_channels_are_all_negative(cuda):
    from rscotr_amd import ops
    logit, label, cw = _inputs(*_BASE)
    label = label.clone()
    label[0, 8:24, 8:40] = 9          # >= C = 7, not ignored
    label[1, 40:48, :16] = 1000
    label[1, :8, 48:] = -3            # below 0
    _check(cuda, 'focal', logit, label, 'outside', class_weight=cw)
    # the same loss as with those pixels moved to a label no channel has
    other = label.clone()
    other[(label < 0) | ((label >= 7) & (label != 255))] = 77
    a = ops.upsample_focal(logit.to(cuda), label.to(cuda))
    b = ops.upsample_focal(logit.to(cuda), other.to(cuda))
    assert torch.equal(a, b)


@pytest.mark.parametrize('which', _LOSSES)
def test_one_image_all_ignored_and_an_absent_class(cuda, which):
    logit, label, cw = _inputs(*_BASE)
    label = label.clone()
    label[0] = 255                    # every pixel of image 0 ignored: no term (focal), num = den = smooth (Tversky)
    label[1][label[1] == 3] = 2       # class 3 absent from image 1
    assert not bool((label[1] == 3).any())
    for kw in ((dict(smooth=1.0), dict(smooth=1e-3)) if which == 'tversky' else (dict(),)):
        _check(cuda, which, logit, label, f'all-ignored image {kw}', class_weight=cw, **kw)
    # image 0 receives no gradient at all
    from rscotr_amd import ops
    ld = logit.to(cuda).requires_grad_(True)
    op = ops.upsample_focal if which == 'focal' else ops.upsample_tversky
    op(ld, label.to(cuda)).backward()
    assert not bool(ld.grad[0].any()) and bool(ld.grad[1].any())


def test_focal_magnitudes(cuda):
    """Logits of +-200: a perfect prediction costs nothing, its mirror image is finite.  Catches an overflowing sigmoid or exp(u)."""
    from rscotr_amd import ops
    label = torch.randint(0, 5, (2, 16, 16), generator=torch.Generator().manual_seed(3))
    logit = 400.0 * F.one_hot(label, 5).permute(0, 3, 1, 2).float() - 200.0
    for gamma in (2.0, 0.0):
        loss = ops.upsample_focal(logit.to(cuda), label.to(cuda), gamma=gamma)
        print('perfect prediction, gamma', gamma, float(loss))
        assert 0 <= float(loss) <= 1e-6
        _check(cuda, 'focal', logit, label, f'perfect gamma {gamma}', gamma=gamma)
        ld = (-logit).to(cuda).requires_grad_(True)
        loss = ops.upsample_focal(ld, label.to(cuda), gamma=gamma)
        loss.backward()
        print('mirrored, gamma', gamma, float(loss))
        assert math.isfinite(float(loss)) and float(loss) > 1 and bool(torch.isfinite(ld.grad).all())
        _check(cuda, 'focal', -logit, label, f'mirrored gamma {gamma}', gamma=gamma)


# ---- Tversky -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('alpha,beta', [(0.3, 0.7), (0.5, 0.5), (0.9, 0.1)])
@pytest.mark.parametrize('smooth,loss_weight,ignore', [(1.0, 1.0, 255), (1e-3, 3.0, 255), (1.0, 3.0, 5), (1e-3, 1.0, 5)])
def test_tversky_options(cuda, alpha, beta, smooth, loss_weight, ignore):
    """alpha / beta, smooth, loss_weight, and TverskyLoss's own ignore_index: 5 of C = 7 is a channel (skipped; the divisor stays
    7) AND the value that masks the sums."""
    logit, label, cw = _inputs(*_BASE, ignore)
    assert int((label == ignore).sum()) > 0
    _check(cuda, 'tversky', logit, label, f'a {alpha} b {beta} smooth {smooth} lw {loss_weight} ignore {ignore}', ignore_index=ignore,
           alpha=alpha, beta=beta, smooth=smooth, class_weight=cw, loss_weight=loss_weight)


def test_tversky_labels_past_the_last_channel_are_clamped(cuda):
    logit, label, cw = _inputs(*_BASE)
    label = label.clone()
    label[0, 8:24, 8:40] = 9          # >= C = 7, not ignored: counts for channel 6
    label[1, 40:48, :16] = 1000
    label[1, :8, 48:] = -3            # below 0: channel 0
    _check(cuda, 'tversky', logit, label, 'clamped', class_weight=cw)


def test_tversky_at_one_half_is_the_soft_dice_ratio(cuda):
    """alpha = beta = 1/2, smooth 1, nothing ignored: the oracle value is 1 - (2 TP + 2) / (sum p + sum t + 2) in fp64, and the
    kernels meet it."""
    B, C, h, w, H, W = _BASE
    logit, label, cw = dice_inputs(B, C, h, w, H, W, ignored=0.0)
    p = F.softmax(F.interpolate(logit.double(), size=(H, W), mode='bilinear', align_corners=False), dim=1)
    t = F.one_hot(label, C).permute(0, 3, 1, 2).double()
    ratio = (2 * (p * t).flatten(2).sum(-1) + 2) / (p.flatten(2).sum(-1) + t.flatten(2).sum(-1) + 2)
    want = float(((1 - ratio).mean(0) * cw.double()).sum() / C)
    got = float(tversky_contract(logit, label, 255, 0.5, 0.5, 1.0, cw)[0].detach())
    assert abs(got - want) <= 1e-12 * want
    _check(cuda, 'tversky', logit, label, 'one half', alpha=0.5, beta=0.5, smooth=1.0, class_weight=cw)


def test_closed_forms(cuda):
    from rscotr_amd import ops
    # all-zero logits (1,4,2,2), all-zero label (1,8,8)
    z, y = torch.zeros(1, 4, 2, 2, device=cuda), torch.zeros(1, 8, 8, dtype=torch.long, device=cuda)
    loss, want = ops.upsample_focal(z, y), 0.125 * math.log(2)
    print('focal uniform:', float(loss), want)
    assert abs(float(loss) - want) <= 1e-5 * want
    loss, want = ops.upsample_tversky(z, y), ((1 - 17 / 50.6) + 3 * (1 - 1 / 5.8)) / 4
    print('tversky uniform:', float(loss), want)
    assert abs(float(loss) - want) <= 1e-5 * want
    # a perfect prediction with nothing ignored: Tversky 0
    label = torch.randint(0, 5, (2, 16, 16), generator=torch.Generator().manual_seed(3))
    logit = 200.0 * F.one_hot(label, 5).permute(0, 3, 1, 2).float()
    assert abs(float(ops.upsample_tversky(logit.to(cuda), label.to(cuda)))) <= 1e-6
    # every pixel ignored: both 0 with a zero gradient
    logit, label, _ = _inputs(*_BASE)
    for op in (ops.upsample_focal, ops.upsample_tversky):
        ld = logit.to(cuda).requires_grad_(True)
        loss = op(ld, torch.full_like(label, 255).to(cuda))
        loss.backward()
        assert float(loss) == 0.0 and not bool(ld.grad.any())


# ---- reproducibility and capture -----------------------------------------------------------------------------------------------
def _op_kw(ops, which, cw_d, cuda):
    if which == 'focal':
        return ops.upsample_focal, dict(class_weight=cw_d, gamma=1.5, alpha=torch.tensor(_ALPHA7, device=cuda), loss_weight=3.0)
    return ops.upsample_tversky, dict(class_weight=cw_d, smooth=1.0, loss_weight=3.0)


def _call(op, logit, label_d, **kw):
    ld = logit.detach().clone().requires_grad_(True)
    loss = op(ld, label_d, **kw)
    (loss * 1.7).backward()
    return loss.detach(), ld.grad


@pytest.mark.parametrize('which', _LOSSES)
@pytest.mark.parametrize('B,C,h,w,H,W', [_SHAPES[0][1:], _SHAPES[1][1:]])
def test_two_calls_are_bit_equal(cuda, B, C, h, w, H, W, which):
    from rscotr_amd import ops
    logit, label, cw = _inputs(B, C, h, w, H, W)
    ld, label_d = logit.to(cuda), label.to(cuda)
    op, kw = _op_kw(ops, which, cw.to(cuda), cuda)
    if C != 7:
        kw.pop('alpha', None)
    a = _call(op, ld, label_d, **kw)
    b = _call(op, ld, label_d, **kw)
    assert float(a[0]) > 0 and float(a[1].abs().max()) > 0
    assert all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize('which', _LOSSES)
def test_op_captured_in_a_graph_replays_bit_equal(cuda, which):
    """Forward and backward captured on a side stream as the runner captures an iteration (warm-up on the same stream, then
    torch.cuda.graph), replayed on fresh inputs copied into the static tensors: bit-equal to the eager call."""
    from rscotr_amd import ops
    B, C, h, w, H, W = _BASE
    _, _, cw = _inputs(B, C, h, w, H, W)
    op, kw = _op_kw(ops, which, cw.to(cuda), cuda)
    s_logit = torch.zeros(B, C, h, w, device=cuda, requires_grad=True)
    s_label = torch.zeros(B, H, W, dtype=torch.long, device=cuda)

    def body():
        loss = op(s_logit, s_label, **kw)
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
        eager = _call(op, lg, lb, **kw)
        assert float(outs[0]) > 0 and float(outs[1].abs().max()) > 0
        assert all(torch.equal(x, y) for x, y in zip(outs, eager)), trial


# ---- the head and the step -----------------------------------------------------------------------------------------------------
def test_head_losses_with_ce_focal_and_tversky(cuda):
    """`Mask2FormerHead.losses` with [CE(class_weight), Focal, Tversky]: loss_ce and acc_seg are the CE-only head's bits, the
    logit gradient is the sum of the three ops' gradients, and a configured OHEM sampler does not reach the Tversky entry."""
    from rscotr_amd import ops
    from test_seg_loss_weighted_cpu import _CW100, _head
    B, C, h, w, H, W = 2, 100, 8, 8, 64, 64
    logit, label, _ = _inputs(B, C, h, w, H, W)
    ld, seg_label = logit.to(cuda), label.to(cuda).unsqueeze(1)
    ce = dict(type='CrossEntropyLoss', loss_name='loss_ce', class_weight=_CW100, loss_weight=1.0)
    focal = dict(type='FocalLoss', loss_name='loss_focal', gamma=1.5, alpha=0.25, loss_weight=2.0)
    tversky = dict(type='TverskyLoss', loss_name='loss_tversky', loss_weight=3.0)

    def run(**over):
        head, _ = _head(**over)
        x = ld.clone().requires_grad_(True)
        out = head.losses(x, seg_label)
        sum(v for k, v in out.items() if 'loss' in k).backward()
        return out, x.grad

    allthree, g_all = run(loss_decode=[ce, focal, tversky])
    only, g_ce = run(loss_decode=[ce])
    assert list(allthree) == ['loss_ce', 'loss_focal', 'loss_tversky', 'acc_seg'] and list(only) == ['loss_ce', 'acc_seg']
    assert torch.equal(allthree['loss_ce'], only['loss_ce']) and torch.equal(allthree['acc_seg'], only['acc_seg'])
    x = ld.clone().requires_grad_(True)
    loss_f = ops.upsample_focal(x, seg_label.squeeze(1), gamma=1.5, alpha=0.25, loss_weight=2.0)
    (g_focal,) = torch.autograd.grad(loss_f, x)
    loss_t = ops.upsample_tversky(x, seg_label.squeeze(1), loss_weight=3.0)
    (g_tversky,) = torch.autograd.grad(loss_t, x)
    assert torch.equal(allthree['loss_focal'], loss_f) and float(loss_f.detach()) > 0
    assert torch.equal(allthree['loss_tversky'], loss_t) and float(loss_t.detach()) > 0
    # (autograd accumulates into the leaf in the order it runs the backward nodes, the latest one first: Tversky, focal, CE)
    print('gradient sum, largest difference by order of addition:',
          {k: float((g_all - v).abs().max()) for k, v in (('(t+f)+c', (g_tversky + g_focal) + g_ce), ('(c+f)+t', (g_ce + g_focal) + g_tversky),
                                                          ('(c+t)+f', (g_ce + g_tversky) + g_focal))})
    assert torch.equal(g_all, (g_tversky + g_focal) + g_ce)
    sampler = dict(type='OHEMPixelSampler', thresh=0.7, min_kept=100)
    ohem, _ = run(loss_decode=[ce, tversky], sampler=sampler)
    ohem_ce, _ = run(loss_decode=[ce], sampler=sampler)
    assert torch.equal(ohem['loss_tversky'], allthree['loss_tversky'])
    assert torch.equal(ohem['loss_ce'], ohem_ce['loss_ce']) and torch.equal(ohem['acc_seg'], allthree['acc_seg'])
    # no CE entry: the accuracy comes from one unweighted forward without a graph
    alone, g_alone = run(loss_decode=[focal, tversky])
    assert list(alone) == ['loss_focal', 'loss_tversky', 'acc_seg'] and not alone['acc_seg'].requires_grad
    assert torch.equal(alone['acc_seg'], only['acc_seg']) and torch.equal(g_alone, g_focal + g_tversky)


def test_seg_iterations_with_ce_focal_and_tversky_graph_equals_eager(cuda):
    """The tiny model with [CE, Focal(loss_weight=2), Tversky(loss_weight=3)] on its seg head: two seg iterations (the second one
    is the captured and replayed one when graphs are on) from identical weights on identical batches.  Losses and the seg head's
    parameter gradients are finite and bit-equal between the graphed and the eager runner; log_vars holds seg.*.loss_focal and
    seg.*.loss_tversky.  A third, eager runner with the default CE-only head on the same weights and batch gives the same loss_ce
    and acc_seg bits in its first iteration.  (DropPath off: its draws differ between captured and eager RNG streams; a seg-only
    loader: the two iterations are consecutive.)"""
    from util import build_model, load_model_cfg
    from rscotr_amd.data import build_synthetic_multidataloader
    from rscotr_amd.runner import build_runner
    cfg, mcfg = load_model_cfg(tiny=True)
    mcfg = copy.deepcopy(mcfg)
    mcfg['backbone']['drop_path_rate'] = 0.0
    mcfg['task_weight'] = dict(cls=1, det=1, seg=2)  # (a power of two: the scaled log values stay exact)
    default_loss = copy.deepcopy(mcfg['seg_head']['loss_decode'])
    three = [dict(type='CrossEntropyLoss', loss_name='loss_ce', loss_weight=1.0),
             dict(type='FocalLoss', loss_name='loss_focal', loss_weight=2.0),
             dict(type='TverskyLoss', loss_name='loss_tversky', loss_weight=3.0)]
    runs = []
    for graphs, loss_decode, iters in ((True, three, 2), (False, three, 2), (False, default_loss, 1)):
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
        (k_focal,) = [k for k in d if k.startswith('seg.') and k.endswith('.loss_focal')]
        (k_tversky,) = [k for k in d if k.startswith('seg.') and k.endswith('.loss_tversky')]
        k_ce = k_focal[:-len('loss_focal')] + 'loss_ce'
        assert d[k_focal] > 0 and d[k_tversky] > 0 and d[k_ce] > 0
    # the default head on the same weights and batch
    k_ce = [k for k in ld[0] if k.endswith('.loss_ce')][0]
    assert not any(k.endswith('loss_focal') or k.endswith('loss_tversky') for k in ld[0])
    assert ld[0][k_ce] == le[0][k_ce] and ld[0][k_ce.replace('loss_ce', 'acc_seg')] == le[0][k_ce.replace('loss_ce', 'acc_seg')]
