"""The fused bilinear upsample + softmax + Lovasz-softmax loss (ops.upsample_lovasz: rscotr_upsample_lovasz_fwd / _bwd) against
the fp64 restatement of the contract in tests/seg_lovasz_oracle.py: on every path of the backward gather, at the boundaries of the
segmented device sort, on the edge cases of the contract, on tied errors, then reproducibility, `Mask2FormerHead.losses` and the
training step.

Gates are those of the other seg-loss tests (tests/test_seg_loss_gpu.py): loss within 1e-5 relative, d(1.7 loss)/d logit within
1e-4 of the largest reference gradient, cells with an exactly zero reference gradient exactly zero.  (The oracle run in fp32
differs from the fp64 one by at most 1e-7 / 2e-5 there: swaps of nearly tied errors sit well inside the gate.)"""
import copy
import functools
import math

import numpy as np
import pytest
import torch

from seg_lovasz_oracle import lovasz_inputs, lovasz_reference
from test_seg_dice_gpu import _SHAPES
from test_seg_loss_gpu import _REACHES, _uce_blocks

pytestmark = pytest.mark.gpu

# csrc/seg_lovasz.hip: the elements one wavefront ranks in a sort pass (one histogram column) and the elements of a sort
# workgroup (4 wavefronts); the scan over the sorted order works in tiles of LOV_SCAN.  The backward gather has the block
# geometry of the cross-entropy one (csrc/seg_upsample.h): the reach predicates of tests/test_seg_loss_gpu.py apply as they stand
LOV_TILE = 2048
LOV_WG = 8192
LOV_SCAN = 2048
_BASE = _SHAPES[0][1:]


@functools.lru_cache(maxsize=None)
def _inputs(B, C, h, w, H, W, ignore=255):
    return lovasz_inputs(B, C, h, w, H, W, ignore)


def _check(cuda, logit, label, ignore=255, classes='present', per_image=False, cw=None, loss_weight=1.0, reduction=None,
           tag='upsample_lovasz', ref=None):
    from rscotr_amd import ops
    reduction = reduction or ('mean' if per_image else 'none')
    loss_r, grad_r = ref if ref is not None else lovasz_reference(logit, label, ignore, classes, per_image, cw, reduction, loss_weight)
    ld = logit.to(cuda).requires_grad_(True)
    loss = ops.upsample_lovasz(ld, label.to(cuda), ignore, classes=classes, per_image=per_image,
                               class_weight=None if cw is None else cw.to(cuda), reduction=reduction, loss_weight=loss_weight)
    assert loss.dim() == 0 and loss.dtype == torch.float32
    loss_v = float(loss.detach())
    (loss * 1.7).backward()
    grad = ld.grad.cpu()
    assert bool(torch.isfinite(grad).all()) and math.isfinite(loss_v)
    err = float((grad.double() - grad_r).abs().max() / (grad_r.abs().max() + 1e-30))
    print(f'{tag}: loss {loss_v:.8f} ref {loss_r:.8f} rel {abs(loss_v - loss_r) / max(abs(loss_r), 1e-3):.2e}  '
          f'gradient max error {err:.3e} of the largest reference gradient {float(grad_r.abs().max()):.3e}')
    assert abs(loss_v - loss_r) <= 1e-5 * max(abs(loss_r), 1e-3), (loss_v, loss_r)
    if float(grad_r.abs().max()) > 0:
        assert err < 1e-4, err
    untouched = grad_r == 0
    assert bool((grad[untouched] == 0).all()), int((grad[untouched] != 0).sum())
    return loss_v


def test_built_sort_constants(cuda):
    from rscotr_amd import ops
    from rscotr_amd.ops.core import lib
    assert (lib.rscotr_upsample_lovasz_sort_tile(), lib.rscotr_upsample_lovasz_sort_workgroup()) == (LOV_TILE, LOV_WG)
    assert (ops.LOVASZ_SORT_TILE, ops.LOVASZ_SORT_WORKGROUP) == (LOV_TILE, LOV_WG)


@pytest.mark.parametrize('per_image', [False, True])
@pytest.mark.parametrize('use_cw', [False, True])
@pytest.mark.parametrize('reaches,B,C,h,w,H,W', _SHAPES)
def test_lovasz_backward_paths(cuda, reaches, B, C, h, w, H, W, use_cw, per_image):
    assert _REACHES[reaches](h, w, H, W, C), (reaches, _uce_blocks(h, w, H, W))
    logit, label, cw = _inputs(B, C, h, w, H, W)
    _check(cuda, logit, label, per_image=per_image, cw=cw if use_cw else None, tag=f'{reaches} per_image {per_image}')


@pytest.mark.parametrize('name,B,C,h,w,H,W,classes', [
    ('shorter_than_a_tile', 1, 3, 3, 2, 5, 4, 'all'),
    ('exactly_one_tile', 1, 3, 4, 4, 32, 64, 'all'),
    ('one_tile_plus_one', 1, 3, 2, 5, 3, 683, 'all'),
    ('several_workgroups', 2, 2, 8, 8, 192, 184, 'present'),
    ('two_class_passes', 1, 130, 5, 6, 70, 30, 'present'),
    ('slot_list_shorter_than_C', 2, 7, 8, 8, 64, 64, (5, 0, 3)),
])
@pytest.mark.parametrize('per_image', [False, True])
def test_lovasz_sort_boundaries(cuda, name, B, C, h, w, H, W, classes, per_image):
    n = H * W if per_image else B * H * W  # elements of a segment
    if name == 'shorter_than_a_tile':
        assert n == 20 < 64
    elif name == 'exactly_one_tile':
        assert n == LOV_TILE == LOV_SCAN
    elif name == 'one_tile_plus_one':
        assert n == LOV_TILE + 1 == LOV_SCAN + 1
    elif name == 'several_workgroups':
        assert n > 4 * LOV_WG and n % LOV_WG != 0 and n % LOV_TILE != 0
    elif name == 'two_class_passes':
        assert C > 128 and n > LOV_TILE
    logit, label, cw = _inputs(B, C, h, w, H, W)
    if name in ('exactly_one_tile', 'one_tile_plus_one'):
        label = label.clone()
        label[label == 255] = 0   # nothing ignored: the valid prefix is the whole tile (+ 1)
        assert int((label != 255).sum()) == B * H * W
    classes = list(classes) if isinstance(classes, tuple) else classes
    _check(cuda, logit, label, classes=classes, per_image=per_image, cw=cw, tag=f'{name} per_image {per_image}')


def test_lovasz_class_with_one_pixel_absent_classes_and_labels_past_the_channels(cuda):
    logit, label, cw = _inputs(*_BASE)
    label = label.clone()
    label[label == 3] = 2
    label[label == 4] = 2
    label[1, 17, 5] = 4               # class 4: exactly one pixel, in image 1; class 3: absent
    label[0, 8:24, 8:40] = 9          # >= C = 7, not ignored: background for every class
    label[1, 40:48, :16] = -3
    assert int((label == 4).sum()) == 1 and not bool((label == 3).any())
    got = {}
    for per_image in (False, True):
        for classes in ('present', 'all', [3, 4, 6]):
            got[(per_image, str(classes))] = _check(cuda, logit, label, classes=classes, per_image=per_image, cw=cw,
                                                    tag=f'edge classes {classes} per_image {per_image}')
    assert got[(False, 'present')] != got[(False, 'all')]


def test_lovasz_all_ignored_images(cuda):
    from rscotr_amd import ops
    logit, label, cw = _inputs(*_BASE)
    one = label.clone()
    one[0] = 255                      # image 0 has no valid pixel: per image it gives 0 and still counts in the mean
    for per_image, reduction in ((False, 'none'), (True, 'mean'), (True, 'sum')):
        for classes in ('present', 'all'):
            _check(cuda, logit, one, classes=classes, per_image=per_image, cw=cw, reduction=reduction,
                   tag=f'image 0 ignored, {classes}, per_image {per_image} {reduction}')
    none = torch.full_like(label, 255)
    for per_image, reduction in ((False, 'none'), (True, 'mean')):
        for classes in ('present', 'all', [1, 2]):
            ld = logit.to(cuda).requires_grad_(True)
            loss = ops.upsample_lovasz(ld, none.to(cuda), classes=classes, per_image=per_image, reduction=reduction)
            loss.backward()
            assert float(loss) == 0.0 and not bool(ld.grad.any())


@pytest.mark.parametrize('loss_weight,ignore,per_image', [(3.0, 255, False), (1.0, 5, False), (0.5, -100, True), (3.0, 5, True)])
def test_lovasz_options(cuda, loss_weight, ignore, per_image):
    """loss_weight and an ignore_index other than 255: 5 of C = 7 is a channel whose label leaves the segments."""
    logit, label, cw = _inputs(*_BASE, ignore)
    assert int((label == ignore).sum()) > 0
    _check(cuda, logit, label, ignore, per_image=per_image, cw=cw, loss_weight=loss_weight,
           reduction='sum' if per_image and loss_weight == 3.0 else None, tag=f'lw {loss_weight} ignore {ignore}')


@pytest.mark.parametrize('scale', [1, 8])
@pytest.mark.parametrize('per_image', [False, True])
def test_lovasz_ties_rank_by_pixel_index(cuda, scale, per_image):
    """Logits constant per class over 2 x 2 cell blocks (multiples of 1/8), at identity resize and at x8: the tap weights are
    multiples of 1/256 there, every product and sum of the interpolation is exact in fp32 as in fp64, and the taps of a pixel
    inside a block read one value, so whole blocks of errors tie bit for bit.  The gradient is the stable-sort oracle's: equal
    errors rank by ascending flat pixel index."""
    g = torch.Generator().manual_seed(7)
    B, C, hb, wb = 2, 4, 4, 4
    coarse = torch.round(torch.randn(B, C, hb, wb, generator=g) * 16) / 8
    logit = coarse.repeat_interleave(2, 2).repeat_interleave(2, 3).contiguous()
    h, w = 2 * hb, 2 * wb
    H, W = h * scale, w * scale
    label = torch.randint(0, C, (B, H, W), generator=g)
    label[torch.rand(B, H, W, generator=g) < 0.05] = 255
    # pixels of one logit block of one image and one label share their error in every class
    up = torch.nn.functional.interpolate(logit.double(), size=(H, W), mode='bilinear', align_corners=False)
    p = torch.softmax(up, 1)
    e0 = (p[:, 0] - (label == 0).double()).abs()[label != 255]
    assert e0.numel() - e0.unique().numel() > e0.numel() // 2, 'the construction ties most errors'
    _check(cuda, logit, label, classes='all', per_image=per_image, tag=f'ties x{scale} per_image {per_image}')


def _call(ops, logit, label_d, **kw):
    ld = logit.detach().clone().requires_grad_(True)
    loss = ops.upsample_lovasz(ld, label_d, **kw)
    (loss * 1.7).backward()
    return loss.detach(), ld.grad


@pytest.mark.parametrize('B,C,h,w,H,W', [_SHAPES[0][1:], _SHAPES[1][1:]])
def test_lovasz_two_calls_are_bit_equal(cuda, B, C, h, w, H, W):
    from rscotr_amd import ops
    logit, label, cw = _inputs(B, C, h, w, H, W)
    ld, label_d, cw_d = logit.to(cuda), label.to(cuda), cw.to(cuda)
    for kw in (dict(class_weight=cw_d, loss_weight=3.0), dict(per_image=True, reduction='mean', classes='all')):
        a = _call(ops, ld, label_d, **kw)
        b = _call(ops, ld, label_d, **kw)
        assert float(a[0]) > 0 and float(a[1].abs().max()) > 0
        assert all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize('per_image', [False, True])
def test_lovasz_op_captured_in_a_graph_replays_bit_equal(cuda, per_image):
    """Forward and backward captured on a side stream as the runner captures an iteration (warm-up on the same stream, then
    torch.cuda.graph), replayed on fresh inputs copied into the static tensors: bit-equal to the eager call.  The labels at
    capture hold every class; the second replay's labels have no pixel of class 2 (a segment that was sorted at capture leaves
    on the device count), the third's none of image 0."""
    from rscotr_amd import ops
    B, C, h, w, H, W = _BASE
    _, _, cw = _inputs(B, C, h, w, H, W)
    kw = dict(class_weight=cw.to(cuda), loss_weight=3.0, per_image=per_image, reduction='mean' if per_image else 'none')
    g = torch.Generator().manual_seed(5)

    def batch(trial):
        lg = (torch.randn(B, C, h, w, generator=g) * 3)
        lb = torch.randint(0, C, (B, H, W), generator=g)
        lb[torch.rand(B, H, W, generator=g) < 0.1] = 255
        if trial == 1:
            lb[lb == 2] = 3
        if trial == 2:
            lb[0] = 255
        return lg.to(cuda), lb.to(cuda)

    lg0, lb0 = batch(0)
    assert all(bool((lb0 == c).any()) for c in range(C))
    s_logit = lg0.clone().requires_grad_(True)
    s_label = lb0.clone()

    def body():
        loss = ops.upsample_lovasz(s_logit, s_label, **kw)
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
    for trial in range(3):
        lg, lb = (lg0, lb0) if trial == 0 else batch(trial)
        if trial == 1:
            assert not bool((lb == 2).any())
        with torch.no_grad():
            s_logit.copy_(lg)
            s_label.copy_(lb)
        graph.replay()
        torch.cuda.synchronize()
        eager = _call(ops, lg, lb, **kw)
        assert float(outs[0]) > 0 and float(outs[1].abs().max()) > 0
        assert all(torch.equal(x, y) for x, y in zip(outs, eager)), trial


# ---- the head and the step -----------------------------------------------------------------------------------------------------
def test_head_losses_with_ce_and_lovasz(cuda):
    """`Mask2FormerHead.losses` with [CE(class_weight), Lovasz]: loss_ce and acc_seg are the CE-only head's bits, loss_lovasz is the
    op's (and the oracle's) with the HEAD's ignore_index, the logit gradient is the sum of the two ops' gradients, and a
    configured OHEM sampler does not reach the Lovasz entry."""
    from rscotr_amd import ops
    from test_seg_loss_weighted_cpu import _CW100, _head
    B, C, h, w, H, W = 2, 100, 8, 8, 64, 64
    logit, label, _ = _inputs(B, C, h, w, H, W)
    ld, seg_label = logit.to(cuda), label.to(cuda).unsqueeze(1)
    ce = dict(type='CrossEntropyLoss', loss_name='loss_ce', class_weight=_CW100, loss_weight=1.0)
    lov = dict(type='LovaszLoss', loss_name='loss_lovasz', reduction='none', classes=[0, 1, 2, 3, 4, 5], loss_weight=3.0)

    def run(**over):
        head, _ = _head(**over)
        x = ld.clone().requires_grad_(True)
        out = head.losses(x, seg_label)
        sum(v for k, v in out.items() if 'loss' in k).backward()
        return out, x.grad

    both, g_both = run(loss_decode=[ce, lov])
    only, g_ce = run(loss_decode=[ce])
    assert list(both) == ['loss_ce', 'loss_lovasz', 'acc_seg'] and list(only) == ['loss_ce', 'acc_seg']
    assert torch.equal(both['loss_ce'], only['loss_ce']) and torch.equal(both['acc_seg'], only['acc_seg'])
    x = ld.clone().requires_grad_(True)
    loss_l = ops.upsample_lovasz(x, seg_label.squeeze(1), classes=[0, 1, 2, 3, 4, 5], loss_weight=3.0)
    (g_lov,) = torch.autograd.grad(loss_l, x)
    assert torch.equal(both['loss_lovasz'], loss_l) and float(loss_l.detach()) > 0
    assert torch.equal(g_both, g_ce + g_lov)
    loss_r, grad_r = lovasz_reference(logit, label, 255, [0, 1, 2, 3, 4, 5], loss_weight=3.0, scale=1.0)
    assert abs(float(loss_l) - loss_r) <= 1e-5 * loss_r
    assert float((g_lov.cpu().double() - grad_r).abs().max()) < 1e-4 * float(grad_r.abs().max())
    sampler = dict(type='OHEMPixelSampler', thresh=0.7, min_kept=100)
    ohem, _ = run(loss_decode=[ce, lov], sampler=sampler)
    assert torch.equal(ohem['loss_lovasz'], both['loss_lovasz'])
    # the head's ignore_index reaches the entry: with ignore_index = 2 the block of class 2 leaves every segment and class 2, a
    # summed class, has no foreground left (it then costs its largest probability).  (Background pixels ranked behind a class's
    # last foreground pixel carry g = 0, so ignoring a class outside the list can leave the fp32 loss where it was.)
    ign = 2
    lab = seg_label.clone()
    lab[0, 0, 16:48, 8:40] = ign
    lab7 = torch.where(lab == 255, torch.full_like(lab, ign), lab)
    head7, _ = _head(loss_decode=[ce, lov], ignore_index=ign)
    out7 = head7.losses(ld, lab7)
    kw = dict(classes=[0, 1, 2, 3, 4, 5], loss_weight=3.0)
    with_ign = ops.upsample_lovasz(ld, lab7.squeeze(1), ign, **kw)
    without = ops.upsample_lovasz(ld, lab.squeeze(1), 255, **kw)
    assert torch.equal(out7['loss_lovasz'], with_ign)
    print('loss_lovasz with the head ignoring class 2:', float(with_ign), 'ignoring 255:', float(without))
    assert abs(float(with_ign) - float(without)) > 1e-3 * float(without)


def test_seg_iterations_with_ce_and_lovasz_graph_equals_eager(cuda):
    """The tiny model with [CE, Lovasz(loss_weight=3)] on its seg head: two seg iterations (the second one is the captured and
    replayed one when graphs are on) from identical weights on identical batches.  Losses and the seg head's parameter gradients
    are finite and bit-equal between the graphed and the eager runner; log_vars holds seg.*.loss_lovasz and loss is
    loss_ce + loss_lovasz.  (DropPath off: its draws differ between captured and eager RNG streams; a seg-only loader: the two
    iterations are consecutive.)"""
    from util import build_model, load_model_cfg
    from rscotr_amd.data import build_synthetic_multidataloader
    from rscotr_amd.runner import build_runner
    cfg, mcfg = load_model_cfg(tiny=True)
    mcfg = copy.deepcopy(mcfg)
    mcfg['backbone']['drop_path_rate'] = 0.0
    mcfg['task_weight'] = dict(cls=1, det=1, seg=2)  # (a power of two: the scaled log values stay exact)
    ce_lov = [dict(type='CrossEntropyLoss', loss_name='loss_ce', loss_weight=1.0),
              dict(type='LovaszLoss', loss_name='loss_lovasz', reduction='none', loss_weight=3.0)]
    runs = []
    for graphs in (True, False):
        mcfg['seg_head']['loss_decode'] = ce_lov
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
    assert [list(d) for d in lg] == [list(d) for d in le]
    for a, b in zip(lg, le):
        for k in a:
            if 'loss' in k:
                assert a[k] == b[k], (k, a[k], b[k])
    worst = {n: float((gg[n] - ge[n]).abs().max()) for n in gg if not torch.equal(gg[n], ge[n])}
    assert not worst, worst
    for d in lg:
        (k_lov,) = [k for k in d if k.startswith('seg.') and k.endswith('.loss_lovasz')]
        k_ce = k_lov[:-len('loss_lovasz')] + 'loss_ce'
        (k_loss,) = [k for k in d if k.startswith('seg.') and k.endswith('.loss')]
        assert d[k_lov] > 0 and d[k_ce] > 0
        assert d[k_loss] == float(np.float32(d[k_ce]) + np.float32(d[k_lov])), d
