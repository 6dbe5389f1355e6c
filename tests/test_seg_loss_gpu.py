"""Fused bilinear-upsample + cross-entropy (+accuracy) kernels vs F.interpolate + F.cross_entropy
(what mmseg's BaseDecodeHead.losses computes), forward and gradient."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# csrc/seg_upsample.h: cells per block edge of the backward gather (upsample_ce_bwd_kernel), the footprint rows / columns it stages
# in LDS (a block whose footprint is larger on either axis takes the gather's second implementation); csrc/seg_loss.hip: the
# forward grid cap
UCE_TB = 4
UCE_FP = 48
UCE_MAX_WG = 4096


def _uce_footprint(c0, n_in, n_out):
    """Output rows (columns) whose taps can meet the block that starts at cell c0: the kernel's y_lo / y_hi (x_lo / x_hi)
    bounds for one axis, in fp32 like the kernel."""
    f = np.float32
    s = f(n_in) / f(n_out)
    lo = max(0, int(np.floor((f(c0) - f(1) + f(0.5)) / s - f(0.5))))
    hi = min(n_out - 1, int(np.ceil((f(c0 + UCE_TB) + f(0.5)) / s - f(0.5))))
    return hi - lo + 1


def _uce_blocks(h, w, H, W):
    """(footprint rows, footprint columns) of every block of a launch, row-major over the block grid."""
    return [(_uce_footprint(cy0, h, H), _uce_footprint(cx0, w, W))
            for cy0 in range(0, h, UCE_TB) for cx0 in range(0, w, UCE_TB)]


def _uce_grid(h, w):
    return (h + UCE_TB - 1) // UCE_TB, (w + UCE_TB - 1) // UCE_TB


# what a case is there for, checked on the host before the GPU is touched: retuning UCE_TB / UCE_FP must fail the case
# instead of leaving it testing a path it was not written for
def _all_staged(h, w, H, W, C):
    return all(ny <= UCE_FP and nx <= UCE_FP for ny, nx in _uce_blocks(h, w, H, W))


_REACHES = {
    'staged': _all_staged,
    'fallback_both_axes_one_block': lambda h, w, H, W, C: (
        _uce_grid(h, w) == (1, 1) and all(ny > UCE_FP and nx > UCE_FP for ny, nx in _uce_blocks(h, w, H, W))),
    'fallback_rows_only_mixed_launch': lambda h, w, H, W, C: (
        sorted(ny > UCE_FP for ny, nx in _uce_blocks(h, w, H, W)) == [False, False, True, True]
        and all(nx <= UCE_FP for ny, nx in _uce_blocks(h, w, H, W))),
    'fallback_cols_only': lambda h, w, H, W, C: (
        any(nx > UCE_FP for ny, nx in _uce_blocks(h, w, H, W))
        and all(ny <= UCE_FP for ny, nx in _uce_blocks(h, w, H, W))),
    'fallback_two_class_passes': lambda h, w, H, W, C: C > 128 and not _all_staged(h, w, H, W, C),
    # rows r >= UCE_FP and columns xx >= UCE_FP exist in the same block, well past the staged tables
    'fallback_records_recomputed': lambda h, w, H, W, C: (
        any(ny >= 2 * UCE_FP and nx >= 2 * UCE_FP for ny, nx in _uce_blocks(h, w, H, W))),
    # a block with a halo on all four sides, at a resize ratio that is no integer on either axis
    'staged_interior_blocks': lambda h, w, H, W, C: (
        _all_staged(h, w, H, W, C) and min(_uce_grid(h, w)) >= 3 and H % h != 0 and W % w != 0),
    'staged_interior_two_class_passes': lambda h, w, H, W, C: (
        _all_staged(h, w, H, W, C) and min(_uce_grid(h, w)) >= 3 and H % h != 0 and W % w != 0 and C > 128),
    'staged_downsample': lambda h, w, H, W, C: _all_staged(h, w, H, W, C) and h > 2 * H and w > 2 * W,
}

_OLD_CASES = [(2, 100, 64, 64, 512, 512), (1, 5, 3, 4, 17, 9), (2, 7, 8, 8, 8, 8), (1, 130, 5, 5, 40, 40), (2, 3, 6, 7, 5, 3)]
_PATH_CASES = [
    ('fallback_both_axes_one_block', 1, 3, 4, 4, 64, 64),
    ('fallback_rows_only_mixed_launch', 1, 2, 5, 6, 70, 30),
    ('fallback_cols_only', 1, 2, 6, 5, 30, 70),
    ('fallback_two_class_passes', 1, 130, 5, 6, 70, 30),
    ('fallback_records_recomputed', 1, 2, 3, 3, 150, 150),
    ('staged_interior_blocks', 1, 2, 13, 11, 50, 37),
    ('staged_interior_two_class_passes', 2, 130, 9, 10, 23, 61),
    ('staged_downsample', 1, 2, 13, 9, 5, 4),      # 59 cells receive no output pixel at all
    ('staged', 1, 2, 1, 1, 7, 5),                  # 1 x 1 map
    ('staged', 1, 2, 5, 5, 1, 1),                  # 1 x 1 label
]


def _uce_inputs(B, C, h, w, H, W, ignore):
    g = torch.Generator().manual_seed(C * H + w)
    logit = torch.randn(B, C, h, w, generator=g) * 3
    label = torch.randint(0, C, (B, H, W), generator=g)
    label[torch.rand(B, H, W, generator=g) < 0.1] = ignore
    return logit, label


def _uce_reference(logit, label, ignore, backward=True):
    """fp64 on the CPU -> (loss, d(1.7 loss)/d logit | None, #non-ignored, #correct, #non-ignored pixels whose two largest
    interpolated logits are closer than 1e-4)."""
    lr = logit.double().requires_grad_(backward)
    up = F.interpolate(lr, size=label.shape[-2:], mode='bilinear', align_corners=False)
    loss_r = F.cross_entropy(up, label, reduction='none', ignore_index=ignore).mean()
    if backward:
        (loss_r * 1.7).backward()
    valid = label != ignore
    up = up.detach()
    correct = int(((up.argmax(1) == label) & valid).sum())
    top2 = up.topk(2, dim=1).values
    n_near = int((((top2[:, 0] - top2[:, 1]) < 1e-4) & valid).sum())
    return float(loss_r.detach()), lr.grad, int(valid.sum()), correct, n_near


def _check_uce_forward(ops, ld, label_d, ignore, loss_r, valid, correct, n_near):
    """Loss within 1e-5; the three sums as counts.  The non-ignored count is exact (integers below 2^24 in fp32).  The
    arg-max may differ from the fp64 one only where the two largest interpolated logits are closer than 1e-4: fp32 bilinear
    interpolation of four logits of magnitude <~ 15 errs by about 4 * 6e-8 * 15 = 4e-6, 1e-4 is 25 x that; such pixels must be
    rare (<= 0.1 %), or the allowance could hide a wrong arg-max."""
    assert n_near <= 0.001 * valid, (n_near, valid)
    loss, acc = ops.upsample_ce(ld, label_d, ignore)
    with torch.no_grad():
        sums = ops.losses._UpsampleCE.apply(ld.detach(), label_d, ignore)[1].cpu()
    loss_v = float(loss.detach())
    print(f'upsample_ce: loss {loss_v:.8f} ref {loss_r:.8f}  sums {sums.tolist()}  valid {valid} correct {correct} '
          f'n_near {n_near}')
    assert abs(loss_v - loss_r) <= 1e-5 * max(abs(loss_r), 1e-3)
    assert valid < 2 ** 24 and float(sums[2]) == valid
    assert abs(float(sums[1]) - correct) <= n_near, (float(sums[1]), correct, n_near)
    # the percentage the wrapper returns is those two sums (three fp32 roundings of a value <= 100: < 1e-4)
    assert abs(float(acc) - float(sums[1]) * 100.0 / max(valid, 1)) <= 1e-4
    return loss


def _check_uce(cuda, B, C, h, w, H, W, ignore=255):
    from rscotr_amd import ops
    logit, label = _uce_inputs(B, C, h, w, H, W, ignore)
    loss_r, grad_r, valid, correct, n_near = _uce_reference(logit, label, ignore)
    ld = logit.to(cuda).requires_grad_(True)
    loss = _check_uce_forward(ops, ld, label.to(cuda), ignore, loss_r, valid, correct, n_near)
    (loss * 1.7).backward()
    grad = ld.grad.cpu()
    err = float((grad.double() - grad_r).abs().max() / (grad_r.abs().max() + 1e-30))
    print(f'upsample_ce: gradient max error {err:.3e} of the largest reference gradient')
    assert err < 1e-4, err
    # dlogit is torch.empty_like: a cell no output pixel touches (reference gradient exactly 0) must still be written, as 0
    untouched = grad_r == 0
    assert bool((grad[untouched] == 0).all()), int((grad[untouched] != 0).sum())
    return int(untouched.sum())


@pytest.mark.parametrize('B,C,h,w,H,W', _OLD_CASES)
def test_upsample_ce(cuda, B, C, h, w, H, W):
    _check_uce(cuda, B, C, h, w, H, W)


@pytest.mark.parametrize('reaches,B,C,h,w,H,W', _PATH_CASES)
def test_upsample_ce_backward_paths(cuda, reaches, B, C, h, w, H, W):
    """Both implementations of upsample_ce_bwd_kernel (staged / footprints past UCE_FP) on every block layout."""
    assert _REACHES[reaches](h, w, H, W, C), (reaches, _uce_blocks(h, w, H, W))
    untouched = _check_uce(cuda, B, C, h, w, H, W)
    if reaches == 'staged_downsample':
        assert untouched >= 59 * C


@pytest.mark.parametrize('reaches,B,C,h,w,H,W', [_PATH_CASES[1], _PATH_CASES[5]])
def test_upsample_ce_other_ignore_index(cuda, reaches, B, C, h, w, H, W):
    """ignore_index is a kernel parameter; the model only ever passes 255."""
    assert _REACHES[reaches](h, w, H, W, C)
    _check_uce(cuda, B, C, h, w, H, W, ignore=-100)


def test_upsample_ce_forward_grid_stride(cuda):
    """More pixels than the capped forward grid covers in one trip (UCE_MAX_WG workgroups of 256).  Forward only: the
    backward footprint at this resize is far past UCE_FP, which test_upsample_ce_backward_paths covers at small sizes."""
    from rscotr_amd import ops
    B, C, h, w, H, W = 1, 2, 8, 8, 1056, 1000
    assert B * H * W > UCE_MAX_WG * 256
    logit, label = _uce_inputs(B, C, h, w, H, W, 255)
    loss_r, _, valid, correct, n_near = _uce_reference(logit, label, 255, backward=False)
    _check_uce_forward(ops, logit.to(cuda), label.to(cuda), 255, loss_r, valid, correct, n_near)


def test_upsample_ce_all_ignored(cuda):
    from rscotr_amd import ops
    logit = torch.randn(1, 4, 2, 2, device=cuda, requires_grad=True)
    label = torch.full((1, 8, 8), 255, dtype=torch.long, device=cuda)
    loss, acc = ops.upsample_ce(logit, label, 255)
    loss.backward()
    assert float(loss) == 0.0 and float(acc) == 0.0 and float(logit.grad.abs().max()) == 0.0


@pytest.mark.parametrize('B,Q,h,w,th,tw', [(2, 100, 64, 64, 8, 8), (2, 100, 64, 64, 32, 32), (2, 100, 64, 64, 64, 64),
                                            (1, 3, 5, 7, 9, 4), (2, 7, 8, 8, 16, 16),
                                            (2, 5, 7, 9, 23, 31), (1, 4, 3, 3, 40, 40)])  # non-integer upsample, x13.3
def test_seg_attn_mask_matches_torch(cuda, B, Q, h, w, th, tw):
    """interpolate -> sigmoid < 0.5 -> all-True rows reset (mask2former_head.py:126-136, :177-178), bit for bit
    except logits within fp32 rounding of 0."""
    from rscotr_amd import ops
    g = torch.Generator().manual_seed(h * 31 + th)
    mp = torch.randn(B, Q, h, w, generator=g)
    mp[0, 0] = -5.0                       # an all-True row: must come out all-False
    mp[-1, -1] = 4.0                      # an all-False row
    ref = F.interpolate(mp, (th, tw), mode='bilinear', align_corners=False).flatten(2)
    near0 = ref.abs() < 1e-6
    assert int(near0.sum()) <= 0.001 * near0.numel()  # the exclusion below stays an exception
    ref = ref.sigmoid() < 0.5
    ref = ref & ~ref.all(-1, keepdim=True)
    out = ops.seg_attn_mask(mp.to(cuda), (th, tw), 8).cpu()
    assert out.dtype == torch.bool and out.shape == ref.shape
    assert not bool(out[0, 0].any()) and not bool(out[-1, -1].any())
    assert bool(((out == ref) | near0).all())
