"""Segmentation test mode 'slide' (mmseg 0.28 EncoderDecoder.slide_inference) without a GPU: the window grid of
ops.slide_windows against a literal double loop of the contract, the argument checks of ops.slide_windows /
ops.seg_predict_slide (all made before the first device call), the model's acceptance of mode='slide', and its host route
(MTL.inference_seg) against the reference below, with the HIP-backed ops routed through the oracle.

This file also holds the reference the GPU tests (tests/test_seg_slide_gpu.py) compare against: `chain`, the contract evaluated
in fp64 on the CPU, and `clear_mask`, the label-comparison rule.  Labels must be EQUAL wherever the fp64 top-1 minus top-2 gap
of the final logits is at least  tol = 2 * (64 + K + 2) * 2^-24 * max|logit|:  64 * 2^-24 * L is the project's bound for the
composed two-stage resample (tests/test_seg_eval_gpu.py), K, the largest window count over a pixel, covers the K-term fp32 sum,
2 the divide, and the gap of two such values errs by twice that.  Pixels under tol are ambiguous (either label is accepted)."""
import copy
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from rscotr_amd import ops, synth
from util import build_model, load_model_cfg, patch_ops_with_oracle

AMBIGUOUS_CAP = 1e-3  # (the cap of tests/test_seg_eval_gpu.py)
_FLIPS = (None, 'horizontal', 'vertical')


def literal_windows(H, W, crop_size, stride):
    """mmseg slide_inference's double loop, restated: -> [(y1, y2, x1, x2)] in visiting order."""
    (h_crop, w_crop), (h_stride, w_stride) = crop_size, stride
    h_grids = max(H - h_crop + h_stride - 1, 0) // h_stride + 1
    w_grids = max(W - w_crop + w_stride - 1, 0) // w_stride + 1
    out = []
    for h_idx in range(h_grids):
        for w_idx in range(w_grids):
            y1, x1 = h_idx * h_stride, w_idx * w_stride
            y2, x2 = min(y1 + h_crop, H), min(x1 + w_crop, W)
            y1, x1 = max(y2 - h_crop, 0), max(x2 - w_crop, 0)
            out.append((y1, y2, x1, x2))
    return out


def chain(logits, batch, canvas, crop_size, stride, img_shape=None, out=None, flip=None, dtype=torch.float64):
    """The contract on the CPU in `dtype`.  logits (windows * batch, C, h, w) in visiting order, batch innermost ->
    (final logits (batch, C, Ho, Wo), K = the largest window count over a pixel)."""
    assert flip in _FLIPS
    H, W = canvas
    windows = literal_windows(H, W, crop_size, stride)
    assert logits.shape[0] == len(windows) * batch, (tuple(logits.shape), len(windows), batch)
    preds = torch.zeros((batch, logits.shape[1], H, W), dtype=dtype)
    count = torch.zeros((1, 1, H, W), dtype=dtype)
    for k, (y1, y2, x1, x2) in enumerate(windows):
        part = logits[k * batch:(k + 1) * batch].detach().to('cpu', dtype)
        preds[:, :, y1:y2, x1:x2] += F.interpolate(part, size=(y2 - y1, x2 - x1), mode='bilinear', align_corners=False)
        count[:, :, y1:y2, x1:x2] += 1
    assert int((count == 0).sum()) == 0
    preds = preds / count
    if out is not None:
        hs, ws = canvas if img_shape is None else img_shape
        preds = F.interpolate(preds[:, :, :hs, :ws], size=tuple(out), mode='bilinear', align_corners=False)
    if flip == 'horizontal':
        preds = preds.flip(dims=(3,))
    elif flip == 'vertical':
        preds = preds.flip(dims=(2,))
    return preds, int(count.max())


def clear_mask(ref, K, L):
    """-> (want (B, Ho, Wo), clear (B, Ho, Wo) bool) of the fp64 final logits `ref`; L = max |logit| of the windows."""
    want = ref.argmax(dim=1)
    if ref.shape[1] == 1:
        return want, torch.ones_like(want, dtype=torch.bool)
    tol = 2 * (64 + K + 2) * 2.0 ** -24 * L
    top = ref.topk(2, dim=1).values
    return want, (top[:, 0] - top[:, 1]) >= tol


def check_labels(got, ref, K, L, tag, cap=AMBIGUOUS_CAP):
    want, clear = clear_mask(ref, K, L)
    got = got.cpu()
    assert got.dtype == torch.uint8 and got.shape == want.shape, (got.dtype, got.shape, want.shape)
    amb = float((~clear).double().mean())
    wrong = int(((got.long() != want) & clear).sum())
    print(f'[seg_predict_slide {tag}] pixels {want.numel()} K {K} ambiguous {int((~clear).sum())} ({amb:.5%}) wrong outside them '
          f'{wrong} differing inside them {int(((got.long() != want) & ~clear).sum())}')
    assert amb <= cap, amb
    assert wrong == 0, wrong
    return want, clear


# name -> (C, B, logit hw, canvas, crop_size, stride, img_shape, out, flip); logits: torch.randn with seed 40 + ord(name)
H_, V_ = 'horizontal', 'vertical'
CASES = dict(
    a=(100, 2, (8, 8), (96, 80), (64, 64), (32, 48), None, (90, 75), None),  # 2 x 2 windows, the last column shifted back
    b=(7, 2, (5, 8), (40, 100), (64, 64), (43, 43), None, (40, 100), H_),    # the image is shorter than the crop
    c=(5, 1, (4, 4), (56, 56), (32, 32), (8, 8), (53, 50), (70, 61), V_),    # 16 windows over a pixel, a padding crop
    d=(6, 2, (8, 8), (128, 64), (64, 64), (64, 64), None, None, None),       # no overlap, no rescale
    e=(1, 1, (1, 1), (5, 3), (2, 2), (1, 2), (4, 3), (3, 2), None),          # one channel: all zeros out
    f=(255, 1, (3, 5), (30, 47), (24, 40), (5, 6), (29, 45), (33, 59), None),  # the channel limit, 9 windows
    g=(100, 2, (16, 16), (64, 64), (64, 64), (42, 42), None, (96, 80), None),  # a single window
)
# Beyond the table: the sizes at which the launch takes another path.  A thread keeps 3 words per tap and window, for each
# of its 2 (1 without rescale) canvas coordinates per axis, in LDS; the tile shrinks from 4 rows of 64 pixels to 2 and 1 to
# keep that under 64 KB, and above Ky + Kx = 42 windows per coordinate pair (21 / 42 / 85 without rescale) the taps are
# recomputed instead.  Ky = Kx = ceil(24 / stride) + 1 (capped by the grid) here.  The mean of K independent draws shrinks
# like 1 / sqrt(K) while tol grows with K, so in the DENSE cases every window carries one common draw plus a quarter of its
# own: the channels stay apart after the merge, and the reference stays under the cap.
CASES.update(
    h=(3, 1, (3, 3), (48, 48), (24, 24), (3, 3), None, (50, 45), None),      # 9 + 9 windows per pixel's axes: tiles of 2 rows
    i=(3, 2, (3, 3), (48, 48), (24, 24), (2, 2), (47, 46), (40, 52), H_),    # 13 + 13: tiles of 1 row
    j=(3, 1, (3, 3), (48, 48), (24, 24), (1, 1), None, (45, 50), None),      # 25 + 25: taps recomputed, 625 windows
    k=(4, 2, (4, 4), (72, 70), (32, 32), (8, 8), None, None, V_),            # overlap without rescale (and its one-window corners)
    l=(3, 1, (3, 3), (48, 48), (24, 24), (1, 1), None, None, None),          # no rescale, 25 + 25: tiles of 1 row
    m=(2, 1, (3, 3), (92, 92), (48, 48), (1, 1), None, None, None),          # no rescale, 45 + 45: taps recomputed, 2025 windows
)
DENSE = 'hijlm'


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (logits, B, kwargs of the op, fp64 reference, K, L): made once per case and shared, never written to."""
    C, B, hw, canvas, crop, stride, img_shape, out, flip = CASES[name]
    n = len(literal_windows(canvas[0], canvas[1], crop, stride))
    g = torch.Generator().manual_seed(40 + ord(name))
    logits = torch.randn((n * B, C) + hw, generator=g)
    if name in DENSE:
        logits = (0.25 * logits.view((n, B, C) + hw) + torch.randn((B, C) + hw, generator=g)).view((n * B, C) + hw)
    ref, K = chain(logits, B, canvas, crop, stride, img_shape, out, flip)
    kw = dict(canvas_hw=canvas, crop_size=crop, stride=stride, crop_hw=img_shape, out_hw=out, flip=flip)
    return logits, B, kw, ref, K, float(logits.abs().max())


GRIDS = [(96, 80, (64, 64), (32, 48)), (40, 100, (64, 64), (43, 43)), (56, 56, (32, 32), (8, 8)),
         (128, 64, (64, 64), (64, 64)), (5, 3, (2, 2), (1, 2)), (30, 47, (24, 40), (5, 6)), (64, 64, (64, 64), (42, 42)),
         (6000, 6000, (512, 512), (341, 341)),
         (48, 48, (24, 24), (1, 1)), (72, 70, (32, 32), (8, 8)), (7, 9, (7, 9), (9, 11))]


@pytest.mark.parametrize('H,W,crop,stride', GRIDS)
def test_slide_windows_against_the_literal_loop(H, W, crop, stride):
    got = ops.slide_windows(H, W, crop, stride)
    assert got == literal_windows(H, W, crop, stride)
    assert all(isinstance(v, int) for win in got for v in win)
    if (H, W) == (6000, 6000):
        assert len(got) == 18 * 18
    # every window has the common size and lies inside the image; the last one ends at the border
    size = (min(crop[0], H), min(crop[1], W))
    assert all((y2 - y1, x2 - x1) == size and 0 <= y1 and y2 <= H and 0 <= x1 and x2 <= W for y1, y2, x1, x2 in got)
    assert got[-1][1] == H and got[-1][3] == W and got[0][0] == 0 and got[0][2] == 0
    # every pixel is covered: the grid is a product, so per axis
    for n, spans in ((H, sorted({(w[0], w[1]) for w in got})), (W, sorted({(w[2], w[3]) for w in got}))):
        cover = np.zeros(n, dtype=np.int64)
        for a, b in spans:
            cover[a:b] += 1
        assert cover.min() >= 1, int(cover.argmin())


def test_slide_windows_takes_one_integer_for_both_axes():
    assert ops.slide_windows(50, 40, 32, 16) == literal_windows(50, 40, (32, 32), (16, 16))


def test_validation():
    for bad in [(96, 80, (64, 64), (65, 32)),   # stride > crop where the image exceeds the crop: rows 64 are never covered
                (96, 80, (64, 64), (32, 65)),
                (0, 80, (64, 64), (32, 32)), (96, -1, (64, 64), (32, 32)),
                (96, 80, (0, 64), (32, 32)), (96, 80, (64, 64), (32, 0)), (96, 80, (64, 64), (-3, 32)),
                (96, 80, (64, 64, 64), (32, 32))]:
        with pytest.raises(ValueError):
            ops.slide_windows(*bad)
    # a stride larger than the crop is harmless where the image does not exceed the crop
    assert ops.slide_windows(40, 64, (64, 64), (100, 70)) == [(0, 40, 0, 64)]
    # seg_predict_slide: every check precedes the first device call, so CPU tensors do here
    z = torch.zeros(4 * 2, 3, 8, 8)  # (96, 80) with crop 64 and stride (32, 48): 2 x 2 windows, batch 2
    good = dict(batch=2, canvas_hw=(96, 80), crop_size=(64, 64), stride=(32, 48))
    for change in [dict(stride=(65, 48)), dict(stride=(0, 48)), dict(crop_size=(64, -1)), dict(canvas_hw=(0, 80)),
                   dict(batch=0), dict(batch=3), dict(flip='diagonal'), dict(crop_hw=(90, 75))]:
        with pytest.raises(ValueError):
            ops.seg_predict_slide(z, **dict(good, **change))
    with pytest.raises(ValueError):
        ops.seg_predict_slide(z[:7], **good)
    with pytest.raises(ValueError):
        ops.seg_predict_slide(z[0], **good)
    with pytest.raises(RuntimeError):  # the checks passed: a CPU tensor has no route
        ops.seg_predict_slide(z, **good)


def test_reference_cases_stay_under_the_ambiguity_cap():
    """The fp64 reference alone: every case leaves at most 0.1 % of its pixels ambiguous, and the fp32 torch chain is wrong
    on no clear pixel, with an error of at most a quarter of tol / 2."""
    for name in sorted(CASES):
        logits, B, kw, ref, K, L = case(name)
        want, clear = clear_mask(ref, K, L)
        assert float((~clear).double().mean()) <= AMBIGUOUS_CAP, name
        C, _, hw, canvas, crop, stride, img_shape, out, flip = CASES[name]
        ref32, _ = chain(logits, B, canvas, crop, stride, img_shape, out, flip, dtype=torch.float32)
        assert int(((ref32.argmax(dim=1) != want) & clear).sum()) == 0, name
        tol = 2 * (64 + K + 2) * 2.0 ** -24 * L
        assert float((ref32.double() - ref).abs().max()) <= tol / 8, name


def _slide_cfg(mcfg, **seg):
    m = copy.deepcopy(mcfg)
    m['test_cfg'] = dict(m['test_cfg'], seg=dict(seg))
    return m


def test_model_accepts_mode_slide_and_runs_the_host_route(monkeypatch):
    """The tiny model with mode='slide' on the CPU (HIP-backed ops through the oracle): inference_seg returns probabilities
    (B, C) + ori_shape whose arg-max equals the reference's on the clear pixels, window_batch stacks windows without changing
    the window order, and an unknown mode still fails."""
    patch_ops_with_oracle(monkeypatch)
    cfg, mcfg = load_model_cfg(tiny=True)
    seg = dict(mode='slide', crop_size=(64, 64), stride=(32, 32))
    model = build_model(_slide_cfg(mcfg, **seg)).eval()
    b = synth.make_batch('seg', 1, 96, seed=6)
    ori = (80, 120, 3)
    metas = [dict(m, ori_shape=ori) for m in b['img_metas']]
    with torch.no_grad():
        logits, windows = model.slide_window_logits(b['img'], metas)
        assert windows == literal_windows(96, 96, (64, 64), (32, 32)) and len(windows) == 4
        assert logits.shape[0] == 4 and tuple(logits.shape[2:]) == (8, 8)
        prob = model.inference_seg(b['img'], metas, True)
        assert tuple(prob.shape) == (1, logits.shape[1]) + ori[:2]
        assert torch.allclose(prob.sum(dim=1), torch.ones(1, *ori[:2]), atol=1e-5)
        ref, K = chain(logits, 1, (96, 96), (64, 64), (32, 32), (96, 96), ori[:2])
        want, clear = clear_mask(ref, K, float(logits.abs().max()))
        assert K == 4 and int(clear.sum()) > 0 and (prob.argmax(dim=1)[clear] == want[clear]).all()
        assert torch.allclose(prob, torch.softmax(ref, dim=1).float(), atol=1e-4)
        host = model.simple_test_seg(b['img'], metas, rescale=True)
        assert len(host) == 1 and host[0].dtype == np.int64 and host[0].shape == ori[:2]
        # three windows per pass (the last pass holds one): the same windows in the same order
        model.test_cfg['seg']['window_batch'] = 3
        stacked, _ = model.slide_window_logits(b['img'], metas)
        assert torch.allclose(stacked, logits, atol=1e-4)
        model.test_cfg['seg']['window_batch'] = 0
        with pytest.raises(ValueError):
            model.slide_window_logits(b['img'], metas)
        # device TTA with slide is refused by name before anything runs
        with pytest.raises(NotImplementedError, match='slide'):
            model.aug_test_seg([b['img']], [metas], rescale=True, on_device=True)
        model.test_cfg['seg'] = dict(mode='tiled')
        with pytest.raises(AssertionError):
            model.inference_seg(b['img'], metas, True)
        with pytest.raises(AssertionError):
            model.predict_seg_device(b['img'], metas, True)
