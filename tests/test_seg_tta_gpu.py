"""Multi-scale / flip test-time augmentation of the segmentation tail on the device (csrc/seg_eval.hip:
rscotr_seg_predict_tta_u8): ops.seg_predict_tta against mmseg's aug_test chain evaluated in fp64 on the CPU (per view
F.interpolate -> [:hs, :ws] -> F.interpolate -> softmax -> un-flip, then the mean over the views), `MTL.aug_test_seg` through
`MTL.forward(..., img=[V views])`, and the pre_eval test loop of rscotr_amd.engine over a MultiScaleFlipAug collate.

Label comparison: labels must be EQUAL wherever the fp64 top-1 minus top-2 gap of the mean probabilities is at least the
per-pixel tolerance  tol = top1 * 2^-24 * (256 L + 2 (C + V + 8)),  L = max |logit| over the views: the composed resampling
errs by at most delta = 64 * 2^-24 * L (the bound of tests/test_seg_eval_gpu.py), a softmax output errs relatively by at most
2 delta plus about (C + 8) ulp for expf, the C-term sum and the divide, the V-term accumulation adds V ulp, and the gap of two
values, each at most top1, errs by twice that.  Pixels under tol are ambiguous (either label is accepted) and may number at
most 0.25 % of a case's pixels: a cap on what the test may leave out.  The seeds below were chosen on the CPU so that the
fp64 reference alone stays under the cap (0 - 0.08 % ambiguous per case: 11 of 15 360 pixels in case a, 2 of 3 894 in d)."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from rscotr_amd import ops, synth
from util import build_model, load_model_cfg

pytestmark = pytest.mark.gpu

AMBIGUOUS_CAP = 2.5e-3


def chain(views, out, dtype=torch.float64):
    """views: [(logit (B, C, h, w), canvas, crop | None, flip | None)] -> the mean over the views of the per-view
    probabilities (B, C, Ho, Wo), on the CPU in `dtype`."""
    acc = None
    for logit, canvas, crop, flip in views:
        x = F.interpolate(logit.detach().to('cpu', dtype), size=tuple(canvas), mode='bilinear', align_corners=False)
        hs, ws = canvas if crop is None else crop
        x = F.interpolate(x[:, :, :hs, :ws], size=tuple(out), mode='bilinear', align_corners=False)
        x = torch.softmax(x, dim=1)
        if flip == 'horizontal':
            x = x.flip(dims=(3,))
        elif flip == 'vertical':
            x = x.flip(dims=(2,))
        acc = x if acc is None else acc + x
    return acc / len(views)


def clear_mask(ref, views):
    """-> (want (B, Ho, Wo), clear (B, Ho, Wo) bool) of the fp64 mean probabilities `ref`."""
    want = ref.argmax(dim=1)
    C, V = ref.shape[1], len(views)
    if C == 1:
        return want, torch.ones_like(want, dtype=torch.bool)
    L = max(float(v[0].abs().max()) for v in views)
    top = ref.topk(2, dim=1).values
    tol = top[:, 0] * 2.0 ** -24 * (256 * L + 2 * (C + V + 8))
    return want, (top[:, 0] - top[:, 1]) >= tol


def check_labels(got, views, out, tag, ref=None):
    ref = chain(views, out) if ref is None else ref
    want, clear = clear_mask(ref, views)
    got = got.cpu()
    assert got.dtype == torch.uint8 and got.shape == want.shape, (got.dtype, got.shape, want.shape)
    amb = float((~clear).double().mean())
    wrong = int(((got.long() != want) & clear).sum())
    print(f'[seg_predict_tta {tag}] pixels {want.numel()} ambiguous {int((~clear).sum())} ({amb:.5%}) wrong outside them {wrong} '
          f'differing inside them {int(((got.long() != want) & ~clear).sum())}')
    assert amb <= AMBIGUOUS_CAP, amb
    assert wrong == 0, wrong
    return want, clear


def call(views, out, device):
    return ops.seg_predict_tta([v[0].to(device) for v in views], [v[1] for v in views], [v[2] for v in views], out,
                               [v[3] for v in views])


# name -> (C, B, output, seed, [(logits hw, canvas, crop, flip)]): the cases of the table
H_, V_ = 'horizontal', 'vertical'
CASES = dict(
    a=(100, 2, (96, 80), 1, [((8, 8), (64, 64), None, None), ((8, 8), (64, 64), None, H_),
                             ((12, 10), (96, 80), (90, 75), None), ((12, 10), (96, 80), (90, 75), H_),
                             ((4, 4), (32, 32), (30, 25), V_)]),
    b=(6, 2, (40, 30), 2, [((8, 8), (64, 64), None, None)]),
    c=(255, 2, (12, 70), 3, [((3, 5), (24, 40), (21, 37), None), ((6, 9), (48, 72), None, H_)]),
    d=(5, 2, (33, 59), 4, [((3 + i, 5 + i), (8 * (3 + i), 8 * (5 + i)), (8 * (3 + i) - 3, 8 * (5 + i) - 3), f)
                           for i in range(6) for f in (None, H_)]),
    e=(1, 1, (3, 2), 5, [((1, 1), (2, 3), (1, 2), None), ((2, 2), (4, 4), None, H_)]),
)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (views, out, fp64 reference): made once per case and shared, never written to."""
    C, B, out, seed, specs = CASES[name]
    g = torch.Generator().manual_seed(seed)
    views = [(torch.randn((B, C) + hw, generator=g), canvas, crop, flip) for hw, canvas, crop, flip in specs]
    return views, out, chain(views, out)


@pytest.mark.parametrize('name', sorted(CASES))
def test_seg_predict_tta_against_fp64_chain(cuda, name):
    views, out, ref = case(name)
    got = call(views, out, cuda)
    assert got.is_cuda and tuple(got.shape) == (views[0][0].shape[0],) + tuple(out)
    want, clear = check_labels(got, views, out, name, ref)
    if ref.shape[1] == 1:
        assert int(got.max()) == 0
    if len(views) == 1:  # one view: the labels of ops.seg_predict (no softmax: monotone) outside the mask
        logit, canvas, crop, flip = views[0]
        single = ops.seg_predict(logit.to(cuda), canvas, crop_hw=crop, out_hw=out, flip=flip).cpu()
        assert (single[clear] == got.cpu()[clear]).all()
    assert torch.equal(got, call(views, out, cuda))  # run to run


def test_seg_predict_tta_ties_and_nan(cuda):
    g = torch.Generator().manual_seed(7)
    # channels 1 and 2 equal and largest in every view -> the lower index
    specs = [((4, 4), (8, 8), None, None), ((5, 3), (10, 6), (9, 5), H_)]
    views = []
    for hw, canvas, crop, flip in specs:
        t = torch.zeros((2, 4) + hw)
        t[:, 1] = torch.randn((2,) + hw, generator=g).abs() + 1.0
        t[:, 2] = t[:, 1]
        views.append((t, canvas, crop, flip))
    assert (call(views, (11, 7), cuda).cpu() == 1).all()
    # one NaN logit in one view: softmax spreads it over every channel of the pixels in its footprint and torch's arg-max then
    # decides; the expected labels there are those of the fp32 torch chain
    clean = [(torch.randn((1, 4) + hw, generator=g), canvas, crop, flip) for hw, canvas, crop, flip in specs]
    dirty = [(clean[0][0].clone(),) + clean[0][1:], clean[1]]
    dirty[0][0][0, 3, 1, 2] = float('nan')
    ref32 = chain(dirty, (10, 9), torch.float32)
    hit = torch.isnan(ref32).any(dim=1)
    assert 0 < int(hit.sum()) < hit.numel()
    got = call(dirty, (10, 9), cuda).cpu()
    assert (got[hit].long() == ref32.argmax(dim=1)[hit]).all()
    # away from the footprint the labels are those of the clean input
    want, clear = clear_mask(chain(clean, (10, 9)), clean)
    keep = clear & ~hit
    assert int(keep.sum()) > 0 and (got[keep].long() == want[keep]).all()


def test_seg_predict_tta_refusals(cuda):
    z = lambda B=1, C=3: torch.zeros(B, C, 2, 2, device=cuda)
    one = lambda n: dict(canvases=[(4, 4)] * n, crops=[None] * n, out_hw=(4, 4), flips=[None] * n)
    with pytest.raises((RuntimeError, ValueError)):
        ops.seg_predict_tta([], **one(0))
    with pytest.raises((RuntimeError, ValueError)):
        ops.seg_predict_tta([z() for _ in range(17)], **one(17))
    with pytest.raises((RuntimeError, ValueError)):
        ops.seg_predict_tta([z(C=256)], **one(1))
    with pytest.raises((RuntimeError, ValueError)):
        ops.seg_predict_tta([z()], [(4, 4)], [(5, 4)], (4, 4), [None])
    with pytest.raises(ValueError):
        ops.seg_predict_tta([z()], [(4, 4)], [None], (4, 4), ['diagonal'])
    with pytest.raises(ValueError):
        ops.seg_predict_tta([z(1), z(2)], **one(2))
    with pytest.raises(ValueError):
        ops.seg_predict_tta([z(), z()], [(4, 4)], [None, None], (4, 4), [None, None])
    # sixteen views are taken
    assert tuple(ops.seg_predict_tta([z() for _ in range(16)], **one(16)).shape) == (1, 4, 4)


@pytest.fixture(scope='module')
def model(cuda):
    """The tiny model with its untrained mask decoder damped.  As initialised, the nine decoder layers wash the 100 queries
    out (their outputs differ by 0.06 across the queries around a common 0.8), so the head emits 100 nearly equal channels on
    top of a common offset of several units: the softmax is flat (top-1 about 0.012), label boundaries run through the whole
    map, and the tolerance, which grows with max |logit|, covers the differences between channels.  With the decoder's
    matrices scaled by 0.25 the queries stay distinct (channel spread about 1 at max |logit| about 8): a head that separates
    its channels, as a trained one does.  The reference is still built from this model's own logits."""
    cfg, mcfg = load_model_cfg(tiny=True)
    m = build_model(mcfg)
    with torch.no_grad():
        for p in m.seg_head.transformer_decoder.parameters():
            if p.dim() > 1:
                p.mul_(0.25)
    ops.WPLANES.bump()  # (parameters rewritten in place)
    return m.to(cuda).eval()


def test_model_aug_test(model, cuda):
    ori = (80, 120, 3)
    b0, b1 = synth.make_batch('seg', 2, 64, seed=6), synth.make_batch('seg', 2, (64, 96), seed=7)
    m0 = [dict(m, ori_shape=ori) for m in b0['img_metas']]
    m1 = [dict(m, ori_shape=ori, flip=True, flip_direction='horizontal') for m in b1['img_metas']]
    imgs = [b0['img'].to(cuda), b1['img'].to(cuda)]
    out = model(task='seg', img=imgs, img_metas=[m0, m1], return_loss=False, rescale=True, on_device=True)
    assert isinstance(out, list) and len(out) == 2
    assert all(o.is_cuda and o.dtype == torch.uint8 and tuple(o.shape) == ori[:2] for o in out)
    views = []
    with torch.no_grad():
        for img, metas in zip(imgs, (m0, m1)):
            neck, bb = model.extract_feat(img)
            logit = model.seg_head.forward_test(neck, bb, metas, model.shared_encoder)
            views.append((logit.cpu(), tuple(img.shape[2:]), tuple(metas[0]['img_shape'][:2]),
                          'horizontal' if metas[0].get('flip') else None))
    want, clear = check_labels(torch.stack(out), views, ori[:2], 'model')
    # the host route: int64 NumPy maps, equal to the device maps outside the mask
    host = model(task='seg', img=imgs, img_metas=[m0, m1], return_loss=False, rescale=True)
    assert isinstance(host, list) and len(host) == 2
    assert all(isinstance(p, np.ndarray) and p.dtype == np.int64 and p.shape == ori[:2] for p in host)
    host = torch.from_numpy(np.stack(host))
    assert (host[clear] == torch.stack(out).cpu().long()[clear]).all()
    # a one-element list is the plain call
    plain = model(task='seg', img=imgs[0], img_metas=m0, return_loss=False, rescale=True, on_device=True)
    listed = model(task='seg', img=[imgs[0]], img_metas=[m0], return_loss=False, rescale=True, on_device=True)
    assert len(plain) == len(listed) == 2 and all(torch.equal(a, b) for a, b in zip(plain, listed))
    # cls and det keep refusing several views
    with pytest.raises(NotImplementedError):
        model(task='det', img=imgs, img_metas=[m0, m1], return_loss=False, rescale=True)


def _same_metrics(a, b):
    assert list(a) == list(b), (list(a), list(b))
    va, vb = np.array(list(a.values()), dtype=np.float64), np.array(list(b.values()), dtype=np.float64)
    assert np.array_equal(va, vb, equal_nan=True), (a, b)


def test_engine_pre_eval_loop_with_tta(model, cuda, tmp_path):
    """single_gpu_test(..., seg=dict(pre_eval=True)) over a MultiScaleFlipAug collate (V = 4: 64 and 96 pixels, each also
    flipped) on an on-disk TileSegDataset of three 64 x 64 tiles: 4-tuples of int64 CPU vectors per image, and evaluate() of
    them exactly what evaluate() gives for the device label maps of a direct loop.  The toy dataset names one class per
    output channel of the head, as the single-view engine test does."""
    from PIL import Image
    from rscotr_amd.engine import single_gpu_test
    from rscotr_amd.pipeline import IMG_NORM, DeviceLoader, SegTTACollate, TileSegDataset, build_collate
    rng = np.random.RandomState(5)
    (tmp_path / 'img').mkdir(); (tmp_path / 'ann').mkdir()
    for i in range(3):
        Image.fromarray(rng.randint(0, 255, size=(64, 64, 3)).astype(np.uint8)).save(tmp_path / 'img' / f't{i}.png')
        Image.fromarray(rng.randint(0, 7, size=(64, 64)).astype(np.uint8)).save(tmp_path / 'ann' / f't{i}.png')
    ds = TileSegDataset(str(tmp_path / 'img'), str(tmp_path / 'ann'))
    ds.CLASSES = tuple(f'class{i}' for i in range(model.seg_head.num_queries))
    pipeline = [dict(type='LoadImageFromFile'),
                dict(type='MultiScaleFlipAug', img_scale=(64, 64), img_ratios=[1.0, 1.5], flip=True,
                     transforms=[dict(type='Resize', keep_ratio=True), dict(type='RandomFlip'),
                                 dict(type='Normalize', **IMG_NORM), dict(type='ImageToTensor', keys=['img']),
                                 dict(type='Collect', keys=['img'])])]
    collate = build_collate('seg', pipeline, cuda)
    assert isinstance(collate, SegTTACollate) and len(collate.views) == 4
    loaders = dict(potsdam=DeviceLoader(ds, collate, 2, test_mode=True))
    first = next(iter(loaders['potsdam']))
    assert [tuple(t.shape) for t in first['img']] == [(2, 3, 64, 64)] * 2 + [(2, 3, 96, 96)] * 2
    assert [m[0]['flip'] for m in first['img_metas']] == [False, True, False, True]
    assert all(m['flip_direction'] == ('horizontal' if m['flip'] else None) for ms in first['img_metas'] for m in ms)
    assert all(m['ori_shape'] == (64, 64, 3) for ms in first['img_metas'] for m in ms)
    assert [ms[0]['img_shape'] for ms in first['img_metas']] == [(64, 64, 3)] * 2 + [(96, 96, 3)] * 2
    # the flipped view is the mirror of the unflipped one (the flip follows the resample: the same values, mirrored), and
    # the two scales differ
    for a, b in ((0, 1), (2, 3)):
        assert torch.allclose(first['img'][b], first['img'][a].flip(3), rtol=0, atol=1e-5)
        assert not torch.equal(first['img'][b], first['img'][a])
    assert 'gt_semantic_seg' not in collate._collate((64, 64), False)(
        [ds[0], ds[1]], np.random.RandomState(0))  # (no label stage at test time)
    old = getattr(model, 'CLASSES', None)
    model.CLASSES = dict(potsdam=ds.CLASSES)
    try:
        res = single_gpu_test(model, loaders, kwargs_dict=dict(seg=dict(pre_eval=True)))['potsdam']
        assert not model.training
        maps = []
        for data in loaders['potsdam']:
            maps.extend(model(return_loss=False, on_device=True, **data))
    finally:
        model.CLASSES = old
    assert len(res) == 3
    for r in res:
        assert isinstance(r, tuple) and len(r) == 4
        assert all(torch.is_tensor(a) and a.dtype == torch.int64 and not a.is_cuda and tuple(a.shape) == (100,) for a in r)
        assert torch.equal(r[1], r[2] + r[3] - r[0])
    assert len(maps) == 3 and all(m.is_cuda and m.dtype == torch.uint8 and tuple(m.shape) == (64, 64) for m in maps)
    metric = ['mFscore', 'mIoU']
    _same_metrics(ds.evaluate(res, metric=metric), ds.evaluate(maps, metric=metric))
