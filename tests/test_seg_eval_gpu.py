"""Segmentation evaluation on the device (csrc/seg_eval.hip): ops.seg_predict against the torch chain of
MTL.whole_inference_seg / inference_seg / argmax evaluated in fp64 on the CPU, ops.seg_areas against a NumPy restatement
of mmseg's intersect_and_union, `MTL.forward(..., on_device=True)` and the pre_eval test loop of rscotr_amd.engine.

Label comparison: the kernel and the reference both form fp32 / fp64 sums of two 16-term convex combinations, a few ulp
each, so labels must be EQUAL wherever the fp64 top-1 minus top-2 gap is at least tol = 64 * 2^-24 * max|logit|; pixels with
a smaller gap are ambiguous (either label is a correct rounding) and may number at most 0.1 % of a case's pixels."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from rscotr_amd import ops, synth
from util import build_model, load_model_cfg

pytestmark = pytest.mark.gpu

AMBIGUOUS_CAP = 1e-3


def chain64(logit, canvas, crop, out, flip):
    """whole_inference_seg + the flip of inference_seg in fp64 (softmax left out: monotone) -> (B, C, Ho, Wo)."""
    x = F.interpolate(logit.double().cpu(), size=tuple(canvas), mode='bilinear', align_corners=False)
    if out is not None:
        if crop is not None:
            x = x[:, :, :crop[0], :crop[1]]
        x = F.interpolate(x, size=tuple(out), mode='bilinear', align_corners=False)
    if flip == 'horizontal':
        x = x.flip(dims=(3,))
    elif flip == 'vertical':
        x = x.flip(dims=(2,))
    return x


def check_labels(got, logit, canvas, crop, out, flip, tag):
    ref = chain64(logit, canvas, crop, out, flip)
    want = ref.argmax(dim=1)
    tol = 64 * 2.0 ** -24 * float(logit.abs().max())
    if ref.shape[1] > 1:
        top = ref.topk(2, dim=1).values
        clear = (top[:, 0] - top[:, 1]) >= tol
    else:
        clear = torch.ones_like(want, dtype=torch.bool)
    got = got.cpu()
    assert got.dtype == torch.uint8 and got.shape == want.shape, (got.dtype, got.shape, want.shape)
    amb = float((~clear).double().mean())
    wrong = int(((got.long() != want) & clear).sum())
    print(f'[seg_predict {tag}] pixels {want.numel()} ambiguous {amb:.5%} wrong outside them {wrong} '
          f'differing inside them {int(((got.long() != want) & ~clear).sum())} tol {tol:.3g}')
    assert amb <= AMBIGUOUS_CAP, amb
    assert wrong == 0, wrong


# (C, logits, canvas, crop, output, flip): the cases of the table; output None = no rescale
CASES = dict(
    a=(100, (8, 8), (64, 64), None, (96, 80), None),
    b=(100, (8, 12), (64, 96), (50, 90), (80, 120), 'horizontal'),
    c=(5, (3, 5), (24, 40), (21, 37), (33, 59), 'vertical'),
    d=(6, (8, 8), (64, 64), None, (40, 30), None),       # second stage is a down-scale
    e=(6, (8, 8), (64, 64), None, None, None),           # no rescale
    f=(1, (1, 1), (2, 3), (1, 2), (3, 2), None),         # one channel: all zeros
)


@pytest.mark.parametrize('name', sorted(CASES))
def test_seg_predict_against_fp64_chain(cuda, name):
    C, hw, canvas, crop, out, flip = CASES[name]
    g = torch.Generator().manual_seed(20 + ord(name))
    logit = torch.randn((2, C) + hw, generator=g)
    got = ops.seg_predict(logit.to(cuda), canvas, crop_hw=crop, out_hw=out, flip=flip)
    assert got.is_cuda and tuple(got.shape) == (2,) + tuple(out if out is not None else canvas)
    check_labels(got, logit, canvas, crop, out, flip, name)
    if C == 1:
        assert int(got.max()) == 0


def test_seg_predict_ties_nan_and_channel_limit(cuda):
    # image 0: channels 1 and 2 equal and largest -> 1; image 1: channel 2 NaN -> 2; image 2: channels 1 and 2 NaN -> 1
    logit = torch.zeros(3, 4, 4, 4)
    logit[0, 1:3] = torch.randn(4, 4, generator=torch.Generator().manual_seed(1)).abs() + 1.0
    logit[1, 3] = 5.0
    logit[1, 2] = float('nan')
    logit[2, 3] = 5.0
    logit[2, 1:3] = float('nan')
    for kw in (dict(), dict(out_hw=(11, 7)), dict(crop_hw=(7, 6), out_hw=(5, 9), flip='horizontal')):
        got = ops.seg_predict(logit.to(cuda), (8, 8), **kw).cpu()
        assert (got[0] == 1).all() and (got[1] == 2).all() and (got[2] == 1).all(), kw
    # a single NaN logit: every pixel the torch chain turns into NaN in that channel gets that channel
    one = torch.randn(1, 4, 4, 4, generator=torch.Generator().manual_seed(2))
    one[0, 3, 1, 2] = float('nan')
    up = F.interpolate(F.interpolate(one, size=(8, 8), mode='bilinear', align_corners=False)[:, :, :7, :6], size=(10, 9),
                       mode='bilinear', align_corners=False)
    hit = torch.isnan(up[0, 3])
    assert 0 < int(hit.sum()) < hit.numel()
    got = ops.seg_predict(one.to(cuda), (8, 8), crop_hw=(7, 6), out_hw=(10, 9)).cpu()[0]
    assert (got[hit] == 3).all()
    clean = one.clone()
    clean[0, 3, 1, 2] = 0.0
    # away from the NaN's footprint the other logits decide as if it were not there
    ref = chain64(clean, (8, 8), (7, 6), (10, 9), None)
    top = ref.topk(2, dim=1).values
    clear = ((top[:, 0] - top[:, 1]) >= 64 * 2.0 ** -24 * float(clean.abs().max()))[0] & ~hit
    assert (got[clear].long() == ref.argmax(1)[0][clear]).all()
    with pytest.raises(RuntimeError):
        ops.seg_predict(torch.zeros(1, 256, 2, 2, device=cuda), (4, 4))
    with pytest.raises(RuntimeError):
        ops.seg_predict(torch.zeros(1, 3, 2, 2, device=cuda), (4, 4), crop_hw=(5, 4), out_hw=(4, 4))
    with pytest.raises(RuntimeError):
        ops.seg_predict(torch.zeros(1, 3, 2, 2, device=cuda), (4, 4), out_hw=(0, 4))


def intersect_and_union(pred, label, num_classes, ignore_index, reduce_zero_label):
    """mmseg.core.evaluation.metrics.intersect_and_union for one image, in NumPy (torch.histc over [0, C - 1] with C bins
    counts the integers 0 .. C - 1 one per bin; values outside fall out)."""
    pred, label = pred.astype(np.int64), label.astype(np.int64)
    if reduce_zero_label:
        label[label == 0] = 255
        label = label - 1
        label[label == 254] = 255
    mask = label != ignore_index
    pred, label = pred[mask], label[mask]
    hist = lambda v: np.bincount(v[(v >= 0) & (v < num_classes)], minlength=num_classes).astype(np.int64)
    inter, ap, al = hist(pred[pred == label]), hist(pred), hist(label)
    return np.stack([inter, ap + al - inter, ap, al])


@pytest.mark.parametrize('C', [5, 6])
@pytest.mark.parametrize('reduce_zero_label', [False, True])
def test_seg_areas_against_numpy(cuda, C, reduce_zero_label):
    rs = np.random.RandomState(3 + C)
    pred = rs.randint(0, C, size=(2, 33, 59)).astype(np.uint8)
    gt = rs.randint(0, C + 1, size=(2, 33, 59)).astype(np.uint8)  # contains 0 and, with C, one value >= C
    gt[:, 3, :17] = 255
    gt[:, 9, 5:9] = 200
    assert (gt == 0).any() and (gt == 255).any() and ((gt >= C) & (gt != 255)).any()
    want = np.stack([intersect_and_union(p, g, C, 255, reduce_zero_label) for p, g in zip(pred, gt)])
    p_d, g_d = torch.from_numpy(pred).to(cuda), torch.from_numpy(gt).to(cuda)
    got = ops.seg_areas(p_d, g_d, C, ignore_index=255, reduce_zero_label=reduce_zero_label)
    again = ops.seg_areas(p_d, g_d, C, ignore_index=255, reduce_zero_label=reduce_zero_label)
    assert got.dtype == torch.int64 and tuple(got.shape) == (2, 4, C)
    assert np.array_equal(got.cpu().numpy(), want), (got.cpu().numpy(), want)
    assert torch.equal(got, again)
    # a prediction >= C falls out of the prediction histogram only
    pred2 = pred.copy()
    pred2[:, 0, :5] = C + 1
    want2 = np.stack([intersect_and_union(p, g, C, 255, reduce_zero_label) for p, g in zip(pred2, gt)])
    got2 = ops.seg_areas(torch.from_numpy(pred2).to(cuda), g_d, C, ignore_index=255, reduce_zero_label=reduce_zero_label)
    assert np.array_equal(got2.cpu().numpy(), want2)


def test_seg_areas_many_blocks_and_classes(cuda):
    """A 300 x 301 map (more pixels than one workgroup's share, several workgroups per image) at C = 100."""
    rs = np.random.RandomState(11)
    pred = rs.randint(0, 100, size=(2, 300, 301)).astype(np.uint8)
    gt = rs.randint(0, 102, size=(2, 300, 301)).astype(np.uint8)
    want = np.stack([intersect_and_union(p, g, 100, 255, True) for p, g in zip(pred, gt)])
    got = ops.seg_areas(torch.from_numpy(pred).to(cuda), torch.from_numpy(gt).to(cuda), 100, 255, True)
    assert np.array_equal(got.cpu().numpy(), want)


@pytest.fixture(scope='module')
def model(cuda):
    cfg, mcfg = load_model_cfg(tiny=True)
    return build_model(mcfg).to(cuda).eval()


@pytest.mark.parametrize('size,ori', [(64, (96, 80, 3)), ((64, 96), (80, 120, 3))])
def test_model_on_device_label_maps(model, cuda, size, ori):
    b = synth.make_batch('seg', 2, size, seed=6)
    metas = [dict(m, ori_shape=ori) for m in b['img_metas']]
    img = b['img'].to(cuda)
    out = model(task='seg', img=img, img_metas=metas, return_loss=False, rescale=True, on_device=True)
    assert isinstance(out, list) and len(out) == 2
    assert all(o.is_cuda and o.dtype == torch.uint8 and tuple(o.shape) == ori[:2] for o in out)
    with torch.no_grad():
        neck, bb = model.extract_feat(img)
        logit = model.seg_head.forward_test(neck, bb, metas, model.shared_encoder)
    check_labels(torch.stack(out), logit, img.shape[2:], metas[0]['img_shape'][:2], ori[:2], None, f'model {size}')
    # the host path is untouched: int64 NumPy maps
    host = model(task='seg', img=img, img_metas=metas, return_loss=False, rescale=True)
    assert isinstance(host[0], np.ndarray) and host[0].dtype == np.int64 and host[0].shape == ori[:2]
    norescale = model(task='seg', img=img, img_metas=metas, return_loss=False, rescale=False, on_device=True)
    assert tuple(norescale[0].shape) == tuple(img.shape[2:])


def _same_metrics(a, b):
    assert list(a) == list(b), (list(a), list(b))
    va, vb = np.array(list(a.values()), dtype=np.float64), np.array(list(b.values()), dtype=np.float64)
    assert np.array_equal(va, vb, equal_nan=True), {k: (a[k], b[k]) for k in a if not (a[k] == b[k] or (a[k] != a[k] and b[k] != b[k]))}


def test_engine_pre_eval_loop(model, cuda, tmp_path):
    """single_gpu_test(..., seg=dict(pre_eval=True)) on an on-disk TileSegDataset: three 64 x 64 tiles in batches of two
    (the last batch holds one), 4-tuples of int64 CPU vectors per image, and evaluate() of them EXACTLY what the existing
    confusion-matrix path gives for the on_device label maps.  The toy dataset names one class per output channel of the
    head (100), so that no prediction lies outside the classes — where mmseg's areas and the confusion matrix differ by
    definition (a prediction >= C still counts in area_label)."""
    from PIL import Image
    from rscotr_amd.engine import single_gpu_test
    from rscotr_amd.pipeline import DeviceCollate, DeviceLoader, TileSegDataset
    rng = np.random.RandomState(5)
    (tmp_path / 'img').mkdir(); (tmp_path / 'ann').mkdir()
    for i in range(3):
        Image.fromarray(rng.randint(0, 255, size=(64, 64, 3)).astype(np.uint8)).save(tmp_path / 'img' / f't{i}.png')
        Image.fromarray(rng.randint(0, 7, size=(64, 64)).astype(np.uint8)).save(tmp_path / 'ann' / f't{i}.png')
    ds = TileSegDataset(str(tmp_path / 'img'), str(tmp_path / 'ann'))
    ds.CLASSES = tuple(f'class{i}' for i in range(model.seg_head.num_queries))
    loaders = dict(potsdam=DeviceLoader(ds, DeviceCollate('seg', cuda, flip_prob=0.0), 2, test_mode=True))
    old = getattr(model, 'CLASSES', None)
    model.CLASSES = dict(potsdam=ds.CLASSES)
    try:
        res = single_gpu_test(model, loaders, kwargs_dict=dict(seg=dict(pre_eval=True)))['potsdam']
        plain = single_gpu_test(model, loaders)['potsdam']
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
    assert len(plain) == 3 and all(isinstance(p, np.ndarray) and p.shape == (64, 64) for p in plain)
    assert len(maps) == 3 and all(m.is_cuda and m.dtype == torch.uint8 for m in maps)
    metric = ['mFscore', 'mIoU']
    _same_metrics(ds.evaluate(res, metric=metric), ds.evaluate(maps, metric=metric))
    # pre_eval of NumPy maps takes the same route
    areas = ds.pre_eval([m.cpu().numpy() for m in maps[:2]], [0, 1])
    assert torch.equal(areas.cpu(), torch.stack([torch.stack(r) for r in res[:2]]))
