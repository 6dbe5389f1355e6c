"""Segmentation test mode 'slide' on the device (csrc/seg_eval.hip: rscotr_seg_predict_slide_u8): ops.seg_predict_slide against
mmseg's slide_inference chain evaluated in fp64 on the CPU, its agreement with ops.seg_predict where the two must coincide,
ties / NaN / refusals, offsets past 2^31 elements, `MTL` with test_cfg seg mode='slide' through `MTL.forward`, and the pre_eval
test loop of rscotr_amd.engine.

The reference, the cases and the label-comparison rule (labels equal wherever the fp64 top-1 minus top-2 gap is at least
tol = 2 * (64 + K + 2) * 2^-24 * max|logit|; at most 0.1 % of a case's pixels under tol) live in tests/test_seg_slide_cpu.py."""
import copy

import numpy as np
import pytest
import torch

from rscotr_amd import ops, synth
from test_seg_slide_cpu import CASES, case, chain, check_labels, clear_mask, literal_windows
from util import build_model, load_model_cfg

pytestmark = pytest.mark.gpu


def call(name, device):
    logits, B, kw, ref, K, L = case(name)
    return ops.seg_predict_slide(logits.to(device), B, **kw)


@pytest.mark.parametrize('name', sorted(CASES))
def test_seg_predict_slide_against_fp64_chain(cuda, name):
    logits, B, kw, ref, K, L = case(name)
    got = call(name, cuda)
    assert got.is_cuda and tuple(got.shape) == (B,) + tuple(kw['out_hw'] if kw['out_hw'] is not None else kw['canvas_hw'])
    check_labels(got, ref, K, L, name)
    if ref.shape[1] == 1:
        assert int(got.max()) == 0
    assert torch.equal(got, call(name, cuda))  # run to run


def test_single_window_is_seg_predict(cuda):
    """Case g has one window: the labels of ops.seg_predict on the same logits."""
    logits, B, kw, ref, K, L = case('g')
    assert K == 1 and logits.shape[0] == B
    want, clear = clear_mask(ref, K, L)
    got = call('g', cuda).cpu()
    single = ops.seg_predict(logits.to(cuda), kw['canvas_hw'], crop_hw=kw['crop_hw'], out_hw=kw['out_hw'], flip=kw['flip']).cpu()
    print(f'[seg_predict_slide g vs seg_predict] differing pixels {int((single != got).sum())} of {got.numel()} (0 expected)')
    assert (single[clear] == got[clear]).all()


def test_disjoint_windows_are_seg_predict_per_window(cuda):
    """Case d has no overlap and no rescale: every window's block is ops.seg_predict of that window alone."""
    logits, B, kw, ref, K, L = case('d')
    assert K == 1
    want, clear = clear_mask(ref, K, L)
    got = call('d', cuda).cpu()
    windows = literal_windows(*kw['canvas_hw'], kw['crop_size'], kw['stride'])
    assert len(windows) == 2
    differing = 0
    for k, (y1, y2, x1, x2) in enumerate(windows):
        alone = ops.seg_predict(logits[k * B:(k + 1) * B].to(cuda), (y2 - y1, x2 - x1)).cpu()
        block, ok = got[:, y1:y2, x1:x2], clear[:, y1:y2, x1:x2]
        differing += int((alone != block).sum())
        assert (alone[ok] == block[ok]).all(), k
    print(f'[seg_predict_slide d vs seg_predict per window] differing pixels {differing} of {got.numel()} (0 expected)')


def test_ties_and_nan(cuda):
    g = torch.Generator().manual_seed(7)
    geo = dict(canvas_hw=(40, 36), crop_size=(24, 24), stride=(16, 12))  # 2 x 2 windows, up to 4 over a pixel
    n = len(literal_windows(40, 36, (24, 24), (16, 12)))
    assert n == 4
    # channels 1 and 2 equal and largest in every window -> the lower index
    t = torch.zeros(n * 2, 4, 3, 3)
    t[:, 1] = torch.randn((n * 2, 3, 3), generator=g).abs() + 1.0
    t[:, 2] = t[:, 1]
    for kw in (dict(), dict(out_hw=(45, 31)), dict(crop_hw=(37, 35), out_hw=(33, 50), flip='horizontal')):
        assert (ops.seg_predict_slide(t.to(cuda), 2, **geo, **kw).cpu() == 1).all(), kw
    # all channels NaN in one image: the first NaN wins
    t2 = t.clone()
    t2[1::2, 1:4] = float('nan')
    got = ops.seg_predict_slide(t2.to(cuda), 2, **geo, out_hw=(45, 31)).cpu()
    assert (got[0] == 1).all() and (got[1] == 1).all()
    # one NaN logit in one window: it claims exactly the pixels the fp32 torch chain turns NaN in that channel
    clean = torch.randn((n, 4, 3, 3), generator=g)
    dirty = clean.clone()
    dirty[1, 3, 1, 2] = float('nan')  # window 1 (top right), channel 3
    for kw in (dict(img_shape=(37, 35), out=(33, 50)), dict()):
        ref32, _ = chain(dirty, 1, (40, 36), (24, 24), (16, 12), dtype=torch.float32, **kw)
        hit = torch.isnan(ref32[:, 3])
        assert 0 < int(hit.sum()) < hit.numel() and not torch.isnan(ref32[:, :3]).any()
        got = ops.seg_predict_slide(dirty.to(cuda), 1, **geo, crop_hw=kw.get('img_shape'), out_hw=kw.get('out')).cpu()
        assert (got[hit] == 3).all()
        # elsewhere the labels are those of the input without the NaN
        stand_in = clean.clone()
        stand_in[1, 3, 1, 2] = 0.0
        ref, K = chain(stand_in, 1, (40, 36), (24, 24), (16, 12), **kw)
        want, clear = clear_mask(ref, K, float(stand_in.abs().max()))
        keep = clear & ~hit
        assert int(keep.sum()) > 0 and (got[keep].long() == want[keep]).all()


def test_refusals(cuda):
    geo = dict(canvas_hw=(8, 8), crop_size=(4, 4), stride=(4, 4))
    z = lambda C=3: torch.zeros(4, C, 2, 2, device=cuda)
    assert tuple(ops.seg_predict_slide(z(255), 1, **geo).shape) == (1, 8, 8)
    with pytest.raises(RuntimeError):
        ops.seg_predict_slide(z(256), 1, **geo)
    with pytest.raises(RuntimeError):
        ops.seg_predict_slide(z(), 1, **geo, out_hw=(0, 4))
    with pytest.raises(RuntimeError):
        ops.seg_predict_slide(z(), 1, **geo, crop_hw=(9, 8), out_hw=(4, 4))
    with pytest.raises(RuntimeError):
        ops.seg_predict_slide(z().cpu(), 1, **geo)
    with pytest.raises(ValueError):
        ops.seg_predict_slide(z(), 1, **dict(geo, stride=(5, 4)))
    with pytest.raises(ValueError):
        ops.seg_predict_slide(z(), 2, **geo)
    with pytest.raises(ValueError):
        ops.seg_predict_slide(z(), 1, **geo, flip='diagonal')
    # the C entry checks the grid itself (a caller that bypasses the op)
    from rscotr_amd._lib import lib
    out = torch.empty(1, 8, 8, dtype=torch.uint8, device=cuda)
    with pytest.raises(RuntimeError, match='uncovered'):
        lib.call('rscotr_seg_predict_slide_u8', z().data_ptr(), out.data_ptr(), 1, 3, 2, 2, 8, 8, 4, 4, 5, 4, 0, 0, 0, 0, 0, 0, None)


def test_offsets_past_31_bits(cuda):
    """130 windows of (255, 256, 256) logits are 2.17e9 elements: the last window's offset does not fit 31 bits.  Zeros except
    the first and the last window, whose blocks must be ops.seg_predict of those windows alone (the one-window path, no
    rescale); an identity rescale (the general path: every outer tap has weight 1 on one canvas pixel) must give the same
    map bit for bit."""
    n, C, hw = 130, 255, (256, 256)
    geo = dict(canvas_hw=(8, 8 * n), crop_size=(8, 8), stride=(8, 8))
    logits = torch.zeros((n, C) + hw, device=cuda)
    assert logits.numel() > 2 ** 31
    g = torch.Generator(device=cuda).manual_seed(3)
    for k in (0, n - 1):
        logits[k] = torch.randn((C,) + hw, device=cuda, generator=g)
    got = ops.seg_predict_slide(logits, 1, **geo)
    for k in (0, n - 1):
        alone = ops.seg_predict(logits[k:k + 1], (8, 8))
        assert torch.equal(got[:, :, 8 * k:8 * k + 8], alone), k
        assert int(alone.max()) > 0
    assert int(got[:, :, 8:8 * (n - 1)].max()) == 0
    assert torch.equal(ops.seg_predict_slide(logits, 1, **geo, out_hw=(8, 8 * n)), got)
    del logits
    torch.cuda.empty_cache()


# ---- the model ---------------------------------------------------------------------------------------------------------------
SLIDE = dict(mode='slide', crop_size=(64, 64), stride=(32, 32))


@pytest.fixture(scope='module')
def model(cuda):
    """The tiny model in test mode 'slide', its untrained mask decoder damped as in tests/test_seg_tta_gpu.py (a head that
    separates its channels, as a trained one does)."""
    cfg, mcfg = load_model_cfg(tiny=True)
    mcfg = copy.deepcopy(mcfg)
    mcfg['test_cfg'] = dict(mcfg['test_cfg'], seg=dict(SLIDE))
    m = build_model(mcfg)
    with torch.no_grad():
        for p in m.seg_head.transformer_decoder.parameters():
            if p.dim() > 1:
                p.mul_(0.25)
    ops.WPLANES.bump()  # (parameters rewritten in place)
    return m.to(cuda).eval()


def _run(model, img, metas, seg_cfg=None, **kw):
    old = model.test_cfg['seg']
    model.test_cfg['seg'] = dict(old if seg_cfg is None else seg_cfg)
    try:
        return model(task='seg', img=img, img_metas=metas, return_loss=False, rescale=True, **kw)
    finally:
        model.test_cfg['seg'] = old


def test_model_slide(model, cuda):
    ori = (80, 120, 3)
    b = synth.make_batch('seg', 2, 96, seed=6)
    metas = [dict(m, ori_shape=ori) for m in b['img_metas']]
    img = b['img'].to(cuda)
    out = _run(model, img, metas, on_device=True)
    assert isinstance(out, list) and len(out) == 2
    assert all(o.is_cuda and o.dtype == torch.uint8 and tuple(o.shape) == ori[:2] for o in out)
    out = torch.stack(out)
    # the reference is built from this model's own window logits
    with torch.no_grad():
        ops.RANGES.begin(cuda)
        logits, windows = model.slide_window_logits(img, metas)
    assert len(windows) == 4 and logits.shape[0] == 8
    ref, K = chain(logits.cpu(), 2, (96, 96), SLIDE['crop_size'], SLIDE['stride'], (96, 96), ori[:2])
    want, clear = check_labels(out, ref, K, float(logits.abs().max()), 'model')
    # the host route: int64 NumPy maps, equal to the device maps on the clear pixels
    host = _run(model, img, metas)
    assert isinstance(host, list) and len(host) == 2
    assert all(isinstance(p, np.ndarray) and p.dtype == np.int64 and p.shape == ori[:2] for p in host)
    host = torch.from_numpy(np.stack(host))
    assert (host[clear] == out.cpu().long()[clear]).all()
    # four windows in one forward pass
    stacked = torch.stack(_run(model, img, metas, seg_cfg=dict(SLIDE, window_batch=4), on_device=True))
    print(f'[model window_batch 4 vs 1] differing pixels {int((stacked != out).sum())} of {out.numel()}, on clear pixels '
          f'{int(((stacked != out).cpu() & clear).sum())}')
    assert (stacked.cpu()[clear] == out.cpu()[clear]).all()
    # without rescale the maps have the canvas size
    plain = model(task='seg', img=img, img_metas=metas, return_loss=False, rescale=False, on_device=True)
    assert all(tuple(p.shape) == (96, 96) and p.dtype == torch.uint8 for p in plain)
    ref0, K0 = chain(logits.cpu(), 2, (96, 96), SLIDE['crop_size'], SLIDE['stride'])
    check_labels(torch.stack(plain), ref0, K0, float(logits.abs().max()), 'model, no rescale')
    # a flipped input: the finished map is flipped back, on both routes
    fmetas = [dict(m, flip=True, flip_direction='horizontal') for m in metas]
    refh, _ = chain(logits.cpu(), 2, (96, 96), SLIDE['crop_size'], SLIDE['stride'], (96, 96), ori[:2], 'horizontal')
    check_labels(torch.stack(_run(model, img, fmetas, on_device=True)), refh, K, float(logits.abs().max()), 'model, flip')
    # a crop that holds the whole image is mode 'whole'
    whole = torch.stack(_run(model, img, metas, seg_cfg=dict(mode='whole'), on_device=True))
    one = torch.stack(_run(model, img, metas, seg_cfg=dict(mode='slide', crop_size=(96, 96), stride=(64, 64)), on_device=True))
    with torch.no_grad():
        ops.RANGES.begin(cuda)
        neck, bb = model.extract_feat(img)
        wl = model.seg_head.forward_test(neck, bb, metas, model.shared_encoder)
    refw, Kw = chain(wl.cpu(), 2, (96, 96), (96, 96), (64, 64), (96, 96), ori[:2])
    assert Kw == 1
    _, clearw = check_labels(whole, refw, Kw, float(wl.abs().max()), 'model, whole')
    print(f'[model slide with one window vs whole] differing pixels {int((one != whole).sum())} of {whole.numel()}')
    assert (one.cpu()[clearw] == whole.cpu()[clearw]).all()
    # device TTA with slide is refused by name
    with pytest.raises(NotImplementedError, match='slide'):
        _run(model, [img, img], [metas, fmetas], on_device=True)
    # ... and runs on the host route
    tta = _run(model, [img, img], [metas, fmetas])
    assert len(tta) == 2 and all(isinstance(p, np.ndarray) and p.shape == ori[:2] for p in tta)


def test_engine_pre_eval_loop_in_slide_mode(model, cuda, tmp_path):
    """single_gpu_test(..., seg=dict(pre_eval=True)) in slide mode on an on-disk TileSegDataset of three 96 x 96 tiles in
    batches of two: 4-tuples of int64 CPU vectors per image, equal to the areas of the device label maps of a direct loop."""
    from PIL import Image
    from rscotr_amd.engine import single_gpu_test
    from rscotr_amd.pipeline import DeviceCollate, DeviceLoader, TileSegDataset
    rng = np.random.RandomState(5)
    (tmp_path / 'img').mkdir(); (tmp_path / 'ann').mkdir()
    for i in range(3):
        Image.fromarray(rng.randint(0, 255, size=(96, 96, 3)).astype(np.uint8)).save(tmp_path / 'img' / f't{i}.png')
        Image.fromarray(rng.randint(0, 7, size=(96, 96)).astype(np.uint8)).save(tmp_path / 'ann' / f't{i}.png')
    ds = TileSegDataset(str(tmp_path / 'img'), str(tmp_path / 'ann'))
    ds.CLASSES = tuple(f'class{i}' for i in range(model.seg_head.num_queries))
    loaders = dict(potsdam=DeviceLoader(ds, DeviceCollate('seg', cuda, flip_prob=0.0), 2, test_mode=True))
    assert model.test_cfg['seg']['mode'] == 'slide'
    old = getattr(model, 'CLASSES', None)
    model.CLASSES = dict(potsdam=ds.CLASSES)
    try:
        res = single_gpu_test(model, loaders, kwargs_dict=dict(seg=dict(pre_eval=True)))['potsdam']
        assert not model.training
        maps = []
        for data in loaders['potsdam']:
            assert tuple(data['img'].shape[2:]) == (96, 96)
            maps.extend(model(return_loss=False, on_device=True, **data))
    finally:
        model.CLASSES = old
    assert len(res) == 3
    for r in res:
        assert isinstance(r, tuple) and len(r) == 4
        assert all(torch.is_tensor(a) and a.dtype == torch.int64 and not a.is_cuda and tuple(a.shape) == (100,) for a in r)
        assert torch.equal(r[1], r[2] + r[3] - r[0])
        assert int(r[2].sum()) > 0
    assert len(maps) == 3 and all(m.is_cuda and m.dtype == torch.uint8 and tuple(m.shape) == (96, 96) for m in maps)
    areas = ds.pre_eval(maps, [0, 1, 2])
    assert torch.equal(torch.as_tensor(areas).cpu(), torch.stack([torch.stack(r) for r in res]))
