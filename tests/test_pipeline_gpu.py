"""Device-side input path on the GPU against the NumPy restatement of the mm* pipeline steps (oracle/pipeline.py):
images within 1e-6 relative (one fp32 subtract and multiply per value), label maps and every geometric decision exact."""
import numpy as np
import pytest
import torch

from oracle import pipeline as OP
from rscotr_amd import pipeline as P

pytestmark = pytest.mark.gpu


def _samples(rng, n, hw_lo, hw_hi, seg=False, det=False):
    out = []
    for _ in range(n):
        h, w = rng.randint(hw_lo, hw_hi), rng.randint(hw_lo, hw_hi)
        s = dict(img=rng.randint(0, 256, (h, w, 3)).astype(np.uint8), gt_label=int(rng.randint(0, 45)))
        if seg:
            s['gt_semantic_seg'] = rng.randint(0, 7, (h, w)).astype(np.uint8)
        if det:
            k = rng.randint(1, 6)
            x1, y1 = rng.uniform(0, w / 2, k), rng.uniform(0, h / 2, k)
            s['gt_bboxes'] = np.stack([x1, y1, x1 + rng.uniform(2, w / 2, k), y1 + rng.uniform(2, h / 2, k)], -1).astype(np.float32)
            s['gt_labels'] = rng.randint(0, 20, k)
        out.append(s)
    return out


def _decisions(batch):
    wins = [(0, 0, m['img_shape'][1], m['img_shape'][0]) for m in batch['img_metas']]
    return wins, [m['flip'] for m in batch['img_metas']]


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_cls_and_det_batches(cuda, seed):
    rng = np.random.RandomState(seed)
    s = _samples(rng, 5, 30, 300, det=True)
    for task in ('cls', 'det'):
        c = P.collate_for(task, cuda)
        b = c(s, np.random.RandomState(seed + 10))
        wins, flips = _decisions(b)
        assert any(flips) or seed  # (seed 0 flips at least one)
        H, W = b['img'].shape[-2:]
        if task == 'det':
            assert H % 32 == 0 and W % 32 == 0 and H - 32 < max(x['img'].shape[0] for x in s) <= H
        ref = OP.prepare_batch([x['img'] for x in s], wins, flips, (H, W), P.IMG_NORM['mean'], P.IMG_NORM['std'], True)
        got = b['img'].cpu().numpy()
        assert got.shape == ref.shape and np.abs(got - ref).max() <= 1e-6 * np.abs(ref).max()
        if task == 'cls':
            assert b['gt_label'].tolist() == [x['gt_label'] for x in s]
        else:
            for x, bb, fl in zip(s, b['gt_bboxes'], flips):
                want = OP.bbox_flip(x['gt_bboxes'], x['img'].shape[1]) if fl else x['gt_bboxes']
                assert np.allclose(bb.cpu().numpy(), want, atol=1e-4)


@pytest.mark.parametrize('seed', [0, 3])
def test_seg_batches_crop_flip_pad_labels(cuda, seed):
    rng = np.random.RandomState(seed)
    s = _samples(rng, 4, 40, 700, seg=True)  # some tiles smaller than the 512x512 crop (padded), some larger (cropped)
    c = P.collate_for('seg', cuda)
    # replay the host decisions to hand them to the oracle
    r2 = np.random.RandomState(seed + 7)
    wins, flips = [], []
    for x in s:
        wins.append(c._crop_window_hw(*x['img'].shape[:2], x['gt_semantic_seg'], r2))
        flips.append(bool(r2.rand() < 0.5))
    b = c(s, np.random.RandomState(seed + 7))
    assert [m['flip'] for m in b['img_metas']] == flips
    ref = OP.prepare_batch([x['img'] for x in s], wins, flips, (512, 512), P.IMG_NORM['mean'], P.IMG_NORM['std'], True)
    got = b['img'].cpu().numpy()
    assert np.abs(got - ref).max() <= 1e-6 * np.abs(ref).max()
    lref = OP.prepare_seg_labels([x['gt_semantic_seg'] for x in s], wins, flips, (512, 512), True, 5)
    assert b['gt_semantic_seg'].dtype == torch.int64 and (b['gt_semantic_seg'].cpu().numpy() == lref).all()


def test_empty_batch_and_bad_arguments(cuda):
    from rscotr_amd._lib import lib
    import ctypes
    f = (ctypes.c_float * 3)(1, 1, 1)
    z = (ctypes.c_float * 3)(1, 0, 1)
    p = ctypes.cast(f, ctypes.c_void_p)
    lib.call('rscotr_img_prep_u8', 0, 0, 0, 0, 8, 8, p, p, 1, 0)  # B = 0: nothing to do
    t = torch.zeros(64, dtype=torch.uint8, device=cuda)
    with pytest.raises(RuntimeError):
        lib.call('rscotr_img_prep_u8', t.data_ptr(), t.data_ptr(), t.data_ptr(), 1, 4, 4, p, ctypes.cast(z, ctypes.c_void_p), 1, 0)
    with pytest.raises(RuntimeError):
        lib.call('rscotr_seg_label_prep_u8', t.data_ptr(), t.data_ptr(), t.data_ptr(), -1, 4, 4, 0, 255, 0)


def test_loader_feeds_a_train_step(cuda, tmp_path):
    """Decoded tiles -> DeviceLoader -> MultiDataLoader tagging -> MTL.train_step: the batch layout is the one the step
    consumes (a seg iteration at 128x128 on a tiny model)."""
    from PIL import Image
    import os
    from util import build_model, load_model_cfg
    from rscotr_amd import data as D
    rng = np.random.RandomState(0)
    os.makedirs(tmp_path / 'img'); os.makedirs(tmp_path / 'ann')
    for k in range(4):
        Image.fromarray(rng.randint(0, 256, (150, 140, 3)).astype(np.uint8)).save(tmp_path / 'img' / f't{k}.png')
        Image.fromarray(rng.randint(0, 7, (150, 140)).astype(np.uint8)).save(tmp_path / 'ann' / f't{k}.png')
    ds = P.TileSegDataset(str(tmp_path / 'img'), str(tmp_path / 'ann'))
    col = P.DeviceCollate('seg', cuda, crop_size=(128, 128), cat_max_ratio=0.75, reduce_zero_label=True, seg_pad_val=5)
    loaders = dict(potsdam=P.DeviceLoader(ds, col, batch_size=2, seed=1))
    m = D.MultiDataLoader(loaders, D.RoundRobinIterationStrategy(loaders))
    batch = next(iter(m))
    assert batch['task'] == 'seg' and batch['dataset_name'] == 'potsdam' and batch['img'].shape == (2, 3, 128, 128)
    cfg, mcfg = load_model_cfg(tiny=True)
    model = build_model(mcfg).to(cuda)
    out = model.train_step(batch)
    assert torch.isfinite(out['loss']) and 'seg.potsdam.seg.loss_ce' in out['log_vars']
