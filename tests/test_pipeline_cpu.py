"""Host side of the device input path (rscotr_amd/pipeline/): dataset readers on the three on-disk layouts, the random
decisions drawn like the mm* transforms draw them, and the oracle's own known answers."""
import json
import os

import numpy as np
import pytest

from oracle import pipeline as OP
from rscotr_amd import pipeline as P


def _save(path, arr):
    from PIL import Image
    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(arr).save(path)


def test_oracle_known_answers():
    img = np.arange(2 * 3 * 3, dtype=np.uint8).reshape(2, 3, 3)  # BGR
    n = OP.imnormalize(img, [1, 2, 3], [2, 4, 8], to_rgb=True)
    # pixel (0,0) = BGR (0,1,2) -> RGB (2,1,0) -> ((2-1)/2, (1-2)/4, (0-3)/8)
    assert np.allclose(n[0, 0], [0.5, -0.25, -0.375])
    assert (OP.imflip(img)[:, 0] == img[:, 2]).all()
    assert OP.impad(n, (4, 5)).shape == (4, 5, 3) and OP.impad(n, (4, 5))[3, 4, 0] == 0
    assert OP.reduce_zero_label(np.array([0, 1, 6, 255])).tolist() == [255, 0, 5, 255]
    assert OP.bbox_flip(np.array([[10., 5., 30., 9.]]), 100).tolist() == [[70., 5., 90., 9.]]


def test_dataset_readers(tmp_path):
    rng = np.random.RandomState(0)
    root = str(tmp_path)
    for c in ('airport', 'beach'):
        for k in range(2):
            _save(f'{root}/cls/{c}/{c}_{k}.png', rng.randint(0, 255, (20, 24, 3), dtype=np.uint8))
    ds = P.FolderClsDataset(f'{root}/cls')
    assert ds.CLASSES == ['airport', 'beach'] and len(ds) == 4 and ds[3]['gt_label'] == 1
    s = ds[0]
    assert s['img'].shape == (20, 24, 3) and s['img'].dtype == np.uint8
    from PIL import Image
    assert (s['img'][..., ::-1] == np.asarray(Image.open(s['filename']).convert('RGB'))).all()  # BGR like mmcv.imread
    # COCO-format detection annotations
    _save(f'{root}/det/img/a.png', rng.randint(0, 255, (64, 80, 3), dtype=np.uint8))
    _save(f'{root}/det/img/b.png', rng.randint(0, 255, (64, 80, 3), dtype=np.uint8))
    coco = dict(images=[dict(id=1, file_name='a.png', width=80, height=64), dict(id=2, file_name='b.png', width=80, height=64)],
                categories=[dict(id=7, name='ship'), dict(id=9, name='dam')],
                annotations=[dict(id=1, image_id=1, category_id=7, bbox=[10, 8, 20, 16], area=320, iscrowd=0),
                             dict(id=2, image_id=1, category_id=9, bbox=[1, 1, 0.5, 4], area=2, iscrowd=0),   # degenerate
                             dict(id=3, image_id=1, category_id=9, bbox=[30, 30, 10, 10], area=100, iscrowd=1)])  # crowd
    with open(f'{root}/det/ann.json', 'w') as fh:
        json.dump(coco, fh)
    dd = P.CocoDetDataset(f'{root}/det/ann.json', f'{root}/det/img', classes=('dam', 'ship'))
    assert len(dd) == 1  # image b has no boxes: filtered
    assert dd[0]['gt_bboxes'].tolist() == [[10., 8., 30., 24.]] and dd[0]['gt_labels'].tolist() == [1]
    # segmentation tiles
    _save(f'{root}/seg/img/t1.png', rng.randint(0, 255, (32, 32, 3), dtype=np.uint8))
    _save(f'{root}/seg/ann/t1.png', rng.randint(0, 7, (32, 32), dtype=np.uint8))
    sd = P.TileSegDataset(f'{root}/seg/img', f'{root}/seg/ann')
    assert len(sd) == 1 and sd[0]['gt_semantic_seg'].shape == (32, 32) and sd[0]['gt_semantic_seg'].max() <= 6


def test_random_decisions_follow_the_reference_draw_order():
    """mmseg RandomCrop.get_crop_bbox draws np.random.randint(0, margin_h + 1), then (0, margin_w + 1); RandomFlip draws
    np.random.rand() < prob afterwards: a seeded run must make those decisions."""
    c = P.DeviceCollate('seg', 'cpu', crop_size=(16, 16), cat_max_ratio=1.0)
    img = np.zeros((40, 50, 3), np.uint8)
    rng = np.random.RandomState(5)
    oy, ox = rng.randint(0, 25), rng.randint(0, 35)
    want = (ox, oy, 16, 16)
    assert c._crop_window_hw(*img.shape[:2], None, np.random.RandomState(5)) == want
    # an image smaller than the crop is taken whole (and padded on the device)
    assert c._crop_window_hw(10, 12, None, np.random.RandomState(1)) == (0, 0, 12, 10)
    # cat_max_ratio: a window dominated by one class is re-drawn (up to 10 times, then the last draw is kept)
    seg = np.ones((40, 50), np.uint8)
    seg[:20] = 2                      # two classes split at row 20: windows with y0 in 5..19 hold both
    seg[20:, :] = 1
    c2 = P.DeviceCollate('seg', 'cpu', crop_size=(16, 16), cat_max_ratio=0.75, reduce_zero_label=True)
    rng = np.random.RandomState(0)
    want = None
    for _ in range(11):               # the reference's loop, restated: first draw + up to 10 re-draws
        oy, ox = rng.randint(0, 25), rng.randint(0, 35)
        w = seg[oy:oy + 16, ox:ox + 16]
        want = (ox, oy, 16, 16)
        frac = max((w == 1).mean(), (w == 2).mean())
        if frac < 0.75:
            break
    assert c2._crop_window_hw(*img.shape[:2], seg, np.random.RandomState(0)) == want
    # raw label 0 is the ignore index after reduce_zero_label: a window of {0, 1} counts as single-class
    seg0 = np.zeros((40, 50), np.uint8)
    seg0[:, 25:] = 1
    r = np.random.RandomState(3)
    last = None
    for _ in range(11):
        oy, ox = r.randint(0, 25), r.randint(0, 35)
        last = (ox, oy, 16, 16)
    assert c2._crop_window_hw(*img.shape[:2], seg0, np.random.RandomState(3)) == last  # all 11 draws used


def test_collate_fails_loudly_without_gpu():
    c = P.collate_for('cls', 'cpu')
    with pytest.raises(RuntimeError):
        c([dict(img=np.zeros((8, 8, 3), np.uint8), gt_label=1)])
