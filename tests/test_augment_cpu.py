"""Host side of the device resampling / colour stages (rscotr_amd/pipeline/) and the NumPy oracle they are tested against
(tests/aug_oracle.py), without a GPU: draw order against hand replays of the mm* sequences, resampling tables against the
oracle and Pillow, oracle known answers, the transform builder and the C ABI declarations."""
import ctypes
import math
import os

import numpy as np
import pytest
from PIL import Image

import aug_oracle as AO
from rscotr_amd import _lib
from rscotr_amd import pipeline as P
from rscotr_amd.pipeline import resample as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'aug_pil_bicubic.npz')


def _apply(img, xt, yt, mode):
    """What the kernel computes from one sample's tables (no flip): the integer rule of include/rscotr.h."""
    p = img.astype(np.int64)
    out = np.zeros((len(yt), len(xt), 3), np.int64)
    for i, ye in enumerate(yt):
        for j, xe in enumerate(xt):
            if mode == P.RESAMPLE_NEAREST:
                out[i, j] = p[ye[0], xe[0]]
                continue
            acc = np.zeros(3, np.int64)
            for a in range(ye[1]):
                hs = np.full(3, (1 << 21) if mode == P.RESAMPLE_PIL else 0, np.int64)
                for t in range(xe[1]):
                    hs += xe[2 + t] * p[ye[0] + a, xe[0] + t]
                acc += ye[2 + a] * (np.clip(hs >> 22, 0, 255) if mode == P.RESAMPLE_PIL else hs)
            out[i, j] = np.clip((acc + (1 << 21)) >> 22, 0, 255)
    return out.astype(np.uint8)


# ---- draw order --------------------------------------------------------------------------------------------------------
def test_seg_draw_order_and_cat_max_ratio_on_the_resized_label_map():
    """mmseg Resize.random_sample_ratio (one random_sample), rescale_size, RandomCrop with the cat_max_ratio retries on the
    NEAREST-RESIZED label map, RandomFlip, then PhotoMetricDistortion's randint / uniform sequence."""
    c = P.train_collate_for('seg', 'cpu')
    lab = np.zeros((300, 400), np.uint8)
    lab[:, 200:] = 1  # raw 0 = ignore after reduce_zero_label: only windows reaching x >= 200 * sf hold label 1 at all
    lab[150:, 200:] = 2
    d = c.draw((300, 400, 3), lab, np.random.RandomState(4))
    r = np.random.RandomState(4)
    ratio = r.random_sample() * 1.5 + 0.5
    scale = int(512 * ratio), int(512 * ratio)
    sf = min(max(scale) / 400, min(scale) / 300)
    nw, nh = int(400 * sf + 0.5), int(300 * sf + 0.5)
    assert d['rsz'] == (nw, nh)
    rl = AO.resize_nearest(lab, nw, nh)
    win = None
    for _ in range(11):
        oy, ox = r.randint(0, max(nh - 512, 0) + 1), r.randint(0, max(nw - 512, 0) + 1)
        win = (ox, oy, min(512, nw - ox), min(512, nh - oy))
        l, cnt = np.unique(rl[oy:oy + win[3], ox:ox + win[2]], return_counts=True)
        cnt = cnt[(l != 0) & (l != 255)]
        if len(cnt) > 1 and cnt.max() / cnt.sum() < 0.75:
            break
    assert d['win'] == win
    assert d['flip'] == bool(r.rand() < 0.5)
    flags, beta, ca, sa, hd = d['pm']
    want_flags = 0
    if r.randint(2):
        want_flags |= P.PM_BRIGHT
        assert beta == r.uniform(-32, 32)
    mode = r.randint(2)
    if mode == 1 and r.randint(2):
        want_flags |= P.PM_CONTRAST | P.PM_CONTRAST_FIRST
        assert ca == r.uniform(0.5, 1.5)
    if r.randint(2):
        want_flags |= P.PM_SAT
        assert sa == r.uniform(0.5, 1.5)
    if r.randint(2):
        want_flags |= P.PM_HUE
        assert hd == r.randint(-18, 18)
    if mode == 0 and r.randint(2):
        want_flags |= P.PM_CONTRAST
        assert ca == r.uniform(0.5, 1.5)
    assert flags == want_flags
    assert np.random.RandomState(4).random_sample() != r.random_sample()  # (the stream moved on)


def test_seg_crop_retries_see_the_resized_map_not_the_raw_one():
    """A 2x upscale moves a class boundary: the retry decisions follow the resized label map."""
    c = P.DeviceCollate('seg', 'cpu', crop_size=(16, 16), cat_max_ratio=0.75, reduce_zero_label=True,
                        resize=dict(img_scale=(80, 60), keep_ratio=True), flip_prob=0.0)
    lab = np.ones((30, 40), np.uint8)
    lab[:10] = 2
    d = c.draw((30, 40, 3), lab, np.random.RandomState(0))
    assert d['rsz'] == (80, 60)
    rl = AO.resize_nearest(lab, 80, 60)
    r = np.random.RandomState(0)
    for _ in range(11):
        oy, ox = r.randint(0, 45), r.randint(0, 65)
        w = rl[oy:oy + 16, ox:ox + 16]
        if max((w == 1).mean(), (w == 2).mean()) < 0.75:
            break
    assert d['win'] == (ox, oy, 16, 16)


def test_cls_draw_order_random_resized_crop_fallback_flip_erasing():
    c = P.train_collate_for('cls', 'cpu')
    for seed, shape in ((0, (256, 256, 3)), (1, (256, 256, 3)), (2, (20, 300, 3)), (3, (300, 20, 3))):
        d = c.draw(shape, None, np.random.RandomState(seed))
        r = np.random.RandomState(seed)
        H, W = shape[:2]
        got = None
        for _ in range(10):
            ta = r.uniform(0.08, 1.0) * H * W
            ar = math.exp(r.uniform(math.log(3 / 4), math.log(4 / 3)))
            tw, th = int(round(math.sqrt(ta * ar))), int(round(math.sqrt(ta / ar)))
            if 0 < tw <= W and 0 < th <= H:
                oy, ox = r.randint(0, H - th + 1), r.randint(0, W - tw + 1)
                got = (ox, oy, tw, th)
                break
        if got is None:  # central fallback
            if W / H > 4 / 3:
                th, tw = H, int(round(H * 4 / 3))
            else:
                tw, th = W, int(round(W / (3 / 4)))
            got = ((W - tw) // 2, (H - th) // 2, tw, th)
        if shape[0] == 20:
            assert got == (136, 0, 27, 20)
        if shape[1] == 20:
            assert got == (0, 136, 20, 27)
        assert d['src'] == got and d['rsz'] == (224, 224) and d['win'] == (0, 0, 224, 224)
        assert d['flip'] == bool(r.rand() < 0.5)
        er = AO.random_erasing(np.zeros((224, 224, 3), np.uint8) + 7, r, **P.CLS_ERASING)
        if d['erase'] is None:
            assert (er == 7).all()
        else:
            x, y, w, h, patch = d['erase']
            assert (er[y:y + h, x:x + w] == patch).all()
            assert not (np.delete(np.delete(er, np.s_[y:y + h], 0), np.s_[x:x + w], 1) != 7).any()


def test_det_draw_order_keep_ratio_then_flip():
    c = P.train_collate_for('det', 'cpu')
    d = c.draw((700, 1000, 3), None, np.random.RandomState(1))
    assert d['rsz'] == (1143, 800) and d['win'] == (0, 0, 1143, 800)
    assert d['flip'] == bool(np.random.RandomState(1).rand() < 0.5)


def test_defaults_stay_on_the_old_path():
    for t in ('cls', 'det', 'seg'):
        assert not P.collate_for(t, 'cpu').augmented
        assert P.train_collate_for(t, 'cpu').augmented and P.eval_collate_for(t, 'cpu').augmented


# ---- tables and oracle ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', ['bilinear', 'bicubic', 'nearest'])
def test_host_tables_reproduce_the_oracle(mode):
    rng = np.random.RandomState(5)
    m = dict(bilinear=P.RESAMPLE_LINEAR, bicubic=P.RESAMPLE_PIL, nearest=P.RESAMPLE_NEAREST)[mode]
    ref = dict(bilinear=AO.resize_bilinear, bicubic=AO.resize_bicubic_pil,
               nearest=lambda a, w, h: AO.resize_nearest(a, w, h))[mode]
    for H, W, h, w in ((1, 1, 3, 4), (1, 7, 2, 5), (6, 1, 3, 3), (16, 24, 8, 12), (13, 17, 29, 31), (40, 9, 7, 23)):
        img = rng.randint(0, 256, (H, W, 3)).astype(np.uint8)
        got = _apply(img, R._AXIS[m](W, w, 0, 0, w), R._AXIS[m](H, h, 0, 0, h), m)
        assert (got == ref(img, w, h)).all(), (H, W, h, w)
    # a window of the resized frame and a source offset (RandomResizedCrop's crop) fold into the entries
    img = rng.randint(0, 256, (30, 40, 3)).astype(np.uint8)
    got = _apply(img, R._AXIS[m](25, 50, 10, 7, 20), R._AXIS[m](12, 30, 4, 3, 21), m)
    assert (got == ref(img[4:16, 10:35], 50, 30)[3:24, 7:27]).all()


def test_oracle_pil_bicubic_path_equals_pillow_on_random_crops():
    rng = np.random.RandomState(11)
    for _ in range(6):
        img = rng.randint(0, 256, (64, 80, 3)).astype(np.uint8)
        y, x = rng.randint(0, 30), rng.randint(0, 40)
        crop = img[y:y + rng.randint(5, 34), x:x + rng.randint(5, 40)]
        for w, h in ((224, 224), (3, 4)):  # up and down
            want = np.asarray(Image.fromarray(np.ascontiguousarray(crop)).resize((w, h), Image.BICUBIC))
            assert (AO.resize_bicubic_pil(crop, w, h) == want).all()
            t = _apply(crop, R._axis_pil_bicubic(crop.shape[1], w, 0, 0, w), R._axis_pil_bicubic(crop.shape[0], h, 0, 0, h),
                       P.RESAMPLE_PIL)
            assert (t == want).all()


def test_committed_pillow_outputs_match_the_installed_pillow():
    from golden import make_aug_golden
    g = np.load(GOLDEN)
    for k, v in make_aug_golden.make().items():
        assert (g[k] == v).all(), k


def test_oracle_known_answers():
    rng = np.random.RandomState(0)
    img = rng.randint(0, 256, (9, 13, 3)).astype(np.uint8)
    for f in (AO.resize_bilinear, AO.resize_nearest, AO.resize_bicubic_pil):
        assert (f(img, 13, 9) == img).all()  # identity size: a copy
    up = AO.resize_nearest(img, 26, 18)
    assert (up[::2, ::2] == img).all() and (up[1::2, 1::2] == img).all()  # x2 nearest duplicates
    grey = np.repeat(np.arange(256, dtype=np.uint8)[:, None, None], 3, 2)
    hsv = AO.bgr2hsv(grey)
    assert (hsv[..., 1] == 0).all() and (hsv[..., 2] == grey[..., 0]).all()
    hsv[..., 1] = AO.convert(hsv[..., 1], alpha=1.0)
    assert (AO.hsv2bgr(hsv) == grey).all()  # grey survives the round trip at saturation 1.0
    assert AO.convert(np.array([200], np.uint8), alpha=1.5)[0] == 255
    assert AO.convert(np.array([10], np.uint8), beta=0.7)[0] == 10  # 10.7 truncates
    assert AO.convert(np.array([5], np.uint8), beta=-9.0)[0] == 0
    red = np.array([[[0, 0, 255]]], np.uint8)  # BGR pure red: hue 0
    h = AO.bgr2hsv(red)
    assert h.tolist() == [[[0, 255, 255]]]
    blue = AO.bgr2hsv(np.array([[[255, 0, 0]]], np.uint8))
    assert blue[0, 0, 0] == 120
    r = type('R', (), {})()
    seq = [0, 0, 0, 1, -18, 0]  # no brightness, mode 0, no saturation, hue -18, no contrast

    def pop(*a):
        return seq.pop(0)
    r.randint = r.uniform = pop
    shifted = AO.photometric(red, r)
    assert AO.bgr2hsv(shifted)[0, 0, 0] == 162  # (0 - 18) mod 180
    boxes = np.array([[10, 20, 300, 90], [-5, 1, 2, 500]], np.float32)
    sf = np.array([1.5, 2.0, 1.5, 2.0], np.float32)
    out = AO.boxes_rescale(boxes, sf, (200, 400, 3))
    assert out.tolist() == [[15, 40, 400, 180], [0, 2, 3, 200]]
    assert (P.scale_boxes(boxes, sf, (200, 400, 3)) == out).all()
    assert AO.rescale_wh(1000, 700, (1333, 800)) == (1143, 800) == P.rescale_size(1000, 700, (1333, 800))[0]


# ---- builder and ABI -----------------------------------------------------------------------------------------------
def _ref_pipelines():
    cfg = P.IMG_NORM
    cls_train = [dict(type='LoadImageFromFile'),
                 dict(type='RandomResizedCrop', size=224, backend='pillow', interpolation='bicubic'),
                 dict(type='RandomFlip', flip_prob=0.5, direction='horizontal'),
                 dict(type='RandAugment', policies=[], num_policies=2, total_level=10, magnitude_level=9),
                 dict(type='RandomErasing', erase_prob=0.25, mode='rand', min_area_ratio=0.02, max_area_ratio=1 / 3,
                      fill_color=cfg['mean'][::-1], fill_std=cfg['std'][::-1]),
                 dict(type='Normalize', **cfg), dict(type='ImageToTensor', keys=['img']),
                 dict(type='ToTensor', keys=['gt_label']), dict(type='Collect', keys=['img', 'gt_label'])]
    seg_train = [dict(type='LoadImageFromFile'), dict(type='LoadAnnotations', reduce_zero_label=True),
                 dict(type='Resize', img_scale=(512, 512), ratio_range=(0.5, 2.0)),
                 dict(type='RandomCrop', crop_size=(512, 512), cat_max_ratio=0.75), dict(type='RandomFlip', prob=0.5),
                 dict(type='PhotoMetricDistortion'), dict(type='Normalize', **cfg),
                 dict(type='Pad', size=(512, 512), pad_val=0, seg_pad_val=5), dict(type='DefaultFormatBundle'),
                 dict(type='Collect', keys=['img', 'gt_semantic_seg'])]
    det_test = [dict(type='LoadImageFromFile'),
                dict(type='MultiScaleFlipAug', img_scale=(1333, 800), flip=False,
                     transforms=[dict(type='Resize', keep_ratio=True), dict(type='RandomFlip'), dict(type='Normalize', **cfg),
                                 dict(type='Pad', size_divisor=32), dict(type='ImageToTensor', keys=['img']),
                                 dict(type='Collect', keys=['img'])])]
    return cls_train, seg_train, det_test


def test_build_collate_refuses_randaugment_unless_told_to_skip():
    cls_train, seg_train, det_test = _ref_pipelines()
    with pytest.raises(NotImplementedError, match='RandAugment'):
        P.build_collate('cls', cls_train, 'cpu')
    c = P.build_collate('cls', cls_train, 'cpu', unsupported='skip')
    assert c.skipped == ['RandAugment'] and c.rrc['size'] == 224 and c.resample == P.RESAMPLE_PIL
    assert c.erasing['erase_prob'] == 0.25 and c.flip_prob == 0.5
    s = P.build_collate('seg', seg_train, 'cpu')
    ref = P.train_collate_for('seg', 'cpu')
    for k in ('resize', 'crop_size', 'cat_max_ratio', 'reduce_zero_label', 'seg_pad_val', 'photometric', 'flip_prob'):
        assert getattr(s, k) == getattr(ref, k), k
    d = P.build_collate('det', det_test, 'cpu')
    e = P.eval_collate_for('det', 'cpu')
    assert d.resize == e.resize and d.size_divisor == 32 and d.flip_prob == 0.0
    with pytest.raises(NotImplementedError, match='interpolation'):
        P.build_collate('cls', [dict(type='Resize', size=(224, 224), backend='pillow', interpolation='lanczos')], 'cpu')


def test_header_declares_the_new_entries_with_c_types_only():
    sigs = _lib.parse_header()
    for name, n in (('rscotr_img_aug_u8', 12), ('rscotr_seg_label_aug_u8', 10)):
        ret, args = sigs[name]
        assert ret is ctypes.c_int and len(args) == n
        assert all(a in (ctypes.c_void_p, ctypes.c_int) for a in args)
    assert _lib.header_abi_version() == 11
