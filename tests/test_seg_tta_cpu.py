"""Host side of the segmentation test-time augmentation: the refusals of rscotr_seg_predict_tta_u8 (every one sits before the
first HIP call, so they run without a device), the MultiScaleFlipAug view planner and build_collate's TTA branch."""
import ctypes

import numpy as np
import pytest

from rscotr_amd import _lib
from rscotr_amd import pipeline as P


@pytest.fixture(scope='module')
def tta_entry():
    dll = ctypes.CDLL(_lib.LIB_PATH)
    ret, args = _lib.parse_header()['rscotr_seg_predict_tta_u8']
    assert ret is ctypes.c_int and args == [ctypes.c_void_p] * 2 + [ctypes.c_int] * 5 + [ctypes.c_void_p]
    fn = dll.rscotr_seg_predict_tta_u8  # AttributeError if the library does not export it
    fn.restype, fn.argtypes = ret, args
    dll.rscotr_last_error.restype = ctypes.c_char_p

    def call(rows, V, C=5):
        rows = np.ascontiguousarray(rows, dtype=np.int64)
        out = np.zeros(2 * 8 * 8, dtype=np.uint8)  # (never written: every call below is refused)
        rc = fn(rows.ctypes.data, out.ctypes.data, V, 2, C, 8, 8, None)
        return rc, dll.rscotr_last_error().decode()
    return call


def test_entry_refuses_bad_view_tables_before_any_hip_call(tta_entry):
    fake = 0x10000  # a non-null "device address": no refused call reads it
    good = [fake, 4, 4, 8, 8, 8, 8, 0]
    for rows, V, C, word in (([good], 0, 5, 'V = 0'), ([good] * 17, 17, 5, 'V = 17'),
                             ([[fake, 4, 4, 8, 8, 9, 8, 0]], 1, 5, 'crop'), ([good, [fake, 4, 4, 8, 8, 8, 9, 1]], 2, 5, 'view 1'),
                             ([good], 1, 256, 'C = 256'), ([[0, 4, 4, 8, 8, 8, 8, 0]], 1, 5, 'null'),
                             ([[fake, 4, 4, 8, 8, 8, 8, 3]], 1, 5, 'flip'), ([[fake, 0, 4, 8, 8, 8, 8, 0]], 1, 5, 'size'),
                             ([[fake, 1 << 15, 1 << 15, 8, 8, 8, 8, 0]], 1, 5, '31 bits')):
        rc, msg = tta_entry(rows, V, C)
        assert rc != 0 and 'rscotr_seg_predict_tta_u8' in msg and word in msg, (rows, V, C, rc, msg)


def test_view_planner_against_hand_worked_lists():
    views = P.plan_tta_views(img_scale=(512, 512), img_ratios=[0.5, 0.75, 1.0, 1.25, 1.5, 1.75], flip=True)
    scales = [(256, 256), (384, 384), (512, 512), (640, 640), (768, 768), (896, 896)]
    assert views == [(s, f, 'horizontal' if f else None) for s in scales for f in (False, True)]
    assert P.plan_tta_views(img_scale=None, img_ratios=[1.0, 1.5], img_hw=(600, 400)) == \
        [((400, 600), False, None), ((600, 900), False, None)]
    assert P.plan_tta_views(img_scale=[(512, 512), (1024, 768)], flip=False) == \
        [((512, 512), False, None), ((1024, 768), False, None)]
    assert P.plan_tta_views(img_scale=(2048, 512), img_ratios=[0.5], flip=True) == \
        [((1024, 256), False, None), ((1024, 256), True, 'horizontal')]
    with pytest.raises(ValueError):
        P.plan_tta_views(img_scale=None, img_ratios=None)


def _seg_test_pipeline(**msfa):
    transforms = [dict(type='Resize', keep_ratio=True), dict(type='RandomFlip'), dict(type='Normalize', **P.IMG_NORM),
                  dict(type='ImageToTensor', keys=['img']), dict(type='Collect', keys=['img'])]
    return [dict(type='LoadImageFromFile'), dict(dict(type='MultiScaleFlipAug', flip=False, transforms=transforms), **msfa)]


def test_build_collate_takes_seg_tta_and_keeps_everything_else():
    ratios = [0.5, 0.75, 1.0, 1.25, 1.5, 1.75]
    c = P.build_collate('seg', _seg_test_pipeline(img_scale=(512, 512), img_ratios=ratios, flip=True), 'cpu')
    assert isinstance(c, P.SegTTACollate) and len(c.views) == 12 and c.task == 'seg'
    assert c.views[:3] == [((256, 256), False, None), ((256, 256), True, 'horizontal'), ((384, 384), False, None)]
    v = c._collate((256, 256), True)
    assert isinstance(v, P.DeviceCollate) and v.flip_prob == 1.0 and v.resize == dict(img_scale=(256, 256), ratio_range=None,
                                                                                      keep_ratio=True)
    assert c._collate((256, 256), False).flip_prob == 0.0
    c = P.build_collate('seg', _seg_test_pipeline(img_scale=None, img_ratios=[1.0, 1.5]), 'cpu')
    assert isinstance(c, P.SegTTACollate) and c.views is None and len(c._plan((600, 400))) == 2
    c = P.build_collate('seg', _seg_test_pipeline(img_scale=[(512, 512), (768, 768)]), 'cpu')
    assert isinstance(c, P.SegTTACollate) and len(c.views) == 2
    # one ratio other than 1.0 is a one-view plan at the scaled size
    c = P.build_collate('seg', _seg_test_pipeline(img_scale=(512, 512), img_ratios=[0.5]), 'cpu')
    assert isinstance(c, P.SegTTACollate) and c.views == [((256, 256), False, None)]
    assert c._collate((256, 256), False).labels is False and P.eval_collate_for('seg', 'cpu').labels is True
    # the kernel's view limit
    with pytest.raises(ValueError, match='16'):
        P.build_collate('seg', _seg_test_pipeline(img_scale=(512, 512), img_ratios=[0.5 + 0.125 * i for i in range(9)], flip=True),
                        'cpu')
    P.build_collate('seg', _seg_test_pipeline(img_scale=(512, 512), img_ratios=[0.5 + 0.125 * i for i in range(8)], flip=True), 'cpu')
    with pytest.raises(NotImplementedError, match='vertical'):
        P.build_collate('seg', _seg_test_pipeline(img_scale=(512, 512), flip=True, flip_direction='vertical'), 'cpu')
    # cls and det keep refusing
    with pytest.raises(NotImplementedError):
        P.build_collate('det', _seg_test_pipeline(img_scale=(1333, 800), flip=True), 'cpu')
    with pytest.raises(NotImplementedError):
        P.build_collate('det', _seg_test_pipeline(img_scale=[(1333, 800), (2000, 1200)]), 'cpu')
    with pytest.raises(NotImplementedError):
        P.build_collate('cls', _seg_test_pipeline(img_scale=(224, 224), flip=True), 'cpu')
    # the single-view pipelines of the Potsdam config build what they build today: val (img_scale=(512, 512)) the eval
    # collate, test (img_scale=None, img_ratios=[1.0]) a plain collate at the image's own size
    e = P.eval_collate_for('seg', 'cpu')
    for cfg in (dict(img_scale=(512, 512)), dict(img_scale=(512, 512), img_ratios=[1.0]), dict(img_scale=[(512, 512)])):
        s = P.build_collate('seg', _seg_test_pipeline(**cfg), 'cpu')
        assert type(s) is P.DeviceCollate
        for k in ('resize', 'flip_prob', 'crop_size', 'size_divisor', 'resample', 'mean', 'std', 'to_rgb', 'augmented',
                  'photometric', 'erasing', 'rrc', 'rand_augment', 'seg_pad_val', 'cat_max_ratio'):
            assert getattr(s, k) == getattr(e, k), (cfg, k)
    s = P.build_collate('seg', _seg_test_pipeline(img_scale=None, img_ratios=[1.0]), 'cpu')
    assert type(s) is P.DeviceCollate and s.resize is None and s.flip_prob == 0.0 and not s.augmented


def test_tta_collate_refuses_mixed_shapes():
    c = P.build_collate('seg', _seg_test_pipeline(img_scale=(64, 64), img_ratios=[1.0, 1.5]), 'cpu')
    samples = [dict(img=np.zeros((64, 64, 3), np.uint8)), dict(img=np.zeros((64, 48, 3), np.uint8))]
    with pytest.raises(ValueError, match='shape'):
        c(samples)
