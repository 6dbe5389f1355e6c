"""The host half of the multi-scale AutoAugment det pipeline (rscotr_amd/pipeline/autoaug.py, DeviceCollate's plan) against the
sequential NumPy restatement tests/det_aug_oracle.py on the same seeded stream: draws, sizes, windows, metas and boxes exact.
Everything in front of a launch is host code, so with `lib.call` stubbed a CPU device runs it; the tables a launch was handed are
then replayed in NumPy (the kernels' integer arithmetic, restated) and must give the helper's uint8 images."""
import ctypes
import json
import os
import random

import numpy as np
import pytest

import det_aug_oracle as DO
from rscotr_amd import pipeline as P

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'reference_det_pipeline.json')
S0 = [(48, 133), (64, 133), (80, 133)]
POLICIES = [[dict(type='Resize', img_scale=S0, multiscale_mode='value', keep_ratio=True)],
            [dict(type='Resize', img_scale=[(40, 420), (50, 420), (60, 420)], multiscale_mode='value', keep_ratio=True),
             dict(type='RandomCrop', crop_type='absolute_range', crop_size=(38, 60), allow_negative_crop=True),
             dict(type='Resize', img_scale=S0, multiscale_mode='value', override=True, keep_ratio=True)]]
SHAPES = [(70, 100), (97, 61), (40, 131), (64, 64)]
SEEDS = range(48)


def pipeline(policies=POLICIES, flip=0.5):
    return [dict(type='LoadImageFromFile'), dict(type='LoadAnnotations', with_bbox=True),
            dict(type='RandomFlip', flip_ratio=flip), dict(type='AutoAugment', policies=policies),
            dict(type='Normalize', **P.IMG_NORM), dict(type='Pad', size_divisor=1), dict(type='DefaultFormatBundle'),
            dict(type='Collect', keys=['img', 'gt_bboxes', 'gt_labels'])]


def samples(seed, shapes=SHAPES):
    """Small ragged sources; boxes of every size, some of them small enough to fall outside a crop."""
    r = np.random.RandomState(1000 + seed)
    out = []
    for h, w in shapes[:3 + seed % 2]:
        n = int(r.randint(1, 5))
        x0, y0 = r.uniform(0, w * 0.8, n), r.uniform(0, h * 0.8, n)
        bb = np.stack([x0, y0, x0 + r.uniform(2, w / 2, n), y0 + r.uniform(2, h / 2, n)], -1).astype(np.float32)
        out.append(dict(img=r.randint(0, 256, (h, w, 3)).astype(np.uint8), gt_bboxes=bb, gt_labels=r.randint(0, 20, n)))
    return out


def _tuples(o):
    """JSON has no tuples: a list of numbers is one again (a scale, a crop size, a mean)."""
    if isinstance(o, dict):
        return {k: _tuples(v) for k, v in o.items()}
    if isinstance(o, list):
        if o and all(isinstance(v, (int, float)) and not isinstance(v, bool) for v in o):
            return tuple(o)
        return [_tuples(v) for v in o]
    return o


def plan(col, s, rng):
    p = col._plan(s, rng, random)
    col._targets(s, p)
    return p


# ---- the reference's recipe -------------------------------------------------------------------------------------------------
def test_reference_dino_pipelines_build():
    with open(GOLDEN) as fh:
        ref = _tuples(json.load(fh))
    c = P.build_collate('det', ref['train'], 'cpu')
    assert c.skipped == [] and c.flip_prob == 0.5 and c.size_divisor == 1 and c.resize is None and c.augmented
    pol = c.auto_augment['policies']
    assert [[t['type'] for t in p] for p in pol] == [['Resize'], ['Resize', 'RandomCrop', 'Resize']]
    assert len(pol[0][0]['img_scale']) == 11 and pol[0][0]['img_scale'][0] == (480, 1333) and pol[0][0]['multiscale_mode'] == 'value'
    assert pol[1][0]['img_scale'] == [(400, 4200), (500, 4200), (600, 4200)] and pol[1][2]['img_scale'] == pol[0][0]['img_scale']
    assert pol[1][1] == dict(type='RandomCrop', crop_type='absolute_range', crop_size=(384, 600))
    t = P.build_collate('det', ref['test'], 'cpu')
    e = P.eval_collate_for('det', 'cpu')
    assert t.skipped == [] and t.resize == e.resize and t.size_divisor == 1 and t.flip_prob == 0.0 and t.auto_augment is None
    # one full-size plan: a 70 x 100 source lands on one of the 11 scales, its long edge within 1333
    s = samples(0)[:1]
    p = plan(c, s, np.random.RandomState(0))
    h, w = p.batch['img_metas'][0]['img_shape'][:2]
    assert min(h, w) in range(480, 801, 32) and max(h, w) <= 1333


# ---- the plan against the helper -----------------------------------------------------------------------------------------
def test_plan_equals_the_helper_over_seeds():
    col = P.build_collate('det', pipeline(), 'cpu')
    assert col.skipped == []
    seen = dict(policy=set(), flip=set(), dropped=0, clipped=0, empty=0, ragged=0, stages=set())
    for seed in SEEDS:
        s = samples(seed)
        ra, rb = np.random.RandomState(seed), np.random.RandomState(seed)
        p = plan(col, s, ra)
        ims, boxes, labels, infos, (Hout, Wout) = DO.det_autoaug_batch(s, rb, POLICIES)
        assert ra.rand() == rb.rand(), 'the plan and the helper consume the same number of draws'
        assert (p.Hout, p.Wout) == (Hout, Wout)
        b = p.batch
        assert len(b['gt_bboxes']) == len(b['gt_labels']) == len(s)
        for k, (x, d, m, im, bb, ll, info) in enumerate(zip(s, p.ds, b['img_metas'], ims, boxes, labels, infos)):
            assert (d['flip'], d['policy']) == (info['flip'], info['policy']) and d['flip_first']
            assert m['flip'] == info['flip'] and m['flip_direction'] == ('horizontal' if info['flip'] else None)
            assert m['ori_shape'] == x['img'].shape and tuple(m['img_shape']) == info['img_shape'] == im.shape
            assert m['pad_shape'] == (Hout, Wout, 3) and m['keep_ratio'] is True and info['keep_ratio'] is True
            assert m['scale_factor'].dtype == np.float32 and np.array_equal(m['scale_factor'], info['scale_factor'])
            # frames and windows of the walk
            assert d['rsz'] == info['sizes'][0] and d['src'] == (0, 0, x['img'].shape[1], x['img'].shape[0])
            if info['policy'] == 0:
                assert d['chain'] is None and d['win'] == (0, 0, *info['sizes'][0])
            else:
                assert d['chain'] == dict(win1=info['windows'][0], rsz2=info['sizes'][1]) and d['win'] == (0, 0, *info['sizes'][1])
            for got, host, want, dt, shape in ((b['gt_bboxes'][k], b['gt_bboxes_host'][k], bb, np.float32, (len(ll), 4)),
                                               (b['gt_labels'][k], b['gt_labels_host'][k], ll, np.int64, (len(ll),))):
                assert host.dtype == dt and host.shape == shape and np.array_equal(host, want)
                assert got.numpy().dtype == dt and np.array_equal(got.numpy(), want)
            seen['policy'].add(info['policy'])
            seen['flip'].add(info['flip'])
            seen['dropped'] += info['dropped']
            seen['clipped'] += info['clipped']
            seen['empty'] += len(ll) == 0
        seen['ragged'] += any(tuple(m['img_shape']) != m['pad_shape'] for m in b['img_metas'])
        seen['stages'].add(frozenset(d['chain'] is not None for d in p.ds))
    # what the seeds were chosen to reach (judged on the helper's own record)
    assert seen['policy'] == {0, 1} and seen['flip'] == {False, True}
    assert seen['dropped'] >= 1 and seen['clipped'] >= 1 and seen['empty'] >= 1 and seen['ragged'] >= 1
    assert frozenset([False, True]) in seen['stages'], 'a batch that mixes one-stage and two-stage samples'


# ---- the launches' tables, replayed ------------------------------------------------------------------------------------------
def _i(ptr, n, ctype, dtype):
    return np.ctypeslib.as_array((ctype * n).from_address(int(ptr))).astype(dtype).copy() if n else np.zeros(0, dtype)


def _rows(tab_p, off, count, k):
    return _i(tab_p + 4 * int(off), count * (k + 2), ctypes.c_int32, np.int64).reshape(count, k + 2)


def _resample(a, tx, ty, nearest):
    """The kernels' integer arithmetic over per-axis entries {first, taps, weights} (resample_u8, bilinear or nearest)."""
    if nearest:
        return a[ty[:, 0]][:, tx[:, 0]]
    p = a.astype(np.int64)
    hs = sum(np.where((tx[:, 1] > t)[None, :, None], tx[:, 2 + t][None, :, None] * p[:, np.minimum(tx[:, 0] + t, a.shape[1] - 1)], 0)
             for t in range(tx.shape[1] - 2))
    acc = sum(np.where((ty[:, 1] > t)[:, None, None], ty[:, 2 + t][:, None, None] * hs[np.minimum(ty[:, 0] + t, a.shape[0] - 1)], 0)
              for t in range(ty.shape[1] - 2))
    return np.clip((acc + (1 << 21)) >> 22, 0, 255).astype(np.uint8)


def _replay(col, s, rng):
    """`_run` on a CPU device with the library stubbed -> (batch, entry names, per sample the uint8 image the launch's rows and
    tables describe)."""
    from rscotr_amd import ops
    from rscotr_amd._lib import lib
    names, ims = [], []

    def call(name, *args):
        names.append(name)
        if name == 'rscotr_img_aug_chain_u8':
            src, meta_p, tab_p, _, B = args[:5]
        else:
            assert name == 'rscotr_img_aug_u8'
            src, meta_p, tab_p, _, _, B = args[:6]
        meta = _i(meta_p, B * P.AUG_META, ctypes.c_int64, np.int64).reshape(B, P.AUG_META)
        for m in meta:
            off, H, W, stride, cw, ch, flip, xt, yt, kx, ky, mode = (int(v) for v in m[:12])
            assert stride == W * 3 and flip == 0 and not m[16:].any()
            a = _i(src + off, H * stride, ctypes.c_uint8, np.uint8).reshape(H, W, 3)
            f1 = _resample(a, _rows(tab_p, xt, cw, kx), _rows(tab_p, yt, ch, ky), mode == 0)
            if name == 'rscotr_img_aug_chain_u8':
                x2, y2, ow, oh = (int(v) for v in m[12:16])
                f1 = _resample(f1, _rows(tab_p, x2, ow, 2), _rows(tab_p, y2, oh, 2), False)
            else:
                assert not m[12:16].any()
            ims.append(f1)
        return 0
    stream = ops._stream
    try:
        lib.call, ops._stream = call, lambda: 0
        batch = col._run(s, rng, random)
    finally:
        del lib.call
        ops._stream = stream
    return batch, names, ims


def test_launch_tables_replayed_in_numpy_give_the_helper_images():
    """One launch per batch: the chain entry when a sample resizes twice, else the table route's; either way the rows and tables,
    replayed, are the helper's images bit for bit (the early flip is in the x entries: no row asks the kernel to flip)."""
    col = P.build_collate('det', pipeline(), 'cpu')
    entries = set()
    for seed in list(SEEDS)[:16]:
        s = samples(seed)
        batch, names, got = _replay(col, s, np.random.RandomState(seed))
        ims, _, _, infos, hw = DO.det_autoaug_batch(s, np.random.RandomState(seed), POLICIES)
        assert names == ['rscotr_img_aug_chain_u8' if any(i['policy'] == 1 for i in infos) else 'rscotr_img_aug_u8']
        entries.add(names[0])
        assert tuple(batch['img'].shape) == (len(s), 3, *hw)
        for g, im in zip(got, ims):
            assert g.shape == im.shape and np.array_equal(g, im)
    assert len(entries) == 2


# ---- hand-made sizes ---------------------------------------------------------------------------------------------------------
class Fixed:
    """A stream that hands out fixed values and records what was asked."""

    def __init__(self, seq):
        self.seq, self.asked = list(seq), []

    def randint(self, *a):
        self.asked.append(('randint',) + a)
        return self.seq.pop(0)

    def rand(self, *a):
        self.asked.append(('rand',) + a)
        return self.seq.pop(0)

    def random_sample(self):
        self.asked.append(('random_sample',))
        return self.seq.pop(0)


def test_multiscale_range_and_value_sizes():
    r = dict(img_scale=[(100, 50), (200, 80)], multiscale_mode='range')
    col = P.DeviceCollate('det', 'cpu', resize=r)
    f = Fixed([150, 60])
    assert col._resize_shape(40, 80, f) == (120, 60) and f.asked == [('randint', 100, 201), ('randint', 50, 81)]
    assert DO.resize_wh(dict(r, keep_ratio=True), 40, 80, Fixed([150, 60])) == (120, 60)
    f = Fixed([150, 60])
    assert P.DeviceCollate('det', 'cpu', resize=dict(r, keep_ratio=False))._resize_shape(40, 80, f) == (150, 60)
    r = dict(img_scale=[(100, 50), (200, 80), (64, 64)], multiscale_mode='value')
    f = Fixed([2])
    assert P.DeviceCollate('seg', 'cpu', resize=r)._resize_shape(40, 80, f) == (64, 32) and f.asked == [('randint', 3)]
    f = Fixed([])  # one scale: no draw, as today
    assert P.DeviceCollate('det', 'cpu', resize=dict(img_scale=(160, 96)))._resize_shape(70, 100, f) == (137, 96) and f.asked == []
    with pytest.raises(ValueError, match='range'):
        P.DeviceCollate('det', 'cpu', resize=dict(img_scale=[(1, 2), (3, 4), (5, 6)], multiscale_mode='range'))
    with pytest.raises(ValueError, match='multiscale_mode'):
        P.DeviceCollate('det', 'cpu', resize=dict(img_scale=[(1, 2), (3, 4)], multiscale_mode='linear'))
    with pytest.raises(ValueError, match='ratio_range'):
        P.DeviceCollate('det', 'cpu', resize=dict(img_scale=[(1, 2), (3, 4)], multiscale_mode='value', ratio_range=(0.5, 2.0)))


@pytest.mark.parametrize('crop, hw, seq, asked, win', [
    (dict(crop_type='absolute', crop_size=(30, 200)), (50, 80), [7, 0], [('randint', 0, 21), ('randint', 0, 1)], (0, 7, 80, 30)),
    (dict(crop_type='absolute_range', crop_size=(38, 60)), (50, 80), [50, 38, 0, 42],
     [('randint', 38, 51), ('randint', 38, 61), ('randint', 0, 1), ('randint', 0, 43)], (42, 0, 38, 50)),
    (dict(crop_type='relative', crop_size=(0.5, 0.25)), (51, 80), [25, 60], [('randint', 0, 26), ('randint', 0, 61)],
     (60, 25, 20, 26)),
    (dict(crop_type='relative_range', crop_size=(0.5, 0.5)), (50, 80), [np.array([0.5, 0.0]), 3, 4],
     [('rand', 2), ('randint', 0, 13), ('randint', 0, 41)], (4, 3, 40, 38)),
])
def test_crop_types_give_exact_sizes(crop, hw, seq, asked, win):
    t = dict(type='RandomCrop', allow_negative_crop=True, **crop)
    col = P.DeviceCollate('det', 'cpu', flip_prob=0.5, auto_augment=dict(policies=[[t]]))
    f = Fixed([0.9, 0] + seq)  # no flip, policy 0
    d = col.draw(hw + (3,), None, f)
    assert f.asked == [('rand',), ('randint', 0, 1)] + asked and not f.seq
    assert d['src'] == win and d['rsz'] == win[2:] and d['win'] == (0, 0, *win[2:]) and d['chain'] is None and not d['flip']
    assert d['scale_factor'] is None
    img = np.zeros(hw + (3,), np.uint8)
    boxes = np.array([[0, 0, hw[1], hw[0]]], np.float32)
    im, bb, _, (ox, oy, cw, ch), _, _ = DO.crop_step(t, img, boxes, np.zeros(1, np.int64), Fixed(seq))
    assert (ox, oy, cw, ch) == win and bb.tolist() == [[0, 0, cw, ch]]
    # the boxes of the same draw: shifted, clipped to the crop
    from rscotr_amd.pipeline import autoaug as A
    hb, hl = A.aa_boxes(boxes, [3], hw[1], False, d['steps'])
    assert hb.tolist() == [[0, 0, cw, ch]] and hl.tolist() == [3]


def test_crop_drops_a_box_outside_and_keeps_the_label_order():
    from rscotr_amd.pipeline import autoaug as A
    boxes = np.array([[0, 0, 5, 5], [10, 10, 30, 40], [25, 5, 90, 20], [20, 20, 20, 30]], np.float32)
    hb, hl = A.aa_boxes(boxes, [1, 2, 3, 4], 100, False, [('crop', (10, 8, 30, 20))])
    assert hb.tolist() == [[0, 2, 20, 20], [15, 0, 30, 12]] and hl.tolist() == [2, 3]
    hb, hl = A.aa_boxes(boxes[:1], [1], 100, False, [('crop', (10, 8, 30, 20))])
    assert hb.shape == (0, 4) and hb.dtype == np.float32 and hl.shape == (0,) and hl.dtype == np.int64
    hb, _ = A.aa_boxes(boxes[:1], [1], 100, True, [])  # the flip is on the SOURCE width
    assert hb.tolist() == [[95, 0, 100, 5]]


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def _pol(*steps):
    return pipeline([list(steps)])


def test_refusals_name_what_they_refuse():
    r0 = dict(type='Resize', img_scale=S0, multiscale_mode='value', keep_ratio=True)
    crop = dict(type='RandomCrop', crop_type='absolute_range', crop_size=(38, 60), allow_negative_crop=True)
    with pytest.raises(NotImplementedError, match='allow_negative_crop'):
        P.build_collate('det', _pol(r0, dict(crop, allow_negative_crop=False), dict(r0, override=True)), 'cpu')
    with pytest.raises(NotImplementedError, match='allow_negative_crop'):  # mmdet's default is False
        P.build_collate('det', _pol(r0, {k: v for k, v in crop.items() if k != 'allow_negative_crop'}), 'cpu')
    with pytest.raises(ValueError, match='override'):
        P.build_collate('det', _pol(r0, crop, r0), 'cpu')
    with pytest.raises(NotImplementedError, match='pillow'):
        P.build_collate('det', _pol(dict(r0, backend='pillow', interpolation='bicubic')), 'cpu')
    with pytest.raises(NotImplementedError, match='Rotate'):
        P.build_collate('det', _pol(r0, dict(type='Rotate', level=3)), 'cpu')
    c = P.build_collate('det', _pol(r0, dict(type='Rotate', level=3)), 'cpu', unsupported='skip')
    assert c.skipped == ['Rotate'] and [t['type'] for t in c.auto_augment['policies'][0]] == ['Resize']
    for task in ('cls', 'seg'):
        with pytest.raises(NotImplementedError, match='AutoAugment'):
            P.build_collate(task, pipeline(), 'cpu')
        assert P.build_collate(task, pipeline(), 'cpu', unsupported='skip').skipped == ['AutoAugment']
    with pytest.raises(ValueError, match='det'):
        P.DeviceCollate('seg', 'cpu', auto_augment=dict(policies=POLICIES))
    for extra, name in ((dict(type='PhotoMetricDistortion'), 'PhotoMetricDistortion'), (dict(type='RandomErasing'), 'RandomErasing'),
                        (dict(type='RandomResizedCrop', size=64), 'RandomResizedCrop'),
                        (dict(type='Resize', img_scale=(64, 64)), 'Resize')):
        with pytest.raises(NotImplementedError, match=name + ' together with AutoAugment'):
            P.build_collate('det', pipeline()[:4] + [extra] + pipeline()[4:], 'cpu')
    with pytest.raises(NotImplementedError, match='RandAugment'):
        P.build_collate('det', pipeline()[:4] + [dict(type='RandAugment', policies=[dict(type='Invert')], num_policies=1,
                                                      magnitude_level=3)] + pipeline()[4:], 'cpu')
    with pytest.raises(NotImplementedError, match='RandomFlip after AutoAugment'):
        P.build_collate('det', [pipeline()[3], pipeline()[2]], 'cpu')
    with pytest.raises(NotImplementedError, match='more than two'):
        P.build_collate('det', _pol(r0, dict(r0, override=True), dict(r0, override=True)), 'cpu')
    with pytest.raises(NotImplementedError, match='several img_scale'):
        P.build_collate('cls', [dict(type='Resize', img_scale=S0, multiscale_mode='value')], 'cpu')


# ---- a top-level multi-scale Resize --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode, scales', [('value', [(64, 48), (96, 64), (80, 80)]), ('range', [(64, 40), (128, 72)])])
def test_seg_top_level_multiscale_resize_draws_like_the_helper(mode, scales):
    t = dict(type='Resize', img_scale=scales, multiscale_mode=mode, keep_ratio=True)
    col = P.build_collate('seg', [dict(type='LoadAnnotations', reduce_zero_label=True), t, dict(type='RandomFlip', prob=0.5),
                                  dict(type='Normalize', **P.IMG_NORM)], 'cpu')
    assert col.skipped == [] and col.resize == dict(img_scale=scales, multiscale_mode=mode, ratio_range=None, keep_ratio=True)
    sizes = set()
    for seed in range(12):
        r = np.random.RandomState(seed)
        s = [dict(img=r.randint(0, 256, (h, w, 3)).astype(np.uint8), gt_semantic_seg=r.randint(0, 7, (h, w)).astype(np.uint8))
             for h, w in SHAPES[:3]]
        ra, rb = np.random.RandomState(seed), np.random.RandomState(seed)
        p = col._plan(s, ra, random)
        for x, d, m in zip(s, p.ds, p.batch['img_metas']):
            h, w = x['img'].shape[:2]
            nw, nh = DO.resize_wh(t, h, w, rb)
            flip = bool(rb.rand() < 0.5)
            assert d['rsz'] == (nw, nh) and d['flip'] == flip and m['img_shape'] == (nh, nw, 3) and m['keep_ratio']
            assert np.array_equal(m['scale_factor'], np.array([nw / w, nh / h, nw / w, nh / h], np.float32))
            sizes.add((nw, nh))
        assert ra.rand() == rb.rand()
    assert len(sizes) > 6


def test_det_top_level_multiscale_resize_scales_the_boxes():
    t = dict(type='Resize', img_scale=S0, multiscale_mode='value', keep_ratio=True)
    col = P.build_collate('det', [t, dict(type='RandomFlip', flip_ratio=0.0), dict(type='Pad', size_divisor=32)], 'cpu')
    s = samples(3)
    ra, rb = np.random.RandomState(5), np.random.RandomState(5)
    p = plan(col, s, ra)
    for x, m, hb in zip(s, p.batch['img_metas'], p.batch['gt_bboxes_host']):
        _, bb, sf = DO.resize_step(t, x['img'], np.asarray(x['gt_bboxes'], np.float32).copy(), rb)
        rb.rand()
        assert np.array_equal(m['scale_factor'], sf) and np.array_equal(hb, bb)
    assert p.Hout % 32 == 0 and p.Wout % 32 == 0


# ---- what builds today builds the same -----------------------------------------------------------------------------------------
def test_base_pipelines_build_the_same_collates():
    cfg = P.IMG_NORM
    det_train = [dict(type='LoadImageFromFile'), dict(type='LoadAnnotations', with_bbox=True),
                 dict(type='Resize', img_scale=(1333, 800), keep_ratio=True), dict(type='RandomFlip', flip_ratio=0.5),
                 dict(type='Normalize', **cfg), dict(type='Pad', size_divisor=32), dict(type='DefaultFormatBundle'),
                 dict(type='Collect', keys=['img', 'gt_bboxes', 'gt_labels'])]
    seg_train = [dict(type='LoadImageFromFile'), dict(type='LoadAnnotations', reduce_zero_label=True),
                 dict(type='Resize', img_scale=(512, 512), ratio_range=(0.5, 2.0)),
                 dict(type='RandomCrop', crop_size=(512, 512), cat_max_ratio=0.75), dict(type='RandomFlip', prob=0.5),
                 dict(type='PhotoMetricDistortion'), dict(type='Normalize', **cfg),
                 dict(type='Pad', size=(512, 512), pad_val=0, seg_pad_val=5), dict(type='DefaultFormatBundle'),
                 dict(type='Collect', keys=['img', 'gt_semantic_seg'])]
    keys = ('resize', 'crop_size', 'cat_max_ratio', 'reduce_zero_label', 'seg_pad_val', 'photometric', 'flip_prob', 'size_divisor',
            'rrc', 'erasing', 'rand_augment', 'auto_augment', 'resample', 'augmented', 'mean', 'std', 'to_rgb')
    for task, pl in (('det', det_train), ('seg', seg_train)):
        got, ref = P.build_collate(task, pl, 'cpu'), P.train_collate_for(task, 'cpu')
        for k in keys:
            assert getattr(got, k) == getattr(ref, k), (task, k)
        assert got.auto_augment is None
    # ... and draw the same: a single scale makes no draw in front of the flip
    d = P.build_collate('det', det_train, 'cpu').draw((70, 100, 3), None, Fixed([0.25]))
    assert d['rsz'] == (1143, 800) and d['flip'] and 'flip_first' not in d
