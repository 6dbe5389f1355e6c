"""The host half of the orientation stages of the device input collate (RandomFlip's directions, mmseg RandomRotate) against the
NumPy restatement tests/orient_oracle.py: the oracle's own identities, the config surface of `build_collate`, the draw stream,
the metas and the box flips.  Everything in front of a launch is host code: no GPU and no library."""
import random

import numpy as np
import pytest

import orient_oracle as OO
import randaug_oracle as RO
from rscotr_amd import pipeline as P
from rscotr_amd.pipeline import rotate as RT
from test_det_autoaug_cpu import POLICIES, samples
from test_det_autoaug_cpu import pipeline as det_aa_pipeline

ROT = dict(type='RandomRotate', prob=0.5, degree=30, pad_val=(10, 20, 30), seg_pad_val=7)


def seg_pipeline(flip=None, rotate=ROT, order=None):
    flip = dict(type='RandomFlip', prob=0.5, direction='vertical') if flip is None else flip
    steps = dict(load=[dict(type='LoadImageFromFile'), dict(type='LoadAnnotations', reduce_zero_label=True)],
                 resize=[dict(type='Resize', img_scale=(48, 36), ratio_range=(0.8, 1.5))],
                 crop=[dict(type='RandomCrop', crop_size=(32, 40), cat_max_ratio=0.75)], flip=[flip],
                 rotate=[rotate] if rotate else [], photo=[dict(type='PhotoMetricDistortion')],
                 norm=[dict(type='Normalize', **P.IMG_NORM)], pad=[dict(type='Pad', size=(32, 40), pad_val=0, seg_pad_val=5)],
                 tail=[dict(type='DefaultFormatBundle'), dict(type='Collect', keys=['img', 'gt_semantic_seg'])])
    order = order or ('load', 'resize', 'crop', 'flip', 'rotate', 'photo', 'norm', 'pad', 'tail')
    return [t for k in order for t in steps[k]]


def seg_samples(seed, shapes=((37, 53), (64, 48), (37, 53))):
    r = np.random.RandomState(seed)
    return [dict(img=r.randint(0, 256, (h, w, 3)).astype(np.uint8), gt_semantic_seg=r.randint(0, 7, (h, w)).astype(np.uint8))
            for h, w in shapes]


# ---- the oracle's own identities ------------------------------------------------------------------------------------------
def test_oracle_rotation_identities():
    r = np.random.RandomState(0)
    img = r.randint(0, 256, (32, 40, 3)).astype(np.uint8)
    sq = r.randint(0, 256, (24, 24, 3)).astype(np.uint8)
    pad = (10, 20, 30)
    assert np.array_equal(OO.rotate(img, 0, 'bilinear', pad), img)
    for deg in (180, -180):
        assert np.array_equal(OO.rotate(img, deg, 'bilinear', pad), img[::-1, ::-1])
    assert np.array_equal(OO.rotate(sq, 90, 'bilinear', pad), np.rot90(sq, -1))  # positive degrees turn clockwise
    const = np.empty((32, 40, 3), np.uint8)
    const[:] = pad
    for deg in (45, 17.3, -123.4):
        assert np.array_equal(OO.rotate(const, deg, 'bilinear', pad), const)
        assert np.array_equal(OO.rotate(img, deg, 'nearest', pad), RO.rotate(img, deg, 'nearest', pad))
    lab = r.randint(0, 7, (32, 40)).astype(np.uint8)
    got = OO.rotate(lab, -123.4, 'nearest', 255)
    assert np.array_equal(got, RO.rotate(np.repeat(lab[..., None], 3, 2), -123.4, 'nearest', (255,) * 3)[..., 0])
    assert 0.15 < (got == 255).mean() < 0.22  # about a fifth of a 32 x 40 window is fill at -123.4 degrees


def test_host_warp_tables_give_the_oracle_coordinates():
    """rotate.py's tables (the pipeline's own matrix and inverse), replayed as the kernels read them, land on the oracle's pixels."""
    r = np.random.RandomState(1)
    img = r.randint(0, 256, (32, 40, 3)).astype(np.uint8)
    for deg, center in ((17.3, None), (-123.4, None), (45, (3.5, 30.0))):
        cfg = RT.rotate_config(dict(prob=1, degree=30, pad_val=(10, 20, 30), seg_pad_val=7, center=center))
        rot, lrot, warp = RT.rotate_rows(cfg, [dict(win=(0, 0, 40, 32), rotate=deg)], labels=True)
        assert rot[0].tolist() == [4, 10, 20, 30] and lrot[0].tolist() == [4 + 144, 7, 0, 0] and warp.size == 4 + 2 * 144
        out = np.zeros_like(img)
        for name, off in (('bilinear', rot[0, 0]), ('nearest', lrot[0, 0])):
            t = warp[off:off + 144].astype(np.int64)
            X = t[80:112, None] + t[None, 0:40]
            Y = t[112:144, None] + t[None, 40:80]
            p = np.pad(img.astype(np.int64), ((64, 64), (64, 64), (0, 0)))
            p[:64], p[-64:], p[:, :64], p[:, -64:] = (10, 20, 30), (10, 20, 30), (10, 20, 30), (10, 20, 30)
            if name == 'nearest':
                out = p[np.clip(Y >> 10, -64, 95) + 64, np.clip(X >> 10, -64, 103) + 64]
            else:
                X, Y = X >> 5, Y >> 5
                sx, sy, ax, ay = np.clip(X >> 5, -64, 102), np.clip(Y >> 5, -64, 94), (X & 31)[..., None], (Y & 31)[..., None]
                acc = ((32 - ay) * (32 - ax) * p[sy + 64, sx + 64] + (32 - ay) * ax * p[sy + 64, sx + 65]
                       + ay * (32 - ax) * p[sy + 65, sx + 64] + ay * ax * p[sy + 65, sx + 65]) * 32
                out = (acc + (1 << 14)) >> 15
            assert np.array_equal(out, OO.rotate(img, deg, name, (10, 20, 30), center)), (deg, name)


# ---- build_collate ----------------------------------------------------------------------------------------------------------
def test_build_collate_takes_directions_and_random_rotate():
    c = P.build_collate('seg', seg_pipeline(), 'cpu')
    assert c.skipped == [] and c.flip_direction == 'vertical' and c.flip_prob == 0.5 and c.augmented
    assert c.rotate == dict(prob=0.5, degree=(-30.0, 30.0), pad_val=(10, 20, 30), seg_pad_val=7, center=None)
    assert c.photometric is not None and c.crop_size == (32, 40) and c.seg_pad_val == 5
    c = P.build_collate('seg', seg_pipeline(rotate=dict(type='RandomRotate', prob=1, degree=(-10, 40), center=(3, 4))), 'cpu')
    assert c.rotate == dict(prob=1.0, degree=(-10.0, 40.0), pad_val=(0, 0, 0), seg_pad_val=255, center=(3.0, 4.0))
    c = P.build_collate('cls', [dict(type='RandomFlip', flip_prob=0.3, direction='vertical')], 'cpu')
    assert c.flip_direction == 'vertical' and c.flip_prob == 0.3
    dirs = ['horizontal', 'vertical', 'diagonal']
    c = P.build_collate('det', [dict(type='RandomFlip', flip_ratio=[0.3, 0.2, 0.1], direction=dirs)], 'cpu')
    assert c.flip_direction == dirs and c.flip_prob == [0.3, 0.2, 0.1]
    c = P.build_collate('det', det_aa_pipeline() + [], 'cpu')
    assert c.flip_direction == 'horizontal' and c.rotate is None
    assert P.build_collate('det', [dict(type='RandomFlip', flip_ratio=0.5, direction='diagonal')], 'cpu').flip_direction == 'diagonal'
    assert P.train_collate_for('seg', 'cpu').flip_direction == 'horizontal' and P.train_collate_for('seg', 'cpu').rotate is None


def test_build_collate_refusals():
    with pytest.raises(NotImplementedError, match='auto_bound'):
        P.build_collate('seg', seg_pipeline(rotate=dict(ROT, auto_bound=True)), 'cpu')
    with pytest.raises(NotImplementedError, match='auto_bound'):
        P.DeviceCollate('seg', 'cpu', rotate=dict(prob=0.5, degree=10, auto_bound=True))
    for order, word in ((('load', 'resize', 'crop', 'flip', 'photo', 'rotate', 'norm', 'pad', 'tail'), 'PhotoMetricDistortion'),
                        (('load', 'resize', 'rotate', 'crop', 'flip', 'photo', 'norm', 'pad', 'tail'), 'RandomCrop'),
                        (('load', 'rotate', 'resize', 'crop', 'flip', 'photo', 'norm', 'pad', 'tail'), 'Resize'),
                        (('load', 'resize', 'crop', 'rotate', 'flip', 'photo', 'norm', 'pad', 'tail'), 'RandomFlip'),
                        (('load', 'resize', 'crop', 'flip', 'photo', 'norm', 'pad', 'rotate', 'tail'), 'PhotoMetricDistortion')):
        with pytest.raises(NotImplementedError, match=f'{word}.*after Resize / RandomCrop / RandomFlip and before'):
            P.build_collate('seg', seg_pipeline(order=order), 'cpu')
    for task in ('det', 'cls'):
        with pytest.raises(ValueError, match='seg'):
            P.build_collate(task, [dict(type='RandomFlip', prob=0.5), ROT], 'cpu')
        with pytest.raises(ValueError, match='seg'):
            P.DeviceCollate(task, 'cpu', rotate=dict(prob=0.5, degree=10))
    for task, direction in (('seg', 'diagonal'), ('cls', 'diagonal'), ('seg', 'sideways'), ('det', 'sideways'),
                            ('det', ['horizontal', 'up']), ('seg', ['horizontal', 'vertical']), ('cls', ['horizontal'])):
        with pytest.raises(ValueError, match='direction'):
            P.build_collate(task, [dict(type='RandomFlip', prob=0.5, direction=direction)], 'cpu')
    with pytest.raises(ValueError, match='at most 1'):
        P.DeviceCollate('det', 'cpu', flip_direction=['horizontal', 'vertical'], flip_prob=[0.7, 0.4])
    with pytest.raises(ValueError):
        P.DeviceCollate('det', 'cpu', flip_direction=['horizontal', 'vertical'], flip_prob=[0.5])
    with pytest.raises(ValueError):
        P.DeviceCollate('det', 'cpu', flip_direction='horizontal', flip_prob=[0.5])


# ---- the draw stream, the metas ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rotate', [None, dict(prob=0.5, degree=30), dict(prob=0.5, degree=(-100, 20), center=(5, 6))])
@pytest.mark.parametrize('direction', ['horizontal', 'vertical'])
def test_seg_draw_stream_and_metas(direction, rotate):
    """A seeded plan makes the oracle's decisions, and the generator stands where the oracle's does after every batch."""
    col = P.DeviceCollate('seg', 'cpu', flip_prob=0.5, flip_direction=direction, crop_size=(32, 40), cat_max_ratio=0.75,
                          reduce_zero_label=True, resize=dict(img_scale=(48, 36), ratio_range=(0.8, 1.5)), photometric=True,
                          rotate=rotate)
    seen = set()
    for seed in range(6):
        s = seg_samples(seed)
        ra, rb = np.random.RandomState(seed), np.random.RandomState(seed)
        p = col._plan(s, ra, random)
        for x, d, m in zip(s, p.ds, p.batch['img_metas']):
            im, lb, info = OO.seg_sample_oriented(x['img'], x['gt_semantic_seg'], rb, img_scale=(48, 36), ratio_range=(0.8, 1.5),
                                                  crop=(32, 40), cat_max_ratio=0.75, direction=direction, rotate_cfg=rotate,
                                                  photo=True)
            assert m['flip'] == info['flip'] and m['flip_direction'] == info['flip_direction'] == d['flip_direction']
            assert tuple(m['img_shape']) == im.shape
            assert ('rotate_degree' in m) == (rotate is not None)
            if rotate is not None:
                assert m['rotate_degree'] == info['rotate_degree'] == d['rotate']
                assert m['rotate_degree'] is None or min(*col.rotate['degree']) <= m['rotate_degree'] <= max(*col.rotate['degree'])
            seen.add((info['flip_direction'], info.get('rotate_degree') is not None))
        assert ra.rand() == rb.rand()
    assert seen == {(f, r) for f in (None, direction) for r in ((False, True) if rotate else (False,))}


def test_one_direction_keeps_the_parent_stream():
    """flip_direction='horizontal' (the default) draws rand() < flip_prob: the flips of a seeded batch are the ones the collate
    made before it knew directions, for every task."""
    for task, kw in (('cls', {}), ('det', dict(size_divisor=32)), ('seg', dict(crop_size=(32, 40)))):
        col = P.DeviceCollate(task, 'cpu', flip_prob=0.5, **kw)
        s = seg_samples(3)
        ra, rb = np.random.RandomState(5), np.random.RandomState(5)
        p = col._plan(s, ra, random)
        for x, d, m in zip(s, p.ds, p.batch['img_metas']):
            if task == 'seg':  # RandomCrop's offsets
                rb.randint(0, max(x['img'].shape[0] - 32, 0) + 1), rb.randint(0, max(x['img'].shape[1] - 40, 0) + 1)
            fl = bool(rb.rand() < 0.5)
            assert d['flip'] is fl and m['flip'] is fl and m['flip_direction'] == ('horizontal' if fl else None)
        assert ra.rand() == rb.rand()


@pytest.mark.parametrize('ratio', [0.6, [0.3, 0.2, 0.25]])
def test_det_direction_list_draw(ratio):
    dirs = ['horizontal', 'vertical', 'diagonal']
    col = P.DeviceCollate('det', 'cpu', flip_prob=ratio, flip_direction=dirs, size_divisor=32)
    ra, rb = np.random.RandomState(2), np.random.RandomState(2)
    got, want = [], []
    for _ in range(64):
        d = col.draw((37, 53, 3), None, ra)
        assert d['flip'] == (d['flip_direction'] is not None)
        got.append(d['flip_direction'])
        want.append(rb.choice(dirs + [None], p=(ratio if isinstance(ratio, list) else [ratio / 3] * 3)
                              + [1 - (sum(ratio) if isinstance(ratio, list) else ratio)]))  # mmdet's own call
    assert got == want and set(got) == set(dirs) | {None} and ra.rand() == rb.rand()
    ra, rb = np.random.RandomState(2), np.random.RandomState(2)
    assert [col.draw((37, 53, 3), None, ra)['flip_direction'] for _ in range(64)] == [OO.flip_draw(rb, dirs, ratio) for _ in range(64)]


# ---- boxes ---------------------------------------------------------------------------------------------------------------------
def _plan(col, s, rng):
    p = col._plan(s, rng, random)
    col._targets(s, p)
    return p


@pytest.mark.parametrize('direction', ['horizontal', 'vertical', 'diagonal'])
def test_box_flips_match_bbox_flip(direction):
    r = np.random.RandomState(4)
    s = []
    for h, w in ((37, 53), (64, 48), (37, 53)):
        x1, y1 = r.uniform(0, w / 2, 4), r.uniform(0, h / 2, 4)
        bb = np.stack([x1, y1, x1 + r.uniform(2, w / 2, 4), y1 + r.uniform(2, h / 2, 4)], -1).astype(np.float32)
        s.append(dict(img=r.randint(0, 256, (h, w, 3)).astype(np.uint8), gt_bboxes=bb, gt_labels=r.randint(0, 20, 4)))
    for scale in (None, (80, 48)):  # the plain route's plan and the table route's (keep-ratio Resize in front of the flip)
        col = P.DeviceCollate('det', 'cpu', flip_prob=0.7, flip_direction=direction, size_divisor=32,
                              resize=None if scale is None else dict(img_scale=scale))
        flips = set()
        for seed in range(4):
            ra, rb = np.random.RandomState(seed), np.random.RandomState(seed)
            p = _plan(col, s, ra)
            for x, m, gb in zip(s, p.batch['img_metas'], p.batch['gt_bboxes_host']):
                im, bb, info = OO.det_sample_oriented(x['img'], x['gt_bboxes'], rb, scale, 0.7, direction)
                assert m['flip_direction'] == info['flip_direction'] and tuple(m['img_shape']) == im.shape
                assert gb.dtype == np.float32 and np.array_equal(gb, bb)
                flips.add(info['flip'])
        assert flips == {True, False}
    # the AutoAugment route: the flip stands in front of the geometry, the boxes flip on the SOURCE size (aa_boxes)
    col = P.build_collate('det', [dict(t, direction=direction) if t['type'] == 'RandomFlip' else t for t in det_aa_pipeline()],
                          'cpu')
    assert col.flip_direction == direction and col.auto_augment is not None
    flips = set()
    for seed in range(6):
        s = samples(seed)
        ra, rb = np.random.RandomState(seed), np.random.RandomState(seed)
        p = _plan(col, s, ra)
        for x, m, gb, gl in zip(s, p.batch['img_metas'], p.batch['gt_bboxes_host'], p.batch['gt_labels_host']):
            im, bb, ll, info = OO.det_autoaug_sample_oriented(x['img'], x['gt_bboxes'], x['gt_labels'], rb, POLICIES, 0.5, direction)
            assert m['flip_direction'] == info['flip_direction'] and tuple(m['img_shape']) == im.shape
            assert np.array_equal(gb, bb) and np.array_equal(gl, ll)
            flips.add((info['flip'], info['policy']))
    assert flips == {(f, k) for f in (True, False) for k in (0, 1)}
    b = np.array([[2, 3, 10, 20]], np.float32)
    want = dict(horizontal=[43, 3, 51, 20], vertical=[2, 17, 10, 34], diagonal=[43, 17, 51, 34])[direction]
    assert OO.bbox_flip(b, (37, 53, 3), direction).tolist() == [want]
