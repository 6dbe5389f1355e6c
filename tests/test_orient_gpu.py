"""Orientation stages of the device input collate against the NumPy restatement tests/orient_oracle.py on the same seeded draws:
RandomFlip's directions (the flip bit set of rscotr_img_prep_u8, rscotr_seg_label_prep_u8, rscotr_img_aug_u8,
rscotr_seg_label_aug_u8, rscotr_img_frames_u8, and the mirrored entries of rscotr_img_aug_chain_u8) on every route and task, and
mmseg RandomRotate (rscotr_img_aug_rot_u8, rscotr_seg_label_rot_u8).  Images within 1e-6 * max|ref| (one LSB of the uint8 stage
is ~0.017 after Normalize, so the uint8 values must be exact), label maps, metas and boxes exact."""
import os
import random

import numpy as np
import pytest
import torch

import aug_oracle as AO
import det_aug_oracle as DO
import orient_oracle as OO
import randaug_oracle as RO
from oracle import pipeline as OP
from rscotr_amd import pipeline as P
from test_det_autoaug_cpu import POLICIES

pytestmark = pytest.mark.gpu
MEAN, STD = P.IMG_NORM['mean'], P.IMG_NORM['std']
SHAPES = ((37, 53), (64, 48), (37, 53))
DIRECTIONS = [None, 'horizontal', 'vertical', 'diagonal']
PAD = (10, 20, 30)


def _close(got, ref):
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.abs(got - ref).max() <= 1e-6 * max(np.abs(ref).max(), 1.0)


def _samples(seed, shapes=SHAPES):
    r = np.random.RandomState(seed)
    out = []
    for h, w in shapes:
        x1, y1 = r.uniform(0, w / 2, 4), r.uniform(0, h / 2, 4)
        bb = np.stack([x1, y1, x1 + r.uniform(2, w / 2, 4), y1 + r.uniform(2, h / 2, 4)], -1).astype(np.float32)
        out.append(dict(img=r.randint(0, 256, (h, w, 3)).astype(np.uint8), gt_semantic_seg=r.randint(0, 7, (h, w)).astype(np.uint8),
                        gt_label=int(r.randint(0, 45)), gt_bboxes=bb, gt_labels=r.randint(0, 20, 4)))
    return out


def _forced(direction):
    """RandomFlip forced: the direction always, or never a flip."""
    return dict(flip_prob=0.0 if direction is None else 1.0, flip_direction=direction or 'horizontal')


def _labels(labs, hw, pad):
    return np.stack([OP.impad(lb, hw, pad)[None] for lb in labs])


def _check_metas(batch, direction):
    for m in batch['img_metas']:
        assert m['flip'] == (direction is not None) and m['flip_direction'] == direction


# ---- flips: every route, every task -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('direction', DIRECTIONS)
def test_flip_plain_route(cuda, direction):
    """rscotr_img_prep_u8 / rscotr_seg_label_prep_u8: cls and det on ragged sources padded to the largest, seg cropped to 32 x 40."""
    s = _samples(0)
    f = _forced(direction)
    if direction != 'diagonal':  # (mmcls and mmseg know horizontal and vertical)
        b = P.DeviceCollate('cls', cuda, **f)(s, np.random.RandomState(1))
        _check_metas(b, direction)
        _close(b['img'], AO.collate_images([OO.imflip(x['img'], direction) for x in s], (64, 53), MEAN, STD))
        if direction == 'horizontal':
            _close(b['img'], OP.prepare_batch([x['img'] for x in s], [(0, 0, w, h) for h, w in SHAPES], [True] * 3, (64, 53), MEAN, STD))
        kw = dict(crop_size=(32, 40), reduce_zero_label=True, seg_pad_val=5)
        b = P.DeviceCollate('seg', cuda, **kw, **f)(s, np.random.RandomState(2))
        _check_metas(b, direction)
        r = np.random.RandomState(2)
        ref = [OO.seg_sample_oriented(x['img'], x['gt_semantic_seg'], r, crop=(32, 40), flip_prob=f['flip_prob'],
                                      direction=f['flip_direction']) for x in s]
        _close(b['img'], AO.collate_images([im for im, _, _ in ref], (32, 40), MEAN, STD))
        assert np.array_equal(b['gt_semantic_seg'].cpu().numpy(), _labels([lb for _, lb, _ in ref], (32, 40), 5))
    else:
        for task in ('cls', 'seg'):
            with pytest.raises(ValueError, match='direction'):
                P.DeviceCollate(task, cuda, **f)
    b = P.DeviceCollate('det', cuda, size_divisor=32, **f)(s, np.random.RandomState(3))
    _check_metas(b, direction)
    r = np.random.RandomState(3)
    ref = [OO.det_sample_oriented(x['img'], x['gt_bboxes'], r, None, f['flip_prob'], f['flip_direction']) for x in s]
    _close(b['img'], AO.collate_images([im for im, _, _ in ref], (64, 64), MEAN, STD))
    for gb, (_, bb, _) in zip(b['gt_bboxes_host'], ref):
        assert np.array_equal(gb, bb)
    if direction == 'horizontal':
        for gb, x in zip(b['gt_bboxes'], s):
            assert np.array_equal(gb.cpu().numpy(), OP.bbox_flip(x['gt_bboxes'], np.float32(x['img'].shape[1])))


@pytest.mark.parametrize('direction', DIRECTIONS)
def test_flip_table_route(cuda, direction):
    """rscotr_img_aug_u8 / rscotr_seg_label_aug_u8: seg Resize + RandomCrop(32 x 40) (the 64 x 48 source lands 36 wide: padded),
    det keep-ratio Resize with boxes."""
    s = _samples(4)
    f = _forced(direction)
    if direction != 'diagonal':
        kw = dict(crop_size=(32, 40), cat_max_ratio=0.75, reduce_zero_label=True, seg_pad_val=5,
                  resize=dict(img_scale=(48, 36), ratio_range=(1.0, 1.0)))
        b = P.DeviceCollate('seg', cuda, **kw, **f)(s, np.random.RandomState(5))
        _check_metas(b, direction)
        assert [m['img_shape'] for m in b['img_metas']] == [(32, 40, 3), (32, 36, 3), (32, 40, 3)]
        r = np.random.RandomState(5)
        ref = [OO.seg_sample_oriented(x['img'], x['gt_semantic_seg'], r, img_scale=(48, 36), ratio_range=(1.0, 1.0), crop=(32, 40),
                                      cat_max_ratio=0.75, flip_prob=f['flip_prob'], direction=f['flip_direction']) for x in s]
        _close(b['img'], AO.collate_images([im for im, _, _ in ref], (32, 40), MEAN, STD))
        assert np.array_equal(b['gt_semantic_seg'].cpu().numpy(), _labels([lb for _, lb, _ in ref], (32, 40), 5))
        if direction == 'horizontal':  # what the same seed gave before the collate knew directions
            r = np.random.RandomState(5)
            old = [AO.seg_sample(x['img'], x['gt_semantic_seg'], r, img_scale=(48, 36), ratio_range=(1.0, 1.0), crop=(32, 40),
                                 flip_prob=1.0, photo=False) for x in s]
            assert all(o[2]['flip'] for o in old)
            _close(b['img'], AO.collate_images([o[0] for o in old], (32, 40), MEAN, STD))
            lref = OP.prepare_seg_labels([o[1] for o in old], [(0, 0, o[1].shape[1], o[1].shape[0]) for o in old], [False] * 3,
                                         (32, 40), True, 5)
            assert np.array_equal(b['gt_semantic_seg'].cpu().numpy(), lref)
    b = P.DeviceCollate('det', cuda, size_divisor=32, resize=dict(img_scale=(80, 48)), **f)(s, np.random.RandomState(6))
    _check_metas(b, direction)
    r = np.random.RandomState(6)
    ref = [OO.det_sample_oriented(x['img'], x['gt_bboxes'], r, (80, 48), f['flip_prob'], f['flip_direction']) for x in s]
    H, W = b['img'].shape[-2:]
    assert (H, W) == (64, 96) and [tuple(m['img_shape']) for m in b['img_metas']] == [im.shape for im, _, _ in ref]
    _close(b['img'], AO.collate_images([im for im, _, _ in ref], (H, W), MEAN, STD))
    for gb, (_, bb, _) in zip(b['gt_bboxes_host'], ref):
        assert np.array_equal(gb, bb)
    if direction == 'horizontal':
        r = np.random.RandomState(6)
        old = [AO.det_sample(x['img'], x['gt_bboxes'], r, img_scale=(80, 48), flip_prob=1.0) for x in s]
        _close(b['img'], AO.collate_images([o[0] for o in old], (H, W), MEAN, STD))
        for gb, o in zip(b['gt_bboxes_host'], old):
            assert np.array_equal(gb, o[1])


@pytest.mark.parametrize('direction', DIRECTIONS[:3])
def test_flip_randaugment_frames_route(cuda, direction):
    """rscotr_img_frames_u8 writes the flipped frame RandAugment works on (cls: RandomResizedCrop(48) -> flip -> RandAugment)."""
    s = _samples(7)
    f = _forced(direction)
    col = P.train_collate_for('cls', cuda, rand_augment=True, random_erasing=None, random_resized_crop=dict(size=48), **f)
    b = col(s, np.random.RandomState(8), random.Random(9))
    _check_metas(b, direction)
    r, py = np.random.RandomState(8), random.Random(9)
    ref = [OO.cls_randaug_sample_oriented(x['img'], r, py, P.RAND_AUGMENT, 48, f['flip_prob'], f['flip_direction'])[0] for x in s]
    _close(b['img'], AO.collate_images(ref, (48, 48), MEAN, STD))
    if direction == 'horizontal':
        r, py = np.random.RandomState(8), random.Random(9)
        old = [RO.cls_sample(x['img'], r, py, P.RAND_AUGMENT, size=48, flip_prob=1.0)[0] for x in s]
        _close(b['img'], AO.collate_images(old, (48, 48), MEAN, STD))


@pytest.mark.parametrize('direction', DIRECTIONS)
def test_flip_chain_route(cuda, direction):
    """rscotr_img_aug_chain_u8 (det, a two-Resize policy): the flip stands in front of the geometry, mirrored into the x and
    the y entries."""
    s = _samples(10)
    f = _forced(direction)
    pol = [POLICIES[1]]
    col = P.DeviceCollate('det', cuda, size_divisor=1, auto_augment=dict(policies=pol), **f)
    b = col(s, np.random.RandomState(11))
    _check_metas(b, direction)
    r = np.random.RandomState(11)
    ref = [OO.det_autoaug_sample_oriented(x['img'], x['gt_bboxes'], x['gt_labels'], r, pol, f['flip_prob'], f['flip_direction'])
           for x in s]
    hw = (max(o[0].shape[0] for o in ref), max(o[0].shape[1] for o in ref))
    assert tuple(b['img'].shape) == (3, 3, *hw)
    _close(b['img'], AO.collate_images([o[0] for o in ref], hw, MEAN, STD))
    for gb, gl, o in zip(b['gt_bboxes_host'], b['gt_labels_host'], ref):
        assert np.array_equal(gb, o[1]) and np.array_equal(gl, o[2])
    if direction == 'horizontal':
        ims, boxes = DO.det_autoaug_batch(s, np.random.RandomState(11), pol, 1.0)[:2]
        _close(b['img'], AO.collate_images(ims, hw, MEAN, STD))
        for gb, bb in zip(b['gt_bboxes_host'], boxes):
            assert np.array_equal(gb, bb)


def test_det_direction_list_batches(cuda):
    """mmdet's list of directions: the drawn direction reaches the kernel's flip word and the boxes."""
    dirs = ['horizontal', 'vertical', 'diagonal']
    col = P.DeviceCollate('det', cuda, size_divisor=32, flip_prob=0.9, flip_direction=dirs, resize=dict(img_scale=(80, 48)))
    seen = set()
    for seed in range(3):
        s = _samples(seed)
        b = col(s, np.random.RandomState(seed))
        r = np.random.RandomState(seed)
        ref = [OO.det_sample_oriented(x['img'], x['gt_bboxes'], r, (80, 48), 0.9, dirs) for x in s]
        _close(b['img'], AO.collate_images([im for im, _, _ in ref], b['img'].shape[-2:], MEAN, STD))
        for m, gb, (_, bb, info) in zip(b['img_metas'], b['gt_bboxes_host'], ref):
            assert m['flip_direction'] == info['flip_direction'] and np.array_equal(gb, bb)
            seen.add(info['flip_direction'])
    assert set(dirs) <= seen


# ---- RandomRotate ------------------------------------------------------------------------------------------------------------
SEG = dict(crop_size=(32, 40), reduce_zero_label=True, seg_pad_val=5, resize=dict(img_scale=(96, 64)))


def _rotated(cuda, s, seed, rot, direction, flip_prob, photo, img_scale=(96, 64), crop=(32, 40)):
    """One seeded seg batch with RandomRotate `rot` on the device and from the oracle -> (batch, [(image, labels, info)])."""
    kw = dict(SEG, photometric=photo or None, rotate=rot, flip_prob=flip_prob, flip_direction=direction)
    if img_scale is None:
        kw.update(resize=None, crop_size=None)
    b = P.DeviceCollate('seg', cuda, **kw)(s, np.random.RandomState(seed))
    r = np.random.RandomState(seed)
    ref = [OO.seg_sample_oriented(x['img'], x['gt_semantic_seg'], r, img_scale=img_scale, crop=crop if img_scale else None,
                                  flip_prob=flip_prob, direction=direction, rotate_cfg=rot, photo=photo) for x in s]
    return b, ref


def _check_rotated(b, ref, hw, rot, need_fill):
    """Image against the oracle; labels exact, the fill of the rotation and the interior apart (the fill is seg_pad_val as
    given: with reduce_zero_label a reduction applied to it would show as seg_pad_val - 1)."""
    _close(b['img'], AO.collate_images([im for im, _, _ in ref], hw, MEAN, STD))
    got = b['gt_semantic_seg'].cpu().numpy()
    assert got.shape == (len(ref), 1, *hw)
    for g, m, (im, lb, info) in zip(got[:, 0], b['img_metas'], ref):
        assert m['rotate_degree'] == info['rotate_degree'] and m['flip_direction'] == info['flip_direction']
        h, w = lb.shape
        deg = info['rotate_degree']
        inside = np.ones((h, w), np.uint8)
        if deg is not None:
            inside = OO.rotate(inside, deg, 'nearest', 0, rot.get('center'))
        fill = inside == 0
        assert np.array_equal(g[:h, :w][fill], np.full(int(fill.sum()), rot.get('seg_pad_val', 255)))
        assert np.array_equal(g[:h, :w][~fill], lb[~fill]) and (~fill).any()
        assert (g[h:] == 5).all() and (g[:, w:] == 5).all()
        if need_fill:
            assert fill.any()


ROTATE_CASES = [  # degree, flip direction in front, photometric, seg_pad_val, center
    (0, None, False, 255, None), (90, 'horizontal', True, 7, None), (180, 'vertical', False, 7, None),
    (45, 'horizontal', True, 255, (5.0, 20.5)), (17.3, 'vertical', True, 7, None), (-123.4, None, False, 7, None),
    (-123.4, 'vertical', True, 255, None), (17.3, None, False, 255, (39.0, 0.0))]


@pytest.mark.parametrize('deg, direction, photo, seg_pad, center', ROTATE_CASES)
def test_rotate_fixed_degrees(cuda, deg, direction, photo, seg_pad, center):
    """32 x 40 windows cut from the resized 37 x 53 / 64 x 48 sources, every sample turned by `deg`."""
    rot = dict(prob=1.0, degree=(deg, deg), pad_val=PAD, seg_pad_val=seg_pad, center=center)
    b, ref = _rotated(cuda, _samples(20), 21, rot, direction or 'horizontal', 0.0 if direction is None else 1.0, photo)
    assert all(info['rotate_degree'] == deg and info['img_shape'] == (32, 40, 3) for _, _, info in ref)
    _check_rotated(b, ref, (32, 40), rot, need_fill=deg not in (0, 180))
    if deg == -123.4 and center is None:  # about a fifth of the window is fill
        assert 0.15 < (OO.rotate(np.ones((32, 40), np.uint8), deg, 'nearest', 0) == 0).mean() < 0.22


@pytest.mark.parametrize('deg', [0, 90, 180, -90])
def test_rotate_square_window_quarter_turns(cuda, deg):
    """A 24 x 24 source, no Resize and no crop (identity entries): quarter turns are exact permutations of the window."""
    s = _samples(22, ((24, 24), (24, 24)))
    rot = dict(prob=1.0, degree=(deg, deg), pad_val=PAD, seg_pad_val=7)
    b, ref = _rotated(cuda, s, 23, rot, 'vertical', 1.0, False, img_scale=None)
    _check_rotated(b, ref, (24, 24), rot, need_fill=False)
    turned = [np.rot90(x['img'][::-1], -deg // 90) for x in s]
    _close(b['img'], AO.collate_images(turned, (24, 24), MEAN, STD))


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_rotate_seeded_draws_mixed_batches(cuda, seed):
    """RandomRotate(prob=0.5, degree=30) behind RandomFlip(0.5) and in front of PhotoMetricDistortion: rotated and unrotated
    samples in the one launch, padded windows (the 64 x 48 source lands 36 wide)."""
    s = _samples(30 + seed, SHAPES + ((64, 48),))
    rot = dict(prob=0.5, degree=30, pad_val=PAD, seg_pad_val=7)
    kw = dict(crop_size=(32, 40), cat_max_ratio=0.75, reduce_zero_label=True, seg_pad_val=5, photometric=True, rotate=rot,
              flip_prob=0.5, flip_direction='vertical', resize=dict(img_scale=(48, 36), ratio_range=(0.8, 1.5)))
    b = P.DeviceCollate('seg', cuda, **kw)(s, np.random.RandomState(seed))
    r = np.random.RandomState(seed)
    ref = [OO.seg_sample_oriented(x['img'], x['gt_semantic_seg'], r, img_scale=(48, 36), ratio_range=(0.8, 1.5), crop=(32, 40),
                                  cat_max_ratio=0.75, flip_prob=0.5, direction='vertical', rotate_cfg=rot, photo=True) for x in s]
    _check_rotated(b, ref, (32, 40), rot, need_fill=False)


def test_rotate_seeds_mix_rotated_and_unrotated_samples():
    """What the seeds of the test above were chosen for (host draws only)."""
    rot = dict(prob=0.5, degree=30, pad_val=PAD, seg_pad_val=7)
    col = P.DeviceCollate('seg', 'cpu', crop_size=(32, 40), cat_max_ratio=0.75, reduce_zero_label=True, rotate=rot, photometric=True,
                          flip_prob=0.5, flip_direction='vertical', resize=dict(img_scale=(48, 36), ratio_range=(0.8, 1.5)))
    mixed = 0
    for seed in (0, 1, 2):
        p = col._plan(_samples(30 + seed, SHAPES + ((64, 48),)), np.random.RandomState(seed), random)
        mixed += len({d['rotate'] is None for d in p.ds}) == 2
    assert mixed


# ---- bit-equalities on the device -----------------------------------------------------------------------------------------------
def _equal_bits(a, b):
    assert torch.equal(a['img'].view(torch.int32), b['img'].view(torch.int32))
    assert torch.equal(a['gt_semantic_seg'], b['gt_semantic_seg'])


def test_unrotated_samples_equal_the_table_route_bitwise(cuda, monkeypatch):
    """Every launch of rscotr_img_aug_u8 / rscotr_seg_label_aug_u8 of a seeded training batch is repeated through the rotating
    entries with all-zero rot rows (no sample rotated: prob = 0): the same words."""
    from rscotr_amd._lib import lib
    real, got = lib.call, {}

    def call(name, *a):
        real(name, *a)
        if name == 'rscotr_img_aug_u8':
            src, meta, tab, prm, out, B, H, W = a[:8]
            zero, o = torch.zeros((B, 4), dtype=torch.int32, device=cuda), torch.full((B, 3, H, W), 7.0, device=cuda)
            real('rscotr_img_aug_rot_u8', src, meta, tab, prm, zero.data_ptr(), zero.data_ptr(), o.data_ptr(), *a[5:])
            got['img'] = o
        elif name == 'rscotr_seg_label_aug_u8':
            src, meta, tab, out, B, H, W = a[:7]
            zero, o = torch.zeros((B, 4), dtype=torch.int32, device=cuda), torch.full((B, 1, H, W), -3, device=cuda)
            real('rscotr_seg_label_rot_u8', src, meta, tab, zero.data_ptr(), zero.data_ptr(), o.data_ptr(), *a[4:])
            got['gt_semantic_seg'] = o
    monkeypatch.setattr(lib, 'call', call)
    s = _samples(40)
    kw = dict(crop_size=(32, 40), cat_max_ratio=0.75, reduce_zero_label=True, seg_pad_val=5, photometric=True, flip_prob=0.5,
              flip_direction='vertical', resize=dict(img_scale=(48, 36), ratio_range=(0.8, 1.5)))
    a = P.DeviceCollate('seg', cuda, **kw)(s, np.random.RandomState(41))
    torch.cuda.synchronize()
    assert sorted(got) == ['gt_semantic_seg', 'img']
    _equal_bits(a, got)


def test_degree_zero_equals_the_table_route_bitwise_and_same_seed_same_batch(cuda):
    s = _samples(42)
    kw = dict(reduce_zero_label=True, seg_pad_val=5, size_divisor=32, flip_prob=1.0, flip_direction='vertical',
              resize=dict(img_scale=(96, 64)))  # (no crop, no photometric: the batch does not depend on the stream)
    a = P.DeviceCollate('seg', cuda, **kw)(s, np.random.RandomState(43))
    col = P.DeviceCollate('seg', cuda, rotate=dict(prob=1.0, degree=(0, 0), pad_val=PAD, seg_pad_val=7), **kw)
    b = col(s, np.random.RandomState(43))
    assert [m['rotate_degree'] for m in b['img_metas']] == [0.0] * 3 and a['img'].shape == (3, 3, 96, 96)
    _equal_bits(a, b)
    col = P.DeviceCollate('seg', cuda, rotate=dict(prob=0.5, degree=30, pad_val=PAD, seg_pad_val=7), photometric=True, **kw)
    c, d = col(s, np.random.RandomState(44)), col(s, np.random.RandomState(44))
    assert any(m['rotate_degree'] is not None for m in c['img_metas'])
    _equal_bits(c, d)


def test_bad_arguments_of_the_rotating_entries(cuda):
    import ctypes
    from rscotr_amd._lib import lib
    f = (ctypes.c_float * 3)(1, 1, 1)
    p = ctypes.cast(f, ctypes.c_void_p)
    lib.call('rscotr_img_aug_rot_u8', 0, 0, 0, 0, 0, 0, 0, 0, 8, 8, p, p, 1, 0)  # B = 0: nothing to do
    lib.call('rscotr_seg_label_rot_u8', 0, 0, 0, 0, 0, 0, 0, 8, 8, 0, 255, 0)
    d = torch.zeros(256, dtype=torch.uint8, device=cuda).data_ptr()
    for args in [(d, d, d, d, 0, d, d, 1, 4, 4, p, p, 1, 0),   # no rot rows
                 (d, d, d, d, d, 0, d, 1, 4, 4, p, p, 1, 0),   # no warp tables
                 (d, d, d, d, d, d, d, 1, 4, 4, 0, p, 1, 0)]:  # no mean
        with pytest.raises(RuntimeError):
            lib.call('rscotr_img_aug_rot_u8', *args)
    with pytest.raises(RuntimeError):
        lib.call('rscotr_seg_label_rot_u8', d, d, d, 0, d, d, 1, 4, 4, 0, 255, 0)


# ---- smoke ------------------------------------------------------------------------------------------------------------------
def test_vertical_flips_and_rotation_feed_a_train_step(cuda, tmp_path):
    """PNG tiles -> DeviceLoader(train_collate_for('seg', vertical flips, RandomRotate)) -> MTL.train_step (tiny model, 64^2)."""
    from PIL import Image
    from util import build_model, load_model_cfg
    from rscotr_amd import data as D
    rng = np.random.RandomState(0)
    os.makedirs(tmp_path / 'img')
    os.makedirs(tmp_path / 'ann')
    for k in range(2):
        Image.fromarray(rng.randint(0, 256, (75, 70, 3)).astype(np.uint8)).save(tmp_path / 'img' / f't{k}.png')
        Image.fromarray(rng.randint(0, 7, (75, 70)).astype(np.uint8)).save(tmp_path / 'ann' / f't{k}.png')
    ds = P.TileSegDataset(str(tmp_path / 'img'), str(tmp_path / 'ann'))
    col = P.train_collate_for('seg', cuda, crop_size=(64, 64), resize=dict(img_scale=(64, 64), ratio_range=(0.5, 2.0)),
                              flip_direction='vertical', rotate=dict(prob=1.0, degree=20, seg_pad_val=255))
    loaders = dict(potsdam=P.DeviceLoader(ds, col, batch_size=2, seed=1))
    batch = next(iter(D.MultiDataLoader(loaders, D.RoundRobinIterationStrategy(loaders))))
    assert batch['task'] == 'seg' and batch['img'].shape == (2, 3, 64, 64)
    assert all(m['rotate_degree'] is not None and m['flip_direction'] in (None, 'vertical') for m in batch['img_metas'])
    out = build_model(load_model_cfg(tiny=True)[1]).to(cuda).train_step(batch)
    assert torch.isfinite(out['loss'])
