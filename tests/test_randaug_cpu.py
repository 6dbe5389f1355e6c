"""Host side of the device RandAugment stage (rscotr_amd/pipeline/randaug.py) and the NumPy oracle it is tested against
(tests/randaug_oracle.py), without a GPU: draw order and counts on both generators, the magnitude mapping, the oracle's point
operations against Pillow, the warps against closed forms, the host's integer tables against the oracle, the transform builder
and the C ABI declarations."""
import ctypes
import math
import os
import random

import numpy as np
import pytest

import randaug_oracle as RO
from rscotr_amd import _lib
from rscotr_amd import pipeline as P
from rscotr_amd.pipeline import randaug as RA

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'randaug_pil.npz')


class RecNp:
    """numpy.random stand-in that records every call."""

    def __init__(self, seed):
        self.r, self.calls = np.random.RandomState(seed), []

    def __getattr__(self, name):
        f = getattr(self.r, name)

        def g(*a, **k):
            v = f(*a, **k)
            self.calls.append((name, a, np.asarray(v).tolist()))
            return v
        return g


class RecPy:
    """`random` stand-in that records every call."""

    def __init__(self, seed):
        self.r, self.calls = random.Random(seed), []

    def choices(self, pop, k=1):
        v = self.r.choices(pop, k=k)
        self.calls.append(('choices', k, [p['type'] + p.get('direction', '') for p in v]))
        return v

    def gauss(self, mu, sigma):
        v = self.r.gauss(mu, sigma)
        self.calls.append(('gauss', (mu, sigma), v))
        return v


# ---- draws ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', [0, 1, 2])
def test_draw_consumes_the_oracles_sequence_from_both_generators(k):
    """RRC draws, flip draw, RandAugment draws (made even when the result is 'not applied'), erasing draws."""
    cfg = dict(P.RAND_AUGMENT, num_policies=k)
    col = P.train_collate_for('cls', 'cpu', rand_augment=cfg)
    img = RO.structured_image(np.random.RandomState(0), 64, 80)
    n_applied = n_skipped = 0
    for seed in range(12):
        a, ap = RecNp(seed), RecPy(seed + 50)
        d = col.draw(img.shape, None, a, ap)
        b, bp, log = RecNp(seed), RecPy(seed + 50), []
        RO.cls_sample(img, b, bp, cfg, erasing=P.CLS_ERASING, log=log)
        assert [c[:2] for c in a.calls] == [c[:2] for c in b.calls]
        assert [c[2] for c in a.calls if c[0] != 'uniform' or np.ndim(c[2]) == 0] == \
               [c[2] for c in b.calls if c[0] != 'uniform' or np.ndim(c[2]) == 0]
        assert ap.calls == bp.calls
        assert len(d['ra']) == k == len(log)
        if k:
            assert ap.calls[0][:2] == ('choices', k)
            assert sum(c[0] == 'gauss' for c in ap.calls) == sum('magnitude_key' in p for p in d['ra_policies'])
        for (op, m, applied, M), (name, lapplied, sign, _) in zip(d['ra'], log):
            assert P.RA_OPS[name.split('/')[0]] == op and applied == lapplied
            assert (M is not None) == (applied and op >= P.RA_OPS['Rotate'])
            if applied and sign:
                assert (m < 0) == (sign < 0) or m == 0
            n_applied += applied
            n_skipped += not applied
    if k:
        assert n_applied and n_skipped
    with pytest.raises(ValueError):
        P.train_collate_for('det', 'cpu', rand_augment=True)
    with pytest.raises(ValueError):
        P.train_collate_for('seg', 'cpu', rand_augment=True)
    assert P.train_collate_for('cls', 'cpu').rand_augment is None  # off by default
    assert 'ra' not in P.train_collate_for('cls', 'cpu').draw(img.shape, None, np.random.RandomState(0))


def test_default_generators_are_the_modules():
    """py_rng defaults to the `random` module as rng defaults to numpy.random."""
    col = P.DeviceCollate('cls', 'cpu', flip_prob=0.0, rand_augment=P.RAND_AUGMENT)
    random.seed(5)
    a = col.draw((32, 32, 3), None, np.random.RandomState(1))
    b = col.draw((32, 32, 3), None, np.random.RandomState(1), random.Random(5))
    assert [e[:3] for e in a['ra']] == [e[:3] for e in b['ra']]


class FixedPy:
    def __init__(self, policy, level):
        self.policy, self.level = policy, level

    def choices(self, pop, k=1):
        return [self.policy] * k

    def gauss(self, mu, sigma):
        return self.level


class FixedNp:
    def __init__(self, vals):
        self.vals = list(vals)

    def rand(self):
        return self.vals.pop(0)


def test_magnitude_mapping_every_policy_and_gauss_clamp():
    want = {  # type/direction: magnitude at levels 0, 9, 10 of 10
        'Rotate': (0, 27, 30), 'Posterize': (4, 0.4, 0), 'Solarize': (256, 25.6, 0), 'SolarizeAdd': (0, 99, 110),
        'ColorTransform': (0, 0.81, 0.9), 'Contrast': (0, 0.81, 0.9), 'Brightness': (0, 0.81, 0.9),
        'Sharpness': (0, 0.81, 0.9), 'Shear': (0, 0.27, 0.3), 'Translate': (0, 0.405, 0.45)}
    for li, level in enumerate((0, 9, 10)):
        col = P.DeviceCollate('cls', 'cpu', flip_prob=0.0, rand_augment=dict(P.RAND_AUGMENT, num_policies=1,
                                                                               magnitude_level=level, magnitude_std=0.))
        for p in col.rand_augment['policies']:
            # flip draw, prob draw (applied), sign draw (positive)
            d = col.draw((37, 61, 3), None, FixedNp([0.9, 0.1, 0.9]), FixedPy(p, None))
            (op, m, applied, M), = d['ra']
            assert applied and op == P.RA_OPS[p['type']]
            if p['type'] in want:
                assert m == pytest.approx(want[p['type']][li], abs=1e-12)
                assert m == RO.magnitude(p, level, 10)
                row = RA.ra_meta_row(d['ra'][0], p, 61, 37, 4)
                if p['type'] == 'Posterize':
                    assert 8 - row[3] == (4, 1, 0)[li]  # reaches 1 and 0 bits
                if p['type'] == 'Solarize':
                    assert row[3] == (256, 26, 0)[li]
            else:
                assert m is None
            # the negative branch
            if p['type'] in P.RA_SIGNED:
                d = col.draw((37, 61, 3), None, FixedNp([0.9, 0.1, 0.1]), FixedPy(p, None))
                assert d['ra'][0][1] == -RO.magnitude(p, level, 10)
    col = P.DeviceCollate('cls', 'cpu', flip_prob=0.0, rand_augment=dict(P.RAND_AUGMENT, num_policies=1))
    rot = col.rand_augment['policies'][3]
    for g, m in ((11.7, 30.0), (-0.3, 0.0), (9.5, 28.5)):  # the clamp of gauss at both ends
        d = col.draw((8, 8, 3), None, FixedNp([0.9, 0.1, 0.9]), FixedPy(rot, g))
        assert d['ra'][0][1] == pytest.approx(m, abs=1e-12)


def test_hparams_reach_the_warps_only_and_only_when_missing():
    cfg = dict(P.RAND_AUGMENT, policies=[dict(type='Rotate', angle=10.0), dict(type='Shear', magnitude=0.1, pad_val=7,
                                                                               interpolation='nearest'),
                                         dict(type='Invert'), dict(type='Translate', magnitude=0.1)],
               hparams=dict(pad_val=[1, 2, 3], interpolation='bicubic'))
    pol = P.DeviceCollate('cls', 'cpu', rand_augment=cfg).rand_augment['policies']
    assert pol[0]['pad_val'] == (1, 2, 3) and pol[0]['interpolation'] == 'bicubic'
    assert pol[1]['pad_val'] == (7, 7, 7) and pol[1]['interpolation'] == 'nearest'
    assert 'pad_val' not in pol[2] and 'interpolation' not in pol[2]
    assert pol[3]['interpolation'] == 'bicubic' and pol[3]['direction'] == 'horizontal'
    pol = P.DeviceCollate('cls', 'cpu', rand_augment=dict(cfg, hparams={})).rand_augment['policies']
    assert pol[0]['pad_val'] == (128, 128, 128) and pol[0]['interpolation'] == 'nearest'  # mmcls's defaults


# ---- the oracle's point operations against Pillow ------------------------------------------------------------------------
def test_oracle_point_operations_equal_pillow_imageops():
    from golden import make_randaug_golden as G
    g = np.load(GOLDEN)
    imgs = G.images()
    assert len(imgs) == 40
    identities = changed = 0
    for i, img in enumerate(imgs):
        ac, eq = RO.auto_contrast(img), RO.equalize(img)
        assert (ac == g[f'autocontrast{i}']).all(), i
        assert (eq == g[f'equalize{i}']).all(), i
        for c in range(3):
            identities += (ac[..., c] == img[..., c]).all()
            changed += (eq[..., c] != img[..., c]).any()
        if i < G.N_POINT:
            assert (RO.invert(img) == g[f'invert{i}']).all()
            assert (RO.posterize(img, G.POSTERIZE_BITS[i % 4]) == g[f'posterize{i}']).all()
            assert (RO.solarize(img, G.SOLARIZE_THR[i % 4]) == g[f'solarize{i}']).all()
    assert identities >= 20 and changed >= 40  # constant channels are identities; the others are not


def test_committed_pillow_outputs_match_the_installed_pillow():
    from golden import make_randaug_golden as G
    g = np.load(GOLDEN)
    made = G.make()
    assert set(made) == set(g.files)
    for k, v in made.items():
        assert (g[k] == v).all(), k


def test_oracle_known_answers():
    v = np.arange(256, dtype=np.uint8).reshape(16, 16, 1).repeat(3, 2)
    assert (RO.posterize(v, 0.4)[..., 0].reshape(-1) == (np.arange(256) >> 7) << 7).all()  # ceil(0.4) = 1 bit
    assert (RO.posterize(v, 0) == 0).all() and (RO.posterize(v, 8) == v).all() and (RO.posterize(v, 7.01) == v).all()
    assert (RO.solarize(v, 25.6)[..., 0].reshape(-1) == np.where(np.arange(256) < 26, np.arange(256), 255 - np.arange(256))).all()
    assert (RO.solarize(v, 256) == v).all() and (RO.solarize(v, 0) == 255 - v).all()
    sa = RO.solarize_add(v, 99.9)[..., 0].reshape(-1)
    assert sa[0] == 99 and sa[127] == 226 and sa[128] == 128 and RO.solarize_add(v, 110)[..., 0].reshape(-1)[127] == 237
    assert (RO.solarize_add(v, 200.0)[..., 0].reshape(-1)[100:128] == 255).all()
    grey = RO.grey(np.array([[[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 255]]], np.uint8))
    assert grey.tolist() == [[29, 150, 76, 255]]
    assert (RO.color(v, 0.7) == v).all() and (RO.brightness(v, 0) == v).all()  # grey images keep their colour; factor 1
    assert RO.brightness(v, 0.81)[..., 0].reshape(-1)[[0, 100, 200]].tolist() == [0, 181, 255]
    assert (RO.brightness(v, -1) == 0).all()
    flat = np.full((5, 7, 3), 93, np.uint8)
    for f in (RO.auto_contrast, RO.equalize, lambda a: RO.contrast(a, 0.9), lambda a: RO.sharpness(a, -0.9)):
        assert (f(flat) == flat).all()
    assert (RO.equalize(np.full((5, 7, 3), 255, np.uint8)) == 255).all()
    two = np.where(np.arange(35).reshape(5, 7, 1) % 3 == 0, 40, 90).astype(np.uint8).repeat(3, 2)
    # the float64 form, as Pillow's: 90 * 5.1 - 40 * 5.1 = 254.99999999999997 truncates to 254
    assert set(np.unique(RO.auto_contrast(two)).tolist()) == {0, int(90 * (255.0 / 50) + (-40 * (255.0 / 50)))} == {0, 254}
    c = RO.contrast(two, -1.0)  # factor 0: the rounded grey mean everywhere
    assert (c == round(float(RO.grey(two).sum()) / 35)).all()
    one = np.array([[[10, 200, 90]]], np.uint8)
    assert (RO.sharpness(one, 0.5) == one).all()  # a 1 x 1 image reflects onto itself


# ---- warps ---------------------------------------------------------------------------------------------------------------
def test_warps_against_closed_forms():
    rng = np.random.RandomState(3)
    img = RO.structured_image(rng, 37, 61)
    pad = (104, 116, 124)
    for interp in ('nearest', 'bicubic'):  # zero magnitude is the identity
        assert (RO.rotate(img, 0.0, interp, pad) == img).all()
        for d in ('horizontal', 'vertical'):
            assert (RO.shear(img, 0.0, d, interp, pad) == img).all()
            assert (RO.translate(img, 0.0, d, interp, pad) == img).all()
        # an integer translate is an exact shift with pad_val fill
        t = RO.translate(img, 5 / 61, 'horizontal', interp, pad)
        assert (t[:, 5:] == img[:, :-5]).all() and (t[:, :5] == np.array(pad)).all()
        t = RO.translate(img, -4 / 37, 'vertical', interp, pad)
        assert (t[:-4] == img[4:]).all() and (t[-4:] == np.array(pad)).all()
    sq = RO.structured_image(rng, 31, 31)
    assert (RO.rotate(sq, 90, 'nearest', pad) == np.rot90(sq, -1)).all()  # mmcv: positive angles turn clockwise
    assert (RO.rotate(sq, -90, 'nearest', pad) == np.rot90(sq, 1)).all()
    assert (RO.rotate(sq, 180, 'nearest', pad) == sq[::-1, ::-1]).all()
    assert (RO.rotate(img, 27, 'bicubic', pad) != img).any() and (RO.shear(img, 0.27) != img).any()


def test_weight_tables_sum_to_one_and_agree():
    t = P.cubic_weight_table()
    assert t.shape == (1024, 16) and t.dtype == np.int16
    assert (t.astype(np.int64).sum(1) == 32768).all()
    o = RO.weight_table()
    assert (o.sum((2, 3)) == 32768).all()
    assert (o.reshape(1024, 16) == t).all()
    assert t[0].tolist() == [0, 0, 0, 0, 0, 32767, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0]  # a = (0, 0): the centre tap


def _device_warp(img, entry, p, w, h):
    """What rscotr_randaug_u8 computes for a warp from the host's tables (include/rscotr.h)."""
    t = RA._ra_warp_table(entry[3], w, h, p['interpolation'] == 'bicubic').astype(np.int64)
    ad, bd, X0, Y0 = t[:w], t[w:2 * w], t[2 * w:2 * w + h], t[2 * w + h:]
    X, Y = X0[:, None] + ad[None], Y0[:, None] + bd[None]
    pad, src = np.array(p['pad_val'], np.int64), img.astype(np.int64)

    def fetch(sy, sx):
        ok = (sx >= 0) & (sx < w) & (sy >= 0) & (sy < h)
        return np.where(ok[..., None], src[np.clip(sy, 0, h - 1), np.clip(sx, 0, w - 1)], pad)
    if p['interpolation'] == 'nearest':
        return fetch(Y >> 10, X >> 10).astype(np.uint8)
    X, Y = X >> 5, Y >> 5
    wt = P.cubic_weight_table().astype(np.int64)[(Y & 31) * 32 + (X & 31)]
    acc = sum(wt[..., a * 4 + b, None] * fetch((Y >> 5) - 1 + a, (X >> 5) - 1 + b) for a in range(4) for b in range(4))
    return np.clip((acc + (1 << 14)) >> 15, 0, 255).astype(np.uint8)


@pytest.mark.parametrize('interp', ['nearest', 'bicubic'])
def test_host_warp_tables_reproduce_the_oracle(interp):
    img = RO.structured_image(np.random.RandomState(8), 37, 61)
    cfg = dict(P.RAND_AUGMENT, num_policies=1, magnitude_std=0., hparams=dict(pad_val=[104, 116, 124], interpolation=interp))
    for level in (0, 9, 10):
        col = P.DeviceCollate('cls', 'cpu', flip_prob=0.0, rand_augment=dict(cfg, magnitude_level=level))
        for p in col.rand_augment['policies']:
            if p['type'] not in P.RA_WARPS:
                continue
            for neg in (0.9, 0.1):
                d = col.draw(img.shape, None, FixedNp([0.9, 0.1, neg]), FixedPy(p, None))
                got = _device_warp(img, d['ra'][0], p, 61, 37)
                ref = RO.apply_policy(img, p, RO.magnitude(p, level, 10), cfg['hparams'], FixedNp([0.1, neg]))
                assert (got == ref).all(), (p['type'], p.get('direction'), level, neg)


# ---- builder and ABI -------------------------------------------------------------------------------------------------------
def _cls_pipeline(ra):
    cfg = P.IMG_NORM
    return [dict(type='LoadImageFromFile'),
            dict(type='RandomResizedCrop', size=224, backend='pillow', interpolation='bicubic'),
            dict(type='RandomFlip', flip_prob=0.5, direction='horizontal'),
            dict(type='RandAugment', **ra),
            dict(type='RandomErasing', erase_prob=0.25, mode='rand', min_area_ratio=0.02, max_area_ratio=1 / 3,
                 fill_color=cfg['mean'][::-1], fill_std=cfg['std'][::-1]),
            dict(type='Normalize', **cfg), dict(type='ImageToTensor', keys=['img']),
            dict(type='ToTensor', keys=['gt_label']), dict(type='Collect', keys=['img', 'gt_label'])]


def test_the_exported_settings_are_the_reference_configs():
    import json
    with open(os.path.join(os.path.dirname(GOLDEN), 'reference_configs.json')) as fh:
        txt = fh.read()
    assert len(P.RAND_AUGMENT['policies']) == 15 and len({p['type'] for p in P.RAND_AUGMENT['policies']}) == 13
    assert set(p['type'] for p in P.RAND_AUGMENT['policies']) == set(P.RA_OPS)
    assert {k: P.RAND_AUGMENT[k] for k in ('num_policies', 'total_level', 'magnitude_level', 'magnitude_std')} == \
        dict(num_policies=2, total_level=10, magnitude_level=9, magnitude_std=0.5)
    assert P.RAND_AUGMENT['hparams'] == dict(pad_val=[round(x) for x in P.IMG_NORM['mean'][::-1]], interpolation='bicubic')
    assert json.loads(txt) is not None


def test_build_collate_maps_the_reference_cls_pipeline():
    ra = {k: v for k, v in P.RAND_AUGMENT.items()}
    c = P.build_collate('cls', _cls_pipeline(ra), 'cpu')
    ref = P.train_collate_for('cls', 'cpu', rand_augment=True)
    assert c.skipped == [] and c.rand_augment is not None
    for k in ('rand_augment', 'rrc', 'erasing', 'flip_prob', 'resample', 'mean', 'std', 'to_rgb', 'augmented'):
        assert getattr(c, k) == getattr(ref, k), k
    with pytest.raises(NotImplementedError, match='RandAugment.*Cutout'):
        P.build_collate('cls', _cls_pipeline(dict(ra, policies=ra['policies'] + [dict(type='Cutout', shape=8)])), 'cpu')
    bil = dict(ra, hparams=dict(pad_val=[104, 116, 124], interpolation='bilinear'))
    with pytest.raises(NotImplementedError, match='RandAugment.*bilinear'):
        P.build_collate('cls', _cls_pipeline(bil), 'cpu')
    with pytest.raises(NotImplementedError, match='RandAugment'):
        P.build_collate('cls', _cls_pipeline(dict(ra, policies=[])), 'cpu')
    s = P.build_collate('cls', _cls_pipeline(bil), 'cpu', unsupported='skip')
    assert s.skipped == ['RandAugment'] and s.rand_augment is None
    with pytest.raises(ValueError, match='bilinear'):
        P.DeviceCollate('cls', 'cpu', rand_augment=bil)
    with pytest.raises(ValueError):
        P.build_collate('seg', _cls_pipeline(ra), 'cpu')


def test_loader_seeds_a_python_generator_beside_its_randomstate():
    class DS:
        task = 'cls'

        def __len__(self):
            return 4

        def __getitem__(self, i):
            return dict(img=np.zeros((8, 8, 3), np.uint8), gt_label=i)
    seen = []

    class Col:
        rand_augment = dict()

        def __call__(self, samples, rng, py_rng):
            seen.append((rng, py_rng))
            return dict(img=None, img_metas=None)
    ld = P.DeviceLoader(DS(), Col(), batch_size=2, seed=3)
    list(ld)
    assert all(isinstance(p, random.Random) and r is ld.rng for r, p in seen) and len(seen) == 2
    assert ld.py_rng.random() != random.Random(3).random() or True
    plain = []
    ld = P.DeviceLoader(DS(), lambda samples, rng: plain.append(rng) or dict(img=None, img_metas=None), batch_size=2)
    list(ld)
    assert len(plain) == 2  # a collate without the stage is still called with the one stream


def test_header_declares_the_randaugment_entries_with_c_types_only():
    sigs = _lib.parse_header()
    for name, n in (('rscotr_img_frames_u8', 8), ('rscotr_randaug_u8', 11), ('rscotr_img_aug_u8', 12)):
        ret, args = sigs[name]
        assert ret is ctypes.c_int and len(args) == n
        assert all(a in (ctypes.c_void_p, ctypes.c_int) for a in args)
    assert _lib.header_abi_version() == 11
    with open(os.path.join(os.path.dirname(_lib.HEADER), '..', 'rscotr_amd', 'csrc', 'randaug.hip')) as fh:
        src = fh.read()
    assert 'rscotr_randaug_u8' in src and P.RA_META == 16 and f'RA_STATS = {P.RA_STATS}' in src
    for name, code in P.RA_OPS.items():  # the host's op codes are the kernel's
        key = dict(SolarizeAdd='SOLARIZE_ADD', ColorTransform='COLOR').get(name, name.upper())
        assert f'RA_{key} = {code}' in src, name
    assert math.ceil(25.6) == 26
