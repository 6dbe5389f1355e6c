"""Device RandAugment (rscotr_img_frames_u8 -> rscotr_randaug_u8 per slot -> rscotr_img_aug_u8) against the NumPy restatement
of mmcls RandAugment (tests/randaug_oracle.py) on the same seeds of both generators.  The tolerance is that of
tests/test_augment_gpu.py: 1e-6 * max|ref| after Normalize, i.e. the uint8 frames must be exact (one LSB is ~0.017 there) --
every operation is integer or a fixed sequence of float32 operations."""
import os
import random

import numpy as np
import pytest
import torch

import aug_oracle as AO
import randaug_oracle as RO
from rscotr_amd import pipeline as P
from rscotr_amd._lib import lib

pytestmark = pytest.mark.gpu
MEAN, STD = P.IMG_NORM['mean'], P.IMG_NORM['std']
# established on the CPU with the oracle alone: the fewest leading seeds that cover every policy and sign; seed 6 is left
# out because its batch applies an AutoContrast to a frame that already spans 0..255 (an applied operation that changes nothing)
RECIPE_SEEDS = (0, 1, 2, 3, 4, 5, 7, 8)


def _close(got, ref):
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.abs(got - ref).max() <= 1e-6 * max(np.abs(ref).max(), 1.0)


def _mismatch(got, ref):
    """Largest |got - ref| when it exceeds the tolerance, else 0 (to name the failing cases of a loop together)."""
    d = float(np.abs(got.cpu().numpy() - ref).max())
    return d if d > 1e-6 * max(np.abs(ref).max(), 1.0) else 0.0


def _collate_ref(ims):
    H, W = max(i.shape[0] for i in ims), max(i.shape[1] for i in ims)
    return AO.collate_images(ims, (H, W), MEAN, STD)


class Chosen:
    """Python-generator stand-in: `choices` hands out the policies at the given indices, in order."""

    def __init__(self, indices):
        self.indices = list(indices)

    def choices(self, pop, k=1):
        out, self.indices = [pop[i] for i in self.indices[:k]], self.indices[k:]
        assert len(out) == k
        return out

    def gauss(self, mu, sigma):
        return mu


def _run_fixed(cuda, imgs, cfg, per_sample, seed=0):
    """Device and oracle on `imgs` with each sample's policies fixed (`per_sample`: one list of indices into cfg['policies']
    per image), no RandomResizedCrop, no flip -> (device batch, oracle images, oracle log)."""
    col = P.DeviceCollate('cls', cuda, flip_prob=0.0, rand_augment=cfg)
    flat = [i for ps in per_sample for i in ps]
    b = col([dict(img=i, gt_label=0) for i in imgs], np.random.RandomState(seed), Chosen(flat))
    r, py, log, refs = np.random.RandomState(seed), Chosen(flat), [], []
    for i in imgs:
        refs.append(RO.cls_sample(i, r, py, cfg, size=None, flip_prob=0.0, log=log)[0])
    assert py.indices == []
    return b, refs, log


def recipe_batch(seed):
    """16 structured 256^2 tiles and the oracle's result for them under the reference recipe -> (samples, images, metas, log)."""
    rng = np.random.RandomState(1000 + seed)
    s = [dict(img=RO.structured_image(rng, 256, 256), gt_label=int(rng.randint(0, 45))) for _ in range(16)]
    r, py, log, ims, metas = np.random.RandomState(seed + 5), random.Random(seed + 9), [], [], []
    for x in s:
        im, m = RO.cls_sample(x['img'], r, py, P.RAND_AUGMENT, erasing=P.CLS_ERASING, log=log)
        ims.append(im)
        metas.append(m)
    return s, ims, metas, log


def recipe_coverage(logs):
    """{policy name: set of signs applied} over oracle logs; every applied operation must have changed its frame."""
    seen = {}
    for name, applied, sign, changed in logs:
        if applied:
            assert changed > 0, name
            seen.setdefault(name, set()).add(sign)
    return seen


def test_reference_recipe_batches_cover_every_policy(cuda):
    """train_collate_for('cls', cuda, rand_augment=True) on 16 x 256^2 tiles for several seeds: images, flips, labels and
    erasing agree; over the batches each of the 15 policies is applied, each signed one in both signs, and every applied
    operation changes its input frame (the oracle's own bookkeeping)."""
    col = P.train_collate_for('cls', cuda, rand_augment=True)
    logs = []
    for seed in RECIPE_SEEDS:
        s, ims, metas, log = recipe_batch(seed)
        b = col(s, np.random.RandomState(seed + 5), random.Random(seed + 9))
        assert [m['flip'] for m in b['img_metas']] == [m['flip'] for m in metas]
        assert b['gt_label'].tolist() == [x['gt_label'] for x in s]
        assert b['img'].shape == (16, 3, 224, 224)
        _close(b['img'], AO.collate_images(ims, (224, 224), MEAN, STD))
        assert len(log) == 32
        plan = [e for m in b['img_metas'] for e in m['rand_augment']]
        assert [e[2] for e in plan] == [l[1] for l in log]
        logs += log
    seen = recipe_coverage(logs)
    names = {p['type'] + ('/' + p['direction'] if 'direction' in p else '') for p in P.RAND_AUGMENT['policies']}
    assert set(seen) == names and len(names) == 15
    for name, signs in seen.items():
        assert signs == ({1, -1} if name.split('/')[0] in RO.SIGNED else {0}), (name, signs)


def _variants():
    out = []
    for p in P.RAND_AUGMENT['policies']:
        q = dict(p, prob=1.0)
        if p['type'] in RO.SIGNED:
            out += [dict(q, random_negative_prob=0.0), dict(q, random_negative_prob=1.0)]
        else:
            out.append(q)
    return out


@pytest.mark.parametrize('interp', ['nearest', 'bicubic'])
@pytest.mark.parametrize('level', [0, 9, 10])
@pytest.mark.parametrize('hw', [(224, 224), (37, 61)])
def test_each_policy_alone(cuda, hw, level, interp):
    """Each of the 15 policies alone (num_policies=1, prob=1.0), in both signs where signed, at levels 0, 9 and 10 of 10, on
    224^2 and on a non-square odd size; nearest and bicubic for the warps (the other operations run with 'bicubic' only:
    they do not read it); a structured and a noise image per batch."""
    rng = np.random.RandomState(hw[0] + level)
    imgs = [RO.structured_image(rng, *hw), rng.randint(0, 256, hw + (3,)).astype(np.uint8)]
    pols = _variants()
    cfg = dict(P.RAND_AUGMENT, policies=pols, num_policies=1, magnitude_level=level, magnitude_std=0.,
               hparams=dict(pad_val=[104, 116, 124], interpolation=interp))
    ran, bad = 0, []
    for i, p in enumerate(pols):
        if interp == 'nearest' and p['type'] not in P.RA_WARPS:
            continue
        b, refs, log = _run_fixed(cuda, imgs, cfg, [[i], [i]])
        d = _mismatch(b['img'], _collate_ref(refs))
        if d:
            bad.append((p['type'], p.get('direction'), p.get('random_negative_prob'), d))
        assert len(log) == 2 and all(l[1] for l in log)
        assert all(l[2] == (0 if p['type'] not in RO.SIGNED else -1 if p['random_negative_prob'] else 1) for l in log)
        if level == 0 and (p['type'] in RO.SIGNED or p['type'] in ('Solarize', 'SolarizeAdd')):
            assert [l[3] for l in log] == [0, 0], p  # zero magnitude: the identity
        elif level > 0 or p['type'] in ('AutoContrast', 'Equalize', 'Invert', 'Posterize'):
            assert log[0][3] > 0, p  # the structured image changes
        ran += 1
    assert not bad, bad
    assert ran == (10 if interp == 'nearest' else 24)


def test_statistics_edge_cases_and_ragged_frames(cuda):
    """A constant image, a channel with two values, a `step == 0` Equalize (fewer than 255 pixels outside the last bin), an
    all-255 image, a 1 x 1 image, under AutoContrast, Equalize, Contrast (both signs) and Sharpness; frames of different
    sizes in one batch."""
    rng = np.random.RandomState(12)
    two = np.where(rng.rand(40, 56, 1) < 0.3, 40, 90).astype(np.uint8).repeat(3, 2)
    two[..., 1] = rng.randint(0, 256, (40, 56))
    imgs = [np.full((33, 47, 3), 93, np.uint8), two, rng.randint(0, 256, (9, 11, 3)).astype(np.uint8),
            np.full((16, 16, 3), 255, np.uint8), RO.structured_image(rng, 64, 50), np.zeros((1, 1, 3), np.uint8) + 7]
    mag = dict(magnitude_key='magnitude', magnitude_range=(0, 0.9), prob=1.0)
    pols = [dict(type='AutoContrast', prob=1.0), dict(type='Equalize', prob=1.0),
            dict(type='Contrast', random_negative_prob=0.0, **mag), dict(type='Contrast', random_negative_prob=1.0, **mag),
            dict(type='Sharpness', random_negative_prob=1.0, **mag)]
    cfg = dict(P.RAND_AUGMENT, policies=pols, num_policies=1, magnitude_std=0.)
    for i, p in enumerate(pols):
        b, refs, log = _run_fixed(cuda, imgs, cfg, [[i]] * len(imgs))
        assert b['img'].shape[-2:] == (64, 56)
        _close(b['img'], _collate_ref(refs))
        if p['type'] in ('AutoContrast', 'Equalize'):
            assert log[0][3] == 0 and log[3][3] == 0 and log[4][3] > 0  # the constant images are identities, others not
    assert (RO.equalize(imgs[2]) == imgs[2]).all()  # step == 0
    assert (RO.auto_contrast(two)[..., 0] != two[..., 0]).all()  # two levels go to 0 and 254


def test_two_slots_ping_pong_orders(cuda):
    """The same operation in both slots, a warp followed by a statistics operation and the reverse, 'not applied' slots
    beside applied ones, and num_policies = 0."""
    rng = np.random.RandomState(21)
    imgs = [RO.structured_image(rng, 48, 72) for _ in range(6)]
    pols = [dict(p, prob=1.0) for p in P.RAND_AUGMENT['policies']] + [dict(type='Invert', prob=-1.0)]  # last: never applied
    ix = {p['type'] + p.get('direction', ''): i for i, p in enumerate(pols[:-1])}
    off = len(pols) - 1
    per = [[ix['Equalize'], ix['Equalize']], [ix['Rotate'], ix['AutoContrast']], [ix['Contrast'], ix['Shearvertical']],
           [ix['Rotate'], ix['Rotate']], [off, ix['Sharpness']], [ix['Translatehorizontal'], off]]
    cfg = dict(P.RAND_AUGMENT, policies=pols, magnitude_std=0.)
    b, refs, log = _run_fixed(cuda, imgs, cfg, per, seed=4)
    _close(b['img'], _collate_ref(refs))
    assert [l[1] for l in log] == [True] * 8 + [False, True, True, False]
    assert all(l[3] > 0 for l in log if l[1])
    b, refs, log = _run_fixed(cuda, imgs, dict(cfg, num_policies=0), [[]] * 6)
    assert log == [] and all((r == i).all() for r, i in zip(refs, imgs))
    _close(b['img'], _collate_ref(imgs))


def _record_calls(monkeypatch):
    names, real = [], lib.call

    def spy(name, *args):
        names.append(name)
        return real(name, *args)
    monkeypatch.setattr(lib, 'call', spy)
    return names


def test_off_is_the_one_launch_path_and_the_stage_adds_its_launches(cuda, monkeypatch):
    """rand_augment=None: the one `rscotr_img_aug_u8` call, and bitwise the batch of the stage with no slot (whose frames take
    the detour through uint8 and the identity entries); the library calls are checked by name."""
    rng = np.random.RandomState(2)
    s = [dict(img=RO.structured_image(rng, 256, 256), gt_label=k) for k in range(8)]
    names = _record_calls(monkeypatch)
    a = P.train_collate_for('cls', cuda)(s, np.random.RandomState(6))
    assert names == ['rscotr_img_aug_u8']
    r = np.random.RandomState(6)
    _close(a['img'], AO.collate_images([AO.cls_sample(x['img'], r, erasing=P.CLS_ERASING)[0] for x in s], (224, 224), MEAN, STD))
    del names[:]
    z = P.train_collate_for('cls', cuda, rand_augment=dict(P.RAND_AUGMENT, num_policies=0))(s, np.random.RandomState(6))
    assert names == ['rscotr_img_frames_u8', 'rscotr_img_aug_u8']
    assert torch.equal(a['img'].view(torch.int32), z['img'].view(torch.int32))
    del names[:]
    P.train_collate_for('cls', cuda, rand_augment=True)(s, np.random.RandomState(6), random.Random(1))
    assert names == ['rscotr_img_frames_u8', 'rscotr_randaug_u8', 'rscotr_randaug_u8', 'rscotr_img_aug_u8']
    assert 'rand_augment' not in a['img_metas'][0]


def test_same_seeds_same_bytes(cuda):
    rng = np.random.RandomState(3)
    s = [dict(img=RO.structured_image(rng, 200, 230), gt_label=k) for k in range(16)]
    col = P.train_collate_for('cls', cuda, rand_augment=True)
    a = col(s, np.random.RandomState(11), random.Random(12))
    b = col(s, np.random.RandomState(11), random.Random(12))
    c = col(s, np.random.RandomState(11), random.Random(13))
    assert torch.equal(a['img'].view(torch.int32), b['img'].view(torch.int32))
    assert not torch.equal(a['img'].view(torch.int32), c['img'].view(torch.int32))  # the second generator matters


def test_empty_batch_and_bad_arguments(cuda):
    lib.call('rscotr_img_frames_u8', 0, 0, 0, 0, 0, 8, 8, 0)  # B = 0: nothing to do
    lib.call('rscotr_randaug_u8', 0, 0, 0, 0, 0, 0, 1, 0, 8, 8, 0)
    t = torch.zeros(4096, dtype=torch.uint8, device=cuda)
    d = t.data_ptr()
    for args in [(d, d + 1024, d, d, d, 0, 0, -1, 4, 4, 0),        # negative B
                 (d, d, d, d, d, 0, 0, 1, 4, 4, 0),                # in == out
                 (d, d + 1024, 0, d, d, 0, 0, 1, 4, 4, 0),         # no meta
                 (d, d + 1024, d, d, 0, 0, 0, 1, 4, 4, 0),         # no weight table
                 (d, d + 1024, d, d, d, 0, 1, 1, 4, 4, 0),         # need_stats without a table
                 (d, d + 1024, d, d, d, d + 2052, 1, 1, 4, 4, 0),  # misaligned statistics table
                 (d, d + 1024, d, d, d, 0, 0, 70000, 4, 4, 0)]:    # B too large
        with pytest.raises(RuntimeError, match='rscotr_randaug_u8'):
            lib.call('rscotr_randaug_u8', *args)
    for args in [(d, d, 0, d + 1024, 1, 4, 4, 0), (d, d, d, d, 1, 4, 4, 0), (d, d, d, d + 1024, 1, -4, 4, 0)]:
        with pytest.raises(RuntimeError, match='rscotr_img_frames_u8'):
            lib.call('rscotr_img_frames_u8', *args)
    torch.cuda.synchronize()
    assert (t == 0).all()  # nothing was launched
    b = P.train_collate_for('cls', cuda, rand_augment=True)([], np.random.RandomState(0), random.Random(0))
    assert b['img'].shape[0] == 0 and b['img_metas'] == [] and b['gt_label'].numel() == 0
    with pytest.raises(ValueError):
        P.train_collate_for('seg', cuda, rand_augment=True)


def test_loader_fed_cls_train_step(cuda, tmp_path):
    """PNG class folders -> DeviceLoader(train_collate_for('cls', rand_augment=True)) -> MultiDataLoader -> MTL.train_step."""
    from PIL import Image
    from util import build_model, load_model_cfg
    from rscotr_amd import data as D
    rng = np.random.RandomState(0)
    for c in ('airport', 'beach'):
        os.makedirs(tmp_path / c)
        for k in range(3):
            Image.fromarray(RO.structured_image(rng, 90, 100)).save(tmp_path / c / f't{k}.png')
    ds = P.FolderClsDataset(str(tmp_path))
    col = P.train_collate_for('cls', cuda, random_resized_crop=dict(size=64), rand_augment=True)
    loaders = dict(resisc=P.DeviceLoader(ds, col, batch_size=4, seed=1))
    m = D.MultiDataLoader(loaders, D.RoundRobinIterationStrategy(loaders))
    batch = next(iter(m))
    assert batch['task'] == 'cls' and batch['img'].shape == (4, 3, 64, 64)
    assert all(len(mt['rand_augment']) == 2 for mt in batch['img_metas'])
    cfg, mcfg = load_model_cfg(tiny=True)
    model = build_model(mcfg).to(cuda)
    out = model.train_step(batch)
    assert torch.isfinite(out['loss'])
