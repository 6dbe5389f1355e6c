"""The multi-scale AutoAugment det pipeline on the device (rscotr_img_aug_chain_u8, and rscotr_img_aug_u8 with the early flip in
its tables) against the sequential NumPy restatement tests/det_aug_oracle.py on the same seeded stream: images within
1e-6 * max|ref| (one LSB of the uint8 stage is ~0.017 after Normalize, so the uint8 values must be exact), boxes, labels and
metas exact; and the chain launch bit-equal to the explicit two passes through a stored uint8 frame."""
import ctypes

import numpy as np
import pytest
import torch

import det_aug_oracle as DO
from rscotr_amd import pipeline as P
from test_det_autoaug_cpu import POLICIES, Fixed, pipeline, samples

pytestmark = pytest.mark.gpu
MEAN, STD = P.IMG_NORM['mean'], P.IMG_NORM['std']
SEEDS = (0, 1, 2, 3, 4, 5, 17, 53)  # (17 and 53: a second stage that reduces)
STEP_SEED = 12  # test_train_step_on_an_autoaugment_batch: an image without boxes on a ragged canvas


def _close(got, ref):
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.abs(got - ref).max() <= 1e-6 * max(np.abs(ref).max(), 1.0)


def _check(batch, s, rng, policies, flip_ratio=0.5):
    """The batch against the helper on the stream `rng` -> the helper's infos."""
    ims, boxes, labels, infos, hw = DO.det_autoaug_batch(s, rng, policies, flip_ratio)
    assert tuple(batch['img'].shape) == (len(s), 3, *hw)
    _close(batch['img'], DO.collate(ims, hw, MEAN, STD))
    for k, (x, m, im, bb, ll, info) in enumerate(zip(s, batch['img_metas'], ims, boxes, labels, infos)):
        assert m['flip'] == info['flip'] and m['flip_direction'] == ('horizontal' if info['flip'] else None)
        assert m['ori_shape'] == x['img'].shape and tuple(m['img_shape']) == im.shape and m['pad_shape'] == (*hw, 3)
        assert m['keep_ratio'] == info['keep_ratio']
        assert m['scale_factor'].dtype == np.float32 and np.array_equal(m['scale_factor'], info['scale_factor'])
        gb, gl = batch['gt_bboxes'][k].cpu().numpy(), batch['gt_labels'][k].cpu().numpy()
        assert gb.dtype == np.float32 and gb.shape == (len(ll), 4) and np.array_equal(gb, bb)
        assert gl.dtype == np.int64 and gl.shape == (len(ll),) and np.array_equal(gl, ll)
        assert np.array_equal(batch['gt_bboxes_host'][k], bb) and np.array_equal(batch['gt_labels_host'][k], ll)
    return infos


def coverage(seeds):
    """What the helper alone meets over `seeds`: (policy, flip) pairs and, per stage, whether an axis grew and whether one shrank."""
    seen = set()
    for seed in seeds:
        s = samples(seed)
        for x, info in zip(s, DO.det_autoaug_batch(s, np.random.RandomState(seed), POLICIES)[3]):
            seen.add(('policy', info['policy'], info['flip']))
            h, w = x['img'].shape[:2]
            ins = [(w, h)] + [win[2:] for win in info['windows']]
            for stage, ((wi, hi), (wo, ho)) in enumerate(zip(ins, info['sizes'])):
                if info['policy'] == 1:
                    seen.add((stage, 'up' if wo > wi else 'down' if wo < wi else 'same'))
    return seen


def test_seeded_batches_equal_the_helper(cuda):
    """The scaled-down recipe on ragged sources, batches of 3 and 4: both policies under both flip states, each stage of the
    chain both enlarging and reducing; mixed batches (one- and two-stage samples in the one chain launch) come with the draws."""
    want = {('policy', k, f) for k in (0, 1) for f in (False, True)} | {(st, d) for st in (0, 1) for d in ('up', 'down')}
    assert want <= coverage(SEEDS)
    col = P.build_collate('det', pipeline(), cuda)
    mixed = 0
    for seed in SEEDS:
        s = samples(seed)
        infos = _check(col(s, np.random.RandomState(seed)), s, np.random.RandomState(seed), POLICIES)
        mixed += len({i['policy'] for i in infos}) == 2
    assert mixed


def _scripted(policy, flip, crop=None):
    """Single-scale policies make no draw of their own: the stream is the flip, the policy index and the crop's offsets."""
    return [0.1 if flip else 0.9, 0] + list(crop or [])


EDGE_CASES = {
    # name: (source (h, w), first scale, crop (h, w), crop offsets (oy, ox) or 'max', last scale)
    'second_x_block': ((60, 120), (120, 60), (30, 100), (15, 10), (200, 400)),  # Wout = 400 > 256
    'top_left': ((70, 100), (60, 420), (38, 50), (0, 0), (80, 133)),
    'bottom_right': ((70, 100), (60, 420), (38, 50), 'max', (80, 133)),
    'upscaled_frame_bottom_right': ((40, 131), (60, 420), (45, 60), 'max', (48, 133)),  # both stages' last taps clamp
    'one_pixel_wide': ((64, 64), (50, 420), (20, 1), (11, 17), (48, 133)),
    'one_pixel_high': ((97, 61), (40, 420), (1, 30), (33, 5), (64, 133)),
    'reduce_after_crop': ((97, 61), (60, 420), (60, 60), (20, 0), (20, 133)),
}


@pytest.mark.parametrize('flip', [False, True])
@pytest.mark.parametrize('case', sorted(EDGE_CASES))
def test_windows_at_the_frame_edges(cuda, case, flip):
    """Crop windows that touch each edge of frame 1 (the single-tap borders of both stages), crops one pixel wide and high,
    and an output wider than one 256-thread block."""
    (h, w), s1, (ch, cw), offs, s2 = EDGE_CASES[case]
    pol = [[dict(type='Resize', img_scale=[s1], keep_ratio=True),
            dict(type='RandomCrop', crop_type='absolute', crop_size=(ch, cw), allow_negative_crop=True),
            dict(type='Resize', img_scale=[s2], keep_ratio=True, override=True)]]
    r = np.random.RandomState(len(case))
    s = [dict(img=r.randint(0, 256, (h, w, 3)).astype(np.uint8),
              gt_bboxes=np.array([[2, 3, w - 1, h - 2], [0, 0, 4, 4]], np.float32), gt_labels=np.array([5, 7]))]
    f1w, f1h = DO.resize_wh(pol[0][0], h, w, None)
    oy, ox = (f1h - min(ch, f1h), f1w - min(cw, f1w)) if offs == 'max' else offs
    assert oy <= f1h - min(ch, f1h) and ox <= f1w - min(cw, f1w)
    col = P.build_collate('det', pipeline(pol), cuda)
    batch = col(s, Fixed(_scripted(0, flip, (oy, ox))))
    info, = _check(batch, s, Fixed(_scripted(0, flip, (oy, ox))), pol)
    assert info['flip'] == flip and info['windows'] == [(ox, oy, min(cw, f1w), min(ch, f1h))]
    if case == 'second_x_block':
        assert batch['img'].shape[-1] == 400


def _u8_collate(cuda, **kw):
    """A one-stage collate whose output IS the uint8 frame (mean 0, std 1, BGR kept): the oracle's way to a stored frame."""
    return P.DeviceCollate('cls', cuda, flip_prob=0.0, img_norm_cfg=dict(mean=[0., 0., 0.], std=[1., 1., 1.], to_rgb=False), **kw)


def test_chain_launch_is_bit_equal_to_the_two_passes(cuda):
    """Stage 1 into a stored uint8 frame (a one-stage launch, copied to the host), the crop on the host, stage 2 by a second
    one-stage launch on the cropped frame: the chain launch's float32 words are the same."""
    col = P.build_collate('det', pipeline(), cuda)
    chains = 0
    for seed in SEEDS[:2] + SEEDS[-2:]:
        s = samples(seed)
        batch = col(s, np.random.RandomState(seed))
        infos = DO.det_autoaug_batch(s, np.random.RandomState(seed), POLICIES)[3]
        for k, (x, info) in enumerate(zip(s, infos)):
            if info['policy'] != 1:
                continue
            chains += 1
            src = np.ascontiguousarray(x['img'][:, ::-1]) if info['flip'] else x['img']
            (w1, h1), (w2, h2) = info['sizes']
            ox, oy, cw, ch = info['windows'][0]
            f1 = _u8_collate(cuda, resize=dict(size=(h1, w1)))([dict(img=src, gt_label=0)])['img'][0]
            f1 = f1.permute(1, 2, 0).cpu().numpy()
            assert f1.shape == (h1, w1, 3) and np.array_equal(f1, np.rint(f1)) and f1.min() >= 0 and f1.max() <= 255
            crop = np.ascontiguousarray(f1.astype(np.uint8)[oy:oy + ch, ox:ox + cw])
            two = P.DeviceCollate('cls', cuda, flip_prob=0.0, resize=dict(size=(h2, w2)))([dict(img=crop, gt_label=0)])['img'][0]
            got = batch['img'][k]
            assert torch.equal(got[:, :h2, :w2].contiguous().view(torch.int32), two.contiguous().view(torch.int32))
            assert not got[:, h2:].any() and not got[:, :, w2:].any()
    assert chains >= 4


def test_same_seed_same_batch_and_empty_batch(cuda):
    col = P.build_collate('det', pipeline(), cuda)
    s = samples(1)
    a, b = col(s, np.random.RandomState(3)), col(s, np.random.RandomState(3))
    assert torch.equal(a['img'].view(torch.int32), b['img'].view(torch.int32))
    for k in ('gt_bboxes', 'gt_labels'):
        assert all(torch.equal(u, v) for u, v in zip(a[k], b[k]))
    e = col([], np.random.RandomState(0))
    assert e['img'].shape[0] == 0 and e['img_metas'] == [] and e['gt_bboxes'] == [] and e['gt_labels'] == []


def test_chain_entry_arguments(cuda):
    from rscotr_amd._lib import lib
    f = (ctypes.c_float * 3)(1, 1, 1)
    z = (ctypes.c_float * 3)(1, 0, 1)
    p, pz = ctypes.cast(f, ctypes.c_void_p), ctypes.cast(z, ctypes.c_void_p)
    lib.call('rscotr_img_aug_chain_u8', 0, 0, 0, 0, 0, 8, 8, p, p, 1, 0)  # B = 0: nothing to do
    t = torch.zeros(256, dtype=torch.uint8, device=cuda)
    d = t.data_ptr()
    for args in [(d, d, d, d, 1, 4, 4, p, pz, 1, 0),      # std <= 0
                 (d, d, d, d, -1, 4, 4, p, p, 1, 0),      # negative B
                 (d, d, 0, d, 1, 4, 4, p, p, 1, 0),       # no tables
                 (d, d, d, d, 1, 4, 4, 0, p, 1, 0),       # no mean
                 (d, d, d, d, 1, 70000, 4, p, p, 1, 0)]:  # Hout beyond the grid
        with pytest.raises(RuntimeError, match='rscotr_img_aug_chain_u8'):
            lib.call('rscotr_img_aug_chain_u8', *args)


def test_one_launch_per_batch(cuda):
    """A batch with a two-stage sample is ONE chain launch; a batch of one-stage samples is the table route's one launch."""
    from rscotr_amd._lib import lib
    names, real = [], lib.call

    def spy(name, *args):
        names.append(name)
        return real(name, *args)
    lib.call = spy
    try:
        P.build_collate('det', pipeline(), cuda)(samples(0), np.random.RandomState(0))
        P.build_collate('det', pipeline(POLICIES[:1]), cuda)(samples(0), np.random.RandomState(0))
    finally:
        del lib.call
    assert names == ['rscotr_img_aug_chain_u8', 'rscotr_img_aug_u8']


def test_train_step_on_an_autoaugment_batch(cuda):
    """One det train_step of the tiny model on an AutoAugment batch in which one image lost every box to its crop and the canvas
    is ragged: finite losses, and the same losses from a second identical run."""
    from util import build_model, load_model_cfg
    from rscotr_amd import synth
    s = samples(STEP_SEED)
    infos = DO.det_autoaug_batch(s, np.random.RandomState(STEP_SEED), POLICIES)
    assert any(len(ll) == 0 for ll in infos[2]) and any(len(ll) > 0 for ll in infos[2])
    assert any(im.shape[:2] != infos[4] for im in infos[0])
    cfg, mcfg = load_model_cfg(tiny=True)
    model = build_model(mcfg).to(cuda)
    col = P.build_collate('det', pipeline(), cuda)

    def once():
        batch = dict(col(s, np.random.RandomState(STEP_SEED)), task='det', dataset_name=synth.TASK_DATASET['det'])
        assert [len(l) for l in batch['gt_labels']] == [len(ll) for ll in infos[2]]
        cpu = dict(batch, img=batch['img'].cpu(), gt_labels=[l.cpu() for l in batch['gt_labels']])
        rnd = synth.make_rnd(model, cpu, seed=STEP_SEED, device=cuda)
        model.zero_grad(set_to_none=True)
        out = model.train_step(dict(batch, rnd=rnd))
        out['loss'].backward()
        torch.cuda.synchronize()
        return out
    a, b = once(), once()
    assert torch.isfinite(a['loss']) and all(np.isfinite(v) for v in a['log_vars'].values())
    assert a['log_vars'] == b['log_vars'] and torch.equal(a['loss'], b['loss'])
