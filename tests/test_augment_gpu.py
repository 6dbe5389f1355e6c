"""Device resampling / photometric / erasing stages of the input collate (rscotr_img_aug_u8, rscotr_seg_label_aug_u8) against
the NumPy restatement of the mm* transforms (tests/aug_oracle.py) on the same seeded draws: images within 1e-6 * max|ref|
(one LSB of the uint8 stage is ~0.017 after Normalize, so the uint8 values must be exact), label maps, metas, scale factors
and boxes exact."""
import ctypes
import os

import numpy as np
import pytest
import torch

import aug_oracle as AO
from oracle import pipeline as OP
from rscotr_amd import pipeline as P
from rscotr_amd.pipeline import resample as R

pytestmark = pytest.mark.gpu
MEAN, STD = P.IMG_NORM['mean'], P.IMG_NORM['std']
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'aug_pil_bicubic.npz')


def _close(got, ref):
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.abs(got - ref).max() <= 1e-6 * max(np.abs(ref).max(), 1.0)


def _seg_samples(rng, n, hw=(512, 512)):
    out = []
    for _ in range(n):
        h, w = hw
        img = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
        lab = np.repeat(np.repeat(rng.randint(0, 7, (h // 16 + 1, w // 16 + 1)), 16, 0), 16, 1)[:h, :w].astype(np.uint8)
        out.append(dict(img=img, gt_semantic_seg=lab))
    return out


@pytest.mark.parametrize('ratio', [0.5, 2.0])
@pytest.mark.parametrize('seed', [0, 1])
def test_seg_resize_crop_photometric(cuda, ratio, seed):
    """Ratio 0.5: a 256^2 tile padded to 512^2; ratio 2.0: 1024^2 cropped to 512^2 (cat_max_ratio retries on the resized
    label map); PhotoMetricDistortion on, its steps drawn on and off over the batch."""
    s = _seg_samples(np.random.RandomState(seed), 4)
    col = P.train_collate_for('seg', cuda, resize=dict(img_scale=(512, 512), ratio_range=(ratio, ratio)))
    b = col(s, np.random.RandomState(seed + 100))
    r = np.random.RandomState(seed + 100)
    ims, labs = [], []
    for x, m in zip(s, b['img_metas']):
        im, lb, om = AO.seg_sample(x['img'], x['gt_semantic_seg'], r, ratio_range=(ratio, ratio))
        ims.append(im)
        labs.append(lb)
        assert m['flip'] == om['flip'] and tuple(m['img_shape']) == om['img_shape'] and m['keep_ratio']
        assert m['scale_factor'].dtype == np.float32 and (m['scale_factor'] == om['scale_factor']).all()
        assert m['pad_shape'] == (512, 512, 3)
    if ratio == 0.5:
        assert all(m['img_shape'] == (256, 256, 3) for m in b['img_metas'])
    _close(b['img'], AO.collate_images(ims, (512, 512), MEAN, STD))
    lref = OP.prepare_seg_labels(labs, [(0, 0, l.shape[1], l.shape[0]) for l in labs], [False] * 4, (512, 512), True, 5)
    assert (b['gt_semantic_seg'].cpu().numpy() == lref).all()


def test_photometric_every_step_on_and_off(cuda):
    """Every step of PhotoMetricDistortion, each forced on and off, in both modes (contrast first / last), per pixel against
    the oracle's restated cv2 HSV conversions: the draws are fixed by replacing the collate's draw with fixed values."""
    rng = np.random.RandomState(7)
    img = rng.randint(0, 256, (48, 64, 3)).astype(np.uint8)
    img[:8] = img[:8, :, :1]  # grey rows (saturation 0)
    img[8:16, :, 0] = img[8:16, :, 2]  # ties of the max channel
    cases = []
    for mode in (0, 1):
        for bright in (0, 1):
            for con in (0, 1):
                for sat in (0, 1):
                    for hue in (0, 1):
                        cases.append((mode, bright, con, sat, hue))
    col = P.DeviceCollate('seg', cuda, flip_prob=0.0, photometric=True)
    samples = [dict(img=img, gt_semantic_seg=np.zeros(img.shape[:2], np.uint8)) for _ in cases]
    ref_ims = []
    draws = []
    for k, (mode, bright, con, sat, hue) in enumerate(cases):
        beta, ca, sa, hd = -31.7 + k, 0.5 + k / 40, 1.49 - k / 40, k - 18
        # the values a RandomState would hand PhotoMetricDistortion, in its order
        seq = [bright] + ([beta] if bright else []) + [mode]
        cseq = [con] + ([ca] if con else [])
        seq += cseq if mode == 1 else []
        seq += [sat] + ([sa] if sat else []) + [hue] + ([hd] if hue else [])
        seq += cseq if mode == 0 else []
        draws.append(seq)

        class Fixed:
            def __init__(self, seq):
                self.seq = list(seq)

            def randint(self, *a):
                return self.seq.pop(0)

            def uniform(self, *a):
                return self.seq.pop(0)

            def rand(self):
                return 1.0
        ref_ims.append(AO.photometric(img, Fixed(seq)))
    seq_all = [v for d in draws for v in ([1.0] + d)]  # each sample: the flip draw (rand) first

    class Stream:
        def rand(self):
            return seq_all.pop(0)

        def randint(self, *a):
            return seq_all.pop(0)

        def uniform(self, *a):
            return seq_all.pop(0)
    b = col(samples, Stream())
    assert not seq_all
    _close(b['img'], AO.collate_images(ref_ims, (48, 64), MEAN, STD))
    assert not all((r == img).all() for r in ref_ims[1:])


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_cls_random_resized_crop_bicubic_and_erasing(cuda, seed):
    """RandomResizedCrop(224, bicubic, pillow) + flip + RandomErasing(0.25, 'rand') on 256^2 tiles; a 300 x 20 strip forces
    the central-crop fallback; crops at the image border come from the draws."""
    rng = np.random.RandomState(seed)
    s = [dict(img=rng.randint(0, 256, (256, 256, 3)).astype(np.uint8), gt_label=k) for k in range(7)]
    s.append(dict(img=rng.randint(0, 256, (20, 300, 3)).astype(np.uint8), gt_label=1))
    col = P.train_collate_for('cls', cuda)
    b = col(s, np.random.RandomState(seed + 5))
    r = np.random.RandomState(seed + 5)
    ims, crops = [], []
    for x, m in zip(s, b['img_metas']):
        im, om = AO.cls_sample(x['img'], r, erasing=P.CLS_ERASING)
        ims.append(im)
        crops.append(om['crop'])
        assert m['flip'] == om['flip'] and (m['scale_factor'] == om['scale_factor']).all()
    assert crops[-1] == (136, 0, 27, 20)  # fallback: th = 20, tw = round(20 * 4 / 3), centred
    _close(b['img'], AO.collate_images(ims, (224, 224), MEAN, STD))
    assert b['gt_label'].tolist() == [x['gt_label'] for x in s]


def test_cls_erasing_always_and_never(cuda):
    rng = np.random.RandomState(3)
    s = [dict(img=rng.randint(0, 256, (256, 256, 3)).astype(np.uint8), gt_label=0) for _ in range(4)]
    for prob in (1.0, 0.0):
        er = dict(P.CLS_ERASING, erase_prob=prob)
        b = P.train_collate_for('cls', cuda, random_erasing=er)(s, np.random.RandomState(9))
        r = np.random.RandomState(9)
        ims = [AO.cls_sample(x['img'], r, erasing=er)[0] for x in s]
        _close(b['img'], AO.collate_images(ims, (224, 224), MEAN, STD))


def test_cls_eval_resize_matches_committed_pillow_outputs(cuda):
    """backend='pillow' bicubic against Pillow outputs committed under tests/golden (up and down, anisotropic)."""
    g = np.load(GOLDEN)
    for i in range(4):
        src, dst = g[f'src{i}'], g[f'dst{i}']
        col = P.eval_collate_for('cls', cuda, resize=dict(size=dst.shape[:2]))
        b = col([dict(img=src, gt_label=0)])
        _close(b['img'], AO.collate_images([dst], dst.shape[:2], MEAN, STD))


@pytest.mark.parametrize('seed', [0, 1])
def test_det_keep_ratio_resize_boxes_and_scale_factor(cuda, seed):
    rng = np.random.RandomState(seed)
    s = []
    for h, w in ((700, 1000), (333, 517)):  # not 800 on the short side
        k = 5
        x1, y1 = rng.uniform(0, w / 2, k), rng.uniform(0, h / 2, k)
        bb = np.stack([x1, y1, x1 + rng.uniform(2, w, k), y1 + rng.uniform(2, h, k)], -1).astype(np.float32)  # some cross
        s.append(dict(img=rng.randint(0, 256, (h, w, 3)).astype(np.uint8), gt_bboxes=bb, gt_labels=rng.randint(0, 20, k)))
    b = P.train_collate_for('det', cuda)(s, np.random.RandomState(seed + 3))
    r = np.random.RandomState(seed + 3)
    ims = []
    for x, m, gb in zip(s, b['img_metas'], b['gt_bboxes_host']):
        im, bb, om = AO.det_sample(x['img'], x['gt_bboxes'], r)
        ims.append(im)
        assert m['flip'] == om['flip'] and tuple(m['img_shape']) == om['img_shape'] and m['keep_ratio']
        assert (m['scale_factor'] == om['scale_factor']).all() and (gb == bb).all()
    assert b['img_metas'][0]['img_shape'][:2] == (800, 1143)
    H, W = b['img'].shape[-2:]
    assert H % 32 == 0 and W % 32 == 0
    _close(b['img'], AO.collate_images(ims, (H, W), MEAN, STD))


def test_det_rescale_decoding_uses_the_scale_factor(cuda):
    """simple_test(rescale=True) of an eval_collate_for('det') batch returns the rescale=False boxes / scale_factor."""
    from util import build_model, load_model_cfg
    rng = np.random.RandomState(0)
    cfg, mcfg = load_model_cfg(tiny=True)
    model = build_model(mcfg).to(cuda).eval()
    col = P.eval_collate_for('det', cuda, resize=dict(img_scale=(160, 96)))
    b = col([dict(img=rng.randint(0, 256, (70, 100, 3)).astype(np.uint8), gt_bboxes=np.zeros((0, 4), np.float32),
                  gt_labels=np.zeros(0, np.int64))])
    m = b['img_metas'][0]
    assert m['img_shape'][:2] == (96, 137) and m['scale_factor'].tolist() == pytest.approx([1.37, 96 / 70, 1.37, 96 / 70])
    with torch.no_grad():
        a = model.simple_test('det', b['img'], [dict(m)], rescale=False)[0]
        c = model.simple_test('det', b['img'], [dict(m)], rescale=True)[0]
    for ka, kc in zip(a, c):
        if len(ka):
            np.testing.assert_allclose(kc[:, :4], ka[:, :4] / m['scale_factor'], rtol=1e-6, atol=1e-4)


@pytest.mark.parametrize('backend', ['cv2', 'pillow'])
@pytest.mark.parametrize('src_hw, dst_hw', [((1, 1), (5, 7)), ((1, 9), (4, 3)), ((9, 1), (2, 6)), ((16, 24), (8, 12)),
                                            ((5, 6), (5, 13)), ((3, 40), (1, 1))])
def test_resample_edge_shapes(cuda, backend, src_hw, dst_hw):
    """1 x 1 and 1 x N sources, an exact 2x downscale, single-tap borders (upscales), a 1 x 1 output."""
    rng = np.random.RandomState(sum(src_hw) + sum(dst_hw))
    img = rng.randint(0, 256, src_hw + (3,)).astype(np.uint8)
    col = P.DeviceCollate('cls', cuda, flip_prob=0.0, resize=dict(size=dst_hw), resize_backend=backend)
    b = col([dict(img=img, gt_label=0)])
    ref = AO.resize_img(img, dst_hw[1], dst_hw[0], backend)
    _close(b['img'], AO.collate_images([ref], dst_hw, MEAN, STD))


def test_label_nearest_and_flip(cuda):
    rng = np.random.RandomState(4)
    img = rng.randint(0, 256, (33, 47, 3)).astype(np.uint8)
    lab = rng.randint(0, 7, (33, 47)).astype(np.uint8)
    col = P.DeviceCollate('seg', cuda, flip_prob=1.0, resize=dict(img_scale=(94, 66)), reduce_zero_label=True, seg_pad_val=5,
                          size_divisor=32)
    b = col([dict(img=img, gt_semantic_seg=lab)], np.random.RandomState(0))
    assert b['img_metas'][0]['img_shape'] == (66, 94, 3)
    want = OP.imflip(OP.reduce_zero_label(AO.resize_nearest(lab, 94, 66).astype(np.int64)))
    assert (b['gt_semantic_seg'][0, 0, :66, :94].cpu().numpy() == want).all()
    assert (b['gt_semantic_seg'][0, 0, 66:].cpu().numpy() == 5).all() and b['img'].shape[-2:] == (96, 96)
    _close(b['img'], AO.collate_images([OP.imflip(AO.resize_bilinear(img, 94, 66))], (96, 96), MEAN, STD))


def test_all_stages_off_equals_img_prep_bitwise(cuda):
    """rscotr_img_aug_u8 over identity nearest entries with every stage off = rscotr_img_prep_u8, bit for bit."""
    from rscotr_amd._lib import lib
    rng = np.random.RandomState(1)
    B, H, W, Hout, Wout = 3, 37, 53, 40, 64
    src = torch.from_numpy(rng.randint(0, 256, (B, H, W, 3)).astype(np.uint8)).to(cuda)
    wins = [(3, 5, 31, 29), (0, 0, 53, 37), (10, 2, 40, 30)]
    flips = [1, 0, 1]
    meta = torch.tensor([[b * H * W * 3, H, W, W * 3, *wins[b], flips[b], 0] for b in range(B)], dtype=torch.int64,
                        device=cuda)
    tabs, ameta, n = [], [], 0
    for b, (x0, y0, cw, ch) in enumerate(wins):
        xt = R._axis_nearest(W, W, 0, x0, cw)
        yt = R._axis_nearest(H, H, 0, y0, ch)
        ameta.append([b * H * W * 3, H, W, W * 3, cw, ch, flips[b], n, n + xt.size, 1, 1, 0] + [0] * 8)
        tabs += [xt.reshape(-1), yt.reshape(-1)]
        n += xt.size + yt.size
    tab = torch.from_numpy(np.concatenate(tabs)).to(cuda)
    am = torch.tensor(ameta, dtype=torch.int64, device=cuda)
    prm = torch.zeros((B, 4), dtype=torch.float32, device=cuda)
    m = (ctypes.c_float * 3)(*MEAN)
    s = (ctypes.c_float * 3)(*STD)
    mp, sp = ctypes.cast(m, ctypes.c_void_p), ctypes.cast(s, ctypes.c_void_p)
    a = torch.full((B, 3, Hout, Wout), 7.0, device=cuda)
    c = torch.full((B, 3, Hout, Wout), -7.0, device=cuda)
    st = torch.cuda.current_stream().cuda_stream
    lib.call('rscotr_img_prep_u8', src.data_ptr(), meta.data_ptr(), a.data_ptr(), B, Hout, Wout, mp, sp, 1, st)
    lib.call('rscotr_img_aug_u8', src.data_ptr(), am.data_ptr(), tab.data_ptr(), prm.data_ptr(), c.data_ptr(), B, Hout, Wout,
             mp, sp, 1, st)
    assert torch.equal(a.view(torch.int32), c.view(torch.int32))


def test_plain_route_equals_table_route_with_a_do_nothing_stage(cuda):
    """One host plan under both launches: the same seeded batch through the plain route (rscotr_img_prep_u8 /
    rscotr_seg_label_prep_u8) and through the table route with a resize to the image's own size (nearest identity entries, no
    extra draw) is the same batch bit for bit.  The crop is narrower than the image one way and wider the other (crop and pad)."""
    r = np.random.RandomState(4)
    seg = [dict(img=r.randint(0, 256, (37, 53, 3)).astype(np.uint8), gt_semantic_seg=r.randint(0, 7, (37, 53)).astype(np.uint8),
                gt_label=int(r.randint(0, 45))) for _ in range(3)]
    kw = dict(crop_size=(24, 64), cat_max_ratio=0.75, reduce_zero_label=True, seg_pad_val=5)
    a = P.DeviceCollate('seg', cuda, **kw)(seg, np.random.RandomState(9))
    b = P.DeviceCollate('seg', cuda, resize=dict(size=(37, 53)), **kw)(seg, np.random.RandomState(9))
    assert a['img'].shape == (3, 3, 24, 64) and torch.equal(a['img'].view(torch.int32), b['img'].view(torch.int32))
    assert torch.equal(a['gt_semantic_seg'], b['gt_semantic_seg'])
    for k in ('flip', 'img_shape', 'pad_shape'):
        assert [m[k] for m in a['img_metas']] == [m[k] for m in b['img_metas']]
    a = P.DeviceCollate('cls', cuda)(seg, np.random.RandomState(9))
    b = P.DeviceCollate('cls', cuda, resize=dict(size=(37, 53)))(seg, np.random.RandomState(9))
    assert a['img'].shape == (3, 3, 37, 53) and torch.equal(a['img'].view(torch.int32), b['img'].view(torch.int32))
    assert torch.equal(a['gt_label'], b['gt_label'])


def test_same_seed_same_batch(cuda):
    s = _seg_samples(np.random.RandomState(2), 3, (300, 400))
    col = P.train_collate_for('seg', cuda)
    a = col(s, np.random.RandomState(11))
    b = col(s, np.random.RandomState(11))
    assert torch.equal(a['img'].view(torch.int32), b['img'].view(torch.int32))
    assert torch.equal(a['gt_semantic_seg'], b['gt_semantic_seg'])


def test_empty_batch_and_bad_arguments(cuda):
    from rscotr_amd._lib import lib
    f = (ctypes.c_float * 3)(1, 1, 1)
    z = (ctypes.c_float * 3)(1, 0, 1)
    p, pz = ctypes.cast(f, ctypes.c_void_p), ctypes.cast(z, ctypes.c_void_p)
    lib.call('rscotr_img_aug_u8', 0, 0, 0, 0, 0, 0, 8, 8, p, p, 1, 0)  # B = 0: nothing to do
    lib.call('rscotr_seg_label_aug_u8', 0, 0, 0, 0, 0, 8, 8, 0, 255, 0)
    t = torch.zeros(256, dtype=torch.uint8, device=cuda)
    d = t.data_ptr()
    for args in [(d, d, d, d, d, 1, 4, 4, p, pz, 1, 0),      # std <= 0
                 (d, d, d, d, d, -1, 4, 4, p, p, 1, 0),      # negative B
                 (d, d, 0, d, d, 1, 4, 4, p, p, 1, 0),       # no tables
                 (d, d, d, d, d, 1, 4, 4, 0, p, 1, 0)]:      # no mean
        with pytest.raises(RuntimeError):
            lib.call('rscotr_img_aug_u8', *args)
    with pytest.raises(RuntimeError):
        lib.call('rscotr_seg_label_aug_u8', d, d, 0, d, 1, 4, 4, 0, 255, 0)
    b = P.train_collate_for('cls', cuda)([], np.random.RandomState(0))
    assert b['img'].shape[0] == 0 and b['img_metas'] == []
    with pytest.raises(ValueError):
        P.DeviceCollate('cls', cuda, resize_backend='lanczos')


def test_train_collate_loaders_feed_a_train_step(cuda, tmp_path):
    """PNG tiles -> DeviceLoader(train_collate_for) -> MultiDataLoader -> MTL.train_step (seg, tiny model, 128^2 crops)."""
    from PIL import Image
    from util import build_model, load_model_cfg
    from rscotr_amd import data as D
    rng = np.random.RandomState(0)
    os.makedirs(tmp_path / 'img')
    os.makedirs(tmp_path / 'ann')
    for k in range(4):
        Image.fromarray(rng.randint(0, 256, (150, 140, 3)).astype(np.uint8)).save(tmp_path / 'img' / f't{k}.png')
        Image.fromarray(rng.randint(0, 7, (150, 140)).astype(np.uint8)).save(tmp_path / 'ann' / f't{k}.png')
    ds = P.TileSegDataset(str(tmp_path / 'img'), str(tmp_path / 'ann'))
    col = P.train_collate_for('seg', cuda, crop_size=(128, 128), resize=dict(img_scale=(128, 128), ratio_range=(0.5, 2.0)))
    loaders = dict(potsdam=P.DeviceLoader(ds, col, batch_size=2, seed=1))
    m = D.MultiDataLoader(loaders, D.RoundRobinIterationStrategy(loaders))
    batch = next(iter(m))
    assert batch['task'] == 'seg' and batch['img'].shape == (2, 3, 128, 128)
    cfg, mcfg = load_model_cfg(tiny=True)
    model = build_model(mcfg).to(cuda)
    out = model.train_step(batch)
    assert torch.isfinite(out['loss'])
