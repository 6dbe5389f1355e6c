"""Detection evaluation on the device (csrc/det_eval.hip): `ops.det_decode` against DINOHead._get_bboxes_single's chain run in
fp32 on the CPU (labels and boxes bit-equal), `ops.det_match` against the packing of the host's `_evaluate_img` (bit-equal),
neither synchronising with the host, and the model + engine route `single_gpu_test(det=dict(on_device=True))` whose
`evaluate` equals `coco_bbox_map` on the same detections."""
import json
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from test_det_eval_cpu import CLASSES, K as MATCH_K, host_flags, match_cases
from rscotr_amd import ops
from rscotr_amd.metrics import coco_area_ranges, coco_bbox_map, coco_iou_thrs
from util import build_model, load_model_cfg

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------------------ decode
def _decode_inputs(B, Q, C, K, seed):
    """Logits: a seeded permutation of linspace(-6, 6) per image; box centres spread so that some corners leave the image;
    a different non-square img_shape per image, w_scale != h_scale."""
    g = torch.Generator().manual_seed(seed)
    N = Q * C
    lin = torch.linspace(-6, 6, N)
    cls = torch.stack([lin[torch.randperm(N, generator=g)] for _ in range(B)]).view(B, Q, C)
    box = torch.cat([torch.rand((B, Q, 2), generator=g) * 1.2 - 0.1, torch.rand((B, Q, 2), generator=g) * 0.5 + 0.01], -1)
    metas = [dict(img_shape=(480 + 37 * i, 640 - 53 * i, 3),
                  scale_factor=np.array([1.25 + 0.1 * i, 0.9375 - 0.05 * i, 1.25 + 0.1 * i, 0.9375 - 0.05 * i], np.float32))
             for i in range(B)]
    # the expected order is unambiguous: the fp32 CPU sigmoids of the top K + 1 logits are pairwise distinct
    for b in range(B):
        top = cls[b].sigmoid().view(-1).topk(min(K + 1, N))[0]
        assert top.unique().numel() == top.numel(), 'pick another seed: tied scores among the top K + 1'
    return cls, box, metas


def _meta_table(metas, device):
    return torch.tensor([[m['img_shape'][0], m['img_shape'][1], *m['scale_factor'].tolist()] for m in metas],
                        dtype=torch.float32).to(device)


def _cpu_chain(cls, box, metas, K, rescale):
    """DINOHead._get_bboxes_single itself, on CPU tensors in fp32."""
    from rscotr_amd.det_head import DINOHead
    stub = SimpleNamespace(test_cfg=dict(max_per_img=K), num_query=cls.shape[1], num_classes=cls.shape[2])
    out = [DINOHead._get_bboxes_single(stub, cls[b], box[b], m['img_shape'], m['scale_factor'], rescale)
           for b, m in enumerate(metas)]
    return torch.stack([d for d, _ in out]), torch.stack([l for _, l in out])


def _sigmoid_bound(cls, cuda):
    """Twice the largest |torch device sigmoid - fp64 sigmoid| on these logits (same formula; the factor allows another exp)."""
    return 2.0 * float((cls.to(cuda).sigmoid().cpu().double() - cls.double().sigmoid()).abs().max())


@pytest.mark.parametrize('rescale', [False, True])
@pytest.mark.parametrize('shape', [(2, 37, 5, 16), (2, 8, 2, 16), (3, 600, 20, 300)])
def test_decode_against_the_cpu_chain(cuda, shape, rescale):
    B, Q, C, K = shape
    cls, box, metas = _decode_inputs(B, Q, C, K, seed=3)
    want_d, want_l = _cpu_chain(cls, box, metas, K, rescale)
    assert (want_d[..., :4] == 0).any() and (want_d[..., 0] > 0).any()  # (the clamps act, and not everywhere)
    dets, labels = ops.det_decode(cls.to(cuda), box.to(cuda), _meta_table(metas, cuda), K, rescale)
    again = ops.det_decode(cls.to(cuda), box.to(cuda), _meta_table(metas, cuda), K, rescale)
    assert dets.shape == (B, K, 5) and labels.shape == (B, K) and labels.dtype == torch.int64
    assert torch.equal(dets, again[0]) and torch.equal(labels, again[1])
    dets, labels = dets.cpu(), labels.cpu()
    assert torch.equal(labels, want_l)
    assert torch.equal(dets[..., :4].view(torch.int32), want_d[..., :4].contiguous().view(torch.int32))  # bit-equal boxes
    bound = _sigmoid_bound(cls, cuda)
    err = float((dets[..., 4].double() - torch.gather(cls.view(B, -1), 1, _flat_index(cls, want_d, want_l)).double().sigmoid())
                .abs().max())
    print(f'det_decode {shape} rescale={rescale}: score error {err:.3e}, bound {bound:.3e}')
    assert err <= bound


def _flat_index(cls, want_d, want_l):
    """Flat (query, class) index of every expected row, recovered from the CPU top-k."""
    B, Q, C = cls.shape
    return torch.stack([cls[b].sigmoid().view(-1).topk(want_l.shape[1])[1] for b in range(B)])


def test_decode_ties_saturation_and_limits(cuda):
    B, Q, C, K = 2, 9, 5, 7
    box = torch.rand((B, Q, 4), generator=torch.Generator().manual_seed(1)).to(cuda)
    meta = torch.tensor([[100., 200., 1, 1, 1, 1]] * B).to(cuda)
    # all-equal logits: flat indices 0 .. K - 1
    dets, labels = ops.det_decode(torch.full((B, Q, C), 0.25, device=cuda), box, meta, K, False)
    assert labels.cpu().tolist() == [[i % C for i in range(K)]] * B
    assert torch.equal(dets.cpu()[..., :4], _boxes_of(box.cpu(), [[i // C for i in range(K)]] * B, 100, 200))
    # logits >= 20 saturate to 1.0f: taken in index order, before any smaller score
    cls = torch.linspace(-3, 3, Q * C).repeat(B, 1)
    sat = [41, 3, 17, 30]
    cls[:, sat] = torch.tensor([20., 25., 31., 88.])
    cls[1, 44] = 10.0  # (large, not saturated: after the four)
    dets, labels = ops.det_decode(cls.view(B, Q, C).to(cuda), box, meta, K, False)
    flat = [sorted(sat) + [44, 43, 42]] * B
    assert labels.cpu().tolist() == [[i % C for i in f] for f in flat]
    assert (dets[:, :4, 4] == 1.0).all() and (dets[:, 4:, 4] < 1.0).all()
    assert torch.equal(dets.cpu()[..., :4], _boxes_of(box.cpu(), [[i // C for i in f] for f in flat], 100, 200))
    # limits: the op raises, nothing is launched
    with pytest.raises(RuntimeError, match='rscotr_det_decode_f32'):
        ops.det_decode(cls.view(B, Q, C).to(cuda), box, meta, Q * C + 1, False)
    big_q = 36864 // 4 + 1
    with pytest.raises(RuntimeError, match='rscotr_det_decode_f32'):
        ops.det_decode(torch.zeros((1, big_q, 4), device=cuda), torch.zeros((1, big_q, 4), device=cuda), meta[:1], 10, False)
    assert ops.det_decode_fits(600, 20, 300) and not ops.det_decode_fits(big_q, 4, 10) and not ops.det_decode_fits(9, 5, 46)


def _boxes_of(box, queries, img_h, img_w):
    b = ops.bbox_cxcywh_to_xyxy(torch.stack([box[i][torch.tensor(q)] for i, q in enumerate(queries)]))
    b[..., 0::2] = (b[..., 0::2] * img_w).clamp(min=0, max=img_w)
    b[..., 1::2] = (b[..., 1::2] * img_h).clamp(min=0, max=img_h)
    return b


def test_head_keeps_the_torch_chain_outside_the_limits(cuda):
    """DINOHead.get_bboxes_device (what simple_test_det(on_device=True) calls) with Q * C > 36864: the torch chain's rows."""
    from rscotr_amd.det_head import DINOHead
    Q, C, K = 1900, 20, 12
    cls, box, metas = _decode_inputs(2, Q, C, K, seed=5)
    stub = SimpleNamespace(test_cfg=dict(max_per_img=K), num_query=Q, num_classes=C)
    stub._get_bboxes_single = lambda *a, **k: DINOHead._get_bboxes_single(stub, *a, **k)
    stub.get_bboxes = lambda *a, **k: DINOHead.get_bboxes(stub, *a, **k)
    got = DINOHead.get_bboxes_device(stub, cls[None].to(cuda), box[None].to(cuda), None, None, metas, rescale=True)
    want_d, want_l = _cpu_chain(cls, box, metas, K, True)
    assert len(got) == 2 and all(d.is_cuda and l.is_cuda for d, l in got)
    assert torch.equal(torch.stack([l for _, l in got]).cpu(), want_l)
    assert torch.equal(torch.stack([d for d, _ in got]).cpu()[..., :4], want_d[..., :4])


# ------------------------------------------------------------------------------------------------------------- match
@pytest.fixture(scope='module')
def cases():
    return match_cases()


def _match_inputs(cases, cuda):
    dets, labels, n_det, gb, gl = cases
    off = np.concatenate([[0], np.cumsum([len(l) for l in gl])]).astype(np.int64)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    return [up(dets), up(labels), up(n_det), up(np.concatenate(gb)), up(np.concatenate(gl)), up(off), up(coco_area_ranges())]


@pytest.mark.parametrize('iou_thrs,max_det', [(None, 100), (None, 3), ([0.5], 3), ([0.75], 100)])
def test_match_is_the_hosts_evaluate_img(cuda, cases, iou_thrs, max_det):
    dets, labels, n_det, gb, gl = cases
    want_f, want_n = host_flags(dets, labels, n_det, gb, gl, iou_thrs, max_det)
    args = _match_inputs(cases, cuda)
    thrs = torch.from_numpy(coco_iou_thrs(iou_thrs)).to(cuda)
    flags, npig = ops.det_match(*args, thrs, len(CLASSES), max_det)
    again = ops.det_match(*args, thrs, len(CLASSES), max_det)
    assert flags.dtype == torch.int32 and tuple(flags.shape) == (3, MATCH_K, 4) and tuple(npig.shape) == (3, 4, 4)
    assert torch.equal(flags, again[0]) and torch.equal(npig, again[1])
    assert np.array_equal(npig.cpu().numpy(), want_n)
    got = flags.cpu().numpy()
    bad = np.argwhere(got != want_f)
    assert len(bad) == 0, [(tuple(i), hex(got[tuple(i)] & 0xffffffff), hex(want_f[tuple(i)] & 0xffffffff)) for i in bad[:8]]


def test_match_equal_iou_takes_the_later_ground_truth(cuda, cases):
    """The detection [10, 10, 30, 30] has IoU 0.5 with two ground truths and must take the later one: the detection that
    overlaps only the earlier one ([10, 11, 30, 21], lower score) then still finds it free at 0.5."""
    dets, labels, n_det, gb, gl = cases
    args = _match_inputs(cases, cuda)
    flags, _ = ops.det_match(*args, torch.from_numpy(coco_iou_thrs([0.5])).to(cuda), len(CLASSES), 100)
    row = lambda b: int(np.nonzero((dets[0, :, :4] == np.float32(b)).all(1))[0][0])
    first, second = row([10, 10, 30, 30]), row([10, 11, 30, 21])
    assert first < second and labels[0, first] == labels[0, second] == 0  # (the two-way detection has the higher score)
    want = host_flags(dets, labels, n_det, gb, gl, [0.5], 100)[0]
    assert flags[0, first, 0].item() == want[0, first, 0] and flags[0, second, 0].item() == want[0, second, 0]
    assert flags[0, first, 0].item() & 1 and flags[0, second, 0].item() & 1


def test_ground_truth_cap_takes_the_host_route(cuda, tmp_path):
    """More than ops.DET_MATCH_MAX_GT ground truths of one class in one image: pre_eval returns the list kind."""
    from rscotr_amd.pipeline import CocoDetDataset
    n = ops.DET_MATCH_MAX_GT + 1
    images = [dict(id=0, file_name='0.png', width=4000, height=4000)]
    anns = [dict(id=i, image_id=0, category_id=1, bbox=[3 * (i % 64), 3 * (i // 64), 2, 2], iscrowd=0) for i in range(n)]
    cats = [dict(id=1, name='a'), dict(id=2, name='b')]
    (tmp_path / 'big.json').write_text(json.dumps(dict(images=images, annotations=anns, categories=cats)))
    (tmp_path / 'ok.json').write_text(json.dumps(dict(images=images, annotations=anns[:-1], categories=cats)))
    dets = torch.tensor([[[0., 0, 2, 2, 0.9], [3., 0, 5, 2, 0.8]]], device=cuda)
    labels = torch.tensor([[0, 1]], device=cuda)
    big = CocoDetDataset(str(tmp_path / 'big.json'), str(tmp_path), classes=('a', 'b'))
    out = big.pre_eval(dets, labels, [0])
    assert not big.device_eval_ok() and isinstance(out[0], list) and len(out[0]) == 2 and out[0][0].shape == (1, 5)
    ok = CocoDetDataset(str(tmp_path / 'ok.json'), str(tmp_path), classes=('a', 'b'))
    out = ok.pre_eval(dets, labels, [0])
    assert ok.device_eval_ok() and isinstance(out[0], tuple) and len(out[0]) == 4 and all(t.is_cuda for t in out[0])
    # at the cap itself the kernel still agrees with the host
    want_f, want_n = host_flags(dets.cpu().numpy(), labels.cpu().numpy(), np.array([2]), [ok.items[0][1]], [ok.items[0][2]],
                                None, 100)
    assert np.array_equal(out[0][2].cpu().numpy(), want_f[0]) and np.array_equal(out[0][3].cpu().numpy(), want_n[0][:2])


def test_neither_op_synchronises(cuda, cases):
    cls, box, metas = _decode_inputs(2, 37, 5, 16, seed=3)
    cls, box, meta = cls.to(cuda), box.to(cuda), _meta_table(metas, cuda)
    args = _match_inputs(cases, cuda)
    thrs = torch.from_numpy(coco_iou_thrs(None)).to(cuda)
    ops.det_decode(cls, box, meta, 16, True)  # (library loaded, attributes set)
    torch.cuda.synchronize()
    old = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode('error')
    try:
        ops.det_decode(cls, box, meta, 16, True)
        ops.det_match(*args, thrs, len(CLASSES), 100)
    finally:
        torch.cuda.set_sync_debug_mode(old)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------- model + engine
def _same(a, b):
    assert list(a.keys()) == list(b.keys())
    for k in a:
        assert a[k] == b[k] or (a[k] != a[k] and b[k] != b[k]), (k, a[k], b[k])


def test_model_and_engine_on_device(cuda, tmp_path, monkeypatch):
    """The tiny model on an on-disk three-image CocoDetDataset in batches of two."""
    from PIL import Image
    from rscotr_amd.engine import single_gpu_test
    from rscotr_amd.mtl import bbox2result
    from rscotr_amd.pipeline import CocoDetDataset, DeviceCollate, DeviceLoader
    cfg, mcfg = load_model_cfg(tiny=True)
    mcfg['test_cfg']['det']['max_per_img'] = 10
    model = build_model(mcfg).to(cuda).eval()
    rng = np.random.RandomState(7)
    (tmp_path / 'det').mkdir()
    names = [f'c{i}' for i in range(20)]
    images, anns = [], []
    for i, (h, w) in enumerate([(64, 64), (64, 96), (80, 64)]):
        Image.fromarray(rng.randint(0, 255, size=(h, w, 3)).astype(np.uint8)).save(tmp_path / 'det' / f'{i}.png')
        images.append(dict(id=i, file_name=f'{i}.png', width=w, height=h))
        for j in range(2):
            anns.append(dict(id=len(anns), image_id=i, category_id=1 + (3 * i + j) % 20, bbox=[4 + 24 * j, 8, 20, 30 + 4 * i],
                             area=20 * (30 + 4 * i), iscrowd=0))
    (tmp_path / 'det.json').write_text(json.dumps(dict(images=images, annotations=anns,
                                                       categories=[dict(id=k + 1, name=n) for k, n in enumerate(names)])))
    ds = CocoDetDataset(str(tmp_path / 'det.json'), str(tmp_path / 'det'), classes=names)
    loaders = dict(dior=DeviceLoader(ds, DeviceCollate('det', cuda, flip_prob=0.0, size_divisor=32), 2, test_mode=True))
    model.CLASSES = dict(dior=ds.CLASSES)
    dev = single_gpu_test(model, loaders, kwargs_dict=dict(det=dict(on_device=True, iou_thrs=[0.5])))['dior']
    host = single_gpu_test(model, loaders)['dior']
    assert len(dev) == 3 and len(host) == 3
    for r in dev:
        assert isinstance(r, tuple) and len(r) == 4 and all(torch.is_tensor(t) and not t.is_cuda for t in r)
        assert tuple(r[0].shape) == (10, 5) and tuple(r[1].shape) == (10,) and tuple(r[2].shape) == (10, 4) and \
            tuple(r[3].shape) == (20, 4)
    assert all(isinstance(r, list) and len(r) == 20 and all(isinstance(a, np.ndarray) and a.shape[1] == 5 for a in r) for r in host)
    # evaluate() of the tuples is coco_bbox_map on bbox2result of those same detections, exactly
    kw = dict(iou_thrs=[0.5], classwise=True)
    same_dets = [bbox2result(r[0], r[1], 20) for r in dev]
    _same(ds.evaluate(dev, **kw), coco_bbox_map(same_dets, [it[1] for it in ds.items], [it[2] for it in ds.items], ds.CLASSES,
                                                iou_thrs=[0.5], max_det=100, classwise=True))
    _same(ds.evaluate(dev, **kw), ds.evaluate(same_dets, **kw))
    with pytest.raises(ValueError):
        ds.evaluate(dev, classwise=True)  # other thresholds than the flags were made for
    # the device detections are the default route's
    logits = torch.linspace(-12, 12, 100001)
    bound = 2.0 * float((logits.to(cuda).sigmoid().cpu().double() - logits.double().sigmoid()).abs().max())
    for r, h in zip(dev, host):
        rows = np.concatenate([np.concatenate([a, np.full((len(a), 1), c, np.float32)], 1) for c, a in enumerate(h)])
        assert len(np.unique(rows[:, 4])) == len(rows) == 10, 'the host result repeats a score: pick another seed'
        rows = rows[np.argsort(-rows[:, 4], kind='mergesort')]
        assert np.array_equal(r[1].numpy(), rows[:, 5].astype(np.int64))
        assert np.array_equal(r[0].numpy()[:, :4], rows[:, :4])
        err = float(np.abs(r[0].numpy()[:, 4].astype(np.float64) - rows[:, 4].astype(np.float64)).max())
        print(f'engine on_device: score difference to the host route {err:.3e}, bound {bound:.3e}')
        assert err <= bound
    # outside the decode limits MTL.simple_test_det(on_device=True) -> DINOHead.simple_test -> get_bboxes_device keeps the
    # torch chain and the loop goes on as before.  (No shape of this model is outside them without torch.topk itself
    # refusing k > Q * C, so the limit is moved, not the model: test_head_keeps_the_torch_chain_outside_the_limits has a
    # real one.)  The rows are then the default route's to the bit, scores included.
    asked = []
    monkeypatch.setattr(ops, 'det_decode_fits', lambda Q, C, K: bool(asked.append((Q, C, K))))
    monkeypatch.setattr(ops, 'det_decode', lambda *a, **k: pytest.fail('det_decode outside its limits'))
    kept = single_gpu_test(model, loaders, kwargs_dict=dict(det=dict(on_device=True, iou_thrs=[0.5])))['dior']
    assert asked == [(30, 20, 10)] * 2
    for r, h in zip(kept, host):
        assert isinstance(r, tuple) and len(r) == 4 and not r[0].is_cuda
        for a, b in zip(bbox2result(r[0], r[1], 20), h):
            assert np.array_equal(a, b)
    _same(ds.evaluate(kept, **kw), ds.evaluate(host, **kw))
