"""Inference path (MTL.forward(return_loss=False) -> simple_test_{cls,det,seg}; models/multi/multitask_learner.py:91-227,
mmdet_detr_head/detr_head.py:590-682) on the GPU against the oracle's restatement: class scores, detections (top-300 of
the sigmoid scores over query x class, boxes in pixels) and segmentation maps."""
import numpy as np
import pytest
import torch

from oracle import model as OM
from rscotr_amd import synth
from util import build_model, load_model_cfg, state_to_oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def setup(cuda):
    cfg, mcfg = load_model_cfg(tiny=True)
    mcfg['test_cfg']['det']['max_per_img'] = 25
    model = build_model(mcfg).to(cuda).eval()
    return mcfg, model, state_to_oracle(model)


def test_simple_test_cls(setup, cuda):
    mcfg, model, P = setup
    b = synth.make_batch('cls', 3, 64, seed=2)
    ref = OM.simple_test(P, mcfg, 'cls', b['img'], b['img_metas']).detach()
    out = model(task='cls', img=b['img'].to(cuda), img_metas=b['img_metas'], return_loss=False)
    assert isinstance(out, list) and len(out) == 3 and out[0].shape == (mcfg['cls_head']['num_classes'],)
    assert np.allclose(np.stack(out), ref.numpy(), rtol=1e-3, atol=1e-6)


def test_simple_test_det(setup, cuda):
    mcfg, model, P = setup
    b = synth.make_batch('det', 2, 64, seed=4)
    metas = [dict(m, scale_factor=np.array([0.5, 0.5, 0.5, 0.5], dtype=np.float32)) for m in b['img_metas']]
    rec = {}
    # the product's own proposal selection is injected into the oracle (hard top-k decision, compared in the train tests)
    with torch.no_grad():
        feat = model.extract_feat(b['img'].to(cuda))[0]
        for m in metas:
            m['batch_input_shape'] = (64, 64)
        model.bbox_head(model.shared_encoder, feat, metas, record=rec)
    ref = OM.simple_test(P, mcfg, 'det', b['img'], metas, rescale=True, inject=dict(det_topk_idx=rec['topk_idx'].cpu()))
    out = model(task='det', img=b['img'].to(cuda), img_metas=[dict(m) for m in metas], return_loss=False, rescale=True)
    ncls = mcfg['bbox_head']['num_classes']
    assert len(out) == 2 and all(len(r) == ncls for r in out)
    for res, (rb, rl) in zip(out, ref):
        got = np.concatenate(res, 0)
        assert got.shape == (25, 5) and got.dtype == np.float32
        # same multiset of (label, box, score): sort both by score
        rb, rl = rb.detach().numpy(), rl.numpy()
        lab = np.concatenate([np.full(len(r), i) for i, r in enumerate(res)])
        o1, o2 = np.argsort(-got[:, 4], kind='stable'), np.argsort(-rb[:, 4], kind='stable')
        assert np.allclose(got[o1, 4], rb[o2, 4], rtol=1e-3, atol=1e-6)
        assert np.allclose(got[o1, :4], rb[o2, :4], rtol=1e-3, atol=0.05) and (lab[o1] == rl[o2]).all()
        assert got[:, :4].min() >= 0 and got[:, :4].max() <= 128.0 + 1e-3  # clipped to the image, then / 0.5


def test_simple_test_seg(setup, cuda):
    mcfg, model, P = setup
    b = synth.make_batch('seg', 2, 64, seed=6)
    metas = [dict(m, ori_shape=(96, 80, 3)) for m in b['img_metas']]
    rec = {}
    with torch.no_grad():
        neck, bb = model.extract_feat(b['img'].to(cuda))
        model.seg_head(model.shared_encoder, neck, bb, metas, record=rec)
    ref = OM.simple_test(P, mcfg, 'seg', b['img'], metas, rescale=True,
                         inject=dict(seg_attn_masks=[m.cpu() for m in rec['attn_masks']]))
    out = model(task='seg', img=b['img'].to(cuda), img_metas=metas, return_loss=False, rescale=True)
    assert isinstance(out, list) and len(out) == 2 and out[0].shape == (96, 80)
    agree = float((np.stack(out) == ref.numpy()).mean())
    assert agree >= 0.995, agree  # arg-max over 100 near-random channels: ties within fp32 rounding may flip


def test_simple_test_det_padded(setup, cuda):
    """A padded, non-square det batch (64 x 96 canvas, images 64 x 70 and 50 x 96): masked route of the head (masks,
    key padding masks, valid ratios, +inf proposals), then every image's boxes clamped to ITS OWN img_shape and
    un-scaled — not the canvas."""
    mcfg, model, P = setup
    shapes = [(64, 70), (50, 96)]
    b = synth.make_batch('det', 2, (64, 96), seed=4, img_shapes=shapes)
    metas = [dict(m, scale_factor=np.array([0.5, 0.625, 0.5, 0.625], dtype=np.float32)) for m in b['img_metas']]
    rec = {}
    with torch.no_grad():
        feat = model.extract_feat(b['img'].to(cuda))[0]
        model.bbox_head(model.shared_encoder, feat, [dict(m, batch_input_shape=(64, 96)) for m in metas], record=rec)
    ref = OM.simple_test(P, mcfg, 'det', b['img'], metas, rescale=True, inject=dict(det_topk_idx=rec['topk_idx'].cpu()))
    out = model(task='det', img=b['img'].to(cuda), img_metas=[dict(m) for m in metas], return_loss=False, rescale=True)
    assert len(out) == 2
    for res, (rb, rl), (h, w) in zip(out, ref, shapes):
        got = np.concatenate(res, 0)
        assert got.shape == (25, 5) and np.isfinite(got).all()
        rb, rl = rb.detach().numpy(), rl.numpy()
        lab = np.concatenate([np.full(len(r), i) for i, r in enumerate(res)])
        o1, o2 = np.argsort(-got[:, 4], kind='stable'), np.argsort(-rb[:, 4], kind='stable')
        assert np.allclose(got[o1, 4], rb[o2, 4], rtol=1e-3, atol=1e-6)
        assert np.allclose(got[o1, :4], rb[o2, :4], rtol=1e-3, atol=0.05) and (lab[o1] == rl[o2]).all()
        assert got[:, :4].min() >= 0
        assert got[:, [0, 2]].max() <= w / 0.5 + 1e-3 and got[:, [1, 3]].max() <= h / 0.625 + 1e-3, (h, w)


def test_simple_test_seg_non_square(setup, cuda):
    """seg inference on a 64 x 96 canvas (the pixel decoder's levels 8 x 12 ... 2 x 3, a W / H swap would not survive),
    resized to a non-square ori_shape."""
    mcfg, model, P = setup
    b = synth.make_batch('seg', 2, (64, 96), seed=6)
    metas = [dict(m, ori_shape=(80, 120, 3)) for m in b['img_metas']]
    rec = {}
    with torch.no_grad():
        neck, bb = model.extract_feat(b['img'].to(cuda))
        model.seg_head(model.shared_encoder, neck, bb, metas, record=rec)
    ref = OM.simple_test(P, mcfg, 'seg', b['img'], metas, rescale=True,
                         inject=dict(seg_attn_masks=[m.cpu() for m in rec['attn_masks']]))
    out = model(task='seg', img=b['img'].to(cuda), img_metas=metas, return_loss=False, rescale=True)
    assert isinstance(out, list) and len(out) == 2 and out[0].shape == (80, 120)
    agree = float((np.stack(out) == ref.numpy()).mean())
    assert agree >= 0.995, agree


def test_forward_test_contract(setup, cuda):
    mcfg, model, P = setup
    b = synth.make_batch('cls', 2, 64, seed=1)
    with pytest.raises(NotImplementedError):
        model.forward_test(['cls', 'seg'], b['img'].to(cuda), b['img_metas'])
    with pytest.raises(NotImplementedError):
        model.forward_test('cls', [b['img'].to(cuda)] * 2, b['img_metas'])
    out = model.forward_test(['cls', 'cls'], [b['img'].to(cuda)], [b['img_metas']])
    assert len(out) == 2
