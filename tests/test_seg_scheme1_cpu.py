"""Mask2FormerHead scheme 1 on the host: construction and state-dict keys, the module wiring of one seg train step against
the oracle (HIP ops patched with the oracle, ops.seg_class_logits by the literal einsums), the checkpoint round trip and the
argument checks of the op wrapper.  The kernels themselves: tests/test_seg_scheme1_gpu.py."""
import copy

import pytest
import torch

from oracle import model as OM
from parity import check_step_pair, run_step_pair
from seg_scheme1_oracle import seg_forward_scheme1
from util import build_model, load_model_cfg, patch_ops_with_oracle


def _cfg(scheme, tiny=True):
    cfg, mcfg = load_model_cfg(tiny=tiny)
    mcfg = copy.deepcopy(mcfg)
    mcfg['seg_head']['scheme'] = scheme
    return cfg, mcfg


def test_scheme1_builds_cls_embed_and_only_that():
    from rscotr_amd import MODELS
    _, m1 = _cfg(1, tiny=False)
    _, m2 = _cfg(2, tiny=False)
    one, two = MODELS.build(copy.deepcopy(m1)), MODELS.build(copy.deepcopy(m2))
    sc = m1['seg_head']
    assert tuple(one.seg_head.cls_embed.weight.shape) == (sc['num_classes'] + 1, sc['feat_channels'])
    assert tuple(one.seg_head.cls_embed.bias.shape) == (sc['num_classes'] + 1,)
    k1, k2 = set(one.state_dict()), set(two.state_dict())
    assert k1 - k2 == {'seg_head.cls_embed.weight', 'seg_head.cls_embed.bias'} and not k2 - k1
    assert not hasattr(two.seg_head, 'cls_embed')
    # init_weights leaves cls_embed as nn.Linear made it (mask2former_head.py:102-109)
    before = one.seg_head.cls_embed.weight.detach().clone()
    one.init_weights()
    assert torch.equal(one.seg_head.cls_embed.weight, before)
    _, m3 = _cfg(3, tiny=False)
    with pytest.raises(NotImplementedError):
        MODELS.build(copy.deepcopy(m3['seg_head']))
    # the reference's own default
    m0 = copy.deepcopy(m1['seg_head'])
    del m0['scheme']
    assert MODELS.build(m0).scheme == 1


def _counted_step(monkeypatch, scheme):
    """One tiny seg train step on the CPU gate of tests/test_model_cpu.py -> (model, calls of the stand-in, calls of
    ops.mask_logits)."""
    from rscotr_amd import ops
    patch_ops_with_oracle(monkeypatch)
    calls = dict(mix=0, mask=0)
    mask_logits = ops.mask_logits

    def counted_mask_logits(e, mask_tokens):
        calls['mask'] += 1
        return mask_logits(e, mask_tokens)

    def seg_class_logits(cls_pred, e, mask_tokens):
        calls['mix'] += 1
        mask_pred = torch.einsum('bqd,bpd->bqp', e, mask_tokens)
        return torch.einsum('bqc,bqp->bcp', cls_pred, mask_pred)

    for mod in (ops, ops.attention):
        monkeypatch.setattr(mod, 'mask_logits', counted_mask_logits)
        monkeypatch.setattr(mod, 'seg_class_logits', seg_class_logits)
    if scheme == 1:
        monkeypatch.setattr(OM, 'seg_forward', seg_forward_scheme1)
    _, mcfg = _cfg(scheme)
    model = build_model(mcfg)
    out, oout, rec, orec, P = run_step_pair(model, mcfg, 'seg', 64, seed=3)
    check_step_pair(model, out, oout, rec, orec, P)
    return model, mcfg, rec, calls


def test_train_step_scheme1_matches_oracle(monkeypatch):
    model, mcfg, rec, calls = _counted_step(monkeypatch, 1)
    sc = mcfg['seg_head']
    assert calls['mix'] == 1  # once per forward: the last prediction only
    nlay = sc['transformer_decoder']['num_layers']
    assert calls['mask'] == nlay  # the initial prediction and every layer's but the last
    assert tuple(rec['seg_logit'].shape[:2]) == (2, sc['num_classes'] + 1)
    assert len(rec['attn_masks']) == nlay
    g = model.seg_head.cls_embed.weight.grad
    assert g is not None and float(g.abs().max()) > 0 and float(model.seg_head.cls_embed.bias.grad.abs().max()) > 0


def test_scheme2_calls_mask_logits_once_more(monkeypatch):
    model, mcfg, rec, calls = _counted_step(monkeypatch, 2)
    assert calls['mix'] == 0
    assert calls['mask'] == mcfg['seg_head']['transformer_decoder']['num_layers'] + 1
    assert rec['seg_logit'].shape[1] == mcfg['seg_head']['num_queries']


def test_checkpoint_round_trip_keeps_cls_embed(tmp_path):
    from rscotr_amd.checkpoint import load_checkpoint, save_checkpoint
    _, mcfg = _cfg(1)
    a, b = build_model(mcfg, seed=1), build_model(mcfg, seed=2)
    assert not torch.equal(a.seg_head.cls_embed.weight, b.seg_head.cls_embed.weight)
    path = str(tmp_path / 'scheme1.pth')
    ck = save_checkpoint(path, a)
    assert 'seg_head.cls_embed.weight' in ck['state_dict'] and 'seg_head.cls_embed.bias' in ck['state_dict']
    _, rep = load_checkpoint(b, path, strict=True)
    assert not rep.missing_keys and not rep.unexpected_keys
    assert torch.equal(a.seg_head.cls_embed.weight, b.seg_head.cls_embed.weight)
    assert torch.equal(a.seg_head.cls_embed.bias, b.seg_head.cls_embed.bias)
    # a scheme-2 model does not take the two keys silently
    _, m2 = _cfg(2)
    with pytest.raises(RuntimeError):
        load_checkpoint(build_model(m2, seed=3), path, strict=True)


@pytest.mark.parametrize('B,Q,K,D,P', [(1, 3, 0, 256, 4), (1, 3, 33, 256, 4), (1, 3, 6, 96, 4), (1, 3, 6, 512, 4)])
def test_op_refuses_unsupported_sizes_before_the_library(monkeypatch, B, Q, K, D, P):
    """CPU tensors: a wrapper that reached the library would raise the RuntimeError of the missing CPU path instead."""
    from rscotr_amd import ops
    from rscotr_amd._lib import lib

    def no_library(*a, **k):
        raise AssertionError('the library was reached')

    monkeypatch.setattr(lib, 'call', no_library)
    with pytest.raises(ValueError, match='K = ' if K in (0, 33) else 'D = '):
        ops.seg_class_logits(torch.zeros(B, Q, K), torch.zeros(B, Q, D), torch.zeros(B, P, D))


def test_op_refuses_disagreeing_shapes():
    from rscotr_amd import ops
    with pytest.raises(ValueError):
        ops.seg_class_logits(torch.zeros(1, 3, 6), torch.zeros(1, 4, 256), torch.zeros(1, 5, 256))
    with pytest.raises(ValueError):
        ops.seg_class_logits(torch.zeros(1, 3, 6), torch.zeros(1, 3, 256), torch.zeros(1, 5, 128))
    with pytest.raises(ValueError):
        ops.seg_class_logits(torch.zeros(1, 3, 6), torch.zeros(1, 3, 256), torch.zeros(5, 256))
