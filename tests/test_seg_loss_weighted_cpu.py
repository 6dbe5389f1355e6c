"""Seg-loss options (class_weight, avg_non_ignore, reduction='sum', OHEMPixelSampler, loss_decode as a list) at the model layer,
without a GPU: the configs build, `Mask2FormerHead.losses` routes and combines, and what the contract refuses raises.

The contract the fused kernels implement is restated here in fp64 torch (`contract_loss`); the GPU tests import it as their
reference.  With B images, N = B*H*W pixels, valid_p = (y_p != ignore_index), nll_p = CE of the bilinearly resized logits:
    s_p   = 1, or with OHEM(thresh t, min_kept m): valid_p and exp(-nll_p) < max(sorted_valid_probs[min(m*B, N_valid-1)], t)
    l_p   = s_p * cw[y_p] * nll_p  (0 where ignored)
    mean: sum l / N, or sum l / (N_valid + eps) with avg_non_ignore;  sum: sum l
"""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from util import load_model_cfg

EPS = torch.finfo(torch.float32).eps


def uce_inputs(B, C, h, w, H, W, ignore, with_weights=True):
    """The generator of tests/test_seg_loss_gpu.py (same seed, same draws), then the class weights from the same generator."""
    g = torch.Generator().manual_seed(C * H + w)
    logit = torch.randn(B, C, h, w, generator=g) * 3
    label = torch.randint(0, C, (B, H, W), generator=g)
    label[torch.rand(B, H, W, generator=g) < 0.1] = ignore
    cw = 0.25 + 4 * torch.rand(C, generator=g)
    return (logit, label, cw) if with_weights else (logit, label)


def contract_loss(logit, label, ignore, class_weight=None, avg_non_ignore=False, reduction='mean', ohem=None, mask=None):
    """fp64 restatement of the contract.  ohem = (thresh, min_kept) or None; `mask` (bool, (B,H,W)) replaces the sampler's own
    selection when given.  -> dict(loss (0-d, differentiable w.r.t. 'logit'), logit (the fp64 leaf), nll, valid, mask,
    nll_T (the selection threshold in the CE domain, -log T; None without a sampler))."""
    lr = logit.detach().double().requires_grad_(True)
    B, C = lr.shape[:2]
    up = F.interpolate(lr, size=label.shape[-2:], mode='bilinear', align_corners=False)
    valid = label != ignore
    nll = F.cross_entropy(up, label, reduction='none', ignore_index=ignore)
    cw = None if class_weight is None else torch.as_tensor(class_weight, dtype=torch.float64)
    wnll = F.cross_entropy(up, label, weight=cw, reduction='none', ignore_index=ignore)
    nll_T = None
    if mask is None:
        mask = valid.clone()
        if ohem is not None:
            thresh, min_kept = ohem
            prob = torch.exp(-nll.detach())
            pv = prob[valid]
            if pv.numel() == 0:
                mask = torch.zeros_like(valid)
            else:
                kth = pv.sort().values[min(min_kept * B, pv.numel() - 1)]
                T = max(float(kth), float(thresh))
                mask = valid & (prob < T)
                nll_T = -float(np.log(T))
    total = (wnll * (mask & valid).double()).sum()
    n_valid = int(valid.sum())
    if reduction == 'sum':
        loss = total
    elif reduction == 'mean':
        loss = total / (n_valid + EPS) if avg_non_ignore else total / valid.numel()
    else:
        raise NotImplementedError(reduction)
    return dict(loss=loss, logit=lr, nll=nll.detach(), valid=valid, mask=mask & valid, nll_T=nll_T, up=up.detach(),
                n_valid=n_valid)


class _FakeOps:
    """Stands in for the two fused ops: the contract in torch, every call recorded."""

    def __init__(self):
        self.calls = []

    def upsample_ce(self, seg_logit, label, ignore_index=255):
        self.calls.append(('upsample_ce', {}))
        r = contract_loss(seg_logit, label, ignore_index)
        return r['loss'].float(), self._acc(r, label)

    def upsample_ce_weighted(self, seg_logit, label, ignore_index=255, class_weight=None, avg_non_ignore=False,
                             reduction='mean', ohem=None):
        self.calls.append(('upsample_ce_weighted', dict(class_weight=class_weight, avg_non_ignore=avg_non_ignore,
                                                        reduction=reduction, ohem=ohem)))
        r = contract_loss(seg_logit, label, ignore_index, class_weight, avg_non_ignore, reduction, ohem)
        cw = torch.ones(seg_logit.shape[1]) if class_weight is None else class_weight
        pix = r['mask'].float() * cw[label.clamp(0, seg_logit.shape[1] - 1)]
        return r['loss'].float(), self._acc(r, label), pix

    @staticmethod
    def _acc(r, label):
        correct = ((r['up'].argmax(1) == label) & r['valid']).sum()
        return (correct * 100.0 / (r['n_valid'] + EPS)).float().reshape(1)


def _head(monkeypatch=None, **over):
    from rscotr_amd import MODELS, seg_head
    cfg, mcfg = load_model_cfg()
    hc = copy.deepcopy(mcfg['seg_head'])
    hc.update(over)
    head = MODELS.build(hc)
    fake = None
    if monkeypatch is not None:
        fake = _FakeOps()
        monkeypatch.setattr(seg_head.ops, 'upsample_ce', fake.upsample_ce)
        monkeypatch.setattr(seg_head.ops, 'upsample_ce_weighted', fake.upsample_ce_weighted, raising=False)
    return head, fake


_CW100 = [0.5 + 0.01 * i for i in range(100)]


def _batch():
    logit, label = uce_inputs(2, 100, 8, 8, 32, 32, 255, with_weights=False)
    return logit, label.unsqueeze(1)


def test_cross_entropy_loss_builds_with_options(tmp_path):
    from rscotr_amd import MODELS
    m = MODELS.build(dict(type='CrossEntropyLoss', class_weight=[1.0, 2.0, 0.5], avg_non_ignore=True, loss_weight=0.4))
    assert m.class_weight == [1.0, 2.0, 0.5] and m.avg_non_ignore and m.loss_weight == 0.4 and m.loss_name == 'loss_ce'
    assert not list(m.state_dict())
    assert torch.equal(m.weight_on(torch.device('cpu'), 3), torch.tensor([1.0, 2.0, 0.5]))
    np.save(tmp_path / 'cw.npy', np.array([0.25, 4.0], dtype=np.float32))
    m = MODELS.build(dict(type='CrossEntropyLoss', class_weight=str(tmp_path / 'cw.npy'), reduction='sum'))
    assert m.class_weight == [0.25, 4.0] and m.reduction == 'sum'
    d = MODELS.build(dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=1.0))
    assert d.class_weight is None and not d.avg_non_ignore and d.reduction == 'mean'


def test_head_builds_with_loss_options_list_and_sampler():
    plain, _ = _head()
    keys = list(plain.state_dict())
    head, _ = _head(loss_decode=dict(type='CrossEntropyLoss', class_weight=_CW100, avg_non_ignore=True))
    assert head.loss_decode.class_weight == _CW100 and head.sampler is None
    assert list(head.state_dict()) == keys
    head, _ = _head(loss_decode=[dict(type='CrossEntropyLoss', loss_name='loss_ce', loss_weight=1.0),
                                 dict(type='CrossEntropyLoss', loss_name='loss_wce', class_weight=_CW100, loss_weight=0.5)])
    assert [m.loss_name for m in head.loss_decode] == ['loss_ce', 'loss_wce']
    assert list(head.state_dict()) == keys
    head, _ = _head(sampler=dict(type='OHEMPixelSampler', thresh=0.7, min_kept=500))
    assert (head.sampler.thresh, head.sampler.min_kept) == (0.7, 500)
    assert list(head.state_dict()) == keys


def test_default_head_still_calls_upsample_ce(monkeypatch):
    head, fake = _head(monkeypatch)
    logit, label = _batch()
    out = head.losses(logit, label)
    assert [c[0] for c in fake.calls] == ['upsample_ce']
    assert set(out) == {'loss_ce', 'acc_seg'}
    ref = float(contract_loss(logit, label.squeeze(1), 255)['loss'].detach())
    assert abs(float(out['loss_ce'].detach()) - ref) <= 1e-6 * ref
    # a one-entry list of the default loss is the default configuration too
    head, fake = _head(monkeypatch, loss_decode=[dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=1.0)])
    out = head.losses(logit, label)
    assert [c[0] for c in fake.calls] == ['upsample_ce'] and set(out) == {'loss_ce', 'acc_seg'}


def test_losses_with_options_routes_scales_and_keeps_acc(monkeypatch):
    logit, label = _batch()
    plain, fake0 = _head(monkeypatch)
    acc0 = plain.losses(logit, label)['acc_seg']
    head, fake = _head(monkeypatch, loss_decode=dict(type='CrossEntropyLoss', class_weight=_CW100, avg_non_ignore=True,
                                                     loss_weight=0.3),
                       sampler=dict(type='OHEMPixelSampler', thresh=0.01, min_kept=100))
    out = head.losses(logit, label)
    assert [c[0] for c in fake.calls] == ['upsample_ce_weighted']
    kw = fake.calls[0][1]
    assert torch.equal(kw['class_weight'], torch.tensor(_CW100)) and kw['avg_non_ignore'] and kw['reduction'] == 'mean'
    assert tuple(kw['ohem']) == (0.01, 100)
    assert set(out) == {'loss_ce', 'acc_seg'}
    ref = contract_loss(logit, label.squeeze(1), 255, torch.tensor(_CW100), True, 'mean', (0.01, 100))
    assert 0 < int(ref['mask'].sum()) < ref['n_valid']          # the sampler decides something in this batch
    assert abs(float(out['loss_ce']) - 0.3 * float(ref['loss'])) <= 1e-6 * float(ref['loss'])
    assert torch.equal(out['acc_seg'], acc0)                    # unweighted, unsampled


def test_losses_list_accumulates_same_name_and_separates_others(monkeypatch):
    logit, label = _batch()
    head, fake = _head(monkeypatch, loss_decode=[
        dict(type='CrossEntropyLoss', loss_name='loss_ce', loss_weight=1.0),
        dict(type='CrossEntropyLoss', loss_name='loss_ce', class_weight=_CW100, loss_weight=0.5),
        dict(type='CrossEntropyLoss', loss_name='loss_sum', reduction='sum', loss_weight=2.0)])
    out = head.losses(logit, label)
    assert [c[0] for c in fake.calls] == ['upsample_ce_weighted'] * 3
    assert set(out) == {'loss_ce', 'loss_sum', 'acc_seg'}
    lab = label.squeeze(1)
    a = float(contract_loss(logit, lab, 255)['loss'])
    b = float(contract_loss(logit, lab, 255, torch.tensor(_CW100))['loss'])
    c = float(contract_loss(logit, lab, 255, reduction='sum')['loss'])
    assert abs(float(out['loss_ce']) - (a + 0.5 * b)) <= 1e-6 * (a + 0.5 * b)
    assert abs(float(out['loss_sum']) - 2.0 * c) <= 1e-6 * 2.0 * c
    # MTL._parse_losses sums every key that contains 'loss'
    assert sum('loss' in k for k in out) == 2


def test_contract_refusals(monkeypatch):
    from rscotr_amd import MODELS
    with pytest.raises(NotImplementedError):
        MODELS.build(dict(type='CrossEntropyLoss', reduction='none'))
    with pytest.raises(NotImplementedError):
        MODELS.build(dict(type='CrossEntropyLoss', use_sigmoid=True))
    with pytest.raises(NotImplementedError):
        MODELS.build(dict(type='CrossEntropyLoss', use_mask=True))
    with pytest.raises(NotImplementedError):
        _head(sampler=dict(type='OHEMPixelSampler', thresh=None, min_kept=10))
    with pytest.raises(NotImplementedError, match='DiceLoss'):
        _head(loss_decode=dict(type='DiceLoss'))
    with pytest.raises(NotImplementedError, match='LovaszLoss'):
        _head(loss_decode=[dict(type='CrossEntropyLoss'), dict(type='LovaszLoss')])
    with pytest.raises((TypeError, ValueError)):
        MODELS.build(dict(type='CrossEntropyLoss', class_weight=3.0))
    with pytest.raises((TypeError, ValueError)):
        MODELS.build(dict(type='CrossEntropyLoss', class_weight='weights.pkl'))
    head, _ = _head(monkeypatch, loss_decode=dict(type='CrossEntropyLoss', class_weight=[1.0] * 6))
    logit, label = _batch()
    with pytest.raises(ValueError, match=r'6\b.*\b100\b'):
        head.losses(logit, label)


def test_op_wrapper_refuses_before_touching_the_device():
    from rscotr_amd import ops
    logit, label = uce_inputs(1, 3, 4, 4, 8, 8, 255, with_weights=False)
    with pytest.raises(NotImplementedError):
        ops.upsample_ce_weighted(logit, label, 255, reduction='none')
    with pytest.raises(NotImplementedError):
        ops.upsample_ce_weighted(logit, label, 255, ohem=(None, 10))
