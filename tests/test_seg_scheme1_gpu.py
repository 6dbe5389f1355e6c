"""ops.seg_class_logits (csrc/seg_mix.hip: rscotr_seg_mix_fwd / _bwd) against the reference's two einsums in fp64
(tests/seg_scheme1_oracle.py), and Mask2FormerHead scheme 1 through a train step, the graph runner and device inference.

Tolerance, derived: every output is a sum of products accumulated in fp32 in SOME order, so with A = the sum of the absolute
values of the terms of its chain (fp64) and n = the number of additions in the chain + 4,
    |got - ref| <= n * 2^-24 * A
holds for any order: n = Q + D for seg, K + Q for dmf, P + D for dcls, P + K for de (each + 4).  Elements whose reference
gradient is exactly zero must be exactly zero."""
import copy
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import model as OM
from parity import check_step_pair, default_dtype, run_step_pair
from seg_scheme1_oracle import class_logits_ref, class_logits_sums, seg_forward_scheme1
from util import build_model, load_model_cfg, state_to_oracle

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


def _grid_shape():
    """(B,Q,K,D,P) with more pixels than one trip of either capped grid."""
    from rscotr_amd import ops
    K, D = 2, 256
    P = max(ops.SEG_MIX_FWD_WG * ops.SEG_MIX_FWD_ROWS, ops.SEG_MIX_BWD_WG * ops.seg_mix_bwd_rows(K, D)) + 515
    return (1, 3, K, D, P)


# (B, Q, K, D, P)
SHAPES = {
    'model_16x16': (2, 100, 6, 256, 256),
    'odd_pixels': (1, 7, 6, 256, 1073),          # no multiple of any tile, several workgroups
    'k1_q1': (1, 1, 1, 256, 3),                  # fewer pixels than one workgroup covers
    'k32': (1, 3, 32, 256, 65),                  # the 32-channel instantiation (one row in flight)
    'k12_d128': (1, 5, 12, 128, 130),            # the 16-channel instantiation, two rows per wavefront
    'k3_d64': (2, 4, 3, 64, 77),                 # four rows per wavefront
    'grid_stride': None,                          # filled from the op's own constants
}


@functools.lru_cache(maxsize=None)
def _case(name, device):
    """-> dict(cls, e, mf, g on the device; ref = fp64 outputs; sums = the chain sums): made once per shape, never written to."""
    B, Q, K, D, P = SHAPES[name] or _grid_shape()
    gen = torch.Generator().manual_seed(100 + sorted(SHAPES).index(name))
    t = dict(cls=torch.randn(B, Q, K, generator=gen), e=torch.randn(B, Q, D, generator=gen),
             mf=torch.randn(B, P, D, generator=gen), g=torch.randn(B, K, P, generator=gen))
    t = {k: v.to(device) for k, v in t.items()}
    t['ref'] = class_logits_ref(t['cls'], t['e'], t['mf'], t['g'])
    t['sums'] = class_logits_sums(t['cls'], t['e'], t['mf'], t['g'])
    t['shape'] = (B, Q, K, D, P)
    return t


def _run(cls, e, mf, g, grads=(True, True, True)):
    from rscotr_amd import ops
    ins = [t.detach().clone().requires_grad_(r) for t, r in zip((cls, e, mf), grads)]
    seg = ops.seg_class_logits(*ins)
    seg.backward(g)
    return dict(seg=seg.detach(), dcls=ins[0].grad, de=ins[1].grad, dmf=ins[2].grad)


def _adds(shape):
    B, Q, K, D, P = shape
    return dict(seg=Q + D, dmf=K + Q, dcls=P + D, de=P + K)


def _check(got, c, names=('seg', 'dcls', 'de', 'dmf')):
    adds = _adds(c['shape'])
    for n in names:
        ref, A = c['ref'][n], c['sums'][n]
        assert got[n].shape == ref.shape and got[n].dtype == torch.float32, n
        err = (got[n].double() - ref).abs()
        bound = (adds[n] + 4) * U * A
        ratio = float((err / bound.clamp_min(1e-300)).max())
        print(f'[seg_class_logits {c["shape"]}] {n}: worst |got - ref| / bound = {ratio:.4f} (n = {adds[n] + 4})')
        assert bool((err <= bound).all()), (n, ratio)
        zero = ref == 0
        assert bool((got[n][zero] == 0).all()), n


@pytest.mark.parametrize('name', sorted(SHAPES))
def test_against_the_two_einsums(cuda, name):
    from rscotr_amd import ops
    c = _case(name, str(cuda))
    B, Q, K, D, P = c['shape']
    if name == 'grid_stride':  # the premise: one trip of neither grid covers the pixels
        assert P > ops.SEG_MIX_FWD_WG // B * ops.SEG_MIX_FWD_ROWS and P > ops.SEG_MIX_BWD_WG // B * ops.seg_mix_bwd_rows(K, D)
    _check(_run(c['cls'], c['e'], c['mf'], c['g']), c)


def test_sparse_upstream_gradient(cuda):
    c = _case('odd_pixels', str(cuda))
    B, Q, K, D, P = c['shape']
    g = torch.zeros_like(c['g'])
    g[0, :, 700] = c['g'][0, :, 700]
    got = _run(c['cls'], c['e'], c['mf'], g)
    rows = torch.ones(P, dtype=torch.bool, device=g.device)
    rows[700] = False
    assert bool((got['dmf'][0, rows] == 0).all()) and float(got['dmf'][0, 700].abs().max()) > 0
    c2 = dict(c, ref=class_logits_ref(c['cls'], c['e'], c['mf'], g), sums=class_logits_sums(c['cls'], c['e'], c['mf'], g))
    _check(got, c2)


@pytest.mark.parametrize('name', ['model_16x16', 'k32'])
def test_doubling_and_permuting_cls_is_exact(cuda, name):
    c = _case(name, str(cuda))
    K = c['shape'][2]
    a = _run(c['cls'], c['e'], c['mf'], c['g'])
    b = _run(c['cls'] * 2, c['e'], c['mf'], c['g'])
    assert torch.equal(b['seg'], a['seg'] * 2) and torch.equal(b['dmf'], a['dmf'] * 2)
    perm = torch.randperm(K, generator=torch.Generator().manual_seed(1)).to(c['cls'].device)
    p = _run(c['cls'][:, :, perm], c['e'], c['mf'], c['g'])
    assert torch.equal(p['seg'], a['seg'][:, perm])


def test_gradient_switches(cuda):
    from rscotr_amd import ops
    c = _case('odd_pixels', str(cuda))
    full = _run(c['cls'], c['e'], c['mf'], c['g'])
    frozen = _run(c['cls'], c['e'], c['mf'], c['g'], grads=(True, True, False))
    assert frozen['dmf'] is None
    _check(frozen, c, names=('seg', 'dcls', 'de'))
    assert torch.equal(frozen['dcls'], full['dcls']) and torch.equal(frozen['de'], full['de'])
    only_mf = _run(c['cls'], c['e'], c['mf'], c['g'], grads=(False, False, True))
    assert only_mf['dcls'] is None and only_mf['de'] is None and torch.equal(only_mf['dmf'], full['dmf'])
    only_cls = _run(c['cls'], c['e'], c['mf'], c['g'], grads=(True, False, False))
    assert only_cls['de'] is None and torch.equal(only_cls['dcls'], full['dcls'])
    with torch.no_grad():
        seg = ops.seg_class_logits(c['cls'].clone().requires_grad_(True), c['e'], c['mf'])
    assert not seg.requires_grad and seg.grad_fn is None and torch.equal(seg, full['seg'])


@pytest.mark.parametrize('name', ['model_16x16', 'odd_pixels', 'k3_d64'])
def test_two_calls_are_bit_equal(cuda, name):
    c = _case(name, str(cuda))
    a, b = (_run(c['cls'], c['e'], c['mf'], c['g']) for _ in range(2))
    assert all(torch.equal(a[k], b[k]) for k in a)


def test_op_captured_in_a_graph_replays_bit_equal(cuda):
    """Forward and backward captured on a side stream as the runner captures an iteration, replayed on fresh inputs copied
    into the static tensors: bit-equal to the eager call."""
    from rscotr_amd import ops
    B, Q, K, D, P = 2, 100, 6, 256, 256
    s_cls = torch.zeros(B, Q, K, device=cuda, requires_grad=True)
    s_e = torch.zeros(B, Q, D, device=cuda, requires_grad=True)
    s_mf = torch.zeros(B, P, D, device=cuda, requires_grad=True)
    s_g = torch.zeros(B, K, P, device=cuda)

    def body():
        seg = ops.seg_class_logits(s_cls, s_e, s_mf)
        return (seg.detach(),) + torch.autograd.grad(seg, (s_cls, s_e, s_mf), s_g)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            body()
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            outs = body()
    torch.cuda.current_stream().wait_stream(side)
    gen = torch.Generator().manual_seed(5)
    for trial in range(2):
        fresh = [torch.randn(t.shape, generator=gen).to(cuda) for t in (s_cls, s_e, s_mf, s_g)]
        with torch.no_grad():
            for s, f in zip((s_cls, s_e, s_mf, s_g), fresh):
                s.copy_(f)
        graph.replay()
        torch.cuda.synchronize()
        eager = _run(*fresh)
        assert float(outs[0].abs().max()) > 0
        assert all(torch.equal(x, eager[k]) for x, k in zip(outs, ('seg', 'dcls', 'de', 'dmf'))), trial


# ---- the head ------------------------------------------------------------------------------------------------------------------
def _tiny_cfg():
    cfg, mcfg = load_model_cfg(tiny=True)
    mcfg = copy.deepcopy(mcfg)
    mcfg['seg_head']['scheme'] = 1
    return cfg, mcfg


def test_train_step_tiny_scheme1(cuda, monkeypatch):
    monkeypatch.setattr(OM, 'seg_forward', seg_forward_scheme1)
    _, mcfg = _tiny_cfg()
    model = build_model(mcfg).to(cuda)
    out, oout, rec, orec, P = run_step_pair(model, mcfg, 'seg', 64, seed=3, device=cuda)
    check_step_pair(model, out, oout, rec, orec, P)
    assert rec['seg_logit'].shape[1] == mcfg['seg_head']['num_classes'] + 1
    assert float(model.seg_head.cls_embed.weight.grad.abs().max()) > 0


def test_seg_iterations_scheme1_graph_equals_eager(cuda):
    """Two seg iterations of the tiny scheme-1 model (the second one is the captured and replayed one when graphs are on) from
    identical weights on identical batches: losses and the seg head's gradients finite and bit-equal, graphed against eager."""
    import numpy as np
    from rscotr_amd.data import build_synthetic_multidataloader
    from rscotr_amd.runner import build_runner
    cfg, mcfg = _tiny_cfg()
    mcfg['backbone']['drop_path_rate'] = 0.0
    runs = []
    for graphs in (True, False):
        torch.manual_seed(0)
        np.random.seed(2022)
        model = build_model(mcfg).to(cuda)
        loader = build_synthetic_multidataloader(cfg, cuda, size=64, batch_size=2, tasks=('seg',))
        runner = build_runner(model, cfg, loader, graph_tasks=('seg',) if graphs else ())
        logs = [dict(runner.train_iter()['log_vars']) for _ in range(2)]
        torch.cuda.synchronize()
        assert set(runner.graphed) == ({'seg'} if graphs else set())
        grads = {n: p.grad.detach().clone() for n, p in model.seg_head.named_parameters()}
        runner.optimizer.close()
        assert all(math.isfinite(v) for lg in logs for v in lg.values()), logs
        assert grads and all(bool(torch.isfinite(v).all()) for v in grads.values())
        assert float(grads['cls_embed.weight'].abs().max()) > 0 and float(grads['cls_embed.bias'].abs().max()) > 0
        runs.append((logs, grads))
    (lg, gg), (le, ge) = runs
    print('graphed', lg, '\neager  ', le)
    assert [list(d) for d in lg] == [list(d) for d in le] and any('seg' in k and 'loss' in k for k in lg[0])
    for a, b in zip(lg, le):
        for k in a:
            if 'loss' in k:
                assert a[k] == b[k], (k, a[k], b[k])
    worst = {n: float((gg[n] - ge[n]).abs().max()) for n in gg if not torch.equal(gg[n], ge[n])}
    assert not worst, worst


def test_device_inference_scheme1(cuda):
    """model(task='seg', return_loss=False, rescale=True, on_device=True): labels equal to the arg-max of the oracle's scheme-1
    logits (fp64, under the product's own attention masks) wherever their top-two margin exceeds 1e-4; the pixels under that
    margin are at most 0.1 % of the input's."""
    from rscotr_amd import synth
    _, mcfg = _tiny_cfg()
    model = build_model(mcfg).to(cuda).eval()
    b = synth.make_batch('seg', 2, 64, seed=6)
    ori = (96, 80)
    metas = [dict(m, ori_shape=ori + (3,)) for m in b['img_metas']]
    img = b['img'].to(cuda)
    rec = {}
    with torch.no_grad():
        neck, bb = model.extract_feat(img)
        model.seg_head(model.shared_encoder, neck, bb, metas, record=rec)
    out = model(task='seg', img=img, img_metas=metas, return_loss=False, rescale=True, on_device=True)
    assert isinstance(out, list) and len(out) == 2 and all(o.is_cuda and tuple(o.shape) == ori for o in out)
    P64 = {k: (v.detach().double() if v.dtype.is_floating_point else v.detach()) for k, v in state_to_oracle(model).items()}
    with default_dtype(torch.float64), torch.no_grad():
        feats = OM.swin_forward(b['img'].double(), P64, mcfg['backbone'], None)
        nk = OM.neck_forward(feats[-3:], P64, mcfg['neck'])
        logit, _ = seg_forward_scheme1(nk, P64, mcfg, mcfg['shared_encoder']['num_layers'],
                                       inject_masks=[m.cpu() for m in rec['attn_masks']])
        logit = F.interpolate(logit, size=b['img'].shape[2:], mode='bilinear', align_corners=False)
        h, w = metas[0]['img_shape'][:2]
        logit = F.interpolate(logit[:, :, :h, :w], size=ori, mode='bilinear', align_corners=False)
    assert logit.shape[1] == mcfg['seg_head']['num_classes'] + 1
    top = logit.topk(2, dim=1).values
    clear = (top[:, 0] - top[:, 1]) > 1e-4
    want = logit.argmax(dim=1)
    got = torch.stack(out).cpu().long()
    amb = float((~clear).double().mean())
    wrong = int(((got != want) & clear).sum())
    print(f'[scheme-1 inference] pixels {want.numel()} ambiguous {int((~clear).sum())} ({amb:.5%}) wrong outside them {wrong} '
          f'labels present {sorted(set(got.flatten().tolist()))} max |logit| {float(logit.abs().max()):.3f}')
    assert amb <= 1e-3, amb
    assert wrong == 0, wrong
