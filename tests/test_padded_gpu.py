"""Padded det batches and non-square canvases on the HIP path, held to the oracle.  mmdet's Resize(keep_ratio=True) +
Pad(size_divisor=32) hands the model such batches for any non-square input: an image smaller than the canvas sends the
det head down its masked route (per-image masks and their sine encodings, a key padding mask into every MSDA node,
valid ratios below 1, +inf proposals on padded tokens, per-level 4-d decoder references), and a non-square canvas is
what tells W from H wherever levels, layout views and caches are assembled.  Every whole-step case goes through the
gate of tests/parity.py (two fp32 tiers, the fp64 anchor, Hungarian indices bit-exact)."""
import pytest
import torch

from parity import check_step_pair, ranges_checked, run_step_pair
from util import build_model, load_model_cfg

pytestmark = pytest.mark.gpu

# case a's det batch: 64 x 96 canvas, one image short in W, one short in H
TINY_PADDED = dict(size=(64, 96), img_shapes=[(64, 70), (50, 96)])
# case c: BASELINE configs[1]'s canvas, both images padded (one in W, one in H)
MAIN_PADDED = dict(size=(512, 512), img_shapes=[(512, 384), (448, 512)])


@pytest.fixture(scope='module')
def tiny(cuda):
    cfg, mcfg = load_model_cfg(tiny=True)
    return mcfg, build_model(mcfg).to(cuda)


@pytest.mark.parametrize('task', ['cls', 'det', 'seg'])
def test_tiny_non_square_and_padded(tiny, task, cuda):
    """(a) tiny config on a 64 x 96 canvas: det with both images padded, cls and seg unpadded."""
    mcfg, model = tiny
    kw = TINY_PADDED if task == 'det' else dict(size=(64, 96))
    out, oout, rec, orec, P = run_step_pair(model, mcfg, task, seed=3, device=cuda, **kw)
    check_step_pair(model, out, oout, rec, orec, P)


@pytest.mark.parametrize('task', ['cls', 'det', 'seg'])
def test_main_config_non_square_384x512(task, cuda):
    """(b) main config, 384 x 512 canvas (levels 48 x 64 ... 6 x 8 in the det head, 12 x 16 at Swin stage 4), unpadded,
    every range word of the iteration checked against its tensor."""
    cfg, mcfg = load_model_cfg(tiny=False)
    model = build_model(mcfg, seed=4).to(cuda)
    with ranges_checked():
        out, oout, rec, orec, P = run_step_pair(model, mcfg, task, seed=17, device=cuda, fp64=True, size=(384, 512))
    check_step_pair(model, out, oout, rec, orec, P)


@pytest.mark.parametrize('prec', [0, 3])
def test_main_config_padded_det_512(prec, cuda):
    """(c) main config at 512 x 512 with images 512 x 384 and 448 x 512, under both fp32-accurate precision modes of the
    GEMM (as test_train_step_main_config_512) and the range-word check."""
    from rscotr_amd._lib import lib
    old = lib.rscotr_gemm_get_precision()
    lib.call('rscotr_gemm_set_precision', prec)
    try:
        cfg, mcfg = load_model_cfg(tiny=False)
        model = build_model(mcfg, seed=4).to(cuda)
        with ranges_checked():
            out, oout, rec, orec, P = run_step_pair(model, mcfg, 'det', seed=17, device=cuda, fp64=True, **MAIN_PADDED)
    finally:
        lib.call('rscotr_gemm_set_precision', old)
    check_step_pair(model, out, oout, rec, orec, P)


def test_main_config_padded_det_strip(cuda):
    """(d) 256 x 256 canvas, one full image next to a 256 x 48 strip: the strip's valid ratio in W is 3/16 at the finest
    level and 1/4 at the coarsest (1 of 4 columns), so most of its references and samples sit at the mask's edge."""
    from rscotr_amd import synth
    kw = dict(size=(256, 256), img_shapes=[(256, 256), (256, 48)])
    b = synth.make_batch('det', 2, seed=9, **kw)
    assert b['img_metas'][1]['img_shape'][:2] == (256, 48)
    cfg, mcfg = load_model_cfg(tiny=False)
    model = build_model(mcfg, seed=6).to(cuda)
    out, oout, rec, orec, P = run_step_pair(model, mcfg, 'det', seed=9, device=cuda, **kw)
    # the strip has ~260 valid tokens for 600 queries: the top-k must take ~340 padded ones, and every padded token scores
    # the same (memory zeroed there before enc_output), so which of them fill the slots is a tie — the product's choice is
    # the one the oracle's loss evaluation was given (run_step_pair).  A position where the two selections differ, both
    # tokens are padded and both score bitwise the same is such a tie: the gate sees the oracle's choice there
    tp, to, sc = rec['topk_idx'].cpu(), orec['topk_idx'], orec['topk_scores']
    levels = [(256 // s, 256 // s) for s in (8, 16, 32, 64)]
    img = torch.ones(2, 256, 256)
    for i, (h, w) in enumerate(kw['img_shapes']):
        img[i, :h, :w] = 0
    padded = torch.cat([torch.nn.functional.interpolate(img[None], size=s).to(torch.bool).squeeze(0).flatten(1) for s in levels], 1)
    mism = tp != to
    ties = mism & (sc.gather(1, tp) == sc.gather(1, to)) & padded.gather(1, tp) & padded.gather(1, to)
    assert int(padded.gather(1, tp)[1].sum()) > 300 and not padded.gather(1, tp)[0].any()
    rec['topk_idx'] = torch.where(ties, to, tp).to(rec['topk_idx'].device)  # (other differences: the gate's own rule)
    check_step_pair(model, out, oout, rec, orec, P)


def test_main_config_padded_det_batch_of_one(cuda):
    """(e) B = 1 on a 384 x 352 canvas with a 360 x 330 image: every image of the batch is padded."""
    cfg, mcfg = load_model_cfg(tiny=False)
    model = build_model(mcfg, seed=7).to(cuda)
    out, oout, rec, orec, P = run_step_pair(model, mcfg, 'det', seed=5, device=cuda, batch_size=1, size=(384, 352),
                                            img_shapes=[(360, 330)])
    check_step_pair(model, out, oout, rec, orec, P)


def _det_step(model, batch, rnd, static_path=True):
    model.bbox_head.static_path = static_path
    try:
        model.zero_grad(set_to_none=True)
        rec = {}
        out = model.train_step(dict(batch, rnd=rnd, record=rec))
        out['loss'].backward()
        torch.cuda.synchronize()
    finally:
        model.bbox_head.static_path = True
    return out, rec


def test_padded_static_path_equals_dynamic_path(cuda):
    """test_det_static_path_equals_dynamic_path_full_size on case c's batch: the static targets take each image's own
    (w, h) factors."""
    from rscotr_amd import synth
    cfg, mcfg = load_model_cfg(tiny=False)
    model = build_model(mcfg, seed=2).to(cuda)
    batch = synth.make_batch('det', 2, seed=21, device=cuda, **MAIN_PADDED)
    rnd = synth.make_rnd(model, synth.make_batch('det', 2, seed=21, **MAIN_PADDED), seed=21, device=cuda)
    (o1, r1), (o2, r2) = _det_step(model, batch, rnd, True), _det_step(model, batch, rnd, False)
    assert list(o1['log_vars']) == list(o2['log_vars']) and len(o1['log_vars']) == 40
    assert r1['match'].keys() == r2['match'].keys() and len(r1['match']) == 14
    for k in r1['match']:
        assert (r1['match'][k][0] == r2['match'][k][0]).all() and (r1['match'][k][1] == r2['match'][k][1]).all(), k
    for k, v in o1['log_vars'].items():
        assert abs(v - o2['log_vars'][k]) <= 1e-4 * max(abs(v), 1e-3), (k, v, o2['log_vars'][k])


def test_padded_det_step_is_bitwise_reproducible(cuda):
    """Case c's det step three times in one process: bitwise-equal forward records and gradients."""
    from test_determinism_gpu import first_difference
    from rscotr_amd import synth

    def once(model):
        batch = synth.make_batch('det', 2, seed=17, device=cuda, **MAIN_PADDED)
        rnd = synth.make_rnd(model, synth.make_batch('det', 2, seed=17, **MAIN_PADDED), seed=17, device=cuda)
        out, rec = _det_step(model, batch, rnd)
        fwd = {'loss': out['loss'].detach().clone()}
        for k, v in rec.items():
            if torch.is_tensor(v):
                fwd[k] = v.detach().clone()
            elif isinstance(v, (list, tuple)) and v and torch.is_tensor(v[0]):
                for i, t in enumerate(v):
                    fwd[f'{k}[{i}]'] = t.detach().clone()
        return fwd, {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}

    cfg, mcfg = load_model_cfg(tiny=False)
    model = build_model(mcfg, seed=4).to(cuda)
    runs = [once(model) for _ in range(3)]
    for fwd, grads in runs[1:]:
        assert first_difference(runs[0][0], fwd) is None, ('forward', first_difference(runs[0][0], fwd))
        assert first_difference(runs[0][1], grads) is None, ('gradients', first_difference(runs[0][1], grads))


def test_padded_graph_replay_equals_eager(cuda):
    """A det-only runner whose loader yields a fixed padded layout (256 x 256 canvas, images 256 x 192 and 208 x 256):
    the captured iteration replayed against eager iterations, as test_graph_replay_equals_eager_at_size.  A batch whose
    img_shapes differ from the captured ones is refused by GraphedTask.accepts, runs eagerly and stays finite."""
    import importlib.util
    import os
    import numpy as np
    from rscotr_amd import Config, MODELS, synth
    from rscotr_amd.data import build_synthetic_multidataloader
    from rscotr_amd.runner import build_runner
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location('bench_mod', os.path.join(root, 'bench.py'))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    cfg = Config.fromfile(bench.CFG)
    shapes = [(256, 192), (208, 256)]
    logs = []
    for graphs in (True, False):
        torch.manual_seed(0)
        np.random.seed(2022)
        model = MODELS.build(bench.workload_model_cfg(cfg, 'det800'))
        model.init_weights()
        model.to(cuda).train()
        model.backbone.drop_path_rates = [0.0 for _ in model.backbone.drop_path_rates]
        loader = build_synthetic_multidataloader(cfg, cuda, size=256, batch_size=2, tasks=('det',), max_gt=20, pool=1,
                                                 img_shapes=shapes)
        runner = build_runner(model, cfg, loader, graph_tasks=('det',) if graphs else ())
        last = None
        for i in range(3):
            out = runner.train_iter()
            if i == 1:
                last = dict(out['log_vars'])
            else:
                assert all(v == v and abs(v) < 1e6 for v in dict(out['log_vars']).values()), i
        torch.cuda.synchronize()
        assert set(runner.graphed) == ({'det'} if graphs else set())
        if graphs:
            # a batch of another layout does not fit the captured iteration: the runner takes it eagerly
            g = runner.graphed['det']
            assert g.accepts(synth.make_batch('det', 2, 256, seed=6, device=cuda, img_shapes=shapes))
            other = synth.make_batch('det', 2, 256, seed=5, device=cuda, img_shapes=[(256, 160), (208, 256)])
            assert not g.accepts(other)
            runner._it = iter([other])
            out = runner.train_iter()
            torch.cuda.synchronize()
            assert runner.graphed['det'] is g
            assert all(v == v and abs(v) < 1e6 for v in dict(out['log_vars']).values()), dict(out['log_vars'])
        for n, p in model.named_parameters():
            assert torch.isfinite(p).all(), n
        logs.append(last)
        runner.optimizer.close()
    lg, le = logs
    assert list(lg) == list(le) and len(lg) > 0
    for k, v in lg.items():
        assert v == v and abs(v) < 1e6, (k, v)
        if 'dn_' in k or k.endswith('.loss') or 'loss' not in k:
            continue
        assert abs(v - le[k]) <= 5e-3 * max(abs(le[k]), 1e-2), (k, v, le[k])
