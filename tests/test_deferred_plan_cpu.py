"""The launch plans of the deferred end-of-backward work (ops.DEFER: split-K combine, LayerNorm and window-attention folds, the three
grouped weight-gradient variants) and of the three weight-plane caches, pinned against tables recorded on the commit before the
operator layer was split into modules (tests/golden/make_deferred_plan_golden.py wrote tests/golden/deferred_plan.npz there).  The
planners are host code: no GPU and no library."""
import importlib.util
import os

import numpy as np

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def _generator():
    spec = importlib.util.spec_from_file_location('make_deferred_plan_golden',
                                                  os.path.join(GOLDEN_DIR, 'make_deferred_plan_golden.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_deferred_and_plane_plans_match_the_recorded_tables():
    gen = _generator()
    want = np.load(gen.GOLDEN)
    tables, seq = gen.record()
    assert seq == [str(s) for s in want['sequence']]
    assert sorted(tables) == sorted(k for k in want.files if k != 'sequence')
    for k, t in tables.items():
        assert t.dtype == want[k].dtype and t.shape == want[k].shape and np.array_equal(t, want[k]), k
    # what the pending set was built to reach: more than one round per queue, all three grouped variants, the voided ranges, cache hits
    n = seq.index('flush', 1)
    assert seq[:n] == seq[n:2 * n], 'the second flush of the same set replays the first'
    first, third = seq[:n], seq[2 * n:seq.index('planes|W')]
    assert sum(s.startswith('rscotr_splitk_flush') for s in first) == 2
    assert sum(s.startswith('rscotr_layernorm_flush') for s in first) == 4
    assert sum(s.startswith('rscotr_swin_wattn_flush') for s in first) == 2
    variants = lambda part: [int(s.split(',')[2]) for s in part if s.startswith('rscotr_gemm_dw_group')]
    assert variants(first) == [0, 6, 7] and variants(third) == [0, 6]
    assert not any(s.startswith('rscotr_amax_group') for s in third)


def test_recording_leaves_the_product_state_alone():
    from rscotr_amd import ops
    from rscotr_amd._lib import lib
    before = [dict(o.__dict__) for o in (ops.DEFER, ops.WPLANES, ops.HPLANES, ops.FPLANES)]
    _generator().record()
    assert before == [dict(o.__dict__) for o in (ops.DEFER, ops.WPLANES, ops.HPLANES, ops.FPLANES)]
    assert 'call' not in vars(lib) and not hasattr(ops.STATE.grad_sink, 'seq')
