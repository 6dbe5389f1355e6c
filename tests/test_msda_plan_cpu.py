"""The host queries of the MSDA backward planner (csrc/msda.hip: plan_msda_bwd) and of the fused forward answer what the library
answered on the commit before csrc/msda.hip was split by backward strategy (tests/golden/make_msda_plan_golden.py wrote
tests/golden/msda_plan.npz there).  rscotr_amd/ops/deform.py sizes the workspace from the two workspace queries and decides from
them whether grad_value is zeroed; rscotr_msda_bwd picks its strategy from the same arithmetic."""
import importlib.util
import os

import numpy as np

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def _maker():
    spec = importlib.util.spec_from_file_location('make_msda_plan_golden', os.path.join(GOLDEN_DIR, 'make_msda_plan_golden.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_msda_workspace_queries_answer_what_the_cascade_answered():
    mk = _maker()
    gold = np.load(os.path.join(GOLDEN_DIR, 'msda_plan.npz'))
    # the recording covers the generator's census (nothing dropped from either side)
    cs, fcs = mk.cases(), mk.fused_cases()
    assert gold['cases'].tolist() == [list(c) for c in cs] and gold['fused_cases'].tolist() == [list(c) for c in fcs]
    assert [[tuple(r) for r in p[:len(q)].tolist()] for p, q in zip(gold['pyramids'], mk.PYRAMIDS)] == mk.PYRAMIDS
    now = mk.record(mk.load(), cs, fcs)
    for key in ('sorted_ws', 'tiled_ws', 'fused_ok'):
        assert now[key].shape == gold[key].shape, key
        bad = np.flatnonzero(now[key] != gold[key])
        src = fcs if key == 'fused_ok' else cs
        assert bad.size == 0, (key, len(bad), [(src[i], int(gold[key][i]), int(now[key][i])) for i in bad[:8]])
    # the census reaches every answer the planner distinguishes
    c = gold['cases']
    L, tiled, srt = c[:, 6], gold['tiled_ws'] > 0, gold['sorted_ws'] > 0
    regular = (c[:, 0] >= 0) & (c[:, 1] > 0) & (c[:, 3] > 0) & (c[:, 3] < (1 << 20)) & (c[:, 4] > 0) & (c[:, 7] > 0)
    assert tiled.any() and srt.any() and (srt & ~tiled & regular).any() and (~srt & ~tiled & regular).any()
    assert not tiled[L > 8].any() and not srt[L > 16].any() and tiled[regular & (L == 8)].any() and srt[regular & (L == 16)].any()
    assert gold['fused_ok'].any() and not gold['fused_ok'].all()
