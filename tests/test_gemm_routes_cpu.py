"""The host views of the GEMM route planner (csrc/gemm.hip: plan_gemm) answer what the library answered on the commit before
csrc/gemm.hip was split into per-family files (tests/golden/make_gemm_routes_golden.py wrote tests/golden/gemm_routes.npz there).
The Python side caches these answers and acts on them — a B operand handed over as planes, a ReLU gate kept as bits, a workspace
whose size feeds back into the split count — so every recorded case is asked again, in all four mode combinations."""
import importlib.util
import os

import numpy as np

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def _maker():
    spec = importlib.util.spec_from_file_location('make_gemm_routes_golden', os.path.join(GOLDEN_DIR, 'make_gemm_routes_golden.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_planner_views_answer_what_the_hand_written_cascades_answered():
    mk = _maker()
    gold = np.load(os.path.join(GOLDEN_DIR, 'gemm_routes.npz'))
    # the recording covers the generator's grid (nothing dropped from either side)
    assert gold['shapes'].tolist() == [list(s) for s in mk.shapes()]
    assert sorted(set(gold['route_cases'][:, 0].tolist())) == list(range(len(gold['shapes'])))
    dll = mk.load()
    before = (dll.rscotr_gemm_get_precision(), dll.rscotr_gemm_set_h3(1))
    dll.rscotr_gemm_set_h3(before[1])
    try:
        now = mk.record(dll, gold['shapes'], gold['route_cases'])
    finally:  # (record restores the modes itself; this holds if it raised half-way)
        dll.rscotr_gemm_set_precision(before[0])
        dll.rscotr_gemm_set_h3(before[1])
    assert (dll.rscotr_gemm_get_precision(), dll.rscotr_gemm_set_h3(before[1])) == before
    for key in ('route', 'bits_ok', 'workspace', 'wplanes_ok', 'wplanes_workspace'):
        assert now[key].shape == gold[key].shape == (len(mk.MODES), gold[key].shape[1]), key
        bad = np.argwhere(now[key] != gold[key])
        assert bad.size == 0, (key, len(bad), [(mk.MODES[m], int(c), int(gold[key][m, c]), int(now[key][m, c])) for m, c in bad[:8]])
    # the grid reaches every answer: no route / plane-fed route / both routes, the bits, both workspace kinds
    full = gold['route'][mk.MODES.index((3, 1))]
    assert set(full.tolist()) == {0, 1, 2} and not gold['route'][:3].any()
    assert gold['bits_ok'][2].any() and not gold['bits_ok'][:2].any()
    assert (gold['workspace'] > 0).any() and (gold['workspace'][0] != gold['workspace'][2]).any()
    assert gold['wplanes_ok'].any() and (gold['wplanes_workspace'] > 0).any()
