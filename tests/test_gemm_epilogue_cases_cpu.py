"""The cases of tests/test_gemm_epilogue_routes_gpu.py are what they claim to be: the fp64 reference's activation branches against
independent torch forms, the FORMS against the selection predicates of the kernels (every outcome reached, every row selecting
the code it is named after), the row-scale boundaries where the kernels can go wrong, and every ROUTES row against the built
library's host views — a retuned planner threshold fails here by the row's name instead of quietly moving a GPU case onto another
kernel."""
import pytest
import torch
import torch.nn.functional as F

import gemm_epilogue_cases as gc
from gemm_epilogue_cases import FORMS, ROUTES, SCALAR_ROUTES, SIX_TERM_ROUTES


def _operands(M=37, N=29, K=24, ak=0, bk=0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return dict(A=torch.randn((K, M) if ak else (M, K), generator=g), B=torch.randn((K, N) if bk else (N, K), generator=g),
                bias=torch.randn(N, generator=g), aux=torch.randn(M, N, generator=g) * 2.0, resid=torch.randn(M, N, generator=g),
                c0=torch.randn(M, N, generator=g))


@pytest.mark.parametrize('ak,bk', [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_reference_product_layouts(ak, bk):
    t = _operands(ak=ak, bk=bk)
    A = t['A'].double().t() if ak else t['A'].double()
    B = t['B'].double().t() if bk else t['B'].double()
    want = torch.einsum('mk,nk->mn', A, B)
    C, pre, C2 = gc.reference(t['A'], t['B'], ak, bk, None, 0, None, None, None, False, None, 0, False)
    assert C.dtype == torch.float64 and C2 is None
    assert float((C - want).abs().max()) < 1e-12 and torch.equal(C, pre)


def test_reference_act_branches_against_torch():
    t = _operands()
    v = t['A'].double() @ t['B'].double().t() + t['bias'].double()

    def run(act):
        return gc.reference(t['A'], t['B'], 0, 0, t['bias'], act, t['aux'], None, None, False, None, 0, False)

    for act in range(5):
        assert float((run(act)[1] - v).abs().max()) < 1e-12  # the pre-activation: in front of every act
    assert float((run(0)[0] - v).abs().max()) < 1e-12
    assert float((run(1)[0] - v.clamp(min=0)).abs().max()) < 1e-12
    assert float((run(2)[0] - F.gelu(v)).abs().max()) < 1e-12
    assert float((run(3)[0] - v * (t['aux'] > 0)).abs().max()) < 1e-12
    a = t['aux'].double().requires_grad_(True)
    F.gelu(a).sum().backward()
    assert float((run(4)[0] - v * a.grad).abs().max()) < 1e-12
    assert int((t['aux'] > 0).sum()) not in (0, t['aux'].numel())


def test_reference_rowscale_residual_and_second_output():
    t = _operands(M=10)
    v = t['A'].double() @ t['B'].double().t()
    rs = torch.tensor([2.0, 0.0, 0.5, -1.0])
    per_row = torch.tensor([2.0] * 3 + [0.0] * 3 + [0.5] * 3 + [-1.0]).double()[:, None]
    C, _, C2 = gc.reference(t['A'], t['B'], 0, 0, None, 0, None, t['resid'], t['c0'], True, rs, 3, False)
    assert C2 is None and float((C - (v * per_row + t['resid'].double() + t['c0'].double())).abs().max()) < 1e-12
    assert torch.equal(C[3:6], t['resid'].double()[3:6] + t['c0'].double()[3:6])
    C, _, C2 = gc.reference(t['A'], t['B'], 0, 0, None, 0, None, t['resid'], t['c0'], True, rs, 3, True)
    assert float((C - (v * per_row + t['c0'].double())).abs().max()) < 1e-12 and torch.equal(C2, C + t['resid'].double())
    C, _, _ = gc.reference(t['A'], t['B'], 0, 0, None, 0, None, t['resid'], t['c0'], False, None, 0, False)
    assert float((C - (v + t['resid'].double())).abs().max()) < 1e-12  # c0 counts only under accumulate
    C, _, _ = gc.reference(None, None, 0, 0, None, 0, None, None, None, False, None, 0, False, product=v)
    assert torch.equal(C, v)


@pytest.mark.parametrize('name', list(FORMS))
def test_form_selects_the_code_it_is_named_after(name):
    f = FORMS[name]
    assert gc.selects(f) == f.selects, (name, gc.selects(f))
    if f.act in (gc.ACT_RELU_GRAD, gc.ACT_GELU_GRAD) or f.pre or f.rowscale or f.resid or f.accumulate or f.out2 or f.act:
        assert gc.selects(f) != 'plain'
    # tiles without the 16-value batch (128-row tiles): what epilogue_tile16 would take goes through epilogue_rows4
    assert gc.selects(f, tile64=False) == ('rows4' if f.selects.startswith('tile16') else f.selects)


def test_forms_reach_every_selection_outcome():
    got = {gc.selects(f) for f in FORMS.values()}
    assert got == {'plain', 'noload', 'tile16_fast', 'tile16_general', 'rows4', 'rows4_c2'}
    # within each: the variants the code distinguishes
    by = lambda sel: [f for f in FORMS.values() if f.selects == sel]
    assert {bool(f.bias) for f in by('plain')} == {False, True}
    assert {bool(f.pre) for f in by('noload')} == {False, True} and {f.act for f in by('noload')} == {gc.ACT_RELU, gc.ACT_GELU}
    fast = by('tile16_fast')  # one each of: residual, old C, the ReLU' gate
    assert sorted((bool(f.resid), bool(f.accumulate), f.act) for f in fast) == [(False, False, 3), (False, True, 0), (True, False, 0)]
    gen = by('tile16_general')  # GELU', an act in front of a residual, a row scale, a stored pre-activation
    assert any(f.act == gc.ACT_GELU_GRAD for f in gen) and any(f.act == gc.ACT_RELU and f.resid for f in gen)
    assert any(f.rowscale for f in gen) and any(f.pre for f in gen)
    assert any(f.rowscale and not f.resid and not f.accumulate for f in by('rows4'))  # rowscale on its own
    assert any(f.bias and f.pre and f.rowscale and f.resid and f.accumulate and f.act == gc.ACT_GELU_GRAD for f in by('rows4'))
    assert {bool(f.resid) for f in by('rows4_c2')} == {False, True}


@pytest.mark.parametrize('r', ROUTES, ids=gc.route_id)
def test_rowscale_boundaries(r):
    rp, M = gc.rows_per(r.M), r.M
    bounds = [b for b in (rp, 2 * rp, 3 * rp) if b < M]
    assert len(bounds) == 3 and -(-M // rp) == 4  # four samples; the second one (rows rp .. 2 rp) is the dropped one
    for b in bounds:
        assert b % 4 and b % 32, b     # inside a group of 4 rows, inside a 32-row accumulator tile
    if M % 32:
        assert bounds[-1] >= M - M % 32, (bounds, M)  # in the last 32 rows of a ragged M: the ragged last tile of any height


def test_case_lists():
    main = gc.cases()
    kk = [r for r in ROUTES if r.ak and r.bk]
    scaled = [f for f in FORMS if FORMS[f].rowscale]
    assert len(kk) == 5 and len(scaled) == 3 and len(main) == len(ROUTES) * len(FORMS) - len(kk) * len(scaled)
    assert not any(r.ak and r.bk and FORMS[f].rowscale for r, f in main)
    for r, f in main:
        small = 'gemm_small_kernel' in r.name
        assert (r.rowscale_name is not None) == small
        assert gc.expected_name(r, f) == (r.rowscale_name if small and FORMS[f].rowscale else r.name)
    assert len({gc.route_id(r) for r in ROUTES}) == len(ROUTES)
    # one row per combine kernel (splits >= 8 with N % 4 == 0: sg; N % 4 == 0: reduce<true>; else reduce<false>) and a main kernel
    assert [(r.sliced, r.N % 4 == 0, r.K) for r in SCALAR_ROUTES] == [(True, True, 1024), (True, True, 2056), (True, False, 1024), (False, True, 192)]
    assert all('bf16x6' in r.name for r in SIX_TERM_ROUTES)


# ---- the library's own word on every row ----------------------------------------------------------------------------
@pytest.fixture
def planner():
    """The built library's host views with the fp16 split product on; precision mode and switch restored."""
    from rscotr_amd._lib import lib
    prec, h3 = lib.rscotr_gemm_get_precision(), lib.rscotr_gemm_set_h3(1)
    try:
        yield lib
    finally:
        lib.call('rscotr_gemm_set_precision', prec)
        lib.rscotr_gemm_set_h3(h3)


def _route_view(lib, r, has_rowscale=0):
    lib.call('rscotr_gemm_set_precision', r.prec)
    ws = lib.rscotr_gemm_f32_workspace(r.M, r.N, r.K)
    lda, ldb = (r.M if r.ak else r.K), (r.N if r.bk else r.K)
    return lib.rscotr_gemm_f32_split_route(r.M, r.N, r.K, lda, ldb, r.ak, r.bk, 0, 0, has_rowscale, 0, ws), ws


@pytest.mark.parametrize('r', ROUTES + SIX_TERM_ROUTES, ids=gc.route_id)
def test_library_routes_the_row_as_the_table_says(planner, r):
    got, ws = _route_view(planner, r)
    assert got == r.split_route, f'{gc.route_id(r)}: rscotr_gemm_f32_split_route answers {got}, the table says {r.split_route}'
    assert (got > 0) == ('_h3_' in r.name or '_bf16x6_' in r.name)
    if r.sliced:
        assert ws >= 2 * (r.M * r.N + r.M) * 4, 'a k-sliced row without workspace for two slabs'
    if got:  # the tile of the name: 2 = the interior pipelined 64 x 64 kernel
        assert got == 1 or '<64, 64, false' in r.name
        assert planner.rscotr_gemm_relu_bits_ok(r.M, r.N, r.K, r.K, r.N if r.bk else r.K, r.ak, r.bk) == \
            int('<128, 128' in r.name and not r.sliced and r.M % 128 == 0 and r.K % 32 == 0 and not r.ak)
    if not (r.ak and r.bk):
        # a row scale moves no row of the table between the split and the fp32 kernels (small rows go small -> tiled: both 0)
        assert _route_view(planner, r, has_rowscale=1)[0] == got
    else:
        assert _route_view(planner, r, has_rowscale=1)[0] == 0  # the planner keeps row scales off the weight-gradient routes
