"""The window-attention reference of tests/wattn_oracle.py anchored to the oracle: in fp64, qkv Linear -> wattn_core -> proj
Linear must be oracle.model.shift_window_msa, output and every gradient, up to fp64 rounding of the same operations in a
different association (1e-12 relative).  Ragged maps, maps smaller than one window, every shift the kernel ABI accepts
(0..6) and a block without qkv bias."""
import pytest
import torch
import torch.nn.functional as F

from oracle.model import shift_window_msa
from wattn_oracle import wattn_core

# (B, H, W, heads, shift, qkv bias)
CASES = [(2, 14, 14, 3, 3, True), (1, 5, 3, 4, 3, True), (2, 9, 20, 2, 1, True), (1, 16, 16, 2, 6, False),
         (2, 8, 8, 3, 0, True), (1, 11, 13, 2, 4, True), (1, 10, 12, 2, 2, True), (2, 6, 15, 3, 5, False),
         (1, 4, 4, 2, 3, False)]


def _rel(a, ref):
    return float((a.detach() - ref).abs().max() / ref.abs().max())


def test_cases_cover_every_shift_and_edge():
    assert {c[4] for c in CASES} == set(range(7))
    assert any(c[1] % 7 or c[2] % 7 for c in CASES) and any(c[1] < 7 and c[2] < 7 for c in CASES)
    assert not all(c[5] for c in CASES)


@pytest.mark.parametrize('B,H,W,heads,shift,bias', CASES)
def test_core_reference_restates_shift_window_msa(B, H, W, heads, shift, bias):
    C = heads * 32
    g = torch.Generator().manual_seed(H * 100 + W + shift)
    d = torch.float64
    x = torch.randn(B, H * W, C, generator=g, dtype=d)
    P = {'a.w_msa.qkv.weight': torch.randn(3 * C, C, generator=g, dtype=d) * C ** -0.5,
         'a.w_msa.proj.weight': torch.randn(C, C, generator=g, dtype=d) * C ** -0.5,
         'a.w_msa.proj.bias': torch.randn(C, generator=g, dtype=d) * 0.1,
         'a.w_msa.relative_position_bias_table': torch.randn(169, heads, generator=g, dtype=d)}
    if bias:
        P['a.w_msa.qkv.bias'] = torch.randn(3 * C, generator=g, dtype=d) * 0.5
    go = torch.randn(B, H * W, C, generator=g, dtype=d)

    xr = x.clone().requires_grad_(True)
    Pr = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    yr = shift_window_msa(xr, (H, W), Pr, 'a', heads, 7, shift)
    yr.backward(go)

    xc = x.clone().requires_grad_(True)
    Pc = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    qb = Pc.get('a.w_msa.qkv.bias')
    qkv = F.linear(xc, Pc['a.w_msa.qkv.weight'], qb)
    o = wattn_core(qkv, (H, W), qb, Pc['a.w_msa.relative_position_bias_table'], heads, shift)
    y = F.linear(o, Pc['a.w_msa.proj.weight'], Pc['a.w_msa.proj.bias'])
    y.backward(go)

    assert y.dtype == torch.float64
    assert _rel(y, yr) <= 1e-12
    assert _rel(xc.grad, xr.grad) <= 1e-12
    for k in P:
        assert _rel(Pc[k].grad, Pr[k].grad) <= 1e-12, k


def test_expf_form_is_the_same_function():
    """exp='expf' only changes how exp is rounded: in fp64 it agrees with the plain softmax to rounding."""
    g = torch.Generator().manual_seed(1)
    d = torch.float64
    qkv = torch.randn(2, 9 * 20, 3 * 64, generator=g, dtype=d)
    qb, tb = torch.randn(3 * 64, generator=g, dtype=d), torch.randn(169, 2, generator=g, dtype=d)
    a = wattn_core(qkv, (9, 20), qb, tb, 2, 3)
    b = wattn_core(qkv, (9, 20), qb, tb, 2, 3, exp='expf')
    assert _rel(b, a) <= 1e-13
