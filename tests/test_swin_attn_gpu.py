"""Fused Swin window-attention kernels (C ABI) vs the oracle's restatement of mmdet ShiftWindowMSA
(pad, roll, partition, bias, mask, softmax, reverse): forward, and gradients of the input tokens,
qkv / proj weights and biases, and the relative-position bias table."""
import math

import pytest
import torch

from oracle.model import shift_window_msa
from parity import ANCHOR_FLOOR, ANCHOR_K
from wattn_oracle import wattn_eval

pytestmark = pytest.mark.gpu


def _rel(a, ref):
    ref = ref.double()
    return float((a.detach().cpu().double() - ref).abs().max() / (ref.abs().max() + 1e-30))


# (B, H, W, heads, shift): multiples of 7, ragged maps that need padding, maps smaller than a window
CASES = [(2, 14, 14, 3, 0), (2, 14, 14, 3, 3), (1, 16, 16, 3, 3), (2, 9, 20, 6, 3), (1, 5, 3, 12, 3),
         (1, 4, 4, 24, 0), (2, 8, 8, 2, 3), (1, 32, 32, 3, 3)]


@pytest.mark.parametrize('B,H,W,heads,shift', CASES)
def test_window_attention_matches_oracle(cuda, B, H, W, heads, shift):
    from rscotr_amd import ops
    C = heads * 32
    g = torch.Generator().manual_seed(H * 100 + W + shift)
    x = torch.randn(B, H * W, C, generator=g)
    P = {'a.w_msa.qkv.weight': torch.randn(3 * C, C, generator=g) * C ** -0.5,
         'a.w_msa.qkv.bias': torch.randn(3 * C, generator=g) * 0.5,
         'a.w_msa.proj.weight': torch.randn(C, C, generator=g) * C ** -0.5,
         'a.w_msa.proj.bias': torch.randn(C, generator=g) * 0.1,
         'a.w_msa.relative_position_bias_table': torch.randn(169, heads, generator=g)}
    go = torch.randn(B, H * W, C, generator=g)
    # oracle in fp64
    xr = x.double().requires_grad_(True)
    Pr = {k: v.double().requires_grad_(True) for k, v in P.items()}
    yr = shift_window_msa(xr, (H, W), Pr, 'a', heads, 7, shift)
    (yr * go.double()).sum().backward()
    # product
    xd = x.to(cuda).requires_grad_(True)
    Pd = {k: v.to(cuda).requires_grad_(True) for k, v in P.items()}
    y = ops.swin_window_attention(xd, (H, W), Pd['a.w_msa.qkv.weight'], Pd['a.w_msa.qkv.bias'],
                                  Pd['a.w_msa.relative_position_bias_table'], None, Pd['a.w_msa.proj.weight'],
                                  Pd['a.w_msa.proj.bias'], heads, 7, shift)
    (y * go.to(cuda)).sum().backward()
    assert _rel(y, yr) < 1e-4
    assert _rel(xd.grad, xr.grad) < 1e-4
    for k in P:
        assert _rel(Pd[k].grad, Pr[k].grad) < 1e-4, k


def test_window_attention_rejects_bad_geometry(cuda):
    from rscotr_amd import ops
    qkv = torch.randn(1, 49, 3 * 40, device=cuda)  # C = 40 is not heads * 32
    with pytest.raises(RuntimeError):
        ops._SwinWindowAttn.apply(qkv, None, torch.zeros(169, 1, device=cuda), 7, 7, 1, 7, 0)


# ----------------------------------------------------------------------------------------------------------------------
# The core (rscotr_swin_wattn_fwd / _bwd) on its own against the fp64 reference of tests/wattn_oracle.py, at the geometries
# the model runs.  Bound (tests/parity.py's fp64 anchor): per tensor, the relative L2 distance ep of the kernel from the fp64
# evaluation is at most ANCHOR_K x the larger of the fp32 reference's own distances eo (plain exp, and exp in the __expf
# form), floored at ANCHOR_FLOOR; the element-wise 1e-4 gate of test_window_attention_matches_oracle holds as well.  Every
# case runs at its full size: the fp64 reference takes ~1 s on the largest map (Swin-B stage 1 at 1024^2).
# ----------------------------------------------------------------------------------------------------------------------
WATTN_PROW_BYTES = 268 * 4  # one partial row of the backward (csrc/swin_attn.hip: WATTN_PROW floats) per workgroup

# (B, H, W, heads, shift)
MODEL_CASES = [
    # Swin-T at 512^2, B = 2: stages 1-4
    (2, 128, 128, 3, 0), (2, 128, 128, 3, 3), (2, 64, 64, 6, 0), (2, 64, 64, 6, 3),
    (2, 32, 32, 12, 0), (2, 32, 32, 12, 3), (2, 16, 16, 24, 0), (2, 16, 16, 24, 3),
    # Swin-T at 384 x 512, B = 2: stages 1-2
    (2, 96, 128, 3, 3), (2, 48, 64, 6, 0),
    # det at 800^2, B = 4: stages 2-4
    (4, 100, 100, 6, 3), (4, 50, 50, 12, 0), (4, 25, 25, 24, 3),
    # Swin-B at 1024^2, B = 1: stages 1-4
    (1, 256, 256, 4, 0), (1, 128, 128, 8, 3), (1, 64, 64, 16, 0), (1, 32, 32, 32, 3),
]


def _geometry(B, H, W, heads):
    """What the backward launch does with a case, from the public workspace query: workgroups, items (windows) per head,
    whether a workgroup loops over several items, whether one workgroup's items span two images, whether the 3-per-SIMD
    register budget (the <3> instantiation, 512 < nwg <= 768) runs."""
    from rscotr_amd._lib import lib
    nwg = lib.rscotr_swin_wattn_bwd_workspace(B, H, W, heads * 32, heads) // WATTN_PROW_BYTES
    per_head = nwg // heads
    nW = math.ceil(H / 7) * math.ceil(W / 7)
    items = B * nW
    span = any(len({bw // nW for bw in range(b0, items, per_head)}) > 1 for b0 in range(per_head))
    return dict(nwg=nwg, items=items, loop=items > per_head, span=span, occ3=512 < nwg <= 768)


def test_model_cases_reach_the_persistent_loop_and_both_register_budgets(cuda):
    geo = [_geometry(B, H, W, heads) for B, H, W, heads, _ in MODEL_CASES]
    assert all(g['nwg'] > 0 and g['nwg'] % h == 0 for g, (_, _, _, h, _) in zip(geo, MODEL_CASES))
    assert any(g['loop'] for g in geo), 'no case has more items than workgroups per head'
    assert any(g['span'] for g in geo), 'no case has a workgroup whose items belong to two images'
    assert any(g['occ3'] for g in geo), 'no case runs the <3> backward body (512 < nwg <= 768)'
    assert any(not g['occ3'] for g in geo)
    assert {s for *_, s in MODEL_CASES} == {0, 3}


def _l2(a, ref):
    return float((a.detach().cpu().double() - ref).norm() / ref.norm())


def _inputs(B, H, W, heads, seed, bias=True):
    C = heads * 32
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B, H * W, 3 * C, generator=g)
    qb = torch.randn(3 * C, generator=g) * 0.5 if bias else None
    tb = torch.randn(169, heads, generator=g)
    dout = torch.randn(B, H * W, C, generator=g)
    return qkv, qb, tb, dout


def _core_on_gpu(cuda, qkv, qb, tb, dout, H, W, heads, shift):
    """_SwinWindowAttn forward + backward -> (out, dqkv, dqkv_bias | None, dtable); out and dqkv are the tensors the forward
    and the backward returned (they carry the range words the kernels left)."""
    from rscotr_amd import ops
    q = qkv.to(cuda).requires_grad_(True)
    b = None if qb is None else qb.to(cuda).requires_grad_(True)
    t = tb.to(cuda).requires_grad_(True)
    got = []
    q.register_hook(got.append)
    out = ops._SwinWindowAttn.apply(q, b, t, H, W, heads, 7, shift)
    out.backward(dout.to(cuda))
    torch.cuda.synchronize()
    return dict(out=out, dqkv=got[0], dqkv_bias=None if b is None else b.grad, dtable=t.grad)


def _check_anchor(case, got, qkv, qb, tb, dout, H, W, heads, shift, names=('out', 'dqkv', 'dqkv_bias', 'dtable')):
    r64 = wattn_eval(qkv, (H, W), qb, tb, heads, shift, dout, torch.float64)
    r32 = wattn_eval(qkv, (H, W), qb, tb, heads, shift, dout, torch.float32)
    r32f = wattn_eval(qkv, (H, W), qb, tb, heads, shift, dout, torch.float32, exp='expf')
    rows = []
    for n in names:
        if r64[n] is None:
            assert got.get(n) is None, n
            continue
        ep = _l2(got[n], r64[n])
        eo = max(_l2(r32[n], r64[n]), _l2(r32f[n], r64[n]))
        rows.append((n, ep, eo))
        print(f'[wattn anchor] {case} {n}: ep {ep:.3e} eo {eo:.3e} ratio {ep / max(eo, ANCHOR_FLOOR):.2f} '
              f'max-rel {_rel(got[n], r64[n]):.3e}', flush=True)
    for n, ep, eo in rows:
        assert ep <= ANCHOR_K * max(eo, ANCHOR_FLOOR), (case, n, ep, eo)
        assert _rel(got[n], r64[n]) < 1e-4, (case, n)
    return rows


@pytest.mark.parametrize('B,H,W,heads,shift', MODEL_CASES)
def test_window_attention_core_at_model_sizes_against_fp64(cuda, B, H, W, heads, shift):
    """Forward and backward of the core alone at the model's maps: out, dqkv, dqkv_bias and dtable within the fp64 anchor;
    the range words of out and dqkv hold the binade of their maxima; a second run is bit-identical (fixed-order
    reductions, no atomics)."""
    from rscotr_amd import ops
    qkv, qb, tb, dout = _inputs(B, H, W, heads, seed=B * 1000 + H + W + heads + shift)
    runs = [_core_on_gpu(cuda, qkv, qb, tb, dout, H, W, heads, shift) for _ in range(2)]
    for n in runs[0]:
        assert torch.equal(runs[0][n], runs[1][n]), f'{n} differs between two runs of the same case'
    got = runs[1]
    if ops.RANGES.enabled:
        for n in ('out', 'dqkv'):
            slot = ops.RANGES.slot_of(got[n])
            assert slot, f'{n} carries no range word'
            lo, hi = ops.RANGES.word(slot)
            assert lo <= float(got[n].abs().max()) < hi, (n, lo, hi, float(got[n].abs().max()))
    _check_anchor((B, H, W, heads, shift), got, qkv, qb, tb, dout, H, W, heads, shift)


# ---- ABI paths the model does not take
@pytest.mark.parametrize('shift', [1, 2, 4, 5, 6])
def test_window_attention_other_shifts_on_a_ragged_map(cuda, shift):
    B, H, W, heads = 2, 19, 23, 3
    qkv, qb, tb, dout = _inputs(B, H, W, heads, seed=50 + shift)
    got = _core_on_gpu(cuda, qkv, qb, tb, dout, H, W, heads, shift)
    _check_anchor((B, H, W, heads, shift), got, qkv, qb, tb, dout, H, W, heads, shift)


def test_window_attention_without_qkv_bias(cuda):
    """qkv_bias = NULL: the pad tokens are zeros (the kernel's pad_vals = nullptr)."""
    B, H, W, heads, shift = 2, 30, 17, 6, 3
    qkv, _, tb, dout = _inputs(B, H, W, heads, seed=61, bias=False)
    got = _core_on_gpu(cuda, qkv, None, tb, dout, H, W, heads, shift)
    _check_anchor((B, H, W, heads, shift), got, qkv, None, tb, dout, H, W, heads, shift)


def _raw_bwd(cuda, qkv, qb, tb, dout, B, H, W, heads, shift, out):
    from rscotr_amd._lib import lib
    from rscotr_amd.ops.core import _stream
    C = heads * 32
    dqkv = torch.empty_like(qkv)
    dqb = torch.zeros_like(qb)
    dtb = torch.zeros_like(tb)
    nws = lib.rscotr_swin_wattn_bwd_workspace(B, H, W, C, heads)
    ws = torch.empty(nws // 4, dtype=torch.float32, device=cuda)
    rc = lib.rscotr_swin_wattn_bwd(qkv.data_ptr(), qb.data_ptr(), tb.data_ptr(), dout.data_ptr(), dqkv.data_ptr(),
                                   dqb.data_ptr(), dtb.data_ptr(), B, H, W, C, heads, 7, shift,
                                   0 if out is None else out.data_ptr(), ws.data_ptr(), nws, 0, _stream())
    assert rc == 0
    torch.cuda.synchronize()
    return dict(dqkv=dqkv, dqkv_bias=dqb, dtable=dtb)


def test_window_attention_backward_without_the_forward_output(cuda):
    """out = NULL: delta_i = sum_j P_ij dP_ij by the half-wave reduction (half_sum) instead of dO_i . O_i.  Same bound, at a
    geometry whose workgroups loop over items of both images; the same call with the forward output agrees to rounding."""
    from rscotr_amd._lib import lib
    from rscotr_amd.ops.core import _stream
    B, H, W, heads, shift = 2, 64, 64, 6, 3
    assert _geometry(B, H, W, heads)['span']
    qkv, qb, tb, dout = _inputs(B, H, W, heads, seed=71)
    q, b, t, d = (x.to(cuda) for x in (qkv, qb, tb, dout))
    out = torch.empty(B, H * W, heads * 32, device=cuda)
    assert lib.rscotr_swin_wattn_fwd(q.data_ptr(), b.data_ptr(), t.data_ptr(), out.data_ptr(), B, H, W, heads * 32, heads,
                                     7, shift, 0, _stream()) == 0
    no_out = _raw_bwd(cuda, q, b, t, d, B, H, W, heads, shift, None)
    _check_anchor((B, H, W, heads, shift, 'out=NULL'), no_out, qkv, qb, tb, dout, H, W, heads, shift,
                  names=('dqkv', 'dqkv_bias', 'dtable'))
    with_out = _raw_bwd(cuda, q, b, t, d, B, H, W, heads, shift, out)
    for n in no_out:
        assert _rel(no_out[n], with_out[n].cpu()) < 1e-4, n


def test_window_attention_empty_batch_writes_nothing(cuda):
    from rscotr_amd._lib import lib
    from rscotr_amd.ops.core import _stream
    H, W, heads = 14, 14, 3
    C = heads * 32
    qkv = torch.randn(1, H * W, 3 * C, device=cuda)
    tb = torch.randn(169, heads, device=cuda)
    guard = [torch.full((n,), 1234.5, device=cuda) for n in (H * W * C, H * W * 3 * C, 3 * C, 169 * heads, 4096)]
    out, dqkv, dqb, dtb, ws = guard
    assert lib.rscotr_swin_wattn_bwd_workspace(0, H, W, C, heads) == 0
    assert lib.rscotr_swin_wattn_fwd(qkv.data_ptr(), qkv.data_ptr(), tb.data_ptr(), out.data_ptr(), 0, H, W, C, heads, 7, 3,
                                     0, _stream()) == 0
    assert lib.rscotr_swin_wattn_bwd(qkv.data_ptr(), qkv.data_ptr(), tb.data_ptr(), out.data_ptr(), dqkv.data_ptr(),
                                     dqb.data_ptr(), dtb.data_ptr(), 0, H, W, C, heads, 7, 3, out.data_ptr(), ws.data_ptr(),
                                     0, 0, _stream()) == 0
    torch.cuda.synchronize()
    for g_ in guard:
        assert bool((g_ == 1234.5).all())


def test_window_attention_error_returns(cuda):
    """Every argument check of the C ABI returns its code before anything is launched."""
    from rscotr_amd._lib import lib
    from rscotr_amd.ops.core import _stream
    E_SHAPE, E_ALIGN, E_ARG = -1, -2, -5
    B, H, W, heads = 1, 14, 14, 3
    C = heads * 32
    qkv = torch.zeros(B, H * W, 3 * C, device=cuda)
    qb = torch.zeros(3 * C + 4, device=cuda)
    tb = torch.zeros(169, heads, device=cuda)
    out = torch.zeros(B, H * W, C + 4, device=cuda)
    dout = torch.zeros(B, H * W, C + 4, device=cuda)
    dqkv = torch.zeros(B, H * W, 3 * C + 4, device=cuda)
    nws = lib.rscotr_swin_wattn_bwd_workspace(B, H, W, C, heads)
    assert nws == 4 * 3 * WATTN_PROW_BYTES  # (4 windows per head, one workgroup each)
    ws = torch.zeros(nws // 4, device=cuda)
    p = dict(qkv=qkv.data_ptr(), qb=qb.data_ptr(), tb=tb.data_ptr(), out=out.data_ptr(), dout=dout.data_ptr(),
             dqkv=dqkv.data_ptr(), ws=ws.data_ptr())
    s = _stream()

    def fwd(C=C, heads=heads, ws_=7, shift=3, **o):
        a = dict(p, **o)
        return lib.rscotr_swin_wattn_fwd(a['qkv'], a['qb'], a['tb'], a['out'], B, H, W, C, heads, ws_, shift, 0, s)

    def bwd(C=C, heads=heads, ws_=7, shift=3, nbytes=nws, **o):
        a = dict(p, **o)
        return lib.rscotr_swin_wattn_bwd(a['qkv'], a['qb'], a['tb'], a['dout'], a['dqkv'], 0, 0, B, H, W, C, heads, ws_,
                                         shift, a['out'], a['ws'], nbytes, 0, s)

    for f in (fwd, bwd):
        assert f(ws_=8) == E_SHAPE and f(ws_=5) == E_SHAPE
        assert f(C=C + 32) == E_SHAPE and f(C=40, heads=1) == E_SHAPE
        assert f(shift=7) == E_SHAPE and f(shift=-1) == E_SHAPE
        assert f(qkv=0) == E_ARG and f(tb=0) == E_ARG
        assert f(qkv=p['qkv'] + 4) == E_ALIGN and f(qb=p['qb'] + 4) == E_ALIGN
    assert fwd(out=0) == E_ARG and fwd(out=p['out'] + 4) == E_ALIGN
    assert bwd(dout=0) == E_ARG and bwd(dqkv=0) == E_ARG
    assert bwd(dout=p['dout'] + 4) == E_ALIGN and bwd(dqkv=p['dqkv'] + 4) == E_ALIGN
    assert bwd(nbytes=nws - WATTN_PROW_BYTES) == E_ARG and bwd(ws=0) == E_ARG
    for bad in ((B, H, W, C + 32, heads), (B, H, W, 40, 1), (B, 0, W, C, heads), (-1, H, W, C, heads)):
        assert lib.rscotr_swin_wattn_bwd_workspace(*bad) == 0, bad
    torch.cuda.synchronize()
    assert bool((dqkv == 0).all()) and bool((out == 0).all())


# ----------------------------------------------------------------------------------------------------------------------
# The arena route: bias table and qkv bias registered in a FlatAdamW, so that the backward adds their gradients straight
# into the gradient arena — with ops.DEFER on, by leaving its partial rows to the end-of-pass flush (rscotr_swin_wattn_flush,
# one launch for every pending block), with it off, by its own fold launch.  Both read the same partial rows in the same
# order: the results are bit-identical.
# ----------------------------------------------------------------------------------------------------------------------
STAGE_GEOS = [(2, 128, 128, 3, 0), (2, 64, 64, 6, 3), (2, 32, 32, 12, 0)]  # Swin-T at 512^2, stages 1-3


class _Arena:
    """Bias tables and qkv biases of `geos` as parameters of one FlatAdamW (the gradient sink armed)."""

    def __init__(self, cuda, geos, seed):
        from rscotr_amd.optim import FlatAdamW
        self.cuda, self.geos = cuda, geos
        self.params, groups, self.data = [], [], []
        for i, (B, H, W, heads, shift) in enumerate(geos):
            qkv, qb, tb, _ = _inputs(B, H, W, heads, seed=seed + i)
            t, b = torch.nn.Parameter(tb.to(cuda)), torch.nn.Parameter(qb.to(cuda))
            self.params.append((t, b))
            groups += [dict(name=f'b{i}.table', param=t, lr=1e-3, weight_decay=0.0),
                       dict(name=f'b{i}.qkv_bias', param=b, lr=1e-3, weight_decay=0.0)]
        self.opt = FlatAdamW(groups)

    def inputs(self, i, seed):
        B, H, W, heads, _ = self.geos[i]
        qkv, _, _, dout = _inputs(B, H, W, heads, seed=seed)
        return qkv.to(self.cuda).requires_grad_(True), dout.to(self.cuda)

    def forward(self, i, qkv):
        from rscotr_amd import ops
        _, H, W, heads, shift = self.geos[i]
        t, b = self.params[i]
        return ops._SwinWindowAttn.apply(qkv, b, t, H, W, heads, 7, shift)

    def grads(self):
        torch.cuda.synchronize()
        return [(t.grad.clone(), b.grad.clone()) for t, b in self.params]

    def close(self):
        from rscotr_amd import ops
        ops.DEFER.enabled = True
        ops.DEFER.drop()
        self.opt.close()


def _flush_planned(ops):
    """Flush the pending deferred work -> the number of rscotr_swin_wattn_flush launches it planned."""
    sig = tuple(ops.DEFER.wattn_entries)
    ops.flush_deferred()
    assert not ops.DEFER.pending()
    return len(ops.DEFER.wattn_cache[sig]) if sig else 0


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def test_deferred_flush_matches_the_immediate_fold_bit_for_bit(cuda):
    """One block: DEFER on (partial rows to wattn_param_flush_kernel at the end of the pass) against DEFER off (the backward's
    own wattn_param_fold_kernel): dtable, dqkv_bias and dqkv identical.  Then accumulation into a pre-filled arena:
    G0 + (the result from zero), bit for bit."""
    from rscotr_amd import ops
    A = _Arena(cuda, STAGE_GEOS[:1], seed=80)
    try:
        qkv, dout = A.inputs(0, seed=90)
        res = {}
        for mode in (True, False):
            ops.DEFER.enabled = mode
            A.opt.zero_grad()
            qkv.grad = None
            A.forward(0, qkv).backward(dout)
            assert len(ops.DEFER.wattn_entries) == (1 if mode else 0)
            assert _flush_planned(ops) == (1 if mode else 0)
            res[mode] = (A.grads()[0], qkv.grad.clone())
        (t1, b1), dq1 = res[True]
        (t0, b0), dq0 = res[False]
        assert float(t1.abs().max()) > 0 and float(b1.abs().max()) > 0
        assert torch.equal(t1, t0) and torch.equal(b1, b0) and torch.equal(dq1, dq0)
        g = torch.Generator().manual_seed(91)
        G0 = torch.randn(A.opt.flat_g.numel(), generator=g).to(cuda)
        for mode in (True, False):
            ops.DEFER.enabled = mode
            A.opt.zero_grad()
            A.opt.flat_g.copy_(G0)
            (g0_t, g0_b), = A.grads()
            A.forward(0, qkv).backward(dout)
            ops.flush_deferred()
            (t, b), = A.grads()
            assert torch.equal(t, g0_t + t1) and torch.equal(b, g0_b + b1), mode
    finally:
        A.close()


def test_one_flush_folds_three_blocks_as_each_alone(cuda):
    """Stages 1-3 in one backward pass: one flush launch with n = 3 entries over 3 + 6 + 12 heads (the entry lookup by first
    head); every destination bit-identical to its block run alone."""
    from rscotr_amd import ops
    A = _Arena(cuda, STAGE_GEOS, seed=100)
    try:
        xs = [A.inputs(i, seed=110 + i) for i in range(3)]
        alone = []
        for i, (qkv, dout) in enumerate(xs):
            A.opt.zero_grad()
            A.forward(i, qkv).backward(dout)
            assert _flush_planned(ops) == 1
            alone.append(A.grads()[i])
        A.opt.zero_grad()
        for qkv, _ in xs:
            qkv.grad = None
        outs = [A.forward(i, qkv) for i, (qkv, _) in enumerate(xs)]
        torch.autograd.backward(outs, [d for _, d in xs])
        ents = ops.DEFER.wattn_entries
        assert len(ents) == 3 and sum(e[3] for e in ents) == 21
        assert _flush_planned(ops) == 1
        for i, (got, want) in enumerate(zip(A.grads(), alone)):
            assert float(want[0].abs().max()) > 0
            assert _same(got, want), f'block {i}'
    finally:
        A.close()


def test_two_passes_into_one_destination_before_the_flush(cuda):
    """Gradient accumulation without a flush in between (FlatAdamW.launch_step tolerates a skipped flush), and one forward that
    applies the same block twice: two pending entries with the same destinations.  The combine is a plain read-add-write,
    so they must go to successive flush launches; the result is then the fp32 sum of the two single-pass results, bit for
    bit."""
    from rscotr_amd import ops
    A = _Arena(cuda, STAGE_GEOS[1:2], seed=120)
    try:
        xs = [A.inputs(0, seed=130 + k) for k in range(2)]
        single = []
        for qkv, dout in xs:
            A.opt.zero_grad()
            A.forward(0, qkv).backward(dout)
            assert _flush_planned(ops) == 1
            single.append(A.grads()[0])
        want = (single[0][0] + single[1][0], single[0][1] + single[1][1])
        # two backward passes, one flush
        A.opt.zero_grad()
        for qkv, dout in xs:
            A.forward(0, qkv).backward(dout)
        assert len(ops.DEFER.wattn_entries) == 2
        planned = _flush_planned(ops)
        got = A.grads()[0]
        assert _same(got, want), 'two passes: an update to a shared destination was lost'
        assert planned == 2
        # one forward through the block twice, one backward
        A.opt.zero_grad()
        outs = [A.forward(0, qkv) for qkv, _ in xs]
        torch.autograd.backward(outs, [d for _, d in xs])
        assert len(ops.DEFER.wattn_entries) == 2
        planned = _flush_planned(ops)
        got = A.grads()[0]
        assert _same(got, want), 'block applied twice: an update to a shared destination was lost'
        assert planned == 2
    finally:
        A.close()


# ----------------------------------------------------------------------------------------------------------------------
# One Swin stage on the arena, as the runner executes it: two blocks (shift 0, then 3) and PatchMerging with every parameter
# in a FlatAdamW, DropPath scales with zero keeps, value ranges verified as they are used, and the LayerNorm / PatchMerging
# folds and the window-attention folds all left to one flush_deferred.  Against the oracle's composition (swin_forward's
# loop body) in fp64, with the same anchor rule; eo is the oracle's own distance in fp32.  GELU, no ReLU gates: no coin-toss
# decisions, so parity.py's amb term is zero.
# ----------------------------------------------------------------------------------------------------------------------
STAGE_CASES = [(2, 128, 128, 96, 3), (2, 32, 32, 384, 12)]  # Swin-T at 512^2, B = 2: stage 1 and stage 3 (nwg = 600: <3>)
DROP_RATES = (0.2, 0.5)  # (1 / (1 - rate) is exact in fp32)
DROP_KEEP = ((1, 0), (1, 1), (0, 1), (1, 1))  # (attn, ffn) of block 0, then of block 1; per image


def _stage_oracle(P, x, dout, hw, heads, dtype):
    import torch.nn.functional as F
    from oracle.model import _droppath, _ln
    Pd = {k: v.detach().cpu().to(dtype).requires_grad_(True) for k, v in P.items()}
    xd = x.detach().cpu().to(dtype).requires_grad_(True)
    y = xd
    for b in range(2):
        bp = f'blocks.{b}'
        ka, kf = (torch.tensor(DROP_KEEP[2 * b + j], dtype=dtype) for j in range(2))
        t = shift_window_msa(_ln(y, Pd, bp + '.norm1'), hw, Pd, bp + '.attn', heads, 7, 0 if b == 0 else 3)
        y = y + _droppath(t, ka, DROP_RATES[b])
        t = F.linear(F.gelu(F.linear(_ln(y, Pd, bp + '.norm2'), Pd[bp + '.ffn.layers.0.0.weight'],
                                     Pd[bp + '.ffn.layers.0.0.bias'])), Pd[bp + '.ffn.layers.1.weight'], Pd[bp + '.ffn.layers.1.bias'])
        y = y + _droppath(t, kf, DROP_RATES[b])
    B, L, C = y.shape
    m = y.view(B, hw[0], hw[1], C).permute(0, 3, 1, 2)
    m = F.pad(m, (0, hw[1] % 2, 0, hw[0] % 2))
    m = F.unfold(m, kernel_size=2, stride=2).transpose(1, 2)
    out = F.linear(_ln(m, Pd, 'downsample.norm'), Pd['downsample.reduction.weight'])
    out.backward(dout.cpu().to(dtype))
    return dict(out=out.detach().double(), x=xd.grad.double(), **{k: v.grad.double() for k, v in Pd.items()})


@pytest.mark.parametrize('B,H,W,C,heads', STAGE_CASES)
def test_swin_stage_on_the_arena_against_fp64(cuda, B, H, W, C, heads):
    from parity import ranges_checked
    from rscotr_amd import ops
    from rscotr_amd.optim import FlatAdamW
    from rscotr_amd.swin import PatchMerging, SwinBlockSequence
    g = torch.Generator().manual_seed(C + heads)
    seq = SwinBlockSequence(C, heads, 4 * C, 2, 7, True, list(DROP_RATES), PatchMerging(C, 2 * C))
    P = {}
    for n, p in seq.named_parameters():
        if n.endswith('relative_position_bias_table'):
            v = torch.randn(p.shape, generator=g) * 0.5
        elif 'norm' in n:
            v = (1.0 if n.endswith('weight') else 0.0) + torch.randn(p.shape, generator=g) * 0.1
        elif n.endswith('bias'):
            v = torch.randn(p.shape, generator=g) * 0.1
        else:
            v = torch.randn(p.shape, generator=g) * p.shape[1] ** -0.5
        P[n] = v
        with torch.no_grad():
            p.copy_(v)
    x = torch.randn(B, H * W, C, generator=g)
    dout = torch.randn(B, (H // 2) * (W // 2), 2 * C, generator=g)
    seq = seq.to(cuda)
    names = [n for n, _ in seq.named_parameters()]
    opt = FlatAdamW([dict(name=n, param=p, lr=1e-3, weight_decay=0.0) for n, p in seq.named_parameters()])
    try:
        keep = torch.tensor(DROP_KEEP, dtype=torch.float32, device=cuda)
        rate = torch.tensor(DROP_RATES, device=cuda).repeat_interleave(2)[:, None]
        scales = keep / (1.0 - rate)
        opt.zero_grad()
        with ranges_checked() as R:
            R.begin(cuda)
            xd = x.to(cuda).requires_grad_(True)
            y, hw = xd, (H, W)
            for i, blk in enumerate(seq.blocks):
                y = blk(y, hw, scales[2 * i], scales[2 * i + 1])
            y, hw = seq.downsample(y, hw)
            assert hw == (H // 2, W // 2)
            y.backward(dout.to(cuda))
            assert ops.DEFER.ln_entries and len(ops.DEFER.wattn_entries) == 2
            assert _flush_planned(ops) == 1
            assert R.enabled is False or R.stats.get('checked', 0) > 0
        torch.cuda.synchronize()
        got = dict(out=y.detach(), x=xd.grad, **{n: p.grad.clone() for n, p in seq.named_parameters()})
    finally:
        ops.DEFER.drop()
        opt.close()
    r64 = _stage_oracle(P, x, dout, (H, W), heads, torch.float64)
    r32 = _stage_oracle(P, x, dout, (H, W), heads, torch.float32)
    rows = []
    for n in ['out', 'x'] + names:
        ep, eo = _l2(got[n], r64[n]), _l2(r32[n], r64[n])
        rows.append((n, ep, eo))
        print(f'[stage anchor] {(B, H, W, C, heads)} {n}: ep {ep:.3e} eo {eo:.3e} ratio {ep / max(eo, ANCHOR_FLOOR):.2f}',
              flush=True)
    bad = [r for r in rows if r[1] > ANCHOR_K * max(r[2], ANCHOR_FLOOR)]
    assert not bad, bad
