"""The item loop of the Swin window-attention kernels (csrc/swin_attn.hip): the backward's register prefetch of the next
item and its LDS -> 16-byte row stores, with the forward beside it, at the smallest shapes that reach each path.
Direct C-ABI calls on buffers with sentinels behind them; the bound is the fp64 anchor of tests/test_swin_attn_gpu.py
(tests/parity.py's ANCHOR_K / ANCHOR_FLOOR per tensor plus the 1e-4 element gate), unchanged."""
import functools
import math

import pytest
import torch

from test_swin_attn_gpu import WATTN_PROW_BYTES, _check_anchor, _inputs

pytestmark = pytest.mark.gpu

SENT = 1234.5
NSENT = 4096


def _loop_plan(B, H, W, heads):
    """Items per workgroup of a head, from the public workspace query (grid rule: per_head = min(B * nW, max(1, 1024 //
    heads)) workgroups per head; workgroup r runs items r, r + per_head, ...)."""
    from rscotr_amd._lib import lib
    nwg = lib.rscotr_swin_wattn_bwd_workspace(B, H, W, heads * 32, heads) // WATTN_PROW_BYTES
    per_head = nwg // heads
    nW = math.ceil(H / 7) * math.ceil(W / 7)
    items = B * nW
    chains = [list(range(r, items, per_head)) for r in range(per_head)]
    return dict(nwg=nwg, per_head=per_head, items=items, nW=nW, chains=chains)


# (B, H, W, heads, shift) -> what the launch must look like for the case to test what it is here for
def _reason_steady(p):       # three-item chains (prefetch in steady state) and two-item chains, last item without successor
    n = [len(c) for c in p['chains']]
    return p['per_head'] == 42 and n.count(3) == 16 and n.count(2) == 26


def _reason_mixed(p):        # one launch with workgroups that prefetch and workgroups that never do
    n = [len(c) for c in p['chains']]
    return p['per_head'] == 341 and n.count(2) == 51 and n.count(1) == 290


def _reason_ragged(p):       # ragged map; the prefetched second item lies in the other image
    two = [c for c in p['chains'] if len(c) == 2]
    return p['nW'] == 30 and p['per_head'] == 42 and len(two) == 18 and all(c[0] // 30 == 0 and c[1] // 30 == 1 for c in two)


def _reason_single(p):       # one window, one workgroup per head: nothing to prefetch
    return p['items'] == 1 and p['per_head'] == 1


SHAPES = {
    'steady': ((4, 35, 35, 24, 3), _reason_steady),
    'mixed': ((2, 98, 98, 3, 0), _reason_mixed),
    'ragged': ((2, 33, 37, 24, 5), _reason_ragged),
    'one_window': ((1, 7, 7, 3, 0), _reason_single),
    'sub_window': ((1, 5, 3, 12, 3), _reason_single),
}

# (shape, with forward output, with qkv bias)
CASES = [(k, True, True) for k in SHAPES] + [('mixed', False, True), ('ragged', False, True),
                                              ('mixed', True, False), ('ragged', True, False)]


@functools.lru_cache(maxsize=None)
def _data(shape, bias):
    B, H, W, heads, shift = SHAPES[shape][0]
    return _inputs(B, H, W, heads, seed=900 + sum(SHAPES[shape][0]), bias=bias)


def _guarded(n, device, dtype=torch.float32, fill=SENT):
    buf = torch.full((n + NSENT,), fill, dtype=dtype, device=device)
    return buf, buf[:n], buf[n:]


def _run(cuda, shape, with_out, bias):
    from rscotr_amd import ops
    from rscotr_amd._lib import lib
    from rscotr_amd.ops.core import _stream
    B, H, W, heads, shift = SHAPES[shape][0]
    C = heads * 32
    qkv, qb, tb, dout = (None if x is None else x.to(cuda) for x in _data(shape, bias))
    _, out, out_tail = _guarded(B * H * W * C, cuda)
    _, dqkv, dqkv_tail = _guarded(B * H * W * 3 * C, cuda)
    nws = lib.rscotr_swin_wattn_bwd_workspace(B, H, W, C, heads)
    _, ws, ws_tail = _guarded(nws, cuda, torch.uint8, 0xA5)
    dqb = torch.zeros(3 * C, device=cuda)
    dtb = torch.zeros(169, heads, device=cuda)
    slots = (ops.RANGES.new_slot(cuda), ops.RANGES.new_slot(cuda)) if ops.RANGES.enabled else (0, 0)
    qbp = 0 if qb is None else qb.data_ptr()
    s = _stream()
    assert lib.rscotr_swin_wattn_fwd(qkv.data_ptr(), qbp, tb.data_ptr(), out.data_ptr(), B, H, W, C, heads, 7, shift,
                                     slots[0], s) == 0
    assert lib.rscotr_swin_wattn_bwd(qkv.data_ptr(), qbp, tb.data_ptr(), dout.data_ptr(), dqkv.data_ptr(),
                                     dqb.data_ptr() if bias else 0, dtb.data_ptr(), B, H, W, C, heads, 7, shift,
                                     out.data_ptr() if with_out else 0, ws.data_ptr(), nws, slots[1], s) == 0
    torch.cuda.synchronize()
    assert bool((out_tail == SENT).all()), 'a store behind out'
    assert bool((dqkv_tail == SENT).all()), 'a store behind dqkv'
    assert bool((ws_tail == 0xA5).all()), 'a store behind the workspace'
    got = dict(out=out.view(B, H * W, C).clone(), dqkv=dqkv.view(B, H * W, 3 * C).clone(),
               dqkv_bias=dqb if bias else None, dtable=dtb)
    words = [ops.RANGES.word(sl) if sl else None for sl in slots]
    return got, words


def test_shapes_reach_the_paths_they_are_here_for(cuda):
    for name, (case, reason) in SHAPES.items():
        assert reason(_loop_plan(*case[:4])), name


@pytest.mark.parametrize('shape,with_out,bias', CASES)
def test_window_attention_item_loop(cuda, shape, with_out, bias):
    """Two runs bit-identical; nothing stored behind out, dqkv or the workspace; the range words bracket the maxima; every
    tensor inside the fp64 anchor."""
    case, reason = SHAPES[shape]
    B, H, W, heads, shift = case
    assert reason(_loop_plan(B, H, W, heads))
    a, _ = _run(cuda, shape, with_out, bias)
    b, words = _run(cuda, shape, with_out, bias)
    for n in a:
        if a[n] is None:
            assert b[n] is None
            continue
        assert torch.equal(a[n], b[n]), f'{n} differs between two runs of the same case'
    for n, wd in zip(('out', 'dqkv'), words):
        if wd is not None:
            lo, hi = wd
            assert lo <= float(b[n].abs().max()) < hi, (n, lo, hi, float(b[n].abs().max()))
    qkv, qb, tb, dout = _data(shape, bias)
    names = ('out', 'dqkv', 'dqkv_bias', 'dtable')
    if H % 7 == 0 and W % 7 == 0 and bias:  # no pad tokens: the qkv-bias gradient of the core is exactly zero (the anchor's
        assert not bool(b['dqkv_bias'].any())  # relative distance is 0 / 0 there)
        names = ('out', 'dqkv', 'dtable')
    _check_anchor(case + (('out' if with_out else 'out=NULL'), ('bias' if bias else 'no bias')), b, qkv, qb, tb, dout,
                  H, W, heads, shift, names=names)
