"""Every epilogue form of rscotr_gemm_f32_r (tests/gemm_epilogue_cases.py: FORMS) on every kernel route behind plan_gemm (ROUTES),
called on the C ABI with ldc != N, against the fp64 reference of the formula at the head of csrc/gemm.hip.

Per case: the launch-site profiler recorded the row's kernel (and a combine launch exactly where the row is k-sliced); C, pre and
out2 within the project's gates — 1e-5 of max |ref| on the fp32-pipe routes (tests/test_gemm_gpu.py), on the split routes the gate
of tests/test_h3_gpu.py against the error of the same call on the fp32 pipe; the relations that hold without a tolerance (rows of a
zero row-scale factor, elements behind a closed ReLU' gate, out2 = C + resid as one fp32 addition, ReLU of the stored
pre-activation); every element of M x N written and no bit changed in the guard columns and rows around it; the range word the
epilogue (of the combine, for k-sliced rows) committed; two calls with equal bits."""
import ctypes
import functools

import pytest
import torch

import gemm_epilogue_cases as gc
from gemm_epilogue_cases import FORMS, ROUTES, SCALAR_FORMS, SCALAR_ROUTES, SIX_TERM_ROUTES

pytestmark = pytest.mark.gpu

SENTINEL = 0x7fc0beef  # a NaN no kernel computes: whatever still holds these bits was not written


def _ids(cs):
    return [f'{gc.route_id(r)}-{f}' for r, f in cs]


@pytest.fixture
def h3_on():
    """The fp16 split product switched on in the library for the duration of a test (RSCOTR_GEMM_H3 may have started it off)."""
    from rscotr_amd._lib import lib
    old = lib.rscotr_gemm_set_h3(1)
    yield
    lib.rscotr_gemm_set_h3(old)


def _profiled(lib, fn):
    """-> (what fn returned, names of the launches the launch-site profiler recorded meanwhile); as tests/test_dw_kmajor_pipe_gpu.py"""
    lib.call('rscotr_prof_enable', 1, 0, 0, 64)
    try:
        out = fn()
        torch.cuda.synchronize()
        n = lib.rscotr_prof_pause()
        names = []
        kind, work, ms, name = ctypes.c_int(), ctypes.c_double(), ctypes.c_float(), ctypes.create_string_buffer(128)
        for i in range(n):
            lib.call('rscotr_prof_get', i, ctypes.byref(kind), ctypes.byref(work), ctypes.byref(ms), name, 128)
            names.append(name.value.decode())
    finally:
        lib.call('rscotr_prof_disable')
    return out, names


def _room_for_slots(ops, dev, need=8):
    """A case takes its range words from ops.RANGES in call order.  When the buffer is about to wrap — which zeroes every word —
    start a new generation first, so that no word is zeroed between its measurement and the product that reads it."""
    R = ops.RANGES
    R.new_slot(dev)
    if R.n + need > R.dyn:
        was, R.enabled = R.enabled, True
        try:
            R.begin(dev)
        finally:
            R.enabled = was


def _range_word(ops, lib, t, rows, cols, ld):
    slot = ops.RANGES.new_slot(t.device)
    lib.call('rscotr_amax_f32', t.data_ptr(), rows, cols, ld, slot, torch.cuda.current_stream().cuda_stream)
    return slot


@functools.lru_cache(maxsize=2)
def _inputs(r, dev):
    """Seeded operands and epilogue tensors of a ROUTES row and its fp64 product, made once for all forms of the row (the cases
    of a row are neighbours).  aux is independent of the product: no gate sits within rounding of zero."""
    g = torch.Generator().manual_seed(r.M * 7 + r.N * 3 + r.K + 2 * r.ak + r.bk)
    rp = gc.rows_per(r.M)
    t = dict(A=torch.randn((r.K, r.M) if r.ak else (r.M, r.K), generator=g),
             B=torch.randn((r.K, r.N) if r.bk else (r.N, r.K), generator=g) * 0.1,
             bias=torch.randn(r.N + 1, generator=g), aux=torch.randn(r.M, r.N, generator=g),
             resid=torch.randn(r.M, r.N, generator=g), c0=torch.randn(r.M, r.N, generator=g),
             rowscale=torch.rand(-(-r.M // rp), generator=g) + 0.5)
    t['rowscale'][1] = 0.0  # a dropped DropPath sample
    t = {k: v.to(dev) for k, v in t.items()}
    t['product'] = gc.product64(t['A'], t['B'], r.ak, r.bk)
    return t


def _buffer(M, N, ldc, dev, src=None):
    """(M + 3, ldc) floats of sentinel bits with `src` inside M x N"""
    buf = torch.full((M + 3, ldc), SENTINEL, dtype=torch.int32, device=dev).view(torch.float32)
    if src is not None:
        buf[:M, :N] = src
    return buf


def _call(lib, ops, r, f, t, ldc, bias_off, slots, ws):
    """One rscotr_gemm_f32_r call on fresh buffers -> dict(C, pre, out2, slot of the committed range word)"""
    M, N, K, dev = r.M, r.N, r.K, t['A'].device
    C = _buffer(M, N, ldc, dev, t['c0'] if f.accumulate else None)
    pre = _buffer(M, N, ldc, dev) if f.pre else None
    out2 = _buffer(M, N, ldc, dev) if f.out2 else None
    aux = _buffer(M, N, ldc, dev, t['aux']) if f.act in (gc.ACT_RELU_GRAD, gc.ACT_GELU_GRAD) else None
    resid = _buffer(M, N, ldc, dev, t['resid']) if f.resid else None
    bias = t['bias'][bias_off:bias_off + N] if f.bias else None
    ptr = lambda x: x.data_ptr() if x is not None else 0
    out_slot = ops.RANGES.new_slot(dev)
    lib.call('rscotr_gemm_f32_r', t['A'].data_ptr(), t['B'].data_ptr(), C.data_ptr(), M, N, K, t['A'].shape[1], t['B'].shape[1], ldc,
             r.ak, r.bk, ptr(bias), f.act, ptr(aux), ptr(pre), ptr(resid), int(f.accumulate), 0, 0,
             t['rowscale'].data_ptr() if f.rowscale else 0, gc.rows_per(M) if f.rowscale else 0, 0, 0, ptr(out2), ws.data_ptr(),
             ws.numel() * 4, slots[0], slots[1], out_slot, torch.cuda.current_stream().cuda_stream)
    return dict(C=C, pre=pre, out2=out2, slot=out_slot, keep=(aux, resid, bias))


def _errors(res, refs, M, N):
    """error of C / pre / out2 in units of max |ref|"""
    out = {}
    for k, ref in refs.items():
        if ref is not None and res[k] is not None:
            out[k] = float((res[k][:M, :N].double() - ref).abs().max() / (ref.abs().max() + 1e-300))
    return out


def _check_case(cuda, gemm_precision, r, form, ldc_pad=4, bias_off=0, ranges=True):
    from rscotr_amd import ops
    from rscotr_amd._lib import lib
    f = FORMS[form]
    M, N, K = r.M, r.N, r.K
    ldc = N + ldc_pad
    t = _inputs(r, cuda)
    name = gc.expected_name(r, form)
    split = '_h3_' in name or '_bf16x6_' in name
    gemm_precision(r.prec)
    _room_for_slots(ops, cuda)
    ws = torch.empty(max(lib.rscotr_gemm_f32_workspace(M, N, K), 16) // 4, device=cuda)
    slots = (0, 0)
    if ranges and split:
        slots = (_range_word(ops, lib, t['A'], *t['A'].shape, t['A'].shape[1]), _range_word(ops, lib, t['B'], *t['B'].shape, t['B'].shape[1]))
    if not ranges:
        name = name.replace('_h3_', '_bf16x6_')
    tag = f'{gc.route_id(r)} {form} ldc=N+{ldc_pad} bias+{bias_off}'

    # ---- route
    res, names = _profiled(lib, lambda: _call(lib, ops, r, f, t, ldc, bias_off, slots, ws))
    print(f'[cell] {tag}: {names}')
    assert name in names, (name, names)
    assert (gc.COMBINE_NAME in names) == r.sliced, names
    assert sum(n.startswith('rscotr::gemm_') and n != gc.COMBINE_NAME for n in names) == 1, names

    # ---- values
    ref_c, ref_pre, ref_c2 = gc.reference(None, None, r.ak, r.bk, t['bias'][bias_off:bias_off + N] if f.bias else None, f.act, t['aux'],
                                          t['resid'] if f.resid else None, t['c0'], f.accumulate, t['rowscale'] if f.rowscale else None,
                                          gc.rows_per(M), f.out2, product=t['product'])
    refs = dict(C=ref_c, pre=ref_pre if f.pre else None, out2=ref_c2)
    err = _errors(res, refs, M, N)
    if split:
        gemm_precision(0)
        e32 = _errors(_call(lib, ops, r, f, t, ldc, bias_off, (0, 0), ws), refs, M, N)
        gemm_precision(r.prec)
    for k, e in err.items():
        if split:
            gate = min(2.0 * e32[k] + 5e-7, max(1e-6, 1.5 * e32[k])) if K <= 2048 else 2.0 * e32[k] + 5e-7
            print(f'[error] {tag} {k}: {e:.3e} gate {gate:.3e} (fp32 pipe {e32[k]:.3e}) ratio {e / gate:.3f} {name}')
            assert e32[k] <= 1e-5, (k, e32[k])
        else:
            gate = 1e-5
            print(f'[error] {tag} {k}: {e:.3e} gate {gate:.3e} ratio {e / gate:.3f} {name}')
        assert e <= gate, (k, e, gate)

    # ---- exact relations
    C, out2 = res['C'][:M, :N], res['out2'][:M, :N] if f.out2 else None
    zero = torch.zeros((), device=cuda)
    rest = (t['resid'] if f.resid and not f.out2 else zero) + (t['c0'] if f.accumulate else zero)  # resid + old C as fp32 sums
    if f.rowscale:
        rp = gc.rows_per(M)
        assert torch.equal(C[rp:2 * rp], rest.expand(M, N)[rp:2 * rp]), 'rows of the zero row-scale factor hold more than resid + old C'
    if f.act == gc.ACT_RELU_GRAD and not f.rowscale:
        closed = t['aux'] <= 0
        assert torch.equal(C[closed], rest.expand(M, N)[closed]), 'elements behind a closed ReLU\' gate hold more than resid + old C'
    if f.out2:
        assert torch.equal(out2, C + t['resid'] if f.resid else C), 'out2 != C + resid as one fp32 addition'
    if form == 'bias_relu':
        withpre = _call(lib, ops, r, f._replace(pre=1), t, ldc, bias_off, slots, ws)
        assert torch.equal(withpre['C'][:M, :N], withpre['pre'][:M, :N].clamp(min=0)), 'C != relu(pre)'
        assert torch.equal(withpre['C'].view(torch.int32), res['C'].view(torch.int32)), 'storing the pre-activation changed C'

    # ---- nothing else written, everything inside written
    for k in ('C', 'pre', 'out2'):
        if res[k] is not None:
            bits = res[k].view(torch.int32)
            assert not bool((bits[:M, :N] == SENTINEL).any()), f'{k}: elements of M x N not written'
            assert bool((bits[M:] == SENTINEL).all()) and bool((bits[:M, N:] == SENTINEL).all()), f'{k}: guard rows / columns written'

    # ---- the committed range word
    top = float(torch.maximum(C.abs().max(), out2.abs().max() if f.out2 else zero))
    lo, hi = ops.RANGES.word(res['slot'])
    assert lo <= top < hi, (lo, top, hi)

    # ---- two calls, equal bits
    again = _call(lib, ops, r, f, t, ldc, bias_off, slots, ws)
    for k in ('C', 'pre', 'out2'):
        if res[k] is not None:
            assert torch.equal(res[k].view(torch.int32), again[k].view(torch.int32)), f'{k}: two calls on the same inputs differ'


MAIN = gc.cases()


@pytest.mark.parametrize('r,form', MAIN, ids=_ids(MAIN))
def test_epilogue_form_on_route(cuda, gemm_precision, h3_on, r, form):
    _check_case(cuda, gemm_precision, r, form)


SCALAR = gc.cases(SCALAR_ROUTES, SCALAR_FORMS)


@pytest.mark.parametrize('ldc_pad,bias_off', [(1, 0), (4, 1)], ids=['ldc_odd', 'bias_unaligned'])
@pytest.mark.parametrize('r,form', SCALAR, ids=_ids(SCALAR))
def test_scalar_branches(cuda, gemm_precision, h3_on, r, form, ldc_pad, bias_off):
    """p.vecC false — rows of C that are not 16-byte aligned, or a bias that is not: epilogue_one in each of the three combine
    kernels, scalar accesses in a main kernel."""
    _check_case(cuda, gemm_precision, r, form, ldc_pad=ldc_pad, bias_off=bias_off)


SIX = gc.cases(SIX_TERM_ROUTES)


@pytest.mark.parametrize('r,form', SIX, ids=_ids(SIX))
def test_six_term_route(cuda, gemm_precision, six_term, r, form):
    """The six-term bf16 product (RSCOTR_GEMM_H3=0 of the README's table): no range words, gemm_bf16x6_kernel on the same tiles."""
    _check_case(cuda, gemm_precision, r, form, ranges=False)
