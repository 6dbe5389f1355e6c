"""The 128 x 128 fp16 split body with two alternating register sets (csrc/gemm_split_body.h, h3_two_tiles): every corner of its k loop
through the public entries — rscotr_gemm_dw_group variant 7 with a hand-built table (gemm_h3_group_kernel) and the product entry
with both operands k-major (gemm_h3_128_kernel<true, true, *>).  Smallest shapes that reach each corner: one, two, three and an odd
number of k-tiles, a short last k-slice, ragged tiles with and without a k tail, a null and a per-row-block kscale, row sums.

Each case three ways: the family's error gate (tests/test_h3_gpu.py: against fp64 at most max(1e-6, 1.5 x the fp32 pipe's error on
the same operands) of max |C|, on unit operands and on operands scaled by 3e-7 / 40), two calls with equal bits, and the row sums
against the fp64 column sums of A within K 2^-24 sum |terms|."""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GROUP_NAME = 'rscotr::gemm_h3_group_kernel'
PRODUCT_NAME = 'rscotr::gemm_h3_kernel<128, 128, true, true, *>'  # (the launch site's name of gemm_h3_128_kernel<true, true, *>)


@contextlib.contextmanager
def ranges_on(ops):
    """the value-range route for the duration of a test (as tests/test_h3_gpu.py)"""
    old = (ops.RANGES.enabled, ops.RANGES.check, ops.WPLANES.enabled)
    ops.RANGES.enabled, ops.RANGES.check, ops.WPLANES.enabled = True, False, False
    try:
        yield ops.RANGES
    finally:
        ops.RANGES.enabled, ops.RANGES.check, ops.WPLANES.enabled = old


def _profiled(lib, fn):
    """-> (what fn returned, names of the launches the launch-site profiler recorded meanwhile)"""
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


def _range_word(ops, lib, t, rows, cols, ld):
    slot = ops.RANGES.new_slot(t.device)
    lib.call('rscotr_amax_f32', t.data_ptr(), rows, cols, ld, slot, torch.cuda.current_stream().cuda_stream)
    return slot


def _group_call(ops, lib, A, B, M, N, K, klen, ks, per):
    """One problem as a grouped launch of its own (a bundle of 8 rows, 7 of them empty) -> (slabs [splits, M, N], row-sum
    partials [splits, M]); csrc/gemm_group.hip has the table layout."""
    dev = A.device
    splits = -(-K // klen)
    tiles = -(-M // 128) * -(-N // 128)
    slabs = torch.full((splits, M, N), float('nan'), device=dev)
    rs = torch.full((splits, M), float('nan'), device=dev)
    sa, sb = _range_word(ops, lib, A, K, M, M), _range_word(ops, lib, B, K, N, N)
    rng = (ops.RANGES.index(sa) + 1) << 32 | (ops.RANGES.index(sb) + 1)
    row = [A.data_ptr(), B.data_ptr(), slabs.data_ptr(), rs.data_ptr(), ks.data_ptr() if ks is not None else 0, M, N, K, M, N, klen,
           splits, 0, max(per, 1), rng, tiles * splits]
    table = torch.from_numpy(np.asarray([row] + [[0] * 16] * 7, dtype=np.int64)).to(dev)
    lib.call('rscotr_gemm_dw_group', table.data_ptr(), 8, 8 * tiles * splits, 7, 2.0 * M * N * K, ops.RANGES.base,
             torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    left, left_rs = slabs.isnan().nonzero(), rs.isnan().nonzero()
    assert not len(left) and not len(left_rs), f'not written: {len(left)} slab elements (first {left[:3].tolist()}), ' \
                                               f'{len(left_rs)} row-sum partials (first {left_rs[:3].tolist()})'
    return slabs, rs


def _gate(C, rs, A64, B64, ks64, per, e32):
    """the family's error gate on the product, the row-sum bound on the bias gradient (A64 / B64: fp64 [K, M] / [K, N])"""
    K = A64.shape[0]
    f = ks64.repeat_interleave(per)[:K, None] if ks64 is not None else torch.ones(K, 1, dtype=torch.float64, device=A64.device)
    As = A64 * f
    ref = As.t() @ B64
    e = float((C.double() - ref).abs().max() / (ref.abs().max() + 1e-300))
    print(f'error {e:.3e} of max |C| (fp32 pipe {e32:.3e})')
    assert e <= (max(1e-6, 1.5 * e32) if K <= 2048 else 2.0 * e32 + 5e-7), (e, e32)
    bound = K * 2.0 ** -24 * As.abs().sum(0)
    err = (rs.double() - As.sum(0)).abs()
    print(f'row sums: worst error / bound {float((err / (bound + 1e-300)).max()):.3e}')
    assert bool((err <= bound).all())


def _fp32_pipe_error(ops, gemm_precision, A, B, M, N, K, ks, per, ref):
    gemm_precision(0)
    o32 = ops.gemm(A, B, M, N, K, M, N, 1, 1, kscale=ks, krows_per=per if ks is not None else 1)
    gemm_precision(3)
    return float((o32.double() - ref).abs().max() / (ref.abs().max() + 1e-300))


CASES = [  # (M, N, K, k-slice length, krows_per of a kscale | 0)
    (128, 128, 32, 32, 0), (128, 128, 64, 64, 0), (128, 128, 96, 96, 0), (128, 128, 160, 160, 0),  # interior tiles: nk = 1, 2, 3, 5
    (256, 128, 224, 128, 0),   # two slices, the last one short (96)
    (96, 288, 80, 80, 0),      # ragged tiles, a k tail of 16
    (192, 576, 64, 64, 0),     # ragged tiles, interior K
    (128, 128, 96, 96, 32),    # row sums under a per-row-block kscale
]


@pytest.mark.parametrize('sa,sb', [(1.0, 1.0), (3e-7, 40.0)])
@pytest.mark.parametrize('M,N,K,klen,per', CASES)
def test_grouped_launch_corners(cuda, gemm_precision, M, N, K, klen, per, sa, sb):
    from rscotr_amd import ops
    from rscotr_amd._lib import lib
    g = torch.Generator().manual_seed(M + N + K + per)
    A = (torch.randn(K, M, generator=g) * sa).to(cuda)
    B = (torch.randn(K, N, generator=g) * sb).to(cuda)
    ks = (torch.rand(-(-K // per), generator=g) + 0.5).to(cuda) if per else None
    A64, B64, ks64 = A.double(), B.double(), ks.double() if per else None
    f = ks64.repeat_interleave(per)[:K, None] if per else 1.0
    ref = (A64 * f).t() @ B64
    with ranges_on(ops):
        e32 = _fp32_pipe_error(ops, gemm_precision, A, B, M, N, K, ks, per, ref)
        (slabs, rs), names = _profiled(lib, lambda: _group_call(ops, lib, A, B, M, N, K, klen, ks, per))
        assert GROUP_NAME in names and not any('gemm_f32' in n or 'bf16x6' in n for n in names), names
        slabs2, rs2 = _group_call(ops, lib, A, B, M, N, K, klen, ks, per)
    assert torch.equal(slabs, slabs2) and torch.equal(rs, rs2), 'two calls on the same inputs differ'
    _gate(slabs.double().sum(0), rs.double().sum(0), A64, B64, ks64, per, e32)


@pytest.mark.parametrize('sa,sb', [(1.0, 1.0), (3e-7, 40.0)])
@pytest.mark.parametrize('M,N,K,per', [(256, 2048, 10880, 0), (2048, 256, 10880, 5440), (256, 2048, 10896, 0)])
def test_product_entry_kmajor(cuda, gemm_precision, M, N, K, per, sa, sb):
    """dW = A^T B with both operands k-major on the interior 128 x 128 kernel, the FFN weight-gradient shapes (16 k-slices of 22
    k-tiles, combined by the entry itself), and K = 10880 + 16: the edge instantiation, a k tail of 16 in the last slice.  K > 2048: the family's bound for long reductions, 2 x the fp32 pipe's error + 5e-7."""
    from rscotr_amd import ops
    from rscotr_amd._lib import lib
    g = torch.Generator().manual_seed(M + N + K)
    A = (torch.randn(K, M, generator=g) * sa).to(cuda)
    B = (torch.randn(K, N, generator=g) * sb).to(cuda)
    ks = (torch.rand(-(-K // per), generator=g) + 0.5).to(cuda) if per else None
    A64, B64, ks64 = A.double(), B.double(), ks.double() if per else None
    f = ks64.repeat_interleave(per)[:K, None] if per else 1.0
    ref = (A64 * f).t() @ B64

    def run():
        rs = torch.zeros(M, device=cuda)
        return ops.gemm(A, B, M, N, K, M, N, 1, 1, rowsum=rs, kscale=ks, krows_per=per if per else 1), rs

    with ranges_on(ops):
        e32 = _fp32_pipe_error(ops, gemm_precision, A, B, M, N, K, ks, per, ref)
        (C, rs), names = _profiled(lib, run)
        assert PRODUCT_NAME in names, names
        C2, rs2 = run()
    assert torch.equal(C, C2) and torch.equal(rs, rs2), 'two calls on the same inputs differ'
    _gate(C, rs, A64, B64, ks64, per, e32)
