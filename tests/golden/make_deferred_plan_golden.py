"""Recorded launch plans of the deferred end-of-backward work and of the three weight-plane caches (rscotr_amd.ops: DEFER, WPLANES /
HPLANES / FPLANES), for tests/test_deferred_plan_cpu.py.

The planners are host code: with `lib.call` and the stream handle stubbed and a CPU device they plan and "launch" without a GPU and
without the library.  `record()` feeds a fixed synthetic pending set and returns every device table a launch was handed (read back
through the pointer the launch received) plus the sequence of (entry point, scalar arguments).  Slab addresses are stored relative to
the first slab block, plane addresses as the index of their cache entry; every other address is a made-up constant.

    python tests/golden/make_deferred_plan_golden.py      # rewrites tests/golden/deferred_plan.npz

The committed file was written by this script on the commit BEFORE the operator layer was split into planes / deferred / fused /
matmul: it pins that the split changed no table and no launch."""
import ctypes
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'deferred_plan.npz')
RANGE_BASE = 0x70000000


def _read(ptr, count, ctype, dtype):
    return np.ctypeslib.as_array((ctype * count).from_address(ptr)).astype(dtype).copy()


def _i64(ptr, rows, cols):
    return _read(ptr, rows * cols, ctypes.c_int64, np.int64).reshape(rows, cols)


def _i32(ptr, rows, cols):
    return _read(ptr, rows * cols, ctypes.c_int32, np.int32).reshape(rows, cols)


class _Param:
    """Stand-in for a parameter tensor: an address, a shape, a device."""

    def __init__(self, ptr, shape):
        self.ptr, self.shape, self.device = ptr, shape, torch.device('cpu')

    def data_ptr(self):
        return self.ptr


class _Sink:
    def __init__(self, seq):
        self.seq = seq

    def params_changed(self):
        self.seq.append('params_changed')

    def _on_ready(self, i):
        self.seq.append(f'on_ready|{i}')


def record():
    """-> (tables: {name: array}, sequence: [str])"""
    from rscotr_amd import ops
    from rscotr_amd._lib import lib
    D, R = ops.DEFER, ops.RANGES
    caches = (ops.WPLANES, ops.HPLANES, ops.FPLANES)
    tables, seq = {}, []

    def rel(col):  # slab addresses relative to the first block (0 stays 0: "no row sums")
        base = D.blocks[0].data_ptr()
        return np.where(col != 0, col - base, 0)

    def call(name, *args):
        assert args[-1] == 0, 'the stubbed stream handle'
        tabs, scal = [], args[1:-1]
        if name.startswith('rscotr_gemm_split_weights'):
            t = _i64(args[0], args[1], 8 if name == 'rscotr_gemm_split_weights' else 9)
            index = {e['planes'].data_ptr(): i for c in caches for i, e in enumerate(c.entries.values())}
            t[:, 1] = [index[p] for p in t[:, 1]]
            tabs = [t]
        elif name in ('rscotr_layernorm_flush', 'rscotr_splitk_flush'):
            wg = _i32(args[1], args[2], 2)
            t = _i64(args[0], int(wg[:, 0].max()) + 1, 5 if name == 'rscotr_layernorm_flush' else 8)
            t[:, 0] = rel(t[:, 0])
            if name == 'rscotr_splitk_flush':
                t[:, 1] = rel(t[:, 1])
            tabs, scal = [t, wg], args[2:-1]
        elif name == 'rscotr_swin_wattn_flush':
            t = _i64(args[0], args[1], 16)
            t[:, 0] = rel(t[:, 0])
            tabs = [t]
        elif name == 'rscotr_gemm_dw_group':
            t = _i64(args[0], args[1], 16)
            t[:, 2], t[:, 3] = rel(t[:, 2]), rel(t[:, 3])
            tabs = [t]
        elif name == 'rscotr_amax_group':
            tabs = [_i64(args[0], args[1], 6)]
        else:
            raise AssertionError(f'unexpected entry point {name}')
        for j, t in enumerate(tabs):
            tables[f'call{len(seq):03d}_{j}'] = t
        seq.append(name + '|' + ','.join(repr(a) for a in scal))

    def fill():
        cpu = torch.device('cpu')
        # split-K slabs: two contractions into one destination (one with row sums), row sums only, another destination
        for out, rs, M, N, sp in ((0x100000, 0x180000, 8, 16, 2), (0x100000, 0, 8, 16, 3), (0, 0x180000, 8, 16, 2),
                                  (0x110000, 0x181000, 12, 20, 4)):
            slab = D.reserve(sp * (M * N + M) * 4, cpu)
            D.entries.append((slab, slab + sp * M * N * 4 if rs else 0, out, rs, M, N, N, sp))
        # LayerNorm partials: the first destination three times, (dw, db) pairs that overlap in one address only
        for dw, db, rows, C in ((0x200000, 0x200400, 4, 96), (0x201000, 0, 2, 192), (0x200000, 0x200400, 4, 96),
                                (0x202000, 0x200400, 1, 96), (0x200000, 0x200400, 3, 96)):
            D.ln_entries.append((D.reserve(rows * 8 * C, cpu), dw, db, rows, C))
        # window-attention partials: one block twice
        for dt, db, heads, C, rows in ((0x300000, 0x300800, 3, 96, 2), (0x301000, 0, 6, 192, 1), (0x300000, 0x300800, 3, 96, 2)):
            D.wattn_entries.append((D.reserve(heads * 268 * 4 * rows, cpu), dt, db, heads, C, rows))
        # grouped problems {a, b, out, rowsum, kscale, M, N, K, lda, ldb, krows_per, range a, range b}: fp32 members (0), members of
        # the six-term body (6), members with both ranges (7), one as the 11 fields a caller without ranges appends
        s = lambda i: RANGE_BASE + 4 * i
        D.group.extend([
            (0x400000, 0x410000, 0x500000, 0x580000, 0, 4, 256, 1600, 4, 256, 1, 0, 0),
            (0x401000, 0x411000, 0x501000, 0, 0, 100, 20, 40, 100, 20, 1, 0, 0),
            (0x402000, 0x412000, 0x502000, 0x582000, 0x590000, 96, 48, 4096, 96, 48, 2048, 0, 0),
            (0x403000, 0x413000, 0x503000, 0, 0, 256, 256, 1600, 256, 256, 1, s(5), s(9)),
            (0x404000, 0x414000, 0x503000, 0x583000, 0, 256, 256, 1600, 256, 256, 1, s(6), s(9)),
            (0x405000, 0x415000, 0x505000, 0, 0, 192, 192, 8192, 192, 192, 1, s(7), 0),
            (0x406000, 0x416000, 0x506000, 0x586000, 0, 128, 64, 512, 128, 64, 1),
            (0x407008, 0x417000, 0x507000, 0, 0, 64, 64, 1024, 64, 64, 1, s(8), s(8)),
        ])
        D.group_keep.append(torch.zeros(1))
        D.group_amax = {(0x403000, 1600, 256, 256): s(5), (0x404000, 1600, 256, 256): s(6), (0x405000, 8192, 192, 192): s(7)}
        D.notify.extend([3, 1])

    mods = [m for n, m in sys.modules.items() if n.startswith('rscotr_amd.ops.') and hasattr(m, '_stream')]
    saved = [dict(o.__dict__) for o in (D, *caches)]
    old = (R.enabled, R.base, dict(R.stats), ops.STATE.grad_sink, [m._stream for m in mods])
    try:
        for o in (D, *caches):
            o.__init__()
        D.BLOCK = 32 << 20
        R.enabled, R.base = True, RANGE_BASE
        ops.STATE.grad_sink = _Sink(seq)
        lib.call = call
        for m in mods:
            m._stream = lambda: 0
        for voided in (False, False, True):  # (the second pass finds every table in its cache)
            fill()
            if voided:  # the range words were zeroed while the problems were pending
                ops._ranges_invalidated()
            seq.append('flush')
            ops.flush_deferred()
            assert not D.pending() and not D.notify and len(D.blocks) == 1
        # the plane caches: two sets of one task, split one by one on first use and together after the parameters changed
        ops.WPLANES.begin('task')
        w1, w2 = _Param(0x600000, (64, 32)), _Param(0x610000, (32, 64))
        gets = (('W', ops.WPLANES, lambda: ops.WPLANES.get(w1, 64, 32, 32, 0), lambda: ops.WPLANES.get(w2, 64, 32, 64, 1)),
                ('H', ops.HPLANES, lambda: ops.HPLANES.get(w1, 64, 32, 32, 0, 0x7100), lambda: ops.HPLANES.get(w2, 64, 32, 64, 1, 0x7104)),
                ('F', ops.FPLANES, lambda: ops.FPLANES.get(w1, 0, 0x7100), lambda: ops.FPLANES.get(w2, 1, 0x7104)))
        results = []
        for label, cache, g1, g2 in gets:
            seq.append(f'planes|{label}')
            first = (g1(), g2())
            ops.WPLANES.bump()
            again = (g1(), g2())
            assert first == again
            planes = [e['planes'].data_ptr() for e in cache.entries.values()]
            for r in first:  # (planes pointer[, padded rows]) -> (entry index[, padded rows])
                r = r if isinstance(r, tuple) else (r,)
                results.append((planes.index(r[0]),) + tuple(r[1:]) + (0,) * (2 - len(r)))
        tables['plane_results'] = np.asarray(results, dtype=np.int64)
    finally:
        del lib.call
        for o, d in zip((D, *caches), saved):
            o.__dict__.clear()
            o.__dict__.update(d)
        R.enabled, R.base, R.stats, ops.STATE.grad_sink = old[:4]
        for m, f in zip(mods, old[4]):
            m._stream = f
    return tables, seq


if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    tabs, sequence = record()
    np.savez_compressed(GOLDEN, sequence=np.asarray(sequence), **tabs)
    print(f'{GOLDEN}: {len(tabs)} tables, {len(sequence)} sequence lines, {os.path.getsize(GOLDEN)} bytes')
