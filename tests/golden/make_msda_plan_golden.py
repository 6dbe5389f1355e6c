"""Recorded answers of the MSDA host queries, for tests/test_msda_plan_cpu.py: rscotr_msda_bwd_workspace,
rscotr_msda_bwd_tiled_workspace and rscotr_msda_fused_ok over a census of geometries.  None of them touches a device: the library
is loaded with ctypes and asked.

    python tests/golden/make_msda_plan_golden.py      # rewrites tests/golden/msda_plan.npz

The committed file was written by this script on the commit BEFORE csrc/msda.hip was split by backward strategy behind
plan_msda_bwd: it pins that the two workspace queries, which the planner and rscotr_amd/ops/deform.py both decide from, answer
what the hand-written cascade answered.

The census:
  * the pyramids of BASELINE configs 1, 3 and 4 (512^2, 800^2, Swin-B 1024^2) and those of tests/test_msda_gpu.py;
  * a 17-level list cut to its first L levels for L = 1 .. 17 (the tiled strategy ends at 8 levels, the sorted one at 16);
  * extents of 32 766 and 32 767 on either axis (the tiled bin word holds 15 bits per axis), a 20 000^2 map (more than 2^20
    tile workgroups), the degenerate [(1, 30000), (2, 2)] whose bin bound exceeds the sorted strategy's LDS histogram;
  * a level list whose token sum differs from Nk (one more, one fewer);
  * per pyramid D in {16, 32, 64} x P in {1, 2, 4, 8} x Nq from 0 to 21 760 and on both sides of 2^20 x B in {1, 2} at H = 8,
    then the degenerate arguments one at a time (B, H, P, Nk, L of 0 or below, D = 24, P = 3, no host shapes);
  * rscotr_msda_fused_ok over Nk up to the 2^31 element limit, H, D, L = 1 .. 17 and P."""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
GOLDEN = os.path.join(HERE, 'msda_plan.npz')
MAXL = 17

_NINE = [(5, 4), (4, 4), (4, 3), (3, 3), (3, 2), (2, 2), (2, 1), (1, 2), (1, 1)]
_SEVENTEEN = (_NINE + _NINE)[:17]
PYRAMIDS = [
    [(64, 64), (32, 32), (16, 16), (8, 8)],          # configs[1]
    [(100, 100), (50, 50), (25, 25), (13, 13)],      # configs[3]
    [(128, 128), (64, 64), (32, 32), (16, 16)],      # configs[4]
    [(12, 9), (6, 5), (3, 3), (2, 1)],               # tests/test_msda_gpu.py from here
    [(8, 8), (4, 4), (2, 2), (1, 1)],
    [(8, 8), (4, 4)],
    [(4, 4)],
    [(16, 16), (8, 8), (4, 4), (2, 2)],
    [(15, 11), (8, 6), (4, 3), (2, 2)],
    [(1, 30000), (2, 2)],
    [(1, 32766)], [(32766, 1)], [(1, 32767)], [(32767, 1)], [(3, 3), (32767, 2)],
    [(20000, 20000)],
] + [_SEVENTEEN[:L] for L in range(1, MAXL + 1)]
NQS = (0, 1, 37, 65, 300, 511, 512, 513, 800, 1100, 5440, 13294, 21760, (1 << 20) - 1, 1 << 20)


def cases():
    """-> list of (pyramid index or -1 for no host shapes, B, Nk, Nq, H, D, L, P)"""
    out = []
    for i, pyr in enumerate(PYRAMIDS):
        L, Nk = len(pyr), sum(h * w for h, w in pyr)
        for D in (16, 32, 64):
            for P in (1, 2, 4, 8):
                for Nq in NQS + (Nk,):
                    for B in (1, 2):
                        out.append((i, B, Nk, Nq, 8, D, L, P))
        for Nk_ in (Nk + 1, Nk - 1, 0):
            out.append((i, 2, Nk_, 300, 8, 32, L, 4))
        for B, H, D, P in ((0, 8, 32, 4), (-1, 8, 32, 4), (2, 0, 32, 4), (2, 8, 24, 4), (2, 8, 32, 0), (2, 8, 32, 3), (4, 2, 16, 8)):
            out.append((i, B, Nk, 300, H, D, L, P))
        for L_ in (0, -1, L - 1, L + 1):
            if L_ <= L:
                out.append((i, 2, Nk, 300, 8, 32, L_, 4))
        out.append((-1, 2, Nk, 300, 8, 32, L, 4))
    return out


def fused_cases():
    """-> list of (Nk, H, D, L, P)"""
    out = []
    for D in (16, 24, 32, 64):
        for H in (1, 8, 16):
            lim = (1 << 31) // (H * D)
            for Nk in (0, 16, 5440, 21760, lim - 2, lim - 1, lim, lim + 1):
                for L in range(0, MAXL + 1):
                    for P in (1, 2, 3, 4, 8, 16):
                        out.append((Nk, H, D, L, P))
    return out


def load(path=None):
    if path is None:
        sys.path.insert(0, ROOT)
        from rscotr_amd import _lib
        path = _lib.LIB_PATH
    dll = ctypes.CDLL(path)
    i, q = ctypes.c_int, ctypes.c_int64
    dll.rscotr_msda_bwd_workspace.argtypes = [i] * 6
    dll.rscotr_msda_bwd_workspace.restype = q
    dll.rscotr_msda_bwd_tiled_workspace.argtypes = [ctypes.c_void_p] + [i] * 7
    dll.rscotr_msda_bwd_tiled_workspace.restype = q
    dll.rscotr_msda_fused_ok.argtypes = [i] * 5
    dll.rscotr_msda_fused_ok.restype = i
    return dll


def record(dll, cs, fcs):
    """-> dict of arrays: sorted / tiled workspace bytes per case, fused_ok per fused case"""
    hosts = [np.ascontiguousarray(np.asarray(p, dtype=np.int64).reshape(-1, 2)) for p in PYRAMIDS]
    sorted_ws, tiled_ws = [], []
    for i, B, Nk, Nq, H, D, L, P in cs:
        sorted_ws.append(dll.rscotr_msda_bwd_workspace(B, Nk, Nq, H, L, P))
        tiled_ws.append(dll.rscotr_msda_bwd_tiled_workspace(None if i < 0 else hosts[i].ctypes.data, B, Nk, Nq, H, D, L, P))
    fused = [dll.rscotr_msda_fused_ok(*c) for c in fcs]
    return dict(sorted_ws=np.asarray(sorted_ws, dtype=np.int64), tiled_ws=np.asarray(tiled_ws, dtype=np.int64),
                fused_ok=np.asarray(fused, dtype=np.int8))


def main():
    cs, fcs = cases(), fused_cases()
    ans = record(load(), cs, fcs)
    pyr = np.zeros((len(PYRAMIDS), MAXL, 2), dtype=np.int32)
    for i, p in enumerate(PYRAMIDS):
        pyr[i, :len(p)] = p
    np.savez_compressed(GOLDEN, pyramids=pyr, cases=np.asarray(cs, dtype=np.int32), fused_cases=np.asarray(fcs, dtype=np.int32), **ans)
    print(GOLDEN, os.path.getsize(GOLDEN), 'bytes;', len(cs), 'workspace cases,', len(fcs), 'fused cases;',
          int((ans['tiled_ws'] > 0).sum()), 'tiled,', int((ans['sorted_ws'] > 0).sum()), 'sorted,', int(ans['fused_ok'].sum()), 'fused')


if __name__ == '__main__':
    main()
