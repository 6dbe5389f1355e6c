"""Recorded answers of the GEMM route planner's host views, for tests/test_gemm_routes_cpu.py: rscotr_gemm_f32_split_route,
rscotr_gemm_relu_bits_ok, rscotr_gemm_f32_workspace, rscotr_gemm_f32_wplanes_ok and rscotr_gemm_f32_wplanes_workspace over a shape
grid, in the four combinations of rscotr_gemm_set_precision(0 | 3) x rscotr_gemm_set_h3(0 | 1).  None of them touches a device:
the library is loaded with ctypes and asked.

    python tests/golden/make_gemm_routes_golden.py      # rewrites tests/golden/gemm_routes.npz

The committed file was written by this script on the commit BEFORE csrc/gemm.hip was split into per-family files behind one
planner: it pins that the planner answers what the four hand-written copies of the cascade answered.

The grid:
  * the step's products: every shape string of the GEMM censuses under profiles/ (r2_gemm_census.txt, history/r1_*).  Those
    censuses are of 512 x 512 only; for 224 x 224 and 800 x 800 (and again for 512 x 512) the Linears are DERIVED from the model's
    widths (Swin 96 / 192 / 384 / 768 with their 3 C and 4 C, encoder / decoder 256, 512, 1024, 2048) and token-count formulas, as
    y = x W^T (00), dx = dy W (01) and dW = dy^T x (11) — an approximation of "every shape the step issues", not a census;
  * the thresholds of choose_split6 and small_gemm_ok at +- one tile / one k-step in all four layouts, those of choose_dw_direct
    in the layouts 11 (its domain) and 01;
  * ragged M / N / K, among them M % 4 != 0 with a k-major operand; leading dimensions that are no multiple of 4;
  * per shape: workspace 0, one float short of the library's own bound, the bound, and 2 GB with no flag; has_pre (with an act) /
    has_rowscale / has_kscale one at a time at 2 GB and all together at the bound (act and has_pre reach no route decision)."""
import ctypes
import glob
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
GOLDEN = os.path.join(HERE, 'gemm_routes.npz')
MODES = ((0, 0), (0, 1), (3, 0), (3, 1))  # (precision, h3)
GENEROUS = 1 << 31


def shapes():
    """-> sorted list of (M, N, K, lda, ldb, a_kmajor, b_kmajor)"""
    mnk = set()  # (M, N, K, a, b)
    for path in [os.path.join(ROOT, 'profiles', 'r2_gemm_census.txt')] + sorted(glob.glob(os.path.join(ROOT, 'profiles', 'history', 'r1_*gemm_census*.txt'))):
        with open(path, errors='replace') as fh:
            for m in re.finditer(r'M=(\d+) N=(\d+) K=(\d+) ([01])([01p])', fh.read()):
                mnk.add((int(m[1]), int(m[2]), int(m[3]), int(m[4]), 0 if m[5] == 'p' else int(m[5])))
    # tokens: Swin stages (batch 2; 800 x 800 runs batch 4 too), the encoder's four levels, decoder queries
    tokens = set()
    for size, batches in ((224, (2,)), (512, (2,)), (800, (2, 4))):
        for b in batches:
            for s in (4, 8, 16, 32):
                tokens.add(b * (-(-size // s)) ** 2)
            tokens.add(b * sum((-(-size // s)) ** 2 for s in (8, 16, 32, 64)))
            tokens.update((b * 900, b * 100, b * 300))
    widths = [(c, k) for c in (96, 192, 384, 768) for k in (c, 3 * c, 4 * c)] + [(256, 256), (256, 1024), (256, 2048), (256, 512)]
    for t in tokens:
        for c, k in widths:
            for n_out, n_in in ((k, c), (c, k)):
                mnk.add((t, n_out, n_in, 0, 0))
                mnk.add((t, n_in, n_out, 0, 1))
                mnk.add((n_out, n_in, t, 1, 1))
    lay = ((0, 0), (0, 1), (1, 0), (1, 1))
    # choose_split6: 128-tile and 64-tile counts around 512 / 256 / 96 / 24, K around 192 / 1024 / 4096, M and N around 64 and
    # 1024 (fit128), ragged rows
    pairs = [(128 * m, 128) for m in (23, 24, 25, 511, 512, 513, 2047, 2048, 2049)]
    pairs += [(64 * m, 64) for m in (95, 96, 97, 255, 256, 257)] + [(64 * m, 256) for m in (23, 24, 25, 63, 64, 65)]
    pairs += [(384, 1024), (384, 896), (512, 768), (2048, 384), (2048, 1536), (512, 3072), (60, 256), (64, 256), (68, 256),
              (256, 60), (960, 2048), (1024, 2048), (1088, 8192), (8192, 1088), (1001, 512), (1002, 512), (1004, 512),
              (512, 1001), (512, 1002), (13294 * 4, 96), (13294 * 4, 288), (10880, 2048), (10880, 256), (4096, 4096)]
    for M, N in pairs:
        for K in (188, 192, 196, 256, 1008, 1024, 1040, 1056, 2304, 4096, 4100, 4112):
            mnk.update((M, N, K, a, b) for a, b in lay)
    # small_gemm_ok: 32 x 32 tiles around 512 and 8, K around 32 / 512 / 4096, K % 8
    for M, N in [(32 * m, 32) for m in (7, 8, 9, 511, 512, 513)] + [(1024, 32 * n) for n in (15, 16, 17)] + \
            [(64, 128), (96, 96), (2, 45), (200, 256), (1600, 256), (1601, 255), (33, 31)]:
        for K in (24, 28, 32, 40, 256, 504, 512, 516, 520, 768, 4096, 4104):
            mnk.update((M, N, K, a, b) for a, b in lay)
    # choose_dw_direct: 3 / 4 wave tiles of 96 x 96, 64 x 128, 128 x 64; K around 16384
    for M, N in ((288, 96), (96, 384), (384, 96), (96, 96), (192, 192), (384, 128), (288, 288), (100, 100), (7, 96), (8, 96),
                 (290, 98), (96, 7), (256, 256), (128, 128)):
        for K in (16376, 16384, 16392, 32768, 53176, 65536, 80000):
            mnk.update((M, N, K, a, b) for a, b in ((1, 1), (0, 1)))
    out = set()
    for i, (M, N, K, a, b) in enumerate(sorted(mnk)):
        lda, ldb = (M if a else K), (N if b else K)
        out.add((M, N, K, lda, ldb, a, b))
        if i % 7 == 0:  # padded rows: 16-byte loads legal (+ 4) or not (+ 1, + 2)
            out.update(((M, N, K, lda + 1, ldb, a, b), (M, N, K, lda, ldb + 2, a, b), (M, N, K, lda + 4, ldb + 4, a, b)))
    return sorted(out)


def load(path=None):
    if path is None:
        sys.path.insert(0, ROOT)
        from rscotr_amd import _lib
        path = _lib.LIB_PATH
    dll = ctypes.CDLL(path)
    i, q = ctypes.c_int, ctypes.c_int64
    dll.rscotr_gemm_f32_split_route.argtypes = [i] * 11 + [q]
    dll.rscotr_gemm_f32_workspace.restype = q
    dll.rscotr_gemm_f32_wplanes_workspace.restype = q
    return dll


def record(dll, shp=None, route_cases=None):
    """Ask the library.  Without `route_cases` the workspace sizes of the route questions are derived from the library's own
    rscotr_gemm_f32_workspace in mode (3, 1); the test passes the recorded ones back in."""
    shp = np.asarray(shapes() if shp is None else shp, dtype=np.int64)
    prec0, h30 = dll.rscotr_gemm_get_precision(), dll.rscotr_gemm_set_h3(1)
    res = {'shapes': shp}
    try:
        if route_cases is None:
            assert dll.rscotr_gemm_set_precision(3) == 0
            rc = []
            for s, (M, N, K, lda, ldb, a, b) in enumerate(shp.tolist()):
                ws = dll.rscotr_gemm_f32_workspace(M, N, K)
                rc += [(s, 0, 0, 0, 0, w) for w in sorted({0, max(ws - 4, 0), ws, GENEROUS})]
                rc += [(s, 1, 1, 0, 0, GENEROUS), (s, 0, 0, 1, 0, GENEROUS), (s, 0, 0, 0, 1, GENEROUS), (s, 2, 1, 1, 1, ws)]
            route_cases = np.asarray(rc, dtype=np.int64)
        res['route_cases'] = route_cases  # (shape index, act, has_pre, has_rowscale, has_kscale, workspace bytes)
        per = {k: [] for k in ('route', 'bits_ok', 'workspace', 'wplanes_ok', 'wplanes_workspace')}
        for prec, h3 in MODES:
            assert dll.rscotr_gemm_set_precision(prec) == 0
            dll.rscotr_gemm_set_h3(h3)
            S = shp.tolist()
            per['route'].append([dll.rscotr_gemm_f32_split_route(*S[s], act, pre, rs, ks, ws)
                                 for s, act, pre, rs, ks, ws in route_cases.tolist()])
            per['bits_ok'].append([dll.rscotr_gemm_relu_bits_ok(*r) for r in S])
            per['workspace'].append([dll.rscotr_gemm_f32_workspace(*r[:3]) for r in S])
            per['wplanes_ok'].append([dll.rscotr_gemm_f32_wplanes_ok(*r[:3], g) for r in S for g in (0, 1)])
            per['wplanes_workspace'].append([dll.rscotr_gemm_f32_wplanes_workspace(*r[:3]) for r in S])
        for k, v in per.items():
            res[k] = np.asarray(v, dtype=np.int64)  # [mode][case]
    finally:
        dll.rscotr_gemm_set_precision(prec0)
        dll.rscotr_gemm_set_h3(h30)
    return res


if __name__ == '__main__':
    r = record(load(sys.argv[1] if len(sys.argv) > 1 else None))
    np.savez_compressed(GOLDEN, **r)
    print(f"{GOLDEN}: {len(r['shapes'])} shapes, {len(r['route_cases'])} route questions x {len(MODES)} modes, "
          f"{os.path.getsize(GOLDEN)} bytes; routes 0/1/2 in mode (3, 1): {np.bincount(r['route'][3], minlength=3).tolist()}")
