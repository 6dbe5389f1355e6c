"""Graph-replayed A/B of the k-major weight-gradient products on the 128 x 128 fp16 split body:
scripts/bench_dw_kmajor.py <parent lib> <new lib> [name A] [name B]

Cases: the FFN weight gradients 256 x 2048 x 10880 and 2048 x 256 x 10880 through the product entry (rscotr_gemm_f32_dw_slabs_r,
both operands k-major, no kscale — as the step's FFN layers call it —, 16 k-slices left as slabs: gemm_h3_128_kernel<true, true, false>), and ONE grouped launch (rscotr_gemm_dw_group
variant 7: gemm_h3_group_kernel) over the weight gradients of the Swin-T backbone at 512^2, B = 2 (stage 1-4 qkv / proj / fc1 / fc2
with their bias gradients), its table built by ops.DEFER as the step builds it.  Per case one hipGraph of 10 calls per library, each
call on the next of 10 operand sets (more than 256 MB in all, so no set is still in the last-level cache when its turn comes),
timed as windows of 20 replays between device events with the empty event bracket taken off, five rounds alternating the two
libraries.  Prints median (min - max) microseconds per call, and whether slabs and row-sum partials of the two libraries are
equal bit for bit (torch.equal).  The value-range words and the tables come from the package's own library (RSCOTR_LIB or the
tree's); the two libraries under test only run the products."""
import ctypes
import json
import os
import statistics
import sys

import torch

SETS, REPLAYS, ROUNDS = 10, 20, 5
P, I, L, D = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_double


def load(path):
    dll = ctypes.CDLL(path)
    dll.rscotr_gemm_f32_dw_slabs_r.argtypes = [P, P, P, I, I, I, I, I, I, P, P, I, P, L, P, P, P, P]
    dll.rscotr_gemm_dw_group.argtypes = [P, I, I, I, D, P, P]
    dll.rscotr_gemm_f32_workspace.argtypes = [I, I, I]
    dll.rscotr_gemm_f32_workspace.restype = L
    dll.rscotr_gemm_set_precision.argtypes = [I]
    dll.rscotr_last_error.restype = ctypes.c_char_p
    assert dll.rscotr_gemm_set_precision(3) == 0
    return dll


def window(graph):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPLAYS):
        graph.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3


def empty_bracket():
    ts = []
    for _ in range(21):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    return statistics.median(ts)


def ab(case, libs, names, call, results):
    """call(dll, set index, stream) -> status; results() -> tensors a run leaves (compared between the libraries)."""
    side = torch.cuda.Stream()
    graphs, outs = [], []
    for dll in libs:
        with torch.cuda.stream(side):
            for i in range(SETS):
                rc = call(dll, i, side.cuda_stream)
                assert rc == 0, dll.rscotr_last_error()
            torch.cuda.synchronize()
            outs.append([t.clone() for t in results()])
            for t in results():
                t.zero_()
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr, stream=side):
                for i in range(SETS):
                    assert call(dll, i, torch.cuda.current_stream().cuda_stream) == 0
        graphs.append(gr)
    equal = all(torch.equal(a, b) for a, b in zip(*outs))
    for gr in graphs:
        window(gr)
    e = empty_bracket()
    t = [[], []]
    for _ in range(ROUNDS):
        for k, gr in enumerate(graphs):
            t[k].append((window(gr) - e) / (REPLAYS * SETS))
    row = dict(case=case, bit_equal=equal, empty_us=round(e, 1))
    for k in range(2):
        row[names[k]] = dict(median=round(statistics.median(t[k]), 2), min=round(min(t[k]), 2), max=round(max(t[k]), 2))
    print(json.dumps(row), flush=True)
    return equal


def swin_t_problems(B=2, side=512):
    """(M, N, K, bias gradient?) of every Linear weight gradient dW = dy^T x of the Swin-T backbone: M = out features, N = in."""
    out = []
    for stage, (C, depth) in enumerate([(96, 2), (192, 2), (384, 6), (768, 2)]):
        T = B * (side // 4 >> stage) ** 2
        for _ in range(depth):
            out += [(3 * C, C, T, True), (C, C, T, True), (4 * C, C, T, True), (C, 4 * C, T, True)]
    return out


def main():
    paths = sys.argv[1:3]
    names = sys.argv[3:5] if len(sys.argv) >= 5 else ['parent', 'new']
    libs = [load(p) for p in paths]
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
    from rscotr_amd import ops
    from rscotr_amd.ops.deferred import DEFER, GroupProblem
    R = ops.RANGES
    dev = torch.device('cuda:0')
    R.enabled, ok = True, True
    g = torch.Generator(device=dev).manual_seed(1)

    # ---- the FFN weight gradients through the product entry
    for M, N, K in ((256, 2048, 10880), (2048, 256, 10880)):
        R.begin(dev)
        A = [torch.randn(K, M, device=dev, generator=g) * 1e-3 for _ in range(SETS)]
        Bm = [torch.randn(K, N, device=dev, generator=g) for _ in range(SETS)]
        sa = [R.of(a, K, M, M) for a in A]
        sb = [R.of(b, K, N, N) for b in Bm]
        nws = libs[0].rscotr_gemm_f32_workspace(M, N, K)
        assert nws == libs[1].rscotr_gemm_f32_workspace(M, N, K) and nws > 0
        ws = [torch.zeros(nws // 4, device=dev) for _ in range(SETS)]
        C, rs = torch.zeros(M, N, device=dev), torch.zeros(M, device=dev)
        splits = ctypes.c_int32(0)

        def call(dll, i, s):
            return dll.rscotr_gemm_f32_dw_slabs_r(A[i].data_ptr(), Bm[i].data_ptr(), C.data_ptr(), M, N, K, M, N, N, rs.data_ptr(),
                                                  None, 1, ws[i].data_ptr(), nws, ctypes.addressof(splits), sa[i], sb[i], s)

        ok &= ab(f'product {M}x{N}x{K} ({SETS * (M + N) * K * 4 >> 20} MB of operands)', libs, names, call, lambda: ws)
        assert splits.value > 1, 'the product was not left as slabs'
        del A, Bm, ws

    # ---- one grouped launch over the Swin-T problem list
    R.begin(dev)
    probs = swin_t_problems()
    tables, keep, nbytes = [], [], 0
    DEFER.cur = DEFER.off = 0
    for i in range(SETS):
        group = []
        for M, N, K, bias in probs:
            A = torch.randn(K, M, device=dev, generator=g) * 1e-3
            Bm = torch.randn(K, N, device=dev, generator=g)
            out, rs = torch.zeros(M, N, device=dev), torch.zeros(M, device=dev)
            keep += [A, Bm, out, rs]
            nbytes += (A.numel() + Bm.numel()) * 4
            group.append(GroupProblem(A.data_ptr(), Bm.data_ptr(), out.data_ptr(), rs.data_ptr() if bias else 0, 0, M, N, K, M, N, 1,
                                      R.of(A, K, M, M), R.of(Bm, K, N, N)))
        DEFER.group, DEFER.group_keep = group, keep
        launches, _ = DEFER._plan_group()
        launches = [x for x in launches if x[3] == 7]
        assert len(launches) == 1 and launches[0][1] >= len(probs), 'every problem is a member of the variant-7 launch'
        tables.append(launches[0])
    DEFER.group, DEFER.group_keep = [], []

    def call(dll, i, s):
        table, n, total, variant, flops = tables[i]
        return dll.rscotr_gemm_dw_group(table.data_ptr(), n, total, variant, flops, R.base, s)

    ok &= ab(f'grouped launch, Swin-T 512^2 B=2, {len(probs)} problems ({nbytes >> 20} MB of operands)', libs, names, call,
             lambda: DEFER.blocks)
    DEFER.cur = DEFER.off = 0
    print('bit-identical: ' + ('yes' if ok else 'NO'), flush=True)
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
