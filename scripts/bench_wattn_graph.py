"""Graph-replayed A/B of the Swin window-attention kernels: scripts/bench_wattn_graph.py <lib A> <lib B> [name A] [name B]

Per stage of Swin-T at 512^2, B = 2, shift 0 and 3, forward and backward: one hipGraph of 10 calls per library, each call on
the next of 10 input sets (stage 1 is 10 x 38 MB of qkv, more than the last-level cache), timed as windows of 20 replays
between device events with the empty event bracket taken off, five rounds alternating the two libraries.  Eager launches
(scripts/bench_wattn.py) time the host at these kernel lengths.  Prints median (min - max) microseconds per call."""
import ctypes
import json
import statistics
import sys

import torch

SETS, REPLAYS, ROUNDS = 10, 20, 5
P, I, L = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64


def load(path):
    dll = ctypes.CDLL(path)
    dll.rscotr_swin_wattn_fwd.argtypes = [P, P, P, P, I, I, I, I, I, I, I, P, P]
    dll.rscotr_swin_wattn_bwd.argtypes = [P, P, P, P, P, P, P, I, I, I, I, I, I, I, P, P, L, P, P]
    dll.rscotr_swin_wattn_bwd_workspace.argtypes = [I, I, I, I, I]
    dll.rscotr_swin_wattn_bwd_workspace.restype = L
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


def main():
    paths = sys.argv[1:3]
    names = sys.argv[3:5] if len(sys.argv) >= 5 else ['A', 'B']
    libs = [load(p) for p in paths]
    dev = torch.device('cuda:0')
    B = 2
    side = torch.cuda.Stream()
    for stage, (H, heads) in enumerate([(128, 3), (64, 6), (32, 12), (16, 24)], 1):
        C = heads * 32
        g = torch.Generator(device=dev).manual_seed(stage)
        qkv = [torch.randn(B, H * H, 3 * C, device=dev, generator=g) for _ in range(SETS)]
        go = [torch.randn(B, H * H, C, device=dev, generator=g) for _ in range(SETS)]
        out = [torch.empty(B, H * H, C, device=dev) for _ in range(SETS)]
        dqkv = [torch.empty(B, H * H, 3 * C, device=dev) for _ in range(SETS)]
        qb = torch.randn(3 * C, device=dev, generator=g)
        tb = torch.randn(169, heads, device=dev, generator=g)
        dqb, dtb = torch.zeros_like(qb), torch.zeros_like(tb)
        nws = libs[0].rscotr_swin_wattn_bwd_workspace(B, H, H, C, heads)
        assert nws == libs[1].rscotr_swin_wattn_bwd_workspace(B, H, H, C, heads)
        ws = torch.empty(nws, dtype=torch.uint8, device=dev)
        for shift in (0, 3):
            def fwd(dll, i, s):
                return dll.rscotr_swin_wattn_fwd(qkv[i].data_ptr(), qb.data_ptr(), tb.data_ptr(), out[i].data_ptr(), B, H, H, C,
                                                 heads, 7, shift, None, s)

            def bwd(dll, i, s):
                return dll.rscotr_swin_wattn_bwd(qkv[i].data_ptr(), qb.data_ptr(), tb.data_ptr(), go[i].data_ptr(),
                                                 dqkv[i].data_ptr(), dqb.data_ptr(), dtb.data_ptr(), B, H, H, C, heads, 7, shift,
                                                 out[i].data_ptr(), ws.data_ptr(), nws, None, s)

            for dname, fn in (('fwd', fwd), ('bwd', bwd)):
                graphs = []
                for dll in libs:
                    with torch.cuda.stream(side):
                        for i in range(SETS):  # (also fills out[] for the backward)
                            assert fn(dll, i, side.cuda_stream) == 0
                        torch.cuda.synchronize()
                        gr = torch.cuda.CUDAGraph()
                        with torch.cuda.graph(gr, stream=side):
                            for i in range(SETS):
                                assert fn(dll, i, torch.cuda.current_stream().cuda_stream) == 0
                    graphs.append(gr)
                for gr in graphs:
                    window(gr)
                e = empty_bracket()
                t = [[], []]
                for _ in range(ROUNDS):
                    for k, gr in enumerate(graphs):
                        t[k].append((window(gr) - e) / (REPLAYS * SETS))
                row = dict(stage=stage, shift=shift, dir=dname, empty_us=round(e, 1))
                for k in range(2):
                    row[names[k]] = dict(median=round(statistics.median(t[k]), 2), min=round(min(t[k]), 2),
                                         max=round(max(t[k]), 2))
                print(json.dumps(row), flush=True)


if __name__ == '__main__':
    main()
