"""ops.seg_class_logits (csrc/seg_mix.hip) at the model's shape — cls (2,100,6), e (2,100,256), mask tokens (2,128^2,256) —
forward alone and backward alone (all three gradients), next to the bytes each must move, and the scheme-2 product it replaces
at the same shape (ops.mask_logits: Q = 100 mask logits, forward / backward).
us per call from device events around windows of warmed-up calls.  Every variant is captured once as a hipGraph of ROT calls,
each on the NEXT of ROT mask-feature tensors (ROT x 33.5 MB > the 256 MB last-level cache, so the pass over the mask features
comes from HBM as it does in the step), and a window replays that graph N / ROT times: the host's ~30 us per eager call would
otherwise be what is timed.  The time of an empty bracket is taken off every window.  Windows alternate between the variants.
`python scripts/bench_seg_mix.py [calls per window]`."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from rscotr_amd import ops

dev = torch.device('cuda:0')
B, Q, K, D, P = 2, 100, 6, 256, 128 * 128
ROT, ROUNDS, N = 10, 5, int(sys.argv[1]) if len(sys.argv) > 1 else 200


def timed(fn, n=N):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for i in range(n):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


print(f'device: {torch.cuda.get_device_name(0)}', flush=True)
g = torch.Generator().manual_seed(0)
cls = torch.randn(B, Q, K, generator=g).to(dev).requires_grad_(True)
e = torch.randn(B, Q, D, generator=g).to(dev).requires_grad_(True)
mfs = [torch.randn(B, P, D, generator=g).to(dev).requires_grad_(True) for _ in range(ROT)]
g_seg = torch.randn(B, K, P, generator=g).to(dev)
g_mask = torch.randn(B, Q, P, generator=g).to(dev)
side = torch.cuda.Stream()
side.wait_stream(torch.cuda.current_stream())
with torch.cuda.stream(side):  # (autograd runs a backward on the stream of its forward: the one the graphs are captured on)
    segs = [ops.seg_class_logits(cls, e, m) for m in mfs]     # autograd graphs kept: backward alone is timed on them
    masks = [ops.mask_logits(e, m) for m in mfs]
MB = 1e-6
bytes_ = {
    'seg_mix forward': 4 * B * P * (D + K),                        # mf read, seg written
    'seg_mix backward': 4 * B * P * (2 * D + K),                   # mf read, dmf written, g read
    'mask_logits forward': 4 * B * P * (D + Q),                    # mf read, mask_pred written
    'mask_logits backward': 4 * B * P * (2 * D + 2 * Q),           # g read twice (two products), mf read, dmf written
}
fns = {
    'seg_mix forward': lambda i: ops.seg_class_logits(cls.detach(), e.detach(), mfs[i % ROT].detach()),
    'seg_mix backward': lambda i: torch.autograd.grad(segs[i % ROT], (cls, e, mfs[i % ROT]), g_seg, retain_graph=True),
    'mask_logits forward': lambda i: ops.mask_logits(e.detach(), mfs[i % ROT].detach()),
    'mask_logits backward': lambda i: torch.autograd.grad(masks[i % ROT], (e, mfs[i % ROT]), g_mask, retain_graph=True),
}
graphs = {}
with torch.cuda.stream(side):
    for k, fn in fns.items():
        for i in range(2 * ROT):
            fn(i)
        side.synchronize()
        graphs[k] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[k], stream=side):
            keep = [fn(i) for i in range(ROT)]
torch.cuda.current_stream().wait_stream(side)
for gr in graphs.values():
    gr.replay()
empty = sorted(timed(lambda i: None, 1) for _ in range(20))[10]  # the bracket itself
times = {k: [] for k in fns}
for _ in range(ROUNDS):
    for k in fns:
        times[k].append((timed(lambda i: graphs[k].replay(), N // ROT) * (N // ROT) - empty) / (N // ROT * ROT))
print(f'B={B} Q={Q} K={K} D={D} P={P}; {ROUNDS} rounds x {N} calls (graphs of {ROT}), {ROT} rotating mask-feature tensors; empty bracket {empty * 1e3:.1f} us', flush=True)
for k in fns:
    med = sorted(times[k])[len(times[k]) // 2]
    print(f'  {k:22s} median {med * 1e3:8.1f} us   min {min(times[k]) * 1e3:8.1f}   max {max(times[k]) * 1e3:8.1f}   '
          f'{bytes_[k] * MB:6.1f} MB -> {bytes_[k] / (med * 1e-3) * 1e-12:5.2f} TB/s', flush=True)
