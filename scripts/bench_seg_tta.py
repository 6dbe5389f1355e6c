"""Multi-scale / flip testing tail at the Potsdam shape: B = 2, C = 100 (the channels the head emits), 512 x 512 originals,
img_ratios 0.5 ... 1.75 x {no flip, horizontal} = 12 views, logits at a quarter of each view's size.  ms per batch of the
torch-op tail of MTL.aug_test_seg (per view two bilinear interpolations, softmax and the un-flip, the sum over the views, the
division and the arg-max; every tensor stays on the device) next to the one launch of ops.seg_predict_tta (csrc/seg_eval.hip).
Device events around warmed-up, alternating rounds.  Random logits: the tail does not care.  The two routes are compared on the
same logits first (labels may differ where the two largest mean probabilities are within rounding of each other)."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F
from rscotr_amd import ops

dev = torch.device('cuda:0')
B, C, HO, WO = 2, 100, 512, 512
RATIOS = (0.5, 0.75, 1.0, 1.25, 1.5, 1.75)
ROUNDS, N = 5, 100  # (a window is 100 calls, about 0.75 s)


def timed(fn, n=N):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


print(f'device: {torch.cuda.get_device_name(0)}', flush=True)
g = torch.Generator(device=dev).manual_seed(0)
logits, canvases, flips = [], [], []
for r in RATIOS:
    s = int(512 * r)
    for flip in (None, 'horizontal'):
        logits.append(torch.randn(B, C, s // 4, s // 4, device=dev, generator=g))
        canvases.append((s, s))
        flips.append(flip)
V = len(logits)
crops = [None] * V


def torch_route():
    acc = None
    for logit, (H, W), flip in zip(logits, canvases, flips):
        x = F.interpolate(logit, size=(H, W), mode='bilinear', align_corners=False)
        x = F.interpolate(x[:, :, :H, :W], size=(HO, WO), mode='bilinear', align_corners=False)
        x = torch.softmax(x, dim=1)
        if flip == 'horizontal':
            x = x.flip(dims=(3,))
        if acc is None:
            acc = x
        else:
            acc += x
    acc /= V
    return acc.argmax(dim=1)


def fused():
    return ops.seg_predict_tta(logits, canvases, crops, (HO, WO), flips)


agree = float((torch_route() == fused().long()).float().mean())
fns = dict(torch_route=torch_route, fused=fused)
for fn in fns.values():
    for _ in range(3):
        fn()
times = {k: [] for k in fns}
for _ in range(ROUNDS):  # alternate the variants: clock and neighbours drift together
    for k, fn in fns.items():
        times[k].append(timed(fn))
med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
print(f'B={B} C={C} {HO}x{WO} V={V}: labels agree on {agree:.4%} of the pixels', flush=True)
for k in fns:
    print(f'  {k:12s} median {med[k]:8.3f} ms   min {min(times[k]):8.3f}   max {max(times[k]):8.3f}   ({ROUNDS} rounds x {N})', flush=True)
print(f'  torch_route / fused = {med["torch_route"] / med["fused"]:.2f}x', flush=True)
