"""The fused seg loss at the Potsdam shape — logits 2 x 100 x 64 x 64, labels 512 x 512, 10 % of the pixels ignored —
forward + backward in three configurations:
    unweighted        ops.upsample_ce (rscotr_upsample_ce_fwd / _bwd: what the default config runs)
    weighted          ops.upsample_ce_weighted with class_weight + avg_non_ignore (rscotr_upsample_ce_w_fwd / _w_bwd)
    weighted + ohem   the same with OHEMPixelSampler(thresh=0.7, min_kept=100000) (+ rscotr_upsample_ce_ohem)
us per forward + backward pair from device events around warmed-up, alternating rounds (the few element-wise torch
launches of the normaliser and grad_scale are inside the window, the same in every configuration), and the launches the
library issues per pair, counted from csrc/seg_loss.hip.  `python scripts/bench_seg_loss_weighted.py [pairs per window]`: a
small window suits a kernel-trace run, which gives the per-kernel times.  Random logits; 60 % of the labels are the arg-max class, so the
probabilities straddle the sampler's threshold."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from rscotr_amd import ops

dev = torch.device('cuda:0')
B, C, h, w, H, W = 2, 100, 64, 64, 512, 512
ROUNDS, N = 5, int(sys.argv[1]) if len(sys.argv) > 1 else 1000  # (a window of 1000 pairs is a few tenths of a second)
# launches per pair: forward kernel + fold, backward kernel; the select adds one memset, 4 x (histogram + pick), the mask
# pass and its fold
LAUNCHES = {'unweighted': 3, 'weighted': 3, 'weighted + ohem': 3 + 11}


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
g = torch.Generator().manual_seed(0)
logit = (torch.randn(B, C, h, w, generator=g) * 3).to(dev).requires_grad_(True)
label = torch.randint(0, C, (B, H, W), generator=g)
# make the labelled class likely, as in a trained model: the probabilities then straddle the threshold
label = torch.where(torch.rand(B, H, W, generator=g) < 0.6,
                    torch.nn.functional.interpolate(logit.detach().cpu(), size=(H, W), mode='bilinear').argmax(1), label)
label[torch.rand(B, H, W, generator=g) < 0.1] = 255
label = label.to(dev)
cw = (0.25 + 4 * torch.rand(C, generator=g)).to(dev)


def unweighted():
    loss, _ = ops.upsample_ce(logit, label, 255)
    return torch.autograd.grad(loss, logit)[0]


def weighted():
    loss, _, _ = ops.upsample_ce_weighted(logit, label, 255, class_weight=cw, avg_non_ignore=True)
    return torch.autograd.grad(loss, logit)[0]


def weighted_ohem():
    loss, _, _ = ops.upsample_ce_weighted(logit, label, 255, class_weight=cw, avg_non_ignore=True, ohem=(0.7, 100000))
    return torch.autograd.grad(loss, logit)[0]


fns = {'unweighted': unweighted, 'weighted': weighted, 'weighted + ohem': weighted_ohem}
pw = ops.upsample_ce_weighted(logit, label, 255, class_weight=cw, avg_non_ignore=True, ohem=(0.7, 100000))[2]
print(f'OHEM keeps {int((pw != 0).sum())} of {int((label != 255).sum())} non-ignored pixels', flush=True)
ones = ops.upsample_ce_weighted(logit, label, 255, class_weight=torch.ones(C, device=dev))[0]
print(f'all-ones weights bit-equal to the unweighted loss: {bool(ones == ops.upsample_ce(logit, label, 255)[0])}', flush=True)
for fn in fns.values():
    for _ in range(10):
        fn()
times = {k: [] for k in fns}
for _ in range(ROUNDS):  # alternate the variants: clock and neighbours drift together
    for k, fn in fns.items():
        times[k].append(timed(fn))
med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
print(f'B={B} C={C} {h}x{w} -> {H}x{W}, forward + backward:', flush=True)
for k in fns:
    print(f'  {k:16s} median {med[k] * 1e3:8.1f} us   min {min(times[k]) * 1e3:8.1f}   max {max(times[k]) * 1e3:8.1f}   '
          f'{LAUNCHES[k]:2d} library launches   ({ROUNDS} rounds x {N})', flush=True)
print(f'  weighted / unweighted = {med["weighted"] / med["unweighted"]:.3f}x   '
      f'weighted + ohem / unweighted = {med["weighted + ohem"] / med["unweighted"]:.3f}x', flush=True)
