"""The fused focal and Tversky seg losses (ops.upsample_focal, ops.upsample_tversky) forward + backward at the step's shape —
logits 2 x 100 x 64 x 64, labels 512 x 512, 10 % of the pixels ignored, 60 % of the labels the arg-max — next to the Dice and
cross-entropy ops measured in the same run: us per forward + backward pair and per forward alone from device events around
warmed-up, alternating rounds (the method of scripts/bench_seg_dice.py).
`python scripts/bench_seg_focal_tversky.py [pairs per window]`."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F
from rscotr_amd import ops

dev = torch.device('cuda:0')
B, C, h, w, H, W = 2, 100, 64, 64, 512, 512
ROUNDS = 5
N = int(sys.argv[1]) if len(sys.argv) > 1 else 300


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


g = torch.Generator().manual_seed(0)
logit = (torch.randn(B, C, h, w, generator=g) * 3).to(dev).requires_grad_(True)
label = torch.randint(0, C, (B, H, W), generator=g)
label = torch.where(torch.rand(B, H, W, generator=g) < 0.6,
                    F.interpolate(logit.detach().cpu(), size=(H, W), mode='bilinear').argmax(1), label)
label[torch.rand(B, H, W, generator=g) < 0.1] = 255
label = label.to(dev)
losses = {'upsample_focal': lambda: ops.upsample_focal(logit, label, 255, loss_weight=2.0),
          'upsample_tversky': lambda: ops.upsample_tversky(logit, label, 255, loss_weight=3.0),
          'upsample_dice': lambda: ops.upsample_dice(logit, label, 255, loss_weight=3.0),
          'upsample_ce': lambda: ops.upsample_ce(logit, label, 255)[0]}


def fwd(f):
    def run():
        with torch.no_grad():
            return f()
    return run


fns = {}
for k, f in losses.items():
    fns[k] = lambda f=f: torch.autograd.grad(f(), logit)[0]
    fns[k + ' fwd'] = fwd(f)
print(f'device: {torch.cuda.get_device_name(0)}; B={B} C={C} {h}x{w} -> {H}x{W}; losses ' +
      ', '.join(f'{k} {float(f().detach()):.6f}' for k, f in losses.items()), flush=True)
for fn in fns.values():
    for _ in range(5):
        fn()
times = {k: [] for k in fns}
for _ in range(ROUNDS):  # alternate the variants: clock and neighbours drift together
    for k, fn in fns.items():
        times[k].append(timed(fn, N))
for k in fns:
    v = times[k]
    print(f'  {k:22s} median {sorted(v)[len(v) // 2] * 1e3:9.1f} us   min {min(v) * 1e3:9.1f}   max {max(v) * 1e3:9.1f}', flush=True)
