"""Sliding-window inference tail at a 1024 x 1024 canvas: B = 2, C = 100 (the channels the head emits), crop 512, stride 341
= 3 x 3 windows with logits at an eighth of the window, ori_shape = the canvas.  ms per batch of the torch-op tail of
MTL.slide_inference_seg + inference_seg (per window a bilinear interpolation added into the (B, C, H, W) accumulator, the
division by the count, the interpolation to ori_shape, softmax and arg-max; every tensor stays on the device) next to the one
launch of ops.seg_predict_slide (csrc/seg_eval.hip).  Device events around warmed-up, alternating rounds.  Random logits: the
tail does not care.  The two routes are compared on the same logits first (labels may differ where the two largest logits are
within rounding of each other)."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F
from rscotr_amd import ops

dev = torch.device('cuda:0')
B, C, H, W = 2, 100, 1024, 1024
CROP, STRIDE = (512, 512), (341, 341)
ROUNDS, N = 5, 50


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
windows = ops.slide_windows(H, W, CROP, STRIDE)
g = torch.Generator(device=dev).manual_seed(0)
logits = torch.randn(len(windows) * B, C, CROP[0] // 8, CROP[1] // 8, device=dev, generator=g)


def torch_route(rescale=True):
    preds = logits.new_zeros((B, C, H, W))
    count = logits.new_zeros((1, 1, H, W))
    for k, (y1, y2, x1, x2) in enumerate(windows):
        preds[:, :, y1:y2, x1:x2] += F.interpolate(logits[k * B:(k + 1) * B], size=(y2 - y1, x2 - x1), mode='bilinear',
                                                   align_corners=False)
        count[:, :, y1:y2, x1:x2] += 1
    preds = preds / count
    if rescale:
        preds = F.interpolate(preds[:, :, :H, :W], size=(H, W), mode='bilinear', align_corners=False)
    return torch.softmax(preds, dim=1).argmax(dim=1)


def fused(rescale=True):
    return ops.seg_predict_slide(logits, B, (H, W), CROP, STRIDE, out_hw=(H, W) if rescale else None)


agree = float((torch_route() == fused().long()).float().mean())
fns = dict(torch_route=torch_route, fused=fused, torch_route_no_rescale=lambda: torch_route(False),
           fused_no_rescale=lambda: fused(False))
for fn in fns.values():
    for _ in range(3):
        fn()
times = {k: [] for k in fns}
for _ in range(ROUNDS):  # alternate the variants: clock and neighbours drift together
    for k, fn in fns.items():
        times[k].append(timed(fn))
med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
print(f'B={B} C={C} {H}x{W} crop {CROP} stride {STRIDE} ({len(windows)} windows): labels agree on {agree:.4%} of the pixels', flush=True)
for k in fns:
    print(f'  {k:24s} median {med[k]:8.3f} ms   min {min(times[k]):8.3f}   max {max(times[k]):8.3f}   ({ROUNDS} rounds x {N})', flush=True)
print(f'  torch_route / fused = {med["torch_route"] / med["fused"]:.2f}x', flush=True)
print(f'  torch_route_no_rescale / fused_no_rescale = {med["torch_route_no_rescale"] / med["fused_no_rescale"]:.2f}x', flush=True)
