"""Segmentation inference tail at the evaluation shape, (1, C, 64, 64) logits -> a 512 x 512 map: us per image of the torch
chain of MTL.simple_test_seg (two bilinear interpolations, the padding slice, softmax, argmax and the .cpu() that hands the
int64 map to the host) next to ops.seg_predict + ops.seg_areas (csrc/seg_eval.hip), whose result stays on the device.
Device events around warmed-up, alternating rounds; the chain's time includes its host transfer because that transfer is
part of what the pre_eval mode removes.  The two paths are compared on the same random logits first."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F
from rscotr_amd import ops

dev = torch.device('cuda:0')
H = W = 512
ROUNDS, N = 5, 50


def timed(fn, n=N):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


print(f'device: {torch.cuda.get_device_name(0)}', flush=True)
for C, what in ((5, "the config's num_classes"), (100, "the head's query channels")):
    logit = torch.randn(1, C, 64, 64, device=dev)
    gt = torch.randint(0, 7, (1, H, W), device=dev, dtype=torch.uint8)

    def chain():
        x = F.interpolate(logit, size=(H, W), mode='bilinear', align_corners=False)
        x = F.interpolate(x[:, :, :H, :W], size=(H, W), mode='bilinear', align_corners=False)
        return torch.softmax(x, dim=1).argmax(dim=1).cpu()

    def chain_device():  # the same without the transfer: what the five passes alone cost
        x = F.interpolate(logit, size=(H, W), mode='bilinear', align_corners=False)
        x = F.interpolate(x[:, :, :H, :W], size=(H, W), mode='bilinear', align_corners=False)
        return torch.softmax(x, dim=1).argmax(dim=1)

    def fused():
        return ops.seg_areas(ops.seg_predict(logit, (H, W), crop_hw=(H, W), out_hw=(H, W)), gt, 6, 255, True)

    def predict_only():
        return ops.seg_predict(logit, (H, W), crop_hw=(H, W), out_hw=(H, W))

    pred_map = predict_only()

    def areas_only():
        return ops.seg_areas(pred_map, gt, 6, 255, True)

    agree = float((chain().to(dev) == predict_only()[0].long()).float().mean())
    fns = dict(chain=chain, chain_device=chain_device, fused=fused, predict_only=predict_only, areas_only=areas_only)
    for fn in fns.values():
        for _ in range(10):
            fn()
    times = {k: [] for k in fns}
    for _ in range(ROUNDS):  # alternate the variants: clock and neighbours drift together
        for k, fn in fns.items():
            times[k].append(timed(fn))
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    print(f'C={C:3d} ({what}): labels agree on {agree:.4%} of the pixels', flush=True)
    for k in fns:
        print(f'  {k:13s} median {med[k]:8.1f} us   min {min(times[k]):8.1f}   max {max(times[k]):8.1f}   ({ROUNDS} rounds x {N})',
              flush=True)
    print(f'  chain / fused = {med["chain"] / med["fused"]:.2f}x   chain_device / fused = {med["chain_device"] / med["fused"]:.2f}x',
          flush=True)
