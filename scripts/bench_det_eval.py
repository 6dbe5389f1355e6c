"""Detection evaluation at DIOR's shape (Q = 600 queries, C = 20 classes, max_per_img K = 300; 64 images in batches of 8, 30
ground truths each): the host route — DINOHead._get_bboxes_single's torch chain per image, mtl.bbox2result (two .cpu() per
image) and metrics.coco_bbox_map over the 64 images — next to the device route — ops.det_decode + CocoDetDataset.pre_eval
(ops.det_match) per batch, one device-to-host copy, metrics.coco_accumulate.  Both routes are first compared (the same dict,
value for value), then timed in alternating rounds after a warm-up: host clock around work that ends in a synchronise for the
routes and their host halves, device events for the launches alone (decode-only, match-only) and for the torch chain they
replace.  The inputs are synthetic: logits from a normal distribution, ground truths = jittered boxes of random queries."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from types import SimpleNamespace

import numpy as np
import torch

from rscotr_amd import ops
from rscotr_amd.det_head import DINOHead
from rscotr_amd.metrics import coco_accumulate, coco_area_ranges, coco_bbox_map, coco_iou_thrs
from rscotr_amd.mtl import bbox2result
from rscotr_amd.pipeline import CocoDetDataset

dev = torch.device('cuda:0')
IMAGES, BATCH, Q, C, K, GTS = 64, 8, 600, 20, 300, 30
ROUNDS = 5
names = tuple(f'c{i}' for i in range(C))
g = torch.Generator().manual_seed(0)
cls = (torch.randn((IMAGES, Q, C), generator=g) * 2.0 - 3.0).to(dev)
box = torch.cat([torch.rand((IMAGES, Q, 2), generator=g), torch.rand((IMAGES, Q, 2), generator=g) * 0.3 + 0.02], -1).to(dev)
metas = [dict(img_shape=(800, 800, 3), scale_factor=np.array([1.0, 1.0, 1.0, 1.0], np.float32)) for _ in range(IMAGES)]
meta = torch.tensor([[800., 800., 1, 1, 1, 1]] * IMAGES).to(dev)
stub = SimpleNamespace(test_cfg=dict(max_per_img=K), num_query=Q, num_classes=C)
batches = [slice(i, i + BATCH) for i in range(0, IMAGES, BATCH)]


def chain_device():  # the torch chain alone, results left on the device
    return [DINOHead._get_bboxes_single(stub, cls[i], box[i], metas[i]['img_shape'], metas[i]['scale_factor'], True)
            for i in range(IMAGES)]


def host_decode():
    return [bbox2result(d, l, C) for d, l in chain_device()]


def dev_decode():
    return [ops.det_decode(cls[s], box[s], meta[s], K, True) for s in batches]


# ground truths: per image GTS random queries' boxes (as decoded), jittered, with the query's best class
rs = np.random.RandomState(1)
ds = CocoDetDataset.__new__(CocoDetDataset)
ds.CLASSES, ds.items = names, []
for i, (d, l) in enumerate(chain_device()):
    q = rs.randint(0, Q, GTS)
    b = ops.bbox_cxcywh_to_xyxy(box[i].cpu())[q].numpy() * 800.0
    b = np.clip(b + rs.uniform(-6, 6, b.shape), 0, 800).astype(np.float32)
    b[:, 2:] = np.maximum(b[:, 2:], b[:, :2] + 2)
    ds.items.append((f'{i}.png', b, cls[i].cpu().numpy()[q].argmax(1).astype(np.int64)))
gt_boxes, gt_labels = [it[1] for it in ds.items], [it[2] for it in ds.items]


def host_map(results):
    return coco_bbox_map(results, gt_boxes, gt_labels, names, max_det=100)


def host_route():
    return host_map(host_decode())


def dev_loop():
    out = []
    for s, (d, l) in zip(batches, dev_decode()):
        out.extend(ds.pre_eval(d, l, range(s.start, s.stop)))
    kinds = [torch.stack([r[i] for r in out]).contiguous() for i in (1, 0, 2, 3)]
    host = torch.cat([k.view(torch.uint8).reshape(-1) for k in kinds]).cpu()
    parts, at = [], 0
    for k in kinds:
        n = k.numel() * k.element_size()
        parts.append(host[at:at + n].view(k.dtype).reshape(k.shape))
        at += n
    return list(zip(parts[1].unbind(0), parts[0].unbind(0), parts[2].unbind(0), parts[3].unbind(0)))


def dev_route():
    return coco_accumulate(dev_loop(), names)


# match-only: inputs already on the device
dets_all = dev_decode()
off = [np.concatenate([[0], np.cumsum([len(gt_labels[i]) for i in range(s.start, s.stop)])]).astype(np.int64) for s in batches]
up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
match_in = [(d, l, torch.full((BATCH,), K, dtype=torch.int32, device=dev), up(np.concatenate(gt_boxes[s])),
             up(np.concatenate(gt_labels[s])), up(o)) for s, (d, l), o in zip(batches, dets_all, off)]
ranges, thrs = up(coco_area_ranges()), up(coco_iou_thrs(None))


def dev_match():
    return [ops.det_match(*m, ranges, thrs, C, 100) for m in match_in]


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def events(fn, n=20):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


print(f'device: {torch.cuda.get_device_name(0)}', flush=True)
a, b = host_route(), dev_route()
print('host route  :', a['bbox_mAP_copypaste'], flush=True)
print('device route:', b['bbox_mAP_copypaste'], '(equal)' if a == b else '(DIFFERENT)', flush=True)
host_results = host_decode()
pre = dev_loop()
fns = dict(host_route=(wall, host_route), host_decode=(wall, host_decode), host_map=(wall, lambda: host_map(host_results)),
           dev_route=(wall, dev_route), dev_accumulate=(wall, lambda: coco_accumulate(pre, names)),
           chain_device=(events, chain_device), decode_only=(events, dev_decode), match_only=(events, dev_match))
for how, fn in fns.values():  # warm-up
    fn()
times = {k: [] for k in fns}
for _ in range(ROUNDS):  # alternate the variants: clock and neighbours drift together
    for k, (how, fn) in fns.items():
        times[k].append(how(fn))
med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
print(f'{IMAGES} images, batches of {BATCH}, Q={Q} C={C} K={K}, {GTS} ground truths per image; ms per {IMAGES} images', flush=True)
for k in fns:
    print(f'  {k:15s} median {med[k]:10.3f} ms   min {min(times[k]):10.3f}   max {max(times[k]):10.3f}   ({ROUNDS} rounds)', flush=True)
print(f'  host_route / dev_route = {med["host_route"] / med["dev_route"]:.1f}x   host_decode / decode_only = '
      f'{med["host_decode"] / med["decode_only"]:.1f}x   chain_device / decode_only = {med["chain_device"] / med["decode_only"]:.1f}x   '
      f'host_map / (match_only + dev_accumulate) = {med["host_map"] / (med["match_only"] + med["dev_accumulate"]):.1f}x', flush=True)
