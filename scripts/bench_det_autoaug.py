"""Kernel time of the det AutoAugment chain launch (rscotr_img_aug_chain_u8) on device-resident bytes: B = 2 sources of 800 x 800
through policy 1 of the reference's DINO recipe (Resize -> RandomCrop(absolute_range (384, 600)) -> Resize(override), the pipeline
recorded in tests/golden/reference_det_pipeline.json, policy 0 taken out so that every sample has two stages), against the
one-stage rscotr_img_aug_u8 launch that resizes the same sources straight to the same canvas (every pixel of it live).  The two are
timed alternately, three rounds; bytes = 3 B read + 12 B written per output pixel."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from rscotr_amd import pipeline as P
from rscotr_amd._lib import lib

dev = torch.device('cuda:0')


def tuples(o):
    if isinstance(o, dict):
        return {k: tuples(v) for k, v in o.items()}
    if isinstance(o, list):
        return tuple(o) if o and all(isinstance(v, (int, float)) for v in o) else [tuples(v) for v in o]
    return o


def timed(f, n=2000):
    for _ in range(20):
        f()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


def capture(col, samples, seed, entry):
    """One collate call with its launch intercepted: the device arguments, kept alive for re-launching."""
    calls, bufs = [], []
    real, upload = lib.call, col._upload

    def keep(arrays, extra=0):
        buf, offs = upload(arrays, extra)
        bufs.append(buf)
        return buf, offs
    col._upload = keep

    def spy(name, *args):
        calls.append((name, args))
        return real(name, *args)
    lib.call = spy
    try:
        batch = col(samples, np.random.RandomState(seed))
    finally:
        del lib.call
        col._upload = upload
    torch.cuda.synchronize()
    (name, args), = calls
    assert name == entry, name
    return (batch, bufs), args


with open(os.path.join(ROOT, 'tests', 'golden', 'reference_det_pipeline.json')) as fh:
    train = tuples(json.load(fh))['train']
for t in train:
    if t['type'] == 'AutoAugment':
        t['policies'] = t['policies'][1:]
rng = np.random.RandomState(0)
samples = [dict(img=rng.randint(0, 256, (800, 800, 3)).astype(np.uint8), gt_bboxes=np.array([[10, 10, 300, 300]], np.float32),
                gt_labels=np.array([1])) for _ in range(2)]
chain = P.build_collate('det', train, dev)
keep_a, chain_args = capture(chain, samples, 1, 'rscotr_img_aug_chain_u8')
metas = keep_a[0]['img_metas']
Hout, Wout = keep_a[0]['img'].shape[-2:]
one = P.DeviceCollate('det', dev, flip_prob=0.5, resize=dict(size=(Hout, Wout)))
keep_b, one_args = capture(one, samples, 1, 'rscotr_img_aug_u8')
live = sum(m['img_shape'][0] * m['img_shape'][1] for m in metas)
rows = []
for _ in range(3):
    rows.append((timed(lambda: lib.call('rscotr_img_aug_chain_u8', *chain_args)),
                 timed(lambda: lib.call('rscotr_img_aug_u8', *one_args))))
c, o = (float(np.median([r[k] for r in rows])) for k in (0, 1))
print(json.dumps(dict(kernel='rscotr_img_aug_chain_u8', images=2, source='800x800', canvas=f'{Hout}x{Wout}',
                      img_shapes=[list(m['img_shape'][:2]) for m in metas], chain_us=[round(r[0], 2) for r in rows],
                      one_stage_us=[round(r[1], 2) for r in rows], ratio=round(c / o, 2),
                      chain_GBps=round((live * 3 + 2 * Hout * Wout * 12) / c / 1e3, 1),
                      one_stage_GBps=round(2 * Hout * Wout * 15 / o / 1e3, 1))), flush=True)
