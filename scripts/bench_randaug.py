"""The cls recipe with RandAugment on the device (16 x 256^2 -> RandomResizedCrop 224^2, Pillow bicubic, flip, RandAugment with
the reference's settings, RandomErasing): microseconds per batch of its launch sequence (rscotr_img_frames_u8, one
rscotr_randaug_u8 per slot, rscotr_img_aug_u8) on device-resident bytes, against the single rscotr_img_aug_u8 launch of the
same batch without the stage, measured in the same run (several repetitions, alternating), plus the host time of one whole
collate call of each."""
import json
import os
import random
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from rscotr_amd import pipeline as P
from rscotr_amd._lib import lib

dev = torch.device('cuda:0')


def timed(f, n=200):
    for _ in range(10):
        f()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


def capture(col, samples, seed):
    """One collate call with its library calls intercepted: their device arguments, kept alive for re-launching."""
    calls, bufs = [], []
    real, upload = lib.call, col._upload

    def keep(arrays, **kw):
        buf, offs = upload(arrays, **kw)
        bufs.append(buf)
        return buf, offs
    col._upload = keep

    def spy(name, *args):
        calls.append((name, args))
        return real(name, *args)
    lib.call = spy
    try:
        batch = col(samples, np.random.RandomState(seed), random.Random(seed))
    finally:
        lib.call, col._upload = real, upload
    torch.cuda.synchronize()
    return (batch, bufs), calls


def host_ms(col, samples):
    hs = []
    for k in range(7):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        col(samples, np.random.RandomState(k), random.Random(k))
        torch.cuda.synchronize()
        hs.append((time.perf_counter() - t0) * 1e3)
    return hs[2:]


rng = np.random.RandomState(0)
cls = [dict(img=rng.randint(0, 256, (256, 256, 3)).astype(np.uint8), gt_label=0) for _ in range(16)]
plain = P.train_collate_for('cls', dev)
ra = P.train_collate_for('cls', dev, rand_augment=True)
keep_a, calls_a = capture(plain, cls, 1)
keep_b, calls_b = capture(ra, cls, 1)
assert [c[0] for c in calls_a] == ['rscotr_img_aug_u8']
plan = [e for m in keep_b[0]['img_metas'] for e in m['rand_augment']]


def run(calls):
    for fn, args in calls:
        lib.call(fn, *args)


a_us, b_us, per = [], [], {}
for rep in range(5):  # alternating, same process, same box
    a_us.append(timed(lambda: run(calls_a)))
    b_us.append(timed(lambda: run(calls_b)))
for i, c in enumerate(calls_b):
    per[f'{i}:{c[0]}'] = round(timed(lambda: run([c])), 2)
ha, hb = host_ms(plain, cls), host_ms(ra, cls)
print(json.dumps(dict(case='cls 16x256^2 -> 224^2', device=torch.cuda.get_device_name(0),
                      sequence=[c[0] for c in calls_b], library_calls=len(calls_b),
                      kernel_launches=2 + sum(1 + 2 * int(c[1][6]) for c in calls_b if c[0] == 'rscotr_randaug_u8'),
                      applied_ops=sum(e[2] for e in plan), slots=len(plan),
                      randaug_sequence_us=[round(v, 2) for v in b_us], single_launch_us=[round(v, 2) for v in a_us],
                      per_call_us=per, collate_host_ms_randaug=[round(v, 2) for v in hb],
                      collate_host_ms_plain=[round(v, 2) for v in ha])), flush=True)
