"""Throughput of the device resampling / colour input kernel (rscotr_img_aug_u8) on device-resident bytes for the reference's
native batches, against rscotr_img_prep_u8 at the same output size (12 B written per output pixel), plus the host time of
one collate call (draws, tables, staging, upload):
  cls  16 x 256^2 -> RandomResizedCrop 224^2, Pillow bicubic
  seg   8 x 512^2 at ratio 2.0 (1024^2) cropped to 512^2, bilinear, PhotoMetricDistortion on every step
  det   1 x 1000 x 700 -> keep-ratio (1333, 800), bilinear."""
import ctypes
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from rscotr_amd import pipeline as P
from rscotr_amd._lib import lib

dev = torch.device('cuda:0')
rng = np.random.RandomState(0)
m = (ctypes.c_float * 3)(*P.IMG_NORM['mean'])
s = (ctypes.c_float * 3)(*P.IMG_NORM['std'])
mp, sp = ctypes.cast(m, ctypes.c_void_p), ctypes.cast(s, ctypes.c_void_p)
st = torch.cuda.current_stream().cuda_stream


def timed(f, n=50):
    for _ in range(5):
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
    """One collate call with the two launches intercepted: their device arguments, kept alive for re-launching."""
    calls, bufs = [], []
    real, upload = lib.call, col._upload

    def keep(arrays):  # the device copy the captured pointers point into stays alive with the returned batch
        buf, offs = upload(arrays)
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
        lib.call, col._upload = real, upload
    torch.cuda.synchronize()
    return (batch, bufs), calls


def case(name, col, samples):
    alive, calls = capture(col, samples, 1)  # noqa: F841 (holds the batch and the uploaded bytes until the case ends)
    (fn, args), = [c for c in calls if c[0] == 'rscotr_img_aug_u8']
    B, Hout, Wout = args[5], args[6], args[7]
    aug_us = timed(lambda: lib.call(fn, *args))
    # the existing launch at the same output size: crop windows of Hout x Wout out of device-resident images
    H, W = max(Hout, 8), max(Wout, 8)
    src = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, device=dev)
    meta = torch.tensor([[b * H * W * 3, H, W, W * 3, 0, 0, Wout, Hout, b & 1, 0] for b in range(B)], dtype=torch.int64,
                        device=dev)
    out = torch.empty((B, 3, Hout, Wout), device=dev)
    prep_us = timed(lambda: lib.call('rscotr_img_prep_u8', src.data_ptr(), meta.data_ptr(), out.data_ptr(), B, Hout, Wout,
                                     mp, sp, 1, st))
    # host time of one whole collate call (ends in a device synchronise)
    hs = []
    for k in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        col(samples, np.random.RandomState(k))
        torch.cuda.synchronize()
        hs.append((time.perf_counter() - t0) * 1e3)
    byt = B * Hout * Wout * 12
    print(json.dumps(dict(case=name, kernel='rscotr_img_aug_u8', images=B, out=f'{Hout}x{Wout}', us=round(aug_us, 2),
                          GBps_written=round(byt / aug_us / 1e3, 1), prep_us_same_out=round(prep_us, 2),
                          ratio_to_prep=round(aug_us / prep_us, 2), collate_host_ms_median=round(float(np.median(hs)), 2))),
          flush=True)


cls = [dict(img=rng.randint(0, 256, (256, 256, 3)).astype(np.uint8), gt_label=0) for _ in range(16)]
case('cls', P.train_collate_for('cls', dev, random_erasing=dict(P.CLS_ERASING, erase_prob=0.0)), cls)
seg = [dict(img=rng.randint(0, 256, (512, 512, 3)).astype(np.uint8), gt_semantic_seg=rng.randint(0, 7, (512, 512)).astype(np.uint8))
       for _ in range(8)]
col = P.train_collate_for('seg', dev, resize=dict(img_scale=(512, 512), ratio_range=(2.0, 2.0)))
col._photometric_draws = lambda r: (P.PM_BRIGHT | P.PM_CONTRAST | P.PM_SAT | P.PM_HUE, 10.0, 1.2, 0.8, 5)  # every step on
case('seg', col, seg)
det = [dict(img=rng.randint(0, 256, (700, 1000, 3)).astype(np.uint8), gt_bboxes=np.array([[10, 10, 100, 100]], np.float32),
            gt_labels=np.array([1]))]
case('det', P.train_collate_for('det', dev), det)
