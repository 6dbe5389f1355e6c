"""Time of the rotating input launches (rscotr_img_aug_rot_u8 / rscotr_seg_label_rot_u8) against the table route's pair
(rscotr_img_aug_u8 / rscotr_seg_label_aug_u8) on the SAME staged batch: the seg training collate (Resize ratio 0.5 .. 2.0,
RandomCrop 512, vertical RandomFlip, RandomRotate(prob=1, degree=20), PhotoMetricDistortion) on 8 tiles of 600 x 600.  The rotating
launches are recorded from one collate call and replayed; the table route's pair is replayed on their meta rows, tables and
parameters, which is that batch without its rotation.  Back-to-back replays: the 8.6 MB of source bytes stay cache-resident."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from rscotr_amd import pipeline as P
from rscotr_amd._lib import lib

dev = torch.device('cuda:0')
rng = np.random.RandomState(0)
B = 8
samples = [dict(img=rng.randint(0, 256, (600, 600, 3)).astype(np.uint8),
                gt_semantic_seg=np.repeat(np.repeat(rng.randint(0, 7, (38, 38)), 16, 0), 16, 1)[:600, :600].astype(np.uint8))
           for _ in range(B)]
col = P.train_collate_for('seg', dev, flip_direction='vertical', rotate=dict(prob=1.0, degree=20, pad_val=0, seg_pad_val=255))
real, rec = lib.call, {}


def call(name, *a):
    rec[name] = a
    real(name, *a)


lib.call = call
batch = col(samples, np.random.RandomState(1))
lib.call = real
torch.cuda.synchronize()
src, meta, tab, prm, rot, warp, out = rec['rscotr_img_aug_rot_u8'][:7]
lsrc, lmeta, ltab, lrot, lwarp, lout = rec['rscotr_seg_label_rot_u8'][:6]
launches = {
    'rscotr_img_aug_rot_u8': lambda: real('rscotr_img_aug_rot_u8', *rec['rscotr_img_aug_rot_u8']),
    'rscotr_img_aug_u8': lambda: real('rscotr_img_aug_u8', src, meta, tab, prm, out, *rec['rscotr_img_aug_rot_u8'][7:]),
    'rscotr_seg_label_rot_u8': lambda: real('rscotr_seg_label_rot_u8', *rec['rscotr_seg_label_rot_u8']),
    'rscotr_seg_label_aug_u8': lambda: real('rscotr_seg_label_aug_u8', lsrc, lmeta, ltab, lout, *rec['rscotr_seg_label_rot_u8'][6:]),
}
res = dict(batch=B, out='512x512', degrees=[round(m['rotate_degree'], 2) for m in batch['img_metas']])
for name, f in launches.items():
    for _ in range(5):
        f()
    torch.cuda.synchronize()
    rounds = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(50):
            f()
        e1.record()
        torch.cuda.synchronize()
        rounds.append(e0.elapsed_time(e1) / 50 * 1e3)
    res[name + '_us'] = round(float(np.median(rounds)), 2)
print(json.dumps(res))
