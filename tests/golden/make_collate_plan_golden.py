"""Recorded host plans of the device input collate (rscotr_amd.pipeline: DeviceCollate's three routes and SegTTACollate), for
tests/test_collate_plan_cpu.py.

Everything in front of a launch is host code: with `lib.call` and `ops._stream` stubbed and a CPU device a collate draws, plans,
"uploads" and "launches" without a GPU and without the library.  `record()` drives seeded batches through `_run` (the body of
`__call__` below its GPU guard) and returns, per launch, the entry name with its scalar arguments and the mean / std floats, and
every meta, table, params, RandAugment meta and warp array the launch was handed, read back through the pointer it received; then
the returned batch (the shape of `img`, every key of every `img_metas` entry, the host-made target tensors).  Nothing recorded
depends on where the upload put a thing:
  an address column (an image, a label map, an erasing patch) is the CRC-32 of the bytes it addresses (H * stride, w * h * 3);
  a table offset is replaced by the table rows it selects (`tabs`: per sample its x rows, then its y rows; `warp` likewise);
  an address into workspace that no launch has written yet (RandAugment's frames and statistics) is which frame it is
  (frame index << 40 | byte offset in the frame; the statistics follow frame 1, so they are "frame 2").

    python tests/golden/make_collate_plan_golden.py      # rewrites tests/golden/collate_plan.npz

The committed file was written by this script on the commit BEFORE rscotr_amd/pipeline.py became a package with one host plan under
its routes.  There the plain route (and SegTTACollate, which calls a DeviceCollate per view) could not be driven on a CPU device:
the guard sat at the top of `__call__`, in front of everything.  The recording used a scratch copy of that commit whose ONLY edit
was the removal of that guard, with `_run` read as `__call__`.  The file pins that the split changed no draw, no table, no row
and no launch."""
import ctypes
import os
import random
import sys
import zlib

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'collate_plan.npz')
AUG_META, RA_META, PREP_META = 20, 16, 10
RA_WARP_OPS = (11, 12, 13)


def _read(ptr, count, ctype, dtype):
    if count == 0:
        return np.zeros(0, dtype)
    return np.ctypeslib.as_array((ctype * count).from_address(ptr)).astype(dtype).copy()


def _i64(ptr, rows, cols):
    return _read(ptr, rows * cols, ctypes.c_int64, np.int64).reshape(rows, cols)


def _i32(ptr, rows, cols):
    return _read(ptr, rows * cols, ctypes.c_int32, np.int32).reshape(rows, cols)


def _crc(ptr, nbytes):
    return zlib.crc32(ctypes.string_at(int(ptr), int(nbytes))) if nbytes else 0


def _floats3(p):
    return ','.join(repr(float(v)) for v in _read(p.value, 3, ctypes.c_float, np.float32))


def _canon(v):
    """A value of a batch as text: exact (repr of floats), with the NumPy dtypes named."""
    if isinstance(v, np.ndarray):
        return f'{v.dtype}{v.shape}{_canon(v.tolist())}'
    if isinstance(v, np.generic):
        return f'{v.dtype}:{v.item()!r}'
    if isinstance(v, dict):
        return '{' + ','.join(f'{k}:{_canon(v[k])}' for k in sorted(v)) + '}'
    if isinstance(v, (list, tuple)):
        return ('[%s]' if isinstance(v, list) else '(%s)') % ','.join(_canon(x) for x in v)
    return repr(v)


class _Recorder:
    def __init__(self):
        self.tables, self.seq, self.case, self.frames = {}, [], None, None

    def put(self, name, arr):
        self.tables[f'{self.case}_{sum(s.startswith(self.case + "|rscotr") for s in self.seq):02d}_{name}'] = arr

    def begin(self, case):
        self.case, self.frames = case, None

    def _aug_meta(self, src, meta_p, tab_p, B):
        """An (B, 20) meta row set of rscotr_img_aug_u8's layout -> (rows, the table rows they select)."""
        m, tabs = _i64(meta_p, B, AUG_META), []
        for r in m:
            off, H, _, stride, ow, oh, _, xt, yt, kx, ky = (int(v) for v in r[:11])
            if self.frames is None:
                r[0] = _crc(src + off, H * stride)
            else:  # the last step of the RandAugment route reads a frame a launch writes
                frame0, fbytes = self.frames
                rel = src + off - frame0
                assert 0 <= rel < 2 * fbytes
                r[0] = (rel // fbytes << 40) | (rel % fbytes)
            tabs += [_i32(tab_p + 4 * xt, ow, kx + 2).reshape(-1), _i32(tab_p + 4 * yt, oh, ky + 2).reshape(-1)]
            r[7] = r[8] = 0
            if r[16] * r[17] > 0:
                r[18] = _crc(src + int(r[18]), int(r[16] * r[17]) * 3)
        return m, np.concatenate(tabs) if tabs else np.zeros(0, np.int32)

    def _prep_meta(self, src, meta_p, B):
        m = _i64(meta_p, B, PREP_META)
        for r in m:
            r[0] = _crc(src + int(r[0]), int(r[1] * r[3]))
        return m

    def _frame(self, p):
        frame0, fbytes = self.frames
        return (p - frame0) // fbytes if fbytes else 0

    def call(self, name, *args):
        assert args[-1] == 0, 'the stubbed stream handle'
        if name == 'rscotr_img_prep_u8':
            src, meta, _, B, Hout, Wout, mean, std, to_rgb = args[:-1]
            self.put('meta', self._prep_meta(src, meta, B))
            scal = f'{B},{Hout},{Wout},{to_rgb}|{_floats3(mean)}|{_floats3(std)}'
        elif name == 'rscotr_seg_label_prep_u8':
            src, meta, _, B, Hout, Wout, rzl, pad = args[:-1]
            self.put('meta', self._prep_meta(src, meta, B))
            scal = f'{B},{Hout},{Wout},{rzl},{pad}'
        elif name == 'rscotr_img_aug_u8':
            src, meta, tab, prm, _, B, Hout, Wout, mean, std, to_rgb = args[:-1]
            m, tabs = self._aug_meta(src, meta, tab, B)
            self.put('meta', m)
            self.put('tabs', tabs)
            self.put('params', _read(prm, B * 4, ctypes.c_float, np.float32).reshape(B, 4))
            scal = f'{B},{Hout},{Wout},{to_rgb}|{_floats3(mean)}|{_floats3(std)}'
        elif name == 'rscotr_seg_label_aug_u8':
            src, meta, tab, _, B, Hout, Wout, rzl, pad = args[:-1]
            m, tabs = self._aug_meta(src, meta, tab, B)
            self.put('meta', m)
            self.put('tabs', tabs)
            scal = f'{B},{Hout},{Wout},{rzl},{pad}'
        elif name == 'rscotr_img_frames_u8':
            src, meta, tab, frames, B, H, W = args[:-1]
            m, tabs = self._aug_meta(src, meta, tab, B)
            self.put('meta', m)
            self.put('tabs', tabs)
            self.frames = (frames, (B * H * W * 3 + 15) // 16 * 16)
            scal = f'{B},{H},{W}'
        elif name == 'rscotr_randaug_u8':
            fin, fout, meta, warp, wtab, stats, need_stats, B, H, W = args[:-1]
            m, warps = _i32(meta, B, RA_META), []
            for r in m:
                if r[0] in RA_WARP_OPS:
                    warps.append(_i32(warp + 4 * int(r[6]), 1, 2 * int(r[1]) + 2 * int(r[2])).reshape(-1))
                    r[6] = 0
            self.put('rmeta', m)
            self.put('warp', np.concatenate(warps) if warps else np.zeros(0, np.int32))
            scal = (f'{self._frame(fin)}>{self._frame(fout)},stats@{self._frame(stats)},wtab:{_crc(wtab, 1024 * 16 * 2)},'
                    f'{need_stats},{B},{H},{W}')
        else:
            raise AssertionError(f'unexpected entry point {name}')
        self.seq.append(f'{self.case}|{name}|{scal}')
        return 0

    def batch(self, out):
        views = out['img'] if isinstance(out['img'], list) else [out['img']]
        metas = out['img_metas'] if isinstance(out['img'], list) else [out['img_metas']]
        self.seq.append(f'{self.case}|batch|keys={sorted(out)}|img=' + ';'.join(f'{tuple(t.shape)}{t.dtype}' for t in views))
        for v, ms in enumerate(metas):
            for b, m in enumerate(ms):
                self.seq.append(f'{self.case}|meta|{v}|{b}|{_canon(m)}')
        if 'gt_semantic_seg' in out:  # (the stubbed launch wrote nothing: the values are not the host's)
            t = out['gt_semantic_seg']
            self.seq.append(f'{self.case}|gt_semantic_seg|{tuple(t.shape)}{t.dtype}')
        if 'gt_label' in out:
            self.tables[f'{self.case}_gt_label'] = out['gt_label'].numpy().copy()
        if 'gt_bboxes' in out:
            for k, dt in (('gt_bboxes', np.float32), ('gt_labels', np.int64)):
                dev, host = [t.numpy() for t in out[k]], out[k + '_host']
                assert all(d.dtype == dt and h.dtype == dt and np.array_equal(d, h) for d, h in zip(dev, host)), k
                self.tables[f'{self.case}_{k}'] = np.concatenate([h.reshape(-1) for h in host])
            self.tables[f'{self.case}_gt_counts'] = np.asarray([len(h) for h in out['gt_labels_host']], np.int64)


def _samples(seed, shapes, task, labels=None):
    r = np.random.RandomState(seed)
    out = []
    for i, (h, w) in enumerate(shapes):
        s = dict(img=r.randint(0, 256, (h, w, 3)).astype(np.uint8))
        if task == 'cls':
            s['gt_label'] = int(r.randint(0, 45))
        elif task == 'det':
            n = i + 1
            x0, y0 = r.uniform(0, w / 2, n), r.uniform(0, h / 2, n)
            s['gt_bboxes'] = np.stack([x0, y0, x0 + r.uniform(2, w / 2, n), y0 + r.uniform(2, h / 2, n)], -1).astype(np.float32)
            s['gt_labels'] = r.randint(0, 20, n).astype(np.int64)
        else:
            s['gt_semantic_seg'] = labels(r, i, h, w)
        out.append(s)
    return out


def _seg_labels(r, i, h, w):
    """Sample 0: one class everywhere, so no window passes cat_max_ratio (every retry is drawn); the others mixed 0 .. 6."""
    return np.full((h, w), 3, np.uint8) if i == 0 else r.randint(0, 7, (h, w)).astype(np.uint8)


RA_SEEDS = (0, 1, 2)


def cases(P):
    """-> [(case name, collate, samples, seed)]; images are at most 64 px on a side."""
    seg_kw = dict(cat_max_ratio=0.75, reduce_zero_label=True, seg_pad_val=5)
    seg_shapes, cls_shapes = [(64, 60), (30, 36), (50, 44)], [(40, 52), (64, 33), (17, 64)]
    seg_aug = dict(seg_kw, crop_size=(40, 40), resize=dict(img_scale=(48, 48), ratio_range=(0.5, 2.0)), photometric=True)
    ra_kw = dict(random_resized_crop=dict(size=32), resize_backend='pillow', random_erasing=P.CLS_ERASING)
    out = [
        ('plain_cls', P.DeviceCollate('cls', 'cpu'), _samples(1, cls_shapes, 'cls'), 11),
        ('plain_det', P.collate_for('det', 'cpu'), _samples(2, [(40, 52), (64, 33), (17, 64), (33, 33)], 'det'), 12),
        # the crop is smaller than sample 0 and larger than sample 1 (both ways)
        ('plain_seg', P.DeviceCollate('seg', 'cpu', crop_size=(48, 40), **seg_kw), _samples(3, seg_shapes, 'seg', _seg_labels), 13),
        ('aug_seg', P.DeviceCollate('seg', 'cpu', **seg_aug), _samples(4, seg_shapes, 'seg', _seg_labels), 14),
        ('aug_seg_nolabels', P.DeviceCollate('seg', 'cpu', labels=False, **seg_aug), _samples(4, seg_shapes, 'seg', _seg_labels), 14),
        ('aug_det', P.DeviceCollate('det', 'cpu', flip_prob=0.5, size_divisor=32, resize=dict(img_scale=(80, 48))),
         _samples(5, [(40, 52), (64, 33), (17, 64)], 'det'), 15),
        ('aug_cls', P.DeviceCollate('cls', 'cpu', random_resized_crop=dict(size=32), resize_backend='pillow',
                                    random_erasing=dict(erase_prob=1.0, mode='rand')), _samples(6, cls_shapes, 'cls'), 16),
        ('eval_cls', P.eval_collate_for('cls', 'cpu', resize=dict(size=(24, 24))), _samples(7, cls_shapes, 'cls'), 17),
    ]
    for seed in RA_SEEDS:
        out.append((f'randaug{seed}', P.DeviceCollate('cls', 'cpu', rand_augment=True, **ra_kw),
                    _samples(20 + seed, cls_shapes + [(48, 48)], 'cls'), seed))
    out += [
        ('randaug_none', P.DeviceCollate('cls', 'cpu', rand_augment=dict(P.RAND_AUGMENT, num_policies=0), **ra_kw),
         _samples(8, cls_shapes, 'cls'), 18),
        ('empty_aug', P.DeviceCollate('seg', 'cpu', **seg_aug), [], 19),
        ('empty_randaug', P.DeviceCollate('cls', 'cpu', rand_augment=True, **ra_kw), [], 19),
        ('tta', P.SegTTACollate('cpu', dict(img_scale=[(32, 32), (48, 40)], flip=True), resize=dict(keep_ratio=True)),
         _samples(9, [(36, 50), (36, 50)], 'seg', _seg_labels), 20),
    ]
    return out


def record():
    """-> (tables: {name: array}, sequence: [str])"""
    from rscotr_amd import ops
    from rscotr_amd import pipeline as P
    from rscotr_amd._lib import lib
    rec = _Recorder()
    stream = ops._stream
    try:
        lib.call = rec.call
        ops._stream = lambda: 0
        for case, col, samples, seed in cases(P):
            rec.begin(case)
            rec.batch(col._run(samples, np.random.RandomState(seed), random.Random(seed)))
    finally:
        del lib.call
        ops._stream = stream
    return rec.tables, rec.seq


if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    tabs, sequence = record()
    np.savez_compressed(GOLDEN, sequence=np.asarray(sequence), **tabs)
    print(f'{GOLDEN}: {len(tabs)} tables, {len(sequence)} sequence lines, {os.path.getsize(GOLDEN)} bytes')
