"""Host side of mmseg RandomRotate on the device (`rotate=`, seg only): the transform's settings, its two draws and the
fixed-point coordinate tables of `rscotr_img_aug_rot_u8` / `rscotr_seg_label_rot_u8`.  mmseg 0.28 / mmcv restated as remembered
(tests/orient_oracle.py spells them out): parity with mm* / cv2 is by reading and unpinned.
    rotate = np.random.rand() < prob; degree = np.random.uniform(min(*degree), max(*degree))      # always both draws
    if rotate: img = mmcv.imrotate(img, angle=degree, border_value=pad_val, center=center, auto_bound=False)
               seg = mmcv.imrotate(seg, ..., border_value=seg_pad_val, interpolation='nearest')
mmcv.imrotate: cv2.getRotationMatrix2D(center or ((w - 1) / 2, (h - 1) / 2), -angle, 1) then cv2.warpAffine (bilinear for the image):
positive degrees turn clockwise.  `auto_bound=True` changes the frame size and is not implemented."""
import math

import numpy as np

from .randaug import warp_table

ROT_ROW = 4  # include/rscotr.h: the rot rows of rscotr_img_aug_rot_u8 / rscotr_seg_label_rot_u8
ROTATE = dict(pad_val=0, seg_pad_val=255, center=None, auto_bound=False)  # mmseg RandomRotate's defaults


def rotate_config(cfg):
    """RandomRotate(prob, degree, pad_val=0, seg_pad_val=255, center=None, auto_bound=False) -> the normalised settings: degree a
    (lo, hi) pair (a number d means (-d, d)), pad_val a BGR triple."""
    cfg = dict(ROTATE, **cfg)
    for k in ('prob', 'degree'):
        if k not in cfg:
            raise ValueError(f'rotate: {k} is required')
    unknown = set(cfg) - {'prob', 'degree', 'pad_val', 'seg_pad_val', 'center', 'auto_bound'}
    if unknown:
        raise ValueError(f'rotate: unknown settings {sorted(unknown)}')
    if cfg['auto_bound']:
        raise NotImplementedError('RandomRotate(auto_bound=True) changes the frame size')
    if not 0 <= cfg['prob'] <= 1:
        raise ValueError(f"rotate: prob {cfg['prob']!r} outside [0, 1]")
    deg = cfg['degree']
    if isinstance(deg, (int, float)):
        if deg <= 0:
            raise ValueError(f'rotate: degree {deg!r} must be positive')  # (mmseg asserts it)
        deg = (-deg, deg)
    if len(deg) != 2:
        raise ValueError(f'rotate: degree {deg!r} must be a number or a (min, max) pair')
    pv = cfg['pad_val']
    pv = tuple(int(v) for v in ((pv,) * 3 if isinstance(pv, (int, float)) else pv))
    if len(pv) != 3 or not all(0 <= v <= 255 for v in pv):
        raise ValueError(f"rotate: pad_val {cfg['pad_val']!r} must be one or three values in [0, 255]")
    if not 0 <= int(cfg['seg_pad_val']) <= 255:
        raise ValueError(f"rotate: seg_pad_val {cfg['seg_pad_val']!r} outside [0, 255]")
    center = cfg['center']
    if center is not None and len(center) != 2:
        raise ValueError(f'rotate: center {center!r} must be an (x, y) pair')
    return dict(prob=float(cfg['prob']), degree=(float(deg[0]), float(deg[1])), pad_val=pv, seg_pad_val=int(cfg['seg_pad_val']),
                center=None if center is None else (float(center[0]), float(center[1])))


def rotate_draw(cfg, rng):
    """RandomRotate.__call__'s draws, always both -> the degree to apply, or None."""
    rotate = bool(rng.rand() < cfg['prob'])
    degree = rng.uniform(min(*cfg['degree']), max(*cfg['degree']))
    return float(degree) if rotate else None


def rotation_matrix(degree, w, h, center=None):
    """The FORWARD matrix mmcv.imrotate hands cv2.warpAffine for a (h, w) frame: cv2.getRotationMatrix2D(center, -degree, 1),
    float64, row-major list of 6."""
    a = -degree * math.pi / 180.0
    al, be = math.cos(a), math.sin(a)
    cx, cy = ((w - 1) * 0.5, (h - 1) * 0.5) if center is None else center
    return [al, be, (1 - al) * cx - be * cy, -be, al, be * cx + (1 - al) * cy]


def rotate_rows(cfg, ds, labels):
    """The rot rows and the coordinate tables of a batch of draws `ds` (DeviceCollate.draw; `rotate`: the degree or None) ->
    (rot (B, 4) int32 for the image launch, lrot likewise for the label launch, warp int32).  A rotated sample owns two
    tables in `warp`, the bilinear one (round_delta 16) and, with `labels`, the nearest one (512); offset 0 means not rotated,
    so `warp` starts with four unused words."""
    B = len(ds)
    rot, lrot = np.zeros((max(B, 1), ROT_ROW), np.int32), np.zeros((max(B, 1), ROT_ROW), np.int32)
    rot[:, 1:4], lrot[:, 1] = cfg['pad_val'], cfg['seg_pad_val']
    warps, n = [np.zeros(4, np.int32)], 4
    for b, d in enumerate(ds):
        if d.get('rotate') is None:
            continue
        cw, ch = d['win'][2], d['win'][3]
        M = rotation_matrix(d['rotate'], cw, ch, cfg['center'])
        for rows, rd in ((rot, 16), (lrot, 512)) if labels else ((rot, 16),):
            t = warp_table(M, cw, ch, rd)
            assert t.size == 2 * (cw + ch)
            if np.abs(t).max() >= 2 ** 29:  # (the kernel adds two entries in 32 bits)
                raise ValueError(f"rotate: center {cfg['center']!r} is too far from a {cw} x {ch} window")
            rows[b, 0], n = n, n + t.size
            warps.append(t)
    return rot, lrot, np.concatenate(warps)
