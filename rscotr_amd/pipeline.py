"""Device-side input path: the per-sample pipeline tail of the reference's dataset configs and
the collate step as ONE HIP launch per batch (`rscotr_img_prep_u8`, `rscotr_seg_label_prep_u8`), plus thin readers for
the three datasets' on-disk layouts.

Reference pipelines (configs/_base_/cls/resisc_swin_224.py:7-39, configs/_base_/det/dior.py:11-20,
configs/_base_/seg/potsdam_IRRG_all.py:8-19):
    decode (host) -> [Resize / RandomResizedCrop] -> RandomCrop window (seg) -> RandomFlip -> [PhotoMetricDistortion]
           -> [RandomErasing] -> Normalize(mean, std, to_rgb) -> Pad -> ImageToTensor / DefaultFormatBundle -> collate
(bracketed: the optional stages below; mmcls RandAugment sits between RandomFlip and RandomErasing in the cls pipeline).
Everything from the crop window on runs on the device; the host only draws the random decisions (with the same NumPy
calls and in the same order as the mm* transforms, so a seeded run makes the same decisions) and uploads the raw bytes
through one pinned staging buffer.  There is no CPU fallback: without the HIP library `collate` raises.

Optional stages (`resize=`, `random_resized_crop=`, `photometric=`, `random_erasing=`; all off by default, and then the
collate is exactly the crop / flip / normalize / pad launch above) move the resampling and colour steps onto the device as
well: one `rscotr_img_aug_u8` launch per batch.  The host draws their random decisions and builds per-axis resampling
tables (source index, tap count and integer weights per output coordinate), so the device arithmetic is integer and exact:
  'cv2'     mmcv imresize / imrescale interpolation='bilinear': the scalar fixed-point form of OpenCV's uint8 INTER_LINEAR
            (11-bit weights).  Parity with cv2 itself is unpinned: +-1 LSB expected (SIMD / IPP / exact-2x paths), unmeasured.
  'pillow'  mmcv backend='pillow', interpolation='bicubic': Pillow's ImagingResample (antialiased, 22-bit weights,
            uint8-clipped horizontal pass then vertical pass); equal to Pillow's own output.
Label maps are resampled 'nearest' (mmcv: cv2 INTER_NEAREST).

RandAugment (`rand_augment=`, cls only, off by default; configs/_base_/cls/resisc_swin_224.py:15-27 with the policies of
configs/_base_/cls/rand_aug.py) turns the one launch into a short sequence: `rscotr_img_frames_u8` writes the resized, flipped
uint8 frames, `rscotr_randaug_u8` runs once per policy slot (each sample its own operation, ping frame to pong frame), and
`rscotr_img_aug_u8` finishes over identity entries (RandomErasing, Normalize, pad).  The host draws from BOTH of mmcls's
generators in its order (Python `random`: the policy choice and the gauss magnitudes; `numpy.random`: each transform's prob and
sign draws) and builds the integer tables of the warps (cv2.warpAffine's fixed point).  The operations are restated from
mmcv / OpenCV as remembered (tests/randaug_oracle.py spells them out): parity with mm* / cv2 is by reading and unpinned.
"""
import ctypes
import json
import math
import os
import random

import numpy as np
import torch

from ._lib import lib
from . import ops

IMG_NORM = dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], to_rgb=True)
META = 10
AUG_META, AUG_PARAMS = 20, 4  # include/rscotr.h: rscotr_img_aug_u8's meta row and params row
RESAMPLE_NEAREST, RESAMPLE_LINEAR, RESAMPLE_PIL = 0, 1, 2
PM_BRIGHT, PM_CONTRAST, PM_CONTRAST_FIRST, PM_SAT, PM_HUE = 1, 2, 4, 8, 16
PHOTOMETRIC = dict(brightness_delta=32, contrast_range=(0.5, 1.5), saturation_range=(0.5, 1.5), hue_delta=18)
RANDOM_ERASING = dict(erase_prob=0.5, min_area_ratio=0.02, max_area_ratio=0.4, aspect_range=(3 / 10, 10 / 3), mode='const',
                      fill_color=(128, 128, 128), fill_std=None)  # mmcls RandomErasing's defaults
RANDOM_RESIZED_CROP = dict(size=224, scale=(0.08, 1.0), ratio=(3. / 4., 4. / 3.), max_attempts=10)
# ---- RandAugment (include/rscotr.h: rscotr_randaug_u8's op codes, meta row and stats row) -------------------------------
RA_OPS = dict(AutoContrast=1, Equalize=2, Invert=3, Posterize=4, Solarize=5, SolarizeAdd=6, ColorTransform=7, Contrast=8,
              Brightness=9, Sharpness=10, Rotate=11, Shear=12, Translate=13)
RA_META, RA_STATS = 16, 770
RA_STATS_OPS = (RA_OPS['AutoContrast'], RA_OPS['Equalize'], RA_OPS['Contrast'])
RA_SIGNED = ('Rotate', 'Shear', 'Translate', 'ColorTransform', 'Contrast', 'Brightness', 'Sharpness')  # random_negative
RA_WARPS = dict(Rotate='nearest', Shear='bicubic', Translate='nearest')  # mmcls's default interpolation of each
_RA_KEY = dict(Rotate='angle', Posterize='bits', Solarize='thr')  # the argument a magnitude lands in (else 'magnitude')
# configs/_base_/cls/rand_aug.py:2-42 and the RandAugment arguments of configs/_base_/cls/resisc_swin_224.py:15-27
RAND_INCREASING_POLICIES = [
    dict(type='AutoContrast'), dict(type='Equalize'), dict(type='Invert'),
    dict(type='Rotate', magnitude_key='angle', magnitude_range=(0, 30)),
    dict(type='Posterize', magnitude_key='bits', magnitude_range=(4, 0)),
    dict(type='Solarize', magnitude_key='thr', magnitude_range=(256, 0)),
    dict(type='SolarizeAdd', magnitude_key='magnitude', magnitude_range=(0, 110)),
    dict(type='ColorTransform', magnitude_key='magnitude', magnitude_range=(0, 0.9)),
    dict(type='Contrast', magnitude_key='magnitude', magnitude_range=(0, 0.9)),
    dict(type='Brightness', magnitude_key='magnitude', magnitude_range=(0, 0.9)),
    dict(type='Sharpness', magnitude_key='magnitude', magnitude_range=(0, 0.9)),
    dict(type='Shear', magnitude_key='magnitude', magnitude_range=(0, 0.3), direction='horizontal'),
    dict(type='Shear', magnitude_key='magnitude', magnitude_range=(0, 0.3), direction='vertical'),
    dict(type='Translate', magnitude_key='magnitude', magnitude_range=(0, 0.45), direction='horizontal'),
    dict(type='Translate', magnitude_key='magnitude', magnitude_range=(0, 0.45), direction='vertical')]
RAND_AUGMENT = dict(policies=RAND_INCREASING_POLICIES, num_policies=2, total_level=10, magnitude_level=9, magnitude_std=0.5,
                    hparams=dict(pad_val=[104, 116, 124], interpolation='bicubic'))


def _host_floats(v):
    arr = (ctypes.c_float * 3)(*[float(x) for x in v])
    return arr, ctypes.cast(arr, ctypes.c_void_p)


def _round_up(x, d):
    return (x + d - 1) // d * d


# ---- per-axis resampling tables: entry j (output coordinate o0 + j of an axis resized n_in -> n_out, whose source starts at
# src0) = {first source index, taps n, n weights}, int32 rows of K + 2 words ------------------------------------------------
def _table(first, n, w):
    K = max(int(w.shape[1]), 1)
    t = np.zeros((len(first), K + 2), np.int32)
    t[:, 0], t[:, 1] = first, n
    t[:, 2:2 + w.shape[1]] = w
    return t


def _axis_nearest(n_in, n_out, src0, o0, count):
    """cv2 INTER_NEAREST (mmcv 'nearest'): sx = min(floor(o * (1 / (n_out / n_in))), n_in - 1), in float64."""
    o = np.arange(o0, o0 + count, dtype=np.float64)
    s = np.minimum(np.floor(o * (1.0 / (n_out / n_in))).astype(np.int64), n_in - 1)
    return _table(s + src0, np.ones(count, np.int64), np.zeros((count, 1), np.int32))


def _axis_linear(n_in, n_out, src0, o0, count):
    """cv2 INTER_LINEAR, uint8 fixed point: f = float32((o + 0.5) * scale - 0.5), s = floor(f), a = f - s; out-of-range
    taps clamp to ONE tap of weight 2048; weights rint((1 - a) * 2048), rint(a * 2048) in float32 (saturate_cast<short>)."""
    o = np.arange(o0, o0 + count, dtype=np.float64)
    f = ((o + 0.5) * (1.0 / (n_out / n_in)) - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    a = (f - s.astype(np.float32)).astype(np.float32)
    clamp = (s < 0) | (s >= n_in - 1)
    s = np.where(s < 0, 0, np.where(s >= n_in - 1, n_in - 1, s))
    a = np.where(clamp, np.float32(0), a).astype(np.float32)
    w = np.stack([np.rint((np.float32(1) - a) * np.float32(2048)), np.rint(a * np.float32(2048))], -1).astype(np.int32)
    w[clamp, 1] = 0
    return _table(s + src0, np.where(clamp, 1, 2), w)


def _bicubic(x):  # Pillow Resample.c bicubic_filter, a = -0.5
    x = np.abs(x)
    a = -0.5
    return np.where(x < 1.0, ((a + 2.0) * x - (a + 3.0)) * x * x + 1,
                    np.where(x < 2.0, (((x - 5) * x + 8) * x - 4) * a, 0.0))


def _axis_pil_bicubic(n_in, n_out, src0, o0, count):
    """Pillow precompute_coeffs + normalize_coeffs_8bpc for BICUBIC (support 2 * max(scale, 1)), coefficients normalised in
    float64 (sequential sum, as the C loop), then 22-bit fixed point rounded away from zero."""
    scale = n_in / n_out
    fscale = max(scale, 1.0)
    support = 2.0 * fscale
    ksize = int(np.ceil(support)) * 2 + 1
    center = (np.arange(o0, o0 + count, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum(np.trunc(center - support + 0.5).astype(np.int64), 0)
    xmax = np.minimum(np.trunc(center + support + 0.5).astype(np.int64), n_in) - xmin
    t = np.arange(ksize)
    live = t[None, :] < xmax[:, None]
    k = np.where(live, _bicubic(((t[None, :] + xmin[:, None]) - center[:, None] + 0.5) * (1.0 / fscale)), 0.0)
    ww = np.zeros(count)
    for i in range(ksize):
        ww = ww + k[:, i]
    k = np.where(ww[:, None] != 0.0, k / np.where(ww == 0.0, 1.0, ww)[:, None], k)
    w = np.where(k < 0, np.trunc(-0.5 + k * (1 << 22)), np.trunc(0.5 + k * (1 << 22))).astype(np.int32)
    w[~live] = 0
    return _table(xmin + src0, xmax, w)


_AXIS = {RESAMPLE_NEAREST: _axis_nearest, RESAMPLE_LINEAR: _axis_linear, RESAMPLE_PIL: _axis_pil_bicubic}


def _scale_size(w, h, scale):  # mmcv _scale_size
    return int(w * float(scale) + 0.5), int(h * float(scale) + 0.5)


def rescale_size(w, h, scale):
    """mmcv rescale_size: a number, or a (long, short) edge pair -> ((new_w, new_h), scale factor)."""
    if isinstance(scale, (float, int)):
        sf = scale
    else:
        sf = min(max(scale) / max(h, w), min(scale) / min(h, w))
    return _scale_size(w, h, sf), sf


def ra_unsupported(cfg):
    """Why the device stage cannot run this RandAugment config (a phrase naming the policy or interpolation), or None."""
    pol = cfg.get('policies')
    if not isinstance(pol, (list, tuple)) or len(pol) == 0:
        return f'policies={pol!r} (a non-empty list of policy dicts is needed)'
    hp = cfg.get('hparams') or {}
    for p in pol:
        typ = p.get('type') if isinstance(p, dict) else p
        if typ not in RA_OPS:
            return f'policy {typ!r}'
        if typ in RA_WARPS:
            interp = p.get('interpolation', hp.get('interpolation', RA_WARPS[typ]))
            if interp not in ('nearest', 'bicubic'):
                return f'{typ} with interpolation={interp!r} (nearest and bicubic are implemented)'
    return None


def _ra_config(cfg):
    """The normalised settings: mmcls RandAugment's defaults filled in and `hparams` merged into the policies that accept
    them and lack them (pad_val / interpolation: Rotate, Shear, Translate), pad_val as a BGR triple."""
    cfg = dict(RAND_AUGMENT) if cfg is True else dict(cfg)
    why = ra_unsupported(cfg)
    if why is not None:
        raise ValueError(f'rand_augment: {why}')
    hp = dict(cfg.get('hparams') or {})
    pols = []
    for p in cfg['policies']:
        p = dict(p)
        if p['type'] in RA_WARPS:
            p.setdefault('interpolation', hp.get('interpolation', RA_WARPS[p['type']]))
            pv = p.get('pad_val', hp.get('pad_val', 128))
            p['pad_val'] = tuple(int(v) for v in ((pv,) * 3 if isinstance(pv, (int, float)) else pv))
            if len(p['pad_val']) != 3 or not all(0 <= v <= 255 for v in p['pad_val']):
                raise ValueError(f'rand_augment: pad_val {pv!r} must be one or three values in [0, 255]')
            if p['type'] != 'Rotate' and p.setdefault('direction', 'horizontal') not in ('horizontal', 'vertical'):
                raise ValueError(f"rand_augment: {p['type']} direction {p['direction']!r}")
        if ('magnitude_key' in p) != ('magnitude_range' in p):
            raise ValueError(f"rand_augment: {p['type']} needs magnitude_key and magnitude_range together")
        pols.append(p)
    out = dict(policies=pols, num_policies=int(cfg.get('num_policies', 0)), magnitude_level=cfg.get('magnitude_level', 0),
               total_level=cfg.get('total_level', 30), magnitude_std=cfg.get('magnitude_std', 0.), hparams=hp)
    if out['num_policies'] < 0 or out['total_level'] <= 0:
        raise ValueError('rand_augment: num_policies >= 0 and total_level > 0 expected')
    return out


def _ra_matrix(p, m, w, h):
    """The FORWARD 2 x 3 matrix mmcv hands cv2.warpAffine (float64, row-major list of 6): imrotate's
    getRotationMatrix2D(((w - 1) / 2, (h - 1) / 2), -angle, 1), imshear's and imtranslate's."""
    if p['type'] == 'Rotate':
        a = -m * math.pi / 180.0
        al, be = math.cos(a), math.sin(a)
        cx, cy = (w - 1) * 0.5, (h - 1) * 0.5
        return [al, be, (1 - al) * cx - be * cy, -be, al, be * cx + (1 - al) * cy]
    hor = p['direction'] == 'horizontal'
    if p['type'] == 'Shear':
        return [1.0, m, 0.0, 0.0, 1.0, 0.0] if hor else [1.0, 0.0, 0.0, m, 1.0, 0.0]
    return [1.0, 0.0, m * w, 0.0, 1.0, 0.0] if hor else [1.0, 0.0, 0.0, 0.0, 1.0, m * h]


def _ra_warp_table(M, w, h, bicubic):
    """cv2.warpAffine without WARP_INVERSE_MAP: M inverted in float64 as OpenCV does, then the int32 coordinate tables
    adelta[w] | bdelta[w] | X0[h] | Y0[h] (AB_SCALE = 1024, round_delta = 16 bicubic / 512 nearest folded into X0, Y0)."""
    m0, m1, m2, m3, m4, m5 = [float(v) for v in M]
    D = m0 * m4 - m1 * m3
    D = 1.0 / D if D != 0 else 0.0
    a11, a22 = m4 * D, m0 * D
    m0, m1, m3, m4 = a11, m1 * -D, m3 * -D, a22
    b1 = -m0 * m2 - m1 * m5
    b2 = -m3 * m2 - m4 * m5
    x, y = np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64)
    rd = 16 if bicubic else 512
    t = np.concatenate([np.rint(m0 * x * 1024), np.rint(m3 * x * 1024), np.rint((m1 * y + b1) * 1024) + rd,
                        np.rint((m4 * y + b2) * 1024) + rd])
    return np.clip(t, -2 ** 30, 2 ** 30).astype(np.int32)  # (a coordinate that large is outside any frame either way)


_CUBIC_WTAB = None


def cubic_weight_table():
    """OpenCV's bicubic remap weights (initInterTab2D, INTER_CUBIC, fixed point): (1024, 16) int16, row ay * 32 + ax = the
    4 x 4 products cy[k1] * cx[k2] of the float32 cubic coefficients (A = -0.75) at a / 32, times 32768, rounded half to even;
    a row that does not sum to 32768 gives its deficit to the largest, or takes its excess from the smallest, of the 2 x 2 block
    k1, k2 in (2, 3) -- OpenCV scans `ksize / 2 .. ksize / 2 + 1`, which for 4 taps is that block, not (1, 2); with (1, 2) the
    row of a = (0, 0) would need the weight 32768, which int16 does not hold."""
    global _CUBIC_WTAB
    if _CUBIC_WTAB is not None:
        return _CUBIC_WTAB
    f = np.float32
    A = f(-0.75)
    x = (np.arange(32, dtype=np.float32) * f(1.0 / 32)).astype(f)
    c = np.zeros((32, 4), f)
    c[:, 0] = ((A * (x + f(1)) - f(5) * A) * (x + f(1)) + f(8) * A) * (x + f(1)) - f(4) * A
    c[:, 1] = ((A + f(2)) * x - (A + f(3))) * x * x + f(1)
    c[:, 2] = ((A + f(2)) * (f(1) - x) - (A + f(3))) * (f(1) - x) * (f(1) - x) + f(1)
    c[:, 3] = f(1) - c[:, 0] - c[:, 1] - c[:, 2]
    v = (c[:, None, :, None] * c[None, :, None, :]).astype(f)  # [ay, ax, k1, k2]
    t = np.clip(np.rint(v * f(32768)), -32768, 32767).astype(np.int64).reshape(1024, 4, 4)
    for row in t:
        diff = int(row.sum()) - 32768
        if diff:
            lo = hi = (2, 2)
            for k1 in (2, 3):
                for k2 in (2, 3):
                    if row[k1, k2] < row[lo]:
                        lo = (k1, k2)
                    elif row[k1, k2] > row[hi]:
                        hi = (k1, k2)
            row[hi if diff < 0 else lo] -= diff
    _CUBIC_WTAB = t.reshape(1024, 16).astype(np.int16)
    return _CUBIC_WTAB


def _f32_bits(v):
    return int(np.float32(v).view(np.int32))


class DeviceCollate:
    """Batch builder for one task.  `__call__(samples, rng=None, py_rng=None)` takes the decoded samples of one batch
    (dicts with `img`: HWC uint8 BGR ndarray, and per task `gt_label` | `gt_bboxes`, `gt_labels` | `gt_semantic_seg`:
    HW uint8) and returns the batch dict `MTL.train_step` consumes, tensors on `device`."""

    def __init__(self, task, device, img_norm_cfg=None, flip_prob=0.5, size_divisor=None, crop_size=None,
                 cat_max_ratio=1.0, reduce_zero_label=False, seg_pad_val=255, ignore_index=255, resize=None,
                 random_resized_crop=None, photometric=None, random_erasing=None, resize_backend='cv2',
                 rand_augment=None, labels=True):
        """Optional stages (None = off; any of them on routes the batch through `rscotr_img_aug_u8`):
        resize: mmseg / mmdet Resize, dict(img_scale=(long, short), ratio_range=None | (lo, hi), keep_ratio=True), or
                mmcls Resize, dict(size=(h, w)) (a fixed size);
        random_resized_crop: mmcls RandomResizedCrop, dict(size, scale, ratio, max_attempts) (RANDOM_RESIZED_CROP);
        photometric: mmseg PhotoMetricDistortion, True or dict (PHOTOMETRIC);
        random_erasing: mmcls RandomErasing, dict (RANDOM_ERASING);
        resize_backend: 'cv2' (bilinear) | 'pillow' (bicubic), the image resample of resize / random_resized_crop;
        rand_augment: mmcls RandAugment (task 'cls' only), True (RAND_AUGMENT, the reference's settings) or dict(policies,
                num_policies, magnitude_level, total_level=30, magnitude_std=0., hparams); it routes the batch through
                `rscotr_img_frames_u8` -> `rscotr_randaug_u8` per slot -> `rscotr_img_aug_u8`;
        labels: False = a seg batch without `gt_semantic_seg` (test time: the label maps are neither staged nor resampled)."""
        assert task in ('cls', 'det', 'seg')
        self.task, self.device = task, torch.device(device)
        cfg = dict(IMG_NORM if img_norm_cfg is None else img_norm_cfg)
        self.mean, self.std, self.to_rgb = cfg['mean'], cfg['std'], bool(cfg.get('to_rgb', True))
        self.flip_prob, self.size_divisor, self.crop_size = flip_prob, size_divisor, crop_size
        self.cat_max_ratio, self.reduce_zero_label = cat_max_ratio, reduce_zero_label
        self.seg_pad_val, self.ignore_index = seg_pad_val, ignore_index
        self._stage = None  # pinned byte staging buffer (grow-only)
        if resize_backend not in ('cv2', 'pillow'):
            raise ValueError(f'resize_backend must be cv2 (bilinear) or pillow (bicubic), not {resize_backend!r}')
        if resize is not None and random_resized_crop is not None:
            raise ValueError('resize and random_resized_crop are exclusive')
        self.resize = None if resize is None else dict(dict(ratio_range=None, keep_ratio=True), **resize)
        if self.resize is not None and ('size' in self.resize) == ('img_scale' in self.resize):
            raise ValueError('resize takes img_scale=(long, short) (mmseg / mmdet) or size=(h, w) (mmcls)')
        self.rrc = None if random_resized_crop is None else dict(RANDOM_RESIZED_CROP, **random_resized_crop)
        self.photometric = None if not photometric else dict(PHOTOMETRIC, **(photometric if isinstance(photometric, dict)
                                                                             else {}))
        self.erasing = None if random_erasing is None else dict(RANDOM_ERASING, **random_erasing)
        self.resample = RESAMPLE_PIL if resize_backend == 'pillow' else RESAMPLE_LINEAR
        if rand_augment is not None and rand_augment is not False and task != 'cls':
            raise ValueError("rand_augment is for task 'cls' only: boxes and label maps do not follow its warps")
        self.rand_augment = None if rand_augment is None or rand_augment is False else _ra_config(rand_augment)
        self._ra_wtab = None  # device copy of cubic_weight_table() (uploaded once)
        self.augmented = any(x is not None for x in (self.resize, self.rrc, self.photometric, self.erasing,
                                                     self.rand_augment))
        self.skipped = []  # transforms build_collate was told to skip
        self.labels = bool(labels)
        self._stage_done = None  # event after the last upload out of the staging buffer (augmented path)

    # ---- host-side random decisions (the draws of mmcv / mmseg / mmdet RandomFlip and mmseg RandomCrop) ----------
    def _crop_window(self, img, seg, rng):
        """mmseg RandomCrop.get_crop_bbox + the cat_max_ratio retry loop (up to 10 draws)."""
        return self._crop_window_hw(img.shape[0], img.shape[1], seg, rng)

    def _crop_window_hw(self, H, W, seg, rng):
        """The same on an (H, W) frame; `seg` = None, an (H, W) label map, or a function (x0, y0, w, h) -> label window."""
        ch, cw = self.crop_size

        def draw():
            my, mx = max(H - ch, 0), max(W - cw, 0)
            oy, ox = rng.randint(0, my + 1), rng.randint(0, mx + 1)
            return ox, oy, min(cw, W - ox), min(ch, H - oy)
        win = draw()
        if self.cat_max_ratio < 1.0 and seg is not None:
            for _ in range(10):
                x0, y0, w, h = win
                lab, cnt = np.unique(seg(x0, y0, w, h) if callable(seg) else seg[y0:y0 + h, x0:x0 + w], return_counts=True)
                # the reference counts on the label map AFTER LoadAnnotations: with reduce_zero_label the raw values 0
                # and 255 are both the ignore index there
                keep = ((lab != 0) & (lab != 255)) if self.reduce_zero_label else (lab != self.ignore_index)
                cnt = cnt[keep]
                if len(cnt) > 1 and cnt.max() / cnt.sum() < self.cat_max_ratio:
                    break
                win = draw()
        return win

    def _stage_bytes(self, arrays):
        total = sum(a.nbytes for a in arrays)
        if self._stage is None or self._stage.numel() < total:
            self._stage = torch.empty(max(total, 1 << 20), dtype=torch.uint8,
                                      pin_memory=self.device.type == 'cuda')
        offs, o = [], 0
        view = self._stage.numpy()
        for a in arrays:
            view[o:o + a.nbytes] = np.ascontiguousarray(a).reshape(-1)
            offs.append(o)
            o += a.nbytes
        return self._stage[:total].to(self.device, non_blocking=True), offs

    # ---- host-side draws of the optional stages -----------------------------------------------------------------------
    def _rrc_params(self, H, W, rng):
        """mmcls RandomResizedCrop.get_params -> (offset_h, offset_w, target_h, target_w)."""
        import math
        scale, ratio = self.rrc['scale'], self.rrc['ratio']
        area = H * W
        for _ in range(self.rrc['max_attempts']):
            target_area = rng.uniform(*scale) * area
            log_ratio = (math.log(ratio[0]), math.log(ratio[1]))
            aspect_ratio = math.exp(rng.uniform(*log_ratio))
            tw = int(round(math.sqrt(target_area * aspect_ratio)))
            th = int(round(math.sqrt(target_area / aspect_ratio)))
            if 0 < tw <= W and 0 < th <= H:
                return rng.randint(0, H - th + 1), rng.randint(0, W - tw + 1), th, tw
        in_ratio = float(W) / float(H)  # fallback: central crop
        if in_ratio < min(ratio):
            tw = W
            th = int(round(tw / min(ratio)))
        elif in_ratio > max(ratio):
            th = H
            tw = int(round(th * max(ratio)))
        else:
            tw, th = W, H
        return (H - th) // 2, (W - tw) // 2, th, tw

    def _resize_shape(self, H, W, rng):
        """mmseg / mmdet Resize (random_sample_ratio, then mmcv rescale_size) or mmcls Resize -> (new_w, new_h)."""
        r = self.resize
        if 'size' in r:
            return int(r['size'][1]), int(r['size'][0])
        scale = tuple(r['img_scale'])
        if r['ratio_range'] is not None:
            lo, hi = r['ratio_range']
            ratio = rng.random_sample() * (hi - lo) + lo
            scale = int(scale[0] * ratio), int(scale[1] * ratio)
        if r['keep_ratio']:
            return rescale_size(W, H, scale)[0]
        return int(scale[0]), int(scale[1])

    def _photometric_draws(self, rng):
        """mmseg PhotoMetricDistortion.__call__'s draws -> (flags, beta, contrast alpha, saturation alpha, hue delta)."""
        p = self.photometric
        flags, beta, ca, sa, hd = 0, 0.0, 1.0, 1.0, 0
        if rng.randint(2):
            flags |= PM_BRIGHT
            beta = rng.uniform(-p['brightness_delta'], p['brightness_delta'])
        mode = rng.randint(2)

        def contrast():
            if rng.randint(2):
                return PM_CONTRAST, rng.uniform(*p['contrast_range'])
            return 0, 1.0
        if mode == 1:
            f, ca = contrast()
            flags |= f | (PM_CONTRAST_FIRST if f else 0)
        if rng.randint(2):
            flags |= PM_SAT
            sa = rng.uniform(*p['saturation_range'])
        if rng.randint(2):
            flags |= PM_HUE
            hd = rng.randint(-p['hue_delta'], p['hue_delta'])
        if mode == 0:
            f, ca = contrast()
            flags |= f
        return flags, beta, ca, sa, hd

    def _erasing_draws(self, img_h, img_w, rng):
        """mmcls RandomErasing.__call__ / _fill_pixels -> (left, top, w, h, HWC uint8 patch) or None."""
        e = self.erasing
        if rng.rand() > e['erase_prob']:
            return None
        log_aspect_range = np.log(np.array(e['aspect_range'], dtype=np.float32))
        aspect_ratio = np.exp(rng.uniform(*log_aspect_range))
        area = img_h * img_w
        area *= rng.uniform(e['min_area_ratio'], e['max_area_ratio'])
        h = min(int(round(np.sqrt(area * aspect_ratio))), img_h)
        w = min(int(round(np.sqrt(area / aspect_ratio))), img_w)
        top = rng.randint(0, img_h - h) if img_h > h else 0
        left = rng.randint(0, img_w - w) if img_w > w else 0
        if e['mode'] == 'const':
            patch = np.empty((h, w, 3), dtype=np.uint8)
            patch[:, :] = np.array(e['fill_color'], dtype=np.uint8)
        elif e['fill_std'] is None:
            patch = rng.uniform(0, 256, (h, w, 3)).astype(np.uint8)
        else:
            patch = rng.normal(e['fill_color'], e['fill_std'], (h, w, 3))
            patch = np.clip(patch.astype(np.int32), 0, 255).astype(np.uint8)
        return left, top, w, h, patch

    def _ra_draws(self, w, h, rng, py_rng):
        """mmcls RandAugment.__call__ on a (h, w) frame -> (plan, chosen policies).  Python's generator: random.choices(policies,
        k=num_policies), then per chosen policy with a magnitude_key one gauss(magnitude_level, magnitude_std) when std > 0.
        NumPy's, per transform in order: rand() > prob -> unchanged; else, for the signed ones, rand() < random_negative_prob.
        A plan entry is (op code, magnitude or None, applied, forward warpAffine matrix or None)."""
        ra = self.rand_augment
        if ra['num_policies'] == 0:
            return [], []
        chosen = py_rng.choices(ra['policies'], k=ra['num_policies'])
        mags = []
        for p in chosen:
            if p.get('magnitude_key') is None:
                mags.append(p.get(_RA_KEY.get(p['type'], 'magnitude')))
                continue
            level = ra['magnitude_level']
            if ra['magnitude_std'] > 0:
                level = py_rng.gauss(ra['magnitude_level'], ra['magnitude_std'])
            level = min(ra['total_level'], max(0, level))
            lo, hi = p['magnitude_range']
            mags.append((level / ra['total_level']) * (hi - lo) + lo)
        plan = []
        for p, m in zip(chosen, mags):
            typ = p['type']
            applied = not (rng.rand() > p.get('prob', 0.5))
            if typ not in ('AutoContrast', 'Equalize', 'Invert') and m is None:
                raise ValueError(f'rand_augment: {typ} has neither a magnitude_key nor a fixed magnitude')
            if applied and typ in RA_SIGNED and rng.rand() < p.get('random_negative_prob', 0.5):
                m = -m
            plan.append((RA_OPS[typ], m, applied, _ra_matrix(p, m, w, h) if applied and typ in RA_WARPS else None))
        return plan, chosen

    def draw(self, img_shape, seg, rng, py_rng=None):
        """Every random decision of one sample, in the reference's order (geometry, crop, flip, photometric, RandAugment,
        erasing): a dict with the source rectangle `src` (x, y, w, h), the resized frame `rsz` (w, h), the window `win`
        (x0, y0, w, h) in that frame, `flip`, `pm` (photometric draws or None), `ra` (the RandAugment plan, `_ra_draws`; absent
        when the stage is off) and `erase` (or None).  `py_rng`: the Python-side generator of RandAugment (default `random`)."""
        H, W = img_shape[:2]
        if self.rrc is not None:
            oy, ox, th, tw = self._rrc_params(H, W, rng)
            size = self.rrc['size']
            sh, sw = (size, size) if isinstance(size, int) else size
            src, rsz = (ox, oy, tw, th), (sw, sh)
        elif self.resize is not None:
            src, rsz = (0, 0, W, H), self._resize_shape(H, W, rng)
        else:
            src, rsz = (0, 0, W, H), (W, H)
        if self.crop_size:
            lab = None
            if seg is not None and self.cat_max_ratio < 1.0:
                if rsz == (W, H):
                    lab = seg
                else:  # the retries look at the nearest-resized label map, as the reference's RandomCrop does
                    def lab(x0, y0, w, h):
                        ys = _axis_nearest(H, rsz[1], 0, y0, h)[:, 0]
                        xs = _axis_nearest(W, rsz[0], 0, x0, w)[:, 0]
                        return seg[ys[:, None], xs[None, :]]
            win = self._crop_window_hw(rsz[1], rsz[0], lab, rng)
        else:
            win = (0, 0, rsz[0], rsz[1])
        d = dict(src=src, rsz=rsz, win=win, flip=bool(rng.rand() < self.flip_prob), pm=None, erase=None)
        if self.photometric is not None:
            d['pm'] = self._photometric_draws(rng)
        if self.rand_augment is not None:
            d['ra'], d['ra_policies'] = self._ra_draws(win[2], win[3], rng, py_rng or random)
        if self.erasing is not None:
            d['erase'] = self._erasing_draws(win[3], win[2], rng)
        return d

    def _upload(self, arrays, extra=0):
        """One host-to-device copy of `arrays` (16-byte aligned) out of the pinned staging buffer -> (device bytes, offsets).
        The buffer is rewritten only after the previous copy out of it has completed.  `extra` > 0: that many workspace bytes
        follow the upload in the SAME device allocation (the RandAugment frames, reached by byte offsets from its start)."""
        offs = self._upload_offsets(arrays)
        total = max(_round_up(offs[-1] + arrays[-1].nbytes, 16), 16)
        if self._stage_done is not None:
            self._stage_done.synchronize()
        if self._stage is None or self._stage.numel() < total:
            self._stage = torch.empty(max(total, 1 << 20), dtype=torch.uint8, pin_memory=self.device.type == 'cuda')
        view = self._stage.numpy()
        for a, o in zip(arrays, offs):
            view[o:o + a.nbytes] = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
        if extra:
            buf = torch.empty(total + extra, dtype=torch.uint8, device=self.device)
            buf[:total].copy_(self._stage[:total], non_blocking=True)
        else:
            buf = self._stage[:total].to(self.device, non_blocking=True)
        if self.device.type == 'cuda':
            self._stage_done = torch.cuda.Event()
            self._stage_done.record()
        return buf, offs

    def _ra_meta_row(self, entry, p, w, h, warp_off):
        """One rscotr_randaug_u8 meta row (include/rscotr.h) of a plan entry."""
        op, m, applied, M = entry
        row = [0, w, h] + [0] * (RA_META - 3)
        if not applied:
            return row
        row[0] = op
        typ = p['type']
        if typ == 'Posterize':
            bits = int(math.ceil(m))
            if not 0 <= bits <= 8:
                raise ValueError(f'rand_augment: Posterize bits {bits} outside [0, 8]')
            row[3] = 8 - bits
        elif typ == 'Solarize':  # v < thr for an integer v <=> v < ceil(thr)
            row[3] = int(min(max(math.ceil(m), 0), 256))
        elif typ == 'SolarizeAdd':  # uint8(min(v + m, 255)) = min(v + floor(m), 255) for m >= 0
            if m < 0:
                raise ValueError(f'rand_augment: SolarizeAdd magnitude {m} is negative')
            row[3] = int(min(math.floor(m), 255))
        elif typ in ('ColorTransform', 'Contrast', 'Brightness', 'Sharpness'):  # addWeighted(img, f, other, 1 - f, 0)
            row[4], row[5] = _f32_bits(1 + m), _f32_bits(1 - (1 + m))
        elif typ in RA_WARPS:
            row[6], row[7] = warp_off, int(p['interpolation'] == 'bicubic')
            row[8:11] = p['pad_val']
        return row

    def _call_randaug(self, samples, rng, py_rng):
        """The cls batch with RandAugment: frames -> one `rscotr_randaug_u8` per slot -> `rscotr_img_aug_u8` over identity
        entries on the last frame (erasing, normalize, pad).  One upload; the frames and the statistics table follow it in the
        same device allocation."""
        B = len(samples)
        imgs = [s['img'] for s in samples]
        ds = []
        for img in imgs:
            assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 3, 'decoded HWC uint8 images expected'
            ds.append(self.draw(img.shape, None, rng, py_rng))
        Hf, Wf = max([d['win'][3] for d in ds], default=0), max([d['win'][2] for d in ds], default=0)
        if self.crop_size:
            Hout, Wout = self.crop_size
        else:
            Hout, Wout = Hf, Wf
            if self.size_divisor:
                Hout, Wout = _round_up(Hout, self.size_divisor), _round_up(Wout, self.size_divisor)
        K = self.rand_augment['num_policies']
        tabs, n_tab = [], 0

        def add(t):
            nonlocal n_tab
            tabs.append(t)
            n_tab += t.size
            return n_tab - t.size, t.shape[1] - 2
        geo = []
        for img, d in zip(imgs, ds):
            (sx, sy, sw, sh), (rw, rh), (x0, y0, cw, ch) = d['src'], d['rsz'], d['win']
            assert 0 <= x0 and 0 <= y0 and x0 + cw <= rw and y0 + ch <= rh and cw <= Wout and ch <= Hout
            mode = RESAMPLE_NEAREST if (sw, sh) == (rw, rh) else self.resample
            xt, kx = add(_AXIS[mode](sw, rw, sx, x0, cw))
            yt, ky = add(_AXIS[mode](sh, rh, sy, y0, ch))
            geo.append((mode, xt, kx, yt, ky))
        for t, dim in zip(tabs, [n for im in imgs for n in (im.shape[1], im.shape[0])]):
            assert (t[:, 0] >= 0).all() and (t[:, 0] + t[:, 1] <= dim).all() and (t[:, 1] >= 1).all()
        L = max(Hf, Wf, 1)
        ident, _ = add(_axis_nearest(L, L, 0, 0, L))  # the last step reads the final frame as is, both axes
        tables = np.concatenate([t.reshape(-1) for t in tabs])
        # the slots' meta rows and the warps' coordinate tables
        rmeta = np.zeros((max(K, 1), max(B, 1), RA_META), np.int32)
        warps, n_warp, need_stats = [np.zeros(4, np.int32)], 4, [False] * K
        for b, d in enumerate(ds):
            cw, ch = d['win'][2], d['win'][3]
            for k, (entry, p) in enumerate(zip(d['ra'], d['ra_policies'])):
                off = 0
                if entry[2] and entry[3] is not None:
                    t = _ra_warp_table(entry[3], cw, ch, p['interpolation'] == 'bicubic')
                    off, n_warp = n_warp, n_warp + t.size
                    warps.append(t)
                rmeta[k, b] = self._ra_meta_row(entry, p, cw, ch, off)
                need_stats[k] = need_stats[k] or (entry[2] and entry[0] in RA_STATS_OPS)
            for k in range(len(d['ra']), K):
                rmeta[k, b, 1:3] = cw, ch
        warp = np.concatenate(warps)
        patches = [d['erase'][4] for d in ds if d['erase'] is not None]
        params = np.zeros((max(B, 1), AUG_PARAMS), np.float32)
        nimg = len(imgs)
        # layout of the one upload: images | erasing patches | tables | params | meta | last step's meta | slot metas | warps;
        # then, not uploaded: frame 0 | frame 1 | statistics
        meta = np.zeros((max(B, 1), AUG_META), np.int64)
        fmeta = np.zeros((max(B, 1), AUG_META), np.int64)
        arrays = list(imgs) + patches + [tables, params, meta, fmeta, rmeta, warp]
        offs = self._upload_offsets(arrays)
        total = max(_round_up(offs[-1] + arrays[-1].nbytes, 16), 16)
        fbytes = _round_up(B * Hf * Wf * 3, 16)
        frame_off = [total, total + fbytes]
        stats_off = total + 2 * fbytes
        last = frame_off[K % 2]
        pi = 0
        for b, (img, d, g) in enumerate(zip(imgs, ds, geo)):
            (x0, y0, cw, ch), (mode, xt, kx, yt, ky) = d['win'], g
            meta[b, :12] = [offs[b], img.shape[0], img.shape[1], img.shape[1] * 3, cw, ch, int(d['flip']), xt, yt, kx, ky, mode]
            fmeta[b, :12] = [last + b * Hf * Wf * 3, Hf, Wf, Wf * 3, cw, ch, 0, ident, ident, 1, 1, RESAMPLE_NEAREST]
            if d['erase'] is not None:
                ex, ey, ew, eh, patch = d['erase']
                assert ex + ew <= cw and ey + eh <= ch
                fmeta[b, 14:19] = [ex, ey, ew, eh, offs[nimg + pi]]
                pi += 1
        buf, offs = self._upload(arrays, extra=2 * fbytes + _round_up(B * RA_STATS * 4, 16))
        ptr = buf.data_ptr()
        p_tab, p_prm, p_meta, p_fmeta, p_rmeta, p_warp = [ptr + o for o in offs[-6:]]
        if self._ra_wtab is None or self._ra_wtab.device != self.device:
            self._ra_wtab = torch.from_numpy(cubic_weight_table()).to(self.device)
        out = torch.empty((B, 3, Hout, Wout), dtype=torch.float32, device=self.device)
        mean_keep, mean_p = _host_floats(self.mean)
        std_keep, std_p = _host_floats(self.std)
        stream = ops._stream()
        lib.call('rscotr_img_frames_u8', ptr, p_meta, p_tab, ptr + frame_off[0], B, Hf, Wf, stream)
        for k in range(K):
            lib.call('rscotr_randaug_u8', ptr + frame_off[k % 2], ptr + frame_off[(k + 1) % 2],
                     p_rmeta + k * max(B, 1) * RA_META * 4, p_warp, self._ra_wtab.data_ptr(), ptr + stats_off,
                     int(need_stats[k]), B, Hf, Wf, stream)
        lib.call('rscotr_img_aug_u8', ptr, p_fmeta, p_tab, p_prm, out.data_ptr(), B, Hout, Wout, mean_p, std_p,
                 int(self.to_rgb), stream)
        metas = []
        for im, d in zip(imgs, ds):
            (sx, sy, sw, sh), (rw, rh), (x0, y0, cw, ch) = d['src'], d['rsz'], d['win']
            m = dict(ori_shape=im.shape, img_shape=(ch, cw, 3), pad_shape=(Hout, Wout, 3), flip=d['flip'],
                     flip_direction='horizontal' if d['flip'] else None, scale_factor=1.0,
                     img_norm_cfg=dict(mean=self.mean, std=self.std, to_rgb=self.to_rgb))
            if self.resize is not None or self.rrc is not None:
                m['scale_factor'] = np.array([rw / sw, rh / sh, rw / sw, rh / sh], dtype=np.float32)
                m['keep_ratio'] = bool(self.resize is not None and self.resize.get('keep_ratio') and 'size' not in self.resize)
            metas.append(m)
        for m, d in zip(metas, ds):
            m['rand_augment'] = d['ra']  # the plan that was applied (`_ra_draws`)
        return dict(img=out, img_metas=metas,
                    gt_label=torch.tensor([int(s['gt_label']) for s in samples], dtype=torch.int64, device=self.device))

    def _call_augmented(self, samples, rng):
        B = len(samples)
        imgs = [s['img'] for s in samples]
        with_labels = self.task == 'seg' and self.labels
        segs = [s.get('gt_semantic_seg') if self.labels else None for s in samples]
        ds = []
        for img, seg in zip(imgs, segs):
            assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 3, 'decoded HWC uint8 images expected'
            ds.append(self.draw(img.shape, seg, rng))
        if self.crop_size:
            Hout, Wout = self.crop_size
        else:
            Hout, Wout = max([d['win'][3] for d in ds], default=0), max([d['win'][2] for d in ds], default=0)
            if self.size_divisor:
                Hout, Wout = _round_up(Hout, self.size_divisor), _round_up(Wout, self.size_divisor)
        # per-axis tables (identity nearest entries where a sample is not resized: its window is read as is)
        tabs, tab_off, n_tab = [], [], 0

        def add(t):
            nonlocal n_tab
            tabs.append(t)
            n_tab += t.size
            return n_tab - t.size, t.shape[1] - 2
        geo = []
        for img, d in zip(imgs, ds):
            (sx, sy, sw, sh), (rw, rh), (x0, y0, cw, ch) = d['src'], d['rsz'], d['win']
            assert 0 <= x0 and 0 <= y0 and x0 + cw <= rw and y0 + ch <= rh and cw <= Wout and ch <= Hout
            mode = RESAMPLE_NEAREST if (sw, sh) == (rw, rh) else self.resample
            xt, kx = add(_AXIS[mode](sw, rw, sx, x0, cw))
            yt, ky = add(_AXIS[mode](sh, rh, sy, y0, ch))
            geo.append((mode, xt, kx, yt, ky))
        lgeo = []
        if with_labels:
            for seg, d in zip(segs, ds):
                (sx, sy, sw, sh), (rw, rh), (x0, y0, cw, ch) = d['src'], d['rsz'], d['win']
                assert seg is not None and seg.shape[:2] == imgs[len(lgeo)].shape[:2]
                xt, kx = add(_axis_nearest(sw, rw, sx, x0, cw))
                yt, ky = add(_axis_nearest(sh, rh, sy, y0, ch))
                lgeo.append((xt, kx, yt, ky))
        tables = np.concatenate([t.reshape(-1) for t in tabs]) if tabs else np.zeros(1, np.int32)
        # bounds of every source read (the kernel cannot check them)
        for t, dim in zip(tabs[:2 * B], [n for im in imgs for n in (im.shape[1], im.shape[0])]):
            assert (t[:, 0] >= 0).all() and (t[:, 0] + t[:, 1] <= dim).all() and (t[:, 1] >= 1).all()
        patches = [d['erase'][4] for d in ds if d['erase'] is not None]
        params = np.zeros((max(B, 1), AUG_PARAMS), np.float32)
        for b, d in enumerate(ds):
            if d['pm'] is not None:
                params[b, :3] = d['pm'][1:4]
        nimg = len(imgs)
        lsegs = [np.ascontiguousarray(sg) for sg in segs] if with_labels else []
        # layout of the one upload: images | label maps | erasing patches | tables | params | meta | label meta
        meta = np.zeros((max(B, 1), AUG_META), np.int64)
        lmeta = np.zeros((max(B, 1), AUG_META), np.int64)
        arrays = list(imgs) + lsegs + patches + [tables, params, meta, lmeta]
        offs = self._upload_offsets(arrays)
        pi = 0
        for b, (img, d, g) in enumerate(zip(imgs, ds, geo)):
            (x0, y0, cw, ch), (mode, xt, kx, yt, ky) = d['win'], g
            row = [offs[b], img.shape[0], img.shape[1], img.shape[1] * 3, cw, ch, int(d['flip']), xt, yt, kx, ky, mode,
                   0, 0, 0, 0, 0, 0, 0, 0]
            if d['pm'] is not None:
                row[12], row[13] = d['pm'][0], d['pm'][4]
            if d['erase'] is not None:
                ex, ey, ew, eh, patch = d['erase']
                assert ex + ew <= cw and ey + eh <= ch
                row[14:19] = [ex, ey, ew, eh, offs[nimg + len(lsegs) + pi]]
                pi += 1
            meta[b] = row
        for b, (seg, d, (xt, kx, yt, ky)) in enumerate(zip(lsegs, ds, lgeo)):
            x0, y0, cw, ch = d['win']
            lmeta[b, :12] = [offs[nimg + b], seg.shape[0], seg.shape[1], seg.shape[1], cw, ch, int(d['flip']), xt, yt, kx,
                             ky, RESAMPLE_NEAREST]
        buf, offs = self._upload(arrays)
        ptr = buf.data_ptr()
        p_tab, p_prm, p_meta, p_lmeta = [ptr + o for o in offs[-4:]]
        out = torch.empty((B, 3, Hout, Wout), dtype=torch.float32, device=self.device)
        mean_keep, mean_p = _host_floats(self.mean)
        std_keep, std_p = _host_floats(self.std)
        lib.call('rscotr_img_aug_u8', ptr, p_meta, p_tab, p_prm, out.data_ptr(), B, Hout, Wout, mean_p, std_p,
                 int(self.to_rgb), ops._stream())
        metas = []
        for im, d in zip(imgs, ds):
            (sx, sy, sw, sh), (rw, rh), (x0, y0, cw, ch) = d['src'], d['rsz'], d['win']
            m = dict(ori_shape=im.shape, img_shape=(ch, cw, 3), pad_shape=(Hout, Wout, 3), flip=d['flip'],
                     flip_direction='horizontal' if d['flip'] else None, scale_factor=1.0,
                     img_norm_cfg=dict(mean=self.mean, std=self.std, to_rgb=self.to_rgb))
            if self.resize is not None or self.rrc is not None:
                m['scale_factor'] = np.array([rw / sw, rh / sh, rw / sw, rh / sh], dtype=np.float32)
                m['keep_ratio'] = bool(self.resize is not None and self.resize.get('keep_ratio') and 'size' not in self.resize)
            metas.append(m)
        batch = dict(img=out, img_metas=metas)
        if self.task == 'cls':
            batch['gt_label'] = torch.tensor([int(s['gt_label']) for s in samples], dtype=torch.int64, device=self.device)
        elif self.task == 'det':
            boxes, labels, hboxes, hlabels = [], [], [], []
            for s, d, m in zip(samples, ds, metas):
                hb = np.asarray(s['gt_bboxes'], dtype=np.float32).reshape(-1, 4)
                if self.resize is not None or self.rrc is not None:
                    hb = scale_boxes(hb, m['scale_factor'], m['img_shape'])
                cw = d['win'][2]
                if d['flip']:
                    hb = np.stack([np.float32(cw) - hb[:, 2], hb[:, 1], np.float32(cw) - hb[:, 0], hb[:, 3]], -1)
                hl = np.asarray(s['gt_labels'], dtype=np.int64).reshape(-1)
                boxes.append(torch.from_numpy(np.ascontiguousarray(hb)).to(self.device))
                labels.append(torch.from_numpy(np.ascontiguousarray(hl)).to(self.device))
                hboxes.append(np.ascontiguousarray(hb))
                hlabels.append(np.ascontiguousarray(hl))
            batch['gt_bboxes'], batch['gt_labels'] = boxes, labels
            batch['gt_bboxes_host'], batch['gt_labels_host'] = hboxes, hlabels
        elif with_labels:
            lab = torch.empty((B, 1, Hout, Wout), dtype=torch.int64, device=self.device)
            lib.call('rscotr_seg_label_aug_u8', ptr, p_lmeta, p_tab, lab.data_ptr(), B, Hout, Wout,
                     int(self.reduce_zero_label), int(self.seg_pad_val), ops._stream())
            batch['gt_semantic_seg'] = lab
        return batch

    @staticmethod
    def _upload_offsets(arrays):
        offs, o = [], 0
        for a in arrays:
            offs.append(o)
            o = _round_up(o + a.nbytes, 16)
        return offs

    def __call__(self, samples, rng=None, py_rng=None):
        if self.device.type != 'cuda':  # (the launches below would hand host pointers to a kernel wherever a GPU is present)
            raise RuntimeError(f'DeviceCollate runs HIP kernels: it needs a GPU device, not {self.device}')
        rng = rng or np.random
        if self.rand_augment is not None:
            return self._call_randaug(samples, rng, py_rng or random)
        if self.augmented:
            return self._call_augmented(samples, rng)
        B = len(samples)
        imgs = [s['img'] for s in samples]
        segs = [s.get('gt_semantic_seg') if self.labels else None for s in samples]
        wins, flips = [], []
        for img, seg in zip(imgs, segs):
            assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 3, 'decoded HWC uint8 images expected'
            H, W = img.shape[:2]
            wins.append(self._crop_window(img, seg, rng) if self.crop_size else (0, 0, W, H))
            flips.append(bool(rng.rand() < self.flip_prob))
        if self.crop_size:
            Hout, Wout = self.crop_size
        else:
            Hout, Wout = max(w[3] for w in wins), max(w[2] for w in wins)
            if self.size_divisor:
                Hout, Wout = _round_up(Hout, self.size_divisor), _round_up(Wout, self.size_divisor)
        buf, offs = self._stage_bytes(imgs)
        meta = torch.tensor([[o, im.shape[0], im.shape[1], im.shape[1] * 3, w[0], w[1], w[2], w[3], int(f), 0]
                             for o, im, w, f in zip(offs, imgs, wins, flips)], dtype=torch.int64).to(self.device)
        out = torch.empty((B, 3, Hout, Wout), dtype=torch.float32, device=self.device)
        mean_keep, mean_p = _host_floats(self.mean)
        std_keep, std_p = _host_floats(self.std)
        lib.call('rscotr_img_prep_u8', buf.data_ptr(), meta.data_ptr(), out.data_ptr(), B, Hout, Wout, mean_p, std_p,
                 int(self.to_rgb), ops._stream())
        metas = [dict(ori_shape=im.shape, img_shape=(w[3], w[2], 3), pad_shape=(Hout, Wout, 3), flip=f,
                      flip_direction='horizontal' if f else None, scale_factor=1.0,
                      img_norm_cfg=dict(mean=self.mean, std=self.std, to_rgb=self.to_rgb))
                 for im, w, f in zip(imgs, wins, flips)]
        batch = dict(img=out, img_metas=metas)
        if self.task == 'cls':
            batch['gt_label'] = torch.tensor([int(s['gt_label']) for s in samples], dtype=torch.int64, device=self.device)
        elif self.task == 'det':
            boxes, labels, hboxes, hlabels = [], [], [], []
            for s, w, f in zip(samples, wins, flips):
                hb = np.asarray(s['gt_bboxes'], dtype=np.float32).reshape(-1, 4)
                if f:  # mmdet RandomFlip.bbox_flip, horizontal (on the host: the boxes are a few dozen floats)
                    hb = np.stack([np.float32(w[2]) - hb[:, 2], hb[:, 1], np.float32(w[2]) - hb[:, 0], hb[:, 3]], -1)
                hl = np.asarray(s['gt_labels'], dtype=np.int64).reshape(-1)
                boxes.append(torch.from_numpy(np.ascontiguousarray(hb)).to(self.device))
                labels.append(torch.from_numpy(np.ascontiguousarray(hl)).to(self.device))
                hboxes.append(np.ascontiguousarray(hb))
                hlabels.append(np.ascontiguousarray(hl))
            batch['gt_bboxes'], batch['gt_labels'] = boxes, labels
            batch['gt_bboxes_host'], batch['gt_labels_host'] = hboxes, hlabels  # (for the det head's packed batch layout)
        elif self.labels:
            lbuf, loffs = self._stage_bytes(segs)
            lmeta = meta.clone()
            lmeta[:, 0] = torch.tensor(loffs, dtype=torch.int64)
            lmeta[:, 3] = torch.tensor([s.shape[1] for s in segs], dtype=torch.int64)
            lab = torch.empty((B, 1, Hout, Wout), dtype=torch.int64, device=self.device)
            lib.call('rscotr_seg_label_prep_u8', lbuf.data_ptr(), lmeta.data_ptr(), lab.data_ptr(), B, Hout, Wout,
                     int(self.reduce_zero_label), int(self.seg_pad_val), ops._stream())
            batch['gt_semantic_seg'] = lab
        return batch


def collate_for(task, device, **kw):
    """The three dataset configs' settings (configs/_base_/{cls/resisc_swin_224,det/dior,seg/potsdam_IRRG_all}.py)."""
    if task == 'cls':
        return DeviceCollate('cls', device, flip_prob=0.5, **kw)
    if task == 'det':
        return DeviceCollate('det', device, flip_prob=0.5, size_divisor=32, **kw)
    return DeviceCollate('seg', device, flip_prob=0.5, crop_size=(512, 512), cat_max_ratio=0.75, reduce_zero_label=True,
                         seg_pad_val=5, **kw)


def scale_boxes(bboxes, scale_factor, img_shape):
    """mmdet Resize._resize_bboxes with bbox_clip_border=True: float32 boxes * scale_factor, clipped to img_shape."""
    b = np.asarray(bboxes, np.float32) * np.asarray(scale_factor, np.float32)
    b[:, 0::2] = np.clip(b[:, 0::2], 0, img_shape[1])
    b[:, 1::2] = np.clip(b[:, 1::2], 0, img_shape[0])
    return b


# the three dataset configs' augmentation settings (configs/_base_/cls/resisc_swin_224.py:10-35,43-48,
# configs/_base_/det/dior.py:13-18,24-33, configs/_base_/seg/potsdam_IRRG_all.py:10-18,24-31); RandAugment's are RAND_AUGMENT above,
# off by default (train_collate_for('cls', device, rand_augment=True) is the reference's whole cls recipe)
CLS_ERASING = dict(erase_prob=0.25, mode='rand', min_area_ratio=0.02, max_area_ratio=1 / 3,
                   fill_color=IMG_NORM['mean'][::-1], fill_std=IMG_NORM['std'][::-1])


def train_collate_for(task, device, **kw):
    """The training pipelines' collate with the resampling and colour stages on the device:
    cls RandomResizedCrop(224, bicubic, pillow) + RandomFlip + RandomErasing; det keep-ratio Resize((1333, 800)) + RandomFlip
    + Pad(32); seg Resize((512, 512), ratio_range=(0.5, 2.0)) + RandomCrop(512, cat_max_ratio=0.75) + RandomFlip +
    PhotoMetricDistortion + Pad(512, seg_pad_val=5).  Keyword arguments override these settings; `rand_augment=True` adds the
    reference's RandAugment (RAND_AUGMENT) to the cls pipeline."""
    if task == 'cls':
        cfg = dict(flip_prob=0.5, random_resized_crop=dict(size=224), resize_backend='pillow', random_erasing=CLS_ERASING)
    elif task == 'det':
        cfg = dict(flip_prob=0.5, size_divisor=32, resize=dict(img_scale=(1333, 800)))
    else:
        cfg = dict(flip_prob=0.5, crop_size=(512, 512), cat_max_ratio=0.75, reduce_zero_label=True, seg_pad_val=5,
                   resize=dict(img_scale=(512, 512), ratio_range=(0.5, 2.0)), photometric=True)
    return DeviceCollate(task, device, **dict(cfg, **kw))


def eval_collate_for(task, device, **kw):
    """The test pipelines' collate (no flip): cls Resize((224, 224), bicubic, pillow); det keep-ratio Resize((1333, 800)) +
    Pad(32); seg keep-ratio Resize((512, 512)) (val_pipeline: no Pad; a batch is padded to its largest image)."""
    if task == 'cls':
        cfg = dict(flip_prob=0.0, resize=dict(size=(224, 224)), resize_backend='pillow')
    elif task == 'det':
        cfg = dict(flip_prob=0.0, size_divisor=32, resize=dict(img_scale=(1333, 800)))
    else:
        cfg = dict(flip_prob=0.0, resize=dict(img_scale=(512, 512)))
    return DeviceCollate(task, device, **dict(cfg, **kw))


SEG_TTA_MAX_VIEWS = 16  # rscotr_seg_predict_tta_u8 takes its view table in the kernel arguments: at most 16 rows


def plan_tta_views(img_scale=None, img_ratios=None, flip=False, flip_direction='horizontal', img_hw=None):
    """The views of mmseg's MultiScaleFlipAug, in its order -> [(scale (w, h), flip, direction | None)].
    An `img_scale` tuple with `img_ratios` gives (int(W * r), int(H * r)) per ratio; `img_scale=None` with `img_ratios` the same
    from the image's own size `img_hw` = (h, w); a list of scales (or one tuple without ratios) is used as is.  Scales are the
    outermost loop, then flip in [False, True] when `flip`, then the directions (mmseg walks the directions for the unflipped
    view too, so several directions repeat it)."""
    ratios = None if img_ratios is None else (list(img_ratios) if isinstance(img_ratios, (list, tuple)) else [img_ratios])
    if img_scale is None:
        if not ratios:
            raise ValueError('MultiScaleFlipAug: img_scale=None needs img_ratios')
        if img_hw is None:
            raise ValueError('MultiScaleFlipAug(img_scale=None): the views depend on the image size (img_hw)')
        h, w = int(img_hw[0]), int(img_hw[1])
        scales = [(int(w * r), int(h * r)) for r in ratios]
    elif isinstance(img_scale, tuple) and ratios:
        assert len(img_scale) == 2
        scales = [(int(img_scale[0] * r), int(img_scale[1] * r)) for r in ratios]
    else:
        scales = [tuple(sc) for sc in img_scale] if isinstance(img_scale, list) else [tuple(img_scale)]
    directions = list(flip_direction) if isinstance(flip_direction, (list, tuple)) else [flip_direction]
    return [(sc, f, d if f else None) for sc in scales for f in ([False, True] if flip else [False]) for d in directions]


class SegTTACollate:
    """Test-time augmentation collate of the seg task: one DeviceCollate pass (device resize + normalise, forced flip) per view
    of a MultiScaleFlipAug -> dict(img=[V tensors], img_metas=[V lists]), what `MTL.forward_test` hands to `aug_test_seg`.
    `tta`: the MultiScaleFlipAug arguments of `plan_tta_views`; `resize`: the keyword arguments of its Resize other than the
    scale; every other keyword goes to the per-view DeviceCollate, which is built without the label stage (a test batch is
    `img` and `img_metas` only).  All images of a batch must have one shape (the views of
    a batch share their sizes and their ori_shape)."""

    def __init__(self, device, tta, resize=None, **kw):
        self.task, self.device = 'seg', torch.device(device)
        self.tta, self.resize_kw, self.kw = dict(tta), dict(resize or {}), dict(kw)
        self.rand_augment, self.skipped = None, []
        dirs = self.tta.get('flip_direction', 'horizontal')
        if self.tta.get('flip', False):
            for d in (dirs if isinstance(dirs, (list, tuple)) else [dirs]):
                if d != 'horizontal':
                    raise NotImplementedError(f"MultiScaleFlipAug(flip_direction={d!r}): the input kernels flip horizontally only")
        self.views = None if self.tta.get('img_scale') is None else self._plan(None)
        self._collates = {}

    def _plan(self, img_hw):
        views = plan_tta_views(img_hw=img_hw, **self.tta)
        if len(views) > SEG_TTA_MAX_VIEWS:
            raise ValueError(f'MultiScaleFlipAug plans {len(views)} views: rscotr_seg_predict_tta_u8 takes at most '
                             f'{SEG_TTA_MAX_VIEWS}')
        return views

    def _collate(self, scale, flip):
        c = self._collates.get((scale, flip))
        if c is None:
            c = self._collates[(scale, flip)] = DeviceCollate(
                'seg', self.device, **dict(self.kw, labels=False, flip_prob=1.0 if flip else 0.0,
                                           resize=dict(self.resize_kw, img_scale=scale)))
        return c

    def __call__(self, samples, rng=None, py_rng=None):
        shapes = {tuple(s['img'].shape) for s in samples}
        if len(shapes) != 1:
            raise ValueError(f'test-time augmentation takes batches of one image shape, got {sorted(shapes)}')
        views = self.views if self.views is not None else self._plan(next(iter(shapes))[:2])
        imgs, metas = [], []
        for scale, flip, _ in views:
            batch = self._collate(scale, flip)(samples, rng)
            imgs.append(batch['img'])
            metas.append(batch['img_metas'])
        return dict(img=imgs, img_metas=metas)


_PASSIVE = {'LoadImageFromFile', 'ImageToTensor', 'ToTensor', 'DefaultFormatBundle', 'Collect', 'Normalize'}


def build_collate(task, pipeline_cfg, device, unsupported='raise'):
    """Map an mm* pipeline (a list of transform dicts, as in the dataset configs) to a DeviceCollate.

    Understood: LoadImageFromFile, LoadAnnotations (reduce_zero_label), Resize (mmseg / mmdet img_scale + ratio_range +
    keep_ratio; mmcls size + backend + interpolation), RandomResizedCrop, RandomCrop, RandomFlip, PhotoMetricDistortion,
    RandomErasing, Normalize, Pad, ImageToTensor, ToTensor, DefaultFormatBundle, Collect, MultiScaleFlipAug (its single
    scale and its transforms; flip=False — for task 'seg' also flip=True, `img_ratios` and several scales, up to
    SEG_TTA_MAX_VIEWS views: the result is then a SegTTACollate) and RandAugment when `policies` is a non-empty list of the 13 implemented types
    (RA_OPS) whose warps ask for 'nearest' or 'bicubic'.  Anything else (a RandAugment with an empty list, another policy or
    another interpolation among them) raises NotImplementedError naming it, unless unsupported='skip': then it is left out and
    listed in `collate.skipped`, and the random stream no longer matches the reference's (the skipped transform's draws are
    not made)."""
    assert unsupported in ('raise', 'skip')
    kw, skipped, norm, tta = dict(flip_prob=0.0), [], None, None

    def visit(t, scale=None):
        nonlocal norm, tta
        t = dict(t)
        typ = t.pop('type')
        if typ in _PASSIVE:
            if typ == 'Normalize':
                norm = t
        elif typ == 'LoadAnnotations':
            kw['reduce_zero_label'] = bool(t.get('reduce_zero_label', False))
        elif typ == 'MultiScaleFlipAug':
            sc, ratios = t.get('img_scale'), t.get('img_ratios')
            rl = [] if ratios is None else (list(ratios) if isinstance(ratios, (list, tuple)) else [ratios])
            # (one ratio other than 1.0 is a one-view plan: the planner applies it, the single-view path below would not)
            several = len(rl) > 1 or any(r != 1.0 for r in rl) or (isinstance(sc, list) and len(sc) != 1)
            if task == 'seg' and (t.get('flip', False) or several):  # test-time augmentation: SegTTACollate plans the views
                tta = dict(img_scale=sc if sc is None or isinstance(sc, list) else tuple(sc), img_ratios=ratios,
                           flip=bool(t.get('flip', False)), flip_direction=t.get('flip_direction', 'horizontal'))
                sc = None
            else:
                if t.get('flip', False):
                    raise NotImplementedError('MultiScaleFlipAug(flip=True)')
                if isinstance(sc, list):
                    if len(sc) != 1:
                        raise NotImplementedError('MultiScaleFlipAug with several scales')
                    sc = sc[0]
            for u in t.get('transforms', []):
                visit(u, tuple(sc) if sc is not None else None)
        elif typ == 'Resize':
            if 'size' in t:  # mmcls
                size = t['size']
                kw['resize'] = dict(size=(size, size) if isinstance(size, int) else tuple(size))
            else:
                sc = t.get('img_scale', scale)
                if tta is not None:  # (the scale is the view's; the other Resize arguments are kept for every view)
                    if sc is not None or t.get('ratio_range') is not None:
                        raise NotImplementedError('Resize with its own img_scale / ratio_range inside a multi-view MultiScaleFlipAug')
                    kw['tta_resize'] = dict(keep_ratio=t.get('keep_ratio', True))
                    kw['resize_backend'] = _backend(t)
                    return
                if sc is None:  # MultiScaleFlipAug(img_scale=None, img_ratios=[1.0]): the image's own size
                    return
                if isinstance(sc, list):
                    if len(sc) != 1:
                        raise NotImplementedError('Resize with several img_scale values')
                    sc = sc[0]
                kw['resize'] = dict(img_scale=tuple(sc), ratio_range=t.get('ratio_range'), keep_ratio=t.get('keep_ratio', True))
            kw['resize_backend'] = _backend(t)
        elif typ == 'RandomResizedCrop':
            kw['random_resized_crop'] = {k: t[k] for k in ('size', 'scale', 'ratio', 'max_attempts') if k in t}
            kw['resize_backend'] = _backend(t)
        elif typ == 'RandomCrop':
            cs = t['crop_size']
            kw['crop_size'] = (cs, cs) if isinstance(cs, int) else tuple(cs)
            kw['cat_max_ratio'] = t.get('cat_max_ratio', 1.0)
            kw['ignore_index'] = t.get('ignore_index', 255)
        elif typ == 'RandomFlip' and tta is not None:
            pass  # (MultiScaleFlipAug sets the flip of every view)
        elif typ == 'RandomFlip':
            kw['flip_prob'] = t.get('flip_prob', t.get('flip_ratio', t.get('prob', 0.0))) or 0.0
        elif typ == 'PhotoMetricDistortion':
            kw['photometric'] = dict(PHOTOMETRIC, **t)
        elif typ == 'RandomErasing':
            kw['random_erasing'] = dict(t)
        elif typ == 'Pad':
            if t.get('size_divisor'):
                kw['size_divisor'] = t['size_divisor']
            if t.get('size') is not None and 'crop_size' not in kw:
                raise NotImplementedError('Pad(size=...) without RandomCrop')
            kw['seg_pad_val'] = t.get('seg_pad_val', 255)
        elif typ == 'RandAugment' and ra_unsupported(t) is None:
            kw['rand_augment'] = t
        elif unsupported == 'skip':
            skipped.append(typ)
        else:
            what = f'RandAugment: {ra_unsupported(t)}' if typ == 'RandAugment' else typ
            raise NotImplementedError(f'{what} is not implemented by the device collate (build_collate(..., '
                                      f"unsupported='skip') leaves it out)")
    for t in pipeline_cfg:
        visit(t)
    if tta is not None:
        kw.pop('flip_prob')
        col = SegTTACollate(device, tta, resize=kw.pop('tta_resize', None), img_norm_cfg=norm, **kw)
    else:
        col = DeviceCollate(task, device, img_norm_cfg=norm, **kw)
    col.skipped = skipped
    return col


def _backend(t):
    backend, interp = t.get('backend', 'cv2'), t.get('interpolation', 'bilinear')
    if (backend, interp) not in (('cv2', 'bilinear'), ('pillow', 'bicubic')):
        raise NotImplementedError(f'{t.get("type", "resize")}: backend={backend!r}, interpolation={interp!r} '
                                  "(cv2 bilinear and pillow bicubic are implemented)")
    return backend


# --------------------------------------------------------------------------------------------------------------
# on-disk layouts of the three datasets (decode with Pillow; BGR like mmcv.imread's default backend)
# --------------------------------------------------------------------------------------------------------------
def _imread_bgr(path):
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im.convert('RGB'))[..., ::-1].copy()


class FolderClsDataset:
    """mmcls CustomDataset without an annotation file: `data_prefix/<class name>/<image>`; classes = sorted folder
    names (data/NWPU-RESISC45/train, configs/_base_/cls/resisc_swin_224.py:55-58)."""
    task = 'cls'
    EXT = ('.jpg', '.jpeg', '.png', '.ppm', '.bmp', '.pgm', '.tif')

    def __init__(self, data_prefix):
        self.CLASSES = sorted(d for d in os.listdir(data_prefix) if os.path.isdir(os.path.join(data_prefix, d)))
        self.items = [(os.path.join(data_prefix, c, f), i) for i, c in enumerate(self.CLASSES)
                      for f in sorted(os.listdir(os.path.join(data_prefix, c))) if f.lower().endswith(self.EXT)]

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        path, label = self.items[i]
        return dict(img=_imread_bgr(path), gt_label=label, filename=path)

    def evaluate(self, results, metric='accuracy', metric_options=None, indices=None, logger=None, **kwargs):
        """mmcls BaseDataset.evaluate: `results` = per-sample score vectors in dataset order -> {'accuracy_top-1', 'accuracy_top-5'}
        in percent (metric_options: topk, thrs)."""
        from .metrics import accuracy
        metrics = [metric] if isinstance(metric, str) else list(metric)
        if set(metrics) - {'accuracy'}:
            raise ValueError(f'metric {set(metrics) - {"accuracy"}} is not supported (accuracy only)')
        opt = dict(topk=(1, 5)) if metric_options is None else dict(metric_options)
        labels = [self.items[i][1] for i in (range(len(self.items)) if indices is None else indices)]
        assert len(results) == len(labels), 'dataset testing results should be of the same length as gt_labels'
        topk = opt.get('topk', (1, 5))
        return accuracy(results, labels, topk=(topk,) if isinstance(topk, int) else tuple(topk), thrs=opt.get('thrs'))


class CocoDetDataset:
    """mmdet CocoDataset on DIOR's converted annotations (configs/_base_/det/dior.py:41-47): images without boxes and
    crowd / degenerate boxes are dropped as mmdet's `_filter_imgs` / `_parse_ann_info` do; labels index `classes`."""
    task = 'det'

    def __init__(self, ann_file, img_prefix, classes):
        with open(ann_file) as fh:
            coco = json.load(fh)
        self.CLASSES = tuple(classes)
        cat = {c['id']: self.CLASSES.index(c['name']) for c in coco['categories'] if c['name'] in self.CLASSES}
        anns = {}
        for a in coco['annotations']:
            anns.setdefault(a['image_id'], []).append(a)
        self.items = []
        for im in coco['images']:
            boxes, labels = [], []
            for a in anns.get(im['id'], []):
                x, y, w, h = a['bbox']
                if a.get('ignore', False) or a.get('iscrowd', False) or a['category_id'] not in cat:
                    continue
                if w < 1 or h < 1 or a.get('area', w * h) <= 0:
                    continue
                if max(0, min(x + w, im['width']) - max(x, 0)) * max(0, min(y + h, im['height']) - max(y, 0)) == 0:
                    continue
                boxes.append([x, y, x + w, y + h])
                labels.append(cat[a['category_id']])
            if boxes and min(im['width'], im['height']) >= 32:
                self.items.append((os.path.join(img_prefix, im['file_name']), np.asarray(boxes, np.float32),
                                   np.asarray(labels, np.int64)))

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        path, boxes, labels = self.items[i]
        return dict(img=_imread_bgr(path), gt_bboxes=boxes, gt_labels=labels, filename=path)

    def device_eval_ok(self):
        """Whether `ops.det_match` takes this dataset: no (image, class) holds more ground truths than its cap (counted once,
        on the host)."""
        ok = getattr(self, '_device_eval_ok', None)
        if ok is None:
            most = max((int(np.bincount(it[2]).max()) for it in self.items if len(it[2])), default=0)
            ok = self._device_eval_ok = most <= ops.DET_MATCH_MAX_GT
        return ok

    def pre_eval(self, dets, labels, indices, iou_thrs=None, max_det=100, device=None):
        """COCOeval.evaluateImg for one batch on the device.  dets: per image (K, 5) device tensors [x1, y1, x2, y2, score] in
        original-image coordinates and descending score order (or one (B, K, 5) tensor), labels: (K,) int64 each, `indices`:
        their positions in the dataset.  The ground truths of those images are uploaded and `ops.det_match` runs with COCO's
        area ranges, `iou_thrs` (default: COCO's ten) and `max_det`.  -> per image a tuple (dets, labels, flags (K, A) int32,
        npig (C, A) int32) of device tensors, the kind `evaluate` accumulates with `metrics.coco_accumulate`; nothing comes
        back to the host.  A dataset with more than `ops.DET_MATCH_MAX_GT` ground truths of one class in one image takes the
        host route instead: -> per image the per-class list of (k, 5) arrays of `mtl.bbox2result`."""
        from .metrics import coco_area_ranges, coco_iou_thrs
        indices = [int(i) for i in indices]
        assert len(dets) == len(labels) == len(indices), 'one index per image'
        C = len(self.CLASSES)
        if not indices:
            return []
        if not self.device_eval_ok():
            from .mtl import bbox2result
            return [bbox2result(d, l, C) for d, l in zip(dets, labels)]
        dets = dets if torch.is_tensor(dets) else torch.stack(list(dets))
        labels = labels if torch.is_tensor(labels) else torch.stack(list(labels))
        dev = torch.device(device) if device is not None else dets.device
        dets, labels = dets.to(dev, torch.float32), labels.to(dev, torch.int64)
        B, K = labels.shape
        thrs = coco_iou_thrs(iou_thrs)
        self._pre_eval_cfg = (tuple(float(t) for t in thrs), int(max_det))
        gb = [self.items[i][1].reshape(-1, 4) for i in indices]
        gl = [self.items[i][2].reshape(-1) for i in indices]
        off = np.concatenate([[0], np.cumsum([len(g) for g in gl])]).astype(np.int64)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        flags, npig = ops.det_match(dets, labels, torch.full((B,), K, dtype=torch.int32, device=dev),
                                    up(np.concatenate(gb).astype(np.float32)), up(np.concatenate(gl).astype(np.int64)), up(off),
                                    up(coco_area_ranges()), up(thrs), C, int(max_det))
        return [tuple(t) for t in zip(dets.unbind(0), labels.unbind(0), flags.unbind(0), npig.unbind(0))]

    def evaluate(self, results, metric='bbox', logger=None, jsonfile_prefix=None, classwise=False, proposal_nums=(100, 300, 1000),
                 iou_thrs=None, metric_items=None, **kwargs):
        """mmdet CocoDataset.evaluate(metric='bbox') -> bbox_mAP / _50 / _75 / _s / _m / _l (COCOeval semantics,
        rscotr_amd/metrics.py).  `results` (dataset order) are either per image a LIST (per class) of (k, 5) arrays in
        original-image coordinates, matched and accumulated on the host (`coco_bbox_map`), or per image a TUPLE (dets, labels,
        flags, npig) of the pre_eval test loop (`engine._test_det(on_device=True)`), matched on the device and only accumulated
        here (`coco_accumulate`): the kind of `results` decides the route, and both give the same dict.  The tuples must have
        been matched with this call's `iou_thrs` and `max_det = proposal_nums[0]`: that is the caller's contract.  The check below only catches the common slip (it
        compares with the last `pre_eval` of THIS object; tuples unpickled from another process are taken on trust)."""
        from .metrics import coco_accumulate, coco_bbox_map, coco_iou_thrs
        metrics = [metric] if isinstance(metric, str) else list(metric)
        if metrics != ['bbox']:
            raise KeyError(f'metric {metrics} is not supported (bbox only)')
        assert len(results) == len(self.items), 'one result per image'
        if len(results) and isinstance(results[0], tuple) and len(results[0]) == 4:
            cfg = getattr(self, '_pre_eval_cfg', None)
            if cfg is not None and cfg != (tuple(float(t) for t in coco_iou_thrs(iou_thrs)), int(proposal_nums[0])):
                raise ValueError(f'results were pre-evaluated with (iou_thrs, max_det) = {cfg}, evaluate() asks for '
                                 f'{(iou_thrs, proposal_nums[0])}')
            out = coco_accumulate(results, self.CLASSES, iou_thrs=iou_thrs, classwise=classwise)
        else:
            out = coco_bbox_map(results, [it[1] for it in self.items], [it[2] for it in self.items], self.CLASSES,
                                iou_thrs=iou_thrs, max_det=proposal_nums[0], classwise=classwise)
        if metric_items is not None:
            keep = {f'bbox_{m}' for m in metric_items}
            out = type(out)((k, v) for k, v in out.items() if k in keep or k == 'bbox_mAP_copypaste' or k.startswith('bbox_AP.'))
        return out


class TileSegDataset:
    """mmseg CustomDataset / PotsdamDataset: `img_dir/<name>.png` + `ann_dir/<name>.png` single-channel label tiles
    (configs/_base_/seg/potsdam_IRRG_all.py:52-62)."""
    task = 'seg'
    CLASSES = ('impervious_surface', 'building', 'low_vegetation', 'tree', 'car', 'clutter')

    def __init__(self, img_dir, ann_dir, img_suffix='.png', seg_map_suffix='.png', reduce_zero_label=True, ignore_index=255):
        names = sorted(f[:-len(img_suffix)] for f in os.listdir(img_dir) if f.endswith(img_suffix))
        self.items = [(os.path.join(img_dir, n + img_suffix), os.path.join(ann_dir, n + seg_map_suffix)) for n in names]
        self.reduce_zero_label, self.ignore_index = reduce_zero_label, ignore_index  # (mmseg PotsdamDataset: True, 255)

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        from PIL import Image
        ip, ap = self.items[i]
        with Image.open(ap) as im:
            seg = np.asarray(im).astype(np.uint8)
        return dict(img=_imread_bgr(ip), gt_semantic_seg=seg, filename=ip)

    def _label_map(self, i):
        from PIL import Image
        with Image.open(self.items[i][1]) as im:
            return np.asarray(im).astype(np.uint8)

    def pre_eval(self, preds, indices, device=None):
        """mmseg CustomDataset.pre_eval for one batch: `preds` = the label maps (uint8 device tensors, or NumPy maps) of the
        images `indices` -> int64 (len(preds), 4, C) on the device: area_intersect, area_union, area_pred_label, area_label
        per image (ops.seg_areas).  The raw label tiles are read and uploaded as uint8; nothing comes back to the host.
        These are mmseg's areas: a kept pixel whose prediction is >= C (a head with more channels than the dataset has
        classes) still counts in area_label, whereas the confusion matrix of the label-map route drops that pixel — see
        `evaluate`."""
        indices = [int(i) for i in indices]
        assert len(preds) == len(indices), 'one index per prediction'
        if device is None:
            device = preds[0].device if torch.is_tensor(preds[0]) and preds[0].is_cuda else 'cuda'
        dev = torch.device(device)

        def u8(p):
            if not torch.is_tensor(p):
                p = torch.from_numpy(np.ascontiguousarray(p))
            if p.dtype != torch.uint8:  # (host maps are int64: a label that does not fit a byte must not wrap into a class)
                if p.numel() and (int(p.min()) < 0 or int(p.max()) > 255):
                    raise ValueError('pre_eval takes label maps with values in 0 .. 255')
                p = p.to(torch.uint8)
            return p.to(dev)
        pred = torch.stack([u8(p) for p in preds])
        gt = torch.from_numpy(np.stack([self._label_map(i) for i in indices])).to(dev)
        return ops.seg_areas(pred, gt, len(self.CLASSES), ignore_index=self.ignore_index,
                             reduce_zero_label=self.reduce_zero_label)

    def evaluate(self, results, metric='mIoU', logger=None, gt_seg_maps=None, device=None, **kwargs):
        """mmseg CustomDataset.evaluate -> aAcc, mIoU / mAcc, mFscore / mPrecision / mRecall, mDice and the per-class values, as
        fractions.  `results` (dataset order) are either per-image label maps at the original size (arrays or tensors: the
        confusion matrix is accumulated on the device, rscotr_amd/metrics.py) or the per-image 4-tuples (area_intersect,
        area_union, area_pred_label, area_label) of the pre_eval test loop (`engine._test_seg(pre_eval=True)`), which are summed
        over the images and need no label map here.  The `pre_eval` / `classwise` keys of the reference's config are accepted:
        the kind of `results` decides the route, and per-class values are always returned.  The two routes agree exactly
        while every prediction is a class of the dataset (< C).  They differ for a pixel predicted >= C: mmseg's areas keep it
        in area_label (it lowers aAcc, Acc and Recall, as in the reference's pre_eval mode), the confusion matrix drops it
        from every count."""
        from .metrics import confusion_matrix, seg_metrics, seg_metrics_from_areas
        assert len(results) == len(self.items), 'one result per image'
        if len(results) and isinstance(results[0], (tuple, list)) and len(results[0]) == 4:
            total = sum(torch.stack([torch.as_tensor(a).reshape(-1).cpu().long() for a in r]) for r in results)
            return seg_metrics_from_areas(total[0], total[2], total[3], self.CLASSES, metrics=metric)

        def gts():
            if gt_seg_maps is not None:
                yield from gt_seg_maps
                return
            for i in range(len(self.items)):
                yield self._label_map(i)
        results = [r.cpu().numpy() if torch.is_tensor(r) else r for r in results]
        cm = confusion_matrix(results, gts(), len(self.CLASSES), ignore_index=self.ignore_index,
                              reduce_zero_label=self.reduce_zero_label, device=device)
        return seg_metrics(cm, self.CLASSES, metrics=metric)


class DeviceLoader:
    """Minimal batch loader over one of the datasets above: shuffled index batches, decoded on the host, everything
    else in `DeviceCollate`.  `len()` = batches per epoch; `.dataset.task` is what MultiDataLoader tags batches with."""

    def __init__(self, dataset, collate, batch_size, shuffle=True, drop_last=True, seed=0, test_mode=False):
        self.dataset, self.collate, self.batch_size = dataset, collate, batch_size
        self.shuffle, self.drop_last, self.rng = shuffle, drop_last, np.random.RandomState(seed)
        self.py_rng = random.Random(seed)  # RandAugment's second generator (mmcls draws its policies from `random`)
        # test_mode: dataset order, every sample, batches of {task, img, img_metas} only — what `engine.single_gpu_test` feeds
        # `model(return_loss=False, **data)` (the collate should be built with flip_prob = 0 and no crop)
        self.test_mode = test_mode
        if test_mode:
            self.shuffle, self.drop_last = False, False

    def __len__(self):
        n = len(self.dataset)
        return n // self.batch_size if self.drop_last else (n + self.batch_size - 1) // self.batch_size

    def __iter__(self):
        order = self.rng.permutation(len(self.dataset)) if self.shuffle else np.arange(len(self.dataset))
        for b in range(len(self)):
            idx = order[b * self.batch_size:(b + 1) * self.batch_size]
            if getattr(self.collate, 'rand_augment', None) is not None:
                batch = self.collate([self.dataset[int(i)] for i in idx], self.rng, self.py_rng)
            else:
                batch = self.collate([self.dataset[int(i)] for i in idx], self.rng)
            yield dict(task=self.dataset.task, img=batch['img'], img_metas=batch['img_metas']) if self.test_mode else batch
