"""The collate of the device input path: `DeviceCollate` (one host plan, then the launches of its route), the three dataset
configs' settings, and the test-time-augmentation collate of the seg task.

The host draws every random decision of a sample with the same NumPy calls and in the same order as the mm* transforms (`draw`), so
a seeded run makes the same decisions, and sends the raw bytes with the launches' rows in ONE copy out of a pinned staging buffer
(`_upload`).  The routes differ in their launches only:
  plain      every optional stage off: `rscotr_img_prep_u8` (+ `rscotr_seg_label_prep_u8`), crop / flip / normalize / pad;
  tables     `resize=`, `random_resized_crop=`, `photometric=`, `random_erasing=`: `rscotr_img_aug_u8` (+ `rscotr_seg_label_aug_u8`)
             over the per-axis tables of resample.py;
  RandAugment `rand_augment=` (cls): `rscotr_img_frames_u8` -> `rscotr_randaug_u8` per slot -> `rscotr_img_aug_u8` (randaug.py);
  chain      `auto_augment=` (det), when a sample of the batch drew a policy with two Resizes: `rscotr_img_aug_chain_u8`, both
             resamplings in one launch (autoaug.py); a batch of one-Resize samples is the table route's;
  rotate     `rotate=` (seg), when a sample of the batch drew a rotation: the table route's upload with the warp tables of
             rotate.py behind it, `rscotr_img_aug_rot_u8` (+ `rscotr_seg_label_rot_u8`), every sample in the one launch; a
             batch that drew none is the table route's.
RandomFlip's direction ('horizontal' | 'vertical' | 'diagonal') is the flip word of the meta rows on every route; in front of
the geometry (`auto_augment=`) it is mirrored into the x / y entries."""
import ctypes
import math
import random
from types import SimpleNamespace

import numpy as np
import torch

from .. import ops
from .._lib import lib
from .autoaug import aa_boxes, aa_config, aa_draw, aa_geometry, chain_tables, check_resize, resize_shape
from .randaug import RA_STATS, _ra_config, ra_draws, ra_slot_rows
from .resample import (FLIP_BITS, RESAMPLE_LINEAR, RESAMPLE_NEAREST, RESAMPLE_PIL, _axis_nearest, _AxisTables, _round_up,
                       cubic_weight_table, flip_boxes, scale_boxes)
from .rotate import rotate_config, rotate_draw, rotate_rows

IMG_NORM = dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], to_rgb=True)
META = 10  # include/rscotr.h: rscotr_img_prep_u8's meta row
AUG_META, AUG_PARAMS = 20, 4  # include/rscotr.h: rscotr_img_aug_u8's meta row and params row
PM_BRIGHT, PM_CONTRAST, PM_CONTRAST_FIRST, PM_SAT, PM_HUE = 1, 2, 4, 8, 16
PHOTOMETRIC = dict(brightness_delta=32, contrast_range=(0.5, 1.5), saturation_range=(0.5, 1.5), hue_delta=18)
RANDOM_ERASING = dict(erase_prob=0.5, min_area_ratio=0.02, max_area_ratio=0.4, aspect_range=(3 / 10, 10 / 3), mode='const',
                      fill_color=(128, 128, 128), fill_std=None)  # mmcls RandomErasing's defaults
RANDOM_RESIZED_CROP = dict(size=224, scale=(0.08, 1.0), ratio=(3. / 4., 4. / 3.), max_attempts=10)


def _host_floats(v):
    arr = (ctypes.c_float * 3)(*[float(x) for x in v])
    return arr, ctypes.cast(arr, ctypes.c_void_p)


def _flip_bits(d):
    """The flip word of a meta row (include/rscotr.h) for the draw `d`; a draw without a direction flips horizontally."""
    return FLIP_BITS[d.get('flip_direction', 'horizontal')] if d['flip'] else 0


def _flip_config(task, direction, prob):
    """RandomFlip's `direction` and probability, validated -> (direction | list of directions, prob | list of probs)."""
    known = ('horizontal', 'vertical', 'diagonal') if task == 'det' else ('horizontal', 'vertical')
    if isinstance(direction, (list, tuple)):
        if task != 'det':
            raise ValueError(f"flip_direction: task {task!r} takes one direction (mmseg / mmcls), not {direction!r}")
        direction = list(direction)
        if not direction or len(set(direction)) != len(direction):
            raise ValueError(f'flip_direction: {direction!r} must be a non-empty list of different directions')
        for dr in direction:
            if dr not in known:
                raise ValueError(f'flip_direction: unknown direction {dr!r} (one of {known})')
        if isinstance(prob, (list, tuple)):
            prob = [float(v) for v in prob]
            if len(prob) != len(direction):
                raise ValueError(f'flip_prob: {len(prob)} ratios for {len(direction)} directions')
        else:
            prob = float(prob or 0.0)
        ratios = prob if isinstance(prob, list) else [prob]
        if min(ratios) < 0 or sum(ratios) > 1:
            raise ValueError(f'flip_prob: {prob!r} must be non-negative and sum to at most 1')
        return direction, prob
    if direction not in known:
        raise ValueError(f'flip_direction: unknown direction {direction!r} for task {task!r} (one of {known})')
    if isinstance(prob, (list, tuple)):
        raise ValueError('flip_prob: a list of ratios needs a list of directions')
    return direction, prob


def _aug_row(off, shape, stride, d, geo, pm=None, erase=None, patch_off=0):
    """One rscotr_img_aug_u8 meta row (include/rscotr.h): a source of `shape` at byte offset `off`, the window and flip of the
    draw `d`, the tables `geo` (`_AxisTables.add_window`), the photometric draws and the erasing draws with their patch's offset."""
    (_, _, cw, ch), (mode, xt, kx, yt, ky) = d['win'], geo
    flip = 0 if d.get('flip_first', False) else _flip_bits(d)  # (a flip in front of the geometry is in the x / y entries)
    row = [off, shape[0], shape[1], stride, cw, ch, flip, xt, yt, kx, ky, mode] + [0] * (AUG_META - 12)
    if pm is not None:
        row[12], row[13] = pm[0], pm[4]
    if erase is not None:
        ex, ey, ew, eh, _ = erase
        assert ex + ew <= cw and ey + eh <= ch
        row[14:19] = [ex, ey, ew, eh, patch_off]
    return row


class DeviceCollate:
    """Batch builder for one task.  `__call__(samples, rng=None, py_rng=None)` takes the decoded samples of one batch
    (dicts with `img`: HWC uint8 BGR ndarray, and per task `gt_label` | `gt_bboxes`, `gt_labels` | `gt_semantic_seg`:
    HW uint8) and returns the batch dict `MTL.train_step` consumes, tensors on `device`.  There is no CPU fallback: without the
    HIP library it raises."""

    def __init__(self, task, device, img_norm_cfg=None, flip_prob=0.5, size_divisor=None, crop_size=None,
                 cat_max_ratio=1.0, reduce_zero_label=False, seg_pad_val=255, ignore_index=255, resize=None,
                 random_resized_crop=None, photometric=None, random_erasing=None, resize_backend='cv2',
                 rand_augment=None, labels=True, auto_augment=None, flip_direction='horizontal', rotate=None):
        """flip_direction: RandomFlip's direction, 'horizontal' | 'vertical' (mmseg, mmcls, mmdet) or, for task 'det', 'diagonal'
                or a list of directions; with a list mmdet draws one of them or none per sample, `flip_prob` a float shared
                equally among them or a list of ratios, one per direction, that sum to at most 1.
        Optional stages (None = off; any of them on routes the batch through `rscotr_img_aug_u8`):
        resize: mmseg / mmdet Resize, dict(img_scale=(long, short), ratio_range=None | (lo, hi), keep_ratio=True), or with
                img_scale=[(long, short), ...] and multiscale_mode='value' | 'range' (a scale drawn per sample), or
                mmcls Resize, dict(size=(h, w)) (a fixed size);
        random_resized_crop: mmcls RandomResizedCrop, dict(size, scale, ratio, max_attempts) (RANDOM_RESIZED_CROP);
        photometric: mmseg PhotoMetricDistortion, True or dict (PHOTOMETRIC);
        random_erasing: mmcls RandomErasing, dict (RANDOM_ERASING);
        resize_backend: 'cv2' (bilinear) | 'pillow' (bicubic), the image resample of resize / random_resized_crop;
        rand_augment: mmcls RandAugment (task 'cls' only), True (RAND_AUGMENT, the reference's settings) or dict(policies,
                num_policies, magnitude_level, total_level=30, magnitude_std=0., hparams); it routes the batch through
                `rscotr_img_frames_u8` -> `rscotr_randaug_u8` per slot -> `rscotr_img_aug_u8`;
        labels: False = a seg batch without `gt_semantic_seg` (test time: the label maps are neither staged nor resampled);
        auto_augment: mmdet AutoAugment (task 'det' only), dict(policies=[[Resize | RandomCrop dicts]]) (autoaug.py): RandomFlip
                is drawn and applied FIRST, then one policy per sample; a sample whose policy resizes twice sends the batch
                through `rscotr_img_aug_chain_u8`.  It is the whole geometry: no other optional stage goes with it;
        rotate: mmseg RandomRotate (task 'seg' only), dict(prob, degree, pad_val=0, seg_pad_val=255, center=None) (rotate.py):
                applied to the cropped, flipped window, in front of `photometric`; a batch in which a sample drew a rotation
                goes through `rscotr_img_aug_rot_u8` (+ `rscotr_seg_label_rot_u8`)."""
        assert task in ('cls', 'det', 'seg')
        self.task, self.device = task, torch.device(device)
        self.flip_direction, flip_prob = _flip_config(task, flip_direction, flip_prob)
        cfg = dict(IMG_NORM if img_norm_cfg is None else img_norm_cfg)
        self.mean, self.std, self.to_rgb = cfg['mean'], cfg['std'], bool(cfg.get('to_rgb', True))
        self.flip_prob, self.size_divisor, self.crop_size = flip_prob, size_divisor, crop_size
        self.cat_max_ratio, self.reduce_zero_label = cat_max_ratio, reduce_zero_label
        self.seg_pad_val, self.ignore_index = seg_pad_val, ignore_index
        if resize_backend not in ('cv2', 'pillow'):
            raise ValueError(f'resize_backend must be cv2 (bilinear) or pillow (bicubic), not {resize_backend!r}')
        if resize is not None and random_resized_crop is not None:
            raise ValueError('resize and random_resized_crop are exclusive')
        self.resize = None if resize is None else dict(dict(ratio_range=None, keep_ratio=True), **resize)
        if self.resize is not None and ('size' in self.resize) == ('img_scale' in self.resize):
            raise ValueError('resize takes img_scale=(long, short) (mmseg / mmdet) or size=(h, w) (mmcls)')
        if self.resize is not None and 'img_scale' in self.resize:
            check_resize(self.resize)
        self.rrc = None if random_resized_crop is None else dict(RANDOM_RESIZED_CROP, **random_resized_crop)
        self.photometric = None if not photometric else dict(PHOTOMETRIC, **(photometric if isinstance(photometric, dict)
                                                                             else {}))
        self.erasing = None if random_erasing is None else dict(RANDOM_ERASING, **random_erasing)
        self.resample = RESAMPLE_PIL if resize_backend == 'pillow' else RESAMPLE_LINEAR
        if rand_augment is not None and rand_augment is not False and task != 'cls':
            raise ValueError("rand_augment is for task 'cls' only: boxes and label maps do not follow its warps")
        self.rand_augment = None if rand_augment is None or rand_augment is False else _ra_config(rand_augment)
        self._ra_wtab = None  # device copy of cubic_weight_table() (uploaded once)
        self.auto_augment = None
        if auto_augment is not None:
            if task != 'det':
                raise ValueError("auto_augment is for task 'det' only")
            for name, v in (('Resize', self.resize), ('RandomResizedCrop', self.rrc), ('PhotoMetricDistortion', self.photometric),
                            ('RandomErasing', self.erasing), ('RandAugment', self.rand_augment), ('RandomCrop', crop_size)):
                if v is not None:
                    raise NotImplementedError(f'{name} together with AutoAugment')
            if resize_backend != 'cv2':
                raise NotImplementedError(f'AutoAugment with resize_backend={resize_backend!r}: a chain resamples cv2 bilinear')
            self.auto_augment = aa_config(auto_augment)
        if rotate is not None and task != 'seg':
            raise ValueError("rotate is for task 'seg' only: mmseg RandomRotate turns the image and its label map, not boxes")
        self.rotate = None if rotate is None else rotate_config(rotate)
        self.augmented = any(x is not None for x in (self.resize, self.rrc, self.photometric, self.erasing,
                                                     self.rand_augment, self.auto_augment, self.rotate))
        self.skipped = []  # transforms build_collate was told to skip
        self.labels = bool(labels)
        self._stage = None  # pinned byte staging buffer (grow-only)
        self._stage_done = None  # event after the last upload out of the staging buffer

    # ---- host-side random decisions (the draws of the mm* transforms, one method per transform) -----------------------
    def _crop_window_hw(self, H, W, seg, rng):
        """mmseg RandomCrop.get_crop_bbox + the cat_max_ratio retry loop (up to 10 draws) on an (H, W) frame; `seg` = None, an
        (H, W) label map, or a function (x0, y0, w, h) -> label window."""
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

    def _rrc_params(self, H, W, rng):
        """mmcls RandomResizedCrop.get_params -> (offset_h, offset_w, target_h, target_w)."""
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
        """mmseg / mmdet Resize (its scale draw, then mmcv rescale_size) or mmcls Resize -> (new_w, new_h)."""
        return resize_shape(self.resize, H, W, rng)

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

    def _flip_draw(self, rng):
        """RandomFlip's draw -> the direction applied, or None.  One direction: rand() < flip_prob.  A list (mmdet):
        np.random.choice(directions + [None], p=ratios + [1 - sum(ratios)]), drawn by index (one uniform, as rand())."""
        if not isinstance(self.flip_direction, list):
            return self.flip_direction if rng.rand() < self.flip_prob else None
        n = len(self.flip_direction)
        ratios = list(self.flip_prob) if isinstance(self.flip_prob, list) else [self.flip_prob / n] * n
        k = int(rng.choice(n + 1, p=ratios + [1 - sum(ratios)]))
        return self.flip_direction[k] if k < n else None

    def draw(self, img_shape, seg, rng, py_rng=None):
        """Every random decision of one sample, in the reference's order (geometry, crop, flip, rotate, photometric,
        RandAugment, erasing): a dict with the source rectangle `src` (x, y, w, h), the resized frame `rsz` (w, h), the window
        `win` (x0, y0, w, h) in that frame, `flip` and `flip_direction` (the direction applied, or None), `rotate` (the degree
        applied or None; absent when the stage is off), `pm` (photometric draws or None), `ra` (the RandAugment plan, `ra_draws`;
        absent when the stage is off) and `erase` (or None).  `py_rng`: the Python-side generator of RandAugment (default `random`).
        With every optional stage off these are the window and flip draws of the plain route.  With `auto_augment` the flip is
        drawn first and applies to the source (`flip_first`), `steps` is the drawn policy's walk (`aa_draw`) and `chain` is None or
        the second stage, dict(win1: the crop window of frame `rsz`, rsz2: the frame `win` lies in) (`aa_geometry`)."""
        H, W = img_shape[:2]
        if self.auto_augment is not None:  # mmdet RandomFlip, then AutoAugment: one policy's Resize / RandomCrop draws
            direction = self._flip_draw(rng)
            policy, steps = aa_draw(self.auto_augment, H, W, rng)
            return dict(aa_geometry(H, W, steps), flip=direction is not None, flip_direction=direction, flip_first=True,
                        policy=policy, steps=steps, pm=None, erase=None)
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
        direction = self._flip_draw(rng)
        d = dict(src=src, rsz=rsz, win=win, flip=direction is not None, flip_direction=direction, pm=None, erase=None)
        if self.rotate is not None:
            d['rotate'] = rotate_draw(self.rotate, rng)
        if self.photometric is not None:
            d['pm'] = self._photometric_draws(rng)
        if self.rand_augment is not None:
            d['ra'], d['ra_policies'] = ra_draws(self.rand_augment, win[2], win[3], rng, py_rng or random)
        if self.erasing is not None:
            d['erase'] = self._erasing_draws(win[3], win[2], rng)
        return d

    # ---- the host plan: draws, output size, img_metas and targets, once for every route ---------------------------------
    def _plan(self, samples, rng, py_rng):
        """-> the sources (`imgs`, `segs`: the label maps, or [] when the batch has no label stage), each sample's draws `ds`,
        the largest window (Hf, Wf), the output size (Hout, Wout) and the `batch` dict with its `img_metas`."""
        imgs = [s['img'] for s in samples]
        # (the label map steers the crop retries; the RandAugment route, cls only, never looked at one)
        segs = [s.get('gt_semantic_seg') if self.labels and self.rand_augment is None else None for s in samples]
        ds = []
        for img, seg in zip(imgs, segs):
            assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 3, 'decoded HWC uint8 images expected'
            ds.append(self.draw(img.shape, seg, rng, py_rng))
        Hf, Wf = max([d['win'][3] for d in ds], default=0), max([d['win'][2] for d in ds], default=0)
        if self.crop_size:
            Hout, Wout = self.crop_size
        else:
            Hout, Wout = Hf, Wf
            if self.size_divisor:
                Hout, Wout = _round_up(Hout, self.size_divisor), _round_up(Wout, self.size_divisor)
        resized = self.resize is not None or self.rrc is not None
        metas = []
        for im, d in zip(imgs, ds):
            (_, _, sw, sh), (rw, rh), (_, _, cw, ch) = d['src'], d['rsz'], d['win']
            m = dict(ori_shape=im.shape, img_shape=(ch, cw, 3), pad_shape=(Hout, Wout, 3), flip=d['flip'],
                     flip_direction=d['flip_direction'], scale_factor=1.0,
                     img_norm_cfg=dict(mean=self.mean, std=self.std, to_rgb=self.to_rgb))
            if self.rotate is not None:
                m['rotate_degree'] = d['rotate']  # the degree that was applied, or None
            if resized:
                m['scale_factor'] = np.array([rw / sw, rh / sh, rw / sw, rh / sh], dtype=np.float32)
                m['keep_ratio'] = bool(self.resize is not None and self.resize.get('keep_ratio') and 'size' not in self.resize)
            if d.get('scale_factor') is not None:  # AutoAugment: the LAST Resize of the drawn policy
                m['scale_factor'], m['keep_ratio'] = d['scale_factor'], d['keep_ratio']
            if self.rand_augment is not None:
                m['rand_augment'] = d['ra']  # the plan that was applied (`ra_draws`)
            metas.append(m)
        if self.task == 'seg' and self.labels:
            for seg, im in zip(segs, imgs):
                assert seg is not None and seg.shape[:2] == im.shape[:2]
            segs = [np.ascontiguousarray(sg) for sg in segs]
        else:
            segs = []
        return SimpleNamespace(imgs=imgs, segs=segs, ds=ds, Hf=Hf, Wf=Wf, Hout=Hout, Wout=Wout, resized=resized,
                               batch=dict(img=None, img_metas=metas))

    def _targets(self, samples, p):
        """The host-made targets of the batch.  Called after the launches: their small synchronous copies then run under the
        upload instead of in front of it."""
        batch = p.batch
        if self.task == 'cls':
            batch['gt_label'] = torch.tensor([int(s['gt_label']) for s in samples], dtype=torch.int64, device=self.device)
        elif self.task == 'det':
            boxes, labels, hboxes, hlabels = [], [], [], []
            for s, d, m in zip(samples, p.ds, batch['img_metas']):
                hb = np.asarray(s['gt_bboxes'], dtype=np.float32).reshape(-1, 4)
                hl = np.asarray(s['gt_labels'], dtype=np.int64).reshape(-1)
                if self.auto_augment is not None:  # flip, then the policy's scale / shift / clip / drop chain
                    hb, hl = aa_boxes(hb, hl, s['img'].shape[1], d['flip_direction'], d['steps'], H=s['img'].shape[0])
                if p.resized:
                    hb = scale_boxes(hb, m['scale_factor'], m['img_shape'])
                if d['flip'] and self.auto_augment is None:
                    # mmdet RandomFlip.bbox_flip on the window (on the host: the boxes are a few dozen floats)
                    hb = flip_boxes(hb, d['flip_direction'], d['win'][2], d['win'][3])
                boxes.append(torch.from_numpy(np.ascontiguousarray(hb)).to(self.device))
                labels.append(torch.from_numpy(np.ascontiguousarray(hl)).to(self.device))
                hboxes.append(np.ascontiguousarray(hb))
                hlabels.append(np.ascontiguousarray(hl))
            batch['gt_bboxes'], batch['gt_labels'] = boxes, labels
            batch['gt_bboxes_host'], batch['gt_labels_host'] = hboxes, hlabels  # (for the det head's packed batch layout)

    # ---- staging: the one host-to-device copy of a batch ------------------------------------------------------------------
    @staticmethod
    def _upload_offsets(arrays):
        offs, o = [], 0
        for a in arrays:
            offs.append(o)
            o = _round_up(o + a.nbytes, 16)
        return offs

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

    # ---- the launches -----------------------------------------------------------------------------------------------------------
    def _launch_img(self, entry, ptrs, p):
        """`entry`(*ptrs, out, B, Hout, Wout, mean, std, to_rgb, stream): the normalizing launch that ends every route."""
        out = torch.empty((len(p.imgs), 3, p.Hout, p.Wout), dtype=torch.float32, device=self.device)
        mean_keep, mean_p = _host_floats(self.mean)
        std_keep, std_p = _host_floats(self.std)
        lib.call(entry, *ptrs, out.data_ptr(), len(p.imgs), p.Hout, p.Wout, mean_p, std_p, int(self.to_rgb), ops._stream())
        p.batch['img'] = out

    def _launch_labels(self, entry, ptrs, p):
        """`entry`(*ptrs, out, B, Hout, Wout, reduce_zero_label, pad_val, stream), when the batch has a label stage."""
        if self.task == 'seg' and self.labels:
            lab = torch.empty((len(p.imgs), 1, p.Hout, p.Wout), dtype=torch.int64, device=self.device)
            lib.call(entry, *ptrs, lab.data_ptr(), len(p.imgs), p.Hout, p.Wout, int(self.reduce_zero_label),
                     int(self.seg_pad_val), ops._stream())
            p.batch['gt_semantic_seg'] = lab

    def _launch_plain(self, p):
        """crop / flip / normalize / pad.  Layout of the one upload: images | label maps | meta | label meta."""
        B = len(p.imgs)
        meta, lmeta = np.zeros((max(B, 1), META), np.int64), np.zeros((max(B, 1), META), np.int64)
        arrays = p.imgs + p.segs + [meta, lmeta]
        offs = self._upload_offsets(arrays)
        for b, (src, d) in enumerate(zip(p.imgs, p.ds)):
            meta[b] = [offs[b], src.shape[0], src.shape[1], src.shape[1] * 3, *d['win'], _flip_bits(d), 0]
        for b, (src, d) in enumerate(zip(p.segs, p.ds)):
            lmeta[b] = [offs[B + b], src.shape[0], src.shape[1], src.shape[1], *d['win'], _flip_bits(d), 0]
        buf, offs = self._upload(arrays)
        ptr = buf.data_ptr()
        self._launch_img('rscotr_img_prep_u8', (ptr, ptr + offs[-2]), p)
        self._launch_labels('rscotr_seg_label_prep_u8', (ptr, ptr + offs[-1]), p)

    def _launch_tables(self, p):
        """The same with a resized frame and the colour stages in front.  Layout of the one upload: images | label maps |
        erasing patches | tables | params | meta | label meta; on the rotate route (a sample of the batch drew a rotation)
        then | rot rows | label rot rows | warp tables, and the launches are the rotating pair."""
        B = len(p.imgs)
        tabs = _AxisTables()
        first = [_flip_bits(d) if d.get('flip_first', False) else 0 for d in p.ds]  # (a flip in front of the geometry)
        geo = [tabs.add_window(self.resample, d, p.Hout, p.Wout, mirror_w=a.shape[1] if f & 1 else None,
                               mirror_h=a.shape[0] if f & 2 else None)
               for a, d, f in zip(p.imgs, p.ds, first)]
        lgeo = [tabs.add_window(RESAMPLE_NEAREST, d, p.Hout, p.Wout) for _, d in zip(p.segs, p.ds)]
        tabs.check([a.shape for a in p.imgs])  # (the label tables are the nearest form of the same geometry on the same shapes)
        patches = [d['erase'][4] for d in p.ds if d['erase'] is not None]
        params = np.zeros((max(B, 1), AUG_PARAMS), np.float32)
        meta, lmeta = np.zeros((max(B, 1), AUG_META), np.int64), np.zeros((max(B, 1), AUG_META), np.int64)
        arrays = p.imgs + p.segs + patches + [tabs.flat(), params, meta, lmeta]
        rotated = self.rotate is not None and any(d['rotate'] is not None for d in p.ds)
        if rotated:
            rot, lrot, warp = rotate_rows(self.rotate, p.ds, labels=bool(p.segs))
            arrays += [rot, lrot, warp]
        offs = self._upload_offsets(arrays)
        patch_offs = iter(offs[B + len(p.segs):])
        for b, (src, d, g) in enumerate(zip(p.imgs, p.ds, geo)):
            if d['pm'] is not None:
                params[b, :3] = d['pm'][1:4]
            meta[b] = _aug_row(offs[b], src.shape, src.shape[1] * 3, d, g, d['pm'], d['erase'],
                               next(patch_offs) if d['erase'] is not None else 0)
        for b, (src, d, g) in enumerate(zip(p.segs, p.ds, lgeo)):
            lmeta[b] = _aug_row(offs[B + b], src.shape, src.shape[1], d, g)
        buf, offs = self._upload(arrays)
        ptr = buf.data_ptr()
        n = len(p.imgs) + len(p.segs) + len(patches)
        p_tab, p_prm, p_meta, p_lmeta = [ptr + o for o in offs[n:n + 4]]
        if rotated:
            p_rot, p_lrot, p_warp = [ptr + o for o in offs[n + 4:]]
            self._launch_img('rscotr_img_aug_rot_u8', (ptr, p_meta, p_tab, p_prm, p_rot, p_warp), p)
            self._launch_labels('rscotr_seg_label_rot_u8', (ptr, p_lmeta, p_tab, p_lrot, p_warp), p)
        else:
            self._launch_img('rscotr_img_aug_u8', (ptr, p_meta, p_tab, p_prm), p)
            self._launch_labels('rscotr_seg_label_aug_u8', (ptr, p_lmeta, p_tab), p)

    def _launch_chain(self, p):
        """The det batch of AutoAugment in which a sample resizes twice: `rscotr_img_aug_chain_u8`, every sample in the one
        launch (a one-Resize sample with identity stage-2 entries).  Layout of the one upload: images | tables | meta."""
        B = len(p.imgs)
        tabs = _AxisTables()
        meta = np.zeros((max(B, 1), AUG_META), np.int64)
        arrays = p.imgs + [None, meta]
        geo = [chain_tables(tabs, d, a.shape, p.Hout, p.Wout) for a, d in zip(p.imgs, p.ds)]
        arrays[-2] = tabs.flat()
        offs = self._upload_offsets(arrays)
        for b, (src, d, (mode, xt, kx, yt, ky, x2, y2, cw, ch)) in enumerate(zip(p.imgs, p.ds, geo)):
            meta[b, :16] = [offs[b], src.shape[0], src.shape[1], src.shape[1] * 3, cw, ch, 0, xt, yt, kx, ky, mode, x2, y2,
                            d['win'][2], d['win'][3]]
        buf, offs = self._upload(arrays)
        ptr = buf.data_ptr()
        self._launch_img('rscotr_img_aug_chain_u8', (ptr, ptr + offs[-1], ptr + offs[-2]), p)

    def _launch_randaug(self, p):
        """The cls batch with RandAugment: frames -> one `rscotr_randaug_u8` per slot -> `rscotr_img_aug_u8` over identity
        entries on the last frame (erasing, normalize, pad).  Layout of the one upload: images | erasing patches | tables |
        params | meta | last step's meta | slot metas | warps; then, not uploaded, in the same device allocation: frame 0 |
        frame 1 | statistics."""
        B, K, Hf, Wf = len(p.imgs), self.rand_augment['num_policies'], p.Hf, p.Wf
        tabs = _AxisTables()
        geo = [tabs.add_window(self.resample, d, p.Hout, p.Wout) for d in p.ds]
        tabs.check([a.shape for a in p.imgs])
        L = max(Hf, Wf, 1)
        ident = tabs.add(_axis_nearest(L, L, 0, 0, L))[0]  # the last step reads the final frame as is, both axes
        rmeta, warp, need_stats = ra_slot_rows(K, p.ds)
        patches = [d['erase'][4] for d in p.ds if d['erase'] is not None]
        params = np.zeros((max(B, 1), AUG_PARAMS), np.float32)
        meta, fmeta = np.zeros((max(B, 1), AUG_META), np.int64), np.zeros((max(B, 1), AUG_META), np.int64)
        arrays = p.imgs + patches + [tabs.flat(), params, meta, fmeta, rmeta, warp]
        offs = self._upload_offsets(arrays)
        total = max(_round_up(offs[-1] + arrays[-1].nbytes, 16), 16)
        fbytes = _round_up(B * Hf * Wf * 3, 16)
        frame_off = [total, total + fbytes]
        stats_off = total + 2 * fbytes
        patch_offs = iter(offs[B:])
        for b, (src, d, g) in enumerate(zip(p.imgs, p.ds, geo)):
            meta[b] = _aug_row(offs[b], src.shape, src.shape[1] * 3, d, g)
            still = dict(win=d['win'], flip=False)  # (the frame is flipped already)
            fmeta[b] = _aug_row(frame_off[K % 2] + b * Hf * Wf * 3, (Hf, Wf), Wf * 3, still, (RESAMPLE_NEAREST, ident, 1, ident, 1),
                                None, d['erase'], next(patch_offs) if d['erase'] is not None else 0)
        buf, offs = self._upload(arrays, extra=2 * fbytes + _round_up(B * RA_STATS * 4, 16))
        ptr = buf.data_ptr()
        p_tab, p_prm, p_meta, p_fmeta, p_rmeta, p_warp = [ptr + o for o in offs[-6:]]
        if self._ra_wtab is None or self._ra_wtab.device != self.device:
            self._ra_wtab = torch.from_numpy(cubic_weight_table()).to(self.device)
        stream = ops._stream()
        lib.call('rscotr_img_frames_u8', ptr, p_meta, p_tab, ptr + frame_off[0], B, Hf, Wf, stream)
        for k in range(K):
            lib.call('rscotr_randaug_u8', ptr + frame_off[k % 2], ptr + frame_off[(k + 1) % 2],
                     p_rmeta + k * rmeta[0].nbytes, p_warp, self._ra_wtab.data_ptr(), ptr + stats_off,
                     int(need_stats[k]), B, Hf, Wf, stream)
        self._launch_img('rscotr_img_aug_u8', (ptr, p_fmeta, p_tab, p_prm), p)

    def _run(self, samples, rng=None, py_rng=None):
        """`__call__` below its GPU guard: plan on the host, then one upload and the launches of the route, then the targets.
        Host code up to the library calls, so with `lib.call` stubbed it runs on a CPU device
        (tests/golden/make_collate_plan_golden.py)."""
        p = self._plan(samples, rng or np.random, py_rng or random)
        if self.rand_augment is not None:
            self._launch_randaug(p)
        elif any(d.get('chain') for d in p.ds):
            self._launch_chain(p)
        elif self.augmented:
            self._launch_tables(p)
        else:
            self._launch_plain(p)
        self._targets(samples, p)
        return p.batch

    def __call__(self, samples, rng=None, py_rng=None):
        if self.device.type != 'cuda':  # (the launches would hand host pointers to a kernel wherever a GPU is present)
            raise RuntimeError(f'DeviceCollate runs HIP kernels: it needs a GPU device, not {self.device}')
        return self._run(samples, rng, py_rng)


def collate_for(task, device, **kw):
    """The three dataset configs' settings (configs/_base_/{cls/resisc_swin_224,det/dior,seg/potsdam_IRRG_all}.py)."""
    if task == 'cls':
        return DeviceCollate('cls', device, flip_prob=0.5, **kw)
    if task == 'det':
        return DeviceCollate('det', device, flip_prob=0.5, size_divisor=32, **kw)
    return DeviceCollate('seg', device, flip_prob=0.5, crop_size=(512, 512), cat_max_ratio=0.75, reduce_zero_label=True,
                         seg_pad_val=5, **kw)


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
                    raise NotImplementedError(f"MultiScaleFlipAug(flip_direction={d!r}): the test-time views flip horizontally only")
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
        return self._run(samples, rng, py_rng, guard=True)

    def _run(self, samples, rng=None, py_rng=None, guard=False):
        """`guard`: run each view's DeviceCollate through its `__call__` (the GPU guard) rather than its `_run`."""
        shapes = {tuple(s['img'].shape) for s in samples}
        if len(shapes) != 1:
            raise ValueError(f'test-time augmentation takes batches of one image shape, got {sorted(shapes)}')
        views = self.views if self.views is not None else self._plan(next(iter(shapes))[:2])
        imgs, metas = [], []
        for scale, flip, _ in views:
            c = self._collate(scale, flip)
            batch = (c if guard else c._run)(samples, rng)
            imgs.append(batch['img'])
            metas.append(batch['img_metas'])
        return dict(img=imgs, img_metas=metas)
