"""NumPy restatement (test infrastructure only) of the orientation transforms of the device input path: RandomFlip's directions
(mmcv imflip, mmdet's direction draw and bbox_flip) and mmseg RandomRotate (rscotr_img_aug_rot_u8 / rscotr_seg_label_rot_u8).
Written apart from the pipeline package on purpose: its own matrix, its own inverse, its own fixed point, so a host-side table
bug shows up as a mismatch.  Resize / crop / photometric are tests/aug_oracle.py's, the nearest warp is compared with
tests/randaug_oracle.py's.

mmseg 0.28 / mmdet 2.25 / mmcv / cv2 are not installed.  Everything below is restated from upstream AS REMEMBERED, so parity with
mm* / cv2 is by reading and UNPINNED, the same status as the warps of tests/randaug_oracle.py; a real cv2 may differ by 1 LSB
(its SIMD bilinear remap, rounding ties).

mmcv.imflip(img, direction): 'horizontal' np.flip(img, 1), 'vertical' np.flip(img, 0), 'diagonal' np.flip(img, (0, 1)).
RandomFlip, mmseg / mmcls (one direction): flip = np.random.rand() < prob.
RandomFlip, mmdet: np.random.choice(direction_list + [None], p=ratios + [1 - sum(ratios)]); a float flip_ratio is shared equally
    among the directions.  choice with p draws ONE uniform u and returns index searchsorted(cumsum(p), u, side='right').  With one
    direction that is `u < ratio`, the draw the collate and tests/aug_oracle.py have always made.
mmdet bbox_flip(bboxes, img_shape, direction): horizontal x1' = w - x2, x2' = w - x1; vertical y1' = h - y2, y2' = h - y1; diagonal
    both.

mmseg RandomRotate(prob, degree, pad_val=0, seg_pad_val=255, center=None, auto_bound=False).__call__:
    rotate = True if np.random.rand() < prob else False
    degree = np.random.uniform(min(*degree), max(*degree))              # (a number d is (-d, d)); always drawn
    if rotate: img = mmcv.imrotate(img, angle=degree, border_value=pad_val, center=center, auto_bound=auto_bound)
               seg = mmcv.imrotate(seg, angle=degree, border_value=seg_pad_val, ..., interpolation='nearest')
mmcv.imrotate: M = cv2.getRotationMatrix2D(center or ((w - 1) * 0.5, (h - 1) * 0.5), -angle, 1);
    cv2.warpAffine(img, M, (w, h), flags=INTER_LINEAR | INTER_NEAREST, borderValue=border_value): positive angles turn clockwise.
    getRotationMatrix2D(c, a, 1): al = cos(a * pi / 180), be = sin(a * pi / 180),
    [[al, be, (1 - al) * cx - be * cy], [-be, al, be * cx + (1 - al) * cy]].
cv2.warpAffine without WARP_INVERSE_MAP inverts M in float64 (the formulas of tests/randaug_oracle.py's docstring), then in fixed
point, AB_SCALE = 1024: adelta[x] = rint(M0 * x * 1024), bdelta[x] = rint(M3 * x * 1024), X0 = rint((M1 * y + M2) * 1024) +
round_delta, Y0 likewise with M4, M5.
    nearest   round_delta = 512, sx = (X0 + adelta[x]) >> 10.
    bilinear  round_delta = 16, X = (X0 + adelta[x]) >> 5, sx = X >> 5, ax = X & 31 (INTER_BITS = 5); taps sy .. sy + 1 by
              sx .. sx + 1 with the weights (1 - ay | ay) * (1 - ax | ax) at a / 32, times 32768: the exact integers
              (32 - ay | ay) * (32 - ax | ax) * 32, which sum to 32768 (no correction); out = (sum w * p + 2^14) >> 15.  At
              ax = ay = 0 cv2 stores the one weight as a saturated 32767, which returns the pixel itself as 32768 does.
    A tap outside the image reads borderValue (BGR for an image)."""
import math

import numpy as np

import aug_oracle as AO
import det_aug_oracle as DO
import randaug_oracle as RO

FLIP_AXES = {'horizontal': 1, 'vertical': 0, 'diagonal': (0, 1)}


# ---- flips ---------------------------------------------------------------------------------------------------------------------
def imflip(img, direction):
    return img if direction is None else np.flip(img, FLIP_AXES[direction])


def flip_draw(rng, direction, ratio):
    """-> the direction applied, or None (see the docstring); `direction` a name or, mmdet, a list of names."""
    if not isinstance(direction, list):
        return direction if rng.rand() < ratio else None
    ratios = list(ratio) if isinstance(ratio, list) else [ratio / len(direction)] * len(direction)
    u = rng.random_sample()
    k = int(np.searchsorted(np.cumsum(ratios + [1 - sum(ratios)]), u, side='right'))
    return (direction + [None])[k]


def bbox_flip(bboxes, img_shape, direction):
    b = np.asarray(bboxes, np.float32).reshape(-1, 4)
    out = b.copy()
    h, w = np.float32(img_shape[0]), np.float32(img_shape[1])
    if direction in ('horizontal', 'diagonal'):
        out[:, 0], out[:, 2] = w - b[:, 2], w - b[:, 0]
    if direction in ('vertical', 'diagonal'):
        out[:, 1], out[:, 3] = h - b[:, 3], h - b[:, 1]
    return out


# ---- the warp ------------------------------------------------------------------------------------------------------------------
def rotation_matrix(angle, w, h, center=None):
    """mmcv.imrotate's cv2.getRotationMatrix2D(center, -angle, 1) (2 x 3, forward)."""
    cx, cy = ((w - 1) * 0.5, (h - 1) * 0.5) if center is None else center
    a = math.radians(-angle)
    al, be = math.cos(a), math.sin(a)
    return np.array([[al, be, (1 - al) * cx - be * cy], [-be, al, be * cx + (1 - al) * cy]], np.float64)


def warp_affine(img, M, interpolation='bilinear', pad_val=(0, 0, 0)):
    """cv2.warpAffine(img, M (2 x 3, forward), (w, h), flags=interpolation, borderValue=pad_val) for an HWC or HW uint8 array;
    'bilinear' | 'nearest'."""
    assert interpolation in ('bilinear', 'nearest')
    h, w = img.shape[:2]
    A = np.array(M, np.float64)
    D = A[0, 0] * A[1, 1] - A[0, 1] * A[1, 0]
    D = 1.0 / D if D != 0 else 0.0
    i00, i01, i10, i11 = A[1, 1] * D, -A[0, 1] * D, -A[1, 0] * D, A[0, 0] * D
    b0 = -i00 * A[0, 2] - i01 * A[1, 2]
    b1 = -i10 * A[0, 2] - i11 * A[1, 2]
    rd = 16 if interpolation == 'bilinear' else 512
    out = np.zeros_like(img)
    pad = np.broadcast_to(np.asarray(pad_val, np.int64), img.shape[2:])
    src = img.astype(np.int64)

    def tap(sy, sx):
        return src[sy, sx] if 0 <= sx < w and 0 <= sy < h else pad
    for y in range(h):
        X0 = int(np.rint((i01 * y + b0) * 1024)) + rd
        Y0 = int(np.rint((i11 * y + b1) * 1024)) + rd
        for x in range(w):
            X, Y = X0 + int(np.rint(i00 * x * 1024)), Y0 + int(np.rint(i10 * x * 1024))
            if interpolation == 'nearest':
                out[y, x] = tap(Y >> 10, X >> 10)
                continue
            X, Y = X >> 5, Y >> 5
            sx, sy, ax, ay = X >> 5, Y >> 5, X & 31, Y & 31
            acc = ((32 - ay) * (32 - ax) * 32 * tap(sy, sx) + (32 - ay) * ax * 32 * tap(sy, sx + 1)
                   + ay * (32 - ax) * 32 * tap(sy + 1, sx) + ay * ax * 32 * tap(sy + 1, sx + 1))
            out[y, x] = (acc + (1 << 14)) >> 15
    return out


def rotate(img, angle, interpolation='bilinear', pad_val=(0, 0, 0), center=None):
    """mmcv.imrotate(img, angle, center=center, border_value=pad_val, interpolation=interpolation, auto_bound=False)."""
    h, w = img.shape[:2]
    return warp_affine(img, rotation_matrix(angle, w, h, center), interpolation, pad_val)


def rotate_draw(rng, prob, degree):
    """RandomRotate's two draws -> the degree to apply, or None."""
    lo, hi = (-degree, degree) if isinstance(degree, (int, float)) else degree
    do = bool(rng.rand() < prob)
    deg = rng.uniform(min(lo, hi), max(lo, hi))
    return float(deg) if do else None


# ---- the pipelines, per sample ------------------------------------------------------------------------------------------------
def seg_sample_oriented(img, lab, rng, img_scale=None, ratio_range=None, crop=None, cat_max_ratio=1.0, flip_prob=0.5,
                        direction='horizontal', rotate_cfg=None, photo=False, reduce_zero=True):
    """mmseg LoadAnnotations(reduce_zero_label) -> Resize -> RandomCrop -> RandomFlip(direction) -> RandomRotate ->
    PhotoMetricDistortion with the draws in that order -> (uint8 image, int64 label window AFTER the reduction, info).
    img_scale=None: no Resize; crop=None: no RandomCrop; rotate_cfg: dict(prob, degree, pad_val, seg_pad_val, center) or None."""
    H, W = img.shape[:2]
    im, lb = img, lab
    if img_scale is not None:
        scale = img_scale
        if ratio_range is not None:
            ratio = rng.random_sample() * (ratio_range[1] - ratio_range[0]) + ratio_range[0]
            scale = int(img_scale[0] * ratio), int(img_scale[1] * ratio)
        nw, nh = AO.rescale_wh(W, H, scale)
        im, lb = AO.resize_img(img, nw, nh, 'cv2'), AO.resize_nearest(lab, nw, nh)
    if crop is not None:
        x0, y0, w, h = AO._crop_seg(im.shape[0], im.shape[1], lb, rng, crop, cat_max_ratio, reduce_zero)
        im, lb = im[y0:y0 + h, x0:x0 + w], lb[y0:y0 + h, x0:x0 + w]
    lb = lb.astype(np.int64)
    if reduce_zero:  # (at load time in mmseg; it commutes with the resampling, the crop and the flip)
        lb = np.where(lb == 0, 255, lb - 1)
        lb = np.where(lb == 254, 255, lb)
    d = flip_draw(rng, direction, flip_prob)
    im, lb = imflip(im, d), imflip(lb, d)
    info = dict(flip=d is not None, flip_direction=d, img_shape=im.shape)
    if rotate_cfg is not None:
        deg = rotate_draw(rng, rotate_cfg['prob'], rotate_cfg['degree'])
        info['rotate_degree'] = deg
        if deg is not None:
            pv = rotate_cfg.get('pad_val', 0)
            im = rotate(np.ascontiguousarray(im), deg, 'bilinear', (pv,) * 3 if isinstance(pv, (int, float)) else pv,
                        rotate_cfg.get('center'))
            lb = rotate(np.ascontiguousarray(lb).astype(np.uint8), deg, 'nearest', rotate_cfg.get('seg_pad_val', 255),
                        rotate_cfg.get('center')).astype(np.int64)
    if photo:
        im = AO.photometric(im, rng)
    return np.ascontiguousarray(im), np.ascontiguousarray(lb), info


def det_sample_oriented(img, boxes, rng, img_scale=None, flip_ratio=0.5, direction='horizontal'):
    """mmdet Resize(keep_ratio) -> RandomFlip(direction); boxes scaled, clipped, flipped.  img_scale=None: no Resize."""
    H, W = img.shape[:2]
    b = np.asarray(boxes, np.float32).reshape(-1, 4)
    im = img
    if img_scale is not None:
        nw, nh = AO.rescale_wh(W, H, img_scale)
        im = AO.resize_img(img, nw, nh, 'cv2')
        b = AO.boxes_rescale(b, AO.scale_factor(W, H, nw, nh), (nh, nw))
    d = flip_draw(rng, direction, flip_ratio)
    if d is not None:
        b = bbox_flip(b, im.shape, d)
    return np.ascontiguousarray(imflip(im, d)), b, dict(flip=d is not None, flip_direction=d, img_shape=im.shape)


def det_autoaug_sample_oriented(img, boxes, labels, rng, policies, flip_ratio=0.5, direction='horizontal'):
    """mmdet RandomFlip(direction) in FRONT of AutoAugment(policies): the source and its boxes are flipped, then the policy's
    transforms run one after the other (tests/det_aug_oracle.py's steps)."""
    boxes = np.asarray(boxes, np.float32).reshape(-1, 4).copy()
    labels = np.asarray(labels, np.int64).reshape(-1).copy()
    d = flip_draw(rng, direction, flip_ratio)
    if d is not None:
        boxes = bbox_flip(boxes, img.shape, d)
    img = imflip(img, d)
    k = int(rng.randint(0, len(policies)))
    for t in policies[k]:
        if t['type'] == 'Resize':
            img, boxes, _ = DO.resize_step(t, img, boxes, rng)
        else:
            img, boxes, labels = DO.crop_step(t, img, boxes, labels, rng)[:3]
    return np.ascontiguousarray(img), boxes.astype(np.float32).reshape(-1, 4), labels, dict(flip=d is not None, flip_direction=d,
                                                                                             policy=k)


def cls_randaug_sample_oriented(img, rng, py_rng, cfg, size, flip_prob=0.5, direction='horizontal', backend='pillow'):
    """mmcls RandomResizedCrop -> RandomFlip(direction) -> RandAugment (tests/randaug_oracle.py's)."""
    H, W = img.shape[:2]
    oy, ox, th, tw = AO.rrc_params(H, W, rng)
    img = AO.resize_img(img[oy:oy + th, ox:ox + tw], size, size, backend)
    d = flip_draw(rng, direction, flip_prob)
    img = RO.rand_augment(np.ascontiguousarray(imflip(img, d)), cfg, rng, py_rng)
    return img, dict(flip=d is not None, flip_direction=d)
