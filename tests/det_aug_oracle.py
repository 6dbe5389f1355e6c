"""NumPy restatement (test infrastructure only) of the multi-scale AutoAugment det pipeline of the reference's DINO recipe
(configs/det/dino_4scale_r50_1x1_50e_dior.py:110-155), per sample and sequential: every transform really produces its uint8
image and its float32 boxes before the next one runs.  Written apart from the pipeline package (rscotr_amd/pipeline/autoaug.py)
on purpose, as tests/aug_oracle.py is: neither its tables nor its walk over frames are reused, only aug_oracle's cv2-bilinear
`resize_img` and oracle/pipeline.py's flip / normalize / pad.

mmdet 2.25.1 / mmcv 1.6.1 are not installed; what they do is restated here from memory (a discrepancy found later is a bug in this
restatement).  Draws come from numpy.random (`rng`), per sample, in this order:

RandomFlip(flip_ratio)   one rng.rand(); flip iff < flip_ratio (np.random.choice([dir, None], p=[r, 1 - r]) draws one uniform).
    Horizontal only.  It stands in FRONT of the geometry: the source array is flipped (mmcv.imflip) and the boxes with it,
    x1' = W - x2, x2' = W - x1 on the source width, before any resize.
AutoAugment(policies)    k = rng.randint(0, len(policies)) (np.random.choice(list) without p), then policy k's transforms in order.
Resize(img_scale, multiscale_mode, keep_ratio, override)
    a list of scales, mode 'value': scale = img_scale[rng.randint(len(img_scale))];
    mode 'range' (exactly two scales): long = rng.randint(min(longs), max(longs) + 1), then
        short = rng.randint(min(shorts), max(shorts) + 1), scale = (long, short);
    one scale with ratio_range: ratio = rng.random_sample() * (hi - lo) + lo, scale = int(s0 * ratio), int(s1 * ratio);
    one scale alone: no draw.
    keep_ratio: mmcv.rescale_size, sf = min(max(scale) / max(h, w), min(scale) / min(h, w)), new = int(w * sf + .5),
        int(h * sf + .5); else new = (scale[0], scale[1]).  The image is resized cv2 bilinear (aug_oracle.resize_bilinear).
    scale_factor = float32 [new_w / w, new_h / h, new_w / w, new_h / h], relative to the image ENTERING this Resize; boxes are
    multiplied by it, then x clipped to [0, new_w] and y to [0, new_h].  A second Resize in one chain must carry override=True
    (mmdet asserts that scale and scale_factor are not both set).  After the chain the meta's scale_factor and keep_ratio are the
    last Resize's.
RandomCrop(crop_size=(a, b), crop_type, allow_negative_crop=True, bbox_clip_border=True) on the current (h, w)
    crop size   'absolute': (min(a, h), min(b, w))
                'absolute_range' (a <= b): ch = rng.randint(min(h, a), min(h, b) + 1), then cw = rng.randint(min(w, a), min(w, b) + 1)
                'relative': (int(h * a + .5), int(w * b + .5))
                'relative_range': r = rng.rand(2); (int(h * (a + r[0] * (1 - a)) + .5), int(w * (b + r[1] * (1 - b)) + .5))
    offsets     oy = rng.randint(0, max(h - ch, 0) + 1), then ox = rng.randint(0, max(w - cw, 0) + 1)
    image       img[oy:oy + ch, ox:ox + cw]
    boxes       minus float32 (ox, oy, ox, oy); x clipped to [0, cw], y to [0, ch]; kept where x2 > x1 and y2 > y1; the labels
                are filtered alike.  With allow_negative_crop=True an image may end with no box: gt_bboxes (0, 4), gt_labels (0,).
Pad(size_divisor=1)      after Normalize, to the largest image of the batch: img_shape (the sample's own) != pad_shape."""
import numpy as np

from aug_oracle import collate_images, resize_img
from oracle import pipeline as OP


def resize_scale(t, rng):
    sc = t['img_scale']
    if isinstance(sc, list) and len(sc) == 1:
        sc = sc[0]
    if isinstance(sc, list):
        if t.get('multiscale_mode', 'range') == 'value':
            return tuple(sc[rng.randint(len(sc))])
        assert len(sc) == 2
        longs, shorts = [max(s) for s in sc], [min(s) for s in sc]
        long_edge = rng.randint(min(longs), max(longs) + 1)
        short_edge = rng.randint(min(shorts), max(shorts) + 1)
        return long_edge, short_edge
    if t.get('ratio_range') is not None:
        lo, hi = t['ratio_range']
        ratio = rng.random_sample() * (hi - lo) + lo
        return int(sc[0] * ratio), int(sc[1] * ratio)
    return tuple(sc)


def resize_wh(t, h, w, rng):
    scale = resize_scale(t, rng)
    if t.get('keep_ratio', True):
        sf = min(max(scale) / max(h, w), min(scale) / min(h, w))
        return int(w * float(sf) + 0.5), int(h * float(sf) + 0.5)
    return int(scale[0]), int(scale[1])


def crop_hw(t, h, w, rng):
    (a, b), ct = t['crop_size'], t.get('crop_type', 'absolute')
    if ct == 'absolute':
        return min(a, h), min(b, w)
    if ct == 'absolute_range':
        assert a <= b
        ch = rng.randint(min(h, a), min(h, b) + 1)
        cw = rng.randint(min(w, a), min(w, b) + 1)
        return ch, cw
    if ct == 'relative':
        return int(h * a + 0.5), int(w * b + 0.5)
    assert ct == 'relative_range'
    r = rng.rand(2)
    return int(h * (a + r[0] * (1 - a)) + 0.5), int(w * (b + r[1] * (1 - b)) + 0.5)


def resize_step(t, img, boxes, rng):
    h, w = img.shape[:2]
    nw, nh = resize_wh(t, h, w, rng)
    sf = np.array([nw / w, nh / h, nw / w, nh / h], dtype=np.float32)
    boxes = boxes * sf
    boxes[:, 0::2] = np.clip(boxes[:, 0::2], 0, nw)
    boxes[:, 1::2] = np.clip(boxes[:, 1::2], 0, nh)
    return resize_img(img, nw, nh, 'cv2'), boxes, sf


def crop_step(t, img, boxes, labels, rng):
    """-> image, boxes, labels, (ox, oy, cw, ch), boxes dropped, boxes clipped (kept but cut by the border)"""
    assert t.get('allow_negative_crop', False) and t.get('bbox_clip_border', True)
    h, w = img.shape[:2]
    ch, cw = crop_hw(t, h, w, rng)
    oy = rng.randint(0, max(h - ch, 0) + 1)
    ox = rng.randint(0, max(w - cw, 0) + 1)
    img = img[oy:oy + ch, ox:ox + cw]
    ch, cw = img.shape[:2]
    shifted = boxes - np.array([ox, oy, ox, oy], dtype=np.float32)
    boxes = shifted.copy()
    boxes[:, 0::2] = np.clip(boxes[:, 0::2], 0, cw)
    boxes[:, 1::2] = np.clip(boxes[:, 1::2], 0, ch)
    valid = (boxes[:, 2] > boxes[:, 0]) & (boxes[:, 3] > boxes[:, 1])
    clipped = int((valid & (boxes != shifted).any(1)).sum())
    return img, boxes[valid], labels[valid], (int(ox), int(oy), cw, ch), int((~valid).sum()), clipped


def det_autoaug_sample(img, boxes, labels, rng, policies, flip_ratio=0.5):
    """RandomFlip -> AutoAugment(policies) on one sample -> (uint8 image, float32 (n, 4) boxes, int64 (n,) labels, info);
    info: flip, policy, img_shape, scale_factor / keep_ratio (the last Resize's), sizes (every frame size met, (w, h)), windows
    (every crop), dropped / clipped (boxes a crop removed / cut)."""
    boxes = np.asarray(boxes, np.float32).reshape(-1, 4).copy()
    labels = np.asarray(labels, np.int64).reshape(-1).copy()
    flip = bool(rng.rand() < flip_ratio)
    if flip:
        boxes = OP.bbox_flip(boxes, img.shape[1])
        img = OP.imflip(img)
    k = int(rng.randint(0, len(policies)))
    info = dict(flip=flip, policy=k, scale_factor=None, keep_ratio=None, sizes=[], windows=[], dropped=0, clipped=0)
    resizes = 0
    for t in policies[k]:
        if t['type'] == 'Resize':
            resizes += 1
            assert resizes == 1 or t.get('override', False), 'scale and scale_factor cannot be both set'
            img, boxes, info['scale_factor'] = resize_step(t, img, boxes, rng)
            info['keep_ratio'] = bool(t.get('keep_ratio', True))
            info['sizes'].append((img.shape[1], img.shape[0]))
        else:
            assert t['type'] == 'RandomCrop'
            img, boxes, labels, win, dropped, clipped = crop_step(t, img, boxes, labels, rng)
            info['windows'].append(win)
            info['dropped'] += dropped
            info['clipped'] += clipped
    info['img_shape'] = tuple(img.shape)
    return np.ascontiguousarray(img), boxes.astype(np.float32).reshape(-1, 4), labels, info


def det_autoaug_batch(samples, rng, policies, flip_ratio=0.5):
    """The samples in order on the one stream, then Pad(size_divisor=1) to the largest image -> (images, boxes, labels, infos,
    (Hout, Wout))."""
    out = [det_autoaug_sample(s['img'], s['gt_bboxes'], s['gt_labels'], rng, policies, flip_ratio) for s in samples]
    hw = (max([o[0].shape[0] for o in out], default=0), max([o[0].shape[1] for o in out], default=0))
    return [o[0] for o in out], [o[1] for o in out], [o[2] for o in out], [o[3] for o in out], hw


def collate(ims, out_hw, mean, std, to_rgb=True):
    return collate_images(ims, out_hw, mean, std, to_rgb)
