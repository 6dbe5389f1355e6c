"""Multi-scale Resize and mmdet's AutoAugment over Resize / RandomCrop policies (the DETR augmentation of the reference's DINO
recipe) on the device input path: the host draws of the two transforms, the box chain, and the tables of the chain launch.

A sample's geometry is a walk over frames: the (flipped) source, then one frame per Resize; a RandomCrop narrows the window of
the frame it meets.  At most two Resizes are carried: flip -> crop -> resize -> crop -> resize -> crop.  With one Resize the sample
is the table route's (`rscotr_img_aug_u8`); with two, `rscotr_img_aug_chain_u8` runs both resamplings in one launch: stage-1
entries describe the crop window of frame 1 from the raw source, stage-2 entries (4 words: first window coordinate, taps <= 2,
two 11-bit weights) describe the final window from that crop.  RandomFlip stands in FRONT of the geometry here, so truth is
"flip the array, then resize": the flip is mirrored into the source indices of the stage-1 x entries (`mirror_x`), not taken at
the output index, which would be "resize, then flip" and differs in the rounded weights."""
import numpy as np

from .resample import (_AXIS, FLIP_BITS, RESAMPLE_LINEAR, RESAMPLE_NEAREST, _axis_linear, _table, flip_boxes, mirror_x, rescale_size,
                       scale_boxes)

CROP_TYPES = ('relative_range', 'relative', 'absolute', 'absolute_range')  # mmdet RandomCrop


# ---- Resize (mmseg 0.28 / mmdet 2.25: the same code) -----------------------------------------------------------------------------
def check_resize(r, where='Resize'):
    """Settings of an mmseg / mmdet Resize, `img_scale` a (long, short) pair or a list of them -> the same dict, validated."""
    sc = r['img_scale']
    if isinstance(sc, list):
        mode = r.get('multiscale_mode', 'range')
        if mode not in ('value', 'range'):
            raise ValueError(f'{where}: multiscale_mode must be value or range, not {mode!r}')
        if r.get('ratio_range') is not None and len(sc) != 1:
            raise ValueError(f'{where}: ratio_range takes one img_scale, not {len(sc)}')
        if mode == 'range' and len(sc) > 1 and len(sc) != 2:
            raise ValueError(f"{where}: multiscale_mode='range' takes exactly two scales, not {len(sc)}")
        if not sc or not all(len(s) == 2 for s in sc):
            raise ValueError(f'{where}: img_scale must be (long, short) pairs')
    elif sc is None or len(sc) != 2:
        raise ValueError(f'{where}: img_scale must be a (long, short) pair or a list of them')
    return r


def resize_shape(r, H, W, rng):
    """Resize._random_scale (ratio_range: random_sample_ratio; a list: random_select for 'value', random_sample for 'range'),
    then mmcv rescale_size when keep_ratio, or mmcls Resize's fixed `size` -> (new_w, new_h)."""
    if 'size' in r:
        return int(r['size'][1]), int(r['size'][0])
    scale = r['img_scale']
    if isinstance(scale, list):
        if len(scale) == 1:
            scale = scale[0]
        elif r.get('multiscale_mode', 'range') == 'value':
            scale = scale[rng.randint(len(scale))]
        else:
            longs, shorts = [max(s) for s in scale], [min(s) for s in scale]
            long_edge = rng.randint(min(longs), max(longs) + 1)
            scale = (long_edge, rng.randint(min(shorts), max(shorts) + 1))
    scale = tuple(scale)
    if r.get('ratio_range') is not None:
        lo, hi = r['ratio_range']
        ratio = rng.random_sample() * (hi - lo) + lo
        scale = int(scale[0] * ratio), int(scale[1] * ratio)
    if r.get('keep_ratio', True):
        return rescale_size(W, H, scale)[0]
    return int(scale[0]), int(scale[1])


# ---- AutoAugment ----------------------------------------------------------------------------------------------------------------
def aa_config(cfg):
    """mmdet AutoAugment(policies) -> dict(policies=[[step]]), every step a validated Resize or RandomCrop dict."""
    policies = cfg['policies'] if isinstance(cfg, dict) else cfg
    if not policies or not all(isinstance(p, (list, tuple)) for p in policies):
        raise ValueError('AutoAugment: policies must be a non-empty list of transform lists')
    out = []
    for k, pol in enumerate(policies):
        where, steps, resizes = f'AutoAugment policy {k}', [], 0
        for t in pol:
            t = dict(t)
            typ = t.pop('type')
            if typ == 'Resize':
                resizes += 1
                if (t.get('backend', 'cv2'), t.get('interpolation', 'bilinear')) != ('cv2', 'bilinear'):
                    raise NotImplementedError(f"{where}: Resize(backend={t.get('backend', 'cv2')!r}, interpolation="
                                              f"{t.get('interpolation', 'bilinear')!r}): a chain resamples cv2 bilinear only")
                if not t.get('bbox_clip_border', True):
                    raise NotImplementedError(f'{where}: Resize(bbox_clip_border=False)')
                if resizes > 1 and not t.get('override', False):
                    raise ValueError(f'{where}: Resize number {resizes} needs override=True (mmdet asserts that scale and '
                                     'scale_factor are not both set)')
                if resizes > 2:
                    raise NotImplementedError(f'{where}: more than two Resize steps')
                sc = t.get('img_scale')
                sc = [tuple(s) for s in sc] if isinstance(sc, list) else (None if sc is None else tuple(sc))
                r = dict(type='Resize', img_scale=sc, ratio_range=t.get('ratio_range'), keep_ratio=t.get('keep_ratio', True))
                if isinstance(sc, list):
                    r['multiscale_mode'] = t.get('multiscale_mode', 'range')
                steps.append(check_resize(r, f'{where}: Resize'))
            elif typ == 'RandomCrop':
                ct, cs = t.get('crop_type', 'absolute'), t['crop_size']
                if ct not in CROP_TYPES:
                    raise ValueError(f'{where}: RandomCrop(crop_type={ct!r})')
                if not t.get('allow_negative_crop', False):
                    raise NotImplementedError(f'{where}: RandomCrop(allow_negative_crop=False) makes the dataset draw another '
                                              'sample when no box survives; the collate cannot')
                if not t.get('bbox_clip_border', True):
                    raise NotImplementedError(f'{where}: RandomCrop(bbox_clip_border=False)')
                a, b = cs
                if ct.startswith('relative'):
                    ok = 0 < a <= 1 and 0 < b <= 1
                else:
                    ok = isinstance(a, int) and isinstance(b, int) and a > 0 and b > 0 and (ct == 'absolute' or a <= b)
                if not ok:
                    raise ValueError(f'{where}: RandomCrop(crop_type={ct!r}, crop_size={cs!r})')
                steps.append(dict(type='RandomCrop', crop_type=ct, crop_size=(a, b)))
            else:
                raise NotImplementedError(f'{where}: {typ} (a policy holds Resize and RandomCrop only)')
        out.append(steps)
    return dict(policies=out)


def crop_shape(c, h, w, rng):
    """mmdet RandomCrop._get_crop_size on an (h, w) frame -> (crop h, crop w)."""
    (a, b), ct = c['crop_size'], c['crop_type']
    if ct == 'absolute':
        return min(a, h), min(b, w)
    if ct == 'absolute_range':  # (a, b) = (least, most), both axes
        ch = rng.randint(min(h, a), min(h, b) + 1)
        return ch, rng.randint(min(w, a), min(w, b) + 1)
    if ct == 'relative':
        return int(h * a + 0.5), int(w * b + 0.5)
    r = rng.rand(2)
    return int(h * (a + r[0] * (1 - a)) + 0.5), int(w * (b + r[1] * (1 - b)) + 0.5)


def aa_draw(cfg, H, W, rng):
    """AutoAugment.__call__ on an (H, W) image: the policy (np.random.choice of the list = one randint), then its transforms'
    draws in order -> (policy index, steps); a step is ('resize', (w, h) in, (w, h) out, keep_ratio) or
    ('crop', (x0, y0, w, h)) in the frame it meets."""
    k = int(rng.randint(0, len(cfg['policies'])))
    h, w, steps = H, W, []
    for t in cfg['policies'][k]:
        if t['type'] == 'Resize':
            nw, nh = resize_shape(t, h, w, rng)
            steps.append(('resize', (w, h), (nw, nh), bool(t['keep_ratio'])))
            h, w = nh, nw
        else:
            ch, cw = crop_shape(t, h, w, rng)
            ch, cw = min(ch, h), min(cw, w)
            oy = int(rng.randint(0, max(h - ch, 0) + 1))
            ox = int(rng.randint(0, max(w - cw, 0) + 1))
            steps.append(('crop', (ox, oy, cw, ch)))
            h, w = ch, cw
    return k, steps


def step_scale_factor(step):
    (w, h), (nw, nh) = step[1], step[2]
    return np.array([nw / w, nh / h, nw / w, nh / h], dtype=np.float32)


def aa_geometry(H, W, steps):
    """The walk of `steps` over the frames -> dict(src: the rectangle of the (flipped) source that is resampled, rsz: frame 1,
    chain: None | dict(win1: the crop window of frame 1, rsz2: frame 2), win: the final window in the last frame,
    scale_factor / keep_ratio: the last Resize's, None when the policy has none)."""
    frames, win, sf, keep = [], (0, 0, W, H), None, None  # frames: [(window of the frame before, size)]
    for s in steps:
        if s[0] == 'resize':
            assert s[1] == (win[2], win[3])
            frames.append((win, s[2]))
            win, sf, keep = (0, 0, *s[2]), step_scale_factor(s), s[3]
        else:
            x, y, cw, ch = s[1]
            assert 0 <= x and 0 <= y and x + cw <= win[2] and y + ch <= win[3]
            win = (win[0] + x, win[1] + y, cw, ch)
    assert len(frames) <= 2
    g = dict(scale_factor=sf, keep_ratio=keep, chain=None, win=win)
    if not frames:
        g.update(src=win, rsz=(win[2], win[3]), win=(0, 0, win[2], win[3]))
    else:
        g.update(src=frames[0][0], rsz=frames[0][1])
        if len(frames) == 2:
            g['chain'] = dict(win1=frames[1][0], rsz2=frames[1][1])
    return g


def aa_boxes(boxes, labels, W, flip, steps, H=None):
    """The box half of the same walk (mmdet 2.25, bbox_clip_border=True): RandomFlip.bbox_flip on the source size, Resize's
    scale + clip, RandomCrop's shift + clip + `x2 > x1 and y2 > y1` filter (labels alike) -> (float32 (n, 4), int64 (n,)).
    `flip`: a direction ('horizontal' | 'vertical' | 'diagonal'; the last two need the source height `H`), None / False, or
    True = 'horizontal'."""
    b = np.asarray(boxes, np.float32).reshape(-1, 4)
    l = np.asarray(labels, np.int64).reshape(-1)
    if flip:
        b = flip_boxes(b, 'horizontal' if flip is True else flip, W, H)
    for s in steps:
        if s[0] == 'resize':
            b = scale_boxes(b, step_scale_factor(s), (s[2][1], s[2][0]))
        else:
            x, y, cw, ch = s[1]
            b = b - np.array([x, y, x, y], dtype=np.float32)
            b[:, 0::2] = np.clip(b[:, 0::2], 0, cw)
            b[:, 1::2] = np.clip(b[:, 1::2], 0, ch)
            keep = (b[:, 2] > b[:, 0]) & (b[:, 3] > b[:, 1])
            b, l = b[keep], l[keep]
    return np.ascontiguousarray(b, np.float32), np.ascontiguousarray(l)


# ---- tables -----------------------------------------------------------------------------------------------------------------------
def _stage2_axis(n_in, n_out, o0, count):
    """Output coordinates o0 .. o0 + count - 1 of an axis of frame 2 (n_out) over the crop window of frame 1 (n_in): 4-word
    entries; sizes that agree read the window as is (one tap of weight 2048: (2048 * 2048 * p + 2^21) >> 22 = p)."""
    if n_in == n_out:
        w = np.zeros((count, 2), np.int32)
        w[:, 0] = 2048
        return _table(np.arange(o0, o0 + count, dtype=np.int64), np.ones(count, np.int64), w)
    return _axis_linear(n_in, n_out, 0, o0, count)


def chain_tables(tabs, d, img_shape, Hout, Wout):
    """The four tables of one sample of the chain launch, added to `tabs` (`_AxisTables`), every index checked against what it
    reads (the kernel cannot) -> (stage-1 mode, x1 offset, x1 taps, y1 offset, y1 taps, x2 offset, y2 offset, window w, h)."""
    H, W = img_shape[:2]
    (sx, sy, sw, sh), (rw, rh), (fx, fy, fw, fh) = d['src'], d['rsz'], d['win']
    x0, y0, cw, ch = d['chain']['win1'] if d['chain'] else d['win']
    r2w, r2h = d['chain']['rsz2'] if d['chain'] else (cw, ch)
    if not d['chain']:
        fx = fy = 0
    assert 0 <= sx and 0 <= sy and sx + sw <= W and sy + sh <= H
    assert 0 <= x0 and 0 <= y0 and x0 + cw <= rw and y0 + ch <= rh
    assert 0 <= fx and 0 <= fy and fx + fw <= r2w and fy + fh <= r2h and fw <= Wout and fh <= Hout
    mode = RESAMPLE_NEAREST if (sw, sh) == (rw, rh) else RESAMPLE_LINEAR
    tx, ty = _AXIS[mode](sw, rw, sx, x0, cw), _AXIS[mode](sh, rh, sy, y0, ch)
    bits = FLIP_BITS[d.get('flip_direction', 'horizontal') if d['flip'] else None]
    if bits & 1:
        tx = mirror_x(tx, W)
    if bits & 2:
        ty = mirror_x(ty, H)
    t2x, t2y = _stage2_axis(cw, r2w, fx, fw), _stage2_axis(ch, r2h, fy, fh)
    for t, dim in ((tx, W), (ty, H), (t2x, cw), (t2y, ch)):
        assert (t[:, 0] >= 0).all() and (t[:, 1] >= 1).all() and (t[:, 0] + t[:, 1] <= dim).all()
        assert (t[:, 1] <= t.shape[1] - 2).all()
    assert t2x.shape == (fw, 4) and t2y.shape == (fh, 4) and len(tx) == cw and len(ty) == ch
    (xt, kx), (yt, ky) = tabs.add(tx), tabs.add(ty)
    return mode, xt, kx, yt, ky, tabs.add(t2x)[0], tabs.add(t2y)[0], cw, ch
