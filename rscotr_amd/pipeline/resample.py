"""Host-built integer resampling tables of the device input path, so that the device arithmetic is integer and exact: per axis
and output coordinate the source index, tap count and integer weights.
  'cv2'     mmcv imresize / imrescale interpolation='bilinear': the scalar fixed-point form of OpenCV's uint8 INTER_LINEAR
            (11-bit weights).  Parity with cv2 itself is unpinned: +-1 LSB expected (SIMD / IPP / exact-2x paths), unmeasured.
  'pillow'  mmcv backend='pillow', interpolation='bicubic': Pillow's ImagingResample (antialiased, 22-bit weights,
            uint8-clipped horizontal pass then vertical pass); equal to Pillow's own output.
Label maps are resampled 'nearest' (mmcv: cv2 INTER_NEAREST).  Also here: mmcv's rescale_size, mmdet's box scaling and OpenCV's
bicubic remap weights (the warps of RandAugment)."""
import numpy as np

RESAMPLE_NEAREST, RESAMPLE_LINEAR, RESAMPLE_PIL = 0, 1, 2


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


def mirror_x(t, W):
    """The x entries of a row of width W that is flipped left-right BEFORE it is resampled: taps first .. first + n - 1 of the
    flipped row are taps W - first - n .. W - first - 1 of the stored one, with the weights in reverse order (<= 2 taps).  The
    y entries of a column of height W that is flipped upside down are the same thing."""
    assert t.shape[1] <= 4
    t = t.copy()
    t[:, 0] = W - t[:, 0] - t[:, 1]
    if t.shape[1] == 4:
        two = t[:, 1] == 2
        t[two, 2:4] = t[two, 2:4][:, ::-1]
    return t


_AXIS = {RESAMPLE_NEAREST: _axis_nearest, RESAMPLE_LINEAR: _axis_linear, RESAMPLE_PIL: _axis_pil_bicubic}


class _AxisTables:
    """The tables of one batch, in the order they were added; `flat()` is what the launches take."""

    def __init__(self):
        self.tabs, self.size = [], 0

    def add(self, t):
        """-> (offset of `t` in int32 elements, its taps K)"""
        self.tabs.append(t)
        self.size += t.size
        return self.size - t.size, t.shape[1] - 2

    def add_window(self, mode, d, Hout, Wout, mirror_w=None, mirror_h=None):
        """The x and y tables of one sample's draw `d` (DeviceCollate.draw): identity nearest entries where it is not resized
        (its window is read as is) -> (mode, x offset, x taps, y offset, y taps).  `mirror_w`: the source, that many pixels
        wide, is flipped left-right in front of the resampling (`mirror_x`); `mirror_h`: that many pixels high, upside down."""
        (sx, sy, sw, sh), (rw, rh), (x0, y0, cw, ch) = d['src'], d['rsz'], d['win']
        assert 0 <= x0 and 0 <= y0 and x0 + cw <= rw and y0 + ch <= rh and cw <= Wout and ch <= Hout
        mode = RESAMPLE_NEAREST if (sw, sh) == (rw, rh) else mode
        tx = _AXIS[mode](sw, rw, sx, x0, cw)
        if mirror_w is not None:
            tx = mirror_x(tx, mirror_w)
        xt, kx = self.add(tx)
        ty = _AXIS[mode](sh, rh, sy, y0, ch)
        if mirror_h is not None:
            ty = mirror_x(ty, mirror_h)
        yt, ky = self.add(ty)
        return mode, xt, kx, yt, ky

    def check(self, shapes):
        """Bounds of every source read (the kernel cannot check them): `shapes` = the (H, W) of the sources, in the order of
        the `add_window` calls."""
        for t, dim in zip(self.tabs, [n for hw in shapes for n in (hw[1], hw[0])]):
            assert (t[:, 0] >= 0).all() and (t[:, 0] + t[:, 1] <= dim).all() and (t[:, 1] >= 1).all()

    def flat(self):
        return np.concatenate([t.reshape(-1) for t in self.tabs]) if self.tabs else np.zeros(1, np.int32)


def _scale_size(w, h, scale):  # mmcv _scale_size
    return int(w * float(scale) + 0.5), int(h * float(scale) + 0.5)


def rescale_size(w, h, scale):
    """mmcv rescale_size: a number, or a (long, short) edge pair -> ((new_w, new_h), scale factor)."""
    if isinstance(scale, (float, int)):
        sf = scale
    else:
        sf = min(max(scale) / max(h, w), min(scale) / min(h, w))
    return _scale_size(w, h, sf), sf


def scale_boxes(bboxes, scale_factor, img_shape):
    """mmdet Resize._resize_bboxes with bbox_clip_border=True: float32 boxes * scale_factor, clipped to img_shape."""
    b = np.asarray(bboxes, np.float32) * np.asarray(scale_factor, np.float32)
    b[:, 0::2] = np.clip(b[:, 0::2], 0, img_shape[1])
    b[:, 1::2] = np.clip(b[:, 1::2], 0, img_shape[0])
    return b


# mmcv imflip's directions as the flip word of the kernels' meta rows (include/rscotr.h): bit 0 mirrors x, bit 1 mirrors y
FLIP_BITS = {None: 0, 'horizontal': 1, 'vertical': 2, 'diagonal': 3}


def flip_boxes(bboxes, direction, w, h):
    """mmdet RandomFlip.bbox_flip on an (h, w) image: 'horizontal' x1' = w - x2, x2' = w - x1; 'vertical' the same in y with h;
    'diagonal' both; None: unchanged.  float32 (n, 4)."""
    b = np.asarray(bboxes, np.float32).reshape(-1, 4)
    x1, y1, x2, y2 = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
    bits = FLIP_BITS[direction]
    if bits & 1:
        x1, x2 = np.float32(w) - x2, np.float32(w) - x1
    if bits & 2:
        y1, y2 = np.float32(h) - y2, np.float32(h) - y1
    return np.stack([x1, y1, x2, y2], -1)


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
