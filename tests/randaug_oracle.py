"""NumPy restatement (test infrastructure only) of mmcls RandAugment with the policies of the reference's cls config
(configs/_base_/cls/rand_aug.py, configs/_base_/cls/resisc_swin_224.py:15-27), for the device path of rscotr_amd/pipeline/
(`rscotr_img_frames_u8` -> `rscotr_randaug_u8` -> `rscotr_img_aug_u8`).  Written apart from the pipeline package on purpose: its own
inverse matrices, its own weight table, its own look-up tables, so a host-side table bug shows up as a mismatch.

mmcls / mmcv / cv2 are not installed.  Everything below is restated from upstream AS REMEMBERED, so parity with mm* / cv2 is by
reading and UNPINNED (as it is for the bilinear resize and the HSV conversions of tests/aug_oracle.py); a real cv2 may differ by
1 LSB at rounding ties.  AutoContrast, Equalize, Invert, Posterize and Solarize are pinned: they equal Pillow's ImageOps
functions of the same name (tests/golden/randaug_pil.npz, tests/test_randaug_cpu.py).

Driver (mmcls RandAugment.__call__), two generators:
    if num_policies == 0: return
    sub_policy = random.choices(policies, k=num_policies)                      # Python `random`
    per chosen policy with a magnitude_key:                                    # Python `random`
        level = magnitude_level; if magnitude_std > 0: level = random.gauss(magnitude_level, magnitude_std)
        level = min(total_level, max(0, level)); (lo, hi) = magnitude_range
        policy[magnitude_key] = (level / total_level) * (hi - lo) + lo
    hparams keys are added to a policy only if it lacks them and its transform accepts them (pad_val, interpolation: Rotate,
    Shear, Translate; mmcls defaults pad_val=128, interpolation 'nearest' for Rotate / Translate and 'bicubic' for Shear)
    then the transforms run in order; each one:                                # numpy.random
        if np.random.rand() > prob (0.5): return unchanged
        Rotate, Shear, Translate, ColorTransform, Contrast, Brightness, Sharpness:
            m = -m if np.random.rand() < random_negative_prob (0.5) else m

Operations on the uint8 BGR image (mmcv):
    AutoContrast   auto_contrast(cutoff=0), per channel: lo, hi = min, max; hi <= lo: unchanged; else s = 255.0 / (hi - lo),
                   lut[i] = clip(i * s + (-lo * s), 0, 255) in float64, truncated to uint8.
    Equalize       imequalize, per channel: h = histogram, step = (sum(h) - last non-zero bin) // 255; step == 0: unchanged;
                   else lut = [0] + ((cumsum(h) + step // 2) // step)[:-1], clipped at 255.
    Invert         255 - v.
    Posterize      bits = ceil(m); 8: unchanged; else (v >> (8 - bits)) << (8 - bits) (0 bits: 0).
    Solarize       v if v < thr else 255 - v (thr a float).
    SolarizeAdd    v < 128: uint8(min(v + m, 255)) (float64 sum, truncated); else v.
    ColorTransform adjust_color(alpha = 1 + m): g = cv2 BGR2GRAY = (B * 3735 + G * 19235 + R * 9798 + 2^14) >> 15;
                   cv2.addWeighted(img, alpha, g, 1 - alpha, 0) on uint8: float32 img * a + g * b, rounded half to even, saturated.
    Contrast       adjust_contrast(f = 1 + m): mean = round(sum(g) / n) (Python round of the float64 quotient); float32
                   img * f + mean * (1 - f), clip(0, 255), truncated.
    Brightness     adjust_brightness: float32 img * f (the other term is 0 * (1 - f)), clip, truncated.
    Sharpness      adjust_sharpness: d = cv2.filter2D(img, [[1,1,1],[1,5,1],[1,1,1]] / 13): float32 coefficients, float32
                   accumulation over the 9 taps in row-major order from 0, BORDER_REFLECT_101, rounded half to even to uint8;
                   float32 img * f + d * (1 - f), clip, truncated.
    Float steps are float32 with the scalars cast to float32 (b = float32(1 - f) of the float64 f), unfused, in that order.

Warps: cv2.warpAffine(img, M, (w, h), flags=interp, borderValue=pad_val) WITHOUT WARP_INVERSE_MAP, so M is inverted in float64:
    D = M0 * M4 - M1 * M3; D = 1 / D (0 if D == 0); A11 = M4 * D; A22 = M0 * D; M0 = A11; M1 *= -D; M3 *= -D; M4 = A22;
    b1 = -M0 * M2 - M1 * M5; b2 = -M3 * M2 - M4 * M5; M2 = b1; M5 = b2
    Shear      horizontal [[1, m, 0], [0, 1, 0]], vertical [[1, 0, 0], [m, 1, 0]]
    Translate  offset m * w in M2 (horizontal) or m * h in M5 (vertical)
    Rotate     cv2.getRotationMatrix2D(((w - 1) / 2, (h - 1) / 2), -m, 1): a = -m * pi / 180, al = cos a, be = sin a,
               [[al, be, (1 - al) * cx - be * cy], [-be, al, be * cx + (1 - al) * cy]]
  fixed point: AB_SCALE = 1024, round_delta = 512 (nearest) | 16 (bicubic); adelta[x] = rint(M0 * x * 1024),
  bdelta[x] = rint(M3 * x * 1024), X0 = rint((M1 * y + M2) * 1024) + round_delta, Y0 likewise with M4, M5;
  nearest: sx = (X0 + adelta[x]) >> 10; bicubic: X = (X0 + adelta[x]) >> 5, sx = X >> 5, ax = X & 31; taps sx - 1 .. sx + 2 by
  sy - 1 .. sy + 2; weights saturate<short>(cy[k1] * cx[k2] * 32768) (rounded half to even) of the float32 cubic coefficients
  (A = -0.75) at a / 32; out = saturate((sum w * p + 2^14) >> 15); a tap outside the image reads pad_val (BGR).
  CHOSEN where the description "central 2 x 2" is not workable: the 16 weights are corrected to sum to 32768 by adding the
  deficit to the largest, or taking the excess from the smallest, of the block k1, k2 in (2, 3) -- OpenCV's initInterTab2D
  scans `ksize / 2 .. ksize / 2 + 1`, which for 4 taps is that block.  With the block (1, 2) the entry of a = (0, 0)
  (weights 32767 + deficit 1) would need 32768 in an int16.  cv2's saturate_cast<short> of the source coordinates is left out
  (it matters beyond +-32767 pixels only)."""
import math

import numpy as np

import aug_oracle as AO
from oracle import pipeline as OP

F = np.float32
SIGNED = ('Rotate', 'Shear', 'Translate', 'ColorTransform', 'Contrast', 'Brightness', 'Sharpness')
WARP_DEFAULT_INTERP = dict(Rotate='nearest', Shear='bicubic', Translate='nearest')
ARG = dict(Rotate='angle', Posterize='bits', Solarize='thr')


# ---- point operations ----------------------------------------------------------------------------------------------------
def _per_channel(img, lut_of):
    out = img.copy()
    for c in range(img.shape[2]):
        lut = lut_of(np.bincount(img[..., c].reshape(-1), minlength=256))
        if lut is not None:
            out[..., c] = np.asarray(lut)[img[..., c]].astype(np.uint8)
    return out


def auto_contrast(img):
    def lut_of(h):
        nz = np.nonzero(h)[0]
        lo, hi = int(nz[0]), int(nz[-1])
        if hi <= lo:
            return None
        s = 255.0 / (hi - lo)
        return np.clip(np.arange(256) * s + (-lo * s), 0, 255).astype(np.uint8)
    return _per_channel(img, lut_of)


def equalize(img):
    def lut_of(h):
        step = (int(h.sum()) - int(h[h > 0][-1])) // 255
        if step == 0:
            return None
        lut = (np.cumsum(h) + step // 2) // step
        return np.minimum(np.concatenate([[0], lut[:-1]]), 255)
    return _per_channel(img, lut_of)


def invert(img):
    return (255 - img.astype(np.int64)).astype(np.uint8)


def posterize(img, bits):
    bits = int(math.ceil(bits))
    if bits == 8:
        return img.copy()
    s = 8 - bits
    return ((img.astype(np.int64) >> s) << s).astype(np.uint8)


def solarize(img, thr):
    return np.where(img < thr, img, 255 - img).astype(np.uint8)


def solarize_add(img, m, thr=128):
    return np.where(img < thr, np.minimum(img + float(m), 255), img).astype(np.uint8)  # (a RandAugment magnitude is a float)


def grey(img):
    p = img.astype(np.int64)
    return (p[..., 0] * 3735 + p[..., 1] * 19235 + p[..., 2] * 9798 + (1 << 14)) >> 15


def _weighted(img, a, other, b):
    """float32 img * a + other * b (two rounded products, one rounded sum)."""
    return (img.astype(F) * F(a)).astype(F) + (np.asarray(other, F) * F(b)).astype(F)


def color(img, m):
    alpha = 1 + m
    v = _weighted(img, alpha, grey(img)[..., None].astype(F), 1 - alpha)
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def contrast(img, m):
    f = 1 + m
    g = grey(img)
    mean = round(float(g.sum()) / g.size)
    return np.clip(_weighted(img, f, F(mean), 1 - f), 0, 255).astype(np.uint8)


def brightness(img, m):
    return np.clip((img.astype(F) * F(1 + m)).astype(F), 0, 255).astype(np.uint8)


def sharpness(img, m):
    f = 1 + m
    k = (np.array([[1., 1., 1.], [1., 5., 1.], [1., 1., 1.]]) / 13).astype(F)
    H, W = img.shape[:2]
    ys = [1 if H > 1 else 0] + list(range(H)) + [H - 2 if H > 1 else 0]  # reflect-101 index lists
    xs = [1 if W > 1 else 0] + list(range(W)) + [W - 2 if W > 1 else 0]
    pad = img[ys][:, xs].astype(F)
    acc = np.zeros(img.shape, F)
    for dy in range(3):
        for dx in range(3):
            acc = (acc + (k[dy, dx] * pad[dy:dy + H, dx:dx + W]).astype(F)).astype(F)
    d = np.clip(np.rint(acc), 0, 255).astype(np.uint8)
    return np.clip(_weighted(img, f, d, 1 - f), 0, 255).astype(np.uint8)


# ---- warps -------------------------------------------------------------------------------------------------------------
def _cubic(x):
    A = F(-0.75)
    one = F(1)
    c0 = ((A * (x + one) - F(5) * A) * (x + one) + F(8) * A) * (x + one) - F(4) * A
    c1 = ((A + F(2)) * x - (A + F(3))) * x * x + one
    c2 = ((A + F(2)) * (one - x) - (A + F(3))) * (one - x) * (one - x) + one
    return [c0, c1, c2, one - c0 - c1 - c2]


_WTAB = []


def weight_table():
    """(32, 32, 4, 4) int64 [ay, ax, k1, k2], see the docstring."""
    if _WTAB:
        return _WTAB[0]
    co = [_cubic(F(i) * F(1.0 / 32)) for i in range(32)]
    tab = np.zeros((32, 32, 4, 4), np.int64)
    for ay in range(32):
        for ax in range(32):
            it = np.zeros((4, 4), np.int64)
            for k1 in range(4):
                for k2 in range(4):
                    v = F(co[ay][k1] * co[ax][k2])
                    it[k1, k2] = min(max(int(np.rint(F(v * F(32768)))), -32768), 32767)
            diff = int(it.sum()) - 32768
            if diff != 0:
                mk, Mk = (2, 2), (2, 2)
                for k1 in (2, 3):
                    for k2 in (2, 3):
                        if it[k1, k2] < it[mk]:
                            mk = (k1, k2)
                        elif it[k1, k2] > it[Mk]:
                            Mk = (k1, k2)
                if diff < 0:
                    it[Mk] -= diff
                else:
                    it[mk] -= diff
            tab[ay, ax] = it
    _WTAB.append(tab)
    return tab


def warp_affine(img, M, interpolation='bicubic', pad_val=(128, 128, 128)):
    """cv2.warpAffine(img, M (2 x 3, forward), (w, h), flags=interpolation, borderValue=pad_val)."""
    h, w = img.shape[:2]
    M = [[float(v) for v in row] for row in M]
    D = M[0][0] * M[1][1] - M[0][1] * M[1][0]
    D = 1.0 / D if D != 0 else 0.0
    A11, A22 = M[1][1] * D, M[0][0] * D
    M[0][0], M[0][1], M[1][0], M[1][1] = A11, M[0][1] * -D, M[1][0] * -D, A22
    b1 = -M[0][0] * M[0][2] - M[0][1] * M[1][2]
    b2 = -M[1][0] * M[0][2] - M[1][1] * M[1][2]
    M[0][2], M[1][2] = b1, b2
    bic = interpolation == 'bicubic'
    assert bic or interpolation == 'nearest'
    rd = 16 if bic else 512
    xs, ys = np.arange(w), np.arange(h)
    X = (np.rint((M[0][1] * ys + M[0][2]) * 1024).astype(np.int64) + rd)[:, None] + np.rint(M[0][0] * xs * 1024).astype(np.int64)[None]
    Y = (np.rint((M[1][1] * ys + M[1][2]) * 1024).astype(np.int64) + rd)[:, None] + np.rint(M[1][0] * xs * 1024).astype(np.int64)[None]
    pad = np.asarray(pad_val, np.int64).reshape(1, 1, 3)
    src = img.astype(np.int64)

    def fetch(sy, sx):
        ok = (sx >= 0) & (sx < w) & (sy >= 0) & (sy < h)
        return np.where(ok[..., None], src[np.clip(sy, 0, h - 1), np.clip(sx, 0, w - 1)], pad)
    if not bic:
        return fetch(Y >> 10, X >> 10).astype(np.uint8)
    X, Y = X >> 5, Y >> 5
    wt = weight_table()[Y & 31, X & 31]  # (h, w, 4, 4)
    acc = np.zeros((h, w, 3), np.int64)
    for k1 in range(4):
        for k2 in range(4):
            acc += wt[:, :, k1, k2, None] * fetch((Y >> 5) - 1 + k1, (X >> 5) - 1 + k2)
    return np.clip((acc + (1 << 14)) >> 15, 0, 255).astype(np.uint8)


def rotate(img, angle, interpolation='nearest', pad_val=(128, 128, 128)):
    h, w = img.shape[:2]
    a = -angle * math.pi / 180.0
    al, be = math.cos(a), math.sin(a)
    cx, cy = (w - 1) * 0.5, (h - 1) * 0.5
    return warp_affine(img, [[al, be, (1 - al) * cx - be * cy], [-be, al, be * cx + (1 - al) * cy]], interpolation, pad_val)


def shear(img, m, direction='horizontal', interpolation='bicubic', pad_val=(128, 128, 128)):
    M = [[1, m, 0], [0, 1, 0]] if direction == 'horizontal' else [[1, 0, 0], [m, 1, 0]]
    return warp_affine(img, M, interpolation, pad_val)


def translate(img, m, direction='horizontal', interpolation='nearest', pad_val=(128, 128, 128)):
    h, w = img.shape[:2]
    M = [[1, 0, m * w], [0, 1, 0]] if direction == 'horizontal' else [[1, 0, 0], [0, 1, m * h]]
    return warp_affine(img, M, interpolation, pad_val)


# ---- the driver ----------------------------------------------------------------------------------------------------------
def magnitude(policy, level, total_level):
    lo, hi = policy['magnitude_range']
    return (level / total_level) * (hi - lo) + lo


def _pad3(v):
    return tuple(int(x) for x in ((v,) * 3 if isinstance(v, (int, float)) else v))


def apply_policy(img, p, m, hparams, rng, log=None):
    """One transform of a sub-policy with its numpy.random draws; `log` collects (name, applied, sign, bytes changed)."""
    typ = p['type']
    name = typ + ('/' + p['direction'] if 'direction' in p else '')
    if rng.rand() > p.get('prob', 0.5):
        if log is not None:
            log.append((name, False, 0, 0))
        return img
    sign = 0
    if typ in SIGNED:
        sign = 1
        if rng.rand() < p.get('random_negative_prob', 0.5):
            m, sign = -m, -1
    if typ in WARP_DEFAULT_INTERP:
        interp = p.get('interpolation', hparams.get('interpolation', WARP_DEFAULT_INTERP[typ]))
        pad = _pad3(p.get('pad_val', hparams.get('pad_val', 128)))
        if typ == 'Rotate':
            out = rotate(img, m, interp, pad)
        elif typ == 'Shear':
            out = shear(img, m, p.get('direction', 'horizontal'), interp, pad)
        else:
            out = translate(img, m, p.get('direction', 'horizontal'), interp, pad)
    else:
        out = dict(AutoContrast=lambda: auto_contrast(img), Equalize=lambda: equalize(img), Invert=lambda: invert(img),
                   Posterize=lambda: posterize(img, m), Solarize=lambda: solarize(img, m),
                   SolarizeAdd=lambda: solarize_add(img, m), ColorTransform=lambda: color(img, m),
                   Contrast=lambda: contrast(img, m), Brightness=lambda: brightness(img, m),
                   Sharpness=lambda: sharpness(img, m))[typ]()
    if log is not None:
        log.append((name, True, sign, int((out != img).sum())))
    return out


def rand_augment(img, cfg, rng, py_rng, log=None):
    """mmcls RandAugment.__call__ (see the docstring); cfg: policies, num_policies, magnitude_level, total_level=30,
    magnitude_std=0., hparams."""
    k = cfg.get('num_policies', 0)
    if k == 0:
        return img
    total, level0, std = cfg.get('total_level', 30), cfg.get('magnitude_level', 0), cfg.get('magnitude_std', 0.)
    sub = py_rng.choices(cfg['policies'], k=k)
    mags = []
    for p in sub:
        if p.get('magnitude_key') is None:
            mags.append(p.get(ARG.get(p['type'], 'magnitude')))
            continue
        level = level0
        if std > 0:
            level = py_rng.gauss(level0, std)
        mags.append(magnitude(p, min(total, max(0, level)), total))
    for p, m in zip(sub, mags):
        img = apply_policy(img, p, m, cfg.get('hparams') or {}, rng, log)
    return img


def cls_sample(img, rng, py_rng, cfg, size=224, flip_prob=0.5, erasing=None, backend='pillow', log=None):
    """mmcls RandomResizedCrop -> RandomFlip -> RandAugment -> RandomErasing (size=None: no RandomResizedCrop)."""
    if size is not None:
        H, W = img.shape[:2]
        oy, ox, th, tw = AO.rrc_params(H, W, rng)
        img = AO.resize_img(img[oy:oy + th, ox:ox + tw], size, size, backend)
    fl = bool(rng.rand() < flip_prob)
    if fl:
        img = OP.imflip(img)
    img = rand_augment(img, cfg, rng, py_rng, log)
    if erasing is not None:
        img = AO.random_erasing(img, rng, **erasing)
    return img, dict(flip=fl)


def structured_image(rng, h, w):
    """A seeded test image that is not uniform noise: per-channel gradients with limited, different ranges plus blocks and
    mild noise, so AutoContrast and Equalize are not identities and warps move visible structure."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    out = np.zeros((h, w, 3), np.uint8)
    for c in range(3):
        lo = rng.randint(5, 80)
        hi = rng.randint(150, 250)
        fx, fy = rng.uniform(0.5, 3.0, 2)
        g = 0.5 + 0.25 * np.sin(fx * xx / max(w, 1) * 6.28 + c) + 0.25 * np.cos(fy * yy / max(h, 1) * 6.28 - c)
        g = lo + (hi - lo) * g + rng.randint(-6, 7, (h, w))
        out[..., c] = np.clip(g, lo, hi).astype(np.uint8)
    by, bx = rng.randint(0, max(h - 3, 1)), rng.randint(0, max(w - 3, 1))
    out[by:by + max(h // 4, 1), bx:bx + max(w // 4, 1)] //= 2
    return out
