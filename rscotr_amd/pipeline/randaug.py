"""Host side of RandAugment on the device (`rand_augment=`, cls only, off by default; configs/_base_/cls/resisc_swin_224.py:15-27
with the policies of configs/_base_/cls/rand_aug.py).  It turns the collate's one launch into a short sequence:
`rscotr_img_frames_u8` writes the resized, flipped uint8 frames, `rscotr_randaug_u8` runs once per policy slot (each sample its own
operation, ping frame to pong frame), and `rscotr_img_aug_u8` finishes over identity entries (RandomErasing, Normalize, pad).  The
host draws from BOTH of mmcls's generators in its order (Python `random`: the policy choice and the gauss magnitudes;
`numpy.random`: each transform's prob and sign draws) and builds the integer tables of the warps (cv2.warpAffine's fixed point).
The operations are restated from mmcv / OpenCV as remembered (tests/randaug_oracle.py spells them out): parity with mm* / cv2 is by
reading and unpinned."""
import math

import numpy as np

# include/rscotr.h: rscotr_randaug_u8's op codes, meta row and stats row
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
    """`warp_table` of a RandAugment warp: bicubic or nearest."""
    return warp_table(M, w, h, 16 if bicubic else 512)


def warp_table(M, w, h, rd):
    """cv2.warpAffine without WARP_INVERSE_MAP: M inverted in float64 as OpenCV does, then the int32 coordinate tables
    adelta[w] | bdelta[w] | X0[h] | Y0[h] (AB_SCALE = 1024, round_delta `rd` = 16 bicubic and bilinear / 512 nearest folded into
    X0, Y0)."""
    m0, m1, m2, m3, m4, m5 = [float(v) for v in M]
    D = m0 * m4 - m1 * m3
    D = 1.0 / D if D != 0 else 0.0
    a11, a22 = m4 * D, m0 * D
    m0, m1, m3, m4 = a11, m1 * -D, m3 * -D, a22
    b1 = -m0 * m2 - m1 * m5
    b2 = -m3 * m2 - m4 * m5
    x, y = np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64)
    t = np.concatenate([np.rint(m0 * x * 1024), np.rint(m3 * x * 1024), np.rint((m1 * y + b1) * 1024) + rd,
                        np.rint((m4 * y + b2) * 1024) + rd])
    return np.clip(t, -2 ** 30, 2 ** 30).astype(np.int32)  # (a coordinate that large is outside any frame either way)


def _f32_bits(v):
    return int(np.float32(v).view(np.int32))


def ra_draws(ra, w, h, rng, py_rng):
    """mmcls RandAugment.__call__ on a (h, w) frame for the config `ra` (`_ra_config`) -> (plan, chosen policies).  Python's
    generator: random.choices(policies, k=num_policies), then per chosen policy with a magnitude_key one gauss(magnitude_level,
    magnitude_std) when std > 0.  NumPy's, per transform in order: rand() > prob -> unchanged; else, for the signed ones, rand() <
    random_negative_prob.  A plan entry is (op code, magnitude or None, applied, forward warpAffine matrix or None)."""
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


def ra_meta_row(entry, p, w, h, warp_off):
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


def ra_slot_rows(K, ds):
    """The K slots' meta rows and the warps' coordinate tables of a batch of draws `ds` (DeviceCollate.draw) ->
    (rmeta (K, B, RA_META) int32, warp int32, per slot whether it needs the statistics pass); K and B at least 1 in `rmeta`."""
    B = len(ds)
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
            rmeta[k, b] = ra_meta_row(entry, p, cw, ch, off)
            need_stats[k] = need_stats[k] or (entry[2] and entry[0] in RA_STATS_OPS)
        for k in range(len(d['ra']), K):
            rmeta[k, b, 1:3] = cw, ch
    return rmeta, np.concatenate(warps), need_stats
