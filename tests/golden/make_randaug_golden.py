"""Writes tests/golden/randaug_pil.npz: Pillow's ImageOps.autocontrast / equalize (40 seeded images) and invert / posterize /
solarize (the first 8) of small uint8 arrays, the pinned targets of the RandAugment oracle's point operations
(tests/randaug_oracle.py), so that the Pillow on the machine that runs the tests cannot move them.
tests/test_randaug_cpu.py checks the file against the Pillow installed where it runs.  The operations are per channel, so the
channel order does not matter.

    python tests/golden/make_randaug_golden.py
"""
import os

import numpy as np
from PIL import Image, ImageOps

N, N_POINT, H, W = 40, 8, 32, 40
POSTERIZE_BITS, SOLARIZE_THR = (1, 2, 4, 7), (0, 26, 128, 255)


def images():
    """Seeded inputs: noise, gradients, constant channels, two-level channels, narrow ranges, full-range ramps."""
    rng = np.random.RandomState(77)
    out = []
    for i in range(N):
        img = np.zeros((H, W, 3), np.uint8)
        for c in range(3):
            kind = (i + c) % 6
            if kind == 0:
                ch = rng.randint(0, 256, (H, W))
            elif kind == 1:  # constant
                ch = np.full((H, W), rng.randint(0, 256))
            elif kind == 2:  # two levels
                a, b = rng.randint(0, 256, 2)
                ch = np.where(rng.rand(H, W) < rng.uniform(0.05, 0.95), a, b)
            elif kind == 3:  # narrow range
                lo = rng.randint(0, 240)
                ch = rng.randint(lo, lo + rng.randint(2, 16), (H, W))
            elif kind == 4:  # gradient with a limited range and noise
                lo, hi = rng.randint(0, 100), rng.randint(120, 256)
                ch = np.clip(np.linspace(lo, hi, H * W).reshape(H, W) + rng.randint(-9, 10, (H, W)), 0, 255)
            else:  # skewed: mostly dark with a bright tail
                ch = np.clip(rng.exponential(30, (H, W)), 0, 255)
            img[..., c] = ch.astype(np.uint8)
        out.append(img)
    return out


def make():
    out = {}
    for i, img in enumerate(images()):
        pil = Image.fromarray(img)
        out[f'autocontrast{i}'] = np.asarray(ImageOps.autocontrast(pil))
        out[f'equalize{i}'] = np.asarray(ImageOps.equalize(pil))
        if i < N_POINT:
            out[f'invert{i}'] = np.asarray(ImageOps.invert(pil))
            out[f'posterize{i}'] = np.asarray(ImageOps.posterize(pil, POSTERIZE_BITS[i % 4]))
            out[f'solarize{i}'] = np.asarray(ImageOps.solarize(pil, SOLARIZE_THR[i % 4]))
    return out


if __name__ == '__main__':
    np.savez_compressed(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'randaug_pil.npz'), **make())
