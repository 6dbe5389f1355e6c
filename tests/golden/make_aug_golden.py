"""Writes tests/golden/aug_pil_bicubic.npz: a few small Pillow BICUBIC resizes (up and down) of seeded uint8 BGR arrays, the
target of the device's backend='pillow' resample (tests/test_augment_gpu.py), so that the Pillow on the machine that runs
the GPU tests cannot move it.  tests/test_augment_cpu.py checks the file against the Pillow installed where it runs.

    python tests/golden/make_aug_golden.py
"""
import os

import numpy as np
from PIL import Image

CASES = [((40, 30), (64, 48)),    # (src h, w) -> (dst h, w): up
         ((90, 70), (33, 41)),    # down, anisotropic
         ((120, 100), (56, 56)),  # down ~2x
         ((17, 60), (50, 20))]    # up in y, down in x


def make():
    rng = np.random.RandomState(2024)
    out = {}
    for i, ((h, w), (oh, ow)) in enumerate(CASES):
        src = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
        out[f'src{i}'] = src
        out[f'dst{i}'] = np.asarray(Image.fromarray(src).resize((ow, oh), Image.BICUBIC))
    return out


if __name__ == '__main__':
    np.savez_compressed(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'aug_pil_bicubic.npz'), **make())
