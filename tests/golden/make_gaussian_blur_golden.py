"""Writes tests/golden/gaussian_blur_ref.npz: small uint8 frames and what Pillow's ``ImageFilter.GaussianBlur`` makes of them -- for
tests/test_gaussian_blur_cpu.py and tests/test_hip_gaussian_blur.py.  The reference's ``RandomGaussianBlur`` is
``img.filter(ImageFilter.GaussianBlur(radius=r))`` on the RGB PIL image.  Needs Pillow (and numpy for the file); imports nothing of the
package.

    python tests/golden/make_gaussian_blur_golden.py

The file holds ``sigmas`` (float64), ``cases`` (int32 rows: h, w, kind, index into sigmas), ``in_<h>x<w>_<kind>`` (h, w, 3) and
``out_<h>x<w>_<kind>_s<index>`` (h, w, 3); kind 0 is noise, 1 is 0 / 255 content.
"""
import os

import numpy as np
from PIL import Image, ImageFilter, __version__ as PIL_VERSION

KINDS = ('noise', 'binary')
SIGMAS = [5, 0.5, 1, 2, 3.3, 0.1, 10, 1.5, 7, 15, 0, 25]
SMALL = [(5, 7), (1, 9), (9, 1), (3, 3), (2, 50), (17, 40), (33, 21), (64, 48)]
SMALL_SIGMAS = [5, 0.5, 1, 2, 3.3, 0.1, 10, 1.5, 7, 15, 0]
LARGE = [(70, 150), (150, 70)]                    # wider and taller than one tile of the device kernels plus its halo
LARGE_SIGMAS = [5, 15]
BEYOND = [((17, 40), 25)]                         # a box radius the device kernels decline


def frame(rng, h, w, kind):
    if kind == 'noise':
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    return (rng.integers(0, 2, (h, w, 3)) * 255).astype(np.uint8)


def main():
    rng = np.random.default_rng(20240923)
    plan = [(hw, s) for hw in SMALL for s in SMALL_SIGMAS] + [(hw, s) for hw in LARGE for s in LARGE_SIGMAS] + BEYOND
    out = {'sigmas': np.array(SIGMAS, dtype=np.float64), 'pillow': np.array(PIL_VERSION)}
    cases = []
    for (h, w), sigma in plan:
        for k, kind in enumerate(KINDS):
            key = f'{h}x{w}_{kind}'
            if 'in_' + key not in out:
                out['in_' + key] = frame(rng, h, w, kind)
            si = SIGMAS.index(sigma)
            blurred = Image.fromarray(out['in_' + key]).filter(ImageFilter.GaussianBlur(radius=sigma))
            out[f'out_{key}_s{si}'] = np.asarray(blurred)
            cases.append((h, w, k, si))
    out['cases'] = np.array(cases, dtype=np.int32)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'gaussian_blur_ref.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes,', len(cases), 'cases, Pillow', PIL_VERSION)


if __name__ == '__main__':
    main()
