"""Writes tests/golden/resample_ref.npz: small uint8 frames and labels with what Pillow makes of them -- ``Image.resize`` (BILINEAR,
BICUBIC, NEAREST) and resize -> paste on a fill canvas -> crop -> flip -- for tests/test_resample_cpu.py and tests/test_hip_resample.py.
Needs Pillow (and numpy for the file); imports nothing of the package.

    python tests/golden/make_resample_golden.py
"""
import os

import numpy as np
from PIL import Image

# (Hi, Wi) -> (Ho, Wo): exact 2x down; odd sizes; up; bicubic ksize 17; one pass skipped (x2); mixed up and down; tiny; odd up
CASES = [((64, 128), (32, 64)), ((37, 53), (19, 31)), ((24, 40), (48, 80)), ((40, 72), (10, 18)), ((30, 50), (30, 25)),
         ((31, 45), (77, 45)), ((16, 16), (5, 37)), ((9, 8), (3, 3)), ((33, 47), (50, 61))]
LABEL_CASES = [((64, 64), (23, 191)), ((37, 53), (19, 31)), ((24, 40), (48, 80)), ((16, 16), (5, 37))]
# (Hi, Wi), resized (Hr, Wr), view (Ho, Wo), offset (oy, ox), hflip, fill
VIEW_CASES = [((24, 48), (12, 24), (20, 31), (-3, -4), 1, (7, 128, 250)), ((24, 48), (48, 96), (20, 31), (9, 40), 0, (0, 0, 0)),
              ((24, 48), (12, 24), (6, 5), (3, 20), 1, (1, 2, 3))]
FILTERS = {'bilinear': Image.BILINEAR, 'bicubic': Image.BICUBIC}


def frame(rng, h, w, kind):
    if kind == 'noise':
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == 'binary':            # bicubic overshoot on both sides of clip8
        return (rng.integers(0, 2, (h, w, 3)) * 255).astype(np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    return np.stack([(yy * 3 + xx * 2) % 256, (yy * xx) % 256, (255 - yy - xx) % 256], -1).astype(np.uint8)


def view_of(img, resized, size, offset, hflip, fill):
    """resize happened; paste on a canvas of ``fill`` that holds the window, crop the window, flip."""
    (hr, wr), (ho, wo), (oy, ox) = resized, size, offset
    top, left = max(-oy, 0), max(-ox, 0)
    canvas = Image.new(img.mode, (left + max(wr, ox + wo), top + max(hr, oy + ho)), fill)
    canvas.paste(img, (left, top))
    out = canvas.crop((ox + left, oy + top, ox + left + wo, oy + top + ho))
    return out.transpose(Image.FLIP_LEFT_RIGHT) if hflip else out


def main():
    rng = np.random.default_rng(20240607)
    out = {'cases': np.array([[*a, *b] for a, b in CASES], dtype=np.int32),
           'label_cases': np.array([[*a, *b] for a, b in LABEL_CASES], dtype=np.int32),
           'view_cases': np.array([[*a, *b, *c, *d, e, *f] for a, b, c, d, e, f in VIEW_CASES], dtype=np.int32)}
    kinds = ('noise', 'binary', 'smooth')
    for i, ((hi, wi), (ho, wo)) in enumerate(CASES):
        x = frame(rng, hi, wi, kinds[i % 3])
        out[f'c{i}_in'] = x
        for name, f in FILTERS.items():
            out[f'c{i}_{name}'] = np.asarray(Image.fromarray(x).resize((wo, ho), f))
    for i, ((hi, wi), (ho, wo)) in enumerate(LABEL_CASES):
        t = rng.integers(0, 20, (hi, wi), dtype=np.uint8)
        out[f'l{i}_in'] = t
        out[f'l{i}_out'] = np.asarray(Image.fromarray(t).resize((wo, ho), Image.NEAREST))
    for i, ((hi, wi), (hr, wr), size, offset, hflip, fill) in enumerate(VIEW_CASES):
        x, t = frame(rng, hi, wi, 'noise'), rng.integers(0, 20, (hi, wi), dtype=np.uint8)
        out[f'v{i}_in'], out[f'v{i}_label_in'] = x, t
        out[f'v{i}_bicubic'] = np.asarray(view_of(Image.fromarray(x).resize((wr, hr), Image.BICUBIC), (hr, wr), size, offset, hflip, fill))
        out[f'v{i}_label'] = np.asarray(view_of(Image.fromarray(t).resize((wr, hr), Image.NEAREST), (hr, wr), size, offset, hflip, 255))
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'resample_ref.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
