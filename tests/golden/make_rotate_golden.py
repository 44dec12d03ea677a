"""Writes tests/golden/rotate_ref.npz: small uint8 frames and labels with what Pillow makes of them -- ``Image.rotate`` (BICUBIC for the RGB
frame, NEAREST for the single-band label, expand=False, about the centre, fill 0) with the six doubles it hands to its affine transform,
and the VOC train chain transpose -> resize -> rotate -> paste on a pad x pad canvas -- for tests/test_rotate_cpu.py and
tests/test_hip_rotate.py.  Needs Pillow (and numpy for the file); imports nothing of the package.

    python tests/golden/make_rotate_golden.py
"""
import os

import numpy as np
from PIL import Image

SIZES = [(21, 33), (32, 32), (17, 40), (64, 48), (5, 7)]                       # (H, W)
ANGLES = [17.3, -29.999, 30, 0.001, -0.5, 12, 45, -45, 3.75, 29, -13.37, 90, 180, 270, 0]
BIG, BIG_ANGLES = (70, 150), [17.3, 270]                                       # wider and taller than one workgroup tile
CONTENTS = ('noise', 'binary')
# (H, W), hflip, scale, angle; pad 48.  An up-scale, and a flipped exact 2:1 reduction (where NEAREST is not mirror-symmetric)
CHAIN = [((30, 40), 0, 1.15, 17.3), ((60, 80), 1, 0.5, -23.5)]
PAD = 48


def frame(rng, h, w, kind):
    if kind == 'noise':
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    return (rng.integers(0, 2, (h, w, 3)) * 255).astype(np.uint8)              # bicubic overshoot on both sides of the clip


def label(rng, h, w):
    t = rng.integers(0, 21, (h, w), dtype=np.uint8)
    t[rng.random((h, w)) < 0.1] = 255
    return t


def matrix_of(img, angle):
    """The six doubles ``rotate`` passes to ``transform`` (an explicit centre at the default keeps it off the transpose fast paths)."""
    seen = []
    orig = Image.Image.transform

    def spy(self, size, method, data=None, *args, **kwargs):
        seen.append([float(v) for v in data])
        return orig(self, size, method, data, *args, **kwargs)
    Image.Image.transform = spy
    try:
        general = img.rotate(angle, Image.BICUBIC if img.mode == 'RGB' else Image.NEAREST, center=(img.width / 2.0, img.height / 2.0))
    finally:
        Image.Image.transform = orig
    return seen[0], np.asarray(general)


def rotations(out, rng, key, h, w, angles, contents):
    t = label(rng, h, w)
    out[f'{key}_label_in'] = t
    out[f'{key}_label_out'] = np.stack([np.asarray(Image.fromarray(t).rotate(a, Image.NEAREST)) for a in angles])
    for a, got in zip(angles, out[f'{key}_label_out']):
        assert (matrix_of(Image.fromarray(t), a)[1] == got).all(), (key, a)       # the transpose fast paths equal the general path
    for kind in contents:
        x = frame(rng, h, w, kind)
        img = Image.fromarray(x)
        out[f'{key}_{kind}_in'] = x
        out[f'{key}_{kind}_out'] = np.stack([np.asarray(img.rotate(a, Image.BICUBIC)) for a in angles])
        for a, got in zip(angles, out[f'{key}_{kind}_out']):
            assert (matrix_of(img, a)[1] == got).all(), (key, kind, a)
    out[f'{key}_m'] = np.array([matrix_of(Image.fromarray(t), a)[0] for a in angles], dtype=np.float64)


def main():
    rng = np.random.default_rng(20240611)
    out = {'sizes': np.array(SIZES, dtype=np.int32), 'angles': np.array(ANGLES, dtype=np.float64),
           'big_size': np.array(BIG, dtype=np.int32), 'big_angles': np.array(BIG_ANGLES, dtype=np.float64),
           'chain': np.array([[h, w, f, s, a, PAD] for (h, w), f, s, a in CHAIN], dtype=np.float64)}
    for i, (h, w) in enumerate(SIZES):
        rotations(out, rng, f's{i}', h, w, ANGLES, CONTENTS)
    rotations(out, rng, 'big', *BIG, BIG_ANGLES, ('noise',))
    for i, ((h, w), hflip, scale, angle) in enumerate(CHAIN):
        x, t = frame(rng, h, w, 'noise'), label(rng, h, w)
        out[f'k{i}_in'], out[f'k{i}_label_in'] = x, t
        img, lbl = Image.fromarray(x), Image.fromarray(t)
        if hflip:
            img, lbl = img.transpose(Image.FLIP_LEFT_RIGHT), lbl.transpose(Image.FLIP_LEFT_RIGHT)
        hr, wr = (int(s) for s in np.round(np.array((h, w)) * scale).astype(int))
        img, lbl = img.resize((wr, hr), Image.BICUBIC), lbl.resize((wr, hr), Image.NEAREST)
        img, lbl = img.rotate(angle, Image.BICUBIC, fillcolor=(0, 0, 0)), lbl.rotate(angle, Image.NEAREST, fillcolor=0)
        canvas, lcanvas = Image.new('RGB', (PAD, PAD), (0, 0, 0)), Image.new('L', (PAD, PAD), 255)
        canvas.paste(img, (0, 0))
        lcanvas.paste(lbl, (0, 0))
        out[f'k{i}_out'], out[f'k{i}_label_out'] = np.asarray(canvas), np.asarray(lcanvas)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'rotate_ref.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
