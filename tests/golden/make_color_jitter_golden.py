"""Writes tests/golden/color_jitter_ref.npz: small uint8 frames and what torchvision's ``ColorJitter`` makes of them through Pillow, for
given orders and factors -- for tests/test_jitter_cpu.py and tests/test_hip_jitter.py.  torchvision's four PIL adjust functions
(transforms/_functional_pil.py) are restated below, a line or two each.  Needs Pillow (and numpy for the file); imports nothing of the
package.

    python tests/golden/make_color_jitter_golden.py
"""
import os

import numpy as np
from PIL import Image, ImageEnhance

OPS = ('brightness', 'contrast', 'saturation', 'hue')
B, C, S, H = OPS
# (order, {operation: factor}); an operation of the order without a factor is skipped, as torchvision skips a None range
PARAMS = [((B, C, S, H), {B: 0.8, C: 1.25, S: 0.75, H: 0.1}),            # contrast in the middle
          ((C, H, S, B), {B: 1.25, C: 0.75, S: 1.5, H: -0.2}),           # contrast first
          ((H, S, B, C), {B: 0.9, C: 2.0, S: 0.5, H: 0.5}),              # contrast last
          ((S, H, C, B), {B: 1.5, C: 0.5, S: 2.0, H: -0.5}),             # contrast in the middle, after hue
          ((B, C, S, H), {B: 1.0, C: 1.0, S: 1.0, H: 0.0}),              # every factor neutral: only the HSV round trip changes bytes
          ((B, C, S, H), {B: 0.0, C: 0.3, S: 0.7, H: 0.25}),             # brightness 0: black, contrast of a constant image
          ((S, C, B), {B: 1.1, C: 0.0, S: 0.0}),                         # saturation 0 (gray), contrast 0 (the mean everywhere)
          ((H,), {H: 0.003}),                                            # shift == 0: the lossy round trip alone
          ((H,), {H: -0.003}),                                           # int(-0.765) == 0 as well: truncation, not floor
          ((C,), {C: 1.5}),
          ((S, B), {B: 2.0, S: 1.25}),
          ((B, C, S, H), {C: 1.25, H: -0.1}),                            # two operations of the order skipped
          ((), {})]                                                      # nothing: the identity
FRAMES = [((37, 53), 'noise'), ((24, 40), 'smooth'), ((16, 16), 'binary'), ((2, 3), 'noise')]


def adjust_brightness(img, f):
    return ImageEnhance.Brightness(img).enhance(f)


def adjust_contrast(img, f):
    return ImageEnhance.Contrast(img).enhance(f)


def adjust_saturation(img, f):
    return ImageEnhance.Color(img).enhance(f)


def adjust_hue(img, f):
    h, s, v = img.convert('HSV').split()
    np_h = np.array(h, dtype=np.uint8)
    with np.errstate(over='ignore'):
        np_h += np.uint8(int(f * 255) % 256)          # torchvision: ``np_h += np.uint8(hue_factor * 255)``, a wrapping add
    return Image.merge('HSV', (Image.fromarray(np_h, 'L'), s, v)).convert('RGB')


ADJUST = {B: adjust_brightness, C: adjust_contrast, S: adjust_saturation, H: adjust_hue}


def color_jitter(a, order, factors):
    img = Image.fromarray(a)
    for name in order:
        if name in factors:
            img = ADJUST[name](img, factors[name])
    return np.asarray(img)


def frame(rng, h, w, kind):
    if kind == 'noise':
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == 'binary':
        return (rng.integers(0, 2, (h, w, 3)) * 255).astype(np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    return np.stack([(yy * 3 + xx * 2) % 256, (yy * xx) % 256, (255 - yy - xx) % 256], -1).astype(np.uint8)


def main():
    rng = np.random.default_rng(20240611)
    orders = np.zeros((len(PARAMS), 4), dtype=np.int32)                   # 1 + index into OPS, 0 past the end
    factors = np.full((len(PARAMS), 4), np.nan)                           # by operation; NaN: None
    for j, (order, f) in enumerate(PARAMS):
        orders[j, :len(order)] = [1 + OPS.index(o) for o in order]
        for name, v in f.items():
            factors[j, OPS.index(name)] = v
    out = {'orders': orders, 'factors': factors, 'frames': np.array([s for s, _ in FRAMES], dtype=np.int32)}
    for i, ((h, w), kind) in enumerate(FRAMES):
        a = frame(rng, h, w, kind)
        out[f'f{i}_in'] = a
        for j, (order, f) in enumerate(PARAMS):
            out[f'f{i}_p{j}'] = color_jitter(a, order, f)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'color_jitter_ref.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
