"""torchvision's ``ColorJitter`` on uint8 RGB frames as data and arithmetic: what the device kernels compute (csrc/hs_jitter.hip) and the
whole operation on the CPU.  The reference's HyperSeg-S and VOC train configs end their image chain with ``ColorJitter`` on a PIL image,
where torchvision only orchestrates Pillow: a drawn order of up to four operations, each reading and writing a uint8 RGB image --
``ImageEnhance.Brightness / Contrast / Color(img).enhance(f)`` and, for hue, ``convert('HSV')``, a wrapping uint8 add on H,
``convert('RGB')``.  The arithmetic is restated here (float32 / float64 where Pillow's C uses float / double); Pillow is not imported.
Results equal Pillow's byte for byte (tests/test_jitter_cpu.py, tests/golden/color_jitter_ref.npz).

  * ``blend(a, b, alpha)`` (``Image.blend``, the core of every ``enhance``; ``alpha`` rounded to float32):
    ``t = float32(a) + float32(alpha * float32(b - a))`` -- two separately rounded float32 operations, never a fused multiply-add --
    then 0 where ``t <= 0``, 255 where ``t >= 255``, ``(int)t`` elsewhere.  (Pillow skips the clip for ``0 <= alpha <= 1``; ``t`` then
    lies in [0, 255] by itself, so the one form covers both.)
  * ``gray``: ``L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16`` (``convert('L')``).
  * brightness ``f``: ``blend(0, x, f)``; saturation ``f``: ``blend(L(pixel), x, f)``; contrast ``f``: ``blend(m, x, f)`` with
    ``m = int(sum(L) / count + 0.5)`` in float64 over the image AS IT STANDS when contrast is applied.
  * hue ``h``: ``shift = int(h * 255) mod 256`` (float64 product, truncated toward zero); RGB -> HSV, ``H' = (H + shift) mod 256``,
    HSV -> RGB.  The round trip is lossy and is applied even when ``shift == 0``.  :func:`rgb_to_hsv` / :func:`hsv_to_rgb` spell the
    two conversions out.

The device reads one record of ``TABLE_WORDS`` int32 words per sample (:func:`params_table`): the order as 4-bit operation codes, the
three float32 factors as bits, the hue shift, and the set of operations present."""
import collections

import numpy as np
import torch

OPS = ('brightness', 'contrast', 'saturation', 'hue')
OP_CODES = {name: i + 1 for i, name in enumerate(OPS)}          # 0 ends the order
TABLE_WORDS = 8

_Params = collections.namedtuple('ColorJitterParams', 'order brightness contrast saturation hue', defaults=(None, None, None, None))


class ColorJitterParams(_Params):
    """One drawn ``ColorJitter``: ``order`` -- a permutation of a subset of ('brightness', 'contrast', 'saturation', 'hue'), the
    operations in the order they run -- and one factor each: brightness / contrast / saturation ``>= 0`` (1 leaves the image as it is),
    hue in ``[-0.5, 0.5]``.  A factor of ``None`` skips its operation (as a ``None`` range does in torchvision); a factor whose
    operation ``order`` does not name is refused."""
    __slots__ = ()

    def __new__(cls, order=(), brightness=None, contrast=None, saturation=None, hue=None):
        order = (order,) if isinstance(order, str) else tuple(order)
        if any(o not in OPS for o in order) or len(set(order)) != len(order):
            raise ValueError(f'order {order!r}: expected distinct names out of {OPS}')
        factors = []
        for name, f in zip(OPS, (brightness, contrast, saturation, hue)):
            if f is not None:
                f = float(f)
                if name not in order:
                    raise ValueError(f'{name} = {f} but order {order!r} does not name it')
                if name == 'hue' and not -0.5 <= f <= 0.5:          # also refuses NaN
                    raise ValueError(f'hue {f} outside [-0.5, 0.5]')
                if name != 'hue' and not 0.0 <= f < float('inf'):
                    raise ValueError(f'{name} {f}: expected a finite factor >= 0')
            factors.append(f)
        return super().__new__(cls, order, *factors)

    def steps(self):
        """[(name, factor)] of the operations that run, in order."""
        return [(name, getattr(self, name)) for name in self.order if getattr(self, name) is not None]


def hue_shift(h):
    """The byte added to H: ``int(h * 255)`` truncated toward zero, mod 256."""
    return int(float(h) * 255) % 256


def per_sample(params, b):
    """``params`` -- one ColorJitterParams for the batch or a sequence of ``b`` -- as a list of ``b`` ColorJitterParams."""
    if isinstance(params, _Params):
        params = [params] * b
    params = [p if isinstance(p, ColorJitterParams) else ColorJitterParams(*p) for p in params]
    if len(params) != b:
        raise ValueError(f'{len(params)} parameter sets for a batch of {b}')
    return params


def params_table(params, b):
    """int32 CPU tensor (b, TABLE_WORDS), the records hs_color_jitter_fwd reads: word 0 the order, 4 bits per operation from the lowest
    (1 brightness, 2 contrast, 3 saturation, 4 hue, 0 ends it); words 1-3 the float32 bits of the brightness, contrast and saturation
    factors; word 4 the hue shift; word 5 the operations present, bit ``code`` each; words 6-7 zero."""
    rec = np.zeros((b, TABLE_WORDS), dtype=np.int32)
    alphas = rec[:, 1:4].view(np.float32)
    for i, p in enumerate(per_sample(params, b)):
        for k, (name, f) in enumerate(p.steps()):
            code = OP_CODES[name]
            rec[i, 0] |= code << (4 * k)
            rec[i, 5] |= 1 << code
            if name == 'hue':
                rec[i, 4] = hue_shift(f)
            else:
                alphas[i, code - 1] = np.float32(f)
    return torch.from_numpy(rec)


# ------------------------------------------------------------------------------------------------------- pixel functions

def gray(r, g, b):
    """``convert('L')`` of integer tensors: int32."""
    return (19595 * r.to(torch.int32) + 38470 * g.to(torch.int32) + 7471 * b.to(torch.int32) + 0x8000) >> 16


def blend(a, b, alpha):
    """``Image.blend(a, b, alpha)`` of integer tensors (``a`` may be a Python int): int32 in [0, 255]."""
    alpha = torch.tensor(float(alpha), dtype=torch.float32)
    a = torch.as_tensor(a, dtype=torch.int32)
    d = (b.to(torch.int32) - a).to(torch.float32)               # exact
    t = a.to(torch.float32) + alpha * d                         # two roundings: the product, then the sum
    return t.clamp(0.0, 255.0).to(torch.int32)                  # (int): truncation


def rgb_to_hsv(r, g, b):
    """``convert('HSV')`` of integer tensors -> int32 (H, S, V).  float32 unless it says double."""
    r, g, b = (c.to(torch.int32) for c in (r, g, b))
    maxc, minc = torch.maximum(torch.maximum(r, g), b), torch.minimum(torch.minimum(r, g), b)
    colour = maxc != minc
    cr = torch.where(colour, maxc - minc, 1).to(torch.float32)          # 1: any divisor, the result is dropped
    s = cr / torch.where(colour, maxc, 1).to(torch.float32)
    rc, gc, bc = ((maxc - c).to(torch.float32) / cr for c in (r, g, b))
    h = torch.where(r == maxc, bc - gc,
                    torch.where(g == maxc, ((2.0 + rc.double()) - bc.double()).float(), ((4.0 + gc.double()) - rc.double()).float()))
    h = torch.fmod(h.double() / 6.0 + 1.0, 1.0).float()
    hh = (h.double() * 255.0).to(torch.int32).clamp(0, 255)
    ss = (s.double() * 255.0).to(torch.int32).clamp(0, 255)
    zero = torch.zeros_like(maxc)
    return torch.where(colour, hh, zero), torch.where(colour, ss, zero), maxc


def _round_half_away(x):
    """C's ``round`` for x >= 0, without the ``x + 0.5`` that rounds 0.49999999999999994 up."""
    fl = torch.floor(x)
    return fl + (x - fl >= 0.5)


def hsv_to_rgb(h, s, v):
    """``convert('RGB')`` of an HSV image, integer tensors -> int32 (R, G, B)."""
    h, s, v = (c.to(torch.int32) for c in (h, s, v))
    hd = h.double() * 6.0 / 255.0
    i = torch.floor(hd)
    f = (hd - i).float()
    sd = s.double() / 255.0
    fs = (sd * f.double()).float().double()
    vd = v.double()
    p = _round_half_away(vd * (1.0 - sd)).clamp(0, 255).to(torch.int32)
    q = _round_half_away(vd * (1.0 - fs)).clamp(0, 255).to(torch.int32)
    t = _round_half_away(vd * (1.0 - sd + fs)).clamp(0, 255).to(torch.int32)
    sector = i.to(torch.int32) % 6
    pick = lambda six: torch.stack(six).gather(0, sector[None].long())[0]
    r, g, b = pick((v, q, p, p, t, v)), pick((t, v, v, q, p, p)), pick((p, p, t, v, v, q))
    grey = s == 0
    return torch.where(grey, v, r), torch.where(grey, v, g), torch.where(grey, v, b)


def contrast_mean(r, g, b):
    """``int(ImageStat.Stat(img.convert('L')).mean[0] + 0.5)`` of ONE image: an integer sum, float64 division and addition."""
    lum = gray(r, g, b)
    return int(int(lum.sum(dtype=torch.int64)) / lum.numel() + 0.5)


def jitter_planes(r, g, b, params):
    """``params`` applied to ONE image given as three integer tensors of one shape -> int32 (R, G, B)."""
    r, g, b = (c.to(torch.int32) for c in (r, g, b))
    for name, f in params.steps():
        if name == 'brightness':
            r, g, b = (blend(0, c, f) for c in (r, g, b))
        elif name == 'contrast':
            m = contrast_mean(r, g, b)
            r, g, b = (blend(m, c, f) for c in (r, g, b))
        elif name == 'saturation':
            lum = gray(r, g, b)
            r, g, b = (blend(lum, c, f) for c in (r, g, b))
        else:
            h, s, v = rgb_to_hsv(r, g, b)
            r, g, b = hsv_to_rgb((h + hue_shift(f)) % 256, s, v)
    return r, g, b


def color_jitter_cpu(x_u8, params, layout='hwc', norm=None):
    """``functional.color_jitter`` on CPU tensors: uint8 frames (B, H, W, 3) / (B, 3, H, W) (``layout``), ``params`` one
    ColorJitterParams for the batch or a sequence of B -> uint8 in the input's layout, or with ``norm`` (an ``InputNorm``) the float32
    (B, 3, H, W) image looked up in its table."""
    if layout not in ('hwc', 'chw'):
        raise ValueError(f"layout {layout!r}: expected 'hwc' or 'chw'")
    if not isinstance(x_u8, torch.Tensor) or x_u8.dtype != torch.uint8 or x_u8.dim() != 4 or x_u8.shape[3 if layout == 'hwc' else 1] != 3:
        raise ValueError(f'frames must be uint8 {"(B, H, W, 3)" if layout == "hwc" else "(B, 3, H, W)"}, got '
                         f'{getattr(x_u8, "dtype", type(x_u8))} {tuple(getattr(x_u8, "shape", ()))}')
    if norm is not None and norm.layout != layout:
        raise ValueError(f"norm describes '{norm.layout}' frames, these are '{layout}'")
    if x_u8.shape[0] == 0 or x_u8.numel() == 0:
        raise ValueError('empty batch')
    params = per_sample(params, x_u8.shape[0])
    chw = (x_u8.permute(0, 3, 1, 2) if layout == 'hwc' else x_u8).cpu()
    out = torch.stack([torch.stack(jitter_planes(img[0], img[1], img[2], p)) for img, p in zip(chw, params)])
    if norm is not None:
        table = norm.table('cpu')
        return torch.stack([table[c][out[:, c].long()] for c in range(3)], 1).contiguous()
    out = out.to(torch.uint8)
    return (out.permute(0, 2, 3, 1) if layout == 'hwc' else out).contiguous()
