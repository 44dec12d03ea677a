"""Pillow's ``ImageFilter.GaussianBlur`` on uint8 RGB frames as data and arithmetic: what the device kernels compute
(csrc/hs_blur.hip) and the whole operation on the CPU.  The reference's ``RandomGaussianBlur`` (hyperseg/datasets/seg_transforms.py:
361-378) is ``img.filter(ImageFilter.GaussianBlur(radius=r))`` on the PIL image, default ``r = 5``, image only.  Pillow's filter is an
EXTENDED BOX BLUR: three box passes along the rows, then three along the columns, every pass reading and writing bytes.  The arithmetic
is restated here; Pillow is not imported.  Results equal Pillow's byte for byte (tests/test_gaussian_blur_cpu.py,
tests/golden/gaussian_blur_ref.npz).

  * the box radius ``fr`` of a Gaussian ``sigma`` (Pillow calls it ``radius``), every step rounded to float32: ``sigma2 = sigma *
    sigma / 3``, ``L = sqrt(12 sigma2 + 1)``, ``l = floor((L - 1) / 2)``, ``a = (2 l + 1) (l (l + 1) - 3 sigma2) / (6 (sigma2 - (l + 1)^2))``,
    ``fr = l + a``; ``r = int(fr)``.
  * the two weights: ``ww = uint32(float32(2^24) / (float32(fr) * 2 + 1))`` -- a float32 quotient: at sigma 1, ``fr = 0.25`` and ``ww`` is
    11184811 where a float64 quotient truncates to 11184810 -- and ``fw = (2^24 - (2 r + 1) ww) / 2`` in integers.
  * one pass along a line of ``n`` pixels, indices clamped to ``[0, n - 1]`` (also when the radius exceeds the line):
    ``out[x] = (ww * sum(in[clamp(x + d)] for |d| <= r) + fw * (in[clamp(x - r - 1)] + in[clamp(x + r + 1)]) + 2^23) >> 24``.
    Everything fits 32 unsigned bits: ``(2 r + 1) ww + 2 fw <= 2^24``.  The clamp applies to each pass's own input, the output of the
    pass before.
  * sigma 0 gives ``r = 0``, ``ww = 2^24``, ``fw = 0``: a copy.

The device reads one record of ``TABLE_WORDS`` int32 words per sample (:func:`params_table`): apply flag, ``r``, ``ww``, ``fw``."""
import collections

import numpy as np
import torch

TABLE_WORDS = 4
MAX_RADIUS = 15                          # HS_BLUR_MAX_RADIUS of include/hyperseg_hip.h: the largest box radius r the device kernels take

_Params = collections.namedtuple('GaussianBlurParams', 'radius apply', defaults=(True,))


class GaussianBlurParams(_Params):
    """One drawn ``RandomGaussianBlur``: ``radius`` -- ``ImageFilter.GaussianBlur``'s, the Gaussian's sigma in pixels, finite and
    ``>= 0`` -- and ``apply``: False leaves the image as it is (the transform did not fire)."""
    __slots__ = ()

    def __new__(cls, radius, apply=True):
        radius = float(radius)
        if not 0.0 <= radius < float('inf'):                    # also refuses NaN
            raise ValueError(f'radius {radius}: expected a finite value >= 0')
        return super().__new__(cls, radius, bool(apply))


def box_radius(sigma):
    """The extended box blur's fractional radius ``fr`` of a Gaussian ``sigma``, in float32 arithmetic; returned as a Python float that
    holds the float32 value."""
    f = np.float32
    sigma = f(sigma)
    sigma2 = f(f(sigma * sigma) / f(3))
    big_l = f(np.sqrt(f(f(f(12) * sigma2) + f(1))))
    l = f(np.floor(f(f(big_l - f(1)) / f(2))))
    num = f(f(f(f(2) * l) + f(1)) * f(f(l * f(l + f(1))) - f(f(3) * sigma2)))
    den = f(f(6) * f(sigma2 - f(f(l + f(1)) * f(l + f(1)))))
    return float(f(l + f(num / den)))


def weights(sigma):
    """``(r, ww, fw)`` of a Gaussian ``sigma``: the integer box radius and the two 8.24 fixed-point weights of one pass."""
    fr = np.float32(box_radius(sigma))
    r = int(fr)
    ww = int(np.float32(1 << 24) / np.float32(np.float32(fr * np.float32(2)) + np.float32(1)))
    fw = ((1 << 24) - (2 * r + 1) * ww) // 2
    return r, ww, fw


def per_sample(params, b):
    """``params`` -- one GaussianBlurParams for the batch or a sequence of ``b``, a ``None`` among them standing for a sample that is
    not blurred -- as a list of ``b`` GaussianBlurParams."""
    if isinstance(params, _Params):
        params = [params] * b
    if params is None or isinstance(params, (int, float, str)):
        raise ValueError(f'blur parameters must be a GaussianBlurParams or a sequence of {b}, got {params!r}')
    params = [GaussianBlurParams(0.0, False) if p is None else p if isinstance(p, GaussianBlurParams) else GaussianBlurParams(*p)
              for p in params]
    if len(params) != b:
        raise ValueError(f'{len(params)} parameter sets for a batch of {b}')
    return params


def params_table(params, b):
    """int32 CPU tensor (b, TABLE_WORDS), the records hs_gaussian_blur_fwd reads: word 0 the apply flag, word 1 ``r``, word 2 ``ww``,
    word 3 ``fw`` (:func:`weights`).  A radius the device kernels do not take (``r > MAX_RADIUS``) is recorded as it is: the functional
    layer refuses it on the host, the kernel declines it through its status word."""
    rec = np.zeros((b, TABLE_WORDS), dtype=np.int32)
    for i, p in enumerate(per_sample(params, b)):
        rec[i] = (int(p.apply),) + weights(p.radius)
    return torch.from_numpy(rec)


def box_pass(x, r, ww, fw, dim):
    """One pass along ``dim`` of an integer tensor of bytes: int64 in [0, 255]."""
    x = x.to(torch.int64)
    n = x.shape[dim]
    at = lambda d: x.index_select(dim, (torch.arange(n) + d).clamp(0, n - 1))
    inner = sum(at(d) for d in range(-r, r + 1))
    return (ww * inner + fw * (at(-r - 1) + at(r + 1)) + (1 << 23)) >> 24


def blur_planes(img, record):
    """One record ``(apply, r, ww, fw)`` applied to ONE image given as an integer tensor (..., H, W): three passes along W, then three
    along H -> int64."""
    img = img.to(torch.int64)
    apply, r, ww, fw = (int(v) for v in record)
    if not apply:
        return img
    for dim in (-1, -2):
        for _ in range(3):
            img = box_pass(img, r, ww, fw, dim)
    return img


def gaussian_blur_cpu(x_u8, params, layout='hwc', norm=None, table=None):
    """``functional.gaussian_blur`` on CPU tensors: uint8 frames (B, H, W, 3) / (B, 3, H, W) (``layout``), ``params`` one
    GaussianBlurParams for the batch or a sequence of B -> uint8 in the input's layout, or with ``norm`` (an ``InputNorm``) the float32
    (B, 3, H, W) image looked up in its table.  ``table``: the records themselves, int32 (B, TABLE_WORDS) as :func:`params_table` makes
    them; ``params`` is then not read.  Any radius: the device kernels' bound does not apply here."""
    if layout not in ('hwc', 'chw'):
        raise ValueError(f"layout {layout!r}: expected 'hwc' or 'chw'")
    if not isinstance(x_u8, torch.Tensor) or x_u8.dtype != torch.uint8 or x_u8.dim() != 4 or x_u8.shape[3 if layout == 'hwc' else 1] != 3:
        raise ValueError(f'frames must be uint8 {"(B, H, W, 3)" if layout == "hwc" else "(B, 3, H, W)"}, got '
                         f'{getattr(x_u8, "dtype", type(x_u8))} {tuple(getattr(x_u8, "shape", ()))}')
    if norm is not None and norm.layout != layout:
        raise ValueError(f"norm describes '{norm.layout}' frames, these are '{layout}'")
    if x_u8.shape[0] == 0 or x_u8.numel() == 0:
        raise ValueError('empty batch')
    if table is None:
        table = params_table(params, x_u8.shape[0])
    elif not isinstance(table, torch.Tensor) or table.dtype != torch.int32 or tuple(table.shape) != (x_u8.shape[0], TABLE_WORDS):
        raise ValueError(f'table must be an int32 tensor of shape {(x_u8.shape[0], TABLE_WORDS)}')
    chw = (x_u8.permute(0, 3, 1, 2) if layout == 'hwc' else x_u8).cpu()
    out = torch.stack([blur_planes(img, record) for img, record in zip(chw, table.tolist())])
    if norm is not None:
        table = norm.table('cpu')
        return torch.stack([table[c][out[:, c]] for c in range(3)], 1).contiguous()
    out = out.to(torch.uint8)
    return (out.permute(0, 2, 3, 1) if layout == 'hwc' else out).contiguous()
