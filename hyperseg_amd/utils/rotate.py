"""Pillow's rotation as data: the per-sample coefficient tables the device kernels read (csrc/hs_rotate.hip), and the whole operation on
the CPU from the same tables.  The reference's VOC train chain rotates the PIL frame and its label with ``RandomRotation``
(datasets/seg_transforms.py:384-426), i.e. ``PIL.Image.rotate(angle, resample, expand=False)`` about the centre -- BICUBIC for the frame,
NEAREST for the label -- and pads the result right and bottom with ``ConstantPad`` (:181-217).  The arithmetic is restated here (Python
and numpy float64 for the frame, integers for the label); Pillow is not imported.  Results equal Pillow's byte for byte
(tests/test_rotate_cpu.py, tests/golden/rotate_ref.npz).

Matrix, ``rotation_matrix(h, w, angle)`` -- Python float64, as ``Image.rotate`` builds it: ``angle %= 360.0``; ``r = -radians(angle)``;
``m = [round(cos r, 15), round(sin r, 15), 0, round(-sin r, 15), round(cos r, 15), 0]``; with ``cx = w / 2``, ``cy = h / 2``:
``m[2] = (m[0] (-cx) + m[1] (-cy)) + m[2]`` then ``m[2] += cx``; ``m[5] = (m[3] (-cx) + m[4] (-cy)) + m[5]`` then ``m[5] += cy``.  Pillow
answers 0, 180 and (square images) 90 / 270 degrees with a transpose; the formulas below give the same bytes there -- the coordinates are
integers and ``d = 0`` -- so there is one code path.

Frame, BICUBIC (Pillow's ImagingGenericTransform with its bicubic filter, ``a = -1``), float64, per output pixel (x, y) and channel:
  * ``xi = x + 0.5``, ``yi = y + 0.5``; ``xin = (m0 xi + m1 yi) + m2``, ``yin = (m3 xi + m4 yi) + m5``, in that association;
  * ``xin < 0 or xin >= W or yin < 0 or yin >= H``: the pixel is the rotation fill;
  * ``xin -= 0.5; yin -= 0.5; x0 = floor(xin); y0 = floor(yin); dx = xin - x0; dy = yin - y0; x0 -= 1; y0 -= 1``;
  * the four columns are ``clamp(x0 + k, 0, W - 1)``; ``cubic(v1, v2, v3, v4, d) = v2 + d (p2 + d (p3 + d p4))`` with ``p2 = -v1 + v3``,
    ``p3 = ((2 (v1 - v2)) + v3) - v4``, ``p4 = ((-v1 + v2) - v3) + v4``;
  * row 0 is taken at ``clamp(y0, 0, H - 1)``; rows 1..3 at ``y0 + k`` where that lies in ``[0, H)``, OTHERWISE THE VALUE IS THE PREVIOUS
    ROW'S HORIZONTAL RESULT -- Pillow does not read again (the rows being consecutive, it is the value a clamped read would give);
  * ``v`` = the vertical ``cubic`` of the four row results with ``dy``; the byte is 0 for ``v <= 0``, 255 for ``v >= 255``, else the
    TRUNCATION ``uint8(v)``: no ``+ 0.5``, unlike the resize.
The row results are not integers: the order of operations above is the result.

Label, NEAREST (Pillow's 16.16 fixed-point affine path), integers, ``nearest_fixed(m)``: ``FIX(v) = floor(v 65536 + 0.5)``;
``a0, a1, a3, a4 = FIX(m0), FIX(m1), FIX(m3), FIX(m4)``; ``a2 = FIX(m2 + m0 0.5 + m1 0.5)``; ``a5 = FIX(m5 + m3 0.5 + m4 0.5)``;
``xs = (a2 + y a1 + x a0) >> 16``, ``ys = (a5 + y a4 + x a3) >> 16`` (arithmetic shifts); the source pixel where ``0 <= xs < W and
0 <= ys < H``, else the fill.  Pillow accumulates these sums in 32-bit ints; up to ``MAX_DIM`` = 8192 per dimension no intermediate
leaves int32 and the closed form equals the accumulation, so larger images are refused.

The pad is a *view*: the output is ``size`` = (Ho, Wo) >= (H, W) with the rotated image at offset (0, 0) and ``pad_fill`` right of and
below it (``ConstantPad`` never crops)."""
import math

import numpy as np
import torch

MAX_DIM = 8192
TABLE_WORDS = 6


def _check_hw(h, w):
    h, w = int(h), int(w)
    if h < 1 or w < 1:
        raise ValueError(f'sizes must be >= 1, got {(h, w)}')
    if h > MAX_DIM or w > MAX_DIM:
        raise ValueError(f'rotation takes images up to {MAX_DIM} x {MAX_DIM} (Pillow\'s 32-bit label arithmetic), got {(h, w)}')
    return h, w


def rotation_matrix(h, w, angle):
    """The six float64 coefficients ``Image.rotate(angle)`` hands to its affine transform for an (h, w) image -- module docstring."""
    h, w = _check_hw(h, w)
    angle = float(angle) % 360.0
    r = -math.radians(angle)
    m = [round(math.cos(r), 15), round(math.sin(r), 15), 0.0, round(-math.sin(r), 15), round(math.cos(r), 15), 0.0]
    cx, cy = w / 2.0, h / 2.0
    m[2] = m[0] * (-cx) + m[1] * (-cy) + m[2]
    m[2] += cx
    m[5] = m[3] * (-cx) + m[4] * (-cy) + m[5]
    m[5] += cy
    return tuple(m)


def _fix(v):
    return int(math.floor(v * 65536.0 + 0.5))


def nearest_fixed(m):
    """The six 16.16 integers of Pillow's NEAREST affine path for matrix ``m`` -- module docstring."""
    m = [float(v) for v in m]
    if len(m) != TABLE_WORDS:
        raise ValueError(f'a matrix has {TABLE_WORDS} coefficients, got {len(m)}')
    return (_fix(m[0]), _fix(m[1]), _fix(m[2] + m[0] * 0.5 + m[1] * 0.5), _fix(m[3]), _fix(m[4]), _fix(m[5] + m[3] * 0.5 + m[4] * 0.5))


def per_sample(angle, b):
    """``angle`` -- one value or a sequence of B -- as a list of B floats."""
    if isinstance(angle, torch.Tensor):
        angle = angle.tolist()
    elif isinstance(angle, np.ndarray):
        angle = angle.tolist()
    angles = [float(angle)] * b if not isinstance(angle, (list, tuple)) else [float(a) for a in angle]
    if len(angles) != b:
        raise ValueError(f'angle takes one value, or one per sample ({b}), got {len(angles)}')
    return angles


def matrix_table(h, w, angle, b):
    """float64 CPU tensor (B, 6): ``rotation_matrix`` per sample -- what ``functional.frame_rotate(table=)`` reads on the device."""
    return torch.tensor([rotation_matrix(h, w, a) for a in per_sample(angle, b)], dtype=torch.float64).reshape(b, TABLE_WORDS)


def fixed_table(h, w, angle, b):
    """int32 CPU tensor (B, 6): ``nearest_fixed(rotation_matrix(...))`` per sample -- what ``functional.label_rotate(table=)`` reads."""
    rows = [nearest_fixed(rotation_matrix(h, w, a)) for a in per_sample(angle, b)]
    return torch.tensor(rows, dtype=torch.int64).to(torch.int32).reshape(b, TABLE_WORDS)


def check_size(size, h, w):
    """``size`` (the padded (Ho, Wo), None = the input's own) as plain ints; it may not crop."""
    if size is None:
        return h, w
    ho, wo = (int(s) for s in size)
    if ho < h or wo < w:
        raise ValueError(f'the rotated image {(h, w)} exceeds the padded size {(ho, wo)}: ConstantPad never crops')
    if ho > MAX_DIM or wo > MAX_DIM:
        raise ValueError(f'the padded size may be up to {MAX_DIM} x {MAX_DIM}, got {(ho, wo)}')
    return ho, wo


def check_fill(fill, name='fill'):
    fill = tuple(int(f) for f in (fill if isinstance(fill, (tuple, list)) else (fill,) * 3))
    if len(fill) != 3 or any(not 0 <= f <= 255 for f in fill):
        raise ValueError(f'{name} must be 3 bytes, got {fill!r}')
    return fill


def check_table(table, b, dtype, device):
    if (not isinstance(table, torch.Tensor) or table.dtype != dtype or tuple(table.shape) != (b, TABLE_WORDS)
            or table.device != device or not table.is_contiguous()):
        raise ValueError(f'table must be a contiguous {dtype} tensor of shape {(b, TABLE_WORDS)} on {device}')
    return table


# ---------------------------------------------------------------------------------------------------------------- CPU

def _cubic(v1, v2, v3, v4, d):
    p2 = -v1 + v3
    p3 = ((2.0 * (v1 - v2)) + v3) - v4
    p4 = ((-v1 + v2) - v3) + v4
    return v2 + d * (p2 + d * (p3 + d * p4))


def _rotate_planes(src, m, fill):
    """uint8 ``src`` (C, H, W) rotated by matrix ``m``: uint8 (C, H, W), the arithmetic of the module docstring."""
    c, h, w = src.shape
    m0, m1, m2, m3, m4, m5 = (np.float64(v) for v in m)
    yi, xi = np.meshgrid(np.arange(h, dtype=np.float64) + 0.5, np.arange(w, dtype=np.float64) + 0.5, indexing='ij')
    with np.errstate(invalid='ignore', over='ignore'):
        xin = (m0 * xi + m1 * yi) + m2
        yin = (m3 * xi + m4 * yi) + m5
        inside = (xin >= 0.0) & (xin < w) & (yin >= 0.0) & (yin < h)
        xin = np.where(inside, xin, 0.5) - 0.5          # what lies outside is overwritten below; keep its indices tame
        yin = np.where(inside, yin, 0.5) - 0.5
    fx, fy = np.floor(xin), np.floor(yin)
    dx, dy = xin - fx, yin - fy
    x0, y0 = fx.astype(np.int64) - 1, fy.astype(np.int64) - 1
    cols = [np.clip(x0 + k, 0, w - 1) for k in range(4)]
    f = src.astype(np.float64)
    rows = []
    for k in range(4):
        ry = y0 + k
        taken = np.clip(ry, 0, h - 1)
        val = _cubic(*(f[:, taken, cols[j]] for j in range(4)), dx)
        if k > 0:
            val = np.where((ry >= 0) & (ry < h), val, rows[k - 1])      # the previous row's horizontal result
        rows.append(val)
    v = _cubic(rows[0], rows[1], rows[2], rows[3], dy)
    byte = np.where(v <= 0.0, 0.0, np.where(v >= 255.0, 255.0, np.trunc(v))).astype(np.uint8)
    return np.where(inside, byte, np.asarray(fill, dtype=np.uint8).reshape(c, 1, 1))


def _check_frames(x_u8, layout):
    if layout not in ('hwc', 'chw'):
        raise ValueError(f"layout {layout!r}: expected 'hwc' or 'chw'")
    if not isinstance(x_u8, torch.Tensor) or x_u8.dtype != torch.uint8 or x_u8.dim() != 4 or x_u8.shape[3 if layout == 'hwc' else 1] != 3:
        raise ValueError(f'frames must be uint8 {"(B, H, W, 3)" if layout == "hwc" else "(B, 3, H, W)"}, got '
                         f'{getattr(x_u8, "dtype", type(x_u8))} {tuple(getattr(x_u8, "shape", ()))}')
    if x_u8.shape[0] == 0:
        raise ValueError('empty batch')
    return _check_hw(*(x_u8.shape[1:3] if layout == 'hwc' else x_u8.shape[2:]))


def _check_labels(t):
    if not isinstance(t, torch.Tensor) or t.dtype not in (torch.uint8, torch.int64) or t.dim() != 3:
        raise ValueError(f'labels must be uint8 or int64 (B, H, W), got {getattr(t, "dtype", type(t))} {tuple(getattr(t, "shape", ()))}')
    if t.shape[0] == 0:
        raise ValueError('empty batch')
    return _check_hw(*t.shape[1:])


def frame_rotate_cpu(x_u8, angle, layout='hwc', size=None, fill=(0, 0, 0), pad_fill=(0, 0, 0), norm=None, table=None):
    """``functional.frame_rotate`` on CPU tensors: uint8 frames (B, H, W, 3) / (B, 3, H, W) rotated by ``angle`` (one value or B; or
    ``table``, a float64 (B, 6) tensor of matrices -- ``angle`` is then not read) with ``fill`` where the rotation looks outside the frame,
    then padded right and bottom to ``size`` with ``pad_fill``; uint8 in the input's layout, or with ``norm`` (an ``InputNorm``) float32
    (B, 3, Ho, Wo) through its table."""
    h, w = _check_frames(x_u8, layout)
    b = x_u8.shape[0]
    ho, wo = check_size(size, h, w)
    fill, pad_fill = check_fill(fill), check_fill(pad_fill, 'pad_fill')
    if norm is not None and norm.layout != layout:
        raise ValueError(f"norm describes '{norm.layout}' frames, these are '{layout}'")
    table = matrix_table(h, w, angle, b) if table is None else check_table(table, b, torch.float64, x_u8.device)
    a = x_u8.cpu().numpy()
    chw = a.transpose(0, 3, 1, 2) if layout == 'hwc' else a
    out = np.empty((b, 3, ho, wo), dtype=np.uint8)
    out[:] = np.asarray(pad_fill, dtype=np.uint8).reshape(1, 3, 1, 1)
    for i in range(b):
        out[i, :, :h, :w] = _rotate_planes(chw[i], table[i].tolist(), fill)
    if norm is None:
        return torch.from_numpy(np.ascontiguousarray(out.transpose(0, 2, 3, 1) if layout == 'hwc' else out))
    idx = torch.from_numpy(out).long()
    lut = norm.table('cpu')
    return torch.stack([lut[c][idx[:, c]] for c in range(3)], 1).contiguous()


def label_rotate_cpu(t, angle, size=None, fill=0, pad_fill=255, out_dtype=None, table=None):
    """``functional.label_rotate`` on CPU tensors: labels (B, H, W), uint8 or int64, rotated by ``angle`` (or ``table``, an int32 (B, 6)
    tensor of ``nearest_fixed`` rows) with ``fill`` outside, padded right and bottom to ``size`` with ``pad_fill``."""
    h, w = _check_labels(t)
    b = t.shape[0]
    ho, wo = check_size(size, h, w)
    table = fixed_table(h, w, angle, b) if table is None else check_table(table, b, torch.int32, t.device)
    a = t.cpu().numpy().astype(np.int64)
    out = np.full((b, ho, wo), int(pad_fill), dtype=np.int64)
    y, x = np.meshgrid(np.arange(h, dtype=np.int64), np.arange(w, dtype=np.int64), indexing='ij')
    for i in range(b):
        a0, a1, a2, a3, a4, a5 = table[i].tolist()
        xs = (a2 + y * a1 + x * a0) >> 16
        ys = (a5 + y * a4 + x * a3) >> 16
        inside = (xs >= 0) & (xs < w) & (ys >= 0) & (ys < h)
        out[i, :h, :w] = np.where(inside, a[i][np.clip(ys, 0, h - 1), np.clip(xs, 0, w - 1)], int(fill))
    return torch.from_numpy(out).to(out_dtype or t.dtype)
