"""Pillow's 8-bit resize as data: the coefficient and index tables the device kernels read (csrc/hs_resample.hip), and the whole
operation on the CPU from the same tables.  The reference's Cityscapes configs resize the camera frame with
``torchvision.transforms.Resize`` on a PIL image, i.e. ``PIL.Image.resize`` -- an antialiased two-pass resample with 8-bit
intermediates and 22-bit fixed-point weights -- and its train chain (datasets/seg_transforms.py:224-334) resizes, pads, crops and
flips with Pillow as well.  The arithmetic is restated here (numpy float64 for the weights, integers for the pixels); Pillow is
not imported.  Results equal Pillow's byte for byte (tests/test_resample_cpu.py, tests/golden/resample_ref.npz).

Tables, per axis:
  * ``resample_coeffs(in, out, filter)`` -> ``bounds`` int32 (out, 2) = (first source index, taps) and ``kk`` int32 (out, ksize),
    zero-padded: ``scale = in / out``, ``filterscale = max(scale, 1)``, ``support = filter_support * filterscale``,
    ``ksize = 2 ceil(support) + 1``; per output index ``center = (i + 0.5) scale``, ``xmin = max(int(center - support + 0.5), 0)``,
    ``n = min(int(center + support + 0.5), in) - xmin``; weights ``filter((x + xmin - center + 0.5) * (1 / filterscale))`` in float64,
    divided by their sequential sum, quantised ``int(+-0.5 + w 2^22)``.  A pixel is ``clip8((2^21 + sum px kk) >> 22)``.  An axis whose
    size does not change is the identity (Pillow skips that pass): one tap of weight 2^22.
  * ``nearest_index(in, out)``: Pillow accumulates ``xo = 0.5 a; index = int(xo); xo += a`` in float64 (``a = in / out``), which is NOT
    ``floor((i + 0.5) a)`` for every i; the table is built by that accumulation, clamped to ``in - 1``.

A *view* (:class:`ResizeView`) selects what is produced from the resized image (Hr, Wr): output pixel (y, x) of size (Ho, Wo) is resized
pixel ``(oy + y, ox + (Wo - 1 - x if hflip else x))``, or ``fill`` where that lies outside -- resize -> pad -> crop -> flip of the train
chain without resampling what the crop throws away.

For a training batch whose samples each draw a scale the device builds the same tables itself, the window of them that the crop reads
(csrc/hs_resample_batch.hip, ``functional.resize_tables``): :func:`window_tables_cpu` is that layout from the host tables, its oracle,
and :func:`ks_for` the row width for a range of scales."""
import collections
import functools
import math
import threading

import numpy as np
import torch

PRECISION_BITS = 32 - 8 - 2          # Pillow's 8-bit path: weights carry 22 fractional bits
FILTERS = ('bilinear', 'bicubic')
_SUPPORT = {'bilinear': 1.0, 'bicubic': 2.0}

ResizeView = collections.namedtuple('ResizeView', 'size offset hflip fill', defaults=((0, 0), False, (0, 0, 0)))
ResizeView.__doc__ = """``size`` (Ho, Wo) of the output, ``offset`` (oy, ox) of its top-left pixel in the resized image (signed), ``hflip``,
``fill`` (3 bytes; frames only -- labels take their own fill)."""


def _bilinear(x):
    x = np.abs(x)
    return np.where(x < 1.0, 1.0 - x, 0.0)


def _bicubic(x):
    a = -0.5
    x = np.abs(x)
    near = ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    far = (((x - 5) * x + 8) * x - 4) * a
    return np.where(x < 1.0, near, np.where(x < 2.0, far, 0.0))


_FILTER_FN = {'bilinear': _bilinear, 'bicubic': _bicubic}


def _check_sizes(in_size, out_size):
    in_size, out_size = int(in_size), int(out_size)
    if in_size < 1 or out_size < 1:
        raise ValueError(f'sizes must be >= 1, got {in_size} -> {out_size}')
    return in_size, out_size


@functools.lru_cache(maxsize=256)
def resample_coeffs(in_size, out_size, filter='bilinear'):
    """``(bounds, kk)``: int32 CPU tensors (out, 2) and (out, ksize) -- module docstring.  Cached; treat them as read-only."""
    in_size, out_size = _check_sizes(in_size, out_size)
    if filter not in FILTERS:
        raise ValueError(f'filter {filter!r}: expected one of {FILTERS}')
    if in_size == out_size:          # the pass Pillow skips
        bounds = np.stack((np.arange(out_size), np.ones(out_size, dtype=np.int64)), 1).astype(np.int32)
        kk = np.full((out_size, 1), 1 << PRECISION_BITS, dtype=np.int32)
        return torch.from_numpy(bounds), torch.from_numpy(kk)
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = _SUPPORT[filter] * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    center = (np.arange(out_size, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)          # C's (int): truncation; negatives clamp to 0 either way
    xmax = np.minimum((center + support + 0.5).astype(np.int64), in_size) - xmin
    w = np.zeros((out_size, ksize), dtype=np.float64)
    ww = np.zeros(out_size, dtype=np.float64)
    fn = _FILTER_FN[filter]
    for x in range(ksize):
        col = np.where(x < xmax, fn((x + xmin - center + 0.5) * ss), 0.0)
        w[:, x] = col
        ww = ww + col                # the sequential sum, tap by tap
    w = np.where(ww[:, None] != 0.0, w / np.where(ww == 0.0, 1.0, ww)[:, None], w)
    kk = np.where(w < 0, -0.5 + w * (1 << PRECISION_BITS), 0.5 + w * (1 << PRECISION_BITS)).astype(np.int64)      # (int): truncation
    # the kernels accumulate in int32: 255 * sum |kk| + 2^21 stays below 2^31 for both filters at every scale
    assert int(np.abs(kk).sum(1).max()) * 255 + (1 << (PRECISION_BITS - 1)) < 2 ** 31
    bounds = np.stack((xmin, xmax), 1).astype(np.int32)
    return torch.from_numpy(bounds), torch.from_numpy(kk.astype(np.int32))


@functools.lru_cache(maxsize=256)
def nearest_index(in_size, out_size):
    """int32 CPU tensor (out,): the source index of every output index of Pillow's NEAREST resize.  Cached; read-only."""
    in_size, out_size = _check_sizes(in_size, out_size)
    a = in_size / out_size
    idx = np.empty(out_size, dtype=np.int64)
    xo = 0.5 * a
    for i in range(out_size):
        idx[i] = int(xo)
        xo += a
    return torch.from_numpy(np.minimum(idx, in_size - 1).astype(np.int32))


def nearest_index_closed_form(in_size, out_size):
    """``floor((i + 0.5) in / out)``: what Pillow's table is NOT (kept for the test that pins the difference)."""
    a = in_size / out_size
    return torch.from_numpy(np.minimum(np.floor((np.arange(out_size) + 0.5) * a).astype(np.int64), in_size - 1).astype(np.int32))


def ks_for(filter, min_scale):
    """The widest ``kk`` row of ``resample_coeffs(in, out, filter)`` for resize factors ``out / in >= min_scale``:
    ``2 ceil(support / min(min_scale, 1)) + 1`` -- the ``ks_max`` of the device-built tables (``functional.resize_tables``)."""
    if filter not in FILTERS:
        raise ValueError(f'filter {filter!r}: expected one of {FILTERS}')
    min_scale = float(min_scale)
    if not min_scale > 0.0:
        raise ValueError(f'min_scale must be > 0, got {min_scale}')
    return int(math.ceil(_SUPPORT[filter] / min(min_scale, 1.0))) * 2 + 1


def ksize_of(in_size, out_size, filter):
    """Columns of ``resample_coeffs(in_size, out_size, filter)``'s ``kk`` without building it."""
    in_size, out_size = _check_sizes(in_size, out_size)
    return 1 if in_size == out_size else int(math.ceil(_SUPPORT[filter] * max(in_size / out_size, 1.0))) * 2 + 1


WindowTables = collections.namedtuple('WindowTables', 'bounds kk nearest')


def window_tables_cpu(in_size, out_size, start, extent, filter, ks_max):
    """Rows ``start .. start + extent - 1`` of the host tables of one axis in the layout the device builds (csrc/hs_resample_batch.hip;
    its oracle): ``bounds`` int32 (extent, 2), ``kk`` int32 (extent, ks_max) zero-padded, ``nearest`` int32 (extent,).  Row j is
    resized index ``start + j``; a row outside ``[0, out_size)`` is (0, 0), zeros and 0."""
    in_size, out_size = _check_sizes(in_size, out_size)
    start, extent, ks_max = int(start), int(extent), int(ks_max)
    if extent < 1:
        raise ValueError(f'extent must be >= 1, got {extent}')
    b, k = resample_coeffs(in_size, out_size, filter)
    if k.shape[1] > ks_max:
        raise ValueError(f'{in_size} -> {out_size} {filter} has {k.shape[1]} taps, ks_max is {ks_max}')
    near = nearest_index(in_size, out_size)
    bounds = torch.zeros(extent, 2, dtype=torch.int32)
    kk = torch.zeros(extent, ks_max, dtype=torch.int32)
    nearest = torch.zeros(extent, dtype=torch.int32)
    lo, hi = max(start, 0), min(start + extent, out_size)
    if lo < hi:
        bounds[lo - start:hi - start] = b[lo:hi]
        kk[lo - start:hi - start, :k.shape[1]] = k[lo:hi]
        nearest[lo - start:hi - start] = near[lo:hi]
    return WindowTables(bounds, kk, nearest)


_DEVICE_TABLES = {}
_LOCK = threading.Lock()


def _on_device(key, build, device):
    device = torch.device(device)
    if device.type == 'cuda' and device.index is None:
        device = torch.device('cuda', torch.cuda.current_device())
    with _LOCK:
        hit = _DEVICE_TABLES.get((key, device))
        if hit is None:
            hit = tuple(t.to(device).contiguous() for t in build())
            if device.type == 'cuda' and not torch.cuda.is_current_stream_capturing():
                torch.cuda.current_stream(device).synchronize()      # other streams (a capture's side stream, replicas) may read them next
            _DEVICE_TABLES[(key, device)] = hit
    return hit


def device_coeffs(in_size, out_size, filter, device):
    """``resample_coeffs`` on ``device`` (uploaded once per (in, out, filter, device))."""
    return _on_device(('coeffs', int(in_size), int(out_size), filter), lambda: resample_coeffs(int(in_size), int(out_size), filter), device)


def device_nearest(in_size, out_size, device):
    return _on_device(('nearest', int(in_size), int(out_size)), lambda: (nearest_index(int(in_size), int(out_size)),), device)[0]


def check_view(view, resized):
    """``view`` (a :class:`ResizeView`, a tuple of its fields, or None = the identity) -> ResizeView with plain ints."""
    if view is None:
        return ResizeView((int(resized[0]), int(resized[1])))
    view = ResizeView(*view)
    ho, wo = (int(s) for s in view.size)
    oy, ox = (int(s) for s in view.offset)
    if ho < 1 or wo < 1:
        raise ValueError(f'view size must be >= 1, got {(ho, wo)}')
    fill = tuple(int(f) for f in (view.fill if isinstance(view.fill, (tuple, list)) else (view.fill,) * 3))
    if len(fill) != 3 or any(not 0 <= f <= 255 for f in fill):
        raise ValueError(f'view fill must be 3 bytes, got {view.fill!r}')
    return ResizeView((ho, wo), (oy, ox), bool(view.hflip), fill)


# ---------------------------------------------------------------------------------------------------------------- CPU

def _pass(src, bounds, kk, axis):
    """One resample pass over ``axis`` of uint8 ``src`` (numpy): int64 accumulation, Pillow's rounding and clip8."""
    src = np.moveaxis(src, axis, 0)
    xmin, n = bounds[:, 0].astype(np.int64), bounds[:, 1].astype(np.int64)
    acc = np.full((bounds.shape[0],) + src.shape[1:], 1 << (PRECISION_BITS - 1), dtype=np.int64)
    tail = (1,) * (src.ndim - 1)
    for k in range(kk.shape[1]):
        live = k < n
        if not live.any():
            break
        idx = np.minimum(xmin + k, src.shape[0] - 1)
        acc += src[idx].astype(np.int64) * np.where(live, kk[:, k].astype(np.int64), 0).reshape((-1,) + tail)
    out = np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)
    return np.moveaxis(out, 0, axis)


def _apply_view(resized, view, fill, y_axis, x_axis):
    """``view`` of ``resized`` (numpy): rows / columns outside come back as ``fill`` (broadcast against the result)."""
    (ho, wo), (oy, ox) = view.size, view.offset
    hr, wr = resized.shape[y_axis], resized.shape[x_axis]
    ys = oy + np.arange(ho)
    xs = ox + (np.arange(wo)[::-1] if view.hflip else np.arange(wo))
    out = np.take(np.take(resized, np.clip(ys, 0, hr - 1), axis=y_axis), np.clip(xs, 0, wr - 1), axis=x_axis)
    shape = [1] * out.ndim
    shape[y_axis] = ho
    inside_y = ((ys >= 0) & (ys < hr)).reshape(shape)
    shape[y_axis], shape[x_axis] = 1, wo
    inside_x = ((xs >= 0) & (xs < wr)).reshape(shape)
    return np.where(inside_y & inside_x, out, fill)


def frame_resize_cpu(x_u8, size, filter='bilinear', layout='hwc', view=None, norm=None):
    """``functional.frame_resize`` on CPU tensors, from the same tables: uint8 frames (B, Hi, Wi, 3) / (B, 3, Hi, Wi) -> the view of
    the frames resized to ``size``; uint8 in the input's layout, or with ``norm`` (an ``InputNorm``) float32 (B, 3, Ho, Wo) through
    its table.  The horizontal pass runs first into a uint8 intermediate, then the vertical pass, as Pillow's."""
    if layout not in ('hwc', 'chw'):
        raise ValueError(f"layout {layout!r}: expected 'hwc' or 'chw'")
    if not isinstance(x_u8, torch.Tensor) or x_u8.dtype != torch.uint8 or x_u8.dim() != 4 or x_u8.shape[3 if layout == 'hwc' else 1] != 3:
        raise ValueError(f'frames must be uint8 {"(B, H, W, 3)" if layout == "hwc" else "(B, 3, H, W)"}, got '
                         f'{getattr(x_u8, "dtype", type(x_u8))} {tuple(getattr(x_u8, "shape", ()))}')
    y_axis, x_axis = (1, 2) if layout == 'hwc' else (2, 3)
    hi, wi = x_u8.shape[y_axis], x_u8.shape[x_axis]
    hr, wr = _check_sizes(hi, size[0])[1], _check_sizes(wi, size[1])[1]
    view = check_view(view, (hr, wr))
    a = x_u8.cpu().numpy()
    if wr != wi:
        b, k = resample_coeffs(wi, wr, filter)
        a = _pass(a, b.numpy(), k.numpy(), x_axis)
    if hr != hi:
        b, k = resample_coeffs(hi, hr, filter)
        a = _pass(a, b.numpy(), k.numpy(), y_axis)
    fill = np.asarray(view.fill, dtype=np.uint8).reshape((1, 1, 1, 3) if layout == 'hwc' else (1, 3, 1, 1))
    out = torch.from_numpy(np.ascontiguousarray(_apply_view(a, view, fill, y_axis, x_axis)))
    if norm is None:
        return out
    chw = (out.permute(0, 3, 1, 2) if layout == 'hwc' else out).long()
    table = norm.table('cpu')
    return torch.stack([table[c][chw[:, c]] for c in range(3)], 1).contiguous()


def label_resize_cpu(t, size, view=None, fill=255, out_dtype=None, codec=None):
    """``functional.label_resize`` on CPU tensors: labels (B, Hi, Wi), uint8 or int64, gathered through the two nearest tables, then the
    view with ``fill`` (the view's own fill is not read).  ``codec`` (a ``utils.labels.LabelCodec``): ``t`` holds raw labels, which are
    encoded first (``codec.encode_cpu``); ``fill`` is not."""
    if codec is not None:
        t = codec.encode_cpu(t)
    if not isinstance(t, torch.Tensor) or t.dtype not in (torch.uint8, torch.int64) or t.dim() != 3:
        raise ValueError(f'labels must be uint8 or int64 (B, H, W), got {getattr(t, "dtype", type(t))} {tuple(getattr(t, "shape", ()))}')
    hi, wi = t.shape[1:]
    hr, wr = _check_sizes(hi, size[0])[1], _check_sizes(wi, size[1])[1]
    view = check_view(view, (hr, wr))
    a = t.cpu().numpy()
    a = a[:, nearest_index(hi, hr).numpy().astype(np.int64)][:, :, nearest_index(wi, wr).numpy().astype(np.int64)]
    out_dtype = out_dtype or t.dtype
    out = _apply_view(a.astype(np.int64), view, np.int64(fill), 1, 2)
    return torch.from_numpy(np.ascontiguousarray(out)).to(out_dtype)
