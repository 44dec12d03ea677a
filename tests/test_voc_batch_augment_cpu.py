"""``training.BatchAugmentVOC`` on CPU tensors, and the shared inputs of tests/test_hip_voc_batch_augment.py: a ragged batch given as a
canvas plus extents must come out as ``training.device_augment_voc`` of the list of cropped samples -- the Pillow-exact chain
tests/test_rotate_cpu.py holds (tests/golden/rotate_ref.npz).  Integer and IEEE-float64 arithmetic throughout: every comparison is
``torch.equal``, no tolerance appears here."""
import functools

import numpy as np
import pytest
import torch

from conftest import G

CANVAS, PAD, B = (40, 56), 64, 6
SIZES = [(40, 56), (33, 47), (17, 23), (40, 9), (5, 56), (1, 1)]
FLIPS = [True, False, True, True, False, True]
SCALES = [0.25, 0.9, 0.4, None, 0.25, 1.0]          # bicubic: 17 taps at 0.25 (the loop), 7 at 0.9 (registers), in == out, untouched
ANGLES = [-30.0, -7.5, 0.0, 13.0, 30.0, 90.0]
FILLS = dict(fill=(5, 6, 7), lbl_fill=250, rotate_fill=(8, 9, 10), lbl_rotate_fill=3)
# two more parameter sets (a graph replays with them): other extents, flips, scales, angles
SETS = [(SIZES, FLIPS, SCALES, ANGLES),
        (SIZES[::-1], FLIPS[::-1], [None, 0.9, 0.25, 0.4, 0.9, 0.25], ANGLES[::-1]),
        ([(40, 56), (40, 56), (8, 8), (39, 55), (2, 3), (21, 56)], [False, True, False, True, False, True], [0.9, 0.25, 0.4, 1.0, 0.9, 0.5],
         [30.0, -30.0, 90.0, 0.0, 45.0, -13.0])]


def jitters(contrast):
    """Six drawn ColorJitters; ``contrast``: all four operations in a drawn order, else the other three."""
    from hyperseg_amd.training import draw_color_jitter
    return [draw_color_jitter(0.5, 0.5 if contrast else 0.0, 0.5, 0.5, generator=G(5100 + i)) for i in range(B)]


def resized(size, scale):
    if scale is None or float(scale) == 1.0:
        return tuple(size)
    return tuple(int(s) for s in np.round(np.array(size) * float(scale)).astype(int))


def test_the_cases_fit_the_pad():
    for sizes, _, scales, _ in SETS:
        for size, s in zip(sizes, scales):
            assert 1 <= min(resized(size, s)) and max(resized(size, s)) <= PAD


@functools.lru_cache(maxsize=None)
def canvas(layout, label_dtype, garbage=0):
    """The canvases (frames, labels): random bytes everywhere, so every extent is an image and everything outside it is garbage;
    ``garbage`` reseeds what lies outside SIZES only.  Computed once, never written to."""
    hm, wm = CANVAS
    frames = torch.randint(0, 256, (B, hm, wm, 3), generator=G(5000), dtype=torch.uint8)
    labels = torch.randint(0, 21, (B, hm, wm), generator=G(5001), dtype=torch.uint8)
    labels[torch.rand(B, hm, wm, generator=G(5002)) < 0.1] = 255
    if garbage:
        noise = torch.randint(0, 256, (B, hm, wm, 3), generator=G(5010 + garbage), dtype=torch.uint8)
        lnoise = torch.randint(0, 256, (B, hm, wm), generator=G(5020 + garbage), dtype=torch.uint8)
        for i, (h, w) in enumerate(SIZES):
            inside = torch.zeros(hm, wm, dtype=torch.bool)
            inside[:h, :w] = True
            frames[i] = torch.where(inside[..., None], frames[i], noise[i])
            labels[i] = torch.where(inside, labels[i], lnoise[i])
    if layout == 'chw':
        frames = frames.permute(0, 3, 1, 2).contiguous()
    return frames, labels.to(label_dtype)


def crops(frames, labels, sizes, layout):
    """The ragged lists ``device_augment_voc`` takes."""
    xs = [frames[i, :h, :w] if layout == 'hwc' else frames[i, :, :h, :w] for i, (h, w) in enumerate(sizes)]
    return xs, [labels[i, :h, :w] for i, (h, w) in enumerate(sizes)]


@functools.lru_cache(maxsize=None)
def expected(layout, label_dtype, jitter=None, which=0):
    """The oracle: ``device_augment_voc`` of the cropped samples of parameter set ``which`` on CPU tensors; ``jitter``: None, 'contrast'
    or 'plain'.  Computed once, never written to."""
    from hyperseg_amd import InputNorm
    from hyperseg_amd.training import device_augment_voc
    sizes, flips, scales, angles = SETS[which]
    frames, labels = canvas(layout, label_dtype)
    xs, ts = crops(frames, labels, sizes, layout)
    return device_augment_voc(xs, ts, flips, None if jitter is None else jitters(jitter == 'contrast'), scales, angles, PAD,
                              InputNorm(layout=layout), **FILLS)


def make(layout, **kw):
    from hyperseg_amd import InputNorm
    from hyperseg_amd.training import BatchAugmentVOC
    return BatchAugmentVOC(CANVAS, PAD, InputNorm(layout=layout), **dict(FILLS, **kw))


@pytest.mark.parametrize('layout', ('hwc', 'chw'))
@pytest.mark.parametrize('label_dtype', (torch.uint8, torch.int64))
@pytest.mark.parametrize('jitter', (None, 'contrast'))
def test_canvas_and_sizes_equal_the_ragged_list(layout, label_dtype, jitter):
    frames, labels = canvas(layout, label_dtype, garbage=1)
    aug = make(layout)
    js = None if jitter is None else jitters(True)
    img, lbl = aug(frames, labels, SIZES, FLIPS, js, SCALES, ANGLES)
    want_img, want_lbl = expected(layout, label_dtype, jitter)
    assert img.dtype == torch.float32 and tuple(img.shape) == (B, 3, PAD, PAD) and lbl.dtype == torch.int64 and tuple(lbl.shape) == (B, PAD, PAD)
    assert torch.equal(img, want_img) and torch.equal(lbl, want_lbl)
    if jitter is not None:
        assert not torch.equal(want_img, expected(layout, label_dtype)[0])


def test_a_list_of_ragged_samples_is_packed():
    frames, labels = canvas('hwc', torch.uint8)
    xs, ts = crops(frames, labels, SIZES, 'hwc')
    aug = make('hwc')
    img, lbl = aug(xs, ts, None, FLIPS, None, SCALES, ANGLES)
    want_img, want_lbl = expected('hwc', torch.uint8)
    assert torch.equal(img, want_img) and torch.equal(lbl, want_lbl)
    packed, lpacked, sizes = aug.pack(xs, ts)
    assert sizes == SIZES and tuple(packed.shape) == (B,) + CANVAS + (3,)
    for i, (h, w) in enumerate(SIZES):
        assert torch.equal(packed[i, :h, :w], xs[i]) and not bool(packed[i, h:].any()) and not bool(packed[i, :, w:].any())
        assert torch.equal(lpacked[i, :h, :w], ts[i])


def test_rows_are_what_the_kernels_read():
    from hyperseg_amd.utils import jitter as J
    from hyperseg_amd.utils import rotate
    aug = make('hwc', batch=B)
    p = aug.rows(SIZES, FLIPS, jitters(True), SCALES, ANGLES)
    assert p.rows.dtype == torch.int32 and tuple(p.rows.shape) == (B, 8) and p.matrices.dtype == torch.float64 and p.fixed.dtype == torch.int32
    for i, (size, s) in enumerate(zip(SIZES, SCALES)):
        hr, wr = resized(size, s)
        assert p.rows[i].tolist() == [size[0], size[1], hr, wr, int(FLIPS[i]), 0, 0, 0]
        m = rotate.rotation_matrix(hr, wr, ANGLES[i])
        assert p.matrices[i].tolist() == list(m) and p.fixed[i].tolist() == list(rotate.nearest_fixed(m))
    assert torch.equal(p.jitter, J.params_table(jitters(True), B)) and p.contrast
    q = aug.rows(SIZES, False, jitters(False), None, 0.0)
    assert not q.contrast and bool(q.jitter.any()) and q.rows[:, 2:4].tolist() == [list(s) for s in SIZES]
    assert not bool(aug.rows(SIZES, False, None, None, 0.0).jitter.any())


def test_ks_max_covers_every_extent_of_the_canvas():
    """Rounding the resized size makes the true ratio larger than 1 / lo for some extents (18 -> round(4.5) = 4 has 19 bicubic taps, not
    17); a row never holds more than its axis has pixels."""
    from hyperseg_amd.utils import resample as R
    aug = make('hwc')
    assert aug.ks_max >= R.ks_for('bicubic', 0.25)
    for n in range(1, 57):
        out = int(np.round(n * 0.25))
        if out >= 1:
            assert min(R.ksize_of(n, out, 'bicubic'), n) <= aug.ks_max
    assert any(min(R.ksize_of(n, int(np.round(n * 0.25)), 'bicubic'), n) == aug.ks_max for n in range(4, 57))


def test_refusals():
    frames, labels = canvas('hwc', torch.uint8)
    aug = make('hwc')
    ok = (SIZES, FLIPS, None, SCALES, ANGLES)
    with pytest.raises(ValueError, match='exceeds pad'):
        make('hwc', scale_range=(0.25, 2.0))(frames, labels, SIZES, FLIPS, None, [2.0] + SCALES[1:], ANGLES)
    with pytest.raises(ValueError, match='scale_range'):
        aug(frames, labels, SIZES, FLIPS, None, [0.2] + SCALES[1:], ANGLES)
    with pytest.raises(ValueError, match='leaves nothing'):
        aug(frames, labels, SIZES, FLIPS, None, SCALES[:5] + [0.25], ANGLES)
    with pytest.raises(ValueError, match='canvas'):
        aug(frames, labels, [(41, 56)] + SIZES[1:], FLIPS, None, SCALES, ANGLES)
    with pytest.raises(ValueError):
        aug(frames, labels, SIZES[:5], FLIPS, None, SCALES, ANGLES)          # mismatched counts
    with pytest.raises(ValueError):
        aug(frames, labels, SIZES, FLIPS[:3], None, SCALES, ANGLES)
    with pytest.raises(ValueError):
        aug(frames, labels, SIZES, FLIPS, jitters(True)[:2], SCALES, ANGLES)
    with pytest.raises(ValueError):
        aug(frames, labels[:5], *ok)
    with pytest.raises(ValueError):
        aug(frames.float(), labels, *ok)                                     # wrong dtype
    with pytest.raises(ValueError):
        aug(frames, labels.float(), *ok)
    with pytest.raises(ValueError):
        aug(frames[:, :39], labels[:, :39], *ok)                             # another canvas
    with pytest.raises(ValueError):
        aug(frames, labels, None, FLIPS, None, SCALES, ANGLES)               # a canvas without sizes
    with pytest.raises(ValueError):
        aug(frames[:4], labels[:4], SIZES[:4], FLIPS[:4], None, SCALES[:4], ANGLES[:4])      # the object holds batches of 6 by now
    assert aug.tables is None                                                # CPU tensors and refusals make nothing on a device
