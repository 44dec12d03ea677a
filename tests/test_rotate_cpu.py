"""Pillow's rotation restated (hyperseg_amd/utils/rotate.py) against Pillow's recorded bytes (tests/golden/rotate_ref.npz, written by
tests/golden/make_rotate_golden.py with Pillow alone): the matrix, ``frame_rotate_cpu`` (BICUBIC, float64) and ``label_rotate_cpu``
(NEAREST, 16.16 fixed point), the rules that are easy to get wrong pinned one by one, and ``training.device_augment_voc`` -- the
reference's VOC train chain -- on CPU tensors.  Every comparison is ``torch.equal``: no tolerance appears in this file."""
import math

import pytest
import torch

from conftest import G, load_golden
from hyperseg_amd.utils import rotate as RT

CONTENTS = ('noise', 'binary')


@pytest.fixture(scope='module')
def ref():
    return load_golden('rotate_ref')


def _cases(ref):
    """(key, (h, w), angles) of every recorded rotation case."""
    out = [(f's{i}', (h, w), ref['angles'].tolist(), CONTENTS) for i, (h, w) in enumerate(ref['sizes'].tolist())]
    return out + [('big', tuple(ref['big_size'].tolist()), ref['big_angles'].tolist(), ('noise',))]


def test_rotation_matrix_equals_pillows_doubles(ref):
    for key, (h, w), angles, _ in _cases(ref):
        for ai, a in enumerate(angles):
            assert list(RT.rotation_matrix(h, w, a)) == ref[f'{key}_m'][ai].tolist(), (key, a)
    table = RT.matrix_table(21, 33, ref['angles'].tolist(), 15)
    assert table.dtype == torch.float64 and torch.equal(table, ref['s0_m'])
    assert RT.matrix_table(21, 33, 12, 3).tolist() == [list(RT.rotation_matrix(21, 33, 12))] * 3


@pytest.mark.parametrize('layout', ['hwc', 'chw'])
def test_frame_rotate_equals_pillow(ref, layout):
    for key, (h, w), angles, contents in _cases(ref):
        for kind in contents:
            x = ref[f'{key}_{kind}_in']
            want = ref[f'{key}_{kind}_out']
            if layout == 'chw':
                x, want = x.permute(2, 0, 1).contiguous(), want.permute(0, 3, 1, 2).contiguous()
            got = RT.frame_rotate_cpu(x[None].expand(len(angles), *x.shape).contiguous(), angles, layout)      # one angle per sample
            assert got.dtype == torch.uint8 and torch.equal(got, want), (key, kind)
    # {0, 255} frames: the negative lobes overshoot, so both ends of the clip decide bytes
    assert int((ref['s0_binary_out'] == 0).sum()) > 0 and int((ref['s0_binary_out'] == 255).sum()) > 0


@pytest.mark.parametrize('dtype', [torch.uint8, torch.int64])
def test_label_rotate_equals_pillow(ref, dtype):
    for key, (h, w), angles, _ in _cases(ref):
        t = ref[f'{key}_label_in'].to(dtype)
        got = RT.label_rotate_cpu(t[None].expand(len(angles), h, w).contiguous(), angles)
        assert got.dtype == dtype and torch.equal(got, ref[f'{key}_label_out'].to(dtype)), key
    assert RT.nearest_fixed((1.0, 0.0, 0.0, 0.0, 1.0, 0.0)) == (65536, 0, 32768, 0, 65536, 32768)
    assert torch.equal(RT.fixed_table(32, 32, [0, 90], 2), torch.tensor([RT.nearest_fixed(RT.rotation_matrix(32, 32, a)) for a in (0, 90)],
                                                                        dtype=torch.int32))


def test_right_angles_are_transposes():
    """0, 90, 180, 270 degrees on a square image: Pillow answers with a transpose; the general formulas give the same bytes."""
    x = torch.randint(0, 256, (2, 32, 32, 3), generator=G(1), dtype=torch.uint8)
    t = torch.randint(0, 21, (2, 32, 32), generator=G(2), dtype=torch.uint8)
    for k, angle in enumerate((0, 90, 180, 270)):
        assert torch.equal(RT.frame_rotate_cpu(x, angle), torch.rot90(x, k, (1, 2))), angle
        assert torch.equal(RT.label_rotate_cpu(t, angle), torch.rot90(t, k, (1, 2))), angle
    assert torch.equal(RT.frame_rotate_cpu(x, 180), x.flip(1).flip(2)) and torch.equal(RT.frame_rotate_cpu(x, 360.0), x)
    odd = torch.randint(0, 256, (1, 5, 7, 3), generator=G(3), dtype=torch.uint8)                 # 180 degrees needs no square
    assert torch.equal(RT.frame_rotate_cpu(odd, 180), odd.flip(1).flip(2)) and torch.equal(RT.label_rotate_cpu(odd[..., 0], 180),
                                                                                          odd[..., 0].flip(1).flip(2))


def _cubic(v1, v2, v3, v4, d):
    p1, p2 = v2, -v1 + v3
    p3 = ((2 * (v1 - v2)) + v3) - v4
    p4 = ((-v1 + v2) - v3) + v4
    return p1 + d * (p2 + d * (p3 + d * p4))


def _pixel(img, m, x, y, fill=0):
    """One output byte of one band ``img`` (list of rows), the rules spelt out as scalar Python: the float value, or None = fill."""
    h, w = len(img), len(img[0])
    xi, yi = x + 0.5, y + 0.5
    xin, yin = (m[0] * xi + m[1] * yi) + m[2], (m[3] * xi + m[4] * yi) + m[5]
    if xin < 0 or xin >= w or yin < 0 or yin >= h:
        return None
    xin, yin = xin - 0.5, yin - 0.5
    x0, y0 = math.floor(xin), math.floor(yin)
    dx, dy = xin - x0, yin - y0
    x0, y0 = x0 - 1, y0 - 1
    cols = [min(max(x0 + k, 0), w - 1) for k in range(4)]
    rows, outside = [], []
    for k in range(4):
        ry = y0 + k
        if k == 0:
            ry = min(max(ry, 0), h - 1)
        if 0 <= ry < h:
            rows.append(_cubic(*(float(img[ry][c]) for c in cols), dx))
        else:
            rows.append(rows[-1])                             # the previous row's horizontal result
            outside.append(k)
    return _cubic(*rows, dy), outside


def test_rows_below_the_frame_repeat_the_previous_row():
    """A translation by a quarter pixel down and right (``table=``): the windows of the last two output rows hang over the bottom edge."""
    band = torch.randint(0, 256, (5, 6), generator=G(4), dtype=torch.uint8)
    m = (1.0, 0.0, 0.25, 0.0, 1.0, 0.25)
    got = RT.frame_rotate_cpu(band[None, :, :, None].expand(1, 5, 6, 3).contiguous(), None, table=torch.tensor([m], dtype=torch.float64))
    hung = 0
    for y in range(5):
        for x in range(6):
            v, outside = _pixel(band.tolist(), m, x, y)
            hung += bool(outside) and y >= 3
            want = 0 if v <= 0 else 255 if v >= 255 else int(v)
            assert got[0, y, x].tolist() == [want] * 3, (y, x)
    assert hung == 12                                         # both bottom output rows, every column


def test_the_byte_is_truncated_not_rounded():
    """Columns 0, 10, 12, 0 in every row, sampled half-way between the two middle ones: 13.75 exactly -> 13, where + 0.5 would give 14."""
    x = torch.tensor([0, 10, 12, 0], dtype=torch.uint8).view(1, 1, 4, 1).expand(1, 3, 4, 3).contiguous()
    m = (1.0, 0.0, 0.5, 0.0, 1.0, 0.0)
    assert _pixel(x[0, :, :, 0].tolist(), m, 1, 1)[0] == 13.75
    got = RT.frame_rotate_cpu(x, None, table=torch.tensor([m], dtype=torch.float64))
    assert got[0, 1, 1].tolist() == [13, 13, 13]


def test_pad_view_fills_and_norm():
    from hyperseg_amd import InputNorm
    x = torch.randint(0, 256, (2, 9, 11, 3), generator=G(5), dtype=torch.uint8)
    t = torch.randint(0, 21, (2, 9, 11), generator=G(6), dtype=torch.uint8)
    plain, lplain = RT.frame_rotate_cpu(x, [20, -20], fill=(1, 2, 3)), RT.label_rotate_cpu(t, [20, -20], fill=7)
    got = RT.frame_rotate_cpu(x, [20, -20], size=(12, 16), fill=(1, 2, 3), pad_fill=(9, 8, 7))
    assert tuple(got.shape) == (2, 12, 16, 3) and torch.equal(got[:, :9, :11], plain)
    assert torch.equal(got[:, 9:], torch.tensor([9, 8, 7], dtype=torch.uint8).expand(2, 3, 16, 3))
    assert torch.equal(got[:, :, 11:], torch.tensor([9, 8, 7], dtype=torch.uint8).expand(2, 12, 5, 3))
    assert plain[0, 0, 0].tolist() == [1, 2, 3] and int(lplain[0, 0, 0]) == 7                 # a corner the rotation leaves empty
    lgot = RT.label_rotate_cpu(t, [20, -20], size=(12, 16), fill=7, pad_fill=255, out_dtype=torch.int64)
    assert lgot.dtype == torch.int64 and torch.equal(lgot[:, :9, :11], lplain.long()) and bool((lgot[:, 9:] == 255).all())
    assert bool((lgot[:, :, 11:] == 255).all())
    norm = InputNorm((0.4137, 0.38291, 0.456789), (0.2719, 0.19283, 0.31415))
    fl = RT.frame_rotate_cpu(x, [20, -20], size=(12, 16), fill=(1, 2, 3), pad_fill=(9, 8, 7), norm=norm)
    assert fl.dtype == torch.float32 and torch.equal(fl, norm.to_float(got))
    from hyperseg_amd import functional as HF                  # CPU tensors go to the CPU functions
    assert torch.equal(HF.frame_rotate(x, [20, -20], size=(12, 16), fill=(1, 2, 3), pad_fill=(9, 8, 7)), got)
    assert torch.equal(HF.label_rotate(t, [20, -20], size=(12, 16), fill=7), RT.label_rotate_cpu(t, [20, -20], size=(12, 16), fill=7))


def test_chain_cases_through_device_augment_voc(ref):
    """transpose -> resize -> rotate -> paste with Pillow alone, against the chain on CPU tensors."""
    from hyperseg_amd import InputNorm
    from hyperseg_amd.training import device_augment_voc
    norm = InputNorm()
    chain = ref['chain'].tolist()
    for i, (h, w, hflip, scale, angle, pad) in enumerate(chain):
        img, lbl = device_augment_voc([ref[f'k{i}_in']], [ref[f'k{i}_label_in']], bool(hflip), None, scale, angle, int(pad), norm)
        assert img.dtype == torch.float32 and lbl.dtype == torch.int64
        assert torch.equal(img, norm.to_float(ref[f'k{i}_out'][None])) and torch.equal(lbl, ref[f'k{i}_label_out'][None].long()), i
    # both at once: a sequence of frames of different sizes, one parameter per sample
    img, lbl = device_augment_voc([ref['k0_in'], ref['k1_in']], [ref['k0_label_in'], ref['k1_label_in']], [bool(c[2]) for c in chain], None,
                                  [c[3] for c in chain], [c[4] for c in chain], 48, norm)
    assert torch.equal(img, norm.to_float(torch.stack([ref['k0_out'], ref['k1_out']])))
    assert torch.equal(lbl, torch.stack([ref['k0_label_out'], ref['k1_label_out']]).long())


def test_resize_then_flip_is_not_the_reference_label(ref):
    """Why the chain flips FIRST: Pillow's NEAREST table of the exact 2:1 reduction is not mirror-symmetric."""
    from hyperseg_amd.utils import resample as R
    t = ref['k1_label_in'][None]
    assert not torch.equal(R.label_resize_cpu(t.flip(2), (30, 40)), R.label_resize_cpu(t, (30, 40)).flip(2))


def test_chain_with_jitter_equals_the_composition():
    from hyperseg_amd import InputNorm
    from hyperseg_amd.training import device_augment_voc, draw_color_jitter
    from hyperseg_amd.utils import jitter as J
    from hyperseg_amd.utils import resample as R
    norm = InputNorm(layout='chw')
    sizes, flips, scales, angles = [(30, 44), (25, 31)], [True, False], [0.8, None], [-17.0, 29.5]
    params = [draw_color_jitter(0.5, 0.5, 0.5, 0.5, generator=G(10 + i)) for i in range(2)]
    frames = [torch.randint(0, 256, (3, h, w), generator=G(20 + i), dtype=torch.uint8) for i, (h, w) in enumerate(sizes)]
    labels = [torch.randint(0, 21, (h, w), generator=G(30 + i)) for i, (h, w) in enumerate(sizes)]
    img, lbl = device_augment_voc(frames, labels, flips, params, scales, angles, 48, norm, fill=(5, 6, 7), lbl_fill=250,
                                  rotate_fill=(8, 9, 10), lbl_rotate_fill=3)
    assert tuple(img.shape) == (2, 3, 48, 48) and tuple(lbl.shape) == (2, 48, 48)
    for i, (h, w) in enumerate(sizes):
        x, t = frames[i][None], labels[i][None]
        if flips[i]:
            x, t = x.flip(3), t.flip(2)
        x = J.color_jitter_cpu(x, params[i], 'chw')
        if scales[i] is not None:
            size = (round(h * scales[i]), round(w * scales[i]))
            x, t = R.frame_resize_cpu(x, size, 'bicubic', 'chw'), R.label_resize_cpu(t, size)
        x = RT.frame_rotate_cpu(x, angles[i], 'chw', (48, 48), (8, 9, 10), (5, 6, 7), norm=norm)
        t = RT.label_rotate_cpu(t, angles[i], (48, 48), 3, 250)
        assert torch.equal(img[i:i + 1], x) and torch.equal(lbl[i:i + 1], t), i
    assert int((lbl == 250).sum()) > 0 and int((lbl == 3).sum()) > 0


def test_refusals():
    from hyperseg_amd import InputNorm
    from hyperseg_amd.training import device_augment_voc
    x, t = torch.zeros(1, 8, 10, 3, dtype=torch.uint8), torch.zeros(1, 8, 10, dtype=torch.uint8)
    norm = InputNorm()
    with pytest.raises(ValueError):
        device_augment_voc(x, t, False, None, 1.0, 10.0, 9, norm)                # 8 x 10 does not fit pad 9
    with pytest.raises(ValueError):
        device_augment_voc(x, t, False, None, 1.5, 10.0, 12, norm)               # 12 x 15 after the resize
    with pytest.raises(ValueError):
        RT.frame_rotate_cpu(x, 10.0, size=(8, 9))
    with pytest.raises(ValueError):
        RT.label_rotate_cpu(t, 10.0, size=(7, 10))
    with pytest.raises(ValueError):
        RT.frame_rotate_cpu(torch.zeros(1, 1, 8193, 3, dtype=torch.uint8), 10.0)
    with pytest.raises(ValueError):
        RT.label_rotate_cpu(torch.zeros(1, 8193, 1, dtype=torch.uint8), 10.0)
    with pytest.raises(ValueError):
        RT.rotation_matrix(8193, 4, 1.0)
    with pytest.raises(ValueError):
        RT.frame_rotate_cpu(x.float(), 10.0)                                     # a wrong dtype
    with pytest.raises(ValueError):
        RT.frame_rotate_cpu(x, 10.0, layout='chw')                               # a wrong layout for these frames
    with pytest.raises(ValueError):
        RT.frame_rotate_cpu(x, 10.0, layout='nhwc')
    with pytest.raises(ValueError):
        RT.label_rotate_cpu(t.float(), 10.0)
    with pytest.raises(ValueError):
        RT.label_rotate_cpu(x, 10.0)                                             # four dimensions
    with pytest.raises(ValueError):
        RT.frame_rotate_cpu(x, [10.0, 20.0])                                     # two angles for one sample
    with pytest.raises(ValueError):
        RT.frame_rotate_cpu(x, None, table=torch.zeros(2, 6, dtype=torch.float64))
    with pytest.raises(ValueError):
        RT.frame_rotate_cpu(x, None, table=torch.zeros(1, 6, dtype=torch.float32))
    with pytest.raises(ValueError):
        RT.label_rotate_cpu(t, None, table=torch.zeros(1, 5, dtype=torch.int32))
    with pytest.raises(ValueError):
        RT.label_rotate_cpu(t, None, table=torch.zeros(1, 6, dtype=torch.int64))
    with pytest.raises(ValueError):
        RT.frame_rotate_cpu(x, 10.0, fill=(0, 0, 256))
