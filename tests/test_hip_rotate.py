"""uint8 frames and labels rotated on the device (csrc/hs_rotate.hip): ``functional.frame_rotate`` / ``label_rotate`` against the CPU
implementation (utils/rotate.py -- itself held to Pillow's bytes by tests/test_rotate_cpu.py) and against Pillow's recorded bytes
(tests/golden/rotate_ref.npz); graph capture with caller-owned tables, and ``training.device_augment_voc`` on top.  The device runs
Pillow's float64 operations in Pillow's order and integer arithmetic: every comparison is ``torch.equal``, no tolerance appears."""
import functools

import pytest
import torch

from conftest import G, load_golden
from hyperseg_amd.utils import rotate as RT

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
LAYOUTS = ('hwc', 'chw')
# tiny; odd; square (the right angles are transposes); wide; tall, more than one row group; wider and taller than one 64 x 4 workgroup tile
SIZES = [(5, 7), (21, 33), (32, 32), (17, 40), (64, 48), (70, 150)]
CONTENTS = ('noise', 'binary', 'zeros', 'ones')
ANGLES = (17.3, -29.999, 90.0)                    # three samples, three angles, one launch
PADDED = (80, 160)
FILLS = dict(fill=(11, 22, 233), pad_fill=(7, 128, 250))


@functools.lru_cache(maxsize=None)
def _frames(h, w, content):
    """uint8 (3, H, W, 3) frames, shared and never written to."""
    if content == 'noise':
        return torch.randint(0, 256, (3, h, w, 3), generator=G(3000 + 7 * h + w), dtype=torch.uint8)
    if content == 'binary':
        return (torch.randint(0, 2, (3, h, w, 3), generator=G(4000 + 7 * h + w)) * 255).to(torch.uint8)
    return torch.full((3, h, w, 3), 0 if content == 'zeros' else 255, dtype=torch.uint8)


@functools.lru_cache(maxsize=None)
def _labels(h, w):
    return torch.randint(0, 256, (3, h, w), generator=G(5000 + 7 * h + w), dtype=torch.uint8)


def _in_layout(x, layout):
    return x if layout == 'hwc' else x.permute(0, 3, 1, 2).contiguous()


@functools.lru_cache(maxsize=None)
def _reference(h, w, content, padded):
    """The CPU implementation's uint8 result for the shared frames, 'hwc'; computed once per case."""
    return RT.frame_rotate_cpu(_frames(h, w, content), ANGLES, 'hwc', **(dict(size=PADDED, **FILLS) if padded else {}))


def _offset_view(t, off, dev=DEV):
    """``t``'s bytes on the device, starting ``off`` bytes into a larger byte buffer."""
    buf = torch.zeros(t.numel() * t.element_size() + 16, dtype=torch.uint8, device=dev)
    view = buf[off:off + t.numel()].view(t.shape)
    view.copy_(t)
    return view


@pytest.mark.parametrize('layout', LAYOUTS)
@pytest.mark.parametrize('size', SIZES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_frame_rotate_equals_cpu(size, layout):
    from hyperseg_amd import functional as HF
    h, w = size
    for content in CONTENTS:
        x = _in_layout(_frames(h, w, content), layout).to(DEV)
        got = HF.frame_rotate(x, ANGLES, layout)
        assert got.dtype == torch.uint8 and tuple(got.shape) == tuple(x.shape)
        assert torch.equal(got.cpu(), _in_layout(_reference(h, w, content, False), layout)), content
        got = HF.frame_rotate(x, ANGLES, layout, size=PADDED, **FILLS)
        assert torch.equal(got.cpu(), _in_layout(_reference(h, w, content, True), layout)), content


@pytest.mark.parametrize('layout', LAYOUTS)
def test_normalised_output_is_the_table_lookup(layout):
    from hyperseg_amd import functional as HF
    from hyperseg_amd import InputNorm
    norm = InputNorm((0.4137, 0.38291, 0.456789), (0.2719, 0.19283, 0.31415), layout=layout)
    for h, w in ((21, 33), (70, 150)):
        x = _in_layout(_frames(h, w, 'noise'), layout).to(DEV)
        for kw in ({}, dict(size=PADDED, **FILLS)):
            u8 = HF.frame_rotate(x, ANGLES, layout, **kw)
            fl = HF.frame_rotate(x, ANGLES, layout, norm=norm, **kw)
            assert fl.dtype == torch.float32 and tuple(fl.shape) == (3, 3) + (PADDED if kw else (h, w))
            assert torch.equal(fl, norm.to_float(u8))
            assert torch.equal(fl.cpu(), RT.frame_rotate_cpu(x.cpu(), ANGLES, layout, norm=norm, **kw))
    big = torch.full((fl.numel() + 3,), float('nan'), device=DEV)                # a destination that is only 4-byte aligned
    sl = big[1:1 + fl.numel()].view(fl.shape)
    assert HF.frame_rotate(x, ANGLES, layout, norm=norm, out=sl, **kw) is sl
    assert torch.equal(sl, fl) and bool(torch.isnan(big[0])) and bool(torch.isnan(big[-2:]).all())


@pytest.mark.parametrize('layout', LAYOUTS)
def test_unaligned_base(layout):
    from hyperseg_amd import functional as HF
    x = _in_layout(_frames(21, 33, 'noise'), layout)
    want = _in_layout(_reference(21, 33, 'noise', False), layout)
    assert torch.equal(HF.frame_rotate(_offset_view(x, 1), ANGLES, layout).cpu(), want)
    big = torch.full((want.numel() + 5,), 77, dtype=torch.uint8, device=DEV)
    sl = big[3:3 + want.numel()].view(want.shape)
    got = HF.frame_rotate(x.to(DEV), ANGLES, layout, out=sl)
    assert got is sl and torch.equal(sl.cpu(), want) and bool((big[:3] == 77).all()) and bool((big[-2:] == 77).all())
    t = _labels(21, 33)
    assert torch.equal(HF.label_rotate(_offset_view(t, 1), ANGLES).cpu(), RT.label_rotate_cpu(t, ANGLES))


@pytest.mark.parametrize('dtype', [torch.uint8, torch.int64])
def test_label_rotate(dtype):
    from hyperseg_amd import functional as HF
    for h, w in SIZES:
        t = _labels(h, w).to(dtype)
        got = HF.label_rotate(t.to(DEV), ANGLES)
        assert got.dtype == dtype and torch.equal(got.cpu(), RT.label_rotate_cpu(t, ANGLES)), (h, w)
        want = RT.label_rotate_cpu(t, ANGLES, size=PADDED, fill=3, pad_fill=250)
        assert torch.equal(HF.label_rotate(t.to(DEV), ANGLES, size=PADDED, fill=3, pad_fill=250).cpu(), want), (h, w)
        other = torch.int64 if dtype == torch.uint8 else torch.uint8              # the other storage type out
        out = torch.empty(want.shape, dtype=other, device=DEV)
        assert torch.equal(HF.label_rotate(t.to(DEV), ANGLES, size=PADDED, fill=3, pad_fill=250, out=out).cpu(), want.to(other))


def test_right_angles_are_transposes():
    from hyperseg_amd import functional as HF
    x, t = _frames(32, 32, 'noise').to(DEV), _labels(32, 32).to(DEV)
    for k, angle in enumerate((0, 90, 180, 270)):
        assert torch.equal(HF.frame_rotate(x, angle), torch.rot90(x, k, (1, 2))), angle
        assert torch.equal(HF.label_rotate(t, angle), torch.rot90(t, k, (1, 2))), angle


def test_fixture_bytes():
    """The GPU reproduces Pillow's recorded bytes directly."""
    from hyperseg_amd import functional as HF
    ref = load_golden('rotate_ref')
    cases = [(f's{i}', ref['angles'].tolist(), ('noise', 'binary')) for i in range(len(ref['sizes']))] + [('big', ref['big_angles'].tolist(), ('noise',))]
    for key, angles, contents in cases:
        n = len(angles)
        for kind in contents:
            x = ref[f'{key}_{kind}_in']
            got = HF.frame_rotate(x[None].expand(n, *x.shape).contiguous().to(DEV), angles)
            assert torch.equal(got.cpu(), ref[f'{key}_{kind}_out']), (key, kind)
        t = ref[f'{key}_label_in']
        got = HF.label_rotate(t[None].expand(n, *t.shape).contiguous().to(DEV), angles)
        assert torch.equal(got.cpu(), ref[f'{key}_label_out']), key


def test_refusals():
    from hyperseg_amd import functional as HF
    from hyperseg_amd import _hip
    x = torch.zeros(1, 8, 8, 3, dtype=torch.uint8, device=DEV)
    t = torch.zeros(1, 8, 8, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError):
        HF.frame_rotate(x.float(), 10.0)
    with pytest.raises(ValueError):
        HF.frame_rotate(x, 10.0, layout='chw')
    with pytest.raises(ValueError):
        HF.frame_rotate(x, 10.0, size=(7, 8))
    with pytest.raises(ValueError):
        HF.frame_rotate(x, None, table=torch.zeros(1, 6, dtype=torch.float64))       # a table on the CPU
    with pytest.raises(ValueError):
        HF.frame_rotate(x, None, table=torch.zeros(2, 6, dtype=torch.float64, device=DEV))
    with pytest.raises(ValueError):
        HF.label_rotate(t, None, table=torch.zeros(1, 6, dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError):
        HF.label_rotate(t.float(), 10.0)
    with pytest.raises(ValueError):
        HF.label_rotate(t, 10.0, fill=256)
    # declined geometries: HS_ERR_UNSUPPORTED, nothing launched -- the output stays as it was
    m = RT.matrix_table(8, 8, 10.0, 1).to(DEV)
    f = RT.fixed_table(8, 8, 10.0, 1).to(DEV)
    y = torch.full((1, 8, 8, 3), 9, dtype=torch.uint8, device=DEV)
    lib, s = _hip.lib, _hip.stream_ptr()
    assert lib.hs_frame_rotate_fwd(x.data_ptr(), 0, 1, 8, 8, m.data_ptr(), 8, 8193, 0, 0, None, y.data_ptr(), s) == -3
    assert lib.hs_frame_rotate_fwd(x.data_ptr(), 0, 65536, 8, 8, m.data_ptr(), 8, 8, 0, 0, None, y.data_ptr(), s) == -3
    assert lib.hs_frame_rotate_fwd(x.data_ptr(), 2, 1, 8, 8, m.data_ptr(), 8, 8, 0, 0, None, y.data_ptr(), s) == -1
    assert lib.hs_label_rotate_fwd(t.data_ptr(), 0, 1, 8193, 8, f.data_ptr(), 8, 8, 0, 255, y.data_ptr(), 0, s) == -3
    assert lib.hs_label_rotate_fwd(t.data_ptr(), 2, 1, 8, 8, f.data_ptr(), 8, 8, 0, 255, y.data_ptr(), 0, s) == -1
    torch.cuda.synchronize()
    assert bool((y == 9).all())


def test_graph_replays_with_the_tables_last_copied_in():
    from hyperseg_amd import functional as HF
    from hyperseg_amd import InputNorm
    norm = InputNorm()
    h, w = 21, 33
    x, t = _frames(h, w, 'noise').to(DEV), _labels(h, w).to(DEV)
    m = RT.matrix_table(h, w, ANGLES, 3).to(DEV)
    f = RT.fixed_table(h, w, ANGLES, 3).to(DEV)
    img = torch.empty(3, 3, 40, 48, device=DEV)
    lbl = torch.empty(3, 40, 48, dtype=torch.int64, device=DEV)
    norm.table(DEV)
    HF.frame_rotate(x, None, size=(40, 48), norm=norm, out=img, table=m)                 # warm-up outside the capture
    HF.label_rotate(t, None, size=(40, 48), out=lbl, table=f)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        HF.frame_rotate(x, None, size=(40, 48), norm=norm, out=img, table=m)
        HF.label_rotate(t, None, size=(40, 48), out=lbl, table=f)
    for angles in ((-12.0, 3.75, 270.0), ANGLES):
        m.copy_(RT.matrix_table(h, w, angles, 3))
        f.copy_(RT.fixed_table(h, w, angles, 3))
        graph.replay()
        assert torch.equal(img, HF.frame_rotate(x, angles, size=(40, 48), norm=norm)), angles
        assert torch.equal(lbl, HF.label_rotate(t, angles, size=(40, 48)).long()), angles
        assert torch.equal(img.cpu(), RT.frame_rotate_cpu(x.cpu(), angles, size=(40, 48), norm=norm)), angles


def test_device_augment_voc_equals_cpu():
    """Three frames of three sizes, every stage set: jitter, flip, scale (up, down, none) and angle per sample; pad 64."""
    from hyperseg_amd import InputNorm
    from hyperseg_amd.training import device_augment_voc, draw_color_jitter
    norm = InputNorm(layout='hwc')
    sizes, flips, scales, angles = [(40, 60), (33, 47), (24, 31)], [True, False, True], [0.5, 1.3, None], [-17.0, 29.5, 8.25]
    params = [draw_color_jitter(0.5, 0.5, 0.5, 0.5, generator=G(40 + i)) for i in range(3)]
    frames = [torch.randint(0, 256, (h, w, 3), generator=G(50 + i), dtype=torch.uint8) for i, (h, w) in enumerate(sizes)]
    labels = [torch.randint(0, 21, (h, w), generator=G(60 + i), dtype=torch.uint8) for i, (h, w) in enumerate(sizes)]
    kw = dict(fill=(5, 6, 7), lbl_fill=250, rotate_fill=(8, 9, 10), lbl_rotate_fill=3)
    want_img, want_lbl = device_augment_voc(frames, labels, flips, params, scales, angles, 64, norm, **kw)
    img, lbl = device_augment_voc([x.to(DEV) for x in frames], [t.to(DEV) for t in labels], flips, params, scales, angles, 64, norm, **kw)
    assert img.dtype == torch.float32 and tuple(img.shape) == (3, 3, 64, 64) and lbl.dtype == torch.int64 and tuple(lbl.shape) == (3, 64, 64)
    assert torch.equal(img.cpu(), want_img) and torch.equal(lbl.cpu(), want_lbl)
    assert int((lbl == 250).sum()) > 0 and int((lbl == 3).sum()) > 0                          # the padding and the empty corners are there


def test_device_augment_voc_fixture_chain():
    """transpose -> resize -> rotate -> paste with Pillow alone, against the chain on the device."""
    from hyperseg_amd import InputNorm
    from hyperseg_amd.training import device_augment_voc
    ref = load_golden('rotate_ref')
    norm = InputNorm()
    for i, (h, w, hflip, scale, angle, pad) in enumerate(ref['chain'].tolist()):
        img, lbl = device_augment_voc(ref[f'k{i}_in'][None].to(DEV), ref[f'k{i}_label_in'][None].to(DEV), bool(hflip), None, scale, angle,
                                      int(pad), norm)
        assert torch.equal(img.cpu(), norm.to_float(ref[f'k{i}_out'][None])) and torch.equal(lbl.cpu(), ref[f'k{i}_label_out'][None].long()), i
