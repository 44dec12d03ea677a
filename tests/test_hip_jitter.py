"""ColorJitter on the device (csrc/hs_jitter.hip): ``functional.color_jitter`` against the CPU implementation of the same arithmetic
(utils/jitter.py -- itself held to Pillow's bytes by tests/test_jitter_cpu.py) and against Pillow's recorded bytes
(tests/golden/color_jitter_ref.npz); ``training.device_augment(jitter=...)`` on top.  Bytes, and floats looked up from bytes: every
comparison is ``torch.equal``, no tolerance appears in this file."""
import functools
import math

import pytest
import torch

from conftest import G, load_golden
from hyperseg_amd.utils import jitter as J

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
LAYOUTS = ('hwc', 'chw')
P = J.ColorJitterParams
B, C, S, H = J.OPS
MIDDLE = P((B, C, S, H), 0.8, 1.25, 0.75, 0.1)                  # four operations, contrast in the middle
MIDDLE2 = P((H, S, C, B), 1.25, 0.5, 1.5, -0.2)                 # contrast behind the HSV round trip and a saturation above 1
NO_CONTRAST = P((S, H), saturation=0.5, hue=0.3)


def fixture_params(ref):
    """The fixture's parameter sets as ColorJitterParams; an operation recorded without a factor was skipped."""
    out = []
    for order, factors in zip(ref['orders'].tolist(), ref['factors'].tolist()):
        given = {n: (None if math.isnan(f) else f) for n, f in zip(J.OPS, factors)}
        out.append(P(tuple(J.OPS[c - 1] for c in order if c and given[J.OPS[c - 1]] is not None), **given))
    return out


def _in_layout(x, layout):
    return x if layout == 'hwc' else x.permute(0, 3, 1, 2).contiguous()


@functools.lru_cache(maxsize=None)
def _frames(b, h, w, seed=0):
    """uint8 (B, H, W, 3) noise frames, shared and never written to."""
    return torch.randint(0, 256, (b, h, w, 3), generator=G(3000 + 7 * h + w + seed), dtype=torch.uint8)


@functools.lru_cache(maxsize=None)
def _cube():
    """All 2^24 colours as one uint8 (1, 4096, 4096, 3) frame; shared and never written to."""
    v = torch.arange(1 << 24, dtype=torch.int32).view(4096, 4096)
    return torch.stack((v >> 16, (v >> 8) & 255, v & 255), -1).to(torch.uint8)[None]


@functools.lru_cache(maxsize=None)
def _cube_on_device():
    return _cube().to(DEV)


@functools.lru_cache(maxsize=None)
def _cube_hsv():
    """The cube through RGB -> HSV on the CPU, once for the four hue shifts."""
    x = _cube()[0].to(torch.int32)
    return J.rgb_to_hsv(x[..., 0], x[..., 1], x[..., 2])


@pytest.mark.parametrize('shift', [0, 1, 128, 255])
def test_hue_on_every_colour(shift):
    """Both HSV directions on all 2^24 colours.  The shift goes into the record itself: int(h * 255) with |h| <= 0.5 never gives 128."""
    from hyperseg_amd import functional as HF
    h, s, v = _cube_hsv()
    want = torch.stack(J.hsv_to_rgb((h + shift) % 256, s, v), -1).to(torch.uint8)[None]
    table = J.params_table(P((H,), hue=0.0), 1)
    table[0, 4] = shift
    got = HF.color_jitter(_cube_on_device(), None, 'hwc', table=table.to(DEV))
    assert torch.equal(got.cpu(), want)
    if shift == 0:
        assert not torch.equal(want, _cube())                            # the round trip alone is lossy


@pytest.mark.parametrize('factor', [0.5, 1.5])
def test_saturation_on_every_colour(factor):
    from hyperseg_amd import functional as HF
    p = P((S,), saturation=factor)
    got = HF.color_jitter(_cube_on_device(), p, 'hwc')
    assert torch.equal(got.cpu(), J.color_jitter_cpu(_cube(), p, 'hwc'))


@pytest.mark.parametrize('layout', LAYOUTS)
def test_fixture_bytes(layout):
    """The GPU reproduces Pillow's recorded bytes directly: uint8 out and, through the table, float32 out."""
    from hyperseg_amd import functional as HF
    from hyperseg_amd import InputNorm
    ref = load_golden('color_jitter_ref')
    norm = InputNorm((0.4137, 0.38291, 0.456789), (0.2719, 0.19283, 0.31415), layout=layout)
    params = fixture_params(ref)
    for i in range(len(ref['frames'])):
        x = _in_layout(ref[f'f{i}_in'][None], layout).to(DEV)
        for j, p in enumerate(params):
            want = _in_layout(ref[f'f{i}_p{j}'][None], layout)
            got = HF.color_jitter(x, p, layout)
            assert got.dtype == torch.uint8 and torch.equal(got.cpu(), want), (i, j, p)
            fl = HF.color_jitter(x, p, layout, norm=norm)
            assert fl.dtype == torch.float32 and torch.equal(fl.cpu(), norm.to_float(want)), (i, j, p)
    # the whole fixture frame 0 as ONE batch, a parameter set per sample
    x = _in_layout(ref['f0_in'][None].repeat(len(params), 1, 1, 1), layout).to(DEV)
    want = _in_layout(torch.stack([ref[f'f0_p{j}'] for j in range(len(params))]), layout)
    assert torch.equal(HF.color_jitter(x, params, layout).cpu(), want)


# 1 pixel; fewer than 4; a column; widths with a scalar tail (53: H W odd, 67 x 4: H W a multiple of 4 behind a tail-free 'chw' plane);
# several workgroups in the reduction with a ragged last one (97 x 131 = 12707 pixels = 3177 groups of 4 = 12.4 workgroups)
SMALL = [(1, 1), (2, 3), (5, 1), (7, 53), (4, 67), (3, 67), (97, 131)]


@pytest.mark.parametrize('layout', LAYOUTS)
@pytest.mark.parametrize('hw', SMALL, ids=lambda s: f'{s[0]}x{s[1]}')
def test_small_shapes(hw, layout):
    from hyperseg_amd import functional as HF
    from hyperseg_amd import InputNorm
    norm = InputNorm(layout=layout)
    for b in (1, 2):                                  # the second image of an odd-sized pair starts at an odd address
        x = _in_layout(_frames(b, *hw), layout)
        for p in (MIDDLE, MIDDLE2):
            want = J.color_jitter_cpu(x, p, layout)
            got = HF.color_jitter(x.to(DEV), p, layout)
            assert got.dtype == torch.uint8 and tuple(got.shape) == tuple(x.shape) and torch.equal(got.cpu(), want), (b, p)
            fl = HF.color_jitter(x.to(DEV), p, layout, norm=norm)
            assert tuple(fl.shape) == (b, 3) + hw and torch.equal(fl.cpu(), norm.to_float(want)), (b, p)


@pytest.mark.parametrize('layout', LAYOUTS)
def test_batch_with_an_order_per_sample(layout):
    """Three samples, three orders, one of them without contrast (its workgroups leave the mean pass)."""
    from hyperseg_amd import functional as HF
    params = [MIDDLE, NO_CONTRAST, MIDDLE2]
    x = _in_layout(_frames(3, 37, 53), layout)
    want = J.color_jitter_cpu(x, params, layout)
    assert torch.equal(HF.color_jitter(x.to(DEV), params, layout).cpu(), want)
    for i, p in enumerate(params):                    # and each sample is what it is alone
        assert torch.equal(HF.color_jitter(x[i:i + 1].to(DEV), p, layout).cpu(), want[i:i + 1])


@pytest.mark.parametrize('layout', LAYOUTS)
def test_unaligned_base_and_out_slice(layout):
    from hyperseg_amd import functional as HF
    from hyperseg_amd import InputNorm
    x = _in_layout(_frames(2, 8, 12), layout)         # H W a multiple of 4: only the base decides the alignment
    want = J.color_jitter_cpu(x, MIDDLE, layout)
    for off in (1, 2, 3):
        buf = torch.zeros(x.numel() + 16, dtype=torch.uint8, device=DEV)
        src = buf[off:off + x.numel()].view(x.shape)
        src.copy_(x)
        assert torch.equal(HF.color_jitter(src, MIDDLE, layout).cpu(), want), off
    big = torch.full((want.numel() + 5,), 77, dtype=torch.uint8, device=DEV)
    sl = big[3:3 + want.numel()].view(want.shape)
    got = HF.color_jitter(x.to(DEV), MIDDLE, layout, out=sl)
    assert got is sl and torch.equal(sl.cpu(), want) and bool((big[:3] == 77).all()) and bool((big[-2:] == 77).all())
    norm = InputNorm(layout=layout)
    fbig = torch.full((want.numel() + 3,), float('nan'), device=DEV)          # a destination that is only 4-byte aligned
    fsl = fbig[1:1 + want.numel()].view(2, 3, 8, 12)
    HF.color_jitter(x.to(DEV), MIDDLE, layout, norm=norm, out=fsl)
    assert torch.equal(fsl.cpu(), norm.to_float(want)) and bool(torch.isnan(fbig[0])) and bool(torch.isnan(fbig[-2:]).all())


def test_integer_accumulator():
    """512 x 1024 pixels of 255: the L sum, 1.3e8, is past 2^24, where a float32 accumulator stops counting."""
    from hyperseg_amd import functional as HF
    x = torch.full((1, 512, 1024, 3), 255, dtype=torch.uint8)
    assert 255 * 512 * 1024 > 1 << 24
    p = P((C,), contrast=0.5)
    got = HF.color_jitter(x.to(DEV), p, 'hwc').cpu()
    assert got.unique().tolist() == [255]                                     # m == 255: blend(255, 255, 0.5)
    assert torch.equal(got, J.color_jitter_cpu(x, p, 'hwc'))
    at0 = HF.color_jitter(x.to(DEV), P((C,), contrast=0.0), 'hwc').cpu()        # contrast 0 writes m itself
    assert at0.unique().tolist() == [255]


def test_determinism_and_a_table_changed_between_replays():
    from hyperseg_amd import functional as HF
    x = _frames(2, 97, 131).to(DEV)
    sets = ([MIDDLE, NO_CONTRAST], [MIDDLE2, MIDDLE])
    want = [J.color_jitter_cpu(x.cpu(), s, 'hwc') for s in sets]
    first, second = HF.color_jitter(x, sets[0], 'hwc'), HF.color_jitter(x, sets[0], 'hwc')
    assert torch.equal(first, second) and torch.equal(first.cpu(), want[0])
    tables = [J.params_table(s, 2).to(DEV) for s in sets]
    table = tables[0].clone()
    out = torch.empty_like(x)
    HF.color_jitter(x, None, 'hwc', out=out, table=table)                      # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        HF.color_jitter(x, None, 'hwc', out=out, table=table)
    for k in (1, 0, 1):
        table.copy_(tables[k])
        graph.replay()
        assert torch.equal(out.cpu(), want[k]), k


def test_refusals():
    from hyperseg_amd import functional as HF
    from hyperseg_amd import InputNorm, _hip
    x = torch.zeros(2, 8, 8, 3, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError):
        HF.color_jitter(x.float(), MIDDLE)
    with pytest.raises(ValueError):
        HF.color_jitter(x, MIDDLE, layout='chw')
    with pytest.raises(ValueError):
        HF.color_jitter(x, MIDDLE, layout='nhwc')
    with pytest.raises(ValueError):
        HF.color_jitter(x, [MIDDLE] * 3)
    with pytest.raises(ValueError):
        HF.color_jitter(x, MIDDLE, norm=InputNorm(layout='chw'))
    with pytest.raises(ValueError):
        HF.color_jitter(x, MIDDLE, out=torch.empty(2, 8, 8, 3, device=DEV))              # float out for a uint8 result
    with pytest.raises(ValueError):
        HF.color_jitter(x, None, table=J.params_table(MIDDLE, 2))                        # a table on the CPU
    with pytest.raises(ValueError):
        HF.color_jitter(x, None, table=J.params_table(MIDDLE, 3).to(DEV))                # three records for two frames
    # declined sizes: HS_ERR_UNSUPPORTED, nothing launched -- the output stays as it was
    y = torch.full((2, 8, 8, 3), 9, dtype=torch.uint8, device=DEV)
    t = J.params_table(MIDDLE, 2).to(DEV)
    sums = torch.zeros(2, dtype=torch.int64, device=DEV)
    lib, s = _hip.lib, _hip.stream_ptr()
    args = lambda batch, w: (x.data_ptr(), 0, batch, 8, w, t.data_ptr(), sums.data_ptr(), None, y.data_ptr(), s)
    assert lib.hs_color_jitter_fwd(*args(65536, 8)) == -3
    assert lib.hs_color_jitter_fwd(*args(2, (1 << 19) + 1)) == -3
    assert lib.hs_color_jitter_fwd(*args(2, 0)) == -1                                   # HS_ERR_BAD_ARG
    torch.cuda.synchronize()
    assert bool((y == 9).all())


# the (scale, crop, offset, hflip) cases of tests/test_hip_resample.py::test_device_augment
@pytest.mark.parametrize('scale,crop,offset,hflip', [(0.5, (32, 64), (-5, -9), True), (2.0, (32, 64), (40, 101), False)])
def test_device_augment_with_jitter(scale, crop, offset, hflip):
    from hyperseg_amd import InputNorm
    from hyperseg_amd.training import device_augment
    norm = InputNorm(layout='hwc')
    frames = torch.randint(0, 256, (2, 48, 96, 3), generator=G(90), dtype=torch.uint8)
    labels = torch.randint(0, 19, (2, 48, 96), generator=G(91), dtype=torch.uint8)
    jitter = [MIDDLE, NO_CONTRAST]
    want_img, want_lbl = device_augment(frames, labels, scale, crop, offset, hflip, norm, lbl_fill=255, jitter=jitter)      # CPU tensors
    img, lbl = device_augment(frames.to(DEV), labels.to(DEV), scale, crop, offset, hflip, norm, lbl_fill=255, jitter=jitter)
    assert img.dtype == torch.float32 and tuple(img.shape) == (2, 3) + crop and lbl.dtype == torch.int64 and tuple(lbl.shape) == (2,) + crop
    assert torch.equal(img.cpu(), want_img) and torch.equal(lbl.cpu(), want_lbl)
    plain = device_augment(frames.to(DEV), labels.to(DEV), scale, crop, offset, hflip, norm, lbl_fill=255)
    none = device_augment(frames.to(DEV), labels.to(DEV), scale, crop, offset, hflip, norm, lbl_fill=255, jitter=None)
    assert torch.equal(plain[0], none[0]) and torch.equal(plain[1], none[1]) and not torch.equal(plain[0], img)
