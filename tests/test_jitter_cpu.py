"""utils/jitter.py on the CPU: the four pixel functions and ``color_jitter_cpu`` against Pillow -- the recorded bytes of
tests/golden/color_jitter_ref.npz always, live Pillow as well where it is installed (the three conversions on all 2^24 colours, ``blend``
on all byte pairs) -- and ``training.device_augment(jitter=...)`` on CPU tensors.  Bytes from stated arithmetic: every comparison is
equality."""
import functools
import math

import numpy as np
import pytest
import torch

from conftest import G, load_golden
from hyperseg_amd.utils import jitter as J
from hyperseg_amd.utils import resample as R

P = J.ColorJitterParams
FOUR = P(('brightness', 'contrast', 'saturation', 'hue'), 0.8, 1.25, 0.75, 0.1)


@pytest.fixture(scope='module')
def ref():
    return load_golden('color_jitter_ref')


def fixture_params(ref):
    """The fixture's parameter sets as ColorJitterParams."""
    out = []
    for order, factors in zip(ref['orders'].tolist(), ref['factors'].tolist()):
        names = tuple(J.OPS[c - 1] for c in order if c)
        given = {n: (None if math.isnan(f) else f) for n, f in zip(J.OPS, factors)}
        out.append(P(tuple(n for n in names if given[n] is not None), **given))       # a None factor: skipped, so not in the order
    return out


@functools.lru_cache(maxsize=None)
def _cube():
    """All 2^24 colours as three int32 tensors (4096, 4096); shared and never written to."""
    v = torch.arange(1 << 24, dtype=torch.int32).view(4096, 4096)
    return v >> 16, (v >> 8) & 255, v & 255


def _hwc(planes):
    return torch.stack(planes, -1).to(torch.uint8)


def test_equals_the_fixture(ref):
    params = fixture_params(ref)
    assert len(params) >= 12 and sum(len(p.steps()) == 4 for p in params) >= 4 and any(not p.steps() for p in params)
    assert {p.order.index('contrast') for p in params if len(p.steps()) == 4} == {0, 1, 2, 3}      # first, in the middle, last
    assert any(p.hue is not None and p.hue != 0 and J.hue_shift(p.hue) == 0 for p in params)
    for i in range(len(ref['frames'])):
        x = ref[f'f{i}_in'][None]
        assert tuple(x.shape[1:3]) == tuple(ref['frames'][i].tolist())
        for j, p in enumerate(params):
            got = J.color_jitter_cpu(x, p, 'hwc')
            assert got.dtype == torch.uint8 and torch.equal(got[0], ref[f'f{i}_p{j}']), (i, j, p)
    assert torch.equal(J.color_jitter_cpu(ref['f0_in'][None], P(), 'hwc')[0], ref['f0_in'])       # nothing to do: the identity


def test_layouts_batches_and_norm(ref):
    from hyperseg_amd import InputNorm
    params = fixture_params(ref)[:3]
    x = ref['f0_in'][None].repeat(3, 1, 1, 1)
    x[1] = x[1].flip(0)
    x[2] = 255 - x[2]
    hwc = J.color_jitter_cpu(x, params, 'hwc')
    chw = J.color_jitter_cpu(x.permute(0, 3, 1, 2).contiguous(), params, 'chw')
    assert tuple(chw.shape) == (3, 3, 37, 53) and torch.equal(chw.permute(0, 2, 3, 1), hwc)
    assert torch.equal(hwc[0], ref['f0_p0'])                                       # a sequence of B: each sample its own set
    for i in range(3):
        assert torch.equal(hwc[i], J.color_jitter_cpu(x[i:i + 1], params[i], 'hwc')[0])
    for layout, src, u8 in (('hwc', x, hwc), ('chw', x.permute(0, 3, 1, 2).contiguous(), chw)):
        norm = InputNorm((0.4137, 0.38291, 0.456789), (0.2719, 0.19283, 0.31415), layout=layout)
        fl = J.color_jitter_cpu(src, params, layout, norm=norm)
        assert fl.dtype == torch.float32 and tuple(fl.shape) == (3, 3, 37, 53) and torch.equal(fl, norm.to_float(u8))


def test_contrast_mean_rounding():
    """m = int(sum(L) / count + 0.5): 10.5 rounds up, 10.25 down."""
    px = lambda *ls: tuple(torch.tensor(ls, dtype=torch.int32) for _ in range(3))          # gray pixels: L == the value
    assert J.gray(*px(10, 11)).tolist() == [10, 11]
    assert J.contrast_mean(*px(10, 11)) == 11
    assert J.contrast_mean(*px(11, 10, 10, 10)) == 10
    # contrast 0 writes the mean everywhere
    x = torch.tensor([10, 11], dtype=torch.uint8).view(1, 1, 2, 1).repeat(1, 1, 1, 3)
    assert J.color_jitter_cpu(x, P(('contrast',), contrast=0.0), 'hwc').unique().tolist() == [11]
    x = torch.tensor([11, 10, 10, 10], dtype=torch.uint8).view(1, 2, 2, 1).repeat(1, 1, 1, 3)
    assert J.color_jitter_cpu(x, P(('contrast',), contrast=0.0), 'hwc').unique().tolist() == [10]


def test_contrast_mean_is_taken_where_contrast_stands():
    """brightness 0.5 before contrast halves the mean contrast sees; after it, it does not."""
    x = torch.full((1, 4, 4, 3), 200, dtype=torch.uint8)
    assert J.color_jitter_cpu(x, P(('brightness', 'contrast'), 0.5, 0.0), 'hwc').unique().tolist() == [100]
    assert J.color_jitter_cpu(x, P(('contrast', 'brightness'), 0.5, 0.0), 'hwc').unique().tolist() == [100]
    x[0, :2] = 0                                               # mean 100
    assert J.color_jitter_cpu(x, P(('brightness', 'contrast'), 0.5, 0.0), 'hwc').unique().tolist() == [50]


def test_hue_shift_truncates_toward_zero():
    assert [J.hue_shift(h) for h in (0.0, 0.003, -0.003, 0.1, -0.1, 0.5, -0.5)] == [0, 0, 0, 25, 231, 127, 129]


def test_params_table():
    t = J.params_table([FOUR, P(('hue', 'contrast'), contrast=0.5, hue=-0.1), P()], 3)
    assert t.dtype == torch.int32 and tuple(t.shape) == (3, J.TABLE_WORDS)
    assert t[0, 0].item() == 1 | 2 << 4 | 3 << 8 | 4 << 12 and t[0, 4].item() == 25 and t[0, 5].item() == 0b11110
    assert t[0, 1:4].view(torch.float32).tolist() == [np.float32(0.8), np.float32(1.25), np.float32(0.75)]
    assert t[1, 0].item() == 4 | 2 << 4 and t[1, 4].item() == 231 and t[1, 5].item() == 0b10100
    assert t[2].tolist() == [0] * J.TABLE_WORDS
    assert torch.equal(J.params_table(FOUR, 2), t[:1].repeat(2, 1))
    # an operation of the order whose factor is None is skipped: it is not in the record
    assert J.params_table(P(('brightness', 'hue'), hue=0.1), 1)[0, 0].item() == 4


def test_parameter_validation():
    for bad in (dict(order=('brightness', 'brightness'), brightness=1.0), dict(order=('gamma',)), dict(order=('hue',), hue=0.51),
                dict(order=('hue',), hue=-0.6), dict(order=('hue',), hue=float('nan')), dict(order=('contrast',), contrast=-0.1),
                dict(order=('saturation',), saturation=float('inf')), dict(order=('brightness',), brightness=float('nan')),
                dict(order=('brightness',), contrast=1.0)):
        with pytest.raises(ValueError):
            P(**bad)
    assert P(['hue', 'brightness'], hue=0.5, brightness=0).steps() == [('hue', 0.5), ('brightness', 0.0)]
    x = torch.zeros(2, 4, 4, 3, dtype=torch.uint8)
    with pytest.raises(ValueError):
        J.color_jitter_cpu(x.float(), FOUR)
    with pytest.raises(ValueError):
        J.color_jitter_cpu(x, FOUR, layout='chw')
    with pytest.raises(ValueError):
        J.color_jitter_cpu(x, FOUR, layout='nhwc')
    with pytest.raises(ValueError):
        J.color_jitter_cpu(x, [FOUR] * 3)                       # three sets for a batch of two
    from hyperseg_amd import InputNorm
    with pytest.raises(ValueError):
        J.color_jitter_cpu(x, FOUR, 'hwc', norm=InputNorm(layout='chw'))


def test_package_exports_the_params():
    import hyperseg_amd
    assert hyperseg_amd.ColorJitterParams is P


# ---------------------------------------------------------------------------------------------------------- device_augment

AUGMENT_CASES = [(0.5, (32, 64), (-5, -9), True), (2.0, (32, 64), (40, 101), False)]       # tests/test_hip_resample.py::test_device_augment's


@pytest.mark.parametrize('scale,crop,offset,hflip', AUGMENT_CASES)
def test_device_augment_with_jitter_on_cpu(scale, crop, offset, hflip):
    from hyperseg_amd import InputNorm
    from hyperseg_amd.training import device_augment
    norm = InputNorm(layout='hwc')
    frames = torch.randint(0, 256, (2, 48, 96, 3), generator=G(90), dtype=torch.uint8)
    labels = torch.randint(0, 19, (2, 48, 96), generator=G(91), dtype=torch.uint8)
    size = tuple(int(s) for s in np.round(np.array((48, 96)) * scale).astype(int))
    view = R.ResizeView(crop, offset, hflip, (0, 0, 0))
    crop_u8 = R.frame_resize_cpu(frames, size, 'bicubic', 'hwc', view=view)
    jit = [FOUR, P(('hue', 'saturation'), saturation=1.5, hue=-0.2)]
    for jitter in (FOUR, jit):
        img, lbl = device_augment(frames, labels, scale, crop, offset, hflip, norm, lbl_fill=255, jitter=jitter)
        assert img.dtype == torch.float32 and tuple(img.shape) == (2, 3) + crop
        assert torch.equal(img, J.color_jitter_cpu(crop_u8, jitter, 'hwc', norm=norm))
        assert torch.equal(lbl, R.label_resize_cpu(labels, size, view=view, fill=255, out_dtype=torch.int64))
    assert not torch.equal(img, norm.to_float(crop_u8))                                   # the jitter did something
    plain = device_augment(frames, labels, scale, crop, offset, hflip, norm, lbl_fill=255)
    none = device_augment(frames, labels, scale, crop, offset, hflip, norm, lbl_fill=255, jitter=None)
    assert torch.equal(plain[0], none[0]) and torch.equal(plain[1], none[1]) and torch.equal(plain[0], norm.to_float(crop_u8))


def test_draw_color_jitter():
    from hyperseg_amd.training import draw_color_jitter
    g = G(5)
    orders = set()
    for _ in range(40):
        p = draw_color_jitter(0.25, 0.25, 0.25, 0.25, generator=g)
        assert isinstance(p, P) and sorted(p.order) == sorted(J.OPS)
        assert all(0.75 <= f <= 1.25 for f in (p.brightness, p.contrast, p.saturation)) and -0.25 <= p.hue <= 0.25
        orders.add(p.order)
    assert len(orders) > 5
    p = draw_color_jitter(1.5, 0, 0, 0, generator=G(6))                                   # [max(0, 1 - x), 1 + x]; 0: not drawn, skipped
    assert 0.0 <= p.brightness <= 2.5 and p.order == ('brightness',) and p.contrast is None and p.hue is None
    a, b = draw_color_jitter(0.5, 0.5, 0.5, 0.5, generator=G(7)), draw_color_jitter(0.5, 0.5, 0.5, 0.5, generator=G(7))
    assert a == b
    with pytest.raises(ValueError):
        draw_color_jitter(0.25, 0.25, 0.25, 0.6)
    with pytest.raises(ValueError):
        draw_color_jitter(-0.1, 0, 0, 0)


# ------------------------------------------------------------------------------------------------------------ live Pillow

def _pil():
    return pytest.importorskip('PIL.Image')


def _cube_image(Image, mode):
    r, g, b = _cube()
    return Image.fromarray(_hwc((r, g, b)).numpy(), 'RGB') if mode == 'RGB' else Image.merge('HSV', [Image.fromarray(c.to(torch.uint8).numpy(), 'L') for c in (r, g, b)])


def test_rgb_to_hsv_equals_live_pillow_on_every_colour():
    Image = _pil()
    want = torch.from_numpy(np.array(_cube_image(Image, 'RGB').convert('HSV')))
    assert torch.equal(_hwc(J.rgb_to_hsv(*_cube())), want)


def test_hsv_to_rgb_equals_live_pillow_on_every_triple():
    Image = _pil()
    want = torch.from_numpy(np.array(_cube_image(Image, 'HSV').convert('RGB')))
    assert torch.equal(_hwc(J.hsv_to_rgb(*_cube())), want)


def test_gray_equals_live_pillow_on_every_colour():
    Image = _pil()
    want = torch.from_numpy(np.array(_cube_image(Image, 'RGB').convert('L')))
    assert torch.equal(J.gray(*_cube()).to(torch.uint8), want)


def test_blend_equals_live_pillow_on_every_byte_pair():
    Image = _pil()
    v = torch.arange(256, dtype=torch.int32)
    a, b = v[:, None].expand(256, 256), v[None, :].expand(256, 256)
    ia, ib = (Image.fromarray(t.to(torch.uint8).numpy(), 'L') for t in (a, b))
    factors = [0.0, 0.003, 0.1, 0.25, 1 / 3, 0.5, 0.75, 0.9, 0.999, 1.0, 1.001, 1.1, 1.25, 1.5, 1.75, 2.0, 2.2] + \
        np.random.default_rng(3).uniform(0, 2.2, 40).tolist()
    for f in factors:
        want = torch.from_numpy(np.array(Image.blend(ia, ib, f)))
        assert torch.equal(J.blend(a, b, f).to(torch.uint8), want), f


def test_jitter_equals_live_pillow(ref):
    """The three ImageEnhance classes and the hue route one at a time, and whole chains, on a fresh noise frame."""
    _pil()
    from PIL import Image, ImageEnhance
    rng = np.random.default_rng(8)
    a = rng.integers(0, 256, (29, 31, 3), dtype=np.uint8)
    x = torch.from_numpy(a)[None]
    enh = {'brightness': ImageEnhance.Brightness, 'contrast': ImageEnhance.Contrast, 'saturation': ImageEnhance.Color}

    def pil_step(img, name, f):
        if name != 'hue':
            return enh[name](img).enhance(f)
        h, s, v = img.convert('HSV').split()
        h = Image.fromarray((np.array(h).astype(np.int32) + int(f * 255)).astype(np.uint8), 'L')      # a wrapping add
        return Image.merge('HSV', (h, s, v)).convert('RGB')
    for name in enh:
        for f in [0.0, 0.5, 1.0, 1.25, 2.0] + rng.uniform(0, 2.2, 12).tolist():
            want = torch.from_numpy(np.array(pil_step(Image.fromarray(a), name, f)))
            assert torch.equal(J.color_jitter_cpu(x, P((name,), **{name: f}), 'hwc')[0], want), (name, f)
    for f in [0.0, 0.003, -0.003, 0.5, -0.5] + rng.uniform(-0.5, 0.5, 12).tolist():
        want = torch.from_numpy(np.array(pil_step(Image.fromarray(a), 'hue', f)))
        assert torch.equal(J.color_jitter_cpu(x, P(('hue',), hue=f), 'hwc')[0], want), f
    for p in fixture_params(ref):
        img = Image.fromarray(a)
        for name, f in p.steps():
            img = pil_step(img, name, f)
        assert torch.equal(J.color_jitter_cpu(x, p, 'hwc')[0], torch.from_numpy(np.array(img))), p
