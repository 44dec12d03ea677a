"""utils/blur.py -- the arithmetic of Pillow's ``ImageFilter.GaussianBlur`` restated, the specification of csrc/hs_blur.hip -- against
Pillow's recorded bytes (tests/golden/gaussian_blur_ref.npz, written by tests/golden/make_gaussian_blur_golden.py with Pillow itself),
and ``training.device_augment(blur=...)`` on CPU tensors on top.  Bytes, and floats looked up from bytes: every comparison is
``torch.equal``, no tolerance appears in this file."""
import pytest
import torch

from conftest import G, load_golden
from hyperseg_amd.utils import blur as BL

P = BL.GaussianBlurParams
KINDS = ('noise', 'binary')
LAYOUTS = ('hwc', 'chw')


def golden_cases(ref):
    """[(key of the input, sigma, Pillow's output (h, w, 3))] of the fixture."""
    out = []
    for h, w, k, si in ref['cases'].tolist():
        key = f'{h}x{w}_{KINDS[k]}'
        out.append(('in_' + key, float(ref['sigmas'][si]), ref[f'out_{key}_s{si}']))
    return out


def _in_layout(x, layout):
    return x if layout == 'hwc' else x.permute(0, 3, 1, 2).contiguous()


def test_the_fixture_holds_what_the_issue_lists():
    ref = load_golden('gaussian_blur_ref')
    have = {(h, w, float(ref['sigmas'][si])) for h, w, _, si in ref['cases'].tolist()}
    small = [(5, 7), (1, 9), (9, 1), (3, 3), (2, 50), (17, 40), (33, 21), (64, 48)]
    want = {(h, w, s) for h, w in small for s in (5, 0.5, 1, 2, 3.3, 0.1, 10, 1.5, 7, 15, 0)}
    want |= {(h, w, s) for h, w in ((70, 150), (150, 70)) for s in (5, 15)} | {(17, 40, 25)}
    assert have == want and len(ref['cases']) == 2 * len(want)                  # noise and 0 / 255 content each


@pytest.mark.parametrize('layout', LAYOUTS)
def test_every_golden_byte(layout):
    ref = load_golden('gaussian_blur_ref')
    for key, sigma, want in golden_cases(ref):
        got = BL.gaussian_blur_cpu(_in_layout(ref[key][None], layout), P(sigma), layout)
        assert got.dtype == torch.uint8 and torch.equal(got, _in_layout(want[None], layout)), (key, sigma)


def test_box_radius_and_weights():
    assert BL.box_radius(1) == 0.2500000298023224                              # float32(0.25 + 2^-25 ...): what a float64 route would call 0.25
    assert BL.weights(1) == (0, 11184811, 2796202)                             # a float64 quotient gives ww = 11184810
    assert abs(BL.box_radius(5) - 4.45) < 1e-6 and BL.weights(5) == (4, 1694668, 762602)
    assert BL.weights(0) == (0, 1 << 24, 0)                                    # a copy
    for sigma in (0.1, 0.5, 1, 1.5, 2, 3.3, 5, 7, 10, 15, 25):
        r, ww, fw = BL.weights(sigma)
        assert r == int(BL.box_radius(sigma)) and (2 * r + 1) * ww + 2 * fw in ((1 << 24) - 1, 1 << 24) and fw >= 0
        assert 255 * ((2 * r + 1) * ww + 2 * fw) + (1 << 23) < 1 << 32             # a pass fits 32 unsigned bits
    assert BL.weights(15)[0] <= BL.MAX_RADIUS < BL.weights(25)[0]
    assert BL.params_table([P(5), P(1, apply=False), None], 3).tolist() == [[1, 4, 1694668, 762602], [0, 0, 11184811, 2796202], [0, 0, 1 << 24, 0]]


@pytest.mark.parametrize('layout', LAYOUTS)
def test_norm_is_the_table_lookup_of_the_bytes(layout):
    from hyperseg_amd import InputNorm
    norm = InputNorm((0.4137, 0.38291, 0.456789), (0.2719, 0.19283, 0.31415), layout=layout)
    x = _in_layout(torch.randint(0, 256, (2, 19, 23, 3), generator=G(4100), dtype=torch.uint8), layout)
    params = [P(2), P(5)]
    u8 = BL.gaussian_blur_cpu(x, params, layout)
    fl = BL.gaussian_blur_cpu(x, params, layout, norm=norm)
    assert fl.dtype == torch.float32 and tuple(fl.shape) == (2, 3, 19, 23) and torch.equal(fl, norm.to_float(u8))


@pytest.mark.parametrize('layout', LAYOUTS)
def test_mixed_batch(layout):
    """Per-sample radii and apply flags: every sample is what it is alone, an unapplied one its input."""
    x = _in_layout(torch.randint(0, 256, (4, 17, 40, 3), generator=G(4101), dtype=torch.uint8), layout)
    params = [P(5), P(1.5, apply=False), P(0.5), None]
    got = BL.gaussian_blur_cpu(x, params, layout)
    for i, p in enumerate(params):
        alone = x[i:i + 1] if p is None or not p.apply else BL.gaussian_blur_cpu(x[i:i + 1], p, layout)
        assert torch.equal(got[i:i + 1], alone), i
    assert not torch.equal(got[0], x[0]) and not torch.equal(got[2], x[2])
    assert torch.equal(BL.gaussian_blur_cpu(x, None, layout, table=BL.params_table(params, 4)), got)
    ref = load_golden('gaussian_blur_ref')                                     # and against Pillow: one input at three radii
    a = ref['in_17x40_noise']
    batch = _in_layout(torch.stack([a, a, a]), layout)
    want = _in_layout(torch.stack([ref['out_17x40_noise_s0'], a, ref['out_17x40_noise_s11']]), layout)      # sigma 5, not applied, sigma 25
    assert torch.equal(BL.gaussian_blur_cpu(batch, [P(5), P(7, False), P(25)], layout), want)


def test_argument_errors():
    from hyperseg_amd import InputNorm
    x = torch.zeros(2, 8, 8, 3, dtype=torch.uint8)
    for bad in (-1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError):
            P(bad)
    with pytest.raises(ValueError):
        BL.gaussian_blur_cpu(x.float(), P(5))
    with pytest.raises(ValueError):
        BL.gaussian_blur_cpu(x, P(5), layout='chw')
    with pytest.raises(ValueError):
        BL.gaussian_blur_cpu(x, P(5), layout='nhwc')
    with pytest.raises(ValueError):
        BL.gaussian_blur_cpu(x, [P(5)] * 3)
    with pytest.raises(ValueError):
        BL.gaussian_blur_cpu(x, None)
    with pytest.raises(ValueError):
        BL.gaussian_blur_cpu(x, 5.0)
    with pytest.raises(ValueError):
        BL.gaussian_blur_cpu(x, P(5), norm=InputNorm(layout='chw'))
    with pytest.raises(ValueError):
        BL.gaussian_blur_cpu(x[:0], P(5))
    with pytest.raises(ValueError):
        BL.gaussian_blur_cpu(x, None, table=BL.params_table(P(5), 3))


def test_draw_gaussian_blur():
    from hyperseg_amd.training import draw_gaussian_blur
    assert draw_gaussian_blur(1.0, 3) == P(3, True) and draw_gaussian_blur(0.0) == P(5, False)
    drawn = [draw_gaussian_blur(generator=G(4102 + i)) for i in range(64)]
    assert {p.radius for p in drawn} == {5.0} and 8 < sum(p.apply for p in drawn) < 56
    assert draw_gaussian_blur(generator=G(7)) == draw_gaussian_blur(generator=G(7))
    with pytest.raises(ValueError):
        draw_gaussian_blur(1.5)


# the (scale, crop, offset, hflip) cases of tests/test_hip_resample.py::test_device_augment
@pytest.mark.parametrize('jitter', [False, True], ids=['plain', 'jitter'])
@pytest.mark.parametrize('scale,crop,offset,hflip', [(0.5, (32, 64), (-5, -9), True), (2.0, (32, 64), (40, 101), False)])
def test_device_augment_with_blur_on_cpu_tensors(scale, crop, offset, hflip, jitter):
    """``blur=`` is the blur of the uint8 crop -- padding included, behind the jitter -- looked up in the table; the label is the same."""
    from hyperseg_amd import ColorJitterParams, InputNorm
    from hyperseg_amd.training import BatchAugment, device_augment
    from hyperseg_amd.utils import jitter as J
    from hyperseg_amd.utils import resample
    norm = InputNorm(layout='hwc')
    frames = torch.randint(0, 256, (2, 48, 96, 3), generator=G(90), dtype=torch.uint8)
    labels = torch.randint(0, 19, (2, 48, 96), generator=G(91), dtype=torch.uint8)
    jit = [ColorJitterParams(('brightness', 'contrast'), 0.8, 1.25), ColorJitterParams(('hue',), hue=0.1)] if jitter else None
    blur = [P(5), P(2)]
    img, lbl = device_augment(frames, labels, scale, crop, offset, hflip, norm, lbl_fill=255, jitter=jit, blur=blur)
    plain_img, plain_lbl = device_augment(frames, labels, scale, crop, offset, hflip, norm, lbl_fill=255, jitter=jit)
    # the uint8 crop of the chain without the blur, from its own parts
    size = tuple(int(round(s * scale)) for s in (48, 96))
    view = resample.ResizeView(crop, offset, hflip, (0, 0, 0))
    crop_u8 = resample.frame_resize_cpu(frames, size, 'bicubic', 'hwc', view=view)
    if jitter:
        crop_u8 = J.color_jitter_cpu(crop_u8, jit, 'hwc')
    assert torch.equal(norm.to_float(crop_u8), plain_img)
    assert torch.equal(img, norm.to_float(BL.gaussian_blur_cpu(crop_u8, blur, 'hwc'))) and not torch.equal(img, plain_img)
    assert torch.equal(lbl, plain_lbl)
    none = device_augment(frames, labels, scale, crop, offset, hflip, norm, lbl_fill=255, jitter=jit, blur=None)
    assert torch.equal(none[0], plain_img) and torch.equal(none[1], plain_lbl)
    off = device_augment(frames, labels, scale, crop, offset, hflip, norm, lbl_fill=255, jitter=jit, blur=[None, P(3, False)])
    assert torch.equal(off[0], plain_img)
    aug = BatchAugment((48, 96), crop, norm, (0.25, 2.0))
    got = aug(frames, labels, scale, offset, hflip, jitter=jit, blur=blur)
    assert torch.equal(got[0], img) and torch.equal(got[1], lbl)
    if not jitter:
        ran = aug.run(frames, labels, params=aug.rows(scale, offset, hflip, 2), blur=BL.params_table(blur, 2))
        assert torch.equal(ran[0], img) and torch.equal(ran[1], lbl)
