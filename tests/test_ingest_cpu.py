"""uint8 frames, host side (no GPU): InputNorm's table is the reference's ToTensor + Normalize arithmetic exactly, attaching a norm leaves
state dicts alone, a uint8 input without a norm is refused with a TypeError that says what to do, the CPU route normalises with stock ops, and
fps.synthetic_batches keeps its float draws."""
import pytest
import torch

from conftest import G
from hyperseg_amd.utils.synthetic import fill_by_name

CONSTANTS = [((0.485, 0.456, 0.406), (0.229, 0.224, 0.225)), ((0.5, 0.5, 0.5), (0.5, 0.5, 0.5)),
             ((0.4137, 0.38291, 0.456789), (0.2719, 0.19283, 0.31415))]


def _expression(mean, std):
    """table[c, v] = (float32(v) / 255 - mean[c]) / std[c] in float32: torchvision's to_tensor (``img.to(float32).div(255)``) followed by
    normalize (``tensor.sub_(mean[:, None, None]).div_(std[:, None, None])`` with float32 mean / std), restated."""
    m, s = torch.as_tensor(mean, dtype=torch.float32), torch.as_tensor(std, dtype=torch.float32)
    v = torch.arange(256, dtype=torch.uint8).to(torch.float32).div(255)
    return torch.stack([(v - m[c]) / s[c] for c in range(3)])


def _reference_float(u8, norm):
    """The reference transforms applied to uint8 frames on the CPU: (B, 3, H, W) float32."""
    chw = u8.permute(0, 3, 1, 2) if norm.layout == 'hwc' else u8
    t = chw.to(torch.float32).div(255)
    return t.sub(norm.mean[None, :, None, None]).div(norm.std[None, :, None, None]).contiguous()


@pytest.mark.parametrize('mean,std', CONSTANTS)
def test_table_is_the_reference_expression(mean, std):
    from hyperseg_amd import InputNorm
    norm = InputNorm(mean, std)
    table = norm.table()
    assert table.shape == (3, 256) and table.dtype == torch.float32 and table.is_contiguous()
    assert torch.equal(table, _expression(mean, std))
    # ... and looking a frame's bytes up in it is the two transforms applied to the frame
    u8 = torch.randint(0, 256, (2, 5, 7, 3), generator=G(41), dtype=torch.uint8)
    looked_up = torch.stack([table[c][u8[..., c].long()] for c in range(3)], dim=1)
    assert torch.equal(looked_up, _reference_float(u8, norm))


def test_defaults_and_export():
    import hyperseg_amd
    from hyperseg_amd.utils.inference import InputNorm
    assert hyperseg_amd.InputNorm is InputNorm
    norm = InputNorm()
    assert norm.layout == 'hwc'
    assert torch.equal(norm.mean, torch.tensor([0.485, 0.456, 0.406])) and torch.equal(norm.std, torch.tensor([0.229, 0.224, 0.225]))
    assert norm.frame_size(torch.zeros(2, 4, 6, 3, dtype=torch.uint8)) == (2, 4, 6)
    assert InputNorm(layout='chw').frame_size(torch.zeros(2, 3, 4, 6, dtype=torch.uint8)) == (2, 4, 6)
    with pytest.raises(ValueError):
        InputNorm(layout='nhwc')
    with pytest.raises(ValueError):
        norm.frame_size(torch.zeros(2, 3, 4, 6, dtype=torch.uint8))          # a 'chw' frame handed to an 'hwc' norm
    with pytest.raises(ValueError):
        norm.frame_size(torch.zeros(2, 4, 6, 3))


@pytest.mark.parametrize('layout', ['hwc', 'chw'])
def test_cpu_route_is_the_reference_transform(layout):
    from hyperseg_amd import InputNorm
    norm = InputNorm(layout=layout)
    shape = (2, 9, 11, 3) if layout == 'hwc' else (2, 3, 9, 11)
    u8 = torch.randint(0, 256, shape, generator=G(42), dtype=torch.uint8)
    out = norm.to_float(u8)
    assert out.shape == (2, 3, 9, 11) and out.is_contiguous()
    assert torch.equal(out, _reference_float(u8, norm))


def _model():
    from hyperseg_amd import configs
    return fill_by_name(configs.build('hyperseg-m').eval(), seed=3)


def test_norm_is_not_state():
    from hyperseg_amd import InputNorm
    from hyperseg_amd.utils.inference import prepare_for_inference
    model = _model()
    assert model.input_norm is None
    before = {k: v.clone() for k, v in model.state_dict().items()}
    model.input_norm = InputNorm()
    after = model.state_dict()
    assert list(after.keys()) == list(before.keys())
    other = _model()
    other.input_norm = InputNorm(layout='chw')
    other.load_state_dict(after, strict=True)                     # round trip, strict
    assert all(torch.equal(v, before[k]) for k, v in other.state_dict().items())
    assert not any('norm' in n and 'input' in n for n, _ in list(model.named_buffers()) + list(model.named_parameters()))
    # prepare_for_inference attaches one as well, and leaves the keys alone too
    third = _model()
    norm = InputNorm((0.5, 0.5, 0.5), (0.5, 0.5, 0.5))
    prepare_for_inference(third, fold_bn=False, input_norm=norm)
    assert third.input_norm is norm
    assert list(third.state_dict().keys()) == list(before.keys())
    with pytest.raises(TypeError):
        prepare_for_inference(_model(), fold_bn=False, input_norm=(0.5, 0.5))


def test_uint8_without_a_norm_is_a_type_error():
    model = _model()
    u8 = torch.zeros(1, 64, 64, 3, dtype=torch.uint8)
    for call in (model, model.segment, model.process_single_tensor):
        with pytest.raises(TypeError, match='input_norm'):
            call(u8)
    with pytest.raises(TypeError, match='input_norm'):
        model([u8])


def test_synthetic_batches_float_draws_unchanged():
    from hyperseg_amd.fps import synthetic_batches
    dev = torch.device('cpu')
    got = synthetic_batches(3, 2, (8, 16), 19, dev, seed=5)
    got_kw = synthetic_batches(3, 2, (8, 16), 19, dev, seed=5, uint8=False)
    g = torch.Generator().manual_seed(5)                             # the draws as they have always been made
    for (x, t), (xk, tk) in zip(got, got_kw):
        ex = torch.rand(2, 3, 8, 16, generator=g)
        et = torch.randint(0, 19, (2, 8, 16), generator=g)
        assert x.dtype == torch.float32 and torch.equal(x, ex) and torch.equal(t, et)
        assert torch.equal(xk, ex) and torch.equal(tk, et)
    for layout, shape in (('hwc', (2, 8, 16, 3)), ('chw', (2, 3, 8, 16))):
        frames = synthetic_batches(2, 2, (8, 16), 19, dev, seed=5, uint8=True, layout=layout)
        assert all(x.dtype == torch.uint8 and tuple(x.shape) == shape and tuple(t.shape) == (2, 8, 16) for x, t in frames)
        again = synthetic_batches(2, 2, (8, 16), 19, dev, seed=5, uint8=True, layout=layout)
        assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(frames, again))
