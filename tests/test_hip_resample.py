"""Camera-size uint8 frames and labels resized on the device (csrc/hs_resample.hip): ``functional.frame_resize`` / ``label_resize`` against the
CPU implementation built on the same tables (utils/resample.py -- itself held to Pillow's bytes by tests/test_resample_cpu.py) and against
Pillow's recorded bytes (tests/golden/resample_ref.npz); the models, GraphedModel and ``training.device_augment`` on top.  Integer
arithmetic and table look-ups: every comparison is ``torch.equal``, no tolerance appears in this file."""
import functools

import pytest
import torch

from conftest import G, load_golden
from hyperseg_amd.utils import resample as R
from hyperseg_amd.utils.synthetic import fill_by_name

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
FILTERS = ('bilinear', 'bicubic')
LAYOUTS = ('hwc', 'chw')
# exact 2x down; odd sizes, clipped windows at every border; up; bicubic ksize 17; one pass skipped (x2); mixed up and down; tiny
SHAPES = [((64, 128), (32, 64)), ((37, 53), (19, 31)), ((24, 40), (48, 80)), ((40, 72), (10, 18)), ((30, 50), (30, 25)),
          ((31, 45), (77, 45)), ((16, 16), (5, 37)), ((9, 8), (3, 3))]
CONTENTS = ('noise', 'binary', 'zeros', 'ones')
# tag -> (config, the smallest frame size tests/test_hip_ingest.py uses for it, classes); camera frames are twice that
MODELS = {'M': ('hyperseg-m', (256, 512), 19), 'Lc': ('hyperseg-l-camvid', (384, 512), 12)}


@pytest.fixture(autouse=True)
def deterministic_stock_convolutions(monkeypatch):
    monkeypatch.setattr(torch.backends.cudnn, 'deterministic', True)      # tests/test_hip_ingest.py's docstring: the float forward then repeats


@functools.lru_cache(maxsize=None)
def _frames(b, h, w, content, seed=0):
    """uint8 (B, H, W, 3) frames, shared and never written to."""
    if content == 'noise':
        return torch.randint(0, 256, (b, h, w, 3), generator=G(1000 + 7 * h + w + seed), dtype=torch.uint8)
    if content == 'binary':          # bicubic overshoot must hit clip8 on both sides
        return (torch.randint(0, 2, (b, h, w, 3), generator=G(2000 + 7 * h + w + seed)) * 255).to(torch.uint8)
    return torch.full((b, h, w, 3), 0 if content == 'zeros' else 255, dtype=torch.uint8)


def _in_layout(x, layout):
    return x if layout == 'hwc' else x.permute(0, 3, 1, 2).contiguous()


@functools.lru_cache(maxsize=None)
def _reference(b, shape, content, filter, view=None):
    """The CPU implementation's uint8 result for the shared frames, 'hwc'; computed once per case."""
    (hi, wi), size = shape
    return R.frame_resize_cpu(_frames(b, hi, wi, content), size, filter, 'hwc', view=view)


def _offset_view(t, off, dev=DEV):
    """``t``'s bytes on the device, starting ``off`` bytes into a larger byte buffer."""
    buf = torch.zeros(t.numel() * t.element_size() + 16, dtype=torch.uint8, device=dev)
    view = buf[off:off + t.numel()].view(t.shape)
    view.copy_(t)
    return view


# ---------------------------------------------------------------------------------------------------------------- kernel

@pytest.mark.parametrize('layout', LAYOUTS)
@pytest.mark.parametrize('filter', FILTERS)
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: f'{s[0][0]}x{s[0][1]}-{s[1][0]}x{s[1][1]}')
def test_frame_resize_equals_cpu(shape, filter, layout):
    from hyperseg_amd import functional as HF
    (hi, wi), size = shape
    for b in (1, 2):
        for content in CONTENTS:
            want = _in_layout(_reference(b, shape, content, filter), layout)
            got = HF.frame_resize(_in_layout(_frames(b, hi, wi, content), layout).to(DEV), size, filter, layout)
            assert got.dtype == torch.uint8 and tuple(got.shape) == tuple(want.shape)
            assert torch.equal(got.cpu(), want), (b, content)
    # {0, 255} frames: bicubic's negative lobes overshoot on both sides, so clip8 decides bytes -- wherever a window is narrow enough for it
    # (at 3x down and more a window averages >= 36 binary pixels and saturation no longer occurs; equality above still holds there)
    if filter == 'bicubic' and max(hi / size[0], wi / size[1]) <= 2:
        ref = _reference(1, shape, 'binary', filter)
        assert int((ref == 0).sum()) > 0 and int((ref == 255).sum()) > 0


def test_wide_windows_and_scale_limits():
    """Scales 1/8 and 8 on each axis (bicubic: ksize 33 and 5; bilinear 17 and 3), more than one workgroup on both grid axes, sizes that are
    no multiple of the 64 x 16 tile."""
    from hyperseg_amd import functional as HF
    x = _frames(1, 136, 200, 'noise')
    for size in [(17, 25), (17, 1600), (1088, 25), (70, 131)]:
        for filter in FILTERS:
            for layout in LAYOUTS:
                got = HF.frame_resize(_in_layout(x, layout).to(DEV), size, filter, layout)
                assert torch.equal(got.cpu(), _in_layout(R.frame_resize_cpu(x, size, filter), layout)), (size, filter, layout)


@pytest.mark.parametrize('layout', LAYOUTS)
def test_unaligned_base_and_out_slice(layout):
    from hyperseg_amd import functional as HF
    shape = SHAPES[1]
    (hi, wi), size = shape
    x = _in_layout(_frames(2, hi, wi, 'noise'), layout)
    want = _in_layout(_reference(2, shape, 'noise', 'bicubic'), layout)
    for off in (1, 2, 3):
        assert torch.equal(HF.frame_resize(_offset_view(x, off), size, 'bicubic', layout).cpu(), want)
    big = torch.full((want.numel() + 5,), 77, dtype=torch.uint8, device=DEV)
    sl = big[3:3 + want.numel()].view(want.shape)
    got = HF.frame_resize(x.to(DEV), size, 'bicubic', layout, out=sl)
    assert got is sl and torch.equal(sl.cpu(), want) and bool((big[:3] == 77).all()) and bool((big[-2:] == 77).all())
    with pytest.raises(ValueError):
        HF.frame_resize(x.to(DEV), size, 'bicubic', layout, out=torch.empty(want.shape, device=DEV))       # float out for a uint8 result


VIEWS = [((13, 17), (-4, -5), False), ((13, 16), (-4, 10), True), ((40, 60), (-3, -2), True), ((6, 7), (5, 9), False), ((6, 7), (5, 9), True),
         ((6, 8), (5, 9), True), ((4, 4), (100, 3), False), ((4, 5), (-9, -9), True), ((30, 8), (10, 25), True), ((19, 31), (0, 0), True)]


@pytest.mark.parametrize('layout', LAYOUTS)
def test_views(layout):
    """Negative and positive offsets with fill, a window inside the image, windows wholly outside (all fill), hflip on odd and even widths."""
    from hyperseg_amd import functional as HF
    shape = SHAPES[1]                                     # 37 x 53 -> 19 x 31
    (hi, wi), size = shape
    x = _in_layout(_frames(2, hi, wi, 'noise'), layout).to(DEV)
    for vsize, offset, hflip in VIEWS:
        view = R.ResizeView(vsize, offset, hflip, (11, 22, 233))
        for filter in FILTERS:
            want = _in_layout(_reference(2, shape, 'noise', filter, view), layout)
            got = HF.frame_resize(x, size, filter, layout, view=view)
            assert torch.equal(got.cpu(), want), (vsize, offset, hflip, filter)
    outside = HF.frame_resize(x, size, 'bilinear', layout, view=R.ResizeView((4, 4), (100, 3), False, (11, 22, 233))).cpu()
    fill = torch.tensor([11, 22, 233], dtype=torch.uint8).view((1, 1, 1, 3) if layout == 'hwc' else (1, 3, 1, 1))
    assert torch.equal(outside, fill.expand_as(outside))


@pytest.mark.parametrize('layout', LAYOUTS)
def test_normalised_output_is_the_table_lookup(layout):
    from hyperseg_amd import functional as HF
    from hyperseg_amd import InputNorm
    norm = InputNorm((0.4137, 0.38291, 0.456789), (0.2719, 0.19283, 0.31415), layout=layout)
    for shape in (SHAPES[1], SHAPES[2]):
        (hi, wi), size = shape
        x = _in_layout(_frames(2, hi, wi, 'noise'), layout).to(DEV)
        for view in (None, R.ResizeView((21, 30), (-3, 4), True, (0, 128, 255))):
            u8 = HF.frame_resize(x, size, 'bicubic', layout, view=view)
            fl = HF.frame_resize(x, size, 'bicubic', layout, view=view, norm=norm)
            assert fl.dtype == torch.float32 and tuple(fl.shape) == (2, 3) + tuple(view.size if view else size)
            assert torch.equal(fl, norm.to_float(u8))
            assert torch.equal(fl.cpu(), R.frame_resize_cpu(x.cpu(), size, 'bicubic', layout, view=view, norm=norm))
    big = torch.full((fl.numel() + 3,), float('nan'), device=DEV)                # a destination that is only 4-byte aligned
    sl = big[1:1 + fl.numel()].view(fl.shape)
    HF.frame_resize(x, size, 'bicubic', layout, view=view, norm=norm, out=sl)
    assert torch.equal(sl, fl) and bool(torch.isnan(big[0])) and bool(torch.isnan(big[-2:]).all())


@pytest.mark.parametrize('dtype', [torch.uint8, torch.int64])
def test_label_resize(dtype):
    from hyperseg_amd import functional as HF
    for (hi, wi), size in [((64, 64), (23, 191)), ((128, 256), (333, 777)), ((37, 53), (19, 31)), ((24, 40), (48, 80))]:
        t = torch.randint(0, 256 if dtype == torch.uint8 else 1000, (2, hi, wi), generator=G(hi + wi)).to(dtype)
        got = HF.label_resize(t.to(DEV), size)
        assert got.dtype == dtype and torch.equal(got.cpu(), R.label_resize_cpu(t, size))
    (hi, wi), size = (37, 53), (19, 31)
    t = torch.randint(0, 19, (2, hi, wi), generator=G(5)).to(dtype)
    for vsize, offset, hflip in VIEWS:
        view = R.ResizeView(vsize, offset, hflip)
        want = R.label_resize_cpu(t, size, view=view, fill=255)
        assert torch.equal(HF.label_resize(t.to(DEV), size, view=view, fill=255).cpu(), want)
        other = torch.int64 if dtype == torch.uint8 else torch.uint8              # the other storage type out
        out = torch.empty(want.shape, dtype=other, device=DEV)
        assert torch.equal(HF.label_resize(t.to(DEV), size, view=view, fill=255, out=out).cpu(), want.to(other))
    if dtype == torch.uint8:                                                      # a base pointer that is not even 2-byte aligned
        assert torch.equal(HF.label_resize(_offset_view(t, 3), size).cpu(), R.label_resize_cpu(t, size))


def test_refusals():
    from hyperseg_amd import functional as HF
    from hyperseg_amd import _hip
    x = torch.zeros(1, 8, 8, 3, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError):
        HF.frame_resize(x.float(), (4, 4))                                       # a wrong dtype
    with pytest.raises(ValueError):
        HF.frame_resize(x, (4, 4), layout='chw')                                 # a wrong layout for these frames
    with pytest.raises(ValueError):
        HF.frame_resize(x, (4, 4), layout='nhwc')
    with pytest.raises(ValueError):
        HF.frame_resize(x, (0, 4))                                               # size 0
    with pytest.raises(ValueError):
        HF.frame_resize(x, (4, 4), filter='lanczos')
    with pytest.raises(ValueError):
        HF.label_resize(torch.zeros(1, 8, 8, device=DEV), (4, 4))
    with pytest.raises(ValueError):
        HF.label_resize(torch.zeros(1, 8, 8, dtype=torch.uint8, device=DEV), (4, 0))
    # declined geometries: HS_ERR_UNSUPPORTED, nothing launched -- the output stays as it was
    yb, ykk = R.device_coeffs(8, 4, 'bilinear', DEV)
    y = torch.full((1, 4, 4, 3), 9, dtype=torch.uint8, device=DEV)
    lib, s = _hip.lib, _hip.stream_ptr()
    args = lambda batch, wo: (x.data_ptr(), 0, batch, 8, 8, yb.data_ptr(), ykk.data_ptr(), ykk.shape[1], 4, yb.data_ptr(), ykk.data_ptr(),
                              ykk.shape[1], 4, 4, wo, 0, 0, 0, 0, None, y.data_ptr(), s)
    assert lib.hs_frame_resize_fwd(*args(65536, 4)) == -3
    assert lib.hs_frame_resize_fwd(*args(1, (1 << 19) + 1)) == -3
    assert lib.hs_frame_resize_fwd(*args(1, 0)) == -1                            # HS_ERR_BAD_ARG
    iy = R.device_nearest(8, 4, DEV)
    t = torch.zeros(1, 8, 8, dtype=torch.uint8, device=DEV)
    assert lib.hs_label_resize_fwd(t.data_ptr(), 0, 65536, 8, 8, iy.data_ptr(), 4, iy.data_ptr(), 4, 4, 4, 0, 0, 0, 255, y.data_ptr(), 0, s) == -3
    assert lib.hs_label_resize_fwd(t.data_ptr(), 2, 1, 8, 8, iy.data_ptr(), 4, iy.data_ptr(), 4, 4, 4, 0, 0, 0, 255, y.data_ptr(), 0, s) == -1
    torch.cuda.synchronize()
    assert bool((y == 9).all())


def test_fixture_bytes():
    """The GPU reproduces Pillow's recorded bytes directly."""
    from hyperseg_amd import functional as HF
    ref = load_golden('resample_ref')
    for i, (hi, wi, ho, wo) in enumerate(ref['cases'].tolist()):
        for f in FILTERS:
            assert torch.equal(HF.frame_resize(ref[f'c{i}_in'][None].to(DEV), (ho, wo), f)[0].cpu(), ref[f'c{i}_{f}']), (i, f)
    for i, (hi, wi, ho, wo) in enumerate(ref['label_cases'].tolist()):
        assert torch.equal(HF.label_resize(ref[f'l{i}_in'][None].to(DEV), (ho, wo))[0].cpu(), ref[f'l{i}_out']), i
    for i, (hi, wi, hr, wr, ho, wo, oy, ox, hflip, *fill) in enumerate(ref['view_cases'].tolist()):
        view = R.ResizeView((ho, wo), (oy, ox), bool(hflip), tuple(fill))
        assert torch.equal(HF.frame_resize(ref[f'v{i}_in'][None].to(DEV), (hr, wr), 'bicubic', view=view)[0].cpu(), ref[f'v{i}_bicubic']), i
        assert torch.equal(HF.label_resize(ref[f'v{i}_label_in'][None].to(DEV), (hr, wr), view=view, fill=255)[0].cpu(), ref[f'v{i}_label']), i


# ----------------------------------------------------------------------------------------------------------------- models

@functools.lru_cache(maxsize=None)
def _model(tag):
    from hyperseg_amd import configs
    from hyperseg_amd.utils.inference import prepare_for_inference
    m = fill_by_name(configs.build(MODELS[tag][0]).eval(), seed=11)
    prepare_for_inference(m, fold_bn=False, fused_depthwise=True, split_gemm=True)
    return m.to(DEV)


def _camera(tag, seed, b=1):
    h, w = MODELS[tag][1]
    return torch.randint(0, 256, (b, 2 * h, 2 * w, 3), generator=G(seed), dtype=torch.uint8).to(DEV)


def _label(tag, seed, b=1):
    (h, w), n = MODELS[tag][1:]
    g = G(seed)
    t = torch.randint(0, n, (b, 2 * h, 2 * w), generator=g)
    t[torch.rand(t.shape, generator=g) < 0.10] = 255
    return t.to(DEV)


def _style(n):
    from hyperseg_amd import Overlay
    return Overlay(torch.randint(0, 256, (n, 3), generator=G(77)), layout='hwc')


@pytest.fixture
def served(request):
    """(model, resize, classes) with input_norm and overlay_style attached and input_resize UNSET; all three detached afterwards."""
    from hyperseg_amd import FrameResize, InputNorm
    tag = request.param
    m = _model(tag)
    size, n = MODELS[tag][1:]
    m.input_norm, m.overlay_style = InputNorm(layout='hwc'), _style(n)
    hflip, m.inference_hflip = m.inference_hflip, False      # inert for a single tensor, but overlay() blends in the last launch only without it
    yield tag, m, FrameResize(size, 'bilinear', 'hwc'), n
    m.inference_hflip = hflip
    for name in ('input_norm', 'overlay_style', 'input_resize'):
        m.__dict__.pop(name, None)


@pytest.mark.parametrize('served', ['M', 'Lc'], indirect=True)
def test_model_with_input_resize_equals_resize_then_model(served):
    from hyperseg_amd.fps import ConfusionMatrix
    tag, m, resize, n = served
    size = MODELS[tag][1]
    cam, lbl = _camera(tag, 31), _label(tag, 32)
    small = resize(cam)
    assert tuple(small.shape) == (1,) + size + (3,) and torch.equal(small.cpu(), resize(cam.cpu()))       # same bytes on either device
    cm_want = ConfusionMatrix(n)
    with torch.no_grad():
        want = (m(small), m.segment(small), m.evaluate(small, lbl, cm_want), m.overlay(small))
    m.input_resize = resize
    assert m.frame_size(cam) == size
    cm_got = ConfusionMatrix(n)
    with torch.no_grad():
        got = (m(cam), m.segment(cam), m.evaluate(cam, lbl, cm_got), m.overlay(cam))
    assert torch.equal(got[0], want[0]) and tuple(got[0].shape) == (1, n) + size
    assert torch.equal(got[1], want[1]) and tuple(got[1].shape) == (1,) + size
    assert torch.equal(got[2], want[2]) and tuple(got[2].shape) == tuple(lbl.shape)           # scored at the label's own size
    assert torch.equal(cm_got.mat, cm_want.mat) and int(cm_got.mat.sum()) == int((lbl < n).sum())
    assert torch.equal(got[3][0], want[3][0]) and torch.equal(got[3][1], want[3][1])
    assert tuple(got[3][1].shape) == tuple(small.shape)                                     # blended over the resized frame
    with torch.no_grad():                                                                   # a frame already at the size: untouched
        assert torch.equal(m.segment(small), want[1])


@pytest.mark.parametrize('served', ['M', 'Lc'], indirect=True)
def test_graphed_model_resizes_inside_the_graph(served):
    from hyperseg_amd.utils.inference import GraphedModel
    from hyperseg_amd.fps import ConfusionMatrix
    tag, m, resize, n = served
    m.input_resize = resize
    masks = GraphedModel(m, masks=True, num_classes=n, clone_output=True)
    total = torch.zeros(n, n, dtype=torch.int64, device=DEV)
    for i in range(2):
        cam, lbl = _camera(tag, 40 + i), _label(tag, 50 + i)
        cm = ConfusionMatrix(n)
        with torch.no_grad():
            want = (m.segment(cam), m.evaluate(cam, lbl, cm), m.overlay(cam))
            got = (masks(cam.cpu().pin_memory()), masks.evaluate(cam, lbl), masks.overlay(cam))
        total += cm.mat
        assert torch.equal(got[0], want[0])
        assert torch.equal(got[1], want[1]) and torch.equal(masks.confusion, total)
        assert torch.equal(got[2][0], want[2][0]) and torch.equal(got[2][1], want[2][1])
    assert len(masks._graphs) == 3
    for entry in masks._graphs.values():
        assert entry[1][0].dtype == torch.uint8 and tuple(entry[1][0].shape) == tuple(cam.shape)      # the static buffer holds the camera frame


@pytest.mark.parametrize('served', ['M'], indirect=True)
def test_without_input_resize_nothing_changes(served):
    tag, m, resize, n = served
    assert m.input_resize is None
    cam = _camera(tag, 60)
    assert m.frame_size(cam) == tuple(cam.shape[1:3])
    with torch.no_grad():
        got, want = m.segment(cam), m.segment(m.input_norm.to_float(cam))
    assert tuple(got.shape) == tuple(cam.shape[:3]) and torch.equal(got, want)


# ---------------------------------------------------------------------------------------------------------- device_augment

def _augment_by_steps(frames, labels, scale, crop, offset, hflip, norm, lbl_fill, fill):
    """resize -> pad -> crop -> flip -> ToTensor + Normalize with the CPU implementation, one step at a time."""
    import numpy as np
    b, h, w, _ = frames.shape
    size = tuple(int(s) for s in np.round(np.array((h, w)) * scale).astype(int))
    img = R.frame_resize_cpu(frames, size, 'bicubic', 'hwc')
    lbl = R.label_resize_cpu(labels, size)
    (ch, cw), (oy, ox) = crop, offset
    top, left = max(-oy, 0), max(-ox, 0)
    hc, wc = top + max(size[0], oy + ch), left + max(size[1], ox + cw)
    canvas = torch.tensor(fill, dtype=torch.uint8).view(1, 1, 1, 3).repeat(b, hc, wc, 1)
    lcanvas = torch.full((b, hc, wc), lbl_fill, dtype=lbl.dtype)
    canvas[:, top:top + size[0], left:left + size[1]] = img
    lcanvas[:, top:top + size[0], left:left + size[1]] = lbl
    img = canvas[:, oy + top:oy + top + ch, ox + left:ox + left + cw]
    lbl = lcanvas[:, oy + top:oy + top + ch, ox + left:ox + left + cw]
    if hflip:
        img, lbl = img.flip(2), lbl.flip(2)
    return norm.to_float(img.contiguous()), lbl.contiguous().long()


@pytest.mark.parametrize('scale,crop,offset,hflip', [(0.5, (32, 64), (-5, -9), True), (2.0, (32, 64), (40, 101), False)])
def test_device_augment(scale, crop, offset, hflip):
    from hyperseg_amd import InputNorm
    from hyperseg_amd.training import device_augment
    norm = InputNorm(layout='hwc')
    frames = torch.randint(0, 256, (1, 48, 96, 3), generator=G(90), dtype=torch.uint8)
    labels = torch.randint(0, 19, (1, 48, 96), generator=G(91), dtype=torch.uint8)
    want_img, want_lbl = _augment_by_steps(frames, labels, scale, crop, offset, hflip, norm, 255, (0, 0, 0))
    img, lbl = device_augment(frames.to(DEV), labels.to(DEV), scale, crop, offset, hflip, norm, lbl_fill=255)
    assert img.dtype == torch.float32 and tuple(img.shape) == (1, 3) + crop and lbl.dtype == torch.int64 and tuple(lbl.shape) == (1,) + crop
    assert torch.equal(img.cpu(), want_img) and torch.equal(lbl.cpu(), want_lbl)
    if scale < 1:
        assert int((lbl == 255).sum()) > 0                                                   # the padding is there
    cpu_img, cpu_lbl = device_augment(frames, labels, scale, crop, offset, hflip, norm, lbl_fill=255)
    assert torch.equal(cpu_img, want_img) and torch.equal(cpu_lbl, want_lbl)


def test_fps_harness_resize():
    from hyperseg_amd import fps
    res = fps.main(['--config', 'hyperseg-m', '--iterations', '3', '--distinct', '2', '--prepare', '--graph', '--uint8', '--resize', '256', '512'])
    assert res['input_dtype'] == 'uint8' and res['input_bytes_per_frame'] == 512 * 1024 * 3 and res['frames'] == 3
    assert res['resize'] == [256, 512] and res['camera_size'] == [512, 1024]
