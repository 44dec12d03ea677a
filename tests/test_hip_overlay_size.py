"""Overlays served at another size than the model's frame (csrc/hs_overlay.hip: hs_upsample2_overlay_fwd): ``functional.upsample2_overlay``
against ``upsample2_argmax``, the standalone overlay launch, the CPU blend and the device-made composed logits; the raw entry's guard regions
and refusals; and ``model.overlay(size=)`` / ``GraphedModel.overlay(size=)`` against ``segment(size=)`` + the standalone launch over the camera
frame.  Masks are class indices and overlays are bytes: every comparison is ``torch.equal``, no tolerance appears in this file.

The model tests run with ``torch.backends.cudnn.deterministic = True``, as tests/test_hip_overlay.py does and for its reason."""
import ctypes as C
import functools

import pytest
import torch

from conftest import G
from hyperseg_amd.utils.synthetic import fill_by_name

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
OK, UNSUPPORTED = 0, -3
GUARD = 0xA5

# form -> (source, mid, out)
FORMS = {
    '2x2x': ((6, 8), (12, 16), (24, 32)),                   # both stages exact 2x: the quad form
    '2x2x_odd_wi': ((5, 7), (10, 14), (20, 28)),            # both 2x, odd Wi: the general form
    'general_wo21': ((6, 8), (12, 16), (16, 21)),           # Wo no multiple of 4: an odd row pitch in 'hwc'
    'down': ((6, 8), (12, 16), (9, 10)),                    # a down-sampling second stage
    'tail1': ((3, 4), (6, 8), (7, 5)),                      # a single-pixel-wide tail
}
PAIRS = [(2, 2), (19, 19), (21, 21), (19, 12)]              # (channels, palette): the last has classes beyond the palette


@pytest.fixture(autouse=True)
def deterministic_stock_convolutions(monkeypatch):
    monkeypatch.setattr(torch.backends.cudnn, 'deterministic', True)


def _style(n, layout='hwc', ignore=None, seed=0):
    from hyperseg_amd import Overlay
    ignore = n // 2 if ignore is None else ignore            # inside the palette
    return Overlay(torch.randint(0, 256, (n, 3), generator=G(7000 + n + seed)), alpha=(0.75, 0.5, 0.3)[n % 3], ignore_index=ignore, layout=layout)


def _frames(b, h, w, seed, layout='hwc'):
    """Random uint8 frames that hold the bytes 0 and 255."""
    x = torch.randint(0, 256, (b, h, w, 3), generator=G(seed), dtype=torch.uint8)
    flat = x.view(b, -1)
    flat[:, 0], flat[:, -1] = 0, 255
    flat[:, flat.shape[1] // 2], flat[:, flat.shape[1] // 2 + 1] = 255, 0
    return x if layout == 'hwc' else x.permute(0, 3, 1, 2).contiguous()


def _logits(b, c, h, w, seed):
    return (torch.randn(b, c, h, w, generator=G(seed)) * 3).contiguous()


# ---------------------------------------------------------------------------------------------------------------------- kernel

@pytest.mark.parametrize('layout', ['hwc', 'chw'])
@pytest.mark.parametrize('form', list(FORMS))
def test_upsample2_overlay_equals_argmax_then_overlay(form, layout):
    from hyperseg_amd import functional as HF
    (hi, wi), mid, size = FORMS[form]
    b = 2
    for c, n in PAIRS:
        style = _style(n, layout)
        x = _logits(b, c, hi, wi, 31 * hi + size[1] + c).to(DEV)
        frames = _frames(b, *size, 100 + size[0] + c, layout)
        assert int(frames.min()) == 0 and int(frames.max()) == 255
        src = frames.to(DEV)
        masks, over = HF.upsample2_overlay(x, mid, size, src, style)
        assert masks.dtype == torch.uint8 and tuple(masks.shape) == (b, *size)
        assert over.dtype == torch.uint8 and over.shape == frames.shape and over.data_ptr() != src.data_ptr()
        # 1. the masks of the masks-only call
        assert torch.equal(masks, HF.upsample2_argmax(x, mid, size))
        # 2. the overlay of the standalone launch and of the CPU blend
        assert torch.equal(over, HF.overlay(masks, src, style))
        assert torch.equal(over.cpu(), style.blend(frames.cpu(), masks.cpu()))
        # 3. the same from the device-made composed logits
        composed = HF.upsample_bilinear(HF.upsample_bilinear(x, mid), size).argmax(1).to(torch.uint8)
        assert torch.equal(masks, composed)
        assert torch.equal(over, HF.overlay(composed, src, style))
        assert torch.equal(over.cpu(), style.blend(frames.cpu(), composed.cpu()))
        assert torch.equal(src.cpu(), frames)                                         # the frame is read, never written
        if n < c:
            assert bool((masks >= n).any())                                           # classes beyond the palette keep the frame's byte


def _guarded(t, off, slack=16):
    """(buffer, view): ``t``'s bytes ``off`` bytes into a guard-filled byte buffer on the device."""
    buf = torch.full((t.numel() + slack,), GUARD, dtype=torch.uint8, device=DEV)
    assert buf.data_ptr() % 4 == 0
    view = buf[off:off + t.numel()].view(t.shape)
    view.copy_(t)
    return buf, view


def _guards_hold(buf, off, n):
    return bool((buf[:off] == GUARD).all()) and bool((buf[off + n:] == GUARD).all())


def _raw(x, mid, size, frames, style, mask, out):
    from hyperseg_amd import _hip
    b, c, hi, wi = x.shape
    tables = style.tables(DEV)
    return _hip.lib.hs_upsample2_overlay_fwd(
        C.c_void_p(x.data_ptr()), b, c, hi, wi, *mid, *size, C.c_void_p(frames.data_ptr()), 0 if style.layout == 'hwc' else 1,
        C.c_void_p(tables.data_ptr()), style.num_colors, style.ignore_index, C.c_void_p(mask.data_ptr()), C.c_void_p(out.data_ptr()),
        C.c_void_p(torch.cuda.current_stream().cuda_stream))


@pytest.mark.parametrize('layout', ['hwc', 'chw'])
@pytest.mark.parametrize('form', list(FORMS))
def test_raw_entry_unaligned_operands_stay_inside_their_regions(form, layout):
    """frames and overlay 3 bytes into guard-filled buffers, in the general forms the mask 5 bytes in: the same bytes, nothing written outside.
    The 2x o 2x form stores the masks as dwords: an unaligned mask is refused with nothing launched."""
    from hyperseg_amd import functional as HF
    (hi, wi), mid, size = FORMS[form]
    b, c = 2, 19
    style = _style(c, layout)
    x = _logits(b, c, hi, wi, 77 + hi).to(DEV)
    frames = _frames(b, *size, 200 + size[1], layout)
    want_masks, want = HF.upsample2_overlay(x, mid, size, frames.to(DEV), style)
    quad = form == '2x2x'
    fbuf, fview = _guarded(frames, 3)
    obuf, oview = _guarded(torch.full_like(frames, GUARD), 3)
    moff = 0 if quad else 5
    mbuf, mview = _guarded(torch.full((b, *size), GUARD, dtype=torch.uint8), moff)
    if quad:
        ubuf, uview = _guarded(torch.full((b, *size), GUARD, dtype=torch.uint8), 5)
        assert _raw(x, mid, size, fview, style, uview, oview) == UNSUPPORTED
        torch.cuda.synchronize()
        assert bool((ubuf == GUARD).all()) and bool((obuf == GUARD).all())
    assert _raw(x, mid, size, fview, style, mview, oview) == OK
    torch.cuda.synchronize()
    assert torch.equal(mview, want_masks) and torch.equal(oview, want)
    assert _guards_hold(mbuf, moff, want_masks.numel()) and _guards_hold(obuf, 3, want.numel())
    assert torch.equal(fview.cpu(), frames) and _guards_hold(fbuf, 3, frames.numel())


def test_raw_entry_refusals():
    (hi, wi), mid, size = FORMS['general_wo21']
    style = _style(19)
    x = _logits(1, 19, hi, wi, 5).to(DEV)
    frames = _frames(1, *size, 6).to(DEV)
    mask = torch.full((1, *size), GUARD, dtype=torch.uint8, device=DEV)
    out = torch.full_like(frames, GUARD)
    from hyperseg_amd import _hip
    call = _hip.lib.hs_upsample2_overlay_fwd
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    good = dict(x=x, batch=1, channels=19, Hi=hi, Wi=wi, Hm=mid[0], Wm=mid[1], Ho=size[0], Wo=size[1], frames=frames, layout=0,
                tables=style.tables(DEV), ncol=19, ignore=style.ignore_index, mask=mask, out=out)

    def status(**changed):
        a = {**good, **changed}
        return call(ptr(a['x']), a['batch'], a['channels'], a['Hi'], a['Wi'], a['Hm'], a['Wm'], a['Ho'], a['Wo'], ptr(a['frames']), a['layout'],
                    ptr(a['tables']), a['ncol'], a['ignore'], ptr(a['mask']), ptr(a['out']), C.c_void_p(torch.cuda.current_stream().cuda_stream))

    for name in ('x', 'frames', 'tables', 'mask', 'out'):
        assert status(**{name: None}) == -1, name
    for name in ('batch', 'channels', 'Hi', 'Wi', 'Hm', 'Wm', 'Ho', 'Wo', 'ncol'):
        assert status(**{name: 0}) == -1, name
    assert status(layout=2) == -1 and status(ncol=257) == -1
    assert status(channels=257) == UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((mask == GUARD).all()) and bool((out == GUARD).all())
    assert status() == OK
    torch.cuda.synchronize()


def test_wrapper_identity_stages_out_and_refusals():
    from hyperseg_amd import functional as HF
    style = _style(19)
    x = _logits(2, 19, 6, 8, 9).to(DEV)
    frames = _frames(2, 13, 18, 10).to(DEV)
    want = HF.upsample_overlay(x, (13, 18), frames, style)
    for mid in ((6, 8), (13, 18)):                                                    # first / second stage the identity
        got = HF.upsample2_overlay(x, mid, (13, 18), frames, style)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    (hi, wi), mid, size = FORMS['2x2x']
    frames = _frames(2, *size, 11).to(DEV)
    masks, over = HF.upsample2_overlay(x, mid, size, frames, style)
    out = torch.full_like(frames, 9)
    m2, o2 = HF.upsample2_overlay(x, mid, size, frames, style, out=out)
    assert o2 is out and torch.equal(m2, masks) and torch.equal(out, over)
    before = out.clone()
    refused = [
        lambda: HF.upsample2_overlay(x, mid, (24, 28), frames, style),                                   # frames of another size
        lambda: HF.upsample2_overlay(x, mid, size, frames.cpu(), style),                                 # ... on another device
        lambda: HF.upsample2_overlay(x, mid, size, frames.float(), style),                               # ... of another dtype
        lambda: HF.upsample2_overlay(x, mid, size, frames.permute(0, 3, 1, 2).contiguous(), style),      # ... in another layout
        lambda: HF.upsample2_overlay(torch.zeros(2, 257, 6, 8, device=DEV), mid, size, frames, _style(256)),
        lambda: HF.upsample2_overlay(x, mid, size, frames, style, out=torch.empty(2, 32, 24, 3, dtype=torch.uint8, device=DEV).transpose(1, 2)),
        lambda: HF.upsample2_overlay(x, mid, size, frames, style, out=frames),                           # out aliasing the frames
        lambda: HF.upsample2_overlay(x, (0, 16), size, frames, style),
    ]
    for call in refused:
        with pytest.raises(ValueError):
            call()
    assert torch.equal(out, before) and torch.equal(frames.cpu(), _frames(2, *size, 11))


# ---------------------------------------------------------------------------------------------------------------------- models

# tag -> (config, model frame, classes): tests/test_hip_overlay.py's small frames; L (v0_1) has no final resize
MODELS = {'M': ('hyperseg-m', (256, 512), 19), 'Sc': ('hyperseg-s-camvid', (192, 256), 12), 'S': ('hyperseg-s', (256, 512), 19),
          'L': ('hyperseg-l', (256, 256), 21)}


@functools.lru_cache(maxsize=None)
def _model(tag):
    from hyperseg_amd import configs
    from hyperseg_amd.utils.inference import prepare_for_inference
    m = fill_by_name(configs.build(MODELS[tag][0]).eval(), seed=11)
    prepare_for_inference(m, fold_bn=False, fused_depthwise=True, split_gemm=True)
    return m.to(DEV)


def _dress(m, tag, layout='hwc', hflip=False):
    from hyperseg_amd import FrameResize, InputNorm
    (h, w), n = MODELS[tag][1:]
    m.input_norm = InputNorm(layout=layout)
    m.input_resize = FrameResize((h, w), 'bilinear', layout)
    m.overlay_style = _style(max(2, n - 2), layout, ignore=0)
    m.inference_hflip = hflip
    return m.overlay_style


def _undress(m):
    m.input_norm = m.overlay_style = m.input_resize = None
    m.inference_hflip = True                      # the configs' value


def _composed(m, x, frames_dev, style, size):
    """The composed route: ``segment(size=)``, then the standalone launch over the frames."""
    from hyperseg_amd import functional as HF
    masks = m.segment(x, size=size)
    return masks, HF.overlay(masks, frames_dev, style)


@pytest.mark.parametrize('tag', list(MODELS))
def test_model_overlay_at_camera_size_eager_and_graphed(tag):
    from hyperseg_amd.utils.inference import GraphedModel
    m = _model(tag)
    (h, w), n = MODELS[tag][1:]
    cam = (2 * h, 2 * w)
    style = _dress(m, tag)
    try:
        graphed = GraphedModel(m, masks=True, clone_output=True)
        seen = []
        for i in range(2):
            camera = _frames(1, *cam, 300 + i).to(DEV)
            want_masks, want = _composed(m, camera, camera, style, cam)
            assert tuple(want_masks.shape) == (1, *cam)
            masks, over = m.overlay(camera, size=cam)
            assert masks.dtype == torch.uint8 and torch.equal(masks, want_masks)
            assert over.dtype == torch.uint8 and over.shape == camera.shape and torch.equal(over, want)
            gm, go = graphed.overlay(camera, size=cam)                                # the second pass: a replay with another frame
            assert torch.equal(gm, want_masks) and torch.equal(go, want)
            seen.append(go)
        assert len(graphed._graphs) == 1 and not torch.equal(seen[0], seen[1])
        gm, go = graphed.overlay(camera.cpu().pin_memory(), size=cam)                 # staged from pinned host memory
        assert torch.equal(gm, want_masks) and torch.equal(go, want)
        # no size=: what the call gave before the argument existed
        small = m.resized(camera)
        old = m.overlay(small)
        for got in (m.overlay(camera), m.overlay(camera, size=(h, w), frames=small), graphed.overlay(camera)):
            assert tuple(got[0].shape) == (1, h, w) and torch.equal(got[0], old[0]) and torch.equal(got[1], old[1])
        # a size that is no multiple of the frame, with frames=
        odd = (300, 500)
        frames = _frames(1, *odd, 310).to(DEV)
        want_masks, want = _composed(m, camera, frames, style, odd)
        for got in (m.overlay(camera, frames=frames, size=odd), graphed.overlay(camera, frames=frames, size=odd)):
            assert torch.equal(got[0], want_masks) and torch.equal(got[1], want)
        with pytest.raises(ValueError, match='300'):
            m.overlay(camera, size=odd)                                               # no frames of that size
        with pytest.raises(ValueError, match='300'):
            graphed.overlay(camera, size=odd)
        with pytest.raises(ValueError):
            m.overlay(camera, frames=small, size=cam)
    finally:
        _undress(m)


@pytest.mark.parametrize('tag', ['M', 'L'])
def test_fallback_routes_give_the_composed_bytes(tag):
    from hyperseg_amd import functional as HF
    m = _model(tag)
    (h, w), n = MODELS[tag][1:]
    cam = (2 * h, 2 * w)
    style = _dress(m, tag)
    try:
        camera = _frames(1, *cam, 400).to(DEV)
        want_masks, want = _composed(m, camera, camera, style, cam)
        # a float x with frames=: the fused route from the same decoder input
        ref = m.input_norm.to_float(m.resized(camera))
        fm, fo = m.overlay(ref, frames=camera, size=cam)
        assert torch.equal(fm, want_masks) and torch.equal(fo, want)
        # frames on the host: logits, resize, arg-max, blend
        cm, co = m.overlay(ref, frames=camera.cpu(), size=cam)
        assert torch.equal(cm, want_masks) and torch.equal(co, want)
        with pytest.raises(ValueError, match=str(cam[0])):
            m.overlay(ref, size=cam)
        # h-flip inference: the logits route, its own masks, the same blend
        m.inference_hflip = True
        hm, ho = m.overlay(camera, size=cam)
        assert torch.equal(hm, m.segment(camera, size=cam)) and torch.equal(ho, HF.overlay(hm, camera, style))
        assert torch.equal(hm, want_masks)                                            # (a tensor input is never flipped)
    finally:
        _undress(m)
