"""Overlays at another size than the model's frame, without a GPU: the route table of ``Epilogue.apply`` for a ``Blend`` with a size (pinned on
recorders, as tests/test_epilogue_cpu.py pins the others), which frames ``model.overlay(size=)`` blends over, and the argument checks of
``hyperseg_amd.fps --overlay-at-camera``."""
import pytest
import torch

from conftest import G
from hyperseg_amd import functional as HF
from hyperseg_amd.models._common import Blend, Epilogue

SIZE, CAMERA = (8, 8), (16, 16)
ENTRIES = {'upsample_overlay': ('blended_masks', 'overlay'), 'upsample2_overlay': ('blended_masks2', 'overlay2')}


@pytest.fixture
def calls(monkeypatch):
    made = []
    for name, result in ENTRIES.items():
        monkeypatch.setattr(HF, name, lambda *args, _name=name, _result=result, **kwargs: made.append((_name, args, kwargs)) or _result,
                            raising=False)
    return made


def _one(calls):
    assert len(calls) == 1, calls
    return calls.pop()


def test_blend_keeps_its_three_field_form():
    blend = Blend('frames', 'style', 'out')
    assert blend.size is None and blend == Blend('frames', 'style', 'out', None)
    assert Blend('frames', 'style', 'out', CAMERA).size == CAMERA and Blend._fields == ('frames', 'style', 'out', 'size')


def test_blend_routes(calls):
    p, at_size = torch.zeros(1, 3, 4, 4), torch.zeros(1, 3, *SIZE)
    frames, style, out = object(), object(), object()
    # no size, or the frame's: today's call
    for blend in (Blend(frames, style, out), Blend(frames, style, out, None), Blend(frames, style, out, SIZE), Blend(frames, style, out, list(SIZE))):
        assert Epilogue(blend=blend).apply(p, SIZE) == ('blended_masks', 'overlay')
        assert _one(calls) == ('upsample_overlay', (p, SIZE, frames, style), dict(out=out))
    # another size: both resizes composed
    assert Epilogue(blend=Blend(frames, style, out, CAMERA)).apply(p, SIZE) == ('blended_masks2', 'overlay2')
    assert _one(calls) == ('upsample2_overlay', (p, SIZE, CAMERA, frames, style), dict(out=out))
    assert Epilogue(blend=Blend(frames, style, out, list(CAMERA))).apply(p, SIZE) == ('blended_masks2', 'overlay2')
    assert _one(calls) == ('upsample2_overlay', (p, SIZE, CAMERA, frames, style), dict(out=out))
    # p at the frame's size already (no final resize): one stage, straight to the frames' size
    assert Epilogue(blend=Blend(frames, style, out, CAMERA)).apply(at_size, SIZE) == ('blended_masks', 'overlay')
    assert _one(calls) == ('upsample_overlay', (at_size, CAMERA, frames, style), dict(out=out))
    # the overlay's size travels in the Blend: another out_size is refused as it always was
    with pytest.raises(ValueError, match='out_size'):
        Epilogue(blend=Blend(frames, style, out, CAMERA), out_size=CAMERA).apply(p, SIZE)
    assert calls == []


# ----------------------------------------------------------------------------------------------------- which frames are blended over

FRAME, CLASSES = (16, 32), 19


def _u8(b, h, w, seed):
    return torch.randint(0, 256, (b, h, w, 3), generator=G(seed), dtype=torch.uint8)


@pytest.fixture(scope='module')
def model():
    """A CPU model whose forward is a recorder's: seeded logits at the frame's size (the route under test starts after the logits)."""
    from hyperseg_amd import InputNorm, Overlay, configs
    m = configs.build('hyperseg-m').eval()
    m.input_norm = InputNorm(layout='hwc')
    m.overlay_style = Overlay(torch.randint(0, 256, (CLASSES - 2, 3), generator=G(1)), ignore_index=3)
    m.inference_hflip = False
    m.logits = torch.randn(1, CLASSES, *FRAME, generator=G(2)) * 3
    # forward() and segment()'s same-size route both go through here
    m.process_single_tensor = lambda x, hflip=False, epilogue=None: m.logits if epilogue is None else m.logits.argmax(1).to(torch.uint8)
    return m


def _want(m, frames, size):
    logits = m.logits if tuple(size) == FRAME else torch.nn.functional.interpolate(m.logits, size=size, mode='bilinear')
    masks = logits.argmax(1).to(torch.uint8)
    return masks, m.overlay_style.blend(frames, masks)


def _same(got, want):
    return got[0].dtype == torch.uint8 and torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_frames_selection_on_a_cpu_model(model):
    from hyperseg_amd import FrameResize
    m = model
    cam = (2 * FRAME[0], 2 * FRAME[1])
    camera, small, other = _u8(1, *cam, 3), _u8(1, *FRAME, 4), _u8(1, 20, 30, 5)
    ref = torch.zeros(1, 3, *FRAME)
    try:
        # 1. frames=, whatever x is
        assert _same(m.overlay(ref, frames=camera, size=cam), _want(m, camera, cam))
        assert _same(m.overlay(small, frames=other, size=(20, 30)), _want(m, other, (20, 30)))
        # 2. a uint8 x of that size: the frame itself where there is no resize ...
        assert _same(m.overlay(small, size=FRAME), _want(m, small, FRAME))
        assert _same(m.overlay(small, size=FRAME), m.overlay(small))
        # ... and the camera frame, before input_resize
        m.input_resize = FrameResize(FRAME, 'bilinear', 'hwc')
        assert _same(m.overlay(camera, size=cam), _want(m, camera, cam))
        assert _same(m.overlay(camera, frames=other, size=(20, 30)), _want(m, other, (20, 30)))         # frames= comes first
        out = torch.zeros_like(camera)
        got = m.overlay(camera, size=cam, out=out)
        assert got[1] is out and _same(got, _want(m, camera, cam))
        # no size=: over the resized frame, as before
        assert _same(m.overlay(camera), _want(m, m.resized(camera), FRAME))
        assert _same(m.overlay(camera, size=FRAME, frames=m.resized(camera)), m.overlay(camera))
        # 3. nothing of that size: an error that names both sizes
        with pytest.raises(ValueError) as err:
            m.overlay(camera, size=(20, 30))
        assert '(20, 30)' in str(err.value) and str(cam) in str(err.value)
        with pytest.raises(ValueError) as err:
            m.overlay(ref, size=cam)                                                                    # a float x is no frame
        assert str(cam) in str(err.value) and str(FRAME) in str(err.value)
        with pytest.raises(ValueError, match='frames are'):
            m.overlay(camera, frames=small, size=cam)                                                   # frames of another size than size=
    finally:
        m.input_resize = None


# ------------------------------------------------------------------------------------------------------------------------ fps

@pytest.mark.parametrize('argv', [
    ['--uint8', '--resize', '64', '128', '--overlay-at-camera'],                      # without --overlay
    ['--uint8', '--overlay', '--overlay-at-camera'],                                  # without --resize
    ['--overlay-at-camera'],
])
def test_fps_refuses_overlay_at_camera_without_its_companions(argv):
    from hyperseg_amd import fps
    with pytest.raises(SystemExit, match='--overlay-at-camera'):
        fps.main(argv)
