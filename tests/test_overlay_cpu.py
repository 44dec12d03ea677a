"""``hyperseg_amd.Overlay`` on the CPU against the reference's display chain ``tensor2rgb(blend_seg(...))``, recorded in
tests/golden/overlay_ref.npz by tests/golden/make_overlay_golden.py: every comparison is ``np.array_equal`` / ``torch.equal`` -- the
overlay is bytes, no tolerance appears in this file."""
import numpy as np
import pytest
import torch

from conftest import G, load_golden


@pytest.fixture(scope='module')
def ref():
    return load_golden('overlay_ref')


def _case(ref, i, layout='hwc'):
    from hyperseg_amd import Overlay
    style = Overlay(ref[f'case{i}_palette'], alpha=float(ref[f'case{i}_alpha']), ignore_index=int(ref[f'case{i}_ignore']), layout=layout)
    return style, ref[f'case{i}_frames'], ref[f'case{i}_classes'], ref[f'case{i}_expected']


def test_fixture_covers_what_it_should(ref):
    n = int(ref['cases'])
    sizes = {ref[f'case{i}_palette'].shape[0] for i in range(n)}
    assert sizes == {2, 12, 19, 21, 256}
    ignores = {int(ref[f'case{i}_ignore']) for i in range(n)}
    assert 0 in ignores and -1 in ignores and any(v > 0 for v in ignores)
    for i in range(n):
        pal, cl, fr = ref[f'case{i}_palette'], ref[f'case{i}_classes'], ref[f'case{i}_frames']
        assert fr.shape[1] <= 48 and fr.shape[2] <= 64 and fr.dtype == torch.uint8 and cl.dtype == torch.uint8
        if pal.shape[0] < 256:
            assert int(cl.max()) >= pal.shape[0]                  # classes the palette does not cover


def test_blend_equals_reference_on_every_case(ref):
    for i in range(int(ref['cases'])):
        style, frames, classes, want = _case(ref, i)
        got = style.blend(frames, classes)
        assert got.dtype == torch.uint8 and got.shape == frames.shape
        assert np.array_equal(got.numpy(), want.numpy()), f'case {i}: {int((got != want).sum())} bytes differ'


def test_layouts_agree(ref):
    for i in range(int(ref['cases'])):
        hwc, frames, classes, want = _case(ref, i, 'hwc')
        chw = _case(ref, i, 'chw')[0]
        got = chw.blend(frames.permute(0, 3, 1, 2).contiguous(), classes)
        assert got.shape == (frames.shape[0], 3) + tuple(frames.shape[1:3]) and got.is_contiguous()
        assert torch.equal(got.permute(0, 2, 3, 1), want)
        assert torch.equal(got.permute(0, 2, 3, 1), hwc.blend(frames, classes))


@pytest.mark.parametrize('tag,alpha', [('a30', 0.3), ('a50', 0.5), ('a75', 0.75)])
def test_tables_reproduce_the_full_sweep(ref, tag, alpha):
    """All 256 x 256 (frame byte, grey colour) pairs, from the tables alone: uint8(rint(((A[v] + S[c]) * 0.5 + 0.5) * 255))."""
    from hyperseg_amd import Overlay
    greys = torch.arange(256)[:, None].expand(256, 3)
    style = Overlay(greys, alpha=alpha, ignore_index=-1)
    assert style.A.dtype == style.A1.dtype == style.S.dtype == torch.float32
    assert style.A.shape == (256,) and style.A1.shape == (256,) and style.S.shape == (256, 3)
    want = ref[f'sweep_{tag}']
    for ch in range(3):
        got = (((style.A[:, None] + style.S[None, :, ch]) * 0.5 + 0.5) * 255.0).round().to(torch.uint8)
        assert np.array_equal(got.numpy(), want.numpy())
    flat = style.tables()
    assert flat.dtype == torch.float32 and flat.shape == (512 + 3 * 256,)
    assert torch.equal(flat, torch.cat((style.A, style.A1, style.S.flatten())))
    # ... and through blend(): frame pixel [v][c] = (v, v, v) of class c
    v = torch.arange(256, dtype=torch.uint8)
    frames = v[:, None, None].expand(256, 256, 3)[None].contiguous()
    classes = v[None, :].expand(256, 256)[None].contiguous()
    got = style.blend(frames, classes)[0]
    assert all(np.array_equal(got[..., ch].numpy(), want.numpy()) for ch in range(3))


@pytest.mark.parametrize('alpha', [0.0, 0.3, 0.75, 1.0])
def test_unblended_pixels_return_the_frame_byte(alpha):
    from hyperseg_amd import Overlay
    style = Overlay(torch.randint(0, 256, (12, 3), generator=G(1)), alpha=alpha, ignore_index=5)
    v = torch.arange(256, dtype=torch.uint8)
    assert torch.equal(((style.A1 * 0.5 + 0.5) * 255.0).round().to(torch.uint8), v)               # the round trip, all 256 values
    frames = v[None, None, :, None].expand(1, 3, 256, 3).contiguous()
    classes = torch.tensor([5, 12, 255], dtype=torch.uint8)[None, :, None].expand(1, 3, 256).contiguous()      # ignored / beyond / beyond
    assert torch.equal(style.blend(frames, classes), frames)


def test_alpha_zero_changes_nothing_and_alpha_one_paints(ref):
    from hyperseg_amd import Overlay
    pal = torch.randint(0, 256, (19, 3), generator=G(2))
    frames = torch.randint(0, 256, (1, 6, 9, 3), generator=G(3), dtype=torch.uint8)
    classes = torch.randint(0, 19, (1, 6, 9), generator=G(4)).to(torch.uint8)
    assert torch.equal(Overlay(pal, alpha=0.0, ignore_index=-1).blend(frames, classes), frames)
    painted = Overlay(pal, alpha=1.0, ignore_index=-1).blend(frames, classes)
    # the reference's colour scale is 1 / 128: colour c shows as rint(c * 255 / 256)
    want = (((pal.float() / 128 - 1) * 0.5 + 0.5) * 255).round().to(torch.uint8)[classes.long()]
    assert torch.equal(painted, want)


def test_argument_validation():
    from hyperseg_amd import Overlay
    pal = torch.randint(0, 256, (12, 3), generator=G(5))
    for bad in (torch.zeros(12, 4, dtype=torch.long), torch.zeros(12, dtype=torch.long), torch.zeros(0, 3, dtype=torch.long),
                torch.zeros(2, 3, 3, dtype=torch.long)):
        with pytest.raises(ValueError, match='color_map must be'):
            Overlay(bad)
    for value in (-1, 256):
        bad = pal.clone()
        bad[7, 1] = value
        with pytest.raises(ValueError, match=r'\[0, 255\]'):
            Overlay(bad)
    with pytest.raises(ValueError, match=r'\[0, 255\]'):
        Overlay(pal.float() / 255)
    with pytest.raises(ValueError, match='at most 256'):
        Overlay(torch.zeros(257, 3, dtype=torch.long))
    for alpha in (-0.01, 1.01, float('nan')):
        with pytest.raises(ValueError, match='alpha'):
            Overlay(pal, alpha=alpha)
    with pytest.raises(ValueError, match='layout'):
        Overlay(pal, layout='nhwc')
    for ignore in (12, -2, 255, 0.5):
        with pytest.raises(ValueError, match='ignore_index'):
            Overlay(pal, ignore_index=ignore)
    style = Overlay(pal.tolist())                                  # a list of lists is a palette too
    assert (style.alpha, style.ignore_index, style.layout, style.num_colors) == (0.75, 0, 'hwc', 12)
    frames = torch.zeros(2, 8, 10, 3, dtype=torch.uint8)
    masks = torch.zeros(2, 8, 10, dtype=torch.uint8)
    style.blend(frames, masks)
    with pytest.raises(ValueError, match='masks have shape'):
        style.blend(frames, masks[:, :, :9])
    with pytest.raises(ValueError, match='masks have shape'):
        style.blend(frames, masks[:1])
    with pytest.raises(ValueError, match='uint8'):
        style.blend(frames, masks.long())
    with pytest.raises(ValueError, match='uint8 frames'):
        style.blend(frames.float(), masks)
    with pytest.raises(ValueError, match='uint8 frames'):
        style.blend(frames.permute(0, 3, 1, 2).contiguous(), masks)             # a 'chw' frame


def _tiny_model():
    from hyperseg_amd import configs
    from hyperseg_amd.utils.synthetic import fill_by_name
    return fill_by_name(configs.build('hyperseg-m').eval(), seed=3)


def test_model_overlay_argument_errors_and_state_dict():
    from hyperseg_amd import InputNorm, Overlay
    m = _tiny_model()
    before = {k: v.clone() for k, v in m.state_dict().items()}
    x = torch.zeros(1, 3, 64, 128)
    with pytest.raises(TypeError, match='style'):
        m.overlay(x, frames=torch.zeros(1, 64, 128, 3, dtype=torch.uint8))
    m.overlay_style = Overlay(torch.randint(0, 256, (19, 3), generator=G(6)))
    with pytest.raises(TypeError, match='frames='):
        m.overlay(x)                                               # a float x without frames
    with pytest.raises(ValueError, match='frames are'):
        m.overlay(x, frames=torch.zeros(1, 64, 120, 3, dtype=torch.uint8))
    m.input_norm = InputNorm(layout='chw')
    with pytest.raises(ValueError, match="'chw'"):
        m.overlay(torch.zeros(1, 3, 64, 128, dtype=torch.uint8))   # the style blends over 'hwc' frames
    after = m.state_dict()
    assert list(after) == list(before) and all(torch.equal(after[k], before[k]) for k in before)
    assert not any('overlay' in k for k in after)


def test_score_and_overlay_are_mutually_exclusive():
    from hyperseg_amd.models._common import Blend, Epilogue, Score
    score, blend = Score(None, 3, None, False), Blend(None, None, None)
    with pytest.raises(ValueError, match='one of them'):
        Epilogue(score=score, blend=blend)
    with pytest.raises(ValueError):
        Epilogue(ignore_index=255)                                 # a loss without a score
    with pytest.raises(ValueError):
        Epilogue(blend=blend, ignore_index=255)                    # a loss with a blend
