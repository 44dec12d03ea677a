"""Served overlays on the GPU (csrc/hs_overlay.hip): ``functional.overlay`` against ``Overlay.blend`` on the CPU -- itself checked against the
reference's ``tensor2rgb(blend_seg(...))`` in tests/test_overlay_cpu.py --, ``functional.upsample_overlay`` against ``upsample_argmax`` and the
standalone launch, and ``model.overlay`` / ``GraphedModel.overlay`` against ``segment()`` + the CPU blend.  The overlay is bytes and the masks are
class indices, so every comparison is ``torch.equal``: no tolerance appears in this file.

The whole file runs with ``torch.backends.cudnn.deterministic = True``: two forwards are compared bit for bit, and with PyTorch's default the
float forward does not repeat itself wherever a stock convolution runs (profiles/float_repeatability.txt; tests/test_hip_ingest.py)."""
import functools

import pytest
import torch

from conftest import G, load_golden
from hyperseg_amd.utils.synthetic import fill_by_name

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
# tag -> (config, a frame size of the config's aspect the encoder strides divide, classes): tests/test_hip_ingest.py's
MODELS = {'M': ('hyperseg-m', (256, 512), 19), 'S': ('hyperseg-s', (256, 512), 19), 'Sc': ('hyperseg-s-camvid', (192, 256), 12),
          'Lc': ('hyperseg-l-camvid', (384, 512), 12), 'L': ('hyperseg-l', (256, 256), 21)}
PALETTE_SIZES = (2, 12, 19, 21, 256)              # the fixture's


@pytest.fixture(autouse=True)
def deterministic_stock_convolutions(monkeypatch):
    monkeypatch.setattr(torch.backends.cudnn, 'deterministic', True)


def _style(n, layout='hwc', alpha=0.75, ignore=0, seed=0):
    from hyperseg_amd import Overlay
    return Overlay(torch.randint(0, 256, (n, 3), generator=G(5000 + n + seed)), alpha=alpha, ignore_index=ignore, layout=layout)


def _frames(b, h, w, seed):
    """uint8 (B, H, W, 3) frames; where the frame has room they hold all 256 values."""
    x = torch.randint(0, 256, (b, h, w, 3), generator=G(seed), dtype=torch.uint8)
    if h * w * 3 >= 256:
        x.view(b, -1)[:, :256] = torch.randperm(256, generator=G(seed + 1)).to(torch.uint8)
    return x


def _classes(b, h, w, n, seed):
    """uint8 class maps in patches (label maps are coherent), with classes the palette does not cover where there are any."""
    g = G(seed)
    coarse = torch.randint(0, n, (b, -(-h // 3), -(-w // 5)), generator=g)
    cl = coarse.repeat_interleave(3, 1).repeat_interleave(5, 2)[:, :h, :w].contiguous()
    noise = torch.rand((b, h, w), generator=g) < 0.2
    cl[noise] = torch.randint(0, n, (int(noise.sum()),), generator=g)
    if n < 256:
        beyond = torch.rand((b, h, w), generator=g) < 0.1
        cl[beyond] = torch.randint(n, 256, (int(beyond.sum()),), generator=g)
    return cl.to(torch.uint8)


def _in_layout(frames_hwc, layout):
    return frames_hwc if layout == 'hwc' else frames_hwc.permute(0, 3, 1, 2).contiguous()


def _offset_view(t, off):
    """``t``'s bytes on the device, starting ``off`` bytes into a larger byte buffer: a sliced, still contiguous view."""
    buf = torch.zeros(t.numel() + 8, dtype=torch.uint8, device=DEV)
    view = buf[off:off + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 4 == (buf.data_ptr() + off) % 4
    return view


# ---------------------------------------------------------------------------------------------------------------- standalone

SIZES = [(1, 1), (1, 5), (3, 6), (2, 7), (5, 4), (37, 53), (48, 64), (64, 129), (512, 1024)]


@pytest.mark.parametrize('layout', ['hwc', 'chw'])
@pytest.mark.parametrize('h,w', SIZES)
def test_overlay_equals_cpu_blend(layout, h, w):
    from hyperseg_amd import functional as HF
    for b in (1, 2):
        for n in PALETTE_SIZES if h * w <= 4096 else (19,):
            style = _style(n, layout, alpha=(0.75, 0.5, 0.3)[n % 3], ignore=(0, n // 2, -1)[(n + b) % 3])
            frames, cl = _in_layout(_frames(b, h, w, 10 * h + w + b), layout), _classes(b, h, w, n, 7 * h + w + n)
            want = style.blend(frames, cl)
            src = frames.to(DEV)
            got = HF.overlay(cl.to(DEV), src, style)
            assert got.dtype == torch.uint8 and got.shape == frames.shape and got.data_ptr() != src.data_ptr()
            assert torch.equal(got.cpu(), want)
            assert torch.equal(src.cpu(), frames)                                          # the frame is read, never written
            assert torch.equal(style.blend(src, cl.to(DEV)).cpu(), want)                   # Overlay.blend on the device: the same launch


@pytest.mark.parametrize('layout', ['hwc', 'chw'])
@pytest.mark.parametrize('h,w', [(37, 53), (9, 8), (6, 13), (64, 128)])
def test_overlay_unaligned_base_pointers_and_out(layout, h, w):
    from hyperseg_amd import functional as HF
    style = _style(19, layout)
    frames, cl = _in_layout(_frames(2, h, w, 3 * h + w), layout), _classes(2, h, w, 19, h + w)
    want = style.blend(frames, cl)
    for off in (1, 2, 3):
        assert torch.equal(HF.overlay(_offset_view(cl, off), frames.to(DEV), style).cpu(), want)
        assert torch.equal(HF.overlay(cl.to(DEV), _offset_view(frames, off), style).cpu(), want)
        big = torch.full((want.numel() + 8,), 77, dtype=torch.uint8, device=DEV)
        out = big[off:off + want.numel()].view(want.shape)
        assert HF.overlay(cl.to(DEV), frames.to(DEV), style, out=out) is out
        assert torch.equal(out.cpu(), want) and bool((big[:off] == 77).all()) and bool((big[off + want.numel():] == 77).all())
    src = frames.to(DEV)
    with pytest.raises(ValueError, match='overlaps'):
        HF.overlay(cl.to(DEV), src, style, out=src)
    with pytest.raises(ValueError, match='out must be'):
        HF.overlay(cl.to(DEV), src, style, out=torch.empty(want.shape, device=DEV))


def test_overlay_on_the_fixture_cases():
    """The reference's own bytes, straight from the device."""
    from hyperseg_amd import Overlay
    from hyperseg_amd import functional as HF
    ref = load_golden('overlay_ref')
    seen = set()
    for i in range(int(ref['cases'])):
        pal = ref[f'case{i}_palette']
        seen.add(pal.shape[0])
        for layout in ('hwc', 'chw'):
            style = Overlay(pal, alpha=float(ref[f'case{i}_alpha']), ignore_index=int(ref[f'case{i}_ignore']), layout=layout)
            got = HF.overlay(ref[f'case{i}_classes'].to(DEV), _in_layout(ref[f'case{i}_frames'], layout).to(DEV), style).cpu()
            assert torch.equal(got if layout == 'hwc' else got.permute(0, 2, 3, 1), ref[f'case{i}_expected'])
    assert seen == set(PALETTE_SIZES)


def test_overlay_refuses_other_inputs():
    from hyperseg_amd import functional as HF
    style = _style(12)
    frames, cl = _frames(1, 8, 8, 1).to(DEV), _classes(1, 8, 8, 12, 2).to(DEV)
    with pytest.raises(ValueError):
        HF.overlay(cl, frames.permute(0, 3, 1, 2).contiguous(), style)               # a 'chw' frame
    with pytest.raises(ValueError):
        HF.overlay(cl.long(), frames, style)
    with pytest.raises(ValueError):
        HF.overlay(cl[:, :7], frames, style)
    with pytest.raises(ValueError):
        HF.overlay(cl.cpu(), frames, style)                                          # masks and frames on different devices
    with pytest.raises(ValueError):
        HF.overlay(cl.cpu(), frames.cpu(), style)                                    # the launch runs on the GPU; Overlay.blend blends CPU tensors


# --------------------------------------------------------------------------------------------------------------------- fused

def _logits(b, c, h, w, seed):
    """Smooth-ish logits: neighbouring pixels mostly agree on the class, with exact ties sprinkled in."""
    g = G(seed)
    x = torch.randn(b, c, h, w, generator=g)
    x = x + 2.0 * torch.nn.functional.interpolate(torch.randn(b, c, -(-h // 4), -(-w // 4), generator=g), size=(h, w), mode='nearest')
    ties = torch.rand(b, 1, h, w, generator=g) < 0.05
    return torch.where(ties, x.round(), x).contiguous()


# (Hi, Wi) -> (Ho, Wo): the identity, exact 2x (its own kernel form), 2x of an odd width and general ratios (the general form)
RESIZES = [((24, 32), (24, 32)), ((7, 9), (7, 9)), ((16, 24), (32, 48)), ((64, 128), (128, 256)), ((9, 7), (18, 14)), ((12, 20), (37, 53)),
           ((32, 64), (128, 256)), ((20, 12), (31, 30))]


@pytest.mark.parametrize('layout', ['hwc', 'chw'])
@pytest.mark.parametrize('c', [2, 12, 19, 21])
@pytest.mark.parametrize('src,dst', RESIZES)
def test_upsample_overlay_equals_argmax_then_overlay(src, dst, c, layout):
    from hyperseg_amd import functional as HF
    (hi, wi), (ho, wo) = src, dst
    for b in (1, 2):
        style = _style(c if b == 1 else max(2, c - 3), layout, ignore=(0, -1)[b - 1])          # b = 2: classes beyond the palette
        x = _logits(b, c, hi, wi, hi * wo + c + b).to(DEV)
        frames = _in_layout(_frames(b, ho, wo, ho + wo + c), layout)
        src_frames = frames.to(DEV)
        masks, over = HF.upsample_overlay(x, (ho, wo), src_frames, style)
        want_masks = HF.upsample_argmax(x, (ho, wo))
        assert masks.dtype == torch.uint8 and tuple(masks.shape) == (b, ho, wo)
        assert torch.equal(masks, want_masks)
        assert over.dtype == torch.uint8 and over.shape == frames.shape
        assert torch.equal(over, HF.overlay(want_masks, src_frames, style))
        assert torch.equal(over.cpu(), style.blend(frames, want_masks.cpu()))
        assert torch.equal(src_frames.cpu(), frames)
        # unaligned frames and out=
        big = torch.full((frames.numel() + 8,), 9, dtype=torch.uint8, device=DEV)
        out = big[3:3 + frames.numel()].view(frames.shape)
        m2, o2 = HF.upsample_overlay(x, (ho, wo), _offset_view(frames, 1), style, out=out)
        assert o2 is out and torch.equal(m2, want_masks) and torch.equal(o2, over)
        assert bool((big[:3] == 9).all()) and bool((big[3 + frames.numel():] == 9).all())


def test_upsample_overlay_refuses_other_inputs():
    from hyperseg_amd import functional as HF
    style = _style(12)
    x = _logits(1, 12, 8, 8, 1).to(DEV)
    frames = _frames(1, 16, 16, 2).to(DEV)
    with pytest.raises(ValueError):
        HF.upsample_overlay(x, (16, 12), frames, style)                               # frames of another size
    with pytest.raises(ValueError):
        HF.upsample_overlay(x, (16, 16), frames.cpu(), style)
    with pytest.raises(ValueError, match='overlaps'):
        HF.upsample_overlay(x, (16, 16), frames, style, out=frames)


# -------------------------------------------------------------------------------------------------------------------- models

@functools.lru_cache(maxsize=None)
def _model(tag):
    from hyperseg_amd import configs
    from hyperseg_amd.utils.inference import prepare_for_inference
    m = fill_by_name(configs.build(MODELS[tag][0]).eval(), seed=11)
    prepare_for_inference(m, fold_bn=False, fused_depthwise=True, split_gemm=True)
    return m.to(DEV)


def _norm(layout):
    from hyperseg_amd import InputNorm
    return InputNorm(layout=layout)


def _dress(m, n, layout, hflip=False):
    """Attach a norm and a style (fewer colours than classes: some predicted classes are left alone).  The configs set inference_hflip -- inert
    for a tensor input, but segment() and overlay() take their logits + argmax routes while it is set: off unless the test is about that."""
    m.input_norm = _norm(layout)
    m.overlay_style = _style(max(2, n - 2), layout, ignore=0)
    m.inference_hflip = hflip
    return m.overlay_style


def _undress(m):
    m.input_norm = m.overlay_style = None
    m.inference_hflip = True                      # the configs' value


@pytest.mark.parametrize('layout', ['hwc', 'chw'])
@pytest.mark.parametrize('tag', ['M', 'S', 'Sc', 'Lc', 'L'])
def test_model_overlay_eager_and_graphed(tag, layout):
    from hyperseg_amd.utils.inference import GraphedModel
    m = _model(tag)
    (h, w), n = MODELS[tag][1:]
    style = _dress(m, n, layout)
    try:
        graphed = GraphedModel(m, masks=True, clone_output=True)
        for b in (1, 2):
            frames = _in_layout(_frames(b, h, w, 600 + h + b), layout)
            u8 = frames.to(DEV)
            want_masks = m.segment(u8)
            want = style.blend(frames, want_masks.cpu())
            masks, over = m.overlay(u8)
            assert masks.dtype == torch.uint8 and tuple(masks.shape) == (b, h, w) and torch.equal(masks, want_masks)
            assert over.dtype == torch.uint8 and over.shape == frames.shape and torch.equal(over.cpu(), want)
            assert torch.equal(u8.cpu(), frames)                                      # the input frame is bit-unchanged
            gm, go = graphed.overlay(u8)
            assert torch.equal(gm, want_masks) and torch.equal(go.cpu(), want)
            gm, go = graphed.overlay(frames.pin_memory())                             # staged from pinned host memory
            assert torch.equal(gm, want_masks) and torch.equal(go.cpu(), want)
            assert torch.equal(u8.cpu(), frames)
            # a float x with frames=: the same masks, the same bytes
            ref = m.input_norm.to_float(u8)
            fm, fo = m.overlay(ref, frames=u8)
            assert torch.equal(fm, want_masks) and torch.equal(fo.cpu(), want)
            gm, go = graphed.overlay(ref, frames=u8)
            assert torch.equal(gm, want_masks) and torch.equal(go.cpu(), want)
        assert len(graphed._graphs) == 4                                              # (uint8 | float + frames) x (batch 1 | 2)
    finally:
        _undress(m)


@pytest.mark.parametrize('tag', ['M', 'Lc'])
def test_graph_replay_has_no_stale_buffer(tag):
    """Three different frames through ONE captured graph each get their own masks and overlay; the returned tensors are the graph's own and
    the next replay overwrites them."""
    from hyperseg_amd.utils.inference import GraphedModel
    m = _model(tag)
    (h, w), n = MODELS[tag][1:]
    style = _dress(m, n, 'hwc')
    try:
        graphed = GraphedModel(m, masks=True)
        seen = []
        for i in range(3):
            frames = _frames(1, h, w, 700 + i)
            want_masks = m.segment(frames.to(DEV))
            gm, go = graphed.overlay(frames.to(DEV))
            assert torch.equal(gm, want_masks) and torch.equal(go.cpu(), style.blend(frames, want_masks.cpu()))
            seen.append((gm.data_ptr(), go.data_ptr(), go.cpu()))
        assert len(graphed._graphs) == 1
        assert len({s[0] for s in seen}) == 1 and len({s[1] for s in seen}) == 1      # graph-owned buffers
        assert not torch.equal(seen[0][2], seen[1][2]) and not torch.equal(seen[1][2], seen[2][2])
        # another style is another graph
        m.overlay_style = _style(n, 'hwc', alpha=0.5, ignore=-1, seed=1)
        frames = _frames(1, h, w, 710)
        gm, go = graphed.overlay(frames.to(DEV))
        assert len(graphed._graphs) == 2
        assert torch.equal(go.cpu(), m.overlay_style.blend(frames, m.segment(frames.to(DEV)).cpu()))
    finally:
        _undress(m)


@pytest.mark.parametrize('tag', ['M', 'L'])
def test_attached_style_changes_no_other_route(tag):
    from hyperseg_amd.fps import ConfusionMatrix
    m = _model(tag)
    (h, w), n = MODELS[tag][1:]
    m.input_norm = _norm('hwc')
    m.inference_hflip = False
    try:
        u8 = _frames(2, h, w, 800).to(DEV)
        t = torch.randint(0, n, (2, h, w), generator=G(801)).to(DEV)
        with torch.no_grad():
            cm0 = ConfusionMatrix(n)
            before = (m(u8), m.segment(u8), m.evaluate(u8, t, cm0))
            m.overlay_style = _style(n)
            m.overlay(u8)
            cm1 = ConfusionMatrix(n)
            after = (m(u8), m.segment(u8), m.evaluate(u8, t, cm1))
        assert all(torch.equal(a, b) for a, b in zip(before, after)) and torch.equal(cm0.mat, cm1.mat)
        assert after[0].dtype == torch.float32 and after[1].dtype == torch.uint8
    finally:
        _undress(m)


@pytest.mark.parametrize('tag', ['M', 'Lc'])
def test_fallback_routes_give_the_same_bytes(tag):
    """h-flip inference, a list input and a float x + frames=: masks as segment() computes them on that route, blended to the bytes the fused
    launch gives for those masks."""
    from hyperseg_amd import functional as HF
    m = _model(tag)
    assert m.inference_hflip
    (h, w), n = MODELS[tag][1:]
    style = _dress(m, n, 'hwc', hflip=True)
    try:
        frames = _frames(1, h, w, 900)
        u8 = frames.to(DEV)
        # the configs run h-flip inference: model.overlay takes the fallback for a single tensor as well
        fm, fo = m.overlay(u8)
        assert torch.equal(fm, m.segment(u8)) and torch.equal(fo.cpu(), style.blend(frames, fm.cpu()))
        lm, lo = m.overlay([u8, _frames(1, h // 2, w // 2, 901).to(DEV)])
        assert tuple(lm.shape) == (1, h, w) and torch.equal(lo.cpu(), style.blend(frames, lm.cpu()))
        m.inference_hflip = False
        dm, do = m.overlay(u8)                                                        # the fused route
        xm, xo = m.overlay(m.input_norm.to_float(u8), frames=u8)                      # float x + frames=
        cm, co = m.overlay(m.input_norm.to_float(u8), frames=frames)                  # frames on the host: segment() + blend
        assert torch.equal(dm, m.segment(u8))
        assert torch.equal(xm, dm) and torch.equal(xo, do) and torch.equal(cm, dm) and torch.equal(co, do)
        # the same masks through every blend there is
        for masks in (fm, lm, dm):
            assert torch.equal(HF.overlay(masks, u8, style).cpu(), style.blend(frames, masks.cpu()))
        with pytest.raises(TypeError, match='frames='):
            m.overlay(m.input_norm.to_float(u8))
    finally:
        _undress(m)
