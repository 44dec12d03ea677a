"""uint8 frames normalised on the device (csrc/hs_ingest.hip, the uint8 form of the stem + depthwise launch in csrc/hs_mbconv_lean.hip):
``functional.image_ingest`` against the reference's ToTensor + Normalize computed on the CPU, ``hs_stem_dw_u8_fwd`` against ``hs_stem_dw_fwd`` on the
ingested frame, and the models / GraphedModel fed uint8 against the same models fed the float image made on the CPU from the same bytes.  The
values are table look-ups, so every comparison is ``torch.equal``: no tolerance appears in this file.

The whole file runs with ``torch.backends.cudnn.deterministic = True``.  With PyTorch's default the FLOAT forward does not repeat itself wherever a
stock convolution runs (profiles/float_repeatability.txt, tools/float_repeatability.py: the first module whose output moves between two runs on
bit-equal inputs is the context head's 2 x 2 stride-2 Conv2d -- stock at batch 2, and at every batch size for HyperSeg-L v0_1 -- and a 1 x 1
project Conv2d in the stock encoder; logits move by up to 7.2e-6), and nothing can be compared bit for bit with a reference that moves.  With
the flag every case in that file repeats exactly (0.0), so equality is the bar at batch 1 and 2 for all five models.  The flag only changes
which algorithm the stock convolutions pick; the package's own launches are the same."""
import functools

import pytest
import torch
import torch.nn.functional as F

from conftest import G
from hyperseg_amd.utils.synthetic import fill_by_name

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
# tag -> (config, a frame size of the config's aspect the encoder strides divide, classes)
MODELS = {'M': ('hyperseg-m', (256, 512), 19), 'S': ('hyperseg-s', (256, 512), 19), 'Sc': ('hyperseg-s-camvid', (192, 256), 12),
          'Lc': ('hyperseg-l-camvid', (384, 512), 12), 'L': ('hyperseg-l', (256, 256), 21)}
FUSED_STEM = ('M', 'S', 'Sc')          # no decoder level reads the image: the uint8 frame goes straight into the stem launch
NORMS = {'default': ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225)), 'odd': ((0.4137, 0.38291, 0.456789), (0.2719, 0.19283, 0.31415))}


@pytest.fixture(autouse=True)
def deterministic_stock_convolutions(monkeypatch):
    monkeypatch.setattr(torch.backends.cudnn, 'deterministic', True)


def _norm(layout, which='default'):
    from hyperseg_amd import InputNorm
    return InputNorm(*NORMS[which], layout=layout)


def _frames(b, h, w, seed):
    """uint8 (B, 3, H, W) 'logical' frames; where the frame has room every channel holds all 256 values."""
    x = torch.randint(0, 256, (b, 3, h, w), generator=G(seed), dtype=torch.uint8)
    if h * w >= 256:
        flat = x.view(b, 3, h * w)
        for c in range(3):
            flat[:, c, 17 * c:17 * c + 256] = torch.randperm(256, generator=G(seed + c)).to(torch.uint8)
    return x


def _in_layout(x, layout):
    return x.permute(0, 2, 3, 1).contiguous() if layout == 'hwc' else x.contiguous()


def _reference_float(x, norm):
    """ToTensor + Normalize of the reference (torchvision's to_tensor / normalize arithmetic) on the CPU, float32, from logical frames."""
    return x.to(torch.float32).div(255).sub(norm.mean[None, :, None, None]).div(norm.std[None, :, None, None]).contiguous()


def _offset_view(t, off):
    """``t``'s bytes on the device, starting ``off`` bytes into a larger byte buffer."""
    buf = torch.zeros(t.numel() + 8, dtype=torch.uint8, device=DEV)
    view = buf[off:off + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 4 == (buf.data_ptr() + off) % 4
    return view


# ---------------------------------------------------------------------------------------------------------------- kernel

SIZES = [(1, 1), (1, 5), (3, 6), (2, 7), (5, 4), (37, 53), (64, 129), (512, 1024), (768, 1024)]


@pytest.mark.parametrize('layout', ['hwc', 'chw'])
@pytest.mark.parametrize('h,w', SIZES)
def test_image_ingest(layout, h, w):
    from hyperseg_amd import functional as HF
    for b in (1, 3):
        norm = _norm(layout, 'odd' if b == 3 else 'default')
        x = _frames(b, h, w, 100 * h + w + b)
        ref = _reference_float(x, norm)
        out = HF.image_ingest(_in_layout(x, layout).to(DEV), norm)
        assert out.dtype == torch.float32 and tuple(out.shape) == (b, 3, h, w)
        assert torch.equal(out.cpu(), ref)


@pytest.mark.parametrize('layout', ['hwc', 'chw'])
@pytest.mark.parametrize('h,w', [(37, 53), (9, 8), (6, 13), (64, 128)])
def test_image_ingest_unaligned_base_and_out(layout, h, w):
    from hyperseg_amd import functional as HF
    norm = _norm(layout)
    x = _frames(2, h, w, 7 * h + w)
    ref = _reference_float(x, norm)
    for off in (1, 2, 3):
        src = _offset_view(_in_layout(x, layout), off)
        assert torch.equal(HF.image_ingest(src, norm).cpu(), ref)
    # out=: written in place, also where the destination is only 4-byte aligned (a slice of a larger float buffer)
    out = torch.full((2, 3, h, w), float('nan'), device=DEV)
    got = HF.image_ingest(_in_layout(x, layout).to(DEV), norm, out=out)
    assert got is out and torch.equal(out.cpu(), ref)
    big = torch.full((ref.numel() + 3,), float('nan'), device=DEV)
    sl = big[1:1 + ref.numel()].view(ref.shape)
    HF.image_ingest(_in_layout(x, layout).to(DEV), norm, out=sl)
    assert torch.equal(sl.cpu(), ref) and bool(torch.isnan(big[0])) and bool(torch.isnan(big[-2:]).all())
    with pytest.raises(ValueError):
        HF.image_ingest(_in_layout(x, layout).to(DEV), norm, out=torch.empty(2, 3, h, w + 1, device=DEV))


def test_image_ingest_refuses_other_inputs():
    from hyperseg_amd import functional as HF
    from hyperseg_amd import _hip
    norm = _norm('hwc')
    with pytest.raises(ValueError):
        HF.image_ingest(torch.zeros(1, 3, 8, 8, dtype=torch.uint8, device=DEV), norm)            # a 'chw' frame
    with pytest.raises(ValueError):
        HF.image_ingest(torch.zeros(1, 8, 8, 3, device=DEV), norm)                               # float
    x = torch.zeros(1, 8, 8, 4, dtype=torch.uint8, device=DEV)
    y = torch.empty(1, 4, 8, 8, device=DEV)
    st = _hip.lib.hs_image_ingest_fwd(x.data_ptr(), 0, 1, 4, 8, 8, norm.table(DEV).data_ptr(), y.data_ptr(), _hip.stream_ptr())
    assert st == -3                                                                              # HS_ERR_UNSUPPORTED: channels != 3


# ------------------------------------------------------------------------------------------------------------------ stem

def _stem_operands(cmid, h, w, seed):
    g = G(seed)
    ws = torch.randn(cmid, 3, 3, 3, generator=g) * 0.3
    wd = torch.randn(cmid, 1, 3, 3, generator=g) * 0.3
    s0, b0 = torch.rand(cmid, generator=g) + 0.5, torch.randn(cmid, generator=g) * 0.3
    s1, b1 = torch.rand(cmid, generator=g) + 0.5, torch.randn(cmid, generator=g) * 0.1
    hs, wsz = -(-h // 2), -(-w // 2)
    ph, pw = max((hs - 1) * 2 + 3 - h, 0), max((wsz - 1) * 2 + 3 - w, 0)
    w28 = F.pad(ws.flatten(1), (0, 1)).contiguous()
    return (w28.to(DEV), s0.to(DEV), b0.to(DEV), ph // 2, pw // 2, (hs, wsz), wd.to(DEV), 1, 1, s1.to(DEV), b1.to(DEV))


# HyperSeg-M's and CamVid-S's frames, and an odd-sized frame whose TF-"SAME" stem padding is (1, 1) on both axes: its border tiles' windows
# leave the image at the top, the bottom, the left and the right
@pytest.mark.parametrize('layout', ['hwc', 'chw'])
@pytest.mark.parametrize('cmid,h,w', [(32, 512, 1024), (32, 576, 768), (32, 65, 95), (16, 50, 64)])
def test_stem_dw_u8_equals_float_stem_on_ingested_frame(layout, cmid, h, w):
    from hyperseg_amd import functional as HF
    norm = _norm(layout)
    b = 2
    x = _in_layout(_frames(b, h, w, cmid + h + w), layout).to(DEV)
    ops = _stem_operands(cmid, h, w, h + w)
    want = HF.stem_dw(HF.image_ingest(x, norm), *ops, pool=True)
    assert want is not None
    frame = HF.U8Frame(x, norm)
    got = HF.stem_dw(frame, *ops, pool=True)
    assert frame.image is None, 'the uint8 launch was declined and the frame ingested'
    assert torch.equal(got[0], want[0])
    assert torch.equal(got[1], want[1])
    assert torch.equal(HF.stem_dw(HF.U8Frame(x, norm), *ops, pool=False), want[0])


@pytest.mark.parametrize('layout', ['hwc', 'chw'])
@pytest.mark.parametrize('cmid,h,w', [(32, 64, 72), (24, 64, 64)])
def test_stem_dw_u8_declines_where_the_float_entry_does(layout, cmid, h, w):
    from hyperseg_amd import functional as HF
    from hyperseg_amd import _hip
    norm = _norm(layout)
    x = _in_layout(_frames(2, h, w, cmid + h + w), layout).to(DEV)
    ops = _stem_operands(cmid, h, w, h + w)
    w28, s0, b0, pt, pl, (hs, wsz), wd, dpt, dpl, s1, b1 = ops
    assert HF.stem_dw(HF.image_ingest(x, norm), *ops, pool=True) is None
    y = torch.empty(2, cmid, hs, wsz, device=DEV)
    st = _hip.lib.hs_stem_dw_u8_fwd(x.data_ptr(), 0 if layout == 'hwc' else 1, norm.table(DEV).data_ptr(), 2, h, w, w28.data_ptr(), cmid,
                                    s0.data_ptr(), b0.data_ptr(), pt, pl, hs, wsz, wd.data_ptr(), 3, dpt, dpl, s1.data_ptr(), b1.data_ptr(),
                                    y.data_ptr(), None, _hip.stream_ptr())
    assert st == -3                                               # HS_ERR_UNSUPPORTED, nothing launched
    frame = HF.U8Frame(x, norm)
    assert HF.stem_dw(frame, *ops, pool=True) is None             # the wrapper: ingest, then the float form's answer
    assert frame.image is not None


# ----------------------------------------------------------------------------------------------------------------- models

@functools.lru_cache(maxsize=None)
def _model(tag, prepared=True):
    from hyperseg_amd import configs
    m = fill_by_name(configs.build(MODELS[tag][0]).eval(), seed=11)
    if prepared:
        from hyperseg_amd.utils.inference import prepare_for_inference
        prepare_for_inference(m, fold_bn=False, fused_depthwise=True, split_gemm=True)
    return m.to(DEV)


def _targets(b, h, w, n, seed):
    g = G(seed)
    t = torch.randint(0, n, (b, h, w), generator=g)
    t[torch.rand(t.shape, generator=g) < 0.10] = 255
    return t


def _no_ingest(monkeypatch):
    from hyperseg_amd import functional as HF

    class FloatImageMade(AssertionError):
        pass

    def refuse(*a, **k):
        raise FloatImageMade('functional.image_ingest was called')
    monkeypatch.setattr(HF, 'image_ingest', refuse)
    return FloatImageMade


def _encoder_features(m, x):
    """The encoder's feature list for ``x`` the way process_single_tensor feeds it: a uint8 frame goes in as it is where the model takes the
    fused route, through one image_ingest launch elsewhere."""
    from hyperseg_amd import functional as HF
    if x.dtype == torch.uint8:
        frame = HF.U8Frame(x, m.input_norm)
        x = frame if m._takes_u8_stem(frame) else m.input_norm.to_float(x)
    return m.backbone(x)


@pytest.mark.parametrize('layout', ['hwc', 'chw'])
@pytest.mark.parametrize('tag', ['M', 'S', 'Sc', 'Lc', 'L'])
def test_prepared_model_uint8_equals_float(tag, layout):
    """forward, segment and evaluate (masks, matrix, per-image matrices) fed uint8 == the same calls fed the float image the CPU made from the
    same bytes, at batch 1 and 2, ``torch.equal``; so are the encoder's feature maps on the way."""
    from hyperseg_amd.fps import ConfusionMatrix
    m = _model(tag)
    (h, w), n = MODELS[tag][1:]
    m.input_norm = norm = _norm(layout)
    for b in (1, 2):
        x = _frames(b, h, w, 900 + h + b)
        u8, ref = _in_layout(x, layout).to(DEV), _reference_float(x, norm).to(DEV)
        with torch.no_grad():
            fu, ff = _encoder_features(m, u8), _encoder_features(m, ref)
            want, again, got = m(ref), m(ref), m(u8)
        assert torch.equal(want, again), 'the float forward does not repeat itself: nothing can be compared with it bit for bit'
        assert len(fu) == len(ff) and all(torch.equal(p, q) for p, q in zip(fu, ff))
        assert tuple(got.shape) == (b, n, h, w)
        assert torch.equal(got, want)
        assert torch.equal(m.segment(u8), m.segment(ref))
        t = _targets(b, h, w, n, 901).to(DEV)
        cu, cf = ConfusionMatrix(n), ConfusionMatrix(n)
        mu, mf = m.evaluate(u8, t, cu), m.evaluate(ref, t, cf)
        assert mu.dtype == torch.uint8 and tuple(mu.shape) == (b, h, w) and int(cu.mat.sum()) == int((t < n).sum())
        assert torch.equal(mu, mf) and torch.equal(cu.mat, cf.mat)
        cu, cf = ConfusionMatrix(n), ConfusionMatrix(n)
        pu, pf = m.evaluate(u8, t, cu, per_image=True), m.evaluate(ref, t, cf, per_image=True)
        assert torch.equal(pu, pf) and torch.equal(cu.per_image[-1], cf.per_image[-1]) and torch.equal(cu.mat, cf.mat)


@pytest.mark.parametrize('b', [1, 2])
@pytest.mark.parametrize('tag', ['M', 'S', 'Sc', 'Lc', 'L'])
def test_graphed_model_uint8_from_pinned_host(tag, b):
    """GraphedModel.forward / evaluate with pinned host uint8 frames, replayed over several distinct frames, against the eager float calls."""
    from hyperseg_amd.utils.inference import GraphedModel
    from hyperseg_amd.fps import ConfusionMatrix
    m = _model(tag)
    (h, w), n = MODELS[tag][1:]
    m.input_norm = norm = _norm('hwc')
    logits = GraphedModel(m, clone_output=True)
    scored = GraphedModel(m, masks=True, num_classes=n, clone_output=True)
    total = torch.zeros(n, n, dtype=torch.int64, device=DEV)
    for i in range(4):
        x = _frames(b, h, w, 950 + i)
        host = _in_layout(x, 'hwc').pin_memory()
        ref = _reference_float(x, norm).to(DEV)
        t = _targets(b, h, w, n, 960 + i)
        cm = ConfusionMatrix(n)
        with torch.no_grad():                      # GraphedModel replays only where nothing can ask for a gradient
            want, got = m(ref), logits(host)
            masks, got_masks = m.evaluate(ref, t.to(DEV), cm), scored.evaluate(host, t.pin_memory())
        assert tuple(got.shape) == (b, n, h, w) and got_masks.dtype == torch.uint8
        assert torch.equal(got, want)
        assert torch.equal(got_masks, masks)
        total += cm.mat
        assert torch.equal(scored.confusion, total)
    assert len(logits._graphs) == 1 and len(scored._graphs) == 1
    (static,) = next(iter(logits._graphs.values()))[1]
    assert static.dtype == torch.uint8 and tuple(static.shape) == (b, h, w, 3)      # the staging copy moves bytes


@pytest.mark.parametrize('tag', FUSED_STEM)
def test_fused_route_makes_no_float_image(tag, monkeypatch):
    """M / S / CamVid-S prepared: with functional.image_ingest refusing to run, uint8 frames are still served -- the stem launch read them."""
    m = _model(tag)
    (h, w), n = MODELS[tag][1:]
    x = _frames(1, h, w, 970)
    for layout in ('hwc', 'chw'):
        m.input_norm = norm = _norm(layout)
        ref = _reference_float(x, norm).to(DEV)
        with torch.no_grad():
            want, want_masks = m(ref), m.segment(ref)
        _no_ingest(monkeypatch)
        with torch.no_grad():
            assert torch.equal(m(_in_layout(x, layout).to(DEV)), want)
            assert torch.equal(m.segment(_in_layout(x, layout).to(DEV)), want_masks)
        monkeypatch.undo()


@pytest.mark.parametrize('tag,prepared', [('Lc', True), ('L', True), ('M', False)])
def test_general_route_ingests(tag, prepared, monkeypatch):
    """A decoder whose last level reads the image (CamVid-L, L v0_1) and a stock encoder take one image_ingest launch."""
    m = _model(tag, prepared)
    h, w = MODELS[tag][1]
    m.input_norm = _norm('hwc')
    raised = _no_ingest(monkeypatch)
    with pytest.raises(raised), torch.no_grad():
        m(_in_layout(_frames(1, h, w, 971), 'hwc').to(DEV))


def test_training_mode_ingests(monkeypatch):
    m = _model('M')
    m.input_norm = _norm('hwc')
    raised = _no_ingest(monkeypatch)
    m.train()
    try:
        with pytest.raises(raised), torch.no_grad():
            m(_in_layout(_frames(2, 128, 256, 972), 'hwc').to(DEV))
    finally:
        m.eval()


@pytest.mark.parametrize('tag', ['M', 'Lc'])
def test_pyramid_and_hflip_uint8_equals_float(tag):
    """A list input (the configs set inference_hflip=True: every entry also runs flipped) with uint8 entries == its float counterpart."""
    m = _model(tag)
    assert m.inference_hflip
    (h, w), n = MODELS[tag][1:]
    m.input_norm = norm = _norm('hwc')
    xs = [_frames(1, h, w, 980), _frames(1, h // 2, w // 2, 981)]
    with torch.no_grad():
        want = m([_reference_float(x, norm).to(DEV) for x in xs])
        got = m([_in_layout(x, 'hwc').to(DEV) for x in xs])
        mixed = m([_in_layout(xs[0], 'hwc').to(DEV), _reference_float(xs[1], norm).to(DEV)])
    assert tuple(got.shape) == (1, n, h, w)
    assert torch.equal(got, want) and torch.equal(mixed, want)
    assert torch.equal(m.segment([_in_layout(x, 'hwc').to(DEV) for x in xs]), want.argmax(1).to(torch.uint8))


def test_stock_encoder_uint8_equals_float():
    """Unprepared HyperSeg-M, batch 1 and 2: the route is one image_ingest launch + the float forward, unchanged -- the tensor the encoder
    receives for a uint8 frame equals the float image the CPU made from the same bytes, and so do the logits and the masks (the stock float
    forward repeats itself under this file's deterministic convolutions: asserted first)."""
    m = _model('M', False)
    h, w = MODELS['M'][1]
    m.input_norm = norm = _norm('hwc')
    seen = []
    hook = m.backbone.register_forward_pre_hook(lambda mod, args: seen.append(args[0]))
    try:
        for b in (1, 2):
            x = _frames(b, h, w, 990 + b)
            u8, ref = _in_layout(x, 'hwc').to(DEV), _reference_float(x, norm).to(DEV)
            with torch.no_grad():
                a, a2 = m(ref), m(ref)
                del seen[:]
                got = m(u8)
            assert torch.equal(a, a2), 'the stock float forward does not repeat itself: nothing can be compared with it bit for bit'
            assert len(seen) == 1 and isinstance(seen[0], torch.Tensor) and torch.equal(seen[0], ref)
            assert torch.equal(got, a)
            assert torch.equal(m.segment(u8), m.segment(ref))
    finally:
        hook.remove()


def test_layouts_get_graphs_of_their_own():
    """One GraphedModel, the same image as an 'hwc' and as a 'chw' frame: equal outputs, two captured graphs."""
    from hyperseg_amd.utils.inference import GraphedModel
    m = _model('M')
    h, w = MODELS['M'][1]
    served = GraphedModel(m, clone_output=True)
    x = _frames(1, h, w, 995)
    outs = {}
    for layout in ('hwc', 'chw', 'hwc'):
        m.input_norm = _norm(layout) if layout not in outs else outs[layout][1]
        with torch.no_grad():
            outs[layout] = (served(_in_layout(x, layout).to(DEV)), m.input_norm)
    assert torch.equal(outs['hwc'][0], outs['chw'][0])
    assert len(served._graphs) == 2
    with torch.no_grad():
        assert torch.equal(outs['hwc'][0], m(_reference_float(x, outs['hwc'][1]).to(DEV)))


def test_fps_harness_uint8():
    from hyperseg_amd import fps
    res = fps.main(['--config', 'hyperseg-m', '--iterations', '3', '--distinct', '2', '--prepare', '--graph', '--uint8'])
    assert res['input_dtype'] == 'uint8' and res['input_bytes_per_frame'] == 512 * 1024 * 3 and res['frames'] == 3
    res = fps.main(['--config', 'hyperseg-m', '--iterations', '2', '--distinct', '1', '--prepare', '--graph'])
    assert res['input_dtype'] == 'float32' and res['input_bytes_per_frame'] == 512 * 1024 * 3 * 4
