"""Confidence maps on the device (csrc/hs_confidence.hip): hs_confidence_fwd, hs_upsample_confidence_fwd and hs_upsample2_confidence_fwd
through their wrappers, the model's ``confidence()`` and ``GraphedModel.confidence``.

Per case: masks bit-identical to the arg-max entries', the fp32 confidence bit-identical between the fused launch and the composed route
(``upsample_bilinear`` + ``confidence``), that confidence within the DERIVED bound of tests/util_confidence_ref.py of float64 soft-max over
the same device-made logits (only the soft-max can err, not the resize), the uint8 form and the thresholded masks equal to their formulas
on the launch's own fp32 output, and guard bytes around ``mask`` and ``conf`` untouched.  With HS_CONFIDENCE_REPORT=<file> the run writes
one line per case with the worst err / bound (profiles/confidence_bound.txt is such a run; nothing here is tuned to it)."""
import os

import pytest
import torch

import util_confidence_ref as R
from conftest import G, load_golden, sub

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
B = 2
CLASSES = (2, 19, 256)
# form -> (Hi, Wi), mid size or None, (Ho, Wo)
FORMS = {
    'exact2x': ((6, 8), None, (12, 16)),
    'general_wo_not_4k': ((5, 7), None, (13, 18)),
    'identity': ((6, 8), None, (6, 8)),
    'two_stage_2x2x': ((6, 8), (12, 16), (24, 32)),
    'two_stage_general': ((6, 8), (12, 16), (16, 21)),
    'two_stage_down': ((6, 8), (12, 16), (9, 10)),
}
_REPORT_STARTED = set()


def _report(form, c, ratio, index):
    path = os.environ.get('HS_CONFIDENCE_REPORT')
    if path:
        mode = 'a' if path in _REPORT_STARTED else 'w'
        _REPORT_STARTED.add(path)
        with open(path, mode) as f:
            f.write(f'{form:20s} C={c:<4d} worst err/bound {ratio:.4f} at flat index {index}\n')


@pytest.fixture(scope='module')
def HF():
    from hyperseg_amd import functional
    return functional


def _x(c, hw, seed):
    return (torch.randn(B, c, *hw, generator=G(seed)) * 3.0).to(DEV)


def _fused(HF, x, mid, size, **kw):
    return HF.upsample_confidence(x, size, **kw) if mid is None else HF.upsample2_confidence(x, mid, size, **kw)


def _logits(HF, x, mid, size):
    """The device-made logits of the composed route: one ``upsample_bilinear``, or two."""
    return HF.upsample_bilinear(x, size) if mid is None else HF.upsample_bilinear(HF.upsample_bilinear(x, mid), size)


GUARD = 0xA5


def _raw_guarded(HF, x, mid, size, dtype, threshold, fill):
    """The library entry itself, writing into the middle of guarded buffers at addresses that are NOT 16- / 4-byte aligned (the
    single-element stores); returns (mask, conf) views and the two whole buffers."""
    from hyperseg_amd import _hip
    from hyperseg_amd.utils.confidence import CONF_DTYPES
    b, c, hi, wi = x.shape
    n = b * size[0] * size[1]
    pad_m, pad_c = 5, 3                                      # mask: 5 bytes in; conf: 3 elements in (12 bytes for fp32)
    mbuf = torch.full((n + 2 * pad_m + 64,), GUARD, dtype=torch.uint8, device=DEV)
    cbuf = torch.full((n + 2 * pad_c + 64,), GUARD, dtype=torch.uint8, device=DEV) if dtype == torch.uint8 else \
        torch.full((n + 2 * pad_c + 64,), -7.5, dtype=torch.float32, device=DEV)
    mask, conf = mbuf[pad_m:pad_m + n], cbuf[pad_c:pad_c + n]
    tail = (CONF_DTYPES[dtype], 0.0 if threshold is None else threshold, fill, mask.data_ptr(), conf.data_ptr(), _hip.stream_ptr())
    if mid is None:
        _hip.run.hs_upsample_confidence_fwd(x.data_ptr(), b, c, hi, wi, *size, *tail)
    else:
        _hip.run.hs_upsample2_confidence_fwd(x.data_ptr(), b, c, hi, wi, *mid, *size, *tail)
    torch.cuda.synchronize()
    for buf, pad, sentinel in ((mbuf, pad_m, GUARD), (cbuf, pad_c, GUARD if dtype == torch.uint8 else -7.5)):
        assert bool((buf[:pad] == sentinel).all()) and bool((buf[pad + n:] == sentinel).all()), 'guard region written'
    return mask.view(b, *size), conf.view(b, *size)


@pytest.mark.parametrize('c', CLASSES)
@pytest.mark.parametrize('form', list(FORMS))
def test_confidence_forms(HF, form, c):
    src, mid, size = FORMS[form]
    x = _x(c, src, 1000 + 7 * c + len(form))
    # 1. masks: the arg-max entries', bit for bit
    want_masks = HF.upsample_argmax(x, size) if mid is None else HF.upsample2_argmax(x, mid, size)
    masks, conf = _fused(HF, x, mid, size, dtype=torch.float32)
    assert masks.dtype == torch.uint8 and conf.dtype == torch.float32 and tuple(masks.shape) == tuple(conf.shape) == (B, *size)
    assert torch.equal(masks, want_masks)
    # 2. the fused and the composed kernels agree exactly
    logits = _logits(HF, x, mid, size)
    masks_c, conf_c = HF.confidence(logits, torch.float32)
    assert torch.equal(masks_c, want_masks)
    assert torch.equal(conf, conf_c)
    # 3. within the derived bound of float64 soft-max over those same logits
    ratio, index, _, _ = R.worst_ratio(conf, logits.cpu())
    print(f'{form} C={c}: worst err/bound {ratio:.4f} at {index}')
    _report(form, c, ratio, index)
    assert ratio <= 1.0, f'{form} C={c}: |conf - ref64| is {ratio:.3f} x the derived bound at flat index {index}'
    # 4. the uint8 output is the quantisation of the launch's own fp32 output
    masks_u, conf_u = _fused(HF, x, mid, size, dtype=torch.uint8)
    assert conf_u.dtype == torch.uint8 and torch.equal(masks_u, want_masks)
    assert torch.equal(conf_u, (conf * 255.0 + 0.5).to(torch.uint8))
    assert torch.equal(HF.confidence(logits, torch.uint8)[1], conf_u)
    # 5. thresholded masks: where(own fp32 conf < t, fill, masks), t exactly one pixel's confidence (strict <: that pixel stays)
    t = float(conf.flatten().sort().values[conf.numel() // 2])
    for fill, dtype in ((255, torch.float32), (3, torch.uint8)):
        masks_t, conf_t = _fused(HF, x, mid, size, dtype=dtype, threshold=t, fill=fill)
        assert torch.equal(masks_t, torch.where(conf < t, torch.full_like(want_masks, fill), want_masks))
        assert torch.equal(conf_t, conf if dtype == torch.float32 else conf_u)
        assert torch.equal(HF.confidence(logits, dtype, threshold=t, fill=fill)[0], masks_t)
    assert 0 < int((conf < t).sum()) < conf.numel() and bool((masks_t[conf == t] == want_masks[conf == t]).all())
    # 6. guard regions, through the library entry at unaligned addresses: same bytes, nothing outside them
    for dtype, want_conf in ((torch.float32, conf), (torch.uint8, conf_u)):
        m_raw, c_raw = _raw_guarded(HF, x, mid, size, dtype, t, 255)
        assert torch.equal(m_raw, torch.where(conf < t, torch.full_like(want_masks, 255), want_masks))
        assert torch.equal(c_raw, want_conf)
    out = torch.empty(B, *size, dtype=torch.float32, device=DEV)
    assert _fused(HF, x, mid, size, dtype=torch.float32, out=out)[1] is out and torch.equal(out, conf)


def test_two_stage_wrapper_falls_to_the_one_stage(HF):
    x = _x(19, (6, 8), 77)
    a = HF.upsample2_confidence(x, (6, 8), (13, 18), dtype=torch.float32)           # first stage the identity
    b = HF.upsample2_confidence(x, (13, 18), (13, 18), dtype=torch.float32)         # second stage the identity
    c = HF.upsample_confidence(x, (13, 18), dtype=torch.float32)
    assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1]) and torch.equal(b[0], c[0]) and torch.equal(b[1], c[1])


def test_one_class_is_sure(HF):
    x = _x(1, (6, 8), 5)
    for mid, size in ((None, (12, 16)), (None, (13, 18)), ((12, 16), (24, 32)), ((12, 16), (9, 10))):
        masks, conf = _fused(HF, x, mid, size, dtype=torch.float32, threshold=0.5)
        assert bool((conf == 1.0).all()) and int(masks.max()) == 0
        assert bool((_fused(HF, x, mid, size)[1] == 255).all())
    assert bool((HF.confidence(x, torch.float32)[1] == 1.0).all())


def test_confidence_from_logits_wide_and_odd_rows(HF):
    """hs_confidence_fwd alone: rows of 4 k pixels take the 16-byte loads, others single elements; several workgroups."""
    from hyperseg_amd.utils.confidence import confidence_cpu
    for c, hw, seed in ((19, (37, 53), 1), (21, (33, 64), 2), (2, (1, 1), 3), (256, (3, 5), 4)):
        logits = _x(c, hw, seed)
        masks, conf = HF.confidence(logits, torch.float32)
        assert torch.equal(masks.long(), logits.argmax(1))
        ratio, index, _, _ = R.worst_ratio(conf, logits.cpu())
        assert ratio <= 1.0, (c, hw, ratio, index)
        cpu_masks, _ = confidence_cpu(logits.cpu(), torch.float32)
        assert torch.equal(cpu_masks, masks.cpu())
        view = logits[:, :, :, 1:].contiguous() if hw[1] > 1 else logits                     # (another width, same bytes otherwise)
        assert torch.equal(HF.confidence(view, torch.float32)[1], conf[:, :, 1:] if hw[1] > 1 else conf)


def test_non_finite_score_changes_no_other_pixel(HF):
    """A NaN / inf in one logit: every other pixel keeps its bits; the fused masks stay what the arg-max entries write, in both forms."""
    logits = _x(19, (8, 12), 9)
    _, clean = HF.confidence(logits, torch.float32)
    for bad in (float('nan'), float('inf'), float('-inf')):
        dirty = logits.clone()
        dirty[1, 4, 3, 5] = bad
        masks, conf = HF.confidence(dirty, torch.float32)
        keep = torch.ones_like(clean, dtype=torch.bool)
        keep[1, 3, 5] = False
        assert torch.equal(conf[keep], clean[keep]) and torch.equal(masks[keep].long(), logits.argmax(1)[keep])
        x = _x(19, (6, 8), 10)
        x[0, 0, 2, 3] = bad
        x[1, 7, 0, 0] = bad
        for mid, size in ((None, (12, 16)), (None, (13, 18)), ((12, 16), (24, 32)), ((12, 16), (16, 21))):
            want = HF.upsample_argmax(x, size) if mid is None else HF.upsample2_argmax(x, mid, size)
            assert torch.equal(_fused(HF, x, mid, size)[0], want), (bad, mid, size)


def test_argument_errors_raise_before_a_launch(HF):
    x = _x(19, (6, 8), 11)
    for call in (lambda: HF.confidence(x.cpu()),
                 lambda: HF.upsample_confidence(x.cpu(), (12, 16)),
                 lambda: HF.upsample2_confidence(x.cpu(), (12, 16), (24, 32)),
                 lambda: HF.confidence(x[0]),
                 lambda: HF.confidence(x.half()),
                 lambda: HF.confidence(x, dtype=torch.float16),
                 lambda: HF.confidence(x, threshold='high'),
                 lambda: HF.confidence(x, fill=256),
                 lambda: HF.confidence(x, out=torch.empty(B, 6, 8, device=DEV)),                          # float32 where uint8 is asked for
                 lambda: HF.confidence(x, torch.float32, out=torch.empty(B, 6, 9, device=DEV)),
                 lambda: HF.upsample_confidence(x, (0, 16)),
                 lambda: HF.upsample2_confidence(x, (12, 16), (24, -1)),
                 lambda: HF.upsample2_confidence(x, (0, 16), (24, 32)),
                 lambda: HF.upsample_confidence(torch.zeros(1, 257, 2, 2, device=DEV), (4, 4)),
                 lambda: HF.upsample_confidence(x.permute(0, 1, 3, 2), (12, 16))):
        with pytest.raises(ValueError):
            call()


# ------------------------------------------------------------------------------ the model

class _Features(torch.nn.Module):
    """A stand-in backbone for the tiny decoder of tests/test_hip_parity.py: level i = the image average-pooled by 2^i, its channels
    elementwise functions of the pooled image (no convolution: nothing here depends on a stock kernel's choice of algorithm)."""

    def __init__(self, feat):
        super().__init__()
        self.feat = list(feat)

    def forward(self, x):
        out = []
        for i, ch in enumerate(self.feat[1:], start=1):
            p = torch.nn.functional.avg_pool2d(x, 2 ** i)
            out.append(torch.stack([torch.sin(p[:, j % 3] * (j + 1) + i) for j in range(ch)], 1).contiguous())
        return out + [out[-1]]


class _Signal(torch.nn.Module):
    def __init__(self, channels):
        super().__init__()
        self.channels = channels

    def forward(self, f):
        return torch.stack([0.3 * torch.cos(f[:, k % f.shape[1]] * (k % 5 + 1) + k) for k in range(self.channels)], 1).contiguous()


def _tiny_model():
    from hyperseg_amd.models._common import HyperGenBase
    from test_hip_parity import make_decoder
    from test_oracle_golden import TINY
    c = TINY['t_v1_0']
    g = load_golden('decoder_t_v1_0')

    class Tiny(HyperGenBase):
        def __init__(self):
            super().__init__()
            self.backbone = _Features(c['feat'])
            self.weight_mapper = _Signal(c['signal'])
            self.decoder = make_decoder(c)
    m = Tiny()
    missing, unexpected = m.decoder.load_state_dict(sub(g, 'p.'), strict=False)
    assert not unexpected
    return m.eval().to(DEV), c


def _frame(c, seed, batch=2):
    return torch.randn(batch, 3, *c['size'], generator=G(seed)).to(DEV)


@torch.no_grad()          # as model.confidence() itself runs: with gradients enabled model(x) would take the decoder's training kernels
def test_model_confidence_eager_graphed_and_composed(HF):
    """The tiny v1_0 decoder of the parity table at its fixture's size (64 x 96: a 2 x 3 weight grid, the final upsample exact 2x)."""
    from hyperseg_amd import Confidence
    from hyperseg_amd.utils.inference import GraphedModel
    model, c = _tiny_model()
    x, x2 = _frame(c, 21), _frame(c, 22)
    for style, size in ((Confidence(torch.float32), None), (Confidence(torch.uint8, threshold=0.6, fill=255), None),
                        (Confidence(torch.float32, threshold=0.5, fill=9), (80, 100)), (Confidence(), (32, 48))):
        model.confidence_style = style
        logits = model._logits_at(x, size or c['size'])
        assert tuple(logits.shape[2:]) == (size or c['size'])
        want = HF.confidence(logits.contiguous(), style.dtype, style.threshold, style.fill)
        got = model.confidence(x, size=size)
        assert got[0].dtype == torch.uint8 and got[1].dtype == style.dtype
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (style, size)
        if style.threshold is None:
            assert torch.equal(got[0], model.segment(x, size=size))
        # h-flip inference set: the composed route over model(x)
        model.inference_hflip = True
        try:
            flip = model.confidence(x, size=size)
        finally:
            model.inference_hflip = False
        assert torch.equal(flip[0], want[0]) and torch.equal(flip[1], want[1])
    # the CPU statement gives the same masks from the same logits
    model.confidence_style = Confidence(torch.float32)
    logits = model(x)
    masks, conf = model.confidence(x)
    cpu_masks, cpu_conf = model.confidence_style.of_logits(logits.cpu())
    assert torch.equal(cpu_masks, masks.cpu())
    ratio, index, _, _ = R.worst_ratio(conf, logits.cpu())
    _report('model t_v1_0', c['num_classes'], ratio, index)
    assert ratio <= 1.0
    # one replay per frame, static outputs, a second frame
    for style, size in ((Confidence(torch.uint8, threshold=0.6), None), (Confidence(torch.float32), (80, 100))):
        model.confidence_style = style
        gm = GraphedModel(model, masks=True)
        first = gm.confidence(x, size=size)
        eager = model.confidence(x, size=size)
        assert torch.equal(first[0], eager[0]) and torch.equal(first[1], eager[1])
        keep = (first[0].clone(), first[1].clone())
        second = gm.confidence(x2.cpu().pin_memory(), size=size)                    # staged from host memory
        eager2 = model.confidence(x2, size=size)
        assert second[0] is first[0] and second[1] is first[1]                       # graph-owned, overwritten
        assert torch.equal(second[0], eager2[0]) and torch.equal(second[1], eager2[1])
        assert not torch.equal(keep[1], second[1])
        assert len(gm._graphs) == 1
        again = gm.confidence(x, size=size)
        assert torch.equal(again[0], keep[0]) and torch.equal(again[1], keep[1]) and len(gm._graphs) == 1
        cl = GraphedModel(model, masks=True, clone_output=True)
        a = cl.confidence(x, size=size)
        b = cl.confidence(x2, size=size)
        assert a[1] is not b[1] and torch.equal(a[1], keep[1]) and torch.equal(b[1], eager2[1])
    # no confidence asked for: segment and its graph are what they were
    model.confidence_style = Confidence(torch.float32, threshold=0.9, fill=0)
    assert torch.equal(model.segment(x), model(x).argmax(1).to(torch.uint8))
    assert torch.equal(GraphedModel(model, masks=True)(x), model.segment(x))
    model.confidence_style = None
    assert model.confidence(x)[1].dtype == torch.uint8                              # the default style
