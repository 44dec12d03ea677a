"""Confidence maps, the CPU statement (hyperseg_amd/utils/confidence.py): held to float64 ``softmax(...).max(1)`` within the derived
per-element bound of tests/util_confidence_ref.py, which also rejects two restatements with a defect on the same inputs; the uint8 form,
the threshold rule and the argument errors of ``Confidence`` and ``Epilogue(confidence=...)``.  No GPU: nothing here launches."""
import pytest
import torch

import util_confidence_ref as R
from hyperseg_amd.utils.confidence import Confidence, confidence_cpu, quantise, softmax_max_f32

CLASSES = (1, 2, 19, 21, 256)
INPUTS = {
    'order_one': lambda C: R.scores_order_one(C, 100 + C),
    'spread40': lambda C: R.scores_spread(C, 200 + C),
    'ties': lambda C: R.scores_ties(C, 300 + C),
    'max_first': lambda C: R.scores_max_at(C, 400 + C, 0),
    'max_last': lambda C: R.scores_max_at(C, 500 + C, -1),
}


@pytest.mark.parametrize('C', CLASSES)
@pytest.mark.parametrize('kind', sorted(INPUTS))
def test_statement_within_derived_bound(kind, C):
    x = INPUTS[kind](C)
    masks, conf = confidence_cpu(x, torch.float32)
    assert masks.dtype == torch.uint8 and conf.dtype == torch.float32 and masks.shape == conf.shape == (x.shape[0],) + x.shape[2:]
    assert torch.equal(masks.long(), x.argmax(1))
    ratio, i = R.assert_within(conf, x, f'{kind} C={C}')
    print(f'{kind} C={C}: worst err/bound {ratio:.4f} at {i}')
    if C == 1:
        assert bool((conf == 1.0).all())


def test_ties_go_to_the_lowest_class():
    x = torch.tensor([1.0, 3.0, 3.0, 2.0, 3.0]).view(1, 5, 1, 1)
    masks, conf = confidence_cpu(x, torch.float32)
    assert int(masks) == 1 and int(x.argmax(1)) == 1          # (torch.argmax documents the first maximum as well)
    R.assert_within(conf, x)


def test_spread_inputs_reach_underflow():
    x = R.scores_spread(19, 219)
    gap = x.max(1).values.unsqueeze(1) - x
    assert float(gap.max()) > 104.0 and bool(((gap > 87.4) & (gap < 103.0)).any())      # expf returns 0 / a denormal there


@pytest.mark.parametrize('C', (2, 19, 21, 256))
@pytest.mark.parametrize('kind', ('order_one', 'spread40'))
@pytest.mark.parametrize('defect', sorted(R.DEFECTS))
def test_defects_fail_the_same_check(defect, kind, C):
    """The same inputs, the same check.  (C = 1 and the maximum in the first class leave nothing for `no_rescale` to get wrong: the
    maximum never moves there.)"""
    x = INPUTS[kind](C)
    assert bool((x.argmax(1) != 0).any())                   # the maximum moves for some pixel
    got = R.DEFECTS[defect](x)
    ref, bound = R.confidence_ref_bound(x)
    bad = ~((got.double() - ref).abs() <= bound)            # (a non-finite result fails as well)
    assert bool(bad.any()), f'{defect} passes the bound on {kind} C={C}'
    with pytest.raises(AssertionError):
        R.assert_within(got, x)
    R.assert_within(softmax_max_f32(x)[1], x)               # ... which the statement passes


@pytest.mark.parametrize('C', CLASSES)
def test_uint8_is_the_quantised_fp32(C):
    x = INPUTS['order_one'](C)
    x[0, :, 0, 0] = 0.0
    x[0, 0, 0, 0] = 60.0                                     # one pixel that is sure: conf = 1 -> 255
    masks_f, conf_f = confidence_cpu(x, torch.float32)
    masks_u, conf_u = confidence_cpu(x, torch.uint8)
    assert conf_u.dtype == torch.uint8 and torch.equal(masks_f, masks_u)
    assert torch.equal(conf_u, (conf_f * 255.0 + 0.5).to(torch.uint8)) and torch.equal(conf_u, quantise(conf_f))
    assert int(conf_u[0, 0, 0]) == 255 and int(conf_u.max()) == 255
    if C > 1:
        assert int(conf_u.min()) < 255


@pytest.mark.parametrize('fill', (255, 0, 7))
def test_threshold_fills_strictly_below(fill):
    x = INPUTS['order_one'](19)
    idx = x.argmax(1)
    _, conf = confidence_cpu(x, torch.float32)
    t = float(conf.flatten()[11])                            # exactly one pixel's fp32 confidence: strict < keeps that pixel
    assert float(conf.min()) < t < float(conf.max())
    for dtype in (torch.float32, torch.uint8):
        masks, c2 = confidence_cpu(x, dtype, threshold=t, fill=fill)
        want = torch.where(conf < t, torch.full_like(idx, fill), idx).to(torch.uint8)
        assert torch.equal(masks, want)
        assert int(masks.flatten()[11]) == int(idx.flatten()[11])
        assert torch.equal(c2, conf if dtype == torch.float32 else quantise(conf))       # the confidence is not changed by it
    assert int((conf < t).sum()) > 0
    none, _ = confidence_cpu(x, torch.float32, threshold=None, fill=fill)
    assert torch.equal(none.long(), idx)
    # a threshold that is no fp32 number is taken in fp32, as the kernels' float argument is
    t64 = 0.3
    masks, _ = confidence_cpu(x, torch.float32, threshold=t64)
    assert torch.equal(masks, torch.where(conf < torch.tensor(t64, dtype=torch.float32), torch.full_like(idx, 255), idx).to(torch.uint8))


def test_confidence_argument_errors():
    for bad in (dict(dtype=torch.float16), dict(dtype=torch.int64), dict(threshold='0.5'), dict(threshold=float('nan')), dict(threshold=True),
                dict(fill=256), dict(fill=-1), dict(fill=1.5)):
        with pytest.raises(ValueError):
            Confidence(**bad)
    c = Confidence()
    assert (c.dtype, c.threshold, c.fill) == (torch.uint8, None, 255)
    assert Confidence(torch.float32, 0.5, 0) == Confidence(torch.float32, 0.5, 0) and Confidence() != Confidence(threshold=0.5)
    assert len({Confidence(), Confidence(), Confidence(fill=3)}) == 2
    with pytest.raises(ValueError):
        confidence_cpu(torch.zeros(2, 3, 4), torch.float32)
    with pytest.raises(ValueError):
        confidence_cpu(torch.zeros(1, 257, 2, 2), torch.float32)
    masks, conf = Confidence(torch.float32).of_logits(torch.zeros(1, 4, 2, 3))
    assert torch.equal(conf, torch.full((1, 2, 3), 0.25)) and int(masks.max()) == 0


def test_confidence_style_is_no_state():
    import torch.nn as nn
    from hyperseg_amd.models._common import HyperGenBase

    class Tiny(HyperGenBase):
        def __init__(self):
            super().__init__()
            self.backbone = nn.Identity()
    m = Tiny()
    assert m.confidence_style is None
    m.confidence_style = Confidence(torch.float32, 0.5)
    assert not m.state_dict() and not list(m.buffers()) and not list(m.parameters())
    with pytest.raises(TypeError):
        m.confidence(torch.zeros(1, 3, 8, 8), style='uint8')


def test_epilogue_argument_errors():
    from hyperseg_amd.models._common import Blend, Epilogue, Score
    style = Confidence()
    target = torch.zeros(1, 4, 4, dtype=torch.uint8)
    with pytest.raises(ValueError, match='one of them per forward'):
        Epilogue(confidence=style, score=Score(target, 3, None, False))
    with pytest.raises(ValueError, match='one of them per forward'):
        Epilogue(confidence=style, blend=Blend(torch.zeros(1, 4, 4, 3, dtype=torch.uint8), None, None))
    with pytest.raises(ValueError):
        Epilogue(confidence=style, score=Score(target, 3, None, False), ignore_index=255)
    e = Epilogue(confidence=style, out_size=[8, 6])
    assert e.out_size == (8, 6) and e.confidence is style
    assert Epilogue().confidence is None
