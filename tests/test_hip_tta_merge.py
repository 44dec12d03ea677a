"""Flip and pyramid inference merged in the forward's last launch (csrc/hs_tta_merge.hip): ``HF.tta_merge`` against the composed route
``HF.tta_merge_composed`` -- one resize per pass, flip, max, one resize per smaller entry, the fold, arg-max, count -- and the models'
``forward`` / ``segment`` / ``evaluate`` of a list with ``HF.TTA_MERGE`` on and off.  Every comparison is ``torch.equal``: logits bits,
masks, counts."""
import pytest
import torch

from conftest import G
from test_hip_eval import DEV, _model, _model_targets, second_trip_shape
from test_hip_validate import _pin_stock_encoder

pytestmark = pytest.mark.gpu

# name -> (B, C, [(decoder output (Hi, Wi), frame (Hm, Wm)) per entry], flips).  The output size is entry 0's frame.
CASES = {
    # entry 0 alone: 2x ratio with an odd input width and Wo % 4 != 0 (the surplus-thread tail); a general ratio with an odd output width
    'plain_2x_tail': (2, 19, [((5, 7), (10, 14))], False),
    'plain_general_odd': (2, 3, [((5, 7), (11, 13))], False),
    'plain_exact2x': (1, 19, [((6, 8), (12, 16))], False),                       # the exact-2x tap form (even input width)
    'plain_identity': (2, 3, [((6, 9), (6, 9))], False),
    'flip_2x_tail': (2, 19, [((5, 7), (10, 14))], True),
    'flip_general_odd': (2, 3, [((5, 7), (11, 13))], True),                      # the mirror has a centre column
    'flip_exact2x': (1, 19, [((6, 8), (12, 16))], True),
    # 2x then a non-integer stage; a DOWN-sampling second stage (an UpDownPyramids entry)
    'three_entries': (2, 19, [((5, 7), (10, 14)), ((3, 4), (6, 8)), ((10, 14), (20, 28))], True),
    # 8 passes, the cap; the last entry's first stage is the identity
    'four_entries': (2, 3, [((5, 7), (11, 13)), ((3, 4), (6, 8)), ((10, 14), (20, 28)), ((6, 9), (6, 9))], True),
    'both_exact2x': (1, 19, [((6, 8), (12, 16)), ((3, 4), (6, 8))], True),       # entry 1: exact 2x twice
    'two_blocks': (1, 3, [((20, 28), (40, 56)), ((10, 14), (20, 28))], True),    # 560 items: more than one workgroup
    'no_flip_pyramid': (2, 3, [((5, 7), (10, 14)), ((3, 4), (6, 8)), ((10, 14), (20, 28))], False),
}


def _passes(name, seed=4200, ties=False):
    b, c, entries, flips = CASES[name]
    g = G(seed)
    passes = []
    for e, (hw, mid) in enumerate(entries):
        for flipped in ((False, True) if flips else (False,)):
            x = torch.randn(b, c, *hw, generator=g)
            if ties:
                x[:, 1:] = x[:, :1]
            passes.append((x.to(DEV), mid, flipped, e))
    return passes, b, c, entries[0][1]


def _target(b, size, n, seed, dtype):
    g = G(seed)
    t = torch.randint(0, n, (b,) + tuple(size), generator=g)
    t[torch.rand(t.shape, generator=g) < 0.15] = 255
    return t.to(dtype).to(DEV)


@pytest.mark.parametrize('gather', ['mean', 'max'])
@pytest.mark.parametrize('name', list(CASES))
def test_tta_merge_equals_the_composed_route(name, gather):
    """Logits, masks and counts of the one launch == the composed route's, for every sink selection; uint8 and int64 targets holding
    255, per_image slabs, and a pre-filled ``out`` that is accumulated into."""
    from hyperseg_amd import functional as HF
    passes, b, c, size = _passes(name)
    n = c + 2                                                   # C < n as well
    per_image = gather == 'max'
    target = _target(b, size, n, 4300, torch.uint8 if gather == 'mean' else torch.int64)
    want = HF.tta_merge_composed(passes, gather, target=target, num_classes=n, per_image=per_image, logits=True, masks=True)
    got = HF.tta_merge(passes, gather, target=target, num_classes=n, per_image=per_image, logits=True, masks=True)
    assert got.logits.shape == (b, c) + tuple(size) and torch.equal(got.logits, want.logits)
    assert got.masks.dtype == torch.uint8 and torch.equal(got.masks, want.masks)
    assert got.out.shape == ((b, n, n) if per_image else (n, n)) and torch.equal(got.out, want.out)
    assert int(got.out.sum()) == int((target != 255).sum())
    # each sink alone
    only = HF.tta_merge(passes, gather)
    assert only.logits is None and only.out is None and torch.equal(only.masks, want.masks)
    only = HF.tta_merge(passes, gather, logits=True, masks=False)
    assert only.masks is None and torch.equal(only.logits, want.logits)
    pre = torch.full_like(want.out, 7)
    only = HF.tta_merge(passes, gather, target=target, num_classes=n, out=pre, per_image=per_image, masks=False)
    assert only.masks is None and only.out is pre and torch.equal(pre, want.out + 7)           # accumulated, never zeroed


def test_one_plain_entry_is_the_final_upsample():
    from hyperseg_amd import functional as HF
    for name in ('plain_2x_tail', 'plain_general_odd', 'plain_exact2x'):
        passes, b, c, size = _passes(name)
        got = HF.tta_merge(passes, 'mean', logits=True, masks=True)
        assert torch.equal(got.logits, HF.upsample_bilinear(passes[0][0], size))
        assert torch.equal(got.masks, HF.upsample_argmax(passes[0][0], size))


@pytest.mark.parametrize('name', ['flip_general_odd', 'four_entries'])
def test_ties_take_the_lowest_index(name):
    """C = 2 with both channels equal (every pixel a tie, through both stages, the flip and the fold): class 0 everywhere."""
    from hyperseg_amd import functional as HF
    passes, b, c, size = _passes(name, ties=True)
    passes = [(x[:, :2].contiguous(), mid, f, e) for x, mid, f, e in passes]
    for gather in ('mean', 'max'):
        got = HF.tta_merge(passes, gather, logits=True)
        assert torch.equal(got.logits[:, 0], got.logits[:, 1]) and int(got.masks.max()) == 0
        assert torch.equal(got.logits, HF.tta_merge_composed(passes, gather, logits=True).logits)


def test_second_grid_trip():
    """More items per image than one pass of the grid: the grid-stride loop's second trip, with surplus lanes on it (Wo % 4 == 2)."""
    from hyperseg_amd import functional as HF
    b, c = 32, 3
    hi, wi, ho, wo = second_trip_shape('rows4', b)
    g = G(4400)
    passes = [(torch.randn(b, c, hi, wi, generator=g).to(DEV), (ho, wo), f, 0) for f in (False, True)]
    target = _target(b, (ho, wo), c, 4401, torch.uint8)
    want = HF.tta_merge_composed(passes, 'mean', target=target, num_classes=c, logits=True)
    got = HF.tta_merge(passes, 'mean', target=target, num_classes=c, logits=True)
    assert torch.equal(got.logits, want.logits) and torch.equal(got.masks, want.masks) and torch.equal(got.out, want.out)


def test_refusals_enqueue_nothing():
    """9 passes, C = 257 and a target of another size: the wrapper's error, the library's HS_ERR_UNSUPPORTED, and sinks left as they were."""
    from hyperseg_amd import _hip, functional as HF
    x = torch.randn(1, 3, 5, 7, generator=G(4500)).to(DEV)
    nine = [(x, (10, 14), False, 0)] * 9
    wide = [(torch.zeros(1, 257, 5, 7, device=DEV), (10, 14), False, 0)]
    small = _target(1, (5, 7), 3, 4501, torch.uint8)
    with pytest.raises(NotImplementedError):
        HF.tta_merge(nine, 'mean')
    with pytest.raises(NotImplementedError):
        HF.tta_merge(wide, 'mean')
    with pytest.raises(ValueError):
        HF.tta_merge(nine[:2], 'mean', target=small, num_classes=3)
    with pytest.raises(NotImplementedError):
        HF.tta_merge(nine[:2], 'mean', target=_target(1, (10, 14), 3, 4502, torch.uint8), num_classes=HF.eval_max_classes() + 1)

    def raw(passes, c, target=None, th=10, tw=14):
        table = (_hip.TtaPassC * len(passes))()
        for rec, (t, (hm, wm), f, e) in zip(table, passes):
            rec.x, rec.Hi, rec.Wi, rec.Hm, rec.Wm, rec.flipped, rec.entry = t.data_ptr(), t.shape[2], t.shape[3], hm, wm, f, e
        mask = torch.full((1, 10, 14), 99, dtype=torch.uint8, device=DEV)
        logits = torch.full((1, c, 10, 14), -5.0, device=DEV)
        mat = torch.full((3, 3), 11, dtype=torch.int64, device=DEV)
        status = _hip.lib.hs_tta_merge_fwd(table, len(passes), 1, c, 0, _hip.ptr(target), 0, th, tw, 3, 0,
                                           mat.data_ptr() if target is not None else None, mask.data_ptr(), logits.data_ptr(),
                                           _hip.stream_ptr())
        torch.cuda.synchronize()
        untouched = bool((mask == 99).all()) and bool((logits == -5.0).all()) and bool((mat == 11).all())
        return status, untouched

    assert raw(nine, 3) == (-3, True)
    assert raw(wide, 257) == (-3, True)
    assert raw(nine[:2], 3, small, 5, 7) == (-3, True)
    status, untouched = raw(nine[:2], 3)                        # (the same call with nothing to refuse does launch)
    assert status == 0 and not untouched


@pytest.fixture(scope='module')
def tta_model():
    m = _pin_stock_encoder(_model('M', prepared=True))
    assert m.inference_hflip and m.inference_gather == 'mean'
    return m


def _count_merges(monkeypatch):
    from hyperseg_amd import _hip
    calls, inner = [], _hip.run.hs_tta_merge_fwd

    def counted(*args):
        calls.append(args[1])                                   # n_passes
        return inner(*args)
    monkeypatch.setattr(_hip.run, 'hs_tta_merge_fwd', counted)
    return calls


def test_model_list_input_routes_agree(tta_model, monkeypatch):
    """model(list), model.segment(list) and model.evaluate(list, target, cm, per_image=True) with the merge launch == with HF.TTA_MERGE off
    (the composed route), bit for bit; with the switch on each of them makes the merge launch exactly once, over all four passes.
    The list is [128 x 256, 64 x 128]: HyperSeg-M's context head (a 2 x 2 convolution on the 1/32 map) does not take a 32 x 64 frame on
    any route, so the smallest two-entry pyramid it runs is this one (the sizes of the model_M_pyramid fixture)."""
    from hyperseg_amd import functional as HF
    from hyperseg_amd.fps import ConfusionMatrix
    m, n = tta_model, 19
    g = G(4600)
    xs = [torch.randn(1, 3, 128, 256, generator=g).to(DEV), torch.randn(1, 3, 64, 128, generator=g).to(DEV)]
    t = _model_targets(xs[0], n, 4601).to(DEV)
    calls = _count_merges(monkeypatch)
    with torch.no_grad():
        assert m._tta_route(xs)
        merged = m(xs)
        assert calls == [4]
        masks = m.segment(xs)
        assert calls == [4, 4]
        cm = ConfusionMatrix(n)
        scored = m.evaluate(xs, t, cm, per_image=True)
        assert calls == [4, 4, 4]
        half = m.evaluate(xs, t[:, ::2, ::2].contiguous(), ConfusionMatrix(n))        # a target of another size: merged logits, then resized
        assert calls == [4, 4, 4, 4]
        monkeypatch.setattr(HF, 'TTA_MERGE', False)
        assert not m._tta_route(xs) and m._tta_deferrable(xs)
        want = m(xs)
        want_masks = m.segment(xs)
        cm_want = ConfusionMatrix(n)
        want_scored = m.evaluate(xs, t, cm_want, per_image=True)
        want_half = m.evaluate(xs, t[:, ::2, ::2].contiguous(), ConfusionMatrix(n))
        assert calls == [4, 4, 4, 4]
    assert merged.shape == (1, n, 128, 256) and torch.equal(merged, want)
    assert masks.dtype == torch.uint8 and torch.equal(masks, want_masks) and torch.equal(masks.long(), want.argmax(1))
    assert torch.equal(scored, want_masks) and torch.equal(cm.mat, cm_want.mat)
    assert len(cm.per_image) == 1 and torch.equal(cm.per_image[0], cm_want.per_image[0])
    assert int(cm.mat.sum()) == int((t != 255).sum())
    assert half.shape == (1, 64, 128) and torch.equal(half, want_half)


def test_model_single_tensor_is_untouched(tta_model, monkeypatch):
    """The reference applies inference_hflip to list inputs only: a tensor makes no merge launch, whatever the switch says."""
    calls = _count_merges(monkeypatch)
    x = torch.randn(1, 3, 64, 128, generator=G(4700)).to(DEV)
    with torch.no_grad():
        assert not tta_model._tta_route(x)
        y = tta_model(x)
        masks = tta_model.segment(x)
    assert calls == [] and torch.equal(masks.long(), y.argmax(1))
