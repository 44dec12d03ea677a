"""Flip and pyramid inference merged in the last launch, the host side (no GPU): the model's route rule, ``tta_merge_composed`` on CPU
tensors against a literal re-statement of the reference's loop (hyperseg_v1_0.py:76-89), and ``Epilogue(defer=True)``'s refusals."""

import pytest
import torch
import torch.nn.functional as F

from conftest import G


def _route_model(monkeypatch, hflip=True, training=False):
    """A HyperGenBase with just enough on it for the route rule; the rule itself never touches the device ("CUDA" entries are
    stand-ins that answer ``is_cuda``)."""
    from hyperseg_amd.models._common import HyperGenBase
    m = HyperGenBase()
    m.decoder = torch.nn.Identity()
    m.inference_hflip = hflip
    m.train(training)
    return m


class _OnDevice(torch.Tensor):
    """A CPU tensor that says it is on the device: what the route rule asks of an entry is ``is_cuda``, ``dim()`` and ``requires_grad``."""
    is_cuda = True


def _entry(h, w, cuda=True):
    t = torch.zeros(1, 3, h, w)
    return t.as_subclass(_OnDevice) if cuda else t


def test_route_predicate(monkeypatch):
    from hyperseg_amd import functional as HF
    m = _route_model(monkeypatch)
    xs = [_entry(64, 128), _entry(32, 64)]
    with torch.no_grad():
        assert m._tta_route(xs) and m._tta_route(tuple(xs))                       # a list input, CUDA, eval
        assert not m._tta_route(xs[0])                                            # a single tensor: not involved at all
        assert not m._tta_route([_entry(64, 128, cuda=False)])                    # a CPU tensor
        assert not _route_model(monkeypatch, training=True)._tta_route(xs)        # train mode
        assert m._tta_route([_entry(8, 8)] * 4) and not m._tta_route([_entry(8, 8)] * 5)        # 8 passes: the cap; 10
        plain = _route_model(monkeypatch, hflip=False)
        assert plain._tta_route([_entry(8, 8)] * 8) and not plain._tta_route([_entry(8, 8)] * 9)    # 9 passes
        monkeypatch.setattr(HF, 'TTA_MERGE', False)
        assert not m._tta_route(xs)                                               # the module switch: no merge launch ...
        assert m._tta_deferrable(xs)                                              # ... the same passes, composed by tta_merge_composed
        assert not m._tta_deferrable([_entry(64, 128, cuda=False)]) and not m._tta_deferrable(xs[0])
        assert plain._tta_deferrable([_entry(8, 8)] * 9)                          # composed has no pass limit
    monkeypatch.setattr(HF, 'TTA_MERGE', True)
    m.p = torch.nn.Parameter(torch.zeros(1))
    assert not m._tta_route(xs)                                                   # a parameter that needs grad, grad enabled
    with torch.no_grad():
        assert m._tta_route(xs)
    assert HF.tta_merge_takes(8, 256) and not HF.tta_merge_takes(9, 19) and not HF.tta_merge_takes(2, 257)
    assert HF.tta_merge_takes(2, 19, HF.eval_max_classes()) and not HF.tta_merge_takes(2, 19, HF.eval_max_classes() + 1)


def test_single_tensor_never_asks_the_route(monkeypatch):
    """forward(tensor) goes to process_single_tensor without the merge being involved."""
    from hyperseg_amd.models._common import HyperGenBase
    m = HyperGenBase().eval()
    seen = []
    m.process_single_tensor = lambda x, **kw: seen.append(kw) or x
    m._tta_merged = lambda *a, **kw: pytest.fail('the merge was asked for a single tensor')
    x = torch.zeros(1, 3, 8, 8)
    assert not m._tta_route(x) and not m._tta_deferrable(x)
    assert m(x) is x and seen == [{}]


class _OnCuda1(torch.Tensor):
    """A CPU tensor that says it lives on cuda:1."""
    is_cuda = True
    device = torch.device('cuda', 1)


def test_the_wrapper_takes_its_device_from_the_pass_list(monkeypatch):
    """``tta_merge`` runs with the device of its passes current (the stream handed to the library is then that device's): the pass list is
    its first operand, and ``_on_operand_device`` resolves the device from the first pass's tensor -- a model on cuda:1 called from a
    cuda:0 context."""
    from hyperseg_amd import functional as HF
    x = torch.zeros(1, 3, 4, 4)
    assert HF._device_of([(x, (8, 8), False, 0)]) == x.device
    assert HF._device_of([(x.as_subclass(_OnCuda1), (8, 8), False, 0), (x, (8, 8), True, 0)]) == torch.device('cuda', 1)
    assert HF._device_of([]) is None and HF._device_of([1, 2]) is None and HF._device_of('mean') is None
    entered = []

    class Scope:
        def __init__(self, dev):
            entered.append(dev)

        def __enter__(self):
            return self

        def __exit__(self, *exc):
            return False
    monkeypatch.setattr(torch.cuda, 'current_device', lambda: 0)
    monkeypatch.setattr(torch.cuda, 'device', Scope)
    monkeypatch.setattr(HF, '_tta_passes', lambda passes: (_ for _ in ()).throw(KeyError('inside the wrapper, under the scope')))
    with pytest.raises(KeyError):
        HF.tta_merge([(x.as_subclass(_OnCuda1), (8, 8), False, 0)], 'mean')
    assert entered == [torch.device('cuda', 1)]


def _reference_loop(logits_of, levels, hflip, gather):
    """hyperseg_v1_0.py:76-89, literally, on given per-pass logits: ``logits_of(i, flipped)`` is what process_single_tensor returns for
    entry i (for a flipped pass: already flipped back, as process_single_tensor's last line does)."""
    out_res = logits_of(0, False).shape[2:]
    out = None
    for i in range(levels):
        p = logits_of(i, False)
        if hflip:
            p = torch.max(p, logits_of(i, True))
        if p.shape[2:] != out_res:
            p = F.interpolate(p, size=out_res, mode='bilinear')
        if out is None:
            out = p
        else:
            out = (p + out) * 0.5 if gather == 'mean' else torch.max(p, out)
    return out


@pytest.mark.parametrize('gather', ['mean', 'max'])
@pytest.mark.parametrize('hflip', [False, True])
def test_composed_equals_the_reference_loop_on_cpu(gather, hflip):
    from hyperseg_amd import functional as HF
    g = G(4100)
    b, c = 2, 5
    mids = [(12, 20), (6, 10), (24, 40)]                   # entry 0, a smaller entry, an UpDownPyramids entry
    ins = [(6, 10), (6, 10), (12, 20)]                     # the decoder's outputs: half size, identity, half size
    raw = {(i, f): torch.randn(b, c, *ins[i], generator=g) for i in range(3) for f in (False, True)}

    def logits_of(i, flipped):
        y = raw[i, flipped]
        if tuple(y.shape[2:]) != mids[i]:
            y = F.interpolate(y, size=mids[i], mode='bilinear')
        return torch.flip(y, [-1]) if flipped else y

    passes = [(raw[i, f], mids[i], f, i) for i in range(3) for f in ((False, True) if hflip else (False,))]
    want = _reference_loop(logits_of, 3, hflip, gather)
    target = torch.randint(0, c, (b,) + mids[0], generator=g)
    target[torch.rand(target.shape, generator=g) < 0.1] = 255
    got = HF.tta_merge_composed(passes, gather, target=target, num_classes=c, per_image=True, logits=True, masks=True)
    assert torch.equal(got.logits, want)
    assert got.masks.dtype == torch.uint8 and torch.equal(got.masks.long(), want.argmax(1))
    mats = torch.zeros(b, c, c, dtype=torch.int64)
    for k in range(b):
        keep = target[k] != 255
        mats[k] = torch.bincount(c * target[k][keep] + want[k].argmax(0)[keep], minlength=c * c).view(c, c)
    assert torch.equal(got.out, mats)
    again = HF.tta_merge_composed(passes, gather, target=target, num_classes=c, out=got.out.sum(0).clone())
    assert again.logits is None and torch.equal(again.out, 2 * mats.sum(0))        # accumulated into


def test_pass_table_errors_on_the_host():
    from hyperseg_amd import functional as HF
    x = torch.zeros(1, 3, 4, 4)
    for bad in ([], [(x, (8, 8), False, 1)], [(x, (8, 8), False, 0), (x, (8, 8), False, 2)],
                [(x, (8, 8), False, 0), (x, (4, 4), True, 0)], [(x, (8, 8), False, 0), (torch.zeros(1, 4, 4, 4), (8, 8), True, 0)]):
        with pytest.raises(ValueError):
            HF.tta_merge_composed(bad, 'mean')
    with pytest.raises(ValueError):
        HF.tta_merge_composed([(x, (8, 8), False, 0)], 'median')


def test_deferred_epilogue():
    from hyperseg_amd.models._common import Blend, Deferred, Epilogue, Score
    p = torch.zeros(1, 3, 4, 6)[:, :, :, ::2]
    got = Epilogue(defer=True).apply(p, torch.Size((8, 6)))
    assert isinstance(got, Deferred) and got.size == (8, 6) and got.x.is_contiguous() and torch.equal(got.x, p)
    score = Score(torch.zeros(1, 8, 6, dtype=torch.uint8), 3, None, False)
    for other in (dict(score=score), dict(blend=Blend(None, None, None)), dict(confidence=object()), dict(out_size=(8, 6)),
                  dict(score=score, ignore_index=255), dict(score=score, ignore_index=255, loss_at_label=True),
                  dict(score=score, ignore_index=255, weight=torch.ones(3))):
        with pytest.raises(ValueError):
            Epilogue(defer=True, **other)
    assert not Epilogue().defer
