"""Validation at the label's resolution, the parts that need no GPU: the routes ``Epilogue(loss_at_label=True)`` adds to ``Epilogue.apply``
(on recorders, as tests/test_epilogue_cpu.py pins the existing ones), the rule of ``HyperGenBase._validate_fused_at_label`` on CPU tensors,
and the CPU's composed route of ``model.validate``, which is what it was."""
import functools

import pytest
import torch

from conftest import G
from hyperseg_amd import functional as HF
from hyperseg_amd.models._common import Epilogue, Score
from hyperseg_amd.utils.synthetic import fill_by_name

SIZE, LABEL = (8, 8), (6, 10)
ENTRIES = {   # entry -> what its recorder returns: sentinels of the entry's own arity
    'upsample_argmax': 'masks',
    'upsample2_argmax': 'masks2',
    'upsample_confusion': ('out', 'scored'),
    'upsample2_confusion': ('out', 'scored2'),
    'upsample_ce_confusion': ('per_pixel', 'out', 'validated'),
    'upsample2_ce_confusion': ('per_pixel2', 'out', 'validated2'),
    'upsample_overlay': ('blended_masks', 'overlay'),
}


@pytest.fixture
def calls(monkeypatch):
    made = []
    for name, result in ENTRIES.items():
        monkeypatch.setattr(HF, name, lambda *args, _name=name, _result=result, **kwargs: made.append((_name, args, kwargs)) or _result)
    return made


def _one(calls):
    assert len(calls) == 1, calls
    return calls.pop()


def test_loss_at_label_routes(calls):
    p, at_size = torch.zeros(1, 3, 4, 4), torch.zeros(1, 3, *SIZE)
    same, other, out, table = torch.zeros(1, *SIZE, dtype=torch.uint8), torch.zeros(1, *LABEL, dtype=torch.uint8), object(), object()
    for n in (5, None):                                                                              # None: nothing counted
        for weight, extra in ((None, {}), (table, dict(weight=table))):
            score = Score(other, n, out, True)
            # the label at another size, p below the frame's: both resizes in the one launch
            got = Epilogue(score=score, ignore_index=255, weight=weight, loss_at_label=True).apply(p, SIZE)
            assert got == ('validated2', 'per_pixel2')
            assert _one(calls) == ('upsample2_ce_confusion', (p, SIZE, other, 255, n), dict(out=out, per_image=True, **extra))
            # p at the frame's size already: the one-stage entry, straight to the label
            got = Epilogue(score=score, ignore_index=255, weight=weight, loss_at_label=True).apply(at_size, SIZE)
            assert got == ('validated', 'per_pixel')
            assert _one(calls) == ('upsample_ce_confusion', (at_size, LABEL, other, 255, n), dict(out=out, per_image=True, **extra))
            # a label at the frame's size: exactly as without the flag
            for flag in (True, False):
                got = Epilogue(score=Score(same, n, out, False), ignore_index=255, weight=weight, loss_at_label=flag).apply(p, SIZE)
                assert got == ('validated', 'per_pixel')
                assert _one(calls) == ('upsample_ce_confusion', (p, SIZE, same, 255, n), dict(out=out, per_image=False, **extra))


def test_what_still_is_rejected(calls):
    p = torch.zeros(1, 3, 4, 4)
    other = torch.zeros(1, *LABEL, dtype=torch.uint8)
    assert Epilogue().loss_at_label is False
    for flag in ({}, dict(loss_at_label=False)):
        with pytest.raises(ValueError, match='target at the output size'):
            Epilogue(score=Score(other, 5, None, False), ignore_index=255, **flag).apply(p, SIZE)
    with pytest.raises(ValueError, match='out_size'):
        Epilogue(score=Score(other, 5, None, False), out_size=LABEL, ignore_index=255, loss_at_label=True).apply(p, SIZE)
    with pytest.raises(ValueError, match='out_size'):
        Epilogue(score=Score(torch.zeros(1, *SIZE), 5, None, False), out_size=LABEL, ignore_index=255, loss_at_label=True).apply(p, SIZE)
    with pytest.raises(ValueError, match='loss_at_label'):
        Epilogue(score=Score(other, 5, None, False), loss_at_label=True)                             # no loss to place
    assert calls == []


@functools.lru_cache(maxsize=None)
def _model():
    from hyperseg_amd import configs
    return fill_by_name(configs.build('hyperseg-m').eval(), seed=11)


def _criterion(k, **kw):
    from hyperseg_amd.training import BootstrappedCrossEntropyLoss
    return BootstrappedCrossEntropyLoss(k=k, thresh=0.3, ignore_index=255, **kw)


def test_predicate_rule():
    """On CPU tensors with ``staged=True`` (a serving wrapper stages them): true for a 2x label with k below its pixels only."""
    m = _model()
    n = 19
    x = torch.zeros(1, 3, 64, 128)
    t2, same = torch.zeros(1, 128, 256, dtype=torch.int64), torch.zeros(1, 64, 128, dtype=torch.int64)
    crit = _criterion(k=64 * 128)                                                                 # k = the FRAME's pixels < the label's
    assert m._validate_fused_at_label(x, t2, crit, n, staged=True)
    assert m._validate_fused_at_label(x, t2.to(torch.uint8), crit, None, staged=True)
    assert m._validate_fused_at_label(x, same[:, :32, :64], _criterion(k=512), n, staged=True)   # a smaller label as well
    assert not m._validate_fused(x, t2, crit, n, staged=True)
    assert not m._validate_fused_at_label(x, t2, crit, n)                                          # not staged: CPU tensors
    assert not m._validate_fused_at_label(x, same, _criterion(k=512), n, staged=True)             # _validate_fused's case
    assert m._validate_fused(x, same, _criterion(k=512), n, staged=True)
    assert not m._validate_fused_at_label(x, t2, _criterion(k=128 * 256), n, staged=True)         # k >= the label's pixels
    assert not m._validate_fused_at_label(x, t2.float(), crit, n, staged=True)
    assert not m._validate_fused_at_label(x, t2, crit, 257, staged=True)
    assert not m._validate_fused_at_label([x], t2, crit, n, staged=True)
    scored = _criterion(k=512)
    scored.score = object()
    assert not m._validate_fused_at_label(x, t2, scored, n, staged=True)
    assert not m._validate_fused_at_label(x, t2, torch.nn.CrossEntropyLoss(), n, staged=True)
    refused = torch.ones(n)
    refused[3] = -1.0                                                                             # the HIP loss takes tables >= 0 only
    assert not m._validate_fused_at_label(x, t2, _criterion(k=512, weight=refused), n, staged=True)
    assert m._validate_fused_at_label(x, t2, _criterion(k=512, weight=torch.ones(n)), n, staged=True)
    try:
        m.train()
        assert not m._validate_fused_at_label(x, t2, crit, n, staged=True)
    finally:
        m.eval()


def _toy_model():
    """tests/test_validate_cpu.py's toy: a HyperGenBase whose single-tensor pass is a CPU 1x1 convolution."""
    from hyperseg_amd.models._common import HyperGenBase

    class Toy(HyperGenBase):
        def __init__(self):
            super().__init__()
            self.net = torch.nn.Conv2d(3, 5, 1)

        def process_single_tensor(self, x, hflip=False, epilogue=None):
            assert not hflip and epilogue is None, 'CPU: nothing rides on the epilogue'
            return self.net(x)

    m = Toy()
    with torch.no_grad():
        for q in m.parameters():
            q.copy_(torch.rand(q.shape, generator=G(9900)) - 0.5)
    return m.eval()


def test_cpu_composed_route_is_unchanged():
    """model.validate on the CPU with a 2x label: criterion(F.interpolate(m(x), label), t), its arg-max and the stock count."""
    import torch.nn.functional as F
    from hyperseg_amd.fps import ConfusionMatrix
    m = _toy_model()
    n = 5
    x = torch.rand(2, 3, 12, 10, generator=G(9901))
    t = torch.randint(0, n, (2, 24, 20), generator=G(9902))
    t[0, :3] = 255
    crit = _criterion(k=16)
    assert not m._validate_fused_at_label(x, t, crit, n)                                          # CPU tensors, not staged
    with torch.no_grad():
        pred = F.interpolate(m(x), size=(24, 20), mode='bilinear')
        want = crit(pred, t)
    for tt in (t, t.to(torch.uint8)):
        cm, stock = ConfusionMatrix(n), ConfusionMatrix(n)
        loss, masks = m.validate(x, tt, crit, cm)
        assert loss.dim() == 0 and torch.equal(loss, want) and torch.equal(masks.long(), pred.argmax(1))
        stock.update_stock(t.flatten(), pred.argmax(1).flatten())
        assert torch.equal(cm.mat, stock.mat)
