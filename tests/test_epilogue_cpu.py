"""The route table of ``models._common.Epilogue.apply``: which ``functional`` entry the decoder's last launch is, with which arguments, and
what comes back -- pinned on recorders, so that a later rider cannot silently re-route an existing one.  No GPU."""
import pytest
import torch

from hyperseg_amd import functional as HF
from hyperseg_amd.models._common import Blend, Epilogue, Score

SIZE, LABEL = (8, 8), (6, 10)
ENTRIES = {   # entry -> what its recorder returns: sentinels of the entry's own arity
    'upsample_argmax': 'masks',
    'upsample2_argmax': 'masks2',
    'upsample_confusion': ('out', 'scored'),
    'upsample2_confusion': ('out', 'scored2'),
    'upsample_ce_confusion': ('per_pixel', 'out', 'validated'),
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


def test_every_route(calls):
    p, at_size = torch.zeros(1, 3, 4, 4), torch.zeros(1, 3, *SIZE)
    same, other, out = torch.zeros(1, *SIZE, dtype=torch.uint8), torch.zeros(1, *LABEL, dtype=torch.uint8), object()

    for epilogue in (Epilogue(), Epilogue(out_size=SIZE), Epilogue(out_size=list(SIZE))):
        assert epilogue.apply(p, SIZE) == 'masks'
        assert _one(calls) == ('upsample_argmax', (p, SIZE), {})
    assert Epilogue(out_size=LABEL).apply(p, SIZE) == 'masks2'
    assert _one(calls) == ('upsample2_argmax', (p, SIZE, LABEL), {})

    counted = dict(out=out, per_image=True, masks=True)
    assert Epilogue(score=Score(same, 5, out, True)).apply(p, SIZE) == 'scored'                      # the label at the frame's size
    assert _one(calls) == ('upsample_confusion', (p, SIZE, same, 5), counted)
    assert Epilogue(score=Score(other, 5, out, True)).apply(at_size, SIZE) == 'scored'               # p at the frame's size already
    assert _one(calls) == ('upsample_confusion', (at_size, LABEL, other, 5), counted)
    assert Epilogue(score=Score(other, 5, out, False)).apply(p, SIZE) == 'scored2'
    assert _one(calls) == ('upsample2_confusion', (p, SIZE, other, 5), dict(out=out, per_image=False, masks=True))

    for n in (5, None):                                                                              # None: nothing counted
        assert Epilogue(score=Score(same, n, out, True), ignore_index=255).apply(p, SIZE) == ('validated', 'per_pixel')
        assert _one(calls) == ('upsample_ce_confusion', (p, SIZE, same, 255, n), dict(out=out, per_image=True))

    frames, style = object(), object()
    assert Epilogue(blend=Blend(frames, style, out)).apply(p, SIZE) == ('blended_masks', 'overlay')
    assert _one(calls) == ('upsample_overlay', (p, SIZE, frames, style), dict(out=out))


def test_what_apply_rejects(calls):
    p = torch.zeros(1, 3, 4, 4)
    other = torch.zeros(1, *LABEL, dtype=torch.uint8)
    with pytest.raises(ValueError, match='target at the output size'):
        Epilogue(score=Score(other, 5, None, False), ignore_index=255).apply(p, SIZE)
    with pytest.raises(ValueError, match='out_size'):
        Epilogue(blend=Blend(None, None, None), out_size=LABEL).apply(p, SIZE)
    with pytest.raises(ValueError, match='out_size'):
        Epilogue(score=Score(torch.zeros(1, *SIZE), 5, None, False), out_size=LABEL, ignore_index=255).apply(p, SIZE)
    assert calls == []
