"""Scoring at the label's resolution (csrc/hs_eval.hip: hs_upsample2_confusion_fwd): the decoder's final resize and test.py:167-168's
resize to the label composed in registers, arg-maxed and counted in one launch -- through functional, the models' ``evaluate`` and
``segment(size=)``, and GraphedModel.evaluate.  The contract is bit-identity with the two-launch composition
``upsample_bilinear(upsample_bilinear(x, mid), label)``: every comparison is ``torch.equal`` on integers, except the one against the
reference's own op sequence (``F.interpolate`` twice on the CPU), which is held on the pixels whose top-2 margin exceeds MARGIN.

The whole file runs with ``torch.backends.cudnn.deterministic = True``, as tests/test_hip_ingest.py and tests/test_hip_overlay.py do: the model
tests compare the arg-max of TWO forwards bit for bit, and with PyTorch's default the stock HyperSeg-M forward does not repeat itself (the 1 x 1
project Conv2d of ``backbone._blocks.22`` moves by an ulp between runs on bit-equal inputs, the logits by up to 7.2e-6:
profiles/float_repeatability.txt), which flips a near-tied pixel of the 256 x 512 masks in some runs.  The flag only changes which algorithm
the stock convolutions pick; the package's own launches are the same."""
import functools

import numpy as np
import pytest
import torch

from conftest import G
from hyperseg_amd.utils.synthetic import fill_by_name

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
MARGIN = 1e-4                           # tests/test_hip_parity.py's rule and value
MAX_LEFT_OUT = 0.01                     # share of pixels at or under MARGIN; the reference alone leaves out <= 0.13 % on these recipes
MIN_TIED = 0.1

# (C, B, (Hi, Wi), (Hm, Wm), (Ho, Wo)); n = max(C, 19)
SHAPES = {
    1: (19, 1, (3, 2), (6, 4), (12, 8)),                # 2x o 2x: the smallest legal case, every output touches an edge, mid-space clamping
    2: (19, 2, (33, 50), (66, 100), (132, 200)),        # 2x o 2x: the last workgroup has surplus lanes
    3: (21, 2, (12, 16), (24, 32), (32, 43)),           # 2x, then general with Wo % 4 != 0; second trip of the stride-20 class loop
    4: (19, 1, (12, 18), (24, 36), (32, 48)),           # 2x, then 4/3 (the HyperSeg-S case)
    5: (5, 3, (16, 24), (32, 48), (16, 24)),            # down-sampling second stage; C < n
    6: (12, 1, (5, 7), (10, 14), (20, 28)),             # general first stage (odd width), then 2x
    7: (19, 1, (8, 12), (16, 24), (16, 24)),            # identity second stage: must equal upsample_confusion
    8: (24, 2, (9, 14), (18, 28), (36, 56)),            # general then 2x; clamped class loads in the second trip
    9: (2, 1, (16, 24), (32, 48), (64, 96)),            # quad lanes without a class of their own
    10: (19, 1, (64, 128), (128, 256), (256, 512)),     # several grid-stride trips per workgroup
}
NOT_ONE_STAGE = (2, 3, 4, 5, 8, 10)     # a direct x -> label resize moves the arg-max somewhere on these


@pytest.fixture(autouse=True)
def deterministic_stock_convolutions(monkeypatch):
    monkeypatch.setattr(torch.backends.cudnn, 'deterministic', True)


def _stock(target, pred, n):
    """The stock CPU ConfusionMatrix (the reference's routine) fed ``target`` and ``pred``."""
    from hyperseg_amd.fps import ConfusionMatrix
    cm = ConfusionMatrix(n)
    cm.update_stock(target.cpu().flatten().long(), pred.cpu().flatten().long())
    return cm.mat


def _targets(pattern, b, h, w, n, seed, dtype=torch.int64):
    """tests/test_hip_eval.py's three patterns -- uniform: every pixel its own class; ignored: 15 % of 255; rects: a few large
    rectangles, one of them 255."""
    g = G(seed)
    t = torch.randint(0, n, (b, h, w), generator=g)
    if pattern == 'ignored':
        t[torch.rand(b, h, w, generator=g) < 0.15] = 255
    elif pattern == 'rects':
        t[:] = 0
        for k in range(6):
            y0, x0 = int(torch.randint(0, max(1, h - 1), (1,), generator=g)), int(torch.randint(0, max(1, w - 1), (1,), generator=g))
            t[:, y0:y0 + max(2, h // 2), x0:x0 + max(2, w // 3)] = 255 if k == 3 else int(torch.randint(0, n, (1,), generator=g))
    else:
        assert pattern == 'uniform'
    return t.to(dtype)


def _logits(b, c, h, w, seed):
    """tests/test_hip_eval.py's recipe: smooth + 0.1 noise -- neighbouring pixels mostly share their arg-max, ties impossible in practice."""
    g = G(seed)
    coarse = torch.randn(b, c, max(1, h // 4), max(1, w // 4), generator=g)
    x = torch.nn.functional.interpolate(coarse, size=(h, w), mode='bilinear') + 0.1 * torch.randn(b, c, h, w, generator=g)
    return x.contiguous()


@functools.lru_cache(maxsize=None)
def _case(k):
    """(logits on the device, host logits, masks of the two-launch composition): computed once per shape and left unchanged."""
    from hyperseg_amd import functional as HF
    c, b, (hi, wi), mid, label = SHAPES[k]
    xc = _logits(b, c, hi, wi, 8000 + 10 * k)
    x = xc.to(DEV)
    two = HF.upsample_bilinear(HF.upsample_bilinear(x, mid), label)
    return x, xc, two.argmax(1).to(torch.uint8)


@pytest.mark.parametrize('pattern', ['uniform', 'ignored', 'rects'])
@pytest.mark.parametrize('tdtype', [torch.int64, torch.uint8], ids=['i64', 'u8'])
@pytest.mark.parametrize('k', sorted(SHAPES))
def test_equals_its_parts(k, tdtype, pattern):
    """upsample2_confusion(masks=True) == arg-max of the two-launch logits + the stock CPU count of those masks; the same matrix
    without the mask output; upsample2_argmax gives the same masks; and the one-stage shortcut x -> label is NOT the same."""
    from hyperseg_amd import functional as HF
    c, b, (hi, wi), mid, label = SHAPES[k]
    n = max(c, 19)
    x, _, want_masks = _case(k)
    t = _targets(pattern, b, label[0], label[1], n, 8100 + k, tdtype)
    td = t.to(DEV)
    out, masks = HF.upsample2_confusion(x, mid, td, n, masks=True)
    assert masks.dtype == torch.uint8 and tuple(masks.shape) == (b,) + label
    assert torch.equal(masks, want_masks)
    want = _stock(t, want_masks, n)
    assert out.dtype == torch.int64 and torch.equal(out.cpu(), want)
    assert torch.equal(HF.upsample2_confusion(x, mid, td, n).cpu(), want)
    assert torch.equal(HF.upsample2_argmax(x, mid, label), want_masks)
    if k == 7:
        o1, m1 = HF.upsample_confusion(x, label, td, n, masks=True)
        assert torch.equal(m1, masks) and torch.equal(o1, out)
    if k in NOT_ONE_STAGE:
        assert not torch.equal(HF.upsample_argmax(x, label), want_masks)


# The smallest shapes at which the four geometries of the last launch differ, x (2, C, 4, 6): (mid or None, target size).  C = 5: the quad
# forms' class split has a tail (c0 + sub < C); C = 21: argmax2x_block's 20-class batch loop takes a second trip.  (7, 10), (9, 13),
# (14, 22): Wo % 4 != 0, the row tail and the forms without vector loads.
SMALL = {'2x': (None, (8, 12)), 'general': (None, (7, 10)), 'two-stage-odd': ((8, 12), (9, 13)), 'two-stage-even': ((8, 12), (14, 22)),
         '2x2x': ((8, 12), (16, 24))}


@functools.lru_cache(maxsize=None)
def _small(geometry, c):
    """(x, logits at the target's size by upsample_bilinear, their arg-max): computed once per cell and left unchanged."""
    from hyperseg_amd import functional as HF
    mid, size = SMALL[geometry]
    x = _logits(2, c, 4, 6, 8700 + c).to(DEV)
    up = HF.upsample_bilinear(x, size) if mid is None else HF.upsample_bilinear(HF.upsample_bilinear(x, mid), size)
    return x, up, up.argmax(1).to(torch.uint8)


def _offset_by_one(t):
    """A copy of ``t`` whose base lies one element into its storage: the forms without vector loads."""
    o = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)[1:].view_as(t).copy_(t)
    assert o.storage_offset() == 1
    return o


@pytest.mark.parametrize('tdtype', [torch.int64, torch.uint8], ids=['i64', 'u8'])
@pytest.mark.parametrize('c', [5, 21])
@pytest.mark.parametrize('geometry', sorted(SMALL))
def test_small_shapes_every_cell(geometry, c, tdtype):
    """Confusion sink, every geometry at its smallest shape: target aligned and one element into its storage, with and without the mask
    output, n = C and n > C, and (two-stage entries) masks alone; masks == arg-max of upsample_bilinear's logits, counts == the stock
    CPU count."""
    from hyperseg_amd import functional as HF
    mid, size = SMALL[geometry]
    x, _, want_masks = _small(geometry, c)
    for n in (c, c + 3):
        t = _targets('ignored', 2, size[0], size[1], n, 8800 + n, tdtype)
        want = _stock(t, want_masks, n)
        for td in (t.to(DEV), _offset_by_one(t.to(DEV))):
            if mid is None:
                out, masks = HF.upsample_confusion(x, size, td, n, masks=True)
                bare = HF.upsample_confusion(x, size, td, n)
            else:
                out, masks = HF.upsample2_confusion(x, mid, td, n, masks=True)
                bare = HF.upsample2_confusion(x, mid, td, n)
            assert torch.equal(masks, want_masks) and torch.equal(out.cpu(), want) and torch.equal(bare.cpu(), want)
    alone = HF.upsample_argmax(x, size) if mid is None else HF.upsample2_argmax(x, mid, size)
    assert torch.equal(alone, want_masks)


def _quantised(t):
    return (t * 4).round().clamp(-4, 4) / 4


def _tie_logits(b, c, h, w, seed):
    """tests/test_hip_argmax_routes.py's recipe: multiples of 0.25 in [-1, 1], piecewise constant over 2 x 3 cells with a tenth of the
    pixels drawn on their own -- classes that agree on all the taps of a label pixel tie there bit for bit."""
    g = G(seed)
    cells = _quantised(0.2 * torch.randn(b, c, -(-h // 2), -(-w // 3), generator=g))
    x = cells.repeat_interleave(2, 2).repeat_interleave(3, 3)[:, :, :h, :w]
    own = torch.rand(b, 1, h, w, generator=g) < 0.1
    return torch.where(own, _quantised(0.2 * torch.randn(b, c, h, w, generator=g)), x).contiguous()


def _tied_fraction(logits):
    top = logits.max(1, keepdims=True)
    return float(((logits == top).sum(1) >= 2).mean())


@pytest.mark.parametrize('kind', ['random', 'equal'])
@pytest.mark.parametrize('c', [1, 2, 21])
@pytest.mark.parametrize('k', [1, 3, 6])
def test_ties_resolve_to_the_first_maximum(k, c, kind):
    """Where classes tie bit for bit the mask is numpy.argmax's (first occurrence) over the two-launch logits: in-lane the strictly
    greater value wins, across the quad's lanes the lower class."""
    from hyperseg_amd import functional as HF
    _, _, (hi, wi), mid, label = SHAPES[k]
    b = 2
    # + 5: the first seed offset at which every random case below has its tenth of tied pixels
    x = _tie_logits(b, c, hi, wi, 8200 + 100 * k + c + 5) if kind == 'random' else torch.full((b, c, hi, wi), 0.25)
    x = x.to(DEV)
    two = HF.upsample_bilinear(HF.upsample_bilinear(x, mid), label).cpu().numpy()
    tied = _tied_fraction(two)
    print(f'shape {k} C={c} {kind}: tied maxima on {tied:.3f} of the label pixels')
    if kind == 'equal':
        assert tied == (1.0 if c > 1 else 0.0)
    elif c > 1:
        assert tied >= MIN_TIED, f'only {tied:.3f} of the label pixels have a tied maximum: choose another seed'
    want = torch.from_numpy(np.argmax(two, axis=1).astype(np.uint8)).to(DEV)
    assert torch.equal(HF.upsample2_argmax(x, mid, label), want)
    t = _targets('ignored', b, label[0], label[1], max(c, 19), 8300 + k + c).to(DEV)
    out, masks = HF.upsample2_confusion(x, mid, t, max(c, 19), masks=True)
    assert torch.equal(masks, want) and torch.equal(out.cpu(), _stock(t, want, max(c, 19)))


@pytest.mark.parametrize('k', sorted(SHAPES))
def test_against_the_reference_op_sequence(k):
    """F.interpolate twice on the CPU, then argmax (the decoder's resize followed by test.py:167-168 + :171): equal masks on every
    pixel whose reference top-2 margin exceeds MARGIN; at most 1 % of the pixels are left out."""
    import torch.nn.functional as F
    from hyperseg_amd import functional as HF
    c, b, (hi, wi), mid, label = SHAPES[k]
    x, xc, _ = _case(k)
    ref = F.interpolate(F.interpolate(xc, size=mid, mode='bilinear'), size=label, mode='bilinear')
    top2 = ref.topk(2, dim=1).values
    clear = (top2[:, 0] - top2[:, 1]) > MARGIN
    left_out = 1.0 - float(clear.float().mean())
    print(f'shape {k}: {left_out:.5f} of the pixels at or under the margin')
    assert left_out <= MAX_LEFT_OUT
    masks = HF.upsample2_argmax(x, mid, label).cpu().long()
    assert torch.equal(masks[clear], ref.argmax(1)[clear])


@pytest.mark.parametrize('k', [3, 5])
def test_accumulation_and_per_image(k):
    """Two calls into one ``out`` = the sum; per_image slabs sum to the (n, n) result and slab b equals a call on image b alone."""
    from hyperseg_amd import functional as HF
    c, b, (hi, wi), mid, label = SHAPES[k]
    n = max(c, 19)
    x1, x2 = _case(k)[0], _logits(b, c, hi, wi, 8400 + k).to(DEV)
    t1, t2 = _targets('ignored', b, *label, n, 8401 + k).to(DEV), _targets('rects', b, *label, n, 8402 + k).to(DEV)
    a, m1 = HF.upsample2_confusion(x1, mid, t1, n, masks=True)
    cc = HF.upsample2_confusion(x2, mid, t2, n)
    both = HF.upsample2_confusion(x1, mid, t1, n)
    r = HF.upsample2_confusion(x2, mid, t2, n, out=both)
    assert r is both and torch.equal(both, a + cc)
    slabs = HF.upsample2_confusion(x1, mid, t1, n, per_image=True)
    assert tuple(slabs.shape) == (b, n, n) and torch.equal(slabs.sum(0), a)
    for i in range(b):
        assert torch.equal(slabs[i], HF.upsample2_confusion(x1[i:i + 1].contiguous(), mid, t1[i:i + 1].contiguous(), n))
        assert torch.equal(slabs[i].cpu(), _stock(t1[i], m1[i], n))
    HF.upsample2_confusion(x2, mid, t2, n, out=slabs, per_image=True)
    assert torch.equal(slabs.sum(0), a + cc)


MODELS = {'M': 'hyperseg-m', 'S': 'hyperseg-s', 'L': 'hyperseg-l'}            # v1_0, unify, v0_1


@functools.lru_cache(maxsize=None)
def _model(tag, prepared=False):
    from hyperseg_amd import configs
    m = fill_by_name(configs.build(MODELS[tag]).eval(), seed=11)
    if prepared:
        from hyperseg_amd.utils.inference import prepare_for_inference
        prepare_for_inference(m, fold_bn=False, fused_depthwise=True)
    return m.to(DEV)


def _label_targets(b, size, n, seed):
    g = G(seed)
    t = torch.randint(0, n, (b,) + tuple(size), generator=g)
    t[torch.rand(t.shape, generator=g) < 0.10] = 255
    return t


def _label_size(frame, ratio):
    h, w = frame
    return (2 * h, 2 * w) if ratio == '2x' else (-(-4 * h // 3), -(-4 * w // 3))


@pytest.mark.parametrize('ratio', ['2x', '4/3'])
@pytest.mark.parametrize('tag', ['M', 'S', 'L'])
def test_model_evaluate_at_label_size(golden, tag, ratio):
    """model.evaluate with a label at 2x and at 4/3 of the frame: masks and matrix equal the old chain
    upsample_bilinear(m(x), label).argmax(1) and its stock count; per_image books the same; segment(x, size=label) gives the masks."""
    from hyperseg_amd import configs
    from hyperseg_amd import functional as HF
    from hyperseg_amd.fps import ConfusionMatrix
    m = _model(tag)
    n = configs.MODELS[MODELS[tag]]['num_classes']
    x = golden(f'model_{tag}')['x'].to(DEV)
    label = _label_size(tuple(x.shape[2:]), ratio)
    t = _label_targets(x.shape[0], label, n, 8500)
    cm = ConfusionMatrix(n)
    with torch.no_grad():
        masks = m.evaluate(x, t.to(DEV), cm)
        ref = HF.upsample_bilinear(m(x).contiguous(), label).argmax(1)
        seg = m.segment(x, size=label)
        plain = m.segment(x)
    assert masks.dtype == torch.uint8 and tuple(masks.shape) == tuple(t.shape) and torch.equal(masks.long(), ref)
    want = _stock(t, ref, n)
    assert cm.mat.is_cuda and torch.equal(cm.mat.cpu(), want)
    assert seg.dtype == torch.uint8 and torch.equal(seg, masks)
    assert tuple(plain.shape[1:]) == tuple(x.shape[2:])
    cm2 = ConfusionMatrix(n)
    with torch.no_grad():
        masks2 = m.evaluate(x, t.to(torch.uint8).to(DEV), cm2, per_image=True)
    print(f'{tag} {ratio}: per_image masks differ from the first call\'s on {int((masks2 != masks).sum())} pixels, '
          f'from the old chain\'s on {int((masks2.long() != ref).sum())}')
    assert torch.equal(masks2, masks)
    assert torch.equal(cm2.mat.cpu(), want) and len(cm2.per_image) == 1
    for b in range(x.shape[0]):
        assert torch.equal(cm2.per_image[0][b].cpu(), _stock(t[b], ref[b], n))


def test_evaluate_at_label_size_is_capturable():
    """A plain torch.cuda.graph capture of model.evaluate with a label at 2x: no synchronisation on the route; replays accumulate."""
    from hyperseg_amd.fps import ConfusionMatrix
    m = _model('M')
    n = 19
    x = torch.rand(1, 3, 128, 256, generator=G(8600)).to(DEV)
    t = _label_targets(1, (256, 512), n, 8601).to(DEV)
    warm, cm = ConfusionMatrix(n), ConfusionMatrix(n)
    cm.matrix(DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        for _ in range(2):
            m.evaluate(x, t, warm)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(graph):
        masks = m.evaluate(x, t, cm)
    assert int(cm.mat.sum()) == 0                       # the capture itself counted nothing
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(cm.mat, warm.mat) and int(cm.mat.sum()) == 2 * int((t != 255).sum())
    with torch.no_grad():
        assert torch.equal(masks, m.segment(x, size=(256, 512)))


def test_graphed_evaluate_at_label_size():
    """GraphedModel.evaluate over 4 frames with labels at 2x, from pinned host memory and from the device: masks and the summed matrix
    equal the eager ones; one 'evaluate' graph per label shape; forward graphs still replay afterwards."""
    from hyperseg_amd.fps import ConfusionMatrix
    from hyperseg_amd.utils.inference import GraphedModel
    m = _model('M', prepared=True)
    n = 19
    served = GraphedModel(m, masks=True, num_classes=n, clone_output=True)
    gx = G(8700)
    frames = [torch.rand(1, 3, 128, 256, generator=gx) for _ in range(4)]
    targets = [_label_targets(1, (256, 512), n, 8701 + i) for i in range(4)]
    eager = ConfusionMatrix(n)
    want_masks = [m.evaluate(f.to(DEV), t.to(DEV), eager) for f, t in zip(frames, targets)]
    for i, (f, t) in enumerate(zip(frames, targets)):
        xin, tin = (f.pin_memory(), t.pin_memory()) if i % 2 == 0 else (f.to(DEV), t.to(DEV))
        masks = served.evaluate(xin, tin)
        assert tuple(masks.shape) == (1, 256, 512) and torch.equal(masks, want_masks[i])
    torch.cuda.synchronize()
    assert torch.equal(served.confusion, eager.mat)
    keys = [k for k in served._graphs if k[0] == 'evaluate']
    assert len(keys) == 1 and (1, 256, 512) in keys[0]
    # a second label size gets a second graph
    t2 = _label_targets(1, (171, 342), n, 8710)
    before = served.confusion.clone()
    cm = ConfusionMatrix(n)
    want = m.evaluate(frames[0].to(DEV), t2.to(DEV), cm)
    assert torch.equal(served.evaluate(frames[0].to(DEV), t2.to(DEV)), want)
    assert torch.equal(served.confusion - before, cm.mat)
    keys = [k for k in served._graphs if k[0] == 'evaluate']
    assert len(keys) == 2 and sum(1 for k in keys if (1, 256, 512) in k) == 1 and sum(1 for k in keys if (1, 171, 342) in k) == 1
    out = served(frames[0].to(DEV))
    again = served(frames[0].to(DEV))
    assert torch.equal(out, m.segment(frames[0].to(DEV))) and torch.equal(out, again)


def test_argument_errors():
    """A CPU target, a wrong batch, no target, too many classes: raised before anything is launched; n = 129 is NotImplementedError
    and evaluate then counts with stock ops."""
    from hyperseg_amd import _hip
    from hyperseg_amd import functional as HF
    from hyperseg_amd.fps import ConfusionMatrix
    x = _logits(1, 5, 8, 12, 8800).to(DEV)
    mid = (16, 24)
    t = _targets('uniform', 1, 32, 48, 5, 8801).to(DEV)
    with pytest.raises(ValueError):
        HF.upsample2_confusion(x, mid, t.cpu(), 5)
    with pytest.raises(ValueError):
        HF.upsample2_confusion(x, mid, torch.cat([t, t]), 5)                         # a wrong batch
    with pytest.raises(ValueError):
        HF.upsample2_confusion(x, mid, None, 5)                                      # masks=False with no target
    with pytest.raises(ValueError):
        HF.upsample2_confusion(x, mid, t, 4)                                         # C > n
    with pytest.raises(ValueError):
        HF.upsample2_confusion(x, mid, t, 257)
    with pytest.raises(NotImplementedError):
        HF.upsample2_confusion(x, mid, t, 129)
    with pytest.raises(ValueError):
        HF.upsample2_confusion(x, mid, t, 5, out=torch.zeros(4, 4, dtype=torch.int64, device=DEV))
    # the C entry on its own: a target without a matrix, neither and no mask, an unknown storage type, n = 129 -- nothing launched
    good = torch.zeros(5, 5, dtype=torch.int64, device=DEV)
    call = _hip.lib.hs_upsample2_confusion_fwd
    assert call(x.data_ptr(), 1, 5, 8, 12, 16, 24, 32, 48, t.data_ptr(), 1, 5, 0, None, None, None) == -1
    assert call(x.data_ptr(), 1, 5, 8, 12, 16, 24, 32, 48, None, 1, 5, 0, None, None, None) == -1
    assert call(x.data_ptr(), 1, 5, 8, 12, 16, 24, 32, 48, t.data_ptr(), 7, 5, 0, good.data_ptr(), None, None) == -1
    assert call(x.data_ptr(), 1, 5, 8, 12, 16, 24, 32, 48, t.data_ptr(), 1, 129, 0, good.data_ptr(), None, None) == -3
    torch.cuda.synchronize()
    assert int(good.sum()) == 0
    # evaluate with more classes than the LDS histogram holds: stock counting of the resized logits' masks, as before
    m = _model('M')
    big = HF.eval_max_classes() + 1
    assert big == 129
    xm = torch.rand(1, 3, 128, 256, generator=G(8802)).to(DEV)
    tb = torch.randint(0, big, (1, 256, 512), generator=G(8803))
    cm = ConfusionMatrix(big)
    with torch.no_grad():
        masks = m.evaluate(xm, tb.to(DEV), cm)
        ref = HF.upsample_bilinear(m(xm).contiguous(), (256, 512)).argmax(1)
    assert torch.equal(masks.long(), ref) and torch.equal(cm.mat.cpu(), _stock(tb, ref, big))
