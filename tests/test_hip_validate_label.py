"""The validation step at the LABEL's resolution (csrc/hs_validate.hip: hs_upsample2_ce_confusion_fwd and its weighted twin): the decoder's
final resize and train.py:119-120's resize to the label composed in registers, and from each label pixel's scores its cross entropy, its
class and its count in one launch -- through functional, the models' ``validate`` and GraphedModel.validate.  The contract is bit-identity
with the composed route: the loss with ``PixelCrossEntropy`` on ``upsample_bilinear(upsample_bilinear(x, mid), label)``, masks and counts
with ``upsample2_argmax`` / ``upsample2_confusion``; every such comparison is ``torch.equal``.  The one against the reference's own op
sequence (``F.interpolate`` twice, float64, on the CPU) holds the losses within a bound derived operation by operation.

cudnn.deterministic for the whole file, as tests/test_hip_eval_label.py (its docstring has the reason)."""
import functools

import numpy as np
import pytest
import torch

from conftest import G
from test_hip_eval import MODELS, _model, _stock
from test_hip_eval_label import MARGIN, MAX_LEFT_OUT, SHAPES, SMALL, _case, _label_size, _label_targets, _logits, _small, _targets, _tie_logits
from test_hip_validate import _ce, _criterion, _pin_stock_encoder

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


@pytest.fixture(autouse=True)
def deterministic_stock_convolutions(monkeypatch):
    monkeypatch.setattr(torch.backends.cudnn, 'deterministic', True)


@functools.lru_cache(maxsize=None)
def _two(k):
    """The two-launch logits of shape ``k`` at the label's size: computed once and left unchanged."""
    from hyperseg_amd import functional as HF
    _, _, _, mid, label = SHAPES[k]
    return HF.upsample_bilinear(HF.upsample_bilinear(_case(k)[0], mid), label)


def _offset_by_one(t):
    """A copy of ``t`` whose base lies one element into its storage: the forms without vector loads."""
    o = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)[1:].view_as(t).copy_(t)
    assert o.storage_offset() == 1
    return o


@pytest.mark.parametrize('pattern', ['uniform', 'ignored', 'rects'])
@pytest.mark.parametrize('tdtype', [torch.int64, torch.uint8], ids=['i64', 'u8'])
@pytest.mark.parametrize('k', sorted(SHAPES))
def test_equals_the_composed_route(k, tdtype, pattern):
    """loss == PixelCrossEntropy on the two-launch logits, masks == upsample2_argmax, matrix == upsample2_confusion -- for ignore_index 255
    and an in-range one that occurs (loss 0 there, still counted), one target of -1 (int64), n = C and n = C + 3, accumulation,
    per_image slabs, num_classes=None and a target one element into its storage."""
    from hyperseg_amd import functional as HF
    c, b, (hi, wi), mid, label = SHAPES[k]
    x = _case(k)[0]
    two = _two(k)
    ref_masks = HF.upsample2_argmax(x, mid, label)
    assert torch.equal(ref_masks, _case(k)[2])
    t = _targets(pattern, b, label[0], label[1], c, 9100 + k, tdtype)
    if tdtype == torch.int64:
        t[0, 0, 0] = -1                                          # never counted, loss 0
    inside = int(t[(t >= 0) & (t < c)][0])
    td = t.to(DEV)
    for ii in (255, inside):
        for n in (c, c + 3):
            loss, out, masks = HF.upsample2_ce_confusion(x, mid, td, ii, n)
            assert loss.dtype == torch.float32 and tuple(loss.shape) == (b,) + label
            assert torch.equal(loss, _ce(two, td.long(), ii)), (ii, n)
            assert masks.dtype == torch.uint8 and torch.equal(masks, ref_masks)
            want = HF.upsample2_confusion(x, mid, td, n)
            assert out.dtype == torch.int64 and torch.equal(out, want)
            if ii == inside:
                assert float(loss[td == ii].abs().max()) == 0.0 and int(want[ii].sum()) == int((t == ii).sum()) > 0
    if tdtype == torch.int64:
        assert float(loss[0, 0, 0]) == 0.0
    loss255 = _ce(two, td.long(), 255)
    again = HF.upsample2_ce_confusion(x, mid, td, 255, n, out=out)[1]
    assert again is out and torch.equal(out, 2 * want)
    slabs = HF.upsample2_ce_confusion(x, mid, td, 255, n, per_image=True)[1]
    assert tuple(slabs.shape) == (b, n, n) and torch.equal(slabs.sum(0), want)
    for i in range(b):
        li, si, mi = HF.upsample2_ce_confusion(x[i:i + 1].contiguous(), mid, td[i:i + 1].contiguous(), 255, n)
        assert torch.equal(slabs[i], si) and torch.equal(li[0], loss255[i]) and torch.equal(mi[0], ref_masks[i])
    loss0, none, masks0 = HF.upsample2_ce_confusion(x, mid, td, 255, None)
    assert none is None and torch.equal(loss0, loss255) and torch.equal(masks0, ref_masks)
    loss1, out1, masks1 = HF.upsample2_ce_confusion(x, mid, _offset_by_one(td), 255, n)
    assert torch.equal(loss1, loss255) and torch.equal(masks1, ref_masks) and torch.equal(out1, want)
    if k == 7:                                                   # identity second stage: upsample_ce_confusion outright
        l7, o7, m7 = HF.upsample_ce_confusion(x, label, td, 255, n)
        assert torch.equal(l7, loss0) and torch.equal(o7, want) and torch.equal(m7, masks0)


@pytest.mark.parametrize('tdtype', [torch.int64, torch.uint8], ids=['i64', 'u8'])
@pytest.mark.parametrize('c', [5, 21])
@pytest.mark.parametrize('geometry', sorted(SMALL))
def test_small_shapes_every_cell(geometry, c, tdtype):
    """Loss sink, every geometry at its smallest shape (tests/test_hip_eval_label.py's SMALL): target aligned and one element into its
    storage, counted (n = C + 3) and not, weighted and not; loss == PixelCrossEntropy on upsample_bilinear's logits bit for bit, masks
    == their arg-max, counts == the stock CPU count."""
    from hyperseg_amd import functional as HF
    from hyperseg_amd.autograd import PixelCrossEntropy
    mid, size = SMALL[geometry]
    x, up, want_masks = _small(geometry, c)
    n = c + 3
    t = _targets('ignored', 2, size[0], size[1], c, 9300 + c, tdtype)
    want = _stock(t, want_masks, n)
    w = (0.25 + 2.0 * torch.rand(c, generator=G(9310 + c))).to(DEV)
    for weight in (None, w):
        want_loss = _ce(up, t.to(DEV).long(), 255) if weight is None else PixelCrossEntropy.apply(up, t.to(DEV).long(), 255, weight)
        for td in (t.to(DEV), _offset_by_one(t.to(DEV))):
            for classes in (n, None):
                if mid is None:
                    loss, out, masks = HF.upsample_ce_confusion(x, size, td, 255, classes, weight=weight)
                else:
                    loss, out, masks = HF.upsample2_ce_confusion(x, mid, td, 255, classes, weight=weight)
                assert torch.equal(loss, want_loss) and torch.equal(masks, want_masks)
                assert (out is None) if classes is None else torch.equal(out.cpu(), want)


@pytest.mark.parametrize('tdtype', [torch.int64, torch.uint8], ids=['i64', 'u8'])
@pytest.mark.parametrize('k', [6, 4, 3, 2])                      # C = 12, 19, 21 in the general form; C = 19 in the 2x o 2x form
def test_weighted_twin(k, tdtype):
    """A table with one 0 and otherwise positive entries: loss == the weighted PixelCrossEntropy on the two-launch logits, bit for bit;
    masks and counts unchanged by the table."""
    from hyperseg_amd import functional as HF
    from hyperseg_amd.autograd import PixelCrossEntropy
    c, b, (hi, wi), mid, label = SHAPES[k]
    x, two = _case(k)[0], _two(k)
    w = (0.25 + 2.0 * torch.rand(c, generator=G(9200 + k)))
    w[c // 2] = 0.0
    w = w.to(DEV)
    td = _targets('ignored', b, label[0], label[1], c, 9210 + k, tdtype).to(DEV)
    plain = HF.upsample2_ce_confusion(x, mid, td, 255, c)
    for t_in in (td, _offset_by_one(td)):
        loss, out, masks = HF.upsample2_ce_confusion(x, mid, t_in, 255, c, weight=w)
        assert torch.equal(loss, PixelCrossEntropy.apply(two, td.long(), 255, w))
        assert torch.equal(loss, HF.upsample_ce_confusion(two, label, td, 255, c, weight=w)[0])
        assert torch.equal(masks, plain[2]) and torch.equal(out, plain[1])
    assert float(loss[td == c // 2].abs().max()) == 0.0 and not torch.equal(loss, plain[0])


@pytest.mark.parametrize('kind', ['duplicate', 'random', 'equal'])
@pytest.mark.parametrize('k', [1, 3, 6])
def test_ties(k, kind):
    """A duplicated channel, quantised logits and an all-equal tensor: masks are numpy's first maximum over the two-launch logits, the
    loss still PixelCrossEntropy's on them."""
    from hyperseg_amd import functional as HF
    _, _, (hi, wi), mid, label = SHAPES[k]
    b, c = 2, 21
    if kind == 'duplicate':
        x = _logits(b, c, hi, wi, 9300 + k)
        x[:, 7] = x[:, 3]
        x[:, 20] = x[:, 0]
    elif kind == 'random':
        x = _tie_logits(b, c, hi, wi, 9310 + k)
    else:
        x = torch.full((b, c, hi, wi), 0.25)
    x = x.to(DEV)
    two = HF.upsample_bilinear(HF.upsample_bilinear(x, mid), label)
    want = torch.from_numpy(np.argmax(two.cpu().numpy(), axis=1).astype(np.uint8)).to(DEV)
    t = _targets('ignored', b, label[0], label[1], c, 9320 + k).to(DEV)
    loss, out, masks = HF.upsample2_ce_confusion(x, mid, t, 255, c)
    assert torch.equal(masks, want) and torch.equal(out.cpu(), _stock(t, want, c))
    assert torch.equal(loss, _ce(two, t, 255))
    if kind == 'duplicate':
        assert not bool(((masks == 7) | (masks == 20)).any())


def test_argument_errors():
    """test_upsample_ce_confusion_argument_errors' list for the new wrapper, and the C entry's own refusals: nothing launched."""
    from hyperseg_amd import _hip
    from hyperseg_amd import functional as HF
    x = _logits(1, 5, 8, 12, 9400).to(DEV)
    mid = (16, 24)
    t = _targets('uniform', 1, 32, 48, 5, 9401).to(DEV)
    with pytest.raises(ValueError):
        HF.upsample2_ce_confusion(x, mid, torch.cat([t, t]), 255, 5)                  # a wrong batch
    with pytest.raises(ValueError):
        HF.upsample2_ce_confusion(x, mid, t.int(), 255, 5)
    with pytest.raises(ValueError):
        HF.upsample2_ce_confusion(x, mid, t, 255, 4)                                  # C > n
    with pytest.raises(ValueError):
        HF.upsample2_ce_confusion(x, mid, t.cpu(), 255, 5)
    with pytest.raises(ValueError):
        HF.upsample2_ce_confusion(x, (0, 24), t, 255, 5)
    with pytest.raises(NotImplementedError):
        HF.upsample2_ce_confusion(x, mid, t, 255, HF.eval_max_classes() + 1)
    with pytest.raises(ValueError):
        HF.upsample2_ce_confusion(x, mid, t, 255, 5, out=torch.zeros(5, 5, device=DEV))          # not int64
    with pytest.raises(ValueError):
        HF.upsample2_ce_confusion(x, mid, t, 255, None, out=torch.zeros(5, 5, dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError):
        HF.upsample2_ce_confusion(x, mid, t, 255, 5, weight=torch.ones(4, device=DEV))
    loss = torch.full((1, 32, 48), -7.0, device=DEV)
    good = torch.zeros(5, 5, dtype=torch.int64, device=DEV)
    call, twin = _hip.lib.hs_upsample2_ce_confusion_fwd, _hip.lib.hs_upsample2_ce_confusion_weighted_fwd
    head = (x.data_ptr(), 1, 5, 8, 12, 16, 24, 32, 48)
    assert call(*head, None, 1, 255, loss.data_ptr(), 5, 0, good.data_ptr(), None, None) == -1
    assert call(*head, t.data_ptr(), 7, 255, loss.data_ptr(), 5, 0, good.data_ptr(), None, None) == -1
    assert call(*head, t.data_ptr(), 1, 255, None, 5, 0, good.data_ptr(), None, None) == -1
    assert call(*head, t.data_ptr(), 1, 255, loss.data_ptr(), 4, 0, good.data_ptr(), None, None) == -1
    assert call(*head, t.data_ptr(), 1, 255, loss.data_ptr(), 129, 0, good.data_ptr(), None, None) == -3
    assert twin(*head, t.data_ptr(), 1, None, 255, loss.data_ptr(), 5, 0, good.data_ptr(), None, None) == -1
    torch.cuda.synchronize()
    assert int(good.sum()) == 0 and float(loss.max()) == -7.0


@pytest.mark.parametrize('k', sorted(SHAPES))
def test_against_the_reference_op_sequence(k):
    """F.interpolate twice, then per-pixel cross entropy, all in float64 on the CPU (the decoder's resize, then train.py:119-120 and the
    criterion's per-pixel term).  The f32 losses lie within a bound derived per pixel from the inputs, u = 2^-24 (round to nearest):

      * a bilinear stage is l0 * a + l1 * b along x, then along y: each output carries at most 3 roundings per axis pass (two products,
        one sum), 6 per stage, each relative to a magnitude <= A, the largest |x| of the tensor (convex combinations do not grow): 6 u A.
        The exact-2x form's weights (0.25, 0.75, 1, 0) are exact.  The general form computes src = scale * (dst + 0.5) - 0.5 in f32 from
        the f32 scale: the scale's rounding (u relative) and the product's each move src by <= S u, S the stage's larger input extent,
        so the weight l1 = src - floor(src) by <= 2 S u (where floor moves as well the interpolant is continuous: the same bound),
        and an axis pass' output by <= 2 S u * |a - b| <= 4 S u A: 8 S u A per general stage, 0 per exact-2x stage.
        Two stages, the second acting on the first's error with weights that sum to 1: E_v = (12 + 8 (S1 + S2)) u A on every score.
      * loss = log(sum_c exp(v_c - m)) + m - v_t.  A common error on all scores cancels; independent errors of E_v per score move
        v_t by E_v and the log-sum-exp by <= E_v (its gradient is a probability vector): 2 E_v.  If the f32 arg-max differs from
        float64's, m differs by no more than 2 E_v and the identity still holds exactly in real arithmetic.
      * the f32 evaluation itself: v - m exact to 1 u (|v - m| <= 2 A), expf to 2 ulp, C - 1 additions of terms <= 1 in a sum <= C:
        relative error of the sum <= (3 + 2 A + C) u, which the log turns into an absolute (3 + 2 A + C) u since sum >= 1; logf to
        2 ulp of log(C); + m and - v_t round relative to <= 2 A + log(C) each.
      bound = [2 (12 + 8 (S1 + S2)) A + (3 + 2 A + C) + 2 log(C) + 2 (2 A + log C)] u, computed from the inputs (A, C and the sizes), not
      from the output.
    The masks are held on the pixels whose float64 top-2 margin exceeds MARGIN; at most MAX_LEFT_OUT of the pixels are left out."""
    import math
    import torch.nn.functional as F
    from hyperseg_amd import functional as HF
    c, b, (hi, wi), mid, label = SHAPES[k]
    x, xc, _ = _case(k)
    ref = F.interpolate(F.interpolate(xc.double(), size=mid, mode='bilinear'), size=label, mode='bilinear')
    t = _targets('ignored', b, label[0], label[1], c, 9500 + k)
    want = F.cross_entropy(ref, t, ignore_index=255, reduction='none')
    loss, _, masks = HF.upsample2_ce_confusion(x, mid, t.to(DEV), 255, c)
    a = float(xc.abs().max())
    u = 2.0 ** -24
    exact = lambda i, o: o[0] == 2 * i[0] and o[1] == 2 * i[1] and i[1] % 2 == 0          # the form hs_upsample_bilinear_fwd takes
    s1, s2 = (0 if exact((hi, wi), mid) else max(hi, wi)), (0 if exact(mid, label) else max(mid))
    bound = (2 * (12 + 8 * (s1 + s2)) * a + (3 + 2 * a + c) + 2 * math.log(c) + 2 * (2 * a + math.log(c))) * u
    err = float((loss.cpu().double() - want).abs().max())
    print(f'shape {k}: max |loss - float64 reference| = {err:.3e}, bound {bound:.3e} (A = {a:.3f}, C = {c}, S1 = {s1}, S2 = {s2})')
    assert err <= bound
    top2 = ref.topk(2, dim=1).values
    clear = (top2[:, 0] - top2[:, 1]) > MARGIN
    left_out = 1.0 - float(clear.float().mean())
    assert left_out <= MAX_LEFT_OUT
    assert torch.equal(masks.cpu().long()[clear], ref.argmax(1)[clear])


def _raising(*a, **k):
    raise AssertionError('the composed route ran: upsample_bilinear was launched')


@pytest.mark.parametrize('ratio', ['up', 'half'])
@pytest.mark.parametrize('tag,prepared', [('M', False), ('S', False), ('L', False), ('Lc', False), ('M', True), ('S', True)])
def test_model_validate_at_label_size(golden, monkeypatch, tag, prepared, ratio):
    """model.validate with a label at 2x the frame (4/3 for S) and at half size: the loss equals crit on the logits resized to the label,
    masks and matrix equal model.evaluate's -- for int64 and uint8 targets, per_image, confmat=None, a weighted criterion and a raw label
    behind model.label_codec; and no resize launch is made."""
    from hyperseg_amd import configs
    from hyperseg_amd import functional as HF
    from hyperseg_amd.fps import ConfusionMatrix
    from hyperseg_amd.training import BootstrappedCrossEntropyLoss
    from hyperseg_amd.utils.labels import LabelCodec
    m = _pin_stock_encoder(_model(tag, prepared))
    n = configs.MODELS[MODELS[tag]]['num_classes']
    x = golden(f'model_{tag}')['x'].to(DEV)
    h, w = tuple(x.shape[2:])
    label = (h // 2, w // 2) if ratio == 'half' else _label_size((h, w), '4/3' if tag == 'S' else '2x')
    t = _label_targets(x.shape[0], label, n, 9600).to(DEV)
    crit = _criterion(k=256)
    assert not m._validate_fused(x, t, crit, n) and m._validate_fused_at_label(x, t, crit, n)
    cm_eval = ConfusionMatrix(n)
    with torch.no_grad():
        logits = HF.upsample_bilinear(m(x).contiguous(), label)
        want_loss = crit(logits, t)
        want_masks = m.evaluate(x, t, cm_eval)
    wcrit = BootstrappedCrossEntropyLoss(k=256, thresh=0.3, ignore_index=255, weight=(0.5 + torch.rand(n, generator=G(9601))).to(DEV))
    assert m._validate_fused_at_label(x, t, wcrit, n)
    with torch.no_grad():
        want_wloss = wcrit(logits, t)
    monkeypatch.setattr(HF, 'upsample_bilinear', _raising)
    cm = ConfusionMatrix(n)
    loss, masks = m.validate(x, t, crit, cm)
    assert loss.dim() == 0 and loss.dtype == torch.float32 and torch.equal(loss, want_loss)
    assert tuple(masks.shape) == tuple(t.shape) and torch.equal(masks, want_masks) and torch.equal(cm.mat, cm_eval.mat)
    cm2 = ConfusionMatrix(n)
    loss2, masks2 = m.validate(x, t.to(torch.uint8), crit, cm2, per_image=True)
    assert torch.equal(loss2, want_loss) and torch.equal(masks2, want_masks) and torch.equal(cm2.mat, cm_eval.mat)
    assert tuple(cm2.per_image[0].shape) == (x.shape[0], n, n)
    loss3, masks3 = m.validate(x, t, crit)
    assert torch.equal(loss3, want_loss) and torch.equal(masks3, want_masks)
    cm4 = ConfusionMatrix(n)
    loss4, masks4 = m.validate(x, t, wcrit, cm4)
    assert torch.equal(loss4, want_wloss) and torch.equal(masks4, want_masks) and torch.equal(cm4.mat, cm_eval.mat)
    # a raw label behind the codec: ids 2 * class + 1, everything else (255 among them) -> 255
    ids = torch.full((256,), 255, dtype=torch.int64)
    ids[2 * torch.arange(n) + 1] = torch.arange(n)
    raw = torch.where(t == 255, torch.full_like(t, 254), 2 * t + 1)
    monkeypatch.setattr(m, 'label_codec', LabelCodec.table(ids.tolist()), raising=False)
    assert torch.equal(m.encoded(raw), t)
    cm5 = ConfusionMatrix(n)
    loss5, masks5 = m.validate(x, raw, crit, cm5)
    assert torch.equal(loss5, want_loss) and torch.equal(masks5, want_masks) and torch.equal(cm5.mat, cm_eval.mat)


def test_graphed_validate_at_label_size():
    """GraphedModel.validate over six distinct frames with labels at 2x (pinned-host and device inputs alternate): every replay's loss and
    masks and the final matrix equal the eager ones; the warm-up did not count; one 'validate' graph for that label shape, a second
    after a same-size label; a raw label with the codec set replays with the encode launch as a node."""
    from hyperseg_amd.fps import ConfusionMatrix
    from hyperseg_amd.utils.inference import GraphedModel
    from hyperseg_amd.utils.labels import LabelCodec
    m = _model('M', prepared=True)
    n = 19
    crit = _criterion()
    served = GraphedModel(m, masks=True, num_classes=n, criterion=crit, clone_output=True)
    gx = G(9700)
    frames = [torch.rand(1, 3, 128, 256, generator=gx) for _ in range(6)]
    targets = [_label_targets(1, (256, 512), n, 9701 + i) for i in range(6)]
    eager = ConfusionMatrix(n)
    want = [m.validate(f.to(DEV), t.to(DEV), crit, eager) for f, t in zip(frames, targets)]
    for i, (f, t) in enumerate(zip(frames, targets)):
        xin, tin = (f.pin_memory(), t.pin_memory()) if i % 2 == 0 else (f.to(DEV), t.to(DEV))
        loss, masks = served.validate(xin, tin)
        assert tuple(masks.shape) == (1, 256, 512) and torch.equal(loss, want[i][0]) and torch.equal(masks, want[i][1]), i
    torch.cuda.synchronize()
    assert torch.equal(served.confusion, eager.mat)
    assert int(served.confusion.sum()) == sum(int((t != 255).sum()) for t in targets)          # the warm-up did not count
    keys = [k for k in served._graphs if k[0] == 'validate']
    assert len(keys) == 1 and (1, 256, 512) in keys[0]
    same = _label_targets(1, (128, 256), n, 9710)
    before = served.confusion.clone()
    cm = ConfusionMatrix(n)
    want_s = m.validate(frames[1].to(DEV), same.to(DEV), crit, cm)
    got_s = served.validate(frames[1].to(DEV), same.to(DEV))
    assert torch.equal(got_s[0], want_s[0]) and torch.equal(got_s[1], want_s[1]) and torch.equal(served.confusion - before, cm.mat)
    keys = [k for k in served._graphs if k[0] == 'validate']
    assert len(keys) == 2 and sum(1 for k in keys if (1, 128, 256) in k) == 1
    # a raw label: the static buffer holds it, the encode launch is the graph's first node
    ids = torch.full((256,), 255, dtype=torch.int64)
    ids[2 * torch.arange(n) + 1] = torch.arange(n)
    try:
        m.label_codec = LabelCodec.table(ids.tolist())
        before = served.confusion.clone()
        for i in (3, 4):
            raw = torch.where(targets[i] == 255, torch.full_like(targets[i], 254), 2 * targets[i] + 1)
            loss, masks = served.validate(frames[i].to(DEV), raw.to(DEV) if i == 3 else raw.pin_memory())
            assert torch.equal(loss, want[i][0]) and torch.equal(masks, want[i][1])
        torch.cuda.synchronize()
        assert int((served.confusion - before).sum()) == sum(int((targets[i] != 255).sum()) for i in (3, 4))
        keys = [k for k in served._graphs if k[0] == 'validate']
        assert len(keys) == 3 and sum(1 for k in keys if m.label_codec in k) == 1
    finally:
        del m.label_codec
