"""The validation step on the device (csrc/hs_validate.hip): loss, masks and counts from one launch, through functional, the loss
module's ``score``, the models' ``validate``, GraphedModel.validate and GraphedTrainStep.  Every comparison is ``torch.equal``: the
losses against the existing cross-entropy launch, masks and matrices against the existing arg-max / counting routes."""
import copy

import pytest
import torch

from conftest import G
from test_hip_eval import MODELS, SHAPES, _logits, _model, _model_targets, _stock, _targets, second_trip_shape

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')

CE_SHAPES = [(1, 3, 5, 7), (2, 12, 16, 24), (3, 19, 17, 23), (2, 21, 8, 40), (1, 5, 64, 128)]      # (B, C, H, W)


def _ce(logits, target, ii):
    from hyperseg_amd.autograd import PixelCrossEntropy
    return PixelCrossEntropy.apply(logits, target, ii)


@pytest.mark.parametrize('pattern', ['uniform', 'ignored', 'rects'])
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16, torch.float16], ids=['f32', 'bf16', 'f16'])
@pytest.mark.parametrize('shape', CE_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_cross_entropy_score_equals_its_parts(shape, dtype, pattern):
    """loss == PixelCrossEntropy, masks == argmax(1), matrix == update_stock, for ignore_index 255 and an in-range one (counted, loss
    0), with n = C and n = C + 3, accumulation, per_image slabs and an unaligned base (a storage offset of one element)."""
    from hyperseg_amd import functional as HF
    b, c, h, w = shape
    logits = _logits(b, c, h, w, 8000 + c + h).to(dtype).to(DEV)
    t = _targets(pattern, b, h, w, c, 8100 + c + h)
    t[0, 0, 0] = -1                                            # never counted, loss 0
    ref_masks = logits.argmax(1)
    inside = int(t[(t >= 0) & (t < c)][0])                     # an in-range ignore_index that occurs
    for ii in (255, inside):
        for n in (c, c + 3):
            td = t.to(DEV)
            loss, out, masks = HF.cross_entropy_score(logits, td, ii, n, masks=True)
            assert loss.dtype == torch.float32 and torch.equal(loss, _ce(logits, td, ii))
            assert masks.dtype == torch.uint8 and torch.equal(masks.long(), ref_masks)
            want = _stock(t, ref_masks, n)
            assert out.dtype == torch.int64 and torch.equal(out.cpu(), want)
            if ii == inside:
                assert float(loss[td == ii].abs().max()) == 0.0 and int(want[ii].sum()) == int((t == ii).sum()) > 0
    loss2, out2 = HF.cross_entropy_score(logits, td, 255, n, out=out)                 # accumulation, no masks
    assert out2 is out and torch.equal(out.cpu(), 2 * want) and torch.equal(loss2, _ce(logits, td, 255))
    _, slabs = HF.cross_entropy_score(logits, td, 255, n, per_image=True)
    assert tuple(slabs.shape) == (b, n, n) and torch.equal(slabs.sum(0).cpu(), want)
    for i in range(b):
        assert torch.equal(slabs[i].cpu(), _stock(t[i], ref_masks[i], n))
    loss0, none = HF.cross_entropy_score(logits, td, 255, None)                       # nothing counted
    assert none is None and torch.equal(loss0, loss2)
    # unaligned bases: views that start one element into their storage
    lo = torch.empty(logits.numel() + 1, dtype=dtype, device=DEV)[1:].view_as(logits).copy_(logits)
    to = torch.empty(td.numel() + 1, dtype=torch.int64, device=DEV)[1:].view_as(td).copy_(td)
    assert lo.storage_offset() == 1 and to.storage_offset() == 1
    loss3, out3, masks3 = HF.cross_entropy_score(lo, to, 255, n, masks=True)
    assert torch.equal(loss3, loss2) and torch.equal(masks3, masks) and torch.equal(out3.cpu(), want)


def test_cross_entropy_score_ties_and_limits():
    """A duplicated channel: the lower class wins, as argmax(1).  n above eval_max_classes() raises; C > n raises; the loss module then
    falls back to its own launches plus the matrix' stock update with the same numbers."""
    from hyperseg_amd import functional as HF
    from hyperseg_amd.fps import ConfusionMatrix
    from hyperseg_amd.training import BootstrappedCrossEntropyLoss
    x = _logits(2, 12, 16, 24, 8200)
    x[:, 7] = x[:, 3]
    x[:, 11] = x[:, 0]
    x = x.to(DEV)
    t = _targets('ignored', 2, 16, 24, 12, 8201).to(DEV)
    loss, out, masks = HF.cross_entropy_score(x, t, 255, 12, masks=True)
    assert torch.equal(masks.long(), x.argmax(1)) and not bool(((masks == 7) | (masks == 11)).any())
    assert torch.equal(loss, _ce(x, t, 255))
    big = HF.eval_max_classes() + 1
    with pytest.raises(NotImplementedError):
        HF.cross_entropy_score(x, t, 255, big)
    with pytest.raises(ValueError):
        HF.cross_entropy_score(x, t, 255, 11)
    with pytest.raises(ValueError):
        HF.cross_entropy_score(x, t.to(torch.uint8), 255, 12)
    with pytest.raises(ValueError):
        HF.cross_entropy_score(x, t[:, :8], 255, 12)
    plain = BootstrappedCrossEntropyLoss(k=64, ignore_index=255)
    for n in (12, big):                                       # in the loss launch / beside it
        scored = BootstrappedCrossEntropyLoss(k=64, ignore_index=255)
        scored.score = ConfusionMatrix(n)
        xa, xb = x.clone().requires_grad_(), x.clone().requires_grad_()
        la, lb = scored(xa, t), plain(xb, t)
        la.backward()
        lb.backward()
        assert torch.equal(la, lb) and torch.equal(xa.grad, xb.grad)
        assert torch.equal(scored.score.mat.cpu(), _stock(t, x.argmax(1), n))


VAL_SHAPES = SHAPES + [(12, 12, 2, 12, 16, 30, 41),          # the issue's (12, 16) -> (30, 41)
                       (19, 19, 2, 24, 40, 13, 18)]          # down-sampling


@pytest.mark.parametrize('tdtype', [torch.int64, torch.uint8])
@pytest.mark.parametrize('shape', VAL_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_upsample_ce_confusion_equals_the_composed_route(shape, tdtype):
    """loss == PixelCrossEntropy on upsample_bilinear's logits, masks == upsample_argmax, counts == upsample_confusion -- ignore_index
    255 and an in-range one, accumulation, per_image slabs, and the uncounted form."""
    from hyperseg_amd import functional as HF
    c, n, b, hi, wi, ho, wo = shape
    x = _logits(b, c, hi, wi, 8300 + c + hi).to(DEV)
    t = _targets('ignored', b, ho, wo, n, 8400 + n + ho, tdtype).to(DEV)
    up = HF.upsample_bilinear(x, (ho, wo))
    ref_masks = HF.upsample_argmax(x, (ho, wo))
    want = HF.upsample_confusion(x, (ho, wo), t, n)
    for ii in (255, 0):
        loss, out, masks = HF.upsample_ce_confusion(x, (ho, wo), t, ii, n)
        assert torch.equal(loss, _ce(up, t.long(), ii)), ii
        assert torch.equal(masks, ref_masks) and torch.equal(out, want)
    again = HF.upsample_ce_confusion(x, (ho, wo), t, 255, n, out=out)[1]
    assert again is out and torch.equal(out, 2 * want)
    slabs = HF.upsample_ce_confusion(x, (ho, wo), t, 255, n, per_image=True)[1]
    assert torch.equal(slabs, HF.upsample_confusion(x, (ho, wo), t, n, per_image=True))
    loss0, none, masks0 = HF.upsample_ce_confusion(x, (ho, wo), t, 255, None)
    assert none is None and torch.equal(loss0, _ce(up, t.long(), 255)) and torch.equal(masks0, ref_masks)
    # an unaligned target base (a view one element into its storage): the forms without vector loads of the target
    to = torch.empty(t.numel() + 1, dtype=tdtype, device=DEV)[1:].view_as(t).copy_(t)
    assert to.storage_offset() == 1
    loss1, out1, masks1 = HF.upsample_ce_confusion(x, (ho, wo), to, 255, n)
    assert torch.equal(loss1, loss0) and torch.equal(masks1, ref_masks) and torch.equal(out1, want)


@pytest.mark.parametrize('tdtype', [torch.int64, torch.uint8])
@pytest.mark.parametrize('mapping', ['rows4', 'quads'])
def test_upsample_ce_confusion_second_grid_trip(mapping, tdtype):
    """Batch 2, C = 5 < n = 21, more items per image than one pass of the grid (test_hip_eval.second_trip_shape): loss, masks and
    counts as the composed route gives them."""
    from hyperseg_amd import functional as HF
    hi, wi, ho, wo = second_trip_shape(mapping, 2)
    x = _logits(2, 5, hi, wi, 8500).to(DEV)
    t = _targets('ignored', 2, ho, wo, 21, 8501, tdtype).to(DEV)
    loss, out, masks = HF.upsample_ce_confusion(x, (ho, wo), t, 255, 21)
    assert torch.equal(loss, _ce(HF.upsample_bilinear(x, (ho, wo)), t.long(), 255))
    ref_masks = HF.upsample_argmax(x, (ho, wo))
    assert torch.equal(masks, ref_masks) and torch.equal(out.cpu(), _stock(t, ref_masks, 21))


def test_upsample_ce_confusion_argument_errors():
    from hyperseg_amd import functional as HF
    x = _logits(1, 5, 8, 12, 8500).to(DEV)
    t = _targets('uniform', 1, 16, 24, 5, 8501).to(DEV)
    with pytest.raises(ValueError):
        HF.upsample_ce_confusion(x, (16, 24), t[:, :15], 255, 5)
    with pytest.raises(ValueError):
        HF.upsample_ce_confusion(x, (16, 24), t.int(), 255, 5)
    with pytest.raises(ValueError):
        HF.upsample_ce_confusion(x, (16, 24), t, 255, 4)                           # C > n
    with pytest.raises(ValueError):
        HF.upsample_ce_confusion(x, (16, 24), t.cpu(), 255, 5)
    with pytest.raises(NotImplementedError):
        HF.upsample_ce_confusion(x, (16, 24), t, 255, HF.eval_max_classes() + 1)
    with pytest.raises(ValueError):
        HF.upsample_ce_confusion(x, (16, 24), t, 255, 5, out=torch.zeros(5, 5, device=DEV))       # not int64


def _pin_stock_encoder(m):
    """An encoder and context head do not always repeat their own bits from call to call (an unprepared model's stock
    torch modules never reliably, a prepared HyperSeg-S not always), so two passes cannot be compared with ``torch.equal``.  Each of the two returns what it returned first for the same
    input bytes: every pass of a test then feeds ONE encoder output to what is under test -- the decoder, its epilogue and the loss."""
    for mod in (m.backbone, m.weight_mapper):
        cache, inner = {}, mod.forward

        def pinned(x, cache=cache, inner=inner):
            if not isinstance(x, torch.Tensor):
                return inner(x)
            key = (tuple(x.shape), x.dtype, x.detach().cpu().numpy().tobytes())
            if key not in cache:
                cache[key] = inner(x)
            return cache[key]
        mod.forward = pinned
    return m


def _criterion(k=512):
    from hyperseg_amd.training import BootstrappedCrossEntropyLoss
    return BootstrappedCrossEntropyLoss(k=k, thresh=0.3, ignore_index=255)


@pytest.mark.parametrize('tag,prepared', [('M', False), ('S', False), ('L', False), ('Lc', False),
                                          ('M', True), ('S', True), ('L', True), ('Lc', True)])
def test_model_validate(golden, tag, prepared):
    """model.validate == (criterion(model(x), t), evaluate's masks and matrix), bit for bit, for int64 and uint8 targets, per_image and
    confmat=None."""
    from hyperseg_amd import configs
    from hyperseg_amd.fps import ConfusionMatrix
    g = golden(f'model_{tag}')
    m = _pin_stock_encoder(_model(tag, prepared))
    n = configs.MODELS[MODELS[tag]]['num_classes']
    x = g['x'].to(DEV)
    t = _model_targets(x, n, 8600).to(DEV)
    crit = _criterion()
    assert m._validate_fused(x, t, crit, n)
    cm, cm_eval = ConfusionMatrix(n), ConfusionMatrix(n)
    with torch.no_grad():
        want_loss = crit(m(x), t)
        want_masks = m.evaluate(x, t, cm_eval)
    loss, masks = m.validate(x, t, crit, cm)
    assert loss.dim() == 0 and loss.dtype == torch.float32 and torch.equal(loss, want_loss)
    assert torch.equal(masks, want_masks) and torch.equal(cm.mat, cm_eval.mat)
    cm2 = ConfusionMatrix(n)
    loss2, masks2 = m.validate(x, t.to(torch.uint8), crit, cm2, per_image=True)
    assert torch.equal(loss2, want_loss) and torch.equal(masks2, want_masks) and torch.equal(cm2.mat, cm_eval.mat)
    assert tuple(cm2.per_image[0].shape) == (x.shape[0], n, n)
    loss3, masks3 = m.validate(x, t, crit)
    assert torch.equal(loss3, want_loss) and torch.equal(masks3, want_masks)


def test_model_validate_fallback_routes(golden):
    """List input (pyramid + h-flip), training mode and a half-size target: the composed statement."""
    from hyperseg_amd import functional as HF
    from hyperseg_amd.fps import ConfusionMatrix
    g = golden('model_M_pyramid')
    m = _pin_stock_encoder(_model('M'))
    crit = _criterion()
    xs = [g['x0'].to(DEV), g['x1'].to(DEV)]
    n = 19
    t = _model_targets(xs[0], n, 8700).to(DEV)
    cm = ConfusionMatrix(n)
    with torch.no_grad():
        pred = m(xs)
    loss, masks = m.validate(xs, t, crit, cm)
    assert torch.equal(loss, crit(pred, t)) and torch.equal(masks.long(), pred.argmax(1))
    assert torch.equal(cm.mat.cpu(), _stock(t, pred.argmax(1), n))
    x = xs[0]
    th = _model_targets(x[:, :, :x.shape[2] // 2, :x.shape[3] // 2], n, 8701).to(DEV)
    assert not m._validate_fused(x, th, crit, n)
    cm = ConfusionMatrix(n)
    with torch.no_grad():
        pred = HF.upsample_bilinear(m(x).contiguous(), tuple(th.shape[1:]))
    loss, masks = m.validate(x, th, crit, cm)
    assert torch.equal(loss, crit(pred, th)) and torch.equal(masks.long(), pred.argmax(1))
    assert torch.equal(cm.mat.cpu(), _stock(th, pred.argmax(1), n))
    m = _pin_stock_encoder(_model('M').train())            # (train mode: the encoder also drops connections at random)
    with torch.no_grad():
        pred = m(x)                                            # (train-mode BatchNorm: the statistics move, the output of a pass does not)
    cm = ConfusionMatrix(n)
    loss, masks = m.validate(x, t, crit, cm)
    assert not loss.requires_grad and torch.equal(loss, crit(pred, t)) and torch.equal(masks.long(), pred.argmax(1))
    assert torch.equal(cm.mat.cpu(), _stock(t, pred.argmax(1), n))


def test_graphed_validate(golden):
    """GraphedModel.validate over six distinct frames (pinned-host and device inputs): every replay's loss and masks and the final
    matrix equal the eager ones; the warm-up's counts did not reach the graph's matrix."""
    from hyperseg_amd.fps import ConfusionMatrix
    from hyperseg_amd.utils.inference import GraphedModel
    m = _model('M', prepared=True)
    n = 19
    crit = _criterion()
    served = GraphedModel(m, masks=True, num_classes=n, criterion=crit, clone_output=True)
    gx = G(8800)
    frames = [torch.rand(1, 3, 128, 256, generator=gx) for _ in range(6)]
    targets = [_model_targets(f, n, 8801 + i) for i, f in enumerate(frames)]
    eager = ConfusionMatrix(n)
    want = [m.validate(f.to(DEV), t.to(DEV), crit, eager) for f, t in zip(frames, targets)]
    for i, (f, t) in enumerate(zip(frames, targets)):
        xin, tin = (f.pin_memory(), t.pin_memory()) if i % 2 == 0 else (f.to(DEV), t.to(DEV))
        loss, masks = served.validate(xin, tin)
        assert torch.equal(loss, want[i][0]) and torch.equal(masks, want[i][1]), i
    torch.cuda.synchronize()
    assert torch.equal(served.confusion, eager.mat)
    assert int(served.confusion.sum()) == sum(int((t != 255).sum()) for t in targets)
    assert sum(1 for k in served._graphs if k[0] == 'validate') == 1
    served.reset_confusion()
    loss, masks = served.validate(frames[0].to(DEV), targets[0].to(DEV))
    assert torch.equal(loss, want[0][0]) and int(served.confusion.sum()) == int((targets[0] != 255).sum())
    # what the graph cannot serve counts into the same matrix: a target at half size
    before = served.confusion.clone()
    th = targets[2][:, :64, :128].contiguous().to(DEV)
    cm = ConfusionMatrix(n)
    want_h = m.validate(frames[2].to(DEV), th, crit, cm)
    got_h = served.validate(frames[2].to(DEV), th)
    assert torch.equal(got_h[0], want_h[0]) and torch.equal(got_h[1], want_h[1]) and torch.equal(served.confusion - before, cm.mat)
    with pytest.raises(ValueError, match='criterion'):
        GraphedModel(m).validate(frames[0], targets[0])


class _Autocast(torch.nn.Module):
    def __init__(self, d):
        super().__init__()
        self.d = d

    def forward(self, x, s):
        with torch.autocast('cuda', dtype=torch.float16):
            return self.d(x, s)


@pytest.mark.parametrize('amp', [False, True], ids=['fp32', 'fp16'])
def test_graphed_train_step_scores(amp):
    """GraphedTrainStep with criterion.score set: losses and every parameter after five replays equal a twin's without a score; the
    matrix equals an eager scored twin's and sums to (warm-up + replays) x valid pixels; reset() between replays zeroes it in place."""
    from oracle import hyperseg_oracle as O
    from test_hip_parity import build_decoder
    from hyperseg_amd.fps import ConfusionMatrix
    from hyperseg_amd.training import Adam, GraphedTrainStep, BootstrappedCrossEntropyLoss
    n = 12
    x, s = O.synth_decoder_inputs('Sc', batch=2, seed=9, size=(96, 96))
    x, s = [t.to(DEV) for t in x], s.to(DEV)
    target = torch.randint(0, n, (2, 96, 96), generator=G(8900))
    target[torch.rand(target.shape, generator=G(8901)) < 0.1] = 255
    valid = int((target != 255).sum())
    target = target.to(DEV)
    d0 = build_decoder('Sc', O).to(DEV).train()
    twins = [d0, copy.deepcopy(d0), copy.deepcopy(d0)]         # graphed + scored, graphed without a score, eager + scored
    models = [_Autocast(d) if amp else d for d in twins]
    crits = [BootstrappedCrossEntropyLoss(ignore_index=255) for _ in twins]
    crits[0].score, crits[2].score = ConfusionMatrix(n), ConfusionMatrix(n)
    opts = [Adam(d.parameters(), lr=torch.tensor(2e-3, device=DEV), betas=(0.5, 0.999)) for d in twins]
    scalers = [torch.amp.GradScaler('cuda') if amp else None for _ in twins]
    warmup, replays = 1, 5
    scored = GraphedTrainStep(models[0], crits[0], opts[0], (x, s), target, warmup=warmup, scaler=scalers[0])
    mat = crits[0].score.mat
    plain = GraphedTrainStep(models[1], crits[1], opts[1], (x, s), target, warmup=warmup, scaler=scalers[1])

    def eager():
        opts[2].zero_grad(set_to_none=True)
        loss = crits[2](models[2](x, s), target)
        if amp:
            scalers[2].scale(loss).backward()
            scalers[2].step(opts[2])
            scalers[2].update()
        else:
            loss.backward()
            opts[2].step()
        return float(loss.detach())
    for _ in range(warmup):
        eager()
    for k in range(replays):
        ls, lp, le = float(scored.step()[0]), float(plain.step()[0]), eager()
        assert ls == lp == le, (k, ls, lp, le)
    torch.cuda.synchronize()
    for (kk, a), (_, b_), (_, c_) in zip(twins[0].state_dict().items(), twins[1].state_dict().items(), twins[2].state_dict().items()):
        assert torch.equal(a, b_) and torch.equal(a, c_), kk
    assert crits[0].score.mat is mat and torch.equal(mat, crits[2].score.mat)
    assert int(mat.sum()) == (warmup + replays) * valid
    crits[0].score.reset()
    assert crits[0].score.mat is mat and int(mat.sum()) == 0
    scored.step()
    torch.cuda.synchronize()
    assert int(mat.sum()) == valid
