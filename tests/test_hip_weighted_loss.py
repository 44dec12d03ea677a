"""Class weights in the HIP loss (csrc/hs_train_aux.hip, csrc/hs_validate.hip: the weighted twins of the four cross-entropy kernels)
through autograd, functional, the criterion, the models' ``validate``, GraphedModel.validate and GraphedTrainStep.

The arithmetic is fixed -- loss = w[t] * (the unweighted loss), one more f32 multiply; the adjoint's upstream w[t] * g -- so the
comparisons against the unweighted launches are ``torch.equal``.  Against torch in float64 the bound per pixel is
max(w) * 1e-5 + 2^-23 * |ref|: 1e-5 is test_pixel_cross_entropy_vs_torch's bound for the same logit scale (randn * 4), the second term the
one extra rounding."""
import copy

import pytest
import torch
import torch.nn.functional as F

from conftest import G, rel_err
from test_weighted_loss_cpu import fixture_cases

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')

# the fixture's four shapes and one with three classes and a single row (N, C, H, W)
SHAPES = [(2, 12, 16, 24), (2, 19, 9, 11), (1, 21, 7, 13), (2, 5, 3, 70), (3, 3, 1, 70)]
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
IDS = ['f32', 'bf16', 'f16']


def _case(shape, dtype, seed):
    """logits randn * 4 in ``dtype``; ~20 % ignored targets (255; -100 for the five-class shape), ONE target equal to C that is not the
    ignore index; weights in (0.4, 4.2) with one class -- which the targets hold -- at exactly 0."""
    n, c, h, w = shape
    g = G(seed)
    ii = -100 if c == 5 else 255
    x = (torch.randn(n, c, h, w, generator=g) * 4).to(dtype)
    t = torch.randint(0, c, (n, h, w), generator=g)
    t[torch.rand(n, h, w, generator=g) < 0.2] = ii
    wt = torch.rand(c, generator=g) * 3.8 + 0.4
    zero = int(torch.randint(0, c, (1,), generator=g))
    wt[zero] = 0.0
    t.view(-1)[0], t.view(-1)[1], t.view(-1)[2] = c, zero, ii
    return x.to(DEV), t.to(DEV), wt.to(DEV), ii


def _live(t, c, ii):
    return (t != ii) & (t >= 0) & (t < c)


def _pce(x, t, ii, w=None):
    from hyperseg_amd.autograd import PixelCrossEntropy
    return PixelCrossEntropy.apply(x, t, ii) if w is None else PixelCrossEntropy.apply(x, t, ii, w)


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_weighted_forward_bits(shape, dtype):
    """weighted loss == w[t] * unweighted loss where live, exactly 0 elsewhere; cross_entropy_score(weight=) makes the same losses and
    the unweighted call's masks and counts."""
    from hyperseg_amd import functional as HF
    x, t, w, ii = _case(shape, dtype, 9100 + shape[1])
    c = shape[1]
    live = _live(t, c, ii)
    assert bool((~live).any()) and bool((t == c).any()) and bool((w[t.clamp(0, c - 1)][live] == 0).any())
    plain = _pce(x, t, ii)
    got = _pce(x, t, ii, w)
    want = torch.where(live, w[t.clamp(0, c - 1)] * plain, torch.zeros_like(plain))
    assert got.dtype == torch.float32 and torch.equal(got, want)
    assert bool((got[~live] == 0).all()) and bool((got[live & (w[t.clamp(0, c - 1)] == 0)] == 0).all())
    loss, out, masks = HF.cross_entropy_score(x, t, ii, c, masks=True, weight=w)
    loss0, out0, masks0 = HF.cross_entropy_score(x, t, ii, c, masks=True)
    assert torch.equal(loss, want) and torch.equal(loss0, plain)
    assert torch.equal(masks, masks0) and torch.equal(out, out0) and int(out.sum()) > 0
    assert torch.equal(HF.cross_entropy_score(x, t, ii, None, weight=w)[0], want)          # the uncounted form


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_weighted_adjoint_bits(shape, dtype):
    """backward with upstream r == the unweighted backward with upstream w[t] * r (0 where not live)."""
    x, t, w, ii = _case(shape, dtype, 9200 + shape[1])
    c = shape[1]
    r = torch.randn(t.shape, generator=G(9250 + c)).to(DEV)
    xa, xb = x.clone().requires_grad_(), x.clone().requires_grad_()
    _pce(xa, t, ii, w).backward(r)
    _pce(xb, t, ii).backward(torch.where(_live(t, c, ii), w[t.clamp(0, c - 1)] * r, torch.zeros_like(r)))
    assert xa.grad.dtype == dtype and torch.equal(xa.grad, xb.grad)
    assert bool((xa.grad.float().abs().sum(1)[~_live(t, c, ii)] == 0).all())


def test_weighted_vs_torch_float64(golden):
    """Against F.cross_entropy in float64 with the table: per pixel |got - ref| <= max(w) * 1e-5 + 2^-23 |ref|; the f32 gradient to
    rel_err < 1e-6."""
    for i, c in fixture_cases(golden('weighted_loss')):
        x64 = c['logits'].double().requires_grad_()
        ref = F.cross_entropy(x64, c['target'], weight=c['weight'].double(), ignore_index=c['ignore'], reduction='none')
        r = torch.randn(ref.shape, generator=G(9300 + i))
        ref.backward(r.double())
        x = c['logits'].to(DEV).requires_grad_()
        got = _pce(x, c['target'].to(DEV), c['ignore'], c['weight'].to(DEV))
        got.backward(r.to(DEV))
        err = (got.detach().cpu().double() - ref.detach()).abs()
        bound = float(c['weight'].max()) * 1e-5 + 2.0 ** -23 * ref.detach().abs()
        gerr = rel_err(x.grad.cpu(), x64.grad)
        print(f'case {i}: max err {float(err.max()):.3e} (bound at that pixel {float(bound.flatten()[err.argmax()]):.3e}), grad rel_err {gerr:.3e}')
        assert bool((err <= bound).all()), i
        assert gerr < 1e-6, i


@pytest.mark.parametrize('dtype', [torch.float32, torch.float16], ids=['f32', 'f16'])
def test_one_function_equals_the_pair(golden, dtype):
    """The weighted BootstrappedCrossEntropy (and its scored variant) == BootstrapMeanOfBatch over the weighted PixelCrossEntropy: loss
    bits and gradient bits; the scored variant's counts are confusion_update's."""
    from hyperseg_amd import functional as HF
    from hyperseg_amd.autograd import BootstrapMeanOfBatch, BootstrappedCrossEntropy, BootstrappedCrossEntropyScored
    for i, c in fixture_cases(golden('weighted_loss')):
        x0 = c['logits'].to(DEV).to(dtype)
        t, w, ii, k, th = c['target'].to(DEV), c['weight'].to(DEV), c['ignore'], c['k'], c['thresh']
        n = x0.shape[1]
        xs = [x0.clone().requires_grad_() for _ in range(3)]
        pair = BootstrapMeanOfBatch.apply(_pce(xs[0], t, ii, w).flatten(1), k, th)
        one = BootstrappedCrossEntropy.apply(xs[1], t, ii, k, th, w)
        mat = torch.zeros(n, n, dtype=torch.int64, device=DEV)
        scored = BootstrappedCrossEntropyScored.apply(xs[2], t, ii, k, th, mat, w)
        for loss in (pair, one, scored):
            loss.backward()
        assert torch.equal(one, pair) and torch.equal(scored, pair), i
        assert float(xs[0].grad.float().abs().max()) > 0
        assert torch.equal(xs[1].grad, xs[0].grad) and torch.equal(xs[2].grad, xs[0].grad), i
        assert torch.equal(mat, HF.confusion_update(x0.argmax(1), t, n)), i
        # the weights matter: the unweighted Function gives another loss
        assert not torch.equal(BootstrappedCrossEntropy.apply(x0, t, ii, k, th), pair), i


def test_criterion_on_cuda_vs_reference(golden):
    """The criterion with the reference's table on CUDA logits against the reference's loss -- test_oracle_golden.py's loss tolerance,
    |got - ref| < 1e-6 |got| + 1e-7 (its lines 228-229), which is tighter than the 1e-5 relative the issue names and so the one that
    holds -- and gradient (rel_err < 1e-5)."""
    from hyperseg_amd.training import BootstrappedCrossEntropyLoss
    for i, c in fixture_cases(golden('weighted_loss')):
        crit = BootstrappedCrossEntropyLoss(k=c['k'], thresh=c['thresh'], weight=c['weight'].clone(), ignore_index=c['ignore']).to(DEV)
        x = c['logits'].to(DEV).requires_grad_()
        assert crit.weight_takes_hip(x.shape[1], x.device)
        loss = crit(x, c['target'].to(DEV))
        loss.backward()
        got, want = float(loss.detach()), float(c['loss'])
        gerr = rel_err(x.grad.cpu(), c['grad'])
        print(f'case {i}: loss {got:.8f} ref {want:.8f} (|diff| {abs(got - want):.3e}, bound {1e-6 * abs(got) + 1e-7:.3e}) grad rel_err {gerr:.3e}')
        assert abs(got - want) < 1e-6 * abs(got) + 1e-7, i
        assert gerr < 1e-5, i


class _StockOpCalled(Exception):
    pass


@pytest.mark.parametrize('scored', [False, True], ids=['plain', 'scored'])
@pytest.mark.parametrize('amp', [False, True], ids=['f32', 'fp16-autocast'])
def test_weighted_criterion_takes_the_hip_route(golden, monkeypatch, amp, scored):
    """With F.cross_entropy made to raise, the weighted criterion still returns (and differentiates) on CUDA logits; a negative weight
    reaches the stock op: today's route."""
    from hyperseg_amd import training
    from hyperseg_amd.fps import ConfusionMatrix
    _, c = next(fixture_cases(golden('weighted_loss')))

    def refuse(*a, **kw):
        raise _StockOpCalled()
    monkeypatch.setattr(torch.nn.functional, 'cross_entropy', refuse)
    crit = training.BootstrappedCrossEntropyLoss(k=c['k'], thresh=c['thresh'], weight=c['weight'].clone(), ignore_index=c['ignore']).to(DEV)
    if scored:
        crit.score = ConfusionMatrix(12)
    t = c['target'].to(DEV)

    def run(criterion):
        x = c['logits'].to(DEV).requires_grad_()
        if amp:
            with torch.autocast('cuda', torch.float16):
                loss = criterion(x.half(), t)
        else:
            loss = criterion(x, t)
        loss.backward()
        return loss.detach(), x.grad
    loss, grad = run(crit)
    assert loss.dtype == torch.float32 and bool(torch.isfinite(loss)) and float(grad.abs().max()) > 0
    if scored:
        assert int(crit.score.mat.sum()) == int(((t >= 0) & (t < 12)).sum())
    crit.weight[3] = -0.5                                        # in place: the cached answer must not survive it
    with pytest.raises(_StockOpCalled):
        run(crit)
    crit.weight[3] = 0.5
    run(crit)
    monkeypatch.setattr(training, 'USE_HIP_CLASS_WEIGHTS', False)     # the switch restores the composed route
    with pytest.raises(_StockOpCalled):
        run(crit)


@pytest.mark.parametrize('tdtype', [torch.int64, torch.uint8], ids=['i64', 'u8'])
@pytest.mark.parametrize('size', [(18, 22), (20, 30), (19, 23), (20, 32)], ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('c', [12, 19, 5])
def test_validation_epilogue_weighted(c, size, tdtype):
    """upsample_ce_confusion(weight=) from (2, C, 9, 11): exact 2x (18, 22); the general kernel's scalar paths (20, 30), (19, 23) and its
    vector path (20, 32).  loss == the weighted PixelCrossEntropy on the resized logits; masks and counts == the unweighted call's; an
    unaligned target view takes the forms without vector loads."""
    from hyperseg_amd import functional as HF
    g = G(9500 + c + size[1])
    x = (torch.randn(2, c, 9, 11, generator=g) * 4).to(DEV)
    t = torch.randint(0, c, (2,) + size, generator=g)
    t[torch.rand(t.shape, generator=g) < 0.2] = 255
    t = t.to(tdtype).to(DEV)
    w = torch.rand(c, generator=g) * 3.8 + 0.4
    w[int(t.view(-1)[5]) % c] = 0.0
    w = w.to(DEV)
    want = _pce(HF.upsample_bilinear(x, size), t.long(), 255, w)
    loss0, out0, masks0 = HF.upsample_ce_confusion(x, size, t, 255, c)
    loss, out, masks = HF.upsample_ce_confusion(x, size, t, 255, c, weight=w)
    assert torch.equal(loss, want) and not torch.equal(loss, loss0)
    assert torch.equal(masks, masks0) and torch.equal(out, out0) and int(out.sum()) == int((t != 255).sum())
    to = torch.empty(t.numel() + 1, dtype=tdtype, device=DEV)[1:].view_as(t).copy_(t)
    assert to.storage_offset() == 1 and to.data_ptr() % 16 != 0
    loss1, out1, masks1 = HF.upsample_ce_confusion(x, size, to, 255, c, weight=w)
    assert torch.equal(loss1, want) and torch.equal(masks1, masks0) and torch.equal(out1, out0)
    with pytest.raises(ValueError):
        HF.upsample_ce_confusion(x, size, t, 255, c, weight=w.double())
    with pytest.raises(ValueError):
        HF.upsample_ce_confusion(x, size, t, 255, c, weight=w.cpu())


def test_model_and_graphed_validate_weighted():
    """model.validate with a weighted criterion: the epilogue route == criterion(model(x), target) on the device (loss bits, masks,
    counts); GraphedModel.validate == eager; a table updated in place is seen by the next replay."""
    from test_hip_eval import _model, _model_targets
    from test_hip_validate import _pin_stock_encoder
    from hyperseg_amd.fps import ConfusionMatrix
    from hyperseg_amd.training import BootstrappedCrossEntropyLoss
    from hyperseg_amd.utils.inference import GraphedModel
    n = 19
    m = _model('M', prepared=True)
    w = torch.rand(n, generator=G(9600)) * 3.8 + 0.4
    w[4] = 0.0
    crit = BootstrappedCrossEntropyLoss(k=512, thresh=0.3, weight=w, ignore_index=255).to(DEV)
    frames = [torch.rand(1, 3, 128, 256, generator=G(9601 + i)).to(DEV) for i in range(2)]
    targets = [_model_targets(f, n, 9610 + i).to(DEV) for i, f in enumerate(frames)]
    assert m._validate_fused(frames[0], targets[0], crit, n)
    served = GraphedModel(m, masks=True, num_classes=n, criterion=crit, clone_output=True)
    eager = ConfusionMatrix(n)
    for f, t in zip(frames, targets):
        want = m.validate(f, t, crit, eager)
        got = served.validate(f, t)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    torch.cuda.synchronize()
    assert torch.equal(served.confusion, eager.mat)
    before = served.validate(frames[0], targets[0])[0].clone()
    ptr = crit.weight.data_ptr()
    crit.weight.mul_(2)                                          # in place: the graph holds the table's address
    after = served.validate(frames[0], targets[0])[0].clone()
    assert crit.weight.data_ptr() == ptr and sum(1 for k in served._graphs if k[0] == 'validate') == 1
    assert torch.equal(after, m.validate(frames[0], targets[0], crit)[0]) and not torch.equal(after, before)
    crit.weight[2] = -1.0                                        # no longer a table the HIP loss takes: the composed route
    assert not m._validate_fused(frames[0], targets[0], crit, n)
    crit.weight[2] = 1.0
    short = BootstrappedCrossEntropyLoss(k=512, thresh=0.3, weight=w[:12].clone(), ignore_index=255).to(DEV)
    assert not m._validate_fused(frames[0], targets[0], short, n)          # a table of another length than the logits' channels
    # the epilogue route against the composed statement, one encoder output for both (the stock encoder does not repeat its bits)
    m = _pin_stock_encoder(m)
    for f, t in zip(frames, targets):
        cm, cm_want = ConfusionMatrix(n), ConfusionMatrix(n)
        with torch.no_grad():
            pred = m(f)
            want_loss = crit(pred, t)
        want_masks = m.evaluate(f, t, cm_want)
        assert m._validate_fused(f, t, crit, n)
        loss, masks = m.validate(f, t, crit, cm)
        assert loss.dim() == 0 and torch.equal(loss, want_loss) and torch.equal(masks, want_masks) and torch.equal(cm.mat, cm_want.mat)
        assert torch.equal(masks.long(), pred.argmax(1))


def test_graphed_train_step_weighted_and_scored():
    """GraphedTrainStep with a weighted, scored criterion: losses, parameters and the score matrix over four replays with fresh data
    are bit-equal to the eager twin's."""
    from oracle import hyperseg_oracle as O
    from test_hip_parity import build_decoder
    from hyperseg_amd.fps import ConfusionMatrix
    from hyperseg_amd.training import Adam, GraphedTrainStep, BootstrappedCrossEntropyLoss
    n = 12
    x, s = O.synth_decoder_inputs('Sc', batch=2, seed=9, size=(96, 96))
    x, s = [t.to(DEV) for t in x], s.to(DEV)

    def fresh(i):
        t = torch.randint(0, n, (2, 96, 96), generator=G(9700 + i))
        t[torch.rand(t.shape, generator=G(9750 + i)) < 0.1] = 255
        return t.to(DEV)
    w = torch.rand(n, generator=G(9790)) * 3.8 + 0.4
    w[11] = 0.0
    d0 = build_decoder('Sc', O).to(DEV).train()
    d1 = copy.deepcopy(d0)
    crits = [BootstrappedCrossEntropyLoss(weight=w.clone(), ignore_index=255).to(DEV) for _ in range(2)]
    for c in crits:
        c.score = ConfusionMatrix(n)
    opts = [Adam(d.parameters(), lr=torch.tensor(2e-3, device=DEV), betas=(0.5, 0.999)) for d in (d0, d1)]
    target = fresh(0)
    step = GraphedTrainStep(d0, crits[0], opts[0], (x, s), target.clone(), warmup=1)

    def eager(t):
        opts[1].zero_grad(set_to_none=True)
        loss = crits[1](d1(x, s), t)
        loss.backward()
        opts[1].step()
        return float(loss.detach())
    eager(target)                                                # the warm-up's step
    for i in range(1, 5):
        t = fresh(i)
        lg, le = float(step.step(target=t)[0]), eager(t)
        assert lg == le, (i, lg, le)
    torch.cuda.synchronize()
    for (k, a), (_, b_) in zip(d0.state_dict().items(), d1.state_dict().items()):
        assert torch.equal(a, b_), k
    assert torch.equal(crits[0].score.mat, crits[1].score.mat) and int(crits[0].score.mat.sum()) > 0
