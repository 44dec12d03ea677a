"""fp16 storage in the training path (torch.autocast's default dtype) and the GradScaler protocol of hyperseg_amd.training.Adam.

fp16 storage is the bf16 contract with IEEE binary16 in memory: activations and their gradients stored as fp16 (rounded to nearest-even
once), every sum in fp32, the bank and its gradient fp32.  The references here are (i) the fp32 kernels on the widened inputs with one
rounding of the result, (ii) the same training step with every storage-typed kernel replaced by its fp32 kernel + fp16 roundings at the
same points (``_emulated``), and (iii) torch.optim.Adam(fused=True) under a GradScaler for the optimizer."""
import os
import re

import pytest
import torch

from conftest import G, REPO, rel_err, sub
from test_oracle_golden import TINY

F16 = torch.float16

# fp16 keeps 11 significant bits: one rounding is 2^-12 rms relative (bf16: 2^-9).  Gradients of the fp16 kernels vs the fp16 emulation
# (identical rounding points; what remains is fp32 summation order and the ReLU units it flips) are held to FP16_GRAD_TOL in relative L2,
# derived as BF16_GRAD_TOL was, from the step-level distances: observed on an MI355X, most gradients 1e-5 .. 7e-4, the largest 5.2e-3 (the
# first BatchNorm weight of the tiny v0_1 decoder's level 2: a few hundred products with heavy cancellation) and 4.0e-3 at config 5.
# Not the 8x below bf16's 2e-2 the format alone would suggest: those BatchNorm-weight reductions amplify one rounding flip.  1e-2 keeps
# a 2x margin over the worst observed value and stays half of the bf16 bar.
FP16_GRAD_TOL = 1e-2


def rel_l2(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / b.norm().clamp(min=1e-30))


# ------------------------------------------------------------------------------ host-only


def test_header_dtype_enum_matches_the_python_codes():
    from hyperseg_amd import autograd as HA
    header = open(os.path.join(REPO, 'include', 'hyperseg_hip.h')).read()
    body = re.search(r'typedef enum \{([^}]*)\} hs_dtype;', header).group(1)
    enum = {k: int(v) for k, v in re.findall(r'HS_DTYPE_(\w+)\s*=\s*(\d+)', body)}
    assert enum == {'F32': 0, 'BF16': 1, 'F16': 2}
    assert HA.DTYPE_CODES == {torch.float32: enum['F32'], torch.bfloat16: enum['BF16'], torch.float16: enum['F16']}


def test_adam_takes_the_grad_scaler_protocol():
    from hyperseg_amd.training import Adam
    assert Adam._step_supports_amp_scaling is True


def test_mixed_half_types_are_refused():
    """bf16 and fp16 tensors in one step raise (naming both types) instead of converting one of them."""
    from hyperseg_amd import autograd as HA, functional as HF
    a, b = torch.zeros(1, 2, 4, 4, dtype=torch.bfloat16), torch.zeros(1, 2, 4, 4, dtype=F16)
    with pytest.raises(NotImplementedError, match=r'torch\.bfloat16.*torch\.float16'):
        HA.storage_dtype(a, b)
    with pytest.raises(NotImplementedError, match='one half type'):
        HF.StageInput(torch.zeros(1, 2, 4, 4), b).materialize(torch.bfloat16)
    assert HA.storage_dtype(a, torch.zeros(1)) == torch.bfloat16
    assert HA.storage_dtype(b) == F16 and HA.storage_dtype(torch.zeros(1)) == torch.float32


# ------------------------------------------------------------------------------ GPU


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.fail('needs the MI355X')
    return torch.device('cuda:0')


@pytest.mark.gpu
def test_mixed_half_types_under_autocast_are_refused(dev):
    from hyperseg_amd.models.layers.meta_patch import MetaPatchConv2d
    m = MetaPatchConv2d(4, 4, 1)
    x = torch.randn(1, 4, 8, 8, device=dev).bfloat16()
    w = torch.randn(1, m.hyper_params, 2, 2, device=dev, requires_grad=True)          # (a gradient: the training route)
    with torch.autocast('cuda'), pytest.raises(NotImplementedError, match=r'torch\.bfloat16.*torch\.float16'):
        m(x, w)


@pytest.mark.gpu
def test_f16_storage_twins_round_the_fp32_kernels_once(dev):
    """hs_stage_input_typed_fwd (f32 -> f16 and f16 -> f16), hs_upsample_bilinear_f16_fwd (exact-2x and general kernels) / _typed_bwd and
    hs_cross_entropy_typed_fwd / _bwd on fp16 storage are the fp32 kernels on the widened values with ONE rounding: bit-equal to
    `fp32 kernel(x.float()).half()`; the loss of fp16 logits (fp32 out) is bit-equal to the fp32 kernel's."""
    from hyperseg_amd import autograd as HA, functional as HF
    g = G(78)
    skip = torch.randn(2, 5, 12, 20, generator=g).to(dev)
    for prev_shape in ((2, 7, 6, 10), (2, 7, 12, 20), (2, 3, 5, 7), None):
        prev = torch.randn(prev_shape, generator=g).to(dev).half() if prev_shape else None
        want = HF.StageInput(skip, prev.float() if prev is not None else None, coords=True).materialize()
        got = HF.StageInput(skip, prev, coords=True).materialize(F16)
        assert got.dtype == F16 and torch.equal(got, want.half())
        assert torch.equal(HF.StageInput(skip, prev, coords=True).materialize(torch.float32), want)
        if prev is None:
            continue
        pa = prev.clone().requires_grad_(True)
        y = HA.StageMaterialize.apply(skip, pa, True)
        assert y.dtype == F16
        r = torch.randn(y.shape, generator=g).to(dev).half()
        y.backward(r)
        pb = prev.float().requires_grad_(True)
        HA.StageMaterialize.apply(skip, pb, True).backward(r.float())
        assert pa.grad.dtype == F16 and torch.equal(pa.grad, pb.grad.half())
    with torch.autocast('cuda'):                                  # fp32 operands, fp16 result under autocast
        y = HA.StageMaterialize.apply(skip, torch.randn(2, 7, 6, 10, generator=g).to(dev), True)
    assert y.dtype == F16
    for shape, size in (((2, 12, 9, 11), (18, 22)), ((2, 12, 9, 11), (36, 44)), ((2, 12, 9, 11), (20, 30)), ((2, 12, 72, 72), (144, 144)),
                        ((1, 1, 2, 2), (4, 4)), ((1, 4, 9, 6), (23, 17))):
        x = (torch.randn(shape, generator=g) * 3).to(dev).half()
        xa, xb = x.clone().requires_grad_(True), x.float().requires_grad_(True)
        ya, yb = HA.upsample_bilinear(xa, size), HA.upsample_bilinear(xb, size)
        assert ya.dtype == F16 and torch.equal(ya, yb.half()), (shape, size)
        r = torch.randn(ya.shape, generator=g).to(dev).half()
        ya.backward(r)
        yb.backward(r.float())
        assert xa.grad.dtype == F16 and torch.equal(xa.grad, xb.grad.half()), (shape, size)
    logits = (torch.randn(2, 12, 16, 24, generator=g) * 4).to(dev).half()
    t = torch.randint(0, 12, (2, 16, 24), generator=g)
    t[torch.rand(t.shape, generator=g) < 0.2] = 255
    t = t.to(dev)
    la, lb = logits.clone().requires_grad_(True), logits.float().requires_grad_(True)
    pa, pb = HA.PixelCrossEntropy.apply(la, t, 255), HA.PixelCrossEntropy.apply(lb, t, 255)
    assert pa.dtype == torch.float32 and torch.equal(pa, pb)
    r = torch.rand(t.shape, generator=g).to(dev)
    (pa * r).sum().backward()
    (pb * r).sum().backward()
    assert la.grad.dtype == F16 and torch.equal(la.grad, lb.grad.half())


@pytest.mark.gpu
def test_f16_rounding_matches_torch_half(dev):
    """One store of the f16 kernels rounds as torch's .half(): nearest-even, overflow to +-inf, NaN stays NaN (the stage-input kernel
    copies its skip channels through one widening and one rounding)."""
    from hyperseg_amd import functional as HF
    vals = torch.tensor([0.0, -0.0, 1.0, 1.0 + 2 ** -11, 1.0 + 3 * 2 ** -11, 65504.0, 65519.0, 65520.0, -1e6, 1e-8, 6e-8, 3e-5,
                         float('inf'), float('-inf'), float('nan')] + torch.randn(49, generator=G(79)).mul(1e3).tolist())
    skip = vals.view(1, 1, 8, 8).to(dev)
    got = HF.StageInput(skip, None, coords=False).materialize(F16)
    want = skip.half()
    assert torch.equal(got.isnan(), want.isnan())
    ok = ~want.isnan()
    assert torch.equal(got[ok], want[ok])


@pytest.mark.gpu
@pytest.mark.parametrize('case', [
    dict(cin=24, cout=48, k=1, groups=1, mode='zeros', b=2, grid=(3, 4), patch=(10, 10)),
    dict(cin=48, cout=48, k=3, groups=48, mode='zeros', b=2, grid=(3, 4), patch=(10, 10)),
    dict(cin=6, cout=4, k=3, groups=1, mode='reflect', b=2, grid=(3, 4), patch=(4, 2)),
    dict(cin=82, cout=64, k=1, groups=1, mode='zeros', b=1, grid=(4, 6), patch=(1, 1)),
    dict(cin=22, cout=44, k=1, groups=1, mode='zeros', b=2, grid=(2, 3), patch=(32, 32)),
    dict(cin=44, cout=12, k=1, groups=1, mode='zeros', b=1, grid=(3, 2), patch=(16, 16)),
    dict(cin=6, cout=20, k=1, groups=1, mode='zeros', b=1, grid=(2, 2), patch=(3, 7)),
    dict(cin=6, cout=6, k=3, groups=6, mode='zeros', b=1, grid=(2, 3), patch=(6, 7)),
])
def test_patch_conv_f16_storage_vs_fp32_oracle(dev, case):
    """hs_patch_conv_plain_{fwd,bwd_in,bwd_w} with fp16 storage (k = 1 matrix-core, depthwise, general and tiny-patch forms) against
    the fp32 oracle fed the SAME fp16-rounded inputs: what remains is fp32 accumulation order + one rounding of each result to fp16
    (2^-12 rms)."""
    from oracle import hyperseg_oracle as O
    from hyperseg_amd.models.layers.meta_patch import MetaPatchConv2d
    c = case
    g = G(24)
    h, w = c['grid'][0] * c['patch'][0], c['grid'][1] * c['patch'][1]
    m = MetaPatchConv2d(c['cin'], c['cout'], c['k'], padding=c['k'] // 2, groups=c['groups'], padding_mode=c['mode'])
    rnd = lambda t: t.half().float()                # noqa: E731
    x = rnd(torch.randn(c['b'], c['cin'], h, w, generator=g))
    wt = rnd(torch.randn(c['b'], m.hyper_params, *c['grid'], generator=g) * (1.0 / (c['cin'] // c['groups'] * c['k'] ** 2)) ** 0.5)
    r = rnd(torch.randn(c['b'], c['cout'], h, w, generator=g))
    xo, wo = x.clone().requires_grad_(True), wt.clone().requires_grad_(True)
    yo = O.meta_patch_conv2d(xo, wo, c['cout'], c['k'], c['k'] // 2, c['mode'], c['groups'])
    (yo * r).sum().backward()
    xg, wg = x.to(dev).requires_grad_(True), wt.to(dev).requires_grad_(True)
    with torch.autocast('cuda'):
        yg = m(xg, wg)
    assert yg.dtype == F16
    (yg.float() * r.to(dev)).sum().backward()
    assert rel_l2(yg.detach().float().cpu(), yo.detach()) < 6e-4
    assert rel_l2(xg.grad.cpu(), xo.grad) < 6e-4
    assert rel_l2(wg.grad.cpu(), wo.grad) < 6e-4


@pytest.mark.gpu
@pytest.mark.parametrize('act', [None, 'relu6'])
@pytest.mark.parametrize('shape', [(2, 6, 200, 160), (648, 5, 18, 18), (1, 3, 300, 211), (2, 44, 36, 54)])
def test_fused_training_batchnorm_f16_storage_vs_the_fp32_kernels(dev, shape, act):
    """hs_bn_act_train_fwd / _bwd on fp16 storage (pair mode on the even planes, single elements otherwise, the one-launch form on the
    small channels) against the same kernels on the widened input: output within one fp16 rounding, gradients at fp16's resolution."""
    import copy
    from hyperseg_amd import autograd as HA
    g = G(shape[0] + shape[2] + 1)
    bn0 = torch.nn.BatchNorm2d(shape[1], momentum=0.1).to(dev).train()
    with torch.no_grad():
        bn0.weight.copy_(torch.rand(shape[1], generator=g) + 0.5)
        bn0.bias.copy_(torch.randn(shape[1], generator=g) * 0.5)
    bn1 = copy.deepcopy(bn0)
    layer = None if act is None else torch.nn.ReLU6()
    x = (torch.randn(shape, generator=g) * 2 + torch.randn(1, shape[1], 1, 1, generator=g)).to(dev).half()
    r = torch.randn(shape, generator=g).to(dev)
    xa, xb = x.float().requires_grad_(True), x.clone().requires_grad_(True)
    ya, yb = HA.bn_act(bn0, layer, xa), HA.bn_act(bn1, layer, xb)
    assert yb.dtype == F16
    (ya * r).sum().backward()
    (yb.float() * r).sum().backward()
    assert rel_err(yb.detach().float().cpu(), ya.detach().cpu()) < 1e-3
    assert rel_l2(xb.grad.float().cpu(), xa.grad.cpu()) < 3e-3
    assert rel_l2(bn1.weight.grad.cpu(), bn0.weight.grad.cpu()) < 3e-3 and rel_l2(bn1.bias.grad.cpu(), bn0.bias.grad.cpu()) < 3e-3
    assert torch.allclose(bn1.running_mean, bn0.running_mean, rtol=1e-5, atol=1e-6)
    assert torch.allclose(bn1.running_var, bn0.running_var, rtol=1e-5, atol=1e-6)


def _emulated(monkeypatch, low):
    """The half-storage training step computed by the FP32 kernels with ``low`` (bf16 / fp16) roundings at the same points: every
    storage-typed kernel of the step -- the patch convolutions (``autograd._plain_conv``), the tile re-layouts, the depthwise tile
    kernels, BatchNorm, the stage input, the logits' upsample and the loss -- runs on widened operands and its half outputs are rounded
    once, where the typed kernel stores them.  (tests/test_hip_training.py's bf16 emulation, parametrised by the storage type.)"""
    import hyperseg_amd.autograd as HA
    real = HA._plain_conv

    def emulated(kind, dtype, a, b, ld, shape, meta, out):
        if dtype != low:
            return real(kind, dtype, a, b, ld, shape, meta, out)
        a32 = a.float().contiguous()
        b32 = b.float().contiguous()
        out32 = torch.zeros(out.shape, device=out.device, dtype=torch.float32)
        ld32 = b32.stride(0) if kind != 'bwd_w' else out32.stride(0)
        real(kind, torch.float32, a32, b32, ld32, shape, meta, out32)
        out.copy_(out32)
        return out
    monkeypatch.setattr(HA, '_plain_conv', emulated)

    def widen(t):
        return t.float() if isinstance(t, torch.Tensor) and t.dtype == low else t

    def rnd(t):
        return t.to(low) if isinstance(t, torch.Tensor) and t.is_floating_point() else t

    low_depth = [0]
    real_dz = HA._dw_tiles_input_gradient

    def emulated_dz(*a, **k):
        out = real_dz(*a, **k)
        return out.to(low).float() if low_depth[0] and out.dtype == torch.float32 else out
    monkeypatch.setattr(HA, '_dw_tiles_input_gradient', emulated_dz)
    monkeypatch.setattr(HA, 'USE_DW_BN_BWD_FUSED', False)
    real_cz = HA._conv_input_gradient

    def emulated_cz(*a, **k):
        out = real_cz(*a, **k)
        return out.to(low).float() if low_depth[0] and out.dtype == torch.float32 else out
    monkeypatch.setattr(HA, '_conv_input_gradient', emulated_cz)

    def wrap(cls, fwd_low=(0,), bwd_low=(0,), low_rule=None, no_autocast=False):
        real_f, real_b = cls.forward, cls.backward

        def fwd(ctx, *args):
            is_low = low_rule(*args) if low_rule is not None else any(isinstance(a, torch.Tensor) and a.dtype == low for a in args)
            ctx._emu_low = bool(is_low)
            ctx._emu_in_dtypes = [a.dtype if isinstance(a, torch.Tensor) else None for a in args]
            if not is_low:
                return real_f(ctx, *args)
            with torch.autocast('cuda', enabled=not no_autocast and torch.is_autocast_enabled('cuda'), dtype=low):
                out = real_f(ctx, *[widen(a) for a in args])
            if isinstance(out, tuple):
                return tuple(rnd(o) if i in fwd_low else o for i, o in enumerate(out))
            assert out.dtype == torch.float32, (cls.__name__, out.dtype)
            return rnd(out) if 0 in fwd_low else out

        def bwd(ctx, *grads):
            if not ctx._emu_low:
                return real_b(ctx, *grads)
            low_depth[0] += 1
            try:
                out = real_b(ctx, *[widen(g) for g in grads])
            finally:
                low_depth[0] -= 1
            out = list(out) if isinstance(out, tuple) else [out]
            for i in bwd_low:
                if out[i] is not None:
                    out[i] = rnd(out[i])
                    dt = ctx._emu_in_dtypes[i]
                    if dt is not None and dt != low:
                        out[i] = out[i].to(dt)
            return tuple(out)
        monkeypatch.setattr(cls, 'forward', staticmethod(fwd))
        monkeypatch.setattr(cls, 'backward', staticmethod(bwd))

    wrap(HA.HaloTiles)
    wrap(HA.TileInterior)
    wrap(HA.DwTilesValid)
    wrap(HA.DwTilesBN)
    wrap(HA.PatchConvBN, no_autocast=True)
    wrap(HA.BNActTrain)
    wrap(HA.PixelCrossEntropy, fwd_low=())
    wrap(HA.BootstrappedCrossEntropy, fwd_low=())
    wrap(HA.UpsampleBilinear)

    def stage_low(skip, prev, coords):
        return (torch.is_autocast_enabled('cuda') and torch.get_autocast_dtype('cuda') == low) or \
            (prev is not None and prev.dtype == low) or skip.dtype == low
    wrap(HA.StageMaterialize, bwd_low=(0, 1), low_rule=stage_low, no_autocast=True)


def _half_step(d, x, w, r):
    """One train-mode forward + backward under plain ``torch.autocast('cuda')`` (fp16 by default)."""
    xs = [t.detach().clone().requires_grad_(True) for t in x]
    ws = [t.detach().clone().requires_grad_(True) for t in w] if isinstance(w, list) else w.detach().clone().requires_grad_(True)
    d.zero_grad()
    with torch.autocast('cuda'):
        y = d(xs, ws)
    (y.float() * r).sum().backward()
    out = {'logits': y.detach().float(), 'dtype': y.dtype}
    for i, t in enumerate(xs):
        if t.grad is not None:
            out[f'd pyramid[{i}]'] = t.grad.clone()
    for i, t in enumerate(ws if isinstance(ws, list) else [ws]):
        out[f'd weights[{i}]'] = t.grad.clone()
    for k, p in d.named_parameters():
        if p.grad is not None:
            out['d ' + k] = p.grad.float().clone()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['t_v1_0', 't_unify', 't_v0_1'])
def test_train_step_under_default_autocast_vs_f16_emulation(golden, dev, name, monkeypatch):
    """The tiny decoders' training step under plain ``torch.autocast('cuda')`` (fp16: it raised NotImplementedError before fp16 storage
    existed) runs with fp16 storage end to end -- every activation the step saves is fp16 -- and matches the same step computed by the
    fp32 kernels + fp16 roundings at the same points: logits 5e-4, gradients FP16_GRAD_TOL (relative L2).  Against the reference's fp32
    fixture the logits are held to 2e-3."""
    from hyperseg_amd import autograd as HA
    from test_hip_training import make_decoder
    assert torch.get_autocast_dtype('cuda') == F16
    g = golden('train_' + name)
    c = TINY[name]
    d = make_decoder(c)
    d.load_state_dict(sub(g, 'p.'), strict=False)
    d = d.to(dev).train()
    x = [g[f'x{i}'].to(dev) for i in range(6)]
    w = [g[f'w{i}'].to(dev) for i in range(6)] if c['variant'] == 'v0_1' else g['s'].to(dev)
    r = g['r'].to(dev)
    bn_state = {k: v.clone() for k, v in d.state_dict().items()}
    seen = set()
    real_plain = HA._plain_conv

    def spy(kind, dtype, *a):
        seen.add(dtype)
        return real_plain(kind, dtype, *a)
    monkeypatch.setattr(HA, '_plain_conv', spy)
    ours = _half_step(d, x, w, r)
    monkeypatch.setattr(HA, '_plain_conv', real_plain)
    assert ours.pop('dtype') == F16 and seen == {F16}, seen
    assert rel_l2(ours['logits'].cpu(), g['y']) < 2e-3
    d.load_state_dict(bn_state)
    _emulated(monkeypatch, F16)
    emu = _half_step(d, x, w, r)
    emu.pop('dtype')
    errs = {k: rel_l2(ours[k].cpu(), emu[k].cpu()) for k in emu}
    bad = {k: v for k, v in errs.items() if not v < (5e-4 if k == 'logits' else FP16_GRAD_TOL)}
    assert not bad, 'fp16 kernels vs emulation: %s\n(all: %s)' % (
        ', '.join(f'{k}={v:.2e}' for k, v in bad.items()), ', '.join(f'{k}={v:.1e}' for k, v in errs.items()))


def _config5(dev):
    from oracle import hyperseg_oracle as O
    from hyperseg_amd.training import BootstrappedCrossEntropyLoss
    x, s = O.synth_decoder_inputs('Sc', batch=2, seed=3, size=(576, 576))
    target = torch.randint(0, 12, (2, 576, 576), generator=G(5)).to(dev)
    return [t.to(dev) for t in x], s.to(dev), target, BootstrappedCrossEntropyLoss(k=4096, thresh=0.3, ignore_index=255)


@pytest.mark.gpu
def test_config5_fp16_training_step_with_grad_scaler(dev, monkeypatch):
    """BASELINE config 5 (CamVid-S decoder, 576x576, batch 2, BootstrappedCrossEntropyLoss(k=4096, thresh=0.3, ignore_index=255)) with
    PyTorch's standard AMP recipe: ``autocast()`` (fp16) + ``GradScaler``.
      * vs the fp32 step: loss within 1e-3 relative (observed 5e-7), gradients with cosine >= 0.99 (observed >= 0.9997; relative L2 up
        to 2.5e-2: the decoder's gradient moves by up to 8e-4 under ONE fp32 ulp, test_config5_full_workload_fp32);
      * vs the fp16 step with every storage-typed kernel emulated by the fp32 kernels + fp16 roundings: gradients within FP16_GRAD_TOL
        (observed <= 4.0e-3), loss 1e-3 (observed 1.5e-6);
      * the scaler settles: within five optimizer steps at least one is taken and the parameters move (no fp16 overflow in the forward
        on the synthetic weights)."""
    from oracle import hyperseg_oracle as O
    from test_hip_parity import build_decoder
    from hyperseg_amd.training import Adam
    x, s, target, crit = _config5(dev)

    def step(mode, scale):
        d = build_decoder('Sc', O).to(dev).train()
        sg = s.clone().requires_grad_(True)
        with torch.autocast('cuda', enabled=(mode != 'fp32')):
            pred = d(x, sg)
        loss = crit(pred, target)
        (loss * scale).backward()
        grads = {'d signal': sg.grad.double() / scale}
        grads.update({'d ' + k: p.grad.double() / scale for k, p in d.named_parameters() if p.grad is not None})
        return float(loss), grads, pred.dtype
    scaler = torch.amp.GradScaler('cuda')
    scale = float(scaler.get_scale())
    for _ in range(8):                                               # the scaler's own rule: halve until the scaled gradients are finite
        l16, g16, dt = step('fp16', scale)
        if all(bool(torch.isfinite(v).all()) for v in g16.values()):
            break
        scale /= 2
    assert dt == F16
    l32, g32, _ = step('fp32', 1.0)
    with monkeypatch.context() as mp:
        _emulated(mp, F16)
        lem, gem, _ = step('fp16-emulated', scale)
    cos = {k: float(torch.nn.functional.cosine_similarity(g16[k].flatten(), g32[k].flatten(), dim=0)) for k in g32}
    errs = {k: rel_l2(g16[k].cpu(), gem[k].cpu()) for k in gem}
    report = 'loss rel fp32 %.1e, vs emu %.1e; min cosine %.5f; emu rel L2 max %.1e; fp32 rel L2 max %.1e (scale %g)' % (
        abs(l16 - l32) / abs(l32), abs(l16 - lem) / abs(lem), min(cos.values()), max(errs.values()),
        max(rel_l2(g16[k].cpu(), g32[k].cpu()) for k in g32), scale)
    print(report)
    assert abs(l16 - l32) / abs(l32) < 1e-3 and abs(l16 - lem) / abs(lem) < 1e-3, report
    assert min(cos.values()) >= 0.99, (report, cos)
    bad = {k: v for k, v in errs.items() if not v < FP16_GRAD_TOL}
    assert not bad, 'fp16 kernels vs emulation: %s\n%s' % (', '.join(f'{k}={v:.2e}' for k, v in bad.items()), report)
    # the recipe itself settles
    d = build_decoder('Sc', O).to(dev).train()
    opt = Adam(d.parameters(), lr=1e-3, betas=(0.5, 0.999))
    scaler = torch.amp.GradScaler('cuda')
    before = [p.detach().clone() for p in d.parameters()]
    for _ in range(5):
        opt.zero_grad(set_to_none=True)
        with torch.autocast('cuda'):
            pred = d(x, s)
        loss = crit(pred, target)
        scaler.scale(loss).backward()
        scaler.step(opt)
        scaler.update()
    assert opt.steps_taken() >= 1, float(scaler.get_scale())
    assert any(not torch.equal(a, p.detach()) for a, p in zip(before, d.parameters()))
    assert all(bool(torch.isfinite(p).all()) for p in d.parameters())


def _no_host_sync(fn):
    """Runs ``fn`` and fails on a host synchronisation inside it: torch's sync debug mode where this build honours it, else the
    Python-level host reads (item / synchronize / bool / float / cpu / tolist) are made to raise."""
    t = torch.zeros(1, device='cuda')
    torch.cuda.set_sync_debug_mode('error')
    try:
        try:
            t.item()
            honoured = False
        except RuntimeError:
            honoured = True
        if honoured:
            return fn()
    finally:
        torch.cuda.set_sync_debug_mode('default')

    def boom(*a, **k):
        raise AssertionError('host synchronisation inside the optimizer step')
    saved = {n: getattr(torch.Tensor, n) for n in ('item', 'cpu', 'tolist', '__bool__', '__float__', '__int__')}
    sync = torch.cuda.synchronize
    try:
        for n in saved:
            setattr(torch.Tensor, n, boom)
        torch.cuda.synchronize = boom
        return fn()
    finally:
        for n, f in saved.items():
            setattr(torch.Tensor, n, f)
        torch.cuda.synchronize = sync


@pytest.mark.gpu
@pytest.mark.parametrize('kw', [dict(betas=(0.5, 0.999)), dict(betas=(0.9, 0.999), weight_decay=0.05, decoupled_weight_decay=True)],
                         ids=['config5', 'adamw'])
def test_adam_under_grad_scaler_equals_torch_fused_adam(dev, kw):
    """hyperseg_amd.training.Adam under a GradScaler (hs_adam_step_amp) against torch.optim.Adam / AdamW(fused=True) under its own scaler,
    8 steps on the awkward-size tensor list of test_adam_one_launch_equals_torch_adam (60 tensors: two launches): step 2 carries an inf in
    one gradient (both skip, both halve the scale, the step count stays), step 5 calls scaler.unscale_ first (grad_scale None).  Parameters
    and moments within 2e-6 of the scale, p.grad after the step equal to torch's, no host synchronisation inside scaler.step(ours)."""
    from hyperseg_amd.training import Adam
    sizes = [(1,), (3,), (1023,), (1024,), (1025,), (37, 53), (4216, 80)] + [(17 + i,) for i in range(53)]
    g = G(4103)
    p0 = [torch.randn(sz, generator=g) for sz in sizes]
    grads = [[torch.randn(sz, generator=g) * (0.1 + 0.3 * k) for sz in sizes] for k in range(8)]
    tkw = {k: v for k, v in kw.items() if k != 'decoupled_weight_decay'}
    ref_cls = torch.optim.AdamW if kw.get('decoupled_weight_decay') else torch.optim.Adam
    pa = [torch.nn.Parameter(t.clone().to(dev)) for t in p0]
    pb = [torch.nn.Parameter(t.clone().to(dev)) for t in p0]
    ours, ref = Adam(pa, lr=3e-3, **kw), ref_cls(pb, lr=3e-3, fused=True, **tkw)
    sa, sb = torch.amp.GradScaler('cuda', init_scale=2.0 ** 10), torch.amp.GradScaler('cuda', init_scale=2.0 ** 10)
    for k in range(8):
        sa.scale(torch.ones((), device=dev))                          # (what creates a scaler's scale tensor: its first scale() call)
        sb.scale(torch.ones((), device=dev))
        scale = float(sb.get_scale())
        assert float(sa.get_scale()) == scale
        for a, b_, gr in zip(pa, pb, grads[k]):
            gs = (gr * scale).to(dev)
            if k == 2 and a is pa[11]:
                gs[3] = float('inf')
            a.grad, b_.grad = gs.clone(), gs.clone()
        if k == 5:
            sa.unscale_(ours)
            sb.unscale_(ref)
        _no_host_sync(lambda: sa.step(ours))
        sb.step(ref)
        sa.update()
        sb.update()
        assert float(sa.get_scale()) == float(sb.get_scale()) == (scale / 2 if k == 2 else scale), k
        for i, (a, b_) in enumerate(zip(pa, pb)):
            assert rel_err(a.detach().cpu(), b_.detach().cpu()) < 2e-6, (k, i, sizes[i])
            assert torch.equal(a.grad, b_.grad), (k, i, 'p.grad')
        assert ours.steps_taken() == int(ref.state[pb[0]]['step']) == (k if k >= 2 else k + 1), k
    for i in (0, 6, 11, 59):
        st_a, st_b = ours.state[pa[i]], ref.state[pb[i]]
        assert rel_err(st_a['exp_avg'].cpu(), st_b['exp_avg'].cpu()) < 2e-6 and rel_err(st_a['exp_avg_sq'].cpu(), st_b['exp_avg_sq'].cpu()) < 2e-6


class _Autocast(torch.nn.Module):
    def __init__(self, d):
        super().__init__()
        self.d = d

    def forward(self, x, s):
        with torch.autocast('cuda'):
            return self.d(x, s)


@pytest.mark.gpu
@pytest.mark.parametrize('size', [96, 576], ids=['small', 'config5'])
def test_graphed_amp_train_step_equals_eager(dev, size):
    """GraphedTrainStep(..., scaler=GradScaler()) around an fp16-autocast decoder and hyperseg_amd.training.Adam: the whole AMP step (scaled
    backward, inf check, optimizer step, scale update) is one HIP graph.  Six replays equal six eager steps of a twin BIT FOR BIT -- loss,
    parameters, moments, BatchNorm buffers, scale and growth tracker after every step -- including a step forced to overflow (scale set
    to 2^40 between steps in both), which both skip."""
    import copy
    from oracle import hyperseg_oracle as O
    from test_hip_parity import build_decoder
    from hyperseg_amd.training import Adam, GraphedTrainStep, BootstrappedCrossEntropyLoss
    if size == 576:
        x, s, target, crit = _config5(dev)
    else:
        x, s = O.synth_decoder_inputs('Sc', batch=2, seed=9, size=(96, 96))
        x, s = [t.to(dev) for t in x], s.to(dev)
        target = torch.randint(0, 12, (2, 96, 96), generator=G(4102)).to(dev)
        crit = BootstrappedCrossEntropyLoss()
    d0 = build_decoder('Sc', O).to(dev).train()
    d1 = copy.deepcopy(d0)
    m0, m1 = _Autocast(d0), _Autocast(d1)
    o0 = Adam(d0.parameters(), lr=torch.tensor(2e-3, device=dev), betas=(0.5, 0.999))
    o1 = Adam(d1.parameters(), lr=torch.tensor(2e-3, device=dev), betas=(0.5, 0.999))
    s0, s1 = torch.amp.GradScaler('cuda'), torch.amp.GradScaler('cuda')
    step = GraphedTrainStep(m0, crit, o0, (x, s), target, warmup=1, scaler=s0)

    def eager():
        o1.zero_grad(set_to_none=True)
        loss = crit(m1(x, s), target)
        s1.scale(loss).backward()
        s1.step(o1)
        s1.update()
        return float(loss.detach())
    eager()                                                  # the twin of the warm-up step
    for k in range(6):
        if k == 3:
            s0._scale.fill_(2.0 ** 40)
            s1._scale.fill_(2.0 ** 40)
        lg = float(step.step()[0])
        le = eager()
        torch.cuda.synchronize()
        assert lg == le, (k, lg, le)
        assert torch.equal(s0._scale, s1._scale) and torch.equal(s0._growth_tracker, s1._growth_tracker), k
        if k == 3:
            assert float(s0.get_scale()) == 2.0 ** 39
    for (kk, a), (_, b_) in zip(d0.state_dict().items(), d1.state_dict().items()):
        assert torch.equal(a, b_), kk
    for a, b_ in zip(d0.parameters(), d1.parameters()):
        assert torch.equal(o0.state[a]['exp_avg'], o1.state[b_]['exp_avg']) and torch.equal(o0.state[a]['exp_avg_sq'], o1.state[b_]['exp_avg_sq'])
    assert o0.steps_taken() == o1.steps_taken() >= 4                 # (the warm-up step may be skipped too: the initial scale's overflow)
