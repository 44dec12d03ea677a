"""hs_gemm_split_se_fwd: the project GEMM of a late MBConv block deriving the block's squeeze-excite gate in its own workgroups
(csrc/hs_se_gate_phases.h, the SEG form of gemm_split_kernel) against the composed route it replaces, hs_se_gate_fwd (FUSED form) +
hs_gemm_split_fwd.  The phases sum every value in the order the gate's own kernel does, whichever number of waves runs them, so the
comparison is torch.equal throughout: outputs, the gate and the squeezed vector.  What the composed route itself is worth is held by
tests/test_hip_encoder_f64.py (the gate against float64) and tests/test_split_gemm.py (the GEMM per element); nothing is restated here."""
import functools

import pytest
import torch

import util_encoder_ref as R

gpu = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.fail('these tests need the MI355X (torch.cuda.is_available() is False)')
    return torch.device('cuda:0')


@functools.lru_cache(maxsize=None)
def _HF():
    from hyperseg_amd import functional
    return functional


# name -> (form, C, Csq, nblk, Cout, H, W)
CASES = {
    'vector partials, K % 32 != 0': ('ks1_w8', 240, 10, 8, 40, 8, 16),
    '1/16 block, NS = 1': ('ks2_w8', 480, 20, 2, 80, 16, 32),
    'KS = 3, scalar partials': ('ks3_w8', 672, 28, 2, 112, 16, 32),
    'KS = 3, one partial': ('ks3_w8', 672, 28, 1, 192, 8, 16),
    'all limits, ragged pixel block': ('ks3_w8', 768, 32, 2, 40, 6, 10),
    'units 2048, 4 waves': ('ks1_w4', 128, 6, 64, 24, 32, 64),
}
# (C, Csq, nblk, Cout, pixels, aligned) the route refuses, one reason each (units 2052 = 108 x 19 comes with K % 8 != 0; 256 x 9 is the units limit alone)
REFUSED = {
    'channels 772': (772, 28, 2, 40, 60, True),
    'csq 33': (240, 33, 8, 40, 128, True),
    'units 2052': (108, 4, 76, 24, 128, True),
    'units 2304': (256, 8, 36, 24, 128, True),
    'K % 8 != 0': (244, 10, 8, 40, 128, True),
    'odd N': (240, 10, 8, 40, 15, True),
    'misaligned partials': (240, 10, 8, 40, 128, False),
}
PARAMS = [(n, b, g) for n in CASES for b in (1, 2) for g in ('benign', 'pixel_sums')]


def test_routes_cover_the_cases_and_refuse_the_rest():
    HF = _HF()
    for name, (form, c, csq, nblk, cout, h, w) in CASES.items():
        assert HF.gemm_split_se_route(c, nblk, csq, cout, h * w) == form, name
        assert HF.se_gate_route(c, nblk, csq) == 'fused', name           # the composed route's gate is the FUSED form: the order shared
    for name, (c, csq, nblk, cout, p, aligned) in REFUSED.items():
        assert HF.gemm_split_se_route(c, nblk, csq, cout, p, aligned=aligned) is None, name
    assert HF.gemm_split_se_route(1288, 1, 8, 40, 128) is None          # K > 1280: no split GEMM at all
    assert HF.gemm_split_se_route(64, 4, 4, 24, 128) == 'ks1_w2'
    with pytest.raises(Exception):
        HF.gemm_split_se_route(0, 2, 8, 40, 128)


def _operands(dev, c, csq, nblk, cout, h, w, batch, gen, seed):
    HF = _HF()
    d = R.se_inputs(gen, batch, c, csq, nblk, cout, seed=seed)
    g = torch.Generator().manual_seed(seed + 1)
    wt = torch.randn(cout, c, generator=g) / c ** 0.5
    t = dict(partial=d['partial'], w1=d['w1'], b1=d['b1'], w2t=d['w2'].t().contiguous(), b2=d['b2'],
             x=torch.randn(batch, c, h, w, generator=g), shift=torch.randn(cout, generator=g) * 0.1,
             residual=torch.randn(batch, cout, h, w, generator=g))
    t = {k: v.to(dev) for k, v in t.items()}
    return HF.gemm_split_weights(wt.to(dev)), t, d['hw']


@gpu
@pytest.mark.parametrize('name,batch,gen', PARAMS)
def test_equals_the_composed_route(dev, name, batch, gen):
    from hyperseg_amd import _hip
    HF = _HF()
    form, c, csq, nblk, cout, h, w = CASES[name]
    sw, t, hw = _operands(dev, c, csq, nblk, cout, h, w, batch, gen, seed=c + csq + nblk)
    se = (t['partial'], hw, t['w1'], t['b1'], t['w2t'], t['b2'])
    # the composed route, and the gate's own launch once more through the raw entry for the squeezed vector
    gate = HF.se_gate(t['partial'], batch, hw, t['w1'], t['b1'], t['w2t'], t['b2'])
    sq_ref, gate_ref = torch.empty(batch, csq, device=dev), torch.empty(batch, c, device=dev)
    _hip.run.hs_se_gate_fwd(t['partial'].data_ptr(), batch, c, nblk, 1.0 / hw, t['w1'].data_ptr(), t['b1'].data_ptr(), csq, t['w2t'].data_ptr(),
                            t['b2'].data_ptr(), sq_ref.data_ptr(), gate_ref.data_ptr(), None, 0, None, None, _hip.stream_ptr())
    assert torch.equal(gate_ref, gate)
    tag = f'{name} / b{batch} / {gen}'
    gate_out, sq_out = torch.full((batch, c), -7.0, device=dev), torch.full((batch, csq), -7.0, device=dev)
    got = HF.gemm_split_se(sw, t['x'], *se, gate_out=gate_out, squeezed_out=sq_out)
    assert torch.equal(sq_out, sq_ref), f'{tag}: squeezed'
    assert torch.equal(gate_out, gate), f'{tag}: gate'
    assert torch.equal(got, HF.gemm_split(sw, t['x'], gate=gate)), f'{tag}: plain'
    assert got.abs().sum() > 0 and torch.isfinite(got).all()
    # shift + activation, a separate residual, accumulation onto the residual itself
    got = HF.gemm_split_se(sw, t['x'], *se, shift=t['shift'], act=HF.ACT_RELU)
    assert torch.equal(got, HF.gemm_split(sw, t['x'], gate=gate, shift=t['shift'], act=HF.ACT_RELU)), f'{tag}: shift + relu'
    got = HF.gemm_split_se(sw, t['x'], *se, shift=t['shift'], residual=t['residual'])
    assert torch.equal(got, HF.gemm_split(sw, t['x'], gate=gate, shift=t['shift'], residual=t['residual'])), f'{tag}: shift + residual'
    acc, acc_ref = t['residual'].clone(), t['residual'].clone()
    assert HF.gemm_split_se(sw, t['x'], *se, residual=acc, out=acc) is acc
    HF.gemm_split(sw, t['x'], gate=gate, residual=acc_ref, out=acc_ref)
    assert torch.equal(acc, acc_ref), f'{tag}: in-place accumulation'
    assert not torch.equal(acc, t['residual'])


@gpu
@pytest.mark.parametrize('name', list(REFUSED))
def test_refused_shapes_raise_before_any_launch(dev, name):
    from hyperseg_amd import _hip
    HF = _HF()
    c, csq, nblk, cout, p, aligned = REFUSED[name]
    h, w = (3, 5) if p == 15 else ((6, 10) if p == 60 else (8, 16))
    sw, t, hw = _operands(dev, c, csq, nblk, cout, h, w, 1, 'benign', seed=5)
    partial = t['partial']
    if not aligned:                                         # the same values 4 bytes off a 16-byte boundary
        partial = torch.empty(partial.numel() + 1, device=dev)[1:].view_as(partial).copy_(partial)
        assert partial.data_ptr() % 16 == 4 and partial.is_contiguous()
    out = torch.full((1, cout, h, w), -7.0, device=dev)
    with pytest.raises(_hip.HipLibraryError, match='hs_gemm_split_se_fwd'):
        HF.gemm_split_se(sw, t['x'], partial, hw, t['w1'], t['b1'], t['w2t'], t['b2'], out=out)
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())


def test_argument_checks():
    HF = _HF()
    sw = HF.SplitWeights(None, None, 40, 240, 256)
    x = torch.zeros(1, 240, 4, 4)
    ok = dict(partial=torch.zeros(240, 2), hw=16.0, w_reduce=torch.zeros(10, 240), b_reduce=torch.zeros(10), w_expand_t=torch.zeros(10, 240),
              b_expand=torch.zeros(240))
    for bad in (dict(partial=torch.zeros(239, 2)), dict(w_reduce=torch.zeros(10, 239)), dict(b_reduce=torch.zeros(9)),
                dict(w_expand_t=torch.zeros(240, 10)), dict(b_expand=torch.zeros(10)), dict(shift=torch.zeros(39)),
                dict(residual=torch.zeros(1, 40, 4, 5)), dict(out=torch.zeros(1, 41, 4, 4)), dict(gate_out=torch.zeros(1, 10)),
                dict(squeezed_out=torch.zeros(1, 240))):
        with pytest.raises(ValueError):
            HF.gemm_split_se(sw, x, **{**ok, **bad})
    with pytest.raises(ValueError):
        HF.gemm_split_se(sw, torch.zeros(1, 200, 4, 4), **ok)


# -------------------------------------------------------------------------------------------------------------------- model

@functools.lru_cache(maxsize=None)
def _prepared(where):
    from hyperseg_amd import configs
    from hyperseg_amd.utils.inference import prepare_for_inference
    from hyperseg_amd.utils.synthetic import fill_by_name
    m = fill_by_name(configs.build('hyperseg-m').eval(), seed=7)
    prepare_for_inference(m, fold_bn=False, fused_depthwise=True, split_gemm=True)
    return m


@gpu
@pytest.mark.parametrize('batch', [1, 2])
def test_backbone_features_equal_with_the_switch_off_and_replay_equals_eager(dev, monkeypatch, batch):
    from hyperseg_amd.utils import inference
    HF = _HF()
    m = _prepared('gpu').to(dev)
    x = torch.rand(batch, 3, 128, 192, generator=torch.Generator().manual_seed(1003)).to(dev)
    taken = {'n': 0}
    real = HF.gemm_split_se

    def counting(*a, **k):
        taken['n'] += 1
        return real(*a, **k)
    monkeypatch.setattr(HF, 'gemm_split_se', counting)
    with torch.no_grad():
        monkeypatch.setattr(inference, 'HS_GEMM_SE', False)
        off = [f.clone() for f in m.backbone(x)]
        assert taken['n'] == 0
        monkeypatch.setattr(inference, 'HS_GEMM_SE', True)
        on = [f.clone() for f in m.backbone(x)]
        assert taken['n'] >= 1, 'no block took the new route at this size'
        assert len(on) == len(off) and all(torch.equal(a, b) for a, b in zip(on, off))
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            m.backbone(x)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            captured = m.backbone(x)
        for _ in range(2):
            graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(captured, on))


def test_cpu_tensors_never_reach_the_new_route(monkeypatch):
    """FusedMBConv.forward on CPU tensors (the stand-in walk of tests/test_model_boundary.py) makes the calls it always made: neither
    the new launch nor its route query is reached, whatever the switch says."""
    import torch.nn.functional as F
    from hyperseg_amd.utils import inference
    HF = _HF()

    def act_of(t, act):
        return t * torch.sigmoid(t) if act == 3 else (torch.relu(t) if act == 1 else (t.clamp(0, 6) if act == 2 else t))

    def dw(x, weight, stride, pad_top, pad_left, out_size, scale=None, shift=None, act=0, pool=False, in_scale=None, in_shift=None, se=None):
        if in_scale is not None:
            x = act_of(x * in_scale.view(1, -1, 1, 1) + in_shift.view(1, -1, 1, 1), 3)
        k, (ho, wo) = weight.shape[-1], out_size
        pb, pr = (ho - 1) * stride + k - x.shape[2] - pad_top, (wo - 1) * stride + k - x.shape[3] - pad_left
        y = F.conv2d(F.pad(x, (pad_left, pr, pad_top, pb)), weight, stride=stride, groups=x.shape[1])
        y = act_of(y * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1), act)
        return (y, y.sum((2, 3)).view(-1, 1)) + ((False,) if se is not None else ())

    def pointwise(x, weight, gate=None, scale=None, shift=None, act=0, residual=None):
        y = F.conv2d(x if gate is None else x * gate[:, :, None, None], weight)
        y = act_of(y * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1), act)
        return y if residual is None else y + residual

    def expand_dw(x, w_expand, scale0, shift0, w_dw, stride, pad_top, pad_left, out_size, scale1, shift1, pool=True, se=None):
        hmid = pointwise(x, w_expand.view(w_expand.shape[0], -1, 1, 1), None, scale0, shift0, 3)
        return dw(hmid, w_dw, stride, pad_top, pad_left, out_size, scale1, shift1, act=3, pool=True, se=se)

    def se_gate(partial, batch, hw, w_reduce, b_reduce, w_expand_t, b_expand, w_proj=None, out_scale=None):
        z = act_of((partial.sum(1).view(batch, -1) / hw) @ w_reduce.flatten(1).t() + b_reduce, 3)
        gate = torch.sigmoid(z @ w_expand_t + b_expand)
        if w_proj is None:
            return gate
        ws = w_proj.flatten(1)[None] * gate[:, None, :]
        return (ws if out_scale is None else ws * out_scale[None, :, None])[..., None, None]

    def affine(x, scale, shift, act=0, residual=None):
        y = act_of((x if scale is None else x * scale.view(1, -1, 1, 1)) + shift.view(1, -1, 1, 1), act)
        return x.copy_(y if residual is None else y + residual)

    calls = {'gated': 0}

    def gemm_split(sw, x, gate=None, shift=None, act=0, residual=None, out=None):
        calls['gated'] += gate is not None
        y = x.new_zeros(x.shape[0], sw.c_out, *x.shape[2:])
        return y if out is None else out

    def refuse(*a, **k):
        raise AssertionError('the one-launch route was reached with CPU tensors')
    for name, fn in (('depthwise_conv_bn_act', dw), ('mbconv_expand_dw', expand_dw), ('se_gate', se_gate), ('gemm_split', gemm_split),
                     ('pointwise_conv', pointwise), ('affine_act_', affine), ('gemm_split_se', refuse), ('gemm_split_se_route', refuse)):
        monkeypatch.setattr(HF, name, fn)
    monkeypatch.setattr(inference, 'HS_GEMM_SE', True)
    bb = _prepared('cpu').backbone
    with torch.no_grad():
        t = F.silu(bb._bn0(bb._conv_stem(torch.rand(1, 3, 64, 96, generator=torch.Generator().manual_seed(3)))))
        for blk in bb._blocks:
            t = blk._fused_dw(t, blk)
    assert calls['gated'] > 10
