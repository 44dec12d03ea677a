"""hs_gemm_split_fwd (the encoder's 1x1 convolutions on the f16 matrix cores, include/hyperseg_hip.h).  The host side (weight
split, fragment order, plan) is checked on the CPU; the GPU tests run under plain ``-m gpu`` since round 3 (first GPU visit r5a:
16 passed; bench.py 1091 -> 1179 frames/s with the route on, profiles/round3_first_visit.txt)."""
import pytest
import torch

from conftest import G, rel_err
from util_split_ref import emulate

def test_split_weights_host_side():
    from hyperseg_amd import functional as HF
    from hyperseg_amd._hip import lib
    # plan: Cin rounded up to (2 | 4 | 8 waves) x (<= 5 k-steps) x 32; beyond 1280 the kernel declines
    assert [lib.hs_gemm_split_kp(k) for k in (1, 32, 80, 112, 192, 240, 480, 672, 1152, 1280)] == \
        [64, 64, 128, 128, 256, 256, 512, 768, 1280, 1280]
    # 1281 ... 2560: two chunks of <= 5 k-steps per wave -- the windowed 2x2 / stride-2 form only (hs_gemm_split_fwd declines)
    assert [lib.hs_gemm_split_kp(k) for k in (1281, 1600, 1920, 2560)] == [1536, 2048, 2048, 2560]
    assert lib.hs_gemm_split_kp(2561) < 0 and lib.hs_gemm_split_kp(0) < 0
    g = torch.Generator().manual_seed(0)
    for m, k in ((40, 240), (19, 80), (112, 672)):
        w = torch.randn(m, k, 1, 1, generator=g) * torch.logspace(-3, 3, m).view(m, 1, 1, 1)      # rows of very different size
        scale = torch.rand(m, generator=g) + 0.5
        sw = HF.gemm_split_weights(w, scale)
        assert (sw.c_out, sw.c_in, sw.kp) == (m, k, lib.hs_gemm_split_kp(k))
        rt, kst = -(-m // 16), sw.kp // 32
        assert tuple(sw.frag.shape) == (rt, kst, 2, 4, 16, 8) and sw.frag.dtype == torch.float16 and sw.inv.numel() == 16 * rt
        # back from fragment order: lane = row % 16 + 16 * kgroup holds w[16 R + row % 16][32 S + 8 kgroup + j]
        back = sw.frag.permute(2, 0, 4, 1, 3, 5).reshape(2, 16 * rt, sw.kp).float()
        ref = (w.flatten(1) * scale[:, None])
        rebuilt = (back[0].double() + back[1].double()) * sw.inv.double()[:, None]
        assert float(back[:, m:].abs().max() if 16 * rt > m else 0.0) == 0.0 and float(back[:, :, k:].abs().max()) == 0.0
        err = (rebuilt[:m, :k] - ref.double()).abs().amax(1) / ref.abs().amax(1).double()
        assert float(err.max()) < 2.0 ** -21                     # two f16 pieces of a row scaled to < 2^15
        assert float((back[0].abs().amax(1)[:m]).max()) < 2.0 ** 15
    assert HF.gemm_split_weights(torch.randn(8, 1920, generator=G(1034))) is None
    sw4 = HF.gemm_split_weights(torch.randn(8, 480, 2, 2, generator=G(1035)), max_k=2560)
    assert (sw4.c_in, sw4.kp) == (1920, 2048) and HF.gemm_split_weights(torch.randn(8, 641, 2, 2, generator=G(1036)), max_k=2560) is None
    with pytest.raises(Exception):
        HF.gemm_split(HF.gemm_split_weights(torch.randn(8, 64, generator=G(1037))), torch.rand(1, 64, 4, 4, generator=G(1038)))       # CPU tensors: no fallback


@pytest.mark.parametrize('m,k', [(40, 240), (112, 672), (192, 1152), (480, 80)])
def test_split_arithmetic_emulated(m, k):
    """The kernel's arithmetic restated with torch on the CPU from the REAL weight preparation: per wave K slice, the gated
    input column of every pixel is scaled by a power of two to < 2^15 and split into two f16 pieces; three f16 x f16 products
    (exact in f32) accumulate; column and row scales are undone at the end.  Against the float64 product the result must be at
    least as close as a plain f32 matmul (the claim DESIGN section 7.2 makes; the GPU probe measured 1.6-2.9e-7)."""
    from hyperseg_amd import functional as HF
    g = torch.Generator().manual_seed(m * k)
    n = 96
    w = torch.randn(m, k, generator=g) / k ** 0.5
    x = torch.randn(k, n, generator=g) * torch.rand(k, 1, generator=g) * 4
    gate = torch.rand(k, generator=g)
    sw = HF.gemm_split_weights(w)
    y = emulate(sw, x, gate)                                  # util_split_ref: the whole kernel, step by step
    ref = w.double() @ (x.double() * gate.double()[:, None])
    err_split = float((y.double() - ref).abs().max() / ref.abs().max())
    err_f32 = float(((w @ (x * gate[:, None])).double() - ref).abs().max() / ref.abs().max())
    assert err_split < 5e-7 and err_split < 2 * err_f32 + 1e-7


@pytest.mark.gpu
@pytest.mark.parametrize('m,k,hw,batch', [(40, 240, (64, 128), 1), (80, 480, (32, 64), 2), (112, 672, (32, 64), 1), (192, 1152, (16, 32), 1),
                                          (320, 1152, (16, 32), 2), (480, 80, (32, 64), 1), (19, 33, (5, 7), 1), (1280, 320, (16, 32), 1),
                                          (40, 36, (33, 129), 1),      # odd pixel count on a wide grid: the scalar-load form, 32-pixel blocks
                                          # round 6: 1280 < K <= 2560 on the two-chunk form (HyperSeg-M's last project conv: K = 1920)
                                          (320, 1920, (16, 32), 1), (320, 1920, (16, 32), 2), (100, 1400, (8, 16), 1), (64, 2560, (8, 8), 1)])
def test_gemm_split_vs_float64(m, k, hw, batch):
    from hyperseg_amd import functional as HF
    dev = torch.device('cuda:0')
    g = torch.Generator().manual_seed(m + k)
    w = (torch.randn(m, k, generator=g) / k ** 0.5).to(dev)
    x = (torch.randn(batch, k, *hw, generator=g) * torch.rand(1, k, 1, 1, generator=g) * 4).to(dev)
    gate = torch.rand(batch, k, generator=g).to(dev)
    scale = (torch.rand(m, generator=g) + 0.5).to(dev)
    sw = HF.gemm_split_weights(w, scale, max_k=2560)
    ref = torch.einsum('ok,bkn->bon', (w * scale[:, None]).double(), (x.flatten(2) * gate[:, :, None]).double()).view(batch, m, *hw)
    y = HF.gemm_split(sw, x, gate=gate)
    assert rel_err(y.double().cpu(), ref.cpu()) < 2e-6
    y0 = HF.gemm_split(HF.gemm_split_weights(w, max_k=2560), x)
    ref0 = torch.einsum('ok,bkn->bon', w.double(), x.flatten(2).double()).view(batch, m, *hw)
    assert rel_err(y0.double().cpu(), ref0.cpu()) < 2e-6
    acc = torch.ones_like(y)
    assert HF.gemm_split(sw, x, gate=gate, residual=acc, out=acc) is acc                   # in place onto a skip tensor
    assert rel_err(acc.double().cpu(), (ref + 1).cpu()) < 2e-6
    shift = torch.randn(m, generator=g).to(dev)
    res = torch.randn(batch, m, *hw, generator=g).to(dev)
    for act, fn in ((0, lambda t: t), (1, torch.relu), (2, lambda t: t.clamp(0, 6)), (3, lambda t: t * torch.sigmoid(t))):
        ya = HF.gemm_split(sw, x, gate=gate, shift=shift, act=act, residual=res)
        want = fn(ref + shift.double().view(1, -1, 1, 1)) + res.double()
        assert rel_err(ya.double().cpu(), want.cpu()) < (2e-5 if act == 3 else 2e-6)       # swish: the fast exp2 / rcp form


@pytest.mark.gpu
@pytest.mark.parametrize('m,c,hw,batch', [(640, 640, (16, 32), 1), (96, 64, (8, 8), 2), (130, 250, (6, 12), 1), (320, 320, (32, 64), 1),
                                          (48, 400, (4, 4), 1)])
def test_gemm_split_conv2x2_vs_float64(m, c, hw, batch):
    """Conv2d(c, m, kernel 2, stride 2) + shift + ReLU with the window read on load (the context head's down blocks,
    hyperseg_v1_0.py:396-401; K = 4 c up to 2560 in two chunks per wave) against the float64 convolution."""
    import torch.nn.functional as F
    from hyperseg_amd import functional as HF
    dev = torch.device('cuda:0')
    g = torch.Generator().manual_seed(m + c)
    w = (torch.randn(m, c, 2, 2, generator=g) / (4 * c) ** 0.5).to(dev)
    x = (torch.randn(batch, c, *hw, generator=g) * torch.rand(1, c, 1, 1, generator=g) * 4).to(dev)
    scale = (torch.rand(m, generator=g) + 0.5).to(dev)
    shift = torch.randn(m, generator=g).to(dev)
    sw = HF.gemm_split_weights(w, scale, max_k=2560)
    assert sw is not None and sw.c_in == 4 * c
    ref = F.conv2d(x.double(), (w * scale.view(-1, 1, 1, 1)).double(), stride=2)
    y = HF.gemm_split_conv2x2(sw, x)
    assert y.shape == ref.shape and rel_err(y.double().cpu(), ref.cpu()) < 2e-6
    ya = HF.gemm_split_conv2x2(sw, x, shift=shift, act=HF.ACT_RELU)
    assert rel_err(ya.double().cpu(), torch.relu(ref + shift.double().view(1, -1, 1, 1)).cpu()) < 2e-6
    assert HF.gemm_split_weights(w, scale) is None or 4 * c <= 1280             # the 1x1 form stops at K = 1280
    # the global average of the result rides along as sums over blocks of 16 pixels; folded into a shift by hs_pooled_shift_fwd
    if batch == 1:
        p = (hw[0] // 2) * (hw[1] // 2)
        part = torch.full((1, m, -(-p // 16)), float('nan'), device=dev)
        yp = HF.gemm_split_conv2x2(sw, x, shift=shift, act=HF.ACT_RELU, pool_partial=part)
        assert torch.equal(yp, ya)
        mean = yp.double().mean((2, 3)).view(m)
        assert rel_err(part.double().sum(2).view(m).cpu() / p, mean.cpu()) < 1e-6
        wb = torch.randn(24, m, generator=g).to(dev)
        base = torch.randn(24, generator=g).to(dev)
        got = HF.pooled_shift(part, p, wb, base)
        assert rel_err(got.double().cpu(), (base.double() + wb.double() @ mean).cpu()) < 1e-6
    with pytest.raises(ValueError):
        HF.gemm_split_conv2x2(sw, x[:, :, :, :hw[1] - 2].contiguous())          # width must be a multiple of 4


@pytest.mark.gpu
@pytest.mark.parametrize('m,k,hw,batch', [(640, 640, (8, 16), 1), (40, 96, (5, 6), 2), (320, 1152, (16, 32), 1)])
def test_gemm_split_up2_vs_float64(m, k, hw, batch):
    """1x1 conv + shift + ReLU stored nearest-2x upsampled (hs_gemm_split_up2_fwd), into a channel slice of a larger tensor."""
    import torch.nn.functional as F
    from hyperseg_amd import functional as HF
    dev = torch.device('cuda:0')
    g = torch.Generator().manual_seed(m * k)
    w = (torch.randn(m, k, generator=g) / k ** 0.5).to(dev)
    x = torch.randn(batch, k, *hw, generator=g).to(dev)
    shift = torch.randn(m, generator=g).to(dev)
    sw = HF.gemm_split_weights(w)
    ref = F.interpolate(torch.relu(torch.einsum('ok,bkn->bon', w.double(), x.flatten(2).double()).view(batch, m, *hw)
                                   + shift.double().view(1, -1, 1, 1)), scale_factor=2, mode='nearest')
    y = HF.gemm_split_up2(sw, x, shift=shift, act=HF.ACT_RELU)
    assert y.shape == ref.shape and rel_err(y.double().cpu(), ref.cpu()) < 2e-6
    if batch == 1:
        big = torch.zeros(1, m + 8, 2 * hw[0], 2 * hw[1], device=dev)
        HF.gemm_split_up2(sw, x, shift=shift, act=HF.ACT_RELU, out=big[:, 8:])
        assert torch.equal(big[:, 8:], y) and float(big[:, :8].abs().max()) == 0.0


@pytest.mark.gpu
@pytest.mark.parametrize('batch,size', [(1, (256, 512)), (2, (256, 256)), (1, (512, 1024))])
def test_prepared_model_with_split_gemm(batch, size):
    import copy
    from hyperseg_amd import configs
    from hyperseg_amd.utils.inference import prepare_for_inference
    from hyperseg_amd.utils.synthetic import fill_by_name
    dev = torch.device('cuda:0')
    stock = fill_by_name(configs.build('hyperseg-m').eval(), seed=9)
    fused = copy.deepcopy(stock)
    prepare_for_inference(fused, fold_bn=False, fused_depthwise=True, split_gemm=True)
    stock, fused = stock.to(dev), fused.to(dev)
    x = torch.rand(batch, 3, *size, generator=G(1039)).to(dev)
    with torch.no_grad():
        for a, b in zip(stock.backbone(x), fused.backbone(x)):
            assert rel_err(b.cpu(), a.cpu()) < 5e-5
        ys = stock(x).cpu()
        assert rel_err(fused(x).cpu(), ys) < 1e-4
        assert rel_err(fused(x).cpu(), ys) < 1e-4          # twice: the in-place skip accumulation


# ============================================================================================================================
# Per-element and range tests (util_split_ref.py: the emulation, the derived bound, the tier-2 reference level)
#
# Case -> instance of gemm_split_kernel<KS, NWV, FAST, NS, MT, NCH, PATCH>, from launch_gemm_split_plain / hs_gemm_split_conv2x2_fwd
# by hand.  B = 1 everywhere, so wgs = ceil(N / 32) * ceil(ceil(M / 16) / 2):
#   grid form   (M, N)                      wgs    narrow (wgs <= 128, N > 16)   tall (wgs >= 257, M > 32)   <NS, MT>
#   narrow      (19, 35 | 36)               2*1    yes                           -                           <1, 2>
#   normal      (19, 13 | 14)               1*1    no (N <= 16)                  no                          <2, 2>
#   normal      (64, 2080)                  65*2   no (130)                      no                          <2, 2>
#   tall        (48, 4128)                  129*2  no                            yes (258; grid.y = 1: row   <2, 4>
#                                                                                tile 3 is the clamped one)
#   FAST = K % 8 == 0 and N even: the odd N (35, 13) and every K of the left column below are FAST = false, the even N (36, 14,
#   2080, 4128) with the right column FAST = true.
#   K depth     K (not FAST | FAST)    steps = ceil(K / 32)     <KS, NWV>
#   nwv 2       33 | 64                2                        <1, 2>
#   nwv 4       100 | 128              4                        <1, 4>
#   ks 1        250 | 256              8                        <1, 8>
#   ks 2        500 | 512              16                       <2, 8>
#   ks 3        700 | 768              22 -> 24 | 24            <3, 8>
#   ks 4        1001 | 1024            32                       <4, 8>
#   ks 5        1270 | 1280            40                       <5, 8>
#   => test_split_matrix[form-K] reaches <KS, NWV, FAST, NS, MT, 1, false> for all 7 x 2 x 3 = 42 plain instances.
#   two-chunk   K = 1400 | 1920 | 2560 (steps 44 | 60 | 80, per wave 6 | 8 | 10 -> two chunks of 3 | 4 | 5), N = 24 | 128, M = 33:
#               test_split_two_chunk -> <3 | 4 | 5, 8, true, 1, 2, 2, false>   (always the 16-pixel grid)
#   window      c = 34 | 100 | 160 | 224 | 288 | 320 (K = 4 c: steps 5 | 13 | 20 | 28 | 36 | 40 -> KS 1 | 2 | 3 | 4 | 5 | 5, one chunk),
#               c = 384 | 480 | 640 (steps 48 | 60 | 80 -> two chunks of 3 | 4 | 5); maps 2x4, 6x12, 8x8 (N = 2, 18, 16), M = 33:
#               test_split_window -> <KS, 8, true, 1, 2, NCH, true>, the 8 window instances
#   nearest-2x  test_split_up2[narrow | normal | tall] -> the FAST = false / true / true plain instance of that form at K = 100 / 128 / 256
#               with up2_wo > 0 (the same kernels; the store branch differs)
# 42 + 3 + 8 = 53 launched instances.
# ============================================================================================================================
import functools
import json
import os

import util_split_ref as S

FORMS = {'narrow': (19, 35, 36), 'normal': (19, 13, 14), 'tall': (48, 4128, 4128)}
DEPTHS = (33, 64, 100, 128, 250, 256, 500, 512, 700, 768, 1001, 1024, 1270, 1280)
RANGE = S.GENERATORS[:5]
PERIOD = 67                 # wide cases repeat PERIOD distinct pixel columns (a column's result depends on that column alone): the
                            # emulation and the float64 product run on the distinct ones, the kernel on all N
REPORT = {}                 # plan -> figures for profiles/split_gemm_bound.txt (written where HS_SPLIT_GEMM_REPORT names a file)


@pytest.fixture(scope='module', autouse=True)
def _split_report():
    yield
    path = os.environ.get('HS_SPLIT_GEMM_REPORT')
    if path and REPORT:
        with open(path, 'w') as f:
            json.dump(REPORT, f, indent=1, sort_keys=True)


def _note(plan, patch, **kw):
    r = REPORT.setdefault(f'nwv{plan.nwv}_ks{plan.ks}_nch{plan.nch}' + ('_window' if patch else ''), {})
    for k, v in kw.items():
        r[k] = max(r.get(k, 0.0), float(v))


@functools.lru_cache(maxsize=None)
def _case(name, m, k, n, seed, patch=False, gated=True):
    """One set of inputs with everything the CPU can say about it, computed once and shared: the float64 product, the bound, the
    in-range mask, the emulation in its nominal order and the tier-2 reference level (the largest q over 32 summation orders)."""
    from hyperseg_amd import functional as HF
    nu = min(n, PERIOD)
    w, x, gate = S.make_inputs(name, m, k, nu, seed, gated=gated and not patch)
    sw = HF.gemm_split_weights(w.view(m, k // 4, 2, 2) if patch else w, max_k=2560)
    assert sw is not None and sw.c_in == k
    xin = S.window_image(x, *_PATCH_HW[nu]) if patch else x
    plan = S.plan_of(k)
    ref = w.double() @ (x.double() if gate is None else x.double() * gate.double()[:, None])
    bound = S.split_bound(sw, xin, gate, plan, patch)
    ok = S.in_range(sw, xin, gate, patch)
    perms, rev = S.orders(plan)
    emu = S.emulate(sw, xin, gate, patch=patch, perms=perms, reverse_waves=rev)
    quiet = S.quiet(sw, xin, gate, patch)
    level = tuple(S.q_of(emu, ref, sw, xin, gate, patch, where=ok & cls)[0] for cls in (~quiet, quiet))       # (loud, quiet) elements
    return dict(name=name, m=m, k=k, n=n, nu=nu, w=w, x=xin, gate=gate, sw=sw, plan=plan, patch=patch, ref=ref, bound=bound, ok=ok,
                emu=emu, level=level, quiet=quiet)


_PATCH_HW = {2: (1, 2), 18: (3, 6), 16: (4, 4)}       # output maps of the 2x4, 6x12 and 8x8 inputs


def _check_emulation(c, what):
    """The emulation inside the bound and inside the tier-2 level for every order; the level sharper than tier 1."""
    worst = max(S.assert_split(e, c['ref'], c['bound'], f'{what} order {i}', where=c['ok']) for i, e in enumerate(c['emu']))
    assert torch.equal(torch.isfinite(c['ref'])[c['ok']], torch.ones_like(c['ok'])[c['ok']])
    exact = S.emulate(c['sw'], c['x'], c['gate'], patch=c['patch'], steps='f64')
    p = c['plan']
    for cls, level, tag in ((~c['quiet'], c['level'][0], 'loud'), (c['quiet'], c['level'][1], 'quiet')):
        q64, _ = S.q_of(exact, c['ref'], c['sw'], c['x'], c['gate'], c['patch'], where=c['ok'] & cls)
        assert q64 <= level * S.MARGIN, (what, tag, q64, level)                             # exact accumulation is inside the level
    # loud elements: representation terms + the (small) floor only; and the level is sharper than tier 1's accumulation term
    q64, _ = S.q_of(exact, c['ref'], c['sw'], c['x'], c['gate'], c['patch'], where=c['ok'] & ~c['quiet'])
    assert q64 <= 3 * 2.0 ** -22 * (1 + 2.0 ** -10) + 2.0 ** -23, (what, q64)
    assert c['level'][0] * S.MARGIN < (96 * p.ks * p.nch + p.nwv + 2) * 2.0 ** -23, (what, c['level'])
    _note(p, c['patch'], level_loud=c['level'][0], level_quiet=c['level'][1], emu_ratio=worst)
    return worst


CPU_PLANS = [(k, False) for k in DEPTHS + (1400, 1920, 2560)] + [(4 * c, True) for c in (34, 100, 160, 224, 288, 320, 384, 480, 640)]


@pytest.mark.parametrize('k,patch', CPU_PLANS)
def test_split_emulation_inside_bound(k, patch):
    """Every plan of the GPU matrix x every range generator, on the CPU: keeps the bound and the level honest before a GPU sees them."""
    for i, name in enumerate(S.GENERATORS):
        m, n = (33, 18) if patch else (19, 35)
        c = _case(name, m, k, n, 7000 + k + i, patch)
        _check_emulation(c, f'{name} K={k}')
        assert int(c['ok'].sum()) >= c['ok'].numel() // 3                  # the range mask leaves most of every case in


def _caught(c, defect):
    got = S.emulate(c['sw'], c['x'], c['gate'], patch=c['patch'], defect=defect)
    try:
        S.assert_split(got, c['ref'], c['bound'], defect, where=c['ok'])
    except AssertionError:
        return 'tier 1'
    for cls, level in ((~c['quiet'], c['level'][0]), (c['quiet'], c['level'][1])):
        if S.q_of(got, c['ref'], c['sw'], c['x'], c['gate'], c['patch'], where=c['ok'] & cls)[0] > S.MARGIN * level:
            return 'tier 2'
    return None


@pytest.mark.parametrize('defect', S.DEFECTS)
def test_split_bound_has_teeth(defect):
    """A kernel with ``defect`` (restated in the emulation only) fails tier 1 or tier 2 on at least one range input."""
    hits = {}
    for k in (100, 700, 1400):
        for i, name in enumerate(S.GENERATORS):
            how = _caught(_case(name, 19, k, 35, 7000 + k + i), defect)
            if how:
                hits[(k, name)] = how
    print(defect, hits)
    assert hits, f'{defect} passes every range input: the inputs are too tame'
    if defect == 'drop_cross':          # a precision-class defect: tier 2 has to see it on EVERY input where the cross term exists
        assert all((k, 'benign') in hits for k in (100, 700, 1400)), hits


def test_split_weights_extreme_rows():
    """Host weight preparation on an all-zero row, a single-nonzero row and row maxima at 2^-110 and 2^125: pieces and inverse scales
    finite, the rebuilt row within 2^-21 of the row maximum."""
    from hyperseg_amd import functional as HF
    k = 100
    w = torch.randn(5, k, generator=G(7100))
    w[0] = 0
    w[1] = 0
    w[1, 17] = -3.0
    w[2] = w[2] / w[2].abs().max() * 2.0 ** -110
    w[3] = w[3] / w[3].abs().max() * 2.0 ** 125
    sw = HF.gemm_split_weights(w)
    assert bool(torch.isfinite(sw.frag.float()).all()) and bool(torch.isfinite(sw.inv).all()) and bool((sw.inv > 0).all())
    back = sw.frag.permute(2, 0, 4, 1, 3, 5).reshape(2, 16, sw.kp).double()
    rebuilt = ((back[0] + back[1]) * sw.inv.double()[:, None])[:5, :k]
    err = (rebuilt - w.double()).abs().amax(1)
    assert float(back[0].abs().max()) < 2.0 ** 15
    assert torch.equal(rebuilt[0], torch.zeros(k, dtype=torch.float64)) and torch.equal(rebuilt[1], w[1].double())
    for r in (2, 3, 4):                                                     # row 2 sits below the row clamp: scaled to 2^4 only, lo still normal
        assert float(err[r]) < 2.0 ** -21 * float(w[r].abs().max())


# ---------------------------------------------------------------------------------------------------------------- GPU side

SENTINEL = 0x7fc5a5a5       # a NaN payload no arithmetic produces
GUARD = 62                  # elements on either side (8-byte aligned for the nearest-2x form's paired stores, not 16)


def _guarded(numel, dev):
    buf = torch.full((GUARD + numel + GUARD,), SENTINEL, dtype=torch.int32, device=dev)
    return buf, buf.view(torch.float32)[GUARD:GUARD + numel]


def _guards_intact(buf, numel):
    b = buf.cpu()
    return bool((b[:GUARD] == SENTINEL).all()) and bool((b[GUARD + numel:] == SENTINEL).all())


def _widen(c, t):
    """A per-distinct-column (.., nu) CPU tensor -> all N columns."""
    return t if c['n'] == c['nu'] else t[..., torch.arange(c['n']) % c['nu']]


def _run(c, dev, x=None, **kw):
    """The kernel on case ``c`` (or on ``x`` in its place) into a guarded buffer: (y (M, N) on the CPU, guards intact)."""
    from hyperseg_amd import functional as HF
    m, n = c['m'], c['n']
    sw = c.setdefault('sw_dev', HF.SplitWeights(c['sw'].frag.to(dev), c['sw'].inv.to(dev), c['sw'].c_out, c['sw'].c_in, c['sw'].kp))
    x = c['x'] if x is None else x
    buf, flat = _guarded(m * n, dev)
    if c['patch']:
        ho, wo = _PATCH_HW[n]
        y = HF.gemm_split_conv2x2(sw, x[None].to(dev), out=flat.view(1, m, ho, wo), **kw)
    else:
        gate = c['gate'][None].to(dev) if c['gate'] is not None else None
        y = HF.gemm_split(sw, _widen(c, x)[None, :, None, :].contiguous().to(dev), gate=gate, out=flat.view(1, m, 1, n), **kw)
    return y.cpu().view(m, n), _guards_intact(buf, m * n)


def _check_gpu(c, dev, what):
    """What every matrix case asserts: tier 1 and tier 2 against float64 (act = none), out-of-range elements as the emulation has them,
    two launches bit-identical, every guard element untouched."""
    y, intact = _run(c, dev)
    y2, intact2 = _run(c, dev)
    assert intact and intact2, f'{what}: a store outside y'
    assert torch.equal(y.view(torch.int32), y2.view(torch.int32)), f'{what}: two launches differ'
    assert not bool((y.view(torch.int32) == SENTINEL).any()), f'{what}: elements of y never stored'
    ref, bound, ok = _widen(c, c['ref']), _widen(c, c['bound']), _widen(c, c['ok'])
    ratio = S.assert_split(y, ref, bound, what, where=ok)
    assert torch.equal(torch.isfinite(y)[~ok], _widen(c, torch.isfinite(c['emu'][0]))[~ok]), f'{what}: out-of-range elements'
    mag, floor, under, _ = S.split_terms(c['sw'], c['x'], c['gate'], None, c['patch'])
    den = _widen(c, mag + floor + 2.0 ** 24 * under)
    live = ok & torch.isfinite(ref) & torch.isfinite(y)
    qs = torch.where(live, (y.double() - ref).abs() / den, torch.zeros_like(den))
    quiet = _widen(c, c['quiet'])
    _note(c['plan'], c['patch'], gpu_ratio=ratio, level_loud=c['level'][0], level_quiet=c['level'][1])
    for cls, level, tag in ((~quiet, c['level'][0], 'loud'), (quiet, c['level'][1], 'quiet')):
        qc = torch.where(cls, qs, torch.zeros_like(qs))
        q = float(qc.max())
        print(f'{what}: plan {tuple(c["plan"])} tier-1 ratio {ratio:.3g}, {tag} q {q:.3e} vs level {level:.3e}')
        _note(c['plan'], c['patch'], **{f'gpu_q_{tag}': q, f'gpu_q_over_level_{tag}': q / level if level > 0 else 0.0})
        assert q <= S.MARGIN * level, f'{what}: {tag} q {q:.3e} at flat index {int(qc.argmax())} above {S.MARGIN} x level {level:.3e}'
    return y


MATRIX = [(f, k, i) for f in FORMS for i, k in enumerate(DEPTHS)] + [('wide', k, i) for i, k in ((2, 100), (3, 128), (12, 1270), (13, 1280))]


@pytest.mark.gpu
@pytest.mark.parametrize('form,k,i', MATRIX, ids=[f'{f}-{k}' for f, k, _ in MATRIX])
def test_split_matrix(form, k, i):
    """Grid form x K depth x FAST; each case runs the benign inputs and one range generator (in rotation: over the 14 depths of a form
    the five generators meet FAST = false, even i, and FAST = true, odd i)."""
    dev = torch.device('cuda:0')
    m, n_odd, n_even = (64, 2080, 2080) if form == 'wide' else FORMS[form]
    n = n_even if i % 2 else n_odd
    for name in ('benign', RANGE[i % 5]):
        _check_gpu(_case(name, m, k, n, 7200 + k), dev, f'{form} K={k} N={n} {name}')


@pytest.mark.gpu
@pytest.mark.parametrize('k', [1400, 1920, 2560])
@pytest.mark.parametrize('n', [24, 128])
def test_split_two_chunk(k, n):
    dev = torch.device('cuda:0')
    i = (k // 100 + n) % 5
    for name in ('benign', RANGE[i], RANGE[(i + 2) % 5]):
        _check_gpu(_case(name, 33, k, n, 7300 + k + n), dev, f'two-chunk K={k} N={n} {name}')


@pytest.mark.gpu
@pytest.mark.parametrize('c', [34, 100, 160, 224, 288, 320, 384, 480, 640])
@pytest.mark.parametrize('n', [2, 18, 16])
def test_split_window(c, n):
    """The 2x2 / stride-2 form, and its pool_partial: block sums of the STORED y within (16 + 2) 2^-23 of sum |y| over the block."""
    from hyperseg_amd import functional as HF
    dev = torch.device('cuda:0')
    i = (c // 2 + n) % 5
    m = 33
    for name in ('benign', RANGE[i]):
        case = _case(name, m, 4 * c, n, 7400 + c + n, True)
        y = _check_gpu(case, dev, f'window c={c} N={n} {name}')
        if bool(torch.isfinite(y).all()):
            nblk = -(-n // 16)
            part = torch.full((1, m, nblk), float('nan'), device=dev)
            yp, intact = _run(case, dev, pool_partial=part)
            assert intact and torch.equal(yp, y)
            blocks = torch.nn.functional.pad(y.double(), (0, 16 * nblk - n)).view(m, nblk, 16)
            err = (part.cpu().double().view(m, nblk) - blocks.sum(2)).abs()
            assert bool((err <= (16 + 2) * 2.0 ** -23 * blocks.abs().sum(2) + 2.0 ** -149).all()), float(err.max())


@pytest.mark.gpu
@pytest.mark.parametrize('form,k,hw', [('narrow', 100, (5, 7)), ('normal', 128, (1, 14)), ('tall', 256, (48, 86))])
def test_split_up2(form, k, hw):
    """The nearest-2x store, into the middle of a larger tensor: every 2x2 block holds the plain result, nothing else is touched."""
    from hyperseg_amd import functional as HF
    dev = torch.device('cuda:0')
    m, n = FORMS[form][0], hw[0] * hw[1]
    for name in ('benign', 'cols'):
        c = _case(name, m, k, n, 7500 + k, gated=False)          # this form takes no gate
        y = _check_gpu(c, dev, f'up2 {form} plain {name}')
        pre, size = 4 * n * 3 + GUARD, 4 * m * n
        buf = torch.full((pre + size + pre,), SENTINEL, dtype=torch.int32, device=dev)
        out = buf.view(torch.float32)[pre:pre + size].view(1, m, 2 * hw[0], 2 * hw[1])
        HF.gemm_split_up2(c['sw_dev'], _widen(c, c['x']).view(1, k, *hw).contiguous().to(dev), out=out)
        b = buf.cpu()
        assert bool((b[:pre] == SENTINEL).all()) and bool((b[pre + size:] == SENTINEL).all())
        want = y.view(m, hw[0], 1, hw[1], 1).expand(m, hw[0], 2, hw[1], 2).reshape(1, m, 2 * hw[0], 2 * hw[1])
        assert torch.equal(out.cpu().view(torch.int32), want.contiguous().view(torch.int32))


@pytest.mark.gpu
@pytest.mark.parametrize('form,k', [('narrow', 250), ('normal', 64), ('tall', 512)])
def test_split_tail(form, k):
    """Shift, activation and residual (separate, and ``residual is out``) under the tail terms of the bound."""
    from hyperseg_amd import functional as HF
    dev = torch.device('cuda:0')
    m, n = FORMS[form][0], FORMS[form][2]
    c = _case('benign', m, k, n, 7600 + k)
    ref, e = _widen(c, c['ref']), _widen(c, c['bound'])
    shift = torch.randn(m, generator=G(7601))
    res = torch.randn(m, n, generator=G(7602))
    z = ref + shift.double()[:, None]
    for act, fn in ((0, lambda t: t), (1, torch.relu), (2, lambda t: t.clamp(0, 6)), (3, lambda t: t * torch.sigmoid(t))):
        y, intact = _run(c, dev, shift=shift.to(dev), act=act, residual=res[None, :, None, :].contiguous().to(dev))
        want = fn(z) + res.double()
        assert intact
        S.assert_split(y, want, S.tail_bound(e, z, fn(z), want, act == 3, True), f'tail {form} act {act}')
    acc = res[None, :, None, :].contiguous().to(dev)
    x = _widen(c, c['x'])[None, :, None, :].contiguous().to(dev)
    assert HF.gemm_split(c['sw_dev'], x, gate=c['gate'][None].to(dev), residual=acc, out=acc) is acc
    want = ref + res.double()
    S.assert_split(acc.cpu().view(m, n), want, S.tail_bound(e, ref, ref, want, False, True), f'tail {form} in place')


@pytest.mark.gpu
@pytest.mark.parametrize('form,k,n', [('narrow', 100, 36), ('normal', 256, 14), ('tall', 33, 4128), ('two-chunk', 1920, 24), ('window', 4 * 288, 18)])
def test_split_nonfinite_contained(form, k, n):
    """+inf at one (k, n) and NaN at another: finite exactly where the float64 product is, every other pixel column bit-identical
    to the run without them."""
    dev = torch.device('cuda:0')
    patch = form == 'window'
    m = 33 if form in ('two-chunk', 'window') else FORMS[form][0]
    c = _case('benign', m, k, n, 7700 + k, patch)
    clean, _ = _run(c, dev)
    xk = S.window_matrix(c['x']) if patch else _widen(c, c['x']).clone()
    xk = xk.clone()
    cols = (1, n - 1)
    xk[k // 3, cols[0]] = float('inf')
    xk[k - 1, cols[1]] = float('nan')
    gx = xk.double() if c['gate'] is None else xk.double() * c['gate'].double()[:, None]
    ref = c['w'].double() @ gx
    wide = dict(c, nu=n, x=S.window_image(xk, *_PATCH_HW[n]) if patch else xk)
    wide.pop('sw_dev', None)
    y, intact = _run(wide, dev)
    assert intact
    assert torch.equal(torch.isfinite(y), torch.isfinite(ref))
    assert not bool(torch.isfinite(y[:, cols[0]]).any()) and not bool(torch.isfinite(y[:, cols[1]]).any())
    keep = torch.ones(n, dtype=torch.bool)
    keep[list(cols)] = False
    assert torch.equal(y[:, keep].view(torch.int32), clean[:, keep].view(torch.int32))
