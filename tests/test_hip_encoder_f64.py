"""The encoder's fp32 helper kernels (hs_encoder.hip, hs_mbconv.hip, hs_mbconv_lean.hip) against float64, element by element, under the
bound derived in util_encoder_ref.py -- and every case first asserts the ROUTE it was written for (hs_*_route: the launchers' own
predicates), so a threshold edit that moves a shape to another kernel fails here instead of silently dropping coverage.

CPU tests (unmarked): the fp32 restatement of every operation lies inside its own bound on every case and generator, every defect of
util_encoder_ref.DEFECTS is rejected, the route queries answer as the case tables say and the tables cover every code.  GPU tests
(``-m gpu``): the kernels.  With HS_ENCODER_F64_REPORT=<file> the GPU run writes one line per kernel, route and output: the worst err / bound,
the tier-2 q against the CPU level where the sum is long, the element index (profiles/encoder_f64_bound.txt is such a run; nothing here is
tuned to it).  Sums of more than 64 terms are held to tier 2 wherever they occur: the pooled partial sums (also against the float64 sums
of the launch's own y, where nothing but the reduction can err), the expand sum at Cin 80, the squeeze and excite mat-vecs (the gate also
against float64 on the launch's own squeezed vector), the 1x1 conv at Cin >= 96.

The route codes name the FORM of a kernel.  Its unrolled depth -- NB of the 1x1 conv, KS of the expand + depthwise kernels -- follows
from c_in alone and is deliberately not part of the coverage table; test_route_coverage_table_names_every_code asserts beside the table
that the cases still run every NB (1..8) and every instantiated KS (lean 4, 6, 8, 10; general 4, 6, 10, 12, 20).

Findings of writing the cases against the queries (kept as cases, with the route they really take):
  * 64 and 60 pixels do NOT sit on either side of the 1x1 conv's interleaved form: below 512 workgroups the launcher shrinks NT to 1 first, so
    both take 'nt1'.  The vector form needs >= 512 workgroups at NT = 4; PW_CASES reaches it with 8256 pixels x 512 output channels and its
    twin with 8252 pixels, and 'nt2' with 256 output channels.
  * 8192 planes of 16 x 64 at stride 2 have 64 output quads and take a vector form; the tiled 3x3 / stride-2 instantiation needs >= 256
    output quads: its case is 8192 planes of 32 x 128 -> 16 x 64.
  * HS_SE_ROUTE_FUSED_WIDE is compiled out of the product build (include/hyperseg_hip.h), so 6144 units is no threshold of it: the shape
    just above it takes 'early'."""
import functools
import os

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


_REPORT_STARTED = set()


def _report(kernel, route, name, output, ratio, index, q=None, level=None, tier2='  tier-2 q {:.3e} vs CPU level (x2) {:.3e}'):
    path = os.environ.get('HS_ENCODER_F64_REPORT')
    if path:
        tier2 = '' if q is None else tier2.format(q, level)
        mode = 'a' if path in _REPORT_STARTED else 'w'          # a run starts its file afresh
        _REPORT_STARTED.add(path)
        with open(path, mode) as f:
            f.write(f'{kernel:10s} {str(route):16s} {name:28s} {output:9s} worst err/bound {ratio:.4f} at {index}{tier2}\n')


def _check_pool(kernel, route, tag, y, partial, ref, group, level, hw, report=True):
    """The partial sums three ways: against float64 under the worst-case bound, under the tier-2 bound (the pool at MARGIN x its CPU
    level), and against the float64 sums of the launch's OWN y (the reduction alone, tier 2); then the pooled mean, which is the HOST's
    division of those partials (checked because callers use it; it says nothing more about the kernel and is not reported)."""
    ratio, i = R.check(partial, ref['partial'], f'{tag} partial')
    R.check(partial, R.pool_stage(R.Chain('bound', q={'pool': level}), ref['y'], group), f'{tag} partial tier 2')
    own = R.pool_own(y, group, level)
    R.check(partial, own, f'{tag} partial against the sums of its own y, tier 2')
    qk, _ = R.q_of(partial, own, group(y.detach().double().cpu().abs()).sum(-1))
    if report:
        _report(kernel, route, tag, 'partial', ratio, i, qk, level, tier2='  tier-2 q (vs its own y) {:.3e} vs CPU level (x2) {:.3e}')
    b, c = ref['mean'][0].shape
    R.check(partial.detach().double().cpu().sum(1).view(b, c) / hw, ref['mean'], f'{tag} mean')


def _to(dev, d):
    return {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in d.items()}


# ------------------------------------------------------------------------------------------------------------ depthwise

# name -> (route, b, c, h, w, k, stride, pads, prologue, generators); pads: 'same' | 'sym' | (pad_t, pad_l, Ho, Wo)
DW_CASES = {
    'v31 same': ('vector_k3s1_pl1', 2, 5, 7, 12, 3, 1, 'same', False, ('benign',)),
    'v31 top0 left1': ('vector_k3s1_pl1', 1, 7, 8, 12, 3, 1, (0, 1, 7, 12), True, ('benign',)),
    'v320 same': ('vector_k3s2_pl0', 2, 13, 10, 16, 3, 2, 'same', True, ('benign', 'preact', 'quiet')),
    'v320 top1 left0': ('vector_k3s2_pl0', 1, 6, 9, 16, 3, 2, (1, 0, 5, 8), False, ('benign',)),
    'v321 sym': ('vector_k3s2_pl1', 2, 5, 10, 16, 3, 2, 'sym', False, ('benign',)),
    'v321 sym pre': ('vector_k3s2_pl1', 1, 13, 16, 32, 3, 2, 'sym', True, ('benign', 'preact')),
    'v512 same': ('vector_k5s1_pl2', 2, 5, 9, 16, 5, 1, 'same', False, ('benign',)),
    'v521 same': ('vector_k5s2_pl1', 2, 9, 12, 16, 5, 2, 'same', False, ('benign',)),
    'v522 sym': ('vector_k5s2_pl2', 2, 5, 12, 16, 5, 2, 'sym', False, ('benign',)),
    'v522 sym pre': ('vector_k5s2_pl2', 1, 13, 14, 24, 5, 2, 'sym', True, ('benign', 'preact')),
    'g31 odd W': ('generic_k3s1', 2, 13, 7, 9, 3, 1, 'same', True, ('benign', 'preact', 'quiet')),
    'g32 odd W': ('generic_k3s2', 2, 5, 9, 13, 3, 2, 'same', False, ('benign',)),
    'g32 sym odd W': ('generic_k3s2', 1, 5, 10, 14, 3, 2, 'sym', False, ('benign',)),
    'g32 pad_l 2': ('generic_k3s2', 1, 5, 10, 16, 3, 2, (1, 2, 5, 8), False, ('benign',)),
    'g51 odd W': ('generic_k5s1', 2, 5, 9, 14, 5, 1, 'same', False, ('benign',)),
    'g52 odd W': ('generic_k5s2', 2, 5, 11, 15, 5, 2, 'same', True, ('benign',)),
    'g52 sym odd W': ('generic_k5s2', 1, 5, 12, 18, 5, 2, 'sym', False, ('benign',)),
    't51 32x32': ('tiled_k5s1', 1, 2, 32, 32, 5, 1, 'same', True, ('benign',)),
    't51 40x32 dead rows': ('tiled_k5s1', 1, 13, 40, 32, 5, 1, 'same', True, ('benign', 'preact', 'quiet')),
    't52 64x64': ('tiled_k5s2', 1, 2, 64, 64, 5, 2, 'same', True, ('benign',)),
    't52 80x64 dead rows': ('tiled_k5s2', 1, 2, 80, 64, 5, 2, 'sym', True, ('benign',)),
    't31 8192 planes': ('tiled_k3s1', 2, 4096, 16, 64, 3, 1, 'same', True, ('benign',)),
    't32 8192 planes': ('tiled_k3s2', 1, 8192, 32, 128, 3, 2, 'same', True, ('benign',)),
}
DW_PARAMS = [(n, g) for n, c in DW_CASES.items() for g in c[-1]]


def _dw_geom(case):
    route, b, c, h, w, k, s, pads, pre, _ = case
    pt, pl, ho, wo = R.same_pads(h, w, k, s) if pads == 'same' else (R.sym_pads(h, w, k, s) if pads == 'sym' else pads)
    return route, (b, c, h, w), k, s, pt, pl, (ho, wo), pre


@functools.lru_cache(maxsize=4)
def _dw_ref(name, gen):
    _, (b, c, h, w), k, s, pt, pl, out, pre = _dw_geom(DW_CASES[name])
    d = R.dw_inputs(gen, b, c, h, w, k, seed=sum(map(ord, name)), prologue=pre)
    ref = R.depthwise_ref(R.Chain('bound'), d['x'], d['wt'], s, pt, pl, out, d['scale'], d['shift'], R.ACT_SWISH, d['in_scale'], d['in_shift'])
    ref['level'] = R.pool_level(ref['y'][0], R.dw_group(*out), 256)          # >= 256 pixels per block: always tier 2
    return d, ref


@pytest.mark.parametrize('name,gen', [p for p in DW_PARAMS if DW_CASES[p[0]][2] < 4096])
def test_depthwise_restatement_within_bound(name, gen):
    _, _, k, s, pt, pl, out, _ = _dw_geom(DW_CASES[name])
    d, ref = _dw_ref(name, gen)
    got = R.depthwise_ref(R.Chain('f32'), d['x'], d['wt'], s, pt, pl, out, d['scale'], d['shift'], R.ACT_SWISH, d['in_scale'], d['in_shift'])
    R.check(got['y'][0], ref['y'], f'{name} {gen} y')
    _check_pool('depthwise', None, f'{name} {gen}', got['y'][0], got['partial'][0], ref, R.dw_group(*out), ref['level'], out[0] * out[1], report=False)


@gpu
@pytest.mark.parametrize('name,gen', DW_PARAMS)
def test_depthwise(dev, name, gen):
    HF = _HF()
    route, shape, k, s, pt, pl, out, pre = _dw_geom(DW_CASES[name])
    assert HF.depthwise_route(shape, k, s, pl, out, prologue=pre) == route
    d, ref = _dw_ref(name, gen)
    g = _to(dev, d)
    args = (g['x'], g['wt'], s, pt, pl, out, g['scale'], g['shift'])
    kw = dict(act=3, in_scale=g['in_scale'], in_shift=g['in_shift'])
    y0 = HF.depthwise_conv_bn_act(*args, pool=False, **kw)
    y, partial = HF.depthwise_conv_bn_act(*args, pool=True, **kw)
    assert torch.equal(y0, y)
    _report('depthwise', route, f'{name} / {gen}', 'y', *R.check(y, ref['y'], f'{name} y'))
    _check_pool('depthwise', route, f'{name} / {gen}', y, partial, ref, R.dw_group(*out), ref['level'], out[0] * out[1])


# ------------------------------------------------------------------------------------------------------------ stem, stem + dw, expand + dw

# name -> (route, b, h, w, cout, (pad_t, pad_l, Ho, Wo))
STEM_CASES = {'even': ('vector_pl0', 2, 20, 24, 13, (0, 0, 10, 12)), 'odd sym': ('generic', 1, 17, 9, 8, (1, 1, 9, 5)),
              'odd W': ('generic', 2, 10, 22, 5, (0, 0, 5, 11)), 'sym W % 4 == 0': ('vector_pl1', 2, 18, 24, 9, (1, 1, 9, 12)),
              'top 0 left 1': ('vector_pl1', 1, 12, 16, 6, (0, 1, 6, 8)), 'pad_l 2': ('generic', 1, 12, 16, 6, (1, 2, 6, 8))}


def _stem_inputs(b, h, w, cout, seed):
    g = torch.Generator().manual_seed(seed)
    return dict(x=torch.rand(b, 3, h, w, generator=g) * 4 - 2, wt=torch.randn(cout, 3, 3, 3, generator=g) * 0.3,
                scale=torch.rand(cout, generator=g) + 0.5, shift=torch.randn(cout, generator=g) * 0.1)


@pytest.mark.parametrize('name', STEM_CASES)
def test_stem_restatement_within_bound(name):
    _, b, h, w, cout, (pt, pl, ho, wo) = STEM_CASES[name]
    d = _stem_inputs(b, h, w, cout, h * w)
    R.check(R.stem_ref(R.Chain('f32'), d['x'], d['wt'], pt, pl, (ho, wo), d['scale'], d['shift'])[0],
            R.stem_ref(R.Chain('bound'), d['x'], d['wt'], pt, pl, (ho, wo), d['scale'], d['shift']), name)


@gpu
@pytest.mark.parametrize('name', STEM_CASES)
def test_stem(dev, name):
    route, b, h, w, cout, (pt, pl, ho, wo) = STEM_CASES[name]
    assert _HF().stem_route(w, pl) == route
    d = _stem_inputs(b, h, w, cout, h * w)
    g = _to(dev, d)
    y = _HF().stem_conv_bn_swish(g['x'], g['wt'], pt, pl, (ho, wo), g['scale'], g['shift'])
    _report('stem', route, name, 'y',
            *R.check(y, R.stem_ref(R.Chain('bound'), d['x'], d['wt'], pt, pl, (ho, wo), d['scale'], d['shift']), name))


# name -> (route, b, cin, cmid, k, stride, h, w, pads, generators)
MB_CASES = {
    'lean k3s1 ragged rows': ('lean_k3s1', 1, 16, 32, 3, 1, 20, 16, 'same', ('benign', 'preact')),
    'lean k3s2 ragged rows': ('lean_k3s2', 2, 24, 32, 3, 2, 24, 32, 'same', ('benign',)),
    'lean k3s2 sym': ('lean_k3s2', 1, 16, 16, 3, 2, 32, 32, 'sym', ('benign',)),
    'lean k5s1': ('lean_k5s1', 1, 40, 16, 5, 1, 16, 16, 'same', ('benign',)),
    'lean k3s1 cin 32': ('lean_k3s1', 1, 32, 16, 3, 1, 16, 16, 'same', ('benign',)),
    'full k3s1 cin 22': ('full_k3s1', 1, 22, 16, 3, 1, 9, 12, 'same', ('benign',)),
    'full k5s2 cin 48': ('full_k5s2', 1, 48, 40, 5, 2, 17, 40, 'same', ('benign',)),
    'lean k5s2': ('lean_k5s2', 1, 16, 32, 5, 2, 32, 32, 'same', ('benign',)),
    'full k3s1 off chunk': ('full_k3s1', 2, 6, 20, 3, 1, 9, 9, 'same', ('benign', 'preact')),
    'full k3s2 ragged': ('full_k3s2', 1, 40, 100, 3, 2, 31, 45, 'same', ('benign',)),
    'full k5s1 cin 80': ('full_k5s1', 1, 80, 40, 5, 1, 20, 36, 'same', ('benign',)),
    'full k5s2 cin 32 (lean spills)': ('full_k5s2', 1, 32, 32, 5, 2, 32, 32, 'same', ('benign',)),
    'full k5s2 sym': ('full_k5s2', 1, 12, 20, 5, 2, 17, 21, 'sym', ('benign',)),
    'cin 84 refused': (None, 1, 84, 16, 3, 1, 8, 16, 'same', ()),
}
MB_PARAMS = [(n, g) for n, c in MB_CASES.items() for g in c[-1]]


def _mb_geom(case):
    route, b, cin, cmid, k, s, h, w, pads, _ = case
    pt, pl, ho, wo = R.same_pads(h, w, k, s) if pads == 'same' else R.sym_pads(h, w, k, s)
    return route, (b, cin, h, w), cmid, k, s, pt, pl, (ho, wo)


@functools.lru_cache(maxsize=4)
def _mb_ref(name, gen):
    _, (b, cin, h, w), cmid, k, s, pt, pl, out = _mb_geom(MB_CASES[name])
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    d = dict(x=torch.randn(b, cin, h, w, generator=g), we=torch.randn(cmid, cin, 1, 1, generator=g) / cin ** 0.5,
             wd=torch.randn(cmid, 1, k, k, generator=g) * 0.3, s0=torch.rand(cmid, generator=g) + 0.5, b0=torch.randn(cmid, generator=g) * 0.3,
             s1=torch.rand(cmid, generator=g) + 0.5, b1=torch.randn(cmid, generator=g) * 0.1)
    if gen == 'preact':
        d['s0'], d['b0'] = R._sweep(cmid, g)
    run = lambda ch: R.mbconv_ref(ch, d['x'], d['we'], d['s0'], d['b0'], d['wd'], s, pt, pl, out, d['s1'], d['b1'])      # noqa: E731
    ref = run(R.Chain('bound'))
    ref['level'] = R.pool_level(ref['y'][0], R.tile_group(16 if s == 1 else 8), 16)          # 256 / 128 pixels per tile: tier 2
    ref['y2'] = None
    if cin > 64:                                      # tier 2 of the expand sum
        ref['expand'] = R.sum_level((d['we'].flatten(1)[None, :, None, :] * d['x'].flatten(2).permute(0, 2, 1)[:, None]), 4)
        ref['y2'] = run(R.Chain('bound', q={'expand': ref['expand']}))['y']
    return d, ref


@pytest.mark.parametrize('name,gen', MB_PARAMS)
def test_mbconv_restatement_within_bound(name, gen):
    _, _, _, _, s, pt, pl, out = _mb_geom(MB_CASES[name])
    d, ref = _mb_ref(name, gen)
    got = R.mbconv_ref(R.Chain('f32'), d['x'], d['we'], d['s0'], d['b0'], d['wd'], s, pt, pl, out, d['s1'], d['b1'])
    R.check(got['y'][0], ref['y'], f'{name} {gen} y')
    if ref['y2']:
        R.check(got['y'][0], ref['y2'], f'{name} {gen} y tier 2')
    _check_pool('expand+dw', None, f'{name} {gen}', got['y'][0], got['partial'][0], ref, R.tile_group(16 if s == 1 else 8), ref['level'], out[0] * out[1],
                report=False)


@gpu
@pytest.mark.parametrize('name,gen', MB_PARAMS)
def test_mbconv_expand_dw(dev, name, gen):
    HF = _HF()
    route, shape, cmid, k, s, pt, pl, out = _mb_geom(MB_CASES[name])
    assert HF.mbconv_route(shape, cmid, k, s, out) == route
    d, ref = _mb_ref(name, gen)
    g = _to(dev, d)
    y, partial = HF.mbconv_expand_dw(g['x'], g['we'], g['s0'], g['b0'], g['wd'], s, pt, pl, out, g['s1'], g['b1'], pool=True)
    ratio, i = R.check(y, ref['y'], f'{name} y')
    if ref['y2']:                                     # Cin > 64: the expand sum at MARGIN x its CPU level, and the bare expand's q beside it
        R.check(y, ref['y2'], f'{name} y tier 2')
        bare = HF.pointwise_conv(g['x'], g['we'].flatten(1).contiguous()).flatten(2)
        w64, x64 = d['we'].double().flatten(1), d['x'].double().flatten(2)
        qk, _ = R.q_of(bare, (torch.einsum('oc,bcp->bop', w64, x64), None), torch.einsum('oc,bcp->bop', w64.abs(), x64.abs()))
        _report('expand+dw', route, f'{name} / {gen}', 'y', ratio, i, qk, ref['expand'], tier2='  tier-2 held; q of the same product by hs_pointwise_conv_fwd {:.3e} vs CPU level (x2) {:.3e}')
    else:
        _report('expand+dw', route, f'{name} / {gen}', 'y', ratio, i)
    _check_pool('expand+dw', route, f'{name} / {gen}', y, partial, ref, R.tile_group(16 if s == 1 else 8), ref['level'], out[0] * out[1])


@gpu
def test_mbconv_refuses_what_its_route_refuses(dev):
    HF = _HF()
    _, shape, cmid, k, s, pt, pl, out = _mb_geom(MB_CASES['cin 84 refused'])
    assert HF.mbconv_route(shape, cmid, k, s, out) is None
    z = lambda *sh: torch.zeros(*sh, device=dev)      # noqa: E731
    with pytest.raises(Exception, match='unsupported shape'):
        HF.mbconv_expand_dw(z(*shape), z(cmid, shape[1], 1, 1), z(cmid), z(cmid), z(cmid, 1, k, k), s, pt, pl, out, z(cmid), z(cmid))


# name -> (route, b, cmid, h, w, stem pads, generator); the depthwise 3x3 pads (1, 1)
STEM_DW_CASES = {'whole tiles': ('stem_k3s1', 1, 16, 64, 32, 'same', 'benign'), 'ragged rows, odd image': ('stem_k3s1', 2, 32, 51, 63, 'same', 'benign'),
                 'sym stem pad': ('stem_k3s1', 1, 16, 40, 64, 'sym', 'benign'), 'stem pad top 0 left 1': ('stem_k3s1', 1, 16, 33, 32, (0, 1, 16, 16), 'benign'),
                 'preact': ('stem_k3s1', 1, 16, 32, 32, 'same', 'preact'), 'preact sym': ('stem_k3s1', 1, 16, 24, 32, 'sym', 'preact'),
                 'ragged tile columns': (None, 1, 32, 32, 72, 'same', 'benign'), 'c_mid off the chunk': (None, 1, 24, 32, 32, 'same', 'benign')}


def _stem_dw_inputs(name):
    route, b, cmid, h, w, pads, gen = STEM_DW_CASES[name]
    d = _stem_inputs(b, h, w, cmid, h + w)
    g = torch.Generator().manual_seed(h * w)
    d.update(wd=torch.randn(cmid, 1, 3, 3, generator=g) * 0.3, s1=torch.rand(cmid, generator=g) + 0.5, b1=torch.randn(cmid, generator=g) * 0.1)
    if gen == 'preact':                               # the stem's BatchNorm sweeps the pre-activation of the recomputed mid per channel
        d['scale'], d['shift'] = R._sweep(cmid, g, ref_mag=3.0)
    return route, d, (R.same_pads(h, w, 3, 2) if pads == 'same' else (R.sym_pads(h, w, 3, 2) if pads == 'sym' else pads))


def _stem_dw_ref(ch, d, pads):
    pt, pl, hs, ws = pads
    return R.stem_dw_ref(ch, d['x'], d['wt'], d['scale'], d['shift'], pt, pl, (hs, ws), d['wd'], 1, 1, d['s1'], d['b1'])


@pytest.mark.parametrize('name', [n for n, c in STEM_DW_CASES.items() if c[0]])
def test_stem_dw_restatement_within_bound(name):
    _, d, pads = _stem_dw_inputs(name)
    got, ref = _stem_dw_ref(R.Chain('f32'), d, pads), _stem_dw_ref(R.Chain('bound'), d, pads)
    assert all(bool(torch.isfinite(t).all()) for v in ref.values() for t in v), name
    R.check(got['y'][0], ref['y'], f'{name} y')
    _check_pool('stem+dw', None, name, got['y'][0], got['partial'][0], ref, R.tile_group(16), R.pool_level(ref['y'][0], R.tile_group(16), 16),
                pads[2] * pads[3], report=False)


@gpu
@pytest.mark.parametrize('name', STEM_DW_CASES)
def test_stem_dw(dev, name):
    HF = _HF()
    route, d, (pt, pl, hs, ws) = _stem_dw_inputs(name)
    b, cmid, h, w = STEM_DW_CASES[name][1:5]
    assert HF.stem_dw_route((h, w), cmid, pt, pl, (hs, ws)) == route
    g = _to(dev, d)
    w28 = torch.nn.functional.pad(g['wt'].flatten(1), (0, 1)).contiguous()
    out = HF.stem_dw(g['x'], w28, g['scale'], g['shift'], pt, pl, (hs, ws), g['wd'], 1, 1, g['s1'], g['b1'], pool=True)
    if route is None:
        assert out is None
        return
    ref = _stem_dw_ref(R.Chain('bound'), d, (pt, pl, hs, ws))
    _report('stem+dw', route, name, 'y', *R.check(out[0], ref['y'], f'{name} y'))
    _check_pool('stem+dw', route, name, out[0], out[1], ref, R.tile_group(16), R.pool_level(ref['y'][0], R.tile_group(16), 16), hs * ws)


# ------------------------------------------------------------------------------------------------------------ squeeze-excite gate

# name -> (route without w_proj, route with w_proj, c, csq, nblk, cout)
SE_CASES = {
    'channels 768': ('fused', 'fused', 768, 28, 2, 40),
    'channels 772': ('two_launch', 'two_launch', 772, 28, 2, 40),
    'units 2048': ('fused', 'fused', 128, 6, 64, 24),
    'units 2052': ('early', 'two_launch', 108, 4, 76, 24),
    'units 6200': ('early', 'two_launch', 100, 5, 248, 7),
    'csq 32': ('fused', 'fused', 240, 32, 8, 40),
    'csq 33': ('two_launch', 'two_launch', 240, 33, 8, 40),
    'early csq 8 fold 2': ('early', 'two_launch', 32, 8, 512, 16),
    'early csq 9': ('two_launch', 'two_launch', 32, 9, 512, 16),
    'early fold 4': ('early', 'two_launch', 16, 4, 1024, 16),
    'nblk 304 = 8 * 38': ('early', 'two_launch', 72, 6, 304, 24),
    'nblk 300 % 8 != 0': ('two_launch', 'two_launch', 72, 6, 300, 24),
    'channels % 4 != 0': ('two_launch', 'two_launch', 50, 3, 5, 7),
    'C 1920': ('two_launch', 'two_launch', 1920, 80, 1, 64),
}
SE_PARAMS = [(n, b, g) for n in SE_CASES for b in (1, 2) for g in ('benign', 'pixel_sums')]


@functools.lru_cache(maxsize=4)
def _se_ref(name, batch, gen):
    _, _, c, csq, nblk, cout = SE_CASES[name]
    d = R.se_inputs(gen, batch, c, csq, nblk, cout, seed=c + csq + nblk)
    inv = 1.0 / d['hw']
    run = lambda ch: R.se_gate_ref(ch, d['partial'], batch, inv, d['w1'], d['b1'], d['w2'], d['b2'], d['wp'], d['osc'])      # noqa: E731
    ref, q = run(R.Chain('bound')), {}
    inv32 = torch.tensor(inv, dtype=torch.float32)
    if c * nblk + 1 > 64:                             # tier 2: the CPU level of the two long sums on these inputs
        q['squeeze'] = R.sum_level((d['w1'][None, :, :, None] * (d['partial'].view(batch, 1, c, nblk) * inv32)).flatten(2), 256)
    if csq > 64:
        q['excite'] = R.sum_level(d['w2'][None] * ref['squeezed'][0].float()[:, None, :], 4)
    return d, ref, (run(R.Chain('bound', q=q)) if q else None), q


@pytest.mark.parametrize('name,batch,gen', [p for p in SE_PARAMS if p[1] == 2])
def test_se_gate_restatement_within_bound(name, batch, gen):
    d, ref, ref2, _ = _se_ref(name, batch, gen)
    got = R.se_gate_ref(R.Chain('f32'), d['partial'], batch, 1.0 / d['hw'], d['w1'], d['b1'], d['w2'], d['b2'], d['wp'], d['osc'])
    for key in ('squeezed', 'gate', 'w_scaled'):
        R.check(got[key][0], ref[key], f'{name} {gen} {key}')
        if ref2:
            R.check(got[key][0], ref2[key], f'{name} {gen} {key} tier 2')


@gpu
@pytest.mark.parametrize('name,batch,gen', SE_PARAMS)
def test_se_gate(dev, name, batch, gen):
    HF = _HF()
    plain, proj, c, csq, nblk, cout = SE_CASES[name]
    assert HF.se_gate_route(c, nblk, csq) == plain and HF.se_gate_route(c, nblk, csq, w_proj=True) == proj
    d, ref, ref2, q = _se_ref(name, batch, gen)
    g = _to(dev, d)
    args = (g['partial'], batch, d['hw'], g['w1'], g['b1'], g['w2'].t().contiguous(), g['b2'])
    gate = HF.se_gate(*args)
    tag = f'{name} / b{batch} / {gen}'
    # the same launch through the raw entry, to see the squeezed vector as well
    from hyperseg_amd import _hip
    csq = d['w1'].shape[0]
    sq, gate_raw = torch.empty(batch, csq, device=dev), torch.empty(batch, c, device=dev)
    _hip.run.hs_se_gate_fwd(args[0].data_ptr(), batch, c, nblk, 1.0 / d['hw'], args[3].data_ptr(), args[4].data_ptr(), csq, args[5].data_ptr(),
                            args[6].data_ptr(), sq.data_ptr(), gate_raw.data_ptr(), None, 0, None, None, _hip.stream_ptr())
    assert torch.equal(gate_raw, gate)
    for out, got in (('squeezed', sq), ('gate', gate)):
        ratio, i = R.check(got, ref[out], f'{tag} {out}')
        if not ref2:
            _report('se_gate', plain, tag, out, ratio, i)
            continue
        R.check(got, ref2[out], f'{tag} {out} tier 2')     # the long sums at MARGIN x their CPU level
        if out == 'squeezed' and 'squeeze' in q:           # the squeeze sum's q, the fast swish's own error included (|swish'| <= 1.0999)
            p64 = d['partial'].double().view(batch, c, nblk).abs().sum(2)
            mag = 1.0999 * (torch.einsum('jc,bc->bj', d['w1'].double().abs(), p64) / d['hw'])
            _report('se_gate', plain, tag, out, ratio, i, R.q_of(sq, ref['squeezed'], mag)[0], q['squeeze'],
                    tier2='  tier-2 q (activation error included) {:.3e} vs CPU level (x2) {:.3e}')
        else:
            _report('se_gate', plain, tag, out, ratio, i)
    # the excite mat-vec + sigmoid alone: float64 on the launch's OWN squeezed vector, no operand error
    own = R.se_excite_ref(R.Chain('bound', q={k: v for k, v in q.items() if k == 'excite'}), (sq.double().cpu(), torch.zeros(batch, csq, dtype=torch.float64)), d['w2'], d['b2'])
    _report('se_gate', plain, tag, 'gate|own z', *R.check(gate, own, f'{tag} gate against its own squeezed vector'))
    ws = HF.se_gate(*args, w_proj=g['wp'])
    wp = d['wp'].double()
    noscale = (ref['gate'][0][:, None, :] * wp[None], ref['gate'][1][:, None, :] * wp.abs()[None] + 3 * R.U32 * (ref['gate'][0][:, None, :] * wp[None]).abs() + R.SUB)
    _report('se_gate', proj, tag, 'w_proj', *R.check(ws.view(batch, cout, c), noscale, f'{tag} w_scaled without out_scale'))
    ws = HF.se_gate(*args, w_proj=g['wp'], out_scale=g['osc'])
    for r in ([ref, ref2] if ref2 else [ref]):
        ratio, i = R.check(ws.view(batch, cout, c), r['w_scaled'], f'{tag} w_scaled')
    _report('se_gate', proj, tag, 'w_scaled', ratio, i)


# ------------------------------------------------------------------------------------------------------------ 1x1 conv, affine epilogue

# name -> (route, b, cin, cout, pixels, generators)
PW_CASES = {
    '64 pixels cin 96': ('nt1_nb6', 2, 96, 40, 64, ('benign', 'gates', 'preact', 'quiet')),
    '60 pixels cin 96': ('nt1_nb6', 2, 96, 40, 60, ('benign', 'gates')),
    'off 4 and 16': ('nt1_nb1', 2, 13, 7, 60, ('benign', 'gates')),
    'cin 22 cout 130': ('nt1_nb2', 1, 22, 130, 64, ('benign',)),
    'cin 128': ('nt1_nb8', 1, 128, 33, 68, ('benign',)),
    'cin 60': ('nt1_nb4', 1, 60, 9, 64, ('benign',)),
    'cin 70': ('nt1_nb5', 1, 70, 9, 60, ('benign',)),
    'cin 100': ('nt1_nb7', 1, 100, 9, 64, ('benign',)),
    'vec 8256 pixels': ('vec_nb3', 1, 40, 512, 8256, ('benign', 'gates')),
    'nt4 8252 pixels': ('nt4_nb3', 1, 40, 512, 8252, ('benign',)),
    'nt2 8256 pixels': ('nt2_nb1', 1, 16, 256, 8256, ('benign',)),
    'cin 130 refused': (None, 1, 130, 8, 64, ()),
}
PW_PARAMS = [(n, g) for n, c in PW_CASES.items() for g in c[-1]]
PW_OPTIONS = [(act, gate, res) for act in (0, 1, 2, 3) for gate in (False, True) for res in (False, True)]


@functools.lru_cache(maxsize=4)
def _pw_ref(name, gen, act=3, gate=True, res=True):
    _, b, cin, cout, p, _ = PW_CASES[name]
    d = R.pw_inputs(gen, b, cin, cout, p, seed=cin * 131 + cout + p, gate=gate, residual=res)
    run = lambda ch: R.pointwise_ref(ch, d['x'], d['w'], d['gate'], d['scale'], d['shift'], act, d['residual'])      # noqa: E731
    ref, ref2, level = run(R.Chain('bound')), None, None
    if cin > 64:                                      # tier 2
        gx = d['x'] if d['gate'] is None else d['x'] * d['gate'][:, :, None]
        level = R.sum_level((d['w'][None, :, None, :] * gx.permute(0, 2, 1)[:, None]), 4)
        ref2 = run(R.Chain('bound', q={'conv': level}))
    return d, ref, ref2, level


@pytest.mark.parametrize('name,gen', [p for p in PW_PARAMS if PW_CASES[p[0]][4] < 1000])
def test_pointwise_restatement_within_bound(name, gen):
    d, ref, ref2, _ = _pw_ref(name, gen)
    got = R.pointwise_ref(R.Chain('f32'), d['x'], d['w'], d['gate'], d['scale'], d['shift'], 3, d['residual'])[0]
    R.check(got, ref, f'{name} {gen}')
    if ref2:
        R.check(got, ref2, f'{name} {gen} tier 2')


def _pw_run(dev, name, gen, act, gate, res):
    HF = _HF()
    route, b, cin, cout, p, _ = PW_CASES[name]
    assert HF.pointwise_route(b, cin, cout, p) == route
    d, ref, ref2, level = _pw_ref(name, gen, act, gate, res)
    g = _to(dev, d)
    y = HF.pointwise_conv(g['x'].view(b, cin, p, 1), g['w'], g['gate'], g['scale'], g['shift'], act,
                          None if g['residual'] is None else g['residual'].view(b, cout, p, 1)).view(b, cout, p)
    tag = f'{name} / {gen} / act {act}{" gate" if gate else ""}{" res" if res else ""}'
    ratio, i = R.check(y, ref, tag)
    if ref2:
        R.check(y, ref2, tag + ' tier 2')
        gx = d['x'].double() if d['gate'] is None else d['x'].double() * d['gate'].double()[:, :, None]
        bare = HF.pointwise_conv(g['x'].view(b, cin, p, 1), g['w'], g['gate']).view(b, cout, p)
        mag = torch.einsum('oc,bcp->bop', d['w'].double().abs(), gx.abs())
        qk, _ = R.q_of(bare, (torch.einsum('oc,bcp->bop', d['w'].double(), gx), None), mag)
        _report('pointwise', route, tag, 'y', ratio, i, qk, level)
    else:
        _report('pointwise', route, tag, 'y', ratio, i)


@gpu
@pytest.mark.parametrize('name,gen', PW_PARAMS)
def test_pointwise(dev, name, gen):
    _pw_run(dev, name, gen, 3, True, True)


@gpu
@pytest.mark.parametrize('act,gate,res', PW_OPTIONS)
@pytest.mark.parametrize('name', ['off 4 and 16', '64 pixels cin 96', 'vec 8256 pixels', 'nt2 8256 pixels'])
def test_pointwise_options(dev, name, act, gate, res):
    _pw_run(dev, name, 'benign', act, gate, res)


@gpu
def test_pointwise_refuses_what_its_route_refuses(dev):
    HF = _HF()
    _, b, cin, cout, p, _ = PW_CASES['cin 130 refused']
    assert HF.pointwise_route(b, cin, cout, p) is None
    with pytest.raises(Exception, match='unsupported shape'):
        HF.pointwise_conv(torch.zeros(b, cin, p, 1, device=dev), torch.zeros(cout, cin, device=dev))


AFFINE_CASES = [(2, 13, 60, 'benign'), (1, 12, 64, 'preact'), (2, 7, 4, 'quiet')]


def _affine_ref(ch, d, act, res, scale=True):
    return R.affine_act_ref(ch, d['residual'], d['scale'] if scale else None, d['shift'], act, d['x2'] if res else None)


def _affine_inputs(b, c, p, gen):
    d = R.pw_inputs(gen, b, 4, c, p, seed=b + c + p)          # 'residual' (B, C, P) is the tensor, 'x2' a second one for the skip add
    d['x2'] = torch.randn(b, c, p, generator=torch.Generator().manual_seed(p))
    return d


@pytest.mark.parametrize('b,c,p,gen', AFFINE_CASES)
@pytest.mark.parametrize('act', [0, 1, 2, 3])
def test_affine_restatement_within_bound(b, c, p, gen, act):
    d = _affine_inputs(b, c, p, gen)
    for res in (False, True):
        R.check(_affine_ref(R.Chain('f32'), d, act, res)[0], _affine_ref(R.Chain('bound'), d, act, res), f'{gen} act {act} res {res}')


@gpu
@pytest.mark.parametrize('b,c,p,gen', AFFINE_CASES)
@pytest.mark.parametrize('act', [0, 1, 2, 3])
def test_affine_act(dev, b, c, p, gen, act):
    HF = _HF()
    d = _affine_inputs(b, c, p, gen)
    g = _to(dev, d)
    for res in (False, True):
        for scale in (True, False):
            y = HF.affine_act_(g['residual'].clone().view(b, c, p, 1), g['scale'] if scale else None, g['shift'], act,
                               g['x2'].view(b, c, p, 1) if res else None)
            _report('affine_act', 'float4', f'{gen} act {act}{" res" if res else ""}{"" if scale else " no scale"}', 'y',
                    *R.check(y, _affine_ref(R.Chain('bound'), d, act, res, scale), f'{gen} act {act} res {res} scale {scale}'))


@gpu
def test_affine_act_refuses_pixels_off_4(dev):
    """hs_affine_act_fwd has no form for pixels % 4 != 0: the documented refusal, and x is left as it was."""
    x = torch.ones(1, 3, 3, 2, device=dev)
    with pytest.raises(Exception, match='unsupported shape'):
        _HF().affine_act_(x, torch.ones(3, device=dev), torch.ones(3, device=dev), 3)
    assert bool((x == 1).all())


# ------------------------------------------------------------------------------------------------------------ routes, teeth, ranges

def _codes():
    """Every answer the queries can give under the default environment (include/hyperseg_hip.h)."""
    dw = {f'tiled_k{k}s{s}' for k in (3, 5) for s in (1, 2)} | {f'generic_k{k}s{s}' for k in (3, 5) for s in (1, 2)} | {
        'vector_k3s1_pl1', 'vector_k3s2_pl0', 'vector_k3s2_pl1', 'vector_k5s1_pl2', 'vector_k5s2_pl1', 'vector_k5s2_pl2'}
    mb = {f'{f}_k{k}s{s}' for f in ('lean', 'full') for k in (3, 5) for s in (1, 2)} | {None}
    return dict(depthwise=dw, mbconv=mb, stem_dw={'stem_k3s1', None}, se_gate={'fused', 'early', 'two_launch'},      # 'fused_wide': compiled out
                pointwise={'vec', 'nt4', 'nt2', 'nt1', None})


ROUTE_COVERAGE = dict(depthwise={c[0] for c in DW_CASES.values()}, mbconv={c[0] for c in MB_CASES.values()},
                      stem_dw={c[0] for c in STEM_DW_CASES.values()}, se_gate={r for c in SE_CASES.values() for r in c[:2]},
                      pointwise={c[0] and c[0].split('_nb')[0] for c in PW_CASES.values()})


def test_route_coverage_table_names_every_code():
    assert ROUTE_COVERAGE == _codes()
    # what the codes leave out -- the unrolled depth of an instantiation, a function of c_in alone -- has a case each as well: the 1x1 conv's
    # NB = ceil(c_in / 16) in 1..8, the lean kernel's KS = c_in / 4 in {4, 6, 8, 10}, the general kernel's KS in {4, 6, 10, 12, 20}
    assert {int(c[0].split('_nb')[1]) for c in PW_CASES.values() if c[0]} == set(range(1, 9))
    ks = lambda form, steps: {next(k for k in steps if -(-c[2] // 4) <= k) for c in MB_CASES.values() if c[0] and c[0].startswith(form)}      # noqa: E731
    assert ks('lean', (4, 6, 8, 10)) == {4, 6, 8, 10} and ks('full', (4, 6, 10, 12, 20)) == {4, 6, 10, 12, 20}
    assert {c[0] for c in STEM_CASES.values()} == {'generic', 'vector_pl0', 'vector_pl1'}


def test_route_queries_answer_as_the_case_tables_expect():
    HF = _HF()
    for name, case in DW_CASES.items():
        route, shape, k, s, _, pl, out, pre = _dw_geom(case)
        assert HF.depthwise_route(shape, k, s, pl, out, prologue=pre) == route, name
        if route.startswith('vector'):               # a misaligned x (asked on the host only) and no prologue's tiles: the generic form
            assert HF.depthwise_route(shape, k, s, pl, out, prologue=pre, aligned=False) == f'generic_k{k}s{s}', name
    for name, case in MB_CASES.items():
        route, shape, cmid, k, s, _, _, out = _mb_geom(case)
        assert HF.mbconv_route(shape, cmid, k, s, out) == route, name
        if route and route.startswith('lean'):
            assert HF.mbconv_route(shape, cmid, k, s, out, aligned=False) == HF.mbconv_route(shape, cmid, k, s, out, se_tail=True) == 'full' + route[4:], name
    for name in STEM_DW_CASES:
        (route, b, cmid, h, w), (_, _, (pt, pl, hs, ws)) = STEM_DW_CASES[name][:5], _stem_dw_inputs(name)
        assert HF.stem_dw_route((h, w), cmid, pt, pl, (hs, ws)) == route, name
        assert HF.stem_dw_route((h, w), cmid, pt, pl, (hs, ws), k=5) is None and HF.stem_dw_route((h, w), cmid, pt, pl, (hs, ws), aligned=False) is None
    for name, (plain, proj, c, csq, nblk, _) in SE_CASES.items():
        assert (HF.se_gate_route(c, nblk, csq), HF.se_gate_route(c, nblk, csq, w_proj=True)) == (plain, proj), name
        if plain == 'early':
            assert HF.se_gate_route(c, nblk, csq, aligned=False) == 'two_launch', name
    for name, (route, b, cin, cout, p, _) in PW_CASES.items():
        assert HF.pointwise_route(b, cin, cout, p) == route, name
        if route and route.startswith('vec'):
            assert HF.pointwise_route(b, cin, cout, p, aligned=False) == 'nt4' + route[3:], name
    for name, (route, _, _, w, _, pads) in STEM_CASES.items():
        assert HF.stem_route(w, pads[1]) == route and HF.stem_route(w, pads[1], aligned=False) == 'generic', name
    assert HF.se_gate_route(8, 4, 70000) is None
    with pytest.raises(Exception):
        HF.depthwise_route((0, 1, 8, 8), 3, 1, 1, (8, 8))
    assert HF.depthwise_route((1, 4, 8, 8), 7, 1, 3, (8, 8)) is None


# defect -> a listed case on which the bound must reject it
def _teeth_dw(name, gen, defect, key='y'):
    _, _, k, s, pt, pl, out, _ = _dw_geom(DW_CASES[name])
    d, ref = _dw_ref(name, gen)
    got = R.depthwise_ref(R.Chain('f32', defect), d['x'], d['wt'], s, pt, pl, out, d['scale'], d['shift'], R.ACT_SWISH, d['in_scale'], d['in_shift'])
    return R.rejects(got[key][0], ref[key])


def _teeth_pw(name, gen, defect):
    d, ref, _, _ = _pw_ref(name, gen)
    return R.rejects(R.pointwise_ref(R.Chain('f32', defect), d['x'], d['w'], d['gate'], d['scale'], d['shift'], 3, d['residual'])[0], ref)


TEETH = {
    'pad_swish': lambda: _teeth_dw('v320 same', 'benign', 'pad_swish'),
    'pad_l_last_quad': lambda: _teeth_dw('v321 sym', 'benign', 'pad_l_last_quad'),
    'mean_padded_count': lambda: _teeth_dw('g31 odd W', 'benign', 'mean_padded_count', 'mean'),
    'pool_dead_rows': lambda: _teeth_dw('t51 40x32 dead rows', 'benign', 'pool_dead_rows', 'partial'),
    'gate_after_scale': lambda: _teeth_pw('off 4 and 16', 'benign', 'gate_after_scale'),
    'residual_before_act': lambda: _teeth_pw('off 4 and 16', 'benign', 'residual_before_act'),
    'exp2_no_log2e': lambda: _teeth_dw('g31 odd W', 'preact', 'exp2_no_log2e'),
}


@pytest.mark.parametrize('defect', R.DEFECTS)
def test_teeth(defect):
    assert TEETH[defect](), f'the bound accepts the defect {defect}'


def test_range_inputs_catch_what_benign_inputs_cannot():
    """sigmoid through exp2(t) instead of exp2(t log2 e) beyond |t| = 8: benign pre-activations never get there."""
    assert not _teeth_dw('g31 odd W', 'benign', 'exp2_no_log2e') and _teeth_dw('g31 odd W', 'preact', 'exp2_no_log2e')
    name, batch = 'channels % 4 != 0', 2
    for gen, caught in (('benign', False), ('pixel_sums', True)):
        d, ref, _, _ = _se_ref(name, batch, gen)
        got = R.se_gate_ref(R.Chain('f32', 'exp2_no_log2e'), d['partial'], batch, 1.0 / d['hw'], d['w1'], d['b1'], d['w2'], d['b2'])
        assert R.rejects(got['gate'][0], ref['gate']) == caught, gen


def test_references_are_finite_and_ranges_reach_their_regimes():
    for name, gen in [p for p in DW_PARAMS if DW_CASES[p[0]][2] < 4096]:
        _, ref = _dw_ref(name, gen)
        assert all(bool(torch.isfinite(t).all()) for k in ('y', 'partial', 'mean') for t in ref[k]), (name, gen)
    for name, gen in MB_PARAMS:
        assert all(bool(torch.isfinite(t).all()) for k in ('y', 'partial', 'mean') for t in _mb_ref(name, gen)[1][k]), (name, gen)
    for name, batch, gen in SE_PARAMS:
        d, ref, _, _ = _se_ref(name, batch, gen)
        assert all(bool(torch.isfinite(t).all()) for v in ref.values() for t in v), (name, gen)
        if gen == 'pixel_sums':
            assert 1e2 <= float(d['partial'].abs().max()) <= 2e4 and float(ref['gate'][0].min()) < 1e-9 and float(ref['gate'][0].max()) > 1 - 1e-9, name
    for name, gen in [p for p in PW_PARAMS if PW_CASES[p[0]][4] < 1000]:
        assert all(bool(torch.isfinite(t).all()) for t in _pw_ref(name, gen)[1]), (name, gen)
    d = R.dw_inputs('preact', 1, 13, 7, 9, 3, 0, True)
    pre = (d['x'] * d['in_scale'].view(1, -1, 1, 1) + d['in_shift'].view(1, -1, 1, 1))
    for i, p in enumerate(R.PREACTS):
        assert bool(((pre[:, i] - p).abs() <= 0.06 * abs(p)).all()), p
    assert float(_dw_ref('g31 odd W', 'quiet')[1]['y'][0][:, 1].abs().max()) < 1e-3 * float(_dw_ref('g31 odd W', 'quiet')[1]['y'][0][:, 0].abs().max())
