"""The decoder's forward kernels against float64, element by element, under the bound derived in util_decoder_ref.py -- and every case
first asserts the ROUTE and FORM it was written for (hs_patch_conv_route, hs_patch_ir_form, hs_patch_ir_v0_route: the launchers' own
predicates), so a threshold edit that moves a shape to another kernel fails here instead of silently dropping coverage.

CPU tests (unmarked): the fp32 restatement of every case lies inside its own bound, every defect of util_decoder_ref.DEFECTS is rejected,
one named defect passes the old tensor norm, the range inputs reach their regimes, the route queries answer as the case tables say and the
tables cover every code.  GPU tests (``-m gpu``): the kernels, each output inside guard bytes.  With HS_DECODER_F64_REPORT=<file> the GPU
run writes one line per case: the worst err / bound, its index, the worst err / mag64 (profiles/decoder_f64_bound.txt is such a run; nothing
here is tuned to it).  No tolerance in this file is a measured constant.

Decoder forward entry points and the test that reaches them:
  hs_patch_conv_fwd         test_patch_conv: all five routes (plain_dw3, plain_k1m, k1m, k1 at every PWL, tiled)
  hs_patch_ir_fwd           test_patch_ir: generic (five exact instantiations, four width classes, residual), f32_mfma (REG 8 and 16)
  hs_patch_ir_v0_ws_fwd     test_patch_ir_v0: d2 (4 x 4, 8 x 8), px, fused, and the unsupported answer
  hs_stage_input_fwd        test_stage_input
  hs_patch_ir_fwd, split_mfma   test_patch_ir_split (RH 8 and 16, one and two regions per patch, row and matrix scales, hid 96 -> 32),
                            test_split_out_of_range_contained, test_split_ir_ranges_f64 (the gains of test_split_ir_ranges at both of its shapes).
  hs_upsample_bilinear_fwd  test_upsample_bilinear;  hs_bn_fold_fwd  test_bn_fold;  hs_bank_pack_fwd  test_bank_pack_is_exact
  hs_patch_conv_gen_fwd, hs_signal2weights_fwd, hs_signal2weights_multi_fwd   test_signal2weights_and_patch_conv_gen (GEN_CASES)
  hs_meta_conv_fwd          test_meta_conv
  hs_k1_chain_fwd, hs_decoder_chain_fwd   left out on purpose: test_k1_chain_equals_the_three_launches ties them to the routes tested here.
  hs_patch_conv_s2w_fwd     the same kernel body as the k1 route with blocked signal2weights workgroups beside it; bit-identity to the
                            separate calls is test_hip_parity.py's.

Findings of writing the cases against the queries (kept as cases, with the route they really take):
  * The weight-stream form takes 2 x 2-pixel patches and EVEN channel counts only: one-pixel patches and cin = 19 at 1024 patches take 'k1'.
  * 1023 patches (grid 31 x 33) take 'k1'."""
import functools
import os

import pytest
import torch

import util_decoder_ref as R

gpu = pytest.mark.gpu
GENS = ('benign', 'range')


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.fail('these tests need the MI355X (torch.cuda.is_available() is False)')
    yield torch.device('cuda:0')
    # hand the module's blocks back: the guard buffers and the lru-cached cases' device copies are not for later modules to inherit
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


@functools.lru_cache(maxsize=None)
def _HF():
    from hyperseg_amd import functional
    return functional


_REPORT_STARTED = set()


def _report(kernel, route, name, ratio, index, rel):
    path = os.environ.get('HS_DECODER_F64_REPORT')
    if path:
        mode = 'a' if path in _REPORT_STARTED else 'w'
        _REPORT_STARTED.add(path)
        with open(path, mode) as f:
            f.write(f'{kernel:12s} {str(route):44s} {name:34s} worst err/bound {ratio:.4f} at {index}  worst err/mag64 {rel:.3e}\n')


GUARD = 64          # floats on either side of an output


def _guarded(dev, shape):
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + 2 * GUARD,), float('nan'), device=dev, dtype=torch.float32)
    bits = buf.view(torch.int32)
    bits[:GUARD] = 0x7fc0dead
    bits[-GUARD:] = 0x7fc0dead
    return buf, buf[GUARD:GUARD + n].view(shape)


def _guards_intact(buf):
    bits = buf.view(torch.int32)
    return bool((bits[:GUARD] == 0x7fc0dead).all()) and bool((bits[-GUARD:] == 0x7fc0dead).all())


def _run_guarded(dev, fn, shape):
    """``fn`` allocates its own output: run it, then copy through a guarded buffer is not a check of the kernel's stores -- so the
    output allocation itself is what is guarded: torch.empty is pointed at the guarded view for the duration of the call."""
    buf, view = _guarded(dev, shape)
    real_empty = torch.empty
    taken = []

    def empty(*size, **kw):
        size = tuple(size[0]) if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)) else tuple(size)
        if not taken and size == tuple(shape) and kw.get('dtype', torch.float32) == torch.float32 and str(kw.get('device', '')).startswith('cuda'):
            taken.append(1)
            return view
        return real_empty(*size, **kw)
    torch.empty = empty
    try:
        y = fn()
    finally:
        torch.empty = real_empty
    torch.cuda.synchronize()
    assert taken and y is not None and y.data_ptr() == view.data_ptr(), 'the output was not allocated inside the guards'
    assert _guards_intact(buf), 'guard bytes around the output were overwritten'
    return y


# ------------------------------------------------------------------------------------------------------------ patch_conv

def _ep(kind):
    return dict(none=(False, R.ACT_NONE), affine=(True, R.ACT_NONE), relu=(True, R.ACT_RELU), relu6=(True, R.ACT_RELU6))[kind]


# name -> (route, form, B, (H, W), c_skip, c_prev, coords, prev_size | None (half), grid, c_out, k, mode, groups, epilogue, ld padding)
CONV_CASES = {
    'k1 1x1 split1':        ('k1', 'pwl0_split1', 1, (3, 4), 1, 0, False, None, (3, 4), 260, 1, 'reflect', 1, 'none', 0),
    'k1 1x1 coords':        ('k1', 'pwl0_split4', 1, (3, 4), 5, 0, True, None, (3, 4), 6, 1, 'reflect', 1, 'affine', 0),
    'k1 2x2 prev':          ('k1', 'pwl1_split8', 2, (6, 8), 3, 4, True, None, (3, 4), 5, 1, 'reflect', 1, 'relu', 0),
    'k1 4x4 groups ld':     ('k1', 'pwl2_split2', 1, (8, 12), 4, 2, True, None, (2, 3), 6, 1, 'reflect', 2, 'relu6', 8),
    'k1 8x8 max split':     ('k1', 'pwl3_split2', 1, (8, 16), 3, 0, True, None, (1, 2), 2, 1, 'reflect', 1, 'none', 0),
    'k1 3x7 cin%split':     ('k1', 'pwl-1_split4', 1, (6, 21), 5, 0, False, None, (2, 3), 3, 1, 'reflect', 1, 'affine', 4),
    'k1 16x20':             ('k1', 'pwl-1_split1', 1, (16, 40), 2, 3, True, (16, 40), (1, 2), 4, 1, 'reflect', 1, 'relu6', 0),
    'k1 1px 1024 patches':  ('k1', 'pwl0_split16', 1, (32, 32), 18, 0, True, None, (32, 32), 9, 1, 'reflect', 1, 'relu', 0),
    'k1 odd cin 1024':      ('k1', 'pwl1_split2', 1, (64, 64), 8, 9, True, None, (32, 32), 20, 1, 'reflect', 1, 'relu', 0),
    'k1 1023 patches':      ('k1', 'pwl1_split1', 1, (62, 66), 8, 10, True, None, (31, 33), 40, 1, 'reflect', 1, 'relu', 0),
    'k1m rt3 al4 prev':     ('k1m', 'rt3_al4_prev1', 1, (64, 64), 8, 10, True, None, (32, 32), 40, 1, 'reflect', 1, 'relu', 0),
    'k1m rt6 al2':          ('k1m', 'rt6_al2_prev0', 1, (64, 64), 16, 0, True, None, (32, 32), 50, 1, 'reflect', 1, 'affine', 0),
    'k1m rt3 al2 prev':     ('k1m', 'rt3_al2_prev1', 2, (32, 64), 4, 4, True, None, (16, 32), 7, 1, 'reflect', 1, 'relu6', 0),
    'tiled k3 reflect':     ('tiled', 'th5_tw7_1x1', 1, (10, 21), 2, 2, True, None, (2, 3), 5, 3, 'reflect', 1, 'relu', 0),
    'tiled k3 zeros g2':    ('tiled', 'th4_tw6_1x1', 2, (8, 12), 4, 0, True, None, (2, 2), 4, 3, 'zeros', 2, 'none', 4),
    'tiled k5 replicate':   ('tiled', 'th6_tw5_1x1', 1, (6, 10), 3, 0, True, None, (1, 2), 3, 5, 'replicate', 1, 'affine', 0),
    'tiled k3 circular dw': ('tiled', 'th3_tw5_1x1', 1, (6, 10), 4, 0, True, None, (2, 2), 6, 3, 'circular', 6, 'relu6', 0),
    'tiled 70 columns':     ('tiled', 'th3_tw64_1x2', 1, (3, 70), 2, 0, True, None, (1, 1), 3, 3, 'reflect', 1, 'none', 0),
    'tiled lds split':      ('tiled', 'th24_tw48_2x1', 1, (48, 48), 14, 0, True, None, (1, 1), 4, 3, 'reflect', 1, 'none', 0),
    'plain k1m 16px':       ('plain_k1m', 'mt2_kq1_px1_affine', 1, (16, 30), 12, 0, False, None, (2, 2), 20, 1, 'reflect', 1, 'relu', 0),
    'plain k1m 21 wide':    ('plain_k1m', 'mt1_kq2_px1', 2, (8, 21), 20, 0, False, None, (1, 1), 9, 1, 'reflect', 1, 'none', 0),
    'plain k1m pairs':      ('plain_k1m', 'mt1_kq1_px2', 1, (16, 16), 7, 0, False, None, (1, 2), 5, 1, 'reflect', 1, 'none', 0),
    'plain dw3 even':       ('plain_dw3', 'pairs', 2, (8, 12), 5, 0, False, None, (2, 3), 5, 3, 'zeros', 5, 'none', 0),
    'plain dw3 odd':        ('plain_dw3', 'single', 1, (9, 15), 3, 0, False, None, (3, 5), 3, 3, 'zeros', 3, 'none', 0),
}
CONV_PARAMS = [(n, g) for n in CONV_CASES for g in GENS]


@functools.lru_cache(maxsize=None)
def _conv_case(name, gen):
    _, _, b, (h, w), cs, cp, coords, psize, grid, c_out, k, mode, groups, ep, ldpad = CONV_CASES[name]
    g = R.G(sum(map(ord, name)) * 2 + (gen == 'range'))
    cin = 2 * coords + cs + cp
    rows = c_out * (cin // groups) * k * k
    ld = (rows + 3) // 4 * 4 + ldpad
    d = dict(skip=R.randn(g, b, cs, h, w), coords=coords, grid=grid, c_out=c_out, k=k, mode=mode, groups=groups)
    if cp:
        d['prev'] = R.randn(g, b, cp, *(psize or (h // 2, w // 2)))
    bank = R.randn(g, b * grid[0] * grid[1], ld) * (cin // groups * k * k) ** -0.5
    affine, act = _ep(ep)
    if affine:
        d['scale'], d['shift'], d['act'] = 0.5 + torch.rand(c_out, generator=g), 0.3 * R.randn(g, c_out), act
    if gen == 'range':                      # per-channel input gains and per-row weight gains spanning powers of two; the BN undoes the rows'
        d['skip'] = d['skip'] * R.pow2_gains(g, cs, -6, 6).view(1, -1, 1, 1)
        gains = R.pow2_gains(g, c_out, -18, 0)
        gains[0], gains[-1] = 1.0, 2.0 ** -18
        bank[:, :rows] = (bank[:, :rows].view(-1, c_out, rows // c_out) * gains.view(1, -1, 1)).reshape(-1, rows)
        if affine:
            d['scale'] = d['scale'] / gains
    d['bank'] = bank
    return d


@functools.lru_cache(maxsize=None)
def _conv_ref(name, gen):
    return R.patch_conv_ref(_conv_case(name, gen))


def _conv_route(name, HF=None):
    _, _, b, (h, w), cs, cp, coords, psize, grid, c_out, k, mode, groups, ep, ldpad = CONV_CASES[name]
    cin = 2 * coords + cs + cp
    ld = (c_out * (cin // groups) * k * k + 3) // 4 * 4 + ldpad
    affine, act = _ep(ep)
    return (HF or _HF()).patch_conv_route((b, h, w), cs, cp, grid, c_out, k=k, padding=(k - 1) // 2, padding_mode=mode, groups=groups,
                                          scale=affine, act=act, coords=coords, prev_size=psize, ld=ld)


@pytest.mark.parametrize('name,gen', CONV_PARAMS)
def test_patch_conv_restatement_within_bound(name, gen):
    R.check(R.patch_conv(_conv_case(name, gen), torch.float32), _conv_ref(name, gen), f'{name} [{gen}]')


@gpu
@pytest.mark.parametrize('name,gen', CONV_PARAMS)
def test_patch_conv(dev, name, gen):
    HF = _HF()
    case = CONV_CASES[name]
    assert _conv_route(name) == case[:2], name
    d = _conv_case(name, gen)
    t = {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in d.items()}
    x = HF.StageInput(t['skip'], t.get('prev'), coords=d['coords']) if (d['coords'] or 'prev' in d) else t['skip']
    b, _, h, w = d['skip'].shape
    y = _run_guarded(dev, lambda: HF.patch_conv(x, d['grid'], t['bank'], d['c_out'], k=d['k'], padding=(d['k'] - 1) // 2, padding_mode=d['mode'],
                                                groups=d['groups'], scale=t.get('scale'), shift=t.get('shift'), act=d.get('act', 0)),
                     (b, d['c_out'], h, w))
    ratio, i, rel = R.check(y, _conv_ref(name, gen), f'{name} [{gen}]')
    _report('patch_conv', '/'.join(case[:2]), f'{name} [{gen}]', ratio, i, rel)


# ------------------------------------------------------------------------------------------------------------ patch_ir (Op C), patch_ir_v0 (Op D)

# name -> (route, form, B, (H, W), c_skip, c_prev, grid, hid, c_out, residual, coords)
IR_CASES = {
    'exact 24 6 16':     ('generic', 'exact_24_6_16_t1x1', 1, (6, 10), 6, 16, (2, 2), 12, 16, False, True),
    'exact 34 16 19':    ('generic', 'exact_34_16_19_t1x1', 1, (6, 10), 16, 16, (2, 2), 10, 19, False, True),
    'exact 14 4 8':      ('generic', 'exact_14_4_8_t1x1', 1, (16, 8), 4, 8, (2, 1), 9, 8, False, True),
    'exact 26 16 19':    ('generic', 'exact_26_16_19_t1x1', 2, (6, 10), 16, 8, (2, 2), 7, 19, False, True),
    'exact 22 4 12':     ('generic', 'exact_22_4_12_t1x1', 1, (3, 10), 4, 16, (1, 2), 11, 12, False, True),
    'class 16':          ('generic', 'class_16_0_16_t1x1', 1, (6, 10), 3, 4, (2, 2), 13, 5, False, True),
    'class 32':          ('generic', 'class_32_0_32_t1x1', 1, (8, 8), 9, 10, (1, 1), 18, 17, False, True),
    'class 64':          ('generic', 'class_64_0_32_t1x1', 1, (6, 10), 20, 14, (2, 2), 8, 6, False, True),
    'class 128':         ('generic', 'class_128_0_64_t1x1', 1, (6, 10), 40, 26, (2, 2), 8, 33, False, True),
    'residual':          ('generic', 'class_16_0_16_t1x1', 1, (6, 10), 9, 0, (2, 2), 13, 9, True, False),
    'tiles 2x2':         ('generic', 'class_16_0_16_t2x2', 1, (20, 18), 3, 4, (1, 1), 6, 5, False, True),
    'f32 reg8':          ('f32_mfma', 'reg8_pwr8_14_4_8', 1, (16, 24), 4, 8, (2, 3), 28, 8, False, True),
    'f32 reg8 24':       ('f32_mfma', 'reg8_pwr8_24_6_16', 1, (8, 16), 6, 16, (1, 2), 48, 16, False, True),
    'f32 reg16':         ('f32_mfma', 'reg16_pwr16_22_4_12', 1, (16, 32), 4, 16, (1, 2), 44, 12, False, True),
    'f32 4-byte bank':   ('f32_mfma', 'reg16_pwr16_24_6_16', 1, (16, 16), 6, 16, (1, 1), 48, 16, False, True),
}
IR_PARAMS = [(n, g) for n in IR_CASES for g in GENS]
# name -> (route, form, B, (H, W), c_skip, c_prev, grid, hid, c_out)
V0_CASES = {
    'd2 4x4 odd grid':   ('d2', 'pw4_rt6_al4_kq6', 1, (12, 20), 12, 34, (3, 5), 96, 12),
    'd2 4x4 1x1 grid':   ('d2', 'pw4_rt3_al2_kq1', 1, (4, 4), 3, 5, (1, 1), 16, 4),
    'd2 8x8 odd grid':   ('d2', 'pw8_rt3_al2_kq3', 1, (24, 8), 8, 12, (3, 1), 44, 8),
    'px 16x16':          ('px', '16_6_6', 1, (16, 32), 6, 8, (1, 2), 32, 6),
    'px 32x32':          ('px', '11_3_21', 1, (32, 32), 3, 6, (1, 1), 22, 21),
    'fused 16x16':       ('fused', 'reg16_pwr16_16_6_6', 1, (32, 16), 6, 8, (2, 1), 48, 6),
}
V0_UNSUPPORTED = ('unsupported', None, 1, (16, 32), 5, 8, (1, 2), 32, 6)
V0_PARAMS = [(n, g) for n in V0_CASES for g in GENS]


def _bn(g, n):
    return 0.5 + torch.rand(n, generator=g), 0.3 * R.randn(g, n)


def _ir_inputs(seed, gen, op, b, h, w, cs, cp, grid, hid, c_out, residual=False, coords=True, offset=0):
    """Benign: order-one activations that exercise both ReLU6 clamps.  Range: per-channel input gains and per-row pw1 / depthwise / pw3
    gains spanning powers of two with the following BatchNorm rescaled, so that the block computes the same function (as _op_c_case);
    Op D scales NEIGHBOURING patches' pw1 rows differently, so the ring's owner matters per element."""
    g = R.G(seed * 2 + (gen == 'range'))
    cin = 2 * coords + cs + cp
    r1, r2, r3 = cin * hid, cin * hid + 9 * hid, cin * hid + 9 * hid + hid * c_out
    ld = (r3 + 3) // 4 * 4
    P = b * grid[0] * grid[1]
    bank = torch.zeros(P, ld + 4)
    rows = bank[:, offset:offset + ld]                # offset = 1: a view 4 bytes off a 16-byte aligned allocation
    rows[:, :r1] = R.randn(g, P, r1) * 2.0 * cin ** -0.5
    rows[:, r1:r2] = R.randn(g, P, 9 * hid) * 0.7
    rows[:, r2:r3] = R.randn(g, P, hid * c_out) * hid ** -0.5
    d = dict(op=op, skip=R.randn(g, b, cs, h, w), coords=coords, grid=grid, hid=hid, c_out=c_out, residual=residual,
             bn1=(1.0 + torch.rand(hid, generator=g), 2.0 + R.randn(g, hid)), bn2=(1.0 + torch.rand(hid, generator=g), 2.0 + R.randn(g, hid)),
             bn3=_bn(g, c_out))
    if cp:
        d['prev'] = R.randn(g, b, cp, h // 2, w // 2)
    if gen == 'range':
        g1 = R.pow2_gains(g, P * hid, 2, 6).view(P, hid) if op == 'd' else R.pow2_gains(g, hid, -8, 4).view(1, hid).expand(P, hid)
        if op == 'd':                                  # one BN1 for all patches: the gain is carried by the patch, undone in the depthwise rows
            rows[:, :r1] = (rows[:, :r1].view(P, hid, cin) * g1.view(P, hid, 1)).reshape(P, r1)
            d['bn1'] = (d['bn1'][0] * 2.0 ** -4, d['bn1'][1])
        else:
            rows[:, :r1] = (rows[:, :r1].view(P, hid, cin) * g1.view(P, hid, 1)).reshape(P, r1)
            d['bn1'] = (d['bn1'][0] / g1[0], d['bn1'][1])
        g2 = R.pow2_gains(g, hid, -9, 3)
        rows[:, r1:r2] = (rows[:, r1:r2].view(P, hid, 9) * g2.view(1, hid, 1)).reshape(P, 9 * hid)
        d['bn2'] = (d['bn2'][0] / g2, d['bn2'][1])
        g3 = R.pow2_gains(g, c_out, -10, 0)
        rows[:, r2:r3] = (rows[:, r2:r3].view(P, c_out, hid) * g3.view(1, c_out, 1)).reshape(P, hid * c_out)
    d['bank'] = rows
    return d


@functools.lru_cache(maxsize=None)
def _ir_case(name, gen):
    table, op = (IR_CASES, 'c') if name in IR_CASES else (V0_CASES, 'd')
    c = table[name]
    b, (h, w), cs, cp, grid, hid, c_out = c[2:9]
    residual, coords = (c[9], c[10]) if op == 'c' else (False, True)
    return _ir_inputs(sum(map(ord, name)), gen, op, b, h, w, cs, cp, grid, hid, c_out, residual, coords, offset=1 if '4-byte' in name else 0)


@functools.lru_cache(maxsize=None)
def _ir_ref(name, gen):
    return R.patch_ir_ref(_ir_case(name, gen))


@pytest.mark.parametrize('name,gen', IR_PARAMS + V0_PARAMS)
def test_patch_ir_restatement_within_bound(name, gen):
    R.check(R.patch_ir(_ir_case(name, gen), torch.float32), _ir_ref(name, gen), f'{name} [{gen}]')


def _ir_form(name):
    route, form, b, (h, w), cs, cp, grid, hid, c_out, residual, coords = IR_CASES[name]
    return _HF().patch_ir_form((b, h, w), cs, cp, grid, hid, c_out, math='f32' if '4-byte' not in name else 'split', residual=residual, coords=coords,
                               bank_aligned='4-byte' not in name)


def _v0_route(c):
    _, _, b, (h, w), cs, cp, grid, hid, c_out = c
    return _HF().patch_ir_v0_route((b, h, w), cs, cp, grid, hid, c_out, workspace=True)


def _ir_operands(dev, d):
    HF = _HF()
    t = {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in d.items()}
    bank = d['bank']
    if bank.storage_offset():                         # keep the 4-byte offset of the view on the device
        base = torch.zeros(bank.shape[0], bank.shape[1] + 4, device=dev)
        base[:, 1:1 + bank.shape[1]] = bank.to(dev)
        t['bank'] = base[:, 1:1 + bank.shape[1]]
        assert t['bank'].data_ptr() % 16 == 4
    x = HF.StageInput(t['skip'], t.get('prev'), coords=d['coords']) if (d['coords'] or 'prev' in d) else t['skip']
    bns = [tuple(v.to(dev) for v in d[k]) for k in ('bn1', 'bn2', 'bn3')]
    return x, t['bank'], bns


@gpu
@pytest.mark.parametrize('name,gen', IR_PARAMS)
def test_patch_ir(dev, name, gen):
    HF = _HF()
    case = IR_CASES[name]
    assert _ir_form(name) == case[:2], name
    d = _ir_case(name, gen)
    x, bank, bns = _ir_operands(dev, d)
    b, _, h, w = d['skip'].shape
    math = 'split' if '4-byte' in name else 'f32'      # a bank 4 bytes off: asked for the split form, takes the direct kernels
    y = _run_guarded(dev, lambda: HF.patch_ir(x, d['grid'], bank, d['hid'], d['c_out'], *bns, residual=d['residual'], math=math), (b, d['c_out'], h, w))
    ratio, i, rel = R.check(y, _ir_ref(name, gen), f'{name} [{gen}]')
    _report('patch_ir', '/'.join(case[:2]), f'{name} [{gen}]', ratio, i, rel)


@gpu
@pytest.mark.parametrize('name,gen', V0_PARAMS)
def test_patch_ir_v0(dev, name, gen):
    HF = _HF()
    case = V0_CASES[name]
    assert _v0_route(case) == case[:2], name
    d = _ir_case(name, gen)
    x, bank, bns = _ir_operands(dev, d)
    b, _, h, w = d['skip'].shape
    y = _run_guarded(dev, lambda: HF.patch_ir_v0(x, d['grid'], bank, d['hid'], d['c_out'], *bns), (b, d['c_out'], h, w))
    ratio, i, rel = R.check(y, _ir_ref(name, gen), f'{name} [{gen}]')
    _report('patch_ir_v0', '/'.join(case[:2]), f'{name} [{gen}]', ratio, i, rel)


@gpu
def test_patch_ir_v0_refuses_what_its_route_refuses(dev):
    HF = _HF()
    _, _, b, (h, w), cs, cp, grid, hid, c_out = V0_UNSUPPORTED
    assert _v0_route(V0_UNSUPPORTED) is None
    d = _ir_inputs(5, 'benign', 'd', b, h, w, cs, cp, grid, hid, c_out)
    x, bank, bns = _ir_operands(dev, d)
    assert HF.patch_ir_v0(x, grid, bank, hid, c_out, *bns) is None


# ------------------------------------------------------------------------------------------------------------ Op C, split mode

# name -> (route, form prefix, regions per patch, B, (H, W), c_skip, c_prev, grid, hid, c_out): odd cin / hid take row scales, even ones matrix scales
SPLIT_CASES = {
    'split 8x16 odd':      ('split_mfma', 'rh8_nw4', 1, 1, (16, 48), 5, 8, (2, 3), 30, 9),
    'split 8x16 even':     ('split_mfma', 'rh8_nw4', 1, 1, (8, 16), 4, 8, (1, 1), 28, 8),
    'split 16x16 even':    ('split_mfma', 'rh16_nw4', 1, 1, (16, 32), 6, 16, (1, 2), 48, 16),
    'split 16x16 odd hid': ('split_mfma', 'rh16_nw4', 1, 2, (16, 16), 3, 4, (1, 1), 18, 5),
    'split 16x32 hid96':   ('split_mfma', 'rh16_nw4', 2, 1, (16, 32), 16, 16, (1, 1), 96, 32),
}
SPLIT_PARAMS = [(n, g) for n in SPLIT_CASES for g in GENS]


@functools.lru_cache(maxsize=None)
def _split_case(name, gen):
    _, _, _, b, (h, w), cs, cp, grid, hid, c_out = SPLIT_CASES[name]
    d = _ir_inputs(sum(map(ord, name)), 'benign', 'c', b, h, w, cs, cp, grid, hid, c_out)
    if gen == 'range':                     # the position scales' business: input magnitude varies by powers of two ALONG the row;
        g = R.G(sum(map(ord, name)) + 7)   # the weight scales': pw1 / pw3 rows 2^-4 .. 1 apart, BatchNorm rescaled (the same function)
        d['skip'] = d['skip'] * R.pow2_gains(g, w, -6, 6).view(1, 1, 1, w)
        d['prev'] = d['prev'] * R.pow2_gains(g, w // 2, -6, 6).view(1, 1, 1, w // 2)
        cin = 2 + cs + cp
        r1, r2 = cin * hid, cin * hid + 9 * hid
        g1, g3 = R.pow2_gains(g, hid, -4, 0), R.pow2_gains(g, c_out, -4, 0)
        bank = d['bank'].clone()
        bank[:, :r1] = (bank[:, :r1].view(-1, hid, cin) * g1.view(1, hid, 1) * 2.0 ** -3).reshape(-1, r1)
        bank[:, r2:r2 + hid * c_out] = (bank[:, r2:r2 + hid * c_out].view(-1, c_out, hid) * g3.view(1, c_out, 1)).reshape(-1, hid * c_out)
        d = dict(d, bank=bank, bn1=(d['bn1'][0] / g1, d['bn1'][1]), bn3=(d['bn3'][0] / g3, d['bn3'][1]))
    return d


@functools.lru_cache(maxsize=None)
def _split_ref(name, gen):
    return R.split_bound(_split_case(name, gen))


@pytest.mark.parametrize('name,gen', SPLIT_PARAMS)
def test_split_emulation_within_bound_and_every_reduction_in_range(name, gen):
    V = _split_ref(name, gen)
    keep = R.in_range(V)
    assert bool(keep.all()), f'{name} [{gen}]: {int((~keep).sum())} elements out of range: the share left out must be zero'
    R.check(R.split_emulate(_split_case(name, gen)), V, f'{name} [{gen}]')


def _split_check(got, d, V, what):
    """What a split-mode output is held to, on the GPU and in test_split_teeth alike: the derived split bound on every element (it
    carries its own floor term), and -- where in_range holds -- the second tier: twice the error level (relative to mag64) of the CPU
    emulation of the SAME case.  The chained bound sits 300 to 3000 times above what the arithmetic does; the second tier is what a
    dropped piece product or a wrong scale cannot pass."""
    keep = R.in_range(V)
    out = R.check_where(got, V, torch.ones_like(keep), what)
    level = R.q_level(torch.where(keep, R.split_emulate(d).double(), V['ref']), V)
    R.check_tier2(got, V, level, keep, what)
    return out


def _split_form(name):
    c = SPLIT_CASES[name]
    r = _HF().patch_ir_form((c[3],) + c[4], c[5], c[6], c[7], c[8], c[9], math='split')
    return r[0], r[1].rsplit('_', 2)[0], int(r[1].split('_')[2][1:])


@gpu
@pytest.mark.parametrize('name,gen', SPLIT_PARAMS)
def test_patch_ir_split(dev, name, gen):
    HF = _HF()
    case = SPLIT_CASES[name]
    assert _split_form(name) == case[:3], name
    d = _split_case(name, gen)
    x, bank, bns = _ir_operands(dev, d)
    b, _, h, w = d['skip'].shape
    y = _run_guarded(dev, lambda: HF.patch_ir(x, d['grid'], bank, d['hid'], d['c_out'], *bns, math='split'), (b, d['c_out'], h, w))
    ratio, i, rel = _split_check(y, d, _split_ref(name, gen), f'{name} [{gen}]')
    _report('patch_ir', '/'.join(map(str, case[:3])), f'{name} [{gen}]', ratio, i, rel)


# the inputs of test_hip_parity.py's test_split_ir_ranges, restated: (in_gain, w1_gain, w3_gain, w3_late_gain), BN rescaled as _op_c_case does
RANGE_GAINS = [(1.0, 1.0, 1.0, 1.0), (2.0 ** 12, 2.0 ** -9, 1.0, 1.0), (2.0 ** -20, 2.0 ** 14, 1.0, 1.0), (1.0, 1.0, 2.0 ** -12, 2.0 ** 9),
               (2.0 ** 16, 1.0, 2.0 ** 20, 1.0)]
# (route, form, (c_skip, c_prev), c_out, hid, patch, grid): the second shape's 8 x 8 patches are below the split form's 8 x 16
RANGE_SHAPES = [('split_mfma', 'rh16_nw4_r1_s4p4m2', (16, 16), 19, 78, 16, (2, 3)), ('f32_mfma', 'reg8_pwr8_24_6_16', (6, 16), 16, 48, 8, (3, 2))]


@functools.lru_cache(maxsize=None)
def _ranges_case(si, gi):
    _, _, (cs, cp), c_out, hid, patch, (fh, fw) = RANGE_SHAPES[si]
    in_gain, w1_gain, w3_gain, late = RANGE_GAINS[gi]
    cin, h, w = 2 + cs + cp, fh * patch, fw * patch
    g = R.G(11)
    skip, prev = R.randn(g, 1, cs, h, w) * in_gain, R.randn(g, 1, cp, h // 2, w // 2) * in_gain
    r1, r2 = cin * hid, cin * hid + 9 * hid
    wt = R.randn(g, 1, r2 + hid * c_out, fh, fw)
    wt[:, :r1] *= (2.0 / cin) ** 0.5 * w1_gain
    wt[:, :r1].view(1, hid, cin, fh, fw)[:, :, :2] *= in_gain          # the coordinates do not carry the input gain
    wt[:, r1:r2] *= (2.0 / 9) ** 0.5
    w3 = wt[:, r2:].view(1, c_out, hid, fh, fw)
    w3 *= (1.0 / hid) ** 0.5 * w3_gain
    w3[:, :, 32:] *= late
    bns = []
    for n, gain in ((hid, in_gain * w1_gain), (hid, 1.0), (c_out, 1.0)):
        wgt, bias = torch.rand(n, generator=g) + 0.5, R.randn(g, n) * 0.1
        mean, var = R.randn(g, n) * 0.1 * gain, (torch.rand(n, generator=g) * 1.5 + 0.5) * gain * gain
        sc = wgt / torch.sqrt(var + 1e-5)
        bns.append((sc, bias - mean * sc))
    rows = wt.shape[1]
    bank = torch.zeros(fh * fw, (rows + 3) // 4 * 4)
    bank[:, :rows] = wt.permute(0, 2, 3, 1).reshape(fh * fw, rows)
    return dict(op='c', skip=skip, prev=prev, coords=True, grid=(fh, fw), hid=hid, c_out=c_out, residual=False, bank=bank,
                bn1=bns[0], bn2=bns[1], bn3=bns[2])


@functools.lru_cache(maxsize=None)
def _ranges_ref(si, gi):
    return R.split_bound(_ranges_case(si, gi)) if si == 0 else R.patch_ir_ref(_ranges_case(si, gi))


RANGES_PARAMS = [(si, gi) for si in range(len(RANGE_SHAPES)) for gi in range(len(RANGE_GAINS))]


@pytest.mark.parametrize('si,gi', RANGES_PARAMS)
def test_split_ir_ranges_restatement_within_bound(si, gi):
    d, V = _ranges_case(si, gi), _ranges_ref(si, gi)
    assert bool(torch.isfinite(V['ref']).all()) and bool(torch.isfinite(V['bound']).all())
    if si == 0:
        assert not V['clamped']
        _split_check(R.split_emulate(d), d, V, f'ranges {si} {gi}')
    else:
        R.check(R.patch_ir(d, torch.float32), V, f'ranges {si} {gi}')


@gpu
@pytest.mark.parametrize('si,gi', RANGES_PARAMS)
def test_split_ir_ranges_f64(dev, si, gi):
    HF = _HF()
    route, form, (cs, cp), c_out, hid, patch, grid = RANGE_SHAPES[si]
    d = _ranges_case(si, gi)
    b, _, h, w = d['skip'].shape
    assert HF.patch_ir_form((1, h, w), cs, cp, grid, hid, c_out, math='split') == (route, form)
    x, bank, bns = _ir_operands(dev, d)
    y = _run_guarded(dev, lambda: HF.patch_ir(x, grid, bank, hid, c_out, *bns, math='split'), (1, c_out, h, w))
    V = _ranges_ref(si, gi)
    ratio, i, rel = _split_check(y, d, V, f'ranges {si} {gi}') if si == 0 else R.check(y, V, f'ranges {si} {gi}')
    keep = float(R.in_range(V).double().mean()) if si == 0 else 1.0
    _report('patch_ir', f'{route}/{form}', f'ranges gains {gi} (in_range {keep:.2f})', ratio, i, rel)


# ------------------------------------------------------------------------------------------------------------ signal2weights, patch_conv_gen, meta_conv

# test_hip_parity.py's GEN_CASES (grids already at most 4 x 8): skip, prev, c_out, patch, grid, batch, signal channels, groups
GEN_CASES = [(80, 0, 64, 1, (4, 8), 1, 416, 32), (28, 64, 32, 2, (4, 8), 1, 224, 16), (10, 32, 16, 4, (4, 8), 1, 128, 8),
             (10, 32, 16, 4, (3, 5), 2, 256, 32),          # a channel spans two groups; 30 patches
             (128, 0, 32, 1, (3, 4), 1, 576, 32), (5, 0, 7, 8, (2, 2), 1, 24, 3)]
GEN_PARAMS = [(i, g) for i in range(len(GEN_CASES)) for g in GENS]


@functools.lru_cache(maxsize=None)
def _gen_case(i, gen):
    cs_, cp, c_out, patch, (fh, fw), b, cs, groups = GEN_CASES[i]
    g = R.G(400 + 2 * i + (gen == 'range'))
    h, w, cin = fh * patch, fw * patch, 2 + cs_ + cp
    hp = c_out * cin
    wc = -(-hp // groups) * groups                       # rows padded to the group multiple, as the reference's Conv2d has them
    d = dict(signal=R.randn(g, b, 8 + cs + 5, fh, fw).clamp(min=0), wsw=R.randn(g, wc, cs // groups) * (groups / cs) ** 0.5, index=8, channels=cs,
             groups=groups, rows=hp, skip=R.randn(g, b, cs_, h, w), coords=True, grid=(fh, fw), c_out=c_out,
             scale=0.5 + torch.rand(c_out, generator=g), shift=0.1 * R.randn(g, c_out), act=R.ACT_RELU)
    if cp:
        d['prev'] = R.randn(g, b, cp, h // 2, w // 2)
    if gen == 'range':                                   # signal channels and generated rows spanning powers of two; the BN undoes the rows'
        d['signal'] = d['signal'] * R.pow2_gains(g, d['signal'].shape[1], -8, 8).view(1, -1, 1, 1)
        gains = R.pow2_gains(g, c_out, -12, 0)
        d['wsw'][:hp] = (d['wsw'][:hp].view(c_out, cin, -1) * gains.view(-1, 1, 1)).reshape(hp, -1)
        d['scale'] = d['scale'] / gains
    return d


def _layer(dev, d):
    return dict(wsw_t=d['wsw'].t().contiguous().to(dev), signal_index=d['index'], signal_channels=d['channels'], groups=d['groups'], rows=d['rows'])


@pytest.mark.parametrize('i,gen', GEN_PARAMS)
def test_gen_restatements_within_bound(i, gen):
    d = _gen_case(i, gen)
    R.check(R.s2w_bank(d['signal'], d['wsw'], d['index'], d['channels'], d['groups'], d['rows'], torch.float32), R.s2w_ref(d), f's2w {i} [{gen}]')
    R.check(R.patch_conv_gen(d, torch.float32), R.patch_conv_gen_ref(d), f'gen {i} [{gen}]')


@gpu
@pytest.mark.parametrize('i,gen', GEN_PARAMS)
def test_signal2weights_and_patch_conv_gen(dev, i, gen):
    """The bank of hs_signal2weights_fwd and of hs_signal2weights_multi_fwd per element (columns [rows, ld) are row padding that the
    launchers do not store and no consumer reads: not compared), then hs_patch_conv_gen_fwd, which never stores the bank."""
    HF = _HF()
    d = _gen_case(i, gen)
    V = R.s2w_ref(d)
    sig, layer = d['signal'].to(dev), _layer(dev, d)
    one = HF.signal2weights(sig, layer['wsw_t'], d['index'], d['channels'], d['groups'], d['rows'])
    ratio, idx, rel = R.check(one[:, :d['rows']], V, f's2w {i} [{gen}]')
    _report('s2w', 'single', f'gen case {i} [{gen}]', ratio, idx, rel)
    multi = HF.signal2weights_multi(sig, [layer])[0].bank
    ratio, idx, rel = R.check(multi[:, :d['rows']], V, f's2w multi {i} [{gen}]')
    _report('s2w', 'multi', f'gen case {i} [{gen}]', ratio, idx, rel)
    x = HF.StageInput(d['skip'].to(dev), d['prev'].to(dev) if 'prev' in d else None, coords=True)
    b, _, h, w = d['skip'].shape
    y = _run_guarded(dev, lambda: HF.patch_conv_gen(x, HF.SignalRef(sig, layer), d['c_out'], d['scale'].to(dev), d['shift'].to(dev), HF.ACT_RELU),
                     (b, d['c_out'], h, w))
    ratio, idx, rel = R.check(y, R.patch_conv_gen_ref(d), f'gen {i} [{gen}]')
    _report('conv_gen', 'gen', f'gen case {i} [{gen}]', ratio, idx, rel)


# name -> (B, c_in, (H, W), c_out, (kh, kw), stride, pad, dilation, mode, groups, epilogue, extra weight columns on either side)
META_CASES = {
    'zeros 3x3':          (2, 4, (7, 9), 5, (3, 3), (1, 1), (1, 1), (1, 1), 'zeros', 1, 'none', 0),
    'reflect 3x5 uneven': (1, 3, (8, 11), 4, (3, 5), (1, 1), (1, 2), (1, 1), 'reflect', 1, 'affine', 0),
    'replicate stride 2': (1, 4, (9, 10), 6, (3, 3), (2, 2), (1, 1), (1, 1), 'replicate', 2, 'relu', 0),
    'circular dilation 2': (2, 2, (8, 8), 3, (3, 2), (1, 1), (2, 1), (2, 2), 'circular', 1, 'relu6', 0),
    'zeros 1x4 s2 d2 dw': (1, 6, (6, 13), 6, (1, 4), (1, 2), (0, 3), (1, 2), 'zeros', 6, 'none', 0),
    'column range':       (2, 5, (5, 6), 3, (2, 2), (1, 1), (0, 0), (1, 1), 'zeros', 1, 'affine', 7),
}
META_PARAMS = [(n, g) for n in META_CASES for g in GENS]


@functools.lru_cache(maxsize=None)
def _meta_case(name, gen):
    b, cin, (h, w), c_out, k, stride, pad, dil, mode, groups, ep, extra = META_CASES[name]
    g = R.G(sum(map(ord, name)) * 2 + (gen == 'range'))
    n = (cin // groups) * k[0] * k[1]
    wide = R.randn(g, b, extra + c_out * n + extra) * n ** -0.5
    d = dict(x=R.randn(g, b, cin, h, w), c_out=c_out, k=k, stride=stride, pad=pad, dil=dil, mode=mode, groups=groups, extra=extra)
    affine, act = _ep(ep)
    if affine:
        d['scale'], d['shift'], d['act'] = 0.5 + torch.rand(c_out, generator=g), 0.3 * R.randn(g, c_out), act
    if gen == 'range':
        d['x'] = d['x'] * R.pow2_gains(g, cin, -6, 6).view(1, -1, 1, 1)
        gains = R.pow2_gains(g, c_out, -12, 0)
        wide[:, extra:extra + c_out * n] = (wide[:, extra:extra + c_out * n].view(b, c_out, n) * gains.view(1, -1, 1)).reshape(b, -1)
        if affine:
            d['scale'] = d['scale'] / gains
    d['wide'], d['w'] = wide, wide[:, extra:extra + c_out * n]
    return d


@pytest.mark.parametrize('name,gen', META_PARAMS)
def test_meta_conv_restatement_within_bound(name, gen):
    d = _meta_case(name, gen)
    R.check(R.meta_conv(d, torch.float32), R.meta_conv_ref(d), f'{name} [{gen}]')


@gpu
@pytest.mark.parametrize('name,gen', META_PARAMS)
def test_meta_conv(dev, name, gen):
    HF = _HF()
    d = _meta_case(name, gen)
    V = R.meta_conv_ref(d)
    wide = d['wide'].to(dev)
    w = wide[:, d['extra']:d['extra'] + d['w'].shape[1]]            # a column range of the wider tensor, read in place
    y = _run_guarded(dev, lambda: HF.meta_conv(d['x'].to(dev), w, d['c_out'], d['k'], d['stride'], d['pad'], d['dil'], d['mode'], d['groups'],
                                               d['scale'].to(dev) if 'scale' in d else None, d['shift'].to(dev) if 'shift' in d else None,
                                               d.get('act', 0)), tuple(V['ref'].shape))
    ratio, i, rel = R.check(y, V, f'{name} [{gen}]')
    _report('meta_conv', d['mode'], f'{name} [{gen}]', ratio, i, rel)


def _out_of_range_case():
    """One skip channel 2^20 above its position's other channels in the left half of the first patch, meeting pw1 rows 2^-20 of the matrix maximum."""
    d = dict(_split_case('split 16x16 even', 'benign'))
    skip = d['skip'].clone()
    skip[:, 0, :, :8] *= 2.0 ** 20
    cin, hid = 24, 48
    bank = d['bank'].clone()
    w1 = bank[:, :cin * hid].view(-1, hid, cin)
    w1[0, 1::2] *= 2.0 ** -20                       # the first patch only: the second stays in range
    d.update(skip=skip, bank=bank)
    return d


def test_out_of_range_inputs_are_named_by_in_range():
    V = R.split_bound(_out_of_range_case())
    keep = R.in_range(V)
    assert not bool(keep.all()) and bool(keep.any())
    R.check_where(R.split_emulate(_out_of_range_case()), V, keep, 'out of range, emulated')


@gpu
def test_split_out_of_range_contained(dev):
    """Inputs out of range on purpose: outputs stay finite and every violation of the bound lies where in_range is false."""
    HF = _HF()
    d = _out_of_range_case()
    assert HF.patch_ir_form((1, 16, 32), 6, 16, (1, 2), 48, 16, math='split')[0] == 'split_mfma'
    x, bank, bns = _ir_operands(dev, d)
    y = _run_guarded(dev, lambda: HF.patch_ir(x, d['grid'], bank, d['hid'], d['c_out'], *bns, math='split'), (1, 16, 16, 32))
    V = R.split_bound(d)
    R.check_where(y, V, R.in_range(V), 'out of range')


@gpu
def test_patch_ir_v0_fused_reg8_without_a_workspace(dev, monkeypatch):
    """48 + 12 -> 12 on 4 x 4 patches takes the fused matrix-core form (8 x 8 regions of 2 x 2 patches) only when the call passes no workspace."""
    HF = _HF()
    args = (1, 8, 16, 12, 34, (2, 4), 96, 12)
    assert HF.patch_ir_v0_route((1, 8, 16), 12, 34, (2, 4), 96, 12, workspace=False) == V0_REG8
    monkeypatch.setattr(HF, 'D2_ROUTE', False)
    for gen in GENS:
        d = _ir_inputs(79, gen, 'd', *args)
        x, bank, bns = _ir_operands(dev, d)
        y = _run_guarded(dev, lambda: HF.patch_ir_v0(x, d['grid'], bank, d['hid'], d['c_out'], *bns), (1, 12, 8, 16))
        ratio, i, rel = R.check(y, R.patch_ir_ref(d), f'fused reg8 [{gen}]')
        _report('patch_ir_v0', '/'.join(V0_REG8), f'fused reg8 [{gen}]', ratio, i, rel)


def test_fused_reg8_restatement_within_bound():
    for gen in GENS:
        d = _ir_inputs(79, gen, 'd', 1, 8, 16, 12, 34, (2, 4), 96, 12)
        R.check(R.patch_ir(d, torch.float32), R.patch_ir_ref(d), f'fused reg8 [{gen}]')


V0_REG8 = ('fused', 'reg8_pwr4_48_12_12')


# ------------------------------------------------------------------------------------------------------------ upsample, bn_fold, bank_pack

# (B, C, (Hi, Wi), (Ho, Wo)): exact 2x, odd sizes at a non-2x ratio, a 1 x 1 source, downscale
UP_CASES = [(2, 3, (5, 7), (10, 14)), (1, 2, (5, 7), (13, 9)), (1, 3, (1, 1), (4, 6)), (1, 2, (9, 11), (4, 5)), (1, 1, (3, 5), (7, 31))]


def _up_case(i, gen):
    b, c, si, so = UP_CASES[i]
    g = R.G(300 + 2 * i + (gen == 'range'))
    p = R.randn(g, b, c, *si)
    return (p * R.pow2_gains(g, c, -12, 12).view(1, -1, 1, 1) if gen == 'range' else p), so


def _up_ref(p, so):
    return dict(ref=R.upsample(p.double(), so), bound=R.upsample_err(p, so), mag=R.upsample(p.double().abs(), so))


@pytest.mark.parametrize('i', range(len(UP_CASES)))
@pytest.mark.parametrize('gen', GENS)
def test_upsample_restatement_within_bound(i, gen):
    p, so = _up_case(i, gen)
    R.check(R.upsample(p, so, torch.float32), _up_ref(p, so), f'upsample {i} [{gen}]')


@gpu
@pytest.mark.parametrize('i', range(len(UP_CASES)))
@pytest.mark.parametrize('gen', GENS)
def test_upsample_bilinear(dev, i, gen):
    HF = _HF()
    p, so = _up_case(i, gen)
    buf, view = _guarded(dev, p.shape[:2] + so)
    y = HF.upsample_bilinear(p.to(dev), so, out=view)
    torch.cuda.synchronize()
    assert _guards_intact(buf)
    ratio, idx, rel = R.check(y, _up_ref(p, so), f'upsample {i} [{gen}]')
    _report('upsample', '2x' if so == (2 * p.shape[2], 2 * p.shape[3]) else 'general', f'upsample {i} [{gen}]', ratio, idx, rel)


@gpu
@pytest.mark.parametrize('n', [1, 19, 257])
def test_bn_fold(dev, n):
    """scale = gamma / sqrt(var + eps), shift = beta - mean * scale: var + eps, sqrt, the division, the product and the difference round once
    each -- scale within 4 * 2^-24 of itself (first order, doubled: 2^-21), shift within 2^-23 (|beta| + |mean scale|) + |mean| d scale."""
    HF = _HF()
    g = R.G(n)
    gamma, beta, mean = R.randn(g, n) * R.pow2_gains(g, n, -8, 8), R.randn(g, n), R.randn(g, n) * R.pow2_gains(g, n, -8, 8)
    var = torch.rand(n, generator=g) * R.pow2_gains(g, n, -20, 8)
    scale, shift = HF.bn_fold(gamma.to(dev), beta.to(dev), mean.to(dev), var.to(dev), 1e-5)
    s64 = gamma.double() / torch.sqrt(var.double() + float(torch.tensor(1e-5, dtype=torch.float32)))
    ds = 2.0 ** -21 * s64.abs()
    R.check(scale, dict(ref=s64, bound=ds), 'bn_fold scale')
    R.check(shift, dict(ref=beta.double() - mean.double() * s64, bound=2.0 ** -22 * (beta.double().abs() + (mean.double() * s64).abs()) + mean.double().abs() * ds
                        + 1e-300), 'bn_fold shift')


@gpu
@pytest.mark.parametrize('b,hp,grid,off,rows', [(1, 7, (3, 5), 0, 7), (2, 40, (2, 3), 5, 30), (1, 9, (1, 1), 8, 1)])
def test_bank_pack_is_exact(dev, b, hp, grid, off, rows):
    """bank[p ld + m] = w[b, off + m, i, j]: a copy, compared bit for bit."""
    HF = _HF()
    w = R.randn(R.G(hp), b, hp, *grid)
    bank = HF.bank_pack(w.to(dev), off, rows).cpu()
    want = w[:, off:off + rows].permute(0, 2, 3, 1).reshape(-1, rows)
    assert torch.equal(bank[:, :rows], want)


# ------------------------------------------------------------------------------------------------------------ stage input

# (B, (H, W), c_skip, c_prev, prev size, coords)
STAGE_CASES = [(1, (5, 7), 3, 2, (5, 7), True), (2, (6, 10), 1, 3, (3, 5), True), (1, (7, 9), 2, 2, (1, 1), True), (1, (9, 5), 2, 3, (4, 3), False),
               (1, (1, 6), 1, 0, None, True)]


def _stage_case(i, gen):
    b, (h, w), cs, cp, ps, coords = STAGE_CASES[i]
    g = R.G(100 + 2 * i + (gen == 'range'))
    skip, prev = R.randn(g, b, cs, h, w), (R.randn(g, b, cp, *ps) if cp else None)
    if gen == 'range' and prev is not None:
        prev = prev * R.pow2_gains(g, cp, -12, 12).view(1, -1, 1, 1)
    return skip, prev, coords


def _stage_ref(skip, prev, coords):
    dt = torch.float64
    return dict(ref=R.stage(skip, prev, coords, dt), bound=R.stage(skip, prev, coords, dt, role='err'), mag=R.stage(skip, prev, coords, dt, role='abs'))


def test_upsample_statement_is_interpolate():
    g = R.G(3)
    p = R.randn(g, 2, 3, 5, 7).double()
    for size in ((10, 14), (9, 4), (5, 7), (13, 20)):
        want = torch.nn.functional.interpolate(p, size, mode='bilinear', align_corners=False)
        assert float((R.upsample(p, size) - want).abs().max()) < 1e-14


@pytest.mark.parametrize('i', range(len(STAGE_CASES)))
@pytest.mark.parametrize('gen', GENS)
def test_stage_restatement_within_bound(i, gen):
    skip, prev, coords = _stage_case(i, gen)
    R.check(R.stage(skip, prev, coords, torch.float32), _stage_ref(skip, prev, coords), f'stage {i} [{gen}]')


@gpu
@pytest.mark.parametrize('i', range(len(STAGE_CASES)))
@pytest.mark.parametrize('gen', GENS)
def test_stage_input(dev, i, gen):
    HF = _HF()
    skip, prev, coords = _stage_case(i, gen)
    st = HF.StageInput(skip.to(dev), prev.to(dev) if prev is not None else None, coords=coords)
    y = _run_guarded(dev, st.materialize, tuple(st.shape))
    ratio, idx, rel = R.check(y, _stage_ref(skip, prev, coords), f'stage {i} [{gen}]')
    _report('stage_input', 'plane', f'stage {i} [{gen}]', ratio, idx, rel)


# ------------------------------------------------------------------------------------------------------------ coverage, teeth, regimes

# every code the new queries can return, by the launchers' own dispatch tables; UNCLAIMED: named here, run by no case of this file
CONV_CODES = {('plain_dw3', 'pairs'), ('plain_dw3', 'single'), ('plain_k1m', 'px1'), ('plain_k1m', 'px2'), ('plain_k1m', 'px1_affine'),
              ('k1m', 'rt3_al4'), ('k1m', 'rt6_al2'), ('k1m', 'rt3_al2'), ('k1', 'pwl0'), ('k1', 'pwl1'), ('k1', 'pwl2'), ('k1', 'pwl3'),
              ('k1', 'pwl-1'), ('tiled', '1x1'), ('tiled', '1x2'), ('tiled', '2x1')}
IR_CODES = {('generic', f'exact_{a}_{b}_{c}') for a, b, c in ((24, 6, 16), (34, 16, 19), (14, 4, 8), (26, 16, 19), (22, 4, 12))} | \
           {('generic', f'class_{a}_0_{c}') for a, c in ((16, 16), (32, 32), (64, 32), (128, 64))} | \
           {('f32_mfma', 'reg8'), ('f32_mfma', 'reg16')}
SPLIT_CODES = {('split_mfma', 'rh8_nw4'), ('split_mfma', 'rh16_nw4')}
V0_CODES = {('d2', 'pw4'), ('d2', 'pw8'), ('px', '16_6_6'), ('px', '11_3_21'), ('fused', 'reg16'), ('fused', 'reg8'), ('unsupported', None)}


def _conv_code(route, form):
    parts = form.split('_')
    if route == 'plain_k1m':
        return route, '_'.join(parts[2:])
    if route == 'k1m':
        return route, '_'.join(parts[:2])
    if route == 'k1':
        return route, parts[0]
    if route == 'tiled':
        return route, parts[-1]
    return route, form


def _ir_code(route, form):
    if form is None:
        return route, form
    if route in ('f32_mfma', 'fused'):
        return route, form.split('_')[0]
    if route == 'generic':
        return route, form.rsplit('_', 1)[0]
    if route == 'd2':
        return route, form.split('_')[0]
    return route, form


def test_route_coverage_table_names_every_code():
    assert {_conv_code(*c[:2]) for c in CONV_CASES.values()} == CONV_CODES
    assert {_ir_code(*c[:2]) for c in IR_CASES.values()} == IR_CODES
    assert {_ir_code(*c[:2]) for c in V0_CASES.values()} | {_ir_code(*V0_UNSUPPORTED[:2]), _ir_code(*V0_REG8)} == V0_CODES
    assert {c[:2] for c in SPLIT_CASES.values()} == SPLIT_CODES
    assert {c[2] for c in SPLIT_CASES.values()} == {1, 2}, 'regions per patch'
    assert any(c[9] for c in IR_CASES.values()), 'residual=True on the generic route'
    assert {CONV_CASES[n][13] for n in CONV_CASES if CONV_CASES[n][0] == 'k1'} == {'none', 'affine', 'relu', 'relu6'}
    assert {CONV_CASES[n][11] for n in CONV_CASES if CONV_CASES[n][0] == 'tiled'} == {'zeros', 'reflect', 'replicate', 'circular'}


def test_route_queries_answer_as_the_case_tables_expect():
    """The launchers' predicates, asked on the host: every case takes the route and form its row names (the GPU tests assert it again)."""
    for name, c in CONV_CASES.items():
        assert _conv_route(name) == c[:2], name
    for name, c in IR_CASES.items():
        assert _ir_form(name) == c[:2], name
    for name, c in V0_CASES.items():
        assert _v0_route(c) == c[:2], name
    assert _v0_route(V0_UNSUPPORTED) is None
    for name, c in SPLIT_CASES.items():
        assert _split_form(name) == c[:3], name
    HF = _HF()
    # the forms this file does not run are still what the queries say they are
    assert HF.patch_ir_form((1, 16, 32), 6, 16, (1, 2), 48, 16, math='split') == ('split_mfma', 'rh16_nw4_r1_s2p4m1')
    assert HF.patch_ir_form((1, 8, 16), 6, 16, (1, 1), 48, 16, math='split') == ('split_mfma', 'rh8_nw4_r1_s2p4m1')
    assert HF.patch_ir_form((1, 16, 32), 6, 16, (1, 2), 48, 16, math='split', bank_aligned=False)[0] == 'f32_mfma'
    assert HF.patch_ir_v0_route((1, 8, 16), 12, 34, (2, 4), 96, 12, workspace=False) == ('fused', 'reg8_pwr4_48_12_12')
    assert HF.patch_ir_route((1, 16, 32), 6, 16, (1, 2), 48, 16, math='auto') == 'split_mfma'


def _teeth_conv(name, gen, defect):
    return R.patch_conv(_conv_case(name, gen), torch.float32, defect), _conv_ref(name, gen)


def _teeth_ir(name, gen, defect):
    return R.patch_ir(_ir_case(name, gen), torch.float32, defect), _ir_ref(name, gen)


TEETH = {
    'drop_last_k': [lambda: _teeth_conv('k1 2x2 prev', 'benign', 'drop_last_k'), lambda: _teeth_ir('class 16', 'benign', 'drop_last_k')],
    'drop_last_k_last_row': [lambda: _teeth_conv('k1 8x8 max split', 'range', 'drop_last_k_last_row')],
    'halo_corner_off_by_one': [lambda: _teeth_conv('tiled k3 reflect', 'benign', 'halo_corner_off_by_one'),
                               lambda: _teeth_ir('class 16', 'range', 'halo_corner_off_by_one')],
    'ring_own_weights': [lambda: _teeth_ir('d2 4x4 odd grid', 'range', 'ring_own_weights')],
    'bn_relu6_order': [lambda: _teeth_conv('k1 4x4 groups ld', 'benign', 'bn_relu6_order'), lambda: _teeth_ir('exact 14 4 8', 'benign', 'bn_relu6_order')],
    'prev_half_pixel': [lambda: _teeth_conv('k1 2x2 prev', 'benign', 'prev_half_pixel')],
    'ld_ignored': [lambda: _teeth_conv('k1 4x4 groups ld', 'benign', 'ld_ignored')],
}


@pytest.mark.parametrize('defect', R.SPLIT_DEFECTS)
def test_split_teeth(defect):
    """'split_low_dropped': the al * bh product of pw1 left out; 'scale_wrong_column': a halo position's input scale taken from its left
    neighbour (rejected on the range set, whose input magnitude varies along the row)."""
    for name, gen in (('split 16x16 even', 'range'), ('split 8x16 odd', 'range')):
        d, V = _split_case(name, gen), _split_ref(name, gen)
        _split_check(R.split_emulate(d), d, V, name)                 # the un-defected emulation passes the GPU test's own check
        with pytest.raises(AssertionError):
            _split_check(R.split_emulate(d, defect), d, V, f'{name} {defect}')


@pytest.mark.parametrize('defect', R.DEFECTS)
def test_teeth(defect):
    assert defect in TEETH
    for make in TEETH[defect]:
        got, V = make()
        assert R.rejects(got, V), defect


def test_a_defect_the_tensor_norm_cannot_see():
    """'drop_last_k_last_row' on the range set of 'k1 8x8 max split': the last output row's weights are 2^-18 of the first row's, and its
    last K term is dropped.  The whole channel is wrong by about a tenth of itself; the tensor norm of test_hip_parity.py
    (max|a - b| / max|b| < 2e-5) passes it, the per-element bound rejects it.  On the benign set both see it."""
    got, V = _teeth_conv('k1 8x8 max split', 'range', 'drop_last_k_last_row')
    assert R.rejects(got, V)
    assert R.old_rel_err(got, V['ref']) < 2e-5
    got, V = _teeth_conv('k1 8x8 max split', 'benign', 'drop_last_k_last_row')
    assert R.rejects(got, V) and R.old_rel_err(got, V['ref']) > 2e-5


def test_references_are_finite_and_ranges_reach_their_regimes():
    for name, gen in IR_PARAMS + V0_PARAMS:
        d = _ir_case(name, gen)
        ref, h1, h2, _ = R.patch_ir(d, parts=True)
        assert bool(torch.isfinite(ref).all()), name
        for t in (h1, h2):                            # ReLU6 saturated on both sides
            assert bool((t == 0).any()) and bool((t == 6).any()), (name, gen)
    for name, gen in CONV_PARAMS:
        V = _conv_ref(name, gen)
        assert bool(torch.isfinite(V['ref']).all()) and bool((V['bound'] > 0).all()), name
    chan = _conv_ref('k1 8x8 max split', 'range')['ref'].abs().amax((0, 2, 3))
    assert float(chan.max() / chan.min()) > 2 ** 10, 'the range set spreads the output channels'
