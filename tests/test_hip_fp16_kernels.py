"""Kernel-level tests of the f16_t instantiation of every storage-typed training kernel, each against a float64 statement of the same
operation (tests/util_f16_ref.py) under an ELEMENTWISE bound derived from the number formats:

    |got - ref64| <= 2^-11 |ref64| + 2^-24 + (terms + 2) 2^-23 mag64

``ref64`` is the float64 value, ``mag64`` the same statement on absolute values, ``terms`` the products per output.  An fp32 sum of n
products, in any order, fused or not, is within gamma_n <= (n + 2) 2^-23 of mag64; the single round-to-nearest to binary16 adds half an
ulp: at most 2^-11 |ref64|, or 2^-24 (half the smallest subnormal) below the normal range.  fp32 outputs (bank gradients, BatchNorm's
weight / bias gradients and statistics, losses) drop the first two terms.  Nothing in it is measured.  Every input is drawn on the CPU
with G(seed) and rounded to binary16 first, so the reference sees exactly the numbers the kernel sees.  A norm at half-type resolution
says little about one element -- a swapped pair of a Pair<f16_t> 4-byte store passes 1e-2 relative L2 of a whole step; it does not pass
this (test_the_bound_rejects_one_moved_element_and_a_swapped_pair).

Where a result goes through two kernels the first one's bound is pushed through the second on absolute values (``extra64``), the
binary16 store between them is repeated in the reference at the same point, and the terms whose ReLU6 unit is undecided within the
pre-activation's bound may count or not (util_f16_ref.bn_train_ref / bn_linear_ref state each step).

Exported entry points reached, f16_t arm (dtype code 2), by test:
  test_halo_tiles_and_interior_f16          hs_halo_tiles_fwd / _bwd (both layouts; adjoint by tile and by patch), hs_tile_interior_fwd / _bwd
  test_dw_tiles_valid_f16                   hs_dw_tiles_fwd / _bwd_in / _bwd_w (both layouts)
  test_patch_dw3_f16                        hs_patch_conv_plain_fwd / _bwd_in / _bwd_w, depthwise 3x3 (pair and single-element forms), hs_bank_pack_fwd / hs_bank_unpack_fwd
  test_patch_k1_f16                         hs_patch_conv_plain_fwd / _bwd_in / _bwd_w, k = 1 (matrix-core *_k1m_kernel with quad_ld(f16_t), tiny-patch forms)
  test_bn_act_train_f16                     hs_bn_act_train_fwd / _bwd (one-launch and two-launch forms, pair mode and single elements)
  test_dw_tiles_bn_f16                      hs_bn_train_stats_fwd, hs_dw_tiles_bn_fwd / _bwd_w / _bwd_in, hs_bn_act_train_bwd_apply; two-step: hs_bn_act_train_*, hs_dw_tiles_*
  test_patch_conv_bn_f16                    hs_bn_train_stats_fwd, hs_patch_conv_bn_fwd / _bwd_w, hs_patch_conv_plain_bwd_in, hs_bn_act_train_bwd
  test_stage_input_f16                      hs_stage_input_typed_fwd, hs_upsample_bilinear_typed_bwd
  test_fused_bootstrapped_cross_entropy_f16 hs_bootstrapped_ce_fwd / _bwd, hs_cross_entropy_typed_fwd / _bwd, hs_bootstrap_mean_of_batch_fwd / _bwd
  test_overflow_and_nan_*                   Pair<f16_t>::st (hs_dw_tiles_fwd, depthwise hs_patch_conv_plain_bwd_in, hs_bn_act_train_bwd), Store<f16_t>::st
                                            (odd-width depthwise), the k1m epilogue; hs_adam_step_amp after such a backward
  (tests/test_hip_training.py test_bank_slices_share_one_gradient_buffer[fp16]: the BankSlices views under fp16 autocast)

f16_t arms left without a test of this kind, and why:
  * hs_patch_conv_plain_* general k x k (groups = 1, reflect): the issue lists the depthwise, k = 1 and tiny-patch forms only; it stays under
    test_patch_conv_f16_storage_vs_fp32_oracle (relative L2).
  * hs_upsample_bilinear_f16_fwd and the non-2x hs_upsample_bilinear_typed_bwd: bit-equal to the fp32 kernel rounded once in
    test_f16_storage_twins_round_the_fp32_kernels_once, which is stronger than a bound.
  * hs_bn_act_train_* with ReLU (act code 1): none and ReLU6 are run here; ReLU shares ReLU6's code path up to the upper clamp."""
import copy

import pytest
import torch

import util_f16_ref as R
from conftest import G

F16 = torch.float16
D = torch.float64


def h16(t):
    """Rounded to binary16 (what the kernel will read), kept as the fp16 tensor."""
    return t.half()


def randn16(seed, *shape, scale=1.0, shift=0.0):
    return h16(torch.randn(*shape, generator=G(seed)) * scale + shift)


HALO_SHAPES = [((1, 3, 8, 12), (4, 3)), ((1, 2, 6, 6), (6, 6)), ((1, 1, 2, 2), (1, 1)), ((2, 3, 12, 8), (3, 2)), ((1, 3, 4, 64), (1, 1)),
               ((1, 7, 16, 24), (2, 3))]
DW_TILES_SHAPES = [(1, 7, (1, 1), (3, 70)), (2, 4, (2, 2), (1, 6)), (2, 3, (3, 5), (5, 2)), (1, 44, (2, 3), (8, 8))]
DW3_CASES = [dict(c=6, b=1, grid=(2, 3), patch=(6, 7)), dict(c=3, b=2, grid=(3, 5), patch=(4, 2)), dict(c=5, b=1, grid=(1, 1), patch=(5, 70))]
K1_CASES = [dict(cin=5, cout=3, grid=(1, 2), patch=(4, 12)), dict(cin=6, cout=20, grid=(2, 2), patch=(3, 7)),
            dict(cin=17, cout=33, grid=(2, 1), patch=(16, 20)), dict(cin=94, cout=32, grid=(2, 2), patch=(4, 4)),
            dict(cin=82, cout=64, grid=(4, 6), patch=(1, 1))]
# hs_bn_act_train_fwd / _bwd (hs_train_aux.hip) have no query; their conditions, quoted:
#     const bool small = (long)batch * pixels <= BN_SMALL_MAX;              // one launch: a workgroup per channel     (BN_SMALL_MAX = 16 * 1024)
#     bn_pairs_ok(a): (a.HW & 1) == 0 && a.HW >= 256   [and 4-byte aligned tensors]                                    (the two-launch kernels)
# Planes of 256 (two image boundaries in every 512-element step of a lane in pair mode), 258 (one or two; bn_slice2 cuts mid-image) and
# 254 (even but below 256: single elements, the control): with 5 / 5 / 3 images they stay below BN_SMALL_MAX and take the one-launch
# kernels (images crossed by bn_small_index); BN_WALK_SHAPES are the same planes past it, where a slice is longer than the workgroup's
# 256 pairs and lanes do step (tests/test_hip_bf16_kernels.py test_bn_shapes_meet_the_quoted_conditions).
BN_WALK_SHAPES = [(65, 2, 16, 16), (130, 2, 6, 43), (67, 2, 2, 127)]
BN_SHAPES = [(3, 16, 1, 1), (1, 3, 7, 5), (2, 5, 129, 33), (1, 3, 300, 211), (5, 3, 16, 16), (5, 2, 6, 43), (3, 2, 2, 127)] + BN_WALK_SHAPES
DW_BN_GEOM = (2, 6, 10, 10, 7, 8)
CONV_BN_CASES = [(13, 5, (12, 12), 8), (24, 8, (2, 3), 8)]
STAGE_CASES = [dict(b=2, cs=5, cp=3, hw=(10, 14), up=False, coords=True), dict(b=2, cs=6, cp=0, hw=(9, 8), up=False, coords=True),
               dict(b=1, cs=3, cp=7, hw=(12, 20), up=True, coords=False), dict(b=2, cs=4, cp=16, hw=(36, 24), up=True, coords=True)]
CE_CASES = [(7, (40, 52)), (19, (33, 47))]


# ------------------------------------------------------------------------------ host-only: the helpers themselves


def _explicit_halo(x, grid):
    """Index arithmetic, no pad / unfold: tile (i, j)[u, v] = x[reflect(i ph + u - 1), reflect(j pw + v - 1)]."""
    b, c, h, w = x.shape
    fh, fw = grid
    ph, pw = h // fh, w // fw

    def refl(i, n):
        return -i if i < 0 else (2 * n - 2 - i if i >= n else i)
    out = torch.empty(b, c, fh * (ph + 2), fw * (pw + 2), dtype=x.dtype)
    for i in range(fh):
        for u in range(ph + 2):
            for j in range(fw):
                for v in range(pw + 2):
                    out[:, :, i * (ph + 2) + u, j * (pw + 2) + v] = x[:, :, refl(i * ph + u - 1, h), refl(j * pw + v - 1, w)]
    return out


@pytest.mark.parametrize('shape,grid', HALO_SHAPES)
def test_ref_halo_tiles_and_interior_match_the_stock_ops(shape, grid):
    x = torch.randn(shape, generator=G(11), dtype=D)
    b, c, h, w = shape
    want = _explicit_halo(x, grid)
    assert torch.equal(R.halo_tiles(x, grid), want)
    assert torch.equal(R.halo_tiles(x, grid, True), R.to_patch_major(want, grid))
    assert torch.equal(R.from_patch_major(R.halo_tiles(x, grid, True), b, grid), want)
    assert torch.equal(R.tile_interior(want, (h, w), grid), x)


@pytest.mark.parametrize('shape', DW_TILES_SHAPES)
def test_ref_dw_tiles_valid_matches_nine_shifted_products(shape):
    b, c, (fh, fw), (ph, pw) = shape
    t = torch.randn(b * fh * fw, c, ph + 2, pw + 2, generator=G(12), dtype=D)
    bank = torch.randn(b * fh * fw, 9 * c, generator=G(13), dtype=D)
    k = bank.view(-1, c, 3, 3)
    want = sum(k[:, :, ky, kx, None, None] * t[:, :, ky:ky + ph, kx:kx + pw] for ky in range(3) for kx in range(3))
    want = R.from_patch_major(want, b, (fh, fw))
    got = R.dw_tiles_valid(t, bank, (fh * ph, fw * pw), (fh, fw), True)
    assert torch.allclose(got, want, rtol=1e-13, atol=1e-13)
    assert torch.equal(R.dw_tiles_valid(R.from_patch_major(t, b, (fh, fw)), bank, (fh * ph, fw * pw), (fh, fw), False), got)


@pytest.mark.parametrize('case', DW3_CASES + K1_CASES, ids=lambda c: 'x'.join(str(v) for v in c.values()))
def test_ref_patch_convolutions_match_the_oracle(case):
    from oracle import hyperseg_oracle as O
    c = case
    b = c.get('b', 1)
    dw = 'c' in c
    cin, cout, k = (c['c'], c['c'], 3) if dw else (c['cin'], c['cout'], 1)
    hp = 9 * cin if dw else cin * cout
    h, w = c['grid'][0] * c['patch'][0], c['grid'][1] * c['patch'][1]
    x = torch.randn(b, cin, h, w, generator=G(14), dtype=D)
    wt = torch.randn(b, hp + 2, *c['grid'], generator=G(15), dtype=D)
    want = O.meta_patch_conv2d(x, wt[:, :hp], cout, k, k // 2, 'zeros', cin if dw else 1)
    bank = R.bank_of(wt, hp)
    got = R.patch_dw3(x, bank, c['grid']) if dw else R.patch_k1(x, bank, c['grid'], cout)
    assert torch.allclose(got, want, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize('relu6', [False, True])
@pytest.mark.parametrize('shape', BN_SHAPES + [(200, 6, 9, 10), (2, 13, 96, 96), (2, 24, 16, 24)])
def test_ref_batchnorm_matches_the_stock_module(shape, relu6):
    """bn_train_ref's values equal nn.BatchNorm2d (train mode, float64) + ReLU6 and their autograd, running statistics included."""
    c = shape[1]
    x = torch.randn(shape, generator=G(16), dtype=D) * 2 + 0.5
    w, b_ = torch.rand(c, generator=G(17), dtype=D) + 0.5, torch.randn(c, generator=G(18), dtype=D)
    r = torch.randn(shape, generator=G(19), dtype=D)
    bn = torch.nn.BatchNorm2d(c, momentum=0.1).double().train()
    with torch.no_grad():
        bn.weight.copy_(w); bn.bias.copy_(b_)
    xa = x.clone().requires_grad_(True)
    y = bn(xa)
    y = torch.nn.functional.relu6(y) if relu6 else y
    (y * r).sum().backward()
    ref = R.bn_train_ref(x, w, b_, r, bn.eps, relu6)
    for got, want in ((ref['y'][0], y.detach()), (ref['dx'][0], xa.grad), (ref['dg'][0], bn.weight.grad), (ref['db'][0], bn.bias.grad),
                      (ref['rm'][0], bn.running_mean), (ref['rv'][0], bn.running_var)):
        assert torch.allclose(got, want, rtol=1e-11, atol=1e-11)
    for k in ('y', 'dx', 'dg', 'db', 'rm', 'rv'):
        assert bool((ref[k][1] >= 0).all()) and (ref[k][2] is None or bool((ref[k][2] >= 0).all()))


@pytest.mark.parametrize('case', STAGE_CASES, ids=lambda c: 'x'.join(str(v) for v in c.values()))
def test_ref_stage_input_matches_the_stock_formulation(case):
    from hyperseg_amd import autograd as HA, functional as HF
    c = case
    h, w = c['hw']
    skip = torch.randn(c['b'], c['cs'], h, w, generator=G(20), dtype=D)
    prev = torch.randn(c['b'], c['cp'], h // 2 if c['up'] else h, w // 2 if c['up'] else w, generator=G(21), dtype=D) if c['cp'] else None
    want = HA.materialize_stage(HF.StageInput(skip.float(), prev.float() if prev is not None else None, coords=c['coords']))      # (CPU tensors: the stock ops)
    got = R.stage_input(skip, prev, c['coords'])
    assert got.shape == want.shape and torch.allclose(got, want.double(), rtol=0, atol=1e-6)


@pytest.mark.parametrize('classes,hw', CE_CASES)
def test_ref_bootstrapped_cross_entropy_matches_the_reference_statement(classes, hw):
    from hyperseg_amd.training import bootstrap_mean_reference
    x, t = _ce_inputs(classes, hw)
    x = x.double()
    lse = torch.logsumexp(x, 1)
    per = (lse - x.gather(1, t.clamp(max=classes - 1).unsqueeze(1)).squeeze(1)) * (t != 255)
    assert torch.allclose(R.pixel_ce(x, t, 255), per, rtol=1e-12, atol=1e-12)
    for k, thresh in _ce_rules(hw):
        want = sum(bootstrap_mean_reference(v, k, thresh) for v in per.flatten(1)) / x.shape[0]
        assert torch.allclose(R.bootstrapped_ce(x, t, 255, k, thresh), want, rtol=1e-12)


def _bound_cases():
    """(ref64, terms, mag64) at the shapes of the GPU tests: the float64 statements on fp16-rounded draws."""
    out = []
    for shape, grid in HALO_SHAPES:
        r = randn16(31, *R.halo_tiles(torch.zeros(shape, dtype=D), grid).shape).double().requires_grad_(True)
        x = randn16(32, *shape).double().requires_grad_(True)
        for v in (r, r.abs()):
            g = torch.autograd.grad(R.halo_tiles(x, grid), x, v.detach())[0]
            out.append(g)
        out[-2:] = [(out[-2], 4, out[-1])]
    for b, c, (fh, fw), (ph, pw) in DW_TILES_SHAPES:
        t = randn16(33, b * fh * fw, c, ph + 2, pw + 2).double()
        bank = randn16(34, b * fh * fw, 9 * c, scale=0.3).double()
        f = lambda a, k: R.dw_tiles_valid(a, k, (fh * ph, fw * pw), (fh, fw), True)          # noqa: E731
        out.append((f(t, bank), 9, f(t.abs(), bank.abs())))
    for c in K1_CASES:
        h, w = c['grid'][0] * c['patch'][0], c['grid'][1] * c['patch'][1]
        x = randn16(35, 1, c['cin'], h, w).double()
        bank = randn16(36, c['grid'][0] * c['grid'][1], c['cin'] * c['cout'], scale=c['cin'] ** -0.5).double()
        out.append((R.patch_k1(x, bank, c['grid'], c['cout']), c['cin'], R.patch_k1(x.abs(), bank.abs(), c['grid'], c['cout'])))
    for shape in BN_SHAPES:
        x = randn16(37, *shape, scale=2.0, shift=0.5).double()
        ref = R.bn_train_ref(x, torch.ones(shape[1], dtype=D), torch.zeros(shape[1], dtype=D), torch.ones(shape, dtype=D), relu6=True)
        out.append((ref['y'][0], ref['n'], ref['y'][1]))
    return out


def test_the_reference_rounded_to_fp16_is_inside_the_bound():
    """ref64.half() passes assert_within_f16 for every statement: the reference alone never uses up the bound."""
    for ref, terms, mag in _bound_cases():
        R.assert_within_f16(ref.half(), ref, terms, mag)
    big = torch.tensor([65504.0, 65519.0, 65520.0, -70000.0, 1e-8, float('nan'), 3e-5], dtype=D)
    R.assert_within_f16(big.half(), big, 1, big.abs())
    with pytest.raises(AssertionError):                                                  # a finite value where binary16 overflows
        R.assert_within_f16(torch.tensor([65504.0]), torch.tensor([70000.0], dtype=D), 1, torch.tensor([70000.0], dtype=D))
    with pytest.raises(AssertionError):                                                  # an infinity where it does not
        R.assert_within_f16(torch.tensor([float('inf')]), torch.tensor([60000.0], dtype=D), 1, torch.tensor([60000.0], dtype=D))
    with pytest.raises(AssertionError):                                                  # a NaN that went missing
        R.assert_within_f16(torch.tensor([1.0]), torch.tensor([float('nan')], dtype=D), 1, torch.tensor([1.0], dtype=D))


def test_the_bound_rejects_one_moved_element_and_a_swapped_pair():
    """The same tensors with ONE element moved by 4 fp16 ulps, and with two horizontally adjacent elements swapped (the hi / lo halves of a
    Pair<f16_t> store), fail the bound."""
    for ref, terms, mag in _bound_cases():
        good = ref.half()
        flat = good.flatten()
        i = int(torch.argmax(ref.abs().flatten()))
        moved = flat.clone().view(torch.int16)
        moved[i] += 4                                                                    # (4 ulps away from zero: finite for these draws)
        if terms <= 1024:              # (BatchNorm over thousands of elements: the issue sets terms = the channel's count, and
            with pytest.raises(AssertionError):          # (terms + 2) 2^-23 mag64 alone then exceeds 4 fp16 ulps; the swap below still fails)
                R.assert_within_f16(moved.view(F16).view(good.shape), ref, terms, mag)
        if good.shape[-1] < 2:
            continue
        rows = ref.reshape(-1, ref.shape[-1])
        gap = (rows[:, 0::2][:, :rows.shape[1] // 2] - rows[:, 1::2]).abs()
        j = int(torch.argmax(gap))                                                       # the pair whose halves differ most
        row, col = j // gap.shape[1], 2 * (j % gap.shape[1])
        swapped = good.reshape(-1, ref.shape[-1]).clone()
        swapped[row, col], swapped[row, col + 1] = good.reshape(-1, ref.shape[-1])[row, col + 1], good.reshape(-1, ref.shape[-1])[row, col]
        with pytest.raises(AssertionError):
            R.assert_within_f16(swapped.view(good.shape), ref, terms, mag)


# ------------------------------------------------------------------------------ GPU


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.fail('needs the MI355X')
    return torch.device('cuda:0')


def _check(tag, got, triple, half=True):
    """``triple``: (ref64, mag64, extra64 or None, terms)."""
    ref, mag, extra, terms = triple
    R.assert_within_f16(got, ref, terms, mag, extra, half=half, what=tag)


@pytest.mark.gpu
@pytest.mark.parametrize('shape,grid', HALO_SHAPES)
def test_halo_tiles_and_interior_f16(dev, shape, grid):
    """hs_halo_tiles_fwd / _bwd (image of tiles and patch-major) and hs_tile_interior_fwd / _bwd at fp16: the forward is a copy (equal to the
    float64 gather cast to fp16); the adjoint sums at most 4 terms (a corner pixel: itself, two edge reflections, the corner reflection ...
    or a neighbour's halo); the interior and its adjoint are copies (zeros on the halos)."""
    from hyperseg_amd import autograd as HA
    b, c, h, w = shape
    x = randn16(sum(shape), *shape)
    x64 = x.double().requires_grad_(True)
    for pm in (False, True):
        want = R.halo_tiles(x64, grid, pm)
        r = randn16(sum(shape) + 1 + pm, *want.shape)
        xg = x.to(dev).requires_grad_(True)
        t = HA.HaloTiles.apply(xg, grid, pm)
        assert t.dtype == F16 and torch.equal(t.detach().cpu(), want.detach().half()), pm
        t.backward(r.to(dev))
        ref = torch.autograd.grad(want, x64, r.double(), retain_graph=True)[0]
        mag = torch.autograd.grad(want, x64, r.double().abs())[0]
        assert xg.grad.dtype == F16
        R.assert_within_f16(xg.grad, ref, 4, mag, what=f'halo adjoint patch_major={pm}')
    tiles = R.halo_tiles(x.double(), grid).half()
    tg = tiles.to(dev).requires_grad_(True)
    y = HA.TileInterior.apply(tg, (h, w), grid)
    assert y.dtype == F16 and torch.equal(y.detach().cpu(), x)
    r2 = randn16(sum(shape) + 3, *shape)
    y.backward(r2.to(dev))
    t64 = tiles.double().requires_grad_(True)
    want = torch.autograd.grad(R.tile_interior(t64, (h, w), grid), t64, r2.double())[0]
    assert torch.equal(tg.grad.cpu(), want.half())


def _dw_tiles_run(dev, shape, pm, seed, t_scale=1.0, bank_scale=0.3, r_scale=1.0, nan_t=None, nan_r=None):
    from hyperseg_amd import autograd as HA
    b, c, (fh, fw), (ph, pw) = shape
    size, grid = (fh * ph, fw * pw), (fh, fw)
    tshape = (b * fh * fw, c, ph + 2, pw + 2) if pm else (b, c, fh * (ph + 2), fw * (pw + 2))
    t = randn16(seed, *tshape, scale=t_scale)
    wide = randn16(seed + 1, b * fh * fw, 9 * c + 5, scale=bank_scale).float()
    r = randn16(seed + 2, b, c, *size, scale=r_scale)
    if nan_t is not None:
        t.view(-1)[nan_t] = float('nan')
    if nan_r is not None:
        r.view(-1)[nan_r] = float('nan')
    tg, kg = t.to(dev).requires_grad_(True), wide.to(dev).requires_grad_(True)
    y = HA.DwTilesValid.apply(tg, kg[:, 2:2 + 9 * c], size, grid, pm)
    y.backward(r.to(dev))
    ref = R.bilinear_with_grads(lambda a, k: R.dw_tiles_valid(a, k, size, grid, pm), t.double(), wide[:, 2:2 + 9 * c].double(), r.double())
    return y.detach(), tg.grad, kg.grad, ref


@pytest.mark.gpu
@pytest.mark.parametrize('patch_major', [False, True])
@pytest.mark.parametrize('shape', DW_TILES_SHAPES)
def test_dw_tiles_valid_f16(dev, shape, patch_major):
    """hs_dw_tiles_fwd / _bwd_in (9 products per output, stored through Pair<f16_t>) and hs_dw_tiles_bwd_w (ph pw products per tap, fp32)
    against F.conv2d(padding 0, groups = B patches C) in float64.  The bank is a column range of a wider tensor: its gradient outside
    the range is exactly zero."""
    b, c, _, (ph, pw) = shape
    y, dt, dk, ref = _dw_tiles_run(dev, shape, patch_major, 100 + c + ph)
    assert y.dtype == F16 and dt.dtype == F16 and dk.dtype == torch.float32
    R.assert_within_f16(y, ref['y'][0], 9, ref['y'][1], what='y')
    R.assert_within_f16(dt, ref['da'][0], 9, ref['da'][1], what='d tiles')
    R.assert_within_f16(dk[:, 2:2 + 9 * c], ref['db'][0], ph * pw, ref['db'][1], half=False, what='d bank')
    assert bool((dk[:, :2] == 0).all()) and bool((dk[:, 2 + 9 * c:] == 0).all())


def _meta_conv_run(dev, cin, cout, k, groups, b, grid, patch, seed, x_scale=1.0, w_scale=None, r_scale=1.0, nan_x=None, nan_r=None):
    """MetaPatchConv2d under fp16 autocast (zero padding) on fp16-valued fp32 leaves -> (y, dx, dbank as (P, hp)), and the float64 statement."""
    from hyperseg_amd.models.layers.meta_patch import MetaPatchConv2d
    h, w = grid[0] * patch[0], grid[1] * patch[1]
    m = MetaPatchConv2d(cin, cout, k, padding=k // 2, groups=groups, padding_mode='zeros')
    hp = m.hyper_params
    x = randn16(seed, b, cin, h, w, scale=x_scale)
    wt = randn16(seed + 1, b, hp, *grid, scale=w_scale if w_scale is not None else (cin // groups * k * k) ** -0.5)
    r = randn16(seed + 2, b, cout, h, w, scale=r_scale)
    if nan_x is not None:
        x.view(-1)[nan_x] = float('nan')
    if nan_r is not None:
        r.view(-1)[nan_r] = float('nan')
    xg, wg = x.float().to(dev).requires_grad_(True), wt.float().to(dev).requires_grad_(True)
    with torch.autocast('cuda'):
        y = m(xg, wg)
    assert y.dtype == F16
    y.backward(r.to(dev))
    fn = (lambda a, bk: R.patch_dw3(a, bk, grid)) if k == 3 else (lambda a, bk: R.patch_k1(a, bk, grid, cout))
    ref = R.bilinear_with_grads(fn, x.double(), R.bank_of(wt.double(), hp), r.double())
    return y.detach(), xg.grad, R.bank_of(wg.grad, hp), ref


@pytest.mark.gpu
@pytest.mark.parametrize('case', DW3_CASES, ids=lambda c: 'x'.join(str(v) for v in c.values()))
def test_patch_dw3_f16(dev, case):
    """hs_patch_conv_plain_fwd / _bwd_in / _bwd_w, depthwise 3x3 with zero padding per patch (patch_dw3_*: the pair form on even widths, the
    single-element form on odd ones) through MetaPatchConv2d under autocast (hs_bank_pack_fwd / hs_bank_unpack_fwd around it: copies):
    9 products per output and input gradient, ph pw per tap."""
    c = case
    y, dx, dbank, ref = _meta_conv_run(dev, c['c'], c['c'], 3, c['c'], c['b'], c['grid'], c['patch'], 200 + c['c'])
    R.assert_within_f16(y, ref['y'][0], 9, ref['y'][1], what='y')
    R.assert_within_f16(dx, ref['da'][0], 9, ref['da'][1], what='dx')
    R.assert_within_f16(dbank, ref['db'][0], c['patch'][0] * c['patch'][1], ref['db'][1], half=False, what='d bank')


@pytest.mark.gpu
@pytest.mark.parametrize('case', K1_CASES, ids=lambda c: 'x'.join(str(v) for v in c.values()))
def test_patch_k1_f16(dev, case):
    """hs_patch_conv_plain_fwd / _bwd_in / _bwd_w at k = 1: the matrix-core forms (*_k1m_kernel, quad_ld(const f16_t*)) and the tiny-patch
    forms, against the per-patch bmm in float64: cin products per output, cout per input gradient, ph pw per weight gradient.  (The kernels
    of test_patch_conv_f16_storage_vs_fp32_oracle, held elementwise.)"""
    c = case
    y, dx, dbank, ref = _meta_conv_run(dev, c['cin'], c['cout'], 1, 1, 1, c['grid'], c['patch'], 300 + c['cin'])
    R.assert_within_f16(y, ref['y'][0], c['cin'], ref['y'][1], what='y')
    R.assert_within_f16(dx, ref['da'][0], c['cout'], ref['da'][1], what='dx')
    R.assert_within_f16(dbank, ref['db'][0], c['patch'][0] * c['patch'][1], ref['db'][1], half=False, what='d bank')


def _bn_module(c, seed, dev):
    bn = torch.nn.BatchNorm2d(c, momentum=0.1).train()
    with torch.no_grad():
        bn.weight.copy_(h16(torch.rand(c, generator=G(seed)) + 0.5).float())
        bn.bias.copy_(randn16(seed + 1, c, scale=0.5).float())
    return bn.to(dev)


@pytest.mark.gpu
@pytest.mark.parametrize('act', [None, 'relu6'])
@pytest.mark.parametrize('shape', BN_SHAPES)
def test_bn_act_train_f16(dev, shape, act):
    """hs_bn_act_train_fwd / _bwd on fp16 storage (one launch up to 16384 elements per channel, two above; pair mode on the even plane of
    300 x 211, single elements elsewhere) against train-mode batch_norm (+ relu6) in float64: output, input gradient (fp16), weight / bias
    gradients and running statistics (fp32), ``terms`` = the channel's element count (util_f16_ref.bn_train_ref derives each mag64)."""
    from hyperseg_amd import autograd as HA
    c = shape[1]
    bn = _bn_module(c, 400 + shape[2], dev)
    x = randn16(402 + shape[2], *shape, scale=2.0) + randn16(403, 1, c, 1, 1)
    r = randn16(404 + shape[2], *shape)
    xg = x.to(dev).requires_grad_(True)
    y = HA.bn_act(bn, torch.nn.ReLU6() if act else None, xg)
    assert y.dtype == F16
    y.backward(r.to(dev))
    ref = R.bn_train_ref(x.double(), bn.weight.detach().double().cpu(), bn.bias.detach().double().cpu(), r.double(), bn.eps, bool(act))
    n = ref['n']
    R.assert_within_f16(y, ref['y'][0], n, ref['y'][1], what='y')
    R.assert_within_f16(xg.grad, ref['dx'][0], n, ref['dx'][1], ref['dx'][2], what='dx')
    for k, got in (('dg', bn.weight.grad), ('db', bn.bias.grad), ('rm', bn.running_mean), ('rv', bn.running_var)):
        R.assert_within_f16(got, ref[k][0], n, ref[k][1], ref[k][2], half=False, what=k)
    assert int(bn.num_batches_tracked) == 1


def _bn_linear_check(tag, out, ref):
    _check(tag + ' y', out['y'], ref['y'])
    _check(tag + ' dx', out['dx'], ref['dx'])
    for k in ('dbank', 'dg', 'db', 'rm', 'rv'):
        _check(f'{tag} {k}', out[k], ref[k], half=False)


@pytest.mark.gpu
@pytest.mark.parametrize('patch_major', [True, False])
def test_dw_tiles_bn_f16(dev, patch_major):
    """autograd.DwTilesBN at fp16 -- hs_bn_train_stats_fwd + hs_dw_tiles_bn_fwd, hs_dw_tiles_bn_bwd_w, and the input gradient both ways:
    USE_DW_BN_BWD_FUSED (hs_dw_tiles_bn_bwd_in + hs_bn_act_train_bwd_apply) and not (hs_dw_tiles_bwd_in + hs_bn_act_train_bwd) -- against
    batch_norm -> relu6 -> valid depthwise in float64 with NO rounding of the normalised copy; the two-step route (hs_bn_act_train_* then
    hs_dw_tiles_*) against the statement WITH that rounding.  Outputs, all four gradients and the running statistics, elementwise."""
    import torch.nn as nn
    from hyperseg_amd import autograd as HA
    b, c, fh, fw, ph, pw = DW_BN_GEOM
    size, grid = (fh * ph, fw * pw), (fh, fw)
    shape = (b * fh * fw, c, ph + 2, pw + 2) if patch_major else (b, c, fh * (ph + 2), fw * (pw + 2))
    t = randn16(501, *shape, scale=1.7, shift=0.4)
    wide = randn16(502, b * fh * fw, 9 * c + 3).float()
    r = randn16(503, b, c, *size)
    bn0 = _bn_module(c, 504, dev)

    def run(fused, bwd_fused):
        prev = HA.USE_DW_BN_FUSED, HA.USE_DW_BN_BWD_FUSED
        HA.USE_DW_BN_FUSED, HA.USE_DW_BN_BWD_FUSED = fused, bwd_fused
        try:
            bn = copy.deepcopy(bn0)
            tg, kg = t.to(dev).requires_grad_(True), wide.to(dev).requires_grad_(True)
            y = HA.dw_tiles_bn(bn, nn.ReLU6(), tg, kg[:, :9 * c], size, grid, patch_major)
            assert y.dtype == F16
            y.backward(r.to(dev))
            assert bool((kg.grad[:, 9 * c:] == 0).all())
            return dict(y=y.detach(), dx=tg.grad, dbank=kg.grad[:, :9 * c], dg=bn.weight.grad, db=bn.bias.grad, rm=bn.running_mean, rv=bn.running_var)
        finally:
            HA.USE_DW_BN_FUSED, HA.USE_DW_BN_BWD_FUSED = prev
    args = (t.double(), bn0.weight.detach().double().cpu(), bn0.bias.detach().double().cpu(), wide[:, :9 * c].double(), r.double(),
            lambda z, k: R.dw_tiles_valid(z, k, size, grid, patch_major), (9, 9, ph * pw), bn0.eps)
    fused_ref, two_ref = R.bn_linear_ref(*args, round_copy=False), R.bn_linear_ref(*args, round_copy=True)
    _bn_linear_check('fused, fused adjoint', run(True, True), fused_ref)
    _bn_linear_check('fused, own statistics launch', run(True, False), fused_ref)
    _bn_linear_check('two-step', run(False, False), two_ref)


@pytest.mark.gpu
@pytest.mark.parametrize('c,cout,grid,p', CONV_BN_CASES)
def test_patch_conv_bn_f16(dev, c, cout, grid, p):
    """autograd.PatchConvBN at fp16 -- hs_bn_train_stats_fwd + hs_patch_conv_bn_fwd, hs_patch_conv_bn_bwd_w, hs_patch_conv_plain_bwd_in +
    hs_bn_act_train_bwd -- against batch_norm -> relu6 -> per-patch bmm in float64 with NO rounding of the normalised copy (what the fused
    form computes); the two-step route (hs_bn_act_train_*, hs_patch_conv_plain_*) against the statement WITH that rounding.  Outputs, all
    four gradients and the running statistics elementwise (for fp16 this replaces bf16's "no worse than the other route and < 1e-1")."""
    import torch.nn as nn
    from hyperseg_amd import autograd as HA
    b = 2
    fh, fw = grid
    h, w = fh * p, fw * p
    x = randn16(601, b, c, h, w, scale=1.3, shift=0.5)
    wide = randn16(602, b * fh * fw, cout * c + 5, scale=c ** -0.5).float()
    r = randn16(603, b, cout, h, w)
    bn0 = _bn_module(c, 604, dev)

    def run(fused):
        prev = HA.USE_CONV_BN_FUSED
        HA.USE_CONV_BN_FUSED = fused
        try:
            bn = copy.deepcopy(bn0)
            xg, kg = x.to(dev).requires_grad_(True), wide.to(dev).requires_grad_(True)
            y = HA.patch_conv_bn(bn, nn.ReLU6(), xg, kg[:, 2:2 + cout * c], grid, cout)
            assert y.dtype == F16
            y.backward(r.to(dev))
            assert bool((kg.grad[:, :2] == 0).all()) and bool((kg.grad[:, 2 + cout * c:] == 0).all())
            return dict(y=y.detach(), dx=xg.grad, dbank=kg.grad[:, 2:2 + cout * c], dg=bn.weight.grad, db=bn.bias.grad, rm=bn.running_mean,
                        rv=bn.running_var)
        finally:
            HA.USE_CONV_BN_FUSED = prev
    args = (x.double(), bn0.weight.detach().double().cpu(), bn0.bias.detach().double().cpu(), wide[:, 2:2 + cout * c].double(), r.double(),
            lambda z, k: R.patch_k1(z, k, grid, cout), (c, cout, p * p), bn0.eps)
    _bn_linear_check('fused', run(True), R.bn_linear_ref(*args, round_copy=False))
    _bn_linear_check('two-step', run(False), R.bn_linear_ref(*args, round_copy=True))


@pytest.mark.gpu
@pytest.mark.parametrize('case', STAGE_CASES, ids=lambda c: 'x'.join(str(v) for v in c.values()))
def test_stage_input_f16(dev, case):
    """autograd.materialize_stage on fp16 operands (hs_stage_input_typed_fwd; backward: a view for the skip, hs_upsample_bilinear_typed_bwd
    for the previous level) against linspace / interpolate(bilinear, align_corners=False) / cat in float64.  Coordinates: 2 products about
    magnitude 2; the skip channels and a same-size previous level are copies (equal); the exact-2x interpolation has 4 taps whose weights
    (1/4, 3/4) are exact; its adjoint gathers at most 4 x 4 outputs per source pixel."""
    from hyperseg_amd import autograd as HA, functional as HF
    c = case
    h, w = c['hw']
    off = 2 * c['coords']
    skip = randn16(700 + c['cs'], c['b'], c['cs'], h, w)
    prev = randn16(701 + c['cp'], c['b'], c['cp'], h // 2 if c['up'] else h, w // 2 if c['up'] else w) if c['cp'] else None
    r = randn16(702, c['b'], off + c['cs'] + c['cp'], h, w)
    sk = skip.to(dev).requires_grad_(True)
    pv = prev.to(dev).requires_grad_(True) if prev is not None else None
    y = HA.materialize_stage(HF.StageInput(sk, pv, coords=c['coords']))
    assert y.dtype == F16
    y.backward(r.to(dev))
    s64 = skip.double().requires_grad_(True)
    p64 = prev.double().requires_grad_(True) if prev is not None else None
    want = R.stage_input(s64, p64, c['coords'])
    yc = y.detach().cpu()
    if off:
        R.assert_within_f16(yc[:, :2], want[:, :2], 2, 2.0, what='coordinates')
    assert torch.equal(yc[:, off:off + c['cs']], skip)
    assert torch.equal(sk.grad.cpu(), r[:, off:off + c['cs']])
    if prev is None:
        return
    mag = R.stage_input(s64, p64.abs(), c['coords'])[:, off + c['cs']:]
    R.assert_within_f16(yc[:, off + c['cs']:], want[:, off + c['cs']:], 4, mag, what='previous level')
    ref = torch.autograd.grad(want, p64, r.double(), retain_graph=True)[0]
    gmag = torch.autograd.grad(want, p64, r.double().abs())[0]
    assert pv.grad.dtype == F16
    if not c['up']:
        assert torch.equal(yc[:, off + c['cs']:], prev) and torch.equal(pv.grad.cpu(), ref.half())
    R.assert_within_f16(pv.grad, ref, 16, gmag, what='d previous level')


def _ce_inputs(classes, hw):
    """The logits and targets of test_fused_bootstrapped_cross_entropy_equals_the_two_functions, rounded to fp16."""
    h, w = hw
    g = G(21)
    x = torch.randn(3, classes, h, w, generator=g) * 3.0
    x[1] *= 0.02
    x[2, :, :, : w // 2] *= 10.0
    t = torch.randint(0, classes, (3, h, w), generator=g)
    t[0, :5] = 255
    t[2, ::3, ::2] = 255
    return h16(x), t


def _ce_rules(hw):
    return ((300, 0.3), (300, 3.0), (hw[0] * hw[1] - 1, 50.0))


@pytest.mark.gpu
@pytest.mark.parametrize('classes,hw', CE_CASES)
def test_fused_bootstrapped_cross_entropy_f16(dev, classes, hw):
    """hs_bootstrapped_ce_fwd / _bwd on fp16 logits == hs_cross_entropy_typed_fwd / _bwd + hs_bootstrap_mean_of_batch_fwd / _bwd bit for bit
    (the three (k, thresh) branches), and both against F.cross_entropy(reduction='none') + the bootstrapped mean in float64.
    Loss (fp32): per pixel max + log sum exp - x_t is C + 8 operations (C exponentials and adds, the log, the subtractions; expf / logf
    within 2 ulp) about |max| + |log s| + |x_t| + 1 (a relative error of the sum is an absolute error of its log); the mean adds one
    term per pixel: terms = C + 8 + H W, mag64 = the same weighted mean of the per-pixel magnitudes.
    Gradient (fp16): upstream * weight * (softmax - onehot), C + 8 terms; softmax = exp(x - lse) carries the absolute error of its argument
    as a relative one: mag64 = upstream * weight * (softmax (1 + |x - lse| + |lse|) + onehot).
    A NaN logit at a pixel that is not ignored gives a NaN loss."""
    import hyperseg_amd.training as T
    x, t = _ce_inputs(classes, hw)
    h, w = hw
    up = 1.75
    for k, thresh in _ce_rules(hw):
        xa, xb = x.to(dev).requires_grad_(True), x.to(dev).requires_grad_(True)
        T.USE_FUSED_LOSS = True
        try:
            la = T.bootstrapped_cross_entropy(xa, t.to(dev), k=k, thresh=thresh, ignore_index=255)
            T.USE_FUSED_LOSS = False
            lb = T.bootstrapped_cross_entropy(xb, t.to(dev), k=k, thresh=thresh, ignore_index=255)
        finally:
            T.USE_FUSED_LOSS = True
        (la * up).backward()
        (lb * up).backward()
        assert la.dtype == torch.float32 and la.dim() == 0 and xa.grad.dtype == F16
        assert torch.equal(la, lb) and torch.equal(xa.grad, xb.grad), (k, thresh)
        x64 = x.double().requires_grad_(True)
        per = R.pixel_ce(x64, t, 255)
        per.retain_grad()
        loss = R.bootstrapped_mean(per, k, thresh)
        (loss * up).backward()
        weight = per.grad / up                                                   # each pixel's share of the batch mean (0: not kept)
        lse = torch.logsumexp(x64.detach(), 1, keepdim=True)
        tt = t.clamp(max=classes - 1).unsqueeze(1)
        xt = x64.detach().gather(1, tt)
        mx = x64.detach().amax(1, keepdim=True)
        per_mag = (mx.abs() + (lse - mx).abs() + xt.abs() + 1).squeeze(1)
        R.assert_within_f16(la.detach(), loss.detach(), classes + 8 + h * w, (weight * per_mag).sum(), half=False, what=f'loss {k} {thresh}')
        soft = (x64.detach() - lse).exp()
        onehot = torch.zeros_like(soft).scatter_(1, tt, 1.0)
        gmag = up * weight.unsqueeze(1) * (soft * (1 + (x64.detach() - lse).abs() + lse.abs()) + onehot)
        R.assert_within_f16(xa.grad, x64.grad, classes + 8, gmag, what=f'd logits {k} {thresh}')
    bad = x.clone()
    bad[0, 0, 10, 3] = float('nan')                                              # (a pixel that is not ignored)
    assert bool(torch.isnan(T.bootstrapped_cross_entropy(bad.to(dev), t.to(dev), k=300, thresh=0.3, ignore_index=255)))


def _assert_overflows(ref64):
    """The case is built so that a known, non-trivial subset of the outputs leaves the binary16 range."""
    fin = ref64[~ref64.isnan()]
    over = int((fin.abs() >= R.F16_INF_FROM).sum())
    assert 0 < over < fin.numel() and int(ref64.isnan().sum()) > 0, (over, fin.numel())


@pytest.mark.gpu
def test_overflow_and_nan_through_the_pair_stores(dev):
    """Pair<f16_t>::st: results above 65520 in fp32 arrive as the infinity of their sign and a NaN operand as NaN, everything else within
    the bound -- hs_dw_tiles_fwd (large tiles, a NaN tile element), the depthwise hs_patch_conv_plain_bwd_in on an even width and
    hs_bn_act_train_bwd in pair mode (even plane of 256) with a large upstream gradient holding one NaN (BatchNorm's adjoint: the NaN
    reaches the channel's two sums, so the whole channel is NaN -- as in float64)."""
    from hyperseg_amd import autograd as HA
    shape = (2, 4, (2, 2), (1, 6))
    y, _, _, ref = _dw_tiles_run(dev, shape, True, 800, t_scale=4096.0, bank_scale=4.0, nan_t=37)
    _assert_overflows(ref['y'][0])
    R.assert_within_f16(y, ref['y'][0], 9, ref['y'][1], what='dw tiles y')
    _, dx, _, ref = _meta_conv_run(dev, 3, 3, 3, 3, 2, (3, 5), (4, 2), 810, w_scale=4.0, r_scale=4096.0, nan_r=101)
    _assert_overflows(ref['da'][0])
    R.assert_within_f16(dx, ref['da'][0], 9, ref['da'][1], what='depthwise dx')
    bshape = (2, 3, 16, 16)
    bn = _bn_module(3, 820, dev)
    x = randn16(822, *bshape, scale=0.05, shift=1.0)                              # invstd ~ 20: the adjoint amplifies
    r = randn16(823, *bshape, scale=2048.0)
    r[1, 2, 5, 7] = float('nan')
    xg = x.to(dev).requires_grad_(True)
    HA.bn_act(bn, None, xg).backward(r.to(dev))
    ref = R.bn_train_ref(x.double(), bn.weight.detach().double().cpu(), bn.bias.detach().double().cpu(), r.double(), bn.eps, False)
    _assert_overflows(ref['dx'][0])
    R.assert_within_f16(xg.grad, ref['dx'][0], ref['n'], ref['dx'][1], ref['dx'][2], what='batchnorm dx')
    R.assert_within_f16(bn.weight.grad, ref['dg'][0], ref['n'], ref['dg'][1], half=False, what='batchnorm dg')


@pytest.mark.gpu
def test_overflow_and_nan_through_the_single_stores_and_the_k1m_epilogue(dev):
    """Store<f16_t>::st (the single-element depthwise forms on an odd width: forward and input adjoint) and the k = 1 matrix-core epilogue
    (forward and input adjoint of hs_patch_conv_plain_*): overflow to the signed infinity, NaN stays NaN (one NaN input pixel: its 3 x 3
    neighbourhood in the patch / every output channel of that pixel), the rest within the bound."""
    y, _, _, ref = _meta_conv_run(dev, 6, 6, 3, 6, 1, (2, 3), (6, 7), 830, x_scale=4096.0, w_scale=4.0, nan_x=200)
    _assert_overflows(ref['y'][0])
    R.assert_within_f16(y, ref['y'][0], 9, ref['y'][1], what='odd-width depthwise y')
    _, dx, _, ref = _meta_conv_run(dev, 6, 6, 3, 6, 1, (2, 3), (6, 7), 840, w_scale=4.0, r_scale=4096.0, nan_r=333)
    _assert_overflows(ref['da'][0])
    R.assert_within_f16(dx, ref['da'][0], 9, ref['da'][1], what='odd-width depthwise dx')
    y, _, _, ref = _meta_conv_run(dev, 17, 33, 1, 1, 1, (2, 1), (16, 20), 850, x_scale=1024.0, w_scale=16.0, nan_x=777)
    _assert_overflows(ref['y'][0])
    R.assert_within_f16(y, ref['y'][0], 17, ref['y'][1], what='k1m y')
    _, dx, _, ref = _meta_conv_run(dev, 17, 33, 1, 1, 1, (2, 1), (16, 20), 860, w_scale=16.0, r_scale=1024.0, nan_r=555)
    _assert_overflows(ref['da'][0])
    R.assert_within_f16(dx, ref['da'][0], 33, ref['da'][1], what='k1m dx')


@pytest.mark.gpu
def test_overflowed_backward_skips_the_adam_step_and_backs_the_scale_off(dev):
    """One step of hyperseg_amd.training.Adam under a GradScaler whose gradients CAME FROM a backward that overflowed fp16 storage (the
    k = 1 input adjoint above, into a leaf that is a parameter): the parameters are unchanged, no step is counted and the scale halves.
    (test_adam_under_grad_scaler_equals_torch_fused_adam plants its infinity by hand and compares with torch's optimizer; it does not
    assert this, so the step is run here.)"""
    from hyperseg_amd.models.layers.meta_patch import MetaPatchConv2d
    from hyperseg_amd.training import Adam
    m = MetaPatchConv2d(17, 33, 1)
    x = torch.nn.Parameter(randn16(870, 1, 17, 32, 20).float().to(dev))
    wt = torch.nn.Parameter(randn16(871, 1, m.hyper_params, 2, 1, scale=16.0).float().to(dev))
    before = [x.detach().clone(), wt.detach().clone()]
    opt = Adam([x, wt], lr=1e-2)
    scaler = torch.amp.GradScaler('cuda', init_scale=2.0 ** 16)
    with torch.autocast('cuda'):
        loss = m(x, wt).float().mean()
    scaler.scale(loss * 1e3).backward()
    assert bool(torch.isinf(x.grad).any())
    scaler.step(opt)
    scaler.update()
    assert float(scaler.get_scale()) == 2.0 ** 15 and opt.steps_taken() == 0
    assert torch.equal(x.detach(), before[0]) and torch.equal(wt.detach(), before[1])
