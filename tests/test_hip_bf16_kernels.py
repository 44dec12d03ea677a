"""Kernel-level tests of the bf16_t instantiation of the storage-typed training kernels: test_hip_fp16_kernels.py's statements, shapes and
``terms`` with the number format swapped (util_f16_ref.BFLOAT16), each output element by element against float64 under

    |got - ref64| <= 2^-8 |ref64| + 2^-126 + (terms + 2) 2^-23 mag64          (fp32 outputs: the last term only)

(derived in util_f16_ref's docstring; nothing in it is measured) -- and the rounding itself, bit for bit.  The bf16 arm has code no other
storage type shares: Store<bf16_t>::st / Pair<bf16_t>::bits round to nearest-even on integer bits with a NaN carve-out (fp16: the hardware
conversion), Pair<bf16_t>::ld, bn_unpack2(.., const bf16_t*) and quad_ld(const bf16_t*) widen by shift / mask, store4_h16(bf16_t*) and
dwt_stored(float, bf16_t*) exist for bf16 alone.  tests/test_hip_training.py holds this arm to relative L2 norms (4e-3 .. 2e-2) and to a
step-level emulation that rounds through torch: a wrong tie, a NaN that the integer rounding carries into +-0, a swapped pair or one
dropped edge element passes both.  They do not pass test_the_bound_rejects_one_moved_element_and_a_swapped_pair / test_exact_rounding_*
(the NaN branch: through fp32 NaN taps in the bank, see NAN_TAP_WORDS -- no bf16 operand can reach it).

Inputs are drawn on the CPU with G(seed) and rounded to bf16 before the reference sees them; a result that goes through two kernels has
the first one's bound pushed through the second (``extra64``) and the bf16 store between them repeated in the reference, as in the fp16
file.  Every output is compared in full.

Exported entry points reached, bf16_t arm (dtype code 1), by test:
  test_halo_tiles_and_interior_bf16          hs_halo_tiles_fwd / _bwd (both layouts; adjoint by tile and by patch), hs_tile_interior_fwd / _bwd
  test_dw_tiles_valid_bf16                   hs_dw_tiles_fwd / _bwd_in / _bwd_w (both layouts)
  test_patch_dw3_bf16                        hs_patch_conv_plain_fwd / _bwd_in / _bwd_w, depthwise 3x3 (pair and single-element forms), hs_bank_pack_fwd / hs_bank_unpack_fwd
  test_patch_k1_bf16                         hs_patch_conv_plain_fwd / _bwd_in / _bwd_w, k = 1 (matrix-core *_k1m_kernel with quad_ld(const bf16_t*); the tiny-patch
                                             typed form behind HS_PLAIN_K1_BF16: the 4 x 4 and 1 x 1 patches)
  test_bn_act_train_bf16                     hs_bn_act_train_fwd / _bwd (the one-launch form; the two-launch form in pair mode -- one image, and BN_WALK_SHAPES
                                             across image boundaries -- and on single elements)
  test_dw_tiles_bn_bf16                      hs_bn_train_stats_fwd, hs_dw_tiles_bn_fwd / _bwd_w / _bwd_in, hs_bn_act_train_bwd_apply; two-step: hs_bn_act_train_*, hs_dw_tiles_*
  test_patch_conv_bn_bf16                    hs_bn_train_stats_fwd, hs_patch_conv_bn_fwd / _bwd_w, hs_patch_conv_plain_bwd_in, hs_bn_act_train_bwd
  test_stage_input_bf16                      hs_stage_input_typed_fwd, hs_upsample_bilinear_typed_bwd
  test_fused_bootstrapped_cross_entropy_bf16 hs_bootstrapped_ce_fwd / _bwd, hs_cross_entropy_typed_fwd / _bwd, hs_bootstrap_mean_of_batch_fwd / _bwd
  test_exact_rounding_pair_store             Pair<bf16_t>::st through hs_dw_tiles_fwd (even patch width), bit for bit
  test_exact_rounding_single_store           Store<bf16_t>::st through the odd-width depthwise hs_patch_conv_plain_fwd, bit for bit

BatchNorm's pair walk (bn_pair_walk, BnWalk2::next: a lane steps 512 elements and takes "at most two image boundaries" as two selects; bn_slice2
cuts the slices in pairs across images).  The launchers' conditions, quoted from hs_train_aux.hip:
    const bool small = (long)batch * pixels <= BN_SMALL_MAX;              // one launch: a workgroup per channel     (BN_SMALL_MAX = 16 * 1024)
    bn_pairs_ok(a): (a.HW & 1) == 0 && a.HW >= 256   [and 4-byte aligned tensors]                                    (the two-launch kernels)
hs_bn_act_train_fwd / _bwd ask ``small`` first, so test_hip_fp16_kernels.BN_SHAPES' (5, 3, 16, 16), (5, 2, 6, 43) and (3, 2, 2, 127) -- 1280, 1290 and
762 elements per channel -- run the one-launch kernels (bn_small_index's division by a reciprocal across 5 / 3 images), not the pair walk.
BN_WALK_SHAPES keep their planes (256: two wraps in every step; 258: one or two, slices cut mid-image; 254: even but below 256, the
single-element walk, the control) with enough images to pass 16384 elements per channel, so a lane does step: they are in BN_SHAPES too.
hs_bn_train_stats_fwd and hs_bn_act_train_bwd_apply (DwTilesBN) have no one-launch form: the fp16 file's DW_BN_GEOM gives them a plane of
90 x 100 as the image of tiles (pairs, one boundary) and 9 x 10 patch-major (90 < 256: single elements), so DW_BN_PAIR_GEOMS add patch-major
tiles of 18 x 18 (324, the training shape the kernel comment names) and 16 x 16 (256), again past 16384 elements per channel.

bf16_t arms left without a test of this kind, and the stronger test that covers each:
  * hs_upsample_bilinear_bf16_fwd and the non-2x hs_upsample_bilinear_typed_bwd: bit-equal to the fp32 kernel rounded once in
    test_hip_training.py (test_upsample_bilinear_bf16_equals_the_fp32_kernel_rounded_once, test_bf16_storage_twins_round_the_fp32_kernels_once).
  * hs_patch_conv_plain_* general k x k (groups = 1, reflect): stays under test_patch_conv_bf16_storage_vs_fp32_oracle (relative L2).
  * hs_bn_act_train_* with ReLU (act code 1): none and ReLU6 run here; ReLU shares ReLU6's code path up to the upper clamp.
  * GradScaler, the Adam-skip test and hs_adam_step_amp: fp16 only.

With HS_BF16_KERNEL_REPORT=<file> the GPU run writes one line per checked output: the worst err / bound and its index
(profiles/bf16_kernel_bound.txt is such a run; no tolerance here is tuned to it)."""
import copy
import functools
import os

import pytest
import torch

import util_f16_ref as R
from conftest import G
from test_hip_fp16_kernels import (BN_SHAPES, BN_WALK_SHAPES, CE_CASES, CONV_BN_CASES, DW3_CASES, DW_BN_GEOM, DW_TILES_SHAPES, HALO_SHAPES,
                                   K1_CASES, STAGE_CASES, _ce_rules)

BF = torch.bfloat16
FMT = R.BFLOAT16
D = torch.float64
BF16_MAX = 2.0 ** 128 * (1 - 2.0 ** -8)

# (B, C, fh, fw, ph, pw), patch-major only: tile planes of 18 x 18 = 324 and 16 x 16 = 256, 52 x 324 = 16848 and 65 x 256 = 16640 elements
# per channel (bn_slice2: 264 / 260 pairs per slice, so lanes 0 .. 7 / 0 .. 3 of every slice take a 512-element step)
DW_BN_PAIR_GEOMS = [(1, 2, 4, 13, 16, 16), (1, 2, 5, 13, 14, 14)]


def b16(t):
    """Rounded to bf16 (what the kernel will read), kept as the bf16 tensor."""
    return t.bfloat16()


def randn16(seed, *shape, scale=1.0, shift=0.0):
    return b16(torch.randn(*shape, generator=G(seed)) * scale + shift)


_REPORT_STARTED = set()


def within(got, ref64, terms, mag64, extra64=None, half=True, what=''):
    """util_f16_ref.assert_within_f16 at bf16, and the report line."""
    ratio, index = R.assert_within_f16(got, ref64, terms, mag64, extra64, half=half, what=what, fmt=FMT)
    path = os.environ.get('HS_BF16_KERNEL_REPORT')
    if path:
        mode = 'a' if path in _REPORT_STARTED else 'w'
        _REPORT_STARTED.add(path)
        case = os.environ.get('PYTEST_CURRENT_TEST', '').split('::')[-1].rsplit(' ', 1)[0]
        with open(path, mode) as f:
            f.write(f'{case:92s} {what:36s} worst err/bound {ratio:.5f} at {index}\n')


# ------------------------------------------------------------------------------ host-only: the format record and the bound


def test_the_format_records():
    """binary16 keeps today's constants; bfloat16's come from the format (8 significant bits, fp32's exponent range)."""
    assert R.BINARY16 == ('fp16', torch.float16, R.U16, R.SUB16, R.F16_INF_FROM) == ('fp16', torch.float16, 2.0 ** -11, 2.0 ** -24, 65520.0)
    fi = torch.finfo(BF)
    assert FMT.dtype is BF and FMT.u == fi.eps / 2 == 2.0 ** -8 and FMT.sub == torch.finfo(torch.float32).tiny == 2.0 ** -126
    assert fi.max == BF16_MAX and FMT.inf_from == (fi.max + 2.0 ** 128) / 2
    at = torch.tensor([FMT.inf_from], dtype=D)
    assert bool(at.float().bfloat16().isinf()) and float((at * (1 - 2.0 ** -20)).float().bfloat16()) == fi.max      # the tie goes to infinity
    assert torch.equal(R.round16(torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8], dtype=D), FMT), torch.tensor([1.0, 1 + 2.0 ** -6], dtype=D))
    assert torch.equal(R.round16(torch.tensor([1 + 2.0 ** -11], dtype=D)), torch.tensor([1.0], dtype=D))


@functools.lru_cache(maxsize=None)
def _bound_cases():
    """(ref64, terms, mag64) at the shapes of the GPU tests: the float64 statements on bf16-rounded draws (computed once, never written to)."""
    out = []
    for shape, grid in HALO_SHAPES:
        r = randn16(31, *R.halo_tiles(torch.zeros(shape, dtype=D), grid).shape).double()
        x = randn16(32, *shape).double().requires_grad_(True)
        g = [torch.autograd.grad(R.halo_tiles(x, grid), x, v)[0] for v in (r, r.abs())]
        out.append((g[0], 4, g[1]))
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


def test_the_reference_rounded_to_bf16_is_inside_the_bound():
    """ref64.bfloat16() passes the bound for every statement, and the overflow / NaN / infinity rules hold at bf16's inf_from: the fp16
    file's cases restated (65504 -> the largest bf16, 65519 / 65520 -> just below / at the midpoint to 2^128, 70000 -> 1.01 x 2^128 ...)."""
    for ref, terms, mag in _bound_cases():
        R.assert_within_f16(ref.bfloat16(), ref, terms, mag, fmt=FMT)
    big = torch.tensor([BF16_MAX, FMT.inf_from * (1 - 2.0 ** -20), FMT.inf_from, -1.01 * 2.0 ** 128, 1e-42, float('nan'), 3e-39], dtype=D)
    stored = big.float().bfloat16()                                                      # (1e-42, 3e-39: below 2^-126, the absolute term's range)
    assert stored.isinf().tolist() == [False, False, True, True, False, False, False] and float(stored[1]) == BF16_MAX
    R.assert_within_f16(stored, big, 1, big.abs(), fmt=FMT)
    one = lambda v: torch.tensor([v], dtype=D)                                           # noqa: E731
    with pytest.raises(AssertionError):                                                  # a finite value where bf16 overflows
        R.assert_within_f16(one(BF16_MAX), one(1.01 * 2.0 ** 128), 1, one(1.01 * 2.0 ** 128), fmt=FMT)
    with pytest.raises(AssertionError):                                                  # an infinity where it does not
        R.assert_within_f16(one(float('inf')), one(0.9 * 2.0 ** 128), 1, one(0.9 * 2.0 ** 128), fmt=FMT)
    with pytest.raises(AssertionError):                                                  # a NaN that went missing
        R.assert_within_f16(one(1.0), one(float('nan')), 1, one(1.0), fmt=FMT)
    with pytest.raises(AssertionError):                                                  # a NaN stored as infinity
        R.assert_within_f16(one(float('inf')), one(float('nan')), 1, one(1.0), fmt=FMT)
    with pytest.raises(AssertionError):                                                  # the infinity of the other sign
        R.assert_within_f16(one(float('-inf')), one(float('inf')), 1, one(1.0), fmt=FMT)
    R.assert_within_f16(one(70000.0), one(70000.0), 1, one(70000.0), fmt=FMT)             # binary16's overflow is not bf16's
    with pytest.raises(AssertionError):
        R.assert_within_f16(one(70000.0), one(70000.0), 1, one(70000.0))


def test_the_bound_rejects_one_moved_element_and_a_swapped_pair():
    """The same tensors with ONE element moved by 4 bf16 ulps, and with two horizontally adjacent elements swapped (the lo / hi halves of a
    Pair<bf16_t> store), fail the bound."""
    for ref, terms, mag in _bound_cases():
        good = ref.bfloat16()
        flat = good.flatten()
        i = int(torch.argmax(ref.abs().flatten()))
        moved = flat.clone().view(torch.int16)
        moved[i] += 4                                                                    # (4 ulps away from zero: finite for these draws)
        if terms <= 1024:              # (BatchNorm over thousands of elements: terms = the channel's count; the swap below still fails)
            with pytest.raises(AssertionError):
                R.assert_within_f16(moved.view(BF).view(good.shape), ref, terms, mag, fmt=FMT)
        if good.shape[-1] < 2:
            continue
        rows = ref.reshape(-1, ref.shape[-1])
        gap = (rows[:, 0::2][:, :rows.shape[1] // 2] - rows[:, 1::2]).abs()
        j = int(torch.argmax(gap))                                                       # the pair whose halves differ most
        row, col = j // gap.shape[1], 2 * (j % gap.shape[1])
        swapped = good.reshape(-1, ref.shape[-1]).clone()
        swapped[row, col], swapped[row, col + 1] = good.reshape(-1, ref.shape[-1])[row, col + 1], good.reshape(-1, ref.shape[-1])[row, col]
        with pytest.raises(AssertionError):
            R.assert_within_f16(swapped.view(good.shape), ref, terms, mag, fmt=FMT)


def test_bn_shapes_meet_the_quoted_conditions():
    """The forms the header claims for the BatchNorm shapes, from the launchers' quoted conditions (a quote, as in test_hip_training_f64.py:
    the launchers have no route query, so a change of BN_SMALL_MAX, BN_CHUNKS or the workgroup size has to be carried over here by hand)."""
    def form(shape, one_launch=True):
        b, hw = shape[0], shape[2] * shape[3]
        return 'small' if one_launch and b * hw <= 16 * 1024 else 'pairs' if hw % 2 == 0 and hw >= 256 else 'single'
    assert [form(s) for s in [(5, 3, 16, 16), (5, 2, 6, 43), (3, 2, 2, 127)]] == ['small'] * 3 and all(s in BN_SHAPES for s in BN_WALK_SHAPES)
    assert [(form(s), s[2] * s[3]) for s in BN_WALK_SHAPES] == [('pairs', 256), ('pairs', 258), ('single', 254)]
    for s in BN_WALK_SHAPES[:2]:                                      # a slice is longer than the workgroup's 256 pairs: lanes step, across images
        assert -(-(s[0] * s[2] * s[3] // 2) // 32) > 256 and s[0] > 2
    assert {form(s) for s in BN_SHAPES} == {'small', 'pairs', 'single'}
    b, c, fh, fw, ph, pw = DW_BN_GEOM
    assert form((b, c, fh * (ph + 2), fw * (pw + 2)), False) == 'pairs' and form((b * fh * fw, c, ph + 2, pw + 2), False) == 'single'
    for b, c, fh, fw, ph, pw in DW_BN_PAIR_GEOMS:
        shape = (b * fh * fw, c, ph + 2, pw + 2)
        assert form(shape) == form(shape, False) == 'pairs' and -(-(shape[0] * shape[2] * shape[3] // 2) // 32) > 256


# ------------------------------------------------------------------------------ exact rounding: the operand table

# (a, b): bf16 values whose a + 2^-8 b is exact in fp32 and lands on the named regime of the round to bf16 (low 16 bits of the fp32 word)
ROUNDING_PAIRS = {
    'tie, even kept bit':   (1.0, 1.0),                          # 0x3f808000 -> 0x3f80
    'tie, odd kept bit':    (1.0 + 2.0 ** -7, 1.0),              # 0x3f818000 -> 0x3f82
    'just above a tie':     (1.0, 1.0 + 2.0 ** -7),              # 0x3f808100 -> 0x3f81
    'just below a tie':     (1.0, 1.0 - 2.0 ** -8),              # 0x3f807f80 -> 0x3f80
    'carry into the next binade': (1.0 - 2.0 ** -8, 0.5),        # 0x3f7f8000 -> 0x3f80
    'rounds up to infinity': (BF16_MAX, 2.0 ** 127),             # 0x7f7f8000 -> 0x7f80
    'plain':                (3.0, 1.0),                          # 0x40404000 -> 0x4040 (makes the period odd: each pair meets both halves of a pair store)
}
REGIMES = [s + k for k in ROUNDING_PAIRS if k != 'plain' for s in ('', 'negative: ')] + ['NaN from a NaN input', '+infinity', '-infinity']
# The NaN carve-out of Store<bf16_t>::st / Pair<bf16_t>::bits cannot be reached from a bf16 operand: a bf16 NaN widens to a word whose low
# 16 bits are zero (0x7fc00000), and the integer rounding without the branch still stores a NaN (0x7fc0) for it.  The branch matters for
# fp32 NaN words from 0x7fff8000 up, where "+ 0x7fff + kept bit" carries out of the exponent into the sign: stored +-0.  Such a word can
# only come from the fp32 bank, so planes 4 and 5 have these words as their centre tap (the arithmetic hands a quiet NaN operand on with
# its payload; the GPU tests assert that on the fp32 arm's output words before they rely on it).
NAN_TAP_WORDS = (0x7fffffff, 0xffffffff)
PLANES = 6


def _store_bits(u, nan_branch=True):
    """Store<bf16_t>::st / Pair<bf16_t>::bits on fp32 words (int64 tensor) -> the 16-bit words; ``nan_branch`` False: the branch removed."""
    nan = (u & 0x7fffffff) > 0x7f800000
    rounded = ((u + 0x7fff + ((u >> 16) & 1)) & 0xffffffff) >> 16
    return torch.where(nan, ((u >> 16) | 0x40) & 0xffff, rounded) if nan_branch else rounded


def _bank32(bank64):
    """The fp32 bank of a case: its float64 taps (all exact in fp32), the two NaN taps as NAN_TAP_WORDS."""
    w = bank64.float().contiguous()
    at = torch.nonzero(bank64.reshape(-1).isnan()).flatten()
    assert at.numel() == len(NAN_TAP_WORDS)
    w.view(torch.int32).view(-1)[at] = torch.tensor(NAN_TAP_WORDS, dtype=torch.int64).to(torch.int32)
    return w


def _rounding_values(rows, width, special):
    """(PLANES, rows, width): the sequence 0, a, b of every pair and its negative, repeated through each plane (period 39: odd, so a pair's
    column parity changes from row to row); plane 0 finite, planes 1 / 2 / 3 with one NaN / +infinity / -infinity at ``special``, planes 4
    and 5 finite (their NaN is a tap: ``_taps``)."""
    seq = []
    for a, b in ROUNDING_PAIRS.values():
        seq += [0.0, a, b, 0.0, -a, -b]
    seq = seq[:-3]                                                 # ('plain' once)
    v = torch.tensor(seq, dtype=D).repeat(rows * width // len(seq) + 1)[:rows * width].reshape(1, rows, width).repeat(PLANES, 1, 1)
    for plane, s in ((1, float('nan')), (2, float('inf')), (3, float('-inf'))):
        v[(plane,) + special] = s
    assert torch.equal(v.bfloat16().double().nan_to_num(nan=7.0), v.nan_to_num(nan=7.0))
    return v


def _classify(ref64):
    """{regime: mask} of a float64 result from its fp32 word.  Raises unless every finite value is exact in fp32."""
    f = ref64.float()
    fin = ref64.isfinite()
    assert torch.equal(f.double()[fin], ref64[fin]) and bool(f[fin].isfinite().all()) and not bool((ref64[fin] == 0).any())
    u = f.view(torch.int32).long() & 0xffffffff
    low, kept, top7, neg = u & 0xffff, (u >> 16) & 1, (u >> 16) & 0x7f, (u >> 31) == 1
    tie = low == 0x8000
    to_inf = fin & ((u & 0x7fffffff) >= 0x7f7f8000)
    named = {'tie, even kept bit': tie & (kept == 0), 'tie, odd kept bit': tie & (kept == 1) & (top7 != 0x7f),
             'just above a tie': (low > 0x8000) & (low <= 0x8100), 'just below a tie': (low < 0x8000) & (low >= 0x7f00),
             'carry into the next binade': tie & (top7 == 0x7f) & ~to_inf, 'rounds up to infinity': to_inf}
    out = {}
    for k, m in named.items():
        out[k], out['negative: ' + k] = fin & m & ~neg, fin & m & neg
    out['NaN from a NaN input'], out['+infinity'], out['-infinity'] = ref64.isnan(), ref64 == float('inf'), ref64 == float('-inf')
    return out


def _taps():
    """(PLANES, 3, 3): centre 1, right neighbour 2^-8; planes 4 / 5: a NaN centre (NAN_TAP_WORDS in the fp32 bank)."""
    k = torch.zeros(PLANES, 3, 3, dtype=D)
    k[:, 1, 1], k[:, 1, 2] = 1.0, 2.0 ** -8
    k[4:, 1, 1] = float('nan')
    return k


@functools.lru_cache(maxsize=None)
def _pair_store_case():
    """hs_dw_tiles_fwd, one patch-major 9 x 38 patch (tile 11 x 40) of PLANES channels."""
    t = _rounding_values(11, 40, (5, 17))
    bank = _taps().reshape(1, 9 * PLANES)
    return t.unsqueeze(0), bank, R.dw_tiles_valid(t.unsqueeze(0), bank, (9, 38), (1, 1), True)


@functools.lru_cache(maxsize=None)
def _single_store_case():
    """The depthwise hs_patch_conv_plain_fwd, one 9 x 39 patch (odd width: the single-element form) of PLANES channels, the same taps."""
    x = _rounding_values(9, 39, (4, 17)).unsqueeze(0)
    wt = _taps().reshape(1, 9 * PLANES, 1, 1)
    return x, wt, R.patch_dw3(x, R.bank_of(wt, 9 * PLANES), (1, 1))


@pytest.mark.parametrize('case', [_pair_store_case, _single_store_case], ids=['pair store', 'single store'])
def test_the_rounding_table_reaches_every_regime(case):
    """The float64 results of the two exact-rounding cases, classified by the low 16 bits of their fp32 word: every named regime occurs
    (in the pair-store case in an even and in an odd column: both halves of the 4-byte store), every finite result is exact in fp32 and
    none is zero, and rounding the table wrongly -- truncation, the tie term dropped, the NaN branch removed (on the NaN taps' words; the
    bf16 NaN input alone would not tell) -- changes the expected bits, so the GPU tests cannot lose a regime silently."""
    ref = case()[2]
    masks = _classify(ref)
    assert sorted(masks) == sorted(REGIMES)
    for k in REGIMES:
        assert bool(masks[k].any()), k
        if case is _pair_store_case:
            assert bool(masks[k][..., 0::2].any()) and bool(masks[k][..., 1::2].any()), k
    assert int(masks['NaN from a NaN input'][0, 1].sum()) == 9 and not bool(masks['NaN from a NaN input'][0, 0].any())
    assert bool(ref[0, 4:].isnan().all())                                        # every output of the NaN-tap planes
    is_nan = lambda h: (h & 0x7fff) > 0x7f80                                     # noqa: E731
    tap_words = _bank32(case()[1]).view(torch.int32).flatten().long() & 0xffffffff
    tap_words = tap_words[(tap_words & 0x7fffffff) > 0x7f800000]
    assert tap_words.tolist() == list(NAN_TAP_WORDS)
    assert is_nan(_store_bits(tap_words)).tolist() == [True, True] and _store_bits(tap_words, False).tolist() == [0x8000, 0x0000]
    widened = torch.tensor([0x7fc00000, 0xffc00000])                             # all a bf16 NaN operand can give: NaN either way
    assert is_nan(_store_bits(widened)).all() and is_nan(_store_bits(widened, False)).all()
    fin_words = ref.float().view(torch.int32).long()[ref.isfinite()] & 0xffffffff
    assert torch.equal(_store_bits(fin_words).to(torch.int16), ref.float().bfloat16().view(torch.int16)[ref.isfinite()])
    want = ref.float().bfloat16()
    fin = ref.isfinite()
    u = ref.float().view(torch.int32)
    truncated = (u >> 16).to(torch.int16).view(BF)
    no_even = ((u + 0x7fff) >> 16).to(torch.int16).view(BF)                      # Store<bf16_t>::st without "+ ((u >> 16) & 1)"
    for k in REGIMES[:12]:
        m = masks[k]
        up = 'above' in k or 'odd' in k or 'carry' in k or 'infinity' in k
        assert bool((want[m] != truncated[m]).all()) == up and bool((want[m] == truncated[m]).all()) == (not up), k
    odd = masks['tie, odd kept bit'] | masks['carry into the next binade'] | masks['rounds up to infinity']
    assert bool((want[odd] != no_even[odd]).all()) and bool(want[fin & masks['rounds up to infinity']].isinf().all())


# ------------------------------------------------------------------------------ GPU


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.fail('needs the MI355X')
    return torch.device('cuda:0')


def _assert_bit_equal(got, ref64, what, fp32_twin):
    """``got`` (bf16) == ref64.float().bfloat16() as 16-bit words; where that is NaN, ``got`` is NaN (any payload).  ``fp32_twin``: the
    same launch on fp32 storage -- its words in the NaN-tap planes must all be NaNs that the carve-out is needed for (from 0x7fff8000 up:
    without the branch they are stored as +-0), so those planes test the branch and not only a NaN's survival."""
    words = fp32_twin.detach().cpu().view(torch.int32).long() & 0x7fffffff
    assert fp32_twin.dtype == torch.float32 and bool((words[0, 4:] >= 0x7fff8000).all()), f'{what}: the NaN taps\' payload did not reach the store'
    assert got.dtype == BF and got.shape == ref64.shape, what
    got, want = got.detach().cpu(), ref64.float().bfloat16()
    nan = want.isnan()
    assert torch.equal(got.isnan(), nan), f'{what}: NaN positions differ, first {torch.nonzero(got.isnan() != nan)[:8].tolist()}'
    g, w = got.view(torch.int16)[~nan], want.view(torch.int16)[~nan]
    if not torch.equal(g, w):
        idx = torch.nonzero((got.view(torch.int16) != want.view(torch.int16)) & ~nan)
        i = tuple(idx[0].tolist())
        raise AssertionError(f'{what}: {idx.shape[0]} words differ; first at {i}: got {int(got.view(torch.int16)[i]) & 0xffff:#06x}, '
                             f'want {int(want.view(torch.int16)[i]) & 0xffff:#06x} (fp32 word {int(ref64.float().view(torch.int32)[i]) & 0xffffffff:#010x})')


@pytest.mark.gpu
def test_exact_rounding_pair_store(dev):
    """Pair<bf16_t>::st / ::bits through hs_dw_tiles_fwd on an even patch width: operands whose fp32 result is exact (ROUNDING_PAIRS), so
    the stored words must equal ref64.float().bfloat16() -- ties to even both ways, either side of a tie, the carry into the next binade,
    the round up to infinity, all of them negated, a NaN input, both infinities, and fp32 NaN words that only the NaN branch keeps a NaN
    (NAN_TAP_WORDS, from the bank); in both halves of the 4-byte store."""
    from hyperseg_amd import autograd as HA
    t, bank, ref = _pair_store_case()
    bank32 = _bank32(bank).to(dev)
    y = HA.DwTilesValid.apply(t.bfloat16().to(dev), bank32, (9, 38), (1, 1), True)
    _assert_bit_equal(y, ref, 'hs_dw_tiles_fwd', HA.DwTilesValid.apply(t.float().to(dev), bank32, (9, 38), (1, 1), True))


@pytest.mark.gpu
def test_exact_rounding_single_store(dev):
    """Store<bf16_t>::st through the depthwise hs_patch_conv_plain_fwd on an odd patch width (the single-element form), same table."""
    from hyperseg_amd.models.layers.meta_patch import MetaPatchConv2d
    x, wt, ref = _single_store_case()
    m = MetaPatchConv2d(PLANES, PLANES, 3, padding=1, groups=PLANES, padding_mode='zeros')
    assert m.hyper_params == 9 * PLANES
    wt32 = _bank32(wt).to(dev).requires_grad_(True)                                   # (a bank that wants its gradient: the training route)
    with torch.autocast('cuda', dtype=BF):
        y = m(x.bfloat16().to(dev), wt32)
    _assert_bit_equal(y.detach(), ref, 'hs_patch_conv_plain_fwd depthwise, odd width', m(x.float().to(dev), wt32))


@pytest.mark.gpu
@pytest.mark.parametrize('shape,grid', HALO_SHAPES)
def test_halo_tiles_and_interior_bf16(dev, shape, grid):
    """hs_halo_tiles_fwd / _bwd (image of tiles and patch-major) and hs_tile_interior_fwd / _bwd at bf16: the copies bit-equal, the halo
    adjoint (at most 4 terms per pixel) within the bound."""
    from hyperseg_amd import autograd as HA
    b, c, h, w = shape
    x = randn16(sum(shape), *shape)
    x64 = x.double().requires_grad_(True)
    for pm in (False, True):
        want = R.halo_tiles(x64, grid, pm)
        r = randn16(sum(shape) + 1 + pm, *want.shape)
        xg = x.to(dev).requires_grad_(True)
        t = HA.HaloTiles.apply(xg, grid, pm)
        assert t.dtype == BF and torch.equal(t.detach().cpu(), want.detach().bfloat16()), pm
        t.backward(r.to(dev))
        ref = torch.autograd.grad(want, x64, r.double(), retain_graph=True)[0]
        mag = torch.autograd.grad(want, x64, r.double().abs())[0]
        assert xg.grad.dtype == BF
        within(xg.grad, ref, 4, mag, what=f'halo adjoint patch_major={pm}')
    tiles = R.halo_tiles(x.double(), grid).bfloat16()
    tg = tiles.to(dev).requires_grad_(True)
    y = HA.TileInterior.apply(tg, (h, w), grid)
    assert y.dtype == BF and torch.equal(y.detach().cpu(), x)
    r2 = randn16(sum(shape) + 3, *shape)
    y.backward(r2.to(dev))
    t64 = tiles.double().requires_grad_(True)
    want = torch.autograd.grad(R.tile_interior(t64, (h, w), grid), t64, r2.double())[0]
    assert tg.grad.dtype == BF and torch.equal(tg.grad.cpu(), want.bfloat16())


@pytest.mark.gpu
@pytest.mark.parametrize('patch_major', [False, True])
@pytest.mark.parametrize('shape', DW_TILES_SHAPES)
def test_dw_tiles_valid_bf16(dev, shape, patch_major):
    """hs_dw_tiles_fwd / _bwd_in (9 products per output, stored through Pair<bf16_t> / dwt_stored) and hs_dw_tiles_bwd_w (ph pw products
    per tap, fp32) against F.conv2d(padding 0, groups = B patches C) in float64; the bank a column range of a wider tensor."""
    from hyperseg_amd import autograd as HA
    b, c, (fh, fw), (ph, pw) = shape
    size, grid, seed = (fh * ph, fw * pw), (fh, fw), 100 + c + ph
    tshape = (b * fh * fw, c, ph + 2, pw + 2) if patch_major else (b, c, fh * (ph + 2), fw * (pw + 2))
    t = randn16(seed, *tshape)
    wide = randn16(seed + 1, b * fh * fw, 9 * c + 5, scale=0.3).float()
    r = randn16(seed + 2, b, c, *size)
    tg, kg = t.to(dev).requires_grad_(True), wide.to(dev).requires_grad_(True)
    y = HA.DwTilesValid.apply(tg, kg[:, 2:2 + 9 * c], size, grid, patch_major)
    y.backward(r.to(dev))
    ref = R.bilinear_with_grads(lambda a, k: R.dw_tiles_valid(a, k, size, grid, patch_major), t.double(), wide[:, 2:2 + 9 * c].double(), r.double())
    dk = kg.grad
    assert y.dtype == BF and tg.grad.dtype == BF and dk.dtype == torch.float32
    within(y.detach(), ref['y'][0], 9, ref['y'][1], what='y')
    within(tg.grad, ref['da'][0], 9, ref['da'][1], what='d tiles')
    within(dk[:, 2:2 + 9 * c], ref['db'][0], ph * pw, ref['db'][1], half=False, what='d bank')
    assert bool((dk[:, :2] == 0).all()) and bool((dk[:, 2 + 9 * c:] == 0).all())


def _meta_conv_run(dev, cin, cout, k, groups, b, grid, patch, seed):
    """MetaPatchConv2d under bf16 autocast (zero padding) on a bf16 map and an fp32 bank of bf16 values -> (y, dx, dbank as (P, hp)), and the
    float64 statement."""
    from hyperseg_amd.models.layers.meta_patch import MetaPatchConv2d
    h, w = grid[0] * patch[0], grid[1] * patch[1]
    m = MetaPatchConv2d(cin, cout, k, padding=k // 2, groups=groups, padding_mode='zeros')
    hp = m.hyper_params
    x = randn16(seed, b, cin, h, w)
    wt = randn16(seed + 1, b, hp, *grid, scale=(cin // groups * k * k) ** -0.5)
    r = randn16(seed + 2, b, cout, h, w)
    xg, wg = x.to(dev).requires_grad_(True), wt.float().to(dev).requires_grad_(True)
    with torch.autocast('cuda', dtype=BF):
        y = m(xg, wg)
    y.backward(r.to(dev))
    assert y.dtype == BF and xg.grad.dtype == BF and wg.grad.dtype == torch.float32
    fn = (lambda a, bk: R.patch_dw3(a, bk, grid)) if k == 3 else (lambda a, bk: R.patch_k1(a, bk, grid, cout))
    ref = R.bilinear_with_grads(fn, x.double(), R.bank_of(wt.double(), hp), r.double())
    return y.detach(), xg.grad, R.bank_of(wg.grad, hp), ref


@pytest.mark.gpu
@pytest.mark.parametrize('case', DW3_CASES, ids=lambda c: 'x'.join(str(v) for v in c.values()))
def test_patch_dw3_bf16(dev, case):
    """hs_patch_conv_plain_fwd / _bwd_in / _bwd_w, depthwise 3x3 with zero padding (the pair form on even widths, the single-element form on
    odd ones) through MetaPatchConv2d under bf16 autocast: 9 products per output and input gradient, ph pw per tap."""
    c = case
    y, dx, dbank, ref = _meta_conv_run(dev, c['c'], c['c'], 3, c['c'], c['b'], c['grid'], c['patch'], 200 + c['c'])
    within(y, ref['y'][0], 9, ref['y'][1], what='y')
    within(dx, ref['da'][0], 9, ref['da'][1], what='dx')
    within(dbank, ref['db'][0], c['patch'][0] * c['patch'][1], ref['db'][1], half=False, what='d bank')


@pytest.mark.gpu
@pytest.mark.parametrize('case', K1_CASES, ids=lambda c: 'x'.join(str(v) for v in c.values()))
def test_patch_k1_bf16(dev, case):
    """hs_patch_conv_plain_fwd / _bwd_in / _bwd_w at k = 1: the matrix-core forms (*_k1m_kernel, quad_ld(const bf16_t*)) and the tiny-patch
    typed form behind HS_PLAIN_K1_BF16, against the per-patch bmm in float64: cin products per output, cout per input gradient, ph pw per
    weight gradient."""
    c = case
    y, dx, dbank, ref = _meta_conv_run(dev, c['cin'], c['cout'], 1, 1, 1, c['grid'], c['patch'], 300 + c['cin'])
    within(y, ref['y'][0], c['cin'], ref['y'][1], what='y')
    within(dx, ref['da'][0], c['cout'], ref['da'][1], what='dx')
    within(dbank, ref['db'][0], c['patch'][0] * c['patch'][1], ref['db'][1], half=False, what='d bank')


def _bn_module(c, seed, dev):
    bn = torch.nn.BatchNorm2d(c, momentum=0.1).train()
    with torch.no_grad():
        bn.weight.copy_(b16(torch.rand(c, generator=G(seed)) + 0.5).float())
        bn.bias.copy_(randn16(seed + 1, c, scale=0.5).float())
    return bn.to(dev)


@pytest.mark.gpu
@pytest.mark.parametrize('act', [None, 'relu6'])
@pytest.mark.parametrize('shape', BN_SHAPES)
def test_bn_act_train_bf16(dev, shape, act):
    """hs_bn_act_train_fwd / _bwd on bf16 storage against train-mode batch_norm (+ relu6) in float64 -- the one-launch form, the two-launch
    form in pair mode on one image (300 x 211) and across image boundaries inside a lane's 512-element step (BN_WALK_SHAPES: planes of 256
    and 258), and on single elements (254, 129 x 33): output and input gradient (bf16), weight / bias gradients and running statistics
    (fp32), ``terms`` = the channel's element count."""
    from hyperseg_amd import autograd as HA
    c = shape[1]
    bn = _bn_module(c, 400 + shape[2], dev)
    x = b16(randn16(402 + shape[2], *shape, scale=2.0).float() + randn16(403, 1, c, 1, 1).float())
    r = randn16(404 + shape[2], *shape)
    xg = x.to(dev).requires_grad_(True)
    y = HA.bn_act(bn, torch.nn.ReLU6() if act else None, xg)
    y.backward(r.to(dev))
    assert y.dtype == BF and xg.grad.dtype == BF
    assert all(t.dtype == torch.float32 for t in (bn.weight.grad, bn.bias.grad, bn.running_mean, bn.running_var))
    ref = R.bn_train_ref(x.double(), bn.weight.detach().double().cpu(), bn.bias.detach().double().cpu(), r.double(), bn.eps, bool(act))
    n = ref['n']
    within(y, ref['y'][0], n, ref['y'][1], what='y')
    within(xg.grad, ref['dx'][0], n, ref['dx'][1], ref['dx'][2], what='dx')
    for k, got in (('dg', bn.weight.grad), ('db', bn.bias.grad), ('rm', bn.running_mean), ('rv', bn.running_var)):
        within(got, ref[k][0], n, ref[k][1], ref[k][2], half=False, what=k)
    assert int(bn.num_batches_tracked) == 1


def _bn_linear_check(tag, out, ref):
    assert out['y'].dtype == BF and out['dx'].dtype == BF and all(out[k].dtype == torch.float32 for k in ('dbank', 'dg', 'db', 'rm', 'rv'))
    for k in ('y', 'dx', 'dbank', 'dg', 'db', 'rm', 'rv'):
        r, mag, extra, terms = ref[k]
        within(out[k], r, terms, mag, extra, half=k in ('y', 'dx'), what=f'{tag} {k}')


@pytest.mark.gpu
@pytest.mark.parametrize('geom,patch_major', [(DW_BN_GEOM, True), (DW_BN_GEOM, False)] + [(g, True) for g in DW_BN_PAIR_GEOMS],
                         ids=['patch-major 9x10 tiles', 'image of tiles', 'patch-major 18x18 tiles', 'patch-major 16x16 tiles'])
def test_dw_tiles_bn_bf16(dev, geom, patch_major):
    """autograd.DwTilesBN at bf16 -- hs_bn_train_stats_fwd + hs_dw_tiles_bn_fwd, hs_dw_tiles_bn_bwd_w, and the input gradient both ways:
    USE_DW_BN_BWD_FUSED (hs_dw_tiles_bn_bwd_in + hs_bn_act_train_bwd_apply) and not (hs_dw_tiles_bwd_in + hs_bn_act_train_bwd) -- against
    batch_norm -> relu6 -> valid depthwise in float64 with NO rounding of the normalised copy; the two-step route (hs_bn_act_train_* then
    hs_dw_tiles_*) against the statement WITH that rounding, in bf16.  The fp16 file's geometry has a patch-major tile plane of 9 x 10 = 90,
    which does not qualify for BatchNorm's pair mode (even and >= 256); DW_BN_PAIR_GEOMS' planes of 324 and 256 do, with slices long
    enough that a lane steps across one or two tiles."""
    import torch.nn as nn
    from hyperseg_amd import autograd as HA
    b, c, fh, fw, ph, pw = geom
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
            y.backward(r.to(dev))
            assert bool((kg.grad[:, 9 * c:] == 0).all())
            return dict(y=y.detach(), dx=tg.grad, dbank=kg.grad[:, :9 * c], dg=bn.weight.grad, db=bn.bias.grad, rm=bn.running_mean, rv=bn.running_var)
        finally:
            HA.USE_DW_BN_FUSED, HA.USE_DW_BN_BWD_FUSED = prev
    args = (t.double(), bn0.weight.detach().double().cpu(), bn0.bias.detach().double().cpu(), wide[:, :9 * c].double(), r.double(),
            lambda z, k: R.dw_tiles_valid(z, k, size, grid, patch_major), (9, 9, ph * pw), bn0.eps)
    fused_ref, two_ref = R.bn_linear_ref(*args, round_copy=False, fmt=FMT), R.bn_linear_ref(*args, round_copy=True, fmt=FMT)
    _bn_linear_check('fused, fused adjoint', run(True, True), fused_ref)
    _bn_linear_check('fused, own statistics launch', run(True, False), fused_ref)
    _bn_linear_check('two-step', run(False, False), two_ref)


@pytest.mark.gpu
@pytest.mark.parametrize('c,cout,grid,p', CONV_BN_CASES)
def test_patch_conv_bn_bf16(dev, c, cout, grid, p):
    """autograd.PatchConvBN at bf16 -- hs_bn_train_stats_fwd + hs_patch_conv_bn_fwd, hs_patch_conv_bn_bwd_w, hs_patch_conv_plain_bwd_in +
    hs_bn_act_train_bwd -- against batch_norm -> relu6 -> per-patch bmm in float64 with NO rounding of the normalised copy; the two-step
    route (hs_bn_act_train_*, hs_patch_conv_plain_*) against the statement WITH that rounding, in bf16."""
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
            y.backward(r.to(dev))
            assert bool((kg.grad[:, :2] == 0).all()) and bool((kg.grad[:, 2 + cout * c:] == 0).all())
            return dict(y=y.detach(), dx=xg.grad, dbank=kg.grad[:, 2:2 + cout * c], dg=bn.weight.grad, db=bn.bias.grad, rm=bn.running_mean,
                        rv=bn.running_var)
        finally:
            HA.USE_CONV_BN_FUSED = prev
    args = (x.double(), bn0.weight.detach().double().cpu(), bn0.bias.detach().double().cpu(), wide[:, 2:2 + cout * c].double(), r.double(),
            lambda z, k: R.patch_k1(z, k, grid, cout), (c, cout, p * p), bn0.eps)
    _bn_linear_check('fused', run(True), R.bn_linear_ref(*args, round_copy=False, fmt=FMT))
    _bn_linear_check('two-step', run(False), R.bn_linear_ref(*args, round_copy=True, fmt=FMT))


@pytest.mark.gpu
@pytest.mark.parametrize('case', STAGE_CASES, ids=lambda c: 'x'.join(str(v) for v in c.values()))
def test_stage_input_bf16(dev, case):
    """autograd.materialize_stage on bf16 operands (hs_stage_input_typed_fwd; backward: a view for the skip, hs_upsample_bilinear_typed_bwd
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
    assert y.dtype == BF
    y.backward(r.to(dev))
    s64 = skip.double().requires_grad_(True)
    p64 = prev.double().requires_grad_(True) if prev is not None else None
    want = R.stage_input(s64, p64, c['coords'])
    yc = y.detach().cpu()
    if off:
        within(yc[:, :2], want[:, :2], 2, 2.0, what='coordinates')
    assert torch.equal(yc[:, off:off + c['cs']], skip)
    assert sk.grad.dtype == BF and torch.equal(sk.grad.cpu(), r[:, off:off + c['cs']])
    if prev is None:
        return
    mag = R.stage_input(s64, p64.abs(), c['coords'])[:, off + c['cs']:]
    within(yc[:, off + c['cs']:], want[:, off + c['cs']:], 4, mag, what='previous level')
    ref = torch.autograd.grad(want, p64, r.double(), retain_graph=True)[0]
    gmag = torch.autograd.grad(want, p64, r.double().abs())[0]
    assert pv.grad.dtype == BF
    if not c['up']:
        assert torch.equal(yc[:, off + c['cs']:], prev) and torch.equal(pv.grad.cpu(), ref.bfloat16())
    within(pv.grad, ref, 16, gmag, what='d previous level')


def _ce_inputs(classes, hw):
    """The logits and targets of the fp16 file's loss test, rounded to bf16."""
    h, w = hw
    g = G(21)
    x = torch.randn(3, classes, h, w, generator=g) * 3.0
    x[1] *= 0.02
    x[2, :, :, : w // 2] *= 10.0
    t = torch.randint(0, classes, (3, h, w), generator=g)
    t[0, :5] = 255
    t[2, ::3, ::2] = 255
    return b16(x), t


def _ce_slack(classes, hw, k, thresh):
    """util_f16_ref.bootstrap_weight_slack of a loss case, as a share of the BATCH mean: the fp32 loss of a pixel is C + 8 operations about
    |max| + |log s| + |x_t| + 1 (the fp16 file's count)."""
    x, t = _ce_inputs(classes, hw)
    x = x.double()
    lse, mx = torch.logsumexp(x, 1), x.amax(1)
    xt = x.gather(1, t.clamp(max=classes - 1).unsqueeze(1)).squeeze(1)
    per_err = R.sum_bound(classes + 8, mx.abs() + (lse - mx).abs() + xt.abs() + 1)
    return R.bootstrap_weight_slack(R.pixel_ce(x, t, 255), per_err, k, thresh, live=t != 255) / x.shape[0]


@pytest.mark.parametrize('classes,hw', CE_CASES)
def test_the_selection_slack_is_confined_to_the_boundary(classes, hw):
    """bootstrap_weight_slack on the loss cases: every rule's branch is decided by the data (it raises otherwise), leaves only a minority
    of each image's live pixels undecided and no ignored pixel any slack (its gradient is exactly 0 whatever the selection); under the
    top-k rule the undecided ones include every live pixel whose loss fp32 cannot tell from the ignored pixels' 0 (the sharp image has
    such pixels), each with the whole weight 1 / k as its slack."""
    x, t = _ce_inputs(classes, hw)
    per, live = R.pixel_ce(x.double(), t, 255), t != 255
    for k, thresh in _ce_rules(hw):
        slack = _ce_slack(classes, hw, k, thresh)
        assert not bool(slack[~live].any())
        for i in range(3):
            assert int((slack[i] > 0)[live[i]].sum()) < int(live[i].sum()) // 2, (k, thresh, i)
    top_k, thresh = _ce_rules(hw)[-1]
    top_slack = _ce_slack(classes, hw, top_k, thresh)
    tiny = live & (per < 2.0 ** -24)
    assert top_k == hw[0] * hw[1] - 1 and bool(tiny[2].any()) and bool((top_slack[tiny] == 1.0 / top_k / 3).all())


@pytest.mark.gpu
@pytest.mark.parametrize('classes,hw', CE_CASES)
def test_fused_bootstrapped_cross_entropy_bf16(dev, classes, hw):
    """hs_bootstrapped_ce_fwd / _bwd on bf16 logits == hs_cross_entropy_typed_fwd / _bwd + hs_bootstrap_mean_of_batch_fwd / _bwd bit for bit
    (the three (k, thresh) branches), and both against F.cross_entropy(reduction='none') + the bootstrapped mean in float64, with the
    fp16 file's ``terms`` and magnitudes: loss (fp32) C + 8 + H W terms about the weighted mean of |max| + |log s| + |x_t| + 1; gradient
    (bf16) C + 8 terms about upstream * weight * (softmax (1 + |x - lse| + |lse|) + onehot).  ``extra64``: the pixels whose selection the fp32
    losses leave undecided (util_f16_ref.bootstrap_weight_slack) times |softmax - onehot| / their loss -- bf16 can store the ~1e-13 gradients
    of pixels whose loss is 0 in fp32 and ties with the ignored pixels at the top-k boundary; binary16 cannot, so the fp16 file never met them.
    A NaN logit at a live pixel gives a NaN loss."""
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
        assert la.dtype == torch.float32 and la.dim() == 0 and xa.grad.dtype == BF
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
        slack = _ce_slack(classes, hw, k, thresh)
        within(la.detach(), loss.detach(), classes + 8 + h * w, (weight * per_mag).sum(), (slack * (per.detach() + R.sum_bound(classes + 8, per_mag))).sum(),
               half=False, what=f'loss {k} {thresh}')
        soft = (x64.detach() - lse).exp()
        onehot = torch.zeros_like(soft).scatter_(1, tt, 1.0)
        gmag = up * weight.unsqueeze(1) * (soft * (1 + (x64.detach() - lse).abs() + lse.abs()) + onehot)
        within(xa.grad, x64.grad, classes + 8, gmag, up * slack.unsqueeze(1) * (soft - onehot).abs(), what=f'd logits {k} {thresh}')
    bad = x.clone()
    bad[0, 0, 10, 3] = float('nan')                                              # (a pixel that is not ignored)
    assert bool(torch.isnan(T.bootstrapped_cross_entropy(bad.to(dev), t.to(dev), k=300, thresh=0.3, ignore_index=255)))
