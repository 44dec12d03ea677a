"""The fp32 arm of the training-path kernels against float64, element by element, under the bound derived in util_training_ref.py -- and
every patch-convolution case first asserts the ROUTE and FORM it was written for (hs_patch_conv_bwd_route: the launchers' own predicates),
so a threshold edit that moves a shape to another kernel fails here instead of silently dropping coverage.

CPU tests (unmarked): the fp32 restatement of every case lies inside its own bound, every defect of util_training_ref.DEFECTS is rejected,
one named defect ('dw_tile_last_row_dropped', at an output channel whose gradient is small) passes the old ``rel_err < 1e-4``, the range
inputs reach their regimes, the route query answers what each case table row says, and the tables cover every form the query can return.
GPU tests (``-m gpu``): the kernels through the Python entries training uses (hyperseg_amd.autograd's Functions, training.Adam), every
output allocated inside NaN-pattern guard words.  With HS_TRAINING_F64_REPORT=<file> the GPU run writes one line per case: the route, the
worst err / bound and its index, the worst err / mag64 (profiles/training_f64_bound.txt is such a run; nothing here is tuned to it).  No
tolerance in this file is a measured constant.

Backward / training entry points of include/hyperseg_hip.h and the test that reaches them:
  hs_patch_conv_bwd_input    test_patch_conv_backward (BWD_CASES: dw3 pairs / single, tiny, k1m at every (CT, KQ) and both pixel forms,
                             generic in four padding modes, k 3 and 5, groups 1 / 2 / cin)
  hs_patch_conv_bwd_weight   test_patch_conv_backward (dw3 pairs / single, tiny up to and just over its LDS condition, k1m at every (MT, NT)
                             and its three load forms incl. the alignment drop, generic with one block, two blocks, 150 KB of LDS, grouped blocks)
  hs_patch_conv_bwd_route    test_route_query_answers_the_table, test_tables_cover_every_form
  hs_bn_act_train_fwd, hs_bn_act_train_bwd   test_bn_act_train (BN_CASES: the one-launch and two-launch forms, pairs and single elements;
                             none, ReLU and ReLU6).  The launchers have no query; the cases come from their conditions, quoted at BN_CASES.
  hs_halo_tiles_fwd / _bwd, hs_tile_interior_fwd / _bwd   test_halo_tiles_and_tile_interior (both layouts; copies bit for bit, the halo adjoint bounded)
  hs_dw_tiles_fwd / _bwd_in / _bwd_w   test_dw_tiles (both layouts; 4 x 4, 8 x 12 and 3 x 4 patches: every rows-per-thread form)
  hs_upsample_bilinear_typed_bwd (hs_upsample_bilinear_bwd is its fp32 alias)   test_upsample_bilinear_bwd (2x, non-2x, 1 x 1 source)
  hs_meta_conv_bwd           test_meta_conv_bwd (four padding modes, stride, dilation, groups, depthwise)
  hs_cross_entropy_typed_fwd / _bwd, hs_cross_entropy_weighted_fwd / _bwd (hs_cross_entropy_fwd / _bwd are the fp32 aliases)
                             test_cross_entropy (C = 3: any-count kernel, C = 21: compile-time kernel; ignored pixels; plain and weighted)
  hs_adam_step               test_adam_step (three steps, 1 / 63 / 64 / 257 / 4097 elements in one launch, with and without weight decay)
  hs_s2w_train_fwd / _bwd   test_s2w_train (one unsliced layer on a 1 x 2 grid; two overlapping slices on 3 x 5, batch 2; two on 4 x 4)
  hs_dw_tiles_bn_fwd / _bwd_in / _bwd_w, hs_bn_train_stats_fwd, hs_bn_act_train_bwd_apply, hs_dw_tiles_bn_bwd_in_partials
                             test_dw_tiles_bn (the f16 file's geometry, both layouts; bn_linear_ref with half=False)
  hs_patch_conv_bn_fwd / _bwd_w, hs_patch_conv_plain_bwd_in (fp32: the k1m forms of test_patch_conv_backward behind the same predicate)
                             test_patch_conv_bn (the f16 file's two cases)
  hs_stage_input_typed_fwd's adjoint (hs_upsample_bilinear_typed_bwd with a batch stride)   test_stage_input_adjoint
  hs_bootstrap_mean_of_batch_fwd / _bwd   test_bootstrap_mean_ties (ties at the threshold and at the k-th rank)
  hs_bootstrapped_ce_fwd / _bwd, hs_bootstrapped_ce_weighted_fwd / _bwd   test_bootstrapped_cross_entropy (both selection branches, plain and weighted)
Left out, with the stronger test that covers each:
  hs_patch_conv_plain_bwd_w (fp32)   the same predicate and kernels as hs_patch_conv_bwd_weight's fast forms (test_patch_conv_backward); its
                             own generic kernel is not reached by fp32 training shapes; test_hip_fp16_kernels.py holds it per element at f16_t
  hs_bootstrap_mean_fwd / _bwd, hs_bootstrap_mean_batched_fwd / _bwd   the per-image and per-batch twins of the launches test_bootstrap_mean_ties
                             runs; test_hip_training.py asserts them bit-equal to hs_bootstrap_mean_of_batch_*
  hs_bank_unpack_fwd         a transposing copy: test_hip_training.py compares it bit for bit
  hs_adam_step_amp           test_hip_fp16_training.py: equality with torch's fused Adam under GradScaler; its arithmetic is hs_adam_step's"""
import functools
import os

import pytest
import torch

import util_training_ref as R

gpu = pytest.mark.gpu
GENS = ('benign', 'range')


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.fail('these tests need the MI355X (torch.cuda.is_available() is False)')
    yield torch.device('cuda:0')
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


@functools.lru_cache(maxsize=None)
def _HF():
    from hyperseg_amd import functional
    return functional


@functools.lru_cache(maxsize=None)
def _A():
    from hyperseg_amd import autograd
    return autograd


_REPORT_STARTED = set()


def _report(kernel, route, name, ratio, index, rel):
    path = os.environ.get('HS_TRAINING_F64_REPORT')
    if path:
        mode = 'a' if path in _REPORT_STARTED else 'w'
        _REPORT_STARTED.add(path)
        with open(path, mode) as f:
            f.write(f'{kernel:11s} {str(route):36s} {name:38s} worst err/bound {ratio:.5f} at {index}  worst err/mag64 {rel:.3e}\n')


# ------------------------------------------------------------------------------------------------------------ guarded outputs

GUARD = 64          # floats on either side of an output
PATTERN = 0x7fc0dead


class Guarded:
    """While active, the next fp32 ``torch.empty`` / ``torch.empty_like`` of each shape in ``wanted`` ({shape: offset in floats}) on the GPU
    is a view inside a buffer of NaN-pattern words, ``offset`` floats past a 256-byte boundary (the unaligned cases: 4-byte offsets inside
    an owned buffer).  ``done()`` synchronises and asserts that every view was taken and no word outside the views changed.

    The substitution keys on the shape and takes the FIRST allocation of it, so each use names shapes that only the output has.  The
    allocation sites it stands on (hyperseg_amd/autograd.py): PatchConv.backward ``dx = torch.empty_like(x)`` and _dbank_for's
    ``torch.empty(bank.shape[0], bank.shape[1])`` (the bank's row stride equals its packed row here, else it would be torch.zeros);
    BNActTrain ``y = torch.empty_like(x)``, _bn_adjoint ``dx = torch.empty_like(x)``; HaloTiles / TileInterior / DwTilesValid /
    UpsampleBilinear.backward / MetaConvGeneral.backward ``torch.empty(shape)`` / ``torch.empty_like``.  A site that moves to another
    allocator fails ``done()`` ('no output of shape ... was allocated inside the guards'): loudly, not silently."""

    def __init__(self, dev, wanted):
        self.dev, self.slots, self.taken = dev, {}, {}
        for shape, off in wanted.items():
            n = 1
            for s in shape:
                n *= s
            buf = torch.full((n + 2 * GUARD + 4,), PATTERN, device=dev, dtype=torch.int32)
            self.slots[tuple(shape)] = (buf, buf.view(torch.float32)[GUARD + off:GUARD + off + n].view(shape), GUARD + off, n)

    def _take(self, shape, dtype, device):
        shape = tuple(shape)
        if shape in self.slots and shape not in self.taken and dtype == torch.float32 and str(device).startswith('cuda'):
            self.taken[shape] = self.slots[shape][1]
            return self.taken[shape]
        return None

    def __enter__(self):
        self.real = (torch.empty, torch.empty_like)
        real_empty, real_like = self.real

        def empty(*size, **kw):
            shape = tuple(size[0]) if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)) else tuple(size)
            got = self._take(shape, kw.get('dtype', torch.float32), kw.get('device', ''))
            return got if got is not None else real_empty(*size, **kw)

        def empty_like(t, **kw):
            got = self._take(t.shape, kw.get('dtype', t.dtype), kw.get('device', t.device)) if t.is_contiguous() else None
            return got if got is not None else real_like(t, **kw)
        torch.empty, torch.empty_like = empty, empty_like
        return self

    def __exit__(self, *exc):
        torch.empty, torch.empty_like = self.real

    def intact(self):
        torch.cuda.synchronize()
        for shape, (buf, view, start, n) in self.slots.items():
            assert bool((buf[:start] == PATTERN).all()) and bool((buf[start + n:] == PATTERN).all()), f'guard words around {shape} were overwritten'

    def done(self, outputs):
        torch.cuda.synchronize()
        for shape, (buf, view, start, n) in self.slots.items():
            assert shape in self.taken, f'no output of shape {shape} was allocated inside the guards'
            assert any(o is not None and o.data_ptr() == view.data_ptr() for o in outputs), f'the output of shape {shape} is not the guarded view'
            assert bool((buf[:start] == PATTERN).all()) and bool((buf[start + n:] == PATTERN).all()), f'guard words around {shape} were overwritten'


class _Ctx:
    """What PatchConv's and BNActTrain's forward / backward touch of their ctx: those two tests call the staticmethods directly, on their
    own thread and with their own operand addresses -- the patch-convolution cases assert a route that depends on the addresses of dy and
    dx, and the autograd engine may hand the gradient over in a tensor of its own.  The fields mirror what the Functions' forwards save
    (ctx.meta, ctx.grad_slot, saved_tensors): a change there fails these tests with an AttributeError or a shape error, not silently.
    Every other test here goes through ``apply`` and ``torch.autograd.grad``."""

    def __init__(self, needs=(True, True)):
        self.needs_input_grad, self.saved_tensors = needs, ()

    def save_for_backward(self, *tensors):
        self.saved_tensors = tensors


def _carved(dev, t, off):
    """``t`` on the device, ``off`` floats past a 256-byte boundary inside a larger owned buffer."""
    buf = torch.zeros(t.numel() + 8, device=dev, dtype=torch.float32)
    v = buf[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 256 == 4 * off and v.is_contiguous()
    return v


# ------------------------------------------------------------------------------------------------------------ patch convolution, backward

# The launchers' conditions (hs::bwd_in_form / hs::bwd_w_form, hs_patch_conv_bwd.hip) the shapes are derived from:
#   dw3      k = 3, pad 1, zeros, groups = cin = cout; pairs: even patch and image width, dy | dx (x | dy) 8-byte aligned
#   tiny     k = 1, groups = 1, ph pw < 16; dX: cout <= 1024; dW: cout cin < 2^21 and (cout + cin) 17 4 <= 64 KB, i.e. cout + cin <= 963
#   k1m      k = 1, groups = 1, ph pw >= 16; dX: (CT, KQ) = 16-channel tiles of (cin, cout), CT <= 4 and KQ <= 4 but not (4, 4), or CT = 6 and
#            KQ <= 2; px 2: the pairs condition and ph pw >= 128.  dW: (MT, NT) = tiles of (cout, cin), MT <= 2 and NT <= 4, or MT <= 4 and
#            NT <= 2; vec: pw % 4 = 0, ph pw % 16 = 0, W % 4 = 0, x | dy 16-byte aligned; pairs: else pw, W even and 8-byte aligned; else scalar
#   generic  the rest; dW: ob = output channels beside the X tile in 64 KB, else in 150 KB (whole groups when grouped)
DX_PAIRS = [(1, 1), (1, 2), (1, 3), (1, 4), (2, 1), (2, 2), (2, 3), (2, 4), (3, 1), (3, 2), (3, 3), (3, 4), (4, 1), (4, 2), (4, 3), (6, 1), (6, 2)]
DW_PAIRS = [(1, 1), (1, 2), (1, 3), (1, 4), (2, 1), (2, 2), (2, 3), (2, 4), (3, 1), (3, 2), (4, 1), (4, 2)]


def _pair_channels(ct, kq):
    return (94, 32) if (ct, kq) == (6, 2) else (16 * ct - 3, 16 * kq - 5)


# name -> (B, cin, (H, W), grid, cout, k, mode, groups, (x, dy, dx offsets in floats), dX (route, form), dW (route, form))
BWD_CASES = {}
for _ct, _kq in DX_PAIRS:          # one case per (CT, KQ), 16-pixel patches; the weight gradient sees (MT, NT) = (KQ, CT)
    _cin, _cout = _pair_channels(_ct, _kq)
    _dw = ('k1m', f'mt{_kq}_nt{_ct}_vec') if (_kq, _ct) in DW_PAIRS else ('generic', f'ob{_cout}_blocks1_lds64')
    BWD_CASES[f'k1m ct{_ct} kq{_kq}'] = (1, _cin, (4, 8), (1, 2), _cout, 1, 'zeros', 1, (0, 0, 0), ('k1m', f'ct{_ct}_kq{_kq}_px1'), _dw)
BWD_CASES.update({
    # the non-instantiated neighbours fall to the generic kernels
    'k1m ct4 kq4 -> generic': (1, 61, (4, 8), (1, 2), 59, 1, 'zeros', 1, (0, 0, 0), ('generic', ''), ('generic', 'ob59_blocks1_lds64')),
    'k1m ct5 -> generic':     (1, 77, (4, 8), (1, 2), 11, 1, 'zeros', 1, (0, 0, 0), ('generic', ''), ('generic', 'ob11_blocks1_lds64')),
    # pixels per lane and the load forms: by shape, then by pointer offset alone
    'k1m 8x16 px2':           (1, 20, (8, 32), (1, 2), 10, 1, 'zeros', 1, (0, 0, 0), ('k1m', 'ct2_kq1_px2'), ('k1m', 'mt1_nt2_vec')),
    'k1m 8x16 dx+4':          (1, 20, (8, 32), (1, 2), 10, 1, 'zeros', 1, (0, 0, 1), ('k1m', 'ct2_kq1_px1'), ('k1m', 'mt1_nt2_vec')),
    'k1m 8x16 dy+4':          (1, 20, (8, 32), (1, 2), 10, 1, 'zeros', 1, (0, 1, 0), ('k1m', 'ct2_kq1_px1'), ('k1m', 'mt1_nt2_scalar')),
    'k1m 8x16 x+8':           (1, 20, (8, 32), (1, 2), 10, 1, 'zeros', 1, (2, 0, 0), ('k1m', 'ct2_kq1_px2'), ('k1m', 'mt1_nt2_pairs')),
    'k1m 8x16 x+4':           (1, 20, (8, 32), (1, 2), 10, 1, 'zeros', 1, (1, 0, 0), ('k1m', 'ct2_kq1_px2'), ('k1m', 'mt1_nt2_scalar')),
    'k1m 3x7 partial chunk':  (2, 20, (6, 14), (2, 2), 24, 1, 'zeros', 1, (0, 0, 0), ('k1m', 'ct2_kq2_px1'), ('k1m', 'mt2_nt2_scalar')),
    'k1m 4x12':               (1, 7, (8, 24), (2, 2), 9, 1, 'zeros', 1, (0, 0, 0), ('k1m', 'ct1_kq1_px1'), ('k1m', 'mt1_nt1_vec')),
    'k1m 4x6 pairs':          (1, 18, (4, 12), (1, 2), 5, 1, 'zeros', 1, (0, 0, 0), ('k1m', 'ct2_kq1_px1'), ('k1m', 'mt1_nt2_pairs')),
    'tiny 1x1':               (1, 9, (3, 4), (3, 4), 64, 1, 'zeros', 1, (0, 0, 0), ('tiny', ''), ('tiny', '')),
    'tiny 2x2':               (2, 5, (4, 6), (2, 3), 7, 1, 'zeros', 1, (0, 0, 0), ('tiny', ''), ('tiny', '')),
    'tiny 3x5':               (1, 33, (6, 10), (2, 2), 17, 1, 'zeros', 1, (0, 0, 0), ('tiny', ''), ('tiny', '')),
    'tiny dW at its LDS':     (1, 481, (1, 2), (1, 2), 482, 1, 'zeros', 1, (0, 0, 0), ('tiny', ''), ('tiny', '')),
    'tiny dW over its LDS':   (1, 482, (1, 2), (1, 2), 482, 1, 'zeros', 1, (0, 0, 0), ('tiny', ''), ('generic', 'ob482_blocks1_lds64')),
    'dw3 even':               (2, 5, (8, 12), (2, 3), 5, 3, 'zeros', 5, (0, 0, 0), ('dw3', 'pairs'), ('dw3', 'pairs')),
    'dw3 odd':                (1, 3, (9, 15), (3, 5), 3, 3, 'zeros', 3, (0, 0, 0), ('dw3', 'single'), ('dw3', 'single')),
    'dw3 dx+4':               (1, 4, (8, 12), (2, 3), 4, 3, 'zeros', 4, (0, 0, 1), ('dw3', 'single'), ('dw3', 'pairs')),
    'dw3 x+4':                (1, 4, (8, 12), (2, 3), 4, 3, 'zeros', 4, (1, 0, 0), ('dw3', 'pairs'), ('dw3', 'single')),
    'dw3 5x70 wide':          (1, 2, (5, 70), (1, 1), 2, 3, 'zeros', 2, (0, 0, 0), ('dw3', 'pairs'), ('dw3', 'pairs')),
    'dw3 4x2 patch':          (1, 3, (8, 6), (2, 3), 3, 3, 'zeros', 3, (0, 0, 0), ('dw3', 'pairs'), ('dw3', 'pairs')),
    'gen k3 zeros g1':        (1, 3, (6, 10), (2, 2), 4, 3, 'zeros', 1, (0, 0, 0), ('generic', ''), ('generic', 'ob4_blocks1_lds64')),
    'gen k3 reflect g2':      (2, 4, (6, 10), (2, 2), 6, 3, 'reflect', 2, (0, 0, 0), ('generic', ''), ('generic', 'ob6_blocks1_lds64')),
    'gen k3 replicate dw':    (1, 4, (8, 8), (1, 2), 8, 3, 'replicate', 4, (0, 0, 0), ('generic', ''), ('generic', 'ob8_blocks1_lds64')),
    'gen k3 circular g1':     (1, 3, (6, 10), (2, 2), 4, 3, 'circular', 1, (0, 0, 0), ('generic', ''), ('generic', 'ob4_blocks1_lds64')),
    'gen k3 zeros dw cout 2x': (1, 3, (6, 10), (2, 2), 6, 3, 'zeros', 3, (0, 0, 0), ('generic', ''), ('generic', 'ob6_blocks1_lds64')),
    'gen k3 reflect dw':      (1, 4, (6, 10), (2, 2), 4, 3, 'reflect', 4, (0, 0, 0), ('generic', ''), ('generic', 'ob4_blocks1_lds64')),
    'gen k5 zeros g2':        (1, 4, (8, 8), (1, 1), 4, 5, 'zeros', 2, (0, 0, 0), ('generic', ''), ('generic', 'ob4_blocks1_lds64')),
    'gen k5 reflect dw':      (1, 3, (8, 8), (2, 2), 3, 5, 'reflect', 3, (0, 0, 0), ('generic', ''), ('generic', 'ob3_blocks1_lds64')),
    'gen k5 replicate g1':    (1, 2, (6, 10), (1, 2), 3, 5, 'replicate', 1, (0, 0, 0), ('generic', ''), ('generic', 'ob3_blocks1_lds64')),
    'gen k5 circular g2':     (2, 4, (8, 8), (2, 1), 4, 5, 'circular', 2, (0, 0, 0), ('generic', ''), ('generic', 'ob4_blocks1_lds64')),
    'gen dW two blocks':      (1, 8, (32, 32), (1, 1), 8, 3, 'reflect', 1, (0, 0, 0), ('generic', ''), ('generic', 'ob6_blocks2_lds64')),
    'gen dW 150 KB':          (1, 16, (32, 32), (1, 1), 3, 3, 'zeros', 1, (0, 0, 0), ('generic', ''), ('generic', 'ob3_blocks1_lds150')),
    'gen dW grouped blocks':  (1, 8, (32, 32), (1, 1), 8, 3, 'replicate', 4, (0, 0, 0), ('generic', ''), ('generic', 'ob6_blocks2_lds64')),
})
BWD_PARAMS = [(n, g) for n in BWD_CASES for g in GENS]


@functools.lru_cache(maxsize=None)
def _bwd_case(name, gen):
    b, cin, size, grid, c_out, k, mode, groups = BWD_CASES[name][:8]
    return R.patch_conv_case(gen, sum(map(ord, name)), b, cin, size, grid, c_out, k, mode, groups)


@functools.lru_cache(maxsize=None)
def _bwd_ref(name, gen):
    return R.patch_conv_bwd_ref(_bwd_case(name, gen))


def _bwd_routes(name, align_in=None, align_w=None):
    b, cin, (h, w), grid, c_out, k, mode, groups, (ox, ody, odx) = BWD_CASES[name][:9]
    q = functools.partial(_HF().patch_conv_bwd_route, shape=(b, h, w), c_in=cin, grid=grid, c_out=c_out, k=k, padding=(k - 1) // 2, padding_mode=mode,
                          groups=groups)
    return q('input', align=align_in or (4 * ody, 4 * odx)), q('weight', align=align_w or (4 * ox, 4 * ody))


@pytest.mark.parametrize('name,gen', BWD_PARAMS)
def test_patch_conv_backward_restatement_within_bound(name, gen):
    V = _bwd_ref(name, gen)
    dx, dw = R.patch_conv_grads(_bwd_case(name, gen), torch.float32)
    R.check(dx, V['dx'], f'dX {name} [{gen}]')
    R.check(dw, V['dw'], f'dW {name} [{gen}]')


@pytest.mark.parametrize('name', list(BWD_CASES))
def test_route_query_answers_the_table(name):
    assert _bwd_routes(name) == BWD_CASES[name][9:11], name


def test_tables_cover_every_form():
    """Every answer hs_patch_conv_bwd_route can give is some row's: both dw3 forms, tiny, every instantiated (CT, KQ) and (MT, NT) -- the
    lists of the launchers' HS_BI / HS_BW lines --, both pixel forms and all three load forms, the generic kernel with one and two
    blocks, at 64 KB and 150 KB; and the non-instantiated neighbours (4, 4), CT = 5 for dX and (3, 3) for dW are rows that answer generic."""
    dxs, dws = [c[9] for c in BWD_CASES.values()], [c[10] for c in BWD_CASES.values()]
    for table in (dxs, dws):
        assert {('dw3', 'pairs'), ('dw3', 'single'), ('tiny', '')} <= set(table)
    def pairs(table):                # ('k1m', 'ct2_kq1_px2') -> (2, 1)
        return {tuple(int(p[2:]) for p in f.split('_')[:2]) for r, f in table if r == 'k1m'}
    assert pairs(dxs) == set(DX_PAIRS) and pairs(dws) == set(DW_PAIRS)
    assert {f.split('_')[2] for r, f in dxs if r == 'k1m'} == {'px1', 'px2'}
    assert {f.split('_')[2] for r, f in dws if r == 'k1m'} == {'vec', 'pairs', 'scalar'}
    assert ('generic', '') in dxs
    gen = {f for r, f in dws if r == 'generic'}
    assert any('blocks1_lds64' in f for f in gen) and any('blocks2_lds64' in f for f in gen) and any('lds150' in f for f in gen)
    assert BWD_CASES['k1m ct4 kq4 -> generic'][9][0] == 'generic' and BWD_CASES['k1m ct5 -> generic'][9][0] == 'generic'
    assert BWD_CASES['k1m ct3 kq3'][10][0] == 'generic'                       # dW (3, 3)
    # a sweep of the query itself: no channel count up to 7 tiles answers a k1m pair outside the lists
    HF = _HF()
    for ci in range(1, 8):
        for co in range(1, 8):
            r, f = HF.patch_conv_bwd_route('input', (1, 4, 8), 16 * ci, (1, 2), 16 * co)
            assert (r == 'k1m') == ((ci, co) in DX_PAIRS), (ci, co, r, f)
            r, f = HF.patch_conv_bwd_route('weight', (1, 4, 8), 16 * ci, (1, 2), 16 * co)
            assert (r == 'k1m') == ((co, ci) in DW_PAIRS), (ci, co, r, f)


def test_range_inputs_reach_their_regimes():
    """Every family of gains spans at least 2^12 (2^8 per patch, where a case has few patches: at least two distinct), all operands stay
    normal and every product of three of them far above the flush threshold."""
    for name in ('k1m ct2 kq2', 'gen k3 reflect g2', 'dw3 even', 'tiny 2x2'):
        d = _bwd_case(name, 'range')
        for key in ('x', 'dy', 'row'):
            g = d['gains'][key]
            assert float(g.max() / g.min()) >= 2.0 ** 12, (name, key)
        assert d['gains']['patch'].unique().numel() >= 2, name
        for t in (d['x'], d['dy'], d['bank']):
            nz = t[t != 0].abs()
            assert float(nz.min()) > 2.0 ** -60 and float(nz.max()) < 2.0 ** 40
    for n in BN_CASES:
        d = _bn_case(n, 'range')
        assert float(d['gains']['x'].max() / d['gains']['x'].min()) >= 2.0 ** 16


@pytest.mark.parametrize('name', R.DEFECTS)
def test_defects_are_rejected(name):
    got, V, clean = R.defective(name)
    assert not R.rejects(clean, V), f'{name}: the clean restatement is outside its own bound'
    assert R.rejects(got, V), f'{name}: the bound admits the defect'


def test_a_named_defect_passes_the_old_norm():
    """'dw_tile_last_row_dropped' at an output channel whose upstream gradient is 2^-14 of the largest channel's: the whole row of the
    weight gradient is wrong (zero), test_hip_training.py's ``rel_err < 1e-4`` passes, the per-element bound does not."""
    d = dict(R.patch_conv_case('range', 77, 1, 20, (6, 14), (2, 2), 16, 1, 'zeros', 1))
    d['dy'] = d['dy'].clone()
    d['dy'][:, -1] *= 2.0 ** -8                             # the generator left this channel at 2^-6 of the largest already
    V = R.patch_conv_bwd_ref(d)['dw']
    bad = R.patch_conv_grads(d, torch.float32, defect='dw_tile_last_row_dropped')[1]
    assert R.old_rel_err(bad, V['ref']) < 1e-4
    assert R.rejects(bad, V) and not R.rejects(R.patch_conv_grads(d, torch.float32)[1], V)


def test_adam_statement_within_bound():
    """Three steps over 1, 63, 64, 257 and 4097 elements, with and without weight decay: the fp32 restatement inside the derived bound."""
    for n in (1, 63, 64, 257, 4097):
        for wd in (0.0, 1e-2):
            g = R.G(n)
            p, grads = R.randn(g, n), [R.randn(g, n) * R.pow2_gains(g, n, -8, 8) for _ in range(3)]
            args = (1e-3, (0.5, 0.999), 1e-8, wd)
            for got, V in zip(R.adam_steps(p, grads, *args, dt=torch.float32), R.adam_ref(p, grads, *args)):
                R.check(got, V, f'adam n {n} wd {wd}')


@gpu
@pytest.mark.parametrize('name,gen', BWD_PARAMS)
def test_patch_conv_backward(dev, name, gen):
    A = _A()
    b, cin, (h, w), grid, c_out, k, mode, groups, (ox, ody, odx), dx_route, dw_route = BWD_CASES[name]
    d, V = _bwd_case(name, gen), _bwd_ref(name, gen)
    x, dy, bank = _carved(dev, d['x'], ox), _carved(dev, d['dy'], ody), d['bank'].to(dev)
    with Guarded(dev, {(b, cin, h, w): odx, tuple(bank.shape): 0}) as guards:
        dxv = guards.slots[(b, cin, h, w)][1]
        routes = _bwd_routes(name, (dy.data_ptr() % 16, dxv.data_ptr() % 16), (x.data_ptr() % 16, dy.data_ptr() % 16))
        assert routes == (dx_route, dw_route), name
        ctx = _Ctx()
        ctx.saved_tensors, ctx.meta, ctx.grad_slot = (x, bank), (tuple(grid), c_out, k, (k - 1) // 2, mode, groups), None
        dx, dbank = A.PatchConv.backward(ctx, dy)[:2]
    guards.done((dx, dbank))
    ratio, i, rel = R.check(dx, V['dx'], f'dX {name} [{gen}]')
    _report('conv_bwd_in', '/'.join(dx_route), f'{name} [{gen}]', ratio, i, rel)
    ratio, i, rel = R.check(dbank, V['dw'], f'dW {name} [{gen}]')
    _report('conv_bwd_w', '/'.join(dw_route), f'{name} [{gen}]', ratio, i, rel)


# ------------------------------------------------------------------------------------------------------------ BatchNorm + activation

# hs_bn_act_train_fwd / _bwd (hs_train_aux.hip) have no query; their conditions, quoted:
#     const bool small = (long)batch * pixels <= BN_SMALL_MAX;              // one launch: a workgroup per channel     (BN_SMALL_MAX = 16 * 1024)
#     bn_pairs_ok(a): (a.HW & 1) == 0 && a.HW >= 256   [and 4-byte aligned tensors: every fp32 tensor is]            (the two-launch kernels)
# name -> (B, C, (H, W), form)
BN_CASES = {
    'one launch odd':              (2, 3, (5, 7), 'small'),
    'one launch at its limit':     (1, 2, (128, 128), 'small'),
    'two launches pairs':          (1, 2, (130, 128), 'pairs'),
    'two launches pairs 2 images': (2, 2, (96, 96), 'pairs'),
    'two launches single':         (1, 2, (129, 129), 'single'),
}
BN_PARAMS = [(n, act, g) for n in BN_CASES for act in (0, 1, 2) for g in GENS]


def test_bn_cases_meet_the_quoted_conditions():
    for name, (b, c, (h, w), form) in BN_CASES.items():
        small, pairs = b * h * w <= 16 * 1024, (h * w) % 2 == 0 and h * w >= 256
        assert form == ('small' if small else 'pairs' if pairs else 'single'), name
    assert {c[3] for c in BN_CASES.values()} == {'small', 'pairs', 'single'}


@functools.lru_cache(maxsize=None)
def _bn_case(name, gen):
    b, c, size, _ = BN_CASES[name]
    return R.bn_case(gen, sum(map(ord, name)), b, c, size)


@functools.lru_cache(maxsize=None)
def _bn_ref(name, act, gen):
    return R.bn_ref(_bn_case(name, gen), act)


@pytest.mark.parametrize('name,act,gen', BN_PARAMS)
def test_bn_act_restatement_within_bound(name, act, gen):
    V, got = _bn_ref(name, act, gen), R.bn_restate(_bn_case(name, gen), act)
    for k in ('y', 'dx', 'dg', 'db'):
        R.check(got[k], V[k], f'bn {k} {name} act {act} [{gen}]')


@gpu
@pytest.mark.parametrize('name,act,gen', BN_PARAMS)
def test_bn_act_train(dev, name, act, gen):
    A = _A()
    b, c, (h, w), form = BN_CASES[name]
    d, V = _bn_case(name, gen), _bn_ref(name, act, gen)
    x, r, wt, bias = (d[k].to(dev) for k in ('x', 'r', 'w', 'b'))
    rm, rv = torch.zeros(c, device=dev), torch.ones(c, device=dev)
    ctx = _Ctx()
    with Guarded(dev, {(b, c, h, w): 0}) as guards:
        y = A.BNActTrain.forward(ctx, x, wt, bias, rm, rv, 0.1, 1e-5, act, None)
    guards.done((y,))
    with Guarded(dev, {(b, c, h, w): 0}) as guards:
        dx, dg, db = A.BNActTrain.backward(ctx, r)[:3]
    guards.done((dx,))
    for k, got in (('y', y), ('dx', dx), ('dg', dg), ('db', db)):
        ratio, i, rel = R.check(got, V[k], f'bn {k} {name} act {act} [{gen}]')
        _report('bn_act_' + k, form, f'{name} act {act} [{gen}]', ratio, i, rel)


# ------------------------------------------------------------------------------------------------------------ tile re-layouts, valid depthwise

# (B, C, (H, W), grid): patches 4 x 4 (dw_tiles_bwd_w's 16-lane rows, three tile rows per thread in bwd_in), 4 x 4 in six patches, 8 x 12
# (even, two rows), 3 x 4 (odd height: one row)
TILE_CASES = [(1, 3, (4, 4), (1, 1)), (2, 5, (8, 12), (2, 3)), (1, 2, (8, 12), (1, 1)), (1, 3, (9, 8), (3, 2))]
TILE_PARAMS = [(i, pm, g) for i in range(len(TILE_CASES)) for pm in (False, True) for g in GENS]


@functools.lru_cache(maxsize=None)
def _tile_case(i, gen):
    b, c, size, grid = TILE_CASES[i]
    return R.dw_tiles_case(gen, 500 + i, b, c, size, grid)


@functools.lru_cache(maxsize=None)
def _tile_ref(i, gen):
    return R.dw_tiles_ref(_tile_case(i, gen))


@pytest.mark.parametrize('i', range(len(TILE_CASES)))
@pytest.mark.parametrize('gen', GENS)
def test_dw_tiles_restatement_within_bound(i, gen):
    V, got = _tile_ref(i, gen), R.dw_tiles_restate(_tile_case(i, gen))
    for k in ('y', 'dt', 'dw'):
        R.check(got[k], V[k], f'dw_tiles {k} {i} [{gen}]')


def _layout(t, grid, pm):
    return R.F16.to_patch_major(t, grid).contiguous() if pm else t


@gpu
@pytest.mark.parametrize('i,pm,gen', TILE_PARAMS)
def test_halo_tiles_and_tile_interior(dev, i, pm, gen):
    """hs_halo_tiles_fwd is a gather and hs_tile_interior_fwd / _bwd are copies: bit for bit.  hs_halo_tiles_bwd sums up to nine halo
    cells per pixel: halo_adjoint_ref's bound."""
    A = _A()
    b, c, (h, w), grid = TILE_CASES[i]
    d = _tile_case(i, gen)
    x = d['x'].to(dev).requires_grad_(True)
    t_ref = _layout(d['t'], grid, pm)
    with Guarded(dev, {tuple(t_ref.shape): 0}) as guards:
        t = A.HaloTiles.apply(x, grid, pm)
    guards.done((t,))
    assert torch.equal(t.detach().cpu(), t_ref)
    g = R.G(900 + 2 * i + (gen == 'range'))
    dt_img = R.randn(g, *d['t'].shape) * (R.pow2_gains(g, c, -6, 6).view(1, -1, 1, 1) if gen == 'range' else 1.0)
    with Guarded(dev, {(b, c, h, w): 0}) as guards:
        dx, = torch.autograd.grad(t, x, _layout(dt_img, grid, pm).to(dev))
    guards.done((dx,))
    ratio, idx, rel = R.check(dx, R.halo_adjoint_ref(d['x'], dt_img, grid), f'halo bwd {i} pm {pm} [{gen}]')
    _report('halo_bwd', 'patch_major' if pm else 'image', f'tile case {i} [{gen}]', ratio, idx, rel)
    if not pm:                                                       # TileInterior takes the image of tiles
        ti = d['t'].to(dev).requires_grad_(True)
        with Guarded(dev, {(b, c, h, w): 0}) as guards:
            y = A.TileInterior.apply(ti, (h, w), grid)
        guards.done((y,))
        assert torch.equal(y.detach().cpu(), R.F16.tile_interior(d['t'], (h, w), grid))
        with Guarded(dev, {tuple(d['t'].shape): 0}) as guards:
            dti, = torch.autograd.grad(y, ti, d['dy'].to(dev))
        guards.done((dti,))
        assert torch.equal(dti.cpu(), R.tile_interior_adjoint(d['t'].shape, d['dy'], (h, w), grid))


@gpu
@pytest.mark.parametrize('i,pm,gen', TILE_PARAMS)
def test_dw_tiles(dev, i, pm, gen):
    A = _A()
    b, c, (h, w), grid = TILE_CASES[i]
    d, V = _tile_case(i, gen), _tile_ref(i, gen)
    t = _layout(d['t'], grid, pm).to(dev).requires_grad_(True)
    bank = d['bank'].to(dev).requires_grad_(True)
    assert A.dw_tiles_supported(t, (h, w), grid)
    with Guarded(dev, {(b, c, h, w): 0}) as guards:
        y = A.DwTilesValid.apply(t, bank, (h, w), grid, pm)
    guards.done((y,))
    with Guarded(dev, {tuple(t.shape): 0, tuple(bank.shape): 0}) as guards:
        dt, dw = torch.autograd.grad(y, (t, bank), d['dy'].to(dev))
    guards.done((dt, dw))
    dt_img = R.F16.from_patch_major(dt.cpu(), b, grid) if pm else dt
    form = 'patch_major' if pm else 'image'
    for k, got in (('y', y), ('dt', dt_img), ('dw', dw)):
        ratio, idx, rel = R.check(got, V[k], f'dw_tiles {k} {i} pm {pm} [{gen}]')
        _report('dw_tiles_' + k, form, f'tile case {i} [{gen}]', ratio, idx, rel)


# ------------------------------------------------------------------------------------------------------------ bilinear resize, adjoint

# (B, C, (Hi, Wi), (Ho, Wo)): exact 2x (the 2 x 2 form), odd sizes at a non-2x ratio, a 1 x 1 source, a wide non-2x row
UPB_CASES = [(2, 3, (5, 7), (10, 14)), (1, 2, (5, 7), (13, 9)), (1, 3, (1, 1), (4, 6)), (1, 1, (3, 5), (7, 31))]


@functools.lru_cache(maxsize=None)
def _upb_case(i, gen):
    b, c, si, so = UPB_CASES[i]
    g = R.G(700 + 2 * i + (gen == 'range'))
    dy = R.randn(g, b, c, *so)
    return dy * R.pow2_gains(g, c, -12, 12).view(1, -1, 1, 1) if gen == 'range' else dy


@pytest.mark.parametrize('i', range(len(UPB_CASES)))
@pytest.mark.parametrize('gen', GENS)
def test_upsample_adjoint_restatement_within_bound(i, gen):
    dy, si = _upb_case(i, gen), UPB_CASES[i][2]
    R.check(R.upsample_adjoint(dy, si, torch.float32), R.upsample_adjoint_ref(dy, si), f'upsample bwd {i} [{gen}]')


@gpu
@pytest.mark.parametrize('i', range(len(UPB_CASES)))
@pytest.mark.parametrize('gen', GENS)
def test_upsample_bilinear_bwd(dev, i, gen):
    A = _A()
    b, c, si, so = UPB_CASES[i]
    dy = _upb_case(i, gen)
    x = torch.zeros(b, c, *si, device=dev, requires_grad=True)
    y = A.upsample_bilinear(x, so)
    assert y.grad_fn is not None and type(y.grad_fn).__name__.startswith('UpsampleBilinear')
    with Guarded(dev, {(b, c) + si: 0}) as guards:
        dx, = torch.autograd.grad(y, x, dy.to(dev))
    guards.done((dx,))
    ratio, idx, rel = R.check(dx, R.upsample_adjoint_ref(dy, si), f'upsample bwd {i} [{gen}]')
    _report('upsample_bwd', '2x' if so == (2 * si[0], 2 * si[1]) else 'general', f'upsample case {i} [{gen}]', ratio, idx, rel)


# ------------------------------------------------------------------------------------------------------------ meta_conv, adjoints

# name -> (B, c_in, (H, W), c_out, (kh, kw), stride, pad, dilation, mode, groups)
METAB_CASES = {
    'zeros 3x3':           (2, 4, (7, 9), 5, (3, 3), (1, 1), (1, 1), (1, 1), 'zeros', 1),
    'reflect 3x5 uneven':  (1, 3, (8, 11), 4, (3, 5), (1, 1), (1, 2), (1, 1), 'reflect', 1),
    'replicate stride 2':  (1, 4, (9, 10), 6, (3, 3), (2, 2), (1, 1), (1, 1), 'replicate', 2),
    'circular dilation 2': (2, 2, (8, 8), 3, (3, 2), (1, 1), (2, 1), (2, 2), 'circular', 1),
    'zeros 1x4 s2 d2 dw':  (1, 6, (6, 13), 6, (1, 4), (1, 2), (0, 3), (1, 2), 'zeros', 6),
}
METAB_PARAMS = [(n, g) for n in METAB_CASES for g in GENS]


@functools.lru_cache(maxsize=None)
def _metab_case(name, gen):
    b, cin, (h, w), c_out, k, stride, pad, dil, mode, groups = METAB_CASES[name]
    g = R.G(sum(map(ord, name)) * 2 + (gen == 'range'))
    n = (cin // groups) * k[0] * k[1]
    d = dict(x=R.randn(g, b, cin, h, w), w=R.randn(g, b, c_out * n) * n ** -0.5, c_out=c_out, k=k, stride=stride, pad=pad, dil=dil, mode=mode, groups=groups)
    dy = R.randn(g, *R.D.meta_conv(d).shape)
    if gen == 'range':
        d['x'] = d['x'] * R.pow2_gains(g, cin, -6, 6).view(1, -1, 1, 1)
        d['w'] = (d['w'].view(b, c_out, n) * R.pow2_gains(g, c_out, -6, 6).view(1, -1, 1) * R.pow2_gains(g, n, -6, 6).view(1, 1, -1)).reshape(b, -1)
        dy = dy * R.pow2_gains(g, c_out, -6, 6).view(1, -1, 1, 1)
    return d, dy


@functools.lru_cache(maxsize=None)
def _metab_ref(name, gen):
    return R.meta_conv_bwd_ref(*_metab_case(name, gen))


@pytest.mark.parametrize('name,gen', METAB_PARAMS)
def test_meta_conv_adjoints_restatement_within_bound(name, gen):
    V, got = _metab_ref(name, gen), R.meta_conv_grads(*_metab_case(name, gen), torch.float32)
    R.check(got[0], V['dx'], f'meta dx {name} [{gen}]')
    R.check(got[1], V['dw'], f'meta dw {name} [{gen}]')


@gpu
@pytest.mark.parametrize('name,gen', METAB_PARAMS)
def test_meta_conv_bwd(dev, name, gen):
    """hs_meta_conv_bwd through autograd.meta_conv_general: the kernel's dx is the PADDED input's for the non-zero modes (F.pad's adjoint,
    stock, folds it back), so the guarded dx has the padded shape there."""
    A = _A()
    b, cin, (h, w), c_out, k, stride, (ph, pw), dil, mode, groups = METAB_CASES[name]
    (d, dy), V = _metab_case(name, gen), _metab_ref(name, gen)
    x, wt = d['x'].to(dev).requires_grad_(True), d['w'].to(dev).requires_grad_(True)
    y = A.meta_conv_general(x, wt, c_out, k, stride, (ph, pw), dil, mode, groups)
    assert tuple(y.shape) == tuple(dy.shape)
    kdx = (b, cin, h, w) if mode == 'zeros' or not (ph or pw) else (b, cin, h + ph + pw, w + ph + pw)
    with Guarded(dev, {kdx: 0, tuple(wt.shape): 0}) as guards:
        dx, dw = torch.autograd.grad(y, (x, wt), dy.to(dev))
    torch.cuda.synchronize()
    guards.intact()
    assert set(guards.taken) == set(guards.slots), 'the kernel outputs were not allocated inside the guards'
    for key, got in (('dx', dx), ('dw', dw)):
        ratio, idx, rel = R.check(got, V[key], f'meta {key} {name} [{gen}]')
        _report('meta_bwd_' + key, mode, f'{name} [{gen}]', ratio, idx, rel)


# ------------------------------------------------------------------------------------------------------------ Adam

ADAM_SIZES = (1, 63, 64, 257, 4097)
ADAM_ARGS = (1e-3, (0.5, 0.999), 1e-8)


@functools.lru_cache(maxsize=None)
def _adam_case(n):
    g = R.G(n)
    return R.randn(g, n), tuple(R.randn(g, n) * R.pow2_gains(g, n, -8, 8) for _ in range(3))


@gpu
@pytest.mark.parametrize('wd', [0.0, 1e-2])
def test_adam_step(dev, wd):
    """Three steps of training.Adam (hs_adam_step: the five tensors in one launch, the vector and the tail forms) against float64 Adam,
    every parameter inside guard words, after every step."""
    from hyperseg_amd.training import Adam
    guards = Guarded(dev, {(n,): 0 for n in ADAM_SIZES})
    params = []
    for n in ADAM_SIZES:
        view = guards.slots[(n,)][1]
        view.copy_(_adam_case(n)[0])
        params.append(torch.nn.Parameter(view))
        assert params[-1].data_ptr() == view.data_ptr()
    opt = Adam(params, lr=ADAM_ARGS[0], betas=ADAM_ARGS[1], eps=ADAM_ARGS[2], weight_decay=wd)
    refs = [R.adam_ref(_adam_case(n)[0], _adam_case(n)[1], *ADAM_ARGS, wd) for n in ADAM_SIZES]
    for s in range(3):
        for p, n in zip(params, ADAM_SIZES):
            p.grad = _adam_case(n)[1][s].to(dev)
        opt.step()
        guards.intact()
        for p, n, V in zip(params, ADAM_SIZES, refs):
            ratio, idx, rel = R.check(p.detach(), V[s], f'adam n {n} step {s + 1} wd {wd}')
            _report('adam', f'wd{wd}', f'n {n} step {s + 1}', ratio, idx, rel)


# ------------------------------------------------------------------------------------------------------------ cross entropy

# (B, C, (H, W)): C = 3 takes the any-count kernel, C = 21 the compile-time one; plain and weighted
CE_CASES = [(2, 3, (5, 7)), (2, 21, (5, 7)), (1, 21, (3, 70))]
CE_PARAMS = [(i, wt, g) for i in range(len(CE_CASES)) for wt in (False, True) for g in GENS]


@functools.lru_cache(maxsize=None)
def _ce_case(i, wt, gen):
    b, c, size = CE_CASES[i]
    return R.ce_case(gen, 800 + i, b, c, size, weighted=wt)


@pytest.mark.parametrize('i,wt,gen', CE_PARAMS)
def test_cross_entropy_restatement_within_bound(i, wt, gen):
    d = _ce_case(i, wt, gen)
    V, (loss, dl) = R.ce_ref(d), R.ce_restate(d)
    assert bool((d['target'] == d['ignore_index']).any()) and bool((V['loss']['ref'][d['target'] == d['ignore_index']] == 0).all())
    R.check(loss, V['loss'], f'ce loss {i} w {wt} [{gen}]')
    R.check(dl, V['dl'], f'ce dl {i} w {wt} [{gen}]')


@gpu
@pytest.mark.parametrize('i,wt,gen', CE_PARAMS)
def test_cross_entropy(dev, i, wt, gen):
    A = _A()
    b, c, size = CE_CASES[i]
    d = _ce_case(i, wt, gen)
    V = R.ce_ref(d)
    x = d['logits'].to(dev).requires_grad_(True)
    weight = d['weight'].to(dev) if wt else None
    with Guarded(dev, {(b,) + size: 0}) as guards:
        loss = A.PixelCrossEntropy.apply(x, d['target'].to(dev), d['ignore_index'], weight)
    guards.done((loss,))
    with Guarded(dev, {(b, c) + size: 0}) as guards:
        dl, = torch.autograd.grad(loss, x, d['g'].to(dev))
    guards.done((dl,))
    form = ('weighted' if wt else 'plain') + ('_c21' if c == 21 else '_any')
    for key, got in (('loss', loss), ('dl', dl)):
        ratio, idx, rel = R.check(got, V[key], f'ce {key} {i} w {wt} [{gen}]')
        _report('ce_' + key, form, f'ce case {i} [{gen}]', ratio, idx, rel)


# ------------------------------------------------------------------------------------------------------------ signal2weights, training

# name -> (B, C, grid, [(signal_index, signal_channels, groups, wc, rows)])
S2W_CASES = {
    'unsliced 1x2':        (1, 12, (1, 2), [(0, 12, 3, 9, 7)]),
    'two slices 3x5 b2':   (2, 29, (3, 5), [(8, 16, 4, 24, 22), (0, 10, 2, 10, 10)]),
    'two slices 4x4':      (1, 24, (4, 4), [(0, 24, 8, 40, 37), (4, 12, 3, 6, 5)]),
}
S2W_PARAMS = [(n, g) for n in S2W_CASES for g in GENS]


@functools.lru_cache(maxsize=None)
def _s2w_case(name, gen):
    b, c, grid, layers = S2W_CASES[name]
    return R.s2w_case(gen, sum(map(ord, name)), b, c, grid, layers)


@functools.lru_cache(maxsize=None)
def _s2w_ref(name, gen):
    return R.s2w_train_ref(_s2w_case(name, gen))


def _s2w_check(got, V, what, report=None):
    banks, ds, dws = got
    for j, (bk, dw) in enumerate(zip(banks, dws)):
        for key, g, v in (('bank', bk, V['banks'][j]), ('dw', dw, V['dws'][j])):
            out = R.check(g, v, f'{what} {key} {j}')
            if report:
                report('s2w_' + key, f'layer{j}', *out)
    out = R.check(ds, V['ds'], f'{what} dsignal')
    if report:
        report('s2w_ds', 'sum', *out)


@pytest.mark.parametrize('name,gen', S2W_PARAMS)
def test_s2w_train_restatement_within_bound(name, gen):
    _s2w_check(R.s2w_train(_s2w_case(name, gen), torch.float32), _s2w_ref(name, gen), f'{name} [{gen}]')


@gpu
@pytest.mark.parametrize('name,gen', S2W_PARAMS)
def test_s2w_train(dev, name, gen):
    """hs_s2w_train_fwd / _bwd through autograd.S2WBanksTrain: every bank (columns [rows, ld) are row padding: not compared), dsignal -- the
    sum over the layers' slices -- and every layer's weight gradient.  The per-layer d signal slices are kernel outputs too and may take
    the guarded buffer of the signal's shape (an unsliced layer's has it): the guards are checked for having been used and left intact."""
    A = _A()
    b, c, grid, layers = S2W_CASES[name]
    d, V = _s2w_case(name, gen), _s2w_ref(name, gen)
    p = b * grid[0] * grid[1]
    meta = [dict(signal_index=l['index'], signal_channels=l['channels'], groups=l['groups'], rows=l['rows']) for l in d['layers']]
    lds = [(l['rows'] + 3) // 4 * 4 for l in d['layers']]
    sig = d['signal'].to(dev).requires_grad_(True)
    ws = [l['wsw'].view(*l['wsw'].shape, 1, 1).to(dev).requires_grad_(True) for l in d['layers']]
    with Guarded(dev, {(p * sum(lds),): 0}) as guards:
        banks = A.S2WBanksTrain.apply(meta, sig, *ws)
    guards.intact()
    assert set(guards.taken) == set(guards.slots)
    ups = []
    for l, ld in zip(d['layers'], lds):
        u = torch.zeros(p, ld, device=dev)
        u[:, :l['rows']] = l['dbank'].to(dev)
        ups.append(u)
    with Guarded(dev, {tuple(t.shape): 0 for t in [sig] + ws}) as guards:
        grads = torch.autograd.grad(banks, [sig] + ws, ups)
    guards.intact()
    assert set(guards.taken) == set(guards.slots)
    got = ([bk[:, :l['rows']] for bk, l in zip(banks, d['layers'])], grads[0], [g.flatten(1) for g in grads[1:]])
    _s2w_check(got, V, f'{name} [{gen}]', lambda k, r, *o: _report(k, r, f'{name} [{gen}]', *o))


# ------------------------------------------------------------------------------------------------------------ stage input, adjoint

# (B, (H, W), c_skip, c_prev, prev size, coords): exact 2x, a 1 x 1 previous level, a non-2x ratio, no coordinates
STAGE_ADJ_CASES = [(2, (6, 10), 1, 3, (3, 5), True), (1, (7, 9), 2, 2, (1, 1), True), (1, (9, 5), 2, 3, (4, 3), False), (2, (10, 14), 5, 3, (5, 7), True)]


def _stage_adj_case(i, gen):
    b, (h, w), cs, cp, ps, coords = STAGE_ADJ_CASES[i]
    g = R.G(1100 + 2 * i + (gen == 'range'))
    skip, prev, r = R.randn(g, b, cs, h, w), R.randn(g, b, cp, *ps), R.randn(g, b, 2 * coords + cs + cp, h, w)
    if gen == 'range':
        r = r * R.pow2_gains(g, r.shape[1], -10, 10).view(1, -1, 1, 1)
    return skip, prev, coords, r


@pytest.mark.parametrize('i', range(len(STAGE_ADJ_CASES)))
@pytest.mark.parametrize('gen', GENS)
def test_stage_adjoint_restatement_within_bound(i, gen):
    skip, prev, coords, r = _stage_adj_case(i, gen)
    ds, V = R.stage_adjoint_ref(skip, prev, coords, r)
    off = 2 * coords + skip.shape[1]
    R.check(R.upsample_adjoint(r[:, off:], tuple(prev.shape[-2:]), torch.float32), V, f'stage adjoint {i} [{gen}]')


@gpu
@pytest.mark.parametrize('i', range(len(STAGE_ADJ_CASES)))
@pytest.mark.parametrize('gen', GENS)
def test_stage_input_adjoint(dev, i, gen):
    A, HF = _A(), _HF()
    skip, prev, coords, r = _stage_adj_case(i, gen)
    ds, V = R.stage_adjoint_ref(skip, prev, coords, r)
    sk, pv = skip.to(dev).requires_grad_(True), prev.to(dev).requires_grad_(True)
    y = A.materialize_stage(HF.StageInput(sk, pv, coords=coords))
    assert type(y.grad_fn).__name__.startswith('StageMaterialize')
    with Guarded(dev, {tuple(prev.shape): 0}) as guards:
        dsk, dpv = torch.autograd.grad(y, (sk, pv), r.to(dev))
    guards.done((dpv,))
    assert torch.equal(dsk.cpu().double(), ds)
    ratio, idx, rel = R.check(dpv, V, f'stage adjoint {i} [{gen}]')
    _report('stage_adj', '2x' if skip.shape[2] == 2 * prev.shape[2] and skip.shape[3] == 2 * prev.shape[3] else 'general', f'stage case {i} [{gen}]', ratio, idx, rel)


# ------------------------------------------------------------------------------------------------------------ BatchNorm + ReLU6 + a linear layer

DW_BN_GEOM = (2, 6, 10, 10, 7, 8)                                   # test_hip_fp16_kernels.py's: B, C, fh, fw, ph, pw
CONV_BN_CASES = [(13, 5, (12, 12), 8), (24, 8, (2, 3), 8)]          # likewise: c, c_out, grid, patch edge (B = 2)


def _bn_module(d, dev):
    bn = torch.nn.BatchNorm2d(d['w'].numel(), momentum=0.1).train()
    with torch.no_grad():
        bn.weight.copy_(d['w'])
        bn.bias.copy_(d['b'])
    return bn.to(dev)


def _bn_linear_compare(kernel, form, name, got, V):
    for k, g in got.items():
        ratio, idx, rel = R.check(g, V[k], f'{name} {k}')
        _report(f'{kernel}_{k}', form, name, ratio, idx, rel)


@functools.lru_cache(maxsize=None)
def _dw_bn_case(pm, gen):
    b, c, fh, fw, ph, pw = DW_BN_GEOM
    shape = (b * fh * fw, c, ph + 2, pw + 2) if pm else (b, c, fh * (ph + 2), fw * (pw + 2))
    d = R.bn_linear_case(gen, 1200 + pm, shape, (b * fh * fw, 9 * c), (b, c, fh * ph, fw * pw))
    size, grid = (fh * ph, fw * pw), (fh, fw)
    return d, R.bn_linear_V(d, lambda z, k: R.F16.dw_tiles_valid(z, k, size, grid, pm), (9, 9, ph * pw))


@gpu
@pytest.mark.parametrize('pm', [True, False])
@pytest.mark.parametrize('gen', GENS)
def test_dw_tiles_bn(dev, pm, gen):
    """autograd.DwTilesBN at fp32 with the flags training runs with: hs_bn_train_stats_fwd + hs_dw_tiles_bn_fwd, hs_dw_tiles_bn_bwd_w,
    hs_dw_tiles_bn_bwd_in + hs_bn_act_train_bwd_apply, against batch_norm -> relu6 -> valid depthwise in float64 (bn_linear_ref,
    half=False): output, all four gradients, the running statistics."""
    import torch.nn as nn
    A = _A()
    b, c, fh, fw, ph, pw = DW_BN_GEOM
    size, grid = (fh * ph, fw * pw), (fh, fw)
    d, V = _dw_bn_case(pm, gen)
    bn = _bn_module(d, dev)
    t, bank = d['x'].to(dev).requires_grad_(True), d['bank'].to(dev).requires_grad_(True)
    assert A.USE_DW_BN_FUSED and A.USE_DW_BN_BWD_FUSED
    with Guarded(dev, {(b, c) + size: 0}) as guards:
        y = A.dw_tiles_bn(bn, nn.ReLU6(), t, bank, size, grid, pm)
    guards.done((y,))
    assert type(y.grad_fn).__name__.startswith('DwTilesBN')
    with Guarded(dev, {tuple(t.shape): 0, tuple(bank.shape): 0}) as guards:
        dx, dbank, dg, db = torch.autograd.grad(y, (t, bank, bn.weight, bn.bias), d['r'].to(dev))
    guards.done((dx, dbank))
    _bn_linear_compare('dw_bn', 'patch_major' if pm else 'image', f'dw_tiles_bn [{gen}]',
                       dict(y=y, dx=dx, dbank=dbank, dg=dg, db=db, rm=bn.running_mean, rv=bn.running_var), V)


@functools.lru_cache(maxsize=None)
def _conv_bn_case(i, gen):
    c, cout, (fh, fw), p = CONV_BN_CASES[i]
    d = R.bn_linear_case(gen, 1300 + i, (2, c, fh * p, fw * p), (2 * fh * fw, cout * c), (2, cout, fh * p, fw * p))
    d['bank'] = d['bank'] * c ** -0.5
    return d, R.bn_linear_V(d, lambda z, k: R.F16.patch_k1(z, k, (fh, fw), cout), (c, cout, p * p))


@gpu
@pytest.mark.parametrize('i', range(len(CONV_BN_CASES)))
@pytest.mark.parametrize('gen', GENS)
def test_patch_conv_bn(dev, i, gen):
    """autograd.PatchConvBN at fp32: hs_bn_train_stats_fwd + hs_patch_conv_bn_fwd, hs_patch_conv_bn_bwd_w, hs_patch_conv_plain_bwd_in +
    hs_bn_act_train_bwd, against batch_norm -> relu6 -> per-patch matmul (util_f16_ref.patch_k1) in float64.  The input gradient is the
    SECOND tensor of x's shape the backward allocates (the first is the never-returned gradient of the normalised map), so the guards
    hold y and the weight gradient."""
    import torch.nn as nn
    A = _A()
    c, cout, grid, p = CONV_BN_CASES[i]
    d, V = _conv_bn_case(i, gen)
    bn = _bn_module(d, dev)
    x, bank = d['x'].to(dev).requires_grad_(True), d['bank'].to(dev).requires_grad_(True)
    with Guarded(dev, {tuple(d['r'].shape): 0}) as guards:
        y = A.patch_conv_bn(bn, nn.ReLU6(), x, bank, grid, cout)
    guards.done((y,))
    fused = type(y.grad_fn).__name__.startswith('PatchConvBN')
    assert fused == (p * p >= 64), 'hs_patch_conv_bn_fwd takes patches of >= 64 pixels; smaller ones the two Functions'
    with Guarded(dev, {tuple(bank.shape): 0}) as guards:
        dx, dbank, dg, db = torch.autograd.grad(y, (x, bank, bn.weight, bn.bias), d['r'].to(dev))
    guards.done((dbank,))
    _bn_linear_compare('conv_bn', 'fused' if fused else 'two_functions', f'patch_conv_bn {i} [{gen}]',
                       dict(y=y, dx=dx, dbank=dbank, dg=dg, db=db, rm=bn.running_mean, rv=bn.running_var), V)


@pytest.mark.parametrize('gen', GENS)
def test_bn_linear_restatements_within_bound(gen):
    """The fp32 CPU restatement of both fused layers inside bn_linear_ref(half=False)'s bound."""
    b, c, fh, fw, ph, pw = DW_BN_GEOM
    cases = [(_dw_bn_case(True, gen), lambda z, k: R.F16.dw_tiles_valid(z, k, (fh * ph, fw * pw), (fh, fw), True))]
    for i, (cc, cout, grid, p) in enumerate(CONV_BN_CASES):
        cases.append((_conv_bn_case(i, gen), lambda z, k, grid=grid, cout=cout: R.F16.patch_k1(z, k, grid, cout)))
    for (d, V), lin in cases:
        x, w, bb, bank = (d[k].clone().requires_grad_(True) for k in ('x', 'w', 'b', 'bank'))
        y = lin(R.F16.bn_relu6(x, w, bb), bank)
        dx, dbank, dg, db = torch.autograd.grad(y, (x, bank, w, bb), d['r'])
        for k, g in dict(y=y.detach(), dx=dx, dbank=dbank, dg=dg, db=db).items():
            R.check(g, V[k], f'bn_linear {k} [{gen}]')


# ------------------------------------------------------------------------------------------------------------ bootstrapped mean and loss

# (k, thresh): the threshold branch with values tied AT the threshold; the top-k branch with values tied at the k-th rank
BM_RULES = [(50, 1.0), (50, 3.0)]


def _bm_values():
    return (R.randn(R.G(41), 2, 300).abs() * 4).round() / 4           # multiples of 1/4: many ties, some exactly at either threshold


def test_bootstrap_statement_equals_the_sorted_one():
    v = _bm_values().double()
    for k, thresh in BM_RULES:
        assert abs(float(R.bootstrap_mean_tied(v, k, thresh) - R.F16.bootstrapped_mean(v, k, thresh))) < 1e-14
        ranked = v.sort(1, descending=True).values
        if bool((ranked[:, k] > thresh).all()):                      # the threshold branch: some values sit exactly AT the threshold
            assert bool((v == thresh).any())
        else:                                                        # the top-k branch, in every image: the k-th and (k+1)-th tie
            assert bool((ranked[:, k] <= thresh).all()) and bool((ranked[:, k - 1] == ranked[:, k]).all())


@gpu
@pytest.mark.parametrize('k,thresh', BM_RULES)
def test_bootstrap_mean_ties(dev, k, thresh):
    A = _A()
    v = _bm_values()
    V = R.bootstrap_mean_ref(v, k, thresh, up=1.75)
    vd = v.to(dev).requires_grad_(True)
    with Guarded(dev, {(2 * 8 + 1,): 0}) as guards:
        loss = A.BootstrapMeanOfBatch.apply(vd, k, thresh)
    guards.intact()
    assert set(guards.taken) == set(guards.slots)
    with Guarded(dev, {tuple(v.shape): 0}) as guards:
        dv, = torch.autograd.grad(loss, vd, torch.tensor(1.75, device=dev))
    guards.done((dv,))
    for key, got in (('loss', loss.detach()), ('dv', dv)):
        ratio, idx, rel = R.check(got, V[key], f'bootstrap mean {key} k {k} thresh {thresh}')
        _report('bm_' + key, 'threshold' if thresh == 1.0 else 'top_k', f'ties k {k} thresh {thresh}', ratio, idx, rel)


# (case of CE_CASES, weighted, k, thresh): 3 x 70 = 210 pixels an image, 5 x 7 = 35
BCE_RULES = [(2, False, 60, 0.3), (2, True, 60, 50.0), (1, False, 12, 0.3), (1, True, 12, 50.0)]
BCE_PARAMS = [r + (g,) for r in BCE_RULES for g in GENS]


@functools.lru_cache(maxsize=None)
def _bce_ref(i, wt, k, thresh, gen):
    return R.bootstrapped_ce_ref(_ce_case(i, wt, gen), k, thresh, up=1.75)


@pytest.mark.parametrize('i,wt,k,thresh,gen', BCE_PARAMS)
def test_bootstrapped_ce_cases_keep_the_selection_decided(i, wt, k, thresh, gen):
    assert _bce_ref(i, wt, k, thresh, gen)['decided']


@gpu
@pytest.mark.parametrize('i,wt,k,thresh,gen', BCE_PARAMS)
def test_bootstrapped_cross_entropy(dev, i, wt, k, thresh, gen):
    import hyperseg_amd.training as T
    b, c, size = CE_CASES[i]
    d, V = _ce_case(i, wt, gen), _bce_ref(i, wt, k, thresh, gen)
    assert V['decided']
    x = d['logits'].to(dev).requires_grad_(True)
    with Guarded(dev, {(b, size[0] * size[1]): 0, (b * 8 + 1,): 0}) as guards:
        loss = T.bootstrapped_cross_entropy(x, d['target'].to(dev), k=k, thresh=thresh, weight=d['weight'].to(dev) if wt else None, ignore_index=d['ignore_index'])
    guards.intact()
    assert type(loss.grad_fn).__name__.startswith('BootstrappedCrossEntropy') and set(guards.taken) == set(guards.slots)
    with Guarded(dev, {(b, c) + size: 0}) as guards:
        dl, = torch.autograd.grad(loss, x, torch.tensor(1.75, device=dev))
    guards.done((dl,))
    form = ('weighted' if wt else 'plain') + ('_topk' if thresh > 10 else '_thresh')
    for key, got in (('loss', loss.detach()), ('dl', dl)):
        ratio, idx, rel = R.check(got, V[key], f'bootstrapped ce {key} {i} [{gen}]')
        _report('bce_' + key, form, f'ce case {i} k {k} [{gen}]', ratio, idx, rel)
