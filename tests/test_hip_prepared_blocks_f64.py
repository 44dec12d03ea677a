"""The prepared encoder blocks of utils/inference.py (FusedMBConv, FusedPointwise, FusedStem via block 0, FusedContextHead, wired by
_fuse_backbone) against the STOCK modules in float64, element by element, under the bound derived in util_block_ref.py -- and every
case first asserts the LAUNCH SEQUENCE it was written for (recorded through pass-through wrappers of hyperseg_amd.functional), so a
threshold edit that moves a block to another sequence fails here instead of silently moving coverage.

The relation: a prepared block receives x32 standing for x32 + in_offset and returns y standing for y + out_offset (both the fp32
buffers of the prepared model, taken as exact float64): reference input x32.double() + in_offset.double(), value compared
got.double() + out_offset.double().  Inputs are x - in_offset rounded to fp32.  One block per case, at a map of the case's choosing.

Branches of FusedMBConv.forward and the case form that reaches them (CASES: block, map, batch, generator, forms with split on / off):
  image input, stem_dw launches            exp 'stem_dw'   (block 0 at 128 x 256 and 64 x 128)
  image input, stem_dw refuses             exp 'stem+dw'   (block 0 at 60 x 136: stem launch + depthwise launch)
  mbconv_expand_dw                         exp 'fused'     (Cin <= 40, output map >= 2048: 32 x 64; just under it, 30 x 68, takes 'raw')
  expand on the MFMA pointwise kernel      exp 'mfma'      (block 9 at 64 x 128; 60 x 136 takes 'raw')
  raw expand GEMM + BN0/swish prologue     exp 'raw_split' / 'raw_lib'
  no expand                                exp 'none'      (block 1)
  gemm_split_se                            proj 'split_se' (deferred; deferred onto the skip in place; not deferred, shift + residual: block 1)
  se_gate + gemm_split                     proj 'se+split' (more than 512 mid channels): deferred, and deferred onto the skip in place
  library fold                             proj 'fold'     (mm; addmm_ on skip blocks; + affine_act_ where not deferred; bmm / baddbmm_ at batch 2;
                                                            with split on: the K = 1920 project of block 22)
  MFMA pointwise project with a gate       proj 'mfma'     (blocks 0 and 1 at >= 8192 pixels)
FusedPointwise.forward: every reducer and the head, 16 x 32 and 6 x 10 (split: gemm_split with the shift; library: conv + affine_act_).
FusedContextHead._forward: 16 x 32 split (gemm_split, gemm_split_conv2x2 with the pool, pooled_shift, gemm_split_up2) and library (addmv);
8 x 12 (ragged, inside WeightMapper.forward's guard); 6 x 10 (the W % 4 fallbacks); 2 x 2 (bottom level 1 x 1: the concatenation route; library
only -- a 4-pixel split GEMM is test_split_gemm's).  Finding: on 6 x 10 and 2 x 2 the down block's 3 x 5 / 1 x 1 map has H W % 4 != 0 and
hs_affine_act_fwd refused it ('unsupported shape') -- WeightMapper.forward never hands the fused head such maps, a direct call raised;
FusedContextHead now runs BN + ReLU of those few pixels with stock ops (_affine_relu), so no affine_act_ is recorded for them.
These two cases exercise code the product cannot reach: WeightMapper.forward's guard (H % 4 == W % 4 == 0, H W % 16 == 0 with two levels)
keeps such maps on the stock route.
The block cases are held in four STAGES that restart the error at what the route itself stored (util_block_ref, 'the restart'): y, the
pooled partial sums, the gate or folded weights a launch returns, and the output at the route's own y and gate.  The end-to-end bound is
far too wide on the late blocks (its median reaches |ref| itself) and is kept only for the stock fp32 block on the CPU.
se_gate + gemm_split has no not-deferred case: test_se_gate_plus_gemm_split_not_deferred_is_unreachable shows why.
'range' parameters are on the fused, raw, split_se, se+split and fold families; the stem forms, the MFMA expand and project, the reducers,
the head and the context head run 'benign' only.
Left out on purpose: the opt-in HS_SE_TAIL route (test_prepared_encoder_with_se_tails_matches_without) and graph replay (the GraphedModel
tests).  Split-GEMM stages are held to util_split_ref.split_bound only; their tier 2 is test_split_gemm.py's.

With HS_PREPARED_F64_REPORT=<file> the GPU run writes one line per case (profiles/prepared_blocks_f64_bound.txt is such a run; nothing
here is tuned to it).  No tolerance in this file is a measured constant."""
import contextlib
import copy
import functools
import inspect
import os

import pytest
import torch

import util_block_ref as B
import util_encoder_ref as R

gpu = pytest.mark.gpu
RECORDED = ('stem_dw', 'stem_conv_bn_swish', 'mbconv_expand_dw', 'depthwise_conv_bn_act', 'pointwise_conv', 'se_gate', 'gemm_split',
            'gemm_split_se', 'affine_act_', 'gemm_split_conv2x2', 'gemm_split_up2', 'pooled_shift')
FLAGS = ('gate', 'residual', 'out', 'shift', 'in_scale', 'w_proj', 'pool_partial')


@functools.lru_cache(maxsize=None)
def _HF():
    from hyperseg_amd import functional
    return functional


class _Seq(list):
    """The recorded sequence; ``calls`` keeps (name, bound arguments, result) of every recorded launch."""

    def __init__(self):
        super().__init__()
        self.calls = []


def own_of(calls):
    """What the route itself stored: y and the pooled partial sums of the depthwise launch, the gate or the gate-folded project weights
    where se_gate returned them (fp32, CPU)."""
    own = {}
    for name, args, res in calls:
        if name in ('stem_dw', 'mbconv_expand_dw', 'depthwise_conv_bn_act') and isinstance(res, tuple):
            own['y'], own['partial'] = res[0], res[1]
        elif name == 'se_gate':
            own['w_scaled' if args.get('w_proj') is not None else 'gate'] = res
    return {k: v.detach().float().cpu().clone() for k, v in own.items()}


@contextlib.contextmanager
def recording():
    """Pass-through recorders around the entries of hyperseg_amd.functional (and torch.addmv, the library form of the pooled shift)."""
    HF = _HF()
    seq, saved = _Seq(), {}

    def wrap(name, fn):
        sig = inspect.signature(fn)

        def rec(*a, **k):
            args = sig.bind(*a, **k).arguments
            flags = [f for f in FLAGS if args.get(f) is not None]
            if args.get('out') is not None and args.get('out') is args.get('residual'):
                flags.append('out_is_residual')
            res = fn(*a, **k)
            seq.append(f"{name}{':none' if res is None else ''}[{','.join(flags)}]")
            seq.calls.append((name, dict(args), res))
            return res
        return rec
    for name in RECORDED:
        saved[name] = getattr(HF, name)
        setattr(HF, name, wrap(name, saved[name]))
    real_addmv = torch.addmv

    def addmv(*a, **k):
        seq.append('addmv[]')
        return real_addmv(*a, **k)
    torch.addmv = addmv
    try:
        yield seq
    finally:
        torch.addmv = real_addmv
        for name, fn in saved.items():
            setattr(HF, name, fn)


def expected_sequence(exp, proj, defer, skip):
    e = {'stem_dw': ['stem_dw[]'], 'stem+dw': ['stem_dw:none[]', 'stem_conv_bn_swish[shift]', 'depthwise_conv_bn_act[shift]'],
         'fused': ['mbconv_expand_dw[]'], 'mfma': ['pointwise_conv[shift]', 'depthwise_conv_bn_act[shift]'],
         'raw_split': ['gemm_split[]', 'depthwise_conv_bn_act[shift,in_scale]'], 'raw_lib': ['depthwise_conv_bn_act[shift,in_scale]'],
         'none': ['depthwise_conv_bn_act[shift]']}[exp]
    res = 'residual,' if skip else ''
    if defer:
        tail = 'residual,out,out_is_residual' if skip else ''
        gated = 'gate,residual,out,out_is_residual' if skip else 'gate'
    else:
        tail, gated = f'{res}shift', f'gate,{res}shift'
    p = {'split_se': [f'gemm_split_se[{tail}]'], 'se+split': ['se_gate[]', f'gemm_split[{gated}]'],
         'fold': ['se_gate[w_proj]'] + ([] if defer else [f'affine_act_[{res}shift]']),
         'mfma': ['se_gate[]', f'pointwise_conv[gate,{res}shift]']}[proj]
    return e + p


# block, input map (the image for block 0), batch, generator, (expand, project) forms with split_gemm on, with split_gemm off
_T = [
    (0, (128, 256), 1, 'benign', ('stem_dw', 'mfma'), ('stem_dw', 'mfma')),
    (0, (64, 128), 1, 'benign', ('stem_dw', 'split_se'), ('stem_dw', 'fold')),
    (0, (60, 136), 1, 'benign', ('stem+dw', 'split_se'), ('stem+dw', 'fold')),
    (1, (64, 128), 1, 'benign', ('none', 'mfma'), ('none', 'mfma')),
    (1, (32, 64), 1, 'benign', ('none', 'split_se'), ('none', 'fold')),
    (1, (32, 64), 1, 'range', ('none', 'split_se'), ('none', 'fold')),
    (1, (6, 10), 1, 'benign', ('none', 'split_se'), ('none', 'fold')),
    (2, (64, 128), 1, 'benign', ('fused', 'split_se'), ('fused', 'fold')),
    (2, (64, 128), 1, 'range', ('fused', 'split_se'), ('fused', 'fold')),
    (2, (60, 136), 1, 'benign', ('raw_split', 'split_se'), ('raw_lib', 'fold')),
    (3, (32, 64), 1, 'benign', ('fused', 'split_se'), ('fused', 'fold')),
    (3, (32, 64), 1, 'range', ('fused', 'split_se'), ('fused', 'fold')),
    (3, (30, 68), 1, 'benign', ('raw_split', 'split_se'), ('raw_lib', 'fold')),
    (4, (32, 64), 1, 'benign', ('fused', 'split_se'), ('fused', 'fold')),
    (5, (64, 128), 1, 'benign', ('fused', 'split_se'), ('fused', 'fold')),
    (6, (32, 64), 1, 'benign', ('fused', 'split_se'), ('fused', 'fold')),
    (6, (32, 64), 2, 'benign', ('fused', 'split_se'), ('fused', 'fold')),
    (6, (30, 68), 1, 'benign', ('raw_split', 'split_se'), ('raw_lib', 'fold')),
    (7, (32, 64), 1, 'benign', ('fused', 'split_se'), ('fused', 'fold')),
    (8, (64, 128), 1, 'benign', ('fused', 'split_se'), ('fused', 'fold')),
    (8, (12, 20), 1, 'benign', ('raw_split', 'split_se'), ('raw_lib', 'fold')),
    (9, (64, 128), 1, 'benign', ('mfma', 'split_se'), ('mfma', 'fold')),
    (9, (60, 136), 1, 'benign', ('raw_split', 'split_se'), ('raw_lib', 'fold')),
    (9, (32, 64), 1, 'range', ('raw_split', 'split_se'), ('raw_lib', 'fold')),
]
for _i in range(9, 16):
    _T += [(_i, (32, 64), 1, 'benign', ('raw_split', 'split_se' if _i < 13 else 'se+split'), ('raw_lib', 'fold')),
           (_i, (6, 10), 1, 'benign', ('raw_split', 'split_se' if _i < 13 else 'se+split'), ('raw_lib', 'fold'))]
_T += [(14, (32, 64), 2, 'benign', ('raw_split', 'se+split'), ('raw_lib', 'fold')),
       (14, (32, 64), 1, 'range', ('raw_split', 'se+split'), ('raw_lib', 'fold')),
       (16, (32, 64), 1, 'benign', ('raw_split', 'se+split'), ('raw_lib', 'fold')),
       (16, (12, 20), 1, 'benign', ('raw_split', 'se+split'), ('raw_lib', 'fold'))]
for _i in range(17, 23):
    _p = 'se+split' if _i < 22 else 'fold'          # block 22: K = 1920 > SPLIT_GEMM_MAX_K, the library fold with split on as well
    _T += [(_i, (16, 32), 1, 'benign', ('raw_split', _p), ('raw_lib', 'fold')), (_i, (6, 10), 1, 'benign', ('raw_split', _p), ('raw_lib', 'fold'))]
_T += [(2, (12, 20), 1, 'quiet', ('raw_split', 'split_se'), ('raw_lib', 'fold')), (3, (6, 10), 1, 'quiet', ('raw_split', 'split_se'), ('raw_lib', 'fold'))]
_T += [(18, (16, 32), 2, 'benign', ('raw_split', 'se+split'), ('raw_lib', 'fold')),
       (22, (16, 32), 1, 'range', ('raw_split', 'fold'), ('raw_lib', 'fold'))]
CASES = {f'b{i} {h}x{w} n{b} {g} {"split" if s else "lib"}': (i, (h, w), b, g, s, (fs if s else fl))
         for (i, (h, w), b, g, fs, fl) in _T for s in (True, False)}
PW_CASES = {f'{key} {h}x{w} {"split" if s else "lib"}': (key, (h, w), s) for key in ('1', '2', '3', '4', 'head') for (h, w) in ((16, 32), (6, 10))
            for s in (True, False)}
CTX_SEQ = {
    ('16x32', True): ['gemm_split[out,shift]', 'gemm_split_conv2x2[shift,pool_partial]', 'pooled_shift[shift,pool_partial]', 'gemm_split_up2[out,shift]'],
    ('16x32', False): ['affine_act_[shift]', 'affine_act_[shift]', 'addmv[]', 'affine_act_[shift]'],
    ('8x12', True): ['gemm_split[out,shift]', 'gemm_split_conv2x2[shift,pool_partial]', 'pooled_shift[shift,pool_partial]', 'gemm_split_up2[out,shift]'],
    ('8x12', False): ['affine_act_[shift]', 'affine_act_[shift]', 'addmv[]', 'affine_act_[shift]'],
    # 6 x 10 and 2 x 2: the 3 x 5 / 1 x 1 maps have H W % 4 != 0, hs_affine_act_fwd refuses them and FusedContextHead takes stock ops there
    ('6x10', True): ['gemm_split[out,shift]', 'addmv[]'],
    ('6x10', False): ['affine_act_[shift]', 'addmv[]'],
    ('2x2', False): ['affine_act_[shift]'],
}
TAPS = {'1': 4, '2': 7, '3': 15, '4': 22, 'head': 22}          # the block whose output (and out_offset) a reducer / the head consumes


# ------------------------------------------------------------------------------------------------------------ models

def _range_edit(model):
    """The 'range' parameters: BN0 pre-activations at util_encoder_ref.PREACTS, a near-zero running variance, a large BN2 shift (the
    deferred offset then dominates the stored values), squeeze-excite gates swept over sigmoid(-30 .. 30)."""
    with torch.no_grad():
        for blk in model.backbone._blocks:
            if blk.expand != 1:
                bn = blk._bn0
                pre = torch.tensor([R.PREACTS[i % len(R.PREACTS)] for i in range(bn.num_features)])
                bn.running_mean.zero_()
                bn.running_var.fill_(1.0)
                bn.weight.copy_(pre.abs() * 0.01)
                bn.bias.copy_(pre)
            blk._bn1.running_var[1] = 1e-6
            blk._bn2.bias.mul_(300.0)
            blk._se_expand.bias.copy_(torch.linspace(-30, 30, blk._se_expand.bias.numel()))
    return model


def _quiet_edit(model):
    """The 'quiet' parameters (util_encoder_ref's 'quiet'): output channel 0 of every block at 1e-4 of its neighbours -- BN2 weight and
    bias scaled -- which is below what a tensor-scale norm resolves."""
    with torch.no_grad():
        for blk in model.backbone._blocks:
            blk._bn2.weight[0] *= 1e-4
            blk._bn2.bias[0] *= 1e-4
    return model


@functools.lru_cache(maxsize=None)
def _models(gen, split):
    """(stock, prepared) HyperSeg-M on the CPU, built once per (generator, split_gemm)."""
    from hyperseg_amd import configs
    from hyperseg_amd.utils.inference import prepare_for_inference
    from hyperseg_amd.utils.synthetic import fill_by_name
    stock = fill_by_name(configs.build('hyperseg-m').eval(), seed=5)
    if gen == 'range':
        _range_edit(stock)
    if gen == 'quiet':
        _quiet_edit(stock)
    fused = copy.deepcopy(stock)
    prepare_for_inference(fused, fold_bn=False, fused_depthwise=True, split_gemm=split)
    return stock, fused


@functools.lru_cache(maxsize=None)
def _on_device(gen, split):
    return copy.deepcopy(_models(gen, split)[1]).to('cuda:0')


def _offsets(fused, idx):
    blocks = fused.backbone._blocks
    prev = blocks[idx - 1]._fused_dw.out_offset if idx > 0 else None
    cpu = lambda t: None if t is None else t.detach().float().cpu()      # noqa: E731
    return cpu(prev), cpu(blocks[idx]._fused_dw.out_offset)


def _cpu_sw(sw):
    if sw is None:
        return None
    return type(sw)(sw.frag.cpu(), sw.inv.cpu(), sw.c_out, sw.c_in, sw.kp)


@functools.lru_cache(maxsize=256)
def _case(name):
    """dict(x32, in_off, out_off, ref (tier 1), ref2 (tier 2), p, defer, skip) of a block case; the reference is computed once."""
    idx, (h, w), b, gen, split, (exp, proj) = CASES[name]
    stock, fused = _models(gen, split)
    blk, f = stock.backbone._blocks[idx], fused.backbone._blocks[idx]._fused_dw
    p = B.block_params(blk)
    in_off, out_off = _offsets(fused, idx)
    g = torch.Generator().manual_seed(1000 + sum(map(ord, name)))
    plan = dict(expand=_cpu_sw(f.expand.split_weights(False, torch.device('cpu'))) if exp == 'raw_split' else None,
                project=_cpu_sw(f.project.split_weights(True, torch.device('cpu'))) if proj in ('split_se', 'se+split') else None)
    d = dict(p=p, in_off=in_off, out_off=out_off, defer=f.defer_shift, skip=f.skip, plan=plan)
    if idx == 0:
        bb = stock.backbone
        d['x32'] = torch.randn(b, 3, h, w, generator=g)
        args = (bb._conv_stem.weight.detach().float(), B.bn_of(bb._bn0), B.conv_pads(bb._conv_stem), p, d['x32'])
        d['ref'] = B.stem_block0_ref('bound', *args)
        d['yref'] = d['yref2'] = B.stem_block0_ref('bound', *args, stop='y')      # every sum in front of y has at most 64 terms
        d['stock'] = lambda x: torch.nn.functional.silu(bb._bn0(bb._conv_stem(x)))      # noqa: E731
        return d
    x = torch.randn(b, blk.in_f, h, w, generator=g)
    d['x32'] = x if in_off is None else (x - in_off.view(1, -1, 1, 1)).float()
    d['ref'] = B.mbconv_block_ref('bound', p, d['x32'], in_off, out_off, plan)          # end to end: the value, and the shape
    d['yref'] = B.mbconv_block_ref('bound', p, d['x32'], in_off, None, plan, stop='y')
    d['yref2'] = B.mbconv_block_ref('bound', p, d['x32'], in_off, None, plan, tier2=True, stop='y') if blk.in_f > B.LONG else d['yref']
    return d


def _compared(got, out_off):
    got = got.detach().double().cpu()
    return got if out_off is None else got + out_off.double().view(1, -1, 1, 1)


_REPORT_STARTED = set()


def _report(name, seq, V, V2, got):
    path = os.environ.get('HS_PREPARED_F64_REPORT')
    if not path:
        return
    _, r1, i1 = B.within(got, V)
    _, r2, _ = B.within(got, V2)
    rel = float(((got - V[0]).abs() / V[0].abs().clamp(min=1e-30)).max())
    mode = 'a' if path in _REPORT_STARTED else 'w'
    _REPORT_STARTED.add(path)
    with open(path, mode) as fh:
        fh.write(f'{name:34s} {" ".join(seq):110s} worst err/bound {r1:.4f} at {i1}  tier-2 err/bound {r2:.4f}  worst err/|ref| {rel:.3e}\n')


def _hold(name, seq, got, d, report=True):
    """A reducer / head / context-head result against its reference, tier 1 then tier 2."""
    ok, r, i = B.within(got, d['ref'])
    assert ok, f'{name}: outside the tier-1 bound, worst err / bound {r:.3g} at flat index {i} ({" ".join(seq)})'
    ok2, r2, i2 = B.within(got, d['ref2'])
    if report:
        _report(name, seq, d['ref'], d['ref2'], got)
    assert ok2, f'{name}: outside the tier-2 bound, worst err / bound {r2:.3g} at flat index {i2} ({" ".join(seq)})'


def staged(d, own, got):
    """The four stages of util_block_ref ('the restart'): [(stage, ok, worst err / bound tier 1, tier 2)], each restarted at what the
    route itself stored (``own``); ``got``: the block's output + out_offset."""
    p, out = d['p'], []
    b, _, ho, wo = own['y'].shape

    def both(stage, value, v1, v2):
        (ok1, r1, _), (ok2, r2, _) = B.within(value, v1), B.within(value, v2)
        out.append((stage, ok1 and ok2, r1, r2))
    both('y', own['y'], d['yref'], d['yref2'])
    both('pool', own['partial'].double().sum(1), B.pool_own_ref(own['y'], own['partial']), B.pool_own_ref(own['y'], own['partial'], tier2=True))
    for key in ('gate', 'w_scaled'):
        if own.get(key) is not None:
            fold = key == 'w_scaled'
            g1, g2 = (B.gate_own_ref(p, own['partial'], b, ho * wo, t2, fold)[key] for t2 in (False, True))
            both(key, own[key].flatten(2) if fold else own[key], g1, g2)
    args = (p, own, d['x32'], d['in_off'], d['out_off'], d['plan'])
    both('out', got, B.tail_own_ref(*args), B.tail_own_ref(*args, tier2=True))
    return out


def _hold_staged(name, seq, got, d, own, report=True):
    res = staged(d, own, got)
    path = os.environ.get('HS_PREPARED_F64_REPORT')
    if report and path:
        mode = 'a' if path in _REPORT_STARTED else 'w'
        _REPORT_STARTED.add(path)
        rel = float(((got - d['ref'][0]).abs() / d['ref'][0].abs().clamp(min=1e-30)).max())
        with open(path, mode) as fh:
            stages = '  '.join(f'{st} {r1:.4f}/{r2:.4f}' for st, _, r1, r2 in res)
            fh.write(f'{name:34s} {" ".join(seq):110s} worst err/bound per stage, tier 1/tier 2: {stages}  end-to-end worst err/|ref| {rel:.3e}\n')
    bad = [r for r in res if not r[1]]
    assert not bad, f'{name}: stages outside their bound (stage, ok, err/bound tier 1, tier 2): {bad} ({" ".join(seq)})'


# ------------------------------------------------------------------------------------------------------------ CPU tests

SMALL = [n for n, c in CASES.items() if c[1][0] * c[1][1] * c[2] <= 4096]


@pytest.mark.parametrize('name', [n for n in CASES if n.endswith('lib')])
def test_stock_fp32_block_within_bound(name):
    """The stock block in fp32 on the CPU lies inside the bound of its float64 statement (offsets: none -- the stock block receives x itself)."""
    idx, (h, w), b, gen, split, _ = CASES[name]
    stock, _ = _models(gen, False)
    blk = stock.backbone._blocks[idx]
    p = B.block_params(blk)
    g = torch.Generator().manual_seed(7 + idx)
    with torch.no_grad():
        if idx == 0:
            bb = stock.backbone
            x = torch.randn(b, 3, h, w, generator=g)
            got = blk(torch.nn.functional.silu(bb._bn0(bb._conv_stem(x))))
            ref = B.stem_block0_ref('bound', bb._conv_stem.weight.detach().float(), B.bn_of(bb._bn0), B.conv_pads(bb._conv_stem), p, x)
        else:
            x = torch.randn(b, blk.in_f, h, w, generator=g)
            got, ref = blk(x), B.mbconv_block_ref('bound', p, x)
            ok2, r2, i2 = B.within(got, B.mbconv_block_ref('bound', p, x, tier2=True))
            assert ok2, f'{name}: the stock fp32 block leaves its tier-2 bound: {r2:.3g} at {i2}'
    ok, r, i = B.within(got, ref)
    assert ok, f'{name}: the stock fp32 block leaves its own bound: {r:.3g} at {i}'


WIDE = ('b18 6x10 n1 benign lib', 'b14 6x10 n1 benign split')          # more than 512 mid channels (1152, 672)


def _defect_cases():
    return ['b3 32x64 n1 benign split', 'b3 32x64 n1 range split', 'b1 6x10 n1 benign lib', 'b9 6x10 n1 benign split', 'b2 12x20 n1 quiet lib'] + list(WIDE)


def _restated(d, defect):
    own = {}
    y, off = B.prepared_block_f32(d['p'], d['x32'], d['in_off'], d['defer'], defect, own=own)
    got = _compared(y, off)
    return got, staged(d, own, got)


def test_restatement_within_bound_and_defects_rejected():
    """The right prepared algebra (fp32, CPU) passes every stage on the defect cases; every defect is rejected on at least one case, and
    every block defect on EACH of the wide blocks (more than 512 mid channels), where the end-to-end bound would hold nothing."""
    rejected = {k: [] for k in B.DEFECTS}
    for name in _defect_cases():
        d = _case(name)
        for defect in (None,) + B.BLOCK_DEFECTS:
            res = _restated(d, defect)[1]
            ok = all(r[1] for r in res)
            if defect is None:
                assert ok, f'{name}: the right restatement leaves the bound: {res}'
            elif not ok:
                rejected[defect].append(name)
    for defect in B.BLOCK_DEFECTS:
        assert set(WIDE) <= set(rejected[defect]), f'{defect} passes on a wide block: rejected only on {rejected[defect]}'
    stock, _ = _models('benign', False)
    wp = B.wm_params(stock.weight_mapper)
    x = torch.randn(1, 1280, 16, 32, generator=torch.Generator().manual_seed(3)).abs()
    ref = B.weight_mapper_ref('bound', wp, x, tier2=True)
    assert B.within(B.context_head_f32(wp, x), ref)[0]
    for defect in B.CTX_DEFECTS:
        if not B.within(B.context_head_f32(wp, x, defect), ref)[0]:
            rejected[defect].append('ctx 16x32')
    assert all(rejected.values()), f'defects no case rejects: {[k for k, v in rejected.items() if not v]}'


def test_a_scaled_output_is_rejected_on_the_wide_blocks():
    """Every stored output multiplied by 1.01 -- what the end-to-end bound let through on the late blocks -- fails the output stage."""
    for name in WIDE:
        d = _case(name)
        own = {}
        y, off = B.prepared_block_f32(d['p'], d['x32'], d['in_off'], d['defer'], None, own=own)
        res = staged(d, own, _compared(y * 1.01, off))
        assert [r[0] for r in res if not r[1]] == ['out'], (name, res)


def test_a_defect_passes_the_old_tensor_norm():
    """'bn_eps_dropped' (BN1 of ONE mid channel folded without eps, a 5e-4 change of its scale) passes rel_err < 5e-5 -- the limit of
    test_prepared_encoder_matches_stock, max |err| / max |ref| over the tensor -- on the output of a wide and of a narrow block, and is
    rejected per element at the y stage.  So do 'deferred_adds_shift' and 'carried_without_in_offset', confined to output channel 0, on
    the 'quiet' cases (channel 0 at 1e-4 of its neighbours), at the output stage."""
    from conftest import rel_err
    for name, defect, stage in (('b18 6x10 n1 benign lib', 'bn_eps_dropped', 'y'), ('b9 6x10 n1 benign split', 'bn_eps_dropped', 'y'),
                                ('b2 12x20 n1 quiet lib', 'deferred_adds_shift', 'out'), ('b3 6x10 n1 quiet split', 'carried_without_in_offset', 'out')):
        d = _case(name)
        got, res = _restated(d, defect)
        assert rel_err(got.float(), d['ref'][0].float()) < 5e-5, (name, defect)
        assert stage in [r[0] for r in res if not r[1]], (name, defect, res)


def test_range_inputs_reach_their_regimes():
    stock, fused = _models('range', True)
    d = _case('b3 32x64 n1 range split')
    blk = stock.backbone._blocks[3]
    with torch.no_grad():
        x = d['x32'] + d['in_off'].view(1, -1, 1, 1)
        pre = blk._bn0(blk._expand_conv(x))
        for c, want in enumerate(R.PREACTS):
            if abs(want) >= 20:
                assert float((pre[:, c] / want - 1).abs().max()) < 0.5, (c, want)
        y = torch.nn.functional.silu(blk._bn1(blk._depthwise_conv(torch.nn.functional.silu(pre))))
        gate = torch.sigmoid(blk._se_expand(torch.nn.functional.silu(blk._se_reduce(y.mean((2, 3), keepdim=True)))))
    assert float(gate.min()) < 1e-6 and float(gate.max()) > 1 - 1e-6
    assert float(blk._bn1.running_var.min()) < 1e-5
    # the deferred offset dominates the stored values: x32 = x - in_offset with x ~ N(0, 1), so |x32| is mostly offset
    assert float(d['x32'].abs().median()) > 4 * float((d['x32'] + d['in_off'].view(1, -1, 1, 1)).abs().median())


def test_table_covers_every_branch_and_block():
    _, fused = _models('benign', True)
    n = len(fused.backbone._blocks)
    assert {c[0] for c in CASES.values()} == set(range(n))
    forms = {(s, e, p, fused.backbone._blocks[i]._fused_dw.defer_shift, fused.backbone._blocks[i]._fused_dw.skip, b > 1)
             for (i, _, b, _, s, (e, p)) in CASES.values()}
    has = lambda **kw: any(all(dict(split=f[0], exp=f[1], proj=f[2], defer=f[3], skip=f[4], batched=f[5])[k] == v for k, v in kw.items()) for f in forms)      # noqa: E731
    for exp in ('stem_dw', 'stem+dw', 'fused', 'mfma', 'raw_split', 'raw_lib', 'none'):
        assert has(exp=exp), exp
    for proj in ('split_se', 'se+split', 'fold'):
        assert has(proj=proj, defer=True, skip=False) and has(proj=proj, defer=True, skip=True), proj
    assert has(proj='split_se', defer=False, skip=True) and has(proj='fold', defer=False, skip=True) and has(proj='fold', defer=False, skip=False)
    assert has(proj='mfma', skip=True) and has(proj='mfma', skip=False)
    assert has(proj='fold', split=True, defer=True)                     # K = 1920 with split on
    assert has(batched=True, proj='split_se') and has(batched=True, proj='se+split') and has(batched=True, proj='fold', split=False)
    ks = {(fused.backbone._blocks[c[0]]._fused_dw.k, fused.backbone._blocks[c[0]]._fused_dw.stride, c[4]) for c in CASES.values()}
    assert {(5, 1, True), (5, 2, True), (3, 2, True), (5, 2, False), (3, 2, False)} <= ks
    # what the table says about thresholds agrees with the product's own predicates on the host
    HF = _HF()
    for name, (i, (h, w), b, _, s, (exp, proj)) in CASES.items():
        f = fused.backbone._blocks[i]._fused_dw
        if i == 0:
            route = HF.stem_dw_route((h, w), 32, 0, 0, ((h + 1) // 2, (w + 1) // 2))
            assert (route is not None) == (exp == 'stem_dw'), name
            continue
        ho, wo = B.out_size(B.block_params(_models('benign', s)[0].backbone._blocks[i]), h, w)
        cin = _models('benign', s)[0].backbone._blocks[i].in_f
        if f.expand is not None:
            fuses = cin <= 40 and ho * wo >= 2048
            assert (exp == 'fused') == fuses and (exp == 'mfma') == (not fuses and cin <= 96 and h * w >= 8192), name


def test_se_gate_plus_gemm_split_not_deferred_is_unreachable():
    """The issue names a third form of se_gate + gemm_split: not deferred, with shift + residual.  Only blocks 0 and 1 are not deferred
    (16 / 32 mid channels, far below GEMM_SE_MAX_CIN), so the form needs a map at which gemm_split_se_route refuses them.  It refuses at
    none: every admissible map (H W % 4 == 0, below the 8192 pixels from which the MFMA project takes over) is asked here, with the
    pooling blocks of the depthwise launch and of the stem + depthwise tiles.  The table therefore has no such case."""
    HF = _HF()
    asked = 0
    for c, csq, cout in ((16, 4, 16), (32, 8, 16)):
        for h in range(2, 130, 2):
            for w in range(2, 260, 2):
                if (h * w) % 4 or h * w >= 8192:
                    continue
                for nblk in {R.dw_threads(h, w)[1], int(HF._hip.lib.hs_mbconv_tiles(3, 1, h, w))}:
                    asked += 1
                    assert HF.gemm_split_se_route(c, nblk, csq, cout, h * w) is not None, (c, h, w, nblk)
    assert asked > 5000


def test_no_in_place_block_receives_a_tapped_feature():
    for gen, split in (('benign', True), ('benign', False), ('range', True), ('range', False)):
        bb = _models(gen, split)[1].backbone
        for idx, blk in enumerate(bb._blocks):
            f = blk._fused_dw
            if f.skip and f.defer_shift:              # accumulates onto its input in place
                assert idx > 0 and not bb._res_feat_mask[idx - 1], idx


@pytest.mark.parametrize('split', [True, False])
def test_prepared_route_through_the_standins_within_bound(monkeypatch, split):
    """The prepared route on CPU tensors (stand-ins of test_deferred_bn_shift_algebra_cpu) per element, on the 1 x 64 x 128 case."""
    import util_prepared_standins
    name = f'b2 64x128 n1 benign {"split" if split else "lib"}'
    d = _case(name)
    util_prepared_standins.install(monkeypatch)
    _, fused = _models('benign', split)
    blk = fused.backbone._blocks[2]
    with torch.no_grad(), recording() as seq:
        got = blk._fused_dw(d['x32'].clone(), blk)
    _hold_staged(name, ['stand-ins'], _compared(got, d['out_off']), d, own_of(seq.calls), report=False)


# ------------------------------------------------------------------------------------------------------------ GPU tests

@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.fail('these tests need the MI355X (torch.cuda.is_available() is False)')
    yield torch.device('cuda:0')
    torch.cuda.synchronize()
    _on_device.cache_clear()
    torch.cuda.empty_cache()


GUARD = 64


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


def _run_guarded(dev, fn, shape, must_return=True, expect_taken=True):
    """As test_hip_decoder_f64._run_guarded: the first torch.empty of the output's shape is pointed at a view between NaN-pattern guard
    words.  ``must_return``: the guarded allocation is the block's result.  False where the depthwise output has the block's output
    shape: the guarded tensor is then that intermediate, and the block's own output is NOT guarded.  ``expect_taken`` False: the
    library-fold routes, whose result torch.mm / bmm allocate themselves -- those outputs are unguarded too."""
    buf, view = _guarded(dev, shape)
    real_empty, taken = torch.empty, []

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
    assert taken or not expect_taken, 'no allocation of the guarded shape was made'
    if must_return:
        assert taken and y.data_ptr() == view.data_ptr(), 'the output was not allocated inside the guards'
    assert _guards_intact(buf), 'guard words around the output were overwritten'
    return y


@gpu
@pytest.mark.parametrize('name', list(CASES))
def test_prepared_block(dev, name):
    idx, (h, w), b, gen, split, (exp, proj) = CASES[name]
    d = _case(name)
    fused = _on_device(gen, split)
    blk = fused.backbone._blocks[idx]
    f = blk._fused_dw
    want = expected_sequence(exp, proj, f.defer_shift, f.skip)
    shape = tuple(d['ref'][0].shape)
    in_place = f.skip and f.defer_shift
    if in_place:
        buf, x = _guarded(dev, tuple(d['x32'].shape))
        x.copy_(d['x32'])
    else:
        x = d['x32'].to(dev)
    with torch.no_grad(), recording() as seq:
        if in_place:
            got = f(x, blk)
            torch.cuda.synchronize()
            assert got.data_ptr() == x.data_ptr(), 'the skip block did not accumulate in place'
            assert _guards_intact(buf), 'guard words around the skip buffer were overwritten'
        elif proj == 'fold' and f.defer_shift:          # torch.mm / bmm allocate the result themselves
            got = f(x, blk)
        else:
            same = blk._depthwise_conv.weight.shape[0] == shape[1] and d['x32'].shape[2:] == shape[2:] or proj == 'fold'
            got = _run_guarded(dev, lambda: f(x, blk), shape, must_return=not same, expect_taken=proj != 'fold')
    assert seq == want, f'{name}: launched {seq}, the case was written for {want}'
    _hold_staged(name, seq, _compared(got, d['out_off']), d, own_of(seq.calls))


@functools.lru_cache(maxsize=None)
def _pw_case(name):
    key, (h, w), split = PW_CASES[name]
    stock, fused = _models('benign', split)
    bb, fb = stock.backbone, fused.backbone
    conv, bn = (bb._conv_head, bb._bn1) if key == 'head' else tuple(getattr(bb, f'_feat_fc_{key}'))
    mod = fb._fused_head if key == 'head' else fb._fused_fc[key]
    off = _offsets(fused, TAPS[key])[1]
    x = torch.randn(1, conv.in_channels, h, w, generator=torch.Generator().manual_seed(31 + sum(map(ord, name))))
    x32 = (x - off.view(1, -1, 1, 1)).float()
    sw = _cpu_sw(mod.split_weights(True, torch.device('cpu'))) if split else None
    args = (conv.weight.detach().float().flatten(1), B.bn_of(bn), R.ACT_SWISH if key == 'head' else R.ACT_NONE, x32, off)
    return dict(x32=x32, ref=B.pointwise_bn_ref('bound', *args, split=sw), ref2=B.pointwise_bn_ref('bound', *args, split=sw, tier2=True), out_off=None)


@pytest.mark.parametrize('name', [n for n in PW_CASES if n.endswith('lib')])
def test_stock_fp32_reducer_within_bound(name):
    key, (h, w), _ = PW_CASES[name]
    bb = _models('benign', False)[0].backbone
    conv, bn = (bb._conv_head, bb._bn1) if key == 'head' else tuple(getattr(bb, f'_feat_fc_{key}'))
    x = torch.randn(1, conv.in_channels, h, w, generator=torch.Generator().manual_seed(5))
    with torch.no_grad():
        got = bn(conv(x))
        got = torch.nn.functional.silu(got) if key == 'head' else got
    ref = B.pointwise_bn_ref('bound', conv.weight.detach().float().flatten(1), B.bn_of(bn), R.ACT_SWISH if key == 'head' else R.ACT_NONE, x)
    assert B.within(got, ref)[0], name


@gpu
@pytest.mark.parametrize('name', list(PW_CASES))
def test_prepared_reducer_and_head(dev, name):
    key, (h, w), split = PW_CASES[name]
    d = _pw_case(name)
    fb = _on_device('benign', split).backbone
    mod = fb._fused_head if key == 'head' else fb._fused_fc[key]
    x = d['x32'].to(dev)
    with torch.no_grad(), recording() as seq:
        got = _run_guarded(dev, lambda: mod(x), tuple(d['ref'][0].shape)) if split else mod(x)
    assert seq == (['gemm_split[shift]'] if split else ['affine_act_[shift]']), f'{name}: launched {seq}'
    _hold(name, seq, _compared(got, None), d)


@functools.lru_cache(maxsize=None)
def _ctx_case(size, split):
    h, w = (int(s) for s in size.split('x'))
    stock, fused = _models('benign', split)
    wp = B.wm_params(stock.weight_mapper)
    x = torch.randn(1, stock.weight_mapper.in_channels, h, w, generator=torch.Generator().manual_seed(h * 100 + w))
    x = torch.nn.functional.silu(x)                  # what the head conv hands over: a swish output
    plan = {}
    if split:
        f = fused.weight_mapper._fused
        wm = fused.weight_mapper
        half = wm.in_channels // 2
        plan['in'] = _cpu_sw(f._split_weights('in', wm.in_conv[0].weight.view(half, -1), f.scale0))
        if size in ('16x32', '8x12'):
            plan['down0'] = _cpu_sw(f._split_weights('down0', wm.down_blocks[0][0].weight, f.scale1, max_k=2560))
            plan['up0'] = _cpu_sw(f._split_weights('up0', wm.up_blocks[0][0].weight.view(half, -1)[:, :half], f.scale2))
    return dict(x32=x, ref=B.weight_mapper_ref('bound', wp, x, plan), ref2=B.weight_mapper_ref('bound', wp, x, plan, tier2=True), out_off=None)


@pytest.mark.parametrize('size', ['16x32', '8x12', '6x10', '2x2'])
def test_stock_fp32_context_head_within_bound(size):
    d = _ctx_case(size, False)
    with torch.no_grad():
        got = _models('benign', False)[0].weight_mapper(d['x32'])
    assert B.within(got, d['ref'])[0], size


@gpu
@pytest.mark.parametrize('size,split', list(CTX_SEQ))
def test_prepared_context_head(dev, size, split):
    d = _ctx_case(size, split)
    head = _on_device('benign', split).weight_mapper._fused
    x = d['x32'].to(dev)
    with torch.no_grad(), recording() as seq:
        got = _run_guarded(dev, lambda: head(x), tuple(d['x32'].shape))
    assert seq == CTX_SEQ[(size, split)], f'ctx {size} split={split}: launched {seq}'
    _hold(f'ctx {size} {"split" if split else "lib"}', seq, _compared(got, None), d)
