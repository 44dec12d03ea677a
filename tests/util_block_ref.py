"""Host-only float64 statements of the STOCK encoder modules that utils/inference.py replaces (MBConvBlock, the stem, the head conv, a
feature reducer, the v1_0 WeightMapper), the per-element bound a prepared route is held to, and fp32 restatements of the prepared
algebra with one mistake each (``DEFECTS``).  Stock torch on the CPU, built on util_encoder_ref.Chain; the project is not imported (a
split-GEMM stage is handed its ``SplitWeights`` by the caller, as in util_split_ref).

THE REFERENCE is the stock module's own statement, from its parameters and buffers, independent of ``_bn_affine`` and of any folding:
expand 1x1 -> BN as (x - mean) / sqrt(var + eps) * w + b -> swish -> the TF-"SAME" zero padding -> depthwise -> BN -> swish -> global
mean -> reduce, swish, expand, sigmoid -> gate * x -> project 1x1 -> BN -> + inputs on skip blocks; all in float64.

THE RELATION TESTED -- the whole contract of the deferred-shift chain.  A prepared block receives ``x32`` that STANDS FOR
``x32 + in_offset`` and returns ``y`` that STANDS FOR ``y + out_offset``; both offsets are the fp32 buffers the prepared model holds,
taken as exact float64 values.  So the reference input is ``x32.double() + in_offset.double()`` and the value compared is
``got.double() + out_offset.double()``.  A reducer or the head with an absorbed offset is tested the same way (``out_offset`` = 0).

THE BOUND composes the steps of util_encoder_ref (u = 2^-23, SUB, the activation rule) with the operands' error carried; nothing new is
measured.  What is added here, each derived:

 bn      the stock statement against an fp32 route, folded or not.  The folded scale s32 = w / sqrt(var + eps) carries 3 roundings (add,
         sqrt, divide), the shift b - mean s32 two more on |mean s| and one on b, the kernel's fused multiply-add one on everything;
         the stock fp32 form (x - mean) * invstd * w + b has at most 7 on s (x - mean) and one on b.  With the convention of
         util_f16_ref.sum_bound (n roundings -> n u, covering order and higher orders):
             e_z = |s| e + 8 u |s| (|v| + e + |mean|) + 2 u |b| + u |z| + SUB.
 absorb  a consumer of a deferred tensor folded scale * (W @ in_offset) into its shift on the host (``absorb_input_offset``): an fp32
         mat-vec of K terms, the product with the scale and the addition to the shift: (K + 4) u |s| (|W| @ |in_offset|).  The sum
         itself is bounded at the operands the route really multiplies, |x32|, not |x32 + in_offset|.
 fold    the BN scale or the gate folded into the weights before a GEMM is one more product rounding per term: terms + 1 each.
 library torch.mm / addmm_ / bmm / baddbmm_ / F.conv2d are fp32 sums in an unknown order: the plain sum rule; beta = 1 accumulation
         onto the skip is the residual's one rounding.
 split   a stage on hs_gemm_split_fwd takes util_split_ref.split_bound.  Its operand is perturbed (|gate y| is known to e only), and
         the slice maxima that set the floor term move with it, so the bound is evaluated at the INFLATED operand |gate y| + e, where
         mag, floor and underflow are all at least the kernel's own, plus sum |w| e_k for the perturbation itself.
 skip    out = z + x32 is one rounding; a deferred skip block's out_offset = fl(shift + in_offset) is one more, u |out_offset|.
 pool    the mean over H W pixels: the sum rule with H W + 1 terms (any blocking); the squeeze then sums C * nblk + 1 terms with nblk
         at most the quad-padded pixel count / 128 (the smallest pooling block of any launch, util_encoder_ref's 'pool' list).

TIER 2 as util_encoder_ref: every sum longer than 64 terms that is NOT on the split GEMM is also held to MARGIN * q_cpu of that sum on
those inputs (``level``: util_encoder_ref.sum_level on a sample of (row, pixel) pairs of the reference operands), in place of its
(K + 2) u; the tier-1 result is kept alongside.  The split stages keep their own bound; their tier 2 lives in test_split_gemm.py.

DEFECTS: fp32 restatements of the prepared algebra (``prepared_block_f32``, ``context_head_f32``) with one mistake.  Confined to one
channel (as util_training_ref does with dw_tile_last_row_dropped): carried_without_in_offset and deferred_adds_shift to output channel 0,
bn_eps_dropped to BN1's channel 0, ctx_wb_left_half to one output row; absorb_without_scale is applied to every expand channel --
confined to one it stays under the bound's squeeze-excite terms.

HOW WIDE THE COMPOSED BOUND IS, AND THE RESTART.  Carried end to end (``mbconv_block_ref``), the worst case goes through three long
contractions in a row -- the pool, the squeeze over C * nblk, the project over up to 1920 channels, each summing the carried errors in
absolute value: the bound's median is 1e-2 .. 1 of |ref| on the blocks with more than 512 mid channels, where it holds nothing.  So
the tests hold a block in STAGES that restart the error at what the route itself stored (as util_encoder_ref.pool_own and
se_excite_ref do per kernel): (1) y, the depthwise launch's output, against the carried front (expand, BN0, swish, depthwise, BN1,
swish: K <= 320 and k*k terms); (2) the pooled partial sums, totalled, against the float64 sum of the route's own y
(``pool_own_ref``); (3) the gate, or the gate-folded project weights, that a launch returns against ``gate_own_ref`` of the route's own
partial sums; (4) the block output against ``tail_own_ref``: the project at the route's own y (error 0) and its own gate (error 0) or,
where gemm_split_se derives the gate inside its launch, ``gate_own_ref``'s value with that short chain's error.  Each stage carries
only its own terms; together they tie the output to the stock statement.  The end-to-end bound is kept for the CPU check of the stock
fp32 block.
"""
import torch
import torch.nn.functional as F

import util_encoder_ref as R
from util_encoder_ref import ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_SWISH, SUB, Chain
from util_f16_ref import U32, sum_bound
from util_split_ref import split_bound

DEFECTS = ('carried_without_in_offset', 'absorb_without_scale', 'deferred_adds_shift', 'bn_eps_dropped', 'mean_padded_count',
           'ctx_wb_left_half', 'ctx_up2_transposed')
BLOCK_DEFECTS, CTX_DEFECTS = DEFECTS[:5], DEFECTS[5:]
LONG = 64


# ------------------------------------------------------------------------------------------------------------ parameters

def bn_of(bn):
    return dict(w=bn.weight.detach().float().cpu(), b=bn.bias.detach().float().cpu(), mean=bn.running_mean.detach().float().cpu(),
                var=bn.running_var.detach().float().cpu(), eps=float(bn.eps))


def conv_pads(conv):
    """(pad_t, pad_l, pad_h, pad_w) of a SamePadConv2d: the module's own statement of its zero padding."""
    if conv._pad is not None:
        return conv._pad[2], conv._pad[0], conv._pad[2] + conv._pad[3], conv._pad[0] + conv._pad[1]
    return conv.padding[0], conv.padding[1], 2 * conv.padding[0], 2 * conv.padding[1]


def block_params(blk):
    """The stock MBConvBlock's parameters and buffers as fp32 CPU tensors."""
    t = lambda p: p.detach().float().cpu().clone()      # noqa: E731
    dwc = blk._depthwise_conv
    return dict(we=t(blk._expand_conv.weight).flatten(1) if blk.expand != 1 else None, bn0=bn_of(blk._bn0) if blk.expand != 1 else None,
                wd=t(dwc.weight), bn1=bn_of(blk._bn1), k=dwc.kernel_size[0], stride=dwc.stride[0], pads=conv_pads(dwc),
                w1=t(blk._se_reduce.weight).flatten(1), b1=t(blk._se_reduce.bias), w2=t(blk._se_expand.weight).flatten(1), b2=t(blk._se_expand.bias),
                wp=t(blk._project_conv.weight).flatten(1), bn2=bn_of(blk._bn2), skip=blk.stride == 1 and blk.in_f == blk.out_f)


def out_size(p, h, w):
    pt, pl, ph, pw = p['pads']
    return (h + ph - p['k']) // p['stride'] + 1, (w + pw - p['k']) // p['stride'] + 1


# ------------------------------------------------------------------------------------------------------------ steps

def bn_scale_shift(bn):
    """float64 (s, shift) of the stock statement (x - mean) / sqrt(var + eps) * w + b = s x + (b - mean s)."""
    s = bn['w'].double() / torch.sqrt(bn['var'].double() + bn['eps'])
    return s, bn['b'].double() - bn['mean'].double() * s


def bn_stage(V, bn, shape, absorbed=None):
    """The ``bn`` rule of the module docstring.  ``absorbed``: (value, error) of a per-channel constant added to the shift (``absorb``)."""
    v, e = V
    s, sh = bn_scale_shift(bn)
    z = (v - bn['mean'].double().view(shape)) / torch.sqrt(bn['var'].double() + bn['eps']).view(shape) * bn['w'].double().view(shape) + bn['b'].double().view(shape)
    if absorbed is not None:
        z = z + absorbed[0].view(shape)
    if e is None:
        return z, None
    sa = s.abs().view(shape)
    ez = sa * e + 8 * U32 * sa * (v.abs() + e + bn['mean'].double().abs().view(shape)) + 2 * U32 * bn['b'].double().abs().view(shape) + U32 * z.abs() + SUB
    if absorbed is not None:
        ez = ez + absorbed[1].view(shape) + U32 * absorbed[0].abs().view(shape)
    return z, ez


def level(w, x, lanes=(4, 16, 1), rows=64, cols=64, seed=0):
    """Tier 2: sum_level of sum_k w[o, k] x[n, k] over a sample of (o, n) pairs; w (O, K), x (N, K), values as fp32."""
    g = torch.Generator().manual_seed(77 + seed)
    k = w.shape[1]
    cap = max(8, int(((1 << 18) // k) ** 0.5))
    oi = torch.randperm(w.shape[0], generator=g)[:min(rows, cap)]
    ni = torch.randperm(x.shape[0], generator=g)[:min(cols, cap)]
    return R.sum_level((w.float()[oi][:, None, :] * x.float()[ni][None, :, :]).reshape(-1, k).contiguous(), lanes)


def conv1x1(ch, X, w, name, tier2, split=None, extra_terms=0):
    """S = W @ x per pixel of a travelling (B, K, H, W): the sum rule (tier 1), MARGIN * q_cpu for K > 64 (``tier2``), or -- ``split``: a
    SplitWeights whose rows carry ``split_rows`` (a float64 (O,) factor already folded into them, else None) -- the ``split`` rule; the
    value is then returned in the rows' units as well.  ``extra_terms``: product roundings per term in front of the sum (``fold``)."""
    v, e = X
    w_ = w.double()
    k = w_.shape[1]
    s = torch.einsum('ok,bkhw->bohw', w_, v)
    if e is None:
        return s, None
    mag = torch.einsum('ok,bkhw->bohw', w_.abs(), v.abs() + e)
    carry = torch.einsum('ok,bkhw->bohw', w_.abs(), e)
    if split is not None:
        b, _, h, wd = v.shape
        infl = ((v.abs() + e) * (1 + U32)).float().reshape(b, k, h * wd)
        es = torch.stack([split_bound(split, infl[i].contiguous(), torch.ones(k)) for i in range(b)]).view(b, -1, h, wd)
        return s, carry + es + SUB
    if tier2 and k > LONG:
        q = level(w, v.permute(0, 2, 3, 1).reshape(-1, k))
        return s, carry + (q + extra_terms * U32) * mag + SUB
    return s, carry + sum_bound(k + extra_terms, mag) + SUB


def absorbed_of(w, bn, off):
    """(value, error) of scale * (W @ in_offset), the constant ``absorb_input_offset`` adds to a consumer's BN shift; (0, 0) without."""
    if off is None:
        return None
    s, _ = bn_scale_shift(bn)
    val = s * (w.double() @ off.double())
    return val, (w.shape[1] + 4) * U32 * s.abs() * (w.double().abs() @ off.double().abs())


# ------------------------------------------------------------------------------------------------------------ the stock block

def mbconv_block_ref(mode, p, x32, in_offset=None, out_offset=None, plan=None, tier2=False, H=None, stop=None):
    """The stock MBConvBlock at ``x32 + in_offset``: (value, error | None), to be compared with ``got + out_offset``.
    ``plan``: dict(expand=SplitWeights | None, project=SplitWeights | None) -- the stages that run on the split GEMM (the project's
    SplitWeights carry the BN2 scale in their rows).  ``H``: a travelling (value, error) that replaces the block input for expand-free
    blocks (block 0 behind the stem).  ``mode``: 'f64' | 'bound'."""
    ch = Chain(mode)
    plan = plan or {}
    pt, pl = p['pads'][:2]
    x = x32.double()
    X = H if H is not None else ch.inp(x32)
    b, _, h, w = X[0].shape
    ho, wo = out_size(p, h, w)
    if p['we'] is not None:
        S = conv1x1(ch, X, p['we'], 'expand', tier2, split=plan.get('expand'))
        if in_offset is not None:                   # the value at x32 + in_offset; the sum's error at the operand the route multiplies
            S = (S[0] + (p['we'].double() @ in_offset.double()).view(1, -1, 1, 1), S[1])
        Hm = ch.act(_bn_absorbing(S, p['bn0'], p['we'], in_offset), ACT_SWISH)
    else:
        Hm = X
    wd, wa = p['wd'].double(), p['wd'].double().abs()
    k, st = p['k'], p['stride']
    D = ch.summed(Hm, lambda t: R._dw_taps(t, wd, k, st, pt, pl, ho, wo), lambda t: R._dw_taps(t, wa, k, st, pt, pl, ho, wo), k * k)
    Y = ch.act(bn_stage(D, p['bn1'], (1, -1, 1, 1)), ACT_SWISH)
    if stop == 'y':
        return Y
    hw = ho * wo
    c = Y[0].shape[1]
    if tier2 and mode == 'bound':
        rows = Y[0].flatten(2).flatten(0, 1)
        ch.q['pool'] = R.sum_level(rows[::max(1, rows.shape[0] // 64)][:64].float().contiguous(), (256, 16, 1))
    M = ch.summed(Y, lambda t: t.sum((2, 3)) / hw, lambda t: t.sum((2, 3)) / hw, hw + 1, 'pool')
    nblk = -(-ho * 4 * ((wo + 3) // 4) // 128)
    w1, w2 = p['w1'].double(), p['w2'].double()
    if tier2 and mode == 'bound':
        if c > LONG:
            ch.q['squeeze'] = level(p['w1'], M[0], (256, 4, 1))
    T = ch.summed(M, lambda t: t @ w1.t(), lambda t: t @ w1.abs().t(), c * nblk + 1, 'squeeze')
    Z = ch.act(ch.affine(T, None, p['b1'], (1, -1)), ACT_SWISH)
    if tier2 and mode == 'bound' and w2.shape[1] > LONG:
        ch.q['excite'] = level(p['w2'], Z[0])
    G = R.se_excite_ref(ch, Z, p['w2'], p['b2'])
    return _tail(ch, p, Y, G, x, in_offset, out_offset, plan, tier2)


def _tail(ch, p, Y, G, x, in_offset, out_offset, plan, tier2, w_scaled=None):
    """gate * y -> project -> BN2 -> + inputs, from travelling Y and G; ``w_scaled`` (B, Cout, C) float64: the route's OWN folded weights
    (gate and BN2 scale inside, error 0) in place of G -- the library fold, whose sum is then the plain rule on those weights."""
    mode = ch.mode
    s2, sh2 = bn_scale_shift(p['bn2'])
    if w_scaled is not None:
        v, e = Y
        S = torch.einsum('bok,bkhw->bohw', w_scaled, v)
        O = (S + sh2.view(1, -1, 1, 1), None)
        if e is not None:
            mag = torch.einsum('bok,bkhw->bohw', w_scaled.abs(), v.abs() + e)
            k = w_scaled.shape[2]
            if tier2 and k > LONG:
                es = level(w_scaled[0], v.permute(0, 2, 3, 1).reshape(-1, k)) * mag
            else:
                es = sum_bound(k, mag)
            bn = p['bn2']
            O = (O[0], es + torch.einsum('bok,bkhw->bohw', w_scaled.abs(), e) + (6 * U32 * (bn['mean'].double() * s2).abs()
                                                                                  + 2 * U32 * bn['b'].double().abs()).view(1, -1, 1, 1) + U32 * O[0].abs() + SUB)
    else:
        GY = ch.mul(Y, tuple(None if t is None else t[:, :, None, None] for t in G))
        sp = plan.get('project')
        if sp is not None:                                  # rows of the SplitWeights carry s2: bound in the scaled units, value unscaled
            P = conv1x1(ch, GY, p['wp'], 'project', tier2)
            if mode == 'bound':
                Ps = conv1x1(ch, (GY[0], GY[1]), p['wp'] * s2.float()[:, None], 'project', tier2, split=sp)
                P = (P[0], Ps[1] / s2.abs().view(1, -1, 1, 1).clamp(min=1e-300))
        else:
            P = conv1x1(ch, GY, p['wp'], 'project', tier2, extra_terms=2)
        O = bn_stage(P, p['bn2'], (1, -1, 1, 1))
    if p['skip']:
        r = x + (0 if in_offset is None else in_offset.double().view(1, -1, 1, 1))
        y = O[0] + r
        O = (y, None if O[1] is None else O[1] + U32 * (y.abs() + O[1]))
    if O[1] is not None and out_offset is not None:
        O = (O[0], O[1] + U32 * out_offset.double().abs().view(1, -1, 1, 1))
    return O


# ------------------------------------------------------------------------------------------------------------ restarting at the route's own intermediates

def pool_own_ref(y_own, partial, tier2=False):
    """The pooled partial sums (B*C, nblk), totalled, against the float64 sum of the route's OWN stored y: (value, error), (B*C,).
    No operand error: the sum rule over H W + nblk terms, or MARGIN * q_cpu of these sums (tier 2)."""
    rows = y_own.double().flatten(2).flatten(0, 1)
    mag = rows.abs().sum(1)
    n = rows.shape[1] + partial.shape[1]
    if tier2 and n > LONG:
        q = R.sum_level(rows[::max(1, rows.shape[0] // 64)][:64].float().contiguous(), (256, 16, 1))
        return rows.sum(1), q * mag + SUB
    return rows.sum(1), sum_bound(n, mag) + SUB


def gate_own_ref(p, partial, batch, hw, tier2=False, fold=False):
    """util_encoder_ref.se_gate_ref on the route's OWN pooled partial sums (fp32, (B*C, nblk)): dict(gate[, w_scaled]) of (value, error).
    ``fold``: also the project weights scaled by the gate and the stock BN2 scale (float64; the fp32 scale buffer's 3 roundings and the
    kernel's two products are added: 4 u |w_scaled|)."""
    c, nblk = partial.shape[0] // batch, partial.shape[1]
    inv32 = torch.tensor(1.0 / float(hw), dtype=torch.float32)
    q = {}
    if tier2 and c * nblk + 1 > LONG:
        q['squeeze'] = R.sum_level((p['w1'][None, :, :, None] * (partial.view(batch, 1, c, nblk) * inv32)).flatten(2), 256)
    ch = Chain('bound', q=q)
    if tier2 and p['w2'].shape[1] > LONG:
        z = R.se_gate_ref(Chain('f64'), partial, batch, float(inv32), p['w1'], p['b1'], p['w2'], p['b2'])['squeezed'][0]
        ch.q['excite'] = R.sum_level(p['w2'][None] * z.float()[:, None, :], 4)
    s2 = bn_scale_shift(p['bn2'])[0] if fold else None
    out = R.se_gate_ref(ch, partial, batch, float(inv32), p['w1'], p['b1'], p['w2'], p['b2'], p['wp'] if fold else None, s2)
    if fold:
        v, e = out['w_scaled']
        out['w_scaled'] = (v, e + 4 * U32 * v.abs())
    return out


def tail_own_ref(p, own, x32, in_offset=None, out_offset=None, plan=None, tier2=False):
    """The block's output from the route's OWN stored intermediates -- ``own``: dict(y fp32 (B, C, Ho, Wo), partial fp32 (B*C, nblk), and
    gate (B, C) or w_scaled (B, Cout, C) where a launch returns one) -- so that the project sum is bounded on its own: y enters with
    error 0, the gate with error 0 where it was stored, else (gemm_split_se derives it inside) as ``gate_own_ref`` of the stored
    partial sums with that short chain's error.  Compared with got + out_offset as everywhere."""
    ch = Chain('bound')
    y = own['y'].double()
    Y = (y, torch.zeros_like(y))
    b = y.shape[0]
    x = x32.double() if p['skip'] else None
    if own.get('w_scaled') is not None:
        return _tail(ch, p, Y, None, x, in_offset, out_offset, plan or {}, tier2, w_scaled=own['w_scaled'].double().flatten(2))
    if own.get('gate') is not None:
        g = own['gate'].double()
        G = (g, torch.zeros_like(g))
    else:
        G = gate_own_ref(p, own['partial'], b, y.shape[2] * y.shape[3], tier2)['gate']
    return _tail(ch, p, Y, G, x, in_offset, out_offset, plan or {}, tier2)


def _bn_absorbing(S, bn, w, off):
    """BN of an expand / reducer / head sum whose VALUE is already at x32 + in_offset while its error is the route's: the ``absorb``
    error is added, the value is not added twice."""
    z, ez = bn_stage(S, bn, (1, -1, 1, 1))
    a = absorbed_of(w, bn, off)
    if ez is not None and a is not None:
        ez = ez + (a[1] + U32 * a[0].abs()).view(1, -1, 1, 1)
    return z, ez


def stem_block0_ref(mode, stem_w, stem_bn, stem_pads, p, img, tier2=False, stop=None):
    """conv_stem + BN + swish, then block 0, of the fp32 image: the stock statement the image-fed forms of block 0 are held to."""
    ch = Chain(mode)
    pt, pl, ph, pw = stem_pads
    ho, wo = (img.shape[2] + ph - 3) // 2 + 1, (img.shape[3] + pw - 3) // 2 + 1
    w_, wa = stem_w.double(), stem_w.double().abs()
    S = ch.summed(ch.inp(img), lambda t: R._dense(t, w_, 2, pt, pl, ho, wo), lambda t: R._dense(t, wa, 2, pt, pl, ho, wo), 28)
    Hs = ch.act(bn_stage(S, stem_bn, (1, -1, 1, 1)), ACT_SWISH)
    return mbconv_block_ref(mode, p, torch.zeros(1), H=Hs, tier2=tier2, stop=stop)


def pointwise_bn_ref(mode, w, bn, act, x32, in_offset=None, split=None, tier2=False):
    """A feature reducer (Conv 1x1 -> BN) or the head (-> swish) at x32 + in_offset.  ``split``: SplitWeights with the BN scale in the rows."""
    ch = Chain(mode)
    X = ch.inp(x32)
    s, _ = bn_scale_shift(bn)
    S = conv1x1(ch, X, w, 'conv', tier2, extra_terms=1)
    if split is not None and mode == 'bound':
        Ss = conv1x1(ch, X, w * s.float()[:, None], 'conv', tier2, split=split)
        S = (S[0], Ss[1] / s.abs().view(1, -1, 1, 1).clamp(min=1e-300))
    if in_offset is not None:
        S = (S[0] + (w.double() @ in_offset.double()).view(1, -1, 1, 1), S[1])
    return ch.act(_bn_absorbing(S, bn, w, in_offset), act)


# ------------------------------------------------------------------------------------------------------------ the stock WeightMapper

def wm_params(wm):
    t = lambda p: p.detach().float().cpu().clone()      # noqa: E731
    return dict(w_in=t(wm.in_conv[0].weight).flatten(1), bn_in=bn_of(wm.in_conv[1]),
                down=[(t(d[0].weight), bn_of(d[1])) for d in wm.down_blocks], up=[(t(u[0].weight).flatten(1), bn_of(u[1])) for u in wm.up_blocks])


def weight_mapper_ref(mode, p, x32, plan=None, tier2=False):
    """The stock v1_0 WeightMapper (one frame) in float64 with the bound.  ``plan``: dict(in / down0.. / up0.. -> SplitWeights with the BN scale
    in the rows) for the stages on the split GEMM.  The pixel-constant half of a merge is bounded as a sum over the FULL K of the
    concatenation, which covers the mat-vec form and the concatenated GEMM alike."""
    ch = Chain(mode)
    plan = plan or {}
    relu = lambda V: ch.act(V, ACT_RELU)      # noqa: E731

    def conv_bn(X, w2d, bn, name, via=None):
        s, _ = bn_scale_shift(bn)
        S = conv1x1(ch, X, w2d, 'conv', tier2, extra_terms=1)
        sw = plan.get(name)
        if sw is not None and mode == 'bound' and via is None:
            S = (S[0], conv1x1(ch, X, w2d * s.float()[:, None], 'conv', tier2, split=sw)[1] / s.abs().view(1, -1, 1, 1).clamp(min=1e-300))
        return relu(bn_stage(S, bn, (1, -1, 1, 1)))

    feat = [conv_bn(ch.inp(x32), p['w_in'], p['bn_in'], 'in')]
    for i, (wd, bn) in enumerate(p['down']):
        v, e = feat[-1]
        _, c, h, w = v.shape
        win = lambda t: t.reshape(1, c, h // 2, 2, w // 2, 2).permute(0, 1, 3, 5, 2, 4).reshape(1, 4 * c, h // 2, w // 2)      # noqa: E731
        feat.append(conv_bn((win(v), None if e is None else win(e)), wd.flatten(1), bn, f'down{i}'))     # k = 4 c + 2 dy + dx: the conv weight's flatten order
    T = feat[-1]
    if T[0].shape[-2:] != (1, 1):
        px = T[0].shape[2] * T[0].shape[3]
        M = ch.summed(T, lambda t: t.mean((2, 3), keepdim=True), lambda t: t.mean((2, 3), keepdim=True), px + 1)
        T = tuple(None if t is None else t.expand_as(T[0]) for t in M)
    for lvl in range(len(p['up']) - 1, -1, -1):
        w, bn = p['up'][lvl]
        skip = feat.pop()
        cat = tuple(None if a is None else torch.cat((a, b_), 1) for a, b_ in zip(skip, T))
        Yv = conv_bn(cat, w, bn, f'up{lvl}', via='cat')
        sw = plan.get(f'up{lvl}')
        if sw is not None and mode == 'bound':          # left half on the split GEMM, right half (pixel-constant) as a mat-vec in the shift
            half = w.shape[1] // 2
            s, _ = bn_scale_shift(bn)
            L = conv1x1(ch, skip, w[:, :half] * s.float()[:, None], 'conv', tier2, split=sw)[1] / s.abs().view(1, -1, 1, 1).clamp(min=1e-300)
            Rt = conv1x1(ch, tuple(t[:, :, :1, :1] for t in T), w[:, half:], 'conv', False, extra_terms=3)[1]
            Sv = conv1x1(Chain('f64'), (cat[0], None), w, 'conv', False)[0]
            Yv = relu(bn_stage((Sv, L + Rt), bn, (1, -1, 1, 1)))
        T = tuple(None if t is None else F.interpolate(t, scale_factor=2, mode='nearest') for t in Yv)
    F0 = feat.pop()
    return tuple(None if a is None else torch.cat((a, b_), 1) for a, b_ in zip(F0, T))


# ------------------------------------------------------------------------------------------------------------ fp32 restatements with defects

def _affine32(bn, defect=None, only=None):
    eps = bn['eps']
    s = bn['w'] / torch.sqrt(bn['var'] + eps)
    if defect == 'bn_eps_dropped':
        bad = bn['w'] / torch.sqrt(bn['var'])
        s = bad if only is None else torch.where(torch.arange(s.numel()) == only, bad, s)
    return s, bn['b'] - bn['mean'] * s


def _swish(t):
    return t * torch.sigmoid(t)


def prepared_block_f32(p, x32, in_offset, defer, defect=None, own=None):
    """The prepared block's algebra in fp32 (stock torch): returns (y, out_offset | None) -- y + out_offset is what is compared.
    ``own``: a dict that receives the intermediates a route stores (y, partial (B*C, 1), gate).
    ``defect``: one of BLOCK_DEFECTS (or None: the right algebra)."""
    assert defect is None or defect in BLOCK_DEFECTS
    pt, pl = p['pads'][:2]
    b, _, h, w = x32.shape
    ho, wo = out_size(p, h, w)
    t = x32
    if p['we'] is not None:
        s0, b0 = _affine32(p['bn0'])
        if in_offset is not None:
            a = p['we'] @ in_offset
            full = s0 * a
            if defect == 'absorb_without_scale':     # every channel: confined to one it is under the bound's squeeze-excite terms
                full = a
            b0 = b0 + full
        t = _swish(torch.einsum('ok,bkhw->bohw', p['we'], t) * s0.view(1, -1, 1, 1) + b0.view(1, -1, 1, 1))
    s1, b1 = _affine32(p['bn1'], defect, only=0)
    y = _swish(R._dw_taps(t, p['wd'], p['k'], p['stride'], pt, pl, ho, wo) * s1.view(1, -1, 1, 1) + b1.view(1, -1, 1, 1))
    count = ho * 4 * ((wo + 3) // 4) if defect == 'mean_padded_count' else ho * wo
    m = y.sum((2, 3)) / count
    g = torch.sigmoid(_swish(m @ p['w1'].t() + p['b1']) @ p['w2'].t() + p['b2'])
    if own is not None:
        own.update(y=y, partial=y.sum((2, 3)).reshape(-1, 1), gate=g)
    s2, b2 = _affine32(p['bn2'])
    out = torch.einsum('ok,bkhw->bohw', p['wp'] * s2[:, None], y * g[:, :, None, None])
    carried = b2.clone()
    if p['skip']:
        out = out + x32
        if in_offset is not None:
            add = in_offset.clone()
            if defect == 'carried_without_in_offset':
                add[0] = 0
            carried = carried + add
    if defer:
        if defect == 'deferred_adds_shift':
            out[:, 0] = out[:, 0] + b2[0]
        return out, carried
    return out + carried.view(1, -1, 1, 1), None


def context_head_f32(p, x32, defect=None):
    """FusedContextHead's algebra in fp32 (one down level: the pooled half as a mat-vec in the shift, nearest 2x into the right half)."""
    assert defect is None or defect in CTX_DEFECTS
    assert len(p['down']) == 1
    _, cin, h, w = x32.shape
    half = cin // 2
    s0, b0 = _affine32(p['bn_in'])
    left = torch.relu(torch.einsum('ok,bkhw->bohw', p['w_in'], x32) * s0.view(1, -1, 1, 1) + b0.view(1, -1, 1, 1))
    wd, bnd = p['down'][0]
    s1, b1 = _affine32(bnd)
    t = torch.relu(F.conv2d(left, wd, stride=2) * s1.view(1, -1, 1, 1) + b1.view(1, -1, 1, 1))
    wu, bnu = p['up'][0]
    s2, b2 = _affine32(bnu)
    wb = s2[:, None] * (wu[:, :half] if defect == 'ctx_wb_left_half' else wu[:, half:])
    if defect == 'ctx_wb_left_half':                 # one output channel only
        wb = torch.cat((wb[:1], s2[1:, None] * wu[1:, half:]))
    shift = b2 + wb @ t.mean((2, 3)).view(half)
    y = torch.relu(torch.einsum('ok,bkhw->bohw', wu[:, :half] * s2[:, None], t) + shift.view(1, -1, 1, 1))
    sh, sw = y.shape[-2:]
    right = torch.empty(1, half, h, w)
    if defect == 'ctx_up2_transposed':
        right.view(half, sw, 2, sh, 2).copy_(y.view(half, sh, sw).transpose(1, 2).reshape(half, sw, 1, sh, 1).expand(half, sw, 2, sh, 2))
    else:
        right.view(half, sh, 2, sw, 2).copy_(y.view(half, sh, 1, sw, 1).expand(half, sh, 2, sw, 2))
    return torch.cat((left, right), 1)


def within(got, V):
    """(ok, worst err / bound, flat index)."""
    v, e = V
    got = got.detach().double().cpu().reshape(v.shape)
    if not bool(torch.isfinite(got).all()):
        return False, float('inf'), -1
    r = (got - v).abs() / e.clamp(min=1e-300)
    i = int(r.argmax())
    return bool((r <= 1).all()), float(r.flatten()[i]), i
