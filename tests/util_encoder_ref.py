"""Host-only float64 statements of the encoder helper kernels (hs_encoder.hip, hs_mbconv.hip, hs_mbconv_lean.hip), the per-element bound
their fp32 results are held to, fp32 restatements (right and deliberately wrong ones) and named range inputs.  Stock torch on the CPU; the
project is not imported.

EVERY OPERATION is a chain of four steps, written ONCE (``Chain``) and run three ways: in float64 (the reference), in float64 on absolute
values with the error carried along (the bound), and in float32 (the CPU restatement, optionally with a defect).  A value travels as
(v, e): v the float64 value, e >= 0 a bound on |kernel's fp32 value - v| for that element, None in the fp32 restatement.

THE BOUND, step by step (u = 2^-23 = util_f16_ref.U32; every input tensor is fp32 and enters with e = 0):

 sum     s = sum_k w_k a_k over K products (K = k*k taps of a depthwise window, 27 / 28 of the stem window, Cin of a 1x1 convolution,
         the pixels of a pooling block, C*nblk and Csq of the squeeze-excite mat-vecs).  With mag = sum_k |w_k| (|a_k| + e_k):
             e_s = sum_k |w_k| e_k  +  (K + 2) u mag  +  SUB
         the first term is the operands' error through the same statement on absolute values (this is how the recomputed ``mid`` of
         expand + depthwise and of stem + depthwise reaches the output), the second util_f16_ref.sum_bound(K, mag): any order, fused or
         unfused products, matrix core or vector ALU; mag carries e_k so that the roundings of the perturbed operands are covered too.  A
         padded tap is an exact 0 on both sides and contributes nothing -- zero padding is applied AFTER the prologue.  A multiplication
         by a gate or a pooled 1/HW in front of a sum is one more product rounding of each term: K + 3.
 affine  z = scale v + shift:  e_z = |scale| e + u (|scale v| + |shift|) + SUB.  One rounding of |scale v| + |shift| for the fused
         multiply-add the kernels use (2^-24), two for an unfused restatement: u covers both.
 act     ReLU / ReLU6 / none are 1-Lipschitz: e.  swish a = z sigmoid(z): |da/dz| <= 1.0999, so the error entering it is multiplied by
         that; the fast form t * rcp(1 + exp2(-log2e t)) gets the project's allowance ACT_ALLOW = 2e-5 of the activation's value (the
         figure of util_split_ref.tail_bound); sigmoid likewise with Lipschitz constant 1/4:
             e_a = 1.0999 (1 + 2e-5) e_z + 2e-5 |a| + FLOOR (|z| + e_z + 1)
         (1 + 2e-5: the allowance is relative to the value at the kernel's own argument).  Why 2e-5 holds over the WHOLE finite range:
         the argument t * -log2e is one fp32 product, and exp2 only matters while |arg| < 128 (beyond, it is inf or 0 exactly like the
         true 2^arg to within FLOOR); there half an ulp of arg is at most 2^-18 and the fp32 constant adds as much again, 2^(2^-17) - 1 <
         5.3e-6 relative in 2^arg; v_exp_f32 and v_rcp_f32 are within 1 ulp each, the addition and the final product half an ulp each:
         < 5.3e-6 + 3 2^-23 < 5.7e-6 relative in the sigmoid (d sigma / sigma = (1 - sigma) d(2^arg) / 2^arg), under 2e-5 with room for
         the CPU restatement's libm.  FLOOR = 2^-126: below the overflow edge (t < -88.7, 2^arg >= 2^128) the kernel's sigmoid is 0 -- the
         swish -0 -- and just above it v_rcp_f32 returns a flushed or imprecise subnormal, while the true sigmoid is under 2^-126: an
         ABSOLUTE error of at most 2^-126 in the sigmoid, |z| 2^-126 in the swish; it reaches a depthwise output multiplied by the taps'
         sum |w| through the ``sum`` rule, which is the floor the outputs get there.
 add     y = a + r (residual): e_y = e_a + 2^-24 (|a| + e_a + |r|).
 SUB = 2^-140 per step: fp32 results in the subnormal range are off by up to 2^-150 per operation whatever their size (<= 2^10 of them).

Per operation (``*_ref`` functions): depthwise = [affine, swish]? -> pad -> sum(k*k) -> affine -> act; stem = pad -> sum(27) -> affine ->
swish; stem + depthwise = stem (K = 28: the padded weight row) -> depthwise on it; expand + depthwise = sum(Cin) -> affine -> swish ->
depthwise; pooled partials = sum over the block's pixels (K = 4 * threads of a depthwise block, OTH * 16 of a tile); their mean over
the nblk blocks adds sum(nblk) and the 1 / HW product; SE gate = mean (K = nblk + 1) -> sum(C) -> +b1 -> swish -> sum(Csq) -> +b2 ->
sigmoid [-> w_proj * gate * out_scale: two product roundings, K = 1]; the kernels sum the squeeze over the flattened (c, i) index, K =
C * nblk + 1, which is what the bound uses; 1x1 conv = (gate * x: K + 3) sum(Cin) -> affine -> act -> add; affine_act_ = affine -> act ->
add.

TIER 2.  For K > 64 the (K + 2) u mag of a sum is orders above what rounding errors do, and a precision-class defect could hide under it.
Following util_split_ref: ``sum_level`` measures q_cpu = max |fp32 sum - float64 sum| / mag of THIS sum on THESE inputs over >= 32
random summation orders of an fp32 restatement on the CPU (a random permutation of the terms, accumulated sequentially in ``lanes``
interleaved partial sums that are then added pairwise -- 4 lanes for the matrix-core k-steps, 256 for the squeeze's workgroup; for the
pools every width from the kernel's down to a plainly sequential sum, since torch's own fp32 ``sum`` is one such order too), and the
tier-2 bound is the tier-1 bound with (K + 2) u replaced by MARGIN * q_cpu, MARGIN = 2 (util_split_ref.MARGIN: the one constant that is a
margin, because the restatement cannot know the kernel's order).  The sums this applies to are NAMED: 'pool' (1024 / 512 / 256 pixels of a
depthwise block, 256 / 128 of a tile), 'expand' (Cin > 64), 'squeeze', 'excite', 'conv'.  Two of them can also be isolated from the error
of their operands, by restating them in float64 on the kernel's OWN stored output: the pooled partial sums on the kernel's y
(``pool_own``) and the excite mat-vec on the kernel's squeezed vector (``se_excite_ref``); there the bound is the sum's alone.  ``q_of``
reports the kernel's own q = max |got - ref| / mag.  The checker is util_f16_ref.assert_within_f16(half=False) with the chain's e as its
``extra64``."""
import functools

import torch
import torch.nn.functional as F

from util_f16_ref import U32, assert_within_f16, sum_bound
from util_split_ref import MARGIN

ACT_NONE, ACT_RELU, ACT_RELU6, ACT_SWISH, ACT_SIGMOID = 0, 1, 2, 3, 4      # 0-3: hs_act; 4 only inside the SE gate
LIP_SWISH, LIP_SIGMOID, ACT_ALLOW = 1.0999, 0.25, 2e-5
FLOOR, SUB = 2.0 ** -126, 2.0 ** -140
DEFECTS = ('pad_swish', 'pad_l_last_quad', 'mean_padded_count', 'pool_dead_rows', 'gate_after_scale', 'residual_before_act', 'exp2_no_log2e')
PREACTS = (0.0, -0.0, 1e-30, -1e-30, 20.0, -20.0, 80.0, -80.0, -88.5, -89.0, -200.0, 1e4)


# ------------------------------------------------------------------------------------------------------------ the four steps

class Chain:
    """Runs the steps in one of three modes: 'f64' (values only), 'bound' (values and errors), 'f32' (the CPU restatement; ``defect``)."""

    def __init__(self, mode, defect=None, q=None):
        assert mode in ('f64', 'bound', 'f32') and (defect is None or defect in DEFECTS)
        self.mode, self.defect, self.dtype = mode, defect, torch.float32 if mode == 'f32' else torch.float64
        self.q = q or {}                  # tier 2: name of a sum -> MARGIN * q_cpu replacing (K + 2) u

    def inp(self, t):
        """An fp32 input tensor (or None) as a travelling value: exact.  A travelling value (v, e) -- another stage's result -- passes
        through as it is, so that the ``*_ref`` stages compose (util_block_ref.py)."""
        if t is None or isinstance(t, tuple):
            return t
        assert t.dtype == torch.float32
        t = t.to(self.dtype)
        return t, (torch.zeros_like(t) if self.mode == 'bound' else None)

    def coef(self, t):
        return None if t is None else t.to(self.dtype)

    def summed(self, V, fn, absfn, terms, name=None):
        """s = fn(v): linear in v; ``absfn`` the same statement with |coefficients|."""
        v, e = V
        s = fn(v)
        if e is None:
            return s, None
        mag = absfn(v.abs() + e)
        return s, absfn(e) + (self.q[name] * mag if name in self.q else sum_bound(terms, mag)) + SUB

    def affine(self, V, scale, shift, shape):
        v, e = V
        sc = None if scale is None else self.coef(scale).view(shape)
        sh = None if shift is None else self.coef(shift).view(shape)
        z = v if sc is None else v * sc
        z = z if sh is None else z + sh
        if e is None:
            return z, None
        a = v.abs() if sc is None else (v * sc).abs()
        e = e if sc is None else e * sc.abs()
        if sc is None and sh is None:
            return z, e
        return z, e + U32 * (a + (0 if sh is None else sh.abs())) + SUB

    def _sigmoid(self, z):
        if self.defect == 'exp2_no_log2e':           # 1 / (1 + 2^-t) instead of 1 / (1 + 2^(-t log2 e)), for |t| > 8 only
            return torch.where(z.abs() > 8, 1 / (1 + torch.exp2(-z)), torch.sigmoid(z))
        return torch.sigmoid(z)

    def act(self, V, code):
        z, e = V
        if code == ACT_NONE:
            return z, e
        if code == ACT_RELU:
            return z.clamp(min=0), e
        if code == ACT_RELU6:
            return z.clamp(0, 6), e
        sg = self._sigmoid(z)
        a = sg if code == ACT_SIGMOID else z * sg
        if e is None:
            return a, None
        lip = LIP_SIGMOID if code == ACT_SIGMOID else LIP_SWISH
        fl = FLOOR if code == ACT_SIGMOID else FLOOR * (z.abs() + e + 1)
        return a, lip * (1 + ACT_ALLOW) * e + ACT_ALLOW * a.abs() + fl

    def mul(self, A, B):
        """The product of two travelling values (broadcast): e = |a| e_b + |b| e_a + e_a e_b + u |a b| (the last: the product's rounding)."""
        (a, ea), (b, eb) = A, B
        p = a * b
        if ea is None or eb is None:
            return p, None
        return p, a.abs() * eb + b.abs() * ea + ea * eb + U32 * p.abs() + SUB

    def add(self, V, R):
        if R is None:
            return V
        (a, e), (r, _) = V, R
        y = a + r
        return y, (None if e is None else e + 2.0 ** -24 * (a.abs() + e + r.abs()))


def _pad_to(t, k, stride, pad_t, pad_l, ho, wo):
    """Zero padding by explicit offsets: top / left as given, bottom / right whatever (ho, wo) outputs need (cropped if negative)."""
    h, w = t.shape[-2:]
    return F.pad(t, (pad_l, (wo - 1) * stride + k - w - pad_l, pad_t, (ho - 1) * stride + k - h - pad_t))


def _dw_taps(t, wt, k, stride, pad_t, pad_l, ho, wo):
    """Depthwise k x k of (B, C, H, W) with (C, 1, k, k) taps as k*k shifted slices (ky, kx ascending: the kernels' order)."""
    p = _pad_to(t, k, stride, pad_t, pad_l, ho, wo)
    out = None
    for ky in range(k):
        for kx in range(k):
            term = p[:, :, ky:ky + (ho - 1) * stride + 1:stride, kx:kx + (wo - 1) * stride + 1:stride] * wt[:, 0, ky, kx].view(1, -1, 1, 1)
            out = term if out is None else out + term
    return out


def _dense(t, wt, stride, pad_t, pad_l, ho, wo):
    return F.conv2d(_pad_to(t, wt.shape[-1], stride, pad_t, pad_l, ho, wo), wt, stride=stride)


def _dw_stage(ch, V, wt, stride, pad_t, pad_l, ho, wo, scale, shift, act):
    """pad -> sum(k*k) -> affine -> act of a (B, C, H, W) value that already carries its prologue."""
    k = wt.shape[-1]
    w_, wa = ch.coef(wt), ch.coef(wt).abs()
    S = ch.summed(V, lambda t: _dw_taps(t, w_, k, stride, pad_t, pad_l, ho, wo), lambda t: _dw_taps(t, wa, k, stride, pad_t, pad_l, ho, wo), k * k)
    if ch.defect == 'pad_l_last_quad' and wo > 4:    # the last quad of every row computed with pad_l + 1
        bad = _dw_taps(V[0], w_, k, stride, pad_t, pad_l + 1, ho, wo)
        cut = 4 * ((wo + 3) // 4 - 1)
        S = (torch.cat([S[0][..., :cut], bad[..., cut:]], -1), None)
    return ch.act(ch.affine(S, scale, shift, (1, -1, 1, 1)), act)


# ------------------------------------------------------------------------------------------------------------ the operations

def dw_threads(ho, wo):
    quads = ho * ((wo + 3) // 4)
    threads = 256 if quads >= 256 else -(-quads // 64) * 64
    return threads, -(-quads // threads)


def pool_stage(ch, Y, group):
    """Sums of Y (B, C, Ho, Wo) over pooling blocks: ``group(t)`` -> (B*C, nblk, pixels) with exact zeros in the dead positions.
    Tier-2 name: 'pool'."""
    terms = group(Y[0]).shape[-1]
    return ch.summed(Y, lambda t: group(t).sum(-1), lambda t: group(t).sum(-1), terms, 'pool')


def dw_group(ho, wo):
    """The depthwise launch's pooling blocks: ``threads`` consecutive output quads in row-major order (4 * threads pixels)."""
    threads, nblk = dw_threads(ho, wo)
    return lambda t: _blocks_of(t, threads, nblk)


def tile_group(oth):
    """The fused launches' pooling blocks: OTH x 16 output tiles."""
    return lambda t: _tiles_of(t, oth)


def pool_level(y, group, lanes, rows=512):
    """``sum_level`` of the pooling sums of y (values as the kernel stores them, fp32), over at most ``rows`` evenly spaced blocks: the level
    is a maximum over blocks x orders, and 512 blocks x 32 orders are more samples than any launch here has blocks."""
    t = group(y.float()).flatten(0, 1)
    step = max(1, t.shape[0] // rows)
    return sum_level(t[::step][:rows].contiguous(), (lanes, 16, 1))


def pool_own(got_y, group, level=None):
    """The partial sums held against the float64 sums of the kernel's OWN stored outputs: no operand error, so the bound is the sum's
    alone -- MARGIN x the CPU level (tier 2) or sum_bound over the block's pixels.  This is the check a defect of the pooling reduction
    itself (wave or LDS reduce, last-block handling) cannot hide from."""
    y = group(got_y.detach().double().cpu())
    mag = y.abs().sum(-1)
    return y.sum(-1), (level * mag if level is not None else sum_bound(y.shape[-1], mag)) + SUB


def _blocks_of(t, threads, nblk):
    b, c, ho, wo = t.shape
    wq = (wo + 3) // 4
    flat = F.pad(t, (0, 4 * wq - wo)).reshape(b * c, ho * wq * 4)
    return F.pad(flat, (0, nblk * threads * 4 - flat.shape[1])).reshape(b * c, nblk, threads * 4)


def _tiles_of(t, oth, otw=16):
    b, c, ho, wo = t.shape
    ty, tx = -(-ho // oth), -(-wo // otw)
    p = F.pad(t, (0, tx * otw - wo, 0, ty * oth - ho)).reshape(b * c, ty, oth, tx, otw)
    return p.permute(0, 1, 3, 2, 4).reshape(b * c, ty * tx, oth * otw)


def pooled_mean(ch, P, hw, batch):
    """(B, C) mean of the outputs from the partial sums (B*C, nblk): sum(nblk) and the product with 1 / HW."""
    nblk = P[0].shape[1]
    M = ch.summed(P, lambda t: t.sum(1) / hw, lambda t: t.sum(1) / hw, nblk + 1)
    return tuple(None if t is None else t.view(batch, -1) for t in M)


def depthwise_ref(ch, x, wt, stride, pad_t, pad_l, out_size, scale=None, shift=None, act=ACT_SWISH, in_scale=None, in_shift=None, pool=True):
    """hs_depthwise_conv_fwd: dict(y, partial (B*C, nblk), mean (B, C)), each (value, error)."""
    ho, wo = out_size
    X = ch.inp(x)
    if in_scale is not None:
        if ch.defect == 'pad_swish':                 # the prologue applied to the zero padding as well: a padded tap is swish(in_shift)
            k = wt.shape[-1]
            X = (_pad_to(X[0], k, stride, pad_t, pad_l, ho, wo), None)
            pad_t = pad_l = 0
        X = ch.act(ch.affine(X, in_scale, in_shift, (1, -1, 1, 1)), ACT_SWISH)
    Y = _dw_stage(ch, X, wt, stride, pad_t, pad_l, ho, wo, scale, shift, act)
    out = dict(y=Y)
    if pool:
        threads, nblk = dw_threads(ho, wo)
        if ch.defect == 'pool_dead_rows':            # the last block's dead quads computed like live rows below the map, and counted
            rows = -(-nblk * threads // ((wo + 3) // 4))
            ext = depthwise_ref(Chain('f32'), x, wt, stride, pad_t, pad_l, (rows, wo), scale, shift, act, in_scale, in_shift, pool=False)['y']
            out['partial'] = (_blocks_of(ext[0], threads, nblk)[:, :, :].sum(-1), None)
        else:
            out['partial'] = pool_stage(ch, Y, dw_group(ho, wo))
        hw = ho * (4 * ((wo + 3) // 4)) if ch.defect == 'mean_padded_count' else ho * wo
        out['mean'] = pooled_mean(ch, out['partial'], float(hw), x.shape[0])
    return out


def stem_ref(ch, x, wt, pad_t, pad_l, out_size, scale, shift, terms=27):
    """hs_stem_conv_fwd: swish(BN(conv3x3 / stride 2 of the zero-padded image))."""
    ho, wo = out_size
    w_, wa = ch.coef(wt), ch.coef(wt).abs()
    S = ch.summed(ch.inp(x), lambda t: _dense(t, w_, 2, pad_t, pad_l, ho, wo), lambda t: _dense(t, wa, 2, pad_t, pad_l, ho, wo), terms)
    return ch.act(ch.affine(S, scale, shift, (1, -1, 1, 1)), ACT_SWISH)


def _tile_pool(ch, Y, oth, batch):
    ho, wo = Y[0].shape[-2:]
    if ch.defect == 'pool_dead_rows':
        raise NotImplementedError
    P = pool_stage(ch, Y, tile_group(oth))
    return dict(y=Y, partial=P, mean=pooled_mean(ch, P, float(ho * wo), batch))


def stem_dw_ref(ch, x, w_stem, s0, b0, stem_pad_t, stem_pad_l, stem_out, w_dw, pad_t, pad_l, s1, b1, oth=16):
    """hs_stem_dw_fwd: the stem (K = 28: the weight row padded with one zero), then depthwise 3x3 / stride 1 + BN + swish, pooled per tile."""
    mid = stem_ref(ch, x, w_stem, stem_pad_t, stem_pad_l, stem_out, s0, b0, terms=28)
    return _tile_pool(ch, _dw_stage(ch, mid, w_dw, 1, pad_t, pad_l, stem_out[0], stem_out[1], s1, b1, ACT_SWISH), oth, x.shape[0])


def mbconv_ref(ch, x, w_e, s0, b0, w_dw, stride, pad_t, pad_l, out_size, s1, b1):
    """hs_mbconv_expand_dw_fwd: swish(BN1(depthwise(zero-pad(swish(BN0(W_e . x)))))), pooled per OTH x 16 tile (OTH = 16 / 8 for stride 1 / 2).
    Tier-2 names: 'expand' (K = Cin), 'pool'."""
    w_ = ch.coef(w_e).flatten(1)
    wa = w_.abs()
    mm = lambda m: (lambda t: torch.einsum('oc,bchw->bohw', m, t))      # noqa: E731
    mid = ch.act(ch.affine(ch.summed(ch.inp(x), mm(w_), mm(wa), w_.shape[1], 'expand'), s0, b0, (1, -1, 1, 1)), ACT_SWISH)
    return _tile_pool(ch, _dw_stage(ch, mid, w_dw, stride, pad_t, pad_l, out_size[0], out_size[1], s1, b1, ACT_SWISH), 16 if stride == 1 else 8, x.shape[0])


def se_excite_ref(ch, Z, w2, b2):
    """gate = sigmoid(b2 + w2 z) from a squeezed value Z (B, Csq) -- the reference's, or the kernel's own output with error 0."""
    w2_ = ch.coef(w2)
    ex = lambda m: (lambda t: t @ m.t())      # noqa: E731
    return ch.act(ch.affine(ch.summed(Z, ex(w2_), ex(w2_.abs()), w2.shape[1], 'excite'), None, b2, (1, -1)), ACT_SIGMOID)


def se_gate_ref(ch, partial, batch, inv_hw32, w1, b1, w2, b2, w_proj=None, out_scale=None):
    """hs_se_gate_fwd: dict(squeezed (B, Csq), gate (B, C)[, w_scaled (B, Cout, C)]).  ``inv_hw32``: the fp32 value the launcher is handed;
    w2 (C, Csq) untransposed.  Tier-2 names: 'squeeze' (K = C * nblk + 1), 'excite' (K = Csq)."""
    c, nblk = partial.shape[0] // batch, partial.shape[1]
    inv = float(torch.tensor(inv_hw32, dtype=torch.float32))
    w1_ = ch.coef(w1)
    P = tuple(None if t is None else t.view(batch, c, nblk) for t in ch.inp(partial))
    sq = lambda m: (lambda t: torch.einsum('jc,bc->bj', m, t.sum(2)) * inv)      # noqa: E731
    T = ch.summed(P, sq(w1_), sq(w1_.abs()), c * nblk + 1, 'squeeze')
    Z = ch.act(ch.affine(T, None, b1, (1, -1)), ACT_SWISH)
    G = se_excite_ref(ch, Z, w2, b2)
    out = dict(squeezed=Z, gate=G)
    if w_proj is not None:
        wp = ch.coef(w_proj).flatten(1)
        if out_scale is not None:
            wp = wp * ch.coef(out_scale)[:, None]          # exact in float64; the kernel's second product rounding is in K = 1
        out['w_scaled'] = ch.summed(G, lambda t: wp[None] * t[:, None, :], lambda t: wp.abs()[None] * t[:, None, :], 1)
    return out


def pointwise_ref(ch, x, w, gate=None, scale=None, shift=None, act=ACT_NONE, residual=None):
    """hs_pointwise_conv_fwd on x (B, Cin, P): act(scale * sum_c w[o,c] (gate[b,c] x[b,c,p]) + shift) + residual.  Tier-2 name: 'conv'."""
    w_ = ch.coef(w).flatten(1)
    cin = w_.shape[1]
    if isinstance(gate, tuple):                      # a travelling gate (B, Cin): the product carries both operands' errors and its own rounding
        x = ch.mul(ch.inp(x), tuple(None if t is None else t[:, :, None] for t in gate))
        gate = None
    g = None if gate is None else ch.coef(gate)
    after = ch.defect == 'gate_after_scale' and g is not None
    gx = lambda t: t if (g is None or after) else t * g[:, :, None]      # noqa: E731
    S = ch.summed(ch.inp(x), lambda t: torch.einsum('oc,bcp->bop', w_, gx(t)), lambda t: torch.einsum('oc,bcp->bop', w_.abs(), gx(t).abs()),
                  cin + (0 if gate is None else 1), 'conv')
    Z = ch.affine(S, scale, shift, (1, -1, 1))
    if after:                                        # the gate of channel o % Cin on the scaled sum instead of on x
        Z = (Z[0] * g[:, torch.arange(w_.shape[0]) % cin, None], None)
    R = ch.inp(residual)
    if ch.defect == 'residual_before_act' and R is not None:
        return ch.act(ch.add(Z, R), act)
    return ch.add(ch.act(Z, act), R)


def affine_act_ref(ch, x, scale, shift, act=ACT_NONE, residual=None):
    """hs_affine_act_fwd on (B, C, P)."""
    Z = ch.affine(ch.inp(x), scale, shift, (1, -1, 1))
    R = ch.inp(residual)
    if ch.defect == 'residual_before_act' and R is not None:
        return ch.act(ch.add(Z, R), act)
    return ch.add(ch.act(Z, act), R)


# ------------------------------------------------------------------------------------------------------------ checking

def check(got, V, what):
    """|got - v| <= e elementwise, got finite; returns (worst err / bound, flat index).  ``V`` from a Chain('bound')."""
    v, e = V
    got = got.detach().double().cpu().reshape(v.shape)
    assert bool(torch.isfinite(v).all()) and bool(torch.isfinite(e).all()), f'{what}: the reference is not finite'
    assert_within_f16(got, v, 0, 0.0, extra64=e, half=False, what=what)      # the chain's e is the whole bound: no further sum term
    ratio = (got - v).abs() / e.clamp(min=1e-300)
    i = int(ratio.argmax())
    return float(ratio.flatten()[i]), i


def rejects(got, V):
    """True when ``got`` leaves the bound somewhere (the teeth test's question)."""
    v, e = V
    got = got.detach().double().reshape(v.shape)
    return bool((~torch.isfinite(got)).any()) or bool(((got - v).abs() > e).any())


def sum_level(terms, lanes, count=32, seed=0):
    """Tier 2: MARGIN * q_cpu for the sum over the LAST dimension of ``terms`` (fp32 products, any leading shape): q_cpu = max over
    ``count`` random orders and all rows of |fp32 sum - float64 sum| / sum |terms|.  An order = a random permutation, accumulated
    sequentially in L interleaved fp32 partial sums which are then added pairwise, for every L of ``lanes`` (an int or several): the
    restatement cannot know how wide the kernel -- or any other fp32 restatement, torch's own ``sum`` included -- accumulates, so the
    widths from the kernel's own down to 1 (plainly sequential) all count as orders.  At most 2^20 / n evenly spaced rows are used."""
    assert terms.dtype == torch.float32 and count >= 32
    n = terms.shape[-1]
    t = terms.reshape(-1, n)
    rows = max(1, (1 << 20) // n)
    t = t[::max(1, t.shape[0] // rows)][:rows]
    g = torch.Generator().manual_seed(2000 + seed)
    exact, mag = t.double().sum(-1)[:, None], t.double().abs().sum(-1).clamp(min=1e-300)[:, None]
    tp = t[:, torch.stack([torch.randperm(n, generator=g) for _ in range(count)])]          # (rows, count, n)
    q = 0.0
    for width in ((lanes,) if isinstance(lanes, int) else lanes):
        steps = -(-n // width)
        u = F.pad(tp, (0, steps * width - n)).reshape(t.shape[0], count, steps, width)
        acc = u[:, :, 0].clone()
        for s in range(1, steps):
            acc = acc + u[:, :, s]
        m = width
        while m > 1:
            half = (m + 1) // 2
            acc = torch.cat([acc[..., :m - half] + acc[..., half:m], acc[..., m - half:half]], -1)
            m = half
        q = max(q, float(((acc[..., 0].double() - exact).abs() / mag).max()))
    return MARGIN * q


def q_of(got, V, mag):
    """The kernel's own q = max |got - v| / mag and its flat index, for the report."""
    got = got.detach().double().cpu().reshape(V[0].shape)
    r = (got - V[0]).abs() / mag.clamp(min=1e-300)
    i = int(r.argmax())
    return float(r.flatten()[i]), i


# ------------------------------------------------------------------------------------------------------------ range inputs

GENERATORS = ('benign', 'preact', 'quiet', 'gates', 'pixel_sums')


def _sweep(c, g, ref_mag=1.0):
    """Per-channel (scale, shift) that put the pre-activation scale * v + shift of channel i at PREACTS[i % 12] (1 +- 0.01 v / ref_mag)."""
    p = torch.tensor([PREACTS[i % len(PREACTS)] for i in range(c)], dtype=torch.float32)
    return (p.abs() * (0.01 / ref_mag)).float(), p


def dw_inputs(name, b, c, h, w, k, seed, prologue):
    """dict(x, wt, scale, shift, in_scale, in_shift) for a depthwise case.  'preact' sweeps the prologue's pre-activation per channel when
    there is one, the output BatchNorm's otherwise; 'quiet' makes every odd channel's output ~1e-4 of its neighbours'."""
    assert name in ('benign', 'preact', 'quiet'), name
    g = torch.Generator().manual_seed(int(seed))
    d = dict(x=torch.randn(b, c, h, w, generator=g), wt=torch.randn(c, 1, k, k, generator=g) * 0.3,
             scale=torch.rand(c, generator=g) + 0.5, shift=torch.randn(c, generator=g) * 0.1,
             in_scale=torch.rand(c, generator=g) + 0.5 if prologue else None, in_shift=torch.randn(c, generator=g) * 0.1 if prologue else None)
    if name == 'preact' and prologue:
        d['in_scale'], d['in_shift'] = _sweep(c, g)
    elif name == 'preact':
        d['scale'], d['shift'] = _sweep(c, g, ref_mag=0.3 * k)
    elif name == 'quiet':
        q = torch.where(torch.arange(c) % 2 == 1, 1e-4, 1.0)
        d['scale'], d['shift'] = d['scale'] * q, d['shift'] * q
    return d


def pw_inputs(name, b, cin, cout, p, seed, gate=True, residual=True):
    """dict(x (B, Cin, P), w, gate, scale, shift, residual).  'gates': exact 0, 1e-20 and 1 in turn; 'preact': the BatchNorm sweep of
    ``_sweep`` per output channel; 'quiet': every odd output row ~1e-4 of the others."""
    assert name in ('benign', 'preact', 'quiet', 'gates'), name
    g = torch.Generator().manual_seed(int(seed))
    d = dict(x=torch.randn(b, cin, p, generator=g), w=torch.randn(cout, cin, generator=g) / cin ** 0.5,
             gate=torch.rand(b, cin, generator=g) if gate else None, scale=torch.rand(cout, generator=g) + 0.5,
             shift=torch.randn(cout, generator=g) * 0.1, residual=torch.randn(b, cout, p, generator=g) if residual else None)
    if name == 'gates':
        d['gate'] = torch.tensor([0.0, 1e-20, 1.0])[torch.arange(b * cin) % 3].view(b, cin).contiguous()
    elif name == 'preact':
        d['scale'], d['shift'] = _sweep(cout, g)
    elif name == 'quiet':
        q = torch.where(torch.arange(cout) % 2 == 1, 1e-4, 1.0)
        d['w'], d['shift'] = d['w'] * q[:, None], d['shift'] * q
    return d


def se_inputs(name, batch, c, csq, nblk, cout, seed):
    """dict(partial, hw, w1, b1, w2, b2, wp, osc).  'pixel_sums': partial sums of 1024-pixel blocks of O(1) activations -- magnitudes 1e2
    to 1e4 -- with HW = 1024 nblk, and an expand bias that sweeps the sigmoid's argument over -30 .. 30 (saturated both ways)."""
    assert name in ('benign', 'pixel_sums'), name
    g = torch.Generator().manual_seed(int(seed))
    d = dict(partial=torch.randn(batch * c, nblk, generator=g), hw=77.0, w1=torch.randn(csq, c, generator=g) / c ** 0.5,
             b1=torch.randn(csq, generator=g) * 0.1, w2=torch.randn(c, csq, generator=g) / csq ** 0.5, b2=torch.randn(c, generator=g) * 0.1,
             wp=torch.randn(cout, c, generator=g), osc=torch.rand(cout, generator=g) + 0.5)
    if name == 'pixel_sums':
        mag = torch.exp(torch.empty(batch * c, 1).uniform_(4.6, 9.2, generator=g))                 # 1e2 .. 1e4
        d['partial'] = (torch.rand(batch * c, nblk, generator=g) * 0.5 + 0.75) * mag * torch.where(torch.rand(batch * c, 1, generator=g) < 0.3, -0.25, 1.0)
        d['hw'] = 1024.0 * nblk
        d['b2'] = torch.linspace(-30, 30, c)
    return d


@functools.lru_cache(maxsize=None)
def same_pads(h, w, k, stride):
    """TF-"SAME": (pad_t, pad_l, Ho, Wo)."""
    ho, wo = -(-h // stride), -(-w // stride)
    return max((ho - 1) * stride + k - h, 0) // 2, max((wo - 1) * stride + k - w, 0) // 2, ho, wo


def sym_pads(h, w, k, stride):
    """torch-style symmetric k // 2: (pad_t, pad_l, Ho, Wo)."""
    p = k // 2
    return p, p, (h + 2 * p - k) // stride + 1, (w + 2 * p - k) // stride + 1
