"""Host-only float64 statements of the fp32 training-path operations (hs_patch_conv_bwd.hip, hs_train_aux.hip), differentiated by float64
autograd, and the per-element bound the fp32 kernels are held to.  Imports neither the project nor the GPU.

What is stated elsewhere is used from there, not copied: util_decoder_ref (pad2d, conv_core, G, randn, pow2_gains, check, rejects,
old_rel_err), util_f16_ref (halo_tiles, bn_train_ref, sum_bound, U32).  New here: the general k x k grouped patch convolution's two adjoints
in all four padding modes (autograd of conv_core), BatchNorm + none / ReLU / ReLU6 in training mode as a case (bn_train_ref), the adjoints
of the halo tiles, the tile interior, the valid depthwise of tiles (dw_tiles_valid through bilinear_with_grads), the bilinear resize
(upsample) and meta_conv, plain and weighted per-pixel cross entropy (pixel_ce) with util_confidence_ref's stated-ulp allowances, and Adam.

The bound is the fp32 part of the project's bound: an output that sums ``terms`` products in fp32 is within

    |got - ref64| <= (terms + 2) 2^-23 mag64 + terms 2^-126

of the float64 value; mag64 is the same statement on absolute values.  ``terms`` is COUNTED by the statement itself, per element: the
adjoint evaluated on all-one operands is the number of products behind each output (cout_g k^2 for an interior dX element, more where a
reflect / replicate / circular halo folds back onto it, fewer at a zero-padded border; ph pw for a bank-gradient element).  The second
term is the f32 matrix-core instruction's possible flush of subnormal products: the generators keep every operand normal and every
product far above 2^-126, so it only ever matters as a statement.  No tolerance here is a measured constant.

Generators (``patch_conv_case(gen=...)``): 'benign' = randn from G(seed); 'range' = the same with power-of-two gains per input channel,
per output channel of dY, per patch and per (row, tap) of the bank, so that a value taken from the wrong channel, patch or tap lands
orders of magnitude outside the bound.

DEFECTS: wrong restatements the bound must reject (``defective(name)`` gives the defective fp32 value and the V it is checked against)."""
import functools

import torch

import util_decoder_ref as D
import util_f16_ref as F16
from util_decoder_ref import G, check, old_rel_err, pow2_gains, randn, rejects  # noqa: F401  (re-exported)
from util_f16_ref import U32, sum_bound

FLUSH = 2.0 ** -126
DEFECTS = ('chunk_tail_pixel_dropped', 'dw_tile_last_row_dropped', 'reflect_corner_off_by_one', 'group_offset_from_group_0', 'swapped_pair',
           'halo_adjoint_without_corner', 'dgamma_without_relu6_mask', 'adam_without_bias_correction', 'ce_weight_of_next_class',
           'ce_ignored_pixel_not_zeroed', 'upsample_tap_off_by_one', 'meta_conv_last_tap_dropped', 'dw_tiles_neighbour_patch_taps',
           's2w_group_offset_from_group_0', 'bootstrap_tie_takes_all')


# ------------------------------------------------------------------------------------------------------------ patch convolution

def patch_conv_case(gen, seed, b, cin, size, grid, c_out, k, mode, groups):
    """{x (B, cin, H, W), bank (P, rows), dy (B, c_out, H, W)} in fp32 plus the geometry; 'range': gains as in the module docstring
    (kept in the case as ``gains`` for test_range_inputs_reach_their_regimes)."""
    g = G(2 * seed + (gen == 'range'))
    (h, w), (fh, fw) = size, grid
    n = (cin // groups) * k * k
    rows, patches = c_out * n, b * fh * fw
    d = dict(x=randn(g, b, cin, h, w), bank=randn(g, patches, rows) * n ** -0.5, dy=randn(g, b, c_out, h, w), grid=grid, c_out=c_out, k=k, mode=mode,
             groups=groups)
    if gen == 'range':
        gx, gy, gp, gr = pow2_gains(g, cin, -6, 6), pow2_gains(g, c_out, -6, 6), pow2_gains(g, patches, -4, 4), pow2_gains(g, rows, -6, 6)
        for t in (gx, gy, gr):                       # the span is there whatever the draw: first and last at the two ends
            t[0], t[-1] = 2.0 ** 6, 2.0 ** -6
        d['x'] = d['x'] * gx.view(1, -1, 1, 1)
        d['dy'] = d['dy'] * gy.view(1, -1, 1, 1)
        d['bank'] = d['bank'] * gp.view(-1, 1) * gr.view(1, -1)
        d['gains'] = dict(x=gx, dy=gy, patch=gp, row=gr)
    return d


def _conv(x, bank, d, defect=None):
    return D.conv_core(x, bank, d['grid'], d['c_out'], d['k'], d['mode'], d['groups'], defect)


def patch_conv_grads(d, dt=torch.float64, role='value', defect=None):
    """(dx, dbank) of y = conv_core(x, bank) for the upstream dy, by autograd in ``dt``.  role 'abs': on absolute values (mag64); 'count':
    on all-one operands (the number of products behind every element)."""
    x, bank, dy = (d[k].to(dt) for k in ('x', 'bank', 'dy'))
    if role == 'abs':
        x, bank, dy = x.abs(), bank.abs(), dy.abs()
    elif role == 'count':
        x, bank, dy = torch.ones_like(x), torch.ones_like(bank), torch.ones_like(dy)
    x, bank = x.clone().requires_grad_(True), bank.clone().requires_grad_(True)
    dx, dw = torch.autograd.grad(_conv(x, bank, d, 'halo_corner_off_by_one' if defect == 'reflect_corner_off_by_one' else None), (x, bank), dy)
    if defect == 'group_offset_from_group_0' and d['groups'] > 1:           # every group's dX computed with group 0's filters
        cout_g, rows = d['c_out'] // d['groups'], d['bank'].shape[1] // d['groups']
        b0 = torch.cat([bank.detach()[:, :rows]] * d['groups'], 1).requires_grad_(True)
        dx = torch.autograd.grad(_conv(x, b0, d), x, dy)[0]
        assert cout_g > 0
    dx, dw = dx.detach().clone(), dw.detach().clone()
    b, cin, h, w = dx.shape
    (fh, fw), c_out = d['grid'], d['c_out']
    ph, pw = h // fh, w // fw
    if defect == 'chunk_tail_pixel_dropped':                                # the last pixel of every patch (a partial 16-pixel chunk's tail) not stored
        dx.view(b, cin, fh, ph, fw, pw)[:, :, :, -1, :, -1] = 0
    if defect == 'swapped_pair':                                            # the two elements of the first pair of every row stored swapped
        dx[..., :2] = dx[..., :2].flip(-1)
    if defect == 'dw_tile_last_row_dropped':                                # the last output-channel row of a 16-row tile
        rows = dw.shape[1] // c_out
        o = min(15, c_out - 1)
        dw[:, o * rows:(o + 1) * rows] = 0
    return dx, dw


def _counted_bound(count, mag):
    return (count + 2.0) * U32 * mag + count * FLUSH


def patch_conv_bwd_ref(d):
    """{'dx': V, 'dw': V}, V = {'ref', 'bound', 'mag', 'terms'} (terms: the per-element count)."""
    out = {}
    ref, mag, cnt = (patch_conv_grads(d, role=r) for r in ('value', 'abs', 'count'))
    for i, key in enumerate(('dx', 'dw')):
        out[key] = dict(ref=ref[i], mag=mag[i], terms=cnt[i], bound=_counted_bound(cnt[i], mag[i]))
    return out


# ------------------------------------------------------------------------------------------------------------ halo tiles (adjoint)

def halo_adjoint(x, dt_tiles, grid, defect=None):
    """The adjoint of util_f16_ref.halo_tiles for the upstream ``dt_tiles`` (the image of tiles); 'halo_adjoint_without_corner': the four
    image corners' diagonal halo cells are not folded back."""
    xa = x.clone().requires_grad_(True)
    t = F16.halo_tiles(xa, grid)
    if defect == 'halo_adjoint_without_corner':
        dt_tiles = dt_tiles.clone()
        for i in (0, -1):
            for j in (0, -1):
                dt_tiles[..., i, j] = 0
    return torch.autograd.grad(t, xa, dt_tiles)[0]


def halo_adjoint_ref(x, dt_tiles, grid):
    """An interior pixel sums at most 4 copies (two tiles per axis), a reflected one at most 9: terms counted on ones."""
    ref = halo_adjoint(x.double(), dt_tiles.double(), grid)
    mag = halo_adjoint(x.double(), dt_tiles.double().abs(), grid)
    cnt = halo_adjoint(x.double(), torch.ones_like(dt_tiles, dtype=torch.float64), grid)
    return dict(ref=ref, mag=mag, terms=cnt, bound=_counted_bound(cnt, mag))


# ------------------------------------------------------------------------------------------------------------ BatchNorm + activation

ACTS = {0: 'none', 1: 'relu', 2: 'relu6'}        # hs_act code -> bn_train_ref's ``act`` argument


def bn_case(gen, seed, b, c, size):
    g = G(2 * seed + (gen == 'range'))
    x, r = randn(g, b, c, *size) * 1.5 + 0.5, randn(g, b, c, *size)
    w, bias = 0.5 + torch.rand(c, generator=g), 1.5 + 0.5 * randn(g, c)       # z around 1.5 +- 1: both ReLU6 clamps are reached
    if gen == 'range':
        gx, gr = pow2_gains(g, c, -8, 8), pow2_gains(g, c, -8, 8)
        gx[0], gx[-1], gr[0], gr[-1] = 2.0 ** 8, 2.0 ** -8, 2.0 ** -8, 2.0 ** 8
        x, r = x * gx.view(1, -1, 1, 1), r * gr.view(1, -1, 1, 1)
        return dict(x=x, r=r, w=w, b=bias, gains=dict(x=gx, r=gr))
    return dict(x=x, r=r, w=w, b=bias)


def bn_ref(d, act, eps=1e-5):
    """bn_train_ref's results as V dicts: y, dx, dg, db, mean, var.  The bound of each is (n + 2) 2^-23 mag64 + extra64 (bn_train_ref's
    docstring: n = B H W, the extra for ReLU units undecided within the forward's own bound)."""
    R = F16.bn_train_ref(d['x'].double(), d['w'].double(), d['b'].double(), d['r'].double(), eps=eps, act=ACTS[act])
    out = {}
    for k in ('y', 'dx', 'dg', 'db', 'mean', 'var'):
        ref, mag, extra = R[k]
        bound = sum_bound(R['n'], mag) + (extra if extra is not None else 0.0)
        out[k] = dict(ref=ref, mag=mag.expand_as(ref) if mag.dim() == ref.dim() else mag, bound=bound.expand_as(ref) if bound.dim() == ref.dim() else bound)
    return out


def bn_restate(d, act, dt=torch.float32, eps=1e-5, defect=None):
    """Train-mode batch_norm + activation and its adjoint in ``dt`` with stock ops; 'dgamma_without_relu6_mask': dgamma sums r x_hat over
    every element instead of the live ones."""
    x, w, b = (d[k].to(dt).clone().requires_grad_(True) for k in ('x', 'w', 'b'))
    y = F16.bn_relu6(x, w, b, eps, act=ACTS[act])
    dx, dg, db = torch.autograd.grad(y, (x, w, b), d['r'].to(dt))
    if defect == 'dgamma_without_relu6_mask':
        xd = d['x'].to(dt)
        mean, var = xd.mean((0, 2, 3), keepdim=True), xd.var((0, 2, 3), unbiased=False, keepdim=True)
        dg = (d['r'].to(dt) * (xd - mean) * (var + eps).rsqrt()).sum((0, 2, 3))
    return dict(y=y.detach(), dx=dx, dg=dg, db=db)


# ------------------------------------------------------------------------------------------------------------ Adam

def adam_steps(p, grads, lr, betas, eps, wd=0.0, dt=torch.float64, defect=None):
    """torch.optim.Adam's arithmetic (coupled weight decay, bias-corrected) over ``grads`` (one per step) from zero moments; returns the
    list of parameters after each step.  'adam_without_bias_correction': 1 - beta^t taken as 1."""
    b1, b2 = betas
    p, m, v = p.to(dt).clone(), torch.zeros_like(p, dtype=dt), torch.zeros_like(p, dtype=dt)
    out = []
    for t, g in enumerate(grads, 1):
        g = g.to(dt) + wd * p if wd else g.to(dt)
        m = m + (1 - b1) * (g - m)
        v = b2 * v + (1 - b2) * g * g
        bc1, bc2 = (1.0, 1.0) if defect == 'adam_without_bias_correction' else (1 - b1 ** t, 1 - b2 ** t)
        p = p - (lr / bc1) * m / (v.sqrt() / bc2 ** 0.5 + eps)
        out.append(p.clone())
    return out


def adam_ref(p, grads, lr, betas, eps, wd=0.0):
    """V per step for hs_adam_step's operation order (hs_train_aux.hip adam_kernel).  Every rounding is allowed u = 2^-23, TWICE the unit
    roundoff of a round-to-nearest fp32 operation -- the same factor two that (terms + 2) 2^-23 carries over the first-order terms 2^-24
    in sum_bound, and the only allowance for the second order here.  The roundings, counted from the kernel:
      g   (weight decay) wd narrowed, wd p, the add: |dg| <= wd |dp| + 3 u (|g| + wd |p|), dp the parameter's own error so far;
      m   om1 = (float)(1 - b1) narrowed, d = g - m, om1 d, m + ..: 4 a step on convex weights, so after s steps |dm| <= 4 s u mag_m + the
          lerp of dg, mag_m the same lerp of |g|;
      v   b2 narrowed, b2 v | om2 narrowed, g g, om2 (g g) | the add: at most 4 a step, every term positive: |dv| <= 4 s u v + 2 |g| dg lerped;
      den sqrtf (halves v's relative error, 1), bc2 narrowed and its sqrtf (1.5 -> 2), the quotient (1), eps narrowed and the add (2);
      step_size  lr narrowed, bc1 narrowed, the quotient (3);  the update  step_size m (1), / den (1).
    That is 1 + 2 + 1 + 2 + 3 + 2 = 11 roundings on the update beside m's and v's own: |d upd| <= step_size / den (|dm| + (11 u + rel_v / 2) |m|).
    The subtraction rounds once on |p|.  The errors add over the steps."""
    u = U32
    b1, b2 = betas
    ref = adam_steps(p, grads, lr, betas, eps, wd)
    pp, m, v, mag_m = p.double().clone(), 0.0, 0.0, 0.0
    perr, dm, dv = torch.zeros_like(p, dtype=torch.float64), 0.0, 0.0
    out = []
    for s, g0 in enumerate(grads, 1):
        g = g0.double() + wd * pp if wd else g0.double()
        dg = wd * perr + 3 * u * (g0.double().abs() + wd * pp.abs()) if wd else 0.0
        m, v = m + (1 - b1) * (g - m), b2 * v + (1 - b2) * g * g
        mag_m = b1 * mag_m + (1 - b1) * g.abs()
        dm = b1 * dm + (1 - b1) * dg
        dv = b2 * dv + (1 - b2) * (2 * g.abs() * dg + dg * dg)
        bc1, bc2 = 1 - b1 ** s, 1 - b2 ** s
        den = v.sqrt() / bc2 ** 0.5 + eps
        rel_v = 4 * s * u + dv / v.clamp(min=1e-300)
        upd_err = (lr / bc1) / den * (4 * s * u * mag_m + dm + (11 * u + rel_v / 2) * m.abs())
        pp = ref[s - 1]
        perr = perr + upd_err + u * pp.abs()
        out.append(dict(ref=pp, bound=perr.clone(), mag=pp.abs() + (lr / bc1) * mag_m / den))
    return out


# ------------------------------------------------------------------------------------------------------------ tile re-layouts, valid depthwise

def tile_interior_adjoint(t_shape, dy, size, grid):
    """The adjoint of util_f16_ref.tile_interior: dy on the interiors, zeros on the halos (a copy: compared bit for bit)."""
    t = torch.zeros(t_shape, dtype=dy.dtype, requires_grad=True)
    return torch.autograd.grad(F16.tile_interior(t, size, grid), t, dy)[0]


def dw_tiles_case(gen, seed, b, c, size, grid):
    """{x, t (its halo tiles, image layout), bank (P, 9 C), dy}; 'range': gains per channel of x and dy, per patch and per tap of the bank."""
    g = G(2 * seed + (gen == 'range'))
    patches = b * grid[0] * grid[1]
    x, bank, dy = randn(g, b, c, *size), randn(g, patches, 9 * c) / 3.0, randn(g, b, c, *size)
    d = dict(size=size, grid=grid)
    if gen == 'range':
        gx, gy, gp, gt = pow2_gains(g, c, -6, 6), pow2_gains(g, c, -6, 6), pow2_gains(g, patches, -4, 4), pow2_gains(g, 9 * c, -6, 6)
        for t in (gx, gy, gt):
            t[0], t[-1] = 2.0 ** 6, 2.0 ** -6
        x, dy, bank = x * gx.view(1, -1, 1, 1), dy * gy.view(1, -1, 1, 1), bank * gp.view(-1, 1) * gt.view(1, -1)
        d['gains'] = dict(x=gx, dy=gy, patch=gp, tap=gt)
    d.update(x=x, bank=bank, dy=dy, t=F16.halo_tiles(x, grid))
    return d


def dw_tiles_ref(d):
    """{'y', 'dt', 'dw'}: V of util_f16_ref.dw_tiles_valid and its two adjoints (bilinear_with_grads), terms counted on ones."""
    fn = lambda t, bank: F16.dw_tiles_valid(t, bank, d['size'], d['grid'])                      # noqa: E731
    t, bank, dy = d['t'].double(), d['bank'].double(), d['dy'].double()
    val = F16.bilinear_with_grads(fn, t, bank, dy)
    cnt = F16.bilinear_with_grads(fn, torch.ones_like(t), torch.ones_like(bank), torch.ones_like(dy))
    return {k: dict(ref=val[s][0], mag=val[s][1], terms=cnt[s][0], bound=_counted_bound(cnt[s][0], val[s][1]))
            for k, s in (('y', 'y'), ('dt', 'da'), ('dw', 'db'))}


def dw_tiles_restate(d, dt=torch.float32):
    fn = lambda t, bank: F16.dw_tiles_valid(t, bank, d['size'], d['grid'])                      # noqa: E731
    r = F16.bilinear_with_grads(fn, d['t'].to(dt), d['bank'].to(dt), d['dy'].to(dt))
    return dict(y=r['y'][0], dt=r['da'][0], dw=r['db'][0])


# ------------------------------------------------------------------------------------------------------------ bilinear resize, adjoint

def upsample_adjoint(dy, in_size, dt=torch.float64, role='value'):
    """The adjoint of util_decoder_ref.upsample for the upstream dy (B, C, Ho, Wo) -> (B, C, Hi, Wi).  role 'abs': on |dy| (mag64);
    'count': the number of taps that reach each source pixel; 'taps': sum of |dy| over every output with the pixel among its four taps
    (weights taken as one)."""
    b, c = dy.shape[:2]
    g = dy.to(dt)
    if role != 'value':
        g = g.abs()
    if role == 'count':
        g = torch.ones_like(g)
    p = torch.zeros(b, c, *in_size, dtype=dt, requires_grad=True)
    if role in ('count', 'taps'):
        y0, y1, _, _ = D._taps(dy.shape[-2], in_size[0], dt)
        x0, x1, _, _ = D._taps(dy.shape[-1], in_size[1], dt)
        y = p[..., y0, :][..., x0] + p[..., y0, :][..., x1] + p[..., y1, :][..., x0] + p[..., y1, :][..., x1]
    else:
        y = D.upsample(p, tuple(dy.shape[-2:]), dt)
    return torch.autograd.grad(y, p, g)[0]


def upsample_adjoint_ref(dy, in_size):
    """dx[s] = sum over the outputs o that tap s of w(o, s) dy[o]: ``count`` products.  At the exact 2x ratio (and from a one-pixel source)
    the weights are exact.  At any other ratio each axis' weights are off by at most d = 2 * 2^-23 * in_size (util_decoder_ref's docstring:
    the rounding of scale, of src and of 1 - l1), and a changed floor moves a tap by one source pixel while its weight is within d of 0 or
    1: every output within one source pixel of s may contribute up to (dy + dx) |dy[o]| more or less -- the 3 x 3 box sum of 'taps'."""
    import torch.nn.functional as F
    out = tuple(dy.shape[-2:])
    mag, cnt = upsample_adjoint(dy, in_size, role='abs'), upsample_adjoint(dy, in_size, role='count')
    bound = _counted_bound(cnt, mag)
    ey = 0.0 if out[0] in (in_size[0], 2 * in_size[0]) or in_size[0] == 1 else 2 * U32 * in_size[0]
    ex = 0.0 if out[1] in (in_size[1], 2 * in_size[1]) or in_size[1] == 1 else 2 * U32 * in_size[1]
    if ey or ex:
        taps = upsample_adjoint(dy, in_size, role='taps')
        box = F.avg_pool2d(taps.flatten(0, 1).unsqueeze(1), 3, 1, 1, divisor_override=1).view(taps.shape)
        bound = bound + (ey + ex) * box
    return dict(ref=upsample_adjoint(dy, in_size), mag=mag, terms=cnt, bound=bound)


# ------------------------------------------------------------------------------------------------------------ meta_conv, adjoints

def meta_conv_grads(d, dy, dt=torch.float64, role='value'):
    """(dx, dw) of util_decoder_ref.meta_conv (no epilogue) on case ``d`` for the upstream dy; roles as patch_conv_grads."""
    rows = d['c_out'] * (d['x'].shape[1] // d['groups']) * d['k'][0] * d['k'][1]
    x, w, g = d['x'].to(dt), d['w'][:, :rows].to(dt), dy.to(dt)
    if role == 'abs':
        x, w, g = x.abs(), w.abs(), g.abs()
    elif role == 'count':
        x, w, g = torch.ones_like(x), torch.ones_like(w), torch.ones_like(g)
    x, w = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    dd = {k: v for k, v in d.items() if k not in ('scale', 'shift', 'act')}
    y = D.meta_conv(dict(dd, x=x, w=w), dt)
    return torch.autograd.grad(y, (x, w), g)


def meta_conv_bwd_ref(d, dy):
    ref, mag, cnt = (meta_conv_grads(d, dy, role=r) for r in ('value', 'abs', 'count'))
    return {k: dict(ref=ref[i], mag=mag[i], terms=cnt[i], bound=_counted_bound(cnt[i], mag[i])) for i, k in enumerate(('dx', 'dw'))}


# ------------------------------------------------------------------------------------------------------------ cross entropy

def ce_case(gen, seed, b, c, size, ignore_index=255, weighted=False):
    """{logits, target (some pixels ignored), g (the upstream of the per-pixel loss), weight | None}; 'range': per-class logit gains 2^-3 ..
    2^4 (soft-max from flat to saturated) and per-image-row upstream gains."""
    g = G(2 * seed + (gen == 'range'))
    logits, up = randn(g, b, c, *size) * 2.0, randn(g, b, *size)
    target = torch.randint(0, c, (b,) + tuple(size), generator=g)
    target[torch.rand(b, *size, generator=g) < 0.2] = ignore_index
    target[0, 0, 0], target[-1, -1, -1] = ignore_index, c - 1
    if gen == 'range':
        logits = logits * pow2_gains(g, c, -3, 4).view(1, -1, 1, 1)
        up = up * pow2_gains(g, size[0], -10, 10).view(1, -1, 1)
    return dict(logits=logits, target=target, g=up, ignore_index=ignore_index, weight=0.25 + 2.0 * torch.rand(c, generator=g) if weighted else None)


def ce_restate(d, dt=torch.float32):
    """(loss, dlogits): F.cross_entropy(reduction='none', weight=...) -- util_f16_ref.pixel_ce times weight[target] -- and its adjoint."""
    x = d['logits'].to(dt).clone().requires_grad_(True)
    loss = F16.pixel_ce(x, d['target'], d['ignore_index'])
    if d['weight'] is not None:
        live = d['target'] != d['ignore_index']
        loss = loss * torch.where(live, d['weight'].to(dt)[d['target'].clamp(0, x.shape[1] - 1)], torch.zeros((), dtype=dt))
    return loss.detach(), torch.autograd.grad(loss, x, d['g'].to(dt))[0]


def ce_ref(d):
    """{'loss', 'dl'} for the kernel's order (hs_train_aux.hip cross_entropy_kernel): m = max (exact), a_c = x_c - m (one rounding, relative
    on |a_c|), s = sum expf(a_c), loss = w ((logf(s) + m) - x_t); d x_c = (expf(a_c) (1 / s) - [c = t]) (w g).  With util_confidence_ref's
    stated allowances -- expf and logf within E = 2 ulp, the division within DIV, a plain rounding within U (allowed 2^-23 here, the factor
    two of sum_bound) -- and |a| e^a <= 1 / e, s >= 1:
      rel s  <= E + C U / e + (C + 2) 2^-23                      (expf, its argument's rounding, the fp32 sum of C positive terms)
      |d log s| <= rel s + E |log s|;  the two adds round on |log s + m| and on |loss|;  the weight multiplies once more
      rel p_c <= E + |a_c| U + rel s + DIV + 2^-23               (p_c = expf(a_c) (1 / s)); p - [c = t] and the product with w g round once each,
                                                                 w g itself once.  A p_c below 2^-126 may be flushed: TINY, absolute."""
    from util_confidence_ref import DIV, E, TINY, U
    x, t, ii = d['logits'].double(), d['target'], d['ignore_index']
    c = x.shape[1]
    live = t != ii
    tc = t.clamp(0, c - 1)
    w = torch.where(live, d['weight'].double()[tc] if d['weight'] is not None else torch.ones((), dtype=torch.float64), torch.zeros((), dtype=torch.float64))
    loss, dl = ce_restate(d, torch.float64)
    m = x.amax(1)
    a = x - m.unsqueeze(1)
    s = a.exp().sum(1)
    xt = x.gather(1, tc.unsqueeze(1)).squeeze(1)
    rel_s = E + c * U / 2.718281828 + (c + 2) * U32
    lmag = s.log() + m.abs() + xt.abs()
    lb = w * (rel_s + E * s.log() + U32 * ((s.log() + m).abs() + lmag)) + U32 * loss.abs() * (d['weight'] is not None)
    p = a.exp() / s.unsqueeze(1)
    hot = torch.zeros_like(x).scatter_(1, tc.unsqueeze(1), 1.0)
    gl = (w * d['g'].double()).abs().unsqueeze(1)
    rel_p = E + a.abs() * U + rel_s + DIV + U32
    db = gl * (rel_p * p + U32 * (p - hot).abs() + TINY) + 2 * U32 * dl.abs() + TINY       # TINY: expf's and the store's underflow, flushed or not
    return dict(loss=dict(ref=loss, bound=lb + 1e-300, mag=w * lmag), dl=dict(ref=dl, bound=db + 1e-300, mag=gl * (p + hot)))


# ------------------------------------------------------------------------------------------------------------ bootstrapped mean / loss

def bootstrap_mean_tied(values, k, thresh, defect=None):
    """util_f16_ref.bootstrapped_mean's VALUE (test_bootstrap_statement_equals_the_sorted_one) written so that autograd gives the
    gradient the kernels give where values tie: per image, if the (k+1)-th largest exceeds ``thresh`` the mean of the values strictly
    above it (a value equal to the threshold is not kept); else the k largest, the values equal to the k-th sharing the places left
    among them evenly (weight (k - #above) / #equal each; a sort hands them to whichever it ranked first).  'bootstrap_tie_takes_all':
    every tied value counted whole."""
    total = 0.0
    for v in values:
        ranked = v.detach().sort(descending=True).values
        if ranked[k] > thresh:
            total = total + v[v.detach() > thresh].mean()
        else:
            cut = ranked[k - 1]
            above, eq = v.detach() > cut, v.detach() == cut
            tie = 1.0 if defect == 'bootstrap_tie_takes_all' else (k - int(above.sum())) / int(eq.sum())
            total = total + (v[above].sum() + tie * v[eq].sum()) / k
    return total / values.shape[0]


def bootstrap_mean_ref(values, k, thresh, up=1.0):
    """{'loss', 'dv'}: the mean sums count <= n values per image and N images, is divided twice: terms = count + N + 2, counted as the
    number of kept values.  A kept value's gradient is up (1 / count) (1 / N) tie: four roundings on itself."""
    v = values.double().clone().requires_grad_(True)
    loss = bootstrap_mean_tied(v, k, thresh)
    dv, = torch.autograd.grad(loss, v, torch.tensor(up, dtype=torch.float64))
    kept = int((dv != 0).sum())
    mag = (dv.abs() * values.double().abs()).sum() / abs(up)
    return dict(loss=dict(ref=loss.detach(), mag=mag, bound=sum_bound(kept + values.shape[0] + 2, mag) + 1e-300),
                dv=dict(ref=dv, mag=dv.abs(), bound=sum_bound(4, dv.abs()) + 1e-300))


def bootstrapped_ce_ref(d, k, thresh, up=1.0):
    """util_f16_ref.bootstrapped_ce on a cross-entropy case and its adjoint.  The per-pixel losses carry ce_ref's bound e; the selection
    is a step function of them, so the case must keep it DECIDED: ``decided`` is False where some live loss lies within its e of the
    threshold or of the k-th / (k+1)-th ranked loss' gap (the test asserts it: the generator, not the kernel, is at fault otherwise).
    Then the kept set is the reference's; loss: the kept pixels' e through their weights + the mean's own (kept + N + 2) 2^-23 mag;
    d logits: ce_ref's bound with the pixel's weight as its upstream + four roundings of that weight."""
    x = d['logits'].double().clone().requires_grad_(True)
    per = F16.pixel_ce(x, d['target'], d['ignore_index'])
    if d['weight'] is not None:
        per = per * d['weight'].double()[d['target'].clamp(0, x.shape[1] - 1)] * (d['target'] != d['ignore_index'])
    per.retain_grad()
    loss = F16.bootstrapped_mean(per, k, thresh)
    (loss * up).backward()
    wmap = per.grad.detach()                                        # up * each pixel's share of the batch mean (0: not kept)
    V = ce_ref(dict(d, g=wmap.float()))                             # (shares are ratios of small integers times up: fp32 carries them to 2^-24)
    e, pd = V['loss']['bound'], per.detach()
    decided = True
    for img, eb in zip(pd.flatten(1), e.flatten(1)):
        ranked = img.sort(descending=True).values
        if ranked[k] > thresh:
            decided &= not bool(((img - thresh).abs() <= eb).any())
        else:
            lo, hi = ranked[k], ranked[k - 1]
            decided &= bool(hi - lo > 2 * eb.max()) and not bool((ranked[k] - thresh).abs() <= eb.max())
    kept = int((wmap != 0).sum())
    mag = (wmap.abs() * V['loss']['mag']).sum() / abs(up)
    lb = (wmap.abs() * e).sum() / abs(up) + sum_bound(kept + x.shape[0] + 2, mag)
    dl = dict(ref=x.grad.detach(), mag=V['dl']['mag'], bound=V['dl']['bound'] + sum_bound(4, x.grad.detach().abs()))
    return dict(loss=dict(ref=loss.detach(), mag=mag, bound=lb), dl=dl, decided=decided)


# ------------------------------------------------------------------------------------------------------------ signal2weights, training

def s2w_case(gen, seed, b, c, grid, layers):
    """{signal (B, C, fh, fw), layers: [{wsw (wc, K), index, channels, groups, rows, dbank (P, rows)}]}; 'range': gains per signal channel,
    per generated row and per upstream column."""
    g = G(2 * seed + (gen == 'range'))
    p = b * grid[0] * grid[1]
    sig = randn(g, b, c, *grid)
    if gen == 'range':
        sig = sig * pow2_gains(g, c, -8, 8).view(1, -1, 1, 1)
    out = []
    for index, channels, groups, wc, rows in layers:
        kk = channels // groups
        w, db = randn(g, wc, kk) * kk ** -0.5, randn(g, p, rows)
        if gen == 'range':
            w, db = w * pow2_gains(g, wc, -8, 8).view(-1, 1), db * pow2_gains(g, rows, -8, 8).view(1, -1)
        out.append(dict(wsw=w, index=index, channels=channels, groups=groups, rows=rows, dbank=db))
    return dict(signal=sig, layers=out)


def s2w_train(d, dt=torch.float64, role='value', defect=None):
    """(banks, dsignal, dws) of util_decoder_ref.s2w_bank over the layer list, by autograd; roles as patch_conv_grads.
    's2w_group_offset_from_group_0': every group's rows generated from group 0's signal slice."""
    f = (lambda t: t.to(dt)) if role == 'value' else (lambda t: t.to(dt).abs()) if role == 'abs' else (lambda t: torch.ones_like(t, dtype=dt))
    sig = f(d['signal']).clone().requires_grad_(True)
    ws = [f(l['wsw']).clone().requires_grad_(True) for l in d['layers']]
    banks = []
    for l, w in zip(d['layers'], ws):
        s_in = sig
        if defect == 's2w_group_offset_from_group_0' and l['groups'] > 1:
            kk = l['channels'] // l['groups']
            s_in = torch.cat([sig[:, :l['index']]] + [sig[:, l['index']:l['index'] + kk]] * l['groups'] + [sig[:, l['index'] + l['channels']:]], 1)
        banks.append(D.s2w_bank(s_in, w, l['index'], l['channels'], l['groups'], l['rows'], dt))
    grads = torch.autograd.grad(banks, [sig] + ws, [f(l['dbank']) for l in d['layers']])
    return [b.detach() for b in banks], grads[0], list(grads[1:])


def s2w_train_ref(d):
    """{'banks': [V], 'ds': V, 'dws': [V]}: K = channels / groups products per bank element, the rows of every layer that read a signal
    channel per dsignal element, B fh fw per weight-gradient element -- all counted on ones."""
    ref, mag, cnt = (s2w_train(d, role=r) for r in ('value', 'abs', 'count'))
    one = lambda i, j=None: (lambda pick: dict(ref=pick(ref), mag=pick(mag), terms=pick(cnt), bound=_counted_bound(pick(cnt), pick(mag))))(   # noqa: E731
        (lambda t: t[i]) if j is None else (lambda t: t[i][j]))
    n = len(d['layers'])
    return dict(banks=[one(0, j) for j in range(n)], ds=one(1), dws=[one(2, j) for j in range(n)])


# ------------------------------------------------------------------------------------------------------------ stage input, adjoint

def stage_adjoint_ref(skip, prev, coords, r):
    """The adjoint of util_f16_ref.stage_input for the upstream r: (d skip -- r's channel range, a copy --, V of d prev): the bilinear
    adjoint of r's last channels, upsample_adjoint_ref's bound (exact weights at 2x, the tap allowance elsewhere)."""
    s64 = skip.double().clone().requires_grad_(True)
    p64 = prev.double().clone().requires_grad_(True)
    y = F16.stage_input(s64, p64, coords)
    ds, dp = torch.autograd.grad(y, (s64, p64), r.double())
    off = (2 if coords else 0) + skip.shape[1]
    V = upsample_adjoint_ref(r[:, off:], tuple(prev.shape[-2:])) if prev.shape[-2:] != skip.shape[-2:] else dict(ref=dp, mag=dp.abs(), bound=torch.zeros_like(dp))
    assert float((V['ref'] - dp).abs().max()) <= 1e-12 * float(V['mag'].max() + 1e-300)        # the two statements of the resize agree
    return ds, dict(V, ref=dp)


# ------------------------------------------------------------------------------------------------------------ BatchNorm + ReLU6 + a linear layer

def bn_linear_case(gen, seed, shape, bank_shape, r_shape):
    """{x, w, b, bank, r}: the operands of util_f16_ref.bn_linear_ref (fp32 storage: half=False); 'range': per-channel gains of x and r."""
    g = G(2 * seed + (gen == 'range'))
    c = shape[1]
    x, r = randn(g, *shape) * 1.5 + 0.4, randn(g, *r_shape)
    bank = randn(g, *bank_shape) * 0.4
    if gen == 'range':
        x = x * pow2_gains(g, c, -6, 6).view(1, -1, 1, 1)
        r = r * pow2_gains(g, r_shape[1], -6, 6).view(1, -1, 1, 1)
    return dict(x=x, w=0.5 + torch.rand(c, generator=g), b=1.5 + 0.5 * randn(g, c), bank=bank, r=r)


def bn_linear_V(d, linear, terms):
    """bn_linear_ref(half=False) as V dicts: bound = (terms + 2) 2^-23 mag64 + extra64 per result."""
    ref = F16.bn_linear_ref(d['x'].double(), d['w'].double(), d['b'].double(), d['bank'].double(), d['r'].double(), linear, terms, half=False)
    out = {}
    for k, (val, mag, extra, n) in ref.items():
        bound = sum_bound(n, mag) + (extra if extra is not None else 0.0)
        out[k] = dict(ref=val, mag=mag.expand_as(val), bound=bound.expand_as(val) + 1e-300)
    return out


# ------------------------------------------------------------------------------------------------------------ defects

@functools.lru_cache(maxsize=None)
def _defect_conv_case(name):
    if name == 'reflect_corner_off_by_one':
        return patch_conv_case('benign', 11, 1, 3, (6, 10), (2, 2), 4, 3, 'reflect', 1)
    if name == 'group_offset_from_group_0':
        return patch_conv_case('benign', 12, 1, 4, (6, 10), (2, 2), 6, 3, 'zeros', 2)
    return patch_conv_case('benign', 13, 1, 20, (6, 14), (2, 2), 24, 1, 'zeros', 1)       # 3 x 7 patches: 21 pixels, one full chunk and 5 more


def defective(name):
    """(got, V, clean): the fp32 restatement with defect ``name``, what it is checked against, and the same restatement without the defect."""
    f = torch.float32
    if name in ('chunk_tail_pixel_dropped', 'swapped_pair', 'reflect_corner_off_by_one', 'group_offset_from_group_0', 'dw_tile_last_row_dropped'):
        d = _defect_conv_case(name)
        i = 1 if name == 'dw_tile_last_row_dropped' else 0
        return patch_conv_grads(d, f, defect=name)[i], patch_conv_bwd_ref(d)['dw' if i else 'dx'], patch_conv_grads(d, f)[i]
    if name == 'halo_adjoint_without_corner':
        g = G(21)
        x, dt = randn(g, 1, 2, 6, 8), randn(g, 1, 2, 2 * 5, 2 * 6)
        return halo_adjoint(x, dt, (2, 2), defect=name), halo_adjoint_ref(x, dt, (2, 2)), halo_adjoint(x, dt, (2, 2))
    if name == 'dgamma_without_relu6_mask':
        d = bn_case('benign', 22, 2, 3, (5, 7))
        return bn_restate(d, 2, defect=name)['dg'], bn_ref(d, 2)['dg'], bn_restate(d, 2)['dg']
    if name == 'adam_without_bias_correction':
        g = G(23)
        p, grads = randn(g, 63), [randn(g, 63) for _ in range(3)]
        a = (1e-3, (0.5, 0.999), 1e-8)
        return adam_steps(p, grads, *a, dt=f, defect=name)[-1], adam_ref(p, grads, *a)[-1], adam_steps(p, grads, *a, dt=f)[-1]
    if name in ('ce_weight_of_next_class', 'ce_ignored_pixel_not_zeroed'):
        d = ce_case('range', 31, 2, 21, (5, 7), weighted=True)
        clean = ce_restate(d, f)[0]
        if name == 'ce_weight_of_next_class':
            bad = ce_restate(dict(d, weight=d['weight'].roll(1)), f)[0]
        else:
            bad = clean.clone()
            bad[d['target'] == d['ignore_index']] = ce_restate(dict(d, target=d['target'].clamp(max=20)), f)[0][d['target'] == d['ignore_index']]
        return bad, ce_ref(d)['loss'], clean
    if name == 'upsample_tap_off_by_one':                           # the last output row gathers into the source row above its own
        dy = randn(G(32), 1, 2, 13, 9)
        clean = upsample_adjoint(dy, (5, 7), f)
        bad = clean.clone()
        last = torch.zeros_like(dy)
        last[..., -1, :] = dy[..., -1, :]
        part = upsample_adjoint(last, (5, 7), f)
        bad = bad - part + torch.cat([part[..., 1:, :], torch.zeros_like(part[..., :1, :])], -2)
        return bad, upsample_adjoint_ref(dy, (5, 7)), clean
    if name == 'meta_conv_last_tap_dropped':
        g = G(33)
        d = dict(x=randn(g, 1, 3, 7, 9), w=randn(g, 1, 4 * 27) / 5, c_out=4, k=(3, 3), stride=(1, 1), pad=(1, 1), dil=(1, 1), mode='zeros', groups=1)
        dy = randn(g, 1, 4, 7, 9)
        clean = meta_conv_grads(d, dy, f)[1]
        bad = clean.clone()
        bad.view(1, 4, 3, 9)[..., -1] = 0
        return bad, meta_conv_bwd_ref(d, dy)['dw'], clean
    if name == 'dw_tiles_neighbour_patch_taps':                     # the second patch filtered with the first patch's taps
        d = dw_tiles_case('range', 34, 1, 3, (4, 8), (1, 2))
        bank = d['bank'].clone()
        bank[1] = bank[0]
        return dw_tiles_restate(dict(d, bank=bank))['y'], dw_tiles_ref(d)['y'], dw_tiles_restate(d)['y']
    if name == 's2w_group_offset_from_group_0':
        d = s2w_case('range', 35, 1, 12, (1, 2), [(0, 12, 3, 9, 7)])
        return s2w_train(d, f, defect=name)[0][0], s2w_train_ref(d)['banks'][0], s2w_train(d, f)[0][0]
    if name == 'bootstrap_tie_takes_all':
        v = (randn(G(36), 2, 300).abs() * 4).round() / 4
        k, thresh = 50, 3.0

        def grad(defect):
            vv = v.clone().requires_grad_(True)
            return torch.autograd.grad(bootstrap_mean_tied(vv, k, thresh, defect), vv)[0]
        return grad(name), bootstrap_mean_ref(v, k, thresh)['dv'], grad(None)
    raise KeyError(name)
