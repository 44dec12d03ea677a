"""Host-only float64 statements of the operations the fp16-storage training kernels replace, and the elementwise bound they are held to.

Nothing here touches the GPU or imports the project: every statement is written with stock PyTorch ops (F.pad / unfold, F.conv2d,
bmm, F.batch_norm, F.relu6, F.interpolate, F.cross_entropy), takes float64 tensors, and is differentiated by float64 autograd.

The bound (``f16_bound`` / ``assert_within_f16``): a kernel that sums ``terms`` products in fp32 and stores the result once as binary16 is
within

    |got - ref64| <= 2^-11 |ref64| + 2^-24 + (terms + 2) 2^-23 mag64

of the float64 value: the fp32 sum of n products is within gamma_n <= (n + 2) 2^-23 (twice the first-order n 2^-24: any order of
summation, fused or unfused products) of ``mag64``, the same statement on absolute values; the one round-to-nearest to binary16 adds half
an ulp, at most 2^-11 |ref64| for normal results and 2^-24 (half the smallest subnormal) below.  fp32 outputs drop the first two terms.
``extra64`` is an ABSOLUTE allowance the caller derives the same way for errors that enter through an operand (the error bound of a
previous kernel's output pushed through this one on absolute values, or the terms whose ReLU6 unit is undecided within that bound) --
never a measured constant.

The 16-bit format is a parameter (``fmt``, a ``Format``; default BINARY16, so every call without it means what it always meant).  With
BFLOAT16 the same argument gives

    |got - ref64| <= 2^-8 |ref64| + 2^-126 + (terms + 2) 2^-23 mag64

bf16 keeps 8 significant bits: half an ulp is at most 2^-8 |ref64|.  It shares fp32's exponent range, so its absolute term has to cover
the low end of the fp32 ARITHMETIC as well as of the store: an fp32 result below the smallest normal 2^-126 is either flushed to zero
(error < 2^-126, and the zero is stored exactly) or kept as an fp32 subnormal (error 2^-150) and rounded to a bf16 subnormal (half of
2^-133: 2^-134); 2^-126, one smallest fp32 normal, covers both.  Round-to-nearest-even goes to infinity from the midpoint between the
largest bf16, 2^128 (1 - 2^-8), and 2^128: 2^128 (1 - 2^-9)."""
import collections

import torch
import torch.nn.functional as F

U16 = 2.0 ** -11          # half an ulp of binary16, relative
SUB16 = 2.0 ** -24        # half the smallest binary16 subnormal
U32 = 2.0 ** -23          # one fp32 ulp, relative: (terms + 2) U32 >= gamma_terms of an fp32 sum of products
F16_MAX = 65504.0
F16_INF_FROM = 65520.0    # round-to-nearest-even gives inf from here on

# A 16-bit storage format as the bound sees it: ``u`` the relative half-ulp, ``sub`` the absolute term, ``inf_from`` the magnitude from
# which round-to-nearest-even stores an infinity (derivations: the module docstring).
Format = collections.namedtuple('Format', 'name dtype u sub inf_from')
BINARY16 = Format('fp16', torch.float16, U16, SUB16, F16_INF_FROM)
BFLOAT16 = Format('bf16', torch.bfloat16, 2.0 ** -8, 2.0 ** -126, 2.0 ** 128 * (1 - 2.0 ** -9))


def f64(t):
    return t.detach().double().cpu()


def sum_bound(terms, mag64):
    """(terms + 2) 2^-23 mag64: the fp32 part of the bound (all of it for an fp32 output)."""
    return (float(terms) + 2.0) * U32 * mag64


def f16_bound(ref64, terms, mag64, half=True, fmt=BINARY16):
    e = sum_bound(terms, mag64)
    return e + fmt.u * ref64.abs() + fmt.sub if half else e


def assert_within_f16(got, ref64, terms, mag64, extra64=None, half=True, what='', fmt=BINARY16):
    """``got`` (any float type, any device) against the float64 ``ref64`` under the bound of this module's docstring.  NaN positions
    must match.  Where the bound reaches past the binary16 range (|ref64| + bound >= 65520) ``got`` may be the infinity of ref64's sign;
    where |ref64| - bound >= 65520 it must be; a finite ``got`` is always held to the bound itself (65504 for 65510 passes, as .half()
    gives it).  ``half=False``: an fp32 output (no binary16 terms, no overflow rule).  ``fmt``: the 16-bit format (its ``u``, ``sub`` and
    ``inf_from`` in place of binary16's).  Returns (worst err / bound, its index) of a tensor that passes, for reports."""
    got = f64(got)
    ref64 = ref64.detach().double()
    assert got.shape == ref64.shape, (what, tuple(got.shape), tuple(ref64.shape))

    def full(t):
        t = t.detach().double() if isinstance(t, torch.Tensor) else torch.tensor(float(t), dtype=torch.float64)
        return t.expand_as(ref64).nan_to_num(nan=0.0, posinf=0.0)
    nan = ref64.isnan()
    assert torch.equal(got.isnan(), nan), f'{what}: NaN positions differ ({int(got.isnan().sum())} got, {int(nan.sum())} expected)'
    rinf = ref64.isinf()
    assert torch.equal(got[rinf], ref64[rinf]), f'{what}: infinities of the reference differ'
    live = ~(nan | rinf)
    r = torch.where(live, ref64, torch.zeros_like(ref64))
    g = torch.where(live, got, torch.zeros_like(got))
    bound = f16_bound(r, terms, full(mag64), half, fmt)
    if extra64 is not None:
        bound = bound + full(extra64)
    ginf = g.isinf()
    if half:
        may = (r.abs() + bound >= fmt.inf_from) & (torch.sign(g) == torch.sign(r))
        must = r.abs() - bound >= fmt.inf_from
        assert bool((ginf <= may).all()), f'{what}: {int((ginf & ~may).sum())} infinities where the reference is finite in {fmt.name}'
        assert bool((must <= ginf).all()), f'{what}: {int((must & ~ginf).sum())} finite values where the reference overflows {fmt.name}'
    else:
        assert not bool(ginf.any()), f'{what}: infinite fp32 output'
    err = torch.where(ginf, torch.zeros_like(g), (g - r).abs())
    bad = err > bound
    ratio = torch.where(err > 0, err / bound.clamp(min=1e-300), torch.zeros_like(err))
    worst = int(torch.argmax(ratio)) if ratio.numel() else 0
    if bool(bad.any()):
        idx = [tuple(int(v) for v in i) for i in torch.nonzero(bad)[:8]]
        raise AssertionError(f'{what}: {int(bad.sum())} of {ref64.numel()} elements outside the {fmt.name} bound; worst |err| {float(err.flatten()[worst]):.3e} '
                             f'vs bound {float(bound.flatten()[worst]):.3e} (ref {float(r.flatten()[worst]):.6g}, got {float(g.flatten()[worst]):.6g}); '
                             f'first indices {idx}')
    if not ratio.numel():
        return 0.0, ()
    index = []
    for size in reversed(ratio.shape):
        worst, at = divmod(worst, size)
        index.insert(0, at)
    return float(ratio.max()), tuple(index)


# ------------------------------------------------------------------------------------------------------------ tile re-layouts

def halo_tiles(x, grid, patch_major=False):
    """F.pad(reflect, 1) -> unfold -> unfold: the image of tiles (B, C, fh (ph+2), fw (pw+2)) or, patch-major, (B fh fw, C, ph+2, pw+2)."""
    b, c, h, w = x.shape
    fh, fw = grid
    ph, pw = h // fh, w // fw
    t = F.pad(x, (1, 1, 1, 1), mode='reflect').unfold(2, ph + 2, ph).unfold(3, pw + 2, pw)           # B C fh fw ph+2 pw+2
    if patch_major:
        return t.permute(0, 2, 3, 1, 4, 5).reshape(b * fh * fw, c, ph + 2, pw + 2)
    return t.permute(0, 1, 2, 4, 3, 5).reshape(b, c, fh * (ph + 2), fw * (pw + 2))


def to_patch_major(t, grid):
    """The image of tiles (or any image cut into fh x fw equal patches) -> one patch after the other, (B fh fw, C, th, tw)."""
    b, c, hh, ww = t.shape
    fh, fw = grid
    return t.reshape(b, c, fh, hh // fh, fw, ww // fw).permute(0, 2, 4, 1, 3, 5).reshape(b * fh * fw, c, hh // fh, ww // fw)


def from_patch_major(p, b, grid):
    """(B fh fw, C, th, tw) -> (B, C, fh th, fw tw)."""
    fh, fw = grid
    _, c, th, tw = p.shape
    return p.reshape(b, fh, fw, c, th, tw).permute(0, 3, 1, 4, 2, 5).reshape(b, c, fh * th, fw * tw)


def tile_interior(t, size, grid):
    b, c = t.shape[:2]
    (h, w), (fh, fw) = size, grid
    ph, pw = h // fh, w // fw
    return t.reshape(b, c, fh, ph + 2, fw, pw + 2)[:, :, :, 1:-1, :, 1:-1].reshape(b, c, h, w)


# ------------------------------------------------------------------------------------------------------------ per-patch convolutions

def dw_tiles_valid(t, bank, size, grid, patch_major=False):
    """The valid depthwise 3x3 of every halo tile with its patch's taps (bank (B fh fw, 9 C), tap [c*9 + ky*3 + kx]): F.conv2d, padding 0,
    groups = B * patches * C -> (B, C, H, W)."""
    (h, w), (fh, fw) = size, grid
    ph, pw = h // fh, w // fw
    tiles = t if patch_major else to_patch_major(t, grid)
    p, c = tiles.shape[:2]
    y = F.conv2d(tiles.reshape(1, p * c, ph + 2, pw + 2), bank.reshape(p * c, 1, 3, 3), padding=0, groups=p * c)
    return from_patch_major(y.reshape(p, c, ph, pw), p // (fh * fw), grid)


def patch_dw3(x, bank, grid):
    """The depthwise 3x3 of x (B, C, H, W), zero-padded as a WHOLE image, every patch filtered with its own taps (bank (B fh fw, 9 C)): a
    patch's border outputs read the neighbouring patch's pixels.  F.pad(zeros) -> unfold -> unfold -> the valid convolution per tile."""
    b, c, h, w = x.shape
    fh, fw = grid
    ph, pw = h // fh, w // fw
    t = F.pad(x, (1, 1, 1, 1)).unfold(2, ph + 2, ph).unfold(3, pw + 2, pw).permute(0, 2, 3, 1, 4, 5).reshape(b * fh * fw, c, ph + 2, pw + 2)
    return dw_tiles_valid(t, bank, (h, w), grid, True)


def patch_k1(x, bank, grid, c_out):
    """The per-patch 1x1 convolution as a batched matmul: bank (B fh fw, c_out C), W[o, c] = bank[p, o*C + c]."""
    b, c = x.shape[:2]
    patches = to_patch_major(x, grid)
    p, _, ph, pw = patches.shape
    y = torch.bmm(bank.reshape(p, c_out, c), patches.reshape(p, c, ph * pw))
    return from_patch_major(y.reshape(p, c_out, ph, pw), b, grid)


def bank_of(wt, hp):
    """The reference-layout weights (B, >= hp, fh, fw) -> the bank (B fh fw, hp)."""
    return wt[:, :hp].permute(0, 2, 3, 1).reshape(-1, hp)


def bilinear_with_grads(fn, a, b_, r):
    """y = fn(a, b_) for a statement that is linear in each operand, its gradients for the upstream ``r``, and the same three on absolute
    values (the bound's ``mag64``): dict of (ref64, mag64) for 'y', 'da', 'db'."""
    out = {}
    for key, (aa, bb, rr) in (('ref', (a, b_, r)), ('mag', (a.abs(), b_.abs(), r.abs()))):
        aa, bb = aa.detach().clone().requires_grad_(True), bb.detach().clone().requires_grad_(True)
        y = fn(aa, bb)
        ga, gb = torch.autograd.grad(y, (aa, bb), rr)
        out[key] = (y.detach(), ga, gb)
    return {k: (out['ref'][i], out['mag'][i]) for i, k in enumerate(('y', 'da', 'db'))}


# ------------------------------------------------------------------------------------------------------------ BatchNorm + ReLU6

def _act_arg(relu6, act):
    """``act`` = 'none' | 'relu' | 'relu6' names the activation where given; ``relu6`` (True / False, and 'relu') is the older spelling."""
    return relu6 if act is None else {'none': False, 'relu': 'relu', 'relu6': True}[act]


def bn_relu6(x, weight, bias, eps=1e-5, relu6=True, act=None):
    """Train-mode batch_norm (batch statistics, biased variance) + relu6 (``relu6`` = 'relu': + relu; False: nothing)."""
    relu6 = _act_arg(relu6, act)
    y = F.batch_norm(x, None, None, weight, bias, True, 0.0, eps)
    return F.relu(y) if relu6 == 'relu' else F.relu6(y) if relu6 else y


def bn_train_ref(x, weight, bias, r, eps=1e-5, relu6=True, momentum=0.1, rm0=None, rv0=None, r_err=None, act=None):
    """The float64 values of train-mode batch_norm (+ relu6) over dim 1 of ``x`` and of its adjoint for the upstream ``r``, each with the
    bound's mag64 and, where needed, an absolute ``extra`` -- derived for the algorithm the kernels document (hs_train_aux.hip): sums over
    the n elements of a channel taken about the channel's first element c, d = x - c; mean = c + E[d], var = E[d^2] - E[d]^2;
    z = w (x - mean) invstd + b; backward g = r [0 < z < 6], db = sum g, dg = sum g xh, dx = w invstd (g - db/n - xh dg/n).

    With E = (n + 2) 2^-23 (``terms`` = n in assert_within_f16) first-order propagation gives
      |d mean| <= E Mm,  Mm = E|d|;   |d var| <= E Mv,  Mv = E[d^2] + E[d]^2 + 2 |E[d]| E|d|;   |d invstd| / invstd <= E (1 + Mv / (2 (var + eps)))
      (the 1: rsqrt, the eps add and the products that follow), so with K = 1 + Mv / (2 (var + eps))
      |d xh| <= E X,   X = invstd Mm + |xh| K;       mag z = |w| (X + invstd (|x| + |mean|)) + |b|
      mag db = sum |g|;   mag dg = sum |g| (|xh| + X);   mag dx = |w| invstd (|g| + mag db / n + |xh| mag dg / n + X |dg| / n) + |dx| K.
    ReLU6's unit is undecided where z lies within E mag z of 0 or 6 (set A): such an element may contribute its term or not, so
      extra db = sum_A |r|,  extra dg = sum_A |r xh|,  extra dx = |w| invstd ([A] |r| + extra db / n + |xh| extra dg / n).
    ``r_err``: an absolute bound on the error of the upstream gradient the kernel sees (it is another kernel's fp16 output); it enters
    the extras exactly like A's terms, with |r| replaced by r_err over all elements.
    Returns {name: (ref64, mag64, extra64)} for y, dx, dg, db, mean, var, rm, rv and 'z_mag' (the pre-activation's mag64), 'n'."""
    relu6 = _act_arg(relu6, act)
    c = x.shape[1]
    dims = [i for i in range(x.dim()) if i != 1]
    shp = [1, c] + [1] * (x.dim() - 2)
    n = x.numel() // c
    xa, wa, ba = x.detach().clone().requires_grad_(True), weight.detach().clone().requires_grad_(True), bias.detach().clone().requires_grad_(True)
    y = bn_relu6(xa, wa, ba, eps, relu6)
    dx, dg, db = torch.autograd.grad(y, (xa, wa, ba), r)
    E = (n + 2.0) * U32
    first = x.movedim(1, 0).reshape(c, -1)[:, 0].view(shp)
    d = x - first
    md, mabs, mq = d.mean(dims, keepdim=True), d.abs().mean(dims, keepdim=True), (d * d).mean(dims, keepdim=True)
    mean, var = first + md, (mq - md * md).clamp(min=0)
    invstd = (var + eps).rsqrt()
    Mm, Mv = mabs, mq + md * md + 2 * md.abs() * mabs
    K = 1 + Mv / (2 * (var + eps))
    xh = (x - mean) * invstd
    w_, b_ = weight.view(shp), bias.view(shp)
    X = invstd * Mm + xh.abs() * K
    z = w_ * xh + b_
    z_mag = w_.abs() * (X + invstd * (x.abs() + mean.abs())) + b_.abs()
    if relu6 == 'relu':                             # one threshold: the unit is undecided within E mag z of 0 only
        amb, mask = z.abs() <= E * z_mag, (z > 0).double()
    else:
        amb = ((z.abs() <= E * z_mag) | ((z - 6).abs() <= E * z_mag)) if relu6 else torch.zeros_like(z, dtype=torch.bool)
        mask = ((z > 0) & (z < 6)).double() if relu6 else torch.ones_like(z)
    g = r * mask
    loose = r.abs() * amb + (r_err if r_err is not None else 0.0) * torch.ones_like(r)
    xdb, xdg = loose.sum(dims, keepdim=True), (loose * xh.abs()).sum(dims, keepdim=True)
    mdb, mdg = g.abs().sum(dims, keepdim=True), (g.abs() * (xh.abs() + X)).sum(dims, keepdim=True)
    k0 = w_.abs() * invstd
    dx_mag = k0 * (g.abs() + mdb / n + xh.abs() * mdg / n + X * dg.view(shp).abs() / n) + dx.abs() * K
    dx_extra = k0 * (loose + xdb / n + xh.abs() * xdg / n)
    unb = var * (n / max(n - 1.0, 1.0))
    rm0 = torch.zeros(c, dtype=torch.float64) if rm0 is None else rm0
    rv0 = torch.ones(c, dtype=torch.float64) if rv0 is None else rv0
    flat = lambda t: t.reshape(c)                   # noqa: E731
    zero = torch.zeros(c, dtype=torch.float64)
    return dict(y=(y.detach(), z_mag, None), dx=(dx, dx_mag, dx_extra), dg=(dg, flat(mdg), flat(xdg)), db=(db, flat(mdb), flat(xdb)),
                mean=(flat(mean), flat(Mm + first.abs()), zero), var=(flat(var), flat(Mv), zero),
                rm=((1 - momentum) * rm0 + momentum * flat(mean), (1 - momentum) * rm0.abs() + momentum * flat(Mm + first.abs()), zero),
                rv=((1 - momentum) * rv0 + momentum * flat(unb), (1 - momentum) * rv0.abs() + momentum * flat(Mv) * (n / max(n - 1.0, 1.0)), zero),
                z_mag=z_mag, n=n, E=E)


# ------------------------------------------------------------------------------------------------------------ stage input

def stage_input(skip, prev, coords=True):
    """cat(linspace coordinates (x then y, -1 .. 1), skip, interpolate(prev, bilinear, align_corners=False))."""
    b, _, h, w = skip.shape
    parts = []
    if coords:
        cx = torch.linspace(-1, 1, steps=w, dtype=torch.float64)
        cy = torch.linspace(-1, 1, steps=h, dtype=torch.float64)
        parts.append(torch.stack([cx.view(1, w).expand(h, w), cy.view(h, 1).expand(h, w)], 0).unsqueeze(0).expand(b, -1, -1, -1))
    parts.append(skip)
    if prev is not None:
        parts.append(prev if prev.shape[-2:] == skip.shape[-2:] else F.interpolate(prev, (h, w), mode='bilinear', align_corners=False))
    return torch.cat(parts, dim=1)


# ------------------------------------------------------------------------------------------------------------ loss

def pixel_ce(logits, target, ignore_index):
    return F.cross_entropy(logits, target, ignore_index=ignore_index, reduction='none')


def bootstrapped_mean(per_pixel, k, thresh):
    """Per image: the mean of the losses above ``thresh`` if the (k+1)-th largest is above it, else of the k largest; then the batch mean."""
    total = 0.0
    for v in per_pixel.flatten(1):
        ranked = v.sort(descending=True).values
        total = total + (ranked[ranked > thresh] if ranked[k] > thresh else ranked[:k]).mean()
    return total / per_pixel.shape[0]


def bootstrapped_ce(logits, target, ignore_index, k, thresh):
    return bootstrapped_mean(pixel_ce(logits, target, ignore_index), k, thresh)


def bootstrap_weight_slack(per_pixel, per_err, k, thresh, live=None):
    """How far a pixel's weight in its image's bootstrapped mean may differ from the float64 one because the selection is decided on
    the kernel's FP32 losses -- the loss's counterpart of ReLU6's undecided unit.  ``per_err``: the absolute bound of each fp32 loss.
    Set A: the pixels whose float64 loss lies within that bound of the selection's boundary.
      * threshold branch (the (k+1)-th largest loss is above ``thresh``: the mean of the losses above it): A = |loss - thresh| <= err;
        the count c of selected pixels lies in [lo, hi] = [c - |A selected|, c + |A not selected|]: a pixel of A may weigh 0 or up to
        1 / lo, any other selected pixel 1 / c' with c' in [lo, hi].
      * top-k branch (the mean of the k largest): the count is k; the boundary is [the (k+1)-th largest, the k-th largest] (its own error:
        the image's largest err); a pixel of A may weigh anything in [0, 1 / k] -- the kernels share the weight left at the boundary
        among the pixels that TIE there, and losses below fp32's resolution all tie at 0 with the ignored pixels (log1p(x) = 0 in fp32 for
        x < 2^-24: the confident pixels of a sharp image).  The window is as wide as the fp32 loss bound, not as those zeros: a pixel's
        own ``err`` plus the boundary pixel's (unknown which pixel: the image's largest), so live pixels with small but non-zero losses
        within that bound of the boundary are undecided too.
    ``live`` (bool, per pixel): pixels that are not ignored; an ignored pixel gets no slack -- its gradient is exactly 0 whatever its weight.
    binary16 hides the difference under its 2^-24 absolute term (such a pixel's gradient is ~1e-13); bf16, with fp32's exponent range, does
    not.  The branch itself must be decided by the data (raises otherwise).  Returns the slack per pixel, in the shape of ``per_pixel``."""
    out = torch.zeros(per_pixel.shape, dtype=per_pixel.dtype)
    for v, err, dev in zip(per_pixel.flatten(1), per_err.flatten(1), out.view(out.shape[0], -1)):
        order = v.sort(descending=True)
        ranked = order.values
        assert float((ranked[k] - thresh).abs()) > float(err[order.indices[k]]), 'the data leave the selection branch undecided'
        if ranked[k] > thresh:
            sel, amb = v > thresh, (v - thresh).abs() <= err
            c = int(sel.sum())
            lo, hi = c - int((amb & sel).sum()), c + int((amb & ~sel).sum())
            assert lo > 0
            dev.copy_(torch.where(amb, torch.full_like(v, 1.0 / lo), sel * max(1.0 / lo - 1.0 / c, 1.0 / c - 1.0 / hi)))
        else:
            e = err + err.max()
            dev.copy_(((v >= ranked[k] - e) & (v <= ranked[k - 1] + e)).to(v.dtype) / k)
    return out if live is None else out * live


# ------------------------------------------------------------------------------------------------------------ BatchNorm + ReLU6 + a linear layer

def round16(t, fmt=BINARY16):
    return t.to(fmt.dtype).double()


def bn_linear_ref(x, weight, bias, bank, r, linear, terms, eps=1e-5, round_copy=False, half=True, fmt=BINARY16):
    """y = linear(relu6(batch_norm(x)), bank) and its adjoint for the upstream ``r``, with the bound's mag64 / extra64 per result.
    ``linear(z, bank)`` is one of the per-patch statements above (linear in each operand); ``terms`` = (forward, input adjoint, bank
    adjoint) products per output.  ``round_copy``: the two-step route stores the normalised copy z as binary16 between its two kernels
    (BNActTrain's output), so the reference rounds z there too; the fused forms never store it and get the unrounded statement.
    Both routes store the linear layer's input gradient dz as binary16 before BatchNorm's adjoint reads it (hs_dw_tiles_bwd_in /
    hs_patch_conv_plain_bwd_in write the storage type): the reference rounds dz at that point.

    Error that enters through an operand is pushed through the next statement on absolute values:
      e_z  = E z_mag (ReLU6 is 1-Lipschitz), plus -- rounded copy -- |rn(a) - rn(b)| <= |a - b| + ulp/2(a) + ulp/2(b): 2 (2^-11 |z| + 2^-24);
      e_dz = (terms_in + 2) 2^-23 mag dz + 2 (2^-11 |dz| + 2^-24), likewise;
      y: extra = linear(e_z, |bank|);  dbank: extra = adjoint_bank(e_z, |r|);  dx, dg, db: bn_train_ref's ``r_err`` = e_dz.
    ``half=False``: fp32 storage -- z and dz are stored as computed, so nothing is rounded to binary16 and the 2^-11 / 2^-24 terms drop:
    e_z = E z_mag, e_dz = (terms_in + 2) 2^-23 mag dz + the share of e_z that dz's own operand carries (none: dz reads r and the bank)."""
    t_fwd, t_in, t_w = terms
    fwd = bn_train_ref(x, weight, bias, torch.zeros_like(x), eps, True)
    z = fwd['y'][0]
    e_z = fwd['E'] * fwd['z_mag']
    if round_copy and half:
        e_z = e_z * (1 + fmt.u) + 2 * (fmt.u * z.abs() + fmt.sub)
        z = round16(z, fmt)
    lin = bilinear_with_grads(linear, z, bank, r)
    za, ba = e_z.clone().requires_grad_(True), bank.abs().clone().requires_grad_(True)
    y_extra = linear(za, ba)
    w_extra = torch.autograd.grad(y_extra, ba, r.abs())[0]
    dz, dz_mag = lin['da']
    e_dz = sum_bound(t_in, dz_mag) + (2 * (fmt.u * dz.abs() + fmt.sub) if half else 0.0)
    bwd = bn_train_ref(x, weight, bias, round16(dz, fmt) if half else dz, eps, True, r_err=e_dz)
    out = dict(y=(lin['y'][0], lin['y'][1], y_extra.detach(), t_fwd), dbank=(lin['db'][0], lin['db'][1], w_extra, t_w))
    for k in ('dx', 'dg', 'db', 'rm', 'rv'):
        out[k] = bwd[k] + (bwd['n'],)
    return out
