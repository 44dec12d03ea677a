"""Host-only statements of the decoder's forward operations (hs_patch_conv*.hip, hs_patch_ir*.hip; stage input and bilinear resize of
hs_common.h / hs_upsample_taps.h): each operation is written ONCE, generic in the dtype, and used in three roles.

(a) ``ref64`` -- the statement in float64 on the fp32 inputs (drawn with ``G(seed)``: the reference sees exactly the numbers the kernel
    sees) -- and ``mag64``, the same statement on absolute values.

(b) A per-element bound with no measured constant, built on util_f16_ref.sum_bound and checked by assert_within_f16(half=False):

    Single layer.  acc = sum of n products in fp32 is within (n + 2) 2^-23 mag of the float64 sum (sum_bound: any order, fused or not).
    The BatchNorm affine v = scale * acc + shift adds a = 2 roundings (one where the kernel uses fmaf; the build has -ffp-contract=off, so
    the plain expression rounds twice), each at most 2^-24 of |scale| mag + |shift| =: mag_out.  ReLU / ReLU6 are 1-Lipschitz and exact.
    An operand error EX (absolute, per input element) arrives as |scale| (|W| . EX).  Together:
        |got - ref64| <= (n + 2 + a) 2^-23 mag_out + |scale| (|W| . EX),     a = 2.

    Inverted residual (Op C, Op D): pw1 -> BN1 -> ReLU6 -> depthwise 3x3 -> BN2 -> ReLU6 -> pw3 -> BN3 (+ x).  Each layer's bound is
    the single-layer bound with the previous layer's bound as its operand error: e1 from (cin, W1, EX of the stage); e2 = the
    depthwise's own term (n = 9) + |s2| (|K| applied to the neighbours' e1); e3 = pw3's own term (n = hidden) + |s3| (|W3| . e2).  ReLU6
    is 1-Lipschitz, so no unit is "undecided" in the forward pass.  The residual adds the stage value's own error and one rounding.

    Stage input (stage_pos / stage_value of hs_common.h).  Skip channels are copied: no error.  A coordinate is -1 + step * i (or
    1 - step * (n - 1 - i)) with step = 2 / (n - 1) rounded to fp32: three roundings of values of magnitude <= 2, the product <= 1: at
    most 3 * 2^-24 < 2^-22 absolute.  The previous level: src = scale * (dst + 0.5) - 0.5.  At the exact 2x pyramid scale = 0.5, src and
    both weights (0.25 / 0.75, or 0 / 1 at the border) are exact; the value is a sum of 4 products, sum_bound(4, bilinear(|prev|)).  At any
    other ratio scale, the product and the difference round: |d src| <= 3 * 2^-24 (|src| + 0.5) <= 3 * 2^-24 * in_size, the weight
    l1 = src - floor(src) inherits it and l0 = 1 - l1 adds 2^-24: each axis' weights are off by at most d = 2 * 2^-23 * in_size, and the
    bilinear value (continuous across a changed floor) moves by at most (dy + dx) * 2 max|4 taps|.  This is EX of the consumer.

    Split mode (hs_patch_irc.hip): split_bound's docstring below.

(c) The restatement in fp32 with torch on the CPU (``dt=torch.float32``), with a ``defect=`` argument (DEFECTS below): what the bound must
    admit un-defected and reject defected.

The module imports neither the project nor the GPU."""
import torch
import torch.nn.functional as F

from util_f16_ref import U32, assert_within_f16, sum_bound

ACT_NONE, ACT_RELU, ACT_RELU6 = 0, 1, 2
DEFECTS = ('drop_last_k', 'drop_last_k_last_row', 'halo_corner_off_by_one', 'ring_own_weights', 'bn_relu6_order', 'prev_half_pixel', 'ld_ignored')
COORD_ERR = 2.0 ** -22


def G(seed):
    g = torch.Generator()
    g.manual_seed(seed)
    return g


def randn(g, *shape):
    return torch.randn(*shape, generator=g, dtype=torch.float32)


def pow2_gains(g, n, lo, hi):
    """n gains 2^e, e uniform in [lo, hi]: exact in fp32, so a rescaled BatchNorm computes the same function."""
    return torch.pow(2.0, torch.randint(lo, hi + 1, (n,), generator=g).float())


# ------------------------------------------------------------------------------------------------------------ stage input

def _taps(out, inn, dt, half_pixel=False):
    scale = (torch.tensor(float(inn), dtype=dt) / torch.tensor(float(out), dtype=dt))
    d = torch.arange(out, dtype=dt)
    src = scale * d if half_pixel else scale * (d + 0.5) - 0.5
    src = src.clamp(min=0)
    i0 = src.floor().long().clamp(max=inn - 1)
    i1 = (i0 + 1).clamp(max=inn - 1)
    l1 = src - i0.to(dt)
    return i0, i1, 1.0 - l1, l1


def upsample(p, size, dt=None, defect=None):
    """F.interpolate(p, size, mode='bilinear', align_corners=False) in the kernels' operation order (top / bottom rows first)."""
    dt = dt or p.dtype
    p = p.to(dt)
    y0, y1, ly0, ly1 = _taps(size[0], p.shape[-2], dt, defect == 'prev_half_pixel')
    x0, x1, lx0, lx1 = _taps(size[1], p.shape[-1], dt, defect == 'prev_half_pixel')
    top, bot = p[..., y0, :], p[..., y1, :]
    top = lx0 * top[..., x0] + lx1 * top[..., x1]
    bot = lx0 * bot[..., x0] + lx1 * bot[..., x1]
    return ly0.view(-1, 1) * top + ly1.view(-1, 1) * bot


def upsample_err(p, size):
    """The absolute allowance of ``upsample`` in fp32 against float64 (module docstring)."""
    a = p.double().abs()
    e = sum_bound(4, upsample(a, size))
    hi, wi = p.shape[-2:]
    dy = 0.0 if size[0] in (hi, 2 * hi) else 2 * U32 * hi
    dx = 0.0 if size[1] in (wi, 2 * wi) else 2 * U32 * wi
    if dy or dx:
        y0, y1, _, _ = _taps(size[0], hi, torch.float64)
        x0, x1, _, _ = _taps(size[1], wi, torch.float64)
        # a changed floor moves a tap by one more source pixel: the maximum over the 3 x 3 source window
        m = F.max_pool2d(a.flatten(0, -3).unsqueeze(0), 3, 1, 1).squeeze(0).view(a.shape)
        tap = torch.maximum(torch.maximum(m[..., y0, :][..., x0], m[..., y0, :][..., x1]),
                            torch.maximum(m[..., y1, :][..., x0], m[..., y1, :][..., x1]))
        e = e + (dy + dx) * 2 * tap
    return e


def _linspace_pm1(n, dt):
    if n == 1:
        return torch.full((1,), -1.0, dtype=dt)
    step = torch.tensor(2.0, dtype=dt) / torch.tensor(float(n - 1), dtype=dt)
    i = torch.arange(n, dtype=dt)
    return torch.where(i < n // 2, -1.0 + step * i, 1.0 - step * (n - 1 - i))


def stage(skip, prev, coords, dt, role='value', defect=None):
    """cat(coords(2)?, skip, resize(prev)?) -- role 'value' | 'abs' (the statement on absolute values) | 'err' (the operand error EX)."""
    b, _, h, w = skip.shape
    parts = []
    if coords:
        cx, cy = _linspace_pm1(w, dt).view(1, w).expand(h, w), _linspace_pm1(h, dt).view(h, 1).expand(h, w)
        c = torch.stack([cx, cy]).unsqueeze(0).expand(b, 2, h, w)
        parts.append(torch.full_like(c, COORD_ERR) if role == 'err' else c.abs() if role == 'abs' else c)
    s = skip.to(dt)
    parts.append(torch.zeros_like(s) if role == 'err' else s.abs() if role == 'abs' else s)
    if prev is not None:
        if role == 'err':
            parts.append(upsample_err(prev, (h, w)) if prev.shape[-2:] != (h, w) else torch.zeros_like(prev, dtype=dt))
        else:
            p = prev.to(dt).abs() if role == 'abs' else prev.to(dt)
            parts.append(p if p.shape[-2:] == (h, w) else upsample(p, (h, w), dt, defect))
    return torch.cat(parts, dim=1)


# ------------------------------------------------------------------------------------------------------------ padding, tiles

def _index(n, pad, mode):
    i = torch.arange(-pad, n + pad)
    if mode == 'reflect':
        j = i.abs()
        return torch.where(j >= n, 2 * (n - 1) - j, j), None
    if mode == 'replicate':
        return i.clamp(0, n - 1), None
    if mode == 'circular':
        return i % n, None
    return i.clamp(0, n - 1), (i >= 0) & (i < n)


def pad2d(x, pad, mode, defect=None):
    """F.pad of the whole image by ``pad`` on every side as an index gather (hs_common.h pad_index)."""
    if pad == 0:
        return x
    h, w = x.shape[-2:]
    ys, vy = _index(h, pad, mode)
    xs, vx = _index(w, pad, mode)
    out = x[..., ys, :][..., xs]
    if vy is not None:
        out = out * (vy.view(-1, 1) & vx.view(1, -1)).to(x.dtype)
    if defect == 'halo_corner_off_by_one' and mode == 'reflect':     # the bottom-right halo corner reads (H-1, W-1) for (H-2, W-2)
        out = out.clone()
        out[..., -1, -1] = x[..., -1, -1]
    return out


def halo_tiles(xp, grid, pad, ph, pw):
    """padded (B, C, H + 2 pad, W + 2 pad) -> (B, C, fh, fw, ph + 2 pad, pw + 2 pad)."""
    fh, fw = grid
    ys = torch.arange(fh).view(fh, 1) * ph + torch.arange(ph + 2 * pad).view(1, -1)
    xs = torch.arange(fw).view(fw, 1) * pw + torch.arange(pw + 2 * pad).view(1, -1)
    return xp[:, :, ys, :][:, :, :, :, xs].permute(0, 1, 2, 4, 3, 5)


def bank_rows(bank, rows, dt, defect=None):
    """The first ``rows`` floats of every patch's bank row (row stride ld = bank.shape[1]); 'ld_ignored': rows read back to back."""
    if defect == 'ld_ignored':
        return bank.reshape(-1)[:bank.shape[0] * rows].view(bank.shape[0], rows).to(dt)
    return bank[:, :rows].to(dt)


# ------------------------------------------------------------------------------------------------------------ Op A / Op B

def conv_core(x, wrows, grid, c_out, k, mode, groups, defect=None):
    """sum_{c, ky, kx} W[p][((o cin_g + c) k + ky) k + kx] xpad[grp(o) cin_g + c, y + ky - pad, x + kx - pad] with p the pixel's patch."""
    b, cin, h, w = x.shape
    fh, fw = grid
    ph, pw, pad = h // fh, w // fw, (k - 1) // 2
    cin_g, cout_g = cin // groups, c_out // groups
    wv = wrows.reshape(b, fh, fw, groups, cout_g, cin_g, k, k)
    if defect == 'drop_last_k':
        wv = wv.clone()
        wv[..., -1, -1, -1] = 0
    if defect == 'drop_last_k_last_row':                  # a ragged tail of the LAST output row only
        wv = wv.clone()
        wv[:, :, :, -1, -1, -1, -1, -1] = 0
    t = halo_tiles(pad2d(x, pad, mode, defect), grid, pad, ph, pw).reshape(b, groups, cin_g, fh, fw, ph + 2 * pad, pw + 2 * pad)
    y = x.new_zeros(b, groups, cout_g, fh, fw, ph, pw)
    for ky in range(k):
        for kx in range(k):
            y = y + torch.einsum('bijgoc,bgcijuv->bgoijuv', wv[..., ky, kx], t[..., ky:ky + ph, kx:kx + pw])
    return y.permute(0, 1, 2, 3, 5, 4, 6).reshape(b, c_out, h, w)


def _act(v, act):
    return v.clamp(min=0) if act == ACT_RELU else v.clamp(0, 6) if act == ACT_RELU6 else v


def _affine(acc, scale, shift, act, dt, defect=None):
    if scale is None:
        return _act(acc, act)
    s, sh = scale.to(dt).view(1, -1, 1, 1), shift.to(dt).view(1, -1, 1, 1)
    if defect == 'bn_relu6_order':
        return _act(acc, act) * s + sh
    return _act(acc * s + sh, act)


def _layer_bound(n, mag, scale, shift, op_err):
    """(n + 2 + a) 2^-23 (|scale| mag + |shift|) + |scale| op_err, a = 2 (0 without an affine)."""
    if scale is None:
        return sum_bound(n, mag) + op_err
    s, sh = scale.double().abs().view(1, -1, 1, 1), shift.double().abs().view(1, -1, 1, 1)
    return sum_bound(n + 2, s * mag + sh) + s * op_err


def patch_conv(d, dt=torch.float64, defect=None):
    """hs_patch_conv_fwd on case ``d``: skip, prev, coords, grid, bank, c_out, k, mode, groups, scale, shift, act."""
    x = stage(d['skip'], d.get('prev'), d.get('coords', False), dt, defect=defect)
    rows = d['c_out'] * (x.shape[1] // d['groups']) * d['k'] ** 2
    acc = conv_core(x, bank_rows(d['bank'], rows, dt, defect), d['grid'], d['c_out'], d['k'], d['mode'], d['groups'], defect)
    return _affine(acc, d.get('scale'), d.get('shift'), d.get('act', ACT_NONE), dt, defect)


def patch_conv_ref(d):
    """{'ref', 'bound', 'mag', 'terms'} of the case: the float64 value, the per-element bound of the module docstring, mag64."""
    dt = torch.float64
    xa, xe = (stage(d['skip'], d.get('prev'), d.get('coords', False), dt, role=r) for r in ('abs', 'err'))
    n = (xa.shape[1] // d['groups']) * d['k'] ** 2
    wa = bank_rows(d['bank'], d['c_out'] * n, dt).abs()
    args = (d['grid'], d['c_out'], d['k'], d['mode'], d['groups'])
    mag, err = conv_core(xa, wa, *args), conv_core(xe, wa, *args)
    return dict(ref=patch_conv(d), bound=_layer_bound(n, mag, d.get('scale'), d.get('shift'), err), mag=mag, terms=n)


# ------------------------------------------------------------------------------------------------------------ Op C / Op D

def _ir_weights(bank, cin, hid, c_out, b, grid, dt, defect=None):
    r1, r2 = cin * hid, cin * hid + 9 * hid
    w = bank_rows(bank, r2 + hid * c_out, dt, defect).view(b, grid[0], grid[1], -1)
    w1, kd, w3 = w[..., :r1].reshape(*w.shape[:3], hid, cin), w[..., r1:r2].reshape(*w.shape[:3], hid, 3, 3), w[..., r2:].reshape(*w.shape[:3], c_out, hid)
    if defect == 'drop_last_k':
        w3 = w3.clone()
        w3[..., -1] = 0
    return w1, kd, w3


def _bn_t(v, bn, dt, relu6, defect=None):
    """BN affine (+ ReLU6) on tiles (B, C, fh, fw, u, v)."""
    s, sh = bn[0].to(dt).view(1, -1, 1, 1, 1, 1), bn[1].to(dt).view(1, -1, 1, 1, 1, 1)
    if not relu6:
        return v * s + sh
    return v.clamp(0, 6) * s + sh if defect == 'bn_relu6_order' else (v * s + sh).clamp(0, 6)


def _dw(h1, kd, ph, pw):
    h2 = 0
    for ky in range(3):
        for kx in range(3):
            h2 = h2 + kd[..., ky, kx].permute(0, 3, 1, 2)[..., None, None] * h1[..., ky:ky + ph, kx:kx + pw]
    return h2


def _untile(t, b, c, h, w):
    return t.permute(0, 1, 2, 4, 3, 5).reshape(b, c, h, w)


def _pw1_tiles(x, w1, grid, ph, pw, own_ring, defect=None):
    """pw1 on the patch's halo tile: with its own weights on the whole tile (Op C), or each pixel with its OWNER's weights (Op D: the
    image-level k = 1 convolution, then the reflect-padded tile)."""
    if own_ring:
        return torch.einsum('bijhc,bcijuv->bhijuv', w1, halo_tiles(pad2d(x, 1, 'reflect', defect), grid, 1, ph, pw))
    b, _, h, w = x.shape
    img = _untile(torch.einsum('bijhc,bcijuv->bhijuv', w1, halo_tiles(x, grid, 0, ph, pw)), b, w1.shape[3], h, w)
    return img


def patch_ir(d, dt=torch.float64, defect=None, parts=False):
    """hs_patch_ir_fwd (d['op'] == 'c') / hs_patch_ir_v0_ws_fwd ('d') on case ``d``: skip, prev, coords, grid, bank, hid, c_out, bn1..3,
    residual.  parts=True: (out, h1 tiles, h2 tiles, x) for the bound."""
    x = stage(d['skip'], d.get('prev'), d.get('coords', True), dt, defect=defect)
    b, cin, h, w = x.shape
    grid, hid, c_out = d['grid'], d['hid'], d['c_out']
    ph, pw = h // grid[0], w // grid[1]
    own_ring = (d['op'] == 'c') != (defect == 'ring_own_weights' and d['op'] == 'd')
    w1, kd, w3 = _ir_weights(d['bank'], cin, hid, c_out, b, grid, dt, defect)
    a1 = _pw1_tiles(x, w1, grid, ph, pw, own_ring, defect)
    if own_ring:
        h1 = _bn_t(a1, d['bn1'], dt, True, defect)
    else:
        h1 = _affine(a1, d['bn1'][0], d['bn1'][1], ACT_RELU6, dt, defect)
        h1 = halo_tiles(pad2d(h1, 1, 'reflect', defect), grid, 1, ph, pw)
    h2 = _bn_t(_dw(h1, kd, ph, pw), d['bn2'], dt, True, defect)
    out = _untile(_bn_t(torch.einsum('bijoh,bhijuv->boijuv', w3, h2), d['bn3'], dt, False), b, c_out, h, w)
    if d.get('residual'):
        out = out + x
    return (out, h1, h2, x) if parts else out


def patch_ir_ref(d):
    """{'ref', 'bound', 'mag'}: e1 -> e2 -> e3 of the module docstring, every |W| applied to the previous layer's bound."""
    dt = torch.float64
    ref, h1, h2, x = patch_ir(d, parts=True)
    b, cin, h, w = x.shape
    grid, hid, c_out = d['grid'], d['hid'], d['c_out']
    ph, pw = h // grid[0], w // grid[1]
    own_ring = d['op'] == 'c'
    w1, kd, w3 = (t.abs() for t in _ir_weights(d['bank'], cin, hid, c_out, b, grid, dt))
    xa, xe = (stage(d['skip'], d.get('prev'), d.get('coords', True), dt, role=r) for r in ('abs', 'err'))
    absbn = lambda bn: (bn[0].double().abs(), bn[1].double().abs())

    def lin(t, bn):            # (n + 2 + 2) 2^-23 (|s| mag + |shift|) and |s| op_err share this affine on absolute values, shift apart
        return t * bn[0].double().abs().view(1, -1, *([1] * (t.dim() - 2)))

    def shift(t, bn):
        return bn[1].double().abs().view(1, -1, *([1] * (t.dim() - 2))).expand_as(t)
    m1, o1 = _pw1_tiles(xa, w1, grid, ph, pw, own_ring), _pw1_tiles(xe, w1, grid, ph, pw, own_ring)
    e1 = sum_bound(cin + 2, lin(m1, d['bn1']) + shift(m1, d['bn1'])) + lin(o1, d['bn1'])
    if not own_ring:
        e1 = halo_tiles(pad2d(e1, 1, 'reflect'), grid, 1, ph, pw)
    m2, o2 = _dw(h1.abs(), kd, ph, pw), _dw(e1, kd, ph, pw)
    e2 = sum_bound(9 + 2, lin(m2, d['bn2']) + shift(m2, d['bn2'])) + lin(o2, d['bn2'])
    m3, o3 = torch.einsum('bijoh,bhijuv->boijuv', w3, h2.abs()), torch.einsum('bijoh,bhijuv->boijuv', w3, e2)
    mag = lin(m3, d['bn3']) + shift(m3, d['bn3'])
    e3 = _untile(sum_bound(hid + 2, mag) + lin(o3, d['bn3']), b, c_out, h, w)
    mag = _untile(mag, b, c_out, h, w)
    if d.get('residual'):
        e3 = e3 + xe + U32 * (ref.abs() + xa)
        mag = mag + xa
    return dict(ref=ref, bound=e3, mag=mag)


# ------------------------------------------------------------------------------------------------------------ Op C, split mode

SPLIT_DEFECTS = ('split_low_dropped', 'scale_wrong_column')
H2_SCALE = 4096.0


def _inv_scale(m):
    """1 / scale of hs_patch_irc.hip for a maximum m >= 0 (irc_exp_of / irc_inv_scale_of): eb = the biased exponent of m clamped to
    [27, 254], scale = 2^(141 - eb) -- m * scale < 2^15 --, 1 / scale = 2^(eb - 141).  Exact powers of two, any float dtype."""
    eb = (torch.floor(torch.log2(m.double().clamp(min=1e-300))) + 127).clamp(27, 254)
    return torch.pow(2.0, eb - 141).to(m.dtype)


def _w_inv_scales(w, cin, hid):
    """Per-row 1 / scale of a weight matrix (..., rows, k): the MATRIX maximum when cin is even and hid a multiple of 4, else the row's."""
    m = w.abs().amax(-1, keepdim=True)
    if cin % 2 == 0 and hid % 4 == 0:
        m = m.amax(-2, keepdim=True).expand_as(m)
    return _inv_scale(m)


def _split16(v):
    hi = v.half().float()
    return hi, (v - hi).half().float()


def _split_parts(d):
    x = stage(d['skip'], d['prev'], True, torch.float64)
    b, cin, h, w = x.shape
    grid, hid, c_out = d['grid'], d['hid'], d['c_out']
    return x, b, cin, h, w, grid, hid, c_out, h // grid[0], w // grid[1]


def split_bound(d):
    """{'ref', 'bound', 'mag', 'floor1', 'rel1', 'floor3', 'rel3', 'clamped'} of Op C in split mode, from what hs_patch_irc.hip states.

    An operand v is scaled by s = 2^(141 - eb), eb the exponent of the maximum the scale is taken over (|v s| < 2^15), and split:
    hi = rne16(v s), lo = rne16(v s - hi).  |v s - hi| <= 2^-11 |v s|; lo rounds that with a relative 2^-11 while normal and an absolute
    2^-25 (half the f16 subnormal spacing) below 2^-14: the residual r obeys |r| <= 2^-22 |v s| + 2^-25, i.e. 2^-22 |v| + 2^-25 / s unscaled.
    A product is ah bh + al bh + ah bl: against (a sa)(b sb) it lacks al bl (<= 2^-22 |a sa| |b sb|) and ra (b sb) + rb (a sa).  Per term,
    unscaled:  3 * 2^-22 |a| |b|  +  2^-25 (|a| / sb + |b| / sa)  -- the second part is the FLOOR: it is relative to the maxima the scales
    were taken over, not to the term.  The 3 n f16 x f16 products are exact in fp32 and accumulated in fp32: sum_bound(3 n, mag).  The
    BatchNorm scale is folded with the (power-of-two) inverse scales and applied by one fmaf: a = 3 covers the fold, the fmaf and h2's
    exact * 4096.  The depthwise is fp32 with BN2's scale folded into the taps (one more rounding per tap: n = 9 + 9).  h2 in [0, 6] is
    scaled by 4096 (no data scale) and split the same way: 1 / s = 2^-12.  e1 -> e2 -> e3 chain as in patch_ir_ref."""
    dt = torch.float64
    x, b, cin, h, w, grid, hid, c_out, ph, pw = _split_parts(d)
    dd = dict(d, op='c', coords=True, residual=False)
    ref, h1, h2, _ = patch_ir(dd, parts=True)
    w1, kd, w3 = (t.abs() for t in _ir_weights(d['bank'], cin, hid, c_out, b, grid, dt))
    xa, xe = (stage(d['skip'], d['prev'], True, dt, role=r) for r in ('abs', 'err'))
    ta, te = (halo_tiles(pad2d(t, 1, 'reflect'), grid, 1, ph, pw) for t in (xa, xe))
    bn = lambda k, t: t * d[k][0].double().abs().view(1, -1, 1, 1, 1, 1)
    sh = lambda k, t: d[k][1].double().abs().view(1, -1, 1, 1, 1, 1).expand_as(t)
    isx = _inv_scale(ta.amax(1))                                  # (B, fh, fw, u, v): per halo position
    isw1, isw3 = _w_inv_scales(w1, cin, hid)[..., 0], _w_inv_scales(w3, cin, hid)[..., 0]      # (B, fh, fw, rows)
    clamped = bool((ta.amax(1) < 2.0 ** -100).any()) or bool((w1.amax(-1) < 2.0 ** -100).any()) or bool((w3.amax(-1) < 2.0 ** -100).any())
    m1 = torch.einsum('bijhc,bcijuv->bhijuv', w1, ta)
    floor1 = 2.0 ** -25 * (torch.einsum('bijh,bijuv->bhijuv', w1.sum(-1), isx) + torch.einsum('bijh,bijuv->bhijuv', isw1, ta.sum(1)))
    rel1 = 3 * 2.0 ** -22 * m1
    e1 = sum_bound(3 * cin + 2 + 3, bn('bn1', m1) + sh('bn1', m1)) + bn('bn1', rel1 + floor1 + torch.einsum('bijhc,bcijuv->bhijuv', w1, te))
    m2 = _dw(h1.abs(), kd, ph, pw)
    e2 = sum_bound(18 + 2 + 2, bn('bn2', m2) + sh('bn2', m2)) + bn('bn2', _dw(e1, kd, ph, pw))
    m3 = torch.einsum('bijoh,bhijuv->boijuv', w3, h2.abs())
    floor3 = 2.0 ** -25 * (w3.sum(-1).permute(0, 3, 1, 2)[..., None, None] * 2.0 ** -12
                           + isw3.permute(0, 3, 1, 2)[..., None, None] * h2.abs().sum(1, keepdim=True))
    rel3 = 3 * 2.0 ** -22 * m3
    mag = bn('bn3', m3) + sh('bn3', m3)
    e3 = sum_bound(3 * hid + 2 + 3, mag) + bn('bn3', rel3 + floor3 + torch.einsum('bijoh,bhijuv->boijuv', w3, e2))
    u = lambda t: _untile(t, b, t.shape[1], h, w)
    return dict(ref=ref, bound=u(e3), mag=u(mag), floor1=floor1, rel1=rel1, floor3=u(floor3), rel3=u(rel3), clamped=clamped)


def in_range(V):
    """Per OUTPUT element (B, c_out, H, W): every reduction behind it stays inside the dynamic range the split form carries -- no scale is
    clamped, and the floor of each reduction (the part of its bound that is relative to the scales' maxima) is no larger than its
    relative part.  pw3's own reduction per element; pw1's over every hidden unit of the element's patch.  From the inputs and the
    float64 reference alone, never from a kernel's output."""
    ok1 = (V['floor1'] <= V['rel1']).flatten(4).all(-1).all(1)            # (B, fh, fw): every pw1 reduction of the patch
    b, c, h, w = V['ref'].shape
    fh, fw = ok1.shape[1:]
    ok1 = ok1.repeat_interleave(h // fh, 1).repeat_interleave(w // fw, 2).unsqueeze(1)
    return (V['floor3'] <= V['rel3']) & ok1 & (not V['clamped'])


def split_emulate(d, defect=None):
    """Op C in split mode step by step in fp32 / f16 with torch on the CPU: scales, hi / lo pieces, the three piece products accumulated
    in fp32, folded BatchNorm, fp32 depthwise with folded taps, h2 * 4096 split, pw3.  ``defect`` in SPLIT_DEFECTS."""
    f = torch.float32
    x = stage(d['skip'], d['prev'], True, f)
    b, cin, h, w = x.shape
    grid, hid, c_out = d['grid'], d['hid'], d['c_out']
    ph, pw = h // grid[0], w // grid[1]
    w1, kd, w3 = _ir_weights(d['bank'], cin, hid, c_out, b, grid, f)
    t = halo_tiles(pad2d(x, 1, 'reflect'), grid, 1, ph, pw)               # B C fh fw u v
    isx = _inv_scale(t.abs().amax(1))
    if defect == 'scale_wrong_column':
        isx = isx.roll(1, -1)
    th, tl = _split16(t / isx.unsqueeze(1))
    isw1, isw3 = _w_inv_scales(w1, cin, hid), _w_inv_scales(w3, cin, hid)
    ah, al = _split16(w1 / isw1)
    mm = lambda a_, b_: torch.einsum('bijhc,bcijuv->bhijuv', a_, b_)
    acc = mm(ah, th) + mm(ah, tl) + (0 if defect == 'split_low_dropped' else mm(al, th))
    s1 = d['bn1'][0].view(1, -1, 1, 1, 1, 1) * isw1[..., 0].permute(0, 3, 1, 2)[..., None, None]
    h1 = (acc * isx.unsqueeze(1) * s1 + d['bn1'][1].view(1, -1, 1, 1, 1, 1)).clamp(0, 6)
    kf = kd * d['bn2'][0].view(1, 1, 1, -1, 1, 1)
    h2 = (_dw(h1, kf, ph, pw) + d['bn2'][1].view(1, -1, 1, 1, 1, 1)).clamp(0, 6)
    hh, hl = _split16(h2 * H2_SCALE)
    bh, bl = _split16(w3 / isw3)
    m3 = lambda a_, b_: torch.einsum('bijoh,bhijuv->boijuv', a_, b_)
    acc3 = m3(bh, hh) + m3(bh, hl) + m3(bl, hh)
    s3 = d['bn3'][0].view(1, -1, 1, 1, 1, 1) * (isw3[..., 0].permute(0, 3, 1, 2)[..., None, None] / H2_SCALE)
    return _untile(acc3 * s3 + d['bn3'][1].view(1, -1, 1, 1, 1, 1), b, c_out, h, w)


def check_where(got, V, keep, what):
    """``check`` on the elements ``keep`` selects (a predicate on the inputs); the others are left out.  Returns check's triple."""
    g = got.detach().double().cpu()
    assert bool(torch.isfinite(g).all()), f'{what}: non-finite output'
    W = dict(V, ref=V['ref'], bound=torch.where(keep, V['bound'], torch.full_like(V['bound'], float('inf'))))
    err = (g - V['ref']).abs()
    bad = (err > W['bound'])
    assert not bool(bad.any()), f'{what}: {int(bad.sum())} elements outside the split bound; worst err/bound {float((err / V["bound"])[keep].max()):.3f}'
    ratio = torch.where(keep, err / V['bound'].clamp(min=1e-300), torch.zeros_like(err))
    i = int(torch.argmax(ratio))
    return float(ratio.flatten()[i]), tuple(int(v) for v in torch.unravel_index(torch.tensor(i), g.shape)), float((err / V['mag'].clamp(min=1e-300))[keep].max())


# ------------------------------------------------------------------------------------------------------------ signal2weights, gen, meta_conv

def s2w_bank(signal, wsw, index, channels, groups, rows, dt=torch.float64, role='value'):
    """signal2weights as a patch-major bank (B fh fw, rows): the grouped 1x1 convolution of signal[:, index:index + channels] with wsw
    (Wc, channels / groups), Wc a multiple of groups; output channel n reads group n // (Wc / groups); the first ``rows`` channels are kept.
    role 'abs': on absolute values (mag64).  n = channels / groups terms: bound sum_bound(n, mag64)."""
    b, _, fh, fw = signal.shape
    wc, k = wsw.shape[0], channels // groups
    sl = signal[:, index:index + channels].to(dt).reshape(b, groups, k, fh, fw)
    wg = wsw.reshape(groups, wc // groups, k).to(dt)
    if role == 'abs':
        sl, wg = sl.abs(), wg.abs()
    out = torch.einsum('gnk,bgkij->bgnij', wg, sl).reshape(b, wc, fh, fw)[:, :rows]
    return out.permute(0, 2, 3, 1).reshape(b * fh * fw, rows)


def s2w_ref(d):
    mag = s2w_bank(d['signal'], d['wsw'], d['index'], d['channels'], d['groups'], d['rows'], role='abs')
    return dict(ref=s2w_bank(d['signal'], d['wsw'], d['index'], d['channels'], d['groups'], d['rows']), mag=mag,
                bound=sum_bound(d['channels'] // d['groups'], mag))


def patch_conv_gen(d, dt=torch.float64):
    """hs_patch_conv_gen_fwd: the bank of s2w_bank, consumed by the k = 1 patch convolution + affine + activation, never stored."""
    bank = s2w_bank(d['signal'], d['wsw'], d['index'], d['channels'], d['groups'], d['rows'], dt)
    return patch_conv(dict(d, bank=bank, k=1, mode='zeros', groups=1), dt)


def patch_conv_gen_ref(d):
    """The single-layer bound with TWO operand errors: the stage's EX through |W|, and the generated weights' own bound EW (s2w_ref)
    through |x|:  (n + 2 + a) 2^-23 mag_out + |scale| (|W| . EX + EW . |x| + EW . EX)."""
    dt = torch.float64
    W = s2w_ref(d)
    xa, xe = (stage(d['skip'], d.get('prev'), d.get('coords', False), dt, role=r) for r in ('abs', 'err'))
    n = xa.shape[1]
    args = (d['grid'], d['c_out'], 1, 'zeros', 1)
    wa, we = W['ref'].abs(), W['bound']
    mag = conv_core(xa, wa, *args)
    err = conv_core(xe, wa, *args) + conv_core(xa + xe, we, *args)
    return dict(ref=patch_conv_gen(d), bound=_layer_bound(n, mag, d.get('scale'), d.get('shift'), err), mag=mag)


def meta_conv(d, dt=torch.float64, role='value'):
    """hs_meta_conv_fwd: per-sample conv2d with kernel (kh, kw), stride, dilation, groups; zero padding (ph, pw) on both sides, the other
    modes through F.pad with (left, right, top, bottom) = (ph, pw, ph, pw) as the reference hands them over; affine + activation."""
    x, w = d['x'].to(dt), d['w'][:, :d['c_out'] * (d['x'].shape[1] // d['groups']) * d['k'][0] * d['k'][1]].to(dt)
    if role == 'abs':
        x, w = x.abs(), w.abs()
    (ph, pw), mode = d['pad'], d['mode']
    outs = []
    for b in range(x.shape[0]):
        xb = x[b:b + 1]
        xb = F.pad(xb, (pw, pw, ph, ph)) if mode == 'zeros' else F.pad(xb, (ph, pw, ph, pw), mode=mode)
        outs.append(F.conv2d(xb, w[b].reshape(d['c_out'], -1, *d['k']), None, stride=d['stride'], dilation=d['dil'], groups=d['groups']))
    acc = torch.cat(outs)
    return acc if role == 'abs' else _affine(acc, d.get('scale'), d.get('shift'), d.get('act', ACT_NONE), dt)


def meta_conv_ref(d):
    mag = meta_conv(d, role='abs')
    n = (d['x'].shape[1] // d['groups']) * d['k'][0] * d['k'][1]
    return dict(ref=meta_conv(d), mag=mag, bound=_layer_bound(n, mag, d.get('scale'), d.get('shift'), torch.zeros_like(mag)))


def q_level(got, V):
    """max |got - ref64| / mag64: the error LEVEL of a computation on a case (second tier: a kernel is held to twice the level of the CPU
    restatement of the SAME case, as util_encoder_ref does for long sums)."""
    return float(((got.detach().double().cpu() - V['ref']).abs() / V['mag'].clamp(min=1e-300)).max())


def check_tier2(got, V, level, keep=None, what=''):
    q = (got.detach().double().cpu() - V['ref']).abs() / V['mag'].clamp(min=1e-300)
    if keep is not None:
        q = torch.where(keep, q, torch.zeros_like(q))
    assert float(q.max()) <= 2 * level, f'{what}: q {float(q.max()):.3e} above twice the CPU level {level:.3e}'
    return float(q.max())


# ------------------------------------------------------------------------------------------------------------ checking

def check(got, V, what):
    """``got`` inside V['bound'] around V['ref'], element by element (assert_within_f16 with the bound as its absolute allowance);
    returns (worst err / bound, its index, worst err / mag64)."""
    ref, bound = V['ref'], V['bound']
    assert bool(torch.isfinite(ref).all()) and bool(torch.isfinite(bound).all()), f'{what}: non-finite reference'
    assert_within_f16(got, ref, -2, torch.zeros_like(ref), extra64=bound, half=False, what=what)
    err = (got.detach().double().cpu() - ref).abs()
    ratio = err / bound.clamp(min=1e-300)
    i = int(torch.argmax(ratio))
    rel = float((err / V['mag'].clamp(min=1e-300)).max()) if 'mag' in V else float('nan')
    return float(ratio.flatten()[i]), tuple(int(v) for v in torch.unravel_index(torch.tensor(i), ref.shape)), rel


def rejects(got, V):
    return bool(((got.detach().double().cpu() - V['ref']).abs() > V['bound']).any())


def old_rel_err(got, ref):
    """The tensor norm of tests/test_hip_parity.py: max|a - b| / max|b|."""
    return float((got.double() - ref.double()).abs().max() / ref.double().abs().max())
