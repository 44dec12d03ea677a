"""Host-only restatement of hs_gemm_split.hip's arithmetic and the per-element bound its results are held to.

Imports the project only for ``gemm_split_weights`` (the callers pass its result in); everything else is stock torch on the CPU.

``emulate`` is the kernel step by step: the plan of ``gemm_split_plan`` (NWV waves x NCH chunks x KS k-steps of 32), K padded with
zeros to the plan's depth, the gate multiplied in f32, one power-of-two scale per (wave, chunk, pixel) from the biased exponent of the
slice maximum clamped to [27, 254], two binary16 pieces of the scaled column, the three products al*bh, ah*bl, ah*bh per k-step (a
product of two binary16 values has 22 significant bits and an exponent far inside f32: exact), an f32 running sum per chunk, the
chunk's scale undone (chunk 1 by one fused multiply-add onto chunk 0), the waves' partial tiles summed in wave order, ``w_inv``.
The 2x2 / stride-2 form is the same product on the window matrix, k = 4 c + 2 dy + dx, n = oy Wo + ox.  What the emulation cannot
know is the order in which one matrix-core instruction adds its 32 products; ``perms`` permutes the products of a chunk and
``reverse_waves`` the wave order, and ``steps='f64'`` gives the sum without any f32 rounding.

THE BOUND (``split_bound``), per element (m, n), on |kernel - float64|.  Notation: s_m = 2^(141 - ebw_m) the row's scale,
R_m = 2^15 / s_m = 2^(ebw_m - 126) the power of two above the row maximum (at the clamp: 2^-99 for every smaller row);
C_{S,n} = 2^(eb - 126) likewise for pixel n in slice S = (wave, chunk); mag = sum_k |w_mk| |g_k x_kn|.

 1. gate multiply, one f32 rounding per term: 2^-24 mag (no gate: 0).
 2. two-piece operands.  hi = rn16(v) leaves |v - hi| <= 2^-11 |v|, lo = rn16(v - hi) leaves 2^-11 of that: 2^-22 |v| while lo is a
    normal binary16, and half the subnormal quantum, 2^-25 in scaled units, below.  max(a, b) <= a + b, so every operand is
    v (1 + d) + f with |d| <= 2^-22, |f| <= 2^-25.  Relative part of a product of two such operands: 2 * 2^-22 |w||x|.
 3. the dropped al*bl: |lo| <= 2^-11 |v| (1 + 2^-11) on both sides: 2^-22 (1 + 2^-10) |w||x|.
    2. and 3. together: 3 * 2^-22 (1 + 2^-10) mag (the (1 + 2^-10) also covers the second-order d d' of 2.).
 4. the floor of 2.: f times the other operand, which is below 2^15 in scaled units: 2^-25 2^15 / (s_m s_c) = 2^-40 R_m C_{S,n} per
    term and operand, so 2 * 2^-40 R_m sum_S cnt_S C_{S,n} with cnt_S the slice's k < K (padded terms are exact zeros on both sides).
    2^-25 rests on binary16 subnormals SURVIVING the split and the matrix cores: v_fma_mix{lo,hi}_f16 is a VALU operation and
    rounds / keeps subnormal results as MODE.fp_denorm's f16/f64 field says; the matrix cores' f16 A / B inputs honour the same field
    and their C / D never flush (CDNA ISA, "Matrix arithmetic: rounding and denormals"; the programming guide's "Subnormals come
    through un-flushed"); the kernel descriptor hipcc writes for this file carries .amdhsa_float_denorm_mode_16_64 3 (keep both ways)
    and nothing in the build passes a flush option.  A flushing device would need 2^-14 here, and the `clamps` inputs below would
    show it.
 5. f32 accumulation.  Along any path a product passes 3*32*KS*NCH chunk additions, NCH - 1 <= 1 chunk join, NWV wave additions and
    the final multiply-add: (3*32*KS*NCH + NWV + 2) first-order roundings, each 2^-24 of a partial sum of absolute values; the
    convention of util_f16_ref.sum_bound doubles that to 2^-23 for any order and the higher orders; the absolute sum of the products
    actually added exceeds mag by the lo pieces, a factor (1 + 2^-9).
 6. underflow: a result in f32's subnormal range is off by up to 2^-150 whatever its size.  NWV*NCH chunk scalings and NWV wave sums
    in row-scaled units (x w_inv_m to the output's), the final rounding, and with a gate sum_k |w_mk| 2^-150 for g_k x_kn.
 7. the tail, when used (``tail_bound``): the shift rides on the final multiply-add, whose rounding is now relative to the
    pre-activation z = t w_inv + shift: 2^-24 (|z| + e); ReLU / ReLU6 are 1-Lipschitz; swish has |d/dz| <= 1.0999 and the project's
    own allowance of 2e-5 of the activation's value for its exp2 / rcp form (test_gemm_split_vs_float64); the residual add is one more
    rounding, 2^-24 (|y| + e).

RANGE (shared by the emulation, so a limit of the design): the partial sums live in ROW-SCALED units until
``w_inv`` is applied, so they overflow f32 where s_m mag >= 2^127 -- about |x| >= 2^112 / K against a row's largest weights --
although the float64 value (and a plain f32 GEMM) may be finite.  ``in_range`` is that predicate; outside it the kernel returns
inf / NaN (never a finite wrong number), which the tests pin against the emulation.

TIER 2.  Term 5 is a worst case three orders above what a sum of rounding errors does, so precision-class defects (a missing ah*bl)
could hide under it at large K.  ``q_of`` = max |got - ref64| / (mag + floor + 2^24 underflow) is therefore also compared with the
largest q the emulation itself reaches over ``orders()`` (>= 32 summation orders), times MARGIN = 2 -- the ONE constant here that is
a margin and not derived: the emulation cannot know the order or width in which the matrix core adds its 32 products.  The level is
taken twice per input, over the ``quiet`` elements (floor above one rounding of mag) and over all others, and the kernel is held to
each: a floor-dominated element reaches q ~ 1e-4 by design and would otherwise set the level for every element of its tensor."""
from collections import namedtuple

import torch

Plan = namedtuple('Plan', 'nwv ks nch')
MARGIN = 2.0
DEFECTS = ('drop_cross', 'shared_chunk_scale', 'lane_group_max', 'no_clamp')


def plan_of(k):
    """gemm_split_plan: the fewest k-steps per wave with 2, 4 or 8 waves; more than 5 per wave go in two chunks."""
    steps = -(-k // 32)
    nwv = 2
    while nwv < 8 and nwv < steps:
        nwv *= 2
    nch = 2 if -(-steps // nwv) > 5 else 1
    ks = -(-steps // (nwv * nch))
    assert ks <= 5, k
    return Plan(nwv, ks, nch)


def window_matrix(x):
    """(C, 2 Ho, 2 Wo) -> the (4 C, Ho Wo) matrix the 2x2 / stride-2 form multiplies: k = 4 c + 2 dy + dx, n = oy Wo + ox."""
    c, h, w = x.shape
    return x.reshape(c, h // 2, 2, w // 2, 2).permute(0, 2, 4, 1, 3).reshape(4 * c, (h // 2) * (w // 2))


def window_image(xk, ho, wo):
    """Inverse of ``window_matrix``."""
    c = xk.shape[0] // 4
    return xk.reshape(c, 2, 2, ho, wo).permute(0, 3, 1, 4, 2).reshape(c, 2 * ho, 2 * wo).contiguous()


def _pow2(e):
    return torch.ldexp(torch.ones(e.shape, dtype=torch.float64), e)


def _pieces(sw):
    rt = sw.frag.shape[0]
    return sw.frag.cpu().permute(2, 0, 4, 1, 3, 5).reshape(2, 16 * rt, sw.kp)             # [piece][row][k], f16


def _slices(sw, x, gate, patch, defect=None):
    """The gated, padded input per slice (Q, L, N) f32, its biased exponents and the scales (per k and per output row, float64)."""
    xk = window_matrix(x) if patch else x
    k, n = xk.shape
    assert k == sw.c_in and xk.dtype == torch.float32
    plan = plan_of(k)
    q, l = plan.nwv * plan.nch, plan.ks * 32
    assert q * l == sw.kp
    xg = xk if gate is None else xk * gate[:, None]                                         # one f32 rounding
    xq = torch.nn.functional.pad(xg, (0, 0, 0, sw.kp - k)).reshape(q, l, n).contiguous()
    bits = xq.view(torch.int32) & 0x7fffffff                                                # the kernel's integer maximum: NaN > inf > finite
    r = 16 * sw.frag.shape[0]
    if defect == 'lane_group_max':       # no reduction over the four lane groups: each 8-k group its own scale, undone on the group's 4 rows
        eb = (bits.view(q, plan.ks, 4, 8, n).amax((1, 3)) >> 23).clamp(27, 254)             # (Q, 4, N)
        eb_k = eb[:, None, :, None, :].expand(q, plan.ks, 4, 8, n).reshape(q, l, n)
        eb_r = eb[:, (torch.arange(r) % 16) // 4, :]                                        # (Q, R, N)
    else:
        eb = bits.amax(1) >> 23
        if defect != 'no_clamp':
            eb = eb.clamp(27, 254)
        if defect == 'shared_chunk_scale' and plan.nch == 2:
            eb = eb.view(plan.nwv, 2, n)[:, :1].expand(plan.nwv, 2, n).reshape(q, n)
        eb_k, eb_r = eb[:, None, :], eb[:, None, :]
    if defect == 'no_clamp':             # 2^(141 - eb) as an f32: no longer a normal float below eb = 14
        f = torch.ones(eb.shape)
        sc, inv = torch.ldexp(f, 141 - eb).double()[:, None, :], torch.ldexp(f, eb - 141).double()[:, None, :]
    else:
        sc, inv = _pow2(141 - eb_k), _pow2(eb_r - 141)
    return plan, xq, eb, sc, inv


def orders(plan, count=32, seed=0):
    """``count`` summation orders for ``emulate``: (perms (count, 96 KS) -- order 0 the nominal one, k-step by k-step, al*bh, ah*bl,
    ah*bh, k ascending --, reverse_waves (count,) -- every odd order sums the waves last to first)."""
    t = 96 * plan.ks
    g = torch.Generator().manual_seed(1000 + seed)
    perms = torch.stack([torch.arange(t)] + [torch.randperm(t, generator=g) for _ in range(count - 1)])
    return perms, [bool(i & 1) for i in range(count)]


def emulate(sw, x, gate, *, patch=False, defect=None, steps='f32', perms=None, reverse_waves=False):
    """The kernel's y (M, N) for ONE frame: ``x`` (K, N) f32, or (C, 2 Ho, 2 Wo) with ``patch``; ``gate`` (K,) or None; no shift,
    activation or residual.  ``perms`` (O, 96 KS): one result per order, (O, M, N), ``reverse_waves`` then a list of O flags.
    ``steps='f64'``: the same products summed exactly (float64 result).  ``defect``: one of DEFECTS -- wrong kernels for the teeth
    test, restated here only."""
    assert defect is None or defect in DEFECTS
    plan, xq, _, sc, inv = _slices(sw, x, gate, patch, defect)
    q, l, n = xq.shape
    xs = xq.double() * sc                                    # exact: an f32 times a power of two
    bh = xs.float().half()
    bl = (xs - bh.double()).float().half()                   # the difference is exact in f32 (v_fma_mix: one rounding, to f16)
    back = _pieces(sw)
    r = back.shape[1]
    ah, al = (back[i].view(r, q, plan.ks, 32).permute(1, 0, 2, 3) for i in (0, 1))          # (Q, R, KS, 32)
    a = torch.stack([al, ah, ah], 3).reshape(q, r, 3 * l)                                   # nominal order of a chunk's products
    bm = torch.zeros_like(bl) if defect == 'drop_cross' else bl
    b = torch.stack([t.view(q, plan.ks, 32, n) for t in (bh, bm, bh)], 2).reshape(q, 3 * l, n)
    w_inv = sw.inv.cpu().double()[:, None]
    if steps == 'f64':
        part = torch.bmm(a.double(), b.double()) * inv                                      # (Q, R, N)
        return (part.sum(0) * w_inv)[:sw.c_out]
    single = perms is None
    if single:
        perms, reverse_waves = torch.arange(3 * l)[None], [bool(reverse_waves)]
    o = perms.shape[0]
    ap = a.float()[:, :, perms].permute(3, 2, 0, 1).unsqueeze(-1).contiguous()              # (T, O, Q, R, 1)
    bp = b.float()[:, perms, :].permute(2, 1, 0, 3).unsqueeze(-2).contiguous()              # (T, O, Q, 1, N)
    acc = torch.zeros(o, q, r, n)
    for t in range(3 * l):
        acc += ap[t] * bp[t]                                 # the product is exact in f32; the addition rounds once
    acc = acc.double().view(o, plan.nwv, plan.nch, r, n)
    inv = inv.expand(q, inv.shape[1], n).reshape(plan.nwv, plan.nch, -1, n)
    tot = (acc[:, :, 0] * inv[:, 0]).float()
    if plan.nch == 2:
        tot = (acc[:, :, 1] * inv[:, 1] + tot.double()).float()                             # fmaf(acc, invb, tot)
    y = torch.zeros(o, r, n)
    for w in range(plan.nwv):
        idx = torch.tensor([plan.nwv - 1 - w if rev else w for rev in reverse_waves])
        y = y + tot[torch.arange(o), idx]
    y = (y.double() * w_inv).float()[:, :sw.c_out]
    return y[0] if single else y


def split_terms(sw, x, gate, plan=None, patch=False):
    """mag, floor, underflow (each (M, N) float64) of the module docstring, and the row-scaled magnitude s_m mag."""
    p, xq, eb, _, _ = _slices(sw, x, gate, patch)
    assert plan is None or tuple(plan) == tuple(p)
    xk = window_matrix(x) if patch else x
    k, n = xk.shape
    m = sw.c_out
    back = _pieces(sw).double()
    ws = (back[0] + back[1])[:m, :k].abs()                                                   # the row in scaled units
    w_inv = sw.inv.cpu().double()[:m, None]
    gx = xk.double().abs() if gate is None else (xk.double() * gate.double()[:, None]).abs()
    scaled = ws @ gx.nan_to_num(nan=float('inf'))
    mag = scaled * w_inv * (1 + 2.0 ** -21)                                                  # |w| from its two pieces: within 2^-21
    l = p.ks * 32
    cnt = torch.tensor([max(0, min(l, k - i * l)) for i in range(p.nwv * p.nch)], dtype=torch.float64)
    c = _pow2(eb - 126)                                                                      # (Q, N)
    floor = 2.0 * 2.0 ** -40 * (w_inv * 2.0 ** 15) * (cnt[:, None] * c).sum(0)[None, :]
    under = 2.0 ** -150 * ((p.nwv * p.nch + p.nwv) * w_inv + 1.0).expand(m, n).clone()
    if gate is not None:
        under = under + 2.0 ** -150 * (ws.sum(1, keepdim=True) * w_inv)
    return mag, floor, under, scaled


def split_bound(sw, x, gate, plan=None, patch=False):
    """Worst-case |kernel - float64| per element (M, N), float64: terms 1-6 of the module docstring."""
    p = plan_of(sw.c_in) if plan is None else plan
    mag, floor, under, _ = split_terms(sw, x, gate, p, patch)
    rel = (2.0 ** -24 if gate is not None else 0.0) + 3 * 2.0 ** -22 * (1 + 2.0 ** -10) \
        + (96 * p.ks * p.nch + p.nwv + 2) * 2.0 ** -23 * (1 + 2.0 ** -9)
    return rel * mag + floor + under


def in_range(sw, x, gate, patch=False):
    """(M, N) bool: the row-scaled absolute sum stays below 2^127, so no partial sum of the kernel can leave f32."""
    return split_terms(sw, x, gate, None, patch)[3] < 2.0 ** 127


def tail_bound(e, z64, a64, y64, swish, residual):
    """Term 7: ``e`` the bound of the bare product, ``z64`` the float64 pre-activation (with the shift), ``a64`` the activation's
    float64 value, ``y64`` the final value (``residual``: whether one was added)."""
    e = e + 2.0 ** -24 * (z64.abs() + e)
    if swish:
        e = 1.0999 * e + 2e-5 * a64.abs()
    if residual:
        e = e + 2.0 ** -24 * (y64.abs() + e)
    return e


def quiet(sw, x, gate, patch=False):
    """(M, N) bool: elements whose floor and underflow terms exceed ONE f32 rounding of mag (2^-24 mag).  There the error may
    legitimately reach the floor itself (q up to 1), so tier 2 takes its level separately over these and over the rest: one such
    element must not set the level for a whole tensor."""
    mag, floor, under, _ = split_terms(sw, x, gate, None, patch)
    return floor + 2.0 ** 24 * under > 2.0 ** -24 * mag


def q_of(got, ref64, sw, x, gate, patch=False, where=None):
    """Tier 2: (max over elements of |got - ref64| / (mag + floor + 2^24 underflow), flat index); got (..., M, N)."""
    mag, floor, under, _ = split_terms(sw, x, gate, None, patch)
    den = mag + floor + 2.0 ** 24 * under
    ok = torch.isfinite(ref64) & torch.isfinite(den)
    if where is not None:
        ok = ok & where
    got = got.detach().double().cpu()
    err = torch.where(ok & torch.isfinite(got), (got - ref64).abs() / den, torch.zeros_like(den))
    err = err.reshape(-1, err.shape[-2] * err.shape[-1]).amax(0)
    i = int(err.argmax())
    return float(err[i]), i


def assert_split(got, ref64, bound, what, where=None):
    """|got - ref64| <= bound elementwise and isfinite(got) == isfinite(ref64), over ``where`` (default: everywhere).  Returns the
    worst element's err / bound; on failure reports it with its index, as util_f16_ref.assert_within_f16 does."""
    got = got.detach().double().cpu().reshape(ref64.shape)
    sel = torch.ones_like(ref64, dtype=torch.bool) if where is None else where
    fr, fg = torch.isfinite(ref64), torch.isfinite(got)
    wrong = sel & (fr != fg)
    if bool(wrong.any()):
        idx = [tuple(int(v) for v in i) for i in torch.nonzero(wrong)[:8]]
        raise AssertionError(f'{what}: {int(wrong.sum())} elements finite on one side only (got finite {int((fg & sel).sum())}, '
                             f'reference finite {int((fr & sel).sum())}); first indices {idx}')
    live = sel & fr
    err = torch.where(live, (got - ref64).abs(), torch.zeros_like(ref64))
    ratio = err / torch.where(live, bound, torch.ones_like(bound)).clamp(min=1e-300)
    worst = int(ratio.argmax())
    r = float(ratio.flatten()[worst])
    if not r <= 1.0:
        bad = ratio > 1.0
        idx = [tuple(int(v) for v in i) for i in torch.nonzero(bad)[:8]]
        raise AssertionError(f'{what}: {int(bad.sum())} of {ref64.numel()} elements outside the split bound; worst ratio {r:.3g} at flat '
                             f'index {worst}: |err| {float(err.flatten()[worst]):.3e} vs bound {float(bound.flatten()[worst]):.3e} '
                             f'(ref {float(ref64.flatten()[worst]):.6g}, got {float(got.flatten()[worst]):.6g}); first indices {idx}')
    return r


# ------------------------------------------------------------------------------------------------------------ range inputs

GENERATORS = ('rows', 'cols', 'slices', 'clamps', 'gate', 'benign')


def _benign(m, k, n, g):
    return (torch.randn(m, k, generator=g) / k ** 0.5, torch.randn(k, n, generator=g) * torch.rand(k, 1, generator=g) * 4,
            torch.rand(k, generator=g))


def make_inputs(name, m, k, n, seed, gated=True):
    """(w (M, K), x (K, N) in GEMM order, gate (K,) or None) of the named range generator; ``gated=False`` (the window form has no
    gate) folds the gate into x's rows."""
    g = torch.Generator().manual_seed(int(seed))
    plan = plan_of(k)
    l = plan.ks * 32
    w, x, gate = _benign(m, k, n, g)
    if name == 'rows':                   # (a) row magnitudes 2^-30 ... 2^30, an all-zero row, a row with a single nonzero
        w = w * torch.ldexp(torch.ones(m), torch.linspace(-30, 30, m).round().int())[:, None]
        w[1 % m] = 0
        w[2 % m] = 0
        w[2 % m, k // 2] = 1.5
    elif name == 'cols':                 # (b) column magnitudes 2^-40 ... 2^40; all-zero, single-nonzero, one-slice-only columns
        x = x * torch.ldexp(torch.ones(n), torch.linspace(-40, 40, n).round().int())[None, :]
        x[:, 0] = 0
        if n > 1:
            x[:, 1] = 0
            x[k // 3, 1] = -2.75
        if n > 2:
            x[:l, 2] = 0
            x[2 * l:, 2] = 0                                                                # alive in slice 1 only (k in [L, 2 L))
    elif name == 'slices':               # (c) 2^+-12 between slices, 2^+-10 inside one
        sl = torch.arange(k) // l
        e = torch.where(sl % 2 == 0, 12, -12) + torch.randint(-10, 11, (k,), generator=g)
        x = x * torch.ldexp(torch.ones(k), e.int())[:, None]
    elif name == 'clamps':               # (d) both exponent clamps; every second row tiny so that the huge columns stay in range
        w = w * 2.0 ** -20
        w[::2] = w[::2] * 2.0 ** -104                                                       # row maxima near 2^-124: below the row clamp
        unit = torch.randn(k, 4, generator=g).clamp(-3, 3) / 4                              # |.| < 1, the maximum set below
        unit[k // 2] = torch.tensor([0.99, -0.99, 0.99, -0.99])
        for j, e in enumerate((-135.0, -105.0, 125.0, 126.99)):
            if j < n:
                x[:, j] = (unit[:, j].double() / 0.99 * 2.0 ** e).float()
    elif name == 'gate':                 # (e) gates over 2^-20 ... 2^10 with exact zeros
        gate = torch.ldexp(torch.rand(k, generator=g) + 0.5, torch.randint(-20, 11, (k,), generator=g).int())
        gate[torch.rand(k, generator=g) < 0.25] = 0
    else:
        assert name == 'benign', name
    if not gated:
        x, gate = x * gate[:, None], None
    return w, x, gate
