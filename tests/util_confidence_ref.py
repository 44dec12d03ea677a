"""The per-element bound the confidence maps are held to, against float64 ``softmax(v, 1).max(1)``, and fp32 restatements with a defect.

Nothing here touches the GPU.  The quantity: for the fp32 class scores v_0 .. v_{C-1} of a pixel (exact inputs: the float64 reference reads
the same numbers), conf = 1 / S with S = sum_c t_c, t_c = exp(v_c - M), M = max_c v_c.  The recurrence under test (csrc/hs_confidence.h,
hyperseg_amd/utils/confidence.py) walks c = 0 .. C-1 with a running maximum m (always one of the inputs: exact) and a running sum s:

    start   m = v_0, s = 1                                               (the term of class 0: exactly 1)
    step k  d_k = v_k - m
            d_k > 0  (the maximum moves):   e = expf(fl(-d_k));  s = fl(fl(s * e) + 1);  m = v_k
            d_k <= 0:                       e = expf(fl(d_k));   s = fl(s + e)
    end     conf = fl(1 / s)

Derivation, with u = 2^-24 (one fp32 rounding, relative), E the relative error of expf on a normal result, and every product of
(1 + small) factors bounded by exp(sum of the smalls):

  * The argument fl(+-d_k) is within u |d_k| of d_k, so exp of it is exp(d_k) times a factor within a_k = expm1(u |d_k|) of 1; expf adds
    E.  (|d_k| <= 104 before the result underflows: a_k is a few 1e-6 at most, but it is computed, not assumed.)
  * A step multiplies every term already in s by one factor, and creates one new term:
        no move:  old terms (1 + delta), |delta| <= u (the add);   new term exp(d_k) (1 + a_k)(1 + E)(1 + delta): own_k = a_k + E + u
        move:     old terms exp(-d_k) (1 + a_k)(1 + E)(1 + delta_mul)(1 + delta_add) -- exp(-d_k) is exactly the change of reference from
                  the old maximum to the new one -- so r_k = a_k + E + 2u;   new term 1 (1 + delta_add): own_k = u
    so with r_k = u (no move) or a_k + E + 2u (move), term c ends as t_c (1 + eta_c), |eta_c| <= expm1(own_c + sum_{k > c} r_k), own_0 = 0.
    Note what this keeps apart: the argument error u |d_k| of a NON-moving step weighs only that step's own (small) term t_k, and the moving
    steps' |d_k| telescope to M - v_0, so scores spread over +-40 do not cost C times 80 u on every term.
  * Underflow.  Where an expf result or the product s * e falls below the smallest normal 2^-126 the relative statement fails; the
    absolute error there is at most 2^-126 per value (flushed to zero or rounded as a denormal alike), in units of the current maximum, and
    later rescales only shrink it.  At most C such terms, and at most C rescales of a sum <= C: C (C + 1) 2^-126 on S in all.
  * So |s - S| <= dS = sum_c t_c expm1(own_c + sum_{k > c} r_k) + C (C + 1) 2^-126, and with rel = dS / S (< 1) and the division within
    one ulp (DIV = 2u; a correctly rounded one is within u):
        |conf_f32 - conf| <= conf (rel / (1 - rel) + DIV (1 + rel / (1 - rel)))

E: HIP documents expf at 1 ulp (ROCm "HIP math API", single precision: expf, max ulp error 1); the CPU's is glibc's / SLEEF's 1-ulp expf
through torch.  EXPF_ULPS = 2 covers either with a factor 2 in hand; an ulp is 2^-23 relative.  No constant here is measured from the
code under test.  For C = 1 every sum is empty: dS = 2 * 2^-126 and the bound is DIV (conf = 1 exactly is well inside it).
"""
import torch

U = 2.0 ** -24
EXPF_ULPS = 2.0
E = EXPF_ULPS * 2.0 ** -23
DIV = 2.0 * U
TINY = 2.0 ** -126


def confidence_ref_bound(scores):
    """``(ref64, bound64)`` for (B, C, ...) fp32 ``scores`` (finite): float64 ``softmax(scores, 1).max(1)`` and the bound of this module's
    header on an fp32 confidence made by the recurrence, per pixel."""
    assert scores.dtype == torch.float32
    v = scores.detach().cpu().double()
    C = v.shape[1]
    ref = torch.softmax(v, 1).max(1).values
    M = v.max(1).values
    t = torch.exp(v - M.unsqueeze(1))
    S = t.sum(1)
    own, r = [torch.zeros_like(M)], [torch.zeros_like(M)]           # class 0: the exact 1; r[0] is never used
    m = v[:, 0].clone()
    for k in range(1, C):
        d = v[:, k] - m
        up = d > 0
        a = torch.expm1(U * d.abs())
        own.append(torch.where(up, torch.full_like(a, U), a + E + U))
        r.append(torch.where(up, a + E + 2 * U, torch.full_like(a, U)))
        m = torch.where(up, v[:, k], m)
    after = torch.zeros_like(M)                                      # sum_{k > c} r_k, walking c down
    dS = torch.zeros_like(M)
    for c in range(C - 1, -1, -1):
        dS = dS + t[:, c] * torch.expm1(own[c] + after)
        after = after + r[c]
    dS = dS + C * (C + 1) * TINY
    rel = dS / S
    assert bool((rel < 0.5).all())
    grow = rel / (1.0 - rel)
    return ref, (1.0 / S) * (grow + DIV * (1.0 + grow))


def worst_ratio(conf_f32, scores):
    """``(max |conf - ref| / bound, its flat index, ref64, bound64)``; the caller asserts ratio <= 1."""
    ref, bound = confidence_ref_bound(scores)
    got = conf_f32.detach().cpu().double()
    assert got.shape == ref.shape, (tuple(got.shape), tuple(ref.shape))
    assert bool(torch.isfinite(got).all()), 'non-finite confidence from finite scores'
    ratio = (got - ref).abs() / bound
    i = int(ratio.argmax())
    return float(ratio.flatten()[i]), i, ref, bound


def assert_within(conf_f32, scores, what=''):
    ratio, i, _, _ = worst_ratio(conf_f32, scores)
    assert ratio <= 1.0, f'{what}: |conf - ref64| is {ratio:.3f} x the derived bound at flat index {i}'
    return ratio, i


# ---- fp32 restatements of the recurrence with one defect each: the same walk as hyperseg_amd.utils.confidence.softmax_max_f32

def _walk(scores, first_sum, on_move):
    v = scores.to(torch.float32)
    m, s = v[:, 0].clone(), torch.full_like(v[:, 0], first_sum)
    for c in range(1, v.shape[1]):
        vc = v[:, c]
        up = vc > m
        e = torch.exp(torch.where(up, m - vc, vc - m))
        s = torch.where(up, on_move(s, e), s + e)
        m = torch.where(up, vc, m)
    return 1.0 / s


def defect_no_own_term(scores):
    """The arg-max's own term (the 1) left out of the sum: conf = 1 / (S - 1)."""
    return _walk(scores, 0.0, lambda s, e: s * e)


def defect_no_rescale(scores):
    """The sum not rescaled when the maximum moves: the old terms stay relative to the old maximum."""
    return _walk(scores, 1.0, lambda s, e: s + 1.0)


DEFECTS = {'no_own_term': defect_no_own_term, 'no_rescale': defect_no_rescale}


# ---- the inputs of the issue: (B, C, H, W) fp32 scores, each drawn from its own seeded generator

def _gen(seed):
    return torch.Generator().manual_seed(int(seed))


def scores_order_one(C, seed, shape=(2, 5, 7)):
    b, h, w = shape
    return torch.randn(b, C, h, w, generator=_gen(seed))


def scores_spread(C, seed, shape=(2, 5, 7)):
    """Spread over +-40 (differences up to 80: terms down to exp(-80) = 1.8e-35, lost against a sum >= 1); the first image row is spread
    over +-60, whose differences reach past 87.3 and 104, where expf returns denormals and 0."""
    b, h, w = shape
    x = (torch.rand(b, C, h, w, generator=_gen(seed)) * 2 - 1) * 40
    x[:, :, 0] *= 1.5                                    # first row: +-60, differences up to 120 -> expf underflows to denormals and 0
    return x


def scores_ties(C, seed, shape=(2, 5, 7)):
    """Exact ties between classes, the maximum included: scores from a grid of 4 values."""
    b, h, w = shape
    return torch.randint(0, 4, (b, C, h, w), generator=_gen(seed)).float() * 0.5


def scores_max_at(C, seed, where, shape=(2, 5, 7)):
    """The maximum in class ``where`` (0: first, -1: last), strictly."""
    x = scores_order_one(C, seed, shape)
    x[:, where] = x.max(1).values + 1.0
    return x
