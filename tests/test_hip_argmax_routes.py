"""The three routes to the final upsample's masks -- ``upsample_argmax``, ``upsample_confusion(masks=True)`` and ``upsample_overlay`` -- held
to each other and to ``numpy.argmax`` (first occurrence) over ``upsample_bilinear``'s logits, on inputs where the tie rules decide: the three
launches share one arg-max core (csrc/hs_upsample_taps.h: argmax2x_block / argmax_row4).  Masks, matrices and overlays are integers and
bytes: every comparison is equality, no tolerance appears in this file.

Logits are multiples of 0.25 in [-1, 1], piecewise constant over 2 x 3 cells with a tenth of the pixels drawn on their own: classes that
agree on all the taps of an output pixel tie there bit for bit in either kernel form, whatever the resize ratio.  ``_case`` asserts that at
least a tenth of the output pixels of every random case have a tied maximum (C = 1 has nothing to tie with); a second tensor is all-equal.
Class counts: 1 and 2 leave lanes of the exact-2x form's quad without a class of their own; 21 and 24 take the second trip of its stride-20
class loop, with and without clamped loads."""
import functools

import numpy as np
import pytest
import torch

from conftest import G

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
BATCH = 2
CLASSES = [1, 2, 5, 19, 21, 24]
# (Hi, Wi) -> (Ho, Wo)
SHAPES = [((3, 2), (6, 4)),             # exact 2x: the smallest legal case, edges everywhere
          ((33, 50), (66, 100)),        # exact 2x: 825 blocks per image -- the last workgroup has surplus lanes that shadow the last block
          ((5, 7), (10, 14)),           # general form: a 2x ratio with an odd input width
          ((4, 6), (9, 13)),            # general form: Wo % 4 != 0
          ((8, 12), (8, 12))]           # general form: the identity
MIN_TIED = 0.1


def _quantised(t):
    return (t * 4).round().clamp(-4, 4) / 4


def _seed(c, src, dst):
    return 1000 * c + src[0] * dst[1] + 10            # + 10: the first offset at which every case below has its tenth of tied pixels


def _logits(c, src, seed):
    (h, w), g = src, G(seed)
    cells = _quantised(0.2 * torch.randn(BATCH, c, -(-h // 2), -(-w // 3), generator=g))
    x = cells.repeat_interleave(2, 2).repeat_interleave(3, 3)[:, :, :h, :w]
    own = torch.rand(BATCH, 1, h, w, generator=g) < 0.1
    return torch.where(own, _quantised(0.2 * torch.randn(BATCH, c, h, w, generator=g)), x).contiguous()


def tied_fraction(logits):
    """Fraction of pixels of (B, C, H, W) host logits whose maximum over C is attained more than once."""
    top = logits.max(1, keepdims=True)
    return float(((logits == top).sum(1) >= 2).mean())


@functools.lru_cache(maxsize=None)
def _case(c, src, dst, kind):
    """(logits on the device, numpy.argmax masks of their upsample_bilinear): computed once per case and left unchanged."""
    from hyperseg_amd import functional as HF
    x = _logits(c, src, _seed(c, src, dst)) if kind == 'random' else torch.full((BATCH, c) + src, 0.25)
    x = x.to(DEV)
    up = HF.upsample_bilinear(x, dst).cpu().numpy()
    tied = tied_fraction(up)
    print(f'C={c} {src}->{dst} {kind}: tied maxima on {tied:.3f} of the output pixels')
    if kind == 'equal':
        assert tied == (1.0 if c > 1 else 0.0)
    elif c > 1:
        assert tied >= MIN_TIED, f'only {tied:.3f} of the output pixels have a tied maximum: choose another seed'
    want = torch.from_numpy(np.argmax(up, axis=1).astype(np.uint8))
    if kind == 'equal':
        assert not want.any()
    return x, want


def _targets(n, dst, seed, dtype):
    g = G(seed)
    t = torch.randint(0, n, (BATCH,) + dst, generator=g)
    t[torch.rand((BATCH,) + dst, generator=g) < 0.15] = 255
    return t.to(dtype)


def _stock(target, pred, n):
    from hyperseg_amd.fps import ConfusionMatrix
    cm = ConfusionMatrix(n)
    cm.update_stock(target.flatten().long(), pred.flatten().long())
    return cm.mat


@pytest.mark.parametrize('kind', ['random', 'equal'])
@pytest.mark.parametrize('src,dst', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('c', CLASSES)
def test_three_routes_give_numpy_first_occurrence_masks(c, src, dst, kind):
    from hyperseg_amd import Overlay
    from hyperseg_amd import functional as HF
    x, want = _case(c, src, dst, kind)
    n, seed = max(c, 2), _seed(c, src, dst)
    plain = HF.upsample_argmax(x, dst)
    assert plain.dtype == torch.uint8 and tuple(plain.shape) == (BATCH,) + dst
    assert torch.equal(plain.cpu(), want)
    for tdtype in (torch.int64, torch.uint8):
        target = _targets(n, dst, seed + 1, tdtype)
        assert bool((target == 255).any()) and bool((target != 255).any())
        mat, masks = HF.upsample_confusion(x, dst, target.to(DEV), n, masks=True)
        assert masks.dtype == torch.uint8 and torch.equal(masks, plain), tdtype
        assert torch.equal(mat.cpu(), _stock(target, want, n)), tdtype
    for layout in ('hwc', 'chw'):
        style = Overlay(torch.randint(0, 256, (n, 3), generator=G(seed + 2)), alpha=0.75, ignore_index=-1, layout=layout)
        frames = torch.randint(0, 256, (BATCH,) + dst + (3,), generator=G(seed + 3), dtype=torch.uint8)
        frames = frames if layout == 'hwc' else frames.permute(0, 3, 1, 2).contiguous()
        masks, over = HF.upsample_overlay(x, dst, frames.to(DEV), style)
        assert masks.dtype == torch.uint8 and torch.equal(masks, plain), layout
        assert over.dtype == torch.uint8 and torch.equal(over.cpu(), style.blend(frames, want)), layout
