"""utils/resample.py on the CPU: the coefficient and nearest tables and the CPU implementation of frame_resize / label_resize against
Pillow -- the recorded bytes of tests/golden/resample_ref.npz always, live Pillow as well where it is installed.  The results are uint8 from
integer arithmetic: every comparison is equality."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from hyperseg_amd.utils import resample as R

FILTERS = ('bilinear', 'bicubic')
# where floor((i + 0.5) in / out) is not Pillow's accumulated index
NEAREST_PINS = [((128, 256), (333, 777)), ((1024, 2048), (777, 1555)), ((64, 64), (23, 191))]


@pytest.fixture(scope='module')
def ref():
    return load_golden('resample_ref')


def _hwc(a):
    return a[None].contiguous()


def _chw(a):
    return a.permute(2, 0, 1)[None].contiguous()


def test_coefficient_tables_follow_the_restatement():
    b, kk = R.resample_coeffs(2048, 1024, 'bilinear')
    assert b.dtype == torch.int32 and kk.dtype == torch.int32 and tuple(b.shape) == (1024, 2) and tuple(kk.shape) == (1024, 5)
    q = 1 << 20                                           # weights 1/4, 3/4, 3/4, 1/4 of sum 2, normalised: 1/8, 3/8, 3/8, 1/8
    assert b[1].tolist() == [1, 4] and kk[1].tolist() == [q // 2, 3 * q // 2, 3 * q // 2, q // 2, 0]
    assert b[0].tolist() == [0, 3] and b[-1].tolist() == [2045, 3]
    assert R.resample_coeffs(40, 10, 'bicubic')[1].shape[1] == 17
    assert R.resample_coeffs(8, 64, 'bicubic')[1].shape[1] == 5 and R.resample_coeffs(64, 8, 'bicubic')[1].shape[1] == 33
    b, kk = R.resample_coeffs(7, 7, 'bicubic')            # the pass Pillow skips: the identity
    assert b.tolist() == [[i, 1] for i in range(7)] and kk.tolist() == [[1 << 22]] * 7
    assert R.resample_coeffs(37, 19, 'bicubic') is R.resample_coeffs(37, 19, 'bicubic')       # cached
    for f in FILTERS:
        for i, o in [(37, 19), (19, 37), (64, 8), (8, 64), (5, 1), (1, 5)]:
            b, kk = R.resample_coeffs(i, o, f)
            assert int(b[:, 0].min()) >= 0 and int(b[:, 1].min()) >= 1 and int((b[:, 0] + b[:, 1]).max()) <= i
            assert int(b[:, 1].max()) <= kk.shape[1]
            assert bool((kk.sum(1) - (1 << 22)).abs().max() <= kk.shape[1])          # rows sum to one, up to a unit per tap
    with pytest.raises(ValueError):
        R.resample_coeffs(8, 4, 'lanczos')
    with pytest.raises(ValueError):
        R.resample_coeffs(8, 0, 'bilinear')


def test_frames_equal_the_fixture(ref):
    for i, (hi, wi, ho, wo) in enumerate(ref['cases'].tolist()):
        x = ref[f'c{i}_in']
        assert tuple(x.shape) == (hi, wi, 3)
        for f in FILTERS:
            want = ref[f'c{i}_{f}']
            got = R.frame_resize_cpu(_hwc(x), (ho, wo), f, 'hwc')
            assert got.dtype == torch.uint8 and torch.equal(got[0], want), (i, f)
            got = R.frame_resize_cpu(_chw(x), (ho, wo), f, 'chw')
            assert torch.equal(got[0].permute(1, 2, 0), want), (i, f)


def test_labels_equal_the_fixture(ref):
    for i, (hi, wi, ho, wo) in enumerate(ref['label_cases'].tolist()):
        t, want = ref[f'l{i}_in'], ref[f'l{i}_out']
        assert torch.equal(R.label_resize_cpu(t[None], (ho, wo))[0], want)
        got = R.label_resize_cpu(t[None].long(), (ho, wo))
        assert got.dtype == torch.int64 and torch.equal(got[0], want.long())


def test_views_equal_the_fixture(ref):
    for i, (hi, wi, hr, wr, ho, wo, oy, ox, hflip, *fill) in enumerate(ref['view_cases'].tolist()):
        view = R.ResizeView((ho, wo), (oy, ox), bool(hflip), tuple(fill))
        got = R.frame_resize_cpu(_hwc(ref[f'v{i}_in']), (hr, wr), 'bicubic', 'hwc', view=view)
        assert torch.equal(got[0], ref[f'v{i}_bicubic']), i
        got = R.label_resize_cpu(ref[f'v{i}_label_in'][None], (hr, wr), view=view, fill=255)
        assert torch.equal(got[0], ref[f'v{i}_label']), i


def test_normalised_form_is_the_table_lookup():
    from hyperseg_amd import InputNorm
    x = torch.randint(0, 256, (2, 9, 8, 3), generator=torch.Generator().manual_seed(3), dtype=torch.uint8)
    view = R.ResizeView((7, 6), (-2, 1), True, (9, 8, 7))
    for layout in ('hwc', 'chw'):
        norm = InputNorm(layout=layout)
        src = x if layout == 'hwc' else x.permute(0, 3, 1, 2).contiguous()
        u8 = R.frame_resize_cpu(src, (5, 11), 'bicubic', layout, view=view)
        fl = R.frame_resize_cpu(src, (5, 11), 'bicubic', layout, view=view, norm=norm)
        assert fl.dtype == torch.float32 and tuple(fl.shape) == (2, 3, 7, 6)
        assert torch.equal(fl, norm.to_float(u8))


def test_frame_resize_class_on_cpu(ref):
    from hyperseg_amd import FrameResize
    hi, wi, ho, wo = ref['cases'][1].tolist()
    fr = FrameResize((ho, wo), 'bicubic', 'hwc')
    x = _hwc(ref['c1_in'])
    assert fr.applies_to(x) and not fr.applies_to(fr(x)) and not fr.applies_to(x.float())
    assert torch.equal(fr(x)[0], ref['c1_bicubic'])
    with pytest.raises(ValueError):
        FrameResize((0, 4))
    with pytest.raises(ValueError):
        FrameResize((4, 4), 'nearest')
    with pytest.raises(ValueError):
        FrameResize((4, 4), layout='nhwc')


def test_refusals_on_the_cpu():
    x = torch.zeros(1, 8, 8, 3, dtype=torch.uint8)
    with pytest.raises(ValueError):
        R.frame_resize_cpu(x.float(), (4, 4))
    with pytest.raises(ValueError):
        R.frame_resize_cpu(x, (4, 4), layout='chw')
    with pytest.raises(ValueError):
        R.frame_resize_cpu(x, (0, 4))
    with pytest.raises(ValueError):
        R.label_resize_cpu(torch.zeros(1, 8, 8), (4, 4))
    with pytest.raises(ValueError):
        R.frame_resize_cpu(x, (4, 4), view=R.ResizeView((0, 3)))


def test_nearest_table_is_the_accumulated_one_not_the_closed_form():
    """Pinned without Pillow: at these sizes the two tables differ on at least one axis (live Pillow below says which one is right)."""
    for (hi, wi), (ho, wo) in NEAREST_PINS:
        dy = int((R.nearest_index(hi, ho) != R.nearest_index_closed_form(hi, ho)).sum())
        dx = int((R.nearest_index(wi, wo) != R.nearest_index_closed_form(wi, wo)).sum())
        assert dy + dx > 0, ((hi, wi), (ho, wo))
        for i, o in ((hi, ho), (wi, wo)):
            idx = R.nearest_index(i, o)
            assert idx.dtype == torch.int32 and int(idx.min()) >= 0 and int(idx.max()) <= i - 1 and bool((idx[1:] >= idx[:-1]).all())


# ------------------------------------------------------------------------------------------------------------ live Pillow

def _pil():
    return pytest.importorskip('PIL.Image')


def test_frames_equal_live_pillow(ref):
    Image = _pil()
    pf = {'bilinear': Image.BILINEAR, 'bicubic': Image.BICUBIC}
    rng = np.random.default_rng(5)
    for i, (hi, wi, ho, wo) in enumerate(ref['cases'].tolist()):
        frames = [ref[f'c{i}_in'].numpy(), rng.integers(0, 256, (hi, wi, 3), dtype=np.uint8),
                  (rng.integers(0, 2, (hi, wi, 3)) * 255).astype(np.uint8), np.zeros((hi, wi, 3), np.uint8), np.full((hi, wi, 3), 255, np.uint8)]
        for a in frames:
            for f in FILTERS:
                want = torch.from_numpy(np.array(Image.fromarray(a).resize((wo, ho), pf[f])))
                assert torch.equal(R.frame_resize_cpu(torch.from_numpy(a)[None], (ho, wo), f)[0], want), (i, f)


def test_labels_equal_live_pillow_where_the_closed_form_fails(ref):
    Image = _pil()
    rng = np.random.default_rng(6)
    shapes = [((a, b), (c, d)) for a, b, c, d in ref['label_cases'].tolist()] + NEAREST_PINS
    for (hi, wi), (ho, wo) in shapes:
        # a label whose value names its own position, so that every wrong index shows
        t = ((np.arange(hi)[:, None] * 7 + np.arange(wi)[None, :] * 3) % 251).astype(np.uint8) if (hi, wi) != (1024, 2048) else \
            rng.integers(0, 256, (hi, wi), dtype=np.uint8)
        want = np.asarray(Image.fromarray(t).resize((wo, ho), Image.NEAREST))
        got = R.label_resize_cpu(torch.from_numpy(t)[None], (ho, wo))[0].numpy()
        assert (got == want).all(), ((hi, wi), (ho, wo))
        if ((hi, wi), (ho, wo)) in NEAREST_PINS:
            iy, ix = R.nearest_index_closed_form(hi, ho).numpy().astype(np.int64), R.nearest_index_closed_form(wi, wo).numpy().astype(np.int64)
            assert (t[iy][:, ix] != want).any(), 'the closed form agrees with Pillow here: the pin shows nothing'


def test_view_semantics_equal_pillow_paste_crop_transpose():
    Image = _pil()
    rng = np.random.default_rng(7)
    x, t = rng.integers(0, 256, (21, 34, 3), dtype=np.uint8), rng.integers(0, 19, (21, 34), dtype=np.uint8)
    views = [((13, 17), (-4, -5), False), ((13, 16), (-4, 30), True), ((40, 60), (-3, -2), True), ((6, 7), (5, 9), False),
             ((6, 7), (5, 9), True), ((4, 4), (100, 3), False), ((4, 5), (-9, -9), True), ((30, 8), (20, 40), True)]
    for hr, wr in [(11, 19), (42, 68), (21, 50)]:
        img = Image.fromarray(x).resize((wr, hr), Image.BICUBIC)
        lbl = Image.fromarray(t).resize((wr, hr), Image.NEAREST)
        for (ho, wo), (oy, ox), hflip in views:
            fill = (11, 22, 33)

            def pil_view(im, fill):
                top, left = max(-oy, 0), max(-ox, 0)
                canvas = Image.new(im.mode, (left + max(wr, ox + wo), top + max(hr, oy + ho)), fill)
                canvas.paste(im, (left, top))
                out = canvas.crop((ox + left, oy + top, ox + left + wo, oy + top + ho))
                return torch.from_numpy(np.array(out.transpose(Image.FLIP_LEFT_RIGHT) if hflip else out))
            view = R.ResizeView((ho, wo), (oy, ox), hflip, fill)
            assert torch.equal(R.frame_resize_cpu(torch.from_numpy(x)[None], (hr, wr), 'bicubic', view=view)[0], pil_view(img, fill))
            assert torch.equal(R.label_resize_cpu(torch.from_numpy(t)[None], (hr, wr), view=view, fill=255)[0], pil_view(lbl, 255))
