"""The VOC train chain for a ragged batch in a fixed number of launches (csrc/hs_augment_ragged.hip): ``training.BatchAugmentVOC`` on
the device against ``training.device_augment_voc`` of the cropped samples on CPU tensors -- the Pillow-exact chain tests/test_rotate_cpu.py
holds -- and the ragged launches one by one against the host's tables and the CPU jitter.  Integer and IEEE-float64 arithmetic
throughout: every comparison is ``torch.equal``, no tolerance appears here."""
import pytest
import torch

from conftest import G, load_golden
from hyperseg_amd.utils import resample as R
from test_voc_batch_augment_cpu import ANGLES, B, CANVAS, FILLS, FLIPS, PAD, SCALES, SETS, SIZES, canvas, crops, expected, jitters, make

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
JITTER_ARG = {None: lambda: None, 'contrast': lambda: jitters(True), 'plain': lambda: jitters(False)}


def on_dev(pair):
    return pair[0].to(DEV), pair[1].to(DEV)


@pytest.mark.parametrize('layout', ('hwc', 'chw'))
@pytest.mark.parametrize('label_dtype', (torch.uint8, torch.int64))
@pytest.mark.parametrize('jitter', (None, 'contrast', 'plain'))
def test_batch_equals_the_oracle(layout, label_dtype, jitter):
    frames, labels = on_dev(canvas(layout, label_dtype, garbage=1))
    aug = make(layout)
    img, lbl = aug(frames, labels, SIZES, FLIPS, JITTER_ARG[jitter](), SCALES, ANGLES)
    want_img, want_lbl = expected(layout, label_dtype, jitter)
    assert img.dtype == torch.float32 and tuple(img.shape) == (B, 3, PAD, PAD) and lbl.dtype == torch.int64 and tuple(lbl.shape) == (B, PAD, PAD)
    assert torch.equal(lbl.cpu(), want_lbl)
    assert torch.equal(img.cpu(), want_img)
    assert not bool(aug.status.any())
    if jitter is not None:
        assert not torch.equal(want_img, expected(layout, label_dtype)[0])


def test_a_list_of_ragged_samples_on_the_device():
    frames, labels = canvas('chw', torch.int64)
    xs, ts = crops(frames, labels, SIZES, 'chw')
    img, lbl = make('chw')([x.to(DEV) for x in xs], [t.to(DEV) for t in ts], None, FLIPS, None, SCALES, ANGLES)
    want_img, want_lbl = expected('chw', torch.int64)
    assert torch.equal(img.cpu(), want_img) and torch.equal(lbl.cpu(), want_lbl)


@pytest.mark.parametrize('layout', ('hwc', 'chw'))
def test_canvas_padding_is_never_read(layout):
    """Everything outside the extents is random bytes, two different fills of it: the results equal each other and the oracle, with the
    contrast mean (a sum over the image) among the operations."""
    got = []
    for garbage in (1, 2):
        frames, labels = on_dev(canvas(layout, torch.uint8, garbage=garbage))
        got.append(make(layout)(frames, labels, SIZES, FLIPS, jitters(True), SCALES, ANGLES))
    assert not torch.equal(canvas(layout, torch.uint8, 1)[0], canvas(layout, torch.uint8, 2)[0])
    assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1])
    want_img, want_lbl = expected(layout, torch.uint8, 'contrast')
    assert torch.equal(got[0][0].cpu(), want_img) and torch.equal(got[0][1].cpu(), want_lbl)


def test_the_flip_mirrors_the_source():
    """A flipped sample at the exact 2:1 reduction (tests/test_rotate_cpu.py::test_resize_then_flip_is_not_the_reference_label's case):
    Pillow's NEAREST table is not mirror-symmetric, so the result is the oracle's flip-then-resize and NOT resize-then-flip."""
    from hyperseg_amd import InputNorm
    from hyperseg_amd.training import BatchAugmentVOC, device_augment_voc
    ref = load_golden('rotate_ref')
    x, t = ref['k1_in'], ref['k1_label_in']                                  # (60, 80, 3), (60, 80)
    norm = InputNorm(layout='hwc')
    frames = torch.randint(0, 256, (2, 64, 88, 3), generator=G(5200), dtype=torch.uint8)
    labels = torch.randint(0, 256, (2, 64, 88), generator=G(5201), dtype=torch.uint8)
    frames[:, :60, :80], labels[:, :60, :80] = x, t
    aug = BatchAugmentVOC((64, 88), 64, norm, **FILLS)
    img, lbl = aug(frames.to(DEV), labels.to(DEV), [(60, 80)] * 2, [True, False], None, 0.5, 0.0)
    want_img, want_lbl = device_augment_voc([x, x], [t, t], [True, False], None, 0.5, 0.0, 64, norm, **FILLS)
    assert torch.equal(img.cpu(), want_img) and torch.equal(lbl.cpu(), want_lbl)
    assert torch.equal(lbl[0, :30, :40].cpu(), R.label_resize_cpu(t[None].flip(2), (30, 40))[0].long())
    assert not torch.equal(lbl[0, :30, :40], lbl[1, :30, :40].flip(1))       # resize-then-flip is another label


@pytest.mark.parametrize('filter', R.FILTERS)
def test_ragged_tables_equal_the_hosts(filter):
    """Mixed input sizes in one launch, in == out among them (one axis, both axes), a one-pixel image, the extreme rows of the canvas:
    ``utils.resample.window_tables_cpu`` integer for integer, rows past the resized size empty."""
    from hyperseg_amd import functional as HF
    canvas_hw, mid = (97, 120), (64, 80)
    rows = [(97, 120, 24, 30), (97, 120, 64, 80), (50, 64, 50, 64), (50, 64, 50, 17), (33, 120, 9, 80), (1, 1, 1, 1), (1, 7, 1, 2), (96, 119, 61, 79),
            (13, 29, 64, 80), (97, 3, 25, 1)]
    ks_max = max(min(R.ksize_of(i, o, filter), i) for r in rows for i, o in ((r[0], r[2]), (r[1], r[3])))
    params = torch.tensor([r + (i & 1, 0, 0, 0) for i, r in enumerate(rows)], dtype=torch.int32).to(DEV)
    t = HF.resize_tables_ragged(params, canvas_hw, mid, filter, ks_max)
    m = max(mid)
    assert tuple(t.bounds.shape) == (len(rows), 2, m, 2) and tuple(t.kk.shape) == (len(rows), 2, m, ks_max) and tuple(t.nearest.shape) == (len(rows), 2, m)
    assert not bool(t.status.any())
    bounds, kk, nearest = t.bounds.cpu(), t.kk.cpu(), t.nearest.cpu()
    for i, r in enumerate(rows):
        for axis in (0, 1):
            size_in, size_out = r[axis], r[2 + axis]
            b, k = R.resample_coeffs(size_in, size_out, filter)
            want_b, want_k = torch.zeros(m, 2, dtype=torch.int32), torch.zeros(m, ks_max, dtype=torch.int32)
            want_n = torch.zeros(m, dtype=torch.int32)
            want_b[:size_out] = b
            taps = min(k.shape[1], ks_max)                                   # a row holds at most `in` taps: the columns beyond are zero
            assert not bool(k[:, taps:].any())
            want_k[:size_out, :taps] = k[:, :taps]
            want_n[:size_out] = R.nearest_index(size_in, size_out)
            assert torch.equal(bounds[i, axis], want_b), (i, axis)
            assert torch.equal(kk[i, axis], want_k), (i, axis)
            assert torch.equal(nearest[i, axis], want_n), (i, axis)
            if k.shape[1] <= ks_max:                                         # the layout's own oracle, where it accepts the pair
                w = R.window_tables_cpu(size_in, size_out, 0, m, filter, ks_max)
                assert torch.equal(bounds[i, axis], w.bounds) and torch.equal(kk[i, axis], w.kk) and torch.equal(nearest[i, axis], w.nearest)
    ident = kk[2]                                                            # in == out: one tap of 2^22, the identity index
    assert bool((ident[0, :50, 0] == 1 << 22).all()) and not bool(ident[0, :, 1:].any()) and nearest[2, 1, :64].tolist() == list(range(64))


@pytest.mark.parametrize('layout', ('hwc', 'chw'))
def test_ragged_contrast_mean_is_the_regions(layout):
    """Contrast against a canvas whose padding is 255 everywhere: the mean is the cropped frame's, the region holds
    ``utils.jitter.color_jitter_cpu`` of the crop, what lies outside is not written."""
    from hyperseg_amd import functional as HF
    from hyperseg_amd.utils import jitter as J
    from hyperseg_amd.utils.jitter import ColorJitterParams
    hm, wm = CANVAS
    frames = torch.full((B, hm, wm, 3), 255, dtype=torch.uint8)
    dark = torch.randint(0, 90, (B, hm, wm, 3), generator=G(5300), dtype=torch.uint8)
    for i, (h, w) in enumerate(SIZES):
        frames[i, :h, :w] = dark[i, :h, :w]
    if layout == 'chw':
        frames = frames.permute(0, 3, 1, 2).contiguous()
    params = [ColorJitterParams(('contrast',), contrast=0.5), ColorJitterParams(('brightness', 'contrast'), brightness=1.4, contrast=1.7),
              ColorJitterParams(('hue', 'contrast', 'saturation'), hue=0.2, contrast=0.3, saturation=1.5), ColorJitterParams(('saturation',), saturation=0.4),
              ColorJitterParams(()), ColorJitterParams(('contrast', 'hue'), contrast=1.2, hue=-0.4)]
    rows = torch.tensor([s + s + (0, 0, 0, 0) for s in SIZES], dtype=torch.int32).to(DEV)
    out = torch.full(frames.shape, 77, dtype=torch.uint8, device=DEV)
    got = HF.color_jitter_ragged(frames.to(DEV), rows, J.params_table(params, B).to(DEV), layout, out=out).cpu()
    for i, (h, w) in enumerate(SIZES):
        crop = frames[i:i + 1, :h, :w] if layout == 'hwc' else frames[i:i + 1, :, :h, :w]
        region = got[i:i + 1, :h, :w] if layout == 'hwc' else got[i:i + 1, :, :h, :w]
        assert torch.equal(region, J.color_jitter_cpu(crop.contiguous(), params[i], layout)), i
        outside = torch.ones(hm, wm, dtype=torch.bool)
        outside[:h, :w] = False
        assert bool(((got[i] if layout == 'hwc' else got[i].permute(1, 2, 0))[outside] == 77).all())
    whole = J.color_jitter_cpu(frames[1:2], params[1], layout)               # the mean over the whole canvas is another image
    assert not torch.equal(got[1:2, :33, :47] if layout == 'hwc' else got[1:2, :, :33, :47], whole[:, :33, :47] if layout == 'hwc' else whole[:, :, :33, :47])


COUNTED = ('hs_frame_resize_fwd', 'hs_label_resize_fwd', 'hs_resize_tables_fwd', 'hs_frame_resize_batch_fwd', 'hs_label_resize_batch_fwd',
           'hs_color_jitter_fwd', 'hs_frame_rotate_fwd', 'hs_label_rotate_fwd', 'hs_resize_tables_ragged_fwd', 'hs_color_jitter_ragged_fwd',
           'hs_frame_resize_ragged_fwd', 'hs_label_resize_ragged_fwd', 'hs_frame_rotate_ragged_fwd', 'hs_label_rotate_ragged_fwd')
SUMS_ARG = {'hs_color_jitter_fwd': 6, 'hs_color_jitter_ragged_fwd': 7}       # these entries launch a clear and a mean pass too when it is given


def count_launches(fn):
    """Launches made through the COUNTED library entries while ``fn`` runs, counted at the ctypes boundary -- in both namespaces of the
    binding, the checked entries the wrappers call (``_hip.run``) and the raw ones (``_hip.lib``): every entry makes one, the two jitter
    entries three when they are handed a sums workspace (include/hyperseg_hip.h)."""
    from hyperseg_amd import _hip
    counts, saved = {}, []
    for space in (_hip.run, _hip.lib):
        for name in COUNTED:
            real = getattr(space, name)
            saved.append((space, name, real))

            def counting(*a, _real=real, _name=name):
                counts[_name] = counts.get(_name, 0) + (3 if _name in SUMS_ARG and a[SUMS_ARG[_name]] is not None else 1)
                return _real(*a)
            setattr(space, name, counting)
    try:
        fn()
    finally:
        for space, name, real in saved:
            setattr(space, name, real)
    return counts


@pytest.mark.parametrize('batch', (2, 6))
def test_launch_counts_do_not_depend_on_the_batch(batch):
    frames, labels = on_dev(canvas('hwc', torch.uint8))
    frames, labels = frames[:batch].contiguous(), labels[:batch].contiguous()
    args = (SIZES[:batch], FLIPS[:batch]), (SCALES[:batch], ANGLES[:batch])
    aug = make('hwc')
    for jitter, want in ((None, 5), (jitters(False)[:batch], 6), (jitters(True)[:batch], 8)):
        counts = count_launches(lambda: aug(frames, labels, *args[0], jitter, *args[1]))
        assert sum(counts.values()) == want, counts
        assert all(name.endswith('_ragged_fwd') for name in counts), counts


def test_captured_run_replays_with_new_parameters():
    """``run`` with the three jitter launches captured once, replayed with three parameter sets -- extents, flips, scales, angles and jitter
    records (the second set without jitter: records of zeros) -- equals the oracle each time; nothing is built or cached on the host."""
    tables_before = len(R._DEVICE_TABLES)
    layout = 'hwc'
    frames, labels = on_dev(canvas(layout, torch.uint8))
    aug = make(layout)
    aug(frames, labels, SIZES, FLIPS, jitters(True), SCALES, ANGLES)         # makes the buffers; first launches of every kernel
    out = (torch.zeros(B, 3, PAD, PAD, device=DEV), torch.zeros(B, PAD, PAD, dtype=torch.int64, device=DEV))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                            # one stream: a linear graph
        aug.run(frames, labels, out=out, jitter=True)
    for which, jitter in ((0, 'contrast'), (1, None), (2, 'plain'), (0, 'contrast')):
        sizes, flips, scales, angles = SETS[which]
        aug.upload(aug.rows(sizes, flips, JITTER_ARG[jitter](), scales, angles))
        graph.replay()
        torch.cuda.synchronize()
        want_img, want_lbl = expected(layout, torch.uint8, jitter, which)
        assert torch.equal(out[1].cpu(), want_lbl), which
        assert torch.equal(out[0].cpu(), want_img), which
        assert not bool(aug.status.any())
    assert len(R._DEVICE_TABLES) == tables_before


def test_status_declines_a_sample_and_leaves_the_others():
    from hyperseg_amd import functional as HF
    layout = 'hwc'
    frames, labels = on_dev(canvas(layout, torch.uint8))
    aug = make(layout)
    aug(frames, labels, SIZES, FLIPS, None, SCALES, ANGLES)
    good = aug.rows(SIZES, FLIPS, jitters(True), SCALES, ANGLES)
    rows = good.rows.clone()
    rows[0, 0] = CANVAS[0] + 1                                               # the extent exceeds the canvas
    rows[2, 3] = PAD + 1                                                     # the resized size exceeds the intermediate canvas
    rows[3, 1] = 0                                                           # an empty extent
    rows[4, 2] = 0                                                           # Hr = 0
    aug.upload(good._replace(rows=rows))
    img, lbl = aug.run(frames, labels, jitter=True)
    S = HF.RAGGED_STATUS
    assert aug.status.tolist() == [S['extent'], 0, S['canvas'], S['extent'], S['hr'], 0]
    want_img, want_lbl = expected(layout, torch.uint8, 'contrast')
    table = aug.norm.table('cpu')
    fill_img = torch.stack([table[c, v] for c, v in enumerate(FILLS['fill'])]).view(3, 1, 1).expand(3, PAD, PAD)
    for i in range(B):
        if i in (0, 2, 3, 4):                                                # all pad fill
            assert torch.equal(img[i].cpu(), fill_img) and bool((lbl[i] == FILLS['lbl_fill']).all())
        else:                                                                # unaffected
            assert torch.equal(img[i].cpu(), want_img[i]) and torch.equal(lbl[i].cpu(), want_lbl[i])
    t = aug.tables
    assert not bool(t.bounds[[0, 2, 3, 4]].any()) and not bool(t.kk[[0, 2, 3, 4]].any()) and not bool(t.nearest[[0, 2, 3, 4]].any())
    # more taps than the rows hold
    small = HF.resize_tables_ragged(torch.tensor([[40, 56, 10, 14, 0, 0, 0, 0], [40, 56, 36, 50, 0, 0, 0, 0]], dtype=torch.int32).to(DEV),
                                    CANVAS, (PAD, PAD), 'bicubic', 9)
    assert small.status.tolist() == [S['y_taps'] | S['x_taps'], 0]


def test_refusals_on_the_device():
    from hyperseg_amd import functional as HF
    frames, labels = on_dev(canvas('hwc', torch.uint8))
    aug = make('hwc')
    with pytest.raises(ValueError, match='exceeds pad'):
        make('hwc', scale_range=(0.25, 2.0))(frames, labels, SIZES, FLIPS, None, [2.0] + SCALES[1:], ANGLES)
    with pytest.raises(ValueError, match='scale_range'):
        aug(frames, labels, SIZES, FLIPS, None, [0.95] + SCALES[1:], ANGLES)
    with pytest.raises(ValueError):
        aug(frames, labels, SIZES[:5], FLIPS, None, SCALES, ANGLES)          # mismatched counts
    with pytest.raises(ValueError):
        aug(frames, labels.float(), SIZES, FLIPS, None, SCALES, ANGLES)      # wrong dtype
    with pytest.raises(ValueError):
        aug(frames, labels.cpu(), SIZES, FLIPS, None, SCALES, ANGLES)        # wrong device
    assert aug.tables is None                                                # refused before anything was made or launched
    aug(frames, labels, SIZES, FLIPS, None, SCALES, ANGLES)
    p, t = aug.params, aug.tables
    with pytest.raises(ValueError):
        HF.resize_tables_ragged(p.rows[:, :6].contiguous(), CANVAS, (PAD, PAD), 'bicubic', aug.ks_max)
    with pytest.raises(ValueError):
        HF.resize_tables_ragged(p.rows, CANVAS, (PAD, PAD), 'lanczos', aug.ks_max)
    with pytest.raises(ValueError):
        HF.resize_tables_ragged(p.rows, CANVAS, (PAD, PAD), 'bicubic', aug.ks_max, workspace=torch.zeros(10, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError):
        HF.frame_resize_ragged(frames[:4].contiguous(), p.rows, t, 'hwc')
    with pytest.raises(ValueError):
        HF.frame_resize_ragged(frames[:, :39].contiguous(), p.rows, t, 'hwc')            # not the canvas the tables were built for
    with pytest.raises(ValueError):
        HF.label_resize_ragged(labels.float(), p.rows, t)
    with pytest.raises(ValueError):
        HF.color_jitter_ragged(frames, p.rows, p.jitter[:, :6].contiguous(), 'hwc')
    with pytest.raises(ValueError):
        HF.frame_rotate_ragged(aug._mid, p.rows, t, p.matrices.float(), 'hwc')
    with pytest.raises(ValueError):
        HF.label_rotate_ragged(aug._mid_label.long(), p.rows, t, p.fixed)
