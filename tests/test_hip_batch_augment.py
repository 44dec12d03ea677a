"""A training batch augmented in three launches (csrc/hs_resample_batch.hip): the device-built resize tables against the host's
(``utils.resample.window_tables_cpu``, i.e. slices of ``resample_coeffs`` / ``nearest_index``), integer for integer, and
``training.BatchAugment`` against ``training.device_augment`` on the CPU copies -- the Pillow-exact chain tests/test_resample_cpu.py and
tests/test_hip_resample.py hold.  Integer work from bit-exact tables: every comparison is ``torch.equal``, no tolerance appears here."""
import functools

import numpy as np
import pytest
import torch

from conftest import G
from hyperseg_amd.utils import resample as R
from test_batch_augment_cpu import CROP, FLIPS, IN_HW, JITTERS, OFFSETS, SCALES, batch

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


def host_tables(in_hw, crop, rows, filter, ks_max):
    """What hs_resize_tables_fwd must write for ``rows`` (Hr, Wr, oy, ox, ...): (bounds, kk, nearest) stacked (B, 2, M, ...)."""
    m = max(crop)
    bounds = torch.zeros(len(rows), 2, m, 2, dtype=torch.int32)
    kk = torch.zeros(len(rows), 2, m, ks_max, dtype=torch.int32)
    nearest = torch.zeros(len(rows), 2, m, dtype=torch.int32)
    for i, row in enumerate(rows):
        for axis in (0, 1):
            w = R.window_tables_cpu(in_hw[axis], row[axis], row[2 + axis], crop[axis], filter, ks_max)
            bounds[i, axis, :crop[axis]], kk[i, axis, :crop[axis]], nearest[i, axis, :crop[axis]] = w
    return bounds, kk, nearest


def check_tables(in_hw, crop, rows, filter, ks_max):
    from hyperseg_amd import functional as HF
    params = torch.tensor(rows, dtype=torch.int32).to(DEV)
    t = HF.resize_tables(params, in_hw, crop, filter, ks_max)
    bounds, kk, nearest = host_tables(in_hw, crop, rows, filter, ks_max)
    assert not bool(t.status.any())
    assert torch.equal(t.bounds.cpu(), bounds)
    assert torch.equal(t.kk.cpu(), kk)
    assert torch.equal(t.nearest.cpu(), nearest)


@pytest.mark.parametrize('filter', R.FILTERS)
def test_tables_97_to_every_size(filter):
    """in = 97 against every out in 12..200 (97 itself, the identity pass, among them), the whole resized axis in the window; both axes
    of a row carry a pair of their own, 189 rows in one launch."""
    rows = [(out, 212 - out, 0, 0, 0, 0) for out in range(12, 201)]
    check_tables((97, 97), (200, 200), rows, filter, R.ksize_of(97, 12, filter))


@pytest.mark.parametrize('filter', R.FILTERS)
def test_tables_identity(filter):
    rows = [(48, 96, 0, 0, 0, 0), (48, 96, -5, 40, 1, 0), (48, 97, 30, -3, 0, 0), (50, 96, 0, 90, 0, 0)]
    check_tables((48, 96), (32, 64), rows, filter, 7)


@pytest.mark.parametrize('filter', R.FILTERS)
def test_tables_seeded_scales_at_camera_size(filter):
    """64 seeded scales in [0.25, 2.0] at in = 1024 (y) and 2048 (x), 64-wide windows that straddle the near edge, the far edge, or lie
    inside (the serial nearest chain then starts thousands of indices before the window)."""
    scales = torch.empty(64, dtype=torch.float64).uniform_(0.25, 2.0, generator=G(4200)).tolist()
    rows = []
    for i, s in enumerate(scales):
        hr, wr = (int(v) for v in np.round(np.array((1024, 2048)) * s).astype(int))
        oy = (-32, hr - 32, hr // 2, -63)[i % 4]
        ox = (wr - 1, wr // 3, -17, wr - 40)[i % 4]
        rows.append((hr, wr, oy, ox, i & 1, 0))
    check_tables((1024, 2048), (64, 64), rows, filter, R.ks_for(filter, 0.25))


@functools.lru_cache(maxsize=None)
def expected(layout, label_dtype, with_jitter=False):
    """``device_augment`` of the shared batch on CPU tensors; computed once, never written to."""
    from hyperseg_amd import InputNorm
    from hyperseg_amd.training import device_augment
    frames, labels = batch(layout, label_dtype)
    return device_augment(frames, labels, SCALES, CROP, OFFSETS, FLIPS, InputNorm(layout=layout), lbl_fill=255, fill=(7, 8, 9),
                          jitter=JITTERS if with_jitter else None)


@pytest.mark.parametrize('layout', ('hwc', 'chw'))
@pytest.mark.parametrize('label_dtype', (torch.uint8, torch.int64))
def test_batch_equals_per_sample_route(layout, label_dtype):
    from hyperseg_amd import InputNorm
    from hyperseg_amd.training import BatchAugment
    frames, labels = batch(layout, label_dtype)
    aug = BatchAugment(IN_HW, CROP, InputNorm(layout=layout), (0.25, 2.0), lbl_fill=255, fill=(7, 8, 9))
    img, lbl = aug(frames.to(DEV), labels.to(DEV), SCALES, OFFSETS, FLIPS)
    want_img, want_lbl = expected(layout, label_dtype)
    assert img.dtype == torch.float32 and tuple(img.shape) == (6, 3) + CROP and lbl.dtype == torch.int64 and tuple(lbl.shape) == (6,) + CROP
    assert torch.equal(img.cpu(), want_img) and torch.equal(lbl.cpu(), want_lbl)
    assert not bool(aug.status.any())
    for i in (0, 1):                                                         # padding is present in the down-scaled samples
        assert bool((lbl[i] == 255).any()) and bool((lbl[i] != 255).any())
    # the uint8 form of the frame launch, in the input's layout
    from hyperseg_amd import functional as HF
    u8 = HF.frame_resize_batch(frames.to(DEV), aug.params, aug.tables, layout, fill=(7, 8, 9))
    for i, (hr, wr, oy, ox, flip, _) in enumerate(aug.rows(SCALES, OFFSETS, FLIPS).tolist()):
        view = R.ResizeView(CROP, (oy, ox), bool(flip), (7, 8, 9))
        assert torch.equal(u8[i:i + 1].cpu(), R.frame_resize_cpu(frames[i:i + 1], (hr, wr), 'bicubic', layout, view=view))


@pytest.mark.parametrize('layout', ('hwc', 'chw'))
def test_batch_with_jitter_equals_per_sample_route(layout):
    from hyperseg_amd import InputNorm
    from hyperseg_amd.training import BatchAugment
    frames, labels = batch(layout, torch.uint8)
    aug = BatchAugment(IN_HW, CROP, InputNorm(layout=layout), (0.25, 2.0), lbl_fill=255, fill=(7, 8, 9))
    img, lbl = aug(frames.to(DEV), labels.to(DEV), SCALES, OFFSETS, FLIPS, jitter=JITTERS)
    want_img, want_lbl = expected(layout, torch.uint8, True)
    assert torch.equal(img.cpu(), want_img) and torch.equal(lbl.cpu(), want_lbl)
    assert not torch.equal(want_img, expected(layout, torch.uint8)[0])


@pytest.mark.parametrize('filter', R.FILTERS)
def test_register_taps_and_loop_in_one_launch(filter):
    """Up-scaling by 2 (bicubic: 5 taps, the weights in registers) and down-scaling to 1/4 (17 taps, the loop) in the same launch, on
    frames of 0 and 255 only, where the overshoot of the bicubic weights makes clip8 decide bytes in both passes."""
    from hyperseg_amd import InputNorm
    from hyperseg_amd.training import BatchAugment
    norm = InputNorm(layout='hwc')
    frames = torch.randint(0, 2, (4, 48, 96, 3), generator=G(4300), dtype=torch.uint8) * 255
    labels = torch.randint(0, 19, (4, 48, 96), generator=G(4301), dtype=torch.uint8)
    scales, offsets, flips = [2.0, 0.25, 0.25, 2.0], [(10, 100), (-4, -8), (0, 0), (70, 130)], [False, True, False, True]
    aug = BatchAugment(IN_HW, CROP, norm, (0.25, 2.0), filter=filter)
    img, lbl = aug(frames.to(DEV), labels.to(DEV), scales, offsets, flips)
    want_img, want_lbl = aug(frames, labels, scales, offsets, flips)          # CPU tensors: utils.resample's implementation
    assert torch.equal(img.cpu(), want_img) and torch.equal(lbl.cpu(), want_lbl)
    if filter == 'bicubic':
        from hyperseg_amd.training import device_augment
        ref = device_augment(frames, labels, scales, CROP, offsets, flips, norm)
        assert torch.equal(want_img, ref[0]) and torch.equal(want_lbl, ref[1])
        table = norm.table('cpu')
        assert bool((want_img[0, 0] == table[0, 0]).any()) and bool((want_img[0, 0] == table[0, 255]).any())      # both clips occur


def test_captured_run_replays_with_new_parameters():
    from hyperseg_amd import InputNorm
    from hyperseg_amd.training import BatchAugment
    tables_before = len(R._DEVICE_TABLES)
    layout = 'hwc'
    norm = InputNorm(layout=layout)
    frames, labels = batch(layout, torch.uint8)
    frames_dev, labels_dev = frames.to(DEV), labels.to(DEV)
    aug = BatchAugment(IN_HW, CROP, norm, (0.25, 2.0), lbl_fill=255, fill=(7, 8, 9))
    sets = [(SCALES, OFFSETS, FLIPS), (SCALES[::-1], OFFSETS, FLIPS[::-1]), ([0.3, 0.77, 1.9, 1.0, 0.25, 1.5], OFFSETS[::-1], FLIPS)]
    eager = [tuple(t.clone() for t in aug(frames_dev, labels_dev, *s)) for s in sets]
    for (img, lbl), s in zip(eager, sets):                                   # the eager results are the CPU chain's
        from hyperseg_amd.training import device_augment
        want = device_augment(frames, labels, s[0], CROP, s[1], s[2], norm, lbl_fill=255, fill=(7, 8, 9))
        assert torch.equal(img.cpu(), want[0]) and torch.equal(lbl.cpu(), want[1])
    out = (torch.zeros(6, 3, *CROP, device=DEV), torch.zeros(6, *CROP, dtype=torch.int64, device=DEV))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                            # one stream: a linear graph of three kernel nodes
        aug.run(frames_dev, labels_dev, out=out)
    for (img, lbl), s in zip(eager, sets):
        aug.params.copy_(aug.rows(*s).to(DEV))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out[0], img) and torch.equal(out[1], lbl)
        assert not bool(aug.status.any())
    assert len(R._DEVICE_TABLES) == tables_before


def test_refusals_and_status():
    from hyperseg_amd import InputNorm
    from hyperseg_amd import functional as HF
    from hyperseg_amd.training import BatchAugment
    layout = 'hwc'
    norm = InputNorm(layout=layout)
    frames, labels = batch(layout, torch.uint8)
    frames_dev, labels_dev = frames.to(DEV), labels.to(DEV)
    aug = BatchAugment(IN_HW, CROP, norm, (0.5, 2.0), lbl_fill=255, fill=(7, 8, 9))
    assert aug.ks_max == 9
    with pytest.raises(ValueError, match='scale_range'):
        aug(frames_dev, labels_dev, [1.0, 1.0, 0.25, 1.0, 1.0, 1.0], (0, 0), False)
    assert aug.tables is None                                                # refused before anything was made or launched
    scales = [0.5, 0.5, 1.0, 1.01, 1.37, 2.0]
    good = aug.rows(scales, OFFSETS, FLIPS)
    rows = good.clone()
    rows[1, 0] = 0                                                           # Hr = 0
    rows[3, :2] = torch.tensor([12, 24])                                     # 17 taps on both axes, ks_max is 9
    rows[4, 1] = -3                                                          # Wr < 1
    img, lbl = aug.run(frames_dev, labels_dev, params=rows.to(DEV))
    S = HF.RESIZE_STATUS
    assert aug.status.tolist() == [0, S['hr'], 0, S['y_taps'] | S['x_taps'], S['wr'], 0]
    want_img, want_lbl = aug.run(frames, labels, params=good)                # CPU tensors
    table = norm.table('cpu')
    fill_img = torch.stack([table[c, v] for c, v in enumerate((7, 8, 9))]).view(3, 1, 1).expand(3, *CROP)
    for i in range(6):
        if i in (1, 3, 4):                                                   # all fill
            assert torch.equal(img[i].cpu(), fill_img) and bool((lbl[i] == 255).all())
        else:                                                                # unaffected
            assert torch.equal(img[i].cpu(), want_img[i]) and torch.equal(lbl[i].cpu(), want_lbl[i])
    t = aug.tables
    assert not bool(t.bounds[[1, 3, 4]].any()) and not bool(t.kk[[1, 3, 4]].any()) and not bool(t.nearest[[1, 3, 4]].any())
    # wrapper refusals
    with pytest.raises(ValueError):
        HF.resize_tables(rows.to(DEV)[:, :5].contiguous(), IN_HW, CROP, 'bicubic', 9)
    with pytest.raises(ValueError):
        HF.resize_tables(rows.to(DEV), IN_HW, CROP, 'lanczos', 9)
    with pytest.raises(ValueError):
        HF.resize_tables(rows.to(DEV), IN_HW, CROP, 'bicubic', 9, workspace=torch.zeros(10, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError):
        HF.frame_resize_batch(frames_dev[:4], rows.to(DEV), t, layout)
    with pytest.raises(ValueError):
        HF.label_resize_batch(labels_dev.float(), rows.to(DEV), t)
