"""The host side of the batched augmentation: ``utils.resample.window_tables_cpu`` (the oracle of the device-built tables) against slices
of ``resample_coeffs`` / ``nearest_index``, ``ks_for`` against ``resample_coeffs``' own row width, and ``training.BatchAugment`` on CPU
tensors against ``training.device_augment`` on CPU tensors.  Integers and bytes from stated arithmetic: every comparison is exact."""
import pytest
import torch

from conftest import G
from hyperseg_amd.utils import jitter as J
from hyperseg_amd.utils import resample as R

# the batch of tests/test_hip_batch_augment.py: 48x96 frames, crop (32, 64)
IN_HW, CROP = (48, 96), (32, 64)
SCALES = [0.25, 0.5, 1.0, 1.01, 1.37, 2.0]                     # 1.0 skips both passes; 1.01 gives 48x97: one pass skipped
OFFSETS = [(-10, -20), (-5, 3), (8, 16), (20, 40), (40, -7), (70, 150)]      # before the image, interior, past the far edge
FLIPS = [True, False, True, False, False, True]
P = J.ColorJitterParams
B_, C_, S_, H_ = J.OPS
JITTERS = [P((B_, C_, S_, H_), 0.8, 1.25, 0.75, 0.1), P((H_, S_, C_, B_), 1.25, 0.5, 1.5, -0.2), P((C_, B_, H_, S_), 1.1, 0.9, 1.2, 0.3),
           P((S_, H_, B_, C_), 0.9, 1.4, 0.6, -0.4), P((B_, S_, C_, H_), 1.2, 0.7, 1.3, 0.25), P((H_, C_, S_, B_), 0.7, 1.1, 0.8, -0.05)]


def batch(layout='hwc', label_dtype=torch.uint8):
    frames = torch.randint(0, 256, (6,) + IN_HW + (3,), generator=G(4100), dtype=torch.uint8)
    labels = torch.randint(0, 19, (6,) + IN_HW, generator=G(4101), dtype=torch.uint8).to(label_dtype)
    return (frames if layout == 'hwc' else frames.permute(0, 3, 1, 2).contiguous()), labels


@pytest.mark.parametrize('filter', R.FILTERS)
@pytest.mark.parametrize('in_size,out_size', [(97, 12), (97, 60), (97, 97), (97, 200), (48, 97)])
def test_window_tables_are_slices_of_the_host_tables(in_size, out_size, filter):
    bounds, kk = R.resample_coeffs(in_size, out_size, filter)
    near = R.nearest_index(in_size, out_size)
    ks = kk.shape[1]
    for start, extent in [(0, out_size), (3, 5), (-7, 20), (out_size - 4, 11), (-3, out_size + 9), (-30, 10), (out_size + 2, 6)]:
        for ks_max in (ks, ks + 3):
            w = R.window_tables_cpu(in_size, out_size, start, extent, filter, ks_max)
            assert w.bounds.dtype == w.kk.dtype == w.nearest.dtype == torch.int32
            assert tuple(w.bounds.shape) == (extent, 2) and tuple(w.kk.shape) == (extent, ks_max) and tuple(w.nearest.shape) == (extent,)
            for j in range(extent):
                r = start + j
                if 0 <= r < out_size:
                    assert torch.equal(w.bounds[j], bounds[r]) and torch.equal(w.kk[j, :ks], kk[r]) and int(w.nearest[j]) == int(near[r])
                    assert not bool(w.kk[j, ks:].any())
                else:
                    assert not bool(w.bounds[j].any()) and not bool(w.kk[j].any()) and int(w.nearest[j]) == 0
    with pytest.raises(ValueError):
        R.window_tables_cpu(in_size, out_size, 0, 0, filter, ks)
    if ks > 1:
        with pytest.raises(ValueError):
            R.window_tables_cpu(in_size, out_size, 0, 4, filter, ks - 1)


@pytest.mark.parametrize('filter', R.FILTERS)
def test_ks_for_is_the_row_width_at_the_lower_end(filter):
    # ranges whose lower end resizes these sizes by an exact ratio; above 1 the filter is not stretched
    for in_size, min_scale in [(1024, 0.375), (2048, 0.375), (48, 0.25), (96, 0.25), (1000, 0.5), (512, 1.5), (300, 0.1), (97, 2.0)]:
        out = int(round(in_size * min_scale))
        ksize = R.resample_coeffs(in_size, out, filter)[1].shape[1]
        assert R.ks_for(filter, min_scale) == ksize and R.ksize_of(in_size, out, filter) == ksize
    assert R.ksize_of(64, 64, filter) == 1
    assert R.ks_for(filter, 2.0) == R.ks_for(filter, 1.0) == R.resample_coeffs(10, 20, filter)[1].shape[1]
    assert R.ks_for('bicubic', 0.25) == 17 and R.ks_for('bicubic', 2.0) == 5 and R.ks_for('bilinear', 0.375) == 7
    with pytest.raises(ValueError):
        R.ks_for(filter, 0.0)
    with pytest.raises(ValueError):
        R.ks_for('lanczos', 0.5)


@pytest.mark.parametrize('layout', ('hwc', 'chw'))
@pytest.mark.parametrize('label_dtype', (torch.uint8, torch.int64))
def test_batch_augment_equals_device_augment_on_cpu(layout, label_dtype):
    from hyperseg_amd import InputNorm
    from hyperseg_amd.training import BatchAugment, device_augment
    norm = InputNorm(layout=layout)
    frames, labels = batch(layout, label_dtype)
    aug = BatchAugment(IN_HW, CROP, norm, (0.25, 2.0), lbl_fill=255, fill=(7, 8, 9))
    assert aug.ks_max == 17
    want = device_augment(frames, labels, SCALES, CROP, OFFSETS, FLIPS, norm, lbl_fill=255, fill=(7, 8, 9))
    got = aug(frames, labels, SCALES, OFFSETS, FLIPS)
    assert got[0].dtype == torch.float32 and tuple(got[0].shape) == (6, 3) + CROP and got[1].dtype == torch.int64
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert bool((got[1][0] == 255).any()) and bool((got[1][1] == 255).any())          # padding in the down-scaled samples
    want = device_augment(frames, labels, SCALES, CROP, OFFSETS, FLIPS, norm, lbl_fill=255, fill=(7, 8, 9), jitter=JITTERS)
    got = aug(frames, labels, SCALES, OFFSETS, FLIPS, jitter=JITTERS)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    rows = aug.rows(SCALES, OFFSETS, FLIPS)
    assert rows.dtype == torch.int32 and rows[:, :2].tolist() == [[12, 24], [24, 48], [48, 96], [48, 97], [66, 132], [96, 192]]
    run = aug.run(frames, labels, params=rows)
    plain = aug(frames, labels, SCALES, OFFSETS, FLIPS)
    assert torch.equal(run[0], plain[0]) and torch.equal(run[1], plain[1])


def test_batch_augment_refusals():
    from hyperseg_amd import InputNorm
    from hyperseg_amd.training import BatchAugment
    norm = InputNorm(layout='hwc')
    frames, labels = batch()
    aug = BatchAugment(IN_HW, CROP, norm, (0.5, 1.5))
    for bad in (0.49, 1.51, [1.0, 1.0, 1.0, 1.0, 1.0, 2.0]):
        with pytest.raises(ValueError, match='scale_range'):
            aug(frames, labels, bad, (0, 0), False)
    with pytest.raises(ValueError):
        aug(frames, labels, [1.0] * 5, (0, 0), False)                       # one value, or one per sample
    with pytest.raises(ValueError):
        aug(frames[:, :40], labels[:, :40], 1.0, (0, 0), False)             # not the size it was made for
    with pytest.raises(ValueError):
        aug(frames, labels[:5], 1.0, (0, 0), False)
    aug(frames, labels, 1.0, (0, 0), False)
    with pytest.raises(ValueError):
        aug(frames[:4], labels[:4], 1.0, (0, 0), False)                     # the batch size is fixed by the first call
    for args in (((48, 96), (32, 64), norm, (0.0, 1.0)), ((48, 96), (32, 64), norm, (1.5, 0.5)), ((48, 0), (32, 64), norm, (0.5, 1.0)),
                 ((48, 96), (32, 64), norm, (0.001, 1.0))):
        with pytest.raises(ValueError):
            BatchAugment(*args)
    with pytest.raises(ValueError):
        BatchAugment(IN_HW, CROP, norm, (0.5, 1.0), filter='lanczos')
    with pytest.raises(ValueError):
        BatchAugment(IN_HW, CROP, norm, (0.5, 1.0), batch=0)
