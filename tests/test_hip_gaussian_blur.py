"""Gaussian blur on the device (csrc/hs_blur.hip): ``functional.gaussian_blur`` against Pillow's recorded bytes
(tests/golden/gaussian_blur_ref.npz) and against the CPU implementation of the same arithmetic (utils/blur.py -- itself held to those
bytes by tests/test_gaussian_blur_cpu.py); ``training.device_augment(blur=...)`` and ``BatchAugment`` on top.  Bytes, and floats looked
up from bytes: every comparison is ``torch.equal`` (floats as their bits), no tolerance appears in this file."""
import functools

import pytest
import torch

from conftest import G, load_golden
from hyperseg_amd.utils import blur as BL

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
LAYOUTS = ('hwc', 'chw')
KINDS = ('noise', 'binary')
P = BL.GaussianBlurParams


def _in_layout(x, layout):
    return x if layout == 'hwc' else x.permute(0, 3, 1, 2).contiguous()


def _bits(t):
    return t.cpu().view(torch.int32)


@functools.lru_cache(maxsize=None)
def _golden():
    """[(input (h, w, 3), sigma, Pillow's output, utils.blur's output)] of the fixture, computed once; shared and never written to."""
    ref = load_golden('gaussian_blur_ref')
    out = []
    for h, w, k, si in ref['cases'].tolist():
        key, sigma = f'{h}x{w}_{KINDS[k]}', float(ref['sigmas'][si])
        out.append((ref['in_' + key], sigma, ref[f'out_{key}_s{si}'], BL.gaussian_blur_cpu(ref['in_' + key][None], P(sigma), 'hwc')[0]))
    return out


@functools.lru_cache(maxsize=None)
def _frames(b, h, w, seed=0):
    """uint8 (B, H, W, 3) noise frames, shared and never written to."""
    return torch.randint(0, 256, (b, h, w, 3), generator=G(5000 + 7 * h + w + seed), dtype=torch.uint8)


@pytest.mark.parametrize('layout', LAYOUTS)
def test_golden_bytes(layout):
    """Every size and sigma of the fixture within the radius bound -- the radius-exceeds-line cases (sigma 10 and 15 on 5 x 7, 1 x 9,
    9 x 1, 3 x 3) and the frames of more than one tile among them: uint8 out, float32 out through the table, and ``out=``."""
    from hyperseg_amd import functional as HF
    from hyperseg_amd import InputNorm
    norm = InputNorm((0.4137, 0.38291, 0.456789), (0.2719, 0.19283, 0.31415), layout=layout)
    seen = set()
    for a, sigma, pillow, cpu in _golden():
        if BL.weights(sigma)[0] > BL.MAX_RADIUS:
            continue
        seen.add((tuple(a.shape[:2]), sigma))
        x, want = _in_layout(a[None], layout).to(DEV), _in_layout(pillow[None], layout)
        got = HF.gaussian_blur(x, P(sigma), layout)
        assert got.dtype == torch.uint8 and tuple(got.shape) == tuple(x.shape), (a.shape, sigma)
        assert torch.equal(got.cpu(), want) and torch.equal(got.cpu(), _in_layout(cpu[None], layout)), (a.shape, sigma)
        fl = HF.gaussian_blur(x, P(sigma), layout, norm=norm)
        assert fl.dtype == torch.float32 and torch.equal(_bits(fl), _bits(norm.to_float(want))), (a.shape, sigma)
        out = torch.full_like(x, 7)
        assert HF.gaussian_blur(x, P(sigma), layout, out=out) is out and torch.equal(out.cpu(), want), (a.shape, sigma)
        fout = torch.full((1, 3) + tuple(a.shape[:2]), float('nan'), device=DEV)
        assert HF.gaussian_blur(x, P(sigma), layout, norm=norm, out=fout) is fout and torch.equal(_bits(fout), _bits(norm.to_float(want)))
    assert {((5, 7), 10.0), ((1, 9), 10.0), ((9, 1), 10.0), ((70, 150), 15.0), ((150, 70), 5.0), ((64, 48), 0.0)} <= seen and len(seen) == 92


# one pixel; lines shorter than a run of 4; W odd ('hwc' rows start at every alignment) and W a multiple of 4 (the 16-byte float
# stores); more than one tile along both axes with ragged last tiles (row tiles: 128 pixels x 16 / 48 rows; column tiles: 48 / 128 pixels
# x 64 rows), at the largest radius
SHAPES = [(1, 1), (2, 3), (3, 67), (67, 4), (131, 52), (49, 261)]


@pytest.mark.parametrize('layout', LAYOUTS)
@pytest.mark.parametrize('hw', SHAPES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_shapes_against_the_cpu(hw, layout):
    from hyperseg_amd import functional as HF
    from hyperseg_amd import InputNorm
    norm = InputNorm(layout=layout)
    x = _in_layout(_frames(2, *hw), layout)                   # the second image of an odd-sized pair starts at an odd address
    for sigma in (1.5, 16):                                   # r = 1 and r = 15 = HS_BLUR_MAX_RADIUS
        assert BL.weights(sigma)[0] == (1 if sigma == 1.5 else BL.MAX_RADIUS)
        want = BL.gaussian_blur_cpu(x, P(sigma), layout)
        got = HF.gaussian_blur(x.to(DEV), P(sigma), layout)
        assert torch.equal(got.cpu(), want), sigma
        fl = HF.gaussian_blur(x.to(DEV), P(sigma), layout, norm=norm)
        assert tuple(fl.shape) == (2, 3) + hw and torch.equal(_bits(fl), _bits(norm.to_float(want))), sigma


@pytest.mark.parametrize('layout', LAYOUTS)
def test_unaligned_base_and_out_slice(layout):
    from hyperseg_amd import functional as HF
    from hyperseg_amd import InputNorm
    x = _in_layout(_frames(2, 8, 12), layout)
    want = BL.gaussian_blur_cpu(x, P(2), layout)
    for off in (1, 2, 3):
        buf = torch.zeros(x.numel() + 16, dtype=torch.uint8, device=DEV)
        src = buf[off:off + x.numel()].view(x.shape)
        src.copy_(x)
        assert torch.equal(HF.gaussian_blur(src, P(2), layout).cpu(), want), off
    big = torch.full((want.numel() + 5,), 77, dtype=torch.uint8, device=DEV)
    sl = big[3:3 + want.numel()].view(want.shape)
    got = HF.gaussian_blur(x.to(DEV), P(2), layout, out=sl)
    assert got is sl and torch.equal(sl.cpu(), want) and bool((big[:3] == 77).all()) and bool((big[-2:] == 77).all())
    norm = InputNorm(layout=layout)
    fbig = torch.full((want.numel() + 3,), float('nan'), device=DEV)          # a destination that is only 4-byte aligned
    fsl = fbig[1:1 + want.numel()].view(2, 3, 8, 12)
    HF.gaussian_blur(x.to(DEV), P(2), layout, norm=norm, out=fsl)
    assert torch.equal(_bits(fsl), _bits(norm.to_float(want))) and bool(torch.isnan(fbig[0])) and bool(torch.isnan(fbig[-2:]).all())


@pytest.mark.parametrize('layout', LAYOUTS)
def test_batch_of_four_with_one_sample_not_applied(layout):
    from hyperseg_amd import functional as HF
    from hyperseg_amd import InputNorm
    norm = InputNorm(layout=layout)
    params = [P(5), P(0.5), P(7, apply=False), P(15)]
    x = _in_layout(_frames(4, 37, 53), layout)
    want = BL.gaussian_blur_cpu(x, params, layout)
    assert torch.equal(want[2], x[2]) and not torch.equal(want[0], x[0])
    status = torch.full((4,), -1, dtype=torch.int32, device=DEV)
    assert torch.equal(HF.gaussian_blur(x.to(DEV), params, layout, status=status).cpu(), want)
    assert status.tolist() == [0, 0, 0, 0]
    fl = HF.gaussian_blur(x.to(DEV), params, layout, norm=norm)                # the unapplied sample is normalised all the same
    assert torch.equal(_bits(fl), _bits(norm.to_float(want)))
    for i, p in enumerate(params):                    # and each sample is what it is alone
        assert torch.equal(HF.gaussian_blur(x[i:i + 1].to(DEV), p, layout).cpu(), want[i:i + 1])


def test_determinism_and_a_table_changed_between_replays():
    from hyperseg_amd import functional as HF
    x = _frames(2, 97, 131).to(DEV)
    sets = ([P(5), P(1)], [P(2, apply=False), P(10)])
    want = [BL.gaussian_blur_cpu(x.cpu(), s, 'hwc') for s in sets]
    first, second = HF.gaussian_blur(x, sets[0], 'hwc'), HF.gaussian_blur(x, sets[0], 'hwc')
    assert torch.equal(first, second) and torch.equal(first.cpu(), want[0])
    tables = [BL.params_table(s, 2).to(DEV) for s in sets]
    table = tables[0].clone()
    out, status = torch.empty_like(x), torch.zeros(2, dtype=torch.int32, device=DEV)
    HF.gaussian_blur(x, None, 'hwc', out=out, table=table, status=status)      # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        HF.gaussian_blur(x, None, 'hwc', out=out, table=table, status=status)
    for k in (1, 0, 1):
        table.copy_(tables[k])
        graph.replay()
        assert torch.equal(out.cpu(), want[k]), k


@pytest.mark.parametrize('layout', LAYOUTS)
def test_a_record_beyond_the_radius_bound(layout):
    """In a caller's table it leaves its sample unblurred and sets its status word, the others are not affected; the host path raises."""
    from hyperseg_amd import functional as HF
    from hyperseg_amd import InputNorm
    ref = load_golden('gaussian_blur_ref')
    a = ref['in_17x40_noise']
    x = _in_layout(torch.stack([a, a, a, a]), layout)
    params = [P(5), P(25), P(15), P(25, apply=False)]
    table = BL.params_table(params, 4)
    assert table[1, 1] == 24 > BL.MAX_RADIUS
    table[2, 1] = -3                                                           # and a negative radius
    status = torch.full((4,), -1, dtype=torch.int32, device=DEV)
    got = HF.gaussian_blur(x.to(DEV), None, layout, table=table.to(DEV), status=status)
    want = _in_layout(torch.stack([ref['out_17x40_noise_s0'], a, a, a]), layout)
    assert torch.equal(got.cpu(), want) and status.tolist() == [0, 1, 1, 0]
    norm = InputNorm(layout=layout)
    fl = HF.gaussian_blur(x.to(DEV), None, layout, norm=norm, table=table.to(DEV), status=status)
    assert torch.equal(_bits(fl), _bits(norm.to_float(want))) and status.tolist() == [0, 1, 1, 0]
    y = torch.full_like(x, 9).to(DEV)
    with pytest.raises(ValueError):
        HF.gaussian_blur(x.to(DEV), params, layout, out=y)
    torch.cuda.synchronize()
    assert bool((y == 9).all())                                                # before any launch
    assert not torch.equal(BL.gaussian_blur_cpu(x[1:2], P(25), layout), x[1:2])      # the CPU statement has no bound ...
    assert torch.equal(BL.gaussian_blur_cpu(x[1:2], P(25), layout), _in_layout(ref['out_17x40_noise_s11'][None], layout))   # ... and is Pillow's


def test_refusals():
    from hyperseg_amd import functional as HF
    from hyperseg_amd import InputNorm, _hip
    x = torch.zeros(2, 8, 8, 3, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError):
        HF.gaussian_blur(x.float(), P(5))
    with pytest.raises(ValueError):
        HF.gaussian_blur(x, P(5), layout='chw')
    with pytest.raises(ValueError):
        HF.gaussian_blur(x, P(5), layout='nhwc')
    with pytest.raises(ValueError):
        HF.gaussian_blur(x, [P(5)] * 3)
    with pytest.raises(ValueError):
        HF.gaussian_blur(x, None)
    with pytest.raises(ValueError):
        HF.gaussian_blur(x, P(5), norm=InputNorm(layout='chw'))
    with pytest.raises(ValueError):
        HF.gaussian_blur(x, P(5), out=torch.empty(2, 8, 8, 3, device=DEV))               # float out for a uint8 result
    with pytest.raises(ValueError):
        HF.gaussian_blur(x, None, table=BL.params_table(P(5), 2))                        # a table on the CPU
    with pytest.raises(ValueError):
        HF.gaussian_blur(x, None, table=BL.params_table(P(5), 3).to(DEV))                # three records for two frames
    with pytest.raises(ValueError):
        HF.gaussian_blur(x, P(5), status=torch.zeros(3, dtype=torch.int32, device=DEV))
    # declined sizes: HS_ERR_UNSUPPORTED, nothing launched -- the output stays as it was
    y = torch.full((2, 8, 8, 3), 9, dtype=torch.uint8, device=DEV)
    t, tmp, status = BL.params_table(P(5), 2).to(DEV), torch.empty_like(x), torch.full((2,), -1, dtype=torch.int32, device=DEV)
    lib, s = _hip.lib, _hip.stream_ptr()
    args = lambda batch, w: (x.data_ptr(), 0, batch, 8, w, t.data_ptr(), tmp.data_ptr(), None, y.data_ptr(), status.data_ptr(), s)
    assert lib.hs_gaussian_blur_fwd(*args(65536, 8)) == -3
    assert lib.hs_gaussian_blur_fwd(*args(2, (1 << 15) + 1)) == -3
    assert lib.hs_gaussian_blur_fwd(*args(2, 0)) == -1                                   # HS_ERR_BAD_ARG
    assert lib.hs_gaussian_blur_fwd(x.data_ptr(), 2, 2, 8, 8, t.data_ptr(), tmp.data_ptr(), None, y.data_ptr(), status.data_ptr(), s) == -1
    torch.cuda.synchronize()
    assert bool((y == 9).all()) and status.tolist() == [-1, -1]


def _chain_inputs():
    frames = torch.randint(0, 256, (2, 48, 96, 3), generator=G(90), dtype=torch.uint8)
    labels = torch.randint(0, 19, (2, 48, 96), generator=G(91), dtype=torch.uint8)
    return frames, labels


# the (scale, crop, offset, hflip) cases of tests/test_hip_resample.py::test_device_augment
@pytest.mark.parametrize('jitter', [False, True], ids=['plain', 'jitter'])
@pytest.mark.parametrize('scale,crop,offset,hflip', [(0.5, (32, 64), (-5, -9), True), (2.0, (32, 64), (40, 101), False)])
def test_batch_augment_and_device_augment_with_blur(scale, crop, offset, hflip, jitter):
    """``BatchAugment(..., blur=)`` == ``device_augment(..., blur=)`` == the CPU route, with and without a jitter in front; ``blur=None``
    gives the bits of a call without the argument."""
    from hyperseg_amd import ColorJitterParams, InputNorm
    from hyperseg_amd.training import BatchAugment, device_augment
    norm = InputNorm(layout='hwc')
    frames, labels = _chain_inputs()
    jit = [ColorJitterParams(('brightness', 'contrast'), 0.8, 1.25), ColorJitterParams(('hue',), hue=0.1)] if jitter else None
    blur = [P(5), P(2)]
    want_img, want_lbl = device_augment(frames, labels, scale, crop, offset, hflip, norm, lbl_fill=255, jitter=jit, blur=blur)     # CPU tensors
    fd, ld = frames.to(DEV), labels.to(DEV)
    img, lbl = device_augment(fd, ld, scale, crop, offset, hflip, norm, lbl_fill=255, jitter=jit, blur=blur)
    assert img.dtype == torch.float32 and tuple(img.shape) == (2, 3) + crop and lbl.dtype == torch.int64
    assert torch.equal(_bits(img), _bits(want_img)) and torch.equal(lbl.cpu(), want_lbl)
    aug = BatchAugment((48, 96), crop, norm, (0.25, 2.0))
    bimg, blbl = aug(fd, ld, scale, offset, hflip, jitter=jit, blur=blur)
    assert torch.equal(_bits(bimg), _bits(want_img)) and torch.equal(blbl.cpu(), want_lbl) and aug.blur_status.tolist() == [0, 0]
    plain = device_augment(fd, ld, scale, crop, offset, hflip, norm, lbl_fill=255, jitter=jit)
    none = device_augment(fd, ld, scale, crop, offset, hflip, norm, lbl_fill=255, jitter=jit, blur=None)
    assert torch.equal(_bits(plain[0]), _bits(none[0])) and torch.equal(plain[1], none[1]) and not torch.equal(plain[0], img)
    assert torch.equal(lbl, plain[1])                                          # the label is untouched
    bplain, bnone = aug(fd, ld, scale, offset, hflip, jitter=jit), aug(fd, ld, scale, offset, hflip, jitter=jit, blur=None)
    assert torch.equal(_bits(bplain[0]), _bits(plain[0])) and torch.equal(_bits(bnone[0]), _bits(plain[0])) and torch.equal(bnone[1], plain[1])
    with pytest.raises(ValueError):
        aug(fd, ld, scale, offset, hflip, blur=P(25))
    with pytest.raises(ValueError):
        device_augment(fd, ld, scale, crop, offset, hflip, norm, blur=P(25))


def test_a_captured_run_replays_with_new_radii():
    from hyperseg_amd import InputNorm
    from hyperseg_amd.training import BatchAugment, device_augment
    norm, crop = InputNorm(layout='hwc'), (32, 64)
    frames, labels = _chain_inputs()
    fd, ld = frames.to(DEV), labels.to(DEV)
    sets = (((0.5, 2.0), [(-5, -9), (40, 101)], [True, False], [P(5), None]), ((1.0, 0.75), [(3, 7), (0, -4)], [False, True], [P(1), P(15)]))
    want = [device_augment(frames, labels, s[0], crop, s[1], s[2], norm, blur=s[3]) for s in sets]
    aug = BatchAugment((48, 96), crop, norm, (0.25, 2.0))
    assert torch.equal(_bits(aug(fd, ld, *sets[0][:3], blur=sets[0][3])[0]), _bits(want[0][0]))          # makes the buffers, warms up
    out = (torch.empty(2, 3, *crop, device=DEV), torch.empty(2, *crop, dtype=torch.int64, device=DEV))
    table = BL.params_table(sets[0][3], 2).to(DEV)
    aug.run(fd, ld, out=out, blur=table)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        aug.run(fd, ld, out=out, blur=table)
    for k in (1, 0, 1):
        aug.params.copy_(aug.rows(*sets[k][:3]).to(DEV))
        table.copy_(BL.params_table(sets[k][3], 2).to(DEV))
        graph.replay()
        assert torch.equal(_bits(out[0]), _bits(want[k][0])) and torch.equal(out[1].cpu(), want[k][1]), k
    own = aug.run(fd, ld, blur=True)                                           # the object's own table: what the last __call__ uploaded
    assert torch.equal(_bits(own[0]), _bits(device_augment(frames, labels, *sets[1][:1], crop, *sets[1][1:3], norm, blur=sets[0][3])[0]))
