"""``hyperseg_amd.LabelCodec`` on the CPU: ``encode_cpu`` against the reference's lines restated in numpy right here (the reference's
dataset modules need torchvision and are not imported) -- hyperseg/datasets/cityscapes.py:210-211 and hyperseg/datasets/camvid.py:93-100
-- then the CPU twins that take a codec (``label_resize_cpu``, the ``device_augment`` / ``BatchAugment`` CPU chains) against
encode-then-the-same-call.  Integers throughout: every comparison is exact."""
import numpy as np
import pytest
import torch

from conftest import G
from hyperseg_amd import LabelCodec
from hyperseg_amd.utils import resample as R

# Cityscapes' ids 0..33 -> train ids (the public label table; cityscapes.py:69-102, :107) and CamVid's class_color (camvid.py:25-38)
CITYSCAPES = [255, 255, 255, 255, 255, 255, 255, 0, 1, 255, 255, 2, 3, 4, 255, 255, 255, 5, 255, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 255, 255,
              16, 17, 18]
CAMVID = [(128, 128, 128), (128, 0, 0), (192, 192, 128), (128, 64, 128), (0, 0, 192), (128, 128, 0), (192, 128, 128), (64, 64, 128),
          (64, 0, 128), (64, 64, 0), (0, 128, 192), (0, 0, 0)]
TABLE_256 = [(37 * i + 11) % 256 for i in range(255)] + [7]           # values[255] = 7: an encoded fill of 255 would show as 7
DUPLICATED = [(10, 20, 30), (1, 2, 3), (10, 20, 30), (200, 100, 0), (1, 2, 3)]


def cityscapes_lines(target, id_to_train_id):
    """cityscapes.py:209-211 on a numpy label."""
    id_to_train_id = np.array(id_to_train_id, dtype='uint8')
    target = np.array(target)
    target[np.bitwise_or(target < 0, target >= len(id_to_train_id))] = 0
    return id_to_train_id[target]


def camvid_lines(label, color_map, start=255):
    """camvid.py:93-98 on a numpy (H, W, 3) label; ``start`` is the 255 the reference fills the image with."""
    label_rgb = np.array(label)
    label_index = np.full(label_rgb.shape[:2], start, dtype='uint8')
    for i, color in enumerate(color_map):
        label_index[np.all(label_rgb == color, axis=2)] = i
    return label_index


def raw_ids(shape, seed, dtype, extremes):
    t = torch.randint(0, 256 if dtype == torch.uint8 else 40, shape, generator=G(seed)).to(dtype)
    for i, v in enumerate(extremes):
        t.view(-1)[3 * i + 1] = v
    return t


def raw_colors(shape, colors, seed, strangers=0.2):
    """(B, H, W, 3) uint8: pixels drawn from ``colors``, a share of them replaced by colours that differ from an entry in one byte."""
    g = G(seed)
    pal = torch.tensor(colors, dtype=torch.uint8)
    t = pal[torch.randint(0, len(colors), shape, generator=g)]
    off = torch.rand(shape, generator=g) < strangers
    t[..., 2][off] ^= 1
    return t.contiguous()


@pytest.mark.parametrize('values', [CITYSCAPES, TABLE_256], ids=['cityscapes34', 'table256'])
@pytest.mark.parametrize('dtype', [torch.uint8, torch.int64])
def test_table_equals_the_cityscapes_lines(values, dtype):
    codec = LabelCodec.table(values)
    t = raw_ids((2, 9, 14), 9100, dtype, (255, 200, 34, 33, 0) if dtype == torch.uint8 else (-3, 300, 34, 33, 0, 255, -1, 1 << 40))
    assert (t.long() >= len(values)).any() or len(values) == 256
    want = torch.from_numpy(cityscapes_lines(t.numpy(), values).astype(np.int64))
    for out_dtype in (None, torch.uint8, torch.int64):
        got = codec.encode_cpu(t, out_dtype=out_dtype) if out_dtype is not None else codec.encode_cpu(t)
        assert got.dtype == (out_dtype or dtype) and tuple(got.shape) == (2, 9, 14)
        assert torch.equal(got.long(), want)
    if len(values) == 256 and dtype == torch.uint8:
        assert int(codec.encode_cpu(torch.full((1, 1, 1), 255, dtype=torch.uint8))) == 7


@pytest.mark.parametrize('colors,unmatched', [(CAMVID, 255), (DUPLICATED, 255), (CAMVID, 11), (DUPLICATED, 0)],
                         ids=['camvid', 'duplicates', 'camvid-unmatched11', 'duplicates-unmatched0'])
def test_colors_equal_the_camvid_lines(colors, unmatched):
    codec = LabelCodec.colors(colors, unmatched=unmatched)
    t = raw_colors((2, 9, 14), colors, 9200)
    want = np.stack([camvid_lines(img, colors, start=unmatched) for img in t.numpy()])
    assert (want == unmatched).any()                                  # some pixels match nothing
    got = codec.encode_cpu(t)
    assert got.dtype == torch.uint8 and torch.equal(got, torch.from_numpy(want))
    assert torch.equal(codec.encode_cpu(t, out_dtype=torch.int64), torch.from_numpy(want.astype(np.int64)))
    if colors is DUPLICATED:                                          # the later index of a repeated colour wins
        px = torch.tensor(DUPLICATED, dtype=torch.uint8).view(1, 1, 5, 3)
        assert codec.encode_cpu(px).flatten().tolist() == [2, 4, 2, 3, 4]


def test_words_identity_and_cache():
    a, b = LabelCodec.table(CITYSCAPES), LabelCodec.table(tuple(CITYSCAPES))
    assert a == b and hash(a) == hash(b) and a != LabelCodec.table(CITYSCAPES + [255]) and len({a, b}) == 1
    c = LabelCodec.colors(CAMVID)
    assert c == LabelCodec.colors(np.array(CAMVID)) and c != LabelCodec.colors(CAMVID, unmatched=0) and c != a
    assert eval(repr(a), {'LabelCodec': LabelCodec}) == a and eval(repr(c), {'LabelCodec': LabelCodec}) == c
    w = a.words()
    assert w.dtype == torch.int32 and tuple(w.shape) == (64,)
    as_bytes = w.numpy().astype('<i4').view(np.uint8).tolist()
    assert as_bytes[:34] == CITYSCAPES and as_bytes[34:] == [CITYSCAPES[0]] * 222
    w = c.words()
    assert w.dtype == torch.int32 and w.tolist() == [12] + [r | g << 8 | bb << 16 for r, g, bb in CAMVID]
    assert a.device_words('cpu') is b.device_words('cpu') and torch.equal(a.device_words('cpu'), a.words())
    with pytest.raises(AttributeError):
        a.values = ()


@pytest.mark.parametrize('kind', ['table', 'colors'])
def test_label_resize_cpu_takes_the_codec_and_does_not_encode_the_fill(kind):
    if kind == 'table':
        codec, t = LabelCodec.table(TABLE_256), raw_ids((2, 11, 17), 9300, torch.uint8, (255, 254))
    else:
        codec, t = LabelCodec.colors(CAMVID, unmatched=200), raw_colors((2, 11, 17), CAMVID, 9301)
    view = R.ResizeView((16, 20), (-3, -4), True)                     # reaches outside the (14, 23) resized image on every side
    for out_dtype in (None, torch.int64):
        got = R.label_resize_cpu(t, (14, 23), view=view, fill=255, out_dtype=out_dtype, codec=codec)
        want = R.label_resize_cpu(codec.encode_cpu(t), (14, 23), view=view, fill=255, out_dtype=out_dtype)
        assert got.dtype == want.dtype == (out_dtype or torch.uint8) and torch.equal(got, want)
        # rows -3..-1 and columns -4..-1 (flipped: the last four) are the fill as given: values[255] = 7 is not applied to it
        assert (got[:, :3] == 255).all() and (got[:, :, -4:] == 255).all()


@pytest.mark.parametrize('kind', ['table', 'colors'])
@pytest.mark.parametrize('jitter', [False, True])
def test_augment_cpu_chains_take_the_codec(kind, jitter):
    from hyperseg_amd.training import BatchAugment, device_augment
    from hyperseg_amd.utils import jitter as J
    from hyperseg_amd.utils.inference import InputNorm
    norm = InputNorm(layout='hwc')
    in_hw, crop = (20, 28), (12, 16)
    frames = torch.randint(0, 256, (3,) + in_hw + (3,), generator=G(9400), dtype=torch.uint8)
    if kind == 'table':
        codec, raw = LabelCodec.table(TABLE_256), raw_ids((3,) + in_hw, 9401, torch.uint8, (255,))
    else:
        codec, raw = LabelCodec.colors(CAMVID), raw_colors((3,) + in_hw, CAMVID, 9402)
    scales, offsets, flips = [0.5, 1.0, 1.3], [(-3, -2), (4, 6), (10, 20)], [True, False, True]
    jit = J.ColorJitterParams((J.OPS[0], J.OPS[1]), 0.8, 1.25, None, None) if jitter else None
    want = device_augment(frames, codec.encode_cpu(raw), scales, crop, offsets, flips, norm, jitter=jit)
    got = device_augment(frames, raw, scales, crop, offsets, flips, norm, jitter=jit, label_codec=codec)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and got[1].dtype == torch.int64
    plain, coded = BatchAugment(in_hw, crop, norm, (0.5, 1.3)), BatchAugment(in_hw, crop, norm, (0.5, 1.3), label_codec=codec)
    got = coded(frames, raw, scales, offsets, flips, jitter=jit)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    if not jitter:
        rows = coded.rows(scales, offsets, flips, 3)
        got, same = coded.run(frames, raw, params=rows), plain.run(frames, codec.encode_cpu(raw), params=rows)
        assert torch.equal(got[0], same[0]) and torch.equal(got[1], same[1]) and torch.equal(got[1], want[1])
    with pytest.raises(ValueError):
        coded(frames, codec.encode_cpu(raw)[:, :-1], scales, offsets, flips)
    if kind == 'colors':
        with pytest.raises(ValueError):                               # encoded labels where the object was made for colour images
            coded(frames, codec.encode_cpu(raw), scales, offsets, flips)
        with pytest.raises(ValueError):
            device_augment(frames, codec.encode_cpu(raw), scales, crop, offsets, flips, norm, label_codec=codec)


def test_model_attribute_encodes_cpu_targets():
    """``HyperGenBase.label_codec``: a plain attribute (no state-dict entry); ``encoded`` takes raw targets of the codec's kind."""
    from hyperseg_amd.models._common import HyperGenBase
    assert HyperGenBase.label_codec is None

    class Bare(HyperGenBase):
        def __init__(self):
            torch.nn.Module.__init__(self)

    m = Bare()
    keys = list(m.state_dict())
    t = raw_ids((1, 5, 6), 9500, torch.int64, (-3, 300))
    assert m.encoded(t) is t
    m.label_codec = LabelCodec.table(CITYSCAPES)
    assert list(m.state_dict()) == keys
    assert torch.equal(m.encoded(t), m.label_codec.encode_cpu(t))
    assert torch.equal(m.encoded(t.to(torch.int32)), m.label_codec.encode_cpu(t))
    f = t.float()
    assert m.encoded(f) is f
    m.label_codec = LabelCodec.colors(CAMVID)
    c = raw_colors((1, 5, 6), CAMVID, 9501)
    assert torch.equal(m.encoded(c), m.label_codec.encode_cpu(c)) and m.encoded(t) is t      # a 3-D target is already encoded


def test_constructor_and_operand_errors():
    for bad in ([], list(range(256)) + [0], [0, 256], [0, -1], [0.5], [True]):
        with pytest.raises(ValueError):
            LabelCodec.table(bad)
    for bad in ([], [(0, 0, 0)] * 256, [(0, 0)], [(0, 0, 256)], [(0, 0, -1)], [5]):
        with pytest.raises(ValueError):
            LabelCodec.colors(bad)
    for bad in (-1, 256, 1.5):
        with pytest.raises(ValueError):
            LabelCodec.colors(CAMVID, unmatched=bad)
    with pytest.raises(ValueError):
        LabelCodec(3, (0,), None)
    table, colors = LabelCodec.table(CITYSCAPES), LabelCodec.colors(CAMVID)
    ids, rgb = torch.zeros(1, 4, 5, dtype=torch.uint8), torch.zeros(1, 4, 5, 3, dtype=torch.uint8)
    for codec, bad in ((table, rgb), (table, ids.float()), (table, ids.to(torch.int32)), (table, ids[0]), (colors, ids), (colors, rgb.long()),
                       (colors, rgb[..., :2]), (table, ids.numpy())):
        with pytest.raises(ValueError):
            codec.encode_cpu(bad)
    with pytest.raises(ValueError):
        table.encode_cpu(ids, out_dtype=torch.int32)
    with pytest.raises(ValueError):
        R.label_resize_cpu(rgb, (4, 5), codec=table)
    from hyperseg_amd.training import BatchAugment
    from hyperseg_amd.utils.inference import InputNorm
    with pytest.raises(ValueError):
        BatchAugment((8, 8), (4, 4), InputNorm(layout='hwc'), (0.5, 1.0), label_codec=CITYSCAPES)
