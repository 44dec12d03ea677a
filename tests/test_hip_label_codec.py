"""A dataset's label encoding on the device (csrc/hs_label_codec.hip and the coded twins of the two label gathers): ``functional.label_encode``,
``label_resize(codec=)`` and ``label_resize_batch(codec=)`` against their CPU twins (``LabelCodec.encode_cpu``, ``label_resize_cpu(codec=)``,
themselves held to the reference's lines by tests/test_label_codec_cpu.py), ``BatchAugment`` with raw labels, and ``model.label_codec``
through ``evaluate`` / ``validate`` and ``GraphedModel``.  Integers and bytes: every comparison is ``torch.equal``."""
import pytest
import torch

from conftest import G
from hyperseg_amd import LabelCodec
from hyperseg_amd.utils import resample as R
from hyperseg_amd.utils.synthetic import fill_by_name
from test_label_codec_cpu import CAMVID, CITYSCAPES, DUPLICATED, TABLE_256, raw_colors, raw_ids

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
SHAPES = [(1, 7, 13), (2, 33, 67), (3, 16, 64)]          # a partial run only; odd planes (images 1.. start unaligned); whole 16-pixel runs
DTYPES = [torch.uint8, torch.int64]


def offset_by_one(t):
    """``t``'s values in a contiguous tensor whose base pointer is one element past an aligned allocation."""
    store = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    out = store[1:].view(t.shape)
    out.copy_(t)
    assert out.is_contiguous() and out.data_ptr() == store.data_ptr() + t.element_size()
    return out


def codecs(kind):
    if kind == 'table':
        return [LabelCodec.table(CITYSCAPES), LabelCodec.table(TABLE_256)]
    return [LabelCodec.colors(CAMVID), LabelCodec.colors(DUPLICATED, unmatched=9)]


def raw_for(codec, shape, seed, dtype=torch.uint8):
    if codec.is_colors:
        return raw_colors(shape, [list(c) for c in codec.values], seed)
    return raw_ids(shape, seed, dtype, (255, 200, 34, 33, 0) if dtype == torch.uint8 else (-3, 300, 34, 33, 0, 255, -1, 1 << 40))


@pytest.mark.parametrize('shape', SHAPES)
@pytest.mark.parametrize('in_dtype', DTYPES)
def test_label_encode_table(shape, in_dtype):
    from hyperseg_amd import functional as HF
    for codec in codecs('table'):
        t = raw_for(codec, shape, 9600, in_dtype)
        assert (t.long() >= len(codec)).any() or len(codec) == 256       # out-of-range ids are in
        for out_dtype in DTYPES:
            want = codec.encode_cpu(t, out_dtype=out_dtype)
            for shifted_in in (False, True):
                for shifted_out in (False, True):
                    x = offset_by_one(t.to(DEV)) if shifted_in else t.to(DEV)
                    out = torch.zeros(shape, dtype=out_dtype, device=DEV)
                    out = offset_by_one(out) if shifted_out else out
                    got = HF.label_encode(x, codec, out=out)
                    assert got is out and torch.equal(got.cpu(), want), (codec, out_dtype, shifted_in, shifted_out)
        got = HF.label_encode(t.to(DEV), codec)
        assert got.dtype == in_dtype and torch.equal(got.cpu(), codec.encode_cpu(t))


@pytest.mark.parametrize('shape', SHAPES)
def test_label_encode_colors(shape):
    from hyperseg_amd import functional as HF
    for codec in codecs('colors'):
        t = raw_for(codec, shape, 9610)
        want8 = codec.encode_cpu(t)
        assert (want8 == codec.unmatched).any() and want8.dtype == torch.uint8
        for out_dtype in DTYPES:
            for shifted_in in (False, True):
                for shifted_out in (False, True):
                    x = offset_by_one(t.to(DEV)) if shifted_in else t.to(DEV)
                    out = torch.zeros(shape, dtype=out_dtype, device=DEV)
                    out = offset_by_one(out) if shifted_out else out
                    got = HF.label_encode(x, codec, out=out)
                    assert got is out and torch.equal(got.cpu(), want8.to(out_dtype)), (codec, out_dtype, shifted_in, shifted_out)
        got = HF.label_encode(t.to(DEV), codec)
        assert got.dtype == torch.uint8 and torch.equal(got.cpu(), want8)


VIEWS = [((23, 41), None),                                               # upscale, the whole image
         ((9, 14), None),                                                # downscale
         ((23, 41), R.ResizeView((16, 20), (3, 5), True)),               # interior window, flipped
         ((14, 23), R.ResizeView((20, 30), (-3, -4), True)),             # a signed offset that leaves the image on every side
         ((17, 29), R.ResizeView((300, 2), (-1, 28), False))]            # more than one workgroup; one column inside


@pytest.mark.parametrize('kind', ['table', 'colors'])
def test_coded_label_resize(kind):
    from hyperseg_amd import functional as HF
    codec = LabelCodec.table(TABLE_256) if kind == 'table' else LabelCodec.colors(CAMVID, unmatched=200)
    for in_dtype in (DTYPES if kind == 'table' else DTYPES[:1]):
        t = raw_for(codec, (2, 17, 29), 9620, in_dtype)
        x = t.to(DEV)
        for size, view in VIEWS:
            for out_dtype in DTYPES:
                ho, wo = size if view is None else view.size
                out = torch.zeros((2, ho, wo), dtype=out_dtype, device=DEV)
                got = HF.label_resize(x, size, view=view, fill=255, out=out, codec=codec)
                want = R.label_resize_cpu(t, size, view=view, fill=255, out_dtype=out_dtype, codec=codec)
                assert got is out and torch.equal(got.cpu(), want), (in_dtype, size, view, out_dtype)
        got = HF.label_resize(x, (23, 41), codec=codec)
        assert got.dtype == codec.out_dtype(t) and torch.equal(got.cpu(), R.label_resize_cpu(t, (23, 41), codec=codec))
    # the fill is stored as given: values[255] = 7 (or unmatched = 200) is not applied to it
    size, view = VIEWS[3]
    got = HF.label_resize(x, size, view=view, fill=255, codec=codec).cpu()
    assert (got[:, :3] == 255).all() and (got[:, :, -4:] == 255).all() and (got[:, 17:] == 255).all()
    assert torch.equal(got, R.label_resize_cpu(codec.encode_cpu(t), size, view=view, fill=255))


@pytest.mark.parametrize('kind', ['table', 'colors'])
def test_coded_label_resize_batch(kind):
    from hyperseg_amd import functional as HF
    codec = LabelCodec.table(TABLE_256) if kind == 'table' else LabelCodec.colors(DUPLICATED, unmatched=9)
    in_hw, crop = (20, 28), (12, 40)
    rows = torch.tensor([[10, 14, -3, -2, 1, 0], [20, 28, 4, -6, 0, 0], [26, 36, 10, 20, 1, 0]], dtype=torch.int32)
    params = rows.to(DEV)
    tables = HF.resize_tables(params, in_hw, crop, 'bicubic', R.ks_for('bicubic', 0.5))
    for in_dtype in (DTYPES if kind == 'table' else DTYPES[:1]):
        t = raw_for(codec, (3,) + in_hw, 9630, in_dtype)
        for out_dtype in DTYPES:
            out = torch.zeros((3,) + crop, dtype=out_dtype, device=DEV)
            got = HF.label_resize_batch(t.to(DEV), params, tables, fill=255, out=out, codec=codec)
            assert got is out
            for i, (hr, wr, oy, ox, flip, _) in enumerate(rows.tolist()):
                want = R.label_resize_cpu(t[i:i + 1], (hr, wr), view=R.ResizeView(crop, (oy, ox), bool(flip)), fill=255, out_dtype=out_dtype,
                                          codec=codec)
                assert torch.equal(got[i:i + 1].cpu(), want), (in_dtype, out_dtype, i)
    assert not bool(tables.status.any())


@pytest.mark.parametrize('kind', ['table', 'colors'])
def test_batch_augment_with_raw_labels(kind):
    """(2, 40, 56) frames, a (24, 24) crop: labels equal those of pre-encoded input, frames are untouched by the codec; captured once and
    replayed with a second parameter set, equal again."""
    from hyperseg_amd.training import BatchAugment
    from hyperseg_amd.utils.inference import InputNorm
    norm = InputNorm(layout='hwc')
    in_hw, crop = (40, 56), (24, 24)
    codec = LabelCodec.table(TABLE_256) if kind == 'table' else LabelCodec.colors(CAMVID)
    frames = torch.randint(0, 256, (2,) + in_hw + (3,), generator=G(9640), dtype=torch.uint8).to(DEV)
    raw = raw_for(codec, (2,) + in_hw, 9641)
    encoded = codec.encode_cpu(raw).to(DEV)
    raw = raw.to(DEV)
    plain, coded = BatchAugment(in_hw, crop, norm, (0.5, 1.5)), BatchAugment(in_hw, crop, norm, (0.5, 1.5), label_codec=codec)
    sets = [([0.5, 1.5], [(-3, -2), (10, 20)], [True, False]), ([1.0, 0.75], [(4, 30), (-5, 3)], [False, True])]
    want = [plain(frames, encoded, *p) for p in sets]
    got = coded(frames, raw, *sets[0])
    assert torch.equal(got[0], want[0][0]) and torch.equal(got[1], want[0][1]) and (got[1] == 255).any()
    out = (torch.zeros_like(got[0]), torch.zeros_like(got[1]))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        coded.run(frames, raw, out=out)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        coded.run(frames, raw, out=out)
    for p, w in zip(sets[::-1], want[::-1]):
        coded.params.copy_(coded.rows(*p).to(DEV))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out[0], w[0]) and torch.equal(out[1], w[1])
    assert not bool(coded.status.any())


def test_uncoded_routes_are_unchanged():
    """``codec=None`` launches the entries it launched before: their output against ``label_resize_cpu`` (the un-coded instantiation)."""
    from hyperseg_amd import functional as HF
    for in_dtype in DTYPES:
        t = raw_ids((2, 17, 29), 9650, in_dtype, (255, 0))
        for size, view in VIEWS:
            for out_dtype in DTYPES:
                ho, wo = size if view is None else view.size
                out = torch.zeros((2, ho, wo), dtype=out_dtype, device=DEV)
                got = HF.label_resize(t.to(DEV), size, view=view, fill=255, out=out, codec=None)
                assert torch.equal(got.cpu(), R.label_resize_cpu(t, size, view=view, fill=255, out_dtype=out_dtype))
    rows = torch.tensor([[10, 14, -3, -2, 1, 0], [26, 36, 10, 20, 0, 0]], dtype=torch.int32)
    tables = HF.resize_tables(rows.to(DEV), (17, 29), (12, 40), 'bicubic', R.ks_for('bicubic', 0.4))      # 14 / 29 is below 0.5
    got = HF.label_resize_batch(t.to(DEV), rows.to(DEV), tables, fill=255)
    assert not bool(tables.status.any())
    for i, (hr, wr, oy, ox, flip, _) in enumerate(rows.tolist()):
        assert torch.equal(got[i:i + 1].cpu(), R.label_resize_cpu(t[i:i + 1], (hr, wr), view=R.ResizeView((12, 40), (oy, ox), bool(flip)), fill=255))


def test_operand_errors():
    from hyperseg_amd import _hip
    from hyperseg_amd import functional as HF
    table, colors = LabelCodec.table(CITYSCAPES), LabelCodec.colors(CAMVID)
    ids, rgb = torch.zeros(1, 4, 5, dtype=torch.uint8, device=DEV), torch.zeros(1, 4, 5, 3, dtype=torch.uint8, device=DEV)
    for codec, bad in ((table, rgb), (table, ids.float()), (table, ids.to(torch.int32)), (colors, ids), (colors, rgb.long()), (colors, rgb[..., :2]),
                       (None, ids), (CITYSCAPES, ids), (table, ids[:0]), (colors, rgb[:0])):
        with pytest.raises(ValueError):
            HF.label_encode(bad, codec)
    with pytest.raises(ValueError):
        HF.label_encode(ids, table, out=torch.zeros(1, 4, 5, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError):
        HF.label_encode(ids, table, out=torch.zeros(1, 4, 4, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError):
        HF.label_encode(ids, table, out=torch.zeros(1, 4, 5, dtype=torch.uint8))
    with pytest.raises(_hip.HipLibraryError):
        HF.label_encode(ids.cpu(), table)
    with pytest.raises(_hip.HipLibraryError):
        HF.label_encode(rgb.permute(0, 2, 1, 3), colors)                     # not contiguous
    with pytest.raises(ValueError):
        HF.label_resize(rgb, (4, 5), codec=table)
    with pytest.raises(ValueError):
        HF.label_resize(ids, (4, 5), codec=colors)
    # the C entries refuse the same on their own, before any launch
    out = torch.zeros(1, 4, 5, dtype=torch.uint8, device=DEV)
    words = table.device_words(DEV)
    args = (ids.data_ptr(), 0, 1, 4, 5, words.data_ptr())
    assert _hip.lib.hs_label_encode_fwd(*args, 3, 34, 0, out.data_ptr(), 0, None) == -1      # no such codec
    assert _hip.lib.hs_label_encode_fwd(*args, 1, 257, 0, out.data_ptr(), 0, None) == -1
    assert _hip.lib.hs_label_encode_fwd(*args, 2, 256, 0, out.data_ptr(), 0, None) == -1
    assert _hip.lib.hs_label_encode_fwd(*args, 2, 12, 256, out.data_ptr(), 0, None) == -1
    assert _hip.lib.hs_label_encode_fwd(ids.data_ptr(), 1, 1, 4, 5, words.data_ptr(), 2, 12, 255, out.data_ptr(), 0, None) == -1      # int64 colours
    assert _hip.lib.hs_label_encode_fwd(*args, 1, 34, 0, out.data_ptr(), 2, None) == -1
    assert _hip.lib.hs_label_encode_fwd(ids.data_ptr(), 0, 65536, 4, 5, words.data_ptr(), 1, 34, 0, out.data_ptr(), 0, None) == -3
    torch.cuda.synchronize()
    assert int(out.sum()) == 0


# ---------------------------------------------------------------------------------------------------------------- model.label_codec

def _model():
    """tests/test_hip_eval.py's smallest model and size: prepared HyperSeg-M at 128 x 256 (a prepared encoder repeats its own bits)."""
    from hyperseg_amd import configs
    from hyperseg_amd.utils.inference import prepare_for_inference
    m = fill_by_name(configs.build('hyperseg-m').eval(), seed=11)
    prepare_for_inference(m, fold_bn=False, fused_depthwise=True)
    return m.to(DEV)


@pytest.fixture(scope='module')
def model():
    return _model()


def _raw_target(codec, shape, seed):
    """(raw, encoded) CPU targets: classes 0..18 and 255, drawn as raw labels of ``codec``."""
    from hyperseg_amd.fps import raw_labels
    g = G(seed)
    t = torch.randint(0, 19, shape, generator=g)
    if not codec.is_colors:
        t[torch.rand(shape, generator=g) < 0.10] = 255
    raw = raw_labels(t, codec, g)
    if codec.is_colors:
        raw[..., 1][torch.rand(shape, generator=g) < 0.10] ^= 255            # colours of no class: unmatched = 255, ignored
    enc = codec.encode_cpu(raw)
    assert (enc == 255).any() and (enc < 19).any()
    return raw, enc


MODEL_CODECS = {'table': LabelCodec.table(CITYSCAPES), 'colors': LabelCodec.colors(CAMVID + [(9, 9, 9 + i) for i in range(7)])}


@pytest.mark.parametrize('kind', ['table', 'colors'])
def test_model_evaluate_and_validate_take_raw_targets(model, kind):
    from hyperseg_amd.fps import ConfusionMatrix
    from hyperseg_amd.training import BootstrappedCrossEntropyLoss
    from hyperseg_amd.utils.inference import GraphedModel
    codec, n = MODEL_CODECS[kind], 19
    x = torch.rand(1, 3, 128, 256, generator=G(9700)).to(DEV)
    raw, enc = _raw_target(codec, (1, 128, 256), 9701)
    half_raw, half_enc = _raw_target(codec, (1, 64, 128), 9702)
    crit = BootstrappedCrossEntropyLoss(k=4096, thresh=0.3, ignore_index=255)
    try:
        model.label_codec = None
        want_cm, want_half = ConfusionMatrix(n), ConfusionMatrix(n)
        want_masks = model.evaluate(x, enc.to(DEV), want_cm)
        want_half_masks = model.evaluate(x, half_enc.to(DEV), want_half)         # the label-resolution route
        vcm = ConfusionMatrix(n)
        want_loss, want_vmasks = model.validate(x, enc.to(DEV), crit, vcm)
        model.label_codec = codec
        cm, half = ConfusionMatrix(n), ConfusionMatrix(n)
        assert torch.equal(model.evaluate(x, raw.to(DEV), cm), want_masks) and torch.equal(cm.mat, want_cm.mat)
        assert torch.equal(model.evaluate(x, half_raw.to(DEV), half), want_half_masks) and torch.equal(half.mat, want_half.mat)
        got_cm = ConfusionMatrix(n)
        loss, vmasks = model.validate(x, raw.to(DEV), crit, got_cm)
        assert torch.equal(loss, want_loss) and torch.equal(vmasks, want_vmasks) and torch.equal(got_cm.mat, vcm.mat)
        # the CPU route of the attribute: the target encoded by encode_cpu
        assert torch.equal(model.encoded(raw), enc.to(codec.out_dtype(raw)))
        # GraphedModel: the static target buffer holds the raw label, the codec is in the key
        served = GraphedModel(model, masks=True, num_classes=n, clone_output=True, criterion=crit)
        for source in (raw.pin_memory(), raw.to(DEV)):
            assert torch.equal(served.evaluate(x, source), want_masks)
        torch.cuda.synchronize()
        assert torch.equal(served.confusion, 2 * want_cm.mat)
        key = next(k for k in served._graphs if k[0] == 'evaluate')
        assert key[-1] == codec and key[-2] == tuple(raw.shape) and served._graphs[key][1][1].shape == raw.shape
        served.reset_confusion()
        loss, vmasks = served.validate(x, raw.to(DEV))
        torch.cuda.synchronize()
        assert torch.equal(loss, want_loss) and torch.equal(vmasks, want_vmasks) and torch.equal(served.confusion, vcm.mat)
        assert any(k[0] == 'validate' and k[-1] == codec for k in served._graphs)
    finally:
        model.label_codec = None


def test_graph_keys_without_a_codec_are_what_they_were(model):
    from hyperseg_amd.training import BootstrappedCrossEntropyLoss
    from hyperseg_amd.utils.inference import GraphedModel
    assert model.label_codec is None
    crit = BootstrappedCrossEntropyLoss(k=4096, thresh=0.3, ignore_index=255)
    x = torch.rand(1, 3, 128, 256, generator=G(9710)).to(DEV)
    t = torch.randint(0, 19, (1, 128, 256), generator=G(9711)).to(DEV)
    keys = []
    for _ in range(2):                                                       # a second wrapper captures under the same keys
        served = GraphedModel(model, masks=True, num_classes=19, criterion=crit)
        served.evaluate(x, t)
        served.validate(x, t)
        keys.append(list(served._graphs))
    assert keys[0] == keys[1] == [
        ('evaluate', (1, 3, 128, 256), torch.float32, torch.int64, DEV, None, (1, 128, 256)),
        ('validate', (1, 3, 128, 256), torch.float32, torch.int64, DEV, None, (1, 128, 256), crit.k, crit.thresh, crit.ignore_index, None)]
    # an encoded colour-codec target (3-D) is not raw: the same keys with a colour codec set
    try:
        model.label_codec = MODEL_CODECS['colors']
        served = GraphedModel(model, masks=True, num_classes=19, criterion=crit)
        served.evaluate(x, t)
        assert list(served._graphs) == keys[0][:1]
    finally:
        model.label_codec = None
