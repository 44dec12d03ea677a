"""On-device evaluation (csrc/hs_eval.hip): the confusion matrix counted from finished masks (hs_confusion_fwd) and inside the
final upsample + arg-max launch (hs_upsample_confusion_fwd), through functional, the models' ``evaluate``, fps.ConfusionMatrix
and GraphedModel.evaluate.  Every matrix and mask comparison is ``torch.equal`` on integers."""
import pytest
import torch

from conftest import G
from hyperseg_amd.utils.synthetic import fill_by_name

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
MODELS = {'M': 'hyperseg-m', 'S': 'hyperseg-s', 'L': 'hyperseg-l', 'Lc': 'hyperseg-l-camvid'}


def _stock(target, pred, n):
    """The stock CPU ConfusionMatrix (the reference's routine) fed ``target`` and ``pred``."""
    from hyperseg_amd.fps import ConfusionMatrix
    cm = ConfusionMatrix(n)
    cm.update_stock(target.cpu().flatten().long(), pred.cpu().flatten().long())
    return cm.mat


def _targets(pattern, b, h, w, n, seed, dtype=torch.int64):
    """uniform: every pixel its own class; ignored: 15 % of 255; rects: piecewise constant -- a few large rectangles (the
    one-bin-per-wave case), one of them 255."""
    g = G(seed)
    t = torch.randint(0, n, (b, h, w), generator=g)
    if pattern == 'ignored':
        t[torch.rand(b, h, w, generator=g) < 0.15] = 255
    elif pattern == 'rects':
        t[:] = 0
        for k in range(6):
            y0, x0 = int(torch.randint(0, max(1, h - 1), (1,), generator=g)), int(torch.randint(0, max(1, w - 1), (1,), generator=g))
            t[:, y0:y0 + max(2, h // 2), x0:x0 + max(2, w // 3)] = 255 if k == 3 else int(torch.randint(0, n, (1,), generator=g))
    else:
        assert pattern == 'uniform'
    return t.to(dtype)


def _logits(b, c, h, w, seed):
    # smooth + noise: neighbouring pixels mostly share their arg-max, as real logits do, with ties impossible in practice
    g = G(seed)
    coarse = torch.randn(b, c, max(1, h // 4), max(1, w // 4), generator=g)
    x = torch.nn.functional.interpolate(coarse, size=(h, w), mode='bilinear') + 0.1 * torch.randn(b, c, h, w, generator=g)
    return x.contiguous()


def test_confusion_update_reference_fixture(golden):
    """hs_confusion_fwd on the reference's own fixture: ``mat`` exactly, for int64 and uint8 storage of both operands,
    accumulated over the three batches into one ``out``; compute() at the existing test's 1e-7 (test_oracle_golden.py:261-262)."""
    from hyperseg_amd import functional as HF
    from hyperseg_amd.fps import ConfusionMatrix
    g = golden('confusion_matrix')
    n = int(g['mat'].shape[0])
    for pd in (torch.int64, torch.uint8):
        for td in (torch.int64, torch.uint8):
            out = torch.zeros(n, n, dtype=torch.int64, device=DEV)
            for t, p in zip(g['target'], g['pred']):
                r = HF.confusion_update(p.to(pd).to(DEV), t.to(td).to(DEV), n, out=out)
                assert r is out
            assert torch.equal(out.cpu(), g['mat']), (pd, td)
    cm = ConfusionMatrix(n)
    for t, p in zip(g['target'], g['pred']):
        cm.update(t.flatten().to(DEV), p.flatten().to(DEV))             # CUDA operands: the kernel route
    assert cm.mat.is_cuda and torch.equal(cm.mat.cpu(), g['mat'])
    acc_global, acc, iu = cm.compute()
    assert abs(float(acc_global) - float(g['acc_global'])) < 1e-7
    assert torch.allclose(acc.cpu(), g['acc'], rtol=0, atol=1e-7) and torch.allclose(iu.cpu(), g['iu'], rtol=0, atol=1e-7)
    mats = cm.update_per_image(g['target'][0].to(DEV), g['pred'][0].to(DEV))
    for b in range(mats.shape[0]):
        assert torch.equal(mats[b].cpu(), _stock(g['target'][0][b], g['pred'][0][b], n))


SHAPES = [  # (C, n, B, Hi, Wi, Ho, Wo)
    (3, 3, 1, 16, 24, 32, 48),          # exact 2x
    (12, 12, 3, 16, 24, 32, 48),
    (19, 19, 1, 20, 36, 40, 72),
    (21, 21, 3, 12, 16, 24, 32),
    (19, 19, 3, 24, 40, 24, 40),        # identity resize
    (12, 12, 1, 24, 38, 24, 38),        # identity, Wo % 4 != 0
    (19, 19, 1, 16, 24, 40, 56),        # non-2x ratio
    (21, 21, 3, 10, 14, 25, 37),        # non-2x, Wo % 4 != 0
    (5, 19, 1, 16, 24, 32, 48),         # C < n
    (5, 21, 3, 16, 24, 23, 30),         # C < n, general form
    (19, 64, 1, 16, 24, 32, 48),        # the largest n the issue requires of the LDS form
    (19, 19, 1, 16, 25, 32, 50),        # 2x with an odd input width: the general form
]


@pytest.mark.parametrize('pattern', ['uniform', 'ignored', 'rects'])
@pytest.mark.parametrize('tdtype', [torch.int64, torch.uint8])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_upsample_confusion_equals_its_parts(shape, tdtype, pattern):
    """upsample_confusion(masks=True) == upsample_argmax + the stock CPU ConfusionMatrix.update: masks bit-identical, matrices
    equal."""
    from hyperseg_amd import functional as HF
    c, n, b, hi, wi, ho, wo = shape
    x = _logits(b, c, hi, wi, 7000 + c + hi).to(DEV)
    t = _targets(pattern, b, ho, wo, n, 7100 + n + ho, tdtype)
    ref_masks = HF.upsample_argmax(x, (ho, wo))
    out, masks = HF.upsample_confusion(x, (ho, wo), t.to(DEV), n, masks=True)
    assert masks.dtype == torch.uint8 and torch.equal(masks, ref_masks)
    want = _stock(t, ref_masks, n)
    assert out.dtype == torch.int64 and torch.equal(out.cpu(), want)
    assert torch.equal(HF.upsample_confusion(x, (ho, wo), t.to(DEV), n).cpu(), want)         # without the mask output
    assert torch.equal(HF.confusion_update(ref_masks, t.to(DEV), n).cpu(), want)             # from the finished masks


@pytest.mark.parametrize('pattern', ['uniform', 'ignored', 'rects'])
def test_upsample_confusion_full_size(pattern):
    from hyperseg_amd import functional as HF
    x = _logits(1, 19, 256, 512, 7200).to(DEV)
    t = _targets(pattern, 1, 512, 1024, 19, 7201)
    ref_masks = HF.upsample_argmax(x, (512, 1024))
    out, masks = HF.upsample_confusion(x, (512, 1024), t.to(DEV), 19, masks=True)
    want = _stock(t, ref_masks, 19)
    assert torch.equal(masks, ref_masks) and torch.equal(out.cpu(), want)
    assert int(want.sum()) == int(((t >= 0) & (t < 19)).sum())
    assert torch.equal(HF.confusion_update(ref_masks, t.to(torch.uint8).to(DEV), 19).cpu(), want)


def second_trip_shape(mapping, batch):
    """(Hi, Wi, Ho, Wo) whose items per image exceed one pass of the scoring grid -- ceil(CUs / batch) workgroups per image of 512
    items (rows of four) or 128 (quads) -- so the grid-stride loop takes a second trip, with surplus lanes on it.  Rows of four: a general
    ratio and Wo % 4 == 2; quads: exact 2x."""
    per_image = -(-torch.cuda.get_device_properties(DEV).multi_processor_count // batch)
    if mapping == 'quads':
        wi = 258
        hi = per_image * 128 // (wi // 2) + 3
        assert hi * (wi // 2) > per_image * 128
        return hi, wi, 2 * hi, 2 * wi
    wo = 518
    ho = per_image * 512 // ((wo + 3) // 4) + 3
    assert ho * ((wo + 3) // 4) > per_image * 512
    return ho // 3 + 1, wo // 3 + 1, ho, wo


@pytest.mark.parametrize('tdtype', [torch.int64, torch.uint8])
@pytest.mark.parametrize('mapping', ['rows4', 'quads'])
def test_upsample_confusion_second_grid_trip(mapping, tdtype):
    """Batch 2, C = 5 < n = 21, more items per image than one pass of the grid: masks and matrix as the parts give them."""
    from hyperseg_amd import functional as HF
    hi, wi, ho, wo = second_trip_shape(mapping, 2)
    x = _logits(2, 5, hi, wi, 7300).to(DEV)
    t = _targets('ignored', 2, ho, wo, 21, 7301, tdtype)
    ref_masks = HF.upsample_argmax(x, (ho, wo))
    out, masks = HF.upsample_confusion(x, (ho, wo), t.to(DEV), 21, masks=True)
    assert torch.equal(masks, ref_masks) and torch.equal(out.cpu(), _stock(t, ref_masks, 21))
    slabs = HF.upsample_confusion(x, (ho, wo), t.to(DEV), 21, per_image=True)
    for b in range(2):
        assert torch.equal(slabs[b].cpu(), _stock(t[b], ref_masks[b], 21))


@pytest.mark.parametrize('size', [(32, 48), (25, 37)])
def test_accumulation_and_per_image(size):
    """Two calls into one ``out`` = the sum; per_image slabs sum to the (n, n) result and slab b equals a call on image b alone."""
    from hyperseg_amd import functional as HF
    n, b = 12, 3
    ho, wo = size
    x1, x2 = _logits(b, n, 16, 24, 7300).to(DEV), _logits(b, n, 16, 24, 7301).to(DEV)
    t1, t2 = _targets('ignored', b, ho, wo, n, 7302).to(DEV), _targets('rects', b, ho, wo, n, 7303).to(DEV)
    a, m1 = HF.upsample_confusion(x1, size, t1, n, masks=True)
    c, m2 = HF.upsample_confusion(x2, size, t2, n, masks=True)
    both = HF.upsample_confusion(x1, size, t1, n)
    r = HF.upsample_confusion(x2, size, t2, n, out=both)
    assert r is both and torch.equal(both, a + c)
    slabs = HF.upsample_confusion(x1, size, t1, n, per_image=True)
    assert tuple(slabs.shape) == (b, n, n) and torch.equal(slabs.sum(0), a)
    slabs2 = HF.confusion_update(m1, t1, n, per_image=True)
    assert torch.equal(slabs2, slabs)
    for i in range(b):
        assert torch.equal(slabs[i], HF.upsample_confusion(x1[i:i + 1].contiguous(), size, t1[i:i + 1].contiguous(), n))
        assert torch.equal(slabs[i].cpu(), _stock(t1[i], m1[i], n))
    HF.confusion_update(m2, t2, n, out=slabs, per_image=True)
    assert torch.equal(slabs.sum(0), a + c)


def _model(tag, prepared=False):
    from hyperseg_amd import configs
    m = fill_by_name(configs.build(MODELS[tag]).eval(), seed=11)
    if prepared:
        from hyperseg_amd.utils.inference import prepare_for_inference
        prepare_for_inference(m, fold_bn=False, fused_depthwise=True)
    return m.to(DEV)


def _model_targets(x, n, seed):
    g = G(seed)
    t = torch.randint(0, n, (x.shape[0],) + tuple(x.shape[2:]), generator=g)
    t[torch.rand(t.shape, generator=g) < 0.10] = 255
    return t


@pytest.mark.parametrize('tag,prepared', [('M', False), ('S', False), ('L', False), ('Lc', False), ('M', True)])
def test_model_evaluate(golden, tag, prepared):
    """model.evaluate(x, t, cm) returns exactly model.segment(x), and cm.mat equals a stock CPU ConfusionMatrix fed t and
    model(x).argmax(1); per_image=True books the same counts image by image."""
    from hyperseg_amd import configs
    from hyperseg_amd.fps import ConfusionMatrix
    g = golden(f'model_{tag}')
    m = _model(tag, prepared)
    n = configs.MODELS[MODELS[tag]]['num_classes']
    x = g['x'].to(DEV)
    t = _model_targets(x, n, 7400)
    cm = ConfusionMatrix(n)
    with torch.no_grad():
        masks = m.evaluate(x, t.to(DEV), cm)
        seg = m.segment(x)
        ref = m(x).argmax(1)
    assert masks.dtype == torch.uint8 and torch.equal(masks, seg)
    want = _stock(t, ref, n)
    assert cm.mat.is_cuda and torch.equal(cm.mat.cpu(), want)
    cm2 = ConfusionMatrix(n)
    m.evaluate(x, t.to(torch.uint8).to(DEV), cm2, per_image=True)
    assert torch.equal(cm2.mat.cpu(), want) and len(cm2.per_image) == 1
    for b in range(x.shape[0]):
        assert torch.equal(cm2.per_image[0][b].cpu(), _stock(t[b], ref[b], n))


def test_model_evaluate_fallback_routes(golden):
    """The routes the fused launch does not serve give the matrix of their own masks: a two-scale list input with
    inference_hflip, a target at half size (the LOGITS are resized to it, test.py:167-168), and n = 129, the smallest number
    of classes the LDS form refuses (stock counting)."""
    from hyperseg_amd import functional as HF
    from hyperseg_amd.fps import ConfusionMatrix
    g = golden('model_M_pyramid')
    m = _model('M')
    assert m.inference_hflip
    xs = [g['x0'].to(DEV), g['x1'].to(DEV)]
    n = 19
    t = _model_targets(xs[0], n, 7500)
    cm = ConfusionMatrix(n)
    with torch.no_grad():
        masks = m.evaluate(xs, t.to(DEV), cm)
        ref = m(xs).argmax(1)
    assert masks.dtype == torch.uint8 and torch.equal(masks.long(), ref)
    assert torch.equal(cm.mat.cpu(), _stock(t, ref, n))
    # half-size target
    x = xs[0]
    hh, hw = x.shape[2] // 2, x.shape[3] // 2
    th = _model_targets(x[:, :, :hh, :hw], n, 7501)
    cm = ConfusionMatrix(n)
    with torch.no_grad():
        masks = m.evaluate(x, th.to(DEV), cm, per_image=True)
        ref = HF.upsample_bilinear(m(x).contiguous(), (hh, hw)).argmax(1)
    assert tuple(masks.shape) == tuple(th.shape) and torch.equal(masks.long(), ref)
    assert torch.equal(cm.mat.cpu(), _stock(th, ref, n)) and tuple(cm.per_image[0].shape) == (x.shape[0], n, n)
    # more classes than the LDS histogram holds
    big = HF.eval_max_classes() + 1
    assert big == 129
    with pytest.raises(NotImplementedError):
        HF.confusion_update(masks, th.to(DEV), big)
    tb = torch.randint(0, big, (x.shape[0],) + tuple(x.shape[2:]), generator=G(7502))
    cm = ConfusionMatrix(big)
    with torch.no_grad():
        masks = m.evaluate(x, tb.to(DEV), cm)
        seg = m.segment(x)
    assert torch.equal(masks, seg) and torch.equal(cm.mat.cpu(), _stock(tb, seg, big))


@pytest.mark.parametrize('per_image', [False, True])
def test_graphed_evaluate(golden, per_image):
    """GraphedModel.evaluate over 6 distinct frames (pinned-host and device inputs) == the eager sum: warm-up and capture leaked
    no counts; reset_confusion() works; forward graphs of the same wrapper still replay afterwards."""
    from hyperseg_amd.fps import ConfusionMatrix
    from hyperseg_amd.utils.inference import GraphedModel
    m = _model('M', prepared=True)
    n = 19
    served = GraphedModel(m, masks=True, num_classes=n, per_image=per_image, clone_output=True)
    gx = G(7600)
    frames = [torch.rand(1, 3, 128, 256, generator=gx) for _ in range(6)]
    targets = [_model_targets(f, n, 7601 + i) for i, f in enumerate(frames)]
    eager = ConfusionMatrix(n)
    for rounds in range(2):
        want_masks = []
        for f, t in zip(frames, targets):
            want_masks.append(m.evaluate(f.to(DEV), t.to(DEV), eager))
        for i, (f, t) in enumerate(zip(frames, targets)):
            xin, tin = (f.pin_memory(), t.pin_memory()) if i % 2 == 0 else (f.to(DEV), t.to(DEV))
            masks = served.evaluate(xin, tin)
            assert torch.equal(masks, want_masks[i])
        torch.cuda.synchronize()
        got = served.confusion.sum(0) if per_image else served.confusion
        assert tuple(served.confusion.shape) == ((1, n, n) if per_image else (n, n))
        assert torch.equal(got, eager.mat)
        assert sum(1 for k in served._graphs if k[0] == 'evaluate') == 1
        served.reset_confusion()
        eager.reset()
        assert int(served.confusion.sum()) == 0
    out = served(frames[0].to(DEV))
    again = served(frames[0].to(DEV))
    assert torch.equal(out, m.segment(frames[0].to(DEV))) and torch.equal(out, again)
    assert torch.equal(served.evaluate(frames[1].to(DEV), targets[1].to(DEV)), m.segment(frames[1].to(DEV)))
    assert int(served.confusion.sum()) == int((targets[1] != 255).sum())
    # what the graph cannot serve is scored eagerly into the same matrix: a target at half size
    before = served.confusion.clone()
    th = targets[2][:, :64, :128].contiguous()
    cm = ConfusionMatrix(n)
    m.evaluate(frames[2].to(DEV), th.to(DEV), cm)
    served.evaluate(frames[2].to(DEV), th.to(DEV))
    assert torch.equal((served.confusion - before).reshape(-1, n, n).sum(0), cm.mat)


def test_evaluate_is_capturable():
    """A plain torch.cuda.graph capture of model.evaluate: the fused route has no synchronisation (a device-to-host read under
    capture raises); replays accumulate."""
    from hyperseg_amd.fps import ConfusionMatrix
    m = _model('M')
    n = 19
    x = torch.rand(1, 3, 128, 256, generator=G(7700)).to(DEV)
    t = _model_targets(x, n, 7701).to(DEV)
    warm, cm = ConfusionMatrix(n), ConfusionMatrix(n)
    cm.matrix(DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        for _ in range(2):
            m.evaluate(x, t, warm)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(graph):
        masks = m.evaluate(x, t, cm)
    assert int(cm.mat.sum()) == 0                       # the capture itself counted nothing
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(cm.mat * 2, warm.mat * 2) and torch.equal(cm.mat, warm.mat)
    with torch.no_grad():
        assert torch.equal(masks, m.segment(x))


def test_argument_errors():
    """C > n, float targets, CPU tensors, a wrong ``out``: raised before anything is launched (``out`` stays zero)."""
    from hyperseg_amd import functional as HF
    from hyperseg_amd._hip import HipLibraryError
    x = _logits(1, 5, 8, 12, 7800).to(DEV)
    t = _targets('uniform', 1, 16, 24, 5, 7801).to(DEV)
    out = torch.zeros(4, 4, dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError):
        HF.upsample_confusion(x, (16, 24), t, 4, out=out)                            # C > n
    with pytest.raises(ValueError):
        HF.upsample_confusion(x, (16, 24), t.float(), 5)
    with pytest.raises(ValueError):
        HF.upsample_confusion(x, (16, 24), t.to(torch.int32), 5)
    with pytest.raises(ValueError):
        HF.upsample_confusion(x, (16, 24), t.cpu(), 5)
    with pytest.raises((ValueError, HipLibraryError)):
        HF.upsample_confusion(x.cpu(), (16, 24), t, 5)
    with pytest.raises(ValueError):
        HF.upsample_confusion(x, (16, 24), t[:, :8], 5)                              # target of another size
    with pytest.raises(ValueError):
        HF.upsample_confusion(x, (16, 24), t, 5, out=out)                            # (4, 4) for n = 5
    with pytest.raises(ValueError):
        HF.upsample_confusion(x, (16, 24), t, 5, out=torch.zeros(5, 5, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError):
        HF.upsample_confusion(x, (16, 24), t, 5, out=torch.zeros(5, 5, dtype=torch.int64), per_image=False)      # CPU out
    with pytest.raises(ValueError):
        HF.upsample_confusion(x, (16, 24), t, 5, out=torch.zeros(5, 5, dtype=torch.int64, device=DEV), per_image=True)
    p = torch.zeros(1, 16, 24, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError):
        HF.confusion_update(p, t.float(), 5)
    with pytest.raises(ValueError):
        HF.confusion_update(p.cpu(), t.cpu(), 5)
    with pytest.raises(ValueError):
        HF.confusion_update(p[:, :8], t, 5)
    with pytest.raises(ValueError):
        HF.confusion_update(p, t, 5, out=out)
    assert int(out.sum()) == 0
    # the C entry refuses the same on its own (nothing launched: status before any launch)
    from hyperseg_amd import _hip
    good = torch.zeros(5, 5, dtype=torch.int64, device=DEV)
    st = _hip.lib.hs_upsample_confusion_fwd(x.data_ptr(), 1, 5, 8, 12, 16, 24, t.data_ptr(), 1, 4, 0, good.data_ptr(), None, None)
    assert st == -1
    st = _hip.lib.hs_upsample_confusion_fwd(x.data_ptr(), 1, 5, 8, 12, 16, 24, t.data_ptr(), 7, 5, 0, good.data_ptr(), None, None)
    assert st == -1
    st = _hip.lib.hs_confusion_fwd(p.data_ptr(), 0, t.data_ptr(), 1, 1, 16 * 24, 129, 0, good.data_ptr(), None)
    assert st == -3
    torch.cuda.synchronize()
    assert int(good.sum()) == 0
