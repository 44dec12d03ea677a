"""The FPS harness with labels of another size than the frames' (hyperseg_amd.fps: ``synthetic_batches(label_size=)``,
``measure_fps``): the logits are resized to the label before the arg-max, as test.py:167-168 does before ``conf.update``.  CPU only."""
import torch

from conftest import G


def _toy():
    net = torch.nn.Sequential(torch.nn.Conv2d(3, 5, 1))
    with torch.no_grad():
        for q in net.parameters():
            q.copy_(torch.rand(q.shape, generator=G(2034)) - 0.5)
    return net.eval()


def test_measure_fps_scores_at_the_label_size():
    """4 x 6 frames with 8 x 12 targets: the accuracy and mean IoU of F.interpolate(net(x), (8, 12), 'bilinear').argmax(1), counted by
    hand here; ``label_size`` appears in the result."""
    from hyperseg_amd.fps import measure_fps, synthetic_batches
    net, n = _toy(), 5
    batches = synthetic_batches(3, 2, (4, 6), n, torch.device('cpu'), seed=3, label_size=(8, 12))
    assert all(tuple(x.shape) == (2, 3, 4, 6) and tuple(t.shape) == (2, 8, 12) for x, t in batches)
    res = measure_fps(net, batches, torch.device('cpu'), n)
    mat = torch.zeros(n, n, dtype=torch.int64)
    with torch.no_grad():
        for x, t in batches:
            pred = torch.nn.functional.interpolate(net(x), size=(8, 12), mode='bilinear').argmax(1)
            for a, b in zip(t.flatten().tolist(), pred.flatten().tolist()):
                mat[a, b] += 1
    h = mat.float()
    diag = torch.diag(h)
    acc = diag.sum() / h.sum()
    iou = diag / (h.sum(1) + h.sum(0) - diag + 1e-6)
    assert int(mat.sum()) == 3 * 2 * 8 * 12 and res['frames'] == 6
    assert res['global_accuracy'] == float(acc) and res['mean_iou'] == float(iou.mean())
    assert res['label_size'] == [8, 12]
    same = measure_fps(net, batches, torch.device('cpu'), n, fused_metrics=True)        # no evaluate on the toy net: the same route
    assert same['mean_iou'] == res['mean_iou'] and same['label_size'] == [8, 12]


def test_synthetic_batches_without_a_label_size_are_unchanged():
    """label_size=None: the same bytes as before the argument existed (restated draw order), and the frames' size in the result."""
    from hyperseg_amd.fps import measure_fps, synthetic_batches
    got = synthetic_batches(2, 2, (4, 6), 5, torch.device('cpu'), seed=7)
    same = synthetic_batches(2, 2, (4, 6), 5, torch.device('cpu'), seed=7, label_size=None)
    g = torch.Generator().manual_seed(7)
    for (x, t), (x2, t2) in zip(got, same):
        wx = torch.rand(2, 3, 4, 6, generator=g)
        wt = torch.randint(0, 5, (2, 4, 6), generator=g)
        assert torch.equal(x, wx) and torch.equal(t, wt) and torch.equal(x2, wx) and torch.equal(t2, wt)
    u8 = synthetic_batches(1, 2, (4, 6), 5, torch.device('cpu'), seed=7, uint8=True, label_size=(8, 12))
    assert u8[0][0].dtype == torch.uint8 and tuple(u8[0][0].shape) == (2, 4, 6, 3) and tuple(u8[0][1].shape) == (2, 8, 12)
    assert measure_fps(_toy(), got, torch.device('cpu'), 5)['label_size'] == [4, 6]
