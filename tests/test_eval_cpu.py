"""Evaluation metrics of hyperseg_amd.fps off the GPU: the stock confusion matrix (unchanged route for CPU operands), the
per-image matrices and Jaccard score of the reference's test.py, the cross-process reduction, and the ``fused_metrics``
switch of the FPS harness falling back on a model that has no ``evaluate``."""
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp

from conftest import G


def _ref_calc_conf_mat(target, pred, num_classes, ignore_index=None):
    """hyperseg/test.py:210-216, restated (test.py itself imports torchvision and cannot be imported here)."""
    mask = (target >= 0) & (target < num_classes)
    if ignore_index is not None:
        mask &= (target != ignore_index)
    inds = num_classes * target[mask].to(torch.int64) + pred[mask]
    return torch.bincount(inds, minlength=num_classes ** 2).reshape(num_classes, num_classes)


def _ref_jaccard(target, pred_labels, num_classes, ignore_index=None, eps=1e-6):
    """hyperseg/test.py:219-227, restated; ``pred_labels`` is already ``pred.argmax(1)``."""
    confmat = _ref_calc_conf_mat(target.flatten(), pred_labels.flatten(), num_classes, ignore_index)
    inter = torch.diag(confmat)
    union = confmat.sum(1) + confmat.sum(0) - inter
    if ignore_index is not None and ignore_index < len(union):
        union[ignore_index] = 0
    score = inter / (union + eps)
    return torch.mean(score[union > 0])


def test_confusion_matrix_cpu_route_unchanged(golden):
    """CPU operands: the reference's fixture (int64 targets with 255s, a never-predicted class) is reproduced exactly, by
    ``update`` and by the stock routine it keeps for them; ``matrix()`` creates ``mat`` as ``update`` does."""
    from hyperseg_amd.fps import ConfusionMatrix
    g = golden('confusion_matrix')
    n = int(g['mat'].shape[0])
    cm, stock = ConfusionMatrix(n), ConfusionMatrix(n)
    assert cm.mat is None
    for t, p in zip(g['target'], g['pred']):
        cm.update(t.flatten(), p.flatten())
        stock.update_stock(t.flatten(), p.flatten())
    assert torch.equal(cm.mat, g['mat']) and torch.equal(stock.mat, g['mat'])
    acc_global, acc, iu = cm.compute()
    assert abs(float(acc_global) - float(g['acc_global'])) < 1e-7
    assert torch.allclose(acc, g['acc'], rtol=0, atol=1e-7) and torch.allclose(iu, g['iu'], rtol=0, atol=1e-7)
    fresh = ConfusionMatrix(n)
    m = fresh.matrix(torch.device('cpu'))
    assert m is fresh.mat and m.dtype == torch.int64 and tuple(m.shape) == (n, n) and int(m.sum()) == 0


@pytest.mark.parametrize('ignore_index', [0, None])
def test_jaccard_per_image_matches_test_py(golden, ignore_index):
    """``update_per_image`` + ``jaccard_per_image`` == the reference's per-image ``jaccard`` (restated above), on the
    fixture's batches plus an image in which a class has an empty union (never a target, never predicted).  Float32
    quotients averaged in a different order: 4 ulp of float32 at a score <= 1 is the bound (4 * 2^-24 < 3e-7)."""
    from hyperseg_amd.fps import ConfusionMatrix, jaccard_per_image
    g = golden('confusion_matrix')
    n = int(g['mat'].shape[0])
    targets, preds = [t.clone() for t in g['target']], [p.clone() for p in g['pred']]
    t0, p0 = targets[0], preds[0]
    t0[0][t0[0] == n - 1] = 1                   # image 0 of batch 0: class n - 1 in neither operand -> empty union
    p0[0][p0[0] == n - 1] = 1
    assert not bool((t0[0] == n - 1).any()) and not bool((p0[0] == n - 1).any())
    cm, total = ConfusionMatrix(n), ConfusionMatrix(n)
    want = []
    for t, p in zip(targets, preds):
        mats = cm.update_per_image(t, p)
        assert tuple(mats.shape) == (t.shape[0], n, n) and mats.dtype == torch.int64
        total.update(t.flatten(), p.flatten())
        for b in range(t.shape[0]):
            want.append(_ref_jaccard(t[b].unsqueeze(0), p[b].unsqueeze(0), n, ignore_index))
            assert torch.equal(mats[b], _ref_calc_conf_mat(t[b].flatten(), p[b].flatten(), n))
    assert torch.equal(cm.mat, total.mat)
    all_mats = cm.per_image_matrices()
    assert all_mats.shape[0] == len(want) and torch.equal(all_mats.sum(0), total.mat)
    got = jaccard_per_image(all_mats, ignore_index=ignore_index)
    want = torch.stack(want)
    assert got.shape == want.shape and not bool(torch.isnan(want).any())
    assert float((got - want).abs().max()) < 3e-7
    cm.reset()
    assert cm.per_image == [] and int(cm.mat.sum()) == 0


def _free_port():
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


def _reduce_worker(rank, world, port, out_dir):
    import torch.distributed as dist
    from hyperseg_amd.fps import ConfusionMatrix
    os.environ['MASTER_ADDR'], os.environ['MASTER_PORT'] = '127.0.0.1', str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        cm = ConfusionMatrix(4)
        t = torch.randint(0, 4, (200,), generator=G(5000 + rank))
        p = torch.randint(0, 4, (200,), generator=G(6000 + rank))
        cm.update(t, p)
        cm.reduce_from_all_processes()
        torch.save(cm.mat, os.path.join(out_dir, f'mat{rank}.pt'))
    finally:
        dist.destroy_process_group()


def test_reduce_from_all_processes_gloo(tmp_path):
    """seg_utils.py:38-44: uninitialised -> no-op; on a gloo group of two, both ranks end with the sum of the two matrices."""
    from hyperseg_amd.fps import ConfusionMatrix
    world = 2
    parts = []
    for rank in range(world):
        cm = ConfusionMatrix(4)
        cm.update(torch.randint(0, 4, (200,), generator=G(5000 + rank)), torch.randint(0, 4, (200,), generator=G(6000 + rank)))
        before = cm.mat.clone()
        assert not torch.distributed.is_initialized()
        cm.reduce_from_all_processes()
        assert torch.equal(cm.mat, before)
        parts.append(before)
    mp.spawn(_reduce_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    for rank in range(world):
        assert torch.equal(torch.load(os.path.join(str(tmp_path), f'mat{rank}.pt')), parts[0] + parts[1])


def test_measure_fps_fused_metrics_falls_back_on_cpu():
    """``fused_metrics=True`` on a model without ``evaluate`` (the CPU toy net of the existing harness test) scores the frames
    as before: same mean IoU and global accuracy as ``fused_metrics=False``."""
    from hyperseg_amd.fps import measure_fps
    net = torch.nn.Sequential(torch.nn.Conv2d(3, 5, 1))
    with torch.no_grad():
        for q in net.parameters():
            q.copy_(torch.rand(q.shape, generator=G(1034)) - 0.5)
    gx, gt = G(1032), G(1033)
    batches = [(torch.rand(2, 3, 4, 6, generator=gx), torch.randint(0, 5, (2, 4, 6), generator=gt)) for _ in range(3)]
    plain = measure_fps(net.eval(), batches, torch.device('cpu'), 5)
    fused = measure_fps(net.eval(), batches, torch.device('cpu'), 5, fused_metrics=True)
    assert fused['frames'] == plain['frames'] == 6
    assert fused['mean_iou'] == plain['mean_iou'] and fused['global_accuracy'] == plain['global_accuracy']
