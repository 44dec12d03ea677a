"""The validation step's host side on CPU tensors: training.running_scores against train.py's runningScore.get_scores, the loss
module's ``score`` attribute on its stock route, HyperGenBase.validate's composed route, and the argument errors."""
import numpy as np
import pytest
import torch

from conftest import G


def _ref_get_scores(hist):
    """hyperseg/train.py:310-335 (runningScore.get_scores) restated on a float numpy matrix."""
    hist = np.asarray(hist, dtype=np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        acc = np.diag(hist).sum() / hist.sum()
        acc_cls = np.diag(hist) / hist.sum(axis=1)
        acc_cls = np.nanmean(acc_cls)
        iu = np.diag(hist) / (hist.sum(axis=1) + hist.sum(axis=0) - np.diag(hist))
        mean_iu = np.nanmean(iu)
        freq = hist.sum(axis=1) / hist.sum()
        fwavacc = (freq[freq > 0] * iu[freq > 0]).sum()
    return {'overall_acc': acc, 'mean_acc': acc_cls, 'freqw_acc': fwavacc, 'mean_iou': mean_iu}, dict(zip(range(hist.shape[0]), iu))


def _same(a, b):
    return (np.isnan(a) and np.isnan(b)) or abs(a - b) <= 1e-12 * max(1.0, abs(b))


@pytest.mark.parametrize('case', ['random5', 'random19', 'empty_row', 'zero_column', 'empty_class'])
def test_running_scores_matches_train_py(case):
    """float64 on both sides: agreement to 1e-12 relative (the two sum in different orders), nan where numpy gives nan."""
    from hyperseg_amd.training import running_scores
    n = 19 if case == 'random19' else 5
    mat = torch.randint(0, 1000, (n, n), generator=G(9000 + n))
    if case == 'empty_row':
        mat[2, :] = 0                 # no pixel of class 2: nan in the class accuracy, left out of the mean
    elif case == 'zero_column':
        mat[:, 3] = 0                 # class 3 never predicted: IoU 0, not nan
    elif case == 'empty_class':
        mat[1, :] = 0
        mat[:, 1] = 0                 # neither labelled nor predicted: nan accuracy AND nan IoU
    want, want_iu = _ref_get_scores(mat.numpy())
    got, got_iu = running_scores(mat)
    assert set(got) == set(want)
    for k in want:
        assert _same(got[k], float(want[k])), (k, got[k], want[k])
    assert list(got_iu) == list(range(n))
    for c in range(n):
        assert _same(got_iu[c], float(want_iu[c])), c
    if case == 'empty_class':
        assert np.isnan(got_iu[1]) and not np.isnan(got['mean_iou'])
    if case == 'zero_column':
        assert got_iu[3] == 0.0
    with pytest.raises(ValueError):
        running_scores(torch.zeros(3, 4))


def _stock(target, pred, n):
    from hyperseg_amd.fps import ConfusionMatrix
    cm = ConfusionMatrix(n)
    cm.update_stock(target.flatten().long(), pred.flatten().long())
    return cm.mat


@pytest.mark.parametrize('ignore_index', [255, 2, -1])
def test_criterion_score_on_cpu(ignore_index):
    """The stock route: the loss is the unscored module's; the matrix is update_stock's of (target, argmax).  An in-range ignore_index is
    COUNTED (runningScore does not know it) while its loss is 0; targets 255 and -1 are never counted."""
    from hyperseg_amd.fps import ConfusionMatrix
    from hyperseg_amd.training import BootstrappedCrossEntropyLoss
    n, c = 7, 5
    g = G(9100)
    pred = torch.randn(2, c, 9, 11, generator=g)
    t_loss = torch.randint(0, c, (2, 9, 11), generator=g)
    t_loss[0, 0, :4] = ignore_index          # (F.cross_entropy takes no other out-of-range value: the GPU tests mix them)
    t_loss[1, 3, 2:6] = ignore_index
    plain = BootstrappedCrossEntropyLoss(k=32, thresh=0.3, ignore_index=ignore_index)
    scored = BootstrappedCrossEntropyLoss(k=32, thresh=0.3, ignore_index=ignore_index)
    assert scored.score is None
    scored.score = ConfusionMatrix(n)
    want_loss = plain(pred, t_loss)
    got_loss = scored(pred, t_loss)
    assert torch.equal(got_loss, want_loss)
    assert torch.equal(scored.score.mat, _stock(t_loss, pred.argmax(1), n))
    valid = int(((t_loss >= 0) & (t_loss < n)).sum())
    assert int(scored.score.mat.sum()) == valid
    if ignore_index == 2:
        assert int(scored.score.mat[2].sum()) == int((t_loss == 2).sum()) > 0        # counted, loss 0
        per = torch.nn.functional.cross_entropy(pred, t_loss, ignore_index=2, reduction='none')
        assert float(per[t_loss == 2].abs().max()) == 0.0
    scored(pred, t_loss)
    assert int(scored.score.mat.sum()) == 2 * valid                                # accumulates
    scored.score.reset()
    assert int(scored.score.mat.sum()) == 0
    assert 'score' not in scored.state_dict() and list(scored.state_dict()) == list(plain.state_dict())
    scored.score = ConfusionMatrix(c - 1)                                           # C > n
    with pytest.raises(ValueError):
        scored(pred, t_loss)


def _toy_model():
    """A HyperGenBase whose single-tensor pass is a CPU 1x1 convolution (tests/test_eval_cpu.py's toy net under the models' wrapper):
    every route of the wrapper that does not need the GPU."""
    from hyperseg_amd.models._common import Epilogue, HyperGenBase

    class Toy(HyperGenBase):
        def __init__(self):
            super().__init__()
            self.net = torch.nn.Conv2d(3, 5, 1)

        def process_single_tensor(self, x, hflip=False, epilogue=None):
            assert not hflip and epilogue in (None, Epilogue()), 'CPU: nothing rides on the epilogue'
            y = self.net(x)
            return y.argmax(1).to(torch.uint8) if epilogue is not None else y

    m = Toy()
    with torch.no_grad():
        for q in m.parameters():
            q.copy_(torch.rand(q.shape, generator=G(9200)) - 0.5)
    return m.eval()


def test_model_validate_on_cpu():
    from hyperseg_amd.fps import ConfusionMatrix
    from hyperseg_amd.training import BootstrappedCrossEntropyLoss
    m = _toy_model()
    n = 5
    x = torch.rand(2, 3, 12, 10, generator=G(9201))
    t = torch.randint(0, n, (2, 12, 10), generator=G(9202))
    t[0, :2] = 255
    crit = BootstrappedCrossEntropyLoss(k=16, thresh=0.3, ignore_index=255)
    with torch.no_grad():
        want_loss, want_masks = crit(m(x), t), m(x).argmax(1)
    for tt in (t, t.to(torch.uint8)):
        cm, cm_eval = ConfusionMatrix(n), ConfusionMatrix(n)
        loss, masks = m.validate(x, tt, crit, cm)
        assert loss.dim() == 0 and not loss.requires_grad and torch.equal(loss, want_loss)
        assert masks.dtype == torch.uint8 and torch.equal(masks.long(), want_masks)
        m.evaluate(x, tt, cm_eval)
        assert torch.equal(cm.mat, cm_eval.mat) and int(cm.mat.sum()) == int((t != 255).sum())
    loss, masks = m.validate(x, t, crit)                                          # confmat=None
    assert torch.equal(loss, want_loss) and torch.equal(masks.long(), want_masks)
    cm = ConfusionMatrix(n)
    m.validate(x, t, crit, cm, per_image=True)
    assert tuple(cm.per_image[0].shape) == (2, n, n) and torch.equal(cm.per_image[0].sum(0), cm_eval.mat)
    # a target of another size: the logits are resized to it
    th = t[:, ::2, ::2].contiguous()
    cm = ConfusionMatrix(n)
    loss, masks = m.validate(x, th, crit, cm)
    with torch.no_grad():
        pred = torch.nn.functional.interpolate(m(x), size=th.shape[1:], mode='bilinear')
    assert torch.equal(loss, crit(pred, th)) and torch.equal(masks.long(), pred.argmax(1))
    # training mode: the composed route as well, and no graph is kept
    m.train()
    loss, _ = m.validate(x, t, crit)
    assert not loss.requires_grad and torch.equal(loss, want_loss)


def test_argument_errors():
    from hyperseg_amd.fps import ConfusionMatrix
    from hyperseg_amd.training import BootstrappedCrossEntropyLoss
    from hyperseg_amd.utils.inference import GraphedModel
    m = _toy_model()
    crit = BootstrappedCrossEntropyLoss(k=16, ignore_index=255)
    x = torch.rand(1, 3, 8, 8, generator=G(9300))
    t = torch.randint(0, 5, (1, 8, 8), generator=G(9301))
    with pytest.raises(ValueError, match='criterion'):
        GraphedModel(m).validate(x, t)
    loss, masks = GraphedModel(m, criterion=crit, num_classes=5).validate(x, t)    # a CPU model: model.validate's routes
    assert torch.equal(loss, crit(m(x), t).detach()) and tuple(masks.shape) == (1, 8, 8)
    with pytest.raises(ValueError, match='target'):
        m.validate(x, t.float(), crit)                                            # a float target
    with pytest.raises(ValueError, match='target'):
        m.validate(x, t[0], crit, ConfusionMatrix(5))                             # no batch dimension
    with pytest.raises(ValueError, match='target'):
        m.validate(x, torch.cat([t, t]), crit)                                    # another batch size
    scored = BootstrappedCrossEntropyLoss(k=16, ignore_index=255)
    scored.score = ConfusionMatrix(4)
    with pytest.raises(ValueError, match='classes'):
        scored(m(x), t)                                                           # C = 5 > n = 4
