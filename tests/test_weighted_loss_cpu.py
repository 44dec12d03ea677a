"""Class weights in the criterion, the parts that need no GPU: the composed route against the reference's fixture
(tests/golden/make_weighted_loss_golden.py), the rule that decides which tables the HIP routes take, and the epilogue's argument check."""
import pytest
import torch

from conftest import rel_err


def fixture_cases(g):
    for i in range(int(g['cases'])):
        c = {k: g[f'case{i}_{k}'] for k in ('logits', 'target', 'weight', 'loss', 'grad')}
        c.update(k=int(g[f'case{i}_k']), thresh=float(g[f'case{i}_thresh']), ignore=int(g[f'case{i}_ignore']))
        yield i, c


def test_fixture_is_what_the_issue_describes(golden):
    g = golden('weighted_loss')
    shapes = [tuple(c['logits'].shape) for _, c in fixture_cases(g)]
    assert shapes == [(2, 12, 16, 24), (2, 19, 9, 11), (1, 21, 7, 13), (2, 5, 3, 70)]
    for _, c in fixture_cases(g):
        n, ch, h, w = c['logits'].shape
        assert c['k'] < h * w and int((c['weight'] == 0).sum()) == 1 and float(c['weight'].max()) < 4.2
        assert 0.1 < float((c['target'] == c['ignore']).float().mean()) < 0.3
    assert sorted(c['ignore'] for _, c in fixture_cases(g)) == [-100, 255, 255, 255]
    assert sorted(c['thresh'] for _, c in fixture_cases(g)) == [0.3, 0.3, 0.3, 5.0]


def test_weighted_criterion_on_cpu_reproduces_the_reference(golden):
    """The composed route (F.cross_entropy with the table, then the top-k rule) against the reference's loss and gradient."""
    from hyperseg_amd.training import BootstrappedCrossEntropyLoss
    for i, c in fixture_cases(golden('weighted_loss')):
        crit = BootstrappedCrossEntropyLoss(k=c['k'], thresh=c['thresh'], weight=c['weight'].clone(), ignore_index=c['ignore'])
        x = c['logits'].clone().requires_grad_()
        loss = crit(x, c['target'])
        loss.backward()
        want, got = float(c['loss']), float(loss.detach())
        print(f'case {i}: loss {got:.8f} ref {want:.8f} grad rel_err {rel_err(x.grad, c["grad"]):.2e}')
        assert abs(got - want) <= 1e-6 * abs(want), i
        assert rel_err(x.grad, c['grad']) < 1e-6, i


def test_weight_fusable_rule():
    """fp32 (C,) on the logits' device, finite and >= 0 (a zero is fine): everything else keeps the composed route."""
    from hyperseg_amd.training import weight_fusable
    cpu = torch.device('cpu')
    w = torch.tensor([1.0, 0.0, 2.5, 0.4])
    assert weight_fusable(w, 4, cpu) is True
    assert weight_fusable(torch.tensor([1.0, -0.1, 2.5, 0.4]), 4, cpu) is False
    assert weight_fusable(torch.tensor([1.0, float('inf'), 2.5, 0.4]), 4, cpu) is False
    assert weight_fusable(torch.tensor([1.0, float('nan'), 2.5, 0.4]), 4, cpu) is False
    assert weight_fusable(w.double(), 4, cpu) is False
    assert weight_fusable(torch.ones(5), 4, cpu) is False
    assert weight_fusable(w.view(1, 4), 4, cpu) is False
    assert weight_fusable(torch.ones(8)[::2], 4, cpu) is False              # not contiguous
    assert weight_fusable(w, 4, torch.device('cuda', 0)) is False           # a CPU table against CUDA logits
    assert weight_fusable(None, 4, cpu) is False
    assert weight_fusable(w, 4, cpu) is True                                # pure: the same answer again


def test_criterion_asks_once_per_table(monkeypatch):
    """The value test reads the device, so the criterion keeps its answer per (address, version) of the buffer."""
    from hyperseg_amd import training
    crit = training.BootstrappedCrossEntropyLoss(k=4, weight=torch.tensor([1.0, 0.0, 2.0]))
    calls = []
    real = training.weight_fusable
    monkeypatch.setattr(training, 'weight_fusable', lambda *a: calls.append(1) or real(*a))
    cpu = torch.device('cpu')
    assert crit.weight_takes_hip(3, cpu) and crit.weight_takes_hip(3, cpu) and len(calls) == 1
    crit.weight.mul_(2)                                                      # in place: a new version, asked again
    assert crit.weight_takes_hip(3, cpu) and len(calls) == 2
    crit.weight[1] = -1.0
    assert not crit.weight_takes_hip(3, cpu) and len(calls) == 3
    monkeypatch.setattr(training, 'USE_HIP_CLASS_WEIGHTS', False)            # the switch: today's routing
    crit.weight[1] = 1.0
    assert not crit.weight_takes_hip(3, cpu) and len(calls) == 3
    assert not training.BootstrappedCrossEntropyLoss().weight_takes_hip(3, cpu)


def test_inference_mode_table_takes_the_composed_route():
    """A buffer made under torch.inference_mode() keeps no version counter: its changes could not be seen, so it is not fusable -- and
    the criterion computes what it computed before."""
    from hyperseg_amd import training
    with torch.inference_mode():
        w = torch.tensor([1.0, 0.0, 2.0])
    crit = training.BootstrappedCrossEntropyLoss(k=4, weight=w)
    assert not crit.weight_takes_hip(3, torch.device('cpu'))
    x, t = torch.randn(1, 3, 4, 4, generator=torch.Generator().manual_seed(1)), torch.zeros(1, 4, 4, dtype=torch.int64)
    assert bool(torch.isfinite(crit(x, t)))


def test_epilogue_weight_needs_the_loss():
    from hyperseg_amd.models._common import Epilogue, Score
    w = torch.ones(3)
    target = torch.zeros(1, 4, 4, dtype=torch.int64)
    with pytest.raises(ValueError):
        Epilogue(weight=w)
    with pytest.raises(ValueError):
        Epilogue(Score(target, 3, None, False), weight=w)                    # a score, but no ignore_index: no loss is made
    with pytest.raises(ValueError):
        Epilogue(ignore_index=255, weight=w)
    assert Epilogue(Score(target, 3, None, False), ignore_index=255, weight=w).weight is w
