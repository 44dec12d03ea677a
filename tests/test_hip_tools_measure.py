"""tools/_measure.py on the device: the timers run ``fn`` exactly ``reps`` times and have synchronised when they return; ``graph_of``
captures exactly ``launches`` calls.  Counted with an in-place add, whose result is exact in float32 at these sizes."""
import math
import os
import sys

import pytest
import torch

TOOLS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools')
if TOOLS not in sys.path:
    sys.path.insert(0, TOOLS)

import _measure as M  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


@pytest.mark.parametrize('timer', [M.region_ms, M.wall_ms], ids=['region_ms', 'wall_ms'])
def test_timer_runs_fn_reps_times_and_synchronises(timer):
    t = torch.zeros(1024, device=DEV)
    ms = timer(lambda: t.add_(1), 8)
    assert torch.cuda.current_stream().query()                     # nothing of the region is still in flight
    assert math.isfinite(ms) and ms > 0
    assert torch.equal(t.cpu(), torch.full((1024,), 8.0))


def test_graph_of_captures_exactly_launches_calls():
    t = torch.zeros(1024, device=DEV)

    def fn():
        t.add_(1)
    graph = M.graph_of(fn, launches=4, warm=3)
    torch.cuda.synchronize()
    assert torch.equal(t.cpu(), torch.full((1024,), 7.0))          # 3 warm calls + the helper's own first replay of 4; the capture adds none
    t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(t.cpu(), torch.full((1024,), 4.0))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(t.cpu(), torch.full((1024,), 8.0))
