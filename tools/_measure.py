"""The measurement protocol of the tools/*_time.py family, written once.

A leg is timed as a region of ``reps`` calls: device events around it (``region_ms``) or a host clock (``wall_ms``, ``protocol_ms``,
``host_ms``).  Every leg of a group is warmed before anything is timed, the legs are timed INTERLEAVED (round r times every leg in turn),
and each leg is reported with its median and its spread (max - min over the rounds).  A difference between two legs is believed only
where it exceeds the sum of the two spreads (``exceeds``, ``verdict``).  The whole-frame check is ``bench.py`` of the parent tree and of
this one in fresh child processes, alternating (``compare_bench``).  The tools hold their workloads, their legs, their byte arithmetic and
their assertions; nothing here falls back to anything where no GPU is found (``require_gpu``)."""
import json
import os
import statistics
import subprocess
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)


def require_gpu(tool):
    if not torch.cuda.is_available():
        raise SystemExit(f'{tool} measures on the GPU: no device found')


# ---- timers: (fn, reps) -> ms per call
def region_ms(fn, reps):
    """Two device events around ``reps`` calls."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def wall_ms(fn, reps):
    """The host clock around ``reps`` calls between two synchronisations."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / reps


def protocol_ms(fn, reps):
    """The reference's frame protocol: synchronize -> perf_counter -> call -> synchronize, per call."""
    total = 0.0
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        total += time.perf_counter() - t0
    return 1e3 * total / reps


def host_ms(fn, reps):
    """The host clock; no device involved."""
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return 1e3 * (time.perf_counter() - t0) / reps


def per_launch(launches):
    """The timer of a leg that replays a graph of ``launches`` calls: ``region_ms`` over the launches of a replay."""
    return lambda fn, reps: region_ms(fn, reps) / launches


# ---- the report
class Lines(list):
    """The report: every line is printed as it is added, so a long run shows where it is."""

    def append(self, line):
        print(line, flush=True)
        super().append(line)


def report(lines, title, samples):
    """One line per leg of ``samples`` (name -> list of ms), indented under ``title`` where there is one; -> (medians, spreads)."""
    indent = '' if title is None else '  '
    if title is not None:
        lines.append(title)
    width = max(map(len, samples), default=0)
    med, spread = {}, {}
    for k, s in samples.items():
        med[k], spread[k] = statistics.median(s), max(s) - min(s)
        lines.append(f'{indent}{k:{width}s} median {med[k]:.4f}  min {min(s):.4f}  max {max(s):.4f}  spread {spread[k]:.4f}   samples ' +
                     ' '.join(f'{v:.4f}' for v in s))
    return med, spread


def interleaved(lines, title, variants, rounds, warmup):
    """variants: name -> (timer, fn, reps).  Every leg warm before anything is timed, then round r times every leg in turn."""
    for _, fn, _ in variants.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    samples = {k: [] for k in variants}
    for _ in range(rounds):
        for k, (timer, fn, reps) in variants.items():
            samples[k].append(timer(fn, reps))
    return report(lines, title, samples)


def exceeds(a, b, med, spread):
    """The rule of this project: leg ``a`` is above leg ``b`` only where the medians differ by more than the sum of the two spreads."""
    return med[a] - med[b] > spread[a] + spread[b]


def verdict(name, a, b, med, spread):
    """'(b) - (a) = difference, summed spreads: within / beyond', the rule read in both directions."""
    beyond = exceeds(a, b, med, spread) or exceeds(b, a, med, spread)
    return f'{name} = {med[b] - med[a]:+.4f} ms, summed spreads {spread[a] + spread[b]:.4f}: {"beyond" if beyond else "within"}'


def write_report(lines, out):
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    text = '\n'.join(lines)
    with open(out, 'w') as f:
        f.write(text + '\n')


# ---- graphs and launch counts
def graph_of(fn, launches, warm=3):
    """``launches`` calls of ``fn`` captured into one graph after ``warm`` eager calls, replayed once."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(launches):
            fn()
    graph.replay()
    return graph


def count_launches(lib, names, fn, weight=lambda name, args: 1):
    """Launches made through the library entries ``names`` while ``fn`` runs: name -> count.  Every call of an entry counts as
    ``weight(name, args)`` launches."""
    counts, saved = {}, {}
    for name in names:
        saved[name] = real = getattr(lib, name)

        def counting(*a, _real=real, _name=name):
            counts[_name] = counts.get(_name, 0) + weight(_name, a)
            return _real(*a)
        setattr(lib, name, counting)
    try:
        fn()
    finally:
        for name, real in saved.items():
            setattr(lib, name, real)
    return counts


# ---- bench.py of two trees
def bench_value(tree):
    """``value`` of the last JSON line that ``bench.py`` of ``tree`` prints, run as a fresh child process."""
    out = subprocess.run([sys.executable, 'bench.py', '--gpus', '1', '--steps', '200', '--warmup', '20'], cwd=tree, capture_output=True,
                         text=True, timeout=300, check=True).stdout
    return float(json.loads([ln for ln in out.splitlines() if ln.startswith('{')][-1])['value'])


def compare_bench(lines, parent_tree, rounds, unit='frames/s'):
    """``bench.py`` of ``parent_tree`` (a checkout of the parent commit, built) and of this tree, alternating, ``rounds`` times each.
    -> the error that stopped the comparison early, for ``main`` to raise once the report is written, or None."""
    if not parent_tree:
        lines.append('bench.py: no --parent-tree given, not compared in this run')
        return None
    vals, error = {'parent': [], 'this tree': []}, None
    try:
        for _ in range(rounds):
            vals['parent'].append(bench_value(parent_tree))
            vals['this tree'].append(bench_value(REPO))
    except (subprocess.SubprocessError, ValueError, IndexError, KeyError) as e:
        error = e
    lines.append(f'bench.py --gpus 1 --steps 200 --warmup 20, fresh processes, alternating, {rounds} each; {unit}')
    for k, s in vals.items():
        if s:
            lines.append(f'  {k:10s} median {statistics.median(s):.2f}  min {min(s):.2f}  max {max(s):.2f}   samples ' + ' '.join(f'{v:.2f}' for v in s))
    if error is not None:
        lines.append(f'  the comparison stopped early: {type(error).__name__}')
    return error
