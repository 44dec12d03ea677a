"""What augmenting a training batch costs when every sample draws a scale of its own: the Cityscapes HyperSeg-S shape -- batch 16,
1024 x 2048 uint8 frames, 768 x 768 crops, bicubic, scales drawn fresh per batch from (0.375, 1.5).

    timeout -k 10 900 python tools/batch_augment_time.py [--rounds 7] [--reps 5] [--parent-tree DIR] [--out profiles/batch_augment_time.txt]

One process, the routes timed INTERLEAVED (``--rounds`` rounds, each round one sample of every route):
  (a) ``training.device_augment`` as a user runs it: new scales, offsets and flips every batch, so its four host tables per sample are
      built, uploaded and kept; WALL time per batch (host clock around the call and a synchronisation);
  (b) ``training.device_augment`` with one fixed parameter set, tables warm: device events around the call (the README's case) -- the
      yardstick, parent code;
  (c) ``training.BatchAugment.__call__`` with the same fresh draws as (a): wall time per batch, and device events;
  (d) ``training.BatchAugment.run`` captured once and replayed with new parameters copied into ``params``: device events per replay;
  (e) the table launch alone, a graph of 50: device events per launch (it prices the serial nearest chain).
Also: the library launches of one call of (a) and of (c), counted at the ctypes boundary (every entry counted makes exactly one kernel
launch); the bytes ``utils.resample._DEVICE_TABLES`` holds after ``--growth-batches`` batches of (a) against (c)'s workspace; (c)'s
result against (a)'s, byte for byte (asserted).  With ``--parent-tree`` (a checkout of the parent commit, built): ``python bench.py
--gpus 1 --steps 200 --warmup 20`` of that tree and of this one, fresh child processes, alternating, ``--bench-rounds`` times each."""
import argparse
import os

import torch

from _measure import REPO, Lines, compare_bench, count_launches, exceeds, graph_of, region_ms, report, require_gpu, wall_ms, write_report

COUNTED = ('hs_frame_resize_fwd', 'hs_label_resize_fwd', 'hs_resize_tables_fwd', 'hs_frame_resize_batch_fwd', 'hs_label_resize_batch_fwd')


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--growth-batches', type=int, default=100)
    ap.add_argument('--parent-tree', default=None)
    ap.add_argument('--bench-rounds', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'batch_augment_time.txt'))
    args = ap.parse_args()
    require_gpu('batch_augment_time.py')
    from hyperseg_amd import _hip
    from hyperseg_amd import functional as HF
    from hyperseg_amd.training import BatchAugment, device_augment
    from hyperseg_amd.utils import resample
    from hyperseg_amd.utils.inference import InputNorm
    dev = torch.device('cuda:0')
    b, (hi, wi), crop, lo, hi_s = 16, (1024, 2048), (768, 768), 0.375, 1.5
    norm = InputNorm(layout='hwc')
    g = torch.Generator().manual_seed(1)
    frames = torch.randint(0, 256, (b, hi, wi, 3), generator=g, dtype=torch.uint8).to(dev)
    labels = torch.randint(0, 19, (b, hi, wi), generator=g, dtype=torch.uint8).to(dev)
    aug = BatchAugment((hi, wi), crop, norm, (lo, hi_s))

    def draw():
        """Scales, crop offsets as RandomCrop(pad_if_needed) places them, flips: a new set per call."""
        scales = (lo + (hi_s - lo) * torch.rand(b, generator=g, dtype=torch.float64)).tolist()
        u = torch.rand(b, 3, generator=g, dtype=torch.float64).tolist()
        offsets = []
        for s, (uy, ux, _) in zip(scales, u):
            hr, wr = aug._resized(s)
            offsets.append((int(uy * (max(hr, crop[0]) - crop[0] + 1)), int(ux * (max(wr, crop[1]) - crop[1] + 1))))
        return scales, offsets, [f[2] < 0.5 for f in u]

    def route_a(p):
        return device_augment(frames, labels, p[0], crop, p[1], p[2], norm)

    def route_c(p):
        return aug(frames, labels, *p)

    lines = Lines()
    lines.append(f'Cityscapes HyperSeg-S train chain, batch {b}, {wi}x{hi} uint8 hwc frames -> {crop[1]}x{crop[0]} crops, bicubic, scales uniform in '
                 f'({lo}, {hi_s}) drawn fresh per batch; {args.rounds} interleaved rounds; ks_max {aug.ks_max}')
    p0 = draw()
    want, got = route_a(p0), route_c(p0)
    same = torch.equal(want[0], got[0]) and torch.equal(want[1], got[1])
    lines.append(f'(c) equals (a), image and label, byte for byte: {same}; status all zero: {not bool(aug.status.any())}')
    counts_a = count_launches(_hip.run, COUNTED, lambda: route_a(draw()))
    counts_c = count_launches(_hip.run, COUNTED, lambda: route_c(draw()))
    lines.append(f'library launches per batch, (a): {sum(counts_a.values())} {counts_a};  (c): {sum(counts_c.values())} {counts_c}')

    fixed = (0.75, (0, 384), False)                               # tools/color_jitter_time.py's (c): the README's 0.636 ms case
    for _ in range(3):
        route_a(fixed)
        aug.run(frames, labels)
    out = (torch.empty(b, 3, *crop, device=dev), torch.empty(b, *crop, dtype=torch.int64, device=dev))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        aug.run(frames, labels, out=out)
    launches = 50
    tgraph = graph_of(lambda: HF.resize_tables(aug.params, (hi, wi), crop, 'bicubic', aug.ks_max, workspace=aug.workspace), launches, warm=0)
    staged = [aug.rows(*draw()).to(dev) for _ in range(args.rounds)]

    keys = {'a': '(a) device_augment, fresh draws, WALL per batch',
            'b': '(b) device_augment, one fixed parameter set (warm tables), device events',
            'cw': '(c) BatchAugment.__call__, fresh draws, WALL per batch',
            'ce': '(c) BatchAugment.__call__, fresh draws, device events',
            'd': '(d) BatchAugment.run, graph replay with new params, device events',
            'e': f'(e) hs_resize_tables_fwd alone, per launch (graph of {launches}), device events'}
    samples = {k: [] for k in keys.values()}
    for r in range(args.rounds):
        samples[keys['a']].append(wall_ms(lambda: route_a(draw()), 1))
        samples[keys['b']].append(region_ms(lambda: route_a(fixed), args.reps))
        samples[keys['cw']].append(wall_ms(lambda: route_c(draw()), 1))
        samples[keys['ce']].append(region_ms(lambda: route_c(draw()), args.reps))
        aug.params.copy_(staged[r])
        samples[keys['d']].append(region_ms(graph.replay, args.reps))
        samples[keys['e']].append(region_ms(tgraph.replay, args.reps) / launches)
    med, spread = report(lines, 'ms per batch of 16 (draw() itself, host, is inside the fresh-draw legs of both routes)', samples)
    a, bb, cw, ce = (keys[k] for k in ('a', 'b', 'cw', 'ce'))
    lines.append(f'  (a) / (c) wall = {med[a] / med[cw]:.1f}x  ({med[a]:.3f} -> {med[cw]:.3f} ms): the user-visible number')
    for name, k in (('(c) device events', ce), ('(d) graph replay', keys['d'])):
        diff, both = med[bb] - med[k], spread[bb] + spread[k]
        verdict = 'beats (b) by more than the sum of the two spreads' if exceeds(bb, k, med, spread) else \
            'is SLOWER than (b) by more than the sum of the two spreads' if exceeds(k, bb, med, spread) else 'does NOT beat (b) by more than the sum of the two spreads'
        lines.append(f'  (b) - {name} = {diff:+.4f} ms, sum of the two spreads {both:.4f}: {name} {verdict}')

    before = sum(t.numel() * t.element_size() for v in resample._DEVICE_TABLES.values() for t in v)
    n_before = len(resample._DEVICE_TABLES)
    for _ in range(args.growth_batches):
        route_a(draw())
    torch.cuda.synchronize()
    after = sum(t.numel() * t.element_size() for v in resample._DEVICE_TABLES.values() for t in v)
    lines.append(f'_DEVICE_TABLES: {n_before} entries / {before / 1e6:.2f} MB before, {len(resample._DEVICE_TABLES)} entries / {after / 1e6:.2f} MB after '
                 f'{args.growth_batches} more batches of (a) = {(after - before) / 1e3 / args.growth_batches:.0f} KB per batch, never freed;  '
                 f"(c)'s workspace: {aug.workspace.numel() * 4 / 1e6:.2f} MB, fixed")

    bench_error = compare_bench(lines, args.parent_tree, args.bench_rounds)
    write_report(lines, args.out)
    assert same, 'BatchAugment disagrees with device_augment'
    assert sum(counts_c.values()) == 3, f'BatchAugment made {counts_c} launches, expected 3'
    if bench_error is not None:
        raise bench_error


if __name__ == '__main__':
    with torch.no_grad():
        main()
