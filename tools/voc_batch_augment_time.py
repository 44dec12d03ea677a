"""What augmenting a VOC-SBD training batch costs: the HyperSeg-L train chain (flip -> ColorJitter -> RandomResize(0.25..0.9) ->
RandomRotation(30) -> ConstantPad(512) -> ToTensor -> Normalize) at batch 32 on a 500 x 500 canvas holding a mix of 500x375 and 375x500
frames, flips, scales and angles drawn fresh per batch, once without and once with colour jitter (all four operations).

    timeout -k 10 1100 python tools/voc_batch_augment_time.py [--rounds 7] [--reps 5] [--parent-tree DIR] [--out profiles/voc_batch_augment_time.txt]

One process, the routes timed INTERLEAVED (``--rounds`` rounds, each round one sample of every route):
  (a) ``training.device_augment_voc`` on the list of cropped (contiguous) frames, fresh draws: the per-sample route and the yardstick --
      WALL time per batch (host clock around the call and a synchronisation) and device events;
  (b) ``training.BatchAugmentVOC.__call__`` on the canvas with the same kind of draws: wall time and device events;
  (c) ``BatchAugmentVOC.run`` captured once and replayed after ``upload`` of new parameters: device events per upload + replay;
  (d) each new launch alone, a graph of 50: device events per launch.
Also: the library launches of one call of (a) and of (b), counted at the ctypes boundary (every entry makes one launch, the jitter entries
three when they are given a sums workspace); what ``utils.resample._DEVICE_TABLES`` holds after ``--growth-batches`` batches of (a)
against (b)'s fixed workspace; (b)'s result against (a)'s on every sample, byte for byte (asserted).  With ``--parent-tree`` (a checkout
of the parent commit, built): ``python bench.py --gpus 1 --steps 200 --warmup 20`` of that tree and of this one, fresh child processes,
alternating, ``--bench-rounds`` times each."""
import argparse
import os

import torch

from _measure import (REPO, Lines, compare_bench, count_launches, exceeds, graph_of, interleaved, per_launch, region_ms, report, require_gpu,
                      wall_ms, write_report)

COUNTED = ('hs_frame_resize_fwd', 'hs_label_resize_fwd', 'hs_color_jitter_fwd', 'hs_frame_rotate_fwd', 'hs_label_rotate_fwd',
           'hs_resize_tables_ragged_fwd', 'hs_color_jitter_ragged_fwd', 'hs_frame_resize_ragged_fwd', 'hs_label_resize_ragged_fwd',
           'hs_frame_rotate_ragged_fwd', 'hs_label_rotate_ragged_fwd')
SUMS_ARG = {'hs_color_jitter_fwd': 6, 'hs_color_jitter_ragged_fwd': 7}


def launches_of(name, args):
    """Every entry makes one launch, the jitter entries three when they are given a sums workspace."""
    return 3 if name in SUMS_ARG and args[SUMS_ARG[name]] is not None else 1


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--growth-batches', type=int, default=20)
    ap.add_argument('--parent-tree', default=None)
    ap.add_argument('--bench-rounds', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'voc_batch_augment_time.txt'))
    args = ap.parse_args()
    require_gpu('voc_batch_augment_time.py')
    from hyperseg_amd import _hip
    from hyperseg_amd import functional as HF
    from hyperseg_amd.training import BatchAugmentVOC, device_augment_voc, draw_color_jitter
    from hyperseg_amd.utils import resample
    from hyperseg_amd.utils.inference import InputNorm
    dev = torch.device('cuda:0')
    b, canvas_hw, pad, lo, hi = 32, (500, 500), 512, 0.25, 0.9
    layout = 'hwc'
    norm = InputNorm(layout=layout)
    g = torch.Generator().manual_seed(1)
    sizes = [(375, 500) if i % 2 == 0 else (500, 375) for i in range(b)]
    frames = torch.randint(0, 256, (b,) + canvas_hw + (3,), generator=g, dtype=torch.uint8).to(dev)
    labels = torch.randint(0, 21, (b,) + canvas_hw, generator=g, dtype=torch.uint8).to(dev)
    ragged = [frames[i, :h, :w].contiguous() for i, (h, w) in enumerate(sizes)]
    lragged = [labels[i, :h, :w].contiguous() for i, (h, w) in enumerate(sizes)]
    aug = BatchAugmentVOC(canvas_hw, pad, norm, (lo, hi))

    def draw(jitter):
        """Flips, scales, angles and (``jitter``) four-operation ColorJitters: a new set per call."""
        u = torch.rand(b, 3, generator=g, dtype=torch.float64).tolist()
        return ([f[0] < 0.5 for f in u], [draw_color_jitter(0.4, 0.4, 0.4, 0.1, generator=g) for _ in range(b)] if jitter else None,
                [lo + (hi - lo) * f[1] for f in u], [-30.0 + 60.0 * f[2] for f in u])

    def route_a(p):
        return device_augment_voc(ragged, lragged, p[0], p[1], p[2], p[3], pad, norm)

    def route_b(p):
        return aug(frames, labels, sizes, *p)

    lines = Lines()
    lines.append(f'VOC-SBD HyperSeg-L train chain, batch {b}, a {canvas_hw[1]}x{canvas_hw[0]} uint8 {layout} canvas of 500x375 and 375x500 frames -> '
                 f'{pad}x{pad}, scales uniform in ({lo}, {hi}) and angles in +-30 drawn fresh per batch; {args.rounds} interleaved rounds; '
                 f'ks_max {aug.ks_max}')
    same, counts_b_all = True, {}
    launches = 50
    for jitter in (False, True):
        tag = 'with jitter (4 operations)' if jitter else 'without jitter'
        p0 = draw(jitter)
        want, got = route_a(p0), route_b(p0)
        eq = all(torch.equal(want[0][i], got[0][i]) and torch.equal(want[1][i], got[1][i]) for i in range(b))
        same = same and eq
        lines.append(f'--- {tag}')
        lines.append(f'(b) equals (a) on every sample, image and label, byte for byte: {eq}; status all zero: {not bool(aug.status.any())}')
        counts_a = count_launches(_hip.run, COUNTED, lambda: route_a(draw(jitter)), weight=launches_of)
        counts_b = count_launches(_hip.run, COUNTED, lambda: route_b(draw(jitter)), weight=launches_of)
        counts_b_all[jitter] = sum(counts_b.values())
        lines.append(f'library launches per batch, (a): {sum(counts_a.values())} {counts_a};  (b): {sum(counts_b.values())} {counts_b}')

        for _ in range(2):
            aug.run(frames, labels, jitter=jitter)
        out = (torch.empty(b, 3, pad, pad, device=dev), torch.empty(b, pad, pad, dtype=torch.int64, device=dev))
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            aug.run(frames, labels, out=out, jitter=jitter)
        staged = [aug.rows(sizes, *draw(jitter)) for _ in range(args.rounds * args.reps)]
        cursor = [0]

        def route_c():
            aug.upload(staged[cursor[0] % len(staged)])
            cursor[0] += 1
            graph.replay()

        keys = {'aw': '(a) device_augment_voc, fresh draws, WALL per batch', 'ae': '(a) device_augment_voc, fresh draws, device events',
                'bw': '(b) BatchAugmentVOC.__call__, fresh draws, WALL per batch', 'be': '(b) BatchAugmentVOC.__call__, fresh draws, device events',
                'c': '(c) upload + graph replay of run, new params, device events'}
        samples = {k: [] for k in keys.values()}
        for _ in range(args.rounds):
            samples[keys['aw']].append(wall_ms(lambda: route_a(draw(jitter)), 1))
            samples[keys['ae']].append(region_ms(lambda: route_a(draw(jitter)), 1))
            samples[keys['bw']].append(wall_ms(lambda: route_b(draw(jitter)), 1))
            samples[keys['be']].append(region_ms(lambda: route_b(draw(jitter)), args.reps))
            samples[keys['c']].append(region_ms(route_c, args.reps))
        med, spread = report(lines, f'ms per batch of {b} (draw() itself, host, is inside the fresh-draw legs of both routes)', samples)
        for name, ka, kb in (('wall', keys['aw'], keys['bw']), ('device events', keys['ae'], keys['be'])):
            diff, both = med[ka] - med[kb], spread[ka] + spread[kb]
            verdict = 'faster than (a) by more than the sum of the two spreads' if exceeds(ka, kb, med, spread) else \
                'NOT faster than (a) by more than the sum of the two spreads'
            lines.append(f'  {name}: (a) / (b) = {med[ka] / med[kb]:.1f}x  ({med[ka]:.3f} -> {med[kb]:.3f} ms); (a) - (b) = {diff:+.4f} ms, sum of the '
                         f'two spreads {both:.4f}: (b) is {verdict}')

    # (d) each new launch alone
    p, t, mid = aug.params, aug.tables, (pad, pad)
    alone = {
        'hs_resize_tables_ragged_fwd': lambda: HF.resize_tables_ragged(p.rows, canvas_hw, mid, 'bicubic', aug.ks_max, workspace=aug.workspace),
        'hs_color_jitter_ragged_fwd (clear + mean + apply)': lambda: HF.color_jitter_ragged(frames, p.rows, p.jitter, layout, out=aug._jittered, sums=aug._sums),
        'hs_color_jitter_ragged_fwd (apply alone)': lambda: HF.color_jitter_ragged(frames, p.rows, p.jitter, layout, contrast=False, out=aug._jittered),
        'hs_frame_resize_ragged_fwd': lambda: HF.frame_resize_ragged(frames, p.rows, t, layout, out=aug._mid),
        'hs_label_resize_ragged_fwd': lambda: HF.label_resize_ragged(labels, p.rows, t, out=aug._mid_label),
        'hs_frame_rotate_ragged_fwd': lambda: HF.frame_rotate_ragged(aug._mid, p.rows, t, p.matrices, layout, mid, norm=norm, out=out[0]),
        'hs_label_rotate_ragged_fwd': lambda: HF.label_rotate_ragged(aug._mid_label, p.rows, t, p.fixed, mid, out=out[1]),
    }
    legs = {f'(d) {name}': (per_launch(launches), graph_of(fn, launches, warm=1).replay, args.reps) for name, fn in alone.items()}
    med_d, _ = interleaved(lines, f'--- each new launch alone, ms per launch (graph of {launches}), the last drawn parameters (with jitter)', legs,
                           args.rounds, warmup=0)
    lines.append(f'  the longest: {max(med_d, key=med_d.get)}')

    before = sum(x.numel() * x.element_size() for v in resample._DEVICE_TABLES.values() for x in v)
    n_before = len(resample._DEVICE_TABLES)
    for _ in range(args.growth_batches):
        route_a(draw(False))
    torch.cuda.synchronize()
    after = sum(x.numel() * x.element_size() for v in resample._DEVICE_TABLES.values() for x in v)
    held = sum(x.numel() * x.element_size() for x in (aug.workspace, aug.buffer, aug._mid, aug._mid_label, aug._jittered, aug._sums))
    lines.append(f'_DEVICE_TABLES: {n_before} entries / {before / 1e6:.2f} MB before, {len(resample._DEVICE_TABLES)} entries / {after / 1e6:.2f} MB after '
                 f'{args.growth_batches} more batches of (a) = {(after - before) / 1e3 / args.growth_batches:.0f} KB per batch, never freed;  '
                 f"(b)'s workspace {aug.workspace.numel() * 4 / 1e6:.2f} MB, with its canvases and parameters {held / 1e6:.2f} MB, fixed")

    bench_error = compare_bench(lines, args.parent_tree, args.bench_rounds)
    write_report(lines, args.out)
    assert same, 'BatchAugmentVOC disagrees with device_augment_voc'
    assert counts_b_all == {False: 5, True: 8}, f'BatchAugmentVOC made {counts_b_all} launches, expected 5 without and 8 with jitter'
    if bench_error is not None:
        raise bench_error


if __name__ == '__main__':
    with torch.no_grad():
        main()
