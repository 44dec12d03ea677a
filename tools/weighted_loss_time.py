"""What class weights cost the HIP loss routes: the training step, the validation batch and the benchmark.

    timeout -k 10 1100 python tools/weighted_loss_time.py [--rounds 7] [--reps 100] [--parent DIR] [--out profiles/weighted_loss_time.txt]

One visit; the legs of each group timed INTERLEAVED (round r times every leg in turn, ``--rounds`` rounds), each sample a region of
``--reps`` steps between two device events (tools/_measure.py's protocol).  No threshold is asserted: the numbers are the record.
``training.USE_HIP_CLASS_WEIGHTS = False`` is the same-tree stand-in for the route a weighted criterion took before the weighted
kernels: F.cross_entropy with the table, stock adjoints, argmax + ConfusionMatrix.update, the composed validation.
Config 5 (CamVid-S decoder, 576 x 576, batch 2) through GraphedTrainStep, a RANDOM 12-entry table of CamVid's shape (11 weights in
(0.4, 4.2) and a 0 for Void; not the reference's numbers, which cannot change the timing), in fp32 and under fp16 autocast with a GradScaler:
  (u) no weights, fused route: the yardstick;
  (w) weights, fused route (the weighted twins of the loss launches);
  (s) weights, switch off.
HyperSeg-M, 1024 x 512, batch 1, prepared, a 19-entry table, GraphedModel.validate:
  (vu) no weights;  (vw) weights, one replay;  (vs) weights, switch off (model.validate's composed route, eager).
``--parent DIR`` (a built checkout of the parent commit): ``bench.py --gpus 1 --steps 200 --warmup 20 --no-cpu-baseline`` in fresh
processes, parent and this tree alternating, three runs each; medians of ``value`` (frames/s).
Reported: medians, spreads (max - min over the rounds), (w) - (u) and (s) - (w) against the summed spreads."""
import argparse
import copy
import json
import os
import statistics
import subprocess
import sys

import torch

from _measure import REPO, Lines, interleaved, region_ms, require_gpu, verdict, write_report

sys.path.insert(0, os.path.join(REPO, 'tests'))


def table(n, seed, dev):
    w = torch.rand(n, generator=torch.Generator().manual_seed(seed)) * 3.8 + 0.4
    w[n - 1] = 0.0
    return w.to(dev)


class _Autocast(torch.nn.Module):
    def __init__(self, d):
        super().__init__()
        self.d = d

    def forward(self, x, s):
        with torch.autocast('cuda', dtype=torch.float16):
            return self.d(x, s)


def training_legs(args, dev, lines, amp):
    from oracle import hyperseg_oracle as O
    from test_hip_parity import build_decoder
    from hyperseg_amd import training
    from hyperseg_amd.fps import ConfusionMatrix
    n = 12
    x, s = O.synth_decoder_inputs('Sc', batch=2, seed=3, size=(576, 576))
    x, s = [t.to(dev) for t in x], s.to(dev)
    target = torch.randint(0, n, (2, 576, 576), generator=torch.Generator().manual_seed(5)).to(dev)
    d0 = build_decoder('Sc', O).to(dev).train()
    steps, crits = {}, {}
    for leg in 'uws':
        d = copy.deepcopy(d0)
        crits[leg] = training.BootstrappedCrossEntropyLoss(k=4096, thresh=0.3, weight=None if leg == 'u' else table(n, 7, dev), ignore_index=255)
        crits[leg].score = ConfusionMatrix(n)
        opt = training.Adam(d.parameters(), lr=torch.tensor(2e-3, device=dev), betas=(0.5, 0.999))
        training.USE_HIP_CLASS_WEIGHTS = leg != 's'              # read while the step is captured
        try:
            steps[leg] = training.GraphedTrainStep(_Autocast(d) if amp else d, crits[leg], opt, (x, s), target, warmup=2,
                                                   scaler=torch.amp.GradScaler('cuda') if amp else None)
        finally:
            training.USE_HIP_CLASS_WEIGHTS = True
    variants = {f'({k})': v.step for k, v in steps.items()}
    for fn in variants.values():                    # the legs are warm before the agreement check; interleaved() warms nothing more
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    same = float(steps['w'].loss) == float(steps['s'].loss) or abs(float(steps['w'].loss) - float(steps['s'].loss)) < 1e-3 * abs(float(steps['s'].loss))
    same = same and int(crits['w'].score.mat.sum()) == int(crits['s'].score.mat.sum())     # (the two adjoints round differently: a few arg-maxes may)
    lines.append(f'config 5 (CamVid-S decoder, 576x576, bs 2), GraphedTrainStep, scored, {"fp16 autocast + GradScaler" if amp else "fp32"}; '
                 f'{args.rounds} interleaved rounds x {args.reps} steps, ms per step; the loss after the warm-up: ' +
                 ', '.join(f'({k}) loss {float(v.loss):.6f}' for k, v in steps.items()))
    lines.append(f'(w) and (s) agree on the loss (1e-3 relative) and on the pixels counted: {same}')
    med, spread = interleaved(lines, None, {k: (region_ms, fn, args.reps) for k, fn in variants.items()}, args.rounds, warmup=0)
    lines.append(verdict('(w) - (u)', '(u)', '(w)', med, spread) + ';  ' + verdict('(s) - (w)', '(w)', '(s)', med, spread))
    return same


def validation_legs(args, dev, lines):
    from hyperseg_amd import configs, training
    from hyperseg_amd.utils.inference import GraphedModel, prepare_for_inference
    from hyperseg_amd.utils.synthetic import fill_by_name
    from _workload import targets
    n, (h, w) = 19, (512, 1024)
    model = fill_by_name(configs.build('hyperseg-m').eval(), seed=0)
    prepare_for_inference(model, fold_bn=False, fused_depthwise=True)
    model.inference_hflip = False
    model = model.to(dev)
    x = torch.rand(1, 3, h, w, generator=torch.Generator().manual_seed(1)).to(dev)
    tgt = targets('rects', h, w, n, 2).to(dev)
    plain = training.BootstrappedCrossEntropyLoss(k=4096, thresh=0.3, ignore_index=255)
    weighted = training.BootstrappedCrossEntropyLoss(k=4096, thresh=0.3, weight=table(n, 8, dev), ignore_index=255)
    served_u = GraphedModel(model, masks=True, num_classes=n, criterion=plain)
    served_w = GraphedModel(model, masks=True, num_classes=n, criterion=weighted)
    served_s = GraphedModel(model, masks=True, num_classes=n, criterion=weighted)
    got = {}

    def vu():
        got['vu'] = served_u.validate(x, tgt)

    def vw():
        got['vw'] = served_w.validate(x, tgt)

    def vs():
        training.USE_HIP_CLASS_WEIGHTS = False
        try:
            got['vs'] = served_s.validate(x, tgt)
        finally:
            training.USE_HIP_CLASS_WEIGHTS = True

    variants = {'(vu)': vu, '(vw)': vw, '(vs)': vs}
    for fn in variants.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    served_w.reset_confusion(); served_s.reset_confusion()
    vw(); vs()
    torch.cuda.synchronize()
    lw, ls = float(got['vw'][0]), float(got['vs'][0])             # (the stock op rounds differently: the loss to 1e-5, the rest exactly)
    same = (abs(lw - ls) <= 1e-5 * abs(ls) and torch.equal(got['vw'][1].long(), got['vs'][1].long())
            and torch.equal(served_w.confusion, served_s.confusion))
    graphs = sum(1 for k in served_s._graphs if k[0] == 'validate')
    lines.append(f'HyperSeg-M {w}x{h} bs 1, prepared, GraphedModel.validate; {args.rounds} interleaved rounds x {args.reps} batches, ms per batch')
    lines.append(f'loss {lw:.7f} / {ls:.7f} (1e-5 relative), masks and matrix of (vw) and (vs) agree: {same}; validate graphs of the switched-off wrapper: {graphs}')
    med, spread = interleaved(lines, None, {k: (region_ms, fn, args.reps) for k, fn in variants.items()}, args.rounds, warmup=0)
    lines.append(verdict('(vw) - (vu)', '(vu)', '(vw)', med, spread) + ';  ' + verdict('(vs) - (vw)', '(vw)', '(vs)', med, spread) +
                 f' ({med["(vs)"] / med["(vw)"]:.2f}x)')
    return same and graphs == 0


def bench_legs(args, lines):
    trees = {'parent': os.path.abspath(args.parent), 'this': REPO}
    runs = {k: [] for k in trees}
    for r in range(3):
        for k, root in trees.items():
            p = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--gpus', '1', '--steps', '200', '--warmup', '20', '--no-cpu-baseline'],
                               cwd=root, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True, timeout=600)
            if p.returncode != 0:
                raise SystemExit(f'bench.py of the {k} tree ended with status {p.returncode}')
            runs[k].append(json.loads(p.stdout.strip().splitlines()[-1]))
            print(f'bench.py, {k} tree, run {r + 1}: value {runs[k][-1].get("value")}', flush=True)
    lines.append('bench.py --gpus 1 --steps 200 --warmup 20 --no-cpu-baseline, fresh processes, parent and this tree alternating, 3 runs each')
    med, spread = {}, {}
    for k, outs in runs.items():
        v = [float(o['value']) for o in outs]
        med[k], spread[k] = statistics.median(v), max(v) - min(v)
        lines.append(f'value ({k}) median {med[k]:.4f}  spread {spread[k]:.4f}   runs ' + ' '.join(f'{x:.4f}' for x in v))
    d, s = med['this'] - med['parent'], spread['this'] + spread['parent']
    lines.append(f'value: this - parent = {d:+.4f}, summed spreads {s:.4f}: {"within" if abs(d) <= s else "beyond"}')


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--reps', type=int, default=100)
    ap.add_argument('--parent', default=None, help='a built checkout of the parent commit: bench.py is then run in both trees')
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'weighted_loss_time.txt'))
    args = ap.parse_args()
    require_gpu('weighted_loss_time.py')
    dev = torch.device('cuda:0')
    lines = Lines()
    ok = training_legs(args, dev, lines, amp=False)
    ok = training_legs(args, dev, lines, amp=True) and ok
    with torch.no_grad():               # GraphedModel replays only where nothing can ask for a gradient
        ok = validation_legs(args, dev, lines) and ok
    write_report(lines, args.out)
    if args.parent:
        torch.cuda.empty_cache()
        bench_lines = Lines()
        bench_legs(args, bench_lines)
        with open(args.out, 'a') as f:
            f.write('\n'.join(bench_lines) + '\n')
    assert ok, 'the legs disagree on what they compute'


if __name__ == '__main__':
    main()
