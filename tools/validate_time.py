"""What a validation batch costs, and what the running score costs a training step.

    timeout -k 10 900 python tools/validate_time.py [--rounds 7] [--reps 100] [--out profiles/validate_time.txt]

One process; the legs of each group timed INTERLEAVED (round r times every leg in turn, ``--rounds`` rounds), each sample a region of
``--reps`` batches between two device events.  No threshold is asserted: the numbers are the record.
HyperSeg-M, 1024 x 512, batch 1, after prepare_for_inference (train.py:118-126 under eval() / no_grad):
  (a) GraphedModel.evaluate -- masks + confusion matrix from the forward's last launch, no loss: the floor;
  (b) composed validation, eager: pred = model(x), criterion(pred, target), pred.argmax(1), ConfusionMatrix.update;
  (c) model.validate, eager: the last launch makes losses, masks and counts;
  (d) GraphedModel.validate: (c) as one replay.
Config 5 (CamVid-S decoder, 576 x 576, batch 2) through GraphedTrainStep:
  (e) no score;
  (f) criterion.score set: the loss launch counts;
  (g) no score, plus pred.argmax(1) and ConfusionMatrix.update after each replay.
Reported: medians, spreads (max - min over the rounds), (d) against (b), and (f) - (e) against (g) - (e).  (b), (c) and (d) must
agree on loss, masks and matrix; (f) and (g) on the matrix."""
import argparse
import os
import sys

import torch

from _measure import REPO, Lines, interleaved, region_ms, require_gpu, write_report

sys.path.insert(0, os.path.join(REPO, 'tests'))


def validation_legs(args, dev, lines):
    from hyperseg_amd import configs
    from hyperseg_amd.fps import ConfusionMatrix
    from hyperseg_amd.training import BootstrappedCrossEntropyLoss
    from hyperseg_amd.utils.inference import GraphedModel, prepare_for_inference
    from hyperseg_amd.utils.synthetic import fill_by_name
    from _workload import targets
    n, (h, w) = 19, (512, 1024)
    model = fill_by_name(configs.build('hyperseg-m').eval(), seed=0)
    prepare_for_inference(model, fold_bn=False, fused_depthwise=True)
    model.inference_hflip = False
    model = model.to(dev)
    crit = BootstrappedCrossEntropyLoss(k=4096, thresh=0.3, ignore_index=255)
    x = torch.rand(1, 3, h, w, generator=torch.Generator().manual_seed(1)).to(dev)
    tgt = targets('rects', h, w, n, 2).to(dev)
    floor = GraphedModel(model, masks=True, num_classes=n)
    served = GraphedModel(model, masks=True, num_classes=n, criterion=crit)
    cm_b, cm_c = ConfusionMatrix(n), ConfusionMatrix(n)
    got = {}

    def a():
        floor.evaluate(x, tgt)

    def b():
        pred = model(x)
        got['b'] = (crit(pred, tgt), pred.argmax(1))
        cm_b.update(tgt.flatten(), got['b'][1].flatten())

    def c():
        got['c'] = model.validate(x, tgt, crit, cm_c)

    def d():
        got['d'] = served.validate(x, tgt)

    variants = {'(a)': a, '(b)': b, '(c)': c, '(d)': d}
    for fn in variants.values():                    # the legs are warm before the equality check; interleaved() warms nothing more
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    cm_b.reset(); cm_c.reset(); served.reset_confusion()
    b(); c(); d()
    torch.cuda.synchronize()
    same = (torch.equal(cm_b.mat, cm_c.mat) and torch.equal(cm_b.mat, served.confusion)
            and all(torch.equal(got[k][0], got['b'][0]) and torch.equal(got[k][1].long(), got['b'][1]) for k in 'cd'))
    lines.append(f'HyperSeg-M {w}x{h} bs 1, prepared; {args.rounds} interleaved rounds x {args.reps} batches, ms per batch')
    lines.append(f'loss, masks and matrix of (b), (c), (d) equal: {same}')
    med, spread = interleaved(lines, None, {k: (region_ms, fn, args.reps) for k, fn in variants.items()}, args.rounds, warmup=0)
    lines.append(f'(d) against (b): {med["(b)"] - med["(d)"]:+.4f} ms saved ({med["(b)"] / med["(d)"]:.2f}x), summed spreads {spread["(b)"] + spread["(d)"]:.4f};  '
                 f'(c) against (b): {med["(b)"] - med["(c)"]:+.4f} ms, summed spreads {spread["(b)"] + spread["(c)"]:.4f};  '
                 f'(d) - (a) = {med["(d)"] - med["(a)"]:+.4f} ms, summed spreads {spread["(d)"] + spread["(a)"]:.4f}')
    return same


def training_legs(args, dev, lines):
    import copy
    from oracle import hyperseg_oracle as O
    from test_hip_parity import build_decoder
    from hyperseg_amd.fps import ConfusionMatrix
    from hyperseg_amd.training import Adam, BootstrappedCrossEntropyLoss, GraphedTrainStep
    n = 12
    x, s = O.synth_decoder_inputs('Sc', batch=2, seed=3, size=(576, 576))
    x, s = [t.to(dev) for t in x], s.to(dev)
    target = torch.randint(0, n, (2, 576, 576), generator=torch.Generator().manual_seed(5)).to(dev)
    d0 = build_decoder('Sc', O).to(dev).train()
    steps, crits = {}, {}
    for leg in 'efg':
        d = copy.deepcopy(d0)
        crits[leg] = BootstrappedCrossEntropyLoss(k=4096, thresh=0.3, ignore_index=255)
        if leg == 'f':
            crits[leg].score = ConfusionMatrix(n)
        opt = Adam(d.parameters(), lr=torch.tensor(2e-3, device=dev), betas=(0.5, 0.999))
        steps[leg] = GraphedTrainStep(d, crits[leg], opt, (x, s), target, warmup=2)
    after = ConfusionMatrix(n)

    def g():
        _, pred = steps['g'].step()
        after.update(target.flatten(), pred.argmax(1).flatten())

    variants = {'(e)': steps['e'].step, '(f)': steps['f'].step, '(g)': g}
    for fn in variants.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    crits['f'].score.reset(); after.reset()
    steps['f'].step(); g()
    torch.cuda.synchronize()
    same = torch.equal(crits['f'].score.mat, after.mat)        # the three twins take the same steps: the same predictions
    lines.append(f'config 5 (CamVid-S decoder, 576x576, bs 2), GraphedTrainStep; {args.rounds} interleaved rounds x {args.reps} steps, ms per step')
    lines.append(f'matrix of (f) and (g) equal: {same}')
    med, spread = interleaved(lines, None, {k: (region_ms, fn, args.reps) for k, fn in variants.items()}, args.rounds, warmup=0)
    lines.append(f'(f) - (e) = {med["(f)"] - med["(e)"]:+.4f} ms, summed spreads {spread["(f)"] + spread["(e)"]:.4f};  '
                 f'(g) - (e) = {med["(g)"] - med["(e)"]:+.4f} ms, summed spreads {spread["(g)"] + spread["(e)"]:.4f};  '
                 f'(g) - (f) = {med["(g)"] - med["(f)"]:+.4f} ms, summed spreads {spread["(g)"] + spread["(f)"]:.4f}')
    return same


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--reps', type=int, default=100)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'validate_time.txt'))
    args = ap.parse_args()
    require_gpu('validate_time.py')
    dev = torch.device('cuda:0')
    lines = Lines()
    with torch.no_grad():               # GraphedModel replays only where nothing can ask for a gradient
        same_v = validation_legs(args, dev, lines)
    same_t = training_legs(args, dev, lines)
    write_report(lines, args.out)
    assert same_v and same_t, 'the legs disagree on what they compute'


if __name__ == '__main__':
    main()
