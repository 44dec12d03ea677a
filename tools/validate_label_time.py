"""What validating a batch at the LABEL's resolution costs: HyperSeg-M at 1024 x 512 and HyperSeg-S at 1536 x 768, batch 1, after
prepare_for_inference, against int64 labels at 2048 x 1024 -- the protocol of the reference's Cityscapes training configs (the image is
resized, the label is not; train.py:119-120 resizes the logits to the label before the criterion and the arg-max) -- with an unweighted
BootstrappedCrossEntropyLoss and with a 19-entry random class-weight table.

    timeout -k 10 1100 python tools/validate_label_time.py [--rounds 7] [--reps 100] [--models m s] [--out profiles/validate_label_time.txt]

Per model and criterion, one process, the legs timed INTERLEAVED (round r times each leg in turn, ``--rounds`` rounds), each sample a region
of ``--reps`` batches between two device events; medians with spreads (max - min over the rounds):
  (a) the composed route, written out here so that it does not depend on the code under test: an eager forward, HF.upsample_bilinear to
      the label, the criterion, argmax(1).to(uint8) and HF.confusion_update;
  (b) GraphedModel.evaluate with the same label: masks and counts at the label's size, no loss -- the yardstick for what the loss adds;
  (c) GraphedModel.validate: one replay whose last launch composes both resizes and makes losses, masks and counts;
  (d) (c) with the general kernel forced where the 2x o 2x form is chosen (HyperSeg-M; the library's HS_VALIDATE_2X2X=0 knob, set while
      that graph is captured): the keep-or-drop measurement of the 2x o 2x form.
(a), (c) and (d) must produce equal losses and matrices, (b) the same matrix (asserted before anything is timed).  Required: (c) below
(a) by more than the sum of the two legs' spreads; the verdict is printed and the exit status is non-zero where it does not hold.  The
2x o 2x form is worth keeping where (d) - (c) exceeds the sum of their spreads.  Then the new kernel alone, back to back, both forms."""
import argparse
import os
import statistics

import torch

from _measure import REPO, Lines, exceeds, interleaved, region_ms, require_gpu, write_report

LABEL = (1024, 2048)
MODELS = {'m': ('hyperseg-m', (512, 1024)), 's': ('hyperseg-s', (768, 1536))}
KNOB = 'HS_VALIDATE_2X2X'


class general_form:
    """The library's dev knob set for the calls (and captures) made inside."""

    def __enter__(self):
        os.environ[KNOB] = '0'

    def __exit__(self, *exc):
        del os.environ[KNOB]


def one_config(tag, weighted, model, n, rounds, reps, lines):
    from hyperseg_amd import functional as HF
    from hyperseg_amd.training import BootstrappedCrossEntropyLoss
    from hyperseg_amd.utils.inference import GraphedModel
    from _workload import label_targets
    dev = torch.device('cuda:0')
    name, (h, w) = MODELS[tag]
    table = (0.5 + torch.rand(n, generator=torch.Generator().manual_seed(5))).to(dev) if weighted else None
    crit = BootstrappedCrossEntropyLoss(ignore_index=255, weight=table)
    x = torch.rand(1, 3, h, w, generator=torch.Generator().manual_seed(1)).to(dev)
    tgt = label_targets(LABEL[0], LABEL[1], n, 2).to(dev)
    has_2x2x = (2 * h, 2 * w) == LABEL
    scorer = GraphedModel(model, masks=True, num_classes=n)
    served = GraphedModel(model, masks=True, num_classes=n, criterion=crit)
    forced = GraphedModel(model, masks=True, num_classes=n, criterion=crit) if has_2x2x else None
    mat_a = torch.zeros(n, n, dtype=torch.int64, device=dev)
    got = {}

    def a():
        up = HF.upsample_bilinear(model(x).contiguous(), LABEL)
        got['a'] = crit(up, tgt)
        HF.confusion_update(up.argmax(1).to(torch.uint8), tgt, n, out=mat_a)

    def b():
        scorer.evaluate(x, tgt)

    def c():
        got['c'] = served.validate(x, tgt)[0]

    def d():
        got['d'] = forced.validate(x, tgt)[0]

    legs = {'(a)': a, '(b)': b, '(c)': c}
    if has_2x2x:
        with general_form():                        # the capture fixes the form this graph replays
            d()
        legs['(d)'] = d
    for fn in legs.values():                        # every shape and graph warmed before anything is timed
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    mat_a.zero_()
    for g in (scorer, served, forced):
        if g is not None:
            g.reset_confusion()
    for fn in legs.values():
        fn()
    torch.cuda.synchronize()
    same = torch.equal(mat_a, served.confusion) and torch.equal(mat_a, scorer.confusion) and float(got['a']) == float(got['c'])
    if has_2x2x:
        same = same and torch.equal(mat_a, forced.confusion) and float(got['d']) == float(got['c'])
    assert same, f'{name}: the legs disagree'
    assert int(mat_a.sum()) == int((tgt != 255).sum())
    if lines:
        lines.append('')
    lines.append(f'{name} {w}x{h} bs 1, prepared; int64 labels {LABEL[1]}x{LABEL[0]}; criterion {"weighted (19-entry table)" if weighted else "unweighted"}; '
                 f'{rounds} interleaved rounds x {reps} batches, ms per batch')
    lines.append(f'losses and matrices of the legs equal: {same} (loss {float(got["c"]):.6f})')
    med, spread = interleaved(lines, None, {k: (region_ms, fn, reps) for k, fn in legs.items()}, rounds, warmup=0)
    ok = exceeds('(a)', '(c)', med, spread)
    lines.append(f'(a) - (c) = {med["(a)"] - med["(c)"]:+.4f} ms vs spread(a) + spread(c) = {spread["(a)"] + spread["(c)"]:.4f}: requirement '
                 f'{"met" if ok else "NOT met"};  the price of the loss (c) - (b) = {med["(c)"] - med["(b)"]:+.4f} ms')
    if has_2x2x:
        keep = exceeds('(d)', '(c)', med, spread)
        lines.append(f'(d) - (c) = {med["(d)"] - med["(c)"]:+.4f} ms vs spread(c) + spread(d) = {spread["(c)"] + spread["(d)"]:.4f}: the 2x o 2x form '
                     f'{"beats the general form by more than the spreads: keep" if keep else "does not beat the general form by more than the spreads: drop"}')
    # the kernel alone, at this model's last-level size
    hi, wi = h // 2, w // 2
    g = torch.Generator().manual_seed(3)
    logits = (torch.nn.functional.interpolate(torch.randn(1, n, hi // 4, wi // 4, generator=g), size=(hi, wi), mode='bilinear')
              + 0.1 * torch.randn(1, n, hi, wi, generator=g)).contiguous().to(dev)
    out = torch.zeros(n, n, dtype=torch.int64, device=dev)

    def one():
        HF.upsample2_ce_confusion(logits, (h, w), tgt, 255, n, out=out, weight=table)

    def timed(label):
        for _ in range(5):
            one()
        s = [1e3 * region_ms(one, 50) for _ in range(3)]
        lines.append(f'kernel alone, {hi}x{wi} -> {h}x{w} -> {LABEL[0]}x{LABEL[1]}: {label:44s} {statistics.median(s):9.2f} us  '
                     f'(min {min(s):.2f} max {max(s):.2f}; eager launches back to back)')
    if has_2x2x:
        timed('upsample2_ce_confusion (2x o 2x form)')
        with general_form():
            timed('upsample2_ce_confusion (general form, forced)')
    else:
        timed('upsample2_ce_confusion (general form)')
    return ok


def one_model(tag, rounds, reps, lines):
    from hyperseg_amd import configs
    from hyperseg_amd.utils.inference import prepare_for_inference
    from hyperseg_amd.utils.synthetic import fill_by_name
    name = MODELS[tag][0]
    n = configs.MODELS[name]['num_classes']
    model = fill_by_name(configs.build(name).eval(), seed=0)
    prepare_for_inference(model, fold_bn=False, fused_depthwise=True)
    model.inference_hflip = False
    model = model.to(torch.device('cuda:0'))
    ok = True
    for weighted in (False, True):
        ok = one_config(tag, weighted, model, n, rounds, reps, lines) and ok
    return ok


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--reps', type=int, default=100)
    ap.add_argument('--models', nargs='+', choices=sorted(MODELS), default=['m', 's'])
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'validate_label_time.txt'))
    args = ap.parse_args()
    require_gpu('validate_label_time.py')
    lines, ok = Lines(), True
    for tag in args.models:
        ok = one_model(tag, args.rounds, args.reps, lines) and ok
    write_report(lines, args.out)
    if not ok:
        raise SystemExit('(c) is not below (a) by more than the sum of the two spreads on every configuration')


if __name__ == '__main__':
    with torch.no_grad():               # GraphedModel replays only where nothing can ask for a gradient
        main()
