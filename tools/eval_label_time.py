"""What scoring a frame at the LABEL's resolution costs: HyperSeg-M at 1024 x 512 and HyperSeg-S at 1536 x 768, batch 1, after
prepare_for_inference, against int64 labels at 2048 x 1024 -- the protocol of the reference's Cityscapes test configs (the image is
resized, the label is not; test.py:167-168 resizes the logits to the label before the arg-max).

    timeout -k 10 900 python tools/eval_label_time.py [--rounds 7] [--reps 200] [--models m s] [--out profiles/eval_label_time.txt]

Per model, one process, four legs timed INTERLEAVED (round r times a, b, c, d in turn, ``--rounds`` rounds), each sample a region of
``--reps`` frames between two device events:
  (a) GraphedModel(masks=True) replay -- masks at the frame's size only, nothing scored (the floor);
  (b) what the route before hs_upsample2_confusion_fwd did for this target, written out here so that it does not depend on the code
      under test: a GraphedModel logits replay + HF.upsample_bilinear to the label + argmax(1).to(uint8) + HF.confusion_update;
  (c) the same chain behind an EAGER forward -- what GraphedModel.evaluate did then (it refused such a target and dropped to
      model.evaluate's fallback);
  (d) GraphedModel.evaluate: one replay whose last launch composes both resizes, takes the arg-max and counts.
(b), (c) and (d) must produce equal matrices (asserted before anything is timed).  Required: (d) below (b) by more than the sum of the
two legs' spreads (max - min over the rounds); the verdict is printed and the exit status is non-zero where it does not hold.
Then the new kernel alone, back to back, against the three launches it replaces (upsample_bilinear to the frame, upsample_bilinear to
the label, arg-max + count), on smooth + noise logits at each model's last-level size: both forms of the kernel."""
import argparse
import os
import statistics

import torch

from _measure import REPO, Lines, exceeds, interleaved, region_ms, require_gpu, write_report

LABEL = (1024, 2048)
MODELS = {'m': ('hyperseg-m', (512, 1024)), 's': ('hyperseg-s', (768, 1536))}


def one_model(tag, rounds, reps, lines):
    from hyperseg_amd import configs, functional as HF
    from hyperseg_amd.utils.inference import GraphedModel, prepare_for_inference
    from hyperseg_amd.utils.synthetic import fill_by_name
    from _workload import label_targets
    dev = torch.device('cuda:0')
    name, (h, w) = MODELS[tag]
    n = configs.MODELS[name]['num_classes']
    model = fill_by_name(configs.build(name).eval(), seed=0)
    prepare_for_inference(model, fold_bn=False, fused_depthwise=True)
    model.inference_hflip = False       # inert for tensor inputs, but segment() takes the logits + argmax route while it is set
    model = model.to(dev)
    x = torch.rand(1, 3, h, w, generator=torch.Generator().manual_seed(1)).to(dev)
    tgt = label_targets(LABEL[0], LABEL[1], n, 2).to(dev)
    served = GraphedModel(model, masks=True, num_classes=n)
    logits_served = GraphedModel(model)
    mats = {k: torch.zeros(n, n, dtype=torch.int64, device=dev) for k in 'bc'}

    def chain(logits, out):
        up = HF.upsample_bilinear(logits.contiguous(), LABEL)
        HF.confusion_update(up.argmax(1).to(torch.uint8), tgt, n, out=out)

    def a():
        served(x)

    def b():
        chain(logits_served(x), mats['b'])

    def c():
        chain(model(x), mats['c'])

    def d():
        served.evaluate(x, tgt)

    legs = {'(a)': a, '(b)': b, '(c)': c, '(d)': d}
    for fn in legs.values():                        # every shape and graph warmed before anything is timed
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    for m in mats.values():
        m.zero_()
    served.reset_confusion()
    b(); c(); d()
    torch.cuda.synchronize()
    same = torch.equal(mats['b'], mats['c']) and torch.equal(mats['b'], served.confusion)
    assert same, f'{name}: the legs disagree on the matrix'
    assert int(mats['b'].sum()) == int((tgt != 255).sum())
    if lines:
        lines.append('')
    lines.append(f'{name} {w}x{h} bs 1, prepared; int64 labels {LABEL[1]}x{LABEL[0]}; {rounds} interleaved rounds x {reps} frames, ms per frame')
    lines.append(f'matrices of (b), (c), (d) equal: {same}')
    med, spread = interleaved(lines, None, {k: (region_ms, fn, reps) for k, fn in legs.items()}, rounds, warmup=0)
    ok = exceeds('(b)', '(d)', med, spread)
    lines.append(f'(b) - (d) = {med["(b)"] - med["(d)"]:+.4f} ms vs spread(b) + spread(d) = {spread["(b)"] + spread["(d)"]:.4f}: requirement '
                 f'{"met" if ok else "NOT met"};  (c) - (d) = {med["(c)"] - med["(d)"]:+.4f} ms;  (d) - (a) = {med["(d)"] - med["(a)"]:+.4f} ms')
    # the kernel alone against the three launches it replaces, at this model's last-level size
    hi, wi = h // 2, w // 2
    g = torch.Generator().manual_seed(3)
    logits = (torch.nn.functional.interpolate(torch.randn(1, n, hi // 4, wi // 4, generator=g), size=(hi, wi), mode='bilinear')
              + 0.1 * torch.randn(1, n, hi, wi, generator=g)).contiguous().to(dev)
    out = torch.zeros(n, n, dtype=torch.int64, device=dev)

    def three():
        up = HF.upsample_bilinear(HF.upsample_bilinear(logits, (h, w)), LABEL)
        HF.upsample_confusion(up, LABEL, tgt, n, out=out, masks=True)

    def one():
        HF.upsample2_confusion(logits, (h, w), tgt, n, out=out, masks=True)

    form = 'both stages exact 2x' if (2 * h, 2 * w) == LABEL else 'general'
    for label, fn in (('three launches (2 x upsample_bilinear + arg-max/count)', three), (f'upsample2_confusion ({form} form)', one)):
        for _ in range(5):
            fn()
        s = [1e3 * region_ms(fn, 50) for _ in range(3)]
        lines.append(f'kernel alone, {hi}x{wi} -> {h}x{w} -> {LABEL[0]}x{LABEL[1]}: {label:56s} {statistics.median(s):9.2f} us  '
                     f'(min {min(s):.2f} max {max(s):.2f}; eager launches back to back)')
    return ok


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--models', nargs='+', choices=sorted(MODELS), default=['m', 's'])
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'eval_label_time.txt'))
    args = ap.parse_args()
    require_gpu('eval_label_time.py')
    lines, ok = Lines(), True
    for tag in args.models:
        ok = one_model(tag, args.rounds, args.reps, lines) and ok
    write_report(lines, args.out)
    if not ok:
        raise SystemExit('(d) is not below (b) by more than the sum of the two spreads on every model')


if __name__ == '__main__':
    with torch.no_grad():               # GraphedModel.forward replays only where nothing can ask for a gradient
        main()
