"""What scoring a frame costs on top of producing its masks: HyperSeg-M, 1024 x 512, batch 1, after prepare_for_inference.

    timeout -k 10 600 python tools/eval_epilogue_time.py [--rounds 7] [--reps 200] [--out profiles/eval_epilogue_time.txt]

One process, four variants timed INTERLEAVED (round r times a, b, c, d in turn, ``--rounds`` rounds), each sample a region of
``--reps`` frames between two device events (the stock route synchronises inside its region by itself):
  (a) GraphedModel(masks=True) replay -- masks only (inference_hflip off, so that segment() takes its fused arg-max route);
  (b) (a) + the stock torch update on the masks (ConfusionMatrix.update_stock: target[valid] ... bincount) -- what scoring a
      frame took before the evaluation kernels existed;
  (c) (a) + one hs_confusion_fwd launch on the masks (functional.confusion_update);
  (d) GraphedModel.evaluate -- the confusion matrix counted by the forward's last launch (hs_upsample_confusion_fwd).
Required (asserted): (d) < (b) and (c) < (b) by more than the spread (max - min over the rounds) of the samples involved.
Reported: (d) - (a), (c) - (a), and the two kernels alone at full size on the three target patterns of the tests (uniform
random, 15 % ignored, piecewise constant).  All four variants must produce the same matrix."""
import argparse
import os
import statistics

import torch

from _measure import REPO, Lines, interleaved, region_ms, require_gpu, write_report


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'eval_epilogue_time.txt'))
    args = ap.parse_args()
    require_gpu('eval_epilogue_time.py')
    from hyperseg_amd import configs, functional as HF
    from hyperseg_amd.fps import ConfusionMatrix
    from hyperseg_amd.utils.inference import GraphedModel, prepare_for_inference
    from hyperseg_amd.utils.synthetic import fill_by_name
    from _workload import targets
    dev = torch.device('cuda:0')
    n, (h, w) = 19, (512, 1024)
    model = fill_by_name(configs.build('hyperseg-m').eval(), seed=0)
    prepare_for_inference(model, fold_bn=False, fused_depthwise=True)
    model.inference_hflip = False       # inert for tensor inputs, but segment() takes the logits + argmax route while it is set:
    model = model.to(dev)               # (a) is meant to be the fused arg-max route
    x = torch.rand(1, 3, h, w, generator=torch.Generator().manual_seed(1)).to(dev)
    tgt = targets('rects', h, w, n, 2).to(dev)
    served = GraphedModel(model, masks=True, num_classes=n)
    stock, kern = ConfusionMatrix(n), ConfusionMatrix(n)
    kern.matrix(dev)

    def a():
        return served(x)

    def b():
        m = served(x)
        stock.update_stock(tgt.flatten(), m.flatten())

    def c():
        HF.confusion_update(served(x), tgt, n, out=kern.mat)

    def d():
        served.evaluate(x, tgt)

    variants = {'(a)': a, '(b)': b, '(c)': c, '(d)': d}
    for fn in variants.values():                    # every shape and graph warmed before anything is timed
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    stock.reset(); kern.reset(); served.reset_confusion()
    b(); c(); d()
    torch.cuda.synchronize()
    same = torch.equal(stock.mat, kern.mat) and torch.equal(stock.mat, served.confusion)
    lines = Lines()
    lines.append(f'HyperSeg-M {w}x{h} bs 1, prepared, HIP-graph replay; {args.rounds} interleaved rounds x {args.reps} frames, ms per frame')
    lines.append(f'matrices of (b), (c), (d) equal: {same}')
    med, spread = interleaved(lines, None, {k: (region_ms, fn, args.reps) for k, fn in variants.items()}, args.rounds, warmup=0)
    lines.append(f'(d) - (a) = {med["(d)"] - med["(a)"]:+.4f} ms   (c) - (a) = {med["(c)"] - med["(a)"]:+.4f} ms   (b) - (a) = {med["(b)"] - med["(a)"]:+.4f} ms')
    lines.append(f'(b) - (d) = {med["(b)"] - med["(d)"]:.4f} ms vs spread {max(spread["(b)"], spread["(d)"]):.4f};  '
                 f'(b) - (c) = {med["(b)"] - med["(c)"]:.4f} ms vs spread {max(spread["(b)"], spread["(c)"]):.4f};  '
                 f'(c) - (d) = {med["(c)"] - med["(d)"]:+.4f} ms vs spread {max(spread["(c)"], spread["(d)"]):.4f}')
    # the two kernels alone, full size, per target pattern (smooth + noise logits stand in for the decoder's last level)
    g = torch.Generator().manual_seed(3)
    logits = (torch.nn.functional.interpolate(torch.randn(1, n, h // 8, w // 8, generator=g), size=(h // 2, w // 2), mode='bilinear')
              + 0.1 * torch.randn(1, n, h // 2, w // 2, generator=g)).contiguous().to(dev)
    masks = HF.upsample_argmax(logits, (h, w))
    out = torch.zeros(n, n, dtype=torch.int64, device=dev)
    kernels = {'upsample_argmax (masks only)': lambda t: HF.upsample_argmax(logits, (h, w)),
               'upsample_confusion (fused, masks written)': lambda t: HF.upsample_confusion(logits, (h, w), t, n, out=out, masks=True),
               'confusion_update (from masks)': lambda t: HF.confusion_update(masks, t, n, out=out)}
    for pattern in ('uniform', 'ignored', 'rects'):
        for dt in (torch.int64, torch.uint8):
            t = targets(pattern, h, w, n, 4).to(dt).to(dev)
            for name, fn in kernels.items():
                for _ in range(10):
                    fn(t)
                s = [1e3 * region_ms(lambda: fn(t), 100) for _ in range(3)]
                lines.append(f'kernel alone, {pattern:8s} {str(dt)[6:]:6s} {name:42s} {statistics.median(s):8.2f} us  '
                             f'(min {min(s):.2f} max {max(s):.2f}; eager launches back to back)')
    write_report(lines, args.out)
    assert same, 'the variants disagree on the matrix'
    assert med['(b)'] - med['(d)'] > max(spread['(b)'], spread['(d)']), '(d) is not below (b) by more than the spread'
    assert med['(b)'] - med['(c)'] > max(spread['(b)'], spread['(c)']), '(c) is not below (b) by more than the spread'


if __name__ == '__main__':
    with torch.no_grad():               # GraphedModel.forward replays only where nothing can ask for a gradient
        main()
