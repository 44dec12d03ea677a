"""What a frame's confidence map costs on top of producing its masks: HyperSeg-M, 1024 x 512, batch 1, after prepare_for_inference.

    timeout -k 10 600 python tools/confidence_time.py [--rounds 5] [--reps 200] [--out profiles/confidence_time.txt]

One process, the routes timed INTERLEAVED (round r times each in turn, ``--rounds`` rounds), each sample a region of ``--reps`` frames
between two device events.  The setup is tools/overlay_time.py's (float image resident on the device, inference_hflip off):
  (1)   GraphedModel(masks=True) replay -- masks only;
  (2u)  GraphedModel.confidence, uint8 -- masks and confidence from the forward's last launch (hs_upsample_confidence_fwd);
  (2f)  the same, float32;
  (3)   a logits replay (GraphedModel(masks=False)) + one hs_confidence_fwd launch on the logits (functional.confidence, float32);
  (4)   a logits replay + stock ``torch.softmax(logits, 1).max(1)`` -- what a user writes without this feature (float32 confidence, int64 masks).
Then a label-size output, ``size=(1024, 2048)``: (2uL) GraphedModel.confidence(x, size) and (4L) the logits replay + upsample_bilinear to that
size + stock softmax / max.
Stated, not asserted: whether (2f) is below (4) by more than the sum of the two spreads (max - min over the rounds).  Asserted: (2f), (3)
give the same confidence bits and the masks of (1); (4) agrees with them to 1e-6."""
import argparse
import os

import torch

from _measure import REPO, Lines, exceeds, interleaved, region_ms, require_gpu, write_report


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'confidence_time.txt'))
    args = ap.parse_args()
    require_gpu('confidence_time.py')
    from hyperseg_amd import Confidence, configs, functional as HF
    from hyperseg_amd.utils.inference import GraphedModel, prepare_for_inference
    from hyperseg_amd.utils.synthetic import fill_by_name
    dev = torch.device('cuda:0')
    (h, w), big = (512, 1024), (1024, 2048)
    model = fill_by_name(configs.build('hyperseg-m').eval(), seed=0)
    prepare_for_inference(model, fold_bn=False, fused_depthwise=True)
    model.inference_hflip = False       # inert for tensor inputs, but segment() / confidence() take their logits routes while it is set
    model = model.to(dev)
    x = torch.rand(1, 3, h, w, generator=torch.Generator().manual_seed(1)).to(dev)
    masks_g, logits_g = GraphedModel(model, masks=True), GraphedModel(model, masks=False)
    conf_u, conf_f = GraphedModel(model, masks=True), GraphedModel(model, masks=True)      # one style per wrapper: the style is read per call
    u8, f32 = Confidence(torch.uint8), Confidence(torch.float32)
    keep = {}

    def with_style(style, fn):
        model.confidence_style = style
        return fn()

    def r1():
        keep['1'] = masks_g(x)

    def r2u():
        keep['2u'] = with_style(u8, lambda: conf_u.confidence(x))

    def r2f():
        keep['2f'] = with_style(f32, lambda: conf_f.confidence(x))

    def r3():
        keep['3'] = HF.confidence(logits_g(x), torch.float32)

    def r4():
        keep['4'] = torch.softmax(logits_g(x), 1).max(1)

    def r2ul():
        keep['2uL'] = with_style(u8, lambda: conf_u.confidence(x, size=big))

    def r4l():
        keep['4L'] = torch.softmax(HF.upsample_bilinear(logits_g(x), big), 1).max(1)

    variants = {'(1)': r1, '(2u)': r2u, '(2f)': r2f, '(3)': r3, '(4)': r4, '(2uL)': r2ul, '(4L)': r4l}
    for fn in variants.values():                    # every shape and graph warmed before anything is timed
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    same_masks = torch.equal(keep['1'], keep['2f'][0]) and torch.equal(keep['1'], keep['2u'][0]) and torch.equal(keep['1'], keep['3'][0])
    same_bits = torch.equal(keep['2f'][1], keep['3'][1]) and torch.equal(keep['2u'][1], (keep['2f'][1] * 255.0 + 0.5).to(torch.uint8))
    stock_gap = float((keep['4'].values - keep['2f'][1]).abs().max())
    lines = Lines()
    lines.append(f'HyperSeg-M {w}x{h} bs 1, prepared, HIP-graph replay, resident input; {args.rounds} interleaved rounds x {args.reps} frames, ms per frame')
    lines.append(f'masks of (1), (2u), (2f), (3) equal: {same_masks};  confidence bits of (2f) and (3) equal, (2u) their quantisation: {same_bits};  '
                 f'max |(4) - (2f)| = {stock_gap:.2e}')
    med, spread = interleaved(lines, None, {k: (region_ms, fn, args.reps) for k, fn in variants.items()}, args.rounds, warmup=0)
    lines.append('   '.join(f'{k} - (1) = {med[k] - med["(1)"]:+.4f} ms' for k in ('(2u)', '(2f)', '(3)', '(4)')))
    for a, b in (('(2f)', '(4)'), ('(2u)', '(4)'), ('(2f)', '(3)'), ('(2uL)', '(4L)')):
        lines.append(f'{b} - {a} = {med[b] - med[a]:+.4f} ms vs the sum of the two spreads {spread[a] + spread[b]:.4f}: {a} is '
                     + ('below' if exceeds(b, a, med, spread) else 'NOT below') + f' {b} by more than that')
    write_report(lines, args.out)
    assert same_masks and same_bits, 'the routes disagree'
    assert stock_gap < 1e-6, 'stock softmax disagrees with the kernels'


if __name__ == '__main__':
    with torch.no_grad():               # GraphedModel.forward replays only where nothing can ask for a gradient
        main()
