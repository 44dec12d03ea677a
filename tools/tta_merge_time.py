"""What merging the passes of flip / pyramid inference in one launch saves: HyperSeg-M, 1024 x 512, batch 1, after prepare_for_inference, eager.

    timeout -k 10 600 python tools/tta_merge_time.py [--rounds 5] [--reps 20] [--out profiles/tta_merge_time.txt]

One process, the routes timed INTERLEAVED (round r times each in turn, ``--rounds`` rounds); the merged route and the composed one
(``HF.TTA_MERGE`` off: the same deferred passes, then ``HF.tta_merge_composed``) are the same model in the same process.  Legs:
  whole calls, host clock around ``--reps`` calls between two synchronisations (the eager passes are host-bound, ~110 launches each):
    segment([x])           with the flip (2 passes), merged / composed;
    segment([x, x/2, x/4]) with the flip (6 passes; smaller entries F.avg_pool2d of the frame), merged / composed;
    evaluate([x], label)   a label at the frame's size, merged (scored in the merge launch) / composed (forward, arg-max, confusion_update);
  the epilogue alone, device events, decoder outputs resident: ``HF.tta_merge`` (one launch) against ``HF.tta_merge_composed`` (the sum of the
    composed epilogue's launches), masks out, for the 2-pass and the 6-pass table.
Asserted: both routes give the same masks and the same matrix.  Stated, not asserted: which differences exceed the sum of the two spreads.
The bytes each epilogue moves are worked out from the shapes timed."""
import argparse
import os

import torch

from _measure import REPO, Lines, interleaved, region_ms, require_gpu, verdict, wall_ms, write_report


def composed_bytes(passes, c, b=1):
    """HBM bytes the composed epilogue's launches read + write for masks (fp32 logits; the uint8 masks and int64 indices counted)."""
    total, out = 0, passes[0][1]
    entries = {}
    for x, mid, flipped, e in passes:
        entries.setdefault(e, []).append((x, mid, flipped))
    px = lambda s: b * c * s[0] * s[1] * 4
    for e, group in entries.items():
        mid = group[0][1]
        for x, _, flipped in group:
            if tuple(x.shape[2:]) != mid:
                total += px(x.shape[2:]) + px(mid)              # resize: read x, write the map
            if flipped:
                total += 2 * px(mid)                            # flip: read, write
        total += (len(group) - 1) * 3 * px(mid)                 # max: two reads, one write
        if mid != out:
            total += px(mid) + px(out)                          # the entry resized
        if e > 0:
            total += 5 * px(out)                                # the 'mean' fold: add (2 reads, 1 write), then scale (1 read, 1 write)
    total += px(out) + b * out[0] * out[1] * (8 + 8 + 1)        # argmax: read logits, write int64; the cast: read int64, write uint8
    return total


def merged_bytes(passes, c, b=1):
    out = passes[0][1]
    return sum(b * c * x.shape[2] * x.shape[3] * 4 for x, _, _, _ in passes) + b * out[0] * out[1]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'tta_merge_time.txt'))
    args = ap.parse_args()
    require_gpu('tta_merge_time.py')
    from hyperseg_amd import configs, functional as HF
    from hyperseg_amd.fps import ConfusionMatrix
    from hyperseg_amd.models._common import Epilogue
    from hyperseg_amd.utils.inference import prepare_for_inference
    from hyperseg_amd.utils.synthetic import fill_by_name
    dev = torch.device('cuda:0')
    h, w, n = 512, 1024, 19
    model = fill_by_name(configs.build('hyperseg-m').eval(), seed=0)
    prepare_for_inference(model, fold_bn=False, fused_depthwise=True)
    model = model.to(dev)
    assert model.inference_hflip and model.inference_gather == 'mean'
    g = torch.Generator().manual_seed(1)
    x = torch.rand(1, 3, h, w, generator=g).to(dev)
    one, three = [x], [x, torch.nn.functional.avg_pool2d(x, 2).contiguous(), torch.nn.functional.avg_pool2d(x, 4).contiguous()]
    label = torch.randint(0, n, (1, h, w), generator=g).to(dev)
    keep = {}

    def route(on, fn):
        def run():
            HF.TTA_MERGE = on
            try:
                with torch.no_grad():
                    return fn()
            finally:
                HF.TTA_MERGE = True
        return run

    def evaluate(key):
        def run():
            cm = ConfusionMatrix(n)
            keep[key] = (model.evaluate(one, label, cm), cm.mat)
        return run

    def segment(key, xs):
        def run():
            keep[key] = model.segment(xs)
        return run

    whole = {
        'segment 2 passes, merged': route(True, segment('s2m', one)), 'segment 2 passes, composed': route(False, segment('s2c', one)),
        'segment 6 passes, merged': route(True, segment('s6m', three)), 'segment 6 passes, composed': route(False, segment('s6c', three)),
        'evaluate 2 passes, merged': route(True, evaluate('e2m')), 'evaluate 2 passes, composed': route(False, evaluate('e2c')),
    }
    # the epilogue alone: the decoder's per-pass outputs, resident
    def deferred(xs):
        with torch.no_grad():
            return [(d.x, d.size, f, e) for e, t in enumerate(xs) for f in (False, True)
                    for d in [model.process_single_tensor(t, hflip=f, epilogue=Epilogue(defer=True))]]
    p2, p6 = deferred(one), deferred(three)
    alone = {
        'epilogue 2 passes, merge launch': lambda: keep.__setitem__('a2m', HF.tta_merge(p2, 'mean').masks),
        'epilogue 2 passes, composed launches': lambda: keep.__setitem__('a2c', HF.tta_merge_composed(p2, 'mean').masks),
        'epilogue 6 passes, merge launch': lambda: keep.__setitem__('a6m', HF.tta_merge(p6, 'mean').masks),
        'epilogue 6 passes, composed launches': lambda: keep.__setitem__('a6c', HF.tta_merge_composed(p6, 'mean').masks),
    }
    for fn in list(whole.values()) + list(alone.values()):
        fn()
    torch.cuda.synchronize()
    assert torch.equal(keep['a2m'], keep['a2c']) and torch.equal(keep['a6m'], keep['a6c'])
    same = (torch.equal(keep['s2m'], keep['s2c']), torch.equal(keep['s6m'], keep['s6c']),
            torch.equal(keep['e2m'][0], keep['e2c'][0]) and torch.equal(keep['e2m'][1], keep['e2c'][1]))
    lines = Lines()
    lines.append(f'HyperSeg-M {w}x{h} bs 1, prepared, eager, resident input, inference_hflip on; {args.rounds} interleaved rounds, ms per call')
    lines.append(f'same masks merged / composed (two separate forwards each): 2 passes {same[0]}, 6 passes {same[1]}; evaluate masks and matrix {same[2]}')
    lines.append('same masks from the same decoder outputs (asserted): 2 passes True, 6 passes True')
    med, spread = interleaved(lines, f'whole calls (host clock, {args.reps} calls per sample)',
                              {k: (wall_ms, fn, args.reps) for k, fn in whole.items()}, args.rounds, 3)
    for k in ('segment 2 passes', 'segment 6 passes', 'evaluate 2 passes'):
        lines.append('  ' + verdict(f'{k}: composed - merged', f'{k}, merged', f'{k}, composed', med, spread))
    med, spread = interleaved(lines, f'the epilogue alone (device events, {10 * args.reps} calls per sample)',
                              {k: (region_ms, fn, 10 * args.reps) for k, fn in alone.items()}, args.rounds, 3)
    for k in ('epilogue 2 passes', 'epilogue 6 passes'):
        lines.append('  ' + verdict(f'{k}: composed - merge', f'{k}, merge launch', f'{k}, composed launches', med, spread))
    for name, p in (('2 passes', p2), ('6 passes', p6)):
        lines.append(f'bytes, {name}: decoder outputs ' + ' + '.join(f'{tuple(t.shape[2:])}' for t, _, _, _ in p) +
                     f'; merge launch reads {merged_bytes(p, n) / 1e6:.1f} MB incl. the masks written; composed launches move {composed_bytes(p, n) / 1e6:.1f} MB')
    write_report(lines, args.out)


if __name__ == '__main__':
    main()
