"""What drawing a frame's overlay costs on top of producing its masks: HyperSeg-M, 1024 x 512, batch 1, after prepare_for_inference.

    timeout -k 10 600 python tools/overlay_time.py [--rounds 7] [--reps 200] [--out profiles/overlay_time.txt]

One process, four variants timed INTERLEAVED (round r times a, b, c, d in turn, ``--rounds`` rounds), each sample a region of ``--reps``
frames between two device events.  The setup is tools/eval_epilogue_time.py's (float image resident on the device, inference_hflip off), so
that (a) is the number recorded in profiles/eval_epilogue_time.txt; the uint8 frame the overlay is blended over is resident as well:
  (a) GraphedModel(masks=True) replay -- masks only;
  (b) (a) + the reference's display chain as stock torch ops on the device (blend_seg: index into the colour map, permute, mask, repeat,
      two multiplies, an add; tensor2rgb: un-normalise, permute, round, cast) -- what a user writes without this feature;
  (c) (a) + one hs_overlay_fwd launch on the masks (functional.overlay);
  (d) GraphedModel.overlay -- the overlay blended by the forward's last launch (hs_upsample_overlay_fwd).
Then the served pipeline, uint8 frame in (the fused stem route): (a8) masks only, (d8) GraphedModel.overlay.
Required (asserted): (c) < (b) and (d) < (b) by more than the spread (max - min over the rounds) of the samples involved; all variants give
the same bytes.  Reported: (d) - (a), (c) - (a), (d) against (c), and the standalone kernel alone (a graph of 50 launches) with its
fraction of the HBM roof for 0.5 MB of masks + 1.5 MB of frame read + 1.5 MB of overlay written.

    timeout -k 10 900 python tools/overlay_time.py --camera [--parent-tree DIR] [--out profiles/overlay_camera_time.txt]

``--camera``: the overlay at the CAMERA frame's size instead -- model frame 1024 x 512 (``input_resize``), camera frame 2048 x 1024 uint8 'hwc'
resident on the device -- four legs, interleaved as above:
  (1) GraphedModel(masks=True) replay -- masks only, at the model's frame (the resize node included in every leg);
  (2) GraphedModel.overlay(camera, size=camera size) -- both resizes of the logits and the blend in the last launch (hs_upsample2_overlay_fwd);
  (3) a replay whose last launch makes segment(size=)'s masks (hs_upsample2_confusion_fwd, masks only), then one hs_overlay_fwd launch;
  (4) the logits replay, then upsample_bilinear to the camera's size, arg-max, hs_overlay_fwd -- the route through the full logits.
Asserted: (2), (3) and (4) give the same bytes.  Reported: the medians and spreads, (2) against (3) by the rule of tools/_measure.py (the
fused route stays ``overlay(size=)``'s unless it is ABOVE (3) by more than the summed spreads), and ``bench.py`` of ``--parent-tree`` and of
this tree, alternating -- it runs none of this."""
import argparse
import os
import statistics

import torch

from _measure import REPO, Lines, compare_bench, exceeds, graph_of, interleaved, region_ms, require_gpu, verdict, write_report

HBM_ROOF = 8.0e12        # bytes / s


def stock_overlay(img, seg, color_map_tensor, alpha, ignore_index):
    """blend_seg + tensor2rgb restated with the same stock ops, everything staying on the device.  img: (B, 3, H, W) float32 normalised with
    mean = std = 0.5; seg: (B, H, W) uint8.  Returns (B, H, W, 3) uint8."""
    seg_classes = seg.long()
    seg_classes[seg_classes >= color_map_tensor.shape[0]] = ignore_index
    seg_rgb = color_map_tensor[seg_classes].permute(0, 3, 1, 2)
    alpha_mask = (1. - (seg_classes != ignore_index).float() * alpha).unsqueeze(1).repeat(1, 3, 1, 1)
    blended = img * alpha_mask + seg_rgb * (1. - alpha_mask)
    out = blended.mul(0.5).add_(0.5).permute(0, 2, 3, 1)
    return torch.round(out * 255).to(torch.uint8)


def camera_rows(args):
    """The ``--camera`` legs: see the module's docstring."""
    from hyperseg_amd import FrameResize, InputNorm, Overlay, configs, functional as HF
    from hyperseg_amd.models._common import Epilogue
    from hyperseg_amd.utils.inference import GraphedModel, prepare_for_inference
    from hyperseg_amd.utils.synthetic import fill_by_name
    dev = torch.device('cuda:0')
    n, (h, w), cam = 19, (512, 1024), (1024, 2048)
    model = fill_by_name(configs.build('hyperseg-m').eval(), seed=0)
    prepare_for_inference(model, fold_bn=False, fused_depthwise=True)
    model.inference_hflip = False
    model = model.to(dev)
    g = torch.Generator().manual_seed(1)
    camera = torch.randint(0, 256, (1, *cam, 3), generator=g, dtype=torch.uint8).to(dev)
    style = Overlay(torch.randint(0, 256, (n, 3), generator=g))
    model.overlay_style, model.input_norm, model.input_resize = style, InputNorm(layout='hwc'), FrameResize((h, w), 'bilinear', 'hwc')
    served, logits_served = GraphedModel(model, masks=True), GraphedModel(model)
    # (3): segment(size=)'s last launch as a graph of the serving wrapper's own kind
    entry = served._capture(('segment-at', cam), [camera], dev,
                            run=lambda xs: model.process_single_tensor(model.resized(xs), epilogue=Epilogue(out_size=cam)))
    out3, out4 = torch.empty_like(camera), torch.empty_like(camera)
    keep = {}

    def r1():
        return served(camera)

    def r2():
        keep['2'] = served.overlay(camera, size=cam)[1]

    def r3():
        keep['3'] = HF.overlay(served._replay(entry, [camera], dev), camera, style, out=out3)

    def r4():
        masks = HF.upsample_bilinear(logits_served(camera), cam).argmax(1).to(torch.uint8)
        keep['4'] = HF.overlay(masks, camera, style, out=out4)

    variants = {'(1) masks only': r1, '(2) overlay(size=), fused': r2, '(3) segment(size=) + hs_overlay_fwd': r3,
                '(4) logits + upsample_bilinear + arg-max + hs_overlay_fwd': r4}
    for fn in variants.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    same = torch.equal(keep['2'], keep['3']) and torch.equal(keep['3'], keep['4'])
    lines = Lines()
    lines.append(f'HyperSeg-M model frame {w}x{h}, camera frame {cam[1]}x{cam[0]} uint8 hwc resident, bs 1, prepared, HIP-graph replay; '
                 f'{args.rounds} interleaved rounds x {args.reps} frames, ms per frame')
    lines.append(f'overlays of (2), (3), (4) equal: {same}')
    med, spread = interleaved(lines, None, {k: (region_ms, fn, args.reps) for k, fn in variants.items()}, args.rounds, warmup=0)
    k1, k2, k3, k4 = variants
    lines.append(verdict('(2) - (1)', k1, k2, med, spread))
    lines.append(verdict('(2) - (3)', k3, k2, med, spread))
    lines.append(verdict('(2) - (4)', k4, k2, med, spread))
    slower = exceeds(k2, k3, med, spread)
    lines.append('routing rule: the fused route is ' + ('ABOVE (3) by more than the summed spreads' if slower else
                                                       'not above (3) by more than the summed spreads: it stays the route of overlay(size=)'))
    error = compare_bench(lines, args.parent_tree, 3)
    write_report(lines, args.out)
    assert same, 'the legs disagree on the overlay'
    if error is not None:
        raise error


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--out', default=None)
    ap.add_argument('--camera', action='store_true', help="the overlay at the camera frame's size: legs (1) - (4) of the docstring")
    ap.add_argument('--parent-tree', default=None, help='with --camera: a built checkout of the parent commit, for the bench.py comparison')
    args = ap.parse_args()
    require_gpu('overlay_time.py')
    if args.camera:
        args.out = args.out or os.path.join(REPO, 'profiles', 'overlay_camera_time.txt')
        return camera_rows(args)
    args.out = args.out or os.path.join(REPO, 'profiles', 'overlay_time.txt')
    from hyperseg_amd import InputNorm, Overlay, configs, functional as HF
    from hyperseg_amd.utils.inference import GraphedModel, prepare_for_inference
    from hyperseg_amd.utils.synthetic import fill_by_name
    dev = torch.device('cuda:0')
    n, (h, w) = 19, (512, 1024)
    model = fill_by_name(configs.build('hyperseg-m').eval(), seed=0)
    prepare_for_inference(model, fold_bn=False, fused_depthwise=True)
    model.inference_hflip = False       # inert for tensor inputs, but segment() / overlay() take their logits + argmax routes while it is set
    model = model.to(dev)
    g = torch.Generator().manual_seed(1)
    x = torch.rand(1, 3, h, w, generator=g).to(dev)
    frames = torch.randint(0, 256, (1, h, w, 3), generator=g, dtype=torch.uint8).to(dev)
    style = Overlay(torch.randint(0, 256, (n, 3), generator=g))
    model.overlay_style = style
    model.input_norm = InputNorm(layout='hwc')
    img = frames.permute(0, 3, 1, 2).to(torch.float32).div(255).sub_(0.5).div_(0.5).contiguous()      # what the reference's user holds
    cmt = style.color_map.to(torch.float32).div_(128.).sub_(1.).to(dev)
    served = GraphedModel(model, masks=True)
    out_c = torch.empty_like(frames)
    keep = {}

    def a():
        return served(x)

    def b():
        keep['b'] = stock_overlay(img, served(x), cmt, style.alpha, style.ignore_index)

    def c():
        keep['c'] = HF.overlay(served(x), frames, style, out=out_c)

    def d():
        keep['d'] = served.overlay(x, frames=frames)[1]

    def a8():
        return served(frames)

    def d8():
        keep['d8'] = served.overlay(frames)[1]

    variants = {'(a)': a, '(b)': b, '(c)': c, '(d)': d, '(a8)': a8, '(d8)': d8}
    for fn in variants.values():                    # every shape and graph warmed before anything is timed
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    same = torch.equal(keep['b'], keep['c']) and torch.equal(keep['c'], keep['d'])
    masks8 = served(frames).clone()
    same8 = torch.equal(keep['d8'], HF.overlay(masks8, frames, style))
    lines = Lines()
    lines.append(f'HyperSeg-M {w}x{h} bs 1, prepared, HIP-graph replay, resident input; {args.rounds} interleaved rounds x {args.reps} frames, ms per frame')
    lines.append(f'overlays of (b), (c), (d) equal: {same};  (d8) equals hs_overlay_fwd on its own masks: {same8}')
    med, spread = interleaved(lines, None, {k: (region_ms, fn, args.reps) for k, fn in variants.items()}, args.rounds, warmup=0)
    lines.append(f'(d) - (a) = {med["(d)"] - med["(a)"]:+.4f} ms   (c) - (a) = {med["(c)"] - med["(a)"]:+.4f} ms   (b) - (a) = {med["(b)"] - med["(a)"]:+.4f} ms   '
                 f'(d8) - (a8) = {med["(d8)"] - med["(a8)"]:+.4f} ms')
    lines.append(f'(b) - (d) = {med["(b)"] - med["(d)"]:.4f} ms vs spread {max(spread["(b)"], spread["(d)"]):.4f};  '
                 f'(b) - (c) = {med["(b)"] - med["(c)"]:.4f} ms vs spread {max(spread["(b)"], spread["(c)"]):.4f};  '
                 f'(c) - (d) = {med["(c)"] - med["(d)"]:+.4f} ms vs spread {max(spread["(c)"], spread["(d)"]):.4f}')
    # the standalone kernel alone: a graph of 50 launches replayed 20 times per sample
    masks = served(x).clone()
    for layout in ('hwc', 'chw'):
        st = Overlay(style.color_map, layout=layout)
        fr = frames if layout == 'hwc' else frames.permute(0, 3, 1, 2).contiguous()
        out = torch.empty_like(fr)
        graph = graph_of(lambda: HF.overlay(masks, fr, st, out=out), 50, warm=3)
        s = [1e3 * region_ms(graph.replay, 20) / 50 for _ in range(5)]
        nbytes = masks.numel() + 2 * fr.numel()
        us = statistics.median(s)
        lines.append(f"hs_overlay_fwd alone, {w}x{h} '{layout}': {us:6.2f} us per launch (min {min(s):.2f} max {max(s):.2f})  {nbytes / 1e6:.2f} MB  ->  "
                     f'{nbytes / us / 1e6:.2f} TB/s = {100 * nbytes / (us * 1e-6) / HBM_ROOF:.0f} % of the 8 TB/s roof')
    lines.append('note: the launches of that graph rewrite one output from inputs that stay in the 256 MB last-level cache: the figure is the cost of '
                 'this small launch inside a graph, not HBM streaming')
    write_report(lines, args.out)
    assert same and same8, 'the variants disagree on the overlay'
    assert med['(b)'] - med['(d)'] > max(spread['(b)'], spread['(d)']), '(d) is not below (b) by more than the spread'
    assert med['(b)'] - med['(c)'] > max(spread['(b)'], spread['(c)']), '(c) is not below (b) by more than the spread'


if __name__ == '__main__':
    with torch.no_grad():               # GraphedModel.forward replays only where nothing can ask for a gradient
        main()
