"""What feeding uint8 frames costs and saves: HyperSeg-M, 1024 x 512, batch 1, after prepare_for_inference, through GraphedModel.

    timeout -k 10 600 python tools/ingest_time.py [--rounds 7] [--reps 200] [--out profiles/uint8_ingest_time.txt]

One process, the variants of each group timed INTERLEAVED (``--rounds`` rounds, every sample ``--reps`` frames):
  (a) the reference's protocol (test_fps.py:173-188: synchronize -> perf_counter -> host-to-device copy of a pinned frame + forward ->
      synchronize, per frame): a pinned float32 (1, 3, H, W) frame against a pinned uint8 'hwc' (1, H, W, 3) frame; the host clock;
  (b) resident-input replay (device events around the region, as bench.py times): the float route, the uint8 frame read by the stem +
      depthwise launch itself (hs_stem_dw_u8_fwd), and the uint8 frame through one image_ingest launch in front of the float route;
  (c) image_ingest alone -- a graph of 50 launches replayed, device events -- in us and achieved GB/s (1 byte read + 4 written per
      value), for HyperSeg-M's frame and for 1024 x 768, both layouts.
All uint8 variants must produce the float route's logits bit for bit (asserted)."""
import argparse
import os
import statistics

import torch

from _measure import REPO, Lines, graph_of, interleaved, protocol_ms, region_ms, require_gpu, write_report


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'uint8_ingest_time.txt'))
    args = ap.parse_args()
    require_gpu('ingest_time.py')
    from hyperseg_amd import configs, functional as HF
    from hyperseg_amd.utils.inference import GraphedModel, InputNorm, prepare_for_inference
    from hyperseg_amd.utils.synthetic import fill_by_name
    dev = torch.device('cuda:0')
    h, w = 512, 1024
    norm = InputNorm(layout='hwc')
    model = fill_by_name(configs.build('hyperseg-m').eval(), seed=0)
    prepare_for_inference(model, fold_bn=False, fused_depthwise=True, split_gemm=True, input_norm=norm)
    model = model.to(dev)
    u8_host = torch.randint(0, 256, (1, h, w, 3), generator=torch.Generator().manual_seed(1), dtype=torch.uint8).pin_memory()
    f32_host = norm.to_float(u8_host).pin_memory()                      # the reference's loader output for the same frame
    u8_dev, f32_dev = u8_host.to(dev), f32_host.to(dev)
    served = GraphedModel(model)                                        # float graph + the fused uint8 graph
    served_ingest = GraphedModel(model)                                 # the uint8 graph with image_ingest in front of the float route
    HF.U8_STEM = False
    try:
        out_ingest = served_ingest(u8_dev).clone()
    finally:
        HF.U8_STEM = True
    out_f32, out_u8 = served(f32_dev).clone(), served(u8_dev).clone()
    same = torch.equal(out_f32, out_u8) and torch.equal(out_f32, out_ingest)

    groups = [('(a) reference protocol: sync, H2D of a pinned frame + replay, sync; host clock, ms per frame', protocol_ms,
               {'float32 pinned (6.3 MB over the host link)': lambda: served(f32_host),
                "uint8 'hwc' pinned (1.6 MB), fused stem": lambda: served(u8_host),
                "uint8 'hwc' pinned (1.6 MB), image_ingest": lambda: served_ingest(u8_host)}),
              ('(b) resident input, replay only; device events, ms per frame', region_ms,
               {'float32 route': lambda: served(f32_dev),
                'uint8 fused stem (hs_stem_dw_u8_fwd)': lambda: served(u8_dev),
                'uint8 through image_ingest + float route': lambda: served_ingest(u8_dev)})]
    lines = Lines()
    lines.append(f'HyperSeg-M {w}x{h} bs 1, prepared (split GEMM), HIP-graph replay; {args.rounds} interleaved rounds x {args.reps} frames')
    lines.append(f'logits of the float route, the fused uint8 stem and the image_ingest route equal: {same}')
    for title, timer, variants in groups:
        med, spread = interleaved(lines, title, {k: (timer, fn, args.reps) for k, fn in variants.items()}, args.rounds, warmup=10)
        keys = list(variants)
        for k in keys[1:]:
            lines.append(f'  [{k}] - [{keys[0]}] = {med[k] - med[keys[0]]:+.4f} ms  (spread of the two: {max(spread[k], spread[keys[0]]):.4f})')
        lines.append(f'  [{keys[1]}] - [{keys[2]}] = {med[keys[1]] - med[keys[2]]:+.4f} ms  (spread of the two: {max(spread[keys[1]], spread[keys[2]]):.4f})')

    lines.append('(c) image_ingest alone: a graph of 50 launches replayed 20 times per sample, device events; bytes = 5 per value (1 read, 4 written)')
    for (hh, ww) in ((512, 1024), (768, 1024)):
        for layout in ('hwc', 'chw'):
            nl = InputNorm(layout=layout)
            shape = (1, hh, ww, 3) if layout == 'hwc' else (1, 3, hh, ww)
            x = torch.randint(0, 256, shape, generator=torch.Generator().manual_seed(2), dtype=torch.uint8).to(dev)
            out = torch.empty(1, 3, hh, ww, device=dev)
            graph = graph_of(lambda: HF.image_ingest(x, nl, out=out), 50, warm=5)
            s = [1e3 * region_ms(graph.replay, 20) / 50 for _ in range(5)]
            us = statistics.median(s)
            mb = 5 * 3 * hh * ww / 1e6
            lines.append(f"  {ww}x{hh} '{layout}': {us:7.2f} us per launch (min {min(s):.2f} max {max(s):.2f})  {mb:.2f} MB  ->  {mb / us:.2f} TB/s "
                         f'= {100 * mb / us / 8:.0f} % of the 8 TB/s roof')
    lines.append('  note: these are launches inside ONE replayed graph writing the same output again and again: what the figure shows is the cost of '
                 'a small launch in a graph with its output staying in the 256 MB last-level cache -- neither the HBM roof nor the cost of '
                 'the launch inside a frame, which (b) gives as the difference between the image_ingest route and the float route')
    write_report(lines, args.out)
    assert same, 'the uint8 routes disagree with the float route'


if __name__ == '__main__':
    with torch.no_grad():               # GraphedModel.forward replays only where nothing can ask for a gradient
        main()
