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
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)


def region_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def protocol_ms(fn, reps):
    total = 0.0
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        total += time.perf_counter() - t0
    return 1e3 * total / reps


def report(lines, title, samples):
    med = {}
    lines.append(title)
    for k, s in samples.items():
        med[k] = statistics.median(s)
        lines.append(f'  {k:46s} median {med[k]:.4f}  min {min(s):.4f}  max {max(s):.4f}  spread {max(s) - min(s):.4f}   samples ' +
                     ' '.join(f'{v:.4f}' for v in s))
    return med, {k: max(s) - min(s) for k, s in samples.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'uint8_ingest_time.txt'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('ingest_time.py measures on the GPU: no device found')
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
    lines = [f'HyperSeg-M {w}x{h} bs 1, prepared (split GEMM), HIP-graph replay; {args.rounds} interleaved rounds x {args.reps} frames',
             f'logits of the float route, the fused uint8 stem and the image_ingest route equal: {same}']
    for title, timer, variants in groups:
        for fn in variants.values():                                   # every graph and shape warm before anything is timed
            for _ in range(10):
                fn()
        torch.cuda.synchronize()
        samples = {k: [] for k in variants}
        for _ in range(args.rounds):
            for k, fn in variants.items():
                samples[k].append(timer(fn, args.reps))
        med, spread = report(lines, title, samples)
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
            for _ in range(5):
                HF.image_ingest(x, nl, out=out)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                for _ in range(50):
                    HF.image_ingest(x, nl, out=out)
            graph.replay()
            s = [1e3 * region_ms(graph.replay, 20) / 50 for _ in range(5)]
            us = statistics.median(s)
            mb = 5 * 3 * hh * ww / 1e6
            lines.append(f"  {ww}x{hh} '{layout}': {us:7.2f} us per launch (min {min(s):.2f} max {max(s):.2f})  {mb:.2f} MB  ->  {mb / us:.2f} TB/s "
                         f'= {100 * mb / us / 8:.0f} % of the 8 TB/s roof')
    lines.append('  note: these are launches inside ONE replayed graph writing the same output again and again: what the figure shows is the cost of '
                 'a small launch in a graph with its output staying in the 256 MB last-level cache -- neither the HBM roof nor the cost of '
                 'the launch inside a frame, which (b) gives as the difference between the image_ingest route and the float route')
    text = '\n'.join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text + '\n')
    assert same, 'the uint8 routes disagree with the float route'


if __name__ == '__main__':
    with torch.no_grad():               # GraphedModel.forward replays only where nothing can ask for a gradient
        main()
