"""What resizing the camera frame on the device costs and saves: HyperSeg-M, 2048 x 1024 camera frames -> 1024 x 512, batch 1, after
prepare_for_inference, through GraphedModel.

    timeout -k 10 900 python tools/frame_resize_time.py [--rounds 7] [--reps 200] [--out profiles/frame_resize_time.txt]

One process, the legs of each group timed INTERLEAVED (``--rounds`` rounds, every sample ``--reps`` frames):
  (a) host: ``PIL.Image.resize(BILINEAR)`` of the camera frame on one thread, then the reference's protocol (test_fps.py:173-188:
      synchronize -> perf_counter -> ... -> synchronize, per frame) around resize + H2D of the 1.5 MB frame + replay; the host clock.
      Skipped, and stated as skipped, where Pillow is not installed;
  (b) device: the same protocol around H2D of the 6.3 MB camera frame + ONE replay with the resize as the graph's first node;
  (c) / (d) the two replays with resident inputs (device events around the region, as bench.py times): (d) - (c) is what the resize
      costs inside a replay;
  (e) hs_frame_resize_fwd alone -- a graph of 50 launches replayed, device events -- beside hs_image_ingest_fwd alone on the resized
      frame, in us and achieved TB/s (6.3 MB read + 1.6 MB written).
The masks of (b) / (d) must equal those of (c) on the frame ``FrameResize`` makes, and -- with Pillow -- that frame Pillow's bytes (asserted)."""
import argparse
import os
import statistics

import torch

from _measure import REPO, Lines, exceeds, graph_of, interleaved, protocol_ms, region_ms, require_gpu, write_report


def launches_us(fn, lines, name, mb):
    graph = graph_of(fn, 50, warm=5)
    s = [1e3 * region_ms(graph.replay, 20) / 50 for _ in range(5)]
    us = statistics.median(s)
    lines.append(f'  {name:46s} {us:7.2f} us per launch (min {min(s):.2f} max {max(s):.2f})  {mb:.2f} MB  ->  {mb / us:.3f} TB/s '
                 f'= {100 * mb / us / 8:.1f} % of the 8 TB/s roof')
    return us


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'frame_resize_time.txt'))
    args = ap.parse_args()
    require_gpu('frame_resize_time.py')
    try:
        from PIL import Image
    except ImportError:
        Image = None
    from hyperseg_amd import configs, functional as HF
    from hyperseg_amd.utils.inference import FrameResize, GraphedModel, InputNorm, prepare_for_inference
    from hyperseg_amd.utils.synthetic import fill_by_name
    dev = torch.device('cuda:0')
    (h, w), (hc, wc) = (512, 1024), (1024, 2048)
    norm, resize = InputNorm(layout='hwc'), FrameResize((h, w), 'bilinear', 'hwc')

    def build(**kw):
        m = fill_by_name(configs.build('hyperseg-m').eval(), seed=0)
        prepare_for_inference(m, fold_bn=False, fused_depthwise=True, split_gemm=True, input_norm=norm, **kw)
        return GraphedModel(m.to(dev), masks=True)
    plain, resizing = build(), build(input_resize=resize)          # two models of equal weights: each graph holds its own route

    cam_host = torch.randint(0, 256, (1, hc, wc, 3), generator=torch.Generator().manual_seed(1), dtype=torch.uint8).pin_memory()
    cam_np = cam_host[0].numpy()
    cam_dev = cam_host.to(dev)
    small_dev = resize(cam_dev)
    small_host = torch.empty((1, h, w, 3), dtype=torch.uint8).pin_memory()
    small_np = small_host[0].numpy()
    small_host.copy_(small_dev)
    same = torch.equal(plain(small_dev).clone(), resizing(cam_dev).clone()) and torch.equal(plain(small_host).clone(), resizing(cam_host).clone())
    pillow_same = None
    if Image is not None:
        import numpy as np
        pillow_same = bool((np.asarray(Image.fromarray(cam_np).resize((w, h), Image.BILINEAR)) == small_dev[0].cpu().numpy()).all())

    def host_leg():
        small_np[...] = Image.fromarray(cam_np).resize((w, h), Image.BILINEAR)
        return plain(small_host)

    lines = Lines()
    lines.append(f'HyperSeg-M, camera {wc}x{hc} -> {w}x{h} bilinear, bs 1, prepared (split GEMM), HIP-graph replay, uint8 masks out; '
                 f'{args.rounds} interleaved rounds x {args.reps} frames')
    lines.append(f'masks with the resize in the graph equal the masks on the resized frame: {same}')
    lines.append(f'the resized frame equals PIL.Image.resize byte for byte: {pillow_same if Image is not None else "Pillow is not installed"}')
    legs = {}
    if Image is not None:
        legs['(a) host PIL resize (1 thread) + H2D 1.6 MB + replay'] = (protocol_ms, host_leg, args.reps)
    else:
        lines.append('(a) SKIPPED: Pillow is not installed on this machine')
    legs['(b) H2D 6.3 MB camera frame + replay with the resize'] = (protocol_ms, lambda: resizing(cam_host), args.reps)
    med, spread = interleaved(lines, '(a) / (b) reference protocol: sync, [resize,] H2D of a pinned frame + replay, sync; host clock, ms per frame',
                              legs, args.rounds, warmup=10)
    keys = list(legs)
    if len(keys) == 2:
        diff, both = med[keys[0]] - med[keys[1]], spread[keys[0]] + spread[keys[1]]
        lines.append(f'  (a) - (b) = {diff:+.4f} ms; sum of the two spreads {both:.4f}: (b) is '
                     f'{"below (a) by more than that" if exceeds(keys[0], keys[1], med, spread) else "NOT below (a) by more than that"}')
    legs = {'(c) resident resized frame, replay': (region_ms, lambda: plain(small_dev), args.reps),
            '(d) resident camera frame, replay with the resize': (region_ms, lambda: resizing(cam_dev), args.reps)}
    med, spread = interleaved(lines, '(c) / (d) resident input, replay only; device events, ms per frame', legs, args.rounds, warmup=10)
    keys = list(legs)
    lines.append(f'  (d) - (c) = {med[keys[1]] - med[keys[0]]:+.4f} ms: the resize inside a replay  (sum of the two spreads: '
                 f'{spread[keys[0]] + spread[keys[1]]:.4f})')

    lines.append('(e) kernels alone: a graph of 50 launches replayed 20 times per sample, device events')
    out_u8, out_f = torch.empty_like(small_dev), torch.empty(1, 3, h, w, device=dev)
    mb = (3 * hc * wc + 3 * h * w) / 1e6
    launches_us(lambda: HF.frame_resize(cam_dev, (h, w), 'bilinear', 'hwc', out=out_u8), lines, 'frame_resize 2048x1024 -> 1024x512 uint8', mb)
    launches_us(lambda: HF.frame_resize(cam_dev, (h, w), 'bilinear', 'hwc', norm=norm, out=out_f), lines, 'frame_resize ... -> float32 planar',
                (3 * hc * wc + 12 * h * w) / 1e6)
    launches_us(lambda: HF.frame_resize(cam_dev, (h, w), 'bicubic', 'hwc', out=out_u8), lines, 'frame_resize ... bicubic uint8', mb)
    launches_us(lambda: HF.image_ingest(small_dev, norm, out=out_f), lines, 'image_ingest 1024x512', 15 * h * w / 1e6)
    lines.append('  note: launches inside ONE replayed graph reading and writing the same buffers again and again -- they stay in the 256 MB '
                 'last-level cache; the cost inside a frame is (d) - (c)')
    write_report(lines, args.out)
    assert same, 'the resize inside the graph disagrees with the resized frame'
    assert pillow_same is not False, 'the device resize disagrees with Pillow'


if __name__ == '__main__':
    with torch.no_grad():               # GraphedModel replays only where nothing can ask for a gradient
        main()
