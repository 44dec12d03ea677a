"""What the Gaussian blur costs on the host and on the device: the Cityscapes HyperSeg-S training shape -- batch 16, 768 x 768 crops,
RandomGaussianBlur's default radius (sigma) 5, every sample blurred.

    timeout -k 10 900 python tools/gaussian_blur_time.py [--rounds 7] [--reps 20] [--parent-tree DIR] [--out profiles/gaussian_blur_time.txt]

One process, the legs of each group timed INTERLEAVED (``--rounds`` rounds):
  (a) host, what a user has today: ``img.filter(ImageFilter.GaussianBlur(5))`` on one thread, per image and per batch of 16; the host
      clock.  Skipped, and stated as skipped, where Pillow is not installed;
  (b) device: ``functional.gaussian_blur`` of the resident uint8 batch into the normalised float32 batch through a caller-owned table --
      a graph of 50 calls (each: the row launch + the column launch) replayed, device events; per batch;
  (c) ``training.device_augment`` of 16 camera frames (2048 x 1024, scale 0.75, crop 768 x 768) with and without ``blur=``: eager
      launches, device events around the call;
  (d) for (b): the bytes it must move (the row launch reads the uint8 batch and writes the uint8 intermediate, the column launch reads
      that and writes float32) over its time, as a fraction of the 8 TB/s roof.
With ``--parent-tree`` (a checkout of the parent commit, built): ``python bench.py --gpus 1 --steps 200 --warmup 20`` of that tree and of
this one, as fresh child processes, alternating, ``--bench-rounds`` times each; both values go into the same file.
The device's bytes must equal the CPU implementation's and -- with Pillow -- Pillow's (asserted)."""
import argparse
import os

import torch

from _measure import REPO, Lines, compare_bench, exceeds, graph_of, host_ms, interleaved, per_launch, region_ms, require_gpu, write_report


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--parent-tree', default=None)
    ap.add_argument('--bench-rounds', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'gaussian_blur_time.txt'))
    args = ap.parse_args()
    require_gpu('gaussian_blur_time.py')
    try:
        import numpy as np
        from PIL import Image, ImageFilter
    except ImportError:
        Image = None
    from hyperseg_amd import functional as HF
    from hyperseg_amd.training import device_augment
    from hyperseg_amd.utils import blur as BL
    from hyperseg_amd.utils.inference import InputNorm
    dev = torch.device('cuda:0')
    b, h, w, sigma = 16, 768, 768, 5
    norm = InputNorm(layout='hwc')
    g = torch.Generator().manual_seed(1)
    params = [BL.GaussianBlurParams(sigma)] * b
    # smooth content with noise on top, a frame of its own per sample
    yy, xx = torch.meshgrid(torch.arange(h), torch.arange(w), indexing='ij')
    base = torch.stack(((yy + 2 * xx) % 256, (3 * yy + xx) % 256, (yy * xx // 64) % 256), -1)
    crops = ((base[None] + torch.randint(0, 64, (b, h, w, 3), generator=g)) % 256).to(torch.uint8)
    crops_dev = crops.to(dev)
    table = BL.params_table(params, b).to(dev)
    status = torch.zeros(b, dtype=torch.int32, device=dev)
    out_f = torch.empty(b, 3, h, w, device=dev)

    got = HF.gaussian_blur(crops_dev, params, 'hwc').cpu()
    cpu_same = torch.equal(got[:2], BL.gaussian_blur_cpu(crops[:2], params[:2], 'hwc'))
    pillow = lambda a: np.asarray(Image.fromarray(a).filter(ImageFilter.GaussianBlur(radius=sigma)))
    pillow_same = None
    if Image is not None:
        pillow_same = all(bool((pillow(crops[i].numpy()) == got[i].numpy()).all()) for i in range(b))
    r, ww, fw = BL.weights(sigma)
    lines = Lines()
    lines.append(f'GaussianBlur({sigma}) = box radius {r}, ww {ww}, fw {fw}; batch {b}, {w}x{h} uint8 hwc crops, every sample blurred; '
                 f'{args.rounds} interleaved rounds')
    lines.append(f'the device bytes equal the CPU implementation (first 2 samples): {cpu_same}')
    lines.append(f'the device bytes equal Pillow (all {b} samples): {pillow_same if Image is not None else "Pillow is not installed"}')

    launches = 50
    call = lambda: HF.gaussian_blur(crops_dev, None, 'hwc', norm=norm, out=out_f, table=table, status=status)
    graph = graph_of(call, launches, warm=3)
    legs = {}
    if Image is not None:
        arrays = [c.numpy() for c in crops]
        legs['(a) host Pillow, 1 thread, per image (sample 0)'] = (host_ms, lambda: pillow(arrays[0]), 3)
        legs[f'(a) host Pillow, 1 thread, per batch of {b}'] = (host_ms, lambda: [pillow(a) for a in arrays], 1)
    else:
        lines.append('(a) SKIPPED: Pillow is not installed on this machine')
    key_b = f'(b) device gaussian_blur -> float32, per batch of {b} (graph of {launches})'
    legs[key_b] = (per_launch(launches), graph.replay, args.reps)
    med, spread = interleaved(lines, '(a) host clock / (b) device events; ms', legs, args.rounds, warmup=3)
    beats = None
    if Image is not None:
        key_a = f'(a) host Pillow, 1 thread, per batch of {b}'
        beats = exceeds(key_a, key_b, med, spread)
        lines.append(f'  (a) / (b) per batch = {med[key_a] / med[key_b]:.0f}x; (a) - (b) = {med[key_a] - med[key_b]:+.4f} ms, sum of the two spreads '
                     f'{spread[key_a] + spread[key_b]:.4f}: the device route beats the host route by more than that: {beats}')
    mb = b * h * w * (3 + 3 + 3 + 12) / 1e6
    us = 1e3 * med[key_b]
    lines.append(f'(d) bytes (b) must move: {b} x {h} x {w} x (3 read + 3 written by the row launch, 3 read + 12 written by the column launch) = '
                 f'{mb:.1f} MB; {us:.1f} us  ->  {mb / us:.3f} TB/s = {100 * mb / us / 8:.1f} % of the 8 TB/s roof  (2 launches per call; the '
                 f'uint8 batch and the intermediate, {b * h * w * 3 / 1e6:.1f} MB each, fit the 256 MB last-level cache between the launches and '
                 f'between replays; the work is 6 passes of byte arithmetic in LDS, not the traffic)')

    hc, wc = 1024, 2048
    frames = torch.randint(0, 256, (b, hc, wc, 3), generator=g, dtype=torch.uint8).to(dev)
    labels = torch.randint(0, 19, (b, hc, wc), generator=g, dtype=torch.uint8).to(dev)
    aug = lambda blur: device_augment(frames, labels, 0.75, (h, w), (0, 384), False, norm, blur=blur)
    legs = {'(c) device_augment, 16 frames 2048x1024 -> 768x768, no blur': (region_ms, lambda: aug(None), 5),
            '(c) device_augment, the same with blur=': (region_ms, lambda: aug(params), 5)}
    med, spread = interleaved(lines, '(c) eager launches, device events; ms per batch', legs, args.rounds, warmup=3)
    keys = list(legs)
    lines.append(f'  with - without = {med[keys[1]] - med[keys[0]]:+.4f} ms per batch (sum of the two spreads {spread[keys[0]] + spread[keys[1]]:.4f})')

    bench_error = compare_bench(lines, args.parent_tree, args.bench_rounds)
    write_report(lines, args.out)
    assert cpu_same, 'the device blur disagrees with the CPU implementation'
    assert pillow_same is not False, 'the device blur disagrees with Pillow'
    assert beats is not False, 'the device route does not beat the host route by more than the sum of the two spreads'
    if bench_error is not None:
        raise bench_error


if __name__ == '__main__':
    with torch.no_grad():
        main()
