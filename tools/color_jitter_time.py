"""What the colour jitter costs on the host and on the device: the Cityscapes HyperSeg-S training shape -- batch 16, 768 x 768 crops,
ColorJitter(0.25, 0.25, 0.25, 0.25), all four operations, an order and factors of its own per sample.

    timeout -k 10 900 python tools/color_jitter_time.py [--rounds 7] [--reps 20] [--parent-tree DIR] [--out profiles/color_jitter_time.txt]

One process, the legs of each group timed INTERLEAVED (``--rounds`` rounds):
  (a) host, what a user has today: Pillow's own calls (ImageEnhance.Brightness / Contrast / Color, convert('HSV') + add + convert('RGB'))
      on one thread, per image and per batch of 16; the host clock.  Skipped, and stated as skipped, where Pillow is not installed;
  (b) device: ``functional.color_jitter`` of the resident uint8 batch into the normalised float32 batch through a caller-owned table --
      a graph of 50 calls (each: clear + mean pass + apply pass) replayed, device events; per batch;
  (c) ``training.device_augment`` of 16 camera frames (2048 x 1024, scale 0.75, crop 768 x 768) with and without ``jitter=``: eager
      launches, device events around the call;
  (d) for (b): the bytes it must move (the mean pass reads the uint8 batch, the apply pass reads it again and writes float32) over its
      time, as a fraction of the 8 TB/s roof.
With ``--parent-tree`` (a checkout of the parent commit, built): ``python bench.py --gpus 1 --steps 200 --warmup 20`` of that tree and of
this one, as fresh child processes, alternating, ``--bench-rounds`` times each; both values go into the same file.
The device's bytes must equal the CPU implementation's and -- with Pillow -- Pillow's (asserted)."""
import argparse
import os

import torch

from _measure import REPO, Lines, compare_bench, graph_of, host_ms, interleaved, per_launch, region_ms, require_gpu, write_report


def pillow_jitter(Image, ImageEnhance, np, a, p):
    img = Image.fromarray(a)
    enh = {'brightness': ImageEnhance.Brightness, 'contrast': ImageEnhance.Contrast, 'saturation': ImageEnhance.Color}
    for name, f in p.steps():
        if name != 'hue':
            img = enh[name](img).enhance(f)
        else:
            h, s, v = img.convert('HSV').split()
            h = Image.fromarray((np.asarray(h).astype(np.int32) + int(f * 255)).astype(np.uint8), 'L')
            img = Image.merge('HSV', (h, s, v)).convert('RGB')
    return np.asarray(img)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--parent-tree', default=None)
    ap.add_argument('--bench-rounds', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'color_jitter_time.txt'))
    args = ap.parse_args()
    require_gpu('color_jitter_time.py')
    try:
        import numpy as np
        from PIL import Image, ImageEnhance
    except ImportError:
        Image = None
    from hyperseg_amd import functional as HF
    from hyperseg_amd.training import device_augment, draw_color_jitter
    from hyperseg_amd.utils import jitter as J
    from hyperseg_amd.utils.inference import InputNorm
    dev = torch.device('cuda:0')
    b, h, w = 16, 768, 768
    norm = InputNorm(layout='hwc')
    g = torch.Generator().manual_seed(1)
    params = [draw_color_jitter(0.25, 0.25, 0.25, 0.25, generator=g) for _ in range(b)]
    # smooth content with noise on top: hue and saturation see real colours, not only gray or only noise
    yy, xx = torch.meshgrid(torch.arange(h), torch.arange(w), indexing='ij')
    base = torch.stack(((yy + 2 * xx) % 256, (3 * yy + xx) % 256, (yy * xx // 64) % 256), -1)
    crops = ((base[None] + torch.randint(0, 64, (b, h, w, 3), generator=g)) % 256).to(torch.uint8)
    crops_dev = crops.to(dev)
    table = J.params_table(params, b).to(dev)
    out_f = torch.empty(b, 3, h, w, device=dev)

    got = HF.color_jitter(crops_dev, params, 'hwc').cpu()
    cpu_same = torch.equal(got[:2], J.color_jitter_cpu(crops[:2], params[:2], 'hwc'))
    pillow_same = None
    if Image is not None:
        pillow_same = all(bool((pillow_jitter(Image, ImageEnhance, np, crops[i].numpy(), params[i]) == got[i].numpy()).all()) for i in range(b))
    lines = Lines()
    lines.append(f'ColorJitter(0.25, 0.25, 0.25, 0.25), batch {b}, {w}x{h} uint8 hwc crops, all four operations, order and factors per sample; '
                 f'{args.rounds} interleaved rounds')
    lines.append(f'the device bytes equal the CPU implementation (first 2 samples): {cpu_same}')
    lines.append(f'the device bytes equal Pillow (all {b} samples): {pillow_same if Image is not None else "Pillow is not installed"}')

    launches = 50
    graph = graph_of(lambda: HF.color_jitter(crops_dev, None, 'hwc', norm=norm, out=out_f, table=table), launches, warm=3)
    legs = {}
    if Image is not None:
        arrays = [c.numpy() for c in crops]
        legs['(a) host Pillow, 1 thread, per image (sample 0)'] = (host_ms, lambda: pillow_jitter(Image, ImageEnhance, np, arrays[0], params[0]), 3)
        legs[f'(a) host Pillow, 1 thread, per batch of {b}'] = (
            host_ms, lambda: [pillow_jitter(Image, ImageEnhance, np, a, p) for a, p in zip(arrays, params)], 1)
    else:
        lines.append('(a) SKIPPED: Pillow is not installed on this machine')
    key_b = f'(b) device color_jitter -> float32, per batch of {b} (graph of {launches})'
    legs[key_b] = (per_launch(launches), graph.replay, args.reps)
    med, spread = interleaved(lines, '(a) host clock / (b) device events; ms', legs, args.rounds, warmup=3)
    if Image is not None:
        key_a = f'(a) host Pillow, 1 thread, per batch of {b}'
        lines.append(f'  (a) / (b) per batch = {med[key_a] / med[key_b]:.0f}x; (a) - (b) = {med[key_a] - med[key_b]:+.4f} ms, sum of the two spreads '
                     f'{spread[key_a] + spread[key_b]:.4f}')
    mb = b * h * w * (3 + 3 + 12) / 1e6
    us = 1e3 * med[key_b]
    lines.append(f'(d) bytes (b) must move: {b} x {h} x {w} x (3 read by the mean pass + 3 read + 12 written by the apply pass) = {mb:.1f} MB; '
                 f'{us:.1f} us  ->  {mb / us:.3f} TB/s = {100 * mb / us / 8:.1f} % of the 8 TB/s roof  (3 launches per call: clear, mean, apply; '
                 f'the uint8 batch, {b * h * w * 3 / 1e6:.1f} MB, fits the 256 MB last-level cache between the two passes and between replays)')

    hc, wc = 1024, 2048
    frames = torch.randint(0, 256, (b, hc, wc, 3), generator=g, dtype=torch.uint8).to(dev)
    labels = torch.randint(0, 19, (b, hc, wc), generator=g, dtype=torch.uint8).to(dev)
    aug = lambda jit: device_augment(frames, labels, 0.75, (h, w), (0, 384), False, norm, jitter=jit)
    legs = {'(c) device_augment, 16 frames 2048x1024 -> 768x768, no jitter': (region_ms, lambda: aug(None), 5),
            '(c) device_augment, the same with jitter=': (region_ms, lambda: aug(params), 5)}
    med, spread = interleaved(lines, '(c) eager launches, device events; ms per batch', legs, args.rounds, warmup=3)
    keys = list(legs)
    lines.append(f'  with - without = {med[keys[1]] - med[keys[0]]:+.4f} ms per batch (sum of the two spreads {spread[keys[0]] + spread[keys[1]]:.4f})')

    bench_error = compare_bench(lines, args.parent_tree, args.bench_rounds)
    write_report(lines, args.out)
    assert cpu_same, 'the device jitter disagrees with the CPU implementation'
    assert pillow_same is not False, 'the device jitter disagrees with Pillow'
    if bench_error is not None:
        raise bench_error


if __name__ == '__main__':
    with torch.no_grad():
        main()
