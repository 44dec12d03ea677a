"""What the rotation of the VOC train chain costs on the host and on the device: the VOC-SBD HyperSeg-L training shape -- batch 32, sources
about 375 x 500 scaled by 0.6 (225 x 300), RandomRotation(30.) with an angle of its own per sample, ConstantPad(512).

    timeout -k 10 900 python tools/rotate_time.py [--rounds 7] [--reps 20] [--parent-tree DIR] [--out profiles/rotate_time.txt]

One process, the legs of each group timed INTERLEAVED (``--rounds`` rounds):
  (a) host, what a user has today: ``PIL.Image.rotate`` (BICUBIC frame + NEAREST label) on one thread, per image and per batch of 32; the
      host clock.  Skipped, and stated as skipped, where Pillow is not installed;
  (b) device: ``functional.frame_rotate`` of the resident uint8 batch into the normalised, padded float32 batch, and
      ``functional.label_rotate`` into the padded int64 batch, each through a caller-owned table -- a graph of 50 launches replayed, device
      events; per launch (= per batch);
  (c) ``training.device_augment_voc`` of 32 frames 375 x 500 (flip, jitter, scale 0.6, angle, pad 512): eager launches, device events
      around the call; with and without ``jitter=``.
With ``--parent-tree`` (a checkout of the parent commit, built): ``python bench.py --gpus 1 --steps 200 --warmup 20`` of that tree and of
this one, as fresh child processes, alternating, ``--bench-rounds`` times each; both values go into the same file.
The device's bytes must equal the CPU implementation's and -- with Pillow -- Pillow's (asserted)."""
import argparse
import os

import torch

from _measure import REPO, Lines, compare_bench, graph_of, host_ms, interleaved, per_launch, region_ms, require_gpu, write_report


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--parent-tree', default=None)
    ap.add_argument('--bench-rounds', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'rotate_time.txt'))
    args = ap.parse_args()
    require_gpu('rotate_time.py')
    try:
        import numpy as np
        from PIL import Image
    except ImportError:
        Image = None
    from hyperseg_amd import functional as HF
    from hyperseg_amd.training import device_augment_voc, draw_color_jitter
    from hyperseg_amd.utils import rotate as RT
    from hyperseg_amd.utils.inference import InputNorm
    dev = torch.device('cuda:0')
    b, hs, ws, scale, pad = 32, 375, 500, 0.6, 512
    h, w = round(hs * scale), round(ws * scale)
    norm = InputNorm(layout='hwc')
    g = torch.Generator().manual_seed(1)
    angles = ((torch.rand(b, generator=g, dtype=torch.float64) * 2 - 1) * 30.0).tolist()
    # smooth content with noise on top
    yy, xx = torch.meshgrid(torch.arange(h), torch.arange(w), indexing='ij')
    base = torch.stack(((yy + 2 * xx) % 256, (3 * yy + xx) % 256, (yy * xx // 64) % 256), -1)
    frames = ((base[None] + torch.randint(0, 64, (b, h, w, 3), generator=g)) % 256).to(torch.uint8)
    labels = torch.randint(0, 21, (b, h, w), generator=g, dtype=torch.uint8)
    frames_dev, labels_dev = frames.to(dev), labels.to(dev)
    m, f = RT.matrix_table(h, w, angles, b).to(dev), RT.fixed_table(h, w, angles, b).to(dev)
    img = torch.empty(b, 3, pad, pad, device=dev)
    lbl = torch.empty(b, pad, pad, dtype=torch.int64, device=dev)

    got, lgot = HF.frame_rotate(frames_dev, angles).cpu(), HF.label_rotate(labels_dev, angles).cpu()
    cpu_same = torch.equal(got[:2], RT.frame_rotate_cpu(frames[:2], angles[:2])) and torch.equal(lgot[:2], RT.label_rotate_cpu(labels[:2], angles[:2]))
    pillow_same = None
    if Image is not None:
        pillow_same = all(bool((np.asarray(Image.fromarray(frames[i].numpy()).rotate(angles[i], Image.BICUBIC)) == got[i].numpy()).all()) and
                          bool((np.asarray(Image.fromarray(labels[i].numpy()).rotate(angles[i], Image.NEAREST)) == lgot[i].numpy()).all())
                          for i in range(b))
    lines = Lines()
    lines.append(f'RandomRotation(30.) + ConstantPad({pad}), batch {b}, {w}x{h} uint8 hwc frames ({ws}x{hs} scaled by {scale}) and uint8 labels, an angle '
                 f'per sample; {args.rounds} interleaved rounds')
    lines.append(f'the device bytes equal the CPU implementation (first 2 samples, frame and label): {cpu_same}')
    lines.append(f'the device bytes equal Pillow (all {b} samples, frame and label): {pillow_same if Image is not None else "Pillow is not installed"}')

    launches = 50
    g_frame = graph_of(lambda: HF.frame_rotate(frames_dev, None, size=(pad, pad), norm=norm, out=img, table=m), launches, warm=3)
    g_label = graph_of(lambda: HF.label_rotate(labels_dev, None, size=(pad, pad), out=lbl, table=f), launches, warm=3)
    legs = {}
    if Image is not None:
        fa, la = [x.numpy() for x in frames], [t.numpy() for t in labels]

        def pillow_rotate(i):
            return (np.asarray(Image.fromarray(fa[i]).rotate(angles[i], Image.BICUBIC)), np.asarray(Image.fromarray(la[i]).rotate(angles[i], Image.NEAREST)))
        legs['(a) host Pillow, 1 thread, frame + label, per image (sample 0)'] = (host_ms, lambda: pillow_rotate(0), 5)
        legs[f'(a) host Pillow, 1 thread, frame + label, per batch of {b}'] = (host_ms, lambda: [pillow_rotate(i) for i in range(b)], 1)
    else:
        lines.append('(a) SKIPPED: Pillow is not installed on this machine')
    key_f = f'(b) device frame_rotate -> padded float32, per launch of {b} (graph of {launches})'
    key_l = f'(b) device label_rotate -> padded int64, per launch of {b} (graph of {launches})'
    legs[key_f] = (per_launch(launches), g_frame.replay, args.reps)
    legs[key_l] = (per_launch(launches), g_label.replay, args.reps)
    med, spread = interleaved(lines, '(a) host clock / (b) device events; ms', legs, args.rounds, warmup=3)
    if Image is not None:
        key_a = f'(a) host Pillow, 1 thread, frame + label, per batch of {b}'
        lines.append(f'  (a) / (b, frame + label) per batch = {med[key_a] / (med[key_f] + med[key_l]):.0f}x')
    mb_f, mb_l = b * (h * w * 3 + pad * pad * 12) / 1e6, b * (h * w + pad * pad * 8) / 1e6
    lines.append(f'  bytes (b) must move: frame {mb_f:.1f} MB (uint8 in, padded float32 out) -> {mb_f / (1e3 * med[key_f]):.3f} TB/s; label {mb_l:.1f} MB '
                 f'(uint8 in, padded int64 out) -> {mb_l / (1e3 * med[key_l]):.3f} TB/s.  Most of both outputs is padding; the frame kernel is a '
                 f'float64 gather on a cache-resident source, not a streaming kernel')

    src = torch.randint(0, 256, (b, hs, ws, 3), generator=g, dtype=torch.uint8).to(dev)
    src_lbl = torch.randint(0, 21, (b, hs, ws), generator=g, dtype=torch.uint8).to(dev)
    flips = [bool(i % 2) for i in range(b)]
    params = [draw_color_jitter(0.5, 0.5, 0.5, 0.5, generator=g) for _ in range(b)]
    aug = lambda jit: device_augment_voc(src, src_lbl, flips, jit, scale, angles, pad, norm)
    legs = {f'(c) device_augment_voc, {b} frames {ws}x{hs} -> {pad}x{pad}, no jitter': (region_ms, lambda: aug(None), 3),
            '(c) device_augment_voc, the same with jitter=': (region_ms, lambda: aug(params), 3)}
    interleaved(lines, '(c) eager launches, device events; ms per batch', legs, args.rounds, warmup=3)

    bench_error = compare_bench(lines, args.parent_tree, args.bench_rounds, unit='value')
    write_report(lines, args.out)
    assert cpu_same, 'the device rotation disagrees with the CPU implementation'
    assert pillow_same is not False, 'the device rotation disagrees with Pillow'
    if bench_error is not None:
        raise bench_error


if __name__ == '__main__':
    with torch.no_grad():
        main()
