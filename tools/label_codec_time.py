"""What a dataset's label encoding costs on the host (the reference's numpy lines, one thread) and on the device (``hyperseg_amd.LabelCodec``):
Cityscapes' id table on 1024 x 2048 labels and CamVid's colour list on 720 x 960 labels, batch 16.

    timeout -k 10 900 python tools/label_codec_time.py [--rounds 7] [--reps 5] [--parent-tree DIR] [--out profiles/label_codec_time.txt]

One process, the routes of a section timed INTERLEAVED (``--rounds`` rounds, each round one sample of every route):
  host      the reference's lines restated in numpy (cityscapes.py:210-211, camvid.py:93-98), wall time per image and per batch of 16;
  encode    ``functional.label_encode`` alone, per launch in a graph of 50, device events, both forms (uint8 in, uint8 out): the bytes the
            launch moves (every input byte read once, every output byte written once) and their share of 8 TB/s;
  augment   ``BatchAugment.run`` at the README's Cityscapes shape (batch 16, 1024 x 2048 -> 768 x 768, bicubic), captured and replayed:
            (a) pre-encoded labels, (b) ``label_codec=``, (c) a ``label_encode`` launch in front of (a);
  evaluate  ``GraphedModel.evaluate``, prepared HyperSeg-M at 1024 x 512 with a 1024 x 2048 label, encoded against raw (table): the
            difference prices the encode launch that is not fused into the count.
Every device result is compared with ``LabelCodec.encode_cpu`` / the pre-encoded route first (asserted).  With ``--parent-tree`` (a
checkout of the parent commit, built): ``python bench.py --gpus 1 --steps 200 --warmup 20`` of that tree and of this one, fresh child
processes, alternating, ``--bench-rounds`` times each."""
import argparse
import os
import time

import numpy as np
import torch

from _measure import REPO, Lines, compare_bench, exceeds, graph_of, interleaved, per_launch, region_ms, report, require_gpu, write_report

HBM_BYTES_PER_S = 8e12
CITYSCAPES = [255, 255, 255, 255, 255, 255, 255, 0, 1, 255, 255, 2, 3, 4, 255, 255, 255, 5, 255, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 255, 255,
              16, 17, 18]
CAMVID = [(128, 128, 128), (128, 0, 0), (192, 192, 128), (128, 64, 128), (0, 0, 192), (128, 128, 0), (192, 128, 128), (64, 64, 128),
          (64, 0, 128), (64, 64, 0), (0, 128, 192), (0, 0, 0)]


def cityscapes_lines(target, table):
    target = np.array(target)
    target[np.bitwise_or(target < 0, target >= len(table))] = 0
    return table[target]


def camvid_lines(label_rgb, color_map):
    label_index = np.full(label_rgb.shape[:2], 255, dtype='uint8')
    for i, color in enumerate(color_map):
        label_index[np.all(label_rgb == color, axis=2)] = i
    return label_index


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--parent-tree', default=None)
    ap.add_argument('--bench-rounds', type=int, default=3)
    ap.add_argument('--skip-evaluate', action='store_true')
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'label_codec_time.txt'))
    args = ap.parse_args()
    require_gpu('label_codec_time.py')
    torch.set_num_threads(1)                                       # the host route is a loader thread's
    from hyperseg_amd import LabelCodec, configs, fps
    from hyperseg_amd import functional as HF
    from hyperseg_amd.training import BatchAugment
    from hyperseg_amd.utils.inference import GraphedModel, InputNorm, prepare_for_inference
    from hyperseg_amd.utils.synthetic import fill_by_name
    dev = torch.device('cuda:0')
    b, launches = 16, 50
    g = torch.Generator().manual_seed(1)
    table, colors = LabelCodec.table(CITYSCAPES), LabelCodec.colors(CAMVID)
    ids = torch.randint(0, 34, (b, 1024, 2048), generator=g, dtype=torch.uint8)
    rgb = torch.tensor(CAMVID, dtype=torch.uint8)[torch.randint(0, 12, (b, 720, 960), generator=g)].contiguous()
    rgb[..., 0][torch.rand(b, 720, 960, generator=g) < 0.02] ^= 1              # a few pixels of no class
    lines = Lines()
    lines.append(f'label encoding, batch {b}: Cityscapes id table on 2048x1024 uint8 labels, CamVid colour list (12) on 960x720 RGB labels; '
                 f'{args.rounds} interleaved rounds')

    # ---- host
    np_table, np_ids, np_rgb = np.array(CITYSCAPES, dtype='uint8'), ids.numpy(), rgb.numpy()
    host = {'Cityscapes lines, numpy, one image': [], 'Cityscapes lines, numpy, batch of 16': [], 'CamVid lines, numpy, one image': [],
            'CamVid lines, numpy, batch of 16': []}
    want_ids = np.stack([cityscapes_lines(x, np_table) for x in np_ids])
    want_rgb = np.stack([camvid_lines(x, CAMVID) for x in np_rgb])
    for _ in range(max(3, args.rounds // 2)):
        t0 = time.perf_counter()
        cityscapes_lines(np_ids[0], np_table)
        t1 = time.perf_counter()
        for x in np_ids:
            cityscapes_lines(x, np_table)
        t2 = time.perf_counter()
        camvid_lines(np_rgb[0], CAMVID)
        t3 = time.perf_counter()
        for x in np_rgb:
            camvid_lines(x, CAMVID)
        t4 = time.perf_counter()
        for k, v in zip(host, (t1 - t0, t2 - t1, t3 - t2, t4 - t3)):
            host[k].append(1e3 * v)
    report(lines, 'host route, ms WALL (one thread)', host)

    # ---- label_encode alone
    d_ids, d_rgb = ids.to(dev), rgb.to(dev)
    o_ids, o_rgb = torch.empty(b, 1024, 2048, dtype=torch.uint8, device=dev), torch.empty(b, 720, 960, dtype=torch.uint8, device=dev)
    same_t = torch.equal(HF.label_encode(d_ids, table, out=o_ids).cpu(), torch.from_numpy(want_ids)) and torch.equal(o_ids.cpu(), table.encode_cpu(ids))
    same_c = torch.equal(HF.label_encode(d_rgb, colors, out=o_rgb).cpu(), torch.from_numpy(want_rgb)) and torch.equal(o_rgb.cpu(), colors.encode_cpu(rgb))
    lines.append(f'label_encode equals the numpy lines and encode_cpu, byte for byte: table {same_t}, colours {same_c}')

    g_t = graph_of(lambda: HF.label_encode(d_ids, table, out=o_ids), launches, warm=1)
    g_c = graph_of(lambda: HF.label_encode(d_rgb, colors, out=o_rgb), launches, warm=1)
    enc = {f'label_encode table, per launch (graph of {launches}), device events': (per_launch(launches), g_t.replay, args.reps),
           f'label_encode colours, per launch (graph of {launches}), device events': (per_launch(launches), g_c.replay, args.reps)}
    med, _ = interleaved(lines, 'ms per launch, batch of 16', enc, args.rounds, warmup=0)
    for k, nbytes in zip(enc, (2 * ids.numel(), rgb.numel() + rgb.numel() // 3)):
        rate = nbytes / (med[k] * 1e-3)
        lines.append(f'  {k.split(",")[0]}: {nbytes / 1e6:.1f} MB moved (read once + written once; both fit the 256 MiB last-level cache '
                     f'across replays), {rate / 1e12:.3f} TB/s = {100 * rate / HBM_BYTES_PER_S:.1f} % of 8 TB/s')
    lines.append('  the colour form is not bound by memory but by its compare loop: per pixel up to n dependent LDS reads, each with a compare and '
                 'a branch, four pixels per thread one after the other, and a wave leaves the loop with its slowest lane')

    # ---- BatchAugment.run, three routes
    in_hw, crop, lo, hi_s = (1024, 2048), (768, 768), 0.375, 1.5
    norm = InputNorm(layout='hwc')
    frames = torch.randint(0, 256, (b,) + in_hw + (3,), generator=g, dtype=torch.uint8).to(dev)
    plain, coded = BatchAugment(in_hw, crop, norm, (lo, hi_s)), BatchAugment(in_hw, crop, norm, (lo, hi_s), label_codec=table)
    encoded = table.encode_cpu(ids).to(dev)
    scratch = torch.empty_like(encoded)
    scales = (lo + (hi_s - lo) * torch.rand(b, generator=g, dtype=torch.float64)).tolist()
    u = torch.rand(b, 3, generator=g, dtype=torch.float64).tolist()
    offsets = []
    for s, (uy, ux, _) in zip(scales, u):
        hr, wr = plain._resized(s)
        offsets.append((int(uy * (max(hr, crop[0]) - crop[0] + 1)), int(ux * (max(wr, crop[1]) - crop[1] + 1))))
    flips = [f[2] < 0.5 for f in u]
    want = plain(frames, encoded, scales, offsets, flips)
    got = coded(frames, d_ids, scales, offsets, flips)
    same_a = torch.equal(want[0], got[0]) and torch.equal(want[1], got[1])
    lines.append(f'BatchAugment(label_codec=) equals BatchAugment on pre-encoded labels, image and label, byte for byte: {same_a}')
    outs = [(torch.empty_like(want[0]), torch.empty_like(want[1])) for _ in range(3)]
    routes = {'(a) BatchAugment.run, pre-encoded labels, graph replay': lambda: plain.run(frames, encoded, out=outs[0]),
              '(b) BatchAugment.run(label_codec=), raw labels, graph replay': lambda: coded.run(frames, d_ids, out=outs[1]),
              '(c) label_encode launch + (a), graph replay': lambda: plain.run(frames, HF.label_encode(d_ids, table, out=scratch), out=outs[2])}
    med, spread = interleaved(lines, f'ms per batch of 16, {in_hw[1]}x{in_hw[0]} -> {crop[1]}x{crop[0]} bicubic, device events',
                              {k: (region_ms, graph_of(fn, 1, warm=3).replay, args.reps) for k, fn in routes.items()}, args.rounds, warmup=0)
    ka, kb, kc = routes
    diff, both = med[kb] - med[ka], spread[ka] + spread[kb]
    lines.append(f'  (b) - (a) = {diff:+.4f} ms, sum of the two spreads {both:.4f}: (b) ' +
                 ('EXCEEDS (a) by more than the sum of the two spreads (the codec staged into LDS per 256-pixel workgroup of the label gather)'
                  if exceeds(kb, ka, med, spread) else 'does NOT exceed (a) by more than the sum of the two spreads'))
    lines.append(f'  (c) - (b) = {med[kc] - med[kb]:+.4f} ms: what encoding inside the label gather saves over a launch in front')

    # ---- GraphedModel.evaluate
    same_e = True
    if not args.skip_evaluate:
        model = fill_by_name(configs.build('hyperseg-m').eval(), seed=0)
        prepare_for_inference(model, fold_bn=False, fused_depthwise=True)
        model = model.to(dev)
        size = tuple(configs.MODELS['hyperseg-m']['size'])
        x = torch.rand(1, 3, *size, generator=g).to(dev)
        t = torch.randint(0, 19, (1, 1024, 2048), generator=g)
        codec = fps.random_codec('table', 19)
        raw = fps.raw_labels(t, codec, g).to(dev)
        t8 = t.to(torch.uint8).to(dev)
        ev = {f'GraphedModel.evaluate, HyperSeg-M {size[1]}x{size[0]}, encoded 2048x1024 uint8 label, per replay': [],
              f'GraphedModel.evaluate, HyperSeg-M {size[1]}x{size[0]}, RAW 2048x1024 uint8 label (model.label_codec), per replay': []}
        served = GraphedModel(model, masks=True, num_classes=19)
        m0 = served.evaluate(x, t8).clone()
        torch.cuda.synchronize()
        c0 = served.confusion.clone()
        served.reset_confusion()
        model.label_codec = codec
        m1 = served.evaluate(x, raw).clone()
        torch.cuda.synchronize()
        same_e = torch.equal(m0, m1) and torch.equal(c0, served.confusion)
        lines.append(f'evaluate with the raw label: same masks and matrix as with the encoded one: {same_e}; graphs held: {len(served._graphs)}')
        for _ in range(args.rounds):
            model.label_codec = None
            ev[list(ev)[0]].append(region_ms(lambda: served.evaluate(x, t8), 4 * args.reps))
            model.label_codec = codec
            ev[list(ev)[1]].append(region_ms(lambda: served.evaluate(x, raw), 4 * args.reps))
        med, spread = report(lines, 'ms per frame (staging copies + replay), device events', ev)
        k0, k1 = ev
        lines.append(f'  raw - encoded = {med[k1] - med[k0]:+.4f} ms (sum of the two spreads {spread[k0] + spread[k1]:.4f}): the price of the encode '
                     'launch that is not fused into the count')

    bench_error = compare_bench(lines, args.parent_tree, args.bench_rounds)
    write_report(lines, args.out)
    assert same_t and same_c, 'label_encode disagrees with the reference lines'
    assert same_a, 'BatchAugment(label_codec=) disagrees with the pre-encoded route'
    assert same_e, 'evaluate with a raw label disagrees with the encoded one'
    if bench_error is not None:
        raise bench_error


if __name__ == '__main__':
    with torch.no_grad():
        main()
