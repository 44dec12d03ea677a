"""Does the FLOAT forward repeat itself bit for bit on this GPU, and if not, which module is the first whose output moves?

    timeout -k 10 600 python tools/float_repeatability.py [--runs 5] [--out profiles/float_repeatability.txt]

For HyperSeg-M / -S / CamVid-S / CamVid-L / L v0_1 prepared (fold_bn=False, fused_depthwise=True, split_gemm=True) and HyperSeg-M stock, at
batch 1 and 2, on one seeded float input: ``--runs`` forwards, the largest pairwise max |a - b| of the logits, of the encoder's features and of
the context head's output; then two traced forwards (a forward hook on every leaf module that runs as a module) and the first leaf whose
inputs are bit-equal between the two while its output is not.  Every line is printed once with PyTorch's defaults and once with
``torch.backends.cudnn.deterministic = True``.  tests/test_hip_ingest.py rests on what this file shows."""
import argparse
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

CASES = [('hyperseg-m', (256, 512), True), ('hyperseg-s', (256, 512), True), ('hyperseg-s-camvid', (192, 256), True),
         ('hyperseg-l-camvid', (384, 512), True), ('hyperseg-l', (256, 256), True), ('hyperseg-m', (256, 512), False)]


def tensors(o):
    if isinstance(o, torch.Tensor):
        return [o]
    if isinstance(o, (list, tuple)):
        return [t for e in o for t in tensors(e)]
    return []


def spread(runs):
    """largest max |a - b| over all pairs of runs (each run a list of tensors); nan: the runs hold no tensors (HyperSeg-L v0_1's head hands
    over bank references)"""
    if not runs[0]:
        return float('nan')
    worst = 0.0
    for i in range(len(runs)):
        for j in range(i + 1, len(runs)):
            for p, q in zip(runs[i], runs[j]):
                worst = max(worst, float((p.float() - q.float()).abs().max()))
    return worst


def trace(model, x):
    recs, hooks = [], []
    for name, mod in model.named_modules():
        if not list(mod.children()):
            def hook(m, i, o, name=name):
                recs.append((name, type(m).__name__, [t.detach().clone() for t in tensors(list(i))], [t.detach().clone() for t in tensors(o)]))
            hooks.append(mod.register_forward_hook(hook))
    try:
        model(x)
    finally:
        for h in hooks:
            h.remove()
    return recs


def first_moving_leaf(model, x):
    a, b = trace(model, x), trace(model, x)
    for (name, kind, ia, oa), (_, _, ib, ob) in zip(a, b):
        same_in = len(ia) == len(ib) and all(torch.equal(p, q) for p, q in zip(ia, ib))
        same_out = all(torch.equal(p, q) for p, q in zip(oa, ob))
        if same_in and not same_out:
            d = max(float((p.float() - q.float()).abs().max()) for p, q in zip(oa, ob))
            return f'{name} ({kind}, input {tuple(ia[0].shape) if ia else ()}, output {tuple(oa[0].shape)}): max |a - b| = {d:.3e}'
    return 'none (every leaf module with equal inputs gave equal outputs)'


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'float_repeatability.txt'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('float_repeatability.py measures on the GPU: no device found')
    from hyperseg_amd import configs
    from hyperseg_amd.utils.inference import prepare_for_inference
    from hyperseg_amd.utils.synthetic import fill_by_name
    dev = torch.device('cuda:0')
    lines = [f'float forward, {args.runs} runs of one input each; largest pairwise max |a - b|; {torch.cuda.get_device_name(0)}, torch {torch.__version__}']
    for name, (h, w), prepared in CASES:
        model = fill_by_name(configs.build(name).eval(), seed=11)
        if prepared:
            prepare_for_inference(model, fold_bn=False, fused_depthwise=True, split_gemm=True)
        model = model.to(dev)
        for b in (1, 2):
            x = torch.randn(b, 3, h, w, generator=torch.Generator().manual_seed(900 + h + b)).to(dev)
            for det in (False, True):
                torch.backends.cudnn.deterministic = det
                try:
                    logits = [[model(x)] for _ in range(args.runs)]
                    feats = [model.backbone(x) for _ in range(args.runs)]
                    heads = [tensors(model.weight_mapper(feats[0][-1])) for _ in range(args.runs)]
                    leaf = first_moving_leaf(model, x)
                finally:
                    torch.backends.cudnn.deterministic = False
                lines.append(f'{name:18s} {"prepared" if prepared else "stock   "} bs {b} cudnn.deterministic={str(det):5s}: logits {spread(logits):.3e}  '
                             f'encoder features {spread(feats):.3e}  context head (one input) {spread(heads):.3e}  first moving leaf: {leaf}')
                print(lines[-1], flush=True)
        del model
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    with torch.no_grad():
        main()
