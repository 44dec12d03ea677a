"""Generate tests/golden/weighted_loss.npz by IMPORTING THE REFERENCE's criterion with class weights:
``BootstrappedCrossEntropyLoss(k, thresh, weight, ignore_index)`` (hyperseg/losses/bootstrapped_ce_loss.py:8-40) on the CPU, forward and
``backward()``.

Run in the build container only (needs /root/reference; the reference never travels):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_weighted_loss_golden.py

The fixture is data: seeded inputs and what the reference made of them.
  case{i}_{logits,target,weight,k,thresh,ignore,loss,grad}: logits (N, C, H, W) f32 = randn * 4; int64 targets with ~20 % set to the
      ignore index (255, once -100); weights uniform in (0.4, 4.2) with ONE class at exactly 0 (CamVid's table has a 0 for Void); k below
      the pixel count; thresh 0.3, once 5.0 so that the ``[:k]`` branch runs; the reference's loss and the gradient of the logits.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, '/root/reference')

from hyperseg.losses.bootstrapped_ce_loss import BootstrappedCrossEntropyLoss          # noqa: E402

# ((N, C, H, W), k, thresh, ignore_index)
CASES = [((2, 12, 16, 24), 64, 0.3, 255), ((2, 19, 9, 11), 32, 5.0, 255), ((1, 21, 7, 13), 16, 0.3, 255), ((2, 5, 3, 70), 48, 0.3, -100)]


def main():
    out = {}
    for i, ((n, c, h, w), k, thresh, ignore) in enumerate(CASES):
        g = torch.Generator().manual_seed(5200 + i)
        logits = (torch.randn(n, c, h, w, generator=g) * 4).requires_grad_()
        target = torch.randint(0, c, (n, h, w), generator=g)
        target[torch.rand((n, h, w), generator=g) < 0.2] = ignore
        weight = torch.rand(c, generator=g) * 3.8 + 0.4
        weight[int(torch.randint(0, c, (1,), generator=g))] = 0.0
        assert h * w > k
        crit = BootstrappedCrossEntropyLoss(k=k, thresh=thresh, weight=weight, ignore_index=ignore)
        loss = crit(logits, target)
        loss.backward()
        for name, v in (('logits', logits.detach()), ('target', target), ('weight', weight), ('loss', loss.detach()), ('grad', logits.grad)):
            out[f'case{i}_{name}'] = v.numpy()
        out[f'case{i}_k'], out[f'case{i}_thresh'], out[f'case{i}_ignore'] = np.int64(k), np.float64(thresh), np.int64(ignore)
    out['cases'] = np.int64(len(CASES))
    path = os.path.join(HERE, 'weighted_loss.npz')
    np.savez_compressed(path, **out)
    print(f'weighted_loss: {os.path.getsize(path) / 1024:.1f} KiB')


if __name__ == '__main__':
    main()
