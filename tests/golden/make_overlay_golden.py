"""Generate tests/golden/overlay_ref.npz by IMPORTING THE REFERENCE's display chain: ``tensor2rgb(blend_seg(img, seg, color_map, alpha,
ignore_index))`` (hyperseg/utils/seg_utils.py:82-103, hyperseg/utils/img_utils.py:62-75) on frames normalised with mean = std = 0.5.

Run in the build container only (needs /root/reference; the reference never travels):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_overlay_golden.py

The fixture is data: seeded uint8 frames, uint8 class maps, RANDOM palettes (nothing of the reference's dataset files) and the uint8 images
the reference made of them.
  sweep_a{30,50,75}: (256, 256) uint8, entry [v][c] = the output byte for frame byte v under grey colour c at alpha 0.3 / 0.5 / 0.75
  case{i}_{frames,classes,palette,alpha,ignore,expected}: small random cases -- frames (B, H, W, 3), classes (B, H, W) with values at and
      beyond the palette's length, palettes of 2, 12, 19, 21 and 256 colours, ignore_index 0 / a middle class / -1.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, '/root/reference')
# img_utils imports torchvision at module level; tensor2rgb and blend_seg use none of it
for name in ('torchvision', 'torchvision.utils', 'torchvision.transforms', 'torchvision.transforms.functional'):
    sys.modules.setdefault(name, types.ModuleType(name))
sys.modules['torchvision'].utils = sys.modules['torchvision.utils']
sys.modules['torchvision'].transforms = sys.modules['torchvision.transforms']
sys.modules['torchvision.transforms'].functional = sys.modules['torchvision.transforms.functional']

from hyperseg.utils.seg_utils import blend_seg          # noqa: E402
from hyperseg.utils.img_utils import tensor2rgb         # noqa: E402

torch.set_grad_enabled(False)

SWEEP_ALPHAS = {'a30': 0.3, 'a50': 0.5, 'a75': 0.75}
# (colours, ignore_index, alpha, B, H, W)
CASES = [(2, 0, 0.75, 1, 8, 12), (2, -1, 0.5, 2, 5, 7), (12, 0, 0.75, 1, 48, 64), (12, 6, 0.3, 2, 9, 13), (19, 0, 0.75, 1, 32, 64),
         (19, -1, 0.6, 1, 17, 31), (19, 9, 1.0, 1, 6, 10), (21, 0, 0.75, 2, 24, 32), (21, 10, 0.0, 1, 7, 9), (256, 0, 0.75, 1, 48, 64),
         (256, 128, 0.5, 1, 16, 21), (256, -1, 0.3, 2, 11, 16)]


def reference_overlay(frames_hwc, classes, palette, alpha, ignore):
    """frames (B, H, W, 3) uint8, classes (B, H, W) uint8 -> (B, H, W, 3) uint8, through the reference."""
    img = frames_hwc.permute(0, 3, 1, 2).to(torch.float32).div(255).sub_(0.5).div_(0.5)           # rgb2tensor's to_tensor + normalize
    blended = blend_seg(img, classes.long(), palette.numpy(), alpha=alpha, ignore_index=ignore)
    return torch.from_numpy(np.stack([tensor2rgb(b) for b in blended]))


def main():
    out = {}
    v = torch.arange(256, dtype=torch.uint8)
    frames = v[:, None, None].expand(256, 256, 3)[None].contiguous()                               # pixel [v][c] = (v, v, v)
    classes = v[None, :].expand(256, 256)[None].contiguous()                                       # ... of class c
    greys = v.long()[:, None].expand(256, 3).contiguous()
    for tag, alpha in SWEEP_ALPHAS.items():
        got = reference_overlay(frames, classes, greys, alpha, -1)[0]
        assert bool((got[..., 0] == got[..., 1]).all()) and bool((got[..., 0] == got[..., 2]).all())
        out[f'sweep_{tag}'] = got[..., 0].numpy()
    for i, (n, ignore, alpha, b, h, w) in enumerate(CASES):
        g = torch.Generator().manual_seed(4100 + i)
        fr = torch.randint(0, 256, (b, h, w, 3), generator=g, dtype=torch.uint8)
        cl = torch.randint(0, n, (b, h, w), generator=g).to(torch.uint8)
        if n < 256:                                                                                # classes the palette does not cover
            beyond = torch.rand((b, h, w), generator=g) < 0.15
            cl[beyond] = torch.randint(n, 256, (int(beyond.sum()),), generator=g).to(torch.uint8)
            cl.view(-1)[0], cl.view(-1)[-1] = n, 255
        pal = torch.randint(0, 256, (n, 3), generator=g)
        out[f'case{i}_frames'], out[f'case{i}_classes'], out[f'case{i}_palette'] = fr.numpy(), cl.numpy(), pal.to(torch.uint8).numpy()
        out[f'case{i}_alpha'], out[f'case{i}_ignore'] = np.float64(alpha), np.int64(ignore)
        out[f'case{i}_expected'] = reference_overlay(fr, cl, pal, alpha, ignore).numpy()
    out['cases'] = np.int64(len(CASES))
    path = os.path.join(HERE, 'overlay_ref.npz')
    np.savez_compressed(path, **out)
    print(f'overlay_ref: {os.path.getsize(path) / 1024:.1f} KiB')


if __name__ == '__main__':
    main()
