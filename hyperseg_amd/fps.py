"""FPS harness -- this build's counterpart of hyperseg/test_fps.py ("harness counterparts (i)").

Reproduces the reference's protocol on synthetic frames (no dataset, checkpoint or network exists here):
  * model from a config name (``hyperseg_amd.configs``) or an ``arch`` string through ``obj_factory`` (test_fps.py:139-144),
  * the optional BatchNorm -> identity switch (``remove_bn``, test_fps.py:147, 319-332) -- off by default, because it
    changes the logits; the reference applies it unconditionally when timing,
  * a warm-up pass followed by the timed pass (test_fps.py:163), per iteration
    ``synchronize -> perf_counter -> host-to-device copy of a pinned batch -> forward -> synchronize`` (:173-188),
    ``fps = frames / total_time`` (:190-191),
  * ``pred.argmax(1)`` masks feeding a confusion matrix (:194; hyperseg/utils/seg_utils.py:5-36) -> global accuracy, mIoU.
``torch.cuda.synchronize()`` is guarded so that the plumbing also runs on a CPU-only box (with a CPU-capable model).

    python -m hyperseg_amd.fps --config hyperseg-m --iterations 200 [--prepare] [--graph] [--remove-bn] [--batch-size 1]
                               [--confidence] [--uint8 [--layout hwc|chw] [--overlay] [--resize H W [--camera-size H W] [--overlay-at-camera]]] [--label-size H W] [--fused-metrics]
                               [--hflip [--pyramid N]]

``--hflip`` feeds every frame as a list (``--pyramid N``: N entries, the smaller ones ``F.avg_pool2d`` of the frame -- NOT ``cv2.pyrDown``) and
runs the reference's flip / pyramid loop, whose passes the device merges in one launch (``functional.tta_merge``); eager only.

``--label-size H W`` draws the targets at that size instead of the frame's: the reference's Cityscapes test configs resize the image
only, so every frame's logits are resized to the label before they are counted (test.py:167-168) -- done here as well, by the
forward's last launch with ``--fused-metrics``.

``--uint8`` feeds uint8 frames (what a decoder or camera delivers) to a model with the default ``InputNorm`` attached: the
host-to-device copy moves one byte per value and ToTensor + Normalize run on the device (``utils.inference.InputNorm``).

``--resize H W`` (with ``--uint8``) attaches ``FrameResize((H, W))``: the synthetic frames are made at ``--camera-size`` (default twice
H W) and resized on the device with ``PIL.Image.resize``'s bilinear arithmetic inside the timed region -- the reference's test configs
do that resize on a host thread before the loop (``utils.inference.FrameResize``).

``bench.py`` is the judged benchmark (resident input, HIP-graph replay); this harness includes the H2D copy and the
per-frame synchronisation exactly like the reference's, and by default its eager launches too, so its number is lower.
``--graph`` keeps the protocol but makes the forward one HIP-graph replay (``utils.inference.GraphedModel``)."""
import argparse
import json
import sys
import time

import torch
import torch.nn as nn


def _kernels():
    """``hyperseg_amd.functional`` when the HIP library is built and loads, else None (a CPU-only use of this module)."""
    try:
        from . import functional
        return functional
    except Exception:           # the library is missing or does not load: CUDA operands then take the stock route too
        return None


class ConfusionMatrix:
    """n x n counts of (target, prediction) pairs; targets outside [0, n) are ignored (seg_utils.py:5-36).  CUDA operands are
    counted by one launch of the package's kernel (``functional.confusion_update``: no device-to-host synchronisation, no
    temporaries, capturable in a HIP graph); CPU operands by the reference's stock ops (``update_stock``).  ``per_image``
    collects the (B, n, n) matrices of ``update_per_image`` / ``HyperGen.evaluate(..., per_image=True)`` calls."""

    def __init__(self, num_classes):
        self.num_classes = num_classes
        self.mat = None
        self.per_image = []

    def matrix(self, device):
        """``mat``, created on first use (as ``update`` always did)."""
        if self.mat is None:
            self.mat = torch.zeros((self.num_classes, self.num_classes), dtype=torch.int64, device=device)
        return self.mat

    @torch.no_grad()
    def update_stock(self, target, pred):
        """The reference's routine on stock torch ops, on whatever device the operands live (``target[valid]`` has a
        data-dependent shape: a device-to-host synchronisation on CUDA tensors)."""
        n = self.num_classes
        if self.mat is None:
            self.mat = torch.zeros((n, n), dtype=torch.int64, device=target.device)
        valid = (target >= 0) & (target < n)
        pairs = n * target[valid].to(torch.int64) + pred[valid].to(torch.int64)
        self.mat += torch.bincount(pairs, minlength=n * n).view(n, n)

    def _kernel_route(self, target, pred):
        if not (target.is_cuda and pred.is_cuda and target.shape == pred.shape and target.numel() > 0
                and target.dtype in (torch.uint8, torch.int64) and pred.dtype in (torch.uint8, torch.int64)):
            return None
        hf = _kernels()
        return hf if hf is not None and self.num_classes <= hf.eval_max_classes() else None

    @torch.no_grad()
    def update(self, target, pred):
        hf = self._kernel_route(target, pred)
        if hf is None:
            return self.update_stock(target, pred)
        hf.confusion_update(pred, target, self.num_classes, out=self.matrix(target.device))

    def add_per_image(self, mats):
        """Books a batch's (B, n, n) matrices: kept in ``per_image`` and summed into ``mat``."""
        self.per_image.append(mats)
        self.matrix(mats.device).add_(mats.sum(0))
        return mats

    @torch.no_grad()
    def update_per_image(self, target, pred):
        """``update`` on operands whose first dimension is the image: returns the batch's (B, n, n) matrices, appends them to
        ``per_image`` and adds their sum to ``mat`` (test.py:174-175 counts each image on its own for the Jaccard score)."""
        n, b = self.num_classes, target.shape[0]
        hf = self._kernel_route(target, pred)
        if hf is not None:
            mats = hf.confusion_update(pred, target, n, per_image=True)
        else:
            mats = torch.zeros((b, n, n), dtype=torch.int64, device=target.device)
            for i in range(b):
                one = ConfusionMatrix(n)
                one.update_stock(target[i].flatten(), pred[i].flatten())
                mats[i] = one.mat
        return self.add_per_image(mats)

    def per_image_matrices(self):
        """All booked per-image matrices as one (images, n, n) tensor."""
        n = self.num_classes
        return torch.cat(self.per_image) if self.per_image else torch.zeros((0, n, n), dtype=torch.int64)

    def reset(self):
        self.mat.zero_()
        self.per_image = []

    @torch.no_grad()
    def compute(self):
        """(global accuracy, per-class accuracy, per-class IoU) with the reference's 1e-6 guards."""
        h = self.mat.float()
        diag = torch.diag(h)
        rows, cols = h.sum(1), h.sum(0)
        return diag.sum() / h.sum(), diag / (rows + 1e-6), diag / (rows + cols - diag + 1e-6)

    def reduce_from_all_processes(self):
        """Sum ``mat`` over the process group (seg_utils.py:38-44): a no-op when torch.distributed is unavailable or not
        initialised, else barrier + all_reduce.  An n x n int64 matrix (2.9 KB at 19 classes) is all that multi-GPU evaluation
        has to move."""
        if not torch.distributed.is_available():
            return
        if not torch.distributed.is_initialized():
            return
        torch.distributed.barrier()
        torch.distributed.all_reduce(self.mat)


@torch.no_grad()
def jaccard_per_image(mats, ignore_index=0, eps=1e-6):
    """Per-image Jaccard score from per-image confusion matrices ``mats`` (images, n, n): what the reference computes with one
    ``.item()`` per image (hyperseg/test.py:219-227 on :210-216's matrix) -- rows of ``ignore_index`` dropped from the
    counts, its union zeroed, intersection / (union + eps) averaged over the classes whose union is positive (NaN for an
    image with none, as torch.mean of an empty tensor is).  test.py cannot be imported here (torchvision), so the tests pin
    this function against a restatement of those lines written out in the test itself."""
    mats = mats.clone()
    n = mats.shape[-1]
    if ignore_index is not None and 0 <= ignore_index < n:
        mats[:, ignore_index, :] = 0                     # calc_conf_mat masks those targets out (test.py:212-213)
    inter = torch.diagonal(mats, dim1=1, dim2=2)
    union = mats.sum(2) + mats.sum(1) - inter
    if ignore_index is not None and ignore_index < n:
        union[:, ignore_index] = 0
    score = inter / (union + eps)
    keep = union > 0
    return (score * keep).sum(1) / keep.sum(1)


def remove_bn(model):
    """Replace every BatchNorm module by the identity, recursively (test_fps.py:319-332).  The fused decoder kernels
    treat an emptied slot as scale 1 / shift 0."""
    for name, m in model.named_children():
        if isinstance(m, (nn.BatchNorm1d, nn.BatchNorm2d, nn.BatchNorm3d)):
            setattr(model, name, nn.Identity())
        else:
            remove_bn(m)
    return model


def _sync(device):
    if device.type == 'cuda':
        torch.cuda.synchronize(device)


@torch.no_grad()
def measure_fps(model, batches, device, num_classes, passes=2, fused_metrics=False, overlay=False, label_codec=None, confidence=False,
                overlay_size=None):
    """``batches``: list of (input, target) host tensors (inputs pinned when CUDA is used).  Runs ``passes`` passes over
    them and reports the LAST one (the reference's warm-up + timed pass).  Returns a dict.  ``fused_metrics``: where the
    model has ``evaluate`` (a HyperGen, a GraphedModel) the frame is scored by the forward's last launch -- INSIDE the timed
    region, which the reference's protocol keeps outside it; models without it are scored as before.  ``overlay``: every frame
    is served by ``model.overlay`` (masks + the uint8 display blended with ``overlay_style``) instead of the forward, inside the
    timed region; the masks are scored outside it as the reference's protocol does.  ``overlay_size`` (with ``overlay``): the display is
    served at that (H, W) -- the camera frame's, with ``input_resize`` set -- by ``model.overlay(x, size=overlay_size)``.  Targets of another size than the frame's are
    scored at their own resolution: the logits are resized to the label before the arg-max (test.py:167-168), outside the timed region
    on the unfused route; a model that returns masks hands them out at the label's size where its ``segment`` takes ``size=``.
    ``confidence``: every frame is served by ``model.confidence`` (masks + the confidence map in ``confidence_style``) instead of the
    forward, inside the timed region; the masks are scored outside it.
    ``label_codec`` (a ``LabelCodec``; the model's ``label_codec``): the targets are RAW dataset labels.  They are encoded where they are
    scored: by ``model.evaluate`` inside the timed region with ``fused_metrics``, outside it otherwise."""
    result = {}
    if overlay and fused_metrics:
        raise ValueError('overlay and fused_metrics both ride on the final upsample launch: one of them per run')
    if confidence and (overlay or fused_metrics):
        raise ValueError('confidence, overlay and fused_metrics all ride on the final upsample launch: one of them per run')
    fused = bool(fused_metrics) and hasattr(model, 'evaluate')
    owns = fused and getattr(model, 'owns_confusion', False)        # GraphedModel: the matrix lives with the graph
    for p in range(passes):
        conf = ConfusionMatrix(num_classes)
        if owns:
            model.reset_confusion()
        total_time, frames = 0.0, 0
        for inp, target in batches:
            target = target.to(device)
            _sync(device)
            t0 = time.perf_counter()
            if isinstance(inp, (list, tuple)):
                x = [t.to(device, non_blocking=True) for t in inp]
            elif getattr(model, 'accepts_host_input', False):
                x = inp                          # GraphedModel: the H2D copy lands in the graph's static input buffer
            else:
                x = inp.to(device, non_blocking=True)
            if fused:
                pred = model.evaluate(x, target) if owns else model.evaluate(x, target, conf)
            elif overlay:
                pred = model.overlay(x)[0] if overlay_size is None else model.overlay(x, size=overlay_size)[0]
            elif confidence:
                pred = model.confidence(x)[0]
            else:
                pred = model(x)
            _sync(device)
            total_time += time.perf_counter() - t0
            frames += pred.shape[0]
            if not fused:
                target = encode_labels(target, label_codec)
                if pred.dim() == 4 and pred.shape[2:] != target.shape[1:]:            # test.py:167-168
                    pred = _resize_logits(pred, tuple(target.shape[1:]))
                elif pred.dim() == 3 and pred.shape[1:] != target.shape[1:]:
                    pred = _masks_at(model, x, tuple(target.shape[1:]))
                conf.update(target.flatten(), pred.argmax(1).flatten() if pred.dim() == 4 else pred.flatten())
        if owns:
            conf.mat = model.confusion.clone()
        acc, _, iou = conf.compute()
        result = {'fps': frames / total_time, 'frames': frames, 'seconds': total_time, 'pass': p,
                  'global_accuracy': float(acc), 'mean_iou': float(iou.mean()),
                  'label_size': list(batches[-1][1].shape[1:3]) if batches else None}
    return result


def _resize_logits(pred, size):
    """``F.interpolate(pred, size, mode='bilinear')`` (test.py:167-168): the package's kernel for CUDA logits, ATen's on the CPU."""
    hf = _kernels() if pred.is_cuda else None
    if hf is not None and pred.dtype == torch.float32:
        return hf.upsample_bilinear(pred.contiguous(), size)
    return torch.nn.functional.interpolate(pred, size=size, mode='bilinear')


def _masks_at(model, x, size):
    """Masks at the label's size from a model whose forward returns masks at the frame's: its ``segment(x, size=...)`` (a
    GraphedModel's wrapped model's).  Masks themselves are never resized: the arg-max is taken after the logits' resize."""
    inner = getattr(model, 'model', model)
    p = next(inner.parameters(), None) if hasattr(inner, 'parameters') else None
    if p is not None:
        x = [t.to(p.device) for t in x] if isinstance(x, (list, tuple)) else x.to(p.device)
    try:
        return inner.segment(x, size=size)
    except (AttributeError, TypeError) as e:
        raise ValueError(f'the model returns masks at the frame\'s size and has no segment(x, size=...) to produce them at the '
                         f'label\'s {size}: score it with logits, or with targets of the frame\'s size') from e


def encode_labels(target, codec):
    """``target`` as class indices: raw labels of ``codec`` (None: nothing is raw) through ``functional.label_encode`` on the device,
    ``codec.encode_cpu`` on the CPU."""
    if codec is None or not codec.is_raw(target):
        return target
    return _kernels().label_encode(target.contiguous(), codec) if target.is_cuda else codec.encode_cpu(target)


def random_codec(kind, num_classes, seed=0):
    """A seeded synthetic ``LabelCodec`` whose inverse image covers every class 0..num_classes-1: ``'table'`` -- 2 n + 15 raw ids, every class
    at two of them and 255 at the rest, shuffled (Cityscapes' table has that form: 34 ids, 19 classes); ``'colors'`` -- n distinct random
    colours."""
    from .utils.labels import LabelCodec
    g = torch.Generator().manual_seed(seed)
    if kind == 'table':
        values = torch.tensor(list(range(num_classes)) * 2 + [255] * 15)
        return LabelCodec.table(values[torch.randperm(len(values), generator=g)].tolist())
    if kind != 'colors':
        raise ValueError(f"kind {kind!r}: expected 'table' or 'colors'")
    packed = torch.unique(torch.randint(0, 1 << 24, (4 * num_classes + 8,), generator=g))
    packed = packed[torch.randperm(len(packed), generator=g)][:num_classes]
    assert len(packed) == num_classes
    return LabelCodec.colors(torch.stack((packed & 255, packed >> 8 & 255, packed >> 16), 1).tolist())


def raw_labels(t, codec, generator):
    """Raw labels that ``codec`` encodes to the class indices ``t`` (int64 (B, H, W), every value one the codec produces): for a table a
    random raw id of the class per pixel, uint8; for a colour list the class's LAST colour, uint8 (B, H, W, 3)."""
    if codec.is_colors:
        last = {tuple(c): i for i, c in enumerate(codec.values)}
        palette = torch.zeros(256, 3, dtype=torch.uint8)
        for c, i in last.items():
            palette[i] = torch.tensor(c, dtype=torch.uint8)
        return palette[t]
    ids = [[i for i, v in enumerate(codec.values) if v == c] for c in range(256)]
    width = max(len(i) for i in ids)
    table = torch.tensor([i + [0] * (width - len(i)) for i in ids])
    count = torch.tensor([max(len(i), 1) for i in ids])
    pick = (torch.rand(t.shape, generator=generator, dtype=torch.float64) * count[t]).long().clamp_(max=width - 1)
    return table[t, torch.minimum(pick, count[t] - 1)].to(torch.uint8)


def synthetic_batches(n, batch_size, size, num_classes, device, seed=0, uint8=False, layout='hwc', label_size=None, label_codec=None):
    """``uint8``: uint8 frames in ``layout`` ('hwc': (B, H, W, 3), 'chw': (B, 3, H, W)) from the same generator seed instead of
    float32 (B, 3, H, W) images.  ``label_size``: (H, W) of the targets where it is not the frames' (None: the frames').
    ``label_codec``: the same targets as RAW labels of that codec (:func:`raw_labels`)."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n):
        if uint8:
            shape = (batch_size,) + tuple(size) + (3,) if layout == 'hwc' else (batch_size, 3) + tuple(size)
            x = torch.randint(0, 256, shape, generator=g, dtype=torch.uint8)
        else:
            x = torch.rand(batch_size, 3, *size, generator=g)
        t = torch.randint(0, num_classes, (batch_size,) + tuple(size if label_size is None else label_size), generator=g)
        if label_codec is not None:
            t = raw_labels(t, label_codec, g)
        out.append((x.pin_memory() if device.type == 'cuda' else x, t))
    return out


def pyramid_of(x, entries, device):
    """The list input of ``--hflip`` / ``--pyramid``: ``[x, avg_pool2d(x, 2), avg_pool2d(x, 4), ...]``, ``entries`` long, pinned like ``x``
    (a synthetic pyramid: NOT cv2.pyrDown's 5 x 5 Gaussian)."""
    out = [x]
    for k in range(1, entries):
        y = torch.nn.functional.avg_pool2d(x, 2 ** k).contiguous()
        out.append(y.pin_memory() if device.type == 'cuda' else y)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--config', default='hyperseg-m', help='a name from hyperseg_amd.configs.MODELS')
    ap.add_argument('--arch', default=None, help='an obj_factory arch string instead of --config (reference checkpoints store one)')
    ap.add_argument('--iterations', type=int, default=100)
    ap.add_argument('--distinct', type=int, default=8, help='distinct synthetic batches cycled through')
    ap.add_argument('--batch-size', type=int, default=None)
    ap.add_argument('--remove-bn', action='store_true', help="the reference's BN -> identity switch (changes the logits)")
    ap.add_argument('--prepare', action='store_true', help='hyperseg_amd.utils.inference.prepare_for_inference (fused encoder)')
    ap.add_argument('--graph', action='store_true', help='replay one HIP graph per frame (utils.inference.GraphedModel) '
                                                         'instead of launching eagerly; same protocol otherwise')
    ap.add_argument('--fused-metrics', action='store_true',
                    help="score every frame inside the forward's last launch (model.evaluate): the scoring then falls INSIDE the timed "
                         "region, which the reference's protocol keeps outside it")
    ap.add_argument('--uint8', action='store_true',
                    help='uint8 frames with the default InputNorm attached to the model: normalised on the device, a quarter of the '
                         'bytes over the host link')
    ap.add_argument('--layout', choices=('hwc', 'chw'), default='hwc', help='layout of the --uint8 frames')
    ap.add_argument('--overlay', action='store_true',
                    help="serve the display as well (model.overlay): the class map coloured with a seeded synthetic palette and alpha-blended "
                         "over the uint8 frame by the forward's last launch, inside the timed region; needs --uint8")
    ap.add_argument('--overlay-at-camera', action='store_true',
                    help="on top of --uint8 --overlay --resize H W: serve masks and overlay at --camera-size, blended over the camera frame "
                         "itself (model.overlay(x, size=camera size)): both resizes of the logits and the blend in the forward's last launch")
    ap.add_argument('--confidence', action='store_true',
                    help="serve the confidence map as well (model.confidence): beside the masks, every pixel's soft-max probability of its "
                         "class as uint8, from the forward's last launch, inside the timed region")
    ap.add_argument('--label-size', nargs=2, type=int, metavar=('H', 'W'), default=None,
                    help="draw the targets at this size instead of the frame's: the logits are resized to it before they are counted "
                         "(test.py:167-168; the reference's Cityscapes test configs: 1024 2048)")
    ap.add_argument('--raw-labels', choices=('table', 'colors'), default=None,
                    help="the targets are RAW dataset labels -- ids (Cityscapes' form) or a colour image (CamVid's) drawn through a seeded "
                         "random LabelCodec whose inverse image covers every class -- and model.label_codec encodes them on the device, "
                         "where they are scored: inside the timed region with --fused-metrics, outside it otherwise")
    ap.add_argument('--resize', nargs=2, type=int, metavar=('H', 'W'), default=None,
                    help="on top of --uint8: attach FrameResize((H, W)) (model.input_resize) -- the synthetic frames are made at "
                         "--camera-size and resized on the device with PIL.Image.resize's bilinear arithmetic, inside the timed region "
                         "(the reference's Cityscapes test configs: Resize([512, 1024]) of the 1024 x 2048 frame, on a host thread)")
    ap.add_argument('--camera-size', nargs=2, type=int, metavar=('H', 'W'), default=None,
                    help='size of the synthetic camera frames with --resize (default: twice --resize)')
    ap.add_argument('-t', '--trace', action='store_true',
                    help="the reference's torch.jit.trace switch (test_fps.py:49-50, 150-152).  The mirror's modules call the C ABI through "
                         "ctypes, which the tracer cannot see, so a traced module would be wrong; the purpose of tracing there -- no Python / "
                         "dispatcher cost per frame -- is served by one HIP-graph replay per frame: --trace selects --graph")
    ap.add_argument('--gpus', nargs='+', type=int, metavar='N', default=None,
                    help='GPU ids (test_fps.py:31-32): more than one wraps the model in nn.DataParallel exactly as the reference does '
                         '(test_fps.py:155-156; one Python thread per replica -- the mirror is re-entrant for that); the first id is the primary device')
    ap.add_argument('--hflip', action='store_true',
                    help="the reference's accuracy mode (hyperseg_v1_0.py:71-91): every frame goes in as a LIST -- one entry, or --pyramid N "
                         "entries -- and is run plain and mirrored (inference_hflip); on the device the passes are merged in one launch "
                         "(functional.tta_merge).  Eager only: a list is never replayed from a graph")
    ap.add_argument('--pyramid', type=int, metavar='N', default=None,
                    help='with or without --hflip: a list of N entries per frame, entry k the frame average-pooled by 2^k '
                         '(F.avg_pool2d: a synthetic stand-in that does NOT reproduce cv2.pyrDown, which seg_transforms.Pyramids uses; '
                         'OpenCV is not a dependency, building the pyramid on the device is out of scope)')
    ap.add_argument('--cpu-only', '--cpu_only', dest='cpu_only', action='store_true')
    args = ap.parse_args(argv)
    lists = args.hflip or args.pyramid is not None
    if args.pyramid is not None and args.pyramid < 1:
        raise SystemExit('--pyramid N: a positive number of entries')
    if lists and (args.uint8 or args.overlay or args.confidence or args.resize is not None):
        raise SystemExit('--hflip / --pyramid feed float lists: not with --uint8, --overlay, --confidence or --resize')
    if args.trace:
        args.graph = True
    if args.overlay and not args.uint8:
        raise SystemExit('--overlay blends over the uint8 frames: it needs --uint8')
    if args.overlay_at_camera and (not args.overlay or args.resize is None):
        raise SystemExit('--overlay-at-camera serves the overlay at the camera frame\'s size: it needs --overlay and --resize H W')
    if args.overlay and args.fused_metrics:
        raise SystemExit('--overlay and --fused-metrics both ride on the final upsample launch: one of them per run')
    if args.confidence and (args.overlay or args.fused_metrics):
        raise SystemExit('--confidence, --overlay and --fused-metrics all ride on the final upsample launch: one of them per run')
    if args.confidence and args.gpus and len(args.gpus) > 1:
        raise SystemExit('--confidence serves one device: with several --gpus run one process per GPU')
    if args.label_size is not None and min(args.label_size) <= 0:
        raise SystemExit('--label-size H W: two positive integers')
    if args.resize is not None and not args.uint8:
        raise SystemExit('--resize resizes uint8 frames: it needs --uint8')
    if args.resize is not None and min(args.resize) <= 0 or args.camera_size is not None and (args.resize is None or min(args.camera_size) <= 0):
        raise SystemExit('--resize H W [--camera-size H W]: positive integers, --camera-size only with --resize')
    if args.overlay and args.gpus and len(args.gpus) > 1:
        raise SystemExit('--overlay serves one device: with several --gpus run one process per GPU')

    from . import configs
    from .utils.synthetic import fill_by_name
    device = torch.device('cpu' if args.cpu_only or not torch.cuda.is_available() else f'cuda:{args.gpus[0] if args.gpus else 0}')
    spec = configs.MODELS[args.config]
    if args.arch:
        from .utils.obj_factory import obj_factory
        model = obj_factory(args.arch)
    else:
        model = configs.build(args.config)
    model = fill_by_name(model.eval(), seed=0)              # synthetic, non-denormal weights (no checkpoint offline)
    if args.remove_bn:
        remove_bn(model)
    elif args.prepare:
        from .utils.inference import prepare_for_inference
        prepare_for_inference(model, fold_bn=False, fused_depthwise=True)
    if args.uint8:
        from .utils.inference import InputNorm
        model.input_norm = InputNorm(layout=args.layout)
    frame_size, label_size = tuple(spec['size']), args.label_size
    if args.resize is not None:
        from .utils.inference import FrameResize
        model.input_resize = FrameResize(args.resize, 'bilinear', args.layout)
        frame_size = tuple(args.camera_size) if args.camera_size is not None else (2 * args.resize[0], 2 * args.resize[1])
        label_size = tuple(args.resize) if label_size is None else label_size       # the masks come at the resized frame's size
        if args.overlay_at_camera and args.label_size is None:
            label_size = frame_size                                                   # ... or, served at the camera's size, at that
    if args.overlay:
        from .utils.inference import Overlay
        palette = torch.randint(0, 256, (spec['num_classes'], 3), generator=torch.Generator().manual_seed(0))
        model.overlay_style = Overlay(palette, layout=args.layout)
        model.inference_hflip = False        # inert for tensor inputs, but overlay() takes its segment() + blend route while it is set
    if args.confidence:
        from .utils.confidence import Confidence
        model.confidence_style = Confidence()
        model.inference_hflip = False        # inert for tensor inputs, but confidence() takes its composed route while it is set
    if lists:
        model.inference_hflip = bool(args.hflip)
        if args.graph:
            print('--hflip / --pyramid: list inputs are served eagerly (a GraphedModel hands them to the wrapped model); running eager',
                  file=sys.stderr)
            args.graph = False
    codec = None if args.raw_labels is None else random_codec(args.raw_labels, spec['num_classes'])
    if codec is not None:
        model.label_codec = codec
    model = model.to(device)
    if args.gpus and len(args.gpus) > 1 and device.type == 'cuda':
        if args.graph:
            raise SystemExit('--graph / --trace replay a captured graph on ONE device: with several --gpus use bench.py --gpus N (one process per GPU)')
        model = torch.nn.DataParallel(model, args.gpus)
    if args.graph and device.type == 'cuda':
        from .utils.inference import GraphedModel
        model = GraphedModel(model, num_classes=spec['num_classes'] if args.fused_metrics else None)
    bs = args.batch_size or spec['batch']
    uniq = synthetic_batches(min(args.distinct, args.iterations), bs, frame_size, spec['num_classes'], device,
                             uint8=args.uint8, layout=args.layout, label_size=label_size, label_codec=codec)
    if lists:
        uniq = [(pyramid_of(x, args.pyramid or 1, device), t) for x, t in uniq]
    batches = [uniq[i % len(uniq)] for i in range(args.iterations)]
    res = measure_fps(model, batches, device, spec['num_classes'], fused_metrics=args.fused_metrics, overlay=args.overlay, label_codec=codec,
                      confidence=args.confidence, overlay_size=frame_size if args.overlay_at_camera else None)
    frame = uniq[0][0][0] if lists else uniq[0][0]
    if lists:
        from . import functional as HF
        res.update(hflip=bool(args.hflip), pyramid=args.pyramid or 1, 
                   tta_merge=bool(HF.TTA_MERGE and device.type == 'cuda'            # the route the model takes for these lists
                                  and (args.pyramid or 1) * (2 if args.hflip else 1) <= HF.TTA_MAX_PASSES))
    res.update(input_dtype=str(frame.dtype).replace('torch.', ''), input_bytes_per_frame=frame[0].numel() * frame.element_size())
    res.update(config=args.config, batch_size=bs, size=list(spec['size']), device=str(device), remove_bn=args.remove_bn,
               prepared=bool(args.prepare and not args.remove_bn), graph=bool(args.graph and device.type == 'cuda'),
               protocol='test_fps.py: per-iteration sync + H2D + ' + ('HIP-graph replay' if args.graph else 'eager forward'))
    if args.resize is not None:
        res.update(resize=list(args.resize), camera_size=list(frame_size), size=list(args.resize),
                   protocol=res['protocol'] + ' + camera frame resized on the device inside the timed region')
    if args.fused_metrics:
        res.update(fused_metrics=True, protocol=res['protocol'] + ' + confusion matrix counted inside the timed region by the '
                   "forward's last launch (the reference scores outside it)")
    if codec is not None:
        res.update(raw_labels=args.raw_labels, protocol=res['protocol'] + f' + raw {args.raw_labels} labels encoded on the device where they are scored')
    if args.overlay:
        res.update(overlay=True, protocol=res['protocol'] + " + uint8 overlay blended inside the timed region by the forward's last launch")
    if args.overlay_at_camera:
        res.update(overlay_size=list(frame_size), protocol=res['protocol'] + " at the camera frame's size, over the camera frame")
    if args.confidence:
        res.update(confidence=True, protocol=res['protocol'] + " + uint8 confidence map made inside the timed region by the forward's last launch")
    print(json.dumps(res))
    return res


if __name__ == '__main__':
    main()
