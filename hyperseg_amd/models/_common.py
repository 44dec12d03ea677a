"""Pieces shared by the three HyperSeg model variants of this package (v1_0, v1_0_unify, v0_1): the HyperGen wrapper
logic (single tensor / pyramid + h-flip inference), per-level argument normalisation, coordinate buffers."""
import numbers
from dataclasses import dataclass
from typing import NamedTuple, Optional

import torch
import torch.nn as nn

from .. import functional as HF


def per_level(value, n, name):
    """Broadcast a scalar hyper-parameter to ``n`` levels, or check a sequence's length."""
    if isinstance(value, numbers.Number):
        return (value,) * n
    if len(value) != n:
        raise AssertionError(f'{name} ({len(value)}) must be of size {n}')
    return tuple(value)


def plan_levels(feat_channels, level_channels, kernel_sizes, level_layers, expand_ratio, groups, num_classes,
                with_out_fc):
    """Channel bookkeeping of a v1_0-style decoder, separated from module construction: for every level (coarse -> fine)
    the list of its layers as dicts ``{cin, cout, k, expand, groups}``.  Rules (hyperseg_v1_0.py:139-163): a level's first
    layer sees everything carried up from the coarser level plus this level's skip feature plus two coordinate channels;
    a level emits ``level_channels[l]`` (or its skip width) channels, except that the very last layer of the decoder emits
    the class logits unless a separate output layer follows."""
    skips = list(feat_channels)[::-1]
    n = len(skips) if level_channels is None else len(level_channels)
    plan, carried = [], 0
    for lvl in range(n):
        width = skips[lvl] if level_channels is None else level_channels[lvl]
        carried += skips[lvl]
        layers = []
        for j in range(level_layers[lvl]):
            last_of_decoder = lvl == n - 1 and j == level_layers[lvl] - 1
            cout = num_classes if (last_of_decoder and not with_out_fc) else width
            layers.append(dict(cin=carried + 2, cout=cout, k=kernel_sizes[lvl], expand=expand_ratio[lvl],
                               groups=groups[lvl] if isinstance(groups, (list, tuple)) else groups))
            carried = cout
        plan.append(layers)
    return plan, carried


def coordinate_grid(h, w, device=None):
    """(1, 2, h, w): channel 0 = x in [-1, 1] over W, channel 1 = y over H, endpoints inclusive.  Same values as the
    reference's cached buffers; the HIP kernels regenerate them analytically."""
    xs = torch.linspace(-1, 1, steps=w, device=device).view(1, w).expand(h, w)
    ys = torch.linspace(-1, 1, steps=h, device=device).view(h, 1).expand(h, w)
    return torch.stack([xs, ys], dim=0).unsqueeze(0).contiguous()


def register_coordinate_buffers(module, coords_res, levels):
    """``coord{h}_{w}`` buffers for every resolution of every listed pyramid -- kept only so that reference checkpoints
    load with strict=True."""
    for res in coords_res or ():
        for i in range(levels):
            h, w = res[0] // 2 ** i, res[1] // 2 ** i
            module.register_buffer(f'coord{h}_{w}', coordinate_grid(h, w))


class Score(NamedTuple):
    """Count every output pixel against ``target`` (B, H, W; uint8 or int64) into the int64 matrix ``out`` -- (n, n), or (B, n, n) with
    ``per_image``; ``num_classes`` None: nothing is counted (a validation step that only wants loss and masks)."""
    target: object
    num_classes: object
    out: object
    per_image: bool


class Blend(NamedTuple):
    """Colour the class map with ``style`` (a ``utils.inference.Overlay``) and blend it over the uint8 ``frames`` into ``out`` (None: a new
    tensor).  ``size``: the (H, W) of ``frames`` where that is another size than the model's frame (a camera frame the model sees
    down-scaled): the logits are resized to it before the arg-max (test.py:167-168), masks and overlay are then at ``size``.  None: the
    model's frame size."""
    frames: object
    style: object
    out: object
    size: object = None


class Deferred(NamedTuple):
    """What a decoder returns for ``Epilogue(defer=True)``: ``x``, the input of its final resize (contiguous f32 (B, C, Hi, Wi)), and
    ``size``, the frame's (H, W) the resize would have gone to -- the launch is left to ``HF.tta_merge``."""
    x: object
    size: tuple


@dataclass
class Epilogue:
    """What rides on the decoder's final upsample launch instead of writing the logits: the uint8 arg-max masks, plain -- at the frame's
    size, or resized once more to ``out_size`` -- or scored by that launch (``score``) or blended over the frames by it (``blend``): one of
    the two per forward.  ``ignore_index`` (with ``score``): the criterion's -- a validation step, the launch also makes every pixel's
    cross entropy against the score's target.  ``weight`` (with ``ignore_index`` and ``score``): the criterion's class-weight table, fp32
    (C,) on the device, finite and >= 0 -- the losses are then the weighted ones.  A scored forward takes its output size from its target.
    ``loss_at_label`` (with ``ignore_index``; off by default): a target of another size than the frame's is then taken at ITS resolution by
    the validation step too, as train.py:119-120 does -- losses, masks and counts at the label's size from the one launch; without it such
    a target is rejected where a loss is asked for.  ``confidence`` (a ``utils.confidence.Confidence``): the launch also makes every
    pixel's confidence -- the soft-max probability of its class -- in the style's dtype, and fills the masks below the style's threshold;
    it goes with ``out_size``, not with ``score`` or ``blend``.  ``defer`` (with nothing else): the last launch is not made at all -- the
    decoder returns a :class:`Deferred`, the input of its final resize and the frame's size, for the one launch that merges the passes of a
    list input (``HF.tta_merge``); the only epilogue a flipped pass takes."""
    score: Optional[Score] = None
    blend: Optional[Blend] = None
    confidence: Optional[object] = None
    out_size: Optional[tuple] = None
    ignore_index: Optional[int] = None
    weight: Optional[object] = None
    loss_at_label: bool = False
    defer: bool = False

    def __post_init__(self):
        if self.defer and (self.score is not None or self.blend is not None or self.confidence is not None or self.out_size is not None
                           or self.ignore_index is not None or self.weight is not None or self.loss_at_label):
            raise ValueError('a deferred last launch makes nothing: defer goes with no other epilogue field')
        if self.ignore_index is not None and (self.score is None or self.blend is not None):
            raise ValueError('the loss rides on a scored epilogue: a score with it, no blend')
        if self.weight is not None and (self.ignore_index is None or self.score is None):
            raise ValueError('class weights weigh the loss: they ride on a scored epilogue with an ignore_index')
        if self.loss_at_label and self.ignore_index is None:
            raise ValueError('loss_at_label places the loss: it rides on a scored epilogue with an ignore_index')
        if self.score is not None and self.blend is not None:
            raise ValueError('score and blend both ride on the final upsample launch: one of them per forward for now')
        if self.confidence is not None and (self.score is not None or self.blend is not None):
            raise ValueError('confidence and score / blend all ride on the final upsample launch: one of them per forward for now')
        if self.out_size is not None:
            self.out_size = tuple(self.out_size)

    def apply(self, p, size):
        """The last level's output ``p`` -> the masks at ``size`` (the frame's), straight from the one launch; ``(masks, per_pixel)`` of a
        validation step (per_pixel: f32 (B, H, W), what ``BootstrappedCrossEntropyLoss`` ranks), ``(masks, overlay)`` of a blend (at the blend's
        ``size`` where it names another one: ``HF.upsample2_overlay``, both resizes composed; ``HF.upsample_overlay`` straight to it where ``p``
        is at the frame's size already), ``(masks, conf)`` of a
        confidence epilogue (at ``out_size`` where one is given, both resizes composed in the one launch).  A
        score's target of another size than ``size`` is scored at ITS resolution, as test.py:167-168 does: the logits at ``size`` are
        resized once more, to the target's size, before the arg-max -- both resizes composed in the one launch, a single one where ``p``
        is at ``size`` already; the masks are then at the target's size.  A validation step takes such a target only with
        ``loss_at_label`` set: the logits at ``size`` are resized to the target before the criterion as well (train.py:119-120), by
        ``HF.upsample2_ce_confusion`` -- ``HF.upsample_ce_confusion`` straight to the target's size where ``p`` is at ``size`` already -- and
        ``per_pixel`` is at the target's size too."""
        size = tuple(int(v) for v in size)
        if self.defer:
            return Deferred(p.contiguous(), size)
        resized = self.out_size is not None and self.out_size != size
        if self.score is not None:
            target, num_classes, out, per_image = self.score
            label = tuple(target.shape[1:])
            if self.ignore_index is not None:
                if resized:
                    raise ValueError('the loss rides on a scored epilogue at the frame\'s size: no other out_size')
                if label != size and not self.loss_at_label:
                    raise ValueError(f'the loss needs a target at the output size {size}, got {label}')
                weighted = {} if self.weight is None else dict(weight=self.weight)          # (the unweighted call is what it was)
                if label != size and tuple(p.shape[2:]) != size:
                    per_pixel, _, masks = HF.upsample2_ce_confusion(p, size, target, self.ignore_index, num_classes, out=out,
                                                                    per_image=per_image, **weighted)
                else:                                                   # (a target at the frame's size: label == size)
                    per_pixel, _, masks = HF.upsample_ce_confusion(p, label, target, self.ignore_index, num_classes, out=out,
                                                                   per_image=per_image, **weighted)
                return masks, per_pixel
            if label != size and tuple(p.shape[2:]) != size:
                return HF.upsample2_confusion(p, size, target, num_classes, out=out, per_image=per_image, masks=True)[1]
            return HF.upsample_confusion(p, label, target, num_classes, out=out, per_image=per_image, masks=True)[1]
        if self.blend is not None:
            if resized:
                raise ValueError('the overlay is blended over the frames, at their size: another out_size does not go with a blend')
            frames, style, out, at = self.blend
            at = size if at is None else tuple(int(v) for v in at)
            if at == size:
                return HF.upsample_overlay(p, size, frames, style, out=out)
            if tuple(p.shape[2:]) == size:                          # (no final resize to compose with: one stage, straight to the frames)
                return HF.upsample_overlay(p, at, frames, style, out=out)
            return HF.upsample2_overlay(p, size, at, frames, style, out=out)
        if self.confidence is not None:
            style = self.confidence
            if not resized:
                return HF.upsample_confidence(p, size, style.dtype, style.threshold, style.fill)
            return HF.upsample2_confidence(p, size, self.out_size, style.dtype, style.threshold, style.fill)
        if not resized:
            return HF.upsample_argmax(p, size)
        return HF.upsample2_argmax(p, size, self.out_size)


def finish_decoder(decoder, p, size, epilogue):
    """What the v1_0 and unify decoders return for their last level's output ``p``: what ``epilogue`` makes of it (:class:`Epilogue`), or,
    without one, the logits, resized to ``size`` -- into ``decoder.output_buffer`` where a serving wrapper has set one."""
    if epilogue is not None:
        return epilogue.apply(p, size)
    if p.shape[2:] != size:
        p = HF.upsample_bilinear(p, size, out=getattr(decoder, 'output_buffer', None))
    return p


class EpochOnModeSwitch:
    """Mixin (before nn.Module in the bases): every train() / eval() switch invalidates the parameter-derived caches of the
    inference route (functional.bump_weights_epoch) -- training steps change parameters and BatchNorm statistics through
    paths that do not bump tensor versions (graph replays, raw-pointer kernels)."""

    def train(self, mode=True):
        HF.bump_weights_epoch()
        return super().train(mode)


class HyperGenBase(EpochOnModeSwitch, nn.Module):
    """backbone -> context head -> dynamic decoder, with the reference's list-input (image pyramid) and horizontal-flip
    inference modes (hyperseg_v1_0.py:52-91).  Subclasses create ``backbone``, ``decoder`` and ``weight_mapper``."""

    inference_hflip = False
    inference_gather = 'mean'
    # a utils.inference.InputNorm: uint8 frames are then accepted and normalised on the device.  A plain attribute -- no parameter,
    # no buffer: state_dict() and strict loading of reference checkpoints are as they were
    input_norm = None
    # a utils.inference.Overlay: what ``overlay()`` colours and blends with.  A plain attribute as well
    overlay_style = None
    # a utils.confidence.Confidence: the dtype, threshold and fill byte ``confidence()`` serves with.  A plain attribute as well
    confidence_style = None
    # a utils.inference.FrameResize: uint8 frames of another size (camera frames) are resized to it on the device first.  A plain attribute
    input_resize = None
    # a utils.labels.LabelCodec: ``evaluate`` and ``validate`` then take RAW dataset labels -- ids, or a colour image -- and encode them
    # first, on every route.  A plain attribute as well
    label_codec = None

    def encoded(self, target):
        """``target`` itself, or -- with ``label_codec`` set and a target of the codec's input kind (uint8 (B, H, W, 3) for a colour
        list; for a table every 3-D integer target: with a codec set targets are raw by contract) -- the class indices:
        ``HF.label_encode`` (one launch) on the device, ``codec.encode_cpu`` on the CPU."""
        codec = self.label_codec
        if codec is None or not codec.is_raw(target):
            return target
        if target.dtype not in (torch.uint8, torch.int64):
            target = target.long()
        return HF.label_encode(target.contiguous(), codec) if target.is_cuda else codec.encode_cpu(target)

    def resized(self, x):
        """``x`` itself, or -- a uint8 frame tensor of another size than ``input_resize``'s -- the resized uint8 frames (one launch)."""
        resize = self.input_resize
        if resize is None or not isinstance(x, torch.Tensor) or x.dtype != torch.uint8:
            return x
        if resize.layout != self._require_norm().layout:
            raise ValueError(f"model.input_resize takes '{resize.layout}' frames, model.input_norm describes '{self.input_norm.layout}' frames")
        return resize(x) if resize.applies_to(x) else x

    def frame_size(self, x, resize=True):
        """(H, W) of an input tensor as the model sees it: a float image (B, 3, H, W), or uint8 frames in ``input_norm``'s layout -- with
        ``input_resize`` set, the size they are resized to (``resize=False``: an entry of a list input, which is never resized)."""
        if x.dtype == torch.uint8:
            size = tuple(self._require_norm().frame_size(x)[1:])
            return tuple(self.input_resize.size) if (resize and self.input_resize is not None) else size
        return tuple(x.shape[2:])

    def _require_norm(self):
        if self.input_norm is None:
            raise TypeError('uint8 input needs the transform that turns it into the image the model was trained on: set '
                            'model.input_norm = hyperseg_amd.InputNorm(mean, std, layout) (or pass input_norm= to '
                            'prepare_for_inference); float32 inputs are taken as already normalised')
        return self.input_norm

    def _takes_u8_stem(self, frame):
        """The fused uint8 route: the prepared backbone's stem + depthwise launch reads the frame itself and no decoder level reads
        the image (fewer levels than pyramid entries), so the float image is never written."""
        bb = self.backbone
        levels, feats = getattr(self.decoder, 'levels', None), getattr(bb, 'feat_channels', None)
        if not HF.U8_STEM or levels is None or feats is None or levels >= len(feats) or not hasattr(bb, 'takes_u8_frame'):
            return False
        return bb.takes_u8_frame(frame)

    @property
    def hyper_params(self):
        return self.decoder.hyper_params

    def process_single_tensor(self, x, hflip=False, epilogue=None):
        """The logits of one tensor; with ``epilogue`` (an :class:`Epilogue`; inference only, unflipped) what it makes of the decoder's last
        launch instead: the uint8 masks, or masks and per-pixel losses / overlay.  ``Epilogue(defer=True)`` also rides on a flipped frame:
        the :class:`Deferred` is then the MIRRORED frame's (not flipped back: ``HF.tta_merge`` reads it mirrored)."""
        frame = None
        if x.dtype == torch.uint8:
            norm = self._require_norm()
            if x.is_cuda and not hflip and not self.training:
                frame = HF.U8Frame(x, norm)
                if not self._takes_u8_stem(frame):
                    frame = None
            if frame is None:
                x = norm.to_float(x)          # one image_ingest launch, then the float path as it is
        if hflip:
            x = torch.flip(x, [-1])
        features = self.backbone(x if frame is None else frame)
        if frame is not None:
            x = frame.size_carrier()          # the decoder reads the output size from it, nothing else
        head_out = self.weight_mapper(features[-1])
        if isinstance(head_out, torch.Tensor):
            head_out = head_out.contiguous()
        pyramid = [t.contiguous() for t in [x] + features[:-1]]
        # (outside training: the decoders assert that themselves)
        assert epilogue is None or not hflip or epilogue.defer, 'an epilogue rides on the last launch of an unflipped frame'
        y = self.decoder(pyramid, head_out, epilogue=epilogue)
        if isinstance(y, Deferred):
            return y
        return torch.flip(y, [-1]) if hflip else y

    def _logits_at(self, x, size):
        """``self(x)``, resized to ``size`` (H, W) where that is another size: the composed routes' logits at a label's resolution
        (test.py:167-168)."""
        pred = self(x)
        if tuple(pred.shape[2:]) == tuple(size):
            return pred
        if pred.is_cuda:
            return HF.upsample_bilinear(pred.contiguous(), tuple(size))
        return torch.nn.functional.interpolate(pred, size=size, mode='bilinear')

    @staticmethod
    def _count(confmat, target, masks, per_image):
        """The composed routes' scoring: ``confmat``'s own update of finished masks."""
        if per_image:
            confmat.update_per_image(target, masks)
        else:
            confmat.update(target.flatten(), masks.flatten())

    @staticmethod
    def _scorable(target, batch, n):
        """What the fused routes of ``evaluate`` and ``validate`` ask of the target and the class count (``n`` None: nothing counted)."""
        return (isinstance(target, torch.Tensor) and target.dtype in (torch.uint8, torch.int64) and target.dim() == 3
                and target.shape[0] == batch and (n is None or n <= min(256, HF.eval_max_classes())))

    @torch.no_grad()
    def segment(self, x, size=None):
        """uint8 class masks (B, H, W) == ``self(x).argmax(1)`` (the reference's test.py:171 / test_fps.py:194 epilogue).
        For a single tensor in eval mode the argmax is taken inside the final upsample kernel and the full-resolution
        logits are never written; a list input (pyramid / h-flip inference) on the device in eval mode gets its masks from the one
        launch that merges its passes (``HF.tta_merge``: :meth:`_tta_route`), no logits of any pass or entry written.  ``size``: masks at that (H, W) instead
        of the frame's -- the logits resized to it before the arg-max, as test.py:167-168 does for a label of another size; from
        the same one launch (``HF.upsample2_argmax``) where the arg-max is, else the logits route plus that resize."""
        x = self.resized(x)
        first = x if isinstance(x, torch.Tensor) else x[0]
        if size is not None and tuple(size) == self.frame_size(first, isinstance(x, torch.Tensor)):
            size = None
        fused = isinstance(x, torch.Tensor) and not self.training and not self.inference_hflip
        if size is None and self._tta_route(x):
            return self._tta_merged(x, masks=True).masks
        if size is None:
            return self.process_single_tensor(x, epilogue=Epilogue()) if fused else self(x).argmax(1).to(torch.uint8)
        size = tuple(int(s) for s in size)
        if fused and x.is_cuda:
            return self.process_single_tensor(x, epilogue=Epilogue(out_size=size))
        return self._logits_at(x, size).argmax(1).to(torch.uint8)

    @torch.no_grad()
    def evaluate(self, x, target, confmat, per_image=False):
        """``segment(x)`` plus scoring: returns the uint8 masks and adds this batch's (target, prediction) counts to ``confmat``
        (a ``hyperseg_amd.fps.ConfusionMatrix``; ``per_image=True`` also appends the batch's (B, n, n) matrices to
        ``confmat.per_image`` -- test.py:174-175 without a host read per image).  A single CUDA tensor in eval mode with a
        target is scored by the forward's last launch: no further launch, no read of the device -- a target of the output's size by
        ``HF.upsample_confusion``, one of another size at ITS resolution (the LOGITS are resized to it, test.py:167-168 -- the
        protocol of the reference's Cityscapes test configs) by ``HF.upsample2_confusion``, the returned masks then at the target's
        size.  A list input (pyramid / h-flip inference) on the device in eval mode is scored by the launch that merges its passes
        (``HF.tta_merge``) when the target is at the first entry's size; a target of another size, or more classes than the kernel
        covers, gets its masks from ``segment()`` / ``forward()`` -- the same launch -- and ``confmat``'s own update.  Everything else --
        training mode, CPU -- computes the masks the way ``segment()`` / ``forward()`` do (resizing the logits to a target of another size) and
        counts them with ``confmat``'s own update.  Same numbers on every route.  With ``label_codec`` set a raw ``target`` is encoded
        first (:meth:`encoded`), whatever the route."""
        n = confmat.num_classes
        x = self.resized(x)
        target = self.encoded(target)
        fused = (isinstance(x, torch.Tensor) and x.is_cuda and not self.training and isinstance(target, torch.Tensor)
                 and target.is_cuda and self._scorable(target, x.shape[0], n))
        if fused:
            mat = confmat.matrix(x.device)
            out = torch.zeros((x.shape[0], n, n), dtype=torch.int64, device=x.device) if per_image else mat
            masks = self.process_single_tensor(x, epilogue=Epilogue(Score(target, n, out, per_image)))
            if per_image:
                confmat.add_per_image(out)
            if masks.dtype == torch.uint8:
                return masks
            raise RuntimeError('the decoder returned logits where its epilogue was asked for: nothing was scored')
        out_res = self.frame_size(x, True) if isinstance(x, torch.Tensor) else self.frame_size(x[0], False)
        if (self._tta_route(x) and isinstance(target, torch.Tensor) and target.is_cuda and tuple(target.shape[1:]) == out_res
                and self._scorable(target, x[0].shape[0], n)):
            mat = confmat.matrix(x[0].device)
            out = torch.zeros((x[0].shape[0], n, n), dtype=torch.int64, device=x[0].device) if per_image else mat
            got = self._tta_merged(x, masks=True, score=Score(target, n, out, per_image))
            if per_image:
                confmat.add_per_image(out)
            return got.masks
        if tuple(target.shape[1:]) != out_res:
            masks = self._logits_at(x, target.shape[1:]).argmax(1).to(torch.uint8)
        else:
            masks = self.segment(x)
        self._count(confmat, target, masks, per_image)
        return masks

    def _validate_route(self, x, target, criterion, n, staged=False):
        """The fused route validate() takes for this batch -- see there: 'frame' (a target at the frame's size), 'label' (a target of
        another size: the route at the LABEL's resolution, ``criterion.k`` and the pixel bound taken on the label's pixels) or None (the
        composed route).  ``staged``: a serving wrapper copies ``x`` and ``target`` to the model's device first
        (``GraphedModel.validate``), so where they live now does not matter."""
        from ..training import BootstrappedCrossEntropyLoss, USE_HIP_BOOTSTRAP, USE_FUSED_LOSS
        if not (isinstance(x, torch.Tensor) and x.dim() == 4 and not self.training and isinstance(target, torch.Tensor)
                and (staged or (x.is_cuda and target.is_cuda)) and self._scorable(target, x.shape[0], n)):
            return None
        if not (isinstance(criterion, BootstrappedCrossEntropyLoss) and criterion.score is None and USE_HIP_BOOTSTRAP and USE_FUSED_LOSS):
            return None
        if criterion.weight is not None:                        # a table the HIP loss takes (asked once per table), on the model's device
            device = next(self.parameters()).device if staged else x.device
            classes = getattr(self.decoder, 'num_classes', None)      # the logits' channels (a decoder that does not say: composed route)
            if classes is None or not criterion.weight_takes_hip(classes, device):
                return None
        if x.shape[0] > 65535 or not criterion.k < target.shape[1] * target.shape[2] < 2 ** 31:
            return None
        return 'frame' if tuple(target.shape[1:]) == self.frame_size(x) else 'label'

    def _validate_fused(self, x, target, criterion, n, staged=False):
        return self._validate_route(x, target, criterion, n, staged) == 'frame'

    def _validate_fused_at_label(self, x, target, criterion, n, staged=False):
        return self._validate_route(x, target, criterion, n, staged) == 'label'

    def _validate_step(self, x, target, criterion, n, out, per_image, route):
        """The fused validation step of ``route`` ('frame' or 'label': ``_validate_route``), eager or under capture: the forward with the
        scoring epilogue as its last launch, then the criterion's batch reduction.  ``x`` resized, ``target`` encoded; returns ``(loss,
        masks)``."""
        from ..autograd import BootstrapMeanOfBatch
        at = dict(loss_at_label=True) if route == 'label' else {}       # (the same-size epilogue is what it was)
        got = self.process_single_tensor(x, epilogue=Epilogue(Score(target, n, out, per_image), ignore_index=criterion.ignore_index,
                                                                   weight=criterion.weight, **at))
        if not isinstance(got, tuple):
            raise RuntimeError('the decoder returned logits where its epilogue was asked for: nothing was scored')
        masks, per_pixel = got
        return BootstrapMeanOfBatch.apply(per_pixel.flatten(1), criterion.k, criterion.thresh), masks

    @torch.no_grad()
    def validate(self, x, target, criterion, confmat=None, per_image=False):
        """One validation batch of the reference's epoch loop (train.py:118-126 in ``eval()`` mode under ``no_grad``): returns ``(loss,
        masks)`` -- ``criterion(self(x), target)`` as a 0-dim f32 tensor (no host read) and the uint8 masks ``self(x).argmax(1)`` -- and
        adds the batch's (target, prediction) counts to ``confmat`` (a ``hyperseg_amd.fps.ConfusionMatrix``; None: loss and masks only;
        ``per_image`` as ``evaluate``'s).  ``training.running_scores(confmat.mat)`` gives the numbers train.py picks ``model_best`` by.

        A single CUDA tensor in eval mode, a ``BootstrappedCrossEntropyLoss`` (without a ``score`` of its own; class weights, if any, a
        table the HIP loss takes: ``training.weight_fusable`` -- fp32 (C,) on the device, finite and >= 0),
        a uint8 / int64 target at the frame's size with more than ``criterion.k`` pixels and at most ``HF.eval_max_classes()`` classes:
        the forward's last launch (``HF.upsample_ce_confusion``) makes the per-pixel losses, the masks and the counts -- the
        full-resolution logits are never written -- and the criterion's own batch reduction follows (the launches its fused forward
        makes after its first).  A target of ANOTHER size than the frame's (the reference's Cityscapes validation: the image is resized,
        the label is not, train.py:119-120 resizes the logits to the label) takes the same route at the label's resolution, under the same
        conditions with ``criterion.k`` taken against the label's pixels: the last launch (``HF.upsample2_ce_confusion``) composes the
        decoder's final resize with the one to the label, and losses, masks and counts are at the label's size; neither the frame-size nor
        the label-size logits are written.  Everything else -- list inputs (whose logits ``self(x)`` come from the launch that merges their
        passes, ``HF.tta_merge``), training mode, CPU, class weights the HIP
        loss does not take, another criterion -- computes ``pred = self(x)``, resizes it to the target as ``evaluate`` does, and takes ``criterion(pred,
        target.long())``, ``argmax`` and ``confmat``'s own update.  On the device every route gives the same loss bits, masks and
        counts from the same decoder input.  (An unprepared model's stock torch encoder does not repeat its own bits from one call to
        the next, so two separate passes of it need not agree to the bit, whichever routes they take: DESIGN 3.11.)  The
        CPU's composed route is stock torch ops: same masks and counts, the loss to rounding."""
        n = None if confmat is None else confmat.num_classes
        x = self.resized(x)
        target = self.encoded(target)
        batch = (x if isinstance(x, torch.Tensor) else x[0]).shape[0]
        if not isinstance(target, torch.Tensor) or target.is_floating_point() or target.dim() != 3 or target.shape[0] != batch:
            raise ValueError(f'target must be ({batch}, H, W) class indices (uint8 or int64), got {getattr(target, "dtype", type(target))} '
                             f'{tuple(getattr(target, "shape", ()))}')
        route = self._validate_route(x, target, criterion, n)
        if route is not None:
            out = None
            if confmat is not None:
                out = torch.zeros((x.shape[0], n, n), dtype=torch.int64, device=x.device) if per_image else confmat.matrix(x.device)
            loss, masks = self._validate_step(x, target, criterion, n, out, per_image, route)
            if confmat is not None and per_image:
                confmat.add_per_image(out)
            return loss, masks
        pred = self._logits_at(x, target.shape[1:])
        target = target.to(pred.device)
        loss = criterion(pred, target.long())
        masks = pred.argmax(1).to(torch.uint8)
        if confmat is not None:
            self._count(confmat, target, masks, per_image)
        return loss.detach(), masks

    @torch.no_grad()
    def overlay(self, x, frames=None, style=None, out=None, size=None):
        """``segment(x)`` plus the display: returns ``(masks, overlay)`` -- the uint8 masks and the class map coloured and alpha-blended
        over the uint8 frames, as uint8 in the frames' layout (``style``: a ``utils.inference.Overlay``, default
        ``self.overlay_style``).  A uint8 ``x`` is its own frame; a float ``x`` needs ``frames=``, the uint8 frames of the same size.
        A single CUDA tensor in eval mode without h-flip inference is blended by the forward's last launch
        (``HF.upsample_overlay``) -- no further launch, no read of the device, whether the frame went into the stem launch or through
        ``image_ingest``.  Everything else -- list inputs, h-flip inference, training mode, CPU -- computes the masks the way
        ``segment()`` does (a list's from the launch that merges its passes, ``HF.tta_merge``) and calls ``style.blend``.  Same bytes on every route.  ``out``: a uint8 tensor of the frames' shape for
        the overlay.

        ``size=(H, W)``: the display at that size instead of the model's frame -- the camera's, when ``input_resize`` shows the model a
        down-scaled copy.  The logits are resized to it before the arg-max, as ``segment(size=)`` does (test.py:167-168); masks and overlay
        are at ``(H, W)``.  The frames blended over are ``frames=`` ((B, H, W) frames), else a uint8 ``x`` whose own size is ``(H, W)`` --
        the camera frame before ``input_resize``, or the frame itself where there is no resize -- else a ``ValueError`` naming both sizes.
        The fused route composes both resizes and the blend in the forward's last launch (``HF.upsample2_overlay``; a decoder without
        a final resize: ``HF.upsample_overlay`` straight to ``size``): neither logits tensor and no frame-size mask are written.  The
        other routes resize the logits (``_logits_at``), arg-max them and call ``style.blend``.  Same bytes on every route."""
        style = self.overlay_style if style is None else style
        if style is None:
            raise TypeError('overlay() needs a style: set model.overlay_style = hyperseg_amd.Overlay(color_map, alpha, ignore_index, '
                            'layout) or pass style=')
        if size is not None:
            return self._overlay_at(x, frames, style, out, tuple(int(s) for s in size))
        x = self.resized(x)
        first = x if isinstance(x, torch.Tensor) else x[0]
        if frames is None:
            if first.dtype != torch.uint8:
                raise TypeError('a float input needs frames=: the uint8 frames of the same size that the overlay is blended over '
                                '(a uint8 input is its own frame)')
            if style.layout != self._require_norm().layout:
                raise ValueError(f"the input frames are '{self.input_norm.layout}' (model.input_norm), the style blends over "
                                 f"'{style.layout}' frames")
            frames = first
        size = (first.shape[0],) + self.frame_size(first, isinstance(x, torch.Tensor))
        if tuple(style.frame_size(frames)) != size:
            raise ValueError(f'frames are {tuple(style.frame_size(frames))} (B, H, W), the input is {size}')
        fused = isinstance(x, torch.Tensor) and x.is_cuda and frames.is_cuda and not self.training and not self.inference_hflip
        if fused:
            got = self.process_single_tensor(x, epilogue=Epilogue(blend=Blend(frames, style, out)))
            if isinstance(got, tuple):
                return got
            raise RuntimeError('the decoder returned logits where its epilogue was asked for: nothing was blended')
        masks = self.segment(x)
        blended = style.blend(frames.to(masks.device), masks)
        if out is not None:
            out.copy_(blended)
            blended = out
        return masks, blended

    def _overlay_frames_at(self, x, frames, style, size):
        """The frames ``overlay(x, frames, size=size)`` blends over: ``frames`` where given, else ``x`` (a list: its first entry) where it
        is uint8 frames of ``size`` already -- the camera frame, before ``input_resize`` -- in the style's layout.  Raises ``ValueError``
        unless they are (B, *size) frames."""
        first = x if isinstance(x, torch.Tensor) else x[0]
        if frames is None:
            if first.dtype == torch.uint8:
                if style.layout != self._require_norm().layout:
                    raise ValueError(f"the input frames are '{self.input_norm.layout}' (model.input_norm), the style blends over "
                                     f"'{style.layout}' frames")
                own = tuple(style.frame_size(first)[1:])
            else:
                own = tuple(first.shape[2:])
            if first.dtype != torch.uint8 or own != size:
                raise ValueError(f'overlay(size={size}) blends over frames of that size: the input is {own} '
                                 f'({str(first.dtype).replace("torch.", "")}), pass frames= with uint8 frames of {size}')
            frames = first
        want = (first.shape[0],) + size
        if tuple(style.frame_size(frames)) != want:
            raise ValueError(f'frames are {tuple(style.frame_size(frames))} (B, H, W), overlay(size=) needs {want}')
        return frames

    def _overlay_at(self, x, frames, style, out, size):
        """``overlay`` with ``size=``: see there."""
        frames = self._overlay_frames_at(x, frames, style, size)
        x = self.resized(x)
        first = x if isinstance(x, torch.Tensor) else x[0]
        if size == self.frame_size(first, isinstance(x, torch.Tensor)):
            return self.overlay(x, frames=frames, style=style, out=out)
        fused = isinstance(x, torch.Tensor) and x.is_cuda and frames.is_cuda and not self.training and not self.inference_hflip
        if fused:
            got = self.process_single_tensor(x, epilogue=Epilogue(blend=Blend(frames, style, out, size)))
            if isinstance(got, tuple):
                return got
            raise RuntimeError('the decoder returned logits where its epilogue was asked for: nothing was blended')
        masks = self._logits_at(x, size).argmax(1).to(torch.uint8)
        blended = style.blend(frames.to(masks.device), masks)
        if out is not None:
            out.copy_(blended)
            blended = out
        return masks, blended

    @torch.no_grad()
    def confidence(self, x, size=None, style=None):
        """``segment(x, size)`` plus how sure the model is: returns ``(masks, conf)`` -- the uint8 masks and, per pixel, the soft-max
        probability of its class, ``softmax(logits, 1).max(1)`` taken in fp32 (csrc/hs_confidence.h), as ``style.dtype`` (``style``: a
        ``utils.confidence.Confidence``, default ``self.confidence_style``, else ``Confidence()``: uint8, no threshold); with a
        threshold the masks carry the style's fill byte where the confidence is below it.  A single CUDA tensor in eval mode without
        h-flip inference gets both from the forward's last launch (``HF.upsample_confidence``; with ``size=`` ``HF.upsample2_confidence``)
        -- no further launch, no read of the device, the full-resolution logits never written; uint8 frames, ``input_resize`` and
        ``size=`` as in ``segment()``.  Everything else -- list inputs, h-flip inference, training mode, CPU -- takes the logits (a
        list's from the launch that merges its passes, ``HF.tta_merge``; resized to ``size``) and ``HF.confidence``, on the CPU ``utils.confidence.confidence_cpu``.  Same masks on every route; on the device the
        same confidence bits from the same decoder input."""
        from ..utils.confidence import Confidence
        style = self.confidence_style if style is None else style
        style = Confidence() if style is None else style
        if not isinstance(style, Confidence):
            raise TypeError('confidence() takes a hyperseg_amd.Confidence as its style')
        x = self.resized(x)
        first = x if isinstance(x, torch.Tensor) else x[0]
        frame = self.frame_size(first, isinstance(x, torch.Tensor))
        size = frame if size is None else tuple(int(s) for s in size)
        fused = isinstance(x, torch.Tensor) and x.is_cuda and not self.training and not self.inference_hflip
        if fused:
            got = self.process_single_tensor(x, epilogue=Epilogue(confidence=style, out_size=None if size == frame else size))
            if isinstance(got, tuple):
                return got
            raise RuntimeError('the decoder returned logits where its epilogue was asked for: no confidence was made')
        return style.of_logits(self._logits_at(x, size))

    def _tta_deferrable(self, x):
        """The passes of a list input can hand over the input of their final resize (``Epilogue(defer=True)``): eval mode, every entry a
        CUDA tensor, nothing that needs grad, a decoder whose route takes an epilogue.  Such a list is merged from its deferred passes --
        by the merge launch (:meth:`_tta_route`) or, launch per step, by ``HF.tta_merge_composed``; training mode, the CPU and tensors
        that need grad keep the loop of :meth:`forward`."""
        if not isinstance(x, (list, tuple)) or len(x) == 0 or self.training:
            return False
        if not all(isinstance(t, torch.Tensor) and t.is_cuda and t.dim() == 4 for t in x):
            return False
        # (asked of the parameters only with grad enabled, and only up to the first that needs it: serving runs under no_grad)
        if torch.is_grad_enabled() and (any(t.requires_grad for t in x) or any(p.requires_grad for p in self.parameters())):
            return False
        groups = getattr(self.decoder, '_hyper_modules', None)      # (several signal-fed modules in a level: the per-module route, no epilogue)
        return groups is None or not any(len(g) > 1 for g in groups())

    def _tta_route(self, x):
        """A list input takes the merge launch (``HF.tta_merge``: the decoder's passes deferred, merged in ONE launch): a deferrable list
        (:meth:`_tta_deferrable`) of at most ``HF.TTA_MAX_PASSES`` passes in total (entries, times two with ``inference_hflip``), with
        ``HF.TTA_MERGE`` on.  A single tensor, which the reference never flips, is not involved at all."""
        if not HF.TTA_MERGE or not isinstance(x, (list, tuple)) or len(x) * (2 if self.inference_hflip else 1) > HF.TTA_MAX_PASSES:
            return False
        return self._tta_deferrable(x)

    def _tta_merged(self, x, logits=False, masks=False, score=None):
        """The passes of the list ``x`` in the reference's order (per entry: plain, then mirrored), each with its last launch deferred, and
        the one launch that merges them -- ``HF.tta_merge``'s result; with ``HF.TTA_MERGE`` off, or more passes or channels than the
        launch takes, ``HF.tta_merge_composed`` of the same passes: the composed route, stated there once."""
        passes = []
        for entry, level in enumerate(x):
            for flipped in ((False, True) if self.inference_hflip else (False,)):
                got = self.process_single_tensor(level, hflip=flipped, epilogue=Epilogue(defer=True))
                if not isinstance(got, Deferred):
                    raise RuntimeError('the decoder returned logits where its last launch was to be deferred')
                passes.append((got.x, got.size, flipped, entry))
        scored = {} if score is None else dict(target=score.target, num_classes=score.num_classes, out=score.out, per_image=score.per_image)
        merge = HF.tta_merge if HF.TTA_MERGE and HF.tta_merge_takes(len(passes), passes[0][0].shape[1]) else HF.tta_merge_composed
        return merge(passes, 'mean' if self.inference_gather == 'mean' else 'max', logits=logits, masks=masks, **scored)

    def gather_results(self, x, y=None):
        assert x is not None
        if y is None:
            return x
        return (x + y) * 0.5 if self.inference_gather == 'mean' else torch.max(x, y)

    def forward(self, x):
        if isinstance(x, torch.Tensor):
            return self.process_single_tensor(self.resized(x))
        assert isinstance(x, (list, tuple)), 'x must be of type list, tuple, or tensor'
        if self._tta_deferrable(x):                     # (on the device in eval mode: the merge launch, or tta_merge_composed)
            return self._tta_merged(x, logits=True).logits
        out_res = self.frame_size(x[0], resize=False)   # the first pyramid level sets the output resolution
        merged = None
        for level in x:
            y = self.process_single_tensor(level)
            if self.inference_hflip:
                y = torch.max(y, self.process_single_tensor(level, hflip=True))
            if tuple(y.shape[2:]) != out_res:
                y = HF.upsample_bilinear(y.contiguous(), out_res)
            merged = self.gather_results(y, merged)
        return merged
