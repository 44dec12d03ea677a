"""Confidence maps on the CPU, and the object that says how a model serves them.

``confidence_cpu`` is the CPU statement of csrc/hs_confidence.h: beside the arg-max mask, the soft-max probability of the winning class,
``softmax(v)[argmax] = 1 / sum_c exp(v_c - v_max)``, taken in float32 in ONE ascending pass over the classes with a running maximum ``m``
and a rescaled running sum ``s`` -- ``v_c > m``: ``s = s * exp(m - v_c) + 1`` then ``m = v_c``; otherwise ``s += exp(v_c - m)`` -- the same
quantisation ``uint8(conf * 255 + 0.5)`` and the same threshold rule (a pixel whose fp32 confidence is ``< threshold`` gets ``fill`` in the
mask; the confidence is not changed by it).  CPU tensors take it; the tests use it as their fp32 restatement of the kernels.  It differs
from the device only by the two ``exp`` implementations' last bit.
"""
import torch

CONF_DTYPES = {torch.float32: 0, torch.uint8: 1}          # hs_conf_dtype of include/hyperseg_hip.h


def check_args(dtype, threshold, fill):
    """``(dtype, threshold as a float or None, fill)`` or ValueError: what every confidence entry point asks of these three."""
    if dtype not in CONF_DTYPES:
        raise ValueError(f'the confidence is float32 or uint8 (conf * 255 + 0.5), got dtype={dtype}')
    if threshold is not None:
        if isinstance(threshold, bool) or not isinstance(threshold, (int, float)) or threshold != threshold:
            raise ValueError(f'threshold must be a number (pixels with a confidence below it take the fill byte) or None, got {threshold!r}')
        threshold = float(threshold)
    if isinstance(fill, bool) or int(fill) != fill or not 0 <= int(fill) <= 255:
        raise ValueError(f'fill must be a byte (0..255): the masks are uint8, got {fill!r}')
    return dtype, threshold, int(fill)


def quantise(conf):
    """The served form of an fp32 confidence: ``uint8(conf * 255 + 0.5)``, 255 for 1.0."""
    return (conf * 255.0 + 0.5).to(torch.uint8)


def softmax_max_f32(logits):
    """``(idx, conf)`` of (B, C, ...) scores: int64 arg-max (first maximum) and the float32 confidence, by the recurrence above."""
    v = logits.to(torch.float32)
    m, s = v[:, 0].clone(), torch.ones_like(v[:, 0])
    idx = torch.zeros(m.shape, dtype=torch.int64, device=v.device)
    for c in range(1, v.shape[1]):
        vc = v[:, c]
        up = vc > m
        e = torch.exp(torch.where(up, m - vc, vc - m))
        s = torch.where(up, s * e + 1.0, s + e)
        m = torch.where(up, vc, m)
        idx = torch.where(up, torch.full_like(idx, c), idx)
    return idx, 1.0 / s


def label(idx, conf, threshold, fill):
    """The uint8 masks: ``idx`` with ``fill`` where the fp32 confidence is strictly below ``threshold`` (taken in float32, as the kernels'
    argument is)."""
    masks = idx.to(torch.uint8)
    if threshold is None:
        return masks
    t = torch.tensor(threshold, dtype=torch.float32, device=conf.device)
    return torch.where(conf < t, torch.full_like(masks, fill), masks)


def confidence_cpu(logits, dtype=torch.uint8, threshold=None, fill=255):
    """``(masks, conf)`` of (B, C, H, W) logits with stock ops: uint8 masks (B, H, W) and the confidence as ``dtype``."""
    dtype, threshold, fill = check_args(dtype, threshold, fill)
    if not isinstance(logits, torch.Tensor) or logits.dim() != 4 or logits.shape[1] < 1:
        raise ValueError('logits must be (B, C, H, W)')
    if logits.shape[1] > 256:
        raise ValueError('more than 256 logit channels: the masks are uint8')
    idx, conf = softmax_max_f32(logits)
    return label(idx, conf, threshold, fill), (conf if dtype == torch.float32 else quantise(conf))


class Confidence:
    """How a model serves its confidence maps: the confidence's ``dtype`` -- ``torch.uint8`` (the served form, ``uint8(conf * 255 + 0.5)``)
    or ``torch.float32`` -- and, optionally, pseudo-labels: with ``threshold`` a pixel whose fp32 confidence is ``< threshold`` gets ``fill``
    (default 255, the usual ignore value) in the masks.  Attached to a model (``model.confidence_style = Confidence(...)``) it serves
    ``model.confidence`` / ``GraphedModel.confidence``.  Not a parameter, not a buffer: state dicts are unaffected."""

    def __init__(self, dtype=torch.uint8, threshold=None, fill=255):
        self.dtype, self.threshold, self.fill = check_args(dtype, threshold, fill)

    def of_logits(self, logits):
        """``(masks, conf)`` of finished (B, C, H, W) logits: one ``functional.confidence`` launch on the GPU, ``confidence_cpu`` on the
        CPU."""
        if logits.is_cuda:
            from .. import functional as HF
            return HF.confidence(logits.contiguous(), self.dtype, self.threshold, self.fill)
        return confidence_cpu(logits, self.dtype, self.threshold, self.fill)

    def _key(self):
        return (self.dtype, self.threshold, self.fill)

    def __eq__(self, other):
        return isinstance(other, Confidence) and self._key() == other._key()

    def __hash__(self):
        return hash(self._key())

    def __repr__(self):
        return f'Confidence(dtype={self.dtype}, threshold={self.threshold}, fill={self.fill})'
