"""Train-step counterparts of the reference's training harness for config 5 ("harness counterparts
(ii)"): the loss, the LR policy and the step that drive the decoder's autograd path.  Plain PyTorch -- the HIP work happens
inside ``model(x)`` / ``backward()`` through hyperseg_amd.autograd.

* :class:`BootstrappedCrossEntropyLoss` -- hyperseg/losses/bootstrapped_ce_loss.py:8-40: per IMAGE (not per batch), the
  pixel-wise cross entropy is sorted in descending order; if the (k+1)-th largest loss exceeds ``thresh`` every pixel above
  ``thresh`` is kept, otherwise the k largest; the image's loss is the mean of what is kept; the batch loss is the mean of
  the image losses.  ``ignore_index`` pixels contribute a loss of exactly 0 and stay in the ranking.
* :class:`PolyLR` -- hyperseg/utils/polylr.py:4-22: lr = base_lr * (1 - step/max_step)**power, stepped per batch.
* :func:`train_step` -- hyperseg/train.py:118-136: forward, resize the prediction to the target if needed, loss,
  zero_grad / backward / optimizer.step / scheduler.step.
"""
import collections

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.optim.lr_scheduler import LRScheduler


USE_HIP_BOOTSTRAP = True       # tests switch it off to reach the torch statements of the rule below
USE_FUSED_LOSS = True          # False: cross entropy and the bootstrapped mean as two Functions (two launches backward; the fused one's equality test)


def bootstrap_mean_reference(per_pixel, k, thresh):
    """The reference's own statement (hyperseg/losses/bootstrapped_ce_loss.py:19-25): two host reads and a full sort per image."""
    ranked = per_pixel.sort(descending=True).values
    kept = ranked[ranked > thresh] if ranked[k] > thresh else ranked[:k]
    return kept.mean()


def bootstrap_mean_on_device(per_pixel, k, thresh):
    """The same rule with ONE host read and, in the common case, no sort: the (k+1)-th largest loss exceeds ``thresh`` exactly when
    more than k losses do, so the count decides the branch -- the mean of everything above ``thresh`` is a masked sum, and only the
    other branch needs the k largest (``topk``).  The reference reads the host twice per image (the comparison, then a boolean
    index) around a full sort of 3e5 losses (18 merge launches, ~0.2 ms per image at config 5).  Values within 1e-6 and gradients
    equal to the reference statement (tests/test_oracle_golden.py)."""
    over = per_pixel > thresh
    count = over.sum()
    if int(count) > k:
        return (per_pixel * over).sum() / count
    return per_pixel.topk(k, sorted=False).values.mean()


def bootstrap_mean_capturable(per_pixel, k, thresh):
    """The rule with NO host read, for a step that is being captured into a HIP graph (GraphedTrainStep): both branches are formed
    (``topk(k + 1)`` -- on ROCm a full merge sort -- and the masked mean) and ``where`` selects; the gradient reaches the selected
    branch only, as in the reference."""
    top = per_pixel.topk(k + 1, sorted=True).values
    over = per_pixel > thresh
    mean_over = (per_pixel * over).sum() / over.sum().clamp(min=1)
    return torch.where(top[k] > thresh, mean_over, top[:k].mean())


def bootstrapped_cross_entropy(pred, target, k=4096, thresh=0.3, weight=None, ignore_index=-100, score=None):
    """pred (N, C, H, W) logits, target (N, H, W) int64 -> scalar.  ``score``: ``BootstrappedCrossEntropyLoss.score``."""
    capturing = pred.is_cuda and torch.cuda.is_current_stream_capturing()
    # the per-pixel losses of the WHOLE batch in one pass over (N, C, H, W) (the reference permutes every image to (HW, C) first,
    # bootstrapped_ce_loss.py:20-23: same values, a transposed copy + a softmax + a gather per image and direction)
    hip_ce = (USE_HIP_BOOTSTRAP and weight is None and pred.is_cuda and pred.dtype in (torch.float32, torch.bfloat16, torch.float16) and pred.dim() == 4
              and target.dtype == torch.int64 and target.device == pred.device)
    fused = hip_ce and USE_FUSED_LOSS and pred.shape[2] * pred.shape[3] > k and pred.shape[0] <= 65535 and pred.shape[2] * pred.shape[3] < 2 ** 31
    if score is not None:
        if pred.dim() < 2 or pred.shape[1] > score.num_classes:
            raise ValueError(f'{pred.shape[1] if pred.dim() > 1 else 0} logit channels but the score counts {score.num_classes} classes')
        if fused and _score_in_loss_launch(score.num_classes):
            from .autograd import BootstrappedCrossEntropyScored           # the loss launch counts the batch: no further launch
            return BootstrappedCrossEntropyScored.apply(pred, target, ignore_index, k, thresh, score.matrix(pred.device))
        score.update(target.flatten(), pred.detach().argmax(1).flatten())  # every other route: the loss as it was, scored by the matrix itself
    if fused:
        from .autograd import BootstrappedCrossEntropy                     # the whole loss as one Function: its adjoint is one launch (round 6)
        return BootstrappedCrossEntropy.apply(pred, target, ignore_index, k, thresh)
    if hip_ce:
        from .autograd import PixelCrossEntropy                            # one launch per direction (hs_cross_entropy_typed_fwd / _bwd)
        per_all = PixelCrossEntropy.apply(pred, target, ignore_index)
    else:
        per_all = F.cross_entropy(pred.float(), target, weight=weight, ignore_index=ignore_index, reduction='none')
    per_rows = per_all.flatten(1)
    if (USE_HIP_BOOTSTRAP and per_rows.is_cuda and per_rows.dtype == torch.float32 and per_rows.shape[1] > k and per_rows.shape[0] <= 65535):
        from .autograd import BootstrapMeanOfBatch                         # every image in one set of launches, no sort, no host read; the
        return BootstrapMeanOfBatch.apply(per_rows, k, thresh)             # batch mean from the same launches (no sum / div launches)
    total = pred.new_zeros((), dtype=torch.float32)
    for per_pixel in per_rows:
        on_device = per_pixel.is_cuda and per_pixel.numel() > k            # (numel <= k: the reference raises; so does its restatement)
        if on_device and per_pixel.dtype == torch.float32 and USE_HIP_BOOTSTRAP:
            from .autograd import BootstrapMean                            # no sort, no host read, 7 small launches: eager and captured alike
            total = total + BootstrapMean.apply(per_pixel, k, thresh)
            continue
        fn = bootstrap_mean_capturable if capturing and on_device else bootstrap_mean_on_device if on_device else bootstrap_mean_reference
        total = total + fn(per_pixel, k, thresh)
    return total / float(pred.shape[0])


def _score_in_loss_launch(num_classes):
    from . import functional as HF
    return num_classes <= min(256, HF.eval_max_classes())


class BootstrappedCrossEntropyLoss(nn.Module):
    """``score``: a plain attribute, default None -- set it to a ``hyperseg_amd.fps.ConfusionMatrix`` and every ``forward`` also adds the
    batch's (target, ``input.argmax(1)``) counts to it: the running score the reference's epoch loop keeps next to the loss
    (train.py:124-126, ``running_metrics.update``).  On the fused-loss route (CUDA logits, no class weights, more than ``k`` pixels, at
    most ``functional.eval_max_classes()`` classes) the loss launch itself counts, from the logits it holds in registers, into
    ``score.matrix(device)``: the same loss bits, the same gradients, no further launch and nothing read back, so a captured step
    (``GraphedTrainStep``) counts with every replay.  Every other route computes the loss as without it and calls ``score.update``.
    Counting follows the reference's ``runningScore``, which does not know ``ignore_index``: every target in [0, n) is counted, also one
    that equals an in-range ``ignore_index`` (its loss is 0).  :func:`running_scores` turns the matrix into train.py's numbers."""

    score = None

    def __init__(self, k=4096, thresh=0.3, weight=None, ignore_index=-100, reduction='mean'):
        super().__init__()
        if reduction != 'mean':
            raise ValueError("only reduction='mean' is meaningful: the reference stores the argument and always averages")
        self.k, self.thresh, self.ignore_index = k, thresh, ignore_index
        self.register_buffer('weight', weight)

    def forward(self, input, target):
        return bootstrapped_cross_entropy(input, target, self.k, self.thresh, self.weight, self.ignore_index, self.score)


@torch.no_grad()
def running_scores(mat):
    """``runningScore.get_scores()`` (hyperseg/train.py:310-335) from an (n, n) count matrix of (target, prediction) pairs -- a
    ``ConfusionMatrix.mat``, a ``GraphedModel.confusion``: ``(scores, class_iou)`` with ``scores`` = {'overall_acc', 'mean_acc',
    'freqw_acc', 'mean_iou'} as floats and ``class_iou`` a dict class -> IoU.  float64 on the host (one read of the matrix), numpy's
    semantics: a class without pixels has a nan accuracy / IoU and is left out of the two means (``nanmean``; nan if every class is).
    Not ``ConfusionMatrix.compute()``, which carries test.py's 1e-6 guards: this is the number train.py picks ``model_best`` by."""
    hist = torch.as_tensor(mat).detach().to('cpu', torch.float64)
    if hist.dim() != 2 or hist.shape[0] != hist.shape[1]:
        raise ValueError(f'expected an (n, n) count matrix, got {tuple(hist.shape)}')
    diag, rows, cols = torch.diag(hist), hist.sum(1), hist.sum(0)
    total = hist.sum()
    acc_cls = diag / rows
    iu = diag / (rows + cols - diag)
    freq = rows / total

    def nanmean(v):
        keep = ~torch.isnan(v)
        return float(v[keep].mean()) if bool(keep.any()) else float('nan')
    scores = {'overall_acc': float(diag.sum() / total), 'mean_acc': nanmean(acc_cls),
              'freqw_acc': float((freq[freq > 0] * iu[freq > 0]).sum()), 'mean_iou': nanmean(iu)}
    return scores, {c: float(v) for c, v in enumerate(iu)}


class PolyLR(LRScheduler):
    def __init__(self, optimizer, max_epoch, power=0.9, last_epoch=-1):
        self.max_epoch, self.power = max_epoch, power
        super().__init__(optimizer, last_epoch)

    def get_lr(self):
        decay = (1.0 - float(self.last_epoch) / float(self.max_epoch)) ** self.power
        return [base * decay for base in self.base_lrs]


class Adam(torch.optim.Optimizer):
    """``torch.optim.Adam`` / ``AdamW`` arithmetic (no amsgrad) with the whole parameter list of a group updated by ONE launch of
    1024-element workgroups (``hs_adam_step``; round 5).  The reference trains with ``optim.Adam(lr, betas=(0.5, 0.999))``
    (hyperseg/train.py:185-188, configs/train/*); torch's fused form is one launch too, but it cuts the list into 65 536-element
    chunks -- a dozen workgroups for the decoder's ~0.7 M parameters, 25 us of a 0.88 ms config-5 step.

    Capturable by construction: the step count lives on the device (one word per workgroup, incremented by the kernel), ``lr`` may be a
    float or a one-element CUDA tensor (what a scheduler updates in place under a captured step, ``GraphedTrainStep``).  fp32 CUDA
    parameters with dense fp32 gradients only; every parameter of a group that has a gradient takes part, and the SET of those
    parameters must not change between steps (the per-workgroup step words are laid out for it; a change raises).

    GradScaler protocol (``_step_supports_amp_scaling``): under ``torch.amp.GradScaler.step`` the ``grad_scale`` / ``found_inf`` device
    tensors the scaler attaches go to ``hs_adam_step_amp`` -- the gradients are unscaled inside the launch (and left unscaled in
    ``p.grad``, as torch's fused Adam leaves them) and a set ``found_inf`` skips the step on the device: no host read, capturable."""

    _step_supports_amp_scaling = True

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled_weight_decay=False, maximize=False):
        if not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0 or eps < 0.0 or weight_decay < 0.0:
            raise ValueError('hyperseg_amd.training.Adam: invalid hyper-parameters')
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay,
                                      decoupled_weight_decay=bool(decoupled_weight_decay), maximize=bool(maximize)))

    @torch.no_grad()
    def step(self, closure=None):
        import ctypes as C
        from . import _hip
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        # set by torch.amp.GradScaler.step for the duration of this call (grad_scale is None after scaler.unscale_(self))
        found_inf, grad_scale = getattr(self, 'found_inf', None), getattr(self, 'grad_scale', None)
        for group in self.param_groups:
            ps = [p for p in group['params'] if p.grad is not None]
            if not ps:
                continue
            for p in ps:
                if not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() and p.grad.dtype == torch.float32
                        and not p.grad.is_sparse and p.grad.device == p.device):
                    raise NotImplementedError('hyperseg_amd.training.Adam: contiguous fp32 CUDA parameters with dense fp32 gradients only')
            dev = ps[0].device
            for lo in range(0, len(ps), 48):                                   # hs_adam_step takes up to 48 tensors per launch
                chunk = ps[lo:lo + 48]
                for p in chunk:
                    st = self.state[p]
                    if not st:
                        st['exp_avg'] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                        st['exp_avg_sq'] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                n = len(chunk)
                numel = (C.c_int64 * n)(*[p.numel() for p in chunk])
                key = f'_hs_steps_{lo}'
                sig = tuple(p.numel() for p in chunk)
                held = group.get(key)
                if held is None:
                    blocks = int(_hip.lib.hs_adam_blocks(numel, n))
                    if blocks <= 0:
                        raise NotImplementedError('hyperseg_amd.training.Adam: parameter list not covered by hs_adam_step')
                    # a loaded state (ours or a torch.optim.Adam checkpoint, train.py:227) carries the steps taken as state[p]['step']:
                    # the bias corrections must continue from there, not restart at t = 1 on warm moments
                    seeds = {float(self.state[p]['step']) for p in chunk if 'step' in self.state[p]}
                    if len(seeds) > 1:
                        raise NotImplementedError('hyperseg_amd.training.Adam: the parameters of one launch must share one step count')
                    held = group[key] = (sig, torch.full((blocks,), seeds.pop() if seeds else 0.0, device=dev, dtype=torch.float32))
                elif held[0] != sig:
                    raise RuntimeError('hyperseg_amd.training.Adam: the set of parameters with gradients changed between steps')
                elif held[1].device != dev:
                    raise RuntimeError('hyperseg_amd.training.Adam: the step words live on another device than the parameters')
                chunks = self.__dict__.setdefault('_hs_chunks', {})
                for p in chunk:
                    chunks[p] = (id(group), key)
                grads = [p.grad if p.grad.is_contiguous() else p.grad.contiguous() for p in chunk]
                arr = lambda ts: (C.c_void_p * n)(*[t.data_ptr() for t in ts])      # noqa: E731
                lr = group['lr']
                lr_dev = lr if isinstance(lr, torch.Tensor) and lr.is_cuda else None
                if lr_dev is not None and (lr_dev.dtype != torch.float32 or lr_dev.numel() != 1):
                    raise NotImplementedError('hyperseg_amd.training.Adam: a device learning rate must be one fp32 element')
                args = (arr(chunk), arr(grads), arr([self.state[p]['exp_avg'] for p in chunk]), arr([self.state[p]['exp_avg_sq'] for p in chunk]),
                        numel, n, lr_dev.data_ptr() if lr_dev is not None else None, 0.0 if lr_dev is not None else float(lr),
                        float(group['betas'][0]), float(group['betas'][1]), float(group['eps']), float(group['weight_decay']),
                        int(group['decoupled_weight_decay']), int(group['maximize']), held[1].data_ptr())
                if found_inf is None:
                    with _hip.device_scope(dev):
                        status = _hip.lib.hs_adam_step(*args, _hip.stream_ptr(dev))
                    _hip.check(status, 'hs_adam_step')
                    continue
                inf_dev = _amp_word(found_inf, dev)
                scale_dev = _amp_word(grad_scale, dev) if grad_scale is not None else None
                with _hip.device_scope(dev):
                    status = _hip.lib.hs_adam_step_amp(*args, scale_dev.data_ptr() if scale_dev is not None else None, inf_dev.data_ptr(),
                                                       _hip.stream_ptr(dev))
                _hip.check(status, 'hs_adam_step_amp')
                if grad_scale is not None:
                    for p, g in zip(chunk, grads):
                        if g is not p.grad:                                        # a non-contiguous gradient: the unscaled copy goes back
                            p.grad.copy_(g)
        return loss

    def _detached_step_words(self):
        """Removes the per-workgroup step words from the param groups (they are launch-layout state, not checkpoint state) and returns
        what it removed plus the count each one holds."""
        removed, counts = [], {}
        for g in self.param_groups:
            for k in [k for k in g if isinstance(k, str) and k.startswith('_hs_steps_')]:
                held = g.pop(k)
                removed.append((g, k, held))
                counts[(id(g), k)] = float(held[1][0].item())
        return removed, counts

    def state_dict(self):
        """torch.optim.Adam's checkpoint format: per-parameter ``step`` / ``exp_avg`` / ``exp_avg_sq``, param groups without the device
        step words -- loadable by torch.optim.Adam and by this class on any device (synchronises: reads the step count)."""
        removed, counts = self._detached_step_words()
        try:
            for p, where in self.__dict__.get('_hs_chunks', {}).items():
                if where in counts and self.state.get(p):
                    self.state[p]['step'] = torch.tensor(counts[where], dtype=torch.float32)
            return super().state_dict()
        finally:
            for g, k, held in removed:
                g[k] = held

    def load_state_dict(self, state_dict):
        """Accepts this class' checkpoints and torch.optim.Adam's (hyperseg/train.py:227 resumes from one): moments go to the
        parameters' device (torch does that), the step count is re-seeded onto the device by the next step() from ``state[p]['step']``."""
        super().load_state_dict(state_dict)
        for g in self.param_groups:                                              # step words of an older checkpoint format: never trusted,
            for k in [k for k in g if isinstance(k, str) and k.startswith('_hs_steps_')]:      # they may sit on the wrong device
                held = g.pop(k)
                try:
                    count = float(held[1].reshape(-1)[0])
                except Exception:                                                # noqa: BLE001
                    continue
                for p in g['params']:
                    if self.state.get(p) and 'step' not in self.state[p]:
                        self.state[p]['step'] = torch.tensor(count, dtype=torch.float32)
        self.__dict__['_hs_chunks'] = {}

    def steps_taken(self, group=0):
        """The step count of a group as the device holds it (synchronises)."""
        held = self.param_groups[group].get('_hs_steps_0')
        return 0 if held is None else int(held[1][0].item())


def _amp_word(t, dev):
    """A GradScaler's one-element scale / found-inf tensor as an fp32 word on ``dev`` (no host read)."""
    if t.dtype != torch.float32 or t.device != dev:
        t = t.to(device=dev, dtype=torch.float32, non_blocking=True)
    if t.numel() != 1:
        raise ValueError(f'hyperseg_amd.training.Adam: GradScaler tensors must hold one element, got {tuple(t.shape)}')
    return t.contiguous()


def train_step(model, criterion, optimizer, scheduler, x, target):
    """One optimisation step; returns (loss, prediction).  ``model`` is any callable producing (N, C, h, w) logits."""
    pred = model(x)
    if pred.shape[2:] != target.shape[1:]:
        pred = F.interpolate(pred, size=target.shape[1:], mode='bilinear')
    loss = criterion(pred, target)
    optimizer.zero_grad()
    loss.backward()
    optimizer.step()
    if scheduler is not None:
        scheduler.step()
    return loss.detach(), pred.detach()


def _flat_tensors(obj):
    if isinstance(obj, torch.Tensor):
        return [obj]
    if isinstance(obj, (list, tuple)):
        return [t for o in obj for t in _flat_tensors(o)]
    return []


class GraphedTrainStep:
    """forward + loss + backward + optimizer step of a fixed-shape batch as ONE HIP graph (the training-side counterpart of
    utils.inference.GraphedModel).  An eager config-5 decoder step is ~300 launches whose host side (4.8 ms) is longer than their GPU
    time (3.4 ms): replaying the captured step removes the difference.

    ``model(*inputs)`` -> logits, ``criterion(logits, target)`` -> scalar.  ``inputs`` (tensors or nested lists of tensors) and
    ``target`` given here are the STATIC buffers the graph reads: ``step(inputs, target)`` copies new data into them and replays.
    The optimizer must be capturable (``torch.optim.Adam(..., capturable=True)``: its step count lives on the device); a learning-rate
    schedule changes ``param_group['lr']`` in place if it is a tensor (``lr=torch.tensor(1e-3, device=...)``).  BatchNorm statistics,
    parameters and optimizer state are updated by every replay exactly as by an eager step.

    One requirement beyond PyTorch's usual ones (static shapes, warm-up before capture): NO autograd graph of an earlier eager step
    may still be alive when this object is built -- e.g. a ``loss`` variable that still carries its ``grad_fn``.  Such a graph keeps the
    parameters' gradient accumulators alive, and those stay bound to the stream of the eager steps; the captured backward would then
    hop to that (non-capturing) stream and hipStreamEndCapture dies on ROCm 7.2 (bisected in round 3: ``del loss`` is the whole fix).
    Keep ``loss.detach()`` / ``float(loss)`` instead.

    ``scaler``: a ``torch.amp.GradScaler`` -- the captured step is then the whole mixed-precision step, ``scaler.scale(loss).backward()``,
    the inf check, ``scaler.step(optimizer)`` and ``scaler.update()``, with the scale and growth tracker updated on the device by every
    replay.  It needs an optimizer that takes the scaler's protocol without a host read (``hyperseg_amd.training.Adam``, or torch's
    ``fused=True`` Adam); the model runs under whatever autocast the caller wraps ``model`` in.

    ``criterion.score`` (``BootstrappedCrossEntropyLoss.score``, a ``ConfusionMatrix``): the loss launch of every replay adds the batch's
    counts to ``score.mat``.  The matrix exists before the capture (the warm-up creates it) and is never replaced: the graph holds its
    address.  The warm-up's steps are counted -- they are real optimiser steps on real data -- so after construction the matrix holds
    ``warmup`` batches (the capture pass records, it does not execute).  ``ConfusionMatrix.reset()`` zeroes the matrix in place, so a
    reset between epochs is safe; assigning a new tensor to ``score.mat`` is not."""

    def __init__(self, model, criterion, optimizer, inputs, target, warmup=3, scaler=None):
        self.model, self.criterion, self.optimizer = model, criterion, optimizer
        self.scaler = scaler
        if scaler is not None and not getattr(optimizer, '_step_supports_amp_scaling', False):
            raise ValueError('GraphedTrainStep(scaler=...): the optimizer must implement the GradScaler protocol '
                             '(_step_supports_amp_scaling); a generic optimizer reads found_inf on the host in every step')
        self.inputs, self.target = inputs, target
        self._unit = None
        dev = target.device
        if dev.type != 'cuda':
            raise ValueError('GraphedTrainStep needs CUDA tensors')
        self._static_in = _flat_tensors(inputs) + [target]
        if warmup < 1 and not optimizer.state:
            # the optimizer creates its state (moments, step count) on first use: inside a capture those zero fills become graph nodes
            # and EVERY replay would reset the moments
            raise ValueError('GraphedTrainStep: warmup >= 1 is required while the optimizer has no state yet')
        score = getattr(criterion, 'score', None)
        if score is not None:
            score.matrix(dev)                               # created here at the latest: a zero fill inside the capture would be replayed
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):                       # first calls allocate, tune and set kernel attributes: not capturable
            for _ in range(warmup):
                self._eager()
        torch.cuda.current_stream(dev).wait_stream(side)
        # gradients left by earlier eager steps (the caller's or the warm-up's) would be FREED inside the capture by zero_grad -- blocks
        # of another stream's pool released while a global-mode capture is open bring hipStreamEndCapture down on ROCm 7.2: drop them now
        self.optimizer.zero_grad(set_to_none=True)
        torch.cuda.synchronize(dev)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.loss, self.pred = self._eager()

    def _eager(self):
        self.optimizer.zero_grad(set_to_none=True)
        pred = self.model(*self.inputs) if isinstance(self.inputs, (list, tuple)) else self.model(self.inputs)
        if pred.shape[2:] != self.target.shape[1:]:
            pred = F.interpolate(pred, size=self.target.shape[1:], mode='bilinear')
        loss = self.criterion(pred, self.target)
        # the root gradient is a tensor this object owns (made in the warm-up, outside the capture): `loss.backward()` alone makes autograd
        # fill a fresh ones_like(loss) -- one more launch in every replay (round 6: 82 -> 81 per config-5 step)
        root = loss if self.scaler is None else self.scaler.scale(loss)
        if self._unit is None or self._unit.shape != root.shape or self._unit.dtype != root.dtype:
            self._unit = torch.ones_like(root)
        root.backward(self._unit)
        if self.scaler is None:
            self.optimizer.step()
        else:
            self.scaler.step(self.optimizer)              # the inf check, then the optimizer's own skip / unscale on the device
            self.scaler.update()
        return loss.detach(), pred.detach()

    def step(self, inputs=None, target=None):
        """Copies ``inputs`` / ``target`` (same structure and shapes; None = keep what is in the static buffers) and replays.
        Returns the static (loss, prediction) tensors: valid until the next call."""
        if inputs is not None or target is not None:
            new = (_flat_tensors(inputs) if inputs is not None else self._static_in[:-1]) + [target if target is not None else self.target]
            if len(new) != len(self._static_in):
                raise ValueError('inputs do not match the captured structure')
            for dst, src in zip(self._static_in, new):
                if dst is not src:
                    dst.copy_(src, non_blocking=True)
        self.graph.replay()
        # the replay moved every parameter and BatchNorm buffer WITHOUT bumping a tensor version: the eval-route caches keyed on
        # versions (folded BN, transposed / packed signal2weights weights, split GEMM weights) must not survive it
        from .functional import bump_weights_epoch
        bump_weights_epoch()
        return self.loss, self.pred


def device_augment(frames_u8, labels, scale, crop, offset, hflip, norm, lbl_fill=255, fill=(0, 0, 0), jitter=None):
    """The reference's train-time chain RandomResize -> RandomCrop(pad_if_needed) -> RandomHorizontalFlip -> ToTensor -> Normalize
    (hyperseg/datasets/seg_transforms.py:224-334) for GIVEN parameters, on the device: per sample one ``functional.frame_resize``
    launch (bicubic, Pillow's bytes, looked up in ``norm``'s table) and one ``functional.label_resize`` launch (nearest), each
    producing only the crop.  Drawing the parameters stays with the caller.

    ``frames_u8``: uint8 (B, H, W, 3) / (B, 3, H, W) as ``norm.layout`` says; ``labels``: (B, H, W) uint8 or int64.  ``scale``: the
    resize factor -- the resized size is ``round((H, W) * scale)``, numpy's rounding as the reference's; ``crop``: (h, w) of the result;
    ``offset``: (top, left) of the crop IN THE RESIZED IMAGE, signed -- what lies outside is padding: ``fill`` for the frame (before
    normalisation, as the reference pads the PIL image) and ``lbl_fill`` for the label; ``hflip``: flip the crop.  ``scale``,
    ``offset`` and ``hflip`` are one value for the batch or a sequence of B.  Returns ``(image float32 (B, 3, h, w), label int64
    (B, h, w))``.  CPU tensors take ``utils.resample``'s CPU implementation: same values.

    ``jitter`` (a ``ColorJitterParams``, or a sequence of B; :func:`draw_color_jitter` draws one): torchvision's ``ColorJitter`` at the
    end of the image chain, as in the reference's Cityscapes HyperSeg-S config -- the resize launch then writes the uint8 crop (padding
    included: the contrast mean sees it, as it does on the padded PIL image) and ``functional.color_jitter`` produces the normalised
    image of the whole batch, Pillow's bytes through ``norm``'s table (``utils.jitter.color_jitter_cpu`` for CPU tensors).  ``None``:
    nothing changes."""
    import numpy as np
    from . import functional as HF
    from .utils import resample
    b, h, w = norm.frame_size(frames_u8)
    if not isinstance(labels, torch.Tensor) or tuple(labels.shape) != (b, h, w):
        raise ValueError(f'labels must be (B, H, W) = {(b, h, w)}, got {tuple(getattr(labels, "shape", ()))}')
    ch, cw = (int(s) for s in crop)

    def per_sample(v, scalar):
        return [v] * b if scalar(v) else list(v)
    scales = per_sample(scale, lambda v: not isinstance(v, (list, tuple)) and getattr(v, 'ndim', 0) == 0)
    offsets = per_sample(offset, lambda v: len(v) == 2 and not isinstance(v[0], (list, tuple)) and getattr(v[0], 'ndim', 0) == 0)
    flips = per_sample(hflip, lambda v: not isinstance(v, (list, tuple)) and getattr(v, 'ndim', 0) == 0)
    if not len(scales) == len(offsets) == len(flips) == b:
        raise ValueError('scale, offset and hflip take one value, or one per sample')
    image = torch.empty(b, 3, ch, cw, dtype=torch.float32, device=frames_u8.device)
    label = torch.empty(b, ch, cw, dtype=torch.int64, device=frames_u8.device)
    frames_u8, labels = frames_u8.contiguous(), labels.contiguous()
    dst, dst_norm = image, norm
    if jitter is not None:                                   # the resize writes the uint8 crop, the jitter normalises
        from .utils import jitter as J
        jitter = J.per_sample(jitter, b)
        dst_norm = None
        dst = torch.empty((b, ch, cw, 3) if norm.layout == 'hwc' else (b, 3, ch, cw), dtype=torch.uint8, device=frames_u8.device)
    for i in range(b):
        size = tuple(int(s) for s in np.round(np.array((h, w)) * float(scales[i])).astype(int))
        view = resample.ResizeView((ch, cw), tuple(int(o) for o in offsets[i]), bool(flips[i]), fill)
        if frames_u8.is_cuda:
            HF.frame_resize(frames_u8[i:i + 1], size, 'bicubic', norm.layout, view=view, norm=dst_norm, out=dst[i:i + 1])
            HF.label_resize(labels[i:i + 1], size, view=view, fill=lbl_fill, out=label[i:i + 1])
        else:
            dst[i:i + 1] = resample.frame_resize_cpu(frames_u8[i:i + 1], size, 'bicubic', norm.layout, view=view, norm=dst_norm)
            label[i:i + 1] = resample.label_resize_cpu(labels[i:i + 1], size, view=view, fill=lbl_fill, out_dtype=torch.int64)
    if jitter is not None:
        if dst.is_cuda:
            HF.color_jitter(dst, jitter, norm.layout, norm=norm, out=image)
        else:
            image = J.color_jitter_cpu(dst, jitter, norm.layout, norm=norm)
    return image, label


class BatchAugment:
    """:func:`device_augment` for training, where RandomResize draws a new scale for every sample: the same chain, the same bytes, in a
    fixed THREE launches per batch -- ``functional.resize_tables`` builds every sample's resize tables on the device, then
    ``functional.frame_resize_batch`` and ``functional.label_resize_batch`` resize the whole batch -- where ``device_augment`` builds four
    tables per new (in, out) pair on the host, uploads and keeps them, and launches twice per sample.  No host table build, no
    synchronisation, nothing cached; every per-sample parameter sits in one small device tensor that the kernels read when they run, so
    :meth:`run` can be captured once and replayed with new parameters.

    ``in_hw``: the frames' (H, W); ``crop``: (h, w) of the result; ``norm``: the ``InputNorm`` (its layout is the frames');
    ``scale_range``: (lo, hi) of the scales that will be asked for -- ``lo`` sizes the tables' rows (``utils.resample.ks_for``);
    ``filter``: the frames' filter (``device_augment`` is 'bicubic'); ``lbl_fill`` / ``fill``: the padding; ``batch``: the batch size, or
    None = the first call's.  The object owns the workspace, the ``params`` tensor (int32 (B, 6) = Hr, Wr, oy, ox, hflip, reserved) and a
    pinned staging buffer, all made at the first GPU call.  One object serves one stream at a time."""

    def __init__(self, in_hw, crop, norm, scale_range, filter='bicubic', lbl_fill=255, fill=(0, 0, 0), batch=None):
        from .utils import resample
        self.in_hw = tuple(int(s) for s in in_hw)
        self.crop = tuple(int(s) for s in crop)
        if len(self.in_hw) != 2 or len(self.crop) != 2 or min(self.in_hw + self.crop) < 1:
            raise ValueError(f'in_hw and crop must be two sizes >= 1, got {in_hw} and {crop}')
        lo, hi = (float(s) for s in scale_range)
        if not 0.0 < lo <= hi:
            raise ValueError(f'scale_range must be 0 < lo <= hi, got {scale_range}')
        if filter not in resample.FILTERS:
            raise ValueError(f'filter {filter!r}: expected one of {resample.FILTERS}')
        if batch is not None and int(batch) < 1:
            raise ValueError(f'batch must be >= 1, got {batch}')
        self.norm, self.scale_range, self.filter, self.lbl_fill, self.fill = norm, (lo, hi), filter, int(lbl_fill), fill
        self.batch = None if batch is None else int(batch)
        smallest = self._resized(lo)
        if min(smallest) < 1:
            raise ValueError(f'scale {lo} leaves nothing of {self.in_hw}')
        # ks_for is the rule; rounding the resized size down can make the true ratio a little larger than 1 / lo
        self.ks_max = max(resample.ks_for(filter, lo), *(resample.ksize_of(i, o, filter) for i, o in zip(self.in_hw, smallest)))
        self.params = self.tables = self._staging = self._copied = None

    def _resized(self, scale):
        import numpy as np
        return tuple(int(s) for s in np.round(np.array(self.in_hw) * float(scale)).astype(int))

    @property
    def status(self):
        """int32 (B,) on the device: 0, or the sum of ``functional.RESIZE_STATUS`` codes of a sample whose parameters the table launch
        declined (that sample is fill).  Reading it synchronises; the caller chooses when."""
        return None if self.tables is None else self.tables.status

    @property
    def workspace(self):
        return None if self.tables is None else self.tables.workspace

    def _check(self, frames_u8, labels):
        b, h, w = self.norm.frame_size(frames_u8)
        if (h, w) != self.in_hw:
            raise ValueError(f'frames are {(h, w)}, this BatchAugment was made for {self.in_hw}')
        if not isinstance(labels, torch.Tensor) or tuple(labels.shape) != (b, h, w) or labels.device != frames_u8.device:
            raise ValueError(f'labels must be (B, H, W) = {(b, h, w)} on {frames_u8.device}, got {tuple(getattr(labels, "shape", ()))}')
        if self.batch is None:
            self.batch = b
        if b != self.batch:
            raise ValueError(f'{b} frames, this BatchAugment holds batches of {self.batch}')
        return b

    def _on(self, device):
        from . import functional as HF
        if self.tables is None or self.params.device != device:
            words = HF.ResizeTables.words(self.batch, self.crop, self.ks_max)
            self.params = torch.zeros(self.batch, HF.RESIZE_PARAM_WORDS, dtype=torch.int32, device=device)
            self.tables = HF.ResizeTables.over(torch.zeros(words, dtype=torch.int32, device=device), self.batch, self.in_hw, self.crop, self.ks_max)
            self._staging = torch.zeros(self.batch, HF.RESIZE_PARAM_WORDS, dtype=torch.int32).pin_memory()
            self._copied = torch.cuda.Event()
            self.norm.table(device)

    def rows(self, scale, offset, hflip, batch=None):
        """The ``params`` rows of given augmentation parameters (each one value or a sequence of B, as ``device_augment``'s): a CPU int32
        (B, 6) tensor.  A scale outside ``scale_range`` raises ValueError."""
        b = self.batch if batch is None else batch

        def per_sample(v, scalar):
            return [v] * b if scalar(v) else list(v)
        scales = per_sample(scale, lambda v: not isinstance(v, (list, tuple)) and getattr(v, 'ndim', 0) == 0)
        offsets = per_sample(offset, lambda v: len(v) == 2 and not isinstance(v[0], (list, tuple)) and getattr(v[0], 'ndim', 0) == 0)
        flips = per_sample(hflip, lambda v: not isinstance(v, (list, tuple)) and getattr(v, 'ndim', 0) == 0)
        if not len(scales) == len(offsets) == len(flips) == b:
            raise ValueError('scale, offset and hflip take one value, or one per sample')
        lo, hi = self.scale_range
        rows = []
        for s, o, f in zip(scales, offsets, flips):
            if not lo <= float(s) <= hi:
                raise ValueError(f'scale {float(s)} is outside scale_range {self.scale_range}')
            rows.append(self._resized(s) + (int(o[0]), int(o[1]), int(bool(f)), 0))
        return torch.tensor(rows, dtype=torch.int32)

    def _cpu(self, frames_u8, labels, rows, jitter):
        from .utils import resample
        norm, (ch, cw) = self.norm, self.crop
        b = frames_u8.shape[0]
        uint8_shape = (b, ch, cw, 3) if norm.layout == 'hwc' else (b, 3, ch, cw)
        dst = torch.empty(uint8_shape, dtype=torch.uint8) if jitter is not None else torch.empty(b, 3, ch, cw, dtype=torch.float32)
        label = torch.empty(b, ch, cw, dtype=torch.int64)
        for i, (hr, wr, oy, ox, flip, _) in enumerate(rows.tolist()):
            view = resample.ResizeView((ch, cw), (oy, ox), bool(flip), self.fill)
            dst[i:i + 1] = resample.frame_resize_cpu(frames_u8[i:i + 1], (hr, wr), self.filter, norm.layout, view=view,
                                                     norm=None if jitter is not None else norm)
            label[i:i + 1] = resample.label_resize_cpu(labels[i:i + 1], (hr, wr), view=view, fill=self.lbl_fill, out_dtype=torch.int64)
        if jitter is not None:
            from .utils import jitter as J
            dst = J.color_jitter_cpu(dst, J.per_sample(jitter, b), norm.layout, norm=norm)
        return dst, label

    def _launch(self, frames_u8, labels, params, dst, dst_norm, label):
        from . import functional as HF
        tables = HF.resize_tables(params, self.in_hw, self.crop, self.filter, self.ks_max, workspace=self.tables.workspace)
        HF.frame_resize_batch(frames_u8, params, tables, self.norm.layout, fill=self.fill, norm=dst_norm, out=dst)
        HF.label_resize_batch(labels, params, tables, fill=self.lbl_fill, out=label)

    def run(self, frames_u8, labels, params=None, out=None):
        """The three launches over whatever ``self.params`` (or the given device tensor of that shape) holds when they RUN: no host
        state is read or written, so a captured ``run`` replays with the parameters last copied into the tensor.  ``frames_u8`` and
        ``labels`` must be contiguous.  ``out``: ``(image, label)`` to write into.  Returns ``(image float32 (B, 3, h, w), label int64
        (B, h, w))``.  Nothing checks the parameters on the host: a row the table launch declines sets :attr:`status`."""
        b = self._check(frames_u8, labels)
        if not frames_u8.is_cuda:
            rows = self.params if params is None else params
            if rows is None:
                raise ValueError('run on CPU tensors needs params')
            return self._cpu(frames_u8, labels, rows, None)
        self._on(frames_u8.device)
        params = self.params if params is None else params
        ch, cw = self.crop
        if out is None:
            image = torch.empty(b, 3, ch, cw, dtype=torch.float32, device=frames_u8.device)
            label = torch.empty(b, ch, cw, dtype=torch.int64, device=frames_u8.device)
        else:
            image, label = out
        self._launch(frames_u8, labels, params, image, self.norm, label)
        return image, label

    def __call__(self, frames_u8, labels, scale, offset, hflip, jitter=None):
        """``device_augment(frames_u8, labels, scale, crop, offset, hflip, norm, lbl_fill, fill, jitter)``: same arguments, same
        results.  The resized sizes are ``round((H, W) * scale)`` on the host; the parameters go up in one non-blocking copy."""
        b = self._check(frames_u8, labels)
        rows = self.rows(scale, offset, hflip, b)                # raises before any launch
        if not frames_u8.is_cuda:
            return self._cpu(frames_u8, labels, rows, jitter)
        from . import functional as HF
        self._on(frames_u8.device)
        frames_u8, labels = frames_u8.contiguous(), labels.contiguous()
        self._copied.synchronize()                               # the previous call's copy has left the staging buffer
        self._staging.copy_(rows)
        self.params.copy_(self._staging, non_blocking=True)
        self._copied.record()
        ch, cw = self.crop
        image = torch.empty(b, 3, ch, cw, dtype=torch.float32, device=frames_u8.device)
        label = torch.empty(b, ch, cw, dtype=torch.int64, device=frames_u8.device)
        if jitter is None:
            self._launch(frames_u8, labels, self.params, image, self.norm, label)
        else:                                                    # the resize writes the uint8 crop, the jitter normalises
            from .utils import jitter as J
            jitter = J.per_sample(jitter, b)
            layout = self.norm.layout
            crop_u8 = torch.empty((b, ch, cw, 3) if layout == 'hwc' else (b, 3, ch, cw), dtype=torch.uint8, device=frames_u8.device)
            self._launch(frames_u8, labels, self.params, crop_u8, None, label)
            HF.color_jitter(crop_u8, jitter, layout, norm=self.norm, out=image)
        return image, label


def device_augment_voc(frames, labels, hflip, jitter, scale, angle, pad, norm, fill=(0, 0, 0), lbl_fill=255, rotate_fill=(0, 0, 0),
                       lbl_rotate_fill=0):
    """The reference's VOC-SBD train chain RandomHorizontalFlip -> ColorJitter -> RandomResize -> RandomRotation -> ConstantPad -> ToTensor
    -> Normalize (configs/train/vocsbd_efficientnet_b3_hyperseg-l.py:21-24, hyperseg/datasets/seg_transforms.py) for GIVEN parameters, on
    the device, Pillow's bytes at every stage.  Drawing the parameters stays with the caller, as in :func:`device_augment`.

    ``frames``: a uint8 tensor (B, H, W, 3) / (B, 3, H, W) as ``norm.layout`` says, or a sequence of B such frames without the batch
    dimension, each of its own size (VOC images differ in size); ``labels``: (B, H, W) uint8 or int64, or a sequence likewise.
    ``hflip``, ``scale``, ``angle``: one value for the batch or a sequence of B; ``jitter``: a ``ColorJitterParams``, a sequence of B, or
    None.  Per sample, in the reference's order:
      * the flip -- an identity-size ``functional.frame_resize`` / ``label_resize`` whose view is flipped.  It is NOT folded into the
        resize: Pillow's NEAREST index table is not symmetric (a 2:1 reduction reads source 1, 3, ..., the mirror image would read 0, 2,
        ...), so resizing and then flipping is another label than the reference's;
      * ``functional.color_jitter``, uint8 out (skipped when ``jitter`` is None; it commutes with the flip exactly -- per-pixel
        operations and one mean over the whole frame -- and runs first so that it reads the caller's frame);
      * ``functional.frame_resize`` (bicubic) / ``label_resize`` to ``round((H, W) * scale)``, numpy's rounding as the reference's, uint8
        out.  ``scale`` None or 1.0: RandomResize did not fire, nothing is resampled;
      * ``functional.frame_rotate`` with ``size=(pad, pad)`` and ``norm``, writing the sample's slice of the batch; ``label_rotate``
        likewise, int64 out.
    Fills, defaults from the reference's config: ``rotate_fill`` (0, 0, 0) and ``lbl_rotate_fill`` 0 -- ``RandomRotation(30.)`` rotates
    frame AND label with its ``fill`` (seg_transforms.py:424), not with ``lbl_fill``; ``fill`` 0 and ``lbl_fill`` 255 --
    ``ConstantPad(512, lbl_fill=255)``.  A resized image larger than ``pad`` in either dimension raises ValueError (the reference would
    return a ragged batch).  Returns ``(image float32 (B, 3, pad, pad), label int64 (B, pad, pad))``.  CPU tensors take the CPU
    implementations (``utils.jitter`` / ``utils.resample`` / ``utils.rotate``): same values."""
    import numpy as np
    from . import functional as HF
    from .utils import jitter as J
    from .utils import resample, rotate
    hwc = norm.layout == 'hwc'
    if isinstance(frames, torch.Tensor):
        norm.frame_size(frames)
        frames = [frames[i] for i in range(frames.shape[0])]
    if isinstance(labels, torch.Tensor):
        labels = [labels[i] for i in range(labels.shape[0])]
    frames, labels = list(frames), list(labels)
    b = len(frames)
    if b == 0 or len(labels) != b:
        raise ValueError(f'frames and labels must hold the same number of samples (>= 1), got {b} and {len(labels)}')
    pad = int(pad)

    def per_sample(v):
        seq = list(v) if isinstance(v, (list, tuple)) or getattr(v, 'ndim', 0) > 0 else [v] * b
        if len(seq) != b:
            raise ValueError('hflip, scale and angle take one value, or one per sample')
        return seq
    flips, scales, angles = per_sample(hflip), per_sample(scale), rotate.per_sample(angle, b)
    jitters = None if jitter is None else J.per_sample(jitter, b)
    device = frames[0].device
    on_gpu = device.type == 'cuda'
    plan = []
    for i in range(b):
        x, t = frames[i], labels[i]
        if not isinstance(x, torch.Tensor) or x.dtype != torch.uint8 or x.dim() != 3 or x.shape[2 if hwc else 0] != 3:
            raise ValueError(f'frame {i} must be uint8 {"(H, W, 3)" if hwc else "(3, H, W)"}, got '
                             f'{getattr(x, "dtype", type(x))} {tuple(getattr(x, "shape", ()))}')
        h, w = (int(s) for s in (x.shape[:2] if hwc else x.shape[1:]))
        if not isinstance(t, torch.Tensor) or t.dtype not in (torch.uint8, torch.int64) or tuple(t.shape) != (h, w):
            raise ValueError(f'label {i} must be uint8 or int64 {(h, w)}, got {getattr(t, "dtype", type(t))} {tuple(getattr(t, "shape", ()))}')
        if x.device != device or t.device != device:
            raise ValueError(f'sample {i} is on {x.device} / {t.device}, the first frame on {device}')
        size = (h, w)
        if scales[i] is not None and float(scales[i]) != 1.0:
            size = tuple(int(s) for s in np.round(np.array((h, w)) * float(scales[i])).astype(int))
        if min(size) < 1:
            raise ValueError(f'sample {i}: scale {scales[i]} leaves nothing of {(h, w)}')
        if size[0] > pad or size[1] > pad:
            raise ValueError(f'sample {i}: the resized image {size} exceeds pad {pad}')
        rotate._check_hw(h, w)
        plan.append(((h, w), size))
    image = torch.empty(b, 3, pad, pad, dtype=torch.float32, device=device)
    label = torch.empty(b, pad, pad, dtype=torch.int64, device=device)
    mirror = resample.ResizeView
    for i, ((h, w), size) in enumerate(plan):
        x, t = frames[i].contiguous()[None], labels[i].contiguous()[None]
        if on_gpu:
            if jitters is not None:
                x = HF.color_jitter(x, jitters[i], norm.layout)
            if flips[i]:
                x = HF.frame_resize(x, (h, w), 'bicubic', norm.layout, view=mirror((h, w), (0, 0), True))
                t = HF.label_resize(t, (h, w), view=mirror((h, w), (0, 0), True))
            if size != (h, w):
                x = HF.frame_resize(x, size, 'bicubic', norm.layout)
                t = HF.label_resize(t, size)
            HF.frame_rotate(x, angles[i], norm.layout, (pad, pad), rotate_fill, fill, norm=norm, out=image[i:i + 1])
            HF.label_rotate(t, angles[i], (pad, pad), lbl_rotate_fill, lbl_fill, out=label[i:i + 1])
        else:
            if jitters is not None:
                x = J.color_jitter_cpu(x, jitters[i], norm.layout)
            if flips[i]:
                x, t = x.flip(2 if hwc else 3), t.flip(2)
            if size != (h, w):
                x = resample.frame_resize_cpu(x, size, 'bicubic', norm.layout)
                t = resample.label_resize_cpu(t, size)
            image[i:i + 1] = rotate.frame_rotate_cpu(x, angles[i], norm.layout, (pad, pad), rotate_fill, fill, norm=norm)
            label[i:i + 1] = rotate.label_rotate_cpu(t, angles[i], (pad, pad), lbl_rotate_fill, lbl_fill, out_dtype=torch.int64)
    return image, label


VOCBatchParams = collections.namedtuple('VOCBatchParams', 'rows matrices fixed jitter jitters contrast')
VOCBatchParams.__doc__ = """The per-sample parameters of one :class:`BatchAugmentVOC` batch as the kernels read them, CPU tensors: ``rows``
int32 (B, 8) = h, w, Hr, Wr, hflip, 3 reserved; ``matrices`` float64 (B, 6) and ``fixed`` int32 (B, 6), the rotation of the (Hr, Wr) image
for the frame and the label; ``jitter`` int32 (B, 8), the colour-jitter records (all zero = leave the sample as it is); ``jitters`` the
``ColorJitterParams`` they were made from, or None; ``contrast``: some record names contrast."""


class BatchAugmentVOC:
    """:func:`device_augment_voc` for training batches, where the samples differ in size and every one draws its own flip, jitter, scale
    and angle: the same chain, the same bytes, in a FIXED number of launches per batch -- 5 (resize tables, frame and label resize, frame
    and label rotate), 6 with a colour jitter that has no contrast, 8 with one that has (the clear and the mean pass) -- where
    ``device_augment_voc`` makes up to nine launches per sample, builds resize tables on the host for every new (in, out) pair, uploads
    them behind a synchronisation and keeps them.  No host table build, no synchronisation, nothing cached; every per-sample parameter
    sits in a device tensor that the kernels read when they run, so :meth:`run` can be captured once and replayed with new parameters.

    A ragged batch is a canvas plus extents, what a padding collate function produces: ``frames`` uint8 (B, Hm, Wm, 3) / (B, 3, Hm, Wm) as
    ``norm.layout`` says, ``labels`` (B, Hm, Wm) uint8 or int64 (values 0..255: the intermediate label is a byte), and ``sizes``, the
    (h, w) of the top-left region of each sample that is the image.  What lies outside the region is never read into a result.

    ``canvas_hw``: (Hm, Wm); ``pad``: the side of the square result, also of the intermediate canvas the resized images go to; ``norm``: the
    ``InputNorm``; ``scale_range``: (lo, hi) of the scales that will be asked for other than None / 1.0 -- ``lo`` sizes the tables' rows
    (``utils.resample.ks_for``, raised to the widest row any extent of the canvas needs at ``lo``); the fills as ``device_augment_voc``'s;
    ``batch``: the batch size, or None = the first call's.  The object owns the workspace, the two intermediate canvases, the jittered
    canvas, the parameter tensors (:attr:`params`, views of one buffer) and one pinned staging buffer, all made at the first GPU call.  One
    object serves one stream at a time."""

    WORDS = 12 + 8 + 6 + 8                   # int32 words per sample of the parameter buffer: matrices (float64), rows, fixed, jitter

    def __init__(self, canvas_hw, pad, norm, scale_range=(0.25, 0.9), lbl_fill=255, fill=(0, 0, 0), rotate_fill=(0, 0, 0), lbl_rotate_fill=0,
                 batch=None):
        import numpy as np
        from . import functional as HF
        from .utils import resample, rotate
        self.canvas_hw = tuple(int(s) for s in canvas_hw)
        self.pad = int(pad)
        if len(self.canvas_hw) != 2 or not 1 <= min(self.canvas_hw) or max(self.canvas_hw) > HF.RAGGED_MAX_DIM or not 1 <= self.pad <= HF.RAGGED_MAX_DIM:
            raise ValueError(f'canvas_hw and pad must be sizes in 1..{HF.RAGGED_MAX_DIM}, got {canvas_hw} and {pad}')
        lo, hi = (float(s) for s in scale_range)
        if not 0.0 < lo <= hi:
            raise ValueError(f'scale_range must be 0 < lo <= hi, got {scale_range}')
        if batch is not None and int(batch) < 1:
            raise ValueError(f'batch must be >= 1, got {batch}')
        self.norm, self.scale_range, self.lbl_fill, self.lbl_rotate_fill = norm, (lo, hi), int(lbl_fill), int(lbl_rotate_fill)
        self.fill, self.rotate_fill = rotate.check_fill(fill), rotate.check_fill(rotate_fill, 'rotate_fill')
        self.batch = None if batch is None else int(batch)

        def widest(n):
            """The most taps a row can hold for any extent 1..n at scale lo: min(ksize, extent), as the table launch counts them."""
            i = np.arange(1, n + 1)
            o = np.round(i * lo).astype(int)
            i, o = i[o >= 1], o[o >= 1]
            ks = np.where(i == o, 1, np.ceil(2.0 * np.maximum(i / np.maximum(o, 1), 1.0)).astype(int) * 2 + 1)
            return int(np.minimum(ks, i).max()) if len(i) else 1
        # ks_for is the rule; rounding the resized size can make the true ratio larger than 1 / lo
        self.ks_max = max(resample.ks_for('bicubic', lo), widest(self.canvas_hw[0]), widest(self.canvas_hw[1]))
        self.params = self.tables = self.buffer = self._staging = self._copied = None
        self._mid = self._mid_label = self._jittered = self._sums = None

    @property
    def status(self):
        """int32 (B,) on the device: 0, or the sum of ``functional.RAGGED_STATUS`` codes of a sample whose parameters the table launch
        declined (that sample is pad fill).  Reading it synchronises; the caller chooses when."""
        return None if self.tables is None else self.tables.status

    @property
    def workspace(self):
        return None if self.tables is None else self.tables.workspace

    def _check(self, frames, labels):
        b, h, w = self.norm.frame_size(frames)
        if (h, w) != self.canvas_hw:
            raise ValueError(f'the canvas is {(h, w)}, this BatchAugmentVOC was made for {self.canvas_hw}')
        if (not isinstance(labels, torch.Tensor) or labels.dtype not in (torch.uint8, torch.int64) or tuple(labels.shape) != (b, h, w)
                or labels.device != frames.device):
            raise ValueError(f'labels must be uint8 or int64 (B, H, W) = {(b, h, w)} on {frames.device}, got '
                             f'{getattr(labels, "dtype", type(labels))} {tuple(getattr(labels, "shape", ()))} on {getattr(labels, "device", None)}')
        if self.batch is None:
            self.batch = b
        if b != self.batch:
            raise ValueError(f'{b} frames, this BatchAugmentVOC holds batches of {self.batch}')
        return b

    def _on(self, device):
        from . import functional as HF
        if self.tables is None or self.buffer.device != device:
            b, mid, hwc = self.batch, (self.pad, self.pad), self.norm.layout == 'hwc'
            self.buffer = torch.zeros(b * self.WORDS, dtype=torch.int32, device=device)
            self.params = self._views(self.buffer)
            self._staging = torch.zeros(b * self.WORDS, dtype=torch.int32).pin_memory()
            self._copied = torch.cuda.Event()
            words = HF.RaggedTables.words(b, mid, self.ks_max)
            self.tables = HF.RaggedTables.over(torch.zeros(words, dtype=torch.int32, device=device), b, self.canvas_hw, mid, self.ks_max)
            self._mid = torch.zeros((b, self.pad, self.pad, 3) if hwc else (b, 3, self.pad, self.pad), dtype=torch.uint8, device=device)
            self._mid_label = torch.zeros(b, self.pad, self.pad, dtype=torch.uint8, device=device)
            self._jittered = torch.zeros((b,) + self.canvas_hw + (3,) if hwc else (b, 3) + self.canvas_hw, dtype=torch.uint8, device=device)
            self._sums = torch.zeros(b, dtype=torch.int64, device=device)
            self.norm.table(device)

    def _views(self, buffer):
        """(rows, matrices, fixed, jitter) over one int32 buffer of ``B * WORDS`` words; the float64 matrices come first (alignment)."""
        b = self.batch
        m, r, f, j = torch.split(buffer, (12 * b, 8 * b, 6 * b, 8 * b))
        return VOCBatchParams(r.view(b, 8), m.view(torch.float64).view(b, 6), f.view(b, 6), j.view(b, 8), None, True)

    def rows(self, sizes, hflip, jitter, scale, angle, batch=None):
        """The parameters of one batch (each of ``hflip``, ``scale``, ``angle`` one value or a sequence of B; ``jitter`` a
        ``ColorJitterParams``, a sequence of B or None; ``sizes`` B pairs (h, w)) as a :class:`VOCBatchParams` of CPU tensors.  Raises
        ValueError for everything ``device_augment_voc`` refuses -- an extent outside the canvas, a scale that leaves nothing, a resized image
        larger than ``pad`` -- and for a scale outside ``scale_range`` other than None / 1.0."""
        import numpy as np
        from .utils import jitter as J
        from .utils import rotate
        b = self.batch if batch is None else batch
        sizes = sizes.tolist() if isinstance(sizes, (torch.Tensor, np.ndarray)) else list(sizes)

        def per_sample(v):
            seq = list(v) if isinstance(v, (list, tuple)) or getattr(v, 'ndim', 0) > 0 else [v] * b
            if len(seq) != b:
                raise ValueError('hflip, scale and angle take one value, or one per sample')
            return seq
        if len(sizes) != b or any(len(s) != 2 for s in sizes):
            raise ValueError(f'sizes must hold one (h, w) per sample ({b}), got {len(sizes)}')
        flips, scales, angles = per_sample(hflip), per_sample(scale), rotate.per_sample(angle, b)
        jitters = None if jitter is None else J.per_sample(jitter, b)
        lo, hi = self.scale_range
        rows, mats, fixed = [], [], []
        for i, (h, w) in enumerate(sizes):
            h, w = int(h), int(w)
            if not (1 <= h <= self.canvas_hw[0] and 1 <= w <= self.canvas_hw[1]):
                raise ValueError(f'sample {i}: the extent {(h, w)} does not lie in the canvas {self.canvas_hw}')
            size = (h, w)
            if scales[i] is not None and float(scales[i]) != 1.0:
                if not lo <= float(scales[i]) <= hi:
                    raise ValueError(f'sample {i}: scale {float(scales[i])} is outside scale_range {self.scale_range}')
                size = tuple(int(s) for s in np.round(np.array((h, w)) * float(scales[i])).astype(int))
            if min(size) < 1:
                raise ValueError(f'sample {i}: scale {scales[i]} leaves nothing of {(h, w)}')
            if size[0] > self.pad or size[1] > self.pad:
                raise ValueError(f'sample {i}: the resized image {size} exceeds pad {self.pad}')
            m = rotate.rotation_matrix(size[0], size[1], angles[i])
            rows.append((h, w) + size + (int(bool(flips[i])), 0, 0, 0))
            mats.append(m)
            fixed.append(rotate.nearest_fixed(m))
        records = torch.zeros(b, J.TABLE_WORDS, dtype=torch.int32) if jitters is None else J.params_table(jitters, b)
        contrast = bool((records[:, 5] >> J.OP_CODES['contrast'] & 1).any())
        return VOCBatchParams(torch.tensor(rows, dtype=torch.int32), torch.tensor(mats, dtype=torch.float64).reshape(b, 6),
                              torch.tensor(fixed, dtype=torch.int64).to(torch.int32).reshape(b, 6), records, jitters, contrast)

    def upload(self, p):
        """Copies a :class:`VOCBatchParams` (:meth:`rows`) into :attr:`params`: one staging buffer, ONE non-blocking host-to-device copy.
        The launches (or a replay) that follow on the same stream read it."""
        if self.buffer is None:
            raise ValueError('upload needs the device buffers: call the object or run() on GPU tensors first')
        self._copied.synchronize()                               # the previous copy has left the staging buffer
        s = self._views(self._staging)
        s.rows.copy_(p.rows)
        s.matrices.copy_(p.matrices)
        s.fixed.copy_(p.fixed)
        s.jitter.copy_(p.jitter)
        self.buffer.copy_(self._staging, non_blocking=True)
        self._copied.record()

    def _list_sizes(self, frames, labels):
        """The (h, w) of every sample of two lists of ragged tensors, after checking them; nothing is launched."""
        hwc = self.norm.layout == 'hwc'
        b = len(frames)
        if b == 0 or len(labels) != b:
            raise ValueError(f'frames and labels must hold the same number of samples (>= 1), got {b} and {len(labels)}')
        sizes = []
        for i, (x, t) in enumerate(zip(frames, labels)):
            if not isinstance(x, torch.Tensor) or x.dtype != torch.uint8 or x.dim() != 3 or x.shape[2 if hwc else 0] != 3:
                raise ValueError(f'frame {i} must be uint8 {"(H, W, 3)" if hwc else "(3, H, W)"}, got '
                                 f'{getattr(x, "dtype", type(x))} {tuple(getattr(x, "shape", ()))}')
            h, w = (int(s) for s in (x.shape[:2] if hwc else x.shape[1:]))
            if not isinstance(t, torch.Tensor) or t.dtype not in (torch.uint8, torch.int64) or tuple(t.shape) != (h, w):
                raise ValueError(f'label {i} must be uint8 or int64 {(h, w)}, got {getattr(t, "dtype", type(t))} {tuple(getattr(t, "shape", ()))}')
            if x.device != frames[0].device or t.device != frames[0].device or t.dtype != labels[0].dtype:
                raise ValueError(f'sample {i} is {t.dtype} on {x.device} / {t.device}, the first {labels[0].dtype} on {frames[0].device}')
            if h > self.canvas_hw[0] or w > self.canvas_hw[1] or min(h, w) < 1:
                raise ValueError(f'sample {i}: {(h, w)} does not fit the canvas {self.canvas_hw}')
            sizes.append((h, w))
        return sizes

    def pack(self, frames, labels):
        """A list of B ragged samples (frames (h, w, 3) / (3, h, w), labels (h, w)) as ``(canvas frames, canvas labels, sizes)``; the
        canvas padding is zero.  One copy per sample and tensor: a loader that collates into a canvas itself saves them."""
        hwc = self.norm.layout == 'hwc'
        frames, labels = list(frames), list(labels)
        sizes = self._list_sizes(frames, labels)
        b, (hm, wm) = len(frames), self.canvas_hw
        canvas = torch.zeros((b, hm, wm, 3) if hwc else (b, 3, hm, wm), dtype=torch.uint8, device=frames[0].device)
        lcanvas = torch.zeros(b, hm, wm, dtype=labels[0].dtype, device=frames[0].device)
        for i, ((h, w), x, t) in enumerate(zip(sizes, frames, labels)):
            if hwc:
                canvas[i, :h, :w] = x
            else:
                canvas[i, :, :h, :w] = x
            lcanvas[i, :h, :w] = t
        return canvas, lcanvas, sizes

    def _cpu(self, frames, labels, p):
        hwc = self.norm.layout == 'hwc'
        crops, lcrops, flips, scales = [], [], [], []
        for i, (h, w, hr, wr, flip, *_) in enumerate(p.rows.tolist()):
            crops.append(frames[i, :h, :w] if hwc else frames[i, :, :h, :w])
            lcrops.append(labels[i, :h, :w])
            flips.append(bool(flip))
            scales.append((hr, wr))
        return _voc_cpu(crops, lcrops, flips, p.jitters, scales, p.matrices, p.fixed, self.pad, self.norm, self.fill, self.lbl_fill,
                        self.rotate_fill, self.lbl_rotate_fill)

    def run(self, frames, labels, params=None, out=None, jitter=False):
        """The launches over whatever :attr:`params` holds when they RUN: no host state is read or written, so a captured ``run`` replays
        with the parameters last copied into the buffer (:meth:`upload`).  ``frames`` and ``labels`` are the contiguous canvases.
        ``jitter``: False = no jitter launches (5 in all); True = the clear, the mean pass and the apply pass (8; a record of zeros leaves
        its sample as it is); ``'no_contrast'`` = the apply pass alone (6), the caller's promise that no record names contrast.  ``out``:
        ``(image, label)`` to write into.  Returns ``(image float32 (B, 3, pad, pad), label int64 (B, pad, pad))``.  Nothing checks the
        parameters on the host: a row the table launch declines sets :attr:`status`.  CPU tensors: ``params`` must be a
        :class:`VOCBatchParams` from :meth:`rows`; same values."""
        b = self._check(frames, labels)
        if not frames.is_cuda:
            if not isinstance(params, VOCBatchParams):
                raise ValueError('run on CPU tensors needs params, a VOCBatchParams from rows()')
            return self._cpu(frames, labels, params if jitter else params._replace(jitters=None))
        if params is not None:
            raise ValueError('run on GPU tensors reads self.params: upload() a VOCBatchParams first')
        from . import functional as HF
        self._on(frames.device)
        p, layout, size = self.params, self.norm.layout, (self.pad, self.pad)
        if out is None:
            image = torch.empty(b, 3, self.pad, self.pad, dtype=torch.float32, device=frames.device)
            label = torch.empty(b, self.pad, self.pad, dtype=torch.int64, device=frames.device)
        else:
            image, label = out
        tables = HF.resize_tables_ragged(p.rows, self.canvas_hw, size, 'bicubic', self.ks_max, workspace=self.tables.workspace)
        if jitter:
            frames = HF.color_jitter_ragged(frames, p.rows, p.jitter, layout, contrast=jitter != 'no_contrast', out=self._jittered,
                                            sums=self._sums)
        HF.frame_resize_ragged(frames, p.rows, tables, layout, out=self._mid)
        HF.label_resize_ragged(labels, p.rows, tables, out=self._mid_label)
        HF.frame_rotate_ragged(self._mid, p.rows, tables, p.matrices, layout, size, self.rotate_fill, self.fill, norm=self.norm, out=image)
        HF.label_rotate_ragged(self._mid_label, p.rows, tables, p.fixed, size, self.lbl_rotate_fill, self.lbl_fill, out=label)
        return image, label

    def __call__(self, frames, labels, sizes, hflip, jitter, scale, angle):
        """``device_augment_voc(list of the B regions, ..., hflip, jitter, scale, angle, pad, norm, fill, lbl_fill, rotate_fill,
        lbl_rotate_fill)``: same results.  ``frames`` / ``labels``: the canvases and ``sizes`` their extents, or two lists of ragged
        tensors (``sizes`` None), which are packed (:meth:`pack`).  Raises before any launch for what ``device_augment_voc`` refuses and for
        a scale outside ``scale_range``; the parameters go up in one non-blocking copy."""
        if not isinstance(frames, torch.Tensor):
            if sizes is not None:
                raise ValueError('a list of ragged samples carries its own sizes: pass sizes=None')
            frames, labels = list(frames), list(labels)
            p = self.rows(self._list_sizes(frames, labels), hflip, jitter, scale, angle, len(frames))       # raises before any launch
            frames, labels, sizes = self.pack(frames, labels)
            self._check(frames, labels)
        else:
            if sizes is None:
                raise ValueError('a canvas needs sizes, the (h, w) of every sample')
            b = self._check(frames, labels)
            p = self.rows(sizes, hflip, jitter, scale, angle, b)     # raises before any launch
        if not frames.is_cuda:
            return self._cpu(frames, labels, p)
        self._on(frames.device)
        self.upload(p)
        return self.run(frames.contiguous(), labels.contiguous(), jitter=False if p.jitters is None else True if p.contrast else 'no_contrast')


def _voc_cpu(frames, labels, flips, jitters, sizes, matrices, fixed, pad, norm, fill, lbl_fill, rotate_fill, lbl_rotate_fill):
    """``device_augment_voc``'s CPU branch for given resized sizes and rotation tables (what :class:`BatchAugmentVOC` holds per sample)."""
    from .utils import jitter as J
    from .utils import resample, rotate
    hwc = norm.layout == 'hwc'
    b = len(frames)
    image = torch.empty(b, 3, pad, pad, dtype=torch.float32)
    label = torch.empty(b, pad, pad, dtype=torch.int64)
    for i in range(b):
        x, t = frames[i].contiguous()[None], labels[i].contiguous()[None]
        if jitters is not None:
            x = J.color_jitter_cpu(x, jitters[i], norm.layout)
        if flips[i]:
            x, t = x.flip(2 if hwc else 3), t.flip(2)
        if tuple(sizes[i]) != tuple(t.shape[1:]):
            x = resample.frame_resize_cpu(x, sizes[i], 'bicubic', norm.layout)
            t = resample.label_resize_cpu(t, sizes[i])
        image[i:i + 1] = rotate.frame_rotate_cpu(x, None, norm.layout, (pad, pad), rotate_fill, fill, norm=norm, table=matrices[i:i + 1])
        label[i:i + 1] = rotate.label_rotate_cpu(t, None, (pad, pad), lbl_rotate_fill, lbl_fill, out_dtype=torch.int64, table=fixed[i:i + 1])
    return image, label


def draw_color_jitter(brightness=0.0, contrast=0.0, saturation=0.0, hue=0.0, generator=None):
    """One ``ColorJitterParams`` drawn with the ranges of ``torchvision.transforms.ColorJitter(brightness, contrast, saturation, hue)``:
    each of the three factors uniform in ``[max(0, 1 - x), 1 + x]``, hue uniform in ``[-x, x]`` (``x <= 0.5``), and a random order of the
    four operations; an argument of 0 leaves its operation out, as torchvision's ``None`` range does.  ``generator``: a CPU
    ``torch.Generator``.  A convenience for ``device_augment(jitter=...)``: it does NOT claim to consume random numbers as torchvision
    does -- torchvision is not a dependency of this package and was not there to compare with, so a seed shared with a torchvision
    pipeline gives other parameters."""
    from .utils.jitter import OPS, ColorJitterParams
    given = dict(zip(OPS, (float(brightness), float(contrast), float(saturation), float(hue))))
    if any(not 0.0 <= v < float('inf') for v in given.values()) or given['hue'] > 0.5:
        raise ValueError(f'ranges must be >= 0 and hue <= 0.5, got {given}')
    order = [OPS[i] for i in torch.randperm(4, generator=generator).tolist()]
    u = torch.rand(4, generator=generator, dtype=torch.float64).tolist()
    factors = {}
    for name, r in zip(OPS, u):
        x = given[name]
        lo, hi = (-x, x) if name == 'hue' else (max(0.0, 1.0 - x), 1.0 + x)
        factors[name] = min(max(lo + (hi - lo) * r, lo), hi) if x > 0 else None
    return ColorJitterParams(tuple(n for n in order if factors[n] is not None), **factors)
