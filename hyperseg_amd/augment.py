"""The reference's train-time frame augmentation for GIVEN parameters, on the device, Pillow's bytes at every stage: the Cityscapes crop
chain (:func:`device_augment` per sample, :class:`BatchAugment` in three launches per batch) and the VOC-SBD chain for samples of
different sizes (:func:`device_augment_voc`, :class:`BatchAugmentVOC` in 5 / 6 / 8 launches).  The per-sample functions are the oracles
the batch classes are tested against; on CPU tensors every entry point takes the CPU implementations of ``utils``, same values.
``hyperseg_amd.training`` re-exports the public names.  ``functional`` (and with it the HIP library) is imported inside the functions
that launch, never on import of this module."""
import collections

import torch


def _per_sample(value, b, what, pair=False):
    """``value`` -- one value for the batch or a sequence of B -- as a list of B.  One value is a Python scalar (or None) or a 0-d tensor
    or array; lists, tuples and tensors or arrays with a dimension are sequences.  ``pair``: one value is a (top, left) pair of such
    scalars; a sequence of pairs is a sequence."""
    probe = value
    if pair:
        probe = value[0] if len(value) == 2 else ()
    one = not isinstance(probe, (list, tuple)) and getattr(probe, 'ndim', 0) == 0
    seq = [value] * b if one else list(value)
    if len(seq) != b:
        raise ValueError(f'{what} takes one value, or one per sample ({b}), got {len(seq)}')
    return seq


def _resized(hw, scale):
    """``round((H, W) * scale)``, numpy's rounding (half to even) as the reference's RandomResize."""
    import numpy as np
    return tuple(int(s) for s in np.round(np.array(hw) * float(scale)).astype(int))


def _frames_shape(layout, b, h, w):
    return (b, h, w, 3) if layout == 'hwc' else (b, 3, h, w)


def _outputs(b, h, w, device):
    """What every entry point returns: ``(image float32 (B, 3, h, w), label int64 (B, h, w))``, new."""
    return torch.empty(b, 3, h, w, dtype=torch.float32, device=device), torch.empty(b, h, w, dtype=torch.int64, device=device)


def _labels_shape(label_codec, b, h, w):
    """The shape of the labels of (B, H, W) frames: raw labels have their codec's (a colour image has three bytes per pixel)."""
    return (b, h, w) if label_codec is None else label_codec.raw_shape(b, h, w)


def _crop_cpu(frames_u8, labels, sizes, offsets, flips, jitter, crop, norm, filter, fill, lbl_fill, label_codec=None, blur=None,
              blur_table=None):
    """The crop chain on CPU tensors for given resized ``sizes`` (Hr, Wr), ``offsets`` and ``flips`` per sample (``utils.resample``,
    ``utils.jitter``, ``utils.blur``): what :func:`device_augment` and :class:`BatchAugment` return for them.  The blur is given as
    ``blur`` (a list of B ``GaussianBlurParams``) or as ``blur_table``, the records :meth:`BatchAugment.run` takes."""
    from .utils import resample
    b, (ch, cw) = frames_u8.shape[0], crop
    blurred = blur is not None or blur_table is not None
    u8 = jitter is not None or blurred                       # then the resize gives the uint8 crop and the last image step normalises
    dst_norm = None if u8 else norm
    dst = torch.empty(_frames_shape(norm.layout, b, ch, cw), dtype=torch.uint8) if u8 else torch.empty((b, 3, ch, cw), dtype=torch.float32)
    label = torch.empty(b, ch, cw, dtype=torch.int64)
    for i, (size, offset, flip) in enumerate(zip(sizes, offsets, flips)):
        view = resample.ResizeView((ch, cw), tuple(int(o) for o in offset), bool(flip), fill)
        dst[i:i + 1] = resample.frame_resize_cpu(frames_u8[i:i + 1], size, filter, norm.layout, view=view, norm=dst_norm)
        label[i:i + 1] = resample.label_resize_cpu(labels[i:i + 1], size, view=view, fill=lbl_fill, out_dtype=torch.int64, codec=label_codec)
    if jitter is not None:
        from .utils import jitter as J
        dst = J.color_jitter_cpu(dst, J.per_sample(jitter, b), norm.layout, norm=None if blurred else norm)
    if blurred:
        from .utils import blur as BL
        dst = BL.gaussian_blur_cpu(dst, blur, norm.layout, norm=norm, table=blur_table)
    return dst, label


def device_augment(frames_u8, labels, scale, crop, offset, hflip, norm, lbl_fill=255, fill=(0, 0, 0), jitter=None, label_codec=None,
                   blur=None):
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
    nothing changes.

    ``label_codec`` (a ``LabelCodec``): ``labels`` are RAW -- ids (B, H, W) or a colour image uint8 (B, H, W, 3) -- and the label launch
    encodes the pixel it gathers (``functional.label_resize(codec=)``): the same launches, no host pass.  ``lbl_fill`` is a class
    value and is not encoded.

    ``blur`` (a ``GaussianBlurParams``, or a sequence of B with ``None`` for a sample that is not blurred; :func:`draw_gaussian_blur`
    draws one): the reference's ``RandomGaussianBlur`` (seg_transforms.py:361-378, ``ImageFilter.GaussianBlur``) as the LAST step of the
    image chain -- after the crop and the flip and after ``jitter`` if one is given, on the uint8 crop (padding included), before the
    normalisation: ``functional.gaussian_blur`` produces the normalised image of the whole batch in two launches
    (``utils.blur.gaussian_blur_cpu`` for CPU tensors), and the jitter, if any, then writes bytes.  The label is not touched.  ``None``:
    nothing changes.  A radius the device kernels do not take raises ValueError before any launch."""
    b, h, w = norm.frame_size(frames_u8)
    want = _labels_shape(label_codec, b, h, w)
    if not isinstance(labels, torch.Tensor) or tuple(labels.shape) != want:
        raise ValueError(f'labels must be {"(B, H, W)" if len(want) == 3 else "(B, H, W, 3)"} = {want}, got {tuple(getattr(labels, "shape", ()))}')
    ch, cw = (int(s) for s in crop)
    sizes = [_resized((h, w), s) for s in _per_sample(scale, b, 'scale')]
    offsets, flips = _per_sample(offset, b, 'offset', pair=True), _per_sample(hflip, b, 'hflip')
    if jitter is not None:
        from .utils import jitter as J
        jitter = J.per_sample(jitter, b)
    if blur is not None:
        from .utils import blur as BL
        blur = BL.per_sample(blur, b)
    frames_u8, labels = frames_u8.contiguous(), labels.contiguous()
    if not frames_u8.is_cuda:
        return _crop_cpu(frames_u8, labels, sizes, offsets, flips, jitter, (ch, cw), norm, 'bicubic', fill, lbl_fill, label_codec, blur)
    from . import functional as HF
    from .utils import resample
    blur_table = None if blur is None else HF.blur_records(blur, b).to(frames_u8.device)       # raises before any launch
    image, label = _outputs(b, ch, cw, frames_u8.device)
    dst, dst_norm = image, norm
    if jitter is not None or blur is not None:               # the resize writes the uint8 crop, the last image step normalises
        dst_norm = None
        dst = torch.empty(_frames_shape(norm.layout, b, ch, cw), dtype=torch.uint8, device=frames_u8.device)
    for i in range(b):
        view = resample.ResizeView((ch, cw), tuple(int(o) for o in offsets[i]), bool(flips[i]), fill)
        HF.frame_resize(frames_u8[i:i + 1], sizes[i], 'bicubic', norm.layout, view=view, norm=dst_norm, out=dst[i:i + 1])
        HF.label_resize(labels[i:i + 1], sizes[i], view=view, fill=lbl_fill, out=label[i:i + 1], codec=label_codec)
    _image_tail(dst, jitter, blur_table, norm, image)
    return image, label


def _image_tail(crop_u8, jitter, blur_table, norm, image, blur_status=None):
    """The steps of the image chain behind the crop, on the device: ``jitter`` (a list of B ``ColorJitterParams`` or None), then the blur
    of the device records ``blur_table`` (or None); the last one looks the bytes up in ``norm``'s table and writes ``image``."""
    from . import functional as HF
    if jitter is not None:
        if blur_table is None:
            HF.color_jitter(crop_u8, jitter, norm.layout, norm=norm, out=image)
        else:
            crop_u8 = HF.color_jitter(crop_u8, jitter, norm.layout)
    if blur_table is not None:
        HF.gaussian_blur(crop_u8, None, norm.layout, norm=norm, out=image, table=blur_table, status=blur_status)


class _DeviceParams:
    """What a batch object holds per device, used by composition: the int32 parameter ``buffer`` the kernels read when they run, a pinned
    staging buffer of the same size and the event of the last copy out of it; ``tables``, the owner's ``functional.ResizeTables`` /
    ``RaggedTables`` over its workspace; and the batch size, latched by the first batch seen.  Nothing here is read by a launch."""

    def __init__(self, batch, owner):
        self.batch, self.owner = batch, owner
        self.buffer = self.tables = self._staging = self._copied = None

    def latch(self, b):
        if self.batch is None:
            self.batch = b
        if b != self.batch:
            raise ValueError(f'{b} frames, this {self.owner} holds batches of {self.batch}')
        return b

    def on(self, device, words, tables, in_hw, out_hw, ks_max):
        """Makes the buffers (``words`` int32 per sample) and the ``tables`` (``functional.ResizeTables`` or ``RaggedTables``, over a new
        workspace) unless they are on ``device`` already; True if it did."""
        if self.tables is not None and self.buffer.device == device:
            return False
        self.buffer = torch.zeros(self.batch * words, dtype=torch.int32, device=device)
        self._staging = torch.zeros(self.batch * words, dtype=torch.int32).pin_memory()
        self._copied = torch.cuda.Event()
        workspace = torch.zeros(tables.words(self.batch, out_hw, ks_max), dtype=torch.int32, device=device)
        self.tables = tables.over(workspace, self.batch, in_hw, out_hw, ks_max)
        return True

    def upload(self, fill_staging):
        """``fill_staging(staging)`` writes the parameters into the pinned buffer; they go up in ONE non-blocking host-to-device copy that
        the launches (or a replay) following on the same stream read."""
        self._copied.synchronize()                               # the previous copy has left the staging buffer
        fill_staging(self._staging)
        self.buffer.copy_(self._staging, non_blocking=True)
        self._copied.record()

    @property
    def status(self):
        return None if self.tables is None else self.tables.status

    @property
    def workspace(self):
        return None if self.tables is None else self.tables.workspace


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
    pinned staging buffer, all made at the first GPU call.  One object serves one stream at a time.  ``label_codec`` (a ``LabelCodec``):
    the labels are RAW, as ``device_augment(label_codec=)`` takes them, and the label launch encodes them -- still three launches.

    A Gaussian blur at the end of the image chain (``blur=`` of ``__call__`` and :meth:`run`, as ``device_augment``'s) adds two launches;
    its records sit behind ``params`` in the same buffer (:attr:`blur_table`, int32 (B, 4)) and go up in the same copy, and
    :attr:`blur_status` (int32 (B,)) holds what the blur launch declined."""

    def __init__(self, in_hw, crop, norm, scale_range, filter='bicubic', lbl_fill=255, fill=(0, 0, 0), batch=None, label_codec=None):
        from .utils import resample
        from .utils.labels import LabelCodec
        if label_codec is not None and not isinstance(label_codec, LabelCodec):
            raise ValueError(f'label_codec must be a hyperseg_amd.LabelCodec or None, got {type(label_codec).__name__}')
        self.label_codec = label_codec
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
        self._dev = _DeviceParams(None if batch is None else int(batch), 'BatchAugment')
        smallest = self._resized(lo)
        if min(smallest) < 1:
            raise ValueError(f'scale {lo} leaves nothing of {self.in_hw}')
        # ks_for is the rule; rounding the resized size down can make the true ratio a little larger than 1 / lo
        self.ks_max = max(resample.ks_for(filter, lo), *(resample.ksize_of(i, o, filter) for i, o in zip(self.in_hw, smallest)))
        self.params = self.blur_table = self.blur_status = self._crop_u8 = None

    def _resized(self, scale):
        return _resized(self.in_hw, scale)

    batch = property(lambda self: self._dev.batch)
    tables = property(lambda self: self._dev.tables)
    status = property(lambda self: self._dev.status, doc="""int32 (B,) on the device: 0, or the sum of ``functional.RESIZE_STATUS`` codes of
        a sample whose parameters the table launch declined (that sample is fill).  Reading it synchronises; the caller chooses when.""")
    workspace = property(lambda self: self._dev.workspace)

    def _check(self, frames_u8, labels):
        b, h, w = self.norm.frame_size(frames_u8)
        if (h, w) != self.in_hw:
            raise ValueError(f'frames are {(h, w)}, this BatchAugment was made for {self.in_hw}')
        want = _labels_shape(self.label_codec, b, h, w)
        if not isinstance(labels, torch.Tensor) or tuple(labels.shape) != want or labels.device != frames_u8.device:
            raise ValueError(f'labels must be {"(B, H, W)" if len(want) == 3 else "(B, H, W, 3)"} = {want} on {frames_u8.device}, got '
                             f'{tuple(getattr(labels, "shape", ()))}')
        return self._dev.latch(b)

    def _views(self, buffer):
        """(params (B, 6), blur records (B, 4)) over one int32 buffer of B * 10 words."""
        from . import functional as HF
        from .utils import blur as BL
        p, r = torch.split(buffer, (self.batch * HF.RESIZE_PARAM_WORDS, self.batch * BL.TABLE_WORDS))
        return p.view(self.batch, HF.RESIZE_PARAM_WORDS), r.view(self.batch, BL.TABLE_WORDS)

    def _on(self, device):
        from . import functional as HF
        from .utils import blur as BL
        if self._dev.on(device, HF.RESIZE_PARAM_WORDS + BL.TABLE_WORDS, HF.ResizeTables, self.in_hw, self.crop, self.ks_max):
            self.params, self.blur_table = self._views(self._dev.buffer)
            self.blur_status = torch.zeros(self.batch, dtype=torch.int32, device=device)
            self._crop_u8 = None
            self.norm.table(device)
            if self.label_codec is not None:
                self.label_codec.device_words(device)

    def rows(self, scale, offset, hflip, batch=None):
        """The ``params`` rows of given augmentation parameters (each one value or a sequence of B, as ``device_augment``'s): a CPU int32
        (B, 6) tensor.  A scale outside ``scale_range`` raises ValueError."""
        b = self.batch if batch is None else batch
        lo, hi = self.scale_range
        rows = []
        for s, o, f in zip(_per_sample(scale, b, 'scale'), _per_sample(offset, b, 'offset', pair=True), _per_sample(hflip, b, 'hflip')):
            if not lo <= float(s) <= hi:
                raise ValueError(f'scale {float(s)} is outside scale_range {self.scale_range}')
            rows.append(self._resized(s) + (int(o[0]), int(o[1]), int(bool(f)), 0))
        return torch.tensor(rows, dtype=torch.int32)

    def _cpu(self, frames_u8, labels, rows, jitter, blur=None, blur_table=None):
        rows = rows.tolist()
        return _crop_cpu(frames_u8, labels, [r[:2] for r in rows], [r[2:4] for r in rows], [r[4] for r in rows], jitter, self.crop,
                         self.norm, self.filter, self.fill, self.lbl_fill, self.label_codec, blur, blur_table)

    def _crop_bytes(self, device):
        """The uint8 crop of the batch between the resize launch and the image steps behind it: made once, so that a captured ``run``
        finds it where it was."""
        if self._crop_u8 is None or self._crop_u8.device != device:
            self._crop_u8 = torch.empty(_frames_shape(self.norm.layout, self.batch, *self.crop), dtype=torch.uint8, device=device)
        return self._crop_u8

    def _launch(self, frames_u8, labels, params, dst, dst_norm, label):
        from . import functional as HF
        tables = HF.resize_tables(params, self.in_hw, self.crop, self.filter, self.ks_max, workspace=self.tables.workspace)
        HF.frame_resize_batch(frames_u8, params, tables, self.norm.layout, fill=self.fill, norm=dst_norm, out=dst)
        HF.label_resize_batch(labels, params, tables, fill=self.lbl_fill, out=label, codec=self.label_codec)

    def run(self, frames_u8, labels, params=None, out=None, blur=None):
        """The three launches over whatever ``self.params`` (or the given device tensor of that shape) holds when they RUN: no host
        state is read or written, so a captured ``run`` replays with the parameters last copied into the tensor.  ``frames_u8`` and
        ``labels`` must be contiguous.  ``out``: ``(image, label)`` to write into.  Returns ``(image float32 (B, 3, h, w), label int64
        (B, h, w))``.  Nothing checks the parameters on the host: a row the table launch declines sets :attr:`status`.

        ``blur``: the blur records the same way -- an int32 (B, ``utils.blur.TABLE_WORDS``) tensor on the frames' device
        (``utils.blur.params_table``), or True for the object's own :attr:`blur_table`, which ``__call__`` fills.  The resize then
        writes the uint8 crop and ``functional.gaussian_blur`` normalises it: FIVE launches, and a captured ``run`` replays with the
        radii last copied into the table (a record with apply 0 leaves its sample unblurred).  A record the kernels do not take sets
        :attr:`blur_status`."""
        b = self._check(frames_u8, labels)
        if not frames_u8.is_cuda:
            rows = self.params if params is None else params
            if rows is None or blur is True:
                raise ValueError('run on CPU tensors needs params, and the blur records themselves')
            return self._cpu(frames_u8, labels, rows, None, blur_table=blur)
        self._on(frames_u8.device)
        params = self.params if params is None else params
        image, label = _outputs(b, *self.crop, frames_u8.device) if out is None else out
        if blur is None:
            self._launch(frames_u8, labels, params, image, self.norm, label)
        else:
            crop_u8 = self._crop_bytes(frames_u8.device)
            self._launch(frames_u8, labels, params, crop_u8, None, label)
            _image_tail(crop_u8, None, self.blur_table if blur is True else blur, self.norm, image, self.blur_status)
        return image, label

    def __call__(self, frames_u8, labels, scale, offset, hflip, jitter=None, blur=None):
        """``device_augment(frames_u8, labels, scale, crop, offset, hflip, norm, lbl_fill, fill, jitter, blur=blur)``: same arguments,
        same results.  The resized sizes are ``round((H, W) * scale)`` on the host; the parameters -- the blur records among them -- go
        up in one non-blocking copy."""
        b = self._check(frames_u8, labels)
        rows = self.rows(scale, offset, hflip, b)                # raises before any launch
        if blur is not None:
            from .utils import blur as BL
            blur = BL.per_sample(blur, b)
        if not frames_u8.is_cuda:
            return self._cpu(frames_u8, labels, rows, jitter, blur)
        from . import functional as HF
        records = None if blur is None else HF.blur_records(blur, b)             # raises before any launch
        self._on(frames_u8.device)
        frames_u8, labels = frames_u8.contiguous(), labels.contiguous()

        def fill_staging(staging):
            s_rows, s_records = self._views(staging)
            s_rows.copy_(rows)
            if records is None:
                s_records.zero_()
            else:
                s_records.copy_(records)
        self._dev.upload(fill_staging)
        image, label = _outputs(b, *self.crop, frames_u8.device)
        if jitter is None and blur is None:
            self._launch(frames_u8, labels, self.params, image, self.norm, label)
        else:                                                    # the resize writes the uint8 crop, the last image step normalises
            if jitter is not None:
                from .utils import jitter as J
                jitter = J.per_sample(jitter, b)
            crop_u8 = torch.empty(_frames_shape(self.norm.layout, b, *self.crop), dtype=torch.uint8, device=frames_u8.device)
            self._launch(frames_u8, labels, self.params, crop_u8, None, label)
            _image_tail(crop_u8, jitter, None if blur is None else self.blur_table, self.norm, image, self.blur_status)
        return image, label


def _ragged_sample(i, x, t, layout, first, canvas_hw=None):
    """The (h, w) of sample ``i`` of a ragged batch after checking it: ``x`` a uint8 frame (H, W, 3) / (3, H, W) as ``layout`` says, ``t``
    its uint8 or int64 label (H, W), both on the device of ``first``, the batch's first (frame, label).  ``canvas_hw``: the sample goes
    into one canvas with the others, so it must also fit it and have the first label's dtype."""
    hwc = layout == 'hwc'
    if not isinstance(x, torch.Tensor) or x.dtype != torch.uint8 or x.dim() != 3 or x.shape[2 if hwc else 0] != 3:
        raise ValueError(f'frame {i} must be uint8 {"(H, W, 3)" if hwc else "(3, H, W)"}, got '
                         f'{getattr(x, "dtype", type(x))} {tuple(getattr(x, "shape", ()))}')
    h, w = (int(s) for s in (x.shape[:2] if hwc else x.shape[1:]))
    if not isinstance(t, torch.Tensor) or t.dtype not in (torch.uint8, torch.int64) or tuple(t.shape) != (h, w):
        raise ValueError(f'label {i} must be uint8 or int64 {(h, w)}, got {getattr(t, "dtype", type(t))} {tuple(getattr(t, "shape", ()))}')
    device = first[0].device
    if x.device != device or t.device != device or (canvas_hw is not None and t.dtype != first[1].dtype):
        raise ValueError(f'sample {i} is {t.dtype} on {x.device} / {t.device}, the first {first[1].dtype} on {device}')
    if canvas_hw is not None and (h > canvas_hw[0] or w > canvas_hw[1] or min(h, w) < 1):
        raise ValueError(f'sample {i}: {(h, w)} does not fit the canvas {canvas_hw}')
    return h, w


def _ragged_lists(frames, labels):
    frames, labels = list(frames), list(labels)
    if len(frames) == 0 or len(labels) != len(frames):
        raise ValueError(f'frames and labels must hold the same number of samples (>= 1), got {len(frames)} and {len(labels)}')
    return frames, labels


def _voc_resized(i, hw, scale, pad, scale_range=None):
    """Sample ``i``'s size after RandomResize -- ``scale`` None or 1.0: it did not fire -- refusing a scale outside ``scale_range`` (if
    given), a size below 1 and one that ``pad`` does not hold."""
    size = tuple(hw)
    if scale is not None and float(scale) != 1.0:
        if scale_range is not None and not scale_range[0] <= float(scale) <= scale_range[1]:
            raise ValueError(f'sample {i}: scale {float(scale)} is outside scale_range {scale_range}')
        size = _resized(hw, scale)
    if min(size) < 1:
        raise ValueError(f'sample {i}: scale {scale} leaves nothing of {tuple(hw)}')
    if size[0] > pad or size[1] > pad:
        raise ValueError(f'sample {i}: the resized image {size} exceeds pad {pad}')
    return size


def _voc_cpu(frames, labels, flips, jitters, sizes, pad, norm, fill, lbl_fill, rotate_fill, lbl_rotate_fill, angles=None, matrices=None,
             fixed=None):
    """The VOC chain on CPU tensors (``utils.jitter`` / ``utils.resample`` / ``utils.rotate``) for lists of B ragged samples and their
    resized ``sizes``.  The rotation is given as ``angles`` (:func:`device_augment_voc`: ``utils.rotate`` makes the matrices) or as the
    ``matrices`` and ``fixed`` tables :class:`BatchAugmentVOC` uploads."""
    from .utils import jitter as J
    from .utils import resample, rotate
    hwc = norm.layout == 'hwc'
    b = len(frames)
    image, label = _outputs(b, pad, pad, 'cpu')
    for i in range(b):
        x, t = frames[i].contiguous()[None], labels[i].contiguous()[None]
        if jitters is not None:
            x = J.color_jitter_cpu(x, jitters[i], norm.layout)
        if flips[i]:
            x, t = x.flip(2 if hwc else 3), t.flip(2)
        if tuple(sizes[i]) != tuple(t.shape[1:]):
            x = resample.frame_resize_cpu(x, sizes[i], 'bicubic', norm.layout)
            t = resample.label_resize_cpu(t, sizes[i])
        angle = None if angles is None else angles[i]
        image[i:i + 1] = rotate.frame_rotate_cpu(x, angle, norm.layout, (pad, pad), rotate_fill, fill, norm=norm,
                                                 table=None if matrices is None else matrices[i:i + 1])
        label[i:i + 1] = rotate.label_rotate_cpu(t, angle, (pad, pad), lbl_rotate_fill, lbl_fill, out_dtype=torch.int64,
                                                 table=None if fixed is None else fixed[i:i + 1])
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
    from .utils import jitter as J
    from .utils import resample, rotate
    if isinstance(frames, torch.Tensor):
        norm.frame_size(frames)
        frames = [frames[i] for i in range(frames.shape[0])]
    if isinstance(labels, torch.Tensor):
        labels = [labels[i] for i in range(labels.shape[0])]
    frames, labels = _ragged_lists(frames, labels)
    b, pad = len(frames), int(pad)
    flips, scales, angles = _per_sample(hflip, b, 'hflip'), _per_sample(scale, b, 'scale'), rotate.per_sample(angle, b)
    jitters = None if jitter is None else J.per_sample(jitter, b)
    plan = []
    for i in range(b):
        h, w = _ragged_sample(i, frames[i], labels[i], norm.layout, (frames[0], labels[0]))
        size = _voc_resized(i, (h, w), scales[i], pad)
        rotate._check_hw(h, w)
        plan.append(((h, w), size))
    device = frames[0].device
    if device.type != 'cuda':
        return _voc_cpu(frames, labels, flips, jitters, [size for _, size in plan], pad, norm, fill, lbl_fill, rotate_fill, lbl_rotate_fill,
                        angles=angles)
    from . import functional as HF
    image, label = _outputs(b, pad, pad, device)
    mirror = resample.ResizeView
    for i, ((h, w), size) in enumerate(plan):
        x, t = frames[i].contiguous()[None], labels[i].contiguous()[None]
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
        self._dev = _DeviceParams(None if batch is None else int(batch), 'BatchAugmentVOC')

        def widest(n):
            """The most taps a row can hold for any extent 1..n at scale lo: min(ksize, extent), as the table launch counts them."""
            i = np.arange(1, n + 1)
            o = np.round(i * lo).astype(int)
            i, o = i[o >= 1], o[o >= 1]
            ks = np.where(i == o, 1, np.ceil(2.0 * np.maximum(i / np.maximum(o, 1), 1.0)).astype(int) * 2 + 1)
            return int(np.minimum(ks, i).max()) if len(i) else 1
        # ks_for is the rule; rounding the resized size can make the true ratio larger than 1 / lo
        self.ks_max = max(resample.ks_for('bicubic', lo), widest(self.canvas_hw[0]), widest(self.canvas_hw[1]))
        self.params = self._mid = self._mid_label = self._jittered = self._sums = None

    batch = property(lambda self: self._dev.batch)
    tables = property(lambda self: self._dev.tables)
    buffer = property(lambda self: self._dev.buffer)
    status = property(lambda self: self._dev.status, doc="""int32 (B,) on the device: 0, or the sum of ``functional.RAGGED_STATUS`` codes of
        a sample whose parameters the table launch declined (that sample is pad fill).  Reading it synchronises; the caller chooses when.""")
    workspace = property(lambda self: self._dev.workspace)

    def _check(self, frames, labels):
        b, h, w = self.norm.frame_size(frames)
        if (h, w) != self.canvas_hw:
            raise ValueError(f'the canvas is {(h, w)}, this BatchAugmentVOC was made for {self.canvas_hw}')
        if (not isinstance(labels, torch.Tensor) or labels.dtype not in (torch.uint8, torch.int64) or tuple(labels.shape) != (b, h, w)
                or labels.device != frames.device):
            raise ValueError(f'labels must be uint8 or int64 (B, H, W) = {(b, h, w)} on {frames.device}, got '
                             f'{getattr(labels, "dtype", type(labels))} {tuple(getattr(labels, "shape", ()))} on {getattr(labels, "device", None)}')
        return self._dev.latch(b)

    def _on(self, device):
        from . import functional as HF
        b, mid, layout = self.batch, (self.pad, self.pad), self.norm.layout
        if self._dev.on(device, self.WORDS, HF.RaggedTables, self.canvas_hw, mid, self.ks_max):
            self.params = self._views(self._dev.buffer)
            self._mid = torch.zeros(_frames_shape(layout, b, *mid), dtype=torch.uint8, device=device)
            self._mid_label = torch.zeros(b, self.pad, self.pad, dtype=torch.uint8, device=device)
            self._jittered = torch.zeros(_frames_shape(layout, b, *self.canvas_hw), dtype=torch.uint8, device=device)
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
        if len(sizes) != b or any(len(s) != 2 for s in sizes):
            raise ValueError(f'sizes must hold one (h, w) per sample ({b}), got {len(sizes)}')
        flips, scales, angles = _per_sample(hflip, b, 'hflip'), _per_sample(scale, b, 'scale'), rotate.per_sample(angle, b)
        jitters = None if jitter is None else J.per_sample(jitter, b)
        rows, mats, fixed = [], [], []
        for i, (h, w) in enumerate(sizes):
            h, w = int(h), int(w)
            if not (1 <= h <= self.canvas_hw[0] and 1 <= w <= self.canvas_hw[1]):
                raise ValueError(f'sample {i}: the extent {(h, w)} does not lie in the canvas {self.canvas_hw}')
            size = _voc_resized(i, (h, w), scales[i], self.pad, self.scale_range)
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

        def fill_staging(staging):
            s = self._views(staging)
            s.rows.copy_(p.rows)
            s.matrices.copy_(p.matrices)
            s.fixed.copy_(p.fixed)
            s.jitter.copy_(p.jitter)
        self._dev.upload(fill_staging)

    def _list_sizes(self, frames, labels):
        """The (h, w) of every sample of two lists of ragged tensors, after checking them; nothing is launched."""
        frames, labels = _ragged_lists(frames, labels)
        return [_ragged_sample(i, x, t, self.norm.layout, (frames[0], labels[0]), self.canvas_hw) for i, (x, t) in enumerate(zip(frames, labels))]

    def pack(self, frames, labels):
        """A list of B ragged samples (frames (h, w, 3) / (3, h, w), labels (h, w)) as ``(canvas frames, canvas labels, sizes)``; the
        canvas padding is zero.  One copy per sample and tensor: a loader that collates into a canvas itself saves them."""
        hwc = self.norm.layout == 'hwc'
        frames, labels = list(frames), list(labels)
        sizes = self._list_sizes(frames, labels)
        b, (hm, wm) = len(frames), self.canvas_hw
        canvas = torch.zeros(_frames_shape(self.norm.layout, b, hm, wm), dtype=torch.uint8, device=frames[0].device)
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
        crops, lcrops, flips, sizes = [], [], [], []
        for i, (h, w, hr, wr, flip, *_) in enumerate(p.rows.tolist()):
            crops.append(frames[i, :h, :w] if hwc else frames[i, :, :h, :w])
            lcrops.append(labels[i, :h, :w])
            flips.append(bool(flip))
            sizes.append((hr, wr))
        return _voc_cpu(crops, lcrops, flips, p.jitters, sizes, self.pad, self.norm, self.fill, self.lbl_fill, self.rotate_fill,
                        self.lbl_rotate_fill, matrices=p.matrices, fixed=p.fixed)

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
        image, label = _outputs(b, self.pad, self.pad, frames.device) if out is None else out
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


def draw_gaussian_blur(p=0.5, r=5, generator=None):
    """One ``GaussianBlurParams`` drawn as the reference's ``RandomGaussianBlur(p, r)`` draws (hyperseg/datasets/seg_transforms.py:361-378):
    with probability ``p`` the image is blurred with ``ImageFilter.GaussianBlur(radius=r)``, else it is left as it is (``apply`` False).
    ``generator``: a CPU ``torch.Generator``.  A convenience for ``device_augment(blur=...)``, one call per sample: it does NOT claim to
    consume random numbers as the reference's ``random.random()`` does."""
    from .utils.blur import GaussianBlurParams
    p = float(p)
    if not 0.0 <= p <= 1.0:
        raise ValueError(f'p must lie in [0, 1], got {p}')
    return GaussianBlurParams(r, float(torch.rand((), generator=generator, dtype=torch.float64)) < p)
