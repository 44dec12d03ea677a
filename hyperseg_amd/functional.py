"""Tensor-level entry points of the HIP decoder kernels (thin wrappers over the C ABI).

Vocabulary: a *bank* is the patch-major per-patch filter bank
``bank[p, m]`` (p = (b*fh + i)*fw + j); a *stage input* is the lazy channel concatenation
[coords | skip | resized previous level] that the reference materialises with torch.cat
(hyperseg_v1_0.py:231-240) and the kernels generate on the fly.
"""
import collections
import ctypes as C
import functools
import os
import threading

import torch

from . import _hip
from ._hip import ACT_NONE, ACT_RELU, ACT_RELU6, PAD_MODES  # noqa: F401  (re-exported)

BN_EPS_DEFAULT = 1e-5
DTYPE_CODES = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}       # hs_dtype of include/hyperseg_hip.h
S2W_TRAIN_MAX_LAYERS = 8     # S2W_MAX_LAYERS of csrc/hs_s2w_blocked.h: layers one hs_s2w_train_* / hs_signal2weights_multi_fwd launch takes
# Round 4: the banks of the later levels produced INSIDE the k = 1 levels' launches (CoScheduledBanks / hs_patch_conv_s2w_fwd).
# MEASURED AND OFF (visit r4e, profiles/round4_coscheduled_banks_ab.txt): the carrying launches grow by what the riders take -- level 2
# with bank 4 aboard 7.3 -> 15.2 us, kernel sum of (signal2weights + levels 0-2) 37.5 -> 39.4 us, replayed decoder 0.086 -> 0.087 ms.
# signal2weights is a per-workgroup latency chain too, not idle-CU filler.  HS_COSCHEDULE_BANKS=1 switches it on.
COSCHEDULE_BANKS = os.environ.get('HS_COSCHEDULE_BANKS', '0') == '1'


def _round_up(n, m):
    return (n + m - 1) // m * m


def _device_of(a):
    if isinstance(a, torch.Tensor):
        return a.device
    if isinstance(a, (StageInput, BankRef, SignalRef, U8Frame)):
        return a.device
    # a pass list of tta_merge, [(x, mid_size, flipped, entry), ...]: its first pass's tensor's
    if isinstance(a, (list, tuple)) and a and isinstance(a[0], (list, tuple)) and a[0] and isinstance(a[0][0], torch.Tensor):
        return a[0][0].device
    return None


def _on_operand_device(fn):
    """Every launch runs with the HIP device of its first tensor operand current: the stream handed to the library
    (``torch.cuda.current_stream()``) then belongs to the device that owns the pointers, also when the caller's current
    device is another one (nn.DataParallel replicas, a model placed on cuda:1 from a cuda:0 context)."""
    @functools.wraps(fn)
    def wrapper(*args, **kwargs):
        dev = next((d for d in map(_device_of, args) if d is not None), None)
        if dev is None or dev.type != 'cuda' or dev.index is None or dev.index == torch.cuda.current_device():
            return fn(*args, **kwargs)
        with torch.cuda.device(dev):
            return fn(*args, **kwargs)
    return wrapper


class U8Frame:
    """A batch of uint8 frames together with the ``utils.inference.InputNorm`` that describes them, standing where the float image
    (B, 3, H, W) would: ``shape`` is that image's.  The prepared encoder's stem + depthwise launch reads the bytes themselves
    (:func:`stem_dw`); ``float_image()`` is the one :func:`image_ingest` launch for whoever needs the float image after all (made at
    most once, and remembered, so the caller can tell afterwards whether it exists)."""

    requires_grad = False
    dtype = torch.uint8

    def __init__(self, data, norm):
        b, h, w = norm.frame_size(data)
        self.data, self.norm = data.contiguous(), norm
        self.shape = torch.Size((b, 3, h, w))
        self.image = None

    @property
    def device(self):
        return self.data.device

    @property
    def is_cuda(self):
        return self.data.is_cuda

    def contiguous(self):
        return self

    def float_image(self):
        if self.image is None:
            self.image = image_ingest(self.data, self.norm)
        return self.image

    def size_carrier(self):
        """The float image if it was made, else a meta tensor of its shape: what the decoder reads the output size from when no
        level consumes the image."""
        return self.image if self.image is not None else torch.empty(self.shape, dtype=torch.float32, device='meta')


class StageInput:
    """Lazy ``cat([coords(2)?, skip, resize(prev)?], dim=1)`` consumed by the stage kernels' prologue."""

    def __init__(self, skip, prev=None, coords=False):
        if skip.dim() != 4:
            raise ValueError('skip must be (B, C, H, W)')
        if prev is not None and (prev.dim() != 4 or prev.shape[0] != skip.shape[0]):
            raise ValueError('prev must be (B, C, h, w) with the same batch as skip')
        if prev is not None and prev.device != skip.device:
            raise ValueError(f'stage input spans two devices ({skip.device}, {prev.device})')
        self.skip, self.prev, self.coords = skip, prev, bool(coords)

    @property
    def channels(self):
        return 2 * self.coords + self.skip.shape[1] + (self.prev.shape[1] if self.prev is not None else 0)

    @property
    def shape(self):
        b, _, h, w = self.skip.shape
        return torch.Size((b, self.channels, h, w))

    @property
    def device(self):
        return self.skip.device

    def c_struct(self, prev_dtype=torch.float32):
        b, cs, h, w = self.skip.shape
        st = _hip.StageInputC()
        st.skip = _hip.dev_ptr(self.skip, 'stage input (skip)')
        st.batch, st.H, st.W, st.c_skip = b, h, w, cs
        st.coords = int(self.coords)
        if self.prev is not None:
            st.prev = _hip.dev_ptr(self.prev, 'stage input (prev)', prev_dtype)
            st.c_prev, st.Hp, st.Wp = self.prev.shape[1], self.prev.shape[2], self.prev.shape[3]
            st.prev_mode = _hip.PREV_SAME if self.prev.shape[2:] == self.skip.shape[2:] else _hip.PREV_BILINEAR
        else:
            st.prev, st.c_prev, st.Hp, st.Wp, st.prev_mode = None, 0, 0, 0, _hip.PREV_NONE
        return st

    def materialize(self, dtype=torch.float32):
        """The concatenated tensor itself (diagnostics / modules that cannot consume a lazy input; the training path, where
        ``dtype`` = the autocast dtype, bf16 or fp16, and the previous level may be stored in it: hs_stage_input_typed_fwd)."""
        codes = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}
        pdt = self.prev.dtype if self.prev is not None else torch.float32
        if dtype not in codes or pdt not in codes:
            raise NotImplementedError(f'stage input: storage types {pdt} -> {dtype} (supported: float32, bfloat16, float16)')
        if pdt != torch.float32 and dtype != torch.float32 and pdt != dtype:
            raise NotImplementedError(f'stage input: storage types {pdt} -> {dtype} (one half type per step)')
        st = self.c_struct(pdt)
        y = torch.empty(self.shape, device=self.device, dtype=dtype)
        with _hip.device_scope(self.device):
            _hip.run.hs_stage_input_typed_fwd(C.byref(st), codes[pdt], codes[dtype], y.data_ptr(), _hip.stream_ptr())
        return y


def _channel_view(t, name):
    """(device pointer, channels of the underlying buffer) of a (B, C, h, w) tensor that is contiguous
    or a channel-range view ``base[:, a:b]`` of a contiguous tensor (what MetaSequential passes)."""
    if t.dim() != 4:
        raise ValueError(f'{name} must be 4-D (B, C, h, w), got {tuple(t.shape)}')
    if not t.is_cuda or t.dtype != torch.float32:
        _hip.dev_ptr(t, name)          # raises with the proper message
    b, c, h, w = t.shape
    sb, sc, sh, sw = t.stride()
    plane = h * w
    ok = (sw == 1 or w == 1) and (sh == w or h == 1) and (sc == plane or c == 1) and \
         (b == 1 or (sb % plane == 0 and sb // plane >= c))
    if not ok:
        t = t.contiguous()
        return t, t.data_ptr(), c
    return t, t.data_ptr(), (sb // plane if b > 1 else c)


def as_stage(x):
    return x if isinstance(x, StageInput) else StageInput(x)


def _epilogue(scale=None, shift=None, act=ACT_NONE):
    ep = _hip.EpilogueC()
    ep.scale = _hip.dev_ptr(scale, 'epilogue scale') if scale is not None else None
    ep.shift = _hip.dev_ptr(shift, 'epilogue shift') if shift is not None else None
    ep.act = int(act)
    return ep


@_on_operand_device
def signal2weights(signal, wsw_t, signal_index, signal_channels, groups, rows, out=None):
    """Grouped 1x1 conv of the signal slice -> patch-major bank (B*fh*fw, ld).  ``wsw_t`` is the
    Conv2d weight transposed to (Cs/G, Wc).  Replaces signal2weights(...)[:, :hp] + permute copy."""
    b, c_view, fh, fw = signal.shape
    if signal_index + signal_channels > c_view:
        raise ValueError(f'signal slice [{signal_index}, {signal_index + signal_channels}) exceeds the '
                         f'{c_view} channels handed to the module')
    signal, sig_ptr, c_signal = _channel_view(signal, 'signal')
    wc = wsw_t.shape[1]
    ld = _round_up(rows, 4)
    if out is None:
        out = torch.empty(b * fh * fw, ld, device=signal.device, dtype=torch.float32)
    _hip.run.hs_signal2weights_fwd(
        sig_ptr, b, c_signal, fh, fw, signal_index, signal_channels, groups,
        _hip.dev_ptr(wsw_t, 'wsw_t'), wc, rows,
        _hip.dev_ptr(out, 'bank'), out.stride(0), _hip.stream_ptr())
    return out


class BankRef:
    """A bank that already exists (produced by :func:`signal2weights_multi` for a whole decoder / context head).  It
    stands in for the signal / weight tensor on its way through MetaSequential to the module that consumes it:
    ``ref[:, a:b]`` (MetaSequential's channel range) is the bank's column range [a, b), clamped like a tensor slice."""

    def __init__(self, bank, batch, rows, grid):
        self.bank, self.rows, self.grid = bank, rows, tuple(grid)
        self.shape = torch.Size((batch, rows) + self.grid)
        self.requires_grad = False

    @property
    def device(self):
        return self.bank.device

    def __getitem__(self, idx):
        if not (isinstance(idx, tuple) and len(idx) == 2 and idx[0] == slice(None) and isinstance(idx[1], slice)
                and idx[1].step in (None, 1)):
            raise IndexError('a filter bank supports only the channel-range slice ref[:, a:b]')
        a, b, _ = idx[1].indices(self.rows)
        if a == 0 and b == self.rows:
            return self
        return BankRef(self.bank[:, a:max(a, b)], self.shape[0], max(b - a, 0), self.grid)

    def dim(self):
        return 4


class TrainBank:
    """A level's bank on the TRAINING path: the patch-major (P, ld) tensor autograd.S2WBanksTrain produced (it carries the graph
    back to the signal and to the level's signal2weights weight).  Travels through MetaSequential like a BankRef."""

    def __init__(self, bank, batch, rows, grid):
        self.bank, self.rows, self.grid = bank, rows, tuple(grid)
        self.shape = torch.Size((batch, rows) + self.grid)
        self.requires_grad = True

    @property
    def device(self):
        return self.bank.device

    def __getitem__(self, idx):
        if not (isinstance(idx, tuple) and len(idx) == 2 and idx[0] == slice(None) and isinstance(idx[1], slice) and idx[1].step in (None, 1)):
            raise IndexError('a filter bank supports only the channel-range slice ref[:, a:b]')
        a, b, _ = idx[1].indices(self.rows)
        if a == 0 and b == self.rows:
            return self
        return TrainBank(self.bank[:, a:max(a, b)], self.shape[0], max(b - a, 0), self.grid)

    def dim(self):
        return 4


# Levels whose patches are at most this many pixels generate their bank inside the consumer (hs_patch_conv_gen_fwd) instead
# of reading one that hs_signal2weights_multi_fwd wrote.  OFF by default (0): measured on MI355X (profiles/round2_bank_in_
# consumer_ab.txt) it removes 2 x 18.4 MB of HBM traffic per HyperSeg-M frame but each fused launch takes 21.8 us against
# 8.8 us + its ~2 us share of the bank launch -- these levels are latency-, not bandwidth-bound, and the fused kernel
# serialises weight / signal / input round trips that the two-launch route overlaps across its 512 workgroups.
# Set HS_BANK_IN_CONSUMER_MAX_PIXELS=64 to switch it on.
BANK_IN_CONSUMER_MAX_PIXELS = int(os.environ.get('HS_BANK_IN_CONSUMER_MAX_PIXELS', '0'))


class SignalRef:
    """Stands in for a filter bank that is NOT materialised: the signal plus the signal2weights layer that would produce
    the bank (wsw_t, signal_index, signal_channels, groups, rows).  The consuming module hands both to
    :func:`patch_conv_gen`, which generates the bank rows it needs in LDS."""

    def __init__(self, signal, layer):
        self.signal, self.layer = signal, layer
        b, _, fh, fw = signal.shape
        self.shape = torch.Size((b, layer['rows'], fh, fw))
        self.requires_grad = False

    @property
    def device(self):
        return self.signal.device

    def __getitem__(self, idx):
        return self            # MetaSequential's channel range of a level with one signal-fed module: the whole bank

    def dim(self):
        return 4


_S2W_BLK = {}        # (wsw_t data_ptr, version, shape, channels, groups) -> (weakref to wsw_t, packed operand image of the blocked kernel)
# Re-entrancy (SURVEY 8b "Threading": nn.DataParallel.parallel_apply runs one Python thread per replica through these functions):
# every process-global cache is read and written under this lock -- the sweep below iterates the dict, which another thread's
# insert would break ("dictionary changed size during iteration") -- and the per-module caches (FoldedBN, TransposedS2W) keep one
# immutable (key, value) entry per DEVICE, replaced atomically, because DataParallel's replicas share those objects by reference.
_CACHE_LOCK = threading.RLock()


def publish_ready(device):
    """Called after the kernels that FILL a cache entry were launched and before the entry is published: the filling stream is drained
    on the host, so a thread that finds the entry from ANOTHER stream (a second request stream, a replica thread) reads finished data
    -- stream order only protects the stream that launched the fill.  Fills happen once per parameter version, so the wait is paid
    once; under stream capture a host wait is illegal and the entry is only ever consumed by the capturing stream's graph."""
    if device.type == 'cuda' and not torch.cuda.is_current_stream_capturing():
        torch.cuda.current_stream(device).synchronize()


def producer_stream(device):
    """Identity of the stream a cache entry is being filled on (kept with the entry; see :func:`adopt`)."""
    return torch.cuda.current_stream(device).cuda_stream if device.type == 'cuda' else 0


def adopt(value, device, filled_on):
    """A cache hit from ANOTHER stream than the one the entry was filled on: tell the caching allocator that the entry's tensors are
    in use on the caller's stream (``Tensor.record_stream``).  Without it the memory goes back to the FILLING stream's pool the moment
    the entry is replaced (a new parameter version) and the last Python reference dies -- while kernels the other stream launched on
    it may still be in flight -- and the filling stream's next allocation overwrites what they read.  (Found by
    tests/test_hip_parity.py::test_two_python_threads_two_streams_through_the_decoder: 23 of 40 outputs of one thread differed.)
    Returns ``value``."""
    if device.type == 'cuda':
        cur = torch.cuda.current_stream(device)
        if cur.cuda_stream != filled_on:
            for t in (value if isinstance(value, (tuple, list)) else (value,)):
                if isinstance(t, torch.Tensor):
                    t.record_stream(cur)
    return value


@_on_operand_device
def s2w_packed(wsw_t, signal_channels, groups):
    """The transposed signal2weights weight re-laid for ``hs_signal2weights_multi_fwd``'s blocked form (hs_s2w_pack_fwd), built
    once per parameter version (the transposed tensor itself is cached per module by version, so its address is the key)."""
    import weakref
    key = (_WEIGHTS_EPOCH[0], wsw_t.data_ptr(), wsw_t._version, tuple(wsw_t.shape), signal_channels, groups, wsw_t.device)
    with _CACHE_LOCK:
        ent = _S2W_BLK.get(key)
        hit = ent[1] if ent is not None and ent[0]() is wsw_t else None       # the address alone could be a dead tensor's, reused
        if hit is not None:
            adopt(hit, wsw_t.device, ent[2])
        if hit is None:
            for k in [k for k, (r, _, _) in list(_S2W_BLK.items()) if r() is None or k[0] != _WEIGHTS_EPOCH[0]]:      # dead sources and earlier weight epochs take their images with them
                del _S2W_BLK[k]
            n = _hip.lib.hs_s2w_pack_floats(signal_channels, groups, wsw_t.shape[1])
            if n < 0:
                _hip.check(int(n), 'hs_s2w_pack_floats')
            hit = torch.empty(n, device=wsw_t.device, dtype=torch.float32)
            _hip.run.hs_s2w_pack_fwd(_hip.dev_ptr(wsw_t, 'wsw_t'), signal_channels, groups, wsw_t.shape[1], hit.data_ptr(), _hip.stream_ptr())
            publish_ready(wsw_t.device)
            _S2W_BLK[key] = (weakref.ref(wsw_t), hit, producer_stream(wsw_t.device))
    return hit


S2W_BLOCKED = os.environ.get('HS_S2W_BLOCKED', '1') == '1'     # dev A/B switch: 0 = the direct (round-2) kernel


@_on_operand_device
def signal2weights_multi(signal, layers, buf=None):
    """All signal2weights layers of a decoder in ONE launch.  ``layers``: list of dicts with wsw_t, signal_index,
    signal_channels, groups, rows.  Returns one BankRef per layer (views of one buffer; ``buf``: the caller's own to lay them out
    in instead of a fresh one, contiguous fp32, at least ``bank_floats(signal, layers)`` elements)."""
    b, _, fh, fw = signal.shape
    signal, sig_ptr, c_signal = _channel_view(signal, 'signal')
    arr, refs = _s2w_layer_table(signal, layers, buf)
    _hip.run.hs_signal2weights_multi_fwd(sig_ptr, b, c_signal, fh, fw, arr, len(layers), _hip.stream_ptr())
    return refs


def _s2w_layer_table(signal, layers, buf=None):
    """The hs_s2w_layer table of ``layers`` over one bank buffer (allocated here unless given) + one BankRef per layer."""
    b, c_view, fh, fw = signal.shape
    p = b * fh * fw
    lds = [_round_up(l['rows'], 4) for l in layers]
    if buf is None:
        buf = torch.empty(p * sum(lds), device=signal.device, dtype=torch.float32)
    elif buf.numel() < p * sum(lds) or buf.dtype != torch.float32 or not buf.is_contiguous():
        raise ValueError('signal2weights_multi: buf is too small / not contiguous fp32')
    arr = (_hip.S2wLayerC * len(layers))()
    refs, off = [], 0
    # The packed weight images are owned by the cache, and the cache drops an entry as soon as the weight epoch moves (another
    # thread's BatchNorm update / mode switch, between two layers of this very loop): every image whose ADDRESS goes into the table
    # is kept alive by the table's first BankRef until the banks themselves die -- i.e. past the launch.  (Round 5's thread test: an
    # image freed between two s2w_packed calls was overwritten by the next layer's pack; wrong banks, 50 % of the logits' scale.)
    keep = []
    for i, (l, ld) in enumerate(zip(layers, lds)):
        if l['signal_index'] + l['signal_channels'] > c_view:
            raise ValueError('signal slice out of range')
        bank = buf[off:off + p * ld].view(p, ld)
        off += p * ld
        a = arr[i]
        a.signal_index, a.signal_channels, a.groups = l['signal_index'], l['signal_channels'], l['groups']
        a.wsw_t, a.wc = _hip.dev_ptr(l['wsw_t'], 'wsw_t'), l['wsw_t'].shape[1]
        a.rows, a.bank, a.ld = l['rows'], bank.data_ptr(), ld
        if S2W_BLOCKED:
            keep.append(s2w_packed(l['wsw_t'], l['signal_channels'], l['groups']))
            a.wsw_blk = keep[-1].data_ptr()
        else:
            a.wsw_blk = None
        keep.append(l['wsw_t'])
        refs.append(BankRef(bank, b, l['rows'], (fh, fw)))
    for r in refs:
        r._operands = keep
    return arr, refs


class CoScheduledBanks:
    """``with CoScheduledBanks(signal, layers) as co:`` -- the NEXT eligible k = 1 :func:`patch_conv` issued inside the block carries
    the signal2weights work of ``layers`` in its own launch (hs_patch_conv_s2w_fwd: a heterogeneous launch, the bank producer's
    blocks filling the idle CUs of a latency-bound k = 1 level).  On exit ``co.refs`` holds one BankRef per layer either way:
    if no launch took the work (or the library said HS_ERR_UNSUPPORTED) it is issued as its own launch then."""
    _active = None

    def __init__(self, signal, layers):
        self.signal, self.layers, self.refs, self.carried = signal, list(layers), None, False

    def __enter__(self):
        if CoScheduledBanks._active is not None:
            raise RuntimeError('CoScheduledBanks blocks do not nest')
        CoScheduledBanks._active = self if self.layers else None
        return self

    def __exit__(self, *exc):
        CoScheduledBanks._active = None
        if self.refs is None and exc[0] is None:
            self.refs = signal2weights_multi(self.signal, self.layers) if self.layers else []
        return False


def bank_floats(signal, layers):
    """fp32 elements of the buffer :func:`signal2weights_multi` lays the banks of ``layers`` out in (what its ``buf`` must hold)."""
    b, _, fh, fw = signal.shape
    return b * fh * fw * sum(_round_up(l['rows'], 4) for l in layers)


@_on_operand_device
def bank_pack(w, ch_offset, rows, out=None):
    """(B, hp_total, fh, fw) channel-major weights -> patch-major bank (B*fh*fw, ld)."""
    b, c_view, fh, fw = w.shape
    if ch_offset + rows > c_view:
        raise ValueError(f'weight has {c_view} channels, the module needs {ch_offset + rows}')
    w, w_ptr, hp_total = _channel_view(w, 'weight')
    ld = _round_up(rows, 4)
    if out is None:
        out = torch.empty(b * fh * fw, ld, device=w.device, dtype=torch.float32)
    _hip.run.hs_bank_pack_fwd(w_ptr, b, hp_total, fh, fw, ch_offset, rows,
                              _hip.dev_ptr(out, 'bank'), out.stride(0), _hip.stream_ptr())
    return out


@_on_operand_device
def bn_fold(gamma, beta, mean, var, eps=BN_EPS_DEFAULT):
    n = mean.numel()
    out = torch.empty(2, n, device=mean.device, dtype=torch.float32)
    _hip.run.hs_bn_fold_fwd(_hip.dev_ptr(gamma, 'bn weight'), _hip.dev_ptr(beta, 'bn bias'),
                            _hip.dev_ptr(mean, 'bn running_mean'), _hip.dev_ptr(var, 'bn running_var'),
                            float(eps), n, out[0].data_ptr(), out[1].data_ptr(), _hip.stream_ptr())
    return out[0], out[1]


def _bank_ptr(bank):
    """A bank is any 2-D fp32 CUDA tensor whose rows are contiguous (row stride = ld)."""
    if bank.dim() != 2 or bank.stride(1) != 1 and bank.shape[1] != 1:
        raise ValueError('bank must be 2-D (patches, rows) with contiguous rows')
    if not bank.is_cuda or bank.dtype != torch.float32:
        _hip.dev_ptr(bank, 'bank')
    return bank.data_ptr(), bank.stride(0)


@_on_operand_device
def patch_conv(x, grid, bank, c_out, k=1, padding=0, padding_mode='reflect', groups=1,
               scale=None, shift=None, act=ACT_NONE):
    """Op A / Op B with fused prologue (x may be a StageInput) and BN-affine + activation epilogue."""
    stage = as_stage(x)
    fh, fw = grid
    b, _, h, w = stage.shape
    st_in = stage.c_struct()
    ep = _epilogue(scale, shift, act)
    y = torch.empty(b, c_out, h, w, device=stage.device, dtype=torch.float32)
    bank_ptr, ld = _bank_ptr(bank)
    co = CoScheduledBanks._active
    if co is not None and k == 1 and padding == 0 and co.signal.device == stage.device:
        signal, sig_ptr, c_signal = _channel_view(co.signal, 'signal')
        arr, refs = _s2w_layer_table(signal, co.layers)
        sb, _, sfh, sfw = signal.shape
        st = _hip.lib.hs_patch_conv_s2w_fwd(C.byref(st_in), fh, fw, bank_ptr, ld, c_out, groups, C.byref(ep), y.data_ptr(),
                                            sig_ptr, sb, c_signal, sfh, sfw, arr, len(co.layers), _hip.stream_ptr())
        if st != -3:                                   # HS_ERR_UNSUPPORTED: nothing was launched, the separate calls follow
            _hip.check(st, 'hs_patch_conv_s2w_fwd')
            co.refs, co.carried = refs, True
            CoScheduledBanks._active = None
            return y
    _hip.run.hs_patch_conv_fwd(C.byref(st_in), fh, fw, bank_ptr, ld, c_out, k,
                               padding, PAD_MODES[padding_mode], groups, C.byref(ep), y.data_ptr(),
                               _hip.stream_ptr())
    return y


class ChainGate:
    """One chained launch at a time per device.  hs_decoder_chain_fwd's workgroups spin on their neighbours: the launch needs its WHOLE
    grid resident, which the host checks against an EMPTY chip -- two chained launches running at once (two streams / threads of one
    model, two prepared models) can starve each other of residency, the bounded spins then give up and the logits are wrong.  The gate
    orders chained launches ACROSS streams with events (a launch on stream B waits for the previous chained launch on stream A; launches
    of one stream are ordered anyway); utils.inference.GraphedModel brackets the replay of a graph that contains a chained launch with the
    same ``enter`` / ``leave`` pair.  Process-wide, per device; the lock spans "wait on the previous event -> launch -> record"."""
    _gates, _glock = {}, threading.Lock()

    def __init__(self):
        self.lock = threading.Lock()
        self.last_stream, self.last_event = None, None
        self._events, self._turn = None, 0

    @classmethod
    def of(cls, device):
        with cls._glock:
            g = cls._gates.get(device.index)
            if g is None:
                g = cls._gates[device.index] = cls()
            return g

    def enter(self, device):
        """Call with ``lock`` held, outside a capture: the current stream waits for the previous chained launch of another stream."""
        cur = torch.cuda.current_stream(device)
        if self.last_event is not None and self.last_stream != cur.cuda_stream:
            cur.wait_event(self.last_event)
        return cur

    def leave(self, cur):
        if self._events is None:
            self._events = [torch.cuda.Event(), torch.cuda.Event()]
        self._turn ^= 1
        ev = self._events[self._turn]
        ev.record(cur)
        self.last_stream, self.last_event = cur.cuda_stream, ev


# counts the chained launches issued while a stream capture is open: a capture site compares it before / after to learn whether its
# graph contains one (GraphedModel then replays through ChainGate)
CHAIN_LAUNCHES_CAPTURED = [0]


class K1Chain:
    """hs_decoder_chain_fwd for one decoder: the three coarse k = 1 levels -- and the first inverted-residual level behind them when
    ``ir`` is given -- as ONE launch whose workgroups hand their level outputs to the neighbouring cells inside the launch
    (csrc/hs_k1_chain.hip).  ``run`` returns the last level's output, or None when the library refuses the shape / the grid is not
    resident at once (the caller then issues the per-level launches).

    Safe by construction (SURVEY 8b "re-entrant"): the launch's workspace -- the generation counter the kernel keeps
    between calls lives there -- belongs to ONE stream (eager) or ONE capture (ExclusiveWorkspaces), so two streams through one
    decoder never share hand-off granules; chained launches of different streams are ordered by ChainGate, so two of them never
    compete for residency; and the kernel's error word (a bounded spin that gave up) is copied to pinned memory every ``POLL_EVERY``
    calls and checked on every call -- a frame computed from an abandoned wait raises instead of being returned silently."""
    POLL_EVERY = 16

    def __init__(self):
        self._ws = {}                        # key -> workspace signature (what has been launched at least once)
        self._refused = set()
        self._pool = ExclusiveWorkspaces()
        self._pool.SPARES = 4                # a zero-copy collective ring captures one graph per slot (three): no zero-fill node in any of them
        self._taken = {}                     # id(tensor) -> (tensor, pinned mirror of its error word)
        self._calls = 0
        self._lock = threading.Lock()

    @property
    def refuses_everything(self):
        return bool(self._refused) and not self._ws

    def _workspace(self, dev, key, nbytes):
        ws = self._pool.take(dev, key[1:], nbytes)
        with self._lock:
            if id(ws) not in self._taken:
                self._taken[id(ws)] = [ws, None]     # the pinned mirror is made by request_error_copy: no host allocation under capture
        return ws

    def check_errors(self):
        """Raises if a launch on any workspace of this object abandoned a wait (reads the pinned mirrors: no synchronisation)."""
        with self._lock:
            bad = [int(m.item()) for _, m in self._taken.values() if m is not None and int(m.item()) != 0]
        if bad:
            raise RuntimeError(f'hs_decoder_chain_fwd abandoned a wait (error word {bad[0]:#x}): its grid was not resident at once -- '
                               'another kernel held the chip; the frame is wrong.  Keep chained launches behind ChainGate '
                               '(GraphedModel does) or turn the chain off (prepare_for_inference(chain_k1=False))')

    def request_error_copy(self, device):
        """Asynchronous copies of every workspace's error word into its pinned mirror, on the current stream (not under capture)."""
        if torch.cuda.is_current_stream_capturing():
            return
        with self._lock:
            for ent in self._taken.values():
                if ent[1] is None:
                    ent[1] = torch.zeros(1, dtype=torch.int32).pin_memory()
            pairs = [(ws, m) for ws, m in self._taken.values() if ws.device == device]
        for ws, m in pairs:
            m.copy_(ws[:1].view(torch.int32)[:1], non_blocking=True)

    def run(self, skips, banks, couts, affines, acts, ir=None):
        """``skips``: the three skip features (B, c, fh << l, fw << l); ``banks``: (P, ld) fp32 tensors; ``affines``: (scale, shift) or
        None per level; ``acts``: activation codes.  ``ir``: dict(skip, bank, hidden, c_out, bn=[(s, b) | None] * 3) of the inverted
        residual on the 8 x 8-pixel patches."""
        dev = skips[0].device
        b, _, fh, fw = skips[0].shape
        key = (dev, b, fh, fw, tuple(couts), tuple(s.shape[1] for s in skips),
               None if ir is None else (ir['skip'].shape[1], ir['hidden'], ir['c_out']))
        if key in self._refused:
            return None
        arr = (_hip.K1LevelC * 3)()
        for l in range(3):
            sk = skips[l]
            if tuple(sk.shape[2:]) != (fh << l, fw << l) or sk.shape[0] != b:
                return None
            a = arr[l]
            a.skip, a.c_skip = _hip.dev_ptr(sk, f'skip feature of level {l}'), sk.shape[1]
            a.bank, a.ld = _bank_ptr(banks[l])
            a.c_out = couts[l]
            if affines[l] is not None:
                a.scale, a.shift = _hip.dev_ptr(affines[l][0], 'scale'), _hip.dev_ptr(affines[l][1], 'shift')
            else:
                a.scale, a.shift = None, None
            a.act = acts[l]
        irc = None
        if ir is not None:
            sk = ir['skip']
            if tuple(sk.shape[2:]) != (fh << 3, fw << 3) or sk.shape[0] != b:
                return None
            irc = _hip.ChainIrLevelC()
            irc.skip, irc.c_skip = _hip.dev_ptr(sk, 'skip feature of the inverted residual'), sk.shape[1]
            irc.bank, irc.ld = _bank_ptr(ir['bank'])
            irc.hidden, irc.c_out = ir['hidden'], ir['c_out']
            for k, bn in enumerate(ir['bn']):
                sc, sh = (None, None) if bn is None else (_hip.dev_ptr(bn[0], 'bn scale'), _hip.dev_ptr(bn[1], 'bn shift'))
                setattr(irc, f's{k + 1}', sc)
                setattr(irc, f'b{k + 1}', sh)
        irp = C.byref(irc) if irc is not None else None
        self.check_errors()
        capturing = torch.cuda.is_current_stream_capturing()
        with _hip.device_scope(dev):
            n = self._ws.get(key)
            if n is None:
                n = int(_hip.lib.hs_decoder_chain_workspace(b, fh, fw, arr, 3, irp))
                if n < 0:
                    self._refused.add(key)
                    return None
            # zero-filled ONCE per (stream | capture): generation 0.  A fill inside a capture would become a node of the graph and every
            # replay would restart at generation 1 -- legal, but a memset node per frame: ExclusiveWorkspaces hands out prepared spares
            ws = self._workspace(dev, key, n)
            scale = 8 if ir is not None else 4
            y = torch.empty(b, ir['c_out'] if ir is not None else couts[2], scale * fh, scale * fw, device=dev, dtype=torch.float32)
            gate = ChainGate.of(dev)
            if capturing:
                st = _hip.lib.hs_decoder_chain_fwd(b, fh, fw, arr, 3, irp, ws.data_ptr(), y.data_ptr(), _hip.stream_ptr())
                CHAIN_LAUNCHES_CAPTURED[0] += 1
            else:
                with gate.lock:
                    cur = gate.enter(dev)
                    st = _hip.lib.hs_decoder_chain_fwd(b, fh, fw, arr, 3, irp, ws.data_ptr(), y.data_ptr(), _hip.stream_ptr())
                    if st == 0:
                        gate.leave(cur)
        if st == -3:                              # HS_ERR_UNSUPPORTED: shape or residency -- nothing was launched
            self._refused.add(key)
            return None
        _hip.check(st, 'hs_decoder_chain_fwd')
        self._ws[key] = n
        self._calls += 1
        if not capturing and self._calls % self.POLL_EVERY == 0:
            self.request_error_copy(dev)
        return y

    def reset(self):
        """Drops every workspace (and a raised error with them): the next call starts at generation 0 on fresh buffers.  Graphs captured
        through this object keep their own references alive and must be re-captured."""
        with self._lock:
            self._taken.clear()
        self._pool = ExclusiveWorkspaces()
        self._pool.SPARES = 4

    def error_word(self):
        """Non-zero if a launch on any of this object's workspaces abandoned a wait (synchronising host read: diagnostics / tests)."""
        with self._lock:
            wss = [ws for ws, _ in self._taken.values()]
        return max([int(ws[:1].view(torch.int32)[0].item()) for ws in wss] or [0])


# The three coarse k = 1 levels (+ the first inverted-residual level) as one launch: opt-in per decoder (``decoder.chain_k1 = True``;
# prepare_for_inference(chain_k1=True) sets it), or process-wide with HS_K1_CHAIN=1 (dev A/B switch).  HS_K1_CHAIN_IR=0 keeps the
# inverted residual out of the chain (A/B).
K1_CHAIN = os.environ.get('HS_K1_CHAIN', '0') == '1'
K1_CHAIN_IR = os.environ.get('HS_K1_CHAIN_IR', '1') == '1'
# Whether a chained decoder carries its first inverted-residual level in the chain launch unless ``decoder.chain_ir`` says otherwise
K1_CHAIN_IR_DEFAULT = os.environ.get('HS_K1_CHAIN_IR_DEFAULT', '0') == '1'


@_on_operand_device
def meta_conv(x, w, c_out, kernel_size, stride=(1, 1), padding=(0, 0), dilation=(1, 1), padding_mode='zeros', groups=1,
              scale=None, shift=None, act=ACT_NONE):
    """MetaConv2d.forward for ANY of the reference's arguments (meta_conv.py:141-186): x (B, Cin, H, W), per-sample weights
    w (B, >= Cout * Cin/groups * kh * kw); non-square kernels, stride, dilation, any padding.  The "same"-padded stride-1
    case runs faster through :func:`patch_conv` with a (1, 1) grid."""
    if isinstance(x, StageInput):
        x = x.materialize()
    b, cin, h, wd = x.shape
    (kh, kw), (sh, sw), (ph, pw), (dh, dw) = kernel_size, stride, padding, dilation
    # zero padding: ph rows / pw columns on both sides.  The other modes: the reference hands (ph, pw, ph, pw) to F.pad, whose
    # order is (left, right, top, bottom) -- left = top = ph, right = bottom = pw (meta_conv.py:159, 175-176); reproduced.
    pt, pb, pl, pr = (ph, ph, pw, pw) if padding_mode == 'zeros' else (ph, pw, ph, pw)
    ho = (h + pt + pb - dh * (kh - 1) - 1) // sh + 1
    wo = (wd + pl + pr - dw * (kw - 1) - 1) // sw + 1
    if ho <= 0 or wo <= 0:
        raise ValueError(f'kernel {kernel_size} (dilation {dilation}) does not fit the padded {h}x{wd} input')
    if w.dim() != 2 or w.shape[0] != b or w.stride(1) != 1:
        raise ValueError(f'w must be (B, rows) with contiguous rows, got {tuple(w.shape)}')
    ep = _epilogue(scale, shift, act)
    y = torch.empty(b, c_out, ho, wo, device=x.device, dtype=torch.float32)
    w_ptr, ldw = _bank_ptr(w)            # a column range w[:, a:b] of a wider tensor (MetaSequential's slice) is read in place: ldw = its row stride
    _hip.run.hs_meta_conv_fwd(_hip.dev_ptr(x, 'x'), b, cin, h, wd, w_ptr, ldw, c_out, kh, kw,
                              sh, sw, pt, pb, pl, pr, dh, dw, PAD_MODES[padding_mode], groups, C.byref(ep), y.data_ptr(),
                              _hip.stream_ptr())
    return y


@_on_operand_device
def patch_conv_gen(x, sref, c_out, scale=None, shift=None, act=ACT_NONE):
    """Op A with the bank generated inside the kernel from ``sref`` (a :class:`SignalRef`): signal2weights + k = 1 patch
    conv + BN affine + activation, one launch, no bank in HBM.  Returns None when the shape is outside what the kernel
    covers (the caller then materialises the bank)."""
    stage = as_stage(x)
    b, _, h, w = stage.shape
    signal, sig_ptr, c_signal = _channel_view(sref.signal, 'signal')
    fh, fw = signal.shape[-2:]
    l = sref.layer
    lay = _hip.S2wLayerC()
    lay.signal_index, lay.signal_channels, lay.groups = l['signal_index'], l['signal_channels'], l['groups']
    lay.wsw_t, lay.wc, lay.rows = _hip.dev_ptr(l['wsw_t'], 'wsw_t'), l['wsw_t'].shape[1], l['rows']
    lay.bank, lay.ld = None, 0
    st_in = stage.c_struct()
    ep = _epilogue(scale, shift, act)
    y = torch.empty(b, c_out, h, w, device=stage.device, dtype=torch.float32)
    st = _hip.lib.hs_patch_conv_gen_fwd(C.byref(st_in), fh, fw, sig_ptr, c_signal, C.byref(lay), c_out, C.byref(ep),
                                        y.data_ptr(), _hip.stream_ptr())
    if st == -3:
        return None
    _hip.check(st, 'hs_patch_conv_gen_fwd')
    return y


@_on_operand_device
def patch_ir(x, grid, bank, hidden, c_out, bn1, bn2, bn3, residual=False, math=None):
    """Op C: fused per-patch inverted residual.  bn* are (scale, shift) pairs; bank rows in the reference's flat order.
    ``math``: 'f32' | 'split' | 'auto' (include/hyperseg_hip.h, hs_ir_math); None = :func:`get_ir_math`."""
    stage = as_stage(x)
    fh, fw = grid
    b, _, h, w = stage.shape
    st_in = stage.c_struct()
    e1, e2, e3 = _epilogue(*bn1), _epilogue(*bn2), _epilogue(*bn3)
    y = torch.empty(b, c_out, h, w, device=stage.device, dtype=torch.float32)
    bank_ptr, ld = _bank_ptr(bank)
    _hip.run.hs_patch_ir_fwd(C.byref(st_in), fh, fw, bank_ptr, ld, hidden, c_out,
                             C.byref(e1), C.byref(e2), C.byref(e3), int(bool(residual)), ir_math_code(math),
                             y.data_ptr(), _hip.stream_ptr())
    return y


D2_ROUTE = os.environ.get('HS_IR_D2', '1') != '0'      # A/B switch: 0 = small-patch Op D levels on the single-launch tiled kernel


@_on_operand_device
def patch_ir_v0(x, grid, bank, hidden, c_out, bn1, bn2, bn3, math=None):
    """Op D (hyperseg_v0_1.py:205-237) as one launch -- two through a scratch hidden map where patches are 4 x 4 / 8 x 8 pixels
    (hs_patch_ir_v0_ws_fwd; the scratch is a torch allocation of this call: the caching allocator hands the same block back every
    step, and under graph capture it belongs to the graph's pool); returns None when the shape has no fused instantiation (the
    caller then runs the block as three patch convolutions).  ``math`` as for :func:`patch_ir` (Op D has the exact-f32 form only)."""
    stage = as_stage(x)
    fh, fw = grid
    b, _, h, w = stage.shape
    st_in = stage.c_struct()
    e1, e2, e3 = _epilogue(*bn1), _epilogue(*bn2), _epilogue(*bn3)
    y = torch.empty(b, c_out, h, w, device=stage.device, dtype=torch.float32)
    bank_ptr, ld = _bank_ptr(bank)
    need = int(_hip.lib.hs_patch_ir_v0_workspace(C.byref(st_in), fh, fw, hidden, c_out)) if D2_ROUTE else 0
    ws = torch.empty(need // 4, device=stage.device, dtype=torch.float32) if need > 0 else None
    st = _hip.lib.hs_patch_ir_v0_ws_fwd(C.byref(st_in), fh, fw, bank_ptr, ld, hidden, c_out, C.byref(e1), C.byref(e2), C.byref(e3),
                                        ir_math_code(math), _hip.ptr(ws), need, y.data_ptr(),
                                        _hip.stream_ptr())
    if st == -3:
        return None
    _hip.check(st, 'hs_patch_ir_v0_ws_fwd')
    return y


IR_MATH = {'auto': 0, 'f32': 1, 'split': 2}
# Arithmetic of the fused inverted-residual levels (include/hyperseg_hip.h, hs_ir_math) is an ARGUMENT of every launch: the
# library keeps no mode.  Who chooses: (1) the ``math`` argument / the calling module's ``ir_math`` attribute (the nn.Module
# mirror defaults to 'f32', the reference's arithmetic; ``prepare_for_inference(ir_math='auto')`` opts a model into the
# f16-split form for serving), unless (2) an override is set here -- ``set_ir_math`` (tests, A/B runs) or the environment
# variable HS_IR_MATH at import time.
_ir_math_override = os.environ.get('HS_IR_MATH') or None
if _ir_math_override is not None and _ir_math_override not in IR_MATH:
    raise ValueError(f'HS_IR_MATH={_ir_math_override!r}: expected one of {sorted(IR_MATH)}')
DEFAULT_IR_MATH = 'f32'


def set_ir_math(mode):
    """Process-wide OVERRIDE of the math mode every fused inverted-residual launch is asked for ('split' | 'f32' | 'auto'),
    or None to hand the choice back to the modules.  A Python-side switch for tests and A/B runs -- the C library itself is
    stateless.  Returns the previous override.  One word, swapped under the cache lock; a thread that wants its OWN mode without
    touching the others' (a replica thread of nn.DataParallel) uses :func:`ir_math_scope`."""
    global _ir_math_override
    if mode is not None and mode not in IR_MATH:
        raise ValueError(f'ir math {mode!r}: expected one of {sorted(IR_MATH)} or None')
    with _CACHE_LOCK:
        prev, _ir_math_override = _ir_math_override, mode
    return prev


_ir_math_local = threading.local()


class ir_math_scope:
    """``with ir_math_scope('split'): ...`` -- a THREAD-LOCAL override (outranks the process-wide one) for the calling thread only."""

    def __init__(self, mode):
        if mode is not None and mode not in IR_MATH:
            raise ValueError(f'ir math {mode!r}: expected one of {sorted(IR_MATH)} or None')
        self.mode = mode

    def __enter__(self):
        self.prev = getattr(_ir_math_local, 'mode', None)
        _ir_math_local.mode = self.mode
        return self

    def __exit__(self, *exc):
        _ir_math_local.mode = self.prev


def get_ir_math(requested=None):
    """The mode a launch uses: the calling thread's scope if one is open, else the process-wide override if one is set, else
    ``requested`` (a module's attribute), else the default."""
    return getattr(_ir_math_local, 'mode', None) or _ir_math_override or requested or DEFAULT_IR_MATH


def ir_math_code(requested=None):
    return IR_MATH[get_ir_math(requested)]


IR_ROUTES = {0: 'generic', 1: 'f32_mfma', 2: 'split_mfma'}


def patch_ir_route(shape, c_skip, c_prev, grid, hidden, c_out, math=None, residual=False, coords=True):
    """Which kernel ``patch_ir`` would run for a stage of ``shape`` = (B, H, W) with ``c_skip`` skip and ``c_prev`` half-resolution
    previous-level channels: 'split_mfma' | 'f32_mfma' | 'generic' (include/hyperseg_hip.h, hs_patch_ir_route).  Host only."""
    b, h, w = shape
    si = _hip.StageInputC()
    si.skip, si.prev, si.batch, si.H, si.W = None, None, b, h, w
    si.c_skip, si.c_prev, si.Hp, si.Wp = c_skip, c_prev, h // 2, w // 2
    si.coords, si.prev_mode = int(bool(coords)), (2 if c_prev > 0 else 0)      # HS_PREV_BILINEAR: the half-resolution previous level
    r = _hip.lib.hs_patch_ir_route(C.byref(si), grid[0], grid[1], hidden, c_out, int(bool(residual)), ir_math_code(math))
    if r < 0:
        _hip.check(r, 'hs_patch_ir_route')
    return IR_ROUTES[r]


def _stage_probe(shape, c_skip, c_prev, coords, prev_size=None):
    """The pointer-free hs_stage_input of a route query: ``shape`` = (B, H, W); the previous level at half the resolution (bilinear)
    unless ``prev_size`` says otherwise (equal to (H, W): taken as it is)."""
    b, h, w = shape
    si = _hip.StageInputC()
    si.skip, si.prev, si.batch, si.H, si.W = None, None, b, h, w
    hp, wp = prev_size if prev_size is not None else (h // 2, w // 2)
    si.c_skip, si.c_prev, si.Hp, si.Wp = c_skip, c_prev, (hp if c_prev > 0 else 0), (wp if c_prev > 0 else 0)
    si.coords = int(bool(coords))
    si.prev_mode = 0 if c_prev == 0 else (_hip.PREV_SAME if (hp, wp) == (h, w) else _hip.PREV_BILINEAR)
    return si


def _ir_inst(word):
    return f'{word >> 16}_{(word >> 8) & 255}_{word & 255}'


def patch_ir_form(shape, c_skip, c_prev, grid, hidden, c_out, math=None, residual=False, coords=True, ld=0, bank_aligned=True,
                  y_aligned=True):
    """(route, form) of ``patch_ir`` (hs_patch_ir_form): the route of :func:`patch_ir_route` and the instantiation inside it --
    'generic': 'exact_24_6_16_t1x1' | 'class_32_0_32_t1x2' ... (tiles per patch); 'split_mfma': 'rh16_nw4_r2_s1p4m1' (region rows, waves,
    regions per patch, skip / previous-level quads and output tiles); 'f32_mfma': 'reg16_pwr16_34_16_19'.  None where the launcher
    refuses the shape.  ``bank_aligned`` / ``y_aligned``: 16-byte alignment of the bank and of the output.  Host only."""
    si = _stage_probe(shape, c_skip, c_prev, coords)
    f = (C.c_int32 * 4)()
    r = _route(_hip.lib.hs_patch_ir_form(C.byref(si), grid[0], grid[1], ld, hidden, c_out, int(bool(residual)), ir_math_code(math),
                                         int(bool(bank_aligned)), int(bool(y_aligned)), f), 'hs_patch_ir_form')
    if r is None:
        return None
    if r == 0:
        form = f'{"exact" if f[1] else "class"}_{_ir_inst(f[0])}_t{f[2]}x{f[3]}'
    elif r == 2:
        form = f'rh{f[0]}_nw{f[1]}_r{f[2]}_s{f[3] >> 8}p{(f[3] >> 4) & 15}m{f[3] & 15}'
    else:
        form = f'reg{f[0]}_pwr{f[1]}_{_ir_inst(f[2])}'
    return IR_ROUTES[r], form


IR_V0_ROUTES = {0: 'd2', 1: 'px', 2: 'fused'}


def patch_ir_v0_route(shape, c_skip, c_prev, grid, hidden, c_out, ld=0, workspace=None, bank_aligned=True):
    """(route, form) of ``patch_ir_v0`` (hs_patch_ir_v0_route): ('d2', 'pw4_rt3_al4_kq2') -- two launches through the workspace --,
    ('px', '16_6_6') or ('fused', 'reg8_pwr4_48_12_12'); None where ``patch_ir_v0`` returns None.  ``workspace``: whether the call
    passes one (None: as ``patch_ir_v0`` does, D2_ROUTE).  Host only."""
    si = _stage_probe(shape, c_skip, c_prev, True)
    f = (C.c_int32 * 4)()
    ws = D2_ROUTE if workspace is None else bool(workspace)
    r = _route(_hip.lib.hs_patch_ir_v0_route(C.byref(si), grid[0], grid[1], ld, hidden, c_out, int(ws), int(bool(bank_aligned)), f),
               'hs_patch_ir_v0_route')
    if r is None:
        return None
    form = (f'pw{f[0]}_rt{f[1]}_al{f[2]}_kq{f[3]}' if r == 0 else _ir_inst(f[2]) if r == 1 else f'reg{f[0]}_pwr{f[1]}_{_ir_inst(f[2])}')
    return IR_V0_ROUTES[r], form


CONV_ROUTES = {0: 'plain_dw3', 1: 'plain_k1m', 2: 'k1m', 3: 'k1', 4: 'tiled'}


def patch_conv_route(shape, c_skip, c_prev, grid, c_out, k=1, padding=0, padding_mode='reflect', groups=1, scale=False, shift=None,
                     act=ACT_NONE, coords=False, prev_size=None, ld=0, bank_aligned=True, aligned8=True):
    """(route, form) of ``patch_conv`` for a stage of ``shape`` = (B, H, W) (hs_patch_conv_route): ('plain_dw3', 'pairs' | 'single'),
    ('plain_k1m', 'mt2_kq1_px2_affine'), ('k1m', 'rt3_al4_prev1'), ('k1', 'pwl2_split4') or ('tiled', 'th35_tw64_2x2').  ``scale`` /
    ``shift`` / ``act``: the epilogue as given to ``patch_conv`` (truth values; shift defaults to scale).  ``ld``: the bank's row stride
    (0: the packed row rounded up to 4).  ``bank_aligned`` / ``aligned8``: 16-byte alignment of the bank, 8-byte alignment of x and y.
    Host only."""
    si = _stage_probe(shape, c_skip, c_prev, coords, prev_size)
    cin = 2 * bool(coords) + c_skip + c_prev
    if ld == 0:
        ld = _round_up(c_out * max(cin // groups, 1) * k * k, 4)
    shift = scale if shift is None else shift
    f = (C.c_int32 * 4)()
    r = _route(_hip.lib.hs_patch_conv_route(C.byref(si), grid[0], grid[1], ld, c_out, k, padding, PAD_MODES[padding_mode], groups,
                                            int(bool(scale)), int(bool(shift)), int(act), int(bool(bank_aligned)), int(bool(aligned8)), f),
               'hs_patch_conv_route')
    if r is None:
        return None
    form = [('pairs' if f[0] else 'single'), f'mt{f[0]}_kq{f[1]}_px{f[2]}' + ('_affine' if f[3] else ''), f'rt{f[0]}_al{f[1]}_prev{f[2]}',
            f'pwl{f[0]}_split{f[1]}', f'th{f[0]}_tw{f[1]}_{f[2]}x{f[3]}'][r]
    return CONV_ROUTES[r], form


BWD_ROUTES = {0: 'dw3', 1: 'tiny', 2: 'k1m', 3: 'generic'}
_BWD_LOADS = {0: 'scalar', 1: 'vec', 2: 'pairs'}


def patch_conv_bwd_route(which, shape, c_in, grid, c_out, k=1, padding=0, padding_mode='reflect', groups=1, dtype=torch.float32, align=(0, 0),
                         ld=0):
    """(route, form) of the backward of ``patch_conv`` for x of ``shape`` = (B, H, W) and ``c_in`` channels (hs_patch_conv_bwd_route):
    ``which`` = 'input' -> ('dw3', 'pairs' | 'single'), ('tiny', ''), ('k1m', 'ct2_kq1_px2'), ('generic', ''); ``which`` = 'weight' ->
    ('dw3', 'pairs' | 'single'), ('tiny', ''), ('k1m', 'mt2_nt1_vec' | '..._pairs' | '..._scalar'), ('generic', 'ob6_blocks2_lds64' |
    '..._lds150').  ``align``: the addresses modulo 16 of (dy, dx) / (x, dy).  ``ld``: the bank's row stride (0: the packed row).  Host only."""
    code = {'input': 0, 'weight': 1}[which]
    if ld == 0:
        ld = c_out * max(c_in // groups, 1) * k * k
    r, f = C.c_int32(-1), (C.c_int32 * 4)()
    _hip.run.hs_patch_conv_bwd_route(code, DTYPE_CODES[dtype], int(align[0]) % 16, int(align[1]) % 16, ld, shape[0], c_in, shape[1], shape[2],
                                     grid[0], grid[1], c_out, k, padding, PAD_MODES[padding_mode], groups, C.byref(r), f)
    route = BWD_ROUTES[r.value]
    if route == 'dw3':
        return route, 'pairs' if f[0] else 'single'
    if route == 'k1m':
        return route, f'ct{f[0]}_kq{f[1]}_px{f[2]}' if code == 0 else f'mt{f[0]}_nt{f[1]}_{_BWD_LOADS[f[2]]}'
    if route == 'generic' and code == 1:
        return route, f'ob{f[0]}_blocks{f[1]}_lds{150 if f[2] else 64}'
    return route, ''


def ir_tile_map(reg, mode, pwr):
    """(n_pixel_tiles, array (n_tiles, 16, 3) of (u, v, live)) -- the fused inverted-residual kernel's tile map
    (host-side introspection, no GPU needed)."""
    import numpy as np
    nt, nt3 = C.c_int32(0), C.c_int32(0)
    _hip.run.hs_ir_tile_map(reg, mode, pwr, C.byref(nt), C.byref(nt3), None, 0)
    buf = (C.c_int32 * (nt.value * 48))()
    _hip.run.hs_ir_tile_map(reg, mode, pwr, C.byref(nt), C.byref(nt3), buf, nt.value * 48)
    return nt3.value, np.ctypeslib.as_array(buf).reshape(nt.value, 16, 3).copy()


class ExclusiveWorkspaces:
    """Zero-initialised device buffers that belong to ONE launch at a time, for kernels that keep protocol state in memory across
    launches (csrc/hs_se_tail.h: generation words + tagged granules; the state a launch leaves is the state the next one expects,
    so a buffer may serve any number of launches IN SEQUENCE but never two at once).

    ``take(device, signature, nbytes)``: eager calls get the buffer of (current stream, signature) -- launches of one stream are
    ordered.  Calls made while a HIP graph is being captured get a buffer that belongs to THAT capture (and is kept alive for as long
    as this object lives: the graph's kernel arguments point at it): prepared, zeroed spares are handed out, because an allocation
    inside a capture would put its zero-fill into the graph and wipe the state at every replay -- correct, but a memset node per use.
    Spares are topped up by every eager call, so "run eagerly once, then capture" (what every capture site of this repository does:
    lazily built buffers have to exist before a capture anyway) never allocates inside a capture; ``captured_zero_fills`` counts the
    times it had to.  A capture is recognised by the eager -> capturing transition seen here: two captures with no eager call
    between them share buffers, which is only wrong if their graphs are then replayed concurrently."""
    SPARES = 2

    def __init__(self):
        self._lock = threading.Lock()
        self._eager, self._spares, self._captured = {}, {}, {}
        self._epoch, self._was_capturing = 0, False
        self.captured_zero_fills = 0

    @staticmethod
    def _zeros(device, nbytes):
        return torch.zeros((nbytes + 7) // 8, dtype=torch.int64, device=device)

    def take(self, device, signature, nbytes):
        capturing = torch.cuda.is_current_stream_capturing()
        stream = torch.cuda.current_stream(device).cuda_stream
        with self._lock:
            if capturing and not self._was_capturing:
                self._epoch += 1
            self._was_capturing = capturing
            skey = (device.index, signature, nbytes)
            if capturing:
                key = (stream, self._epoch) + skey
                t = self._captured.get(key)
                if t is None:
                    pool = self._spares.get(skey)
                    if pool:
                        t = pool.pop()
                    else:
                        self.captured_zero_fills += 1
                        t = self._zeros(device, nbytes)
                    self._captured[key] = t
                return t
            key = (stream,) + skey
            t = self._eager.get(key)
            if t is None:
                t = self._eager[key] = self._zeros(device, nbytes)
            pool = self._spares.setdefault(skey, [])
            while len(pool) < self.SPARES:
                pool.append(self._zeros(device, nbytes))
            return t


SE_WORKSPACES = ExclusiveWorkspaces()
# Opt-in (HS_SE_TAIL=1): measured on the MI355X (visits r5v7 / r5v8, profiles/round5_se_tail_negative.txt) the tails are correct
# (tests/test_hip_encoder.py runs them whatever this says) but cost 5-9 us per block -- two memory-side hand-offs of ~2.5 us each --
# against the 5.3 / 9.6 us of the launches they remove: 0.796 ms per HyperSeg-M frame against 0.776.
SE_TAIL = os.environ.get('HS_SE_TAIL', '0') != '0'


def se_tail_descriptor(device, batch, channels, nblk, wgs_per_batch, w_reduce, b_reduce, w_expand_t, b_expand):
    """(hs_se_tail struct, gate tensor, keep-alive tuple) for a pooling launch that finishes the squeeze-excite gate itself
    (include/hyperseg_hip.h hs_se_tail), or None when the shape is not covered (the caller then pools and calls :func:`se_gate`)."""
    csq = w_reduce.shape[0]
    nbytes = int(_hip.lib.hs_se_tail_workspace(batch, channels, csq, nblk, wgs_per_batch))
    if nbytes <= 0:
        return None
    ws = SE_WORKSPACES.take(device, (batch, channels, csq, nblk, int(wgs_per_batch)), nbytes)
    gate = torch.empty(batch, channels, device=device, dtype=torch.float32)
    d = _hip.SeTailC()
    d.w_reduce, d.b_reduce = _hip.dev_ptr(w_reduce, 'w_reduce'), _hip.dev_ptr(b_reduce, 'b_reduce')
    d.w_expand_t, d.b_expand = _hip.dev_ptr(w_expand_t, 'w_expand_t'), _hip.dev_ptr(b_expand, 'b_expand')
    d.c_squeezed = csq
    d.gate, d.squeezed, d.workspace = gate.data_ptr(), None, ws.data_ptr()
    return d, gate, ws


def se_tail_error(ws, batch):
    """The error word of a tail workspace (nonzero: a bounded wait gave up and the gate of that launch is NaN); synchronises."""
    return int(ws[batch].item())


@_on_operand_device
def depthwise_conv_bn_act(x, weight, stride, pad_top, pad_left, out_size, scale=None, shift=None, act=0, pool=False,
                          in_scale=None, in_shift=None, se=None):
    """Depthwise conv (k 3|5, stride 1|2, TF-"SAME" zero padding given as top/left offsets) + affine + activation
    (3 = swish) in one launch.  ``pool=True`` also returns the per-workgroup partial sums of the outputs (B*C, nblk)
    for :func:`se_gate`.  ``in_scale``/``in_shift`` (C): the taps are swish(in_scale*x + in_shift) -- x is then the RAW
    output of the 1x1 expand GEMM.  ``se=(w_reduce, b_reduce, w_expand_t, b_expand)`` with ``pool=True``: the launch finishes the
    squeeze-excite gate itself where it can (hs_depthwise_conv_se_fwd) and returns (y, gate (B, C), True) instead of
    (y, partial, False).  Encoder-side helper, opt-in (utils/inference.py)."""
    b, c, h, w = x.shape
    k = weight.shape[-1]
    ho, wo = out_size
    y = torch.empty(b, c, ho, wo, device=x.device, dtype=torch.float32)
    if se is not None and pool and SE_TAIL:
        nblk = _hip.lib.hs_depthwise_pool_blocks(ho, wo)
        desc = se_tail_descriptor(x.device, b, c, nblk, c * nblk, *se)
        if desc is not None:
            d, gate, _ws = desc
            _hip.run.hs_depthwise_conv_se_fwd(_hip.dev_ptr(x, 'x'), b, c, h, w, _hip.dev_ptr(weight, 'weight'), k, stride,
                                              pad_top, pad_left, ho, wo,
                                              _hip.dev_ptr(scale, 'scale') if scale is not None else None,
                                              _hip.dev_ptr(shift, 'shift') if shift is not None else None, int(act), y.data_ptr(),
                                              _hip.dev_ptr(in_scale, 'in_scale') if in_scale is not None else None,
                                              _hip.dev_ptr(in_shift, 'in_shift') if in_shift is not None else None,
                                              C.byref(d), _hip.stream_ptr())
            return y, gate, True
    partial = None
    if pool:
        partial = torch.empty(b * c, _hip.lib.hs_depthwise_pool_blocks(ho, wo), device=x.device, dtype=torch.float32)
    _hip.run.hs_depthwise_conv_fwd(_hip.dev_ptr(x, 'x'), b, c, h, w, _hip.dev_ptr(weight, 'weight'), k, stride,
                                   pad_top, pad_left, ho, wo,
                                   _hip.dev_ptr(scale, 'scale') if scale is not None else None,
                                   _hip.dev_ptr(shift, 'shift') if shift is not None else None, int(act),
                                   y.data_ptr(), partial.data_ptr() if pool else None,
                                   _hip.dev_ptr(in_scale, 'in_scale') if in_scale is not None else None,
                                   _hip.dev_ptr(in_shift, 'in_shift') if in_shift is not None else None,
                                   _hip.stream_ptr())
    if se is not None and pool:
        return y, partial, False
    return (y, partial) if pool else y


@_on_operand_device
def stem_conv_bn_swish(x, weight, pad_top, pad_left, out_size, scale, shift):
    """3x3 stride-2 conv of the 3-channel image + folded BN + swish, one launch (encoder stem).  Opt-in helper."""
    b, cin, h, w = x.shape
    cout = weight.shape[0]
    ho, wo = out_size
    y = torch.empty(b, cout, ho, wo, device=x.device, dtype=torch.float32)
    _hip.run.hs_stem_conv_fwd(_hip.dev_ptr(x, 'x'), b, cin, h, w, _hip.dev_ptr(weight, 'weight'), cout, pad_top, pad_left,
                              ho, wo, _hip.dev_ptr(scale, 'scale'), _hip.dev_ptr(shift, 'shift'), y.data_ptr(),
                              _hip.stream_ptr())
    return y


# uint8 frames into the stem + depthwise launch itself wherever the model allows (models/_common.py); 0: always one image_ingest launch
# in front of the float route (profiles/uint8_ingest_time.txt has both)
U8_STEM = os.environ.get('HS_U8_STEM', '1') != '0'
_LAYOUT_CODES = {'hwc': 0, 'chw': 1}                       # HS_LAYOUT_* of include/hyperseg_hip.h


@_on_operand_device
def image_ingest(x_u8, norm, out=None):
    """uint8 frames -> the float32 image (B, 3, H, W) of the reference's ToTensor + Normalize, one launch (hs_image_ingest_fwd).
    ``x_u8``: (B, H, W, 3) or (B, 3, H, W) as ``norm.layout`` says (``norm``: a ``utils.inference.InputNorm``); the values are
    looked up in ``norm``'s table, so the result equals the host transform bit for bit.  ``out``: a contiguous float32
    (B, 3, H, W) tensor on the same device to write into."""
    b, h, w = norm.frame_size(x_u8)
    if out is None:
        out = torch.empty(b, 3, h, w, device=x_u8.device, dtype=torch.float32)
    elif not isinstance(out, torch.Tensor) or tuple(out.shape) != (b, 3, h, w) or out.device != x_u8.device:
        raise ValueError(f'out must be a float32 tensor of shape {(b, 3, h, w)} on {x_u8.device}')
    _hip.run.hs_image_ingest_fwd(_hip.dev_ptr(x_u8, 'x_u8', torch.uint8), _LAYOUT_CODES[norm.layout], b, 3, h, w,
                                 _hip.dev_ptr(norm.table(x_u8.device), 'table'), _hip.dev_ptr(out, 'out'), _hip.stream_ptr())
    return out


@_on_operand_device
def stem_dw(x, w_stem28, scale0, shift0, stem_pad_top, stem_pad_left, stem_out_size, w_dw, pad_top, pad_left, scale1, shift1, pool=True):
    """The encoder's stem (3x3 stride-2 conv of the image + BN + swish) and the first block's depthwise 3x3 + BN + swish (+ SE
    pooling partial sums) in ONE launch: the stem's output map never reaches HBM (hs_stem_dw_fwd).  ``w_stem28``: the stem weight
    flattened to (Cmid, 27) plus one zero column.  Returns ``(y, partial)`` / ``y``, or ``None`` when the launch does not cover the
    shape (the caller then runs the two launches).  ``x`` may be a :class:`U8Frame`: the launch then reads the uint8 frame itself
    (hs_stem_dw_u8_fwd; same values as on ``image_ingest``'s result), and where it does not cover the shape the frame is ingested
    and handed to the float form.  Encoder-side helper, opt-in."""
    b, _, h, w = x.shape
    cmid, k = w_dw.shape[0], w_dw.shape[-1]
    hs_, ws_ = stem_out_size
    y = torch.empty(b, cmid, hs_, ws_, device=x.device, dtype=torch.float32)
    partial = torch.empty(b * cmid, _hip.lib.hs_mbconv_tiles(k, 1, hs_, ws_), device=x.device, dtype=torch.float32) if pool else None
    if isinstance(x, U8Frame):
        st = _hip.lib.hs_stem_dw_u8_fwd(_hip.dev_ptr(x.data, 'x', torch.uint8), _LAYOUT_CODES[x.norm.layout],
                                        _hip.dev_ptr(x.norm.table(x.device), 'table'), b, h, w, _hip.dev_ptr(w_stem28, 'w_stem28'), cmid,
                                        _hip.dev_ptr(scale0, 'scale0'), _hip.dev_ptr(shift0, 'shift0'), stem_pad_top, stem_pad_left, hs_, ws_,
                                        _hip.dev_ptr(w_dw, 'w_dw'), k, pad_top, pad_left, _hip.dev_ptr(scale1, 'scale1'),
                                        _hip.dev_ptr(shift1, 'shift1'), y.data_ptr(), partial.data_ptr() if pool else None, _hip.stream_ptr())
        if st == -3:                   # HS_ERR_UNSUPPORTED: nothing was launched -- the float form on the ingested frame
            return stem_dw(x.float_image(), w_stem28, scale0, shift0, stem_pad_top, stem_pad_left, stem_out_size, w_dw, pad_top, pad_left,
                           scale1, shift1, pool=pool)
        _hip.check(st, 'hs_stem_dw_u8_fwd')
        return (y, partial) if pool else y
    st = _hip.lib.hs_stem_dw_fwd(_hip.dev_ptr(x, 'x'), b, h, w, _hip.dev_ptr(w_stem28, 'w_stem28'), cmid, _hip.dev_ptr(scale0, 'scale0'),
                                 _hip.dev_ptr(shift0, 'shift0'), stem_pad_top, stem_pad_left, hs_, ws_, _hip.dev_ptr(w_dw, 'w_dw'), k,
                                 pad_top, pad_left, _hip.dev_ptr(scale1, 'scale1'), _hip.dev_ptr(shift1, 'shift1'), y.data_ptr(),
                                 partial.data_ptr() if pool else None, _hip.stream_ptr())
    if st == -3:                       # HS_ERR_UNSUPPORTED: nothing was launched
        return None
    _hip.check(st, 'hs_stem_dw_fwd')
    return (y, partial) if pool else y


@_on_operand_device
def mbconv_expand_dw(x, w_expand, scale0, shift0, w_dw, stride, pad_top, pad_left, out_size, scale1, shift1, pool=True, se=None):
    """1x1 expand + BN + swish + depthwise k x k (TF-"SAME" zero padding of the ACTIVATION) + BN + swish in one launch
    (+ SE pooling partial sums): the expanded tensor never reaches HBM.  x (B,Cin,H,W), w_expand (Cmid,Cin[,1,1]),
    w_dw (Cmid,1,k,k) -> y (B,Cmid,Ho,Wo)[, partial (B*Cmid, ntiles)].  ``se``: as in :func:`depthwise_conv_bn_act`
    (hs_mbconv_expand_dw_se_fwd; returns (y, gate | partial, bool)).  Encoder-side helper, opt-in."""
    b, cin, h, w = x.shape
    cmid, k = w_dw.shape[0], w_dw.shape[-1]
    ho, wo = out_size
    y = torch.empty(b, cmid, ho, wo, device=x.device, dtype=torch.float32)
    if se is not None and pool and SE_TAIL:
        nblk = _hip.lib.hs_mbconv_tiles(k, stride, ho, wo)
        desc = se_tail_descriptor(x.device, b, cmid, nblk, int(_hip.lib.hs_mbconv_se_workgroups(b, cmid, k, stride, ho, wo)), *se)
        if desc is not None:
            d, gate, _ws = desc
            _hip.run.hs_mbconv_expand_dw_se_fwd(_hip.dev_ptr(x, 'x'), b, cin, h, w, _hip.dev_ptr(w_expand, 'w_expand'), cmid,
                                                _hip.dev_ptr(scale0, 'scale0'), _hip.dev_ptr(shift0, 'shift0'),
                                                _hip.dev_ptr(w_dw, 'w_dw'), k, stride, pad_top, pad_left, ho, wo,
                                                _hip.dev_ptr(scale1, 'scale1'), _hip.dev_ptr(shift1, 'shift1'), y.data_ptr(),
                                                C.byref(d), _hip.stream_ptr())
            return y, gate, True
    partial = None
    if pool:
        partial = torch.empty(b * cmid, _hip.lib.hs_mbconv_tiles(k, stride, ho, wo), device=x.device, dtype=torch.float32)
    _hip.run.hs_mbconv_expand_dw_fwd(_hip.dev_ptr(x, 'x'), b, cin, h, w, _hip.dev_ptr(w_expand, 'w_expand'), cmid,
                                     _hip.dev_ptr(scale0, 'scale0'), _hip.dev_ptr(shift0, 'shift0'),
                                     _hip.dev_ptr(w_dw, 'w_dw'), k, stride, pad_top, pad_left, ho, wo,
                                     _hip.dev_ptr(scale1, 'scale1'), _hip.dev_ptr(shift1, 'shift1'), y.data_ptr(),
                                     partial.data_ptr() if pool else None, _hip.stream_ptr())
    if se is not None and pool:
        return y, partial, False
    return (y, partial) if pool else y


@_on_operand_device
def pointwise_conv(x, weight, gate=None, scale=None, shift=None, act=0, residual=None):
    """1x1 conv (fp32 MFMA GEMM) + optional input gate (B,Cin) + affine + activation (3 = swish) + residual, one launch."""
    b, cin, h, w = x.shape
    cout = weight.shape[0]
    y = torch.empty(b, cout, h, w, device=x.device, dtype=torch.float32)
    opt = lambda t, n: _hip.dev_ptr(t, n) if t is not None else None   # noqa: E731
    _hip.run.hs_pointwise_conv_fwd(_hip.dev_ptr(x, 'x'), b, cin, h * w, _hip.dev_ptr(weight, 'weight'), cout,
                                   opt(gate, 'gate'), opt(scale, 'scale'), opt(shift, 'shift'), int(act),
                                   opt(residual, 'residual'), y.data_ptr(), _hip.stream_ptr())
    return y


@_on_operand_device
def affine_act_(x, scale, shift, act=0, residual=None):
    """In place: x = act(scale[c]*x + shift[c]) + residual  (folded BN + activation + skip add, one launch);
    ``scale=None`` means 1."""
    b, c, h, w = x.shape
    _hip.run.hs_affine_act_fwd(_hip.dev_ptr(x, 'x'), b, c, h * w,
                               _hip.dev_ptr(scale, 'scale') if scale is not None else None,
                               _hip.dev_ptr(shift, 'shift'), int(act),
                               _hip.dev_ptr(residual, 'residual') if residual is not None else None, x.data_ptr(),
                               _hip.stream_ptr())
    return x


@_on_operand_device
def se_gate(partial, batch, hw, w_reduce, b_reduce, w_expand, b_expand, w_proj=None, out_scale=None):
    """Squeeze-excite gate from pooled partial sums; with ``w_proj`` (Cout, C[,1,1]) returns the project weights scaled by
    the gate (and by ``out_scale`` (Cout), the project conv's folded BN scale), (B, Cout, C, 1, 1); otherwise the gate
    (B, C).  One launch for blocks with small reduce weights (C <= 768, Csq <= 32), else two (squeeze, excite)."""
    c = partial.shape[0] // batch
    csq = w_reduce.shape[0]
    dev = partial.device
    w_scaled = None
    cout = 0
    work = torch.empty(batch, c + csq, device=dev, dtype=torch.float32)      # gate | squeezed activations
    gate, squeezed = work[:, :c], work[:, c:]
    if batch > 1:
        gate, squeezed = torch.empty(batch, c, device=dev), torch.empty(batch, csq, device=dev)
    if w_proj is not None:
        cout = w_proj.shape[0]
        w_scaled = torch.empty(batch, cout, c, 1, 1, device=dev, dtype=torch.float32)
    _hip.run.hs_se_gate_fwd(_hip.dev_ptr(partial, 'partial'), batch, c, partial.shape[1], 1.0 / float(hw),
                            _hip.dev_ptr(w_reduce, 'w_reduce'), _hip.dev_ptr(b_reduce, 'b_reduce'), csq,
                            _hip.dev_ptr(w_expand, 'w_expand'), _hip.dev_ptr(b_expand, 'b_expand'),
                            squeezed.data_ptr(), gate.data_ptr(),
                            _hip.dev_ptr(w_proj, 'w_proj') if w_proj is not None else None, cout,
                            _hip.dev_ptr(out_scale, 'out_scale') if out_scale is not None else None,
                            _hip.ptr(w_scaled), _hip.stream_ptr())
    return w_scaled if w_proj is not None else gate


def _route(code, what):
    """A route query's answer: None for HS_ERR_UNSUPPORTED (the launcher refuses the shape), HipLibraryError for any other error."""
    if code == -3:
        return None
    if code < 0:
        _hip.check(code, what)
    return code


_DW_FORMS = {0: 'generic', 1: 'vector', 2: 'tiled'}
_MB_FORMS = {0: 'full', 1: 'lean', 2: 'stem'}
SE_ROUTES = {0: 'fused', 1: 'early', 2: 'fused_wide', 3: 'two_launch'}


def depthwise_route(shape, k, stride, pad_left, out_size, prologue=False, aligned=True):
    """Which instantiation ``depthwise_conv_bn_act`` launches for x of ``shape`` = (B, C, H, W) (include/hyperseg_hip.h,
    hs_depthwise_route): 'tiled_k5s1' | 'vector_k3s2_pl1' | 'generic_k3s2' ..., None where the launcher refuses.  ``aligned``: x is
    16-byte aligned (the allocator's tensors are).  Host only."""
    b, c, h, w = shape
    r = _route(_hip.lib.hs_depthwise_route(b, c, h, w, k, stride, pad_left, out_size[0], out_size[1], int(bool(aligned)), int(bool(prologue))),
               'hs_depthwise_route')
    if r is None:
        return None
    form, name = _DW_FORMS[r >> 8], f'k{(r >> 4) & 15}s{(r >> 2) & 3}'
    return f'{form}_{name}_pl{r & 3}' if form == 'vector' else f'{form}_{name}'


def mbconv_route(shape, c_mid, k, stride, out_size, aligned=True, se_tail=False):
    """Which kernel ``mbconv_expand_dw`` launches for x of ``shape`` = (B, Cin, H, W): 'lean_k3s1' | 'full_k5s2' ..., None where the
    launcher refuses (hs_mbconv_route).  ``aligned``: y, scale0 and shift0 are 16-byte aligned.  Host only."""
    b, cin, h, w = shape
    r = _route(_hip.lib.hs_mbconv_route(b, cin, h, w, c_mid, k, stride, out_size[0], out_size[1], int(bool(aligned)), int(bool(se_tail))),
               'hs_mbconv_route')
    return None if r is None else f'{_MB_FORMS[r >> 8]}_k{(r >> 4) & 15}s{r & 15}'


def stem_dw_route(size, c_mid, stem_pad_top, stem_pad_left, stem_out_size, k=3, aligned=True):
    """'stem_k3s1' where ``stem_dw`` launches for an image of ``size`` = (H, W), None where it returns None (hs_stem_dw_route).  Host only."""
    r = _route(_hip.lib.hs_stem_dw_route(size[0], size[1], c_mid, stem_pad_top, stem_pad_left, stem_out_size[0], stem_out_size[1], k,
                                         int(bool(aligned))), 'hs_stem_dw_route')
    return None if r is None else f'{_MB_FORMS[r >> 8]}_k{(r >> 4) & 15}s{r & 15}'


def se_gate_route(channels, nblk, c_squeezed, w_proj=False, aligned=True):
    """The form ``se_gate`` takes: 'fused' | 'early' | 'fused_wide' | 'two_launch', None where it refuses (hs_se_gate_route).  ``aligned``: partial and
    w_reduce are 16-byte aligned.  Host only."""
    r = _route(_hip.lib.hs_se_gate_route(channels, nblk, c_squeezed, int(bool(w_proj)), int(bool(aligned))), 'hs_se_gate_route')
    return None if r is None else SE_ROUTES[r]


STEM_ROUTES = {0: 'generic', 1: 'vector_pl0', 2: 'vector_pl1'}


def stem_route(width, pad_left, aligned=True):
    """The form ``stem_conv_bn_swish`` takes for an image ``width`` wide: 'vector_pl0' | 'vector_pl1' | 'generic' (hs_stem_route).  Host only."""
    return STEM_ROUTES[_route(_hip.lib.hs_stem_route(width, pad_left, int(bool(aligned))), 'hs_stem_route')]


def pointwise_route(batch, c_in, c_out, pixels, aligned=True):
    """The instantiation ``pointwise_conv`` launches: 'vec_nb6' (interleaved 16-byte form) | 'nt4_nb6' | 'nt2_nb1' | 'nt1_nb2' ... with nb
    = ceil(c_in / 16) and nt the 16-pixel tiles per wave; None for c_in > 128 (hs_pointwise_route).  ``aligned``: x, y and the residual
    are 16-byte aligned.  Host only."""
    r = _route(_hip.lib.hs_pointwise_route(batch, c_in, c_out, pixels, int(bool(aligned))), 'hs_pointwise_route')
    if r is None:
        return None
    return f'vec_nb{r >> 8}' if r & 1 else f'nt{(r >> 4) & 15}_nb{r >> 8}'


class SplitWeights:
    """A static 1x1-conv weight prepared for ``hs_gemm_split_fwd``: f16 hi / lo pieces of the power-of-two row-scaled weight in
    MFMA-fragment order + the inverse row scales (include/hyperseg_hip.h)."""
    __slots__ = ('frag', 'inv', 'c_out', 'c_in', 'kp')

    def __init__(self, frag, inv, c_out, c_in, kp):
        self.frag, self.inv, self.c_out, self.c_in, self.kp = frag, inv, c_out, c_in, kp


@torch.no_grad()
def gemm_split_weights(w, row_scale=None, max_k=1280):
    """``w`` (Cout, Cin[, 1, 1]) f32 -> SplitWeights, or None when the kernel does not cover Cin (> 1280; the 2x2 / stride-2
    form of ``gemm_split_conv2x2`` takes K = 4 Cin up to 2560: ``max_k=2560`` with the (Cout, Cin, 2, 2) weight).  ``row_scale``
    (Cout): folded into the rows first (a BatchNorm scale).  Torch tensor ops only; runs once per weight."""
    w = w.detach().flatten(1).float()
    m, k = w.shape
    kp = _hip.lib.hs_gemm_split_kp(k) if k <= max_k else -1
    if kp < 0:
        return None
    if row_scale is not None:
        w = w * row_scale.detach().float()[:, None]
    # 2^(141 - eb), eb = biased exponent of the row maximum clamped to [27, 254]: row * scale < 2^15 (gs_exp_of / gs_scale_of)
    eb = (w.abs().amax(1).contiguous().view(torch.int32) >> 23).clamp(27, 254)
    one = torch.ones(m, device=w.device)
    ws = w * torch.ldexp(one, 141 - eb)[:, None]
    hi = ws.half()
    lo = (ws - hi.float()).half()
    rt = -(-m // 16)
    pad = (0, kp - k, 0, 16 * rt - m)
    hi, lo = torch.nn.functional.pad(hi, pad), torch.nn.functional.pad(lo, pad)
    inv = torch.nn.functional.pad(torch.ldexp(one, eb - 141), (0, 16 * rt - m), value=1.0)

    def fragment_order(t):      # [RT][16 rows][KST][4 kgroups][8] -> [RT][KST][kgroup][row][8]: lane = row + 16 * kgroup
        return t.view(rt, 16, kp // 32, 4, 8).permute(0, 2, 3, 1, 4)
    frag = torch.stack([fragment_order(hi), fragment_order(lo)], dim=2).contiguous()
    return SplitWeights(frag, inv.contiguous(), m, k, kp)


@_on_operand_device
def gemm_split(sw, x, gate=None, shift=None, act=ACT_NONE, residual=None, out=None):
    """y (B, Cout, H, W) = act(W @ (gate[:, :, None] * x) + shift[:, None]) + residual per frame, on the f16 matrix cores with
    split operands (hs_gemm_split_fwd).  ``out``: written in place; ``residual`` may be ``out`` itself (accumulation onto a
    skip tensor).  ``act``: ACT_* or 3 = swish."""
    b, cin, h, w = x.shape
    if cin != sw.c_in:
        raise ValueError(f'input has {cin} channels, the weight {sw.c_in}')
    shape = (b, sw.c_out, h, w)
    if out is None:
        out = torch.empty(shape, device=x.device, dtype=torch.float32)
    elif tuple(out.shape) != shape:
        raise ValueError(f'out has shape {tuple(out.shape)}, expected {shape}')
    if residual is not None and tuple(residual.shape) != shape:
        raise ValueError(f'residual has shape {tuple(residual.shape)}, expected {shape}')
    if gate is not None and tuple(gate.shape) != (b, cin):
        raise ValueError(f'gate has shape {tuple(gate.shape)}, expected {(b, cin)}')
    if shift is not None and shift.numel() != sw.c_out:
        raise ValueError(f'shift has {shift.numel()} entries, expected {sw.c_out}')
    _hip.run.hs_gemm_split_fwd(_hip.dev_ptr(sw.frag, 'w_frag', torch.float16), _hip.dev_ptr(sw.inv, 'w_inv'),
                               _hip.dev_ptr(gate, 'gate') if gate is not None else None, _hip.dev_ptr(x, 'x'),
                               _hip.dev_ptr(shift, 'shift') if shift is not None else None, int(act),
                               _hip.dev_ptr(residual, 'residual') if residual is not None else None,
                               _hip.dev_ptr(out, 'out'), b, sw.c_out, cin, sw.kp, h * w, _hip.stream_ptr())
    return out


def gemm_split_se_route(channels, nblk, c_squeezed, c_out, pixels, aligned=True):
    """The form ``gemm_split_se`` launches: 'ks2_w8' ... (k-steps per wave, waves per workgroup), None where it refuses -- anything
    but a shape for which ``se_gate`` is 'fused' and ``gemm_split`` a paired-load single-chunk launch (hs_gemm_split_se_route).
    ``aligned``: partial and w_reduce are 16-byte aligned.  Host only."""
    r = _route(_hip.lib.hs_gemm_split_se_route(channels, nblk, c_squeezed, c_out, pixels, int(bool(aligned))), 'hs_gemm_split_se_route')
    return None if r is None else f'ks{r >> 4}_w{r & 15}'


@_on_operand_device
def gemm_split_se(sw, x, partial, hw, w_reduce, b_reduce, w_expand_t, b_expand, shift=None, act=ACT_NONE, residual=None, out=None,
                  gate_out=None, squeezed_out=None):
    """``gemm_split(sw, x, gate=se_gate(partial, B, hw, w_reduce, b_reduce, w_expand_t, b_expand), ...)`` as ONE launch: every
    workgroup of the GEMM derives the gate from the pool partial sums (B C, nblk) itself (hs_gemm_split_se_fwd); the result equals
    the composed route's bit for bit.  ``gate_out`` (B, C) / ``squeezed_out`` (B, Csq): optional f32 tensors that receive the gate
    and the squeezed activations.  Raises HipLibraryError where ``gemm_split_se_route`` answers None."""
    b, cin, h, w = x.shape
    if cin != sw.c_in:
        raise ValueError(f'input has {cin} channels, the weight {sw.c_in}')
    shape = (b, sw.c_out, h, w)
    if out is None:
        out = torch.empty(shape, device=x.device, dtype=torch.float32)
    elif tuple(out.shape) != shape:
        raise ValueError(f'out has shape {tuple(out.shape)}, expected {shape}')
    if residual is not None and tuple(residual.shape) != shape:
        raise ValueError(f'residual has shape {tuple(residual.shape)}, expected {shape}')
    if shift is not None and shift.numel() != sw.c_out:
        raise ValueError(f'shift has {shift.numel()} entries, expected {sw.c_out}')
    if partial.dim() != 2 or partial.shape[0] != b * cin:
        raise ValueError(f'partial has shape {tuple(partial.shape)}, expected ({b * cin}, nblk)')
    csq = w_reduce.shape[0]
    if w_reduce.numel() != csq * cin or b_reduce.numel() != csq:
        raise ValueError(f'w_reduce / b_reduce have {w_reduce.numel()} / {b_reduce.numel()} entries, expected {csq * cin} / {csq}')
    if tuple(w_expand_t.shape) != (csq, cin) or b_expand.numel() != cin:
        raise ValueError(f'w_expand_t has shape {tuple(w_expand_t.shape)} and b_expand {b_expand.numel()} entries, expected {(csq, cin)} and {cin}')
    if gate_out is not None and tuple(gate_out.shape) != (b, cin):
        raise ValueError(f'gate_out has shape {tuple(gate_out.shape)}, expected {(b, cin)}')
    if squeezed_out is not None and tuple(squeezed_out.shape) != (b, csq):
        raise ValueError(f'squeezed_out has shape {tuple(squeezed_out.shape)}, expected {(b, csq)}')
    _hip.run.hs_gemm_split_se_fwd(_hip.dev_ptr(sw.frag, 'w_frag', torch.float16), _hip.dev_ptr(sw.inv, 'w_inv'),
                                  _hip.dev_ptr(partial, 'partial'), partial.shape[1], 1.0 / float(hw),
                                  _hip.dev_ptr(w_reduce, 'w_reduce'), _hip.dev_ptr(b_reduce, 'b_reduce'), csq,
                                  _hip.dev_ptr(w_expand_t, 'w_expand_t'), _hip.dev_ptr(b_expand, 'b_expand'), _hip.dev_ptr(x, 'x'),
                                  _hip.dev_ptr(shift, 'shift') if shift is not None else None, int(act),
                                  _hip.dev_ptr(residual, 'residual') if residual is not None else None,
                                  _hip.dev_ptr(out, 'out'), b, sw.c_out, cin, sw.kp, h * w,
                                  _hip.dev_ptr(gate_out, 'gate_out') if gate_out is not None else None,
                                  _hip.dev_ptr(squeezed_out, 'squeezed_out') if squeezed_out is not None else None, _hip.stream_ptr())
    return out


@_on_operand_device
def gemm_split_conv2x2(sw, x, shift=None, act=ACT_NONE, out=None, pool_partial=None):
    """y (B, Cout, H/2, W/2) = act(Conv2d(kernel 2, stride 2)(x) + shift[:, None, None]) on the f16 matrix cores with split
    operands, the window read on load (hs_gemm_split_conv2x2_fwd; no im2col copy).  ``sw`` = gemm_split_weights(conv.weight
    (Cout, Cin, 2, 2), scale, max_k=2560).  ``pool_partial``: a (B, Cout, ceil(H W / 64)) f32 tensor that receives the sums of y
    over blocks of 16 pixels (``pooled_shift`` turns them into the global average's contribution)."""
    b, cin, h, w = x.shape
    if 4 * cin != sw.c_in:
        raise ValueError(f'input has {cin} channels, the weight {sw.c_in} / 4')
    if h % 2 or w % 4:
        raise ValueError(f'map {h}x{w}: height must be even and width a multiple of 4')
    shape = (b, sw.c_out, h // 2, w // 2)
    if out is None:
        out = torch.empty(shape, device=x.device, dtype=torch.float32)
    elif tuple(out.shape) != shape:
        raise ValueError(f'out has shape {tuple(out.shape)}, expected {shape}')
    if shift is not None and shift.numel() != sw.c_out:
        raise ValueError(f'shift has {shift.numel()} entries, expected {sw.c_out}')
    nblk = -(-(h // 2) * (w // 2) // 16)
    if pool_partial is not None and tuple(pool_partial.shape) != (b, sw.c_out, nblk):
        raise ValueError(f'pool_partial has shape {tuple(pool_partial.shape)}, expected {(b, sw.c_out, nblk)}')
    _hip.run.hs_gemm_split_conv2x2_fwd(_hip.dev_ptr(sw.frag, 'w_frag', torch.float16), _hip.dev_ptr(sw.inv, 'w_inv'),
                                       _hip.dev_ptr(x, 'x'), _hip.dev_ptr(shift, 'shift') if shift is not None else None,
                                       int(act), _hip.dev_ptr(out, 'out'),
                                       _hip.dev_ptr(pool_partial, 'pool_partial') if pool_partial is not None else None,
                                       b, sw.c_out, cin, sw.kp, h // 2, w // 2, _hip.stream_ptr())
    return out


@_on_operand_device
def gemm_split_up2(sw, x, shift=None, act=ACT_NONE, out=None):
    """nearest-2x upsample of act(W @ x + shift): (B, Cin, H, W) -> (B, Cout, 2H, 2W), the small map never stored
    (hs_gemm_split_up2_fwd).  ``out``: e.g. the right half of the context head's signal."""
    b, cin, h, w = x.shape
    if cin != sw.c_in:
        raise ValueError(f'input has {cin} channels, the weight {sw.c_in}')
    shape = (b, sw.c_out, 2 * h, 2 * w)
    if out is None:
        out = torch.empty(shape, device=x.device, dtype=torch.float32)
    elif tuple(out.shape) != shape:
        raise ValueError(f'out has shape {tuple(out.shape)}, expected {shape}')
    if shift is not None and shift.numel() != sw.c_out:
        raise ValueError(f'shift has {shift.numel()} entries, expected {sw.c_out}')
    _hip.run.hs_gemm_split_up2_fwd(_hip.dev_ptr(sw.frag, 'w_frag', torch.float16), _hip.dev_ptr(sw.inv, 'w_inv'),
                                   _hip.dev_ptr(x, 'x'), _hip.dev_ptr(shift, 'shift') if shift is not None else None,
                                   int(act), _hip.dev_ptr(out, 'out'), b, sw.c_out, cin, sw.kp, h, w, _hip.stream_ptr())
    return out


@_on_operand_device
def pooled_shift(pool_partial, pixels, wb, shift):
    """shift + wb @ mean, mean = the global average whose 16-pixel block sums ``pool_partial`` (1, C, nblk) holds
    (hs_pooled_shift_fwd): the pooled half of ``cat(feat, pooled.expand_as(feat))`` in front of a 1x1 conv, as a row constant."""
    _, c, nblk = pool_partial.shape
    m = shift.numel()
    if pool_partial.shape[0] != 1 or tuple(wb.shape) != (m, c):
        raise ValueError(f'pool_partial {tuple(pool_partial.shape)} / wb {tuple(wb.shape)} / shift {m}: expected (1, C, nblk), (M, C), M')
    out = torch.empty(m, device=shift.device, dtype=torch.float32)
    _hip.run.hs_pooled_shift_fwd(_hip.dev_ptr(pool_partial, 'pool_partial'), nblk, 1.0 / pixels, _hip.dev_ptr(wb, 'wb'),
                                 _hip.dev_ptr(shift, 'shift'), _hip.dev_ptr(out, 'shift_out'), m, c, _hip.stream_ptr())
    return out


@_on_operand_device
def upsample_bilinear(x, size, out=None):
    """F.interpolate(x, size, mode='bilinear', align_corners=False).  ``out``: a contiguous (B, C, *size) f32 tensor on x's device
    to write into (a collective's send slot: hyperseg_amd.distributed.LogitsGatherer.slot); ignored if it does not fit."""
    b, c, hi, wi = x.shape
    ho, wo = size
    if out is not None and tuple(out.shape) == (b, c, ho, wo) and out.dtype == torch.float32 and out.device == x.device and out.is_contiguous():
        y = out
    else:
        y = torch.empty(b, c, ho, wo, device=x.device, dtype=torch.float32)
    _hip.run.hs_upsample_bilinear_fwd(_hip.dev_ptr(x, 'x'), b, c, hi, wi, ho, wo, y.data_ptr(),
                                      _hip.stream_ptr())
    return y


@_on_operand_device
def upsample_argmax(x, size):
    """``F.interpolate(x, size, 'bilinear', align_corners=False).argmax(1)`` as uint8 masks (B, Ho, Wo), one launch; the
    upsampled logits never exist in memory.  Bit-identical to ``upsample_bilinear(x, size).argmax(1)``."""
    b, c, hi, wi = x.shape
    ho, wo = size
    mask = torch.empty(b, ho, wo, device=x.device, dtype=torch.uint8)
    _hip.run.hs_upsample_argmax_fwd(_hip.dev_ptr(x, 'x'), b, c, hi, wi, ho, wo, mask.data_ptr(), _hip.stream_ptr())
    return mask


_EVAL_DTYPES = {torch.uint8: 0, torch.int64: 1}          # hs_eval_dtype of include/hyperseg_hip.h


def eval_max_classes():
    """Largest ``num_classes`` the two evaluation kernels take (their per-workgroup LDS histogram); beyond it they raise
    NotImplementedError and the caller counts with stock ops (``fps.ConfusionMatrix``)."""
    return int(_hip.lib.hs_eval_max_classes())


def _eval_labels(t, name):
    if not isinstance(t, torch.Tensor) or t.dtype not in _EVAL_DTYPES:
        raise ValueError(f'{name} must be a uint8 or int64 tensor, got {getattr(t, "dtype", type(t))}')
    if not t.is_cuda:
        raise ValueError(f'{name} is on {t.device}: the evaluation kernels run on the GPU (fps.ConfusionMatrix.update counts CPU tensors)')
    return t if t.is_contiguous() else t.contiguous()


def _eval_out(out, shape, device):
    if out is None:
        return torch.zeros(shape, dtype=torch.int64, device=device)
    if not isinstance(out, torch.Tensor) or out.dtype != torch.int64 or tuple(out.shape) != tuple(shape) or out.device != device \
            or not out.is_contiguous():
        raise ValueError(f'out must be a contiguous int64 tensor of shape {tuple(shape)} on {device}, got '
                         f'{getattr(out, "dtype", type(out))} {tuple(getattr(out, "shape", ()))} on {getattr(out, "device", None)}')
    return out


def _eval_classes(num_classes):
    n = int(num_classes)
    if n <= 0:
        raise ValueError(f'num_classes must be positive, got {num_classes}')
    if n > eval_max_classes():
        raise NotImplementedError(f'num_classes = {n}: the evaluation kernels cover up to {eval_max_classes()} classes')
    return n


def _logits_shape(x):
    if not isinstance(x, torch.Tensor) or x.dim() != 4:
        raise ValueError('x must be (B, C, Hi, Wi) logits')
    return x.shape


def _eval_target(target, shape, x):
    """``target`` as the kernels read it: uint8 or int64, of ``shape`` = (B, Ho, Wo), on the logits' device."""
    target = _eval_labels(target, 'target')
    if tuple(target.shape) != shape:
        raise ValueError(f'target has shape {tuple(target.shape)}, expected {shape}')
    if target.device != x.device:
        raise ValueError(f'target is on {target.device}, the logits on {x.device}')
    return target


def _score_out(num_classes, channels, out, batch, per_image, device, counted=False):
    """(n, matrix) of the scoring entries.  The two loss + score entries: ``num_classes=None`` counts nothing (loss and masks only).
    ``counted`` (the two upsample + count entries): there is always a count, and what the uint8 masks rule out -- more channels than
    classes, more than 256 classes -- is a ValueError before the kernels' own limit is a NotImplementedError."""
    if counted:
        if channels > int(num_classes):
            raise ValueError(f'{channels} logit channels but num_classes = {num_classes}')
        if int(num_classes) > 256:
            raise ValueError('num_classes > 256: the masks are uint8')
    elif num_classes is None:
        if out is not None:
            raise ValueError('out= needs num_classes: nothing is counted without it')
        if channels > 256:
            raise ValueError('more than 256 logit channels: the masks are uint8')
        return 0, None
    n = _eval_classes(num_classes)            # NotImplementedError above eval_max_classes() (<= 256: the masks are uint8)
    if channels > n:
        raise ValueError(f'{channels} logit channels but num_classes = {num_classes}')
    return n, _eval_out(out, (batch, n, n) if per_image else (n, n), device)


def _scoring_operands(x, sizes, target, num_classes, out, per_image, counted=False, masks=True, loss=False):
    """What the four scoring wrappers share.  ``sizes``: what follows (Hi, Wi) in the entry's argument list -- (Ho, Wo), or (Hm, Wm, Ho, Wo) --
    the target's size last.  Checks the logits, the target and the matrix (``_score_out``), allocates the masks and the per-pixel losses that
    were asked for, and returns ``(head, tail, out, mask, loss)``: the entry is called with ``*head, *tail`` -- a loss entry puts the ignore
    index and the losses between the two."""
    b, c, hi, wi = _logits_shape(x)
    ho, wo = sizes[-2:]
    target = _eval_target(target, (b, ho, wo), x)
    n, out = _score_out(num_classes, c, out, b, per_image, x.device, counted=counted)
    xp = _hip.dev_ptr(x, 'x')
    loss = torch.empty(b, ho, wo, device=x.device, dtype=torch.float32) if loss else None
    mask = torch.empty(b, ho, wo, device=x.device, dtype=torch.uint8) if masks else None
    head = (xp, b, c, hi, wi, *sizes, target.data_ptr(), _EVAL_DTYPES[target.dtype])
    tail = (n, 1 if per_image else 0, _hip.ptr(out), _hip.ptr(mask), _hip.stream_ptr())
    return head, tail, out, mask, loss


def _size2(size, name):
    h, w = (int(s) for s in size)
    if h <= 0 or w <= 0:
        raise ValueError(f'{name} must be a positive (H, W), got {tuple(size)}')
    return h, w


def _label_stages(x, mid_size, target):
    """The two stages of a wrapper at the label's resolution: ``(target, (hm, wm, ho, wo), one_stage)`` -- ``one_stage``: the target is at
    ``mid_size`` already, or ``x`` is, and the one-stage wrapper serves, resizing straight to (ho, wo)."""
    b, _, hi, wi = _logits_shape(x)
    hm, wm = _size2(mid_size, 'mid_size')
    target = _eval_labels(target, 'target')
    if target.dim() != 3 or target.shape[0] != b:
        raise ValueError(f'target has shape {tuple(target.shape)}, expected ({b}, Ho, Wo)')
    ho, wo = int(target.shape[1]), int(target.shape[2])
    return target, (hm, wm, ho, wo), (ho, wo) == (hm, wm) or (hi, wi) == (hm, wm)


@_on_operand_device
def upsample_confusion(x, size, target, num_classes, out=None, per_image=False, masks=False):
    """``upsample_argmax(x, size)`` with every output pixel counted against ``target`` (B, Ho, Wo; uint8 or int64) in the same
    launch (hs_upsample_confusion_fwd): ``out[t, p] += 1`` for every pixel whose target ``t`` is in [0, num_classes), every
    other target value ignored (seg_utils.py:15-17).  ``out``: an int64 (n, n) -- ``per_image``: (B, n, n) -- matrix to
    ACCUMULATE into; None allocates a zeroed one.  Returns ``out``, or ``(out, masks)`` with ``masks=True`` (the uint8 masks,
    bit-identical to ``upsample_argmax``'s).  Nothing here reads the device: the call is capturable in a HIP graph."""
    ho, wo = (int(s) for s in size)
    head, tail, out, mask, _ = _scoring_operands(x, (ho, wo), target, num_classes, out, per_image, counted=True, masks=masks)
    _hip.run.hs_upsample_confusion_fwd(*head, *tail)
    return (out, mask) if masks else out


@_on_operand_device
def upsample2_confusion(x, mid_size, target, num_classes, out=None, per_image=False, masks=False):
    """``upsample_confusion`` at the LABEL's resolution: the logits ``x`` (B, C, Hi, Wi) are resized to ``mid_size`` (the frame's size,
    where the model's logits live) and from there to ``target``'s size (test.py:167-168), arg-maxed and counted against ``target``
    (B, Ho, Wo; uint8 or int64) in one launch (hs_upsample2_confusion_fwd); neither resized tensor exists in memory.  Masks and
    counts are bit-identical to ``upsample_bilinear(upsample_bilinear(x, mid_size), target.shape[1:]).argmax(1)`` and its count.
    ``out``, ``per_image``, ``masks``, the returned value and the errors raised are ``upsample_confusion``'s, which this simply
    calls when the target is at ``mid_size`` already (or ``x`` is).  Nothing here reads the device: the call is capturable."""
    target, sizes, one_stage = _label_stages(x, mid_size, target)
    if one_stage:
        return upsample_confusion(x, sizes[2:], target, num_classes, out=out, per_image=per_image, masks=masks)
    head, tail, out, mask, _ = _scoring_operands(x, sizes, target, num_classes, out, per_image, counted=True, masks=masks)
    _hip.run.hs_upsample2_confusion_fwd(*head, *tail)
    return (out, mask) if masks else out


@_on_operand_device
def upsample2_argmax(x, mid_size, size):
    """uint8 masks (B, *size) of the logits ``x`` resized to ``mid_size`` and from there to ``size``, one launch with nothing counted
    (hs_upsample2_confusion_fwd without a target); neither resized tensor exists in memory.  Bit-identical to
    ``upsample_bilinear(upsample_bilinear(x, mid_size), size).argmax(1)``; ``upsample_argmax`` where one of the stages is the identity."""
    b, c, hi, wi = _logits_shape(x)
    (hm, wm), (ho, wo) = _size2(mid_size, 'mid_size'), _size2(size, 'size')
    if (ho, wo) == (hm, wm) or (hi, wi) == (hm, wm):
        return upsample_argmax(x, (ho, wo))
    mask = torch.empty(b, ho, wo, device=x.device, dtype=torch.uint8)
    _hip.run.hs_upsample2_confusion_fwd(_hip.dev_ptr(x, 'x'), b, c, hi, wi, hm, wm, ho, wo, None, 0, 0, 0, None, mask.data_ptr(),
                                        _hip.stream_ptr())
    return mask


@_on_operand_device
def confusion_update(pred, target, num_classes, out=None, per_image=False):
    """The same counting from finished predictions (hs_confusion_fwd): ``pred`` and ``target`` uint8 or int64 of one shape;
    with ``per_image`` their first dimension is the image and ``out`` is (B, n, n).  A prediction outside [0, num_classes) is
    not counted.  Returns ``out`` (accumulated into when given, else a new zeroed matrix plus this call's counts)."""
    pred, target = _eval_labels(pred, 'pred'), _eval_labels(target, 'target')
    if pred.shape != target.shape or pred.numel() == 0:
        raise ValueError(f'pred {tuple(pred.shape)} and target {tuple(target.shape)} must have one non-empty shape')
    if pred.device != target.device:
        raise ValueError(f'pred is on {pred.device}, target on {target.device}')
    n = _eval_classes(num_classes)
    b = pred.shape[0] if per_image else 1
    if per_image and pred.dim() < 2:
        raise ValueError('per_image needs a leading image dimension')
    out = _eval_out(out, (b, n, n) if per_image else (n, n), pred.device)
    _hip.run.hs_confusion_fwd(pred.data_ptr(), _EVAL_DTYPES[pred.dtype], target.data_ptr(), _EVAL_DTYPES[target.dtype], b,
                              pred.numel() // b, n, 1 if per_image else 0, out.data_ptr(), _hip.stream_ptr())
    return out


# Flip and pyramid inference (the reference's list-input mode, hyperseg_v1_0.py:71-91) merged in the forward's last launch (hs_tta_merge_fwd).
# HS_TTA_MERGE=0 (or TTA_MERGE = False) sends every model through the composed route, tta_merge_composed: the same bits.
TTA_MERGE = os.environ.get('HS_TTA_MERGE', '1') != '0'
TTA_MAX_PASSES = 8                                         # HS_TTA_MAX_PASSES of include/hyperseg_hip.h
TtaMerged = collections.namedtuple('TtaMerged', 'logits masks out')


def _tta_passes(passes):
    """The pass list checked: ``[(x, (hm, wm), flipped, entry), ...]`` with x contiguous-checked later; returns (passes, b, c, (ho, wo))."""
    passes = [(x, _size2(mid, 'mid_size'), bool(flipped), int(entry)) for x, mid, flipped, entry in passes]
    if not passes:
        raise ValueError('passes is empty')
    b, c = _logits_shape(passes[0][0])[:2]
    last = -1
    for i, (x, mid, _, entry) in enumerate(passes):
        if tuple(_logits_shape(x)[:2]) != (b, c) or x.device != passes[0][0].device:
            raise ValueError(f'pass {i}: x is {tuple(x.shape)} on {x.device}, pass 0 is ({b}, {c}, ., .) on {passes[0][0].device}')
        if entry not in (last, last + 1) or (entry == last and mid != passes[i - 1][1]):
            raise ValueError('passes are sorted by entry, entries 0, 1, ... without a gap, one mid_size per entry')
        last = entry
    return passes, b, c, passes[0][1]


def tta_merge_takes(n_passes, channels, num_classes=None):
    """What hs_tta_merge_fwd launches for (a host predicate: the model's route rule and ``tta_merge``'s own refusals): at most 8 passes, at
    most 256 logit channels and, where it counts, at most ``eval_max_classes()`` classes."""
    return n_passes <= TTA_MAX_PASSES and channels <= 256 and (num_classes is None or int(num_classes) <= min(256, eval_max_classes()))


def _tta_gather_max(gather):
    if gather not in ('mean', 'max'):
        raise ValueError(f"gather must be 'mean' or 'max', got {gather!r}")
    return gather != 'mean'


@_on_operand_device
def tta_merge(passes, gather, target=None, num_classes=None, out=None, per_image=False, logits=False, masks=True):
    """The reference's list-input inference (hyperseg_v1_0.py:76-89) from the decoder's per-pass outputs in ONE launch (hs_tta_merge_fwd).
    ``passes``: a list of ``(x, mid_size, flipped, entry)`` -- x f32 (B, C, Hi, Wi), what the decoder hands to its final resize;
    ``mid_size`` that pass's frame size; ``flipped``: the pass ran on the mirrored frame; ``entry``: its pyramid entry (sorted, from 0).
    Per entry the passes are resized to ``mid_size`` (a flipped one mirrored back) and their max taken, an entry of another size than
    entry 0's is resized to it, and the entries are folded in order -- ``gather`` 'mean': ``(p + out) * 0.5``, 'max': ``max(p, out)``.
    Returns ``TtaMerged(logits, masks, out)``: the f32 logits (B, C, Ho, Wo) with ``logits=True``, the uint8 arg-max masks with
    ``masks=True``, and with ``target`` (B, Ho, Wo; uint8 or int64) the int64 matrix ``out`` ((n, n), ``per_image``: (B, n, n)) with this
    call's (target, prediction) counts ACCUMULATED (``upsample_confusion``'s rule); what was not asked for is None.  Bit-identical to
    ``tta_merge_composed`` for finite inputs; none of the per-pass, per-entry or merged logits exist in memory unless asked for.  More than
    8 passes, more than 256 channels or more classes than ``eval_max_classes()``: NotImplementedError (``tta_merge_takes``; the caller
    takes the composed route).  Nothing here reads the device: the call is capturable."""
    passes, b, c, (ho, wo) = _tta_passes(passes)
    gather_max = _tta_gather_max(gather)
    dev = passes[0][0].device
    if not (logits or masks or target is not None):
        raise ValueError('nothing asked for: logits, masks or a target to count against')
    n, tp, tdtype = 0, None, 0
    if target is not None:
        target = _eval_target(target, (b, ho, wo), passes[0][0])
        if num_classes is None:
            raise ValueError('a target needs num_classes')
        if c > int(num_classes):
            raise ValueError(f'{c} logit channels but num_classes = {num_classes}')
        if int(num_classes) > 256:
            raise ValueError('num_classes > 256: the masks are uint8')
        n = _eval_classes(num_classes)
        tp, tdtype = target.data_ptr(), _EVAL_DTYPES[target.dtype]
    elif out is not None:
        raise ValueError('out= needs a target: nothing is counted without it')
    if not tta_merge_takes(len(passes), c):
        raise NotImplementedError(f'{len(passes)} passes of {c} channels: the merge launch takes up to {TTA_MAX_PASSES} passes of up to 256')
    table = (_hip.TtaPassC * len(passes))()
    for rec, (x, (hm, wm), flipped, entry) in zip(table, passes):
        rec.x, rec.Hi, rec.Wi, rec.Hm, rec.Wm, rec.flipped, rec.entry = _hip.dev_ptr(x, 'x'), x.shape[2], x.shape[3], hm, wm, flipped, entry
    out = _eval_out(out, (b, n, n) if per_image else (n, n), dev) if target is not None else None
    y = torch.empty(b, c, ho, wo, device=dev, dtype=torch.float32) if logits else None
    mask = torch.empty(b, ho, wo, device=dev, dtype=torch.uint8) if masks else None
    _hip.run.hs_tta_merge_fwd(table, len(passes), b, c, 1 if gather_max else 0, tp, tdtype, ho, wo, n, 1 if per_image else 0,
                              _hip.ptr(out), _hip.ptr(mask), _hip.ptr(y), _hip.stream_ptr())
    return TtaMerged(y, mask, out)


def tta_merge_composed(passes, gather, target=None, num_classes=None, out=None, per_image=False, logits=False, masks=True):
    """``tta_merge`` stated with one launch per step -- the route ``HyperGenBase.forward`` took for a list before the merge launch and
    takes with ``TTA_MERGE`` off: ``upsample_bilinear`` per pass (none where x is at ``mid_size``), ``torch.flip`` and ``torch.max`` per
    entry, ``upsample_bilinear`` per entry of another size than entry 0's, the fold, ``argmax`` and ``confusion_update``.  On CPU tensors
    the resizes are ``F.interpolate(..., 'bilinear')`` and the count ``fps.ConfusionMatrix``'s: the reference's statement."""
    passes, b, c, size = _tta_passes(passes)
    gather_max = _tta_gather_max(gather)
    cuda = passes[0][0].is_cuda

    def resize(t, to):
        if tuple(t.shape[2:]) == tuple(to):
            return t
        return upsample_bilinear(t.contiguous(), to) if cuda else torch.nn.functional.interpolate(t, size=to, mode='bilinear')

    merged, i = None, 0
    while i < len(passes):
        entry, mid, y = passes[i][3], passes[i][1], None
        while i < len(passes) and passes[i][3] == entry:
            x, _, flipped, _ = passes[i]
            v = resize(x, mid)
            v = torch.flip(v, [-1]) if flipped else v
            y = v if y is None else torch.max(y, v)
            i += 1
        y = resize(y, size)
        merged = y if merged is None else (torch.max(y, merged) if gather_max else (y + merged) * 0.5)
    mask = merged.argmax(1).to(torch.uint8) if (masks or target is not None) else None
    if target is not None:
        if tuple(target.shape) != (b,) + tuple(size):
            raise ValueError(f'target has shape {tuple(target.shape)}, expected {(b,) + tuple(size)}')
        if cuda:
            out = confusion_update(mask, target, num_classes, out=out, per_image=per_image)
        else:
            from .fps import ConfusionMatrix
            n = int(num_classes)
            out = torch.zeros((b, n, n) if per_image else (n, n), dtype=torch.int64) if out is None else out
            for k in range(b) if per_image else (slice(None),):
                cm = ConfusionMatrix(n)
                cm.update_stock(target[k].flatten().long(), mask[k].flatten().long())
                (out[k] if per_image else out).add_(cm.mat)
    elif out is not None:
        raise ValueError('out= needs a target: nothing is counted without it')
    return TtaMerged(merged if logits else None, mask if masks else None, out if target is not None else None)


def class_weight_table(weight, classes, device, what='weight'):
    """The class-weight table as the weighted cross-entropy launches read it (here and in ``autograd``): None, or the fp32 (C,) contiguous
    tensor on the logits' device, detached; anything else raises.  Its VALUES -- finite, >= 0 -- are the caller's word
    (``training.weight_fusable`` checks them once per table): nothing here reads the device."""
    if weight is None:
        return None
    if not isinstance(weight, torch.Tensor) or weight.dtype != torch.float32 or tuple(weight.shape) != (classes,) or weight.device != device \
            or not weight.is_contiguous():
        raise ValueError(f'{what} must be a contiguous float32 ({classes},) tensor on {device}, got {getattr(weight, "dtype", type(weight))} '
                         f'{tuple(getattr(weight, "shape", ()))} on {getattr(weight, "device", None)}')
    return weight.detach()


# loss entry -> (its class-weighted twin, where the twin's argument list takes the table: after the target, or after the target's type code)
_WEIGHTED_TWINS = {'hs_cross_entropy_typed_fwd': ('hs_cross_entropy_weighted_fwd', 3), 'hs_cross_entropy_typed_bwd': ('hs_cross_entropy_weighted_bwd', 3),
                   'hs_bootstrapped_ce_fwd': ('hs_bootstrapped_ce_weighted_fwd', 3), 'hs_bootstrapped_ce_bwd': ('hs_bootstrapped_ce_weighted_bwd', 3),
                   'hs_cross_entropy_score_fwd': ('hs_cross_entropy_score_weighted_fwd', 3),
                   'hs_upsample_ce_confusion_fwd': ('hs_upsample_ce_confusion_weighted_fwd', 9),
                   'hs_upsample2_ce_confusion_fwd': ('hs_upsample2_ce_confusion_weighted_fwd', 11)}


def loss_launch(entry, table, *args):
    """``entry(*args)`` -- with a class-weight ``table`` (``class_weight_table``'s) the weighted twin, the table's pointer spliced in."""
    if table is None:
        return getattr(_hip.run, entry)(*args)
    twin, at = _WEIGHTED_TWINS[entry]
    return getattr(_hip.run, twin)(*args[:at], table.data_ptr(), *args[at:])


@_on_operand_device
def cross_entropy_score(logits, target, ignore_index, num_classes, out=None, per_image=False, masks=False, weight=None):
    """The per-pixel cross entropy of (B, C, H, W) logits (f32 / bf16 / f16) against int64 ``target`` (B, H, W) AND the batch's score, one
    launch (hs_cross_entropy_score_fwd): returns ``(loss, out)`` -- ``(loss, out, masks)`` with ``masks=True``.  ``loss`` (B, H, W) f32 is
    ``autograd.PixelCrossEntropy``'s bit for bit (0 where the target is ``ignore_index`` or outside [0, C)); the masks are
    ``logits.argmax(1)`` as uint8; ``out[t, p] += 1`` for every pixel whose target is in [0, num_classes) -- ``confusion_update``'s rule,
    which does not know ``ignore_index``: an in-range ignored pixel has loss 0 and is still counted, as in the reference's train.py.
    ``out`` follows ``upsample_confusion``'s convention (accumulated into when given, a new zeroed matrix otherwise; (B, n, n) with
    ``per_image``); ``num_classes=None`` counts nothing and returns ``out`` None.  ``weight``: the fp32 (C,) class-weight table on the
    logits' device (hs_cross_entropy_score_weighted_fwd) -- ``loss`` is then the weighted ``PixelCrossEntropy``'s bit for bit, masks and
    counts are as without.  Nothing here reads the device: capturable (a graph holds the table's address)."""
    if not isinstance(logits, torch.Tensor) or logits.dim() != 4 or logits.dtype not in DTYPE_CODES:
        raise ValueError('logits must be (B, C, H, W) float32, bfloat16 or float16')
    b, c, h, w = logits.shape
    target = _eval_target(target, (b, h, w), logits)
    if target.dtype != torch.int64:
        raise ValueError(f'target must be int64 (what the loss takes), got {target.dtype}')
    n, out = _score_out(num_classes, c, out, b, per_image, logits.device)
    xp = _hip.dev_ptr(logits, 'logits', logits.dtype)
    loss = torch.empty(b, h, w, device=logits.device, dtype=torch.float32)
    mask = torch.empty(b, h, w, device=logits.device, dtype=torch.uint8) if masks else None
    tail = (loss.data_ptr(), n, 1 if per_image else 0, _hip.ptr(out), mask.data_ptr() if masks else None, _hip.stream_ptr())
    loss_launch('hs_cross_entropy_score_fwd', class_weight_table(weight, c, logits.device),
                DTYPE_CODES[logits.dtype], xp, target.data_ptr(), b, c, h * w, int(ignore_index), *tail)
    return (loss, out, mask) if masks else (loss, out)


@_on_operand_device
def upsample_ce_confusion(x, size, target, ignore_index, num_classes, out=None, per_image=False, weight=None):
    """The validation step's last launch (hs_upsample_ce_confusion_fwd): ``x`` (B, C, Hi, Wi) f32 resized to ``size`` in registers, and from
    each output pixel's scores its cross entropy against ``target`` (B, Ho, Wo; uint8 or int64), its class and its count.  Returns
    ``(loss, out, masks)``: ``loss`` (B, Ho, Wo) f32 bit-identical to ``PixelCrossEntropy`` on ``upsample_bilinear(x, size)``, the uint8
    masks to ``upsample_argmax``'s, the counts to ``upsample_confusion``'s (``out``, ``per_image`` and the errors raised: that
    function's; ``num_classes=None``: nothing counted, ``out`` None).  ``weight``: the fp32 (C,) class-weight table on ``x``'s device
    (hs_upsample_ce_confusion_weighted_fwd): ``loss`` is the weighted ``PixelCrossEntropy``'s, masks and counts as without.  The resized
    logits never exist in memory.  Capturable (a graph holds the table's address)."""
    head, tail, out, mask, loss = _scoring_operands(x, _size2(size, 'size'), target, num_classes, out, per_image, loss=True)
    loss_launch('hs_upsample_ce_confusion_fwd', class_weight_table(weight, x.shape[1], x.device), *head, int(ignore_index), loss.data_ptr(), *tail)
    return loss, out, mask


@_on_operand_device
def upsample2_ce_confusion(x, mid_size, target, ignore_index, num_classes, out=None, per_image=False, weight=None):
    """``upsample_ce_confusion`` at the LABEL's resolution (hs_upsample2_ce_confusion_fwd): the logits ``x`` (B, C, Hi, Wi) f32 are resized
    to ``mid_size`` (the frame's size, where the model's logits live) and from there to ``target``'s size (train.py:119-120), both resizes
    composed in registers, and from each label pixel's scores come its cross entropy against ``target`` (B, Ho, Wo; uint8 or int64), its
    class and its count -- one launch; neither resized tensor exists in memory.  Returns ``(loss, out, masks)``: ``loss`` (B, Ho, Wo) f32
    bit-identical to ``PixelCrossEntropy`` on ``upsample_bilinear(upsample_bilinear(x, mid_size), target.shape[1:])``, masks and counts to
    ``upsample2_confusion``'s.  ``ignore_index``, ``num_classes``, ``out``, ``per_image``, ``weight`` and the errors raised are
    ``upsample_ce_confusion``'s, which this simply calls when the target is at ``mid_size`` already (or ``x`` is).  Capturable."""
    target, sizes, one_stage = _label_stages(x, mid_size, target)
    if one_stage:
        return upsample_ce_confusion(x, sizes[2:], target, ignore_index, num_classes, out=out, per_image=per_image, weight=weight)
    head, tail, out, mask, loss = _scoring_operands(x, sizes, target, num_classes, out, per_image, loss=True)
    loss_launch('hs_upsample2_ce_confusion_fwd', class_weight_table(weight, x.shape[1], x.device), *head, int(ignore_index), loss.data_ptr(), *tail)
    return loss, out, mask


def _overlay_out(out, frames):
    if out is None:
        return torch.empty_like(frames)
    if not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or tuple(out.shape) != tuple(frames.shape) or out.device != frames.device \
            or not out.is_contiguous():
        raise ValueError(f'out must be a contiguous uint8 tensor of shape {tuple(frames.shape)} on {frames.device}, got '
                         f'{getattr(out, "dtype", type(out))} {tuple(getattr(out, "shape", ()))} on {getattr(out, "device", None)}')
    lo, hi = frames.data_ptr(), frames.data_ptr() + frames.numel()
    if out.data_ptr() < hi and lo < out.data_ptr() + out.numel():
        raise ValueError('out overlaps the frames: the overlay is written beside its input, never over it')
    return out


def _overlay_frames(frames, style, name='frames'):
    if not frames.is_cuda:
        raise ValueError(f'{name} are on {frames.device}: the overlay kernels run on the GPU (Overlay.blend blends CPU tensors)')
    return frames if frames.is_contiguous() else frames.contiguous()


@_on_operand_device
def overlay(masks, frames, style, out=None):
    """``style`` (a ``utils.inference.Overlay``) applied to finished uint8 ``masks`` (B, H, W) and the uint8 ``frames`` they belong to
    ((B, H, W, 3) or (B, 3, H, W) as ``style.layout`` says): the uint8 overlay in the frames' layout, one launch (hs_overlay_fwd), equal
    to ``style.blend`` on the CPU byte for byte.  ``out``: a contiguous uint8 tensor of the frames' shape to write into (not the frames
    themselves).  Nothing here reads the device: the call is capturable in a HIP graph."""
    style.check(frames, masks)
    frames = _overlay_frames(frames, style)
    masks = masks if masks.is_contiguous() else masks.contiguous()
    b, h, w = style.frame_size(frames)
    out = _overlay_out(out, frames)
    _hip.run.hs_overlay_fwd(masks.data_ptr(), frames.data_ptr(), _LAYOUT_CODES[style.layout], b, h, w,
                            _hip.dev_ptr(style.tables(frames.device), 'tables'), style.num_colors, style.ignore_index,
                            out.data_ptr(), _hip.stream_ptr())
    return out


@_on_operand_device
def upsample_overlay(x, size, frames, style, out=None):
    """``upsample_argmax(x, size)`` with ``style`` blended over ``frames`` (uint8, at ``size``, in ``style.layout``) as the same launch's
    epilogue (hs_upsample_overlay_fwd).  Returns ``(masks, overlay)``: the uint8 masks, bit-identical to ``upsample_argmax``'s, and the
    uint8 overlay, equal to ``overlay(masks, frames, style)``.  ``out``: as :func:`overlay`'s.  Capturable."""
    b, c, hi, wi = _logits_shape(x)
    ho, wo = (int(s) for s in size)
    if tuple(style.frame_size(frames)) != (b, ho, wo):
        raise ValueError(f'the frames are {tuple(style.frame_size(frames))} (B, H, W), the masks will be {(b, ho, wo)}')
    frames = _overlay_frames(frames, style)
    if frames.device != x.device:
        raise ValueError(f'the frames are on {frames.device}, the logits on {x.device}')
    out = _overlay_out(out, frames)
    mask = torch.empty(b, ho, wo, device=x.device, dtype=torch.uint8)
    _hip.run.hs_upsample_overlay_fwd(_hip.dev_ptr(x, 'x'), b, c, hi, wi, ho, wo, frames.data_ptr(), _LAYOUT_CODES[style.layout],
                                     _hip.dev_ptr(style.tables(x.device), 'tables'), style.num_colors, style.ignore_index,
                                     mask.data_ptr(), out.data_ptr(), _hip.stream_ptr())
    return mask, out


@_on_operand_device
def upsample2_overlay(x, mid_size, size, frames, style, out=None):
    """``upsample_overlay`` over two composed resizes (hs_upsample2_overlay_fwd): the logits ``x`` resized to ``mid_size`` (the model's
    frame) and from there to ``size`` (the camera frame's), arg-maxed and blended over ``frames`` (uint8, at ``size``, in ``style.layout``)
    in one launch; neither resized tensor exists in memory.  Returns ``(masks, overlay)``: the masks bit-identical to
    ``upsample2_argmax``'s, the overlay equal to ``overlay(masks, frames, style)``.  ``out`` and the errors raised are
    ``upsample_overlay``'s, which this simply calls where one of the stages is the identity.  Capturable."""
    b, c, hi, wi = _logits_shape(x)
    (hm, wm), (ho, wo) = _size2(mid_size, 'mid_size'), _size2(size, 'size')
    if (ho, wo) == (hm, wm) or (hi, wi) == (hm, wm):
        return upsample_overlay(x, (ho, wo), frames, style, out=out)
    if tuple(style.frame_size(frames)) != (b, ho, wo):
        raise ValueError(f'the frames are {tuple(style.frame_size(frames))} (B, H, W), the masks will be {(b, ho, wo)}')
    frames = _overlay_frames(frames, style)
    if frames.device != x.device:
        raise ValueError(f'the frames are on {frames.device}, the logits on {x.device}')
    if c > 256:
        raise ValueError('more than 256 logit channels: the masks are uint8')
    out = _overlay_out(out, frames)
    mask = torch.empty(b, ho, wo, device=x.device, dtype=torch.uint8)
    _hip.run.hs_upsample2_overlay_fwd(_hip.dev_ptr(x, 'x'), b, c, hi, wi, hm, wm, ho, wo, frames.data_ptr(), _LAYOUT_CODES[style.layout],
                                      _hip.dev_ptr(style.tables(x.device), 'tables'), style.num_colors, style.ignore_index,
                                      mask.data_ptr(), out.data_ptr(), _hip.stream_ptr())
    return mask, out


def _confidence_operands(x, size, dtype, threshold, fill, out, name='x'):
    """What the three confidence wrappers share: checks (ValueError, before any launch), the uint8 masks and the confidence tensor at
    ``(B, *size)``.  Returns ``(b, c, hi, wi, tail, mask, conf)``: an entry is called with its shape arguments followed by ``*tail``."""
    from .utils.confidence import CONF_DTYPES, check_args
    dtype, threshold, fill = check_args(dtype, threshold, fill)
    b, c, hi, wi = _logits_shape(x)
    if not x.is_cuda:
        raise ValueError(f'{name} is on {x.device}: the confidence kernels run on the GPU (utils.confidence.confidence_cpu takes CPU tensors)')
    if x.dtype != torch.float32 or not x.is_contiguous():
        raise ValueError(f'{name} must be contiguous float32 (B, C, H, W) logits, got {x.dtype}')
    if c > 256:
        raise ValueError('more than 256 logit channels: the masks are uint8')
    shape = (b,) + tuple(size)
    if out is None:
        conf = torch.empty(shape, device=x.device, dtype=dtype)
    else:
        if not isinstance(out, torch.Tensor) or out.dtype != dtype or tuple(out.shape) != shape or out.device != x.device or not out.is_contiguous():
            raise ValueError(f'out must be a contiguous {dtype} tensor of shape {shape} on {x.device}, got '
                             f'{getattr(out, "dtype", type(out))} {tuple(getattr(out, "shape", ()))} on {getattr(out, "device", None)}')
        conf = out
    mask = torch.empty(shape, device=x.device, dtype=torch.uint8)
    tail = (CONF_DTYPES[dtype], 0.0 if threshold is None else threshold, fill, mask.data_ptr(), conf.data_ptr(), _hip.stream_ptr())
    return b, c, hi, wi, tail, mask, conf


@_on_operand_device
def confidence(logits, dtype=torch.uint8, threshold=None, fill=255, out=None):
    """``(masks, conf)`` of finished fp32 logits (B, C, H, W), one launch (hs_confidence_fwd): the uint8 masks ``logits.argmax(1)`` and
    the soft-max probability of that class, ``softmax(logits, 1).max(1)``, taken in fp32 by the recurrence of csrc/hs_confidence.h --
    ``dtype`` float32, or uint8 as ``uint8(conf * 255 + 0.5)``.  ``threshold``: a pixel whose fp32 confidence is ``< threshold`` gets
    ``fill`` in the masks (pseudo-labels with an ignore value); the confidence is not changed by it.  ``out``: a contiguous ``dtype``
    (B, H, W) tensor for the confidence.  The composed route's kernel: the fused entries below give the same bits.  Capturable."""
    b, c, h, w, tail, mask, conf = _confidence_operands(logits, tuple(_logits_shape(logits)[2:]), dtype, threshold, fill, out, name='logits')
    _hip.run.hs_confidence_fwd(logits.data_ptr(), b, c, h, w, *tail)
    return mask, conf


@_on_operand_device
def upsample_confidence(x, size, dtype=torch.uint8, threshold=None, fill=255, out=None):
    """``upsample_argmax(x, size)`` with the confidence as the same launch's epilogue (hs_upsample_confidence_fwd).  Returns ``(masks,
    conf)``: the uint8 masks, bit-identical to ``upsample_argmax``'s (before the threshold), and the confidence, bit-identical to
    ``confidence(upsample_bilinear(x, size))``'s; the resized logits never exist in memory.  ``dtype``, ``threshold``, ``fill``, ``out``:
    as :func:`confidence`'s.  Capturable."""
    ho, wo = _size2(size, 'size')
    b, c, hi, wi, tail, mask, conf = _confidence_operands(x, (ho, wo), dtype, threshold, fill, out)
    _hip.run.hs_upsample_confidence_fwd(x.data_ptr(), b, c, hi, wi, ho, wo, *tail)
    return mask, conf


@_on_operand_device
def upsample2_confidence(x, mid_size, size, dtype=torch.uint8, threshold=None, fill=255, out=None):
    """``upsample_confidence`` over two composed resizes (hs_upsample2_confidence_fwd): ``x`` resized to ``mid_size`` and from there to
    ``size``, one launch; neither resized tensor exists in memory.  Masks bit-identical to ``upsample2_argmax``'s, the confidence to
    ``confidence(upsample_bilinear(upsample_bilinear(x, mid_size), size))``'s; ``upsample_confidence`` where one of the stages is the
    identity.  Capturable."""
    _, _, hi, wi = _logits_shape(x)
    (hm, wm), (ho, wo) = _size2(mid_size, 'mid_size'), _size2(size, 'size')
    if (ho, wo) == (hm, wm) or (hi, wi) == (hm, wm):
        return upsample_confidence(x, (ho, wo), dtype=dtype, threshold=threshold, fill=fill, out=out)
    b, c, hi, wi, tail, mask, conf = _confidence_operands(x, (ho, wo), dtype, threshold, fill, out)
    _hip.run.hs_upsample2_confidence_fwd(x.data_ptr(), b, c, hi, wi, hm, wm, ho, wo, *tail)
    return mask, conf


# ------------------------------------------------------------------------------------------
# uint8 frames and their labels: resize, colour jitter, blur, rotate (csrc/hs_resample.hip, hs_jitter.hip, hs_blur.hip, hs_rotate.hip).  Every wrapper
# checks its operands with the helpers below -- each raises ValueError, before any launch or host-to-device copy -- allocates, calls
# its library entry and checks the status.
# ------------------------------------------------------------------------------------------
_LABEL_DTYPES = {torch.uint8: 0, torch.int64: 1}           # HS_EVAL_U8 / HS_EVAL_I64
_FILTER_CODES = {'bilinear': 0, 'bicubic': 1}              # HS_RESIZE_* of include/hyperseg_hip.h


def _frames_bhw(x_u8, layout, name='frames'):
    """(B, H, W) of uint8 frames (B, H, W, 3) / (B, 3, H, W) as ``layout`` says."""
    if layout not in _LAYOUT_CODES:
        raise ValueError(f'layout {layout!r}: expected one of {tuple(_LAYOUT_CODES)}')
    hwc = layout == 'hwc'
    if not isinstance(x_u8, torch.Tensor) or x_u8.dtype != torch.uint8 or x_u8.dim() != 4 or x_u8.shape[3 if hwc else 1] != 3:
        raise ValueError(f'{name} must be uint8 {"(B, H, W, 3)" if hwc else "(B, 3, H, W)"}, got '
                         f'{getattr(x_u8, "dtype", type(x_u8))} {tuple(getattr(x_u8, "shape", ()))}')
    return (x_u8.shape[0],) + tuple(x_u8.shape[1:3] if hwc else x_u8.shape[2:])


def _labels_bhw(t, dtypes=_LABEL_DTYPES, name='labels'):
    """(B, H, W) of labels (B, H, W), uint8 or int64."""
    if not isinstance(t, torch.Tensor) or t.dtype not in dtypes or t.dim() != 3:
        raise ValueError(f'{name} must be {" or ".join(str(d)[6:] for d in dtypes)} (B, H, W), got {getattr(t, "dtype", type(t))} '
                         f'{tuple(getattr(t, "shape", ()))}')
    return tuple(t.shape)


def _out(out, shape, dtype, device):
    """``out`` after checking it, or a new tensor."""
    if out is None:
        return torch.empty(shape, device=device, dtype=dtype)
    if not isinstance(out, torch.Tensor) or tuple(out.shape) != tuple(shape) or out.dtype != dtype or out.device != device:
        raise ValueError(f'out must be a {dtype} tensor of shape {tuple(shape)} on {device}')
    return out


def _frame_out(out, b, h, w, layout, norm, device):
    """The frame output: float32 (B, 3, H, W) through ``norm``'s table, else uint8 in ``layout``."""
    if norm is not None:
        return _out(out, (b, 3, h, w), torch.float32, device)
    return _out(out, (b, h, w, 3) if layout == 'hwc' else (b, 3, h, w), torch.uint8, device)


def _label_out(out, shape, dtype, device):
    """The label output: ``out``, uint8 or int64, or a new ``dtype`` tensor."""
    if out is not None and (not isinstance(out, torch.Tensor) or out.dtype not in _LABEL_DTYPES):
        raise ValueError(f'out must be a uint8 or int64 tensor of shape {tuple(shape)} on {device}')
    return _out(out, shape, dtype if out is None else out.dtype, device)


def _label_fill(fill, out, name='fill'):
    fill = int(fill)
    if not (0 <= fill <= 255 or (out.dtype == torch.int64 and -2 ** 31 <= fill < 2 ** 31)):
        raise ValueError(f'{name} {fill} does not fit the output labels')
    return fill


def _fill_word(fill, name='fill'):
    """Three fill bytes (or one for all) as the word the kernels take: r | g << 8 | b << 16."""
    from .utils import rotate
    r, g, b = rotate.check_fill(fill, name)
    return r | g << 8 | b << 16


def _norm_table(norm, layout, device):
    """Pointer of ``norm``'s table on ``device`` (None without a norm).  The first use on a device copies the table there: call it after
    every other check."""
    if norm is None:
        return None
    if norm.layout != layout:
        raise ValueError(f"norm describes '{norm.layout}' frames, these are '{layout}'")
    return _hip.dev_ptr(norm.table(device), 'table')


def _param_rows(params, words, fields, device=None):
    """B of the int32 (B, ``words``) parameter tensor the batch kernels read."""
    if (not isinstance(params, torch.Tensor) or params.dtype != torch.int32 or params.dim() != 2 or params.shape[1] != words
            or params.shape[0] == 0 or not params.is_contiguous() or (device is not None and params.device != device)):
        raise ValueError(f'params must be a contiguous int32 tensor of shape (B, {words}) = {fields}{"" if device is None else f" on {device}"}; '
                         f'got {getattr(params, "dtype", type(params))} {tuple(getattr(params, "shape", ()))}')
    return params.shape[0]


def _workspace(workspace, words, device):
    if workspace is None:
        return torch.empty(words, device=device, dtype=torch.int32)
    if (not isinstance(workspace, torch.Tensor) or workspace.dtype != torch.int32 or workspace.dim() != 1 or workspace.numel() < words
            or workspace.device != device or not workspace.is_contiguous()):
        raise ValueError(f'workspace must be a contiguous int32 vector of at least {words} elements on {device}')
    return workspace


def _jitter_table(table, b, device):
    from .utils import jitter
    if (not isinstance(table, torch.Tensor) or table.dtype != torch.int32 or tuple(table.shape) != (b, jitter.TABLE_WORDS)
            or table.device != device or not table.is_contiguous()):
        raise ValueError(f'table must be a contiguous int32 tensor of shape {(b, jitter.TABLE_WORDS)} on {device}')
    return table


def _filter_code(filter):
    if filter not in _FILTER_CODES:
        raise ValueError(f'filter {filter!r}: expected one of {tuple(_FILTER_CODES)}')
    return _FILTER_CODES[filter]


def _resize_geometry(in_hw, size, view):
    from .utils import resample
    hi, wi = (int(s) for s in in_hw)
    hr, wr = (int(s) for s in size)
    if min(hi, wi, hr, wr) < 1:
        raise ValueError(f'sizes must be >= 1, got {(hi, wi)} -> {(hr, wr)}')
    return hi, wi, hr, wr, resample.check_view(view, (hr, wr))


@_on_operand_device
def frame_resize(x_u8, size, filter='bilinear', layout='hwc', view=None, norm=None, out=None):
    """uint8 frames (B, Hi, Wi, 3) / (B, 3, Hi, Wi) (``layout``) resized to ``size`` = (Hr, Wr) with ``PIL.Image.resize``'s 8-bit
    arithmetic (``filter``: 'bilinear' | 'bicubic'), byte for byte, in one launch (hs_frame_resize_fwd; the tables come from
    ``utils.resample``).  ``view`` (a ``utils.resample.ResizeView``): the (Ho, Wo) window of the resized image to produce, at a signed
    offset, optionally flipped, ``fill`` outside -- default the whole image.  Returns uint8 in the input's layout, or with ``norm`` (a
    ``utils.inference.InputNorm``) the float32 (B, 3, Ho, Wo) image looked up in its table.  ``out``: a contiguous tensor of that
    shape and dtype to write into.  Equal to ``utils.resample.frame_resize_cpu``.  Nothing here reads the device once the tables are
    uploaded (first call per geometry): capturable."""
    from .utils import resample
    b, hi, wi = _frames_bhw(x_u8, layout)
    _filter_code(filter)
    hi, wi, hr, wr, view = _resize_geometry((hi, wi), size, view)
    (ho, wo), (oy, ox) = view.size, view.offset
    out = _frame_out(out, b, ho, wo, layout, norm, x_u8.device)
    if b == 0:
        raise ValueError('empty batch')
    table = _norm_table(norm, layout, x_u8.device)
    yb, ykk = resample.device_coeffs(hi, hr, filter, x_u8.device)
    xb, xkk = resample.device_coeffs(wi, wr, filter, x_u8.device)
    _hip.run.hs_frame_resize_fwd(_hip.dev_ptr(x_u8, 'x_u8', torch.uint8), _LAYOUT_CODES[layout], b, hi, wi,
                                 yb.data_ptr(), ykk.data_ptr(), ykk.shape[1], hr, xb.data_ptr(), xkk.data_ptr(), xkk.shape[1], wr,
                                 ho, wo, oy, ox, int(view.hflip), _fill_word(view.fill), table,
                                 _hip.dev_ptr(out, 'out', out.dtype), _hip.stream_ptr())
    return out


def _raw_labels_bhw(t, codec, name='labels'):
    """(B, H, W) of labels as ``codec`` (a ``utils.labels.LabelCodec``, or None: class indices) takes them."""
    from .utils.labels import LabelCodec
    if codec is None:
        return _labels_bhw(t, name=name)
    if not isinstance(codec, LabelCodec):
        raise ValueError(f'codec must be a hyperseg_amd.LabelCodec or None, got {type(codec).__name__}')
    return codec.check_raw(t, name)


def _codec_operands(codec, device):
    """``(codec_words, codec_kind, n, unmatched)`` of the coded entries.  The first use on a device copies the words there: call it
    after every other check."""
    return (_hip.dev_ptr(codec.device_words(device), 'codec words', torch.int32), *codec.launch_operands)


@_on_operand_device
def label_encode(t, codec, out=None):
    """A dataset's label encoding on the device, one launch (hs_label_encode_fwd): raw labels -- uint8 / int64 (B, H, W) ids for
    ``LabelCodec.table``, uint8 (B, H, W, 3) colour images for ``LabelCodec.colors`` -- become class indices (B, H, W).  Returns the
    input's dtype for a table and uint8 for colours, or ``out``'s (uint8 | int64, contiguous, (B, H, W)).  Equal to
    ``codec.encode_cpu``.  Nothing is read back once the codec's words are on the device (first call per codec): capturable."""
    if codec is None:
        raise ValueError('label_encode needs a codec: hyperseg_amd.LabelCodec.table(values) or .colors(colors)')
    b, h, w = _raw_labels_bhw(t, codec)
    out = _label_out(out, (b, h, w), codec.out_dtype(t), t.device)
    if b == 0 or h == 0 or w == 0:
        raise ValueError('empty batch')
    x = _hip.dev_ptr(t, 'labels', t.dtype)
    y = _hip.dev_ptr(out, 'out', out.dtype)
    _hip.run.hs_label_encode_fwd(x, _LABEL_DTYPES[t.dtype], b, h, w, *_codec_operands(codec, t.device), y, _LABEL_DTYPES[out.dtype],
                                 _hip.stream_ptr())
    return out


@_on_operand_device
def label_resize(t, size, view=None, fill=255, out=None, codec=None):
    """Labels (B, Hi, Wi), uint8 or int64, resized to ``size`` with ``PIL.Image.resize(..., NEAREST)``'s index tables (hs_label_resize_fwd,
    one launch), then ``view`` as :func:`frame_resize`'s with ``fill`` outside (the view's own fill is the frames').  Returns the
    input's dtype, or ``out``'s (uint8 | int64, contiguous, (B, Ho, Wo)).  Equal to ``utils.resample.label_resize_cpu``.

    ``codec`` (a ``LabelCodec``): ``t`` holds RAW labels as :func:`label_encode` takes them and the same one launch encodes the pixel it
    gathers (hs_label_resize_coded_fwd); ``fill`` is stored as given, never encoded -- the reference pads after its dataset has
    encoded.  The default output is then uint8 for a colour image.  ``None``: today's entry with today's arguments."""
    from .utils import resample
    b, hi, wi = _raw_labels_bhw(t, codec)
    hi, wi, hr, wr, view = _resize_geometry((hi, wi), size, view)
    (ho, wo), (oy, ox) = view.size, view.offset
    out = _label_out(out, (b, ho, wo), t.dtype if codec is None else codec.out_dtype(t), t.device)
    if b == 0:
        raise ValueError('empty batch')
    fill = _label_fill(fill, out)
    iy, ix = resample.device_nearest(hi, hr, t.device), resample.device_nearest(wi, wr, t.device)
    if codec is None:
        _hip.run.hs_label_resize_fwd(_hip.dev_ptr(t, 'labels', t.dtype), _LABEL_DTYPES[t.dtype], b, hi, wi, iy.data_ptr(), hr, ix.data_ptr(), wr,
                                     ho, wo, oy, ox, int(view.hflip), fill, _hip.dev_ptr(out, 'out', out.dtype), _LABEL_DTYPES[out.dtype],
                                     _hip.stream_ptr())
        return out
    x, y = _hip.dev_ptr(t, 'labels', t.dtype), _hip.dev_ptr(out, 'out', out.dtype)
    _hip.run.hs_label_resize_coded_fwd(x, _LABEL_DTYPES[t.dtype], b, hi, wi, iy.data_ptr(), hr, ix.data_ptr(), wr, ho, wo, oy, ox,
                                       int(view.hflip), fill, *_codec_operands(codec, t.device), y, _LABEL_DTYPES[out.dtype],
                                       _hip.stream_ptr())
    return out


RESIZE_STATUS = {'hr': 1, 'wr': 2, 'y_taps': 4, 'x_taps': 8, 'size': 16}      # HS_RESIZE_STATUS_*: what a sample's status word sums
RESIZE_PARAM_WORDS = 6                                     # Hr, Wr, oy, ox, hflip, reserved


class ResizeTables(collections.namedtuple('ResizeTables', 'bounds kk nearest status workspace in_hw crop ks_max')):
    """The device-built tables of a batch (:func:`resize_tables`): int32 views of one ``workspace`` -- ``bounds`` (B, 2, M, 2), ``kk``
    (B, 2, M, ks_max), ``nearest`` (B, 2, M), ``status`` (B,), M = max(crop), axis 0 = y -- and the geometry they were laid out for."""
    __slots__ = ()

    @staticmethod
    def words(batch, crop, ks_max):
        return batch * 2 * max(crop) * (3 + ks_max) + batch

    @classmethod
    def over(cls, workspace, batch, in_hw, crop, ks_max):
        m = max(crop)
        sizes = (batch * 2 * m * 2, batch * 2 * m * ks_max, batch * 2 * m, batch)
        b, k, n, s = torch.split(workspace[:sum(sizes)], sizes)
        return cls(b.view(batch, 2, m, 2), k.view(batch, 2, m, ks_max), n.view(batch, 2, m), s, workspace, tuple(in_hw), tuple(crop), ks_max)


def _tables_over(cls, workspace, batch, in_hw, out_hw, ks_max, device):
    """``cls.over`` a workspace that holds the tables (default a new one): ``cls`` is ResizeTables or RaggedTables."""
    return cls.over(_workspace(workspace, cls.words(batch, out_hw, ks_max), device), batch, in_hw, out_hw, ks_max)


def _resize_params(params):
    return _param_rows(params, RESIZE_PARAM_WORDS, 'Hr, Wr, oy, ox, hflip, reserved')


def _batch_tables(tables, params, n, in_hw, device):
    """B of ``params`` after checking that ``tables`` were built for them and for the ``n`` samples of ``in_hw`` at hand."""
    b = _resize_params(params)
    if not isinstance(tables, ResizeTables):
        raise ValueError('tables must be what resize_tables returned')
    if params.device != device or tables.workspace.device != device:
        raise ValueError(f'params and tables must be on {device}')
    if tables.status.shape[0] != b or tables.in_hw != tuple(in_hw):
        raise ValueError(f'the tables were built for {tables.status.shape[0]} samples of {tables.in_hw}, these are {b} of {tuple(in_hw)}')
    if n != b:
        raise ValueError(f'{n} samples, {b} parameter rows')
    return b


@_on_operand_device
def resize_tables(params, in_hw, crop, filter, ks_max, workspace=None):
    """The resize tables of a whole batch built on the device, one launch (hs_resize_tables_fwd).  ``params``: int32 (B, 6) on the
    device = ``Hr, Wr, oy, ox, hflip, reserved`` per sample -- the resized size, the signed offset of the ``crop`` = (h, w) window in the
    resized image, its flip; ``in_hw`` the frames' (H, W); ``filter`` 'bilinear' | 'bicubic'; ``ks_max`` the tables' row width
    (``utils.resample.ks_for``).  Returns a :class:`ResizeTables` over ``workspace`` (int32, contiguous, at least
    ``ResizeTables.words(B, crop, ks_max)`` elements; default a new one): the window of ``utils.resample``'s host tables, integer for
    integer (``utils.resample.window_tables_cpu``).  ``status``: 0 per sample, or a sum of ``RESIZE_STATUS`` codes (a resized size
    below 1 or above 2^19, more taps than ``ks_max``) -- that sample's tables are empty and the resize launches write fill.  ``params`` is
    read when the kernel runs and nothing is read back: capturable."""
    b = _resize_params(params)
    code = _filter_code(filter)
    hi, wi = (int(s) for s in in_hw)
    ho, wo = (int(s) for s in crop)
    ks_max = int(ks_max)
    if min(hi, wi, ho, wo, ks_max) < 1:
        raise ValueError(f'sizes must be >= 1, got {(hi, wi)} -> {(ho, wo)}, ks_max {ks_max}')
    t = _tables_over(ResizeTables, workspace, b, (hi, wi), (ho, wo), ks_max, params.device)
    _hip.run.hs_resize_tables_fwd(_hip.dev_ptr(params, 'params', torch.int32), b, hi, wi, ho, wo, code, ks_max,
                                  t.bounds.data_ptr(), t.kk.data_ptr(), t.nearest.data_ptr(), t.status.data_ptr(), _hip.stream_ptr())
    return t


@_on_operand_device
def frame_resize_batch(x_u8, params, tables, layout='hwc', fill=(0, 0, 0), norm=None, out=None):
    """:func:`frame_resize` for a batch whose samples each have a geometry of their own, one launch (hs_frame_resize_batch_fwd): sample
    b of the uint8 frames (B, Hi, Wi, 3) / (B, 3, Hi, Wi) is resized to ``params[b]``'s (Hr, Wr) with the filter ``tables`` (a
    :class:`ResizeTables` built from the same ``params``) were made for, and the ``tables.crop`` window at its offset comes back, flipped
    where it says, ``fill`` (3 bytes) outside.  Returns uint8 in the input's layout, or with ``norm`` float32 (B, 3, h, w) through its
    table; ``out`` as :func:`frame_resize`'s.  Per sample the bytes of ``frame_resize(x[b:b+1], (Hr, Wr), view=...)``.  Capturable."""
    n, hi, wi = _frames_bhw(x_u8, layout)
    b = _batch_tables(tables, params, n, (hi, wi), x_u8.device)
    ho, wo = tables.crop
    fill = _fill_word(fill)
    out = _frame_out(out, b, ho, wo, layout, norm, x_u8.device)
    table = _norm_table(norm, layout, x_u8.device)
    _hip.run.hs_frame_resize_batch_fwd(_hip.dev_ptr(x_u8, 'x_u8', torch.uint8), _LAYOUT_CODES[layout], b, hi, wi,
                                       _hip.dev_ptr(params, 'params', torch.int32), tables.bounds.data_ptr(), tables.kk.data_ptr(),
                                       tables.status.data_ptr(), tables.ks_max, ho, wo, fill, table,
                                       _hip.dev_ptr(out, 'out', out.dtype), _hip.stream_ptr())
    return out


@_on_operand_device
def label_resize_batch(t, params, tables, fill=255, out=None, codec=None):
    """:func:`label_resize` for a batch whose samples each have a geometry of their own, one launch (hs_label_resize_batch_fwd):
    labels (B, Hi, Wi), uint8 or int64, through ``tables``' nearest indices, the ``tables.crop`` window of each sample with ``fill``
    outside.  Returns the input's dtype, or ``out``'s (uint8 | int64, contiguous, (B, h, w)).  ``codec``: raw labels, encoded by the same
    launch (hs_label_resize_batch_coded_fwd), as :func:`label_resize`'s.  Capturable."""
    n, hi, wi = _raw_labels_bhw(t, codec)
    b = _batch_tables(tables, params, n, (hi, wi), t.device)
    ho, wo = tables.crop
    out = _label_out(out, (b, ho, wo), t.dtype if codec is None else codec.out_dtype(t), t.device)
    fill = _label_fill(fill, out)
    if codec is None:
        _hip.run.hs_label_resize_batch_fwd(_hip.dev_ptr(t, 'labels', t.dtype), _LABEL_DTYPES[t.dtype], b, hi, wi,
                                           _hip.dev_ptr(params, 'params', torch.int32), tables.nearest.data_ptr(), tables.status.data_ptr(),
                                           ho, wo, fill, _hip.dev_ptr(out, 'out', out.dtype), _LABEL_DTYPES[out.dtype], _hip.stream_ptr())
        return out
    x, p, y = _hip.dev_ptr(t, 'labels', t.dtype), _hip.dev_ptr(params, 'params', torch.int32), _hip.dev_ptr(out, 'out', out.dtype)
    _hip.run.hs_label_resize_batch_coded_fwd(x, _LABEL_DTYPES[t.dtype], b, hi, wi, p, tables.nearest.data_ptr(), tables.status.data_ptr(),
                                             ho, wo, fill, *_codec_operands(codec, t.device), y, _LABEL_DTYPES[out.dtype], _hip.stream_ptr())
    return out


@_on_operand_device
def color_jitter(x_u8, params, layout='hwc', norm=None, out=None, table=None):
    """torchvision's ``ColorJitter`` for given parameters on uint8 frames (B, H, W, 3) / (B, 3, H, W) (``layout``), Pillow's bytes
    (hs_color_jitter_fwd; the arithmetic: ``utils.jitter``).  ``params``: one ``ColorJitterParams`` for the batch or a sequence of B.
    Returns uint8 in the input's layout, or with ``norm`` (a ``utils.inference.InputNorm``) the float32 (B, 3, H, W) image looked up
    in its table.  ``out``: a contiguous tensor of that shape and dtype to write into.  Equal to ``utils.jitter.color_jitter_cpu``.

    ``table``: the caller's own parameter records on the device -- int32 (B, ``utils.jitter.TABLE_WORDS``), contiguous, what
    ``utils.jitter.params_table(params, B).to(device)`` gives; ``params`` is then not read (pass None).  The kernels read the table when
    they run, so a captured graph replays with what the caller last copied into it.  Launches: a clear of B sums, the mean pass (only
    samples whose order holds contrast do work) and the apply pass; without ``table``, the apply pass alone when no sample has contrast,
    and one small host-to-device copy of the records in front.  Nothing is read back: with ``table`` the call is capturable."""
    from .utils import jitter
    b, h, w = _frames_bhw(x_u8, layout)
    if b == 0 or h == 0 or w == 0:
        raise ValueError('empty batch')
    if table is None:
        records = jitter.params_table(params, b)
        need_mean = bool((records[:, 5] >> jitter.OP_CODES['contrast'] & 1).any())
    else:
        _jitter_table(table, b, x_u8.device)
        need_mean = True                                       # what it will hold when the kernels run is the caller's business
    out = _frame_out(out, b, h, w, layout, norm, x_u8.device)
    norm_table = _norm_table(norm, layout, x_u8.device)
    if table is None:
        table = records.to(x_u8.device)
    sums = torch.empty(b, device=x_u8.device, dtype=torch.int64) if need_mean else None
    _hip.run.hs_color_jitter_fwd(_hip.dev_ptr(x_u8, 'x_u8', torch.uint8), _LAYOUT_CODES[layout], b, h, w,
                                 _hip.dev_ptr(table, 'table', torch.int32), None if sums is None else sums.data_ptr(), norm_table,
                                 _hip.dev_ptr(out, 'out', out.dtype), _hip.stream_ptr())
    return out


def _blur_table(table, b, device):
    from .utils import blur
    if (not isinstance(table, torch.Tensor) or table.dtype != torch.int32 or tuple(table.shape) != (b, blur.TABLE_WORDS)
            or table.device != device or not table.is_contiguous()):
        raise ValueError(f'table must be a contiguous int32 tensor of shape {(b, blur.TABLE_WORDS)} on {device}')
    return table


def blur_records(params, b):
    """``utils.blur.params_table(params, b)`` after refusing, on the host, a radius whose box radius the device kernels do not take."""
    from .utils import blur
    records = blur.params_table(params, b)
    beyond = (records[:, 0] != 0) & (records[:, 1] > blur.MAX_RADIUS)
    if bool(beyond.any()):
        i = int(beyond.nonzero()[0])
        raise ValueError(f'sample {i}: radius {blur.per_sample(params, b)[i].radius} has the box radius {int(records[i, 1])}, the device '
                         f'kernels take up to {blur.MAX_RADIUS} (HS_BLUR_MAX_RADIUS)')
    return records


@_on_operand_device
def gaussian_blur(x_u8, params, layout='hwc', norm=None, out=None, table=None, status=None):
    """Pillow's ``ImageFilter.GaussianBlur`` for given parameters on uint8 frames (B, H, W, 3) / (B, 3, H, W) (``layout``), Pillow's bytes
    (hs_gaussian_blur_fwd; the arithmetic: ``utils.blur``).  ``params``: one ``GaussianBlurParams`` for the batch or a sequence of B (a
    ``None`` among them: that sample is not blurred).  Returns uint8 in the input's layout, or with ``norm`` (a
    ``utils.inference.InputNorm``) the float32 (B, 3, H, W) image looked up in its table -- a sample that is not blurred too.  ``out``: a
    contiguous tensor of that shape and dtype to write into.  Equal to ``utils.blur.gaussian_blur_cpu``.  A radius whose box radius
    exceeds ``utils.blur.MAX_RADIUS`` (a sigma of about 16) raises ValueError before anything is launched or copied.

    ``table``: the caller's own parameter records on the device -- int32 (B, ``utils.blur.TABLE_WORDS``), contiguous, what
    ``utils.blur.params_table(params, B).to(device)`` gives; ``params`` is then not read (pass None).  The kernels read the table when
    they run, so a captured graph replays with what the caller last copied into it; a record whose box radius the kernels do not take
    leaves its sample unblurred and sets its word of ``status`` -- int32 (B,) on the device, written by every call (default a new one,
    never read here).  Two launches (rows, columns) and a uint8 intermediate of the frames' size; without ``table`` one small
    host-to-device copy of the records in front.  Nothing is read back: with ``table`` the call is capturable."""
    b, h, w = _frames_bhw(x_u8, layout)
    if b == 0 or h == 0 or w == 0:
        raise ValueError('empty batch')
    device = x_u8.device
    if table is None:
        records = blur_records(params, b)
    else:
        _blur_table(table, b, device)
    if status is not None and (not isinstance(status, torch.Tensor) or status.dtype != torch.int32 or tuple(status.shape) != (b,)
                               or status.device != device or not status.is_contiguous()):
        raise ValueError(f'status must be a contiguous int32 tensor of shape {(b,)} on {device}')
    out = _frame_out(out, b, h, w, layout, norm, device)
    norm_table = _norm_table(norm, layout, device)
    if table is None:
        table = records.to(device)
    if status is None:
        status = torch.empty(b, device=device, dtype=torch.int32)
    tmp = torch.empty_like(x_u8, memory_format=torch.contiguous_format)
    _hip.run.hs_gaussian_blur_fwd(_hip.dev_ptr(x_u8, 'x_u8', torch.uint8), _LAYOUT_CODES[layout], b, h, w,
                                  _hip.dev_ptr(table, 'table', torch.int32), tmp.data_ptr(), norm_table,
                                  _hip.dev_ptr(out, 'out', out.dtype), status.data_ptr(), _hip.stream_ptr())
    return out


@_on_operand_device
def frame_rotate(x_u8, angle, layout='hwc', size=None, fill=(0, 0, 0), pad_fill=(0, 0, 0), norm=None, out=None, table=None):
    """uint8 frames (B, H, W, 3) / (B, 3, H, W) (``layout``), all of one size, rotated by ``angle`` degrees counter-clockwise about the
    centre with ``PIL.Image.rotate(angle, BICUBIC)``'s float64 arithmetic, byte for byte, in one launch (hs_frame_rotate_fwd; the
    arithmetic: ``utils.rotate``) -- the reference's ``RandomRotation`` and, through ``size``, the ``ConstantPad`` after it.  ``angle``: one
    value or B values.  ``size``: the padded (Ho, Wo) >= (H, W), the rotated image at its top-left corner -- default the input's own size.
    ``fill``: 3 bytes where the rotation looks outside the frame; ``pad_fill``: 3 bytes for the padding.  The defaults are the reference's
    VOC config: ``RandomRotation(30.)`` fills with 0 and ``ConstantPad(512, lbl_fill=255)`` pads the frame with 0.  Returns uint8 in the
    input's layout, or with ``norm`` (a ``utils.inference.InputNorm``) the float32 (B, 3, Ho, Wo) image looked up in its table, both
    fills included.  ``out``: a contiguous tensor of that shape and dtype to write into.  Equal to ``utils.rotate.frame_rotate_cpu``.

    ``table``: the caller's own matrices on the device -- float64 (B, 6), contiguous, what ``utils.rotate.matrix_table(H, W, angle,
    B).to(device)`` gives; ``angle`` is then not read (pass None).  The kernel reads the table when it runs, so a captured graph replays
    with what the caller last copied into it; without ``table`` there is one small host-to-device copy in front.  Nothing is read back."""
    from .utils import rotate
    h, w = rotate._check_frames(x_u8, layout)
    if not x_u8.is_cuda:                                       # CPU tensors: the same values from the CPU implementation
        res = rotate.frame_rotate_cpu(x_u8, angle, layout, size, fill, pad_fill, norm, table)
        return res if out is None else _out(out, res.shape, res.dtype, res.device).copy_(res)
    b = x_u8.shape[0]
    ho, wo = rotate.check_size(size, h, w)
    fill, pad_fill = _fill_word(fill), _fill_word(pad_fill, 'pad_fill')
    table = rotate.matrix_table(h, w, angle, b) if table is None else rotate.check_table(table, b, torch.float64, x_u8.device)
    out = _frame_out(out, b, ho, wo, layout, norm, x_u8.device)
    norm_table = _norm_table(norm, layout, x_u8.device)
    table = table.to(x_u8.device)                              # the host-built one goes up here; the caller's is there already
    _hip.run.hs_frame_rotate_fwd(_hip.dev_ptr(x_u8, 'x_u8', torch.uint8), _LAYOUT_CODES[layout], b, h, w,
                                 _hip.dev_ptr(table, 'table', torch.float64), ho, wo, fill, pad_fill, norm_table,
                                 _hip.dev_ptr(out, 'out', out.dtype), _hip.stream_ptr())
    return out


@_on_operand_device
def label_rotate(t, angle, size=None, fill=0, pad_fill=255, out=None, table=None):
    """Labels (B, H, W), uint8 or int64, rotated by ``angle`` with ``PIL.Image.rotate(angle, NEAREST)``'s 16.16 fixed-point arithmetic
    (hs_label_rotate_fwd, one launch; ``utils.rotate``), ``fill`` where the rotation looks outside, padded right and bottom to ``size``
    with ``pad_fill``.  The defaults are the reference's VOC config: its ``RandomRotation`` rotates the label with ``self.fill`` (0),
    NOT its ``lbl_fill`` (seg_transforms.py:424), and ``ConstantPad(512, lbl_fill=255)`` pads it with 255.  Returns the input's dtype, or
    ``out``'s (uint8 | int64, contiguous, (B, Ho, Wo)).  ``table``: the caller's int32 (B, 6) device tensor of
    ``utils.rotate.fixed_table`` rows, read when the kernel runs (``angle`` is then not read).  Equal to
    ``utils.rotate.label_rotate_cpu``."""
    from .utils import rotate
    h, w = rotate._check_labels(t)
    if not t.is_cuda:
        res = rotate.label_rotate_cpu(t, angle, size, fill, pad_fill, None if out is None else getattr(out, 'dtype', None), table)
        return res if out is None else _out(out, res.shape, res.dtype, res.device).copy_(res)
    b = t.shape[0]
    ho, wo = rotate.check_size(size, h, w)
    out = _label_out(out, (b, ho, wo), t.dtype, t.device)
    fill, pad_fill = _label_fill(fill, out), _label_fill(pad_fill, out, 'pad_fill')
    table = rotate.fixed_table(h, w, angle, b) if table is None else rotate.check_table(table, b, torch.int32, t.device)
    table = table.to(t.device)                                 # the host-built one goes up here; the caller's is there already
    _hip.run.hs_label_rotate_fwd(_hip.dev_ptr(t, 'labels', t.dtype), _LABEL_DTYPES[t.dtype], b, h, w,
                                 _hip.dev_ptr(table, 'table', torch.int32), ho, wo, fill, pad_fill,
                                 _hip.dev_ptr(out, 'out', out.dtype), _LABEL_DTYPES[out.dtype], _hip.stream_ptr())
    return out


# ------------------------------------------------------------------------------------------
# the VOC train chain for a ragged batch (csrc/hs_augment_ragged.hip): a canvas plus per-sample extents
# ------------------------------------------------------------------------------------------
RAGGED_PARAM_WORDS = 8                                     # h, w, Hr, Wr, hflip, 3 reserved: HS_RAGGED_PARAM_WORDS
RAGGED_STATUS = dict(RESIZE_STATUS, extent=32, canvas=64)  # HS_RESIZE_STATUS_*: what a ragged sample's status word sums
RAGGED_MAX_DIM = 8192                                      # every canvas and output dimension (the rotation's limit)


class RaggedTables(collections.namedtuple('RaggedTables', 'bounds kk nearest status workspace canvas_hw mid_hw ks_max')):
    """The device-built resize tables of a ragged batch (:func:`resize_tables_ragged`): int32 views of one ``workspace`` -- ``bounds``
    (B, 2, M, 2), ``kk`` (B, 2, M, ks_max), ``nearest`` (B, 2, M), ``status`` (B,), M = max(mid_hw), axis 0 = y -- and the geometry they
    were laid out for: ``canvas_hw`` the frames' canvas, ``mid_hw`` the intermediate canvas the resized images go to."""
    __slots__ = ()
    words = staticmethod(ResizeTables.words)

    @classmethod
    def over(cls, workspace, batch, canvas_hw, mid_hw, ks_max):
        t = ResizeTables.over(workspace, batch, canvas_hw, mid_hw, ks_max)
        return cls(t.bounds, t.kk, t.nearest, t.status, workspace, tuple(canvas_hw), tuple(mid_hw), ks_max)


def _ragged_params(params, device=None):
    return _param_rows(params, RAGGED_PARAM_WORDS, 'h, w, Hr, Wr, hflip, 3 reserved', device)


def _ragged_hw(hw, name):
    h, w = (int(s) for s in hw)
    if not (1 <= h <= RAGGED_MAX_DIM and 1 <= w <= RAGGED_MAX_DIM):
        raise ValueError(f'{name} must be two sizes in 1..{RAGGED_MAX_DIM}, got {(h, w)}')
    return h, w


def _ragged_tables(tables, params, n, device, canvas_hw=None, mid_hw=None):
    """B of ``params`` after checking that ``tables`` were built for them and for the ``n`` samples of the canvas at hand."""
    _ragged_hw(canvas_hw or mid_hw, 'canvas')
    b = _ragged_params(params, device)
    if not isinstance(tables, RaggedTables):
        raise ValueError('tables must be what resize_tables_ragged returned')
    if tables.workspace.device != device:
        raise ValueError(f'tables must be on {device}')
    if tables.status.shape[0] != b or (canvas_hw is not None and tables.canvas_hw != tuple(canvas_hw)) or \
            (mid_hw is not None and tables.mid_hw != tuple(mid_hw)):
        raise ValueError(f'the tables were built for {tables.status.shape[0]} samples, canvas {tables.canvas_hw} -> {tables.mid_hw}; these are '
                         f'{b} samples of {canvas_hw or mid_hw}')
    if n != b:
        raise ValueError(f'{n} samples, {b} parameter rows')
    return b


@_on_operand_device
def resize_tables_ragged(params, canvas_hw, mid_hw, filter, ks_max, workspace=None):
    """:func:`resize_tables` for a batch whose samples differ in INPUT size, one launch (hs_resize_tables_ragged_fwd).  ``params``: int32
    (B, 8) on the device = ``h, w, Hr, Wr, hflip, 3 reserved`` per sample -- the extent of the image in the ``canvas_hw`` = (Hm, Wm)
    canvas, its resized size, the flip of the source; ``mid_hw`` = (Hc, Wc) the intermediate canvas the resized images go to.  The
    window is the whole resized image.  Returns a :class:`RaggedTables` over ``workspace`` (int32, contiguous, at least
    ``RaggedTables.words(B, mid_hw, ks_max)`` elements; default a new one): per sample and axis ``utils.resample.window_tables_cpu(in, out,
    0, M, filter, ks_max)``, integer for integer.  ``status``: 0 per sample, or a sum of ``RAGGED_STATUS`` codes -- an extent outside
    the canvas, a resized size below 1 or above ``mid_hw``, more taps than ``ks_max`` (an axis of ``in`` pixels has at most
    ``min(ksize, in)``); that sample's tables are empty and it comes out as pad fill.  Nothing is read back: capturable."""
    b = _ragged_params(params)
    code = _filter_code(filter)
    hm, wm = _ragged_hw(canvas_hw, 'canvas_hw')
    hc, wc = _ragged_hw(mid_hw, 'mid_hw')
    ks_max = int(ks_max)
    if ks_max < 1:
        raise ValueError(f'ks_max must be >= 1, got {ks_max}')
    t = _tables_over(RaggedTables, workspace, b, (hm, wm), (hc, wc), ks_max, params.device)
    _hip.run.hs_resize_tables_ragged_fwd(_hip.dev_ptr(params, 'params', torch.int32), b, hm, wm, hc, wc, code, ks_max,
                                         t.bounds.data_ptr(), t.kk.data_ptr(), t.nearest.data_ptr(), t.status.data_ptr(),
                                         _hip.stream_ptr())
    return t


@_on_operand_device
def color_jitter_ragged(x_u8, params, table, layout='hwc', contrast=True, out=None, sums=None):
    """:func:`color_jitter` over the top-left ``(h, w)`` region of every sample of a uint8 canvas (B, Hm, Wm, 3) / (B, 3, Hm, Wm)
    (hs_color_jitter_ragged_fwd): ``params`` the ragged int32 (B, 8) rows, ``table`` the int32 (B, ``utils.jitter.TABLE_WORDS``) records,
    both on the device and read when the kernels run.  The contrast mean is taken over the region only; nothing outside it is read or
    written.  Returns a uint8 canvas of the same shape (``out``).  ``contrast=True``: a clear of B sums, the mean pass and the apply pass;
    ``False`` -- the caller's promise that no record names contrast -- the apply pass alone.  ``sums``: an int64 (B,) device tensor to use
    as the mean's workspace (default a new one).  Per sample the region holds ``utils.jitter.color_jitter_cpu`` of the cropped frame.
    Capturable."""
    n, hm, wm = _frames_bhw(x_u8, layout, 'canvas')
    _ragged_hw((hm, wm), 'canvas')
    b = _ragged_params(params, x_u8.device)
    if n != b:
        raise ValueError(f'{n} frames, {b} parameter rows')
    _jitter_table(table, b, x_u8.device)
    out = _out(out, x_u8.shape, torch.uint8, x_u8.device)
    if contrast:
        sums = _out(sums, (b,), torch.int64, x_u8.device)
    _hip.run.hs_color_jitter_ragged_fwd(_hip.dev_ptr(x_u8, 'canvas', torch.uint8), _LAYOUT_CODES[layout], b, hm, wm,
                                        _hip.dev_ptr(params, 'params', torch.int32), _hip.dev_ptr(table, 'table', torch.int32),
                                        _hip.dev_ptr(sums, 'sums', torch.int64) if contrast else None,
                                        _hip.dev_ptr(out, 'out', torch.uint8), _hip.stream_ptr())
    return out


@_on_operand_device
def frame_resize_ragged(x_u8, params, tables, layout='hwc', out=None):
    """:func:`frame_resize_batch` for a ragged batch, one launch (hs_frame_resize_ragged_fwd): the ``(h, w)`` region of sample b of the
    uint8 canvas (B, Hm, Wm, 3) / (B, 3, Hm, Wm), mirrored left-right FIRST where ``params[b]`` says hflip, resized to its (Hr, Wr) with
    the filter ``tables`` (a :class:`RaggedTables` built from the same ``params``) were made for.  Returns the uint8 intermediate canvas
    (B, Hc, Wc, 3) / (B, 3, Hc, Wc) (``out``), the resized image at its top left: the bytes of ``frame_resize(region.flip(), (Hr, Wr))``;
    the pixels outside it are not specified.  Capturable."""
    n, hm, wm = _frames_bhw(x_u8, layout, 'canvas')
    b = _ragged_tables(tables, params, n, x_u8.device, canvas_hw=(hm, wm))
    hc, wc = tables.mid_hw
    out = _frame_out(out, b, hc, wc, layout, None, x_u8.device)
    _hip.run.hs_frame_resize_ragged_fwd(_hip.dev_ptr(x_u8, 'canvas', torch.uint8), _LAYOUT_CODES[layout], b, hm, wm,
                                        _hip.dev_ptr(params, 'params', torch.int32), tables.bounds.data_ptr(), tables.kk.data_ptr(),
                                        tables.status.data_ptr(), tables.ks_max, hc, wc, _hip.dev_ptr(out, 'out', torch.uint8),
                                        _hip.stream_ptr())
    return out


@_on_operand_device
def label_resize_ragged(t, params, tables, out=None):
    """:func:`label_resize_batch` for a ragged batch, one launch (hs_label_resize_ragged_fwd): labels (B, Hm, Wm), uint8 or int64 with
    values in 0..255, the region mirrored first where hflip says, through ``tables``' nearest indices.  Returns the uint8 intermediate
    canvas (B, Hc, Wc) (``out``), the resized label at its top left.  Capturable."""
    n, hm, wm = _labels_bhw(t)
    b = _ragged_tables(tables, params, n, t.device, canvas_hw=(hm, wm))
    hc, wc = tables.mid_hw
    out = _out(out, (b, hc, wc), torch.uint8, t.device)
    _hip.run.hs_label_resize_ragged_fwd(_hip.dev_ptr(t, 'labels', t.dtype), _LABEL_DTYPES[t.dtype], b, hm, wm,
                                        _hip.dev_ptr(params, 'params', torch.int32), tables.nearest.data_ptr(), tables.status.data_ptr(),
                                        hc, wc, _hip.dev_ptr(out, 'out', torch.uint8), _hip.stream_ptr())
    return out


@_on_operand_device
def frame_rotate_ragged(x_u8, params, tables, matrices, layout='hwc', size=None, fill=(0, 0, 0), pad_fill=(0, 0, 0), norm=None, out=None):
    """:func:`frame_rotate` for a ragged batch, one launch (hs_frame_rotate_ragged_fwd): sample b's (Hr, Wr) image at the top left of the
    uint8 intermediate canvas (B, Hc, Wc, 3) / (B, 3, Hc, Wc) rotated by ``matrices[b]`` (float64 (B, 6) on the device, the rows of
    ``utils.rotate.rotation_matrix(Hr, Wr, angle)``), at the top left of the ``size`` = (Ho, Wo) output (default the canvas's), ``fill``
    where the rotation looks outside the image, ``pad_fill`` right of and below it -- and everywhere for a sample whose ``tables.status``
    is not 0.  Returns uint8 in the input's layout, or with ``norm`` float32 (B, 3, Ho, Wo) through its table; ``out`` likewise.
    Capturable."""
    from .utils import rotate
    n, hc, wc = _frames_bhw(x_u8, layout, 'canvas')
    b = _ragged_tables(tables, params, n, x_u8.device, mid_hw=(hc, wc))
    ho, wo = (hc, wc) if size is None else _ragged_hw(size, 'size')
    fill, pad_fill = _fill_word(fill), _fill_word(pad_fill, 'pad_fill')
    rotate.check_table(matrices, b, torch.float64, x_u8.device)
    out = _frame_out(out, b, ho, wo, layout, norm, x_u8.device)
    table = _norm_table(norm, layout, x_u8.device)
    _hip.run.hs_frame_rotate_ragged_fwd(_hip.dev_ptr(x_u8, 'canvas', torch.uint8), _LAYOUT_CODES[layout], b, hc, wc,
                                        _hip.dev_ptr(params, 'params', torch.int32), tables.status.data_ptr(),
                                        _hip.dev_ptr(matrices, 'matrices', torch.float64), ho, wo, fill, pad_fill,
                                        table, _hip.dev_ptr(out, 'out', out.dtype), _hip.stream_ptr())
    return out


@_on_operand_device
def label_rotate_ragged(t, params, tables, fixed, size=None, fill=0, pad_fill=255, out=None):
    """:func:`label_rotate` for a ragged batch, one launch (hs_label_rotate_ragged_fwd): sample b's (Hr, Wr) label at the top left of the
    uint8 intermediate canvas (B, Hc, Wc) through ``fixed[b]`` (int32 (B, 6) on the device, ``utils.rotate.nearest_fixed`` rows), padded to
    ``size`` with ``pad_fill`` (everywhere for a sample whose status is not 0).  Returns int64 (B, Ho, Wo), or ``out``'s dtype (uint8 |
    int64).  Capturable."""
    from .utils import rotate
    n, hc, wc = _labels_bhw(t, (torch.uint8,), 'the intermediate labels')
    b = _ragged_tables(tables, params, n, t.device, mid_hw=(hc, wc))
    ho, wo = (hc, wc) if size is None else _ragged_hw(size, 'size')
    rotate.check_table(fixed, b, torch.int32, t.device)
    out = _label_out(out, (b, ho, wo), torch.int64, t.device)
    fill, pad_fill = _label_fill(fill, out), _label_fill(pad_fill, out, 'pad_fill')
    _hip.run.hs_label_rotate_ragged_fwd(_hip.dev_ptr(t, 'labels', torch.uint8), b, hc, wc, _hip.dev_ptr(params, 'params', torch.int32),
                                        tables.status.data_ptr(), _hip.dev_ptr(fixed, 'fixed', torch.int32), ho, wo, fill, pad_fill,
                                        _hip.dev_ptr(out, 'out', out.dtype), _LABEL_DTYPES[out.dtype], _hip.stream_ptr())
    return out


# ------------------------------------------------------------------------------------------
# small caches keyed on parameter versions (host-side only; used by the fused inference route --
# tensors that require grad take the hyperseg_amd.autograd route, which folds nothing)
# ------------------------------------------------------------------------------------------
_WEIGHTS_EPOCH = [0]


def bump_weights_epoch():
    """Invalidates every host-side cache derived from parameters or BatchNorm statistics (folded BN affines, transposed /
    packed signal2weights weights, the prepared encoder's folded and split weights).  The caches are keyed on
    (address, tensor._version, shape) -- but a HIP-graph replay of a training step, this package's raw-pointer BatchNorm
    kernels and stock BatchNorm's running-statistics update all change values WITHOUT bumping ``_version``.
    Called by ``training.GraphedTrainStep.step``, by ``autograd.bn_act`` and by every train() / eval() switch of the
    package's modules, so a validation pass after any number of training steps re-derives everything once."""
    with _CACHE_LOCK:
        _WEIGHTS_EPOCH[0] += 1


def _key(*tensors):
    return (_WEIGHTS_EPOCH[0],) + tuple((t.data_ptr(), t._version, tuple(t.shape)) for t in tensors)


class FoldedBN:
    """Per-module cache of the folded (scale, shift) of an eval-mode nn.BatchNorm2d."""

    def __init__(self):
        self._ent = {}          # device -> (key, value): one immutable pair per device, replaced in ONE assignment (see _CACHE_LOCK)

    def get(self, bn):
        if bn.training or not bn.track_running_stats:
            raise NotImplementedError('hyperseg_amd: a train-mode BatchNorm cannot be folded into a kernel epilogue; '
                                      'the training route (hyperseg_amd.autograd) keeps BatchNorm as a module')
        ts = (bn.weight, bn.bias, bn.running_mean, bn.running_var)
        k = _key(*ts)
        dev = bn.weight.device
        ent = self._ent.get(dev)
        if ent is None or ent[0] != k:
            with torch.no_grad():
                ent = (k, bn_fold(bn.weight.detach(), bn.bias.detach(), bn.running_mean, bn.running_var, bn.eps), producer_stream(dev))
            publish_ready(dev)
            self._ent[dev] = ent
            return ent[1]
        return adopt(ent[1], dev, ent[2])


class TransposedS2W:
    """Per-module cache of the signal2weights Conv2d weight transposed to (Cs/G, Wc)."""

    def __init__(self):
        self._ent = {}          # device -> (key, value), as FoldedBN

    def get(self, conv):
        w = conv.weight
        k = _key(w)
        ent = self._ent.get(w.device)
        if ent is None or ent[0] != k:
            with torch.no_grad():
                ent = (k, w.detach().reshape(w.shape[0], w.shape[1]).t().contiguous(), producer_stream(w.device))
            publish_ready(w.device)
            self._ent[w.device] = ent
            return ent[1]
        return adopt(ent[1], w.device, ent[2])
