"""A dataset's label encoding as data: the per-pixel step the reference's loaders run on the host before their transforms see a label,
restated once on the CPU (:meth:`LabelCodec.encode_cpu`, the checker of everything else) and handed to the device kernels as one small
int32 tensor (:meth:`LabelCodec.device_words`; csrc/hs_label_codec.hip, csrc/hs_label_codec.h).  Two rules:

  * ``LabelCodec.table(values)`` -- Cityscapes, hyperseg/datasets/cityscapes.py:107, 209-211: the label file holds raw ids;
    ``__getitem__`` sets every id outside ``[0, len(id_to_train_id))`` to 0 and then looks every pixel up in ``id_to_train_id``.  So a
    raw label ``v`` becomes ``values[v]``, or ``values[0]`` where ``v`` lies outside ``[0, len(values))``.  Labels (B, H, W), uint8 or int64.
  * ``LabelCodec.colors(colors, unmatched=255)`` -- CamVid, hyperseg/datasets/camvid.py:93-100: the label file is an RGB image;
    ``convert_label`` starts from an image full of 255 and writes index ``i`` wherever the pixel equals ``class_color[i]``, entry after
    entry, so a later entry overwrites an earlier one.  A pixel becomes the index of the LAST entry equal to it, or ``unmatched``.
    Labels uint8 (B, H, W, 3).

Every result is a byte value.  A codec is a plain object -- no module, no parameter, no buffer -- that compares and hashes by its
contents: it is part of the keys of captured graphs."""
import threading

import torch

TABLE, COLORS = 1, 2                       # HS_CODEC_TABLE / HS_CODEC_COLORS of include/hyperseg_hip.h
TABLE_WORDS = 64                           # the 256 table bytes, four to a word
MAX_COLORS = 255

_DEVICE_WORDS = {}
_LOCK = threading.Lock()


def _bytes(seq, what):
    out = []
    for v in seq:
        if isinstance(v, bool) or int(v) != v or not 0 <= int(v) <= 255:
            raise ValueError(f'{what} must be integers in 0..255, got {v!r}')
        out.append(int(v))
    return tuple(out)


class LabelCodec:
    """Module docstring.  Make one with :meth:`table` or :meth:`colors`."""

    __slots__ = ('kind', 'values', 'unmatched')

    def __init__(self, kind, values, unmatched):
        if kind not in (TABLE, COLORS):
            raise ValueError('make a LabelCodec with LabelCodec.table(values) or LabelCodec.colors(colors)')
        object.__setattr__(self, 'kind', kind)
        object.__setattr__(self, 'values', values)
        object.__setattr__(self, 'unmatched', unmatched)

    def __setattr__(self, name, value):
        raise AttributeError('a LabelCodec does not change: it is part of graph keys')

    @classmethod
    def table(cls, values):
        """The id table: ``values`` is 1..256 integers in 0..255 (Cityscapes' ``id_to_train_id``)."""
        values = values.tolist() if hasattr(values, 'tolist') else list(values)
        if not 1 <= len(values) <= 256:
            raise ValueError(f'a table holds 1..256 values, got {len(values)}')
        return cls(TABLE, _bytes(values, 'table values'), None)

    @classmethod
    def colors(cls, colors, unmatched=255):
        """The colour list: ``colors`` is 1..255 RGB triples of bytes (CamVid's ``class_color``); ``unmatched`` (0..255) is what a pixel
        equal to none of them becomes.  Duplicates are allowed: the later entry wins."""
        colors = colors.tolist() if hasattr(colors, 'tolist') else list(colors)
        if not 1 <= len(colors) <= MAX_COLORS:
            raise ValueError(f'a colour list holds 1..{MAX_COLORS} entries, got {len(colors)}')
        rows = []
        for c in colors:
            c = c.tolist() if hasattr(c, 'tolist') else c
            if not isinstance(c, (list, tuple)) or len(c) != 3:
                raise ValueError(f'a colour is an (r, g, b) triple, got {c!r}')
            rows.append(_bytes(c, 'colour components'))
        return cls(COLORS, tuple(rows), _bytes([unmatched], 'unmatched')[0])

    # ------------------------------------------------------------------------------------------------------------ identity
    def _contents(self):
        return (self.kind, self.values, self.unmatched)

    def __eq__(self, other):
        return isinstance(other, LabelCodec) and self._contents() == other._contents()

    def __ne__(self, other):
        return not self == other

    def __hash__(self):
        return hash(self._contents())

    def __repr__(self):
        if self.kind == TABLE:
            return f'LabelCodec.table({list(self.values)})'
        return f'LabelCodec.colors({[list(c) for c in self.values]}, unmatched={self.unmatched})'

    def __len__(self):
        return len(self.values)

    # ------------------------------------------------------------------------------------------------------------ operands
    @property
    def is_colors(self):
        return self.kind == COLORS

    def is_raw(self, t):
        """``t`` has this codec's input kind: uint8 (B, H, W, 3) for colours; for a table every 3-D integer tensor (with a codec set,
        labels are raw by contract)."""
        if not isinstance(t, torch.Tensor):
            return False
        if self.kind == COLORS:
            return t.dtype == torch.uint8 and t.dim() == 4 and t.shape[3] == 3
        return t.dim() == 3 and not t.is_floating_point() and not t.is_complex() and t.dtype != torch.bool

    def check_raw(self, t, name='labels'):
        """(B, H, W) of raw labels the kernels and :meth:`encode_cpu` take: uint8 (B, H, W, 3), or uint8 / int64 (B, H, W)."""
        if self.kind == COLORS:
            ok, want = self.is_raw(t), 'uint8 (B, H, W, 3) colour labels'
        else:
            ok, want = self.is_raw(t) and t.dtype in (torch.uint8, torch.int64), 'uint8 or int64 (B, H, W) raw ids'
        if not ok:
            raise ValueError(f'{name} must be {want}, got {getattr(t, "dtype", type(t))} {tuple(getattr(t, "shape", ()))}')
        return tuple(t.shape[:3])

    def raw_shape(self, b, h, w):
        """The shape of (B, H, W) raw labels."""
        return (b, h, w, 3) if self.kind == COLORS else (b, h, w)

    def out_dtype(self, t):
        """The default dtype of the encoded labels: uint8 for a colour image, else the input's."""
        return torch.uint8 if self.kind == COLORS else t.dtype

    def encoded_like(self, t):
        """A meta tensor with the shape and dtype ``t`` has once it is encoded (for checks that only look at those)."""
        return torch.empty(tuple(t.shape[:3]), dtype=self.out_dtype(t), device='meta')

    @property
    def launch_operands(self):
        """``(codec_kind, n, unmatched)`` as the library's entries take them."""
        return self.kind, len(self.values), 0 if self.unmatched is None else self.unmatched

    # ------------------------------------------------------------------------------------------------------------ the rules
    def encode_cpu(self, t, out_dtype=None):
        """The reference's lines on a CPU tensor, in torch: raw labels -> ``out_dtype`` (uint8 | int64; default :meth:`out_dtype`)."""
        self.check_raw(t)
        if t.device.type != 'cpu':
            raise ValueError(f'encode_cpu takes CPU tensors, got one on {t.device} (functional.label_encode is the device route)')
        out_dtype = out_dtype or self.out_dtype(t)
        if out_dtype not in (torch.uint8, torch.int64):
            raise ValueError(f'out_dtype must be uint8 or int64, got {out_dtype}')
        if self.kind == TABLE:
            lut = torch.tensor(self.values, dtype=torch.int64)
            v = t.to(torch.int64).clone()
            v[(v < 0) | (v >= len(self.values))] = 0               # cityscapes.py:210
            return lut[v].to(out_dtype)                            # cityscapes.py:211
        out = torch.full(tuple(t.shape[:3]), self.unmatched, dtype=torch.int64)
        for i, color in enumerate(self.values):                    # camvid.py:96-98: entry after entry, a later one overwrites
            out[(t == torch.tensor(color, dtype=torch.uint8)).all(dim=3)] = i
        return out.to(out_dtype)

    def words(self):
        """The codec as the kernels read it, a CPU int32 tensor: the 256 table bytes four to a word, little-endian, entries from
        ``len(values)`` on holding ``values[0]`` (64 words); or the count followed by the colours ``r | g << 8 | b << 16`` (1 + n words)."""
        if self.kind == TABLE:
            padded = list(self.values) + [self.values[0]] * (256 - len(self.values))
            words = [padded[i] | padded[i + 1] << 8 | padded[i + 2] << 16 | padded[i + 3] << 24 for i in range(0, 256, 4)]
            return torch.tensor([w - (1 << 32) if w >= 1 << 31 else w for w in words], dtype=torch.int32)
        return torch.tensor([len(self.values)] + [r | g << 8 | b << 16 for r, g, b in self.values], dtype=torch.int32)

    def device_words(self, device):
        """:meth:`words` on ``device``, uploaded once per (codec, device) -- as ``utils.resample.device_nearest`` keeps its tables."""
        device = torch.device(device)
        if device.type == 'cuda' and device.index is None:
            device = torch.device('cuda', torch.cuda.current_device())
        with _LOCK:
            hit = _DEVICE_WORDS.get((self, device))
            if hit is None:
                hit = self.words().to(device).contiguous()
                if device.type == 'cuda' and not torch.cuda.is_current_stream_capturing():
                    torch.cuda.current_stream(device).synchronize()      # other streams (a capture's side stream) may read it next
                _DEVICE_WORDS[(self, device)] = hit
        return hit

