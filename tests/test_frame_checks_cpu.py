"""What the frame wrappers of ``functional`` and the four augmentation entry points of ``training`` REFUSE, and which forms of a per-sample
argument they take as the same thing -- pinned on CPU tensors, where every ``ValueError`` is raised before the library is reached.  A
wrapper handed good operands on the CPU gets as far as the library boundary and fails there with ``HipLibraryError`` (a RuntimeError: there
is no CPU fallback), so each refusal below is the one thing wrong with its call.  Tiny tensors: frames 5 x 7, batch 2."""
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO

B, H, W = 2, 5, 7
KS = 5
MOVED = ('device_augment', 'BatchAugment', 'device_augment_voc', 'VOCBatchParams', 'BatchAugmentVOC', '_voc_cpu', 'draw_color_jitter')


def hf():
    from hyperseg_amd import functional
    return functional


def norm(layout='hwc'):
    from hyperseg_amd import InputNorm
    return InputNorm(layout=layout)


def frames(layout='hwc'):
    x = (torch.arange(B * H * W * 3) % 251).to(torch.uint8).view(B, H, W, 3)
    return x if layout == 'hwc' else x.permute(0, 3, 1, 2).contiguous()


def labels(dtype=torch.uint8):
    return (torch.arange(B * H * W) % 19).view(B, H, W).to(dtype)


def meta(shape, dtype):
    return torch.empty(shape, dtype=dtype, device='meta')


def params(words=6):
    rows = [[H, W, 0, 0, 0, 0], [3, 4, -1, 1, 1, 0]] if words == 6 else [[H, W, H, W, 0, 0, 0, 0], [3, 4, 3, 4, 1, 0, 0, 0]]
    return torch.tensor(rows, dtype=torch.int32)


def strided(words):
    """(B, words) int32, not contiguous."""
    return torch.zeros(B, 2 * words, dtype=torch.int32)[:, ::2]


def tables():
    HF = hf()
    return HF.ResizeTables.over(torch.zeros(HF.ResizeTables.words(B, (H, W), KS), dtype=torch.int32), B, (H, W), (H, W), KS)


def ragged():
    HF = hf()
    return HF.RaggedTables.over(torch.zeros(HF.RaggedTables.words(B, (H, W), KS), dtype=torch.int32), B, (H, W), (H, W), KS)


def view(fill=(0, 0, 0)):
    from hyperseg_amd.utils.resample import ResizeView
    return ResizeView((H, W), (0, 0), False, fill)


def records():
    return torch.zeros(B, 8, dtype=torch.int32)


def table64():
    return torch.zeros(B, 6, dtype=torch.float64)


def fixed():
    return torch.zeros(B, 6, dtype=torch.int32)


def short(cls):
    return torch.zeros(cls.words(B, (H, W), KS) - 1, dtype=torch.int32)


U8, F32, I64 = torch.uint8, torch.float32, torch.int64

# every wrapper with good operands: where it ends on CPU tensors ('library' = HipLibraryError at the boundary, 'cpu' = the CPU route's result)
GOOD = {
    'frame_resize': ('library', lambda HF: HF.frame_resize(frames(), (4, 6), 'bicubic', norm=norm(), out=torch.empty(B, 3, 4, 6))),
    'label_resize': ('library', lambda HF: HF.label_resize(labels(), (4, 6), fill=300, out=torch.empty(B, 4, 6, dtype=I64))),
    'resize_tables': ('library', lambda HF: HF.resize_tables(params(), (H, W), (H, W), 'bicubic', KS, workspace=tables().workspace)),
    'frame_resize_batch': ('library', lambda HF: HF.frame_resize_batch(frames(), params(), tables(), fill=(1, 2, 255), norm=norm())),
    'label_resize_batch': ('library', lambda HF: HF.label_resize_batch(labels(I64), params(), tables(), fill=300)),
    'color_jitter': ('library', lambda HF: HF.color_jitter(frames(), None, norm=norm(), table=records())),
    'frame_rotate': ('cpu', lambda HF: HF.frame_rotate(frames(), 10.0, size=(6, 8), norm=norm(), out=torch.empty(B, 3, 6, 8))),
    'label_rotate': ('cpu', lambda HF: HF.label_rotate(labels(), [10.0, -10.0], size=(6, 8), out=torch.empty(B, 6, 8, dtype=I64))),
    'resize_tables_ragged': ('library', lambda HF: HF.resize_tables_ragged(params(8), (H, W), (H, W), 'bicubic', KS, workspace=ragged().workspace)),
    'color_jitter_ragged': ('library', lambda HF: HF.color_jitter_ragged(frames(), params(8), records(), sums=torch.zeros(B, dtype=I64))),
    'frame_resize_ragged': ('library', lambda HF: HF.frame_resize_ragged(frames('chw'), params(8), ragged(), 'chw')),
    'label_resize_ragged': ('library', lambda HF: HF.label_resize_ragged(labels(I64), params(8), ragged())),
    'frame_rotate_ragged': ('library', lambda HF: HF.frame_rotate_ragged(frames(), params(8), ragged(), table64(), fill=(1, 2, 255), norm=norm())),
    'label_rotate_ragged': ('library', lambda HF: HF.label_rotate_ragged(labels(), params(8), ragged(), fixed(), fill=300)),
}

REFUSED = {
    # frames: dtype, rank, channel position for the layout
    'frame_resize-dtype': lambda HF: HF.frame_resize(frames().float(), (4, 6)),
    'frame_resize-rank': lambda HF: HF.frame_resize(frames()[0], (4, 6)),
    'frame_resize-channels': lambda HF: HF.frame_resize(frames('chw'), (4, 6), layout='hwc'),
    'frame_resize-layout': lambda HF: HF.frame_resize(frames(), (4, 6), layout='nhwc'),
    'frame_resize-norm': lambda HF: HF.frame_resize(frames(), (4, 6), norm=norm('chw')),
    'frame_resize-fill4': lambda HF: HF.frame_resize(frames(), (H, W), view=view((1, 2, 3, 4))),
    'frame_resize-fill256': lambda HF: HF.frame_resize(frames(), (H, W), view=view((0, 0, 256))),
    'frame_resize-out_shape': lambda HF: HF.frame_resize(frames(), (4, 6), out=torch.empty(B, 4, 7, 3, dtype=U8)),
    'frame_resize-out_dtype': lambda HF: HF.frame_resize(frames(), (4, 6), norm=norm(), out=torch.empty(B, 3, 4, 6, dtype=U8)),
    'frame_resize-out_uint8_shape_with_norm': lambda HF: HF.frame_resize(frames(), (4, 6), norm=norm(), out=torch.empty(B, 4, 6, 3)),
    'frame_resize-out_device': lambda HF: HF.frame_resize(frames(), (4, 6), out=meta((B, 4, 6, 3), U8)),
    'frame_resize_batch-dtype': lambda HF: HF.frame_resize_batch(frames().float(), params(), tables()),
    'frame_resize_batch-rank': lambda HF: HF.frame_resize_batch(frames()[0], params(), tables()),
    'frame_resize_batch-channels': lambda HF: HF.frame_resize_batch(frames(), params(), tables(), 'chw'),
    'frame_resize_batch-norm': lambda HF: HF.frame_resize_batch(frames(), params(), tables(), norm=norm('chw')),
    'frame_resize_batch-fill4': lambda HF: HF.frame_resize_batch(frames(), params(), tables(), fill=(1, 2, 3, 4)),
    'frame_resize_batch-fill256': lambda HF: HF.frame_resize_batch(frames(), params(), tables(), fill=256),
    'frame_resize_batch-out_shape': lambda HF: HF.frame_resize_batch(frames(), params(), tables(), out=torch.empty(B, H, W + 1, 3, dtype=U8)),
    'frame_resize_batch-out_dtype': lambda HF: HF.frame_resize_batch(frames(), params(), tables(), out=torch.empty(B, H, W, 3)),
    'frame_resize_batch-out_device': lambda HF: HF.frame_resize_batch(frames(), params(), tables(), out=meta((B, H, W, 3), U8)),
    'frame_resize_batch-params_words': lambda HF: HF.frame_resize_batch(frames(), params()[:, :5].contiguous(), tables()),
    'frame_resize_batch-params_strided': lambda HF: HF.frame_resize_batch(frames(), strided(6), tables()),
    'frame_resize_batch-tables': lambda HF: HF.frame_resize_batch(frames(), params(), ragged()),
    'frame_resize_batch-rows': lambda HF: HF.frame_resize_batch(frames()[:1], params(), tables()),
    'color_jitter-dtype': lambda HF: HF.color_jitter(frames().float(), None, table=records()),
    'color_jitter-rank': lambda HF: HF.color_jitter(frames()[0], None, table=records()),
    'color_jitter-channels': lambda HF: HF.color_jitter(frames('chw'), None, table=records()),
    'color_jitter-norm': lambda HF: HF.color_jitter(frames(), None, norm=norm('chw'), table=records()),
    'color_jitter-table_shape': lambda HF: HF.color_jitter(frames(), None, table=records()[:, :6].contiguous()),
    'color_jitter-table_dtype': lambda HF: HF.color_jitter(frames(), None, table=records().long()),
    'color_jitter-table_strided': lambda HF: HF.color_jitter(frames(), None, table=strided(8)),
    'color_jitter-out_shape': lambda HF: HF.color_jitter(frames(), None, out=torch.empty(B, H, W, 4, dtype=U8), table=records()),
    'color_jitter-out_dtype': lambda HF: HF.color_jitter(frames(), None, norm=norm(), out=torch.empty(B, 3, H, W, dtype=U8), table=records()),
    'color_jitter-out_device': lambda HF: HF.color_jitter(frames(), None, out=meta((B, H, W, 3), U8), table=records()),
    'frame_rotate-dtype': lambda HF: HF.frame_rotate(frames().float(), 10.0),
    'frame_rotate-rank': lambda HF: HF.frame_rotate(frames()[0], 10.0),
    'frame_rotate-channels': lambda HF: HF.frame_rotate(frames('chw'), 10.0),
    'frame_rotate-norm': lambda HF: HF.frame_rotate(frames(), 10.0, norm=norm('chw')),
    'frame_rotate-fill4': lambda HF: HF.frame_rotate(frames(), 10.0, fill=(1, 2, 3, 4)),
    'frame_rotate-pad_fill256': lambda HF: HF.frame_rotate(frames(), 10.0, pad_fill=256),
    'frame_rotate-out_shape': lambda HF: HF.frame_rotate(frames(), 10.0, out=torch.empty(B, H, W + 1, 3, dtype=U8)),
    'frame_rotate-out_dtype': lambda HF: HF.frame_rotate(frames(), 10.0, norm=norm(), out=torch.empty(B, 3, H, W, dtype=U8)),
    'frame_rotate-out_device': lambda HF: HF.frame_rotate(frames(), 10.0, out=meta((B, H, W, 3), U8)),
    'frame_rotate-table': lambda HF: HF.frame_rotate(frames(), None, table=table64().float()),
    'frame_rotate-angles': lambda HF: HF.frame_rotate(frames(), [1.0] * (B + 1)),
    'color_jitter_ragged-dtype': lambda HF: HF.color_jitter_ragged(frames().float(), params(8), records()),
    'color_jitter_ragged-channels': lambda HF: HF.color_jitter_ragged(frames('chw'), params(8), records()),
    'color_jitter_ragged-params_words': lambda HF: HF.color_jitter_ragged(frames(), params(), records()),
    'color_jitter_ragged-params_strided': lambda HF: HF.color_jitter_ragged(frames(), strided(8), records()),
    'color_jitter_ragged-table_shape': lambda HF: HF.color_jitter_ragged(frames(), params(8), records()[:, :6].contiguous()),
    'color_jitter_ragged-out_shape': lambda HF: HF.color_jitter_ragged(frames(), params(8), records(), out=torch.empty(B, H, W + 1, 3, dtype=U8)),
    'color_jitter_ragged-out_device': lambda HF: HF.color_jitter_ragged(frames(), params(8), records(), out=meta((B, H, W, 3), U8)),
    'color_jitter_ragged-sums': lambda HF: HF.color_jitter_ragged(frames(), params(8), records(), sums=torch.zeros(B, dtype=torch.int32)),
    'frame_resize_ragged-dtype': lambda HF: HF.frame_resize_ragged(frames().float(), params(8), ragged()),
    'frame_resize_ragged-rank': lambda HF: HF.frame_resize_ragged(frames()[0], params(8), ragged()),
    'frame_resize_ragged-channels': lambda HF: HF.frame_resize_ragged(frames(), params(8), ragged(), 'chw'),
    'frame_resize_ragged-params_words': lambda HF: HF.frame_resize_ragged(frames(), params(), ragged()),
    'frame_resize_ragged-params_strided': lambda HF: HF.frame_resize_ragged(frames(), strided(8), ragged()),
    'frame_resize_ragged-tables': lambda HF: HF.frame_resize_ragged(frames(), params(8), tables()),
    'frame_resize_ragged-out_shape': lambda HF: HF.frame_resize_ragged(frames(), params(8), ragged(), out=torch.empty(B, 3, H, W, dtype=U8)),
    'frame_resize_ragged-out_dtype': lambda HF: HF.frame_resize_ragged(frames(), params(8), ragged(), out=torch.empty(B, H, W, 3)),
    'frame_resize_ragged-out_device': lambda HF: HF.frame_resize_ragged(frames(), params(8), ragged(), out=meta((B, H, W, 3), U8)),
    'frame_rotate_ragged-dtype': lambda HF: HF.frame_rotate_ragged(frames().float(), params(8), ragged(), table64()),
    'frame_rotate_ragged-channels': lambda HF: HF.frame_rotate_ragged(frames('chw'), params(8), ragged(), table64()),
    'frame_rotate_ragged-norm': lambda HF: HF.frame_rotate_ragged(frames(), params(8), ragged(), table64(), norm=norm('chw')),
    'frame_rotate_ragged-fill4': lambda HF: HF.frame_rotate_ragged(frames(), params(8), ragged(), table64(), fill=(1, 2, 3, 4)),
    'frame_rotate_ragged-pad_fill256': lambda HF: HF.frame_rotate_ragged(frames(), params(8), ragged(), table64(), pad_fill=(0, 256, 0)),
    'frame_rotate_ragged-matrices': lambda HF: HF.frame_rotate_ragged(frames(), params(8), ragged(), table64().float()),
    'frame_rotate_ragged-params_words': lambda HF: HF.frame_rotate_ragged(frames(), params(), ragged(), table64()),
    'frame_rotate_ragged-out_shape': lambda HF: HF.frame_rotate_ragged(frames(), params(8), ragged(), table64(), size=(6, 8),
                                                                        out=torch.empty(B, H, W, 3, dtype=U8)),
    'frame_rotate_ragged-out_dtype': lambda HF: HF.frame_rotate_ragged(frames(), params(8), ragged(), table64(), norm=norm(),
                                                                        out=torch.empty(B, 3, H, W, dtype=U8)),
    'frame_rotate_ragged-out_device': lambda HF: HF.frame_rotate_ragged(frames(), params(8), ragged(), table64(), out=meta((B, H, W, 3), U8)),
    # labels: a dtype other than uint8 / int64, the rank
    'label_resize-dtype': lambda HF: HF.label_resize(labels(torch.int32), (4, 6)),
    'label_resize-float': lambda HF: HF.label_resize(labels().float(), (4, 6)),
    'label_resize-rank': lambda HF: HF.label_resize(labels()[0], (4, 6)),
    'label_resize-fill300_uint8': lambda HF: HF.label_resize(labels(), (4, 6), fill=300),
    'label_resize-fill300_uint8_out': lambda HF: HF.label_resize(labels(I64), (4, 6), fill=300, out=torch.empty(B, 4, 6, dtype=U8)),
    'label_resize-fill_wide': lambda HF: HF.label_resize(labels(I64), (4, 6), fill=2 ** 31),
    'label_resize-out_shape': lambda HF: HF.label_resize(labels(), (4, 6), out=torch.empty(B, 4, 7, dtype=U8)),
    'label_resize-out_dtype': lambda HF: HF.label_resize(labels(), (4, 6), out=torch.empty(B, 4, 6, dtype=torch.int32)),
    'label_resize-out_device': lambda HF: HF.label_resize(labels(), (4, 6), out=meta((B, 4, 6), U8)),
    'label_resize_batch-dtype': lambda HF: HF.label_resize_batch(labels(torch.int32), params(), tables()),
    'label_resize_batch-rank': lambda HF: HF.label_resize_batch(labels()[0], params(), tables()),
    'label_resize_batch-fill300_uint8': lambda HF: HF.label_resize_batch(labels(), params(), tables(), fill=300),
    'label_resize_batch-out_shape': lambda HF: HF.label_resize_batch(labels(), params(), tables(), out=torch.empty(B, H, W + 1, dtype=U8)),
    'label_resize_batch-out_dtype': lambda HF: HF.label_resize_batch(labels(), params(), tables(), out=torch.empty(B, H, W)),
    'label_resize_batch-out_device': lambda HF: HF.label_resize_batch(labels(), params(), tables(), out=meta((B, H, W), U8)),
    'label_resize_batch-params_words': lambda HF: HF.label_resize_batch(labels(), params(8), tables()),
    'label_resize_batch-params_strided': lambda HF: HF.label_resize_batch(labels(), strided(6), tables()),
    'label_rotate-dtype': lambda HF: HF.label_rotate(labels(torch.int32), 10.0),
    'label_rotate-rank': lambda HF: HF.label_rotate(labels()[0], 10.0),
    'label_rotate-out_shape': lambda HF: HF.label_rotate(labels(), 10.0, out=torch.empty(B, H, W + 1, dtype=U8)),
    'label_rotate-out_device': lambda HF: HF.label_rotate(labels(), 10.0, out=meta((B, H, W), U8)),
    'label_rotate-table': lambda HF: HF.label_rotate(labels(), None, table=fixed().long()),
    'label_resize_ragged-dtype': lambda HF: HF.label_resize_ragged(labels(torch.int32), params(8), ragged()),
    'label_resize_ragged-rank': lambda HF: HF.label_resize_ragged(labels()[0], params(8), ragged()),
    'label_resize_ragged-params_words': lambda HF: HF.label_resize_ragged(labels(), params(), ragged()),
    'label_resize_ragged-out_shape': lambda HF: HF.label_resize_ragged(labels(), params(8), ragged(), out=torch.empty(B, H, W + 1, dtype=U8)),
    'label_resize_ragged-out_dtype': lambda HF: HF.label_resize_ragged(labels(), params(8), ragged(), out=torch.empty(B, H, W, dtype=I64)),
    'label_resize_ragged-out_device': lambda HF: HF.label_resize_ragged(labels(), params(8), ragged(), out=meta((B, H, W), U8)),
    'label_rotate_ragged-dtype': lambda HF: HF.label_rotate_ragged(labels(I64), params(8), ragged(), fixed()),
    'label_rotate_ragged-rank': lambda HF: HF.label_rotate_ragged(labels()[0], params(8), ragged(), fixed()),
    'label_rotate_ragged-fill300_uint8': lambda HF: HF.label_rotate_ragged(labels(), params(8), ragged(), fixed(), fill=300,
                                                                            out=torch.empty(B, H, W, dtype=U8)),
    'label_rotate_ragged-pad_fill300_uint8': lambda HF: HF.label_rotate_ragged(labels(), params(8), ragged(), fixed(), pad_fill=300,
                                                                                out=torch.empty(B, H, W, dtype=U8)),
    'label_rotate_ragged-fixed': lambda HF: HF.label_rotate_ragged(labels(), params(8), ragged(), fixed()[:, :5].contiguous()),
    'label_rotate_ragged-params_strided': lambda HF: HF.label_rotate_ragged(labels(), strided(8), ragged(), fixed()),
    'label_rotate_ragged-out_shape': lambda HF: HF.label_rotate_ragged(labels(), params(8), ragged(), fixed(), out=torch.empty(B, H, W + 1, dtype=I64)),
    'label_rotate_ragged-out_dtype': lambda HF: HF.label_rotate_ragged(labels(), params(8), ragged(), fixed(), out=torch.empty(B, H, W)),
    'label_rotate_ragged-out_device': lambda HF: HF.label_rotate_ragged(labels(), params(8), ragged(), fixed(), out=meta((B, H, W), I64)),
    # the table launches: params, the workspace one element short
    'resize_tables-params_words': lambda HF: HF.resize_tables(params()[:, :5].contiguous(), (H, W), (H, W), 'bicubic', KS),
    'resize_tables-params_strided': lambda HF: HF.resize_tables(strided(6), (H, W), (H, W), 'bicubic', KS),
    'resize_tables-params_dtype': lambda HF: HF.resize_tables(params().long(), (H, W), (H, W), 'bicubic', KS),
    'resize_tables-filter': lambda HF: HF.resize_tables(params(), (H, W), (H, W), 'lanczos', KS),
    'resize_tables-workspace_short': lambda HF: HF.resize_tables(params(), (H, W), (H, W), 'bicubic', KS, workspace=short(HF.ResizeTables)),
    'resize_tables-workspace_dtype': lambda HF: HF.resize_tables(params(), (H, W), (H, W), 'bicubic', KS, workspace=tables().workspace.long()),
    'resize_tables-workspace_device': lambda HF: HF.resize_tables(params(), (H, W), (H, W), 'bicubic', KS,
                                                                  workspace=meta((HF.ResizeTables.words(B, (H, W), KS),), torch.int32)),
    'resize_tables_ragged-params_words': lambda HF: HF.resize_tables_ragged(params(), (H, W), (H, W), 'bicubic', KS),
    'resize_tables_ragged-params_strided': lambda HF: HF.resize_tables_ragged(strided(8), (H, W), (H, W), 'bicubic', KS),
    'resize_tables_ragged-filter': lambda HF: HF.resize_tables_ragged(params(8), (H, W), (H, W), 'lanczos', KS),
    'resize_tables_ragged-workspace_short': lambda HF: HF.resize_tables_ragged(params(8), (H, W), (H, W), 'bicubic', KS,
                                                                               workspace=short(HF.RaggedTables)),
    'resize_tables_ragged-workspace_strided': lambda HF: HF.resize_tables_ragged(
        params(8), (H, W), (H, W), 'bicubic', KS, workspace=torch.zeros(2 * HF.RaggedTables.words(B, (H, W), KS), dtype=torch.int32)[::2]),
}


@pytest.mark.parametrize('name', sorted(GOOD))
def test_good_operands_reach_the_library(name):
    from hyperseg_amd._hip import HipLibraryError
    where, call = GOOD[name]
    if where == 'cpu':
        assert isinstance(call(hf()), torch.Tensor)
    else:
        with pytest.raises(HipLibraryError):
            call(hf())


@pytest.mark.parametrize('name', sorted(REFUSED))
def test_wrapper_refuses(name):
    with pytest.raises(ValueError):
        REFUSED[name](hf())


# ------------------------------------------------------------------------------------------------ the four augment entry points
CROP, PAD = (4, 6), 8
OFFSETS = [(1, -2), (0, 3)]


def crop_augment(scale, offset, hflip, x=None, t=None, **kw):
    from hyperseg_amd.training import device_augment
    return device_augment(frames() if x is None else x, labels() if t is None else t, scale, CROP, offset, hflip, norm(), **kw)


def batch_augment(**kw):
    from hyperseg_amd.training import BatchAugment
    return BatchAugment((H, W), CROP, norm(), (0.5, 2.0), **kw)


def voc_augment(hflip, scale, angle, x=None, t=None, jitter=None, **kw):
    from hyperseg_amd.training import device_augment_voc
    return device_augment_voc(frames() if x is None else x, labels() if t is None else t, hflip, jitter, scale, angle, PAD, norm(), **kw)


def voc_batch(**kw):
    from hyperseg_amd.training import BatchAugmentVOC
    return BatchAugmentVOC((H, W), PAD, norm(), (0.5, 1.5), **kw)


SIZES = [(H, W), (3, 4)]
JITTER = (('brightness',), 1.2)          # as a ColorJitterParams: one for the batch; as a plain tuple only inside a sequence


def one_jitter():
    from hyperseg_amd import ColorJitterParams
    return ColorJitterParams(*JITTER)

AUGMENT_REFUSED = {
    'device_augment-scales': lambda: crop_augment([1.0] * (B + 1), (0, 0), False),
    'device_augment-offsets': lambda: crop_augment(1.0, [(0, 0)] * (B + 1), False),
    'device_augment-flips': lambda: crop_augment(1.0, (0, 0), [True] * (B + 1)),
    'device_augment-scale_tensor': lambda: crop_augment(torch.ones(B + 1), (0, 0), False),
    'device_augment-frames_dtype': lambda: crop_augment(1.0, (0, 0), False, x=frames().float()),
    'device_augment-frames_channels': lambda: crop_augment(1.0, (0, 0), False, x=frames('chw')),
    'device_augment-labels_shape': lambda: crop_augment(1.0, (0, 0), False, t=labels()[:, :4]),
    'device_augment-labels_dtype': lambda: crop_augment(1.0, (0, 0), False, t=labels().float()),
    'device_augment-fill4': lambda: crop_augment(1.0, (0, 0), False, fill=(1, 2, 3, 4)),
    'device_augment-jitters': lambda: crop_augment(1.0, (0, 0), False, jitter=[JITTER] * (B + 1)),
    'BatchAugment-scales': lambda: batch_augment(batch=B).rows([1.0] * (B + 1), (0, 0), False),
    'BatchAugment-offsets': lambda: batch_augment(batch=B).rows(1.0, [(0, 0)] * (B + 1), False),
    'BatchAugment-flips': lambda: batch_augment(batch=B).rows(1.0, (0, 0), [False] * (B + 1)),
    'BatchAugment-scale_range': lambda: batch_augment(batch=B).rows([1.0, 0.4], (0, 0), False),
    'BatchAugment-call_scales': lambda: batch_augment()(frames(), labels(), [1.0] * (B + 1), (0, 0), False),
    'BatchAugment-frames_dtype': lambda: batch_augment()(frames().float(), labels(), 1.0, (0, 0), False),
    'BatchAugment-frames_size': lambda: batch_augment()(frames()[:, :4], labels()[:, :4], 1.0, (0, 0), False),
    'BatchAugment-labels_shape': lambda: batch_augment()(frames(), labels()[:1], 1.0, (0, 0), False),
    'BatchAugment-labels_device': lambda: batch_augment()(frames(), meta((B, H, W), U8), 1.0, (0, 0), False),
    'BatchAugment-batch_latch': lambda: batch_augment(batch=B + 1)(frames(), labels(), 1.0, (0, 0), False),
    'BatchAugment-run_without_params': lambda: batch_augment().run(frames(), labels()),
    'BatchAugment-nothing_left': lambda: batch_augment().__class__((H, W), CROP, norm(), (0.01, 1.0)),
    'BatchAugment-scale_range_order': lambda: batch_augment().__class__((H, W), CROP, norm(), (2.0, 1.0)),
    'device_augment_voc-flips': lambda: voc_augment([True] * (B + 1), 1.0, 0.0),
    'device_augment_voc-scales': lambda: voc_augment(False, [1.0] * (B + 1), 0.0),
    'device_augment_voc-angles': lambda: voc_augment(False, 1.0, [0.0] * (B + 1)),
    'device_augment_voc-scale_tensor': lambda: voc_augment(False, torch.ones(B + 1), 0.0),
    'device_augment_voc-jitters': lambda: voc_augment(False, 1.0, 0.0, jitter=[JITTER] * (B + 1)),
    'device_augment_voc-frames_dtype': lambda: voc_augment(False, 1.0, 0.0, x=list(frames().float())),
    'device_augment_voc-frames_rank': lambda: voc_augment(False, 1.0, 0.0, x=[frames()[0], frames()[1:]]),
    'device_augment_voc-frames_channels': lambda: voc_augment(False, 1.0, 0.0, x=list(frames('chw'))),
    'device_augment_voc-labels_dtype': lambda: voc_augment(False, 1.0, 0.0, t=list(labels(torch.int32))),
    'device_augment_voc-labels_shape': lambda: voc_augment(False, 1.0, 0.0, t=[labels()[0], labels()[1, :4]]),
    'device_augment_voc-labels_count': lambda: voc_augment(False, 1.0, 0.0, t=labels()[:1]),
    'device_augment_voc-labels_device': lambda: voc_augment(False, 1.0, 0.0, t=[labels()[0], meta((H, W), U8)]),
    'device_augment_voc-exceeds_pad': lambda: voc_augment(False, 2.0, 0.0),
    'device_augment_voc-nothing_left': lambda: voc_augment(False, 0.01, 0.0),
    'device_augment_voc-fill4': lambda: voc_augment(False, 1.0, 0.0, fill=(1, 2, 3, 4)),
    'device_augment_voc-rotate_fill256': lambda: voc_augment(False, 1.0, 0.0, rotate_fill=256),
    'BatchAugmentVOC-flips': lambda: voc_batch(batch=B).rows(SIZES, [True] * (B + 1), None, 1.0, 0.0),
    'BatchAugmentVOC-scales': lambda: voc_batch(batch=B).rows(SIZES, False, None, [1.0] * (B + 1), 0.0),
    'BatchAugmentVOC-angles': lambda: voc_batch(batch=B).rows(SIZES, False, None, 1.0, [0.0] * (B + 1)),
    'BatchAugmentVOC-sizes': lambda: voc_batch(batch=B).rows(SIZES + SIZES[:1], False, None, 1.0, 0.0),
    'BatchAugmentVOC-extent': lambda: voc_batch(batch=B).rows([(H + 1, W), (3, 4)], False, None, 1.0, 0.0),
    'BatchAugmentVOC-scale_range': lambda: voc_batch(batch=B).rows(SIZES, False, None, [1.0, 1.6], 0.0),
    'BatchAugmentVOC-exceeds_pad': lambda: voc_batch(batch=B).rows(SIZES, False, None, [1.5, 1.0], 0.0),
    'BatchAugmentVOC-fill4': lambda: voc_batch(fill=(1, 2, 3, 4)),
    'BatchAugmentVOC-rotate_fill256': lambda: voc_batch(rotate_fill=(0, 0, 256)),
    'BatchAugmentVOC-labels_dtype': lambda: voc_batch()(frames(), labels(torch.int32), SIZES, False, None, 1.0, 0.0),
    'BatchAugmentVOC-labels_device': lambda: voc_batch()(frames(), meta((B, H, W), U8), SIZES, False, None, 1.0, 0.0),
    'BatchAugmentVOC-canvas': lambda: voc_batch()(frames()[:, :4], labels()[:, :4], SIZES, False, None, 1.0, 0.0),
    'BatchAugmentVOC-batch_latch': lambda: voc_batch(batch=B + 1)(frames(), labels(), SIZES, False, None, 1.0, 0.0),
    'BatchAugmentVOC-no_sizes': lambda: voc_batch()(frames(), labels(), None, False, None, 1.0, 0.0),
    'BatchAugmentVOC-list_with_sizes': lambda: voc_batch()(list(frames()), list(labels()), SIZES, False, None, 1.0, 0.0),
    'BatchAugmentVOC-list_frames_dtype': lambda: voc_batch()(list(frames().float()), list(labels()), None, False, None, 1.0, 0.0),
    'BatchAugmentVOC-list_frames_channels': lambda: voc_batch()(list(frames('chw')), list(labels()), None, False, None, 1.0, 0.0),
    'BatchAugmentVOC-list_labels_dtype': lambda: voc_batch()(list(frames()), list(labels(torch.int32)), None, False, None, 1.0, 0.0),
    'BatchAugmentVOC-list_labels_mixed': lambda: voc_batch()(list(frames()), [labels()[0], labels(I64)[1]], None, False, None, 1.0, 0.0),
    'BatchAugmentVOC-list_labels_shape': lambda: voc_batch()(list(frames()), [labels()[0], labels()[1, :4]], None, False, None, 1.0, 0.0),
    'BatchAugmentVOC-list_labels_count': lambda: voc_batch()(list(frames()), list(labels())[:1], None, False, None, 1.0, 0.0),
    'BatchAugmentVOC-list_does_not_fit': lambda: voc_batch().__class__((4, W), PAD, norm())(list(frames()), list(labels()), None, False, None, 1.0, 0.0),
    'BatchAugmentVOC-run_without_params': lambda: voc_batch().run(frames(), labels()),
    'BatchAugmentVOC-upload_before_buffers': lambda: voc_batch(batch=B).upload(voc_batch(batch=B).rows(SIZES, False, None, 1.0, 0.0)),
}


@pytest.mark.parametrize('name', sorted(AUGMENT_REFUSED))
def test_augment_refuses(name):
    with pytest.raises(ValueError):
        AUGMENT_REFUSED[name]()


def same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b)) and len(a) == len(b)


def test_crop_forms_of_a_per_sample_argument():
    """One value, a 0-d tensor or array, a list, a tuple, a tensor or array with a dimension: the same rows, the same result."""
    aug = batch_augment(batch=B)
    want = aug.rows([0.5, 0.5], [(1, -2), (1, -2)], [True, True])
    assert want.tolist() == [[2, 4, 1, -2, 1, 0]] * B                     # numpy's rounding of (2.5, 3.5): half to even
    for scale in (0.5, torch.tensor(0.5), np.float64(0.5), np.array(0.5), (0.5, 0.5), torch.tensor([0.5, 0.5]), np.array([0.5, 0.5])):
        for offset in ((1, -2), [1, -2], torch.tensor([1, -2]), np.array([1, -2]), [(1, -2), (1, -2)], torch.tensor([[1, -2], [1, -2]])):
            for hflip in (True, 1, torch.tensor(True), np.bool_(True), (True, True), torch.tensor([True, True])):
                assert torch.equal(aug.rows(scale, offset, hflip), want)
    # a single (top, left) pair against a list of pairs: with B = 2 only the nesting tells them apart
    assert aug.rows(1.0, (1, 2), False)[:, 2:4].tolist() == [[1, 2], [1, 2]]
    assert aug.rows(1.0, [(1, 2), (3, 4)], False)[:, 2:4].tolist() == [[1, 2], [3, 4]]
    assert aug.rows(1.0, ([1, 2], [3, 4]), False)[:, 2:4].tolist() == [[1, 2], [3, 4]]
    assert aug.rows([2.0, 0.5], OFFSETS, [False, True]).tolist() == [[10, 14, 1, -2, 0, 0], [2, 4, 0, 3, 1, 0]]
    # the per-sample route and the batch object take the same forms and give the same result
    want = crop_augment([0.5, 0.5], [(1, -2), (1, -2)], [True, True])
    for scale, offset, hflip in ((0.5, (1, -2), True), (torch.tensor(0.5), torch.tensor([1, -2]), torch.tensor(True)),
                                 (np.array([0.5, 0.5]), [[1, -2], [1, -2]], (1, 1))):
        assert same(crop_augment(scale, offset, hflip), want)
        assert same(batch_augment()(frames(), labels(), scale, offset, hflip), want)
    assert same(batch_augment().run(frames(), labels(), params=aug.rows(0.5, (1, -2), True)), want)
    want = crop_augment([2.0, 0.5], OFFSETS, [False, True], jitter=[JITTER, JITTER], lbl_fill=7, fill=(1, 2, 3))
    assert same(batch_augment(lbl_fill=7, fill=(1, 2, 3))(frames(), labels(), [2.0, 0.5], OFFSETS, [False, True], jitter=one_jitter()), want)
    assert not same(want, crop_augment([2.0, 0.5], OFFSETS, [False, True], lbl_fill=7, fill=(1, 2, 3)))


def test_voc_forms_of_a_per_sample_argument():
    aug = voc_batch(batch=B)
    want = aug.rows(SIZES, [True, True], None, [0.5, 0.5], [10.0, 10.0])
    assert want.rows.tolist() == [[H, W, 2, 4, 1, 0, 0, 0], [3, 4, 2, 2, 1, 0, 0, 0]]
    for sizes in (SIZES, torch.tensor(SIZES), np.array(SIZES)):
        for hflip in (True, torch.tensor(True), (True, True), torch.tensor([True, True])):
            for scale in (0.5, torch.tensor(0.5), np.array(0.5), [0.5, 0.5], np.array([0.5, 0.5])):
                for angle in (10.0, 10, torch.tensor(10.0), [10.0, 10.0], torch.tensor([10.0, 10.0]), np.array([10.0, 10.0])):
                    got = aug.rows(sizes, hflip, None, scale, angle)
                    assert all(torch.equal(getattr(got, f), getattr(want, f)) for f in ('rows', 'matrices', 'fixed', 'jitter'))
                    assert got.jitters is None and not got.contrast
    untouched = aug.rows(SIZES, False, None, [None, 1.0], 0.0)                # RandomResize did not fire: outside scale_range, not refused
    assert untouched.rows[:, 2:4].tolist() == [list(s) for s in SIZES]
    assert torch.equal(aug.rows(SIZES, False, None, None, 0.0).rows, untouched.rows)
    # the per-sample route, the canvas and the list of ragged samples
    xs = [frames()[0], frames()[1, :3, :4]]
    ts = [labels()[0], labels()[1, :3, :4]]
    kw = dict(fill=(5, 6, 7), lbl_fill=250, rotate_fill=(8, 9, 10), lbl_rotate_fill=3)
    want = voc_augment([True, True], [0.5, 0.5], [10.0, 10.0], x=xs, t=ts, jitter=[JITTER, JITTER], **kw)
    for hflip, scale, angle in ((True, 0.5, 10.0), (torch.tensor(True), torch.tensor(0.5), torch.tensor(10.0)),
                                ((1, 1), np.array([0.5, 0.5]), [10, 10])):
        assert same(voc_augment(hflip, scale, angle, x=xs, t=ts, jitter=one_jitter(), **kw), want)
        assert same(voc_batch(**kw)(frames(), labels(), SIZES, hflip, one_jitter(), scale, angle), want)
        assert same(voc_batch(**kw)(xs, ts, None, hflip, one_jitter(), scale, angle), want)
    assert same(voc_augment(True, 0.5, 10.0, jitter=one_jitter(), **kw), voc_batch(**kw)(frames(), labels(), [(H, W)] * B, True, one_jitter(), 0.5, 10.0))
    assert not same(want, voc_augment(True, 0.5, 10.0, x=xs, t=ts, **kw))


def test_augment_module_and_import_hygiene():
    """The moved names are the same objects under both modules, and importing the package with them does not load the HIP library."""
    code = ('import sys, hyperseg_amd, hyperseg_amd.augment as A\n'
            'assert "hyperseg_amd.training" not in sys.modules                # augment stands without training\n'
            'import hyperseg_amd.training as T\n'
            'assert "hyperseg_amd._hip" not in sys.modules and "hyperseg_amd.functional" not in sys.modules\n'
            f'assert all(getattr(T, n) is getattr(A, n) for n in {MOVED!r})\n')
    subprocess.run([sys.executable, '-c', code], cwd=REPO, check=True, timeout=120)
