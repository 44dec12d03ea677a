"""The scoring entries of the forward's last launch (hs_eval.hip, hs_validate.hip) at the C boundary: what each refuses, with which status,
and that a refused call launches nothing.  The statuses are literals read off the entries as they stood before their launch fronts were
shared (hs_eval_count.h): the fronts must keep every entry's own order of refusals, the places where the entries differ
included -- 257 classes are a bad argument to the two counting-only entries and unsupported to the loss entries, which ask the LDS limit
first; the loss entries ask nothing of num_classes where there is no matrix.

Smallest legal shapes: x 1 x 5 x 8 x 12, mid 16 x 24, label 32 x 48, five classes; a one-stage entry resizes to the mid.  Inputs are zeros,
outputs are pre-filled with a sentinel byte: a refused call must leave them as they were.  The accepted side of every kernel form is
test_hip_eval*.py's, test_hip_validate*.py's and test_hip_weighted_loss.py's; here one accepted call per entry shows that the operands the
refusals are cut from are good."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

OK, BAD_ARG, UNSUPPORTED = 0, -1, -3
SENTINEL = 0xA5
B, CH, HI, WI, HM, WM, HO, WO, CLS = 1, 5, 8, 12, 16, 24, 32, 48, 5
LABEL = HO * WO
RESIZE1 = dict(Hi=HI, Wi=WI, Ho=HM, Wo=WM)
RESIZE2 = dict(Hi=HI, Wi=WI, Hm=HM, Wm=WM, Ho=HO, Wo=WO)

# entry -> (its arguments in order, its sizes, the pointers it cannot do without)
ENTRIES = {
    'hs_upsample_confusion_fwd': ('x batch channels Hi Wi Ho Wo target tdt ncls per_image confusion mask stream', RESIZE1, 'x target confusion'),
    'hs_upsample2_confusion_fwd': ('x batch channels Hi Wi Hm Wm Ho Wo target tdt ncls per_image confusion mask stream', RESIZE2, 'x target confusion'),
    'hs_confusion_fwd': ('pred pdt target tdt batch elements ncls per_image confusion stream', dict(elements=LABEL), 'pred target confusion'),
    'hs_cross_entropy_score_fwd': ('sdt logits target64 batch channels pixels ignore loss ncls per_image confusion mask stream',
                                   dict(pixels=HM * WM), 'logits target64 loss'),
    'hs_cross_entropy_score_weighted_fwd': ('sdt logits target64 weight batch channels pixels ignore loss ncls per_image confusion mask stream',
                                            dict(pixels=HM * WM), 'logits target64 loss weight'),
    'hs_upsample_ce_confusion_fwd': ('x batch channels Hi Wi Ho Wo target tdt ignore loss ncls per_image confusion mask stream', RESIZE1,
                                     'x target loss'),
    'hs_upsample_ce_confusion_weighted_fwd': ('x batch channels Hi Wi Ho Wo target tdt weight ignore loss ncls per_image confusion mask stream',
                                              RESIZE1, 'x target loss weight'),
    'hs_upsample2_ce_confusion_fwd': ('x batch channels Hi Wi Hm Wm Ho Wo target tdt ignore loss ncls per_image confusion mask stream', RESIZE2,
                                      'x target loss'),
    'hs_upsample2_ce_confusion_weighted_fwd': ('x batch channels Hi Wi Hm Wm Ho Wo target tdt weight ignore loss ncls per_image confusion mask stream',
                                               RESIZE2, 'x target loss weight'),
}
COUNTING = ('hs_upsample_confusion_fwd', 'hs_upsample2_confusion_fwd')
LOSS = tuple(e for e in ENTRIES if 'ce_confusion' in e or 'cross_entropy' in e)
TYPE_CODES = {'tdt', 'pdt', 'sdt'}                       # target / prediction storage (HS_EVAL_*), logits storage (HS_DTYPE_*): 0 is valid in each


class _Operands:
    """The good operands of every entry (each takes the ones it names), kept alive for the case."""

    def __init__(self):
        dev = torch.device('cuda:0')
        self.ins = dict(x=torch.zeros(B * CH * HI * WI, device=dev), logits=torch.zeros(B * CH * HM * WM, device=dev),
                        target=torch.zeros(B * LABEL, dtype=torch.uint8, device=dev), pred=torch.zeros(B * LABEL, dtype=torch.uint8, device=dev),
                        target64=torch.zeros(B * HM * WM, dtype=torch.int64, device=dev), weight=torch.ones(CH, device=dev))
        self.outs = dict(confusion=torch.full((8 * CLS * CLS,), SENTINEL, dtype=torch.uint8, device=dev),
                         loss=torch.full((4 * B * LABEL,), SENTINEL, dtype=torch.uint8, device=dev),
                         mask=torch.full((B * LABEL,), SENTINEL, dtype=torch.uint8, device=dev))
        self.good = dict(batch=B, channels=CH, tdt=0, pdt=0, sdt=0, ncls=CLS, per_image=0, ignore=255,
                         stream=C.c_void_p(torch.cuda.current_stream().cuda_stream))
        self.good.update({k: C.c_void_p(t.data_ptr()) for k, t in {**self.ins, **self.outs}.items()})

    def call(self, entry, **changed):
        from hyperseg_amd import _hip
        order, sizes, _ = ENTRIES[entry]
        args = {**self.good, **sizes, **changed}
        unknown = set(changed) - set(order.split())
        assert not unknown, (entry, unknown)
        return getattr(_hip.lib, entry)(*[args[k] for k in order.split()])

    def untouched(self):
        torch.cuda.synchronize()
        return all(bool((t == SENTINEL).all()) for t in self.outs.values())

    def refused(self, entry, status, **changed):
        got = self.call(entry, **changed)
        assert got == status, f'{entry}({changed}) returned {got}, expected {status}'
        assert self.untouched(), f'{entry}({changed}) was refused but an output buffer changed'


@pytest.fixture(scope='module')
def ops():
    return _Operands()


@pytest.mark.parametrize('entry', list(ENTRIES))
def test_good_operands_are_accepted(entry, ops):
    assert ops.call(entry) == OK
    torch.cuda.synchronize()
    for t in ops.outs.values():
        t.fill_(SENTINEL)


@pytest.mark.parametrize('entry', list(ENTRIES))
def test_null_pointers_zero_sizes_and_unknown_type_codes_are_bad_arguments(entry, ops):
    order, sizes, required = ENTRIES[entry]
    for name in required.split():
        ops.refused(entry, BAD_ARG, **{name: None})
    for name in ['batch', 'channels', *sizes]:
        if name in order.split():
            ops.refused(entry, BAD_ARG, **{name: 0})
    for name in TYPE_CODES & set(order.split()):
        ops.refused(entry, BAD_ARG, **{name: 7})
    if entry == 'hs_confusion_fwd':
        ops.refused(entry, BAD_ARG, ncls=0)
    if entry == 'hs_upsample2_confusion_fwd':                 # masks only is target AND matrix null, with a mask to write
        ops.refused(entry, BAD_ARG, target=None, confusion=None, mask=None)


@pytest.mark.parametrize('entry', list(ENTRIES))
def test_batch_past_the_grid_limit_is_unsupported(entry, ops):
    ops.refused(entry, UNSUPPORTED, batch=65536)


@pytest.mark.parametrize('entry', COUNTING)
@pytest.mark.parametrize('ncls, status', [(0, BAD_ARG), (4, BAD_ARG), (129, UNSUPPORTED), (257, BAD_ARG)])
def test_num_classes_ladder_of_the_counting_entries(entry, ncls, status, ops):
    ops.refused(entry, status, ncls=ncls)


@pytest.mark.parametrize('entry', LOSS)
@pytest.mark.parametrize('ncls, status', [(0, BAD_ARG), (4, BAD_ARG), (129, UNSUPPORTED), (257, UNSUPPORTED)])
def test_num_classes_ladder_of_the_loss_entries(entry, ncls, status, ops):
    ops.refused(entry, status, ncls=ncls)
    assert ops.call(entry, ncls=ncls, confusion=None) == OK   # no matrix: nothing is asked of num_classes
    torch.cuda.synchronize()
    assert bool((ops.outs['confusion'] == SENTINEL).all())
    for t in ops.outs.values():
        t.fill_(SENTINEL)


def test_masks_only_call_with_257_channels_is_unsupported(ops):
    ops.refused('hs_upsample2_confusion_fwd', UNSUPPORTED, target=None, confusion=None, channels=257)


def test_confusion_of_finished_masks_past_the_lds_limit_is_unsupported(ops):
    ops.refused('hs_confusion_fwd', UNSUPPORTED, ncls=129)
