"""The storage-type dispatcher of the typed training launchers (hs_common.h: with_storage) at the C boundary: a `dtype` code that is none of
HS_DTYPE_F32 / BF16 / F16 is answered with HS_ERR_BAD_ARG before anything is launched, and each of the three real codes is launched.

One entry per translation unit that dispatches on the code, plus the entries whose type ladder ended in a bare `else` (the bf16 arm) before
the dispatcher existed.  Smallest legal shapes: batch 1, 4 channels, an 8 x 8 map, a 2 x 2 weight grid, 4 classes.  Inputs are zeros (valid
in every storage type), outputs are pre-filled with a sentinel byte: a refused call must leave them as they were."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

F32, BF16, F16 = 0, 1, 2
BAD_ARG = -1
SENTINEL = 0xA5
B, CH, H, W, FH, FW, CLS = 1, 4, 8, 8, 2, 2, 4
PH, PW = H // FH, W // FW
PIX = H * W
TILED = B * CH * FH * (PH + 2) * FW * (PW + 2)          # the halo-tile image
BN_LARGE_PIX = 16 * 1024 + 64                           # past BN_SMALL_MAX: the two-launch BatchNorm path


class _Bufs:
    """Device buffers of one case, kept alive for its duration.  zeros(n): n fp32 zeros (room for any storage type); out(n): room for n
    fp32 elements filled with the sentinel byte; ptr(t): its address."""

    def __init__(self):
        self.dev = torch.device('cuda:0')
        self.outs = []

    def zeros(self, n, dtype=torch.float32):
        return torch.zeros(n, dtype=dtype, device=self.dev)

    def ones(self, n):
        return torch.ones(n, dtype=torch.float32, device=self.dev)

    def out(self, n):
        t = torch.full((4 * n,), SENTINEL, dtype=torch.uint8, device=self.dev)
        self.outs.append(t)
        return t

    def untouched(self):
        torch.cuda.synchronize()
        return all(bool((t == SENTINEL).all()) for t in self.outs)

    def refill(self):
        for t in self.outs:
            t.fill_(SENTINEL)


def _p(t):
    return C.c_void_p(t.data_ptr())


def _bn_fwd(lib, m, pixels=PIX):
    x, g, b, y, mean, invstd = m.zeros(CH * pixels), m.ones(CH), m.zeros(CH), m.out(CH * pixels), m.out(CH), m.out(CH)
    ws, steps = m.out(lib.hs_bn_train_workspace(CH) // 4), m.zeros(1, torch.int64)
    return lambda d, s: lib.hs_bn_act_train_fwd(d, _p(x), B, CH, pixels, _p(g), _p(b), None, None, 0.1, 1e-5, 2, _p(mean), _p(invstd), _p(ws), _p(y),
                                                _p(steps), s)


def _bn_bwd(lib, m, pixels=PIX):
    x, dy, g, b, mean, invstd = m.zeros(CH * pixels), m.zeros(CH * pixels), m.ones(CH), m.zeros(CH), m.zeros(CH), m.ones(CH)
    ws, dx, dg, db = m.out(lib.hs_bn_train_workspace(CH) // 4), m.out(CH * pixels), m.out(CH), m.out(CH)
    return lambda d, s: lib.hs_bn_act_train_bwd(d, _p(x), _p(dy), B, CH, pixels, _p(g), _p(b), _p(mean), _p(invstd), 1e-5, 2, _p(ws), _p(dx), _p(dg),
                                                _p(db), s)


def _halo_bwd(lib, m):
    dt, dx = m.zeros(TILED), m.out(B * CH * PIX)
    return lambda d, s: lib.hs_halo_tiles_bwd(d, _p(dt), B, CH, H, W, FH, FW, _p(dx), 0, s)


def _upsample_bwd(lib, m):
    dy, dx = m.zeros(B * CH * PIX), m.out(B * CH * (H // 2) * (W // 2))
    return lambda d, s: lib.hs_upsample_bilinear_typed_bwd(d, _p(dy), 0, B, CH, H // 2, W // 2, H, W, _p(dx), s)


def _bootstrapped_ce_fwd(lib, m):
    logits, target = m.zeros(B * CLS * PIX), m.zeros(B * PIX, torch.int64)
    ws, loss, out8, mean = m.out(B * lib.hs_bootstrap_mean_workspace() // 4), m.out(B * PIX), m.out(B * 8), m.out(1)
    return lambda d, s: lib.hs_bootstrapped_ce_fwd(d, _p(logits), _p(target), B, CLS, PIX, 255, 4, 0.3, _p(ws), _p(loss), _p(out8), _p(mean), s)


def _dw_tiles_fwd(lib, m):
    tiled, bank, y = m.zeros(TILED), m.zeros(FH * FW * 9 * CH), m.out(B * CH * PIX)
    return lambda d, s: lib.hs_dw_tiles_fwd(d, _p(tiled), _p(bank), 9 * CH, B, CH, H, W, FH, FW, _p(y), 0, s)


def _dw_tiles_bwd_w(lib, m):
    tiled, dy, dbank = m.zeros(TILED), m.zeros(B * CH * PIX), m.out(FH * FW * 9 * CH)
    return lambda d, s: lib.hs_dw_tiles_bwd_w(d, _p(tiled), _p(dy), B, CH, H, W, FH, FW, _p(dbank), 9 * CH, 0, s)


def _patch_conv_bn_bwd_w(lib, m):
    x, dy, g, b, mean, invstd = m.zeros(B * CH * PIX), m.zeros(B * CH * PIX), m.ones(CH), m.zeros(CH), m.zeros(CH), m.ones(CH)
    dbank = m.out(FH * FW * CH * CH)
    return lambda d, s: lib.hs_patch_conv_bn_bwd_w(d, _p(x), _p(dy), _p(g), _p(b), _p(mean), _p(invstd), 2, B, CH, H, W, FH, FW, CH, _p(dbank), CH * CH, s)


def _plain_fwd(lib, m):          # k = 1: fp32 takes the generic kernel, the half types hs_patch_conv.hip's typed k = 1 form
    x, bank, y = m.zeros(B * CH * PIX), m.zeros(FH * FW * CH * CH), m.out(B * CH * PIX)
    return lambda d, s: lib.hs_patch_conv_plain_fwd(d, _p(x), _p(bank), CH * CH, B, CH, H, W, FH, FW, CH, 1, 0, 0, 1, _p(y), s)


def _stage_input(lib, m, bad_side):
    from hyperseg_amd._hip import StageInputC
    skip, prev, y = m.zeros(B * 2 * PIX), m.zeros(B * 2 * (H // 2) * (W // 2)), m.out(B * CH * PIX)
    si = StageInputC(skip.data_ptr(), prev.data_ptr(), B, H, W, 2, 2, H // 2, W // 2, 0, 2)        # bilinear previous level, no coordinates
    m.keep = (skip, prev, si)

    def call(d, s):
        real = d in (F32, BF16, F16)
        return lib.hs_stage_input_typed_fwd(C.byref(si), d if real or bad_side == 'prev' else F32, d if real or bad_side == 'out' else F32, _p(y), s)
    return call


def _ce_score(lib, m):
    logits, target = m.zeros(B * CLS * PIX), m.zeros(B * PIX, torch.int64)
    loss, conf, mask = m.out(B * PIX), m.out(2 * CLS * CLS), m.out(B * PIX)
    return lambda d, s: lib.hs_cross_entropy_score_fwd(d, _p(logits), _p(target), B, CLS, PIX, 255, _p(loss), CLS, 0, _p(conf), _p(mask), s)


CASES = {
    # hs_train_aux.hip
    'bn_act_train_fwd': _bn_fwd,
    'bn_act_train_fwd_two_launches': lambda lib, m: _bn_fwd(lib, m, BN_LARGE_PIX),
    'bn_act_train_bwd': _bn_bwd,
    'bn_act_train_bwd_two_launches': lambda lib, m: _bn_bwd(lib, m, BN_LARGE_PIX),
    'halo_tiles_bwd': _halo_bwd,
    'upsample_bilinear_typed_bwd': _upsample_bwd,
    'bootstrapped_ce_fwd': _bootstrapped_ce_fwd,             # cross entropy, then the selection's memset and launches
    # hs_patch_conv_bwd.hip
    'dw_tiles_fwd': _dw_tiles_fwd,
    'dw_tiles_bwd_w': _dw_tiles_bwd_w,
    'patch_conv_bn_bwd_w': _patch_conv_bn_bwd_w,
    # hs_patch_conv_train.hip (and, for the half types, hs_patch_conv.hip's launch_conv1x1_h16)
    'patch_conv_plain_fwd': _plain_fwd,
    # hs_patch_conv.hip
    'stage_input_typed_fwd_prev': lambda lib, m: _stage_input(lib, m, 'prev'),
    'stage_input_typed_fwd_out': lambda lib, m: _stage_input(lib, m, 'out'),
    # hs_validate.hip
    'cross_entropy_score_fwd': _ce_score,
}


@pytest.mark.parametrize('name', list(CASES))
def test_unknown_storage_code_is_refused_before_any_launch(name):
    from hyperseg_amd import _hip
    m = _Bufs()
    call = CASES[name](_hip.lib, m)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for code in (3, -1):
        assert call(code, stream) == BAD_ARG, (name, code)
        assert m.untouched(), f'{name}: dtype code {code} was refused but an output buffer changed'
    for code in (F32, BF16, F16):
        m.refill()
        assert call(code, stream) == 0, (name, code)
        torch.cuda.synchronize()
