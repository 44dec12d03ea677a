"""Plain-torch stand-ins of the HIP entry points that utils/inference.py calls, by their documented semantics, for walking the prepared
encoder and context head on CPU tensors (the product path refuses them).  ``install(monkeypatch)`` swaps them into
``hyperseg_amd.functional`` and returns the ``used`` counters of the split-GEMM family.  The split stand-ins rebuild W from the REAL
host-side weight preparation (row scaling, f16 pieces, fragment order), so both the wiring and the preparation are exercised.  What the
stand-ins cannot reach: the routes guarded by ``y.is_cuda`` (gemm_split_se), stem_dw and the squeeze-excite tail."""
import torch
import torch.nn.functional as F


def act_of(t, act):
    return t * torch.sigmoid(t) if act == 3 else (torch.relu(t) if act == 1 else (t.clamp(0, 6) if act == 2 else t))


def dw(x, weight, stride, pad_top, pad_left, out_size, scale=None, shift=None, act=0, pool=False, in_scale=None,
       in_shift=None, se=None):                          # se: the stand-in leaves the gate to se_gate below (gated = False)
    if in_scale is not None:
        x = act_of(x * in_scale.view(1, -1, 1, 1) + in_shift.view(1, -1, 1, 1), 3)
    k = weight.shape[-1]
    ho, wo = out_size
    pb, pr = (ho - 1) * stride + k - x.shape[2] - pad_top, (wo - 1) * stride + k - x.shape[3] - pad_left
    y = F.conv2d(F.pad(x, (pad_left, pr, pad_top, pb)), weight, stride=stride, groups=x.shape[1])
    y = act_of(y * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1), act)
    return (y, y.sum((2, 3)).view(-1, 1)) + ((False,) if se is not None else ())


def se_gate(partial, batch, hw, w_reduce, b_reduce, w_expand_t, b_expand, w_proj=None, out_scale=None):
    pooled = partial.sum(1).view(batch, -1) / hw
    z = act_of(pooled @ w_reduce.flatten(1).t() + b_reduce, 3)
    gate = torch.sigmoid(z @ w_expand_t + b_expand)
    if w_proj is None:
        return gate
    ws = w_proj.flatten(1)[None] * gate[:, None, :]
    if out_scale is not None:
        ws = ws * out_scale[None, :, None]
    return ws[..., None, None]


def pointwise(x, weight, gate=None, scale=None, shift=None, act=0, residual=None):
    if gate is not None:
        x = x * gate[:, :, None, None]
    y = act_of(F.conv2d(x, weight) * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1), act)
    return y if residual is None else y + residual


def affine(x, scale, shift, act=0, residual=None):
    y = x if scale is None else x * scale.view(1, -1, 1, 1)
    y = act_of(y + shift.view(1, -1, 1, 1), act)
    x.copy_(y if residual is None else y + residual)
    return x


def expand_dw(x, w_expand, scale0, shift0, w_dw, stride, pad_top, pad_left, out_size, scale1, shift1, pool=True, se=None):
    hmid = pointwise(x, w_expand.view(w_expand.shape[0], -1, 1, 1), None, scale0, shift0, 3)
    return dw(hmid, w_dw, stride, pad_top, pad_left, out_size, scale1, shift1, act=3, pool=True, se=se)


def weight_of(sw):
    rt = sw.frag.shape[0]
    back = sw.frag.permute(2, 0, 4, 1, 3, 5).reshape(2, 16 * rt, sw.kp).float()        # [piece][row][k]
    return ((back[0] + back[1]) * sw.inv[:, None])[:sw.c_out, :sw.c_in]


def install(monkeypatch):
    """Swap the stand-ins into hyperseg_amd.functional; returns the counters the split-GEMM stand-ins keep."""
    from hyperseg_amd import functional as HF
    used = {'n': 0, 'gated': 0, 'accumulated': 0}

    def gemm_split(sw, x, gate=None, shift=None, act=0, residual=None, out=None):
        w = weight_of(sw)
        y = F.conv2d(x if gate is None else x * gate[:, :, None, None], w[:, :, None, None])
        if shift is not None:
            y = y + shift.view(1, -1, 1, 1)
        y = act_of(y, act)
        if residual is not None:
            y = y + residual
        used['n'] += 1
        used['gated'] += gate is not None
        used['accumulated'] += residual is not None and residual is out
        if out is None:
            return y
        assert out.shape == y.shape
        return out.copy_(y)

    def gemm_split_conv2x2(sw, x, shift=None, act=0, out=None, pool_partial=None):           # K = 4 Cin in the conv weight's flatten order
        y = F.conv2d(x, weight_of(sw).reshape(sw.c_out, x.shape[1], 2, 2), stride=2)
        y = act_of(y if shift is None else y + shift.view(1, -1, 1, 1), act)
        used['conv2x2'] = used.get('conv2x2', 0) + 1
        if pool_partial is not None:                                                         # sums over blocks of 16 pixels
            flat = y.flatten(2)
            flat = F.pad(flat, (0, pool_partial.shape[2] * 16 - flat.shape[2]))
            pool_partial.copy_(flat.view(*pool_partial.shape, 16).sum(-1))
        return y

    def gemm_split_up2(sw, x, shift=None, act=0, out=None):
        y = F.conv2d(x, weight_of(sw)[:, :, None, None])
        y = act_of(y if shift is None else y + shift.view(1, -1, 1, 1), act)
        used['up2'] = used.get('up2', 0) + 1
        return out.copy_(F.interpolate(y, scale_factor=2, mode='nearest'))

    def pooled_shift(pool_partial, pixels, wb, shift):
        used['pooled_shift'] = used.get('pooled_shift', 0) + 1
        return shift + wb @ (pool_partial[0].sum(1) / pixels)

    monkeypatch.setattr(HF, 'gemm_split', gemm_split)
    monkeypatch.setattr(HF, 'gemm_split_conv2x2', gemm_split_conv2x2)
    monkeypatch.setattr(HF, 'gemm_split_up2', gemm_split_up2)
    monkeypatch.setattr(HF, 'pooled_shift', pooled_shift)
    monkeypatch.setattr(HF, 'mbconv_expand_dw', expand_dw)
    monkeypatch.setattr(HF, 'depthwise_conv_bn_act', dw)
    monkeypatch.setattr(HF, 'se_gate', se_gate)
    monkeypatch.setattr(HF, 'pointwise_conv', pointwise)
    monkeypatch.setattr(HF, 'affine_act_', affine)
    return used
