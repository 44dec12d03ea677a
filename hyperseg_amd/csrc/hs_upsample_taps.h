// Tap arithmetic of the final logits resize (F.interpolate(..., 'bilinear', align_corners=False)), shared by every kernel that
// has to round identically: the logits kernels and the fused arg-max kernel (hs_patch_conv.hip) and the fused arg-max +
// confusion-matrix kernel (hs_eval.hip).  Moved here unchanged from hs_patch_conv.hip.
#pragma once
#include "hs_common.h"

namespace hs {

// Exact 2x bilinear upsample (align_corners=False): taps are {0.25, 0.75} with edge clamping.  One thread =
// 2 output rows x 4 output columns from a 3 x 4 input neighbourhood: two 16-byte stores per 12 cached loads.
// up2x_block is shared by the logits kernel and the fused argmax kernel so that both round identically.
__device__ __forceinline__ void up2x_block(const float* __restrict__ base, int Hi, int Wi, int yi, int q,
                                           float (&o0)[4], float (&o1)[4]) {
    const int xi = 2 * q;
    const int xm = xi > 0 ? xi - 1 : 0, xp = xi + 2 < Wi ? xi + 2 : Wi - 1;
    const int ym = yi > 0 ? yi - 1 : 0, yp = yi + 1 < Hi ? yi + 1 : Hi - 1;
    float in[3][4];
    const int ys[3] = {ym, yi, yp};
#pragma unroll
    for (int rr = 0; rr < 3; ++rr) {
        const float* row = base + (size_t)ys[rr] * Wi;
        in[rr][0] = row[xm]; in[rr][1] = row[xi]; in[rr][2] = row[xi + 1]; in[rr][3] = row[xp];
    }
    // horizontal pass, same operation order as ATen: l0*a + l1*b with (l0, l1) = (0.25, 0.75) / (0.75, 0.25)
    float hz[3][4];
#pragma unroll
    for (int rr = 0; rr < 3; ++rr) {
        hz[rr][0] = 0.25f * in[rr][0] + 0.75f * in[rr][1];
        hz[rr][1] = 0.75f * in[rr][1] + 0.25f * in[rr][2];
        hz[rr][2] = 0.25f * in[rr][1] + 0.75f * in[rr][2];
        hz[rr][3] = 0.75f * in[rr][2] + 0.25f * in[rr][3];
    }
    // ATen clamps the SOURCE index at 0 (lambda = 0 there): first output row/col equal the edge sample
    if (xi == 0) {
#pragma unroll
        for (int rr = 0; rr < 3; ++rr) hz[rr][0] = 1.0f * in[rr][1] + 0.0f * in[rr][2];
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        o0[c] = (yi == 0) ? (1.0f * hz[1][c] + 0.0f * hz[2][c]) : (0.25f * hz[0][c] + 0.75f * hz[1][c]);
        o1[c] = 0.75f * hz[1][c] + 0.25f * hz[2][c];
    }
}

// Bilinear resize (align_corners=False).  One thread = 4 consecutive output pixels of a row; bilinear_row4 is shared by
// the logits kernel and the fused argmax kernel.
struct Row4 { Tap ty; Tap tx[4]; };
__device__ __forceinline__ Row4 row4_taps(int yo, int q, int Hi, int Wi, int Wo, float scale_y, float scale_x) {
    Row4 t;
    t.ty = bilinear_tap(yo, scale_y, Hi);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int xo = 4 * q + i;
        t.tx[i] = bilinear_tap(xo < Wo ? xo : Wo - 1, scale_x, Wi);
    }
    return t;
}
__device__ __forceinline__ void bilinear_row4(const float* __restrict__ plane, int Wi, const Row4& t, float (&out)[4]) {
    const float* r0 = plane + (size_t)t.ty.i0 * Wi;
    const float* r1 = plane + (size_t)t.ty.i1 * Wi;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float top = t.tx[i].l0 * r0[t.tx[i].i0] + t.tx[i].l1 * r0[t.tx[i].i1];
        const float bot = t.tx[i].l0 * r1[t.tx[i].i0] + t.tx[i].l1 * r1[t.tx[i].i1];
        out[i] = t.ty.l0 * top + t.ty.l1 * bot;
    }
}

}  // namespace hs
