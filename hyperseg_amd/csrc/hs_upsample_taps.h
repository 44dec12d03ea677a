// Tap arithmetic of the final logits resize (F.interpolate(..., 'bilinear', align_corners=False)) and the class arg-max taken over
// it in registers, shared by every kernel that has to round and break ties identically: the logits kernels and the fused arg-max
// kernels (hs_patch_conv.hip), the arg-max + confusion-matrix kernels (hs_eval.hip) and the arg-max + overlay kernels (hs_overlay.hip).
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

// "This shape takes the exact-2x form" (up2x_block: pairs of input columns), for every entry point that chooses between the two forms.
inline bool is_exact2x(int Hi, int Wi, int Ho, int Wo) { return Ho == 2 * Hi && Wo == 2 * Wi && (Wi & 1) == 0; }

// Class arg-max of the exact-2x form, the one copy behind the masks of hs_upsample_argmax_fwd, hs_upsample_confusion_fwd and
// hs_upsample_overlay_fwd.  Four consecutive lanes (sub = 0..3) share the 2 x 4 output block (yi, q) of image `xb` and split the
// classes among them (c = sub, sub + 4, ...): with one thread per block the launch is a single wave per SIMD walking 19 dependent
// load batches; this way it is four waves per SIMD with <= 5 classes (60 loads, one batch) per trip, combined with two shuffles:
// the larger value wins, the lower class on ties -- the first maximum, as argmax(1).  On return all four lanes hold the block's
// eight class indices (idx0: upper row, idx1: lower row).
// Precondition: the call is wave-convergent (the shuffles read the quad's other lanes) -- a caller with surplus lanes lets them
// shadow a real block and decides after the call who stores.
__device__ __forceinline__ void argmax2x_block(const float* __restrict__ xb, int C, int Hi, int Wi, int yi, int q, int sub,
                                               int (&idx0)[4], int (&idx1)[4]) {
    constexpr float NEG = -3.402823466e38f;
    float best0[4] = {NEG, NEG, NEG, NEG}, best1[4] = {NEG, NEG, NEG, NEG};
#pragma unroll
    for (int i = 0; i < 4; ++i) idx0[i] = idx1[i] = sub;
    for (int c0 = sub; c0 < C; c0 += 20) {
        float o0[5][4], o1[5][4];
#pragma unroll
        for (int u = 0; u < 5; ++u) {                        // 5 classes = 60 loads in flight
            const int c = min(c0 + 4 * u, C - 1);
            up2x_block(xb + (size_t)c * Hi * Wi, Hi, Wi, yi, q, o0[u], o1[u]);
        }
#pragma unroll
        for (int u = 0; u < 5; ++u) {
            const int c = c0 + 4 * u;
            if (c < C) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    if (o0[u][i] > best0[i]) { best0[i] = o0[u][i]; idx0[i] = c; }
                    if (o1[u][i] > best1[i]) { best1[i] = o1[u][i]; idx1[i] = c; }
                }
            }
        }
    }
#pragma unroll
    for (int m = 1; m <= 2; m <<= 1) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float v0 = __shfl_xor(best0[i], m, 64), v1 = __shfl_xor(best1[i], m, 64);
            const int j0 = __shfl_xor(idx0[i], m, 64), j1 = __shfl_xor(idx1[i], m, 64);
            if (v0 > best0[i] || (v0 == best0[i] && j0 < idx0[i])) { best0[i] = v0; idx0[i] = j0; }
            if (v1 > best1[i] || (v1 == best1[i] && j1 < idx1[i])) { best1[i] = v1; idx1[i] = j1; }
        }
    }
}

// Class arg-max of the general form (any ratio, the identity included) over the four output pixels of `t`: strictly greater wins,
// so the first maximum is kept.  The same one copy behind the three entry points' masks.
__device__ __forceinline__ void argmax_row4(const float* __restrict__ xb, int C, int Hi, int Wi, const Row4& t, int (&idx)[4]) {
    float best[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) idx[i] = 0;
    bilinear_row4(xb, Wi, t, best);
#pragma unroll 6
    for (int c = 1; c < C; ++c) {
        float o[4];
        bilinear_row4(xb + (size_t)c * Hi * Wi, Wi, t, o);
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (o[i] > best[i]) { best[i] = o[i]; idx[i] = c; }
    }
}

}  // namespace hs
