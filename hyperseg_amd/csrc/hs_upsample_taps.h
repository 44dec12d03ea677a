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
// (hs_validate.hip keeps a copy that also hands out the maxima, argmax2x_block_best: an edit here is made there too.)
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
// (hs_validate.hip keeps a copy that also hands out the maxima, argmax_row4_best: an edit here is made there too.)
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

// ------------------------------------------------------------------------------------------
// Two resizes composed in registers (hs_upsample2_confusion_fwd): x (Hi, Wi) -> mid (Hm, Wm) -> label (Ho, Wo), the class score of a
// label pixel being exactly what hs_upsample_bilinear_fwd(hs_upsample_bilinear_fwd(x -> mid) -> label) stores.  Both forms of that
// entry are, per axis, l0 * v[i0] + l1 * v[i1] taken horizontally first and vertically second; the second stage's indices are
// clamped in MID space (ATen's edge rule applied to the mid tensor), never in x's.

// One axis of up2x_block as a Tap over `in_size` samples: odd outputs (0.75, 0.25) on (i, i + 1), even ones (0.25, 0.75) on (i - 1, i),
// output 0 the edge sample itself (1.0, 0.0), the upper index clamped.
__device__ __forceinline__ Tap up2x_tap(int dst, int in_size) {
    const int i = dst >> 1, ip = i + 1 < in_size ? i + 1 : in_size - 1;
    Tap t;
    if (dst & 1)    { t.i0 = i;     t.i1 = ip; t.l0 = 0.75f; t.l1 = 0.25f; }
    else if (i > 0) { t.i0 = i - 1; t.i1 = i;  t.l0 = 0.25f; t.l1 = 0.75f; }
    else            { t.i0 = 0;     t.i1 = ip; t.l0 = 1.0f;  t.l1 = 0.0f; }
    return t;
}
// The tap of one resize stage: the exact-2x form's where hs_upsample_bilinear_fwd takes that form (is_exact2x), bilinear_row4's otherwise.
__device__ __forceinline__ Tap stage_tap(int dst, bool exact2x, float scale, int in_size) {
    return exact2x ? up2x_tap(dst, in_size) : bilinear_tap(dst, scale, in_size);
}
// The value either form stores for the output pixel with taps (ty, tx) of `plane`: the operation order of up2x_block and bilinear_row4.
__device__ __forceinline__ float tap_value(const float* __restrict__ plane, int Wi, const Tap& ty, const Tap& tx) {
    const float* r0 = plane + (size_t)ty.i0 * Wi;
    const float* r1 = plane + (size_t)ty.i1 * Wi;
    const float top = tx.l0 * r0[tx.i0] + tx.l1 * r0[tx.i1];
    const float bot = tx.l0 * r1[tx.i0] + tx.l1 * r1[tx.i1];
    return ty.l0 * top + ty.l1 * bot;
}

// General composition, any first and any second stage.  One thread = 4 consecutive label pixels of a row, as Row4: the label row's
// two mid rows (ty2) and each pixel's two mid columns (tx2), and for each of those mid rows / columns its taps in x (ty1 / tx1).
struct Stages2 { int Hi, Wi, Hm, Wm, Ho, Wo; int exact1, exact2; float sy1, sx1, sy2, sx2; };
// (host) each stage in the form hs_upsample_bilinear_fwd takes for it
inline Stages2 stages2(int Hi, int Wi, int Hm, int Wm, int Ho, int Wo) {
    return {Hi, Wi, Hm, Wm, Ho, Wo, is_exact2x(Hi, Wi, Hm, Wm), is_exact2x(Hm, Wm, Ho, Wo),
            (float)Hi / (float)Hm, (float)Wi / (float)Wm, (float)Hm / (float)Ho, (float)Wm / (float)Wo};
}
struct Row4x2 { Tap ty2; Tap ty1[2]; Tap tx2[4]; Tap tx1[4][2]; };
__device__ __forceinline__ Row4x2 row4x2_taps(int yo, int q, const Stages2& s) {
    Row4x2 t;
    t.ty2 = stage_tap(yo, s.exact2 != 0, s.sy2, s.Hm);
    t.ty1[0] = stage_tap(t.ty2.i0, s.exact1 != 0, s.sy1, s.Hi);
    t.ty1[1] = stage_tap(t.ty2.i1, s.exact1 != 0, s.sy1, s.Hi);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int xo = 4 * q + i;
        t.tx2[i] = stage_tap(xo < s.Wo ? xo : s.Wo - 1, s.exact2 != 0, s.sx2, s.Wm);
        t.tx1[i][0] = stage_tap(t.tx2[i].i0, s.exact1 != 0, s.sx1, s.Wi);
        t.tx1[i][1] = stage_tap(t.tx2[i].i1, s.exact1 != 0, s.sx1, s.Wi);
    }
    return t;
}
__device__ __forceinline__ void bilinear2_row4(const float* __restrict__ plane, int Wi, const Row4x2& t, float (&out)[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float m00 = tap_value(plane, Wi, t.ty1[0], t.tx1[i][0]), m01 = tap_value(plane, Wi, t.ty1[0], t.tx1[i][1]);
        const float m10 = tap_value(plane, Wi, t.ty1[1], t.tx1[i][0]), m11 = tap_value(plane, Wi, t.ty1[1], t.tx1[i][1]);
        const float top = t.tx2[i].l0 * m00 + t.tx2[i].l1 * m01;
        const float bot = t.tx2[i].l0 * m10 + t.tx2[i].l1 * m11;
        out[i] = t.ty2.l0 * top + t.ty2.l1 * bot;
    }
}
// Pixel i of bilinear2_row4 alone, by the same operations (hs_validate.hip's second pass takes the four pixels two at a time).
__device__ __forceinline__ float bilinear2_at(const float* __restrict__ plane, int Wi, const Row4x2& t, int i) {
    const float m00 = tap_value(plane, Wi, t.ty1[0], t.tx1[i][0]), m01 = tap_value(plane, Wi, t.ty1[0], t.tx1[i][1]);
    const float m10 = tap_value(plane, Wi, t.ty1[1], t.tx1[i][0]), m11 = tap_value(plane, Wi, t.ty1[1], t.tx1[i][1]);
    const float top = t.tx2[i].l0 * m00 + t.tx2[i].l1 * m01;
    const float bot = t.tx2[i].l0 * m10 + t.tx2[i].l1 * m11;
    return t.ty2.l0 * top + t.ty2.l1 * bot;
}
// argmax_row4 over the composition: strictly greater wins, the first maximum is kept.
__device__ __forceinline__ void argmax2_row4(const float* __restrict__ xb, int C, int Hi, int Wi, const Row4x2& t, int (&idx)[4]) {
    float best[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) idx[i] = 0;
    bilinear2_row4(xb, Wi, t, best);
#pragma unroll 1
    for (int c = 1; c < C; ++c) {
        float o[4];
        bilinear2_row4(xb + (size_t)c * Hi * Wi, Wi, t, o);
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (o[i] > best[i]) { best[i] = o[i]; idx[i] = c; }
    }
}

// Both stages exact 2x: the 3 x 4 neighbourhood of x that up2x_block loads for block (yi, q) determines the 4 x 6 mid values of rows
// 2 yi - 1 .. 2 yi + 2 and columns 4 q - 1 .. 4 q + 4 (clamped in mid space), and those the 4 x 8 label block at (4 yi, 8 q).
__device__ __forceinline__ void load2x_block(const float* __restrict__ base, int Hi, int Wi, int yi, int q, float (&in)[3][4]) {
    const int xi = 2 * q;
    const int xm = xi > 0 ? xi - 1 : 0, xp = xi + 2 < Wi ? xi + 2 : Wi - 1;
    const int ym = yi > 0 ? yi - 1 : 0, yp = yi + 1 < Hi ? yi + 1 : Hi - 1;
    const int ys[3] = {ym, yi, yp};
#pragma unroll
    for (int rr = 0; rr < 3; ++rr) {
        const float* row = base + (size_t)ys[rr] * Wi;
        in[rr][0] = row[xm]; in[rr][1] = row[xi]; in[rr][2] = row[xi + 1]; in[rr][3] = row[xp];
    }
}
// One axis of the second stage: NOUT consecutive outputs, the first of them even, from the NOUT / 2 + 2 mid samples m[] that start one
// before the first output's own (m[1]).  `lo`: m[1] is the axis' first sample (output 0 is the edge sample itself, m[0] is not read);
// `hi`: the last m[] lies past the axis' end (the one before it stands for it: the upper index clamped in mid space).
// Eight outputs along a row (six mid columns), four along a column (four mid rows).
template <int NOUT>
__device__ __forceinline__ void up2x_line(const float (&m)[NOUT / 2 + 2], bool lo, bool hi, float (&o)[NOUT]) {
    constexpr int L = NOUT / 2 + 2;
    o[0] = lo ? (1.0f * m[1] + 0.0f * m[2]) : (0.25f * m[0] + 0.75f * m[1]);
#pragma unroll
    for (int k = 1; k < NOUT - 1; ++k) {
        const int i = 1 + (k >> 1);                              // mid sample of output k: odd k -> (i, i + 1), even k -> (i - 1, i)
        o[k] = (k & 1) ? (0.75f * m[i] + 0.25f * m[i + 1]) : (0.25f * m[i - 1] + 0.75f * m[i]);
    }
    o[NOUT - 1] = 0.75f * m[L - 2] + 0.25f * (hi ? m[L - 2] : m[L - 1]);
}
__device__ __forceinline__ void up2x2x_block(const float (&in)[3][4], bool top, bool bottom, bool left, bool right, float (&o)[4][8]) {
    // first stage, horizontal: mid columns 4 q - 1 .. 4 q + 4 of the three x rows (up2x_block's hz, plus one column on either side)
    float hz[3][6];
#pragma unroll
    for (int rr = 0; rr < 3; ++rr) {
        hz[rr][0] = 0.75f * in[rr][0] + 0.25f * in[rr][1];
        hz[rr][1] = left ? (1.0f * in[rr][1] + 0.0f * in[rr][2]) : (0.25f * in[rr][0] + 0.75f * in[rr][1]);
        hz[rr][2] = 0.75f * in[rr][1] + 0.25f * in[rr][2];
        hz[rr][3] = 0.25f * in[rr][1] + 0.75f * in[rr][2];
        hz[rr][4] = 0.75f * in[rr][2] + 0.25f * in[rr][3];
        hz[rr][5] = 0.25f * in[rr][2] + 0.75f * in[rr][3];
    }
    // first stage, vertical: mid rows 2 yi - 1 .. 2 yi + 2; second stage, horizontal, on each of them
    float h2[8][4];                                              // [label column][mid row]
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        float mid[6], line[8];
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            mid[c] = r == 0 ? (0.75f * hz[0][c] + 0.25f * hz[1][c])
                   : r == 1 ? (top ? (1.0f * hz[1][c] + 0.0f * hz[2][c]) : (0.25f * hz[0][c] + 0.75f * hz[1][c]))
                   : r == 2 ? (0.75f * hz[1][c] + 0.25f * hz[2][c])
                            : (0.25f * hz[1][c] + 0.75f * hz[2][c]);
        }
        up2x_line<8>(mid, left, right, line);
#pragma unroll
        for (int k = 0; k < 8; ++k) h2[k][r] = line[k];
    }
    // second stage, vertical
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        float col[4];
        up2x_line<4>(h2[k], top, bottom, col);
#pragma unroll
        for (int r = 0; r < 4; ++r) o[r][k] = col[r];
    }
}

// Class arg-max of the composed exact-2x form: argmax2x_block's split -- four consecutive lanes share x block (yi, q), classes
// c = sub, sub + 4, ..., five of them (60 loads) in flight per trip -- over the 4 x 8 label block, combined with the same two shuffles
// (the larger value wins, the lower class on ties).  On return all four lanes hold the block's 32 class indices, idx[label row][column].
// Precondition: wave-convergent, as argmax2x_block.
__device__ __forceinline__ void argmax2x2x_block(const float* __restrict__ xb, int C, int Hi, int Wi, int yi, int q, int sub,
                                                 int (&idx)[4][8]) {
    constexpr float NEG = -3.402823466e38f;
    const bool top = yi == 0, bottom = yi == Hi - 1, left = q == 0, right = 2 * q + 2 >= Wi;
    float best[4][8];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int k = 0; k < 8; ++k) { best[r][k] = NEG; idx[r][k] = sub; }
    for (int c0 = sub; c0 < C; c0 += 20) {
        float in[5][3][4];
#pragma unroll
        for (int u = 0; u < 5; ++u) {
            const int c = min(c0 + 4 * u, C - 1);
            load2x_block(xb + (size_t)c * Hi * Wi, Hi, Wi, yi, q, in[u]);
        }
#pragma unroll
        for (int u = 0; u < 5; ++u) {
            const int c = c0 + 4 * u;
            if (c < C) {
                float o[4][8];
                up2x2x_block(in[u], top, bottom, left, right, o);
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int k = 0; k < 8; ++k)
                        if (o[r][k] > best[r][k]) { best[r][k] = o[r][k]; idx[r][k] = c; }
            }
        }
    }
#pragma unroll
    for (int m = 1; m <= 2; m <<= 1) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const float v = __shfl_xor(best[r][k], m, 64);
                const int j = __shfl_xor(idx[r][k], m, 64);
                if (v > best[r][k] || (v == best[r][k] && j < idx[r][k])) { best[r][k] = v; idx[r][k] = j; }
            }
    }
}

}  // namespace hs
