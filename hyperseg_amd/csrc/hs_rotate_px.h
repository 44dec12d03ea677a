// The per-pixel code of Pillow's rotation, shared by the launch whose frames have one size (hs_rotate.hip) and the launch whose source
// size differs per sample and sits inside a wider canvas (hs_augment_ragged.hip): ImagingGenericTransform + bicubic_filter (a = -1) in
// float64 for the frame, operation for operation (spelt __dmul_rn / __dadd_rn; the library is built with -ffp-contract=off), and the
// 16.16 fixed-point affine path for the label.  What the launches differ in -- where (H, W) and the source's pitch come from -- stays with
// each kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "hs_ingest.h"

namespace hs {

constexpr int RT_COLS = 64;                    // output columns per wave
constexpr int RT_ROWS = 4;                     // waves per workgroup, one output row each
constexpr int RT_MAX_DIM = 8192;               // Pillow's 32-bit accumulation of the label path stays inside int32 up to here

// Pillow's BICUBIC macro: p1 + d (p2 + d (p3 + d p4))
__device__ __forceinline__ double rotate_cubic(double v1, double v2, double v3, double v4, double d) {
    const double p2 = __dadd_rn(-v1, v3);
    const double p3 = __dadd_rn(__dadd_rn(__dmul_rn(2.0, __dadd_rn(v1, -v2)), v3), -v4);
    const double p4 = __dadd_rn(__dadd_rn(__dadd_rn(-v1, v2), -v3), v4);
    return __dadd_rn(v2, __dmul_rn(d, __dadd_rn(p2, __dmul_rn(d, __dadd_rn(p3, __dmul_rn(d, p4))))));
}

// Output pixel (x, y), 0 <= x < W, 0 <= y < H, of the (H, W) image rotated by matrix m: its three bytes into out.  `src` is the image's
// first byte, `pitch` its pixels per row and `plane` its pixels per channel plane ('chw'); (W, H * W) for a frame that is not part of a
// canvas.  The inside test is written so that a NaN coordinate is "outside", and inside it every index is clamped to the (H, W) image.
template <bool HWC>
__device__ __forceinline__ void rotate_frame_pixel(const uint8_t* __restrict__ src, size_t plane, int pitch, int H, int W,
                                                   const double* __restrict__ m, int x, int y, unsigned fill,
                                                   unsigned (&out)[INGEST_CHANNELS]) {
#pragma unroll
    for (int c = 0; c < INGEST_CHANNELS; ++c) out[c] = (fill >> (8 * c)) & 255u;
    const double xi = (double)x + 0.5, yi = (double)y + 0.5;
    double xin = __dadd_rn(__dadd_rn(__dmul_rn(m[0], xi), __dmul_rn(m[1], yi)), m[2]);
    double yin = __dadd_rn(__dadd_rn(__dmul_rn(m[3], xi), __dmul_rn(m[4], yi)), m[5]);
    if (xin >= 0.0 && xin < (double)W && yin >= 0.0 && yin < (double)H) {      // false for a NaN
        xin = __dadd_rn(xin, -0.5);
        yin = __dadd_rn(yin, -0.5);
        const double fx = floor(xin), fy = floor(yin);
        const double dx = __dadd_rn(xin, -fx), dy = __dadd_rn(yin, -fy);
        const int x0 = (int)fx - 1, y0 = (int)fy - 1;                           // in [-2, W - 2] x [-2, H - 2]
        int cx[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) cx[k] = min(max(x0 + k, 0), W - 1);
        double row[4][INGEST_CHANNELS];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int ry = y0 + k;
            if (k == 0 || (ry >= 0 && ry < H)) {
                const size_t r = (size_t)min(max(ry, 0), H - 1) * pitch;
#pragma unroll
                for (int c = 0; c < INGEST_CHANNELS; ++c) {
                    double v[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        v[j] = (double)(HWC ? src[(r + cx[j]) * INGEST_CHANNELS + c] : src[c * plane + r + cx[j]]);
                    row[k][c] = rotate_cubic(v[0], v[1], v[2], v[3], dx);
                }
            } else {
#pragma unroll
                for (int c = 0; c < INGEST_CHANNELS; ++c) row[k][c] = row[k > 0 ? k - 1 : 0][c];      // the previous row's result
            }
        }
#pragma unroll
        for (int c = 0; c < INGEST_CHANNELS; ++c) {
            const double v = rotate_cubic(row[0][c], row[1][c], row[2][c], row[3][c], dy);
            out[c] = v <= 0.0 ? 0u : v >= 255.0 ? 255u : (unsigned)(int)v;      // truncation; a NaN gives 0
            out[c] = min(out[c], 255u);
        }
    }
}

// pixel (x, y) of sample b's (Ho, Wo) output: the byte in the frames' layout, or -- NORM -- its float32 entry of the table in LDS, planar
template <bool HWC, bool NORM>
__device__ __forceinline__ void rotate_store(void* __restrict__ yout, const float* __restrict__ tab, size_t b, int Ho, int Wo, int x, int y,
                                             const unsigned (&out)[INGEST_CHANNELS]) {
    const size_t oplane = (size_t)Ho * Wo;
    const size_t pix = (size_t)y * Wo + x;
#pragma unroll
    for (int c = 0; c < INGEST_CHANNELS; ++c) {
        if constexpr (NORM) {
            static_cast<float*>(yout)[(b * INGEST_CHANNELS + c) * oplane + pix] = ingest_dequant(tab, c, out[c]);
        } else if constexpr (HWC) {
            static_cast<uint8_t*>(yout)[(b * oplane + pix) * 3 + c] = (uint8_t)out[c];
        } else {
            static_cast<uint8_t*>(yout)[(b * INGEST_CHANNELS + c) * oplane + pix] = (uint8_t)out[c];
        }
    }
}

// labels: the source pixel of output (xx, yy) on Pillow's 16.16 fixed-point affine path.  The sums wrap as 32-bit words (they cannot for a
// table built from a rotation of a frame up to RT_MAX_DIM); the caller uses the index only after its range test.
__device__ __forceinline__ void rotate_label_source(const int32_t* __restrict__ a, int xx, int yy, int& xs, int& ys) {
    xs = (int)((uint32_t)a[2] + (uint32_t)yy * (uint32_t)a[1] + (uint32_t)xx * (uint32_t)a[0]) >> 16;
    ys = (int)((uint32_t)a[5] + (uint32_t)yy * (uint32_t)a[4] + (uint32_t)xx * (uint32_t)a[3]) >> 16;
}

}  // namespace hs
