// The per-pixel code of Pillow's 8-bit two-pass resize, shared by the one-geometry launch (hs_resample.hip) and the batched launch whose
// geometry and tables differ per sample (hs_resample_batch.hip): a thread owns one output column x RS_TY output rows, streams the source
// rows those rows' vertical windows cover, makes the horizontal pass of its column per source row in registers -- Pillow's uint8
// intermediate -- and adds it into the int32 accumulators of the rows whose window holds that source row.  Integer work only; what the
// two launches differ in is where the tables come from and how a table row is found, which stays with each kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "hs_ingest.h"

namespace hs {

constexpr int RS_BITS = 22;                    // Pillow's PRECISION_BITS for 8-bit images
constexpr int RS_HALF = 1 << (RS_BITS - 1);
constexpr int RS_COLS = 64;                    // output columns per wave
constexpr int RS_GROUPS = 4;                   // waves per workgroup, each with its own rows
constexpr int RS_TY = 4;                       // output rows per thread
constexpr int RS_XREG = 8;                     // horizontal taps kept in registers
constexpr int RS_MAX_DIM = 1 << 19;            // any frame or view dimension (the grid's y extent stays below 65536)

__device__ __forceinline__ int clip8(int v) { return min(max(v >> RS_BITS, 0), 255); }

// first index and tap count of table row i, clamped to a source of `size` and a table of `ks` columns
__device__ __forceinline__ void resize_bounds(const int32_t* __restrict__ bounds, int i, int size, int ks, int& first, int& n) {
    first = min(max(bounds[2 * i], 0), size - 1);
    n = max(min(min(bounds[2 * i + 1], ks), size - first), 0);
}

// Source rows [s0, s1) of one sample through the column's horizontal taps (xmin, xn, xk) into acc: `x` is the sample's first byte,
// `plane` = Hi Wi.  XREG: xn <= RS_XREG and the column's weights sit in registers.  STEP = -1: tap k reads source column xmin - k -- a
// mirrored source, whose first column the caller passes as xmin (hs_augment_ragged.hip flips the SOURCE, as the reference does).  Wi is
// used as the row pitch only: a frame inside a wider canvas passes the canvas's width and plane.
template <bool HWC, bool XREG, int STEP = 1>
__device__ __forceinline__ void resize_accumulate(const uint8_t* __restrict__ x, size_t plane, int Wi, int xmin, int xn,
                                                  const int32_t* __restrict__ xk, int s0, int s1, const int (&ymin)[RS_TY],
                                                  const int (&yn)[RS_TY], const int32_t* const (&yk)[RS_TY],
                                                  int (&acc)[RS_TY][INGEST_CHANNELS]) {
    int wx[RS_XREG];
    if constexpr (XREG) {
#pragma unroll
        for (int k = 0; k < RS_XREG; ++k) wx[k] = k < xn ? xk[k] : 0;
    }
    for (int sy = s0; sy < s1; ++sy) {
        int h[INGEST_CHANNELS] = {RS_HALF, RS_HALF, RS_HALF};
        if constexpr (HWC) {
            const uint8_t* __restrict__ p = x + ((size_t)sy * Wi + xmin) * 3;
            if constexpr (XREG) {
#pragma unroll
                for (int k = 0; k < RS_XREG; ++k) {
                    if (k < xn) {
#pragma unroll
                        for (int c = 0; c < INGEST_CHANNELS; ++c) h[c] += (int)p[3 * k * STEP + c] * wx[k];
                    }
                }
            } else {
                for (int k = 0; k < xn; ++k) {
                    const int w = xk[k];
#pragma unroll
                    for (int c = 0; c < INGEST_CHANNELS; ++c) h[c] += (int)p[3 * k * STEP + c] * w;
                }
            }
        } else {
            const uint8_t* __restrict__ p = x + (size_t)sy * Wi + xmin;
            if constexpr (XREG) {
#pragma unroll
                for (int k = 0; k < RS_XREG; ++k) {
                    if (k < xn) {
#pragma unroll
                        for (int c = 0; c < INGEST_CHANNELS; ++c) h[c] += (int)p[(long)(c * plane) + k * STEP] * wx[k];
                    }
                }
            } else {
                for (int k = 0; k < xn; ++k) {
                    const int w = xk[k];
#pragma unroll
                    for (int c = 0; c < INGEST_CHANNELS; ++c) h[c] += (int)p[(long)(c * plane) + k * STEP] * w;
                }
            }
        }
#pragma unroll
        for (int c = 0; c < INGEST_CHANNELS; ++c) h[c] = clip8(h[c]);          // Pillow's uint8 intermediate
#pragma unroll
        for (int r = 0; r < RS_TY; ++r) {
            const int k = sy - ymin[r];
            if ((unsigned)k < (unsigned)yn[r]) {
                const int w = yk[r][k];
#pragma unroll
                for (int c = 0; c < INGEST_CHANNELS; ++c) acc[r][c] += h[c] * w;
            }
        }
    }
}

// The thread's RS_TY output pixels of sample b: + 2^21, >> 22, clip8 where the pixel lies inside the resized image, the fill byte where
// not; the byte in the input's layout, or -- NORM -- its float32 entry of the table in LDS, planar.
template <bool HWC, bool NORM>
__device__ __forceinline__ void resize_store(void* __restrict__ y, const float* __restrict__ tab, size_t b, int Ho, int Wo, int x, int y0,
                                             bool col_in, const bool (&row_in)[RS_TY], const int (&acc)[RS_TY][INGEST_CHANNELS],
                                             unsigned fill) {
    const size_t oplane = (size_t)Ho * Wo;
#pragma unroll
    for (int r = 0; r < RS_TY; ++r) {
        const int yy = y0 + r;
        if (yy >= Ho) break;
        const bool inside = col_in && row_in[r];
        const size_t pix = (size_t)yy * Wo + x;
#pragma unroll
        for (int c = 0; c < INGEST_CHANNELS; ++c) {
            const unsigned v = inside ? (unsigned)clip8(acc[r][c]) : (fill >> (8 * c)) & 255u;
            if constexpr (NORM) {
                static_cast<float*>(y)[(b * INGEST_CHANNELS + c) * oplane + pix] = ingest_dequant(tab, c, v);
            } else if constexpr (HWC) {
                static_cast<uint8_t*>(y)[(b * oplane + pix) * 3 + c] = (uint8_t)v;
            } else {
                static_cast<uint8_t*>(y)[(b * INGEST_CHANNELS + c) * oplane + pix] = (uint8_t)v;
            }
        }
    }
}

}  // namespace hs
