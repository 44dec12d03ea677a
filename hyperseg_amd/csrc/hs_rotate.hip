// uint8 frames and their labels rotated on the device with Pillow's arithmetic (PIL.Image.rotate, expand=False, about the centre: what the
// reference's RandomRotation runs on PIL images, hyperseg/datasets/seg_transforms.py:384-426 -- BICUBIC for the frame, NEAREST for the
// label), and the ConstantPad that follows it (:181-217) as a VIEW: the output is (Ho, Wo) with the rotated image at its top-left corner
// and a pad fill right of and below it.  The transform is data: per sample six float64 coefficients (frames) or six 16.16 fixed-point
// integers (labels), built on the host (hyperseg_amd/utils/rotate.py) and read from a device table when the kernels RUN.
//
// hs_frame_rotate_fwd, ONE launch, one thread per output pixel, all three channels in it -- the source coordinates, floor, dx / dy and the
// 16 clamped addresses are computed once:
//   * Pillow's ImagingGenericTransform + bicubic_filter (a = -1) in float64, operation for operation: the output pixel's centre through
//     the matrix, (m0 xi + m1 yi) + m2; outside [0, W) x [0, H) the rotation fill; else a 4 x 4 window around floor(xin - 0.5), columns
//     clamped, four horizontal cubics and one vertical.  A window row outside the frame is not read: it repeats the previous row's
//     horizontal result, as Pillow's does.  The byte is 0 at v <= 0, 255 at v >= 255, else TRUNCATION -- no + 0.5;
//   * the horizontal results are not integers, so the order of the float64 operations is Pillow's, spelt __dmul_rn / __dadd_rn (and the
//     library is built with -ffp-contract=off);
//   * a workgroup is 4 waves, a wave 64 consecutive output columns of one row; neighbouring threads read neighbouring windows of a source
//     that sits in L1 / L2: a latency-bound gather;
//   * epilogue: the byte in the input's layout, or -- with InputNorm's table in LDS -- its float32 entry in planar layout; both fills go
//     through the table as well.
// The inside test is written so that a NaN coordinate is "outside", and inside it every index is clamped: no table can make a read leave
// the frame.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "hyperseg_hip.h"
#include "hs_common.h"
#include "hs_ingest.h"
#include "hs_rotate_px.h"

namespace hs {

struct RotateArgs {
    const uint8_t* x; void* y; const float* table; const double* m;
    int H, W, Ho, Wo;
    unsigned fill, pad_fill;                   // r | g << 8 | b << 16
};

// the per-pixel arithmetic is hs_rotate_px.h's, shared with the ragged launch of hs_augment_ragged.hip
template <bool HWC, bool NORM>
__global__ __launch_bounds__(RT_COLS * RT_ROWS)
void frame_rotate_kernel(const RotateArgs a) {
    __shared__ float tab[NORM ? INGEST_TABLE_FLOATS : 1];
    if constexpr (NORM) {
        ingest_table_to_lds(a.table, tab, (int)threadIdx.x);
        __syncthreads();
    }
    const int x = blockIdx.x * RT_COLS + (threadIdx.x & (RT_COLS - 1));
    const int y = blockIdx.y * RT_ROWS + (threadIdx.x / RT_COLS);
    if (x >= a.Wo || y >= a.Ho) return;
    const size_t b = blockIdx.z;
    const int H = a.H, W = a.W;
    unsigned out[INGEST_CHANNELS];
#pragma unroll
    for (int c = 0; c < INGEST_CHANNELS; ++c) out[c] = (a.pad_fill >> (8 * c)) & 255u;
    if (x < W && y < H) {
        const size_t plane = (size_t)H * W;
        rotate_frame_pixel<HWC>(a.x + b * INGEST_CHANNELS * plane, plane, W, H, W, a.m + 6 * b, x, y, a.fill, out);
    }
    rotate_store<HWC, NORM>(a.y, tab, b, a.Ho, a.Wo, x, y, out);
}

// labels: Pillow's 16.16 fixed-point affine path, integers only; one thread per output pixel
template <typename TI, typename TO>
__global__ __launch_bounds__(256)
void label_rotate_kernel(const TI* __restrict__ x, const int32_t* __restrict__ fixed, TO* __restrict__ y,
                         int H, int W, int Ho, int Wo, int fill, int pad_fill) {
    const long item = (long)blockIdx.x * 256 + threadIdx.x;
    if (item >= (long)Ho * Wo) return;
    const int yy = (int)(item / Wo), xx = (int)(item - (long)yy * Wo);
    const size_t b = blockIdx.y;
    TO v = (TO)pad_fill;
    if (yy < H && xx < W) {
        int xs, ys;
        rotate_label_source(fixed + 6 * b, xx, yy, xs, ys);
        v = (TO)fill;
        if (xs >= 0 && xs < W && ys >= 0 && ys < H) v = (TO)x[(b * H + ys) * (size_t)W + xs];
    }
    y[b * (size_t)Ho * Wo + (size_t)item] = v;
}

}  // namespace hs

using namespace hs;

static bool rotate_dims_ok(int32_t a, int32_t b, int32_t c, int32_t d) {
    return a <= RT_MAX_DIM && b <= RT_MAX_DIM && c <= RT_MAX_DIM && d <= RT_MAX_DIM;
}

extern "C" int hs_frame_rotate_fwd(const uint8_t* x, int32_t layout, int32_t batch, int32_t H, int32_t W, const double* matrices,
                                   int32_t Ho, int32_t Wo, uint32_t fill_rgb, uint32_t pad_fill_rgb, const float* norm_table,
                                   void* y, void* stream) {
    if (!x || !y || !matrices) return HS_ERR_BAD_ARG;
    if (batch <= 0 || H <= 0 || W <= 0 || Ho <= 0 || Wo <= 0) return HS_ERR_BAD_ARG;
    if (layout != HS_LAYOUT_HWC && layout != HS_LAYOUT_CHW) return HS_ERR_BAD_ARG;
    if (batch > 65535 || !rotate_dims_ok(H, W, Ho, Wo)) return HS_ERR_UNSUPPORTED;
    RotateArgs a;
    a.x = x; a.y = y; a.table = norm_table; a.m = matrices;
    a.H = H; a.W = W; a.Ho = Ho; a.Wo = Wo;
    a.fill = fill_rgb & 0xffffffu; a.pad_fill = pad_fill_rgb & 0xffffffu;
    const dim3 grid((unsigned)((Wo + RT_COLS - 1) / RT_COLS), (unsigned)((Ho + RT_ROWS - 1) / RT_ROWS), (unsigned)batch);
    const dim3 block(RT_COLS * RT_ROWS);
    hipStream_t s = (hipStream_t)stream;
    const bool hwc = layout == HS_LAYOUT_HWC;
    if (norm_table) {
        if (hwc) hipLaunchKernelGGL((frame_rotate_kernel<true, true>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((frame_rotate_kernel<false, true>), grid, block, 0, s, a);
    } else {
        if (hwc) hipLaunchKernelGGL((frame_rotate_kernel<true, false>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((frame_rotate_kernel<false, false>), grid, block, 0, s, a);
    }
    return launch_status();
}

extern "C" int hs_label_rotate_fwd(const void* x, int32_t in_dtype, int32_t batch, int32_t H, int32_t W, const int32_t* fixed,
                                   int32_t Ho, int32_t Wo, int32_t fill, int32_t pad_fill, void* y, int32_t out_dtype, void* stream) {
    if (!x || !y || !fixed) return HS_ERR_BAD_ARG;
    if (batch <= 0 || H <= 0 || W <= 0 || Ho <= 0 || Wo <= 0) return HS_ERR_BAD_ARG;
    if ((in_dtype != HS_EVAL_U8 && in_dtype != HS_EVAL_I64) || (out_dtype != HS_EVAL_U8 && out_dtype != HS_EVAL_I64)) return HS_ERR_BAD_ARG;
    if (batch > 65535 || !rotate_dims_ok(H, W, Ho, Wo)) return HS_ERR_UNSUPPORTED;
    const long blocks = ((long)Ho * Wo + 255) / 256;
    const dim3 grid((unsigned)blocks, (unsigned)batch), block(256);
    hipStream_t s = (hipStream_t)stream;
#define HS_LABEL_LAUNCH(TI, TO) hipLaunchKernelGGL((label_rotate_kernel<TI, TO>), grid, block, 0, s, static_cast<const TI*>(x), fixed, \
                                                   static_cast<TO*>(y), H, W, Ho, Wo, fill, pad_fill)
    if (in_dtype == HS_EVAL_U8 && out_dtype == HS_EVAL_U8) HS_LABEL_LAUNCH(uint8_t, uint8_t);
    else if (in_dtype == HS_EVAL_U8) HS_LABEL_LAUNCH(uint8_t, int64_t);
    else if (out_dtype == HS_EVAL_U8) HS_LABEL_LAUNCH(int64_t, uint8_t);
    else HS_LABEL_LAUNCH(int64_t, int64_t);
#undef HS_LABEL_LAUNCH
    return launch_status();
}
