// Camera-size uint8 frames resized on the device with Pillow's 8-bit arithmetic (PIL.Image.resize, BILINEAR / BICUBIC: what the
// reference's torchvision Resize / RandomResize run on PIL images, hyperseg/datasets/seg_transforms.py:224-246), and labels with its
// NEAREST index tables.  The device does integer work only: the per-axis tables -- (first source index, taps) and 22-bit fixed-point
// weights, or nearest indices -- are built on the host in float64 (hyperseg_amd/utils/resample.py), so nothing here has a rounding
// that would have to be argued about.
//
// hs_frame_resize_fwd, ONE launch, the 8-bit intermediate of Pillow's horizontal pass never leaves registers:
//   * a workgroup is 4 waves; a wave owns 64 consecutive output columns x RS_TY output rows, a thread one column of them (3 channels);
//   * the thread streams the source rows its RS_TY rows' vertical windows cover (monotone in the row, so one contiguous range): per
//     source row it makes the horizontal pass of its column -- taps x 3 byte loads against its column's weights, + 2^21, >> 22, clip8:
//     Pillow's uint8 intermediate -- and adds it, times the vertical weight, into the int32 accumulators of the rows whose window holds
//     that source row.  Any ksize on either axis: the loops are over the tables' own tap counts;
//   * up to 8 horizontal taps (every scale down to 1/3 bilinear, bicubic upscaling) the column's weights sit in registers;
//   * epilogue: + 2^21, >> 22, clip8, then the byte in the input's layout, or -- with InputNorm's table in LDS -- its float32 entry in
//     planar layout.  A position of the view outside the resized image is the fill byte, through the table as well.
// Neighbouring threads read overlapping windows of the same source rows: L1 / L2 traffic, HBM sees each source byte about
// (1 + 2 support / (RS_TY scale)) times.  Bounds read from the tables are clamped to the source, so a wrong table cannot leave the frame.
// The per-pixel code (the streaming loop, the epilogue) lives in hs_resample_px.h, shared with the batched launch of hs_resample_batch.hip.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <climits>
#include "hyperseg_hip.h"
#include "hs_common.h"
#include "hs_ingest.h"
#include "hs_resample_px.h"
#include "hs_label_codec.h"

namespace hs {

struct ResizeArgs {
    const uint8_t* x; void* y; const float* table;
    const int32_t* yb; const int32_t* ykk; const int32_t* xb; const int32_t* xkk;
    int Hi, Wi, Hr, Wr, Ho, Wo, oy, ox, yks, xks, hflip;
    unsigned fill;                             // r | g << 8 | b << 16
};

template <bool HWC, bool NORM, bool XREG>
__global__ __launch_bounds__(RS_COLS * RS_GROUPS)
void frame_resize_kernel(const ResizeArgs a) {
    __shared__ float tab[NORM ? INGEST_TABLE_FLOATS : 1];
    if constexpr (NORM) {
        ingest_table_to_lds(a.table, tab, (int)threadIdx.x);
        __syncthreads();
    }
    const int x = blockIdx.x * RS_COLS + (threadIdx.x & (RS_COLS - 1));
    const int y0 = (blockIdx.y * RS_GROUPS + (threadIdx.x / RS_COLS)) * RS_TY;
    if (x >= a.Wo || y0 >= a.Ho) return;
    const size_t b = blockIdx.z;
    const int rx = a.ox + (a.hflip ? a.Wo - 1 - x : x);
    const bool col_in = rx >= 0 && rx < a.Wr;

    int ymin[RS_TY], yn[RS_TY], acc[RS_TY][INGEST_CHANNELS];
    const int32_t* yk[RS_TY];
    bool row_in[RS_TY];
    int s0 = INT_MAX, s1 = 0;
#pragma unroll
    for (int r = 0; r < RS_TY; ++r) {
        const int ry = a.oy + y0 + r;
        row_in[r] = y0 + r < a.Ho && ry >= 0 && ry < a.Hr;
        ymin[r] = 0; yn[r] = 0; yk[r] = a.ykk;
        if (row_in[r]) {
            resize_bounds(a.yb, ry, a.Hi, a.yks, ymin[r], yn[r]);
            yk[r] = a.ykk + (size_t)ry * a.yks;
            if (yn[r] > 0) { s0 = min(s0, ymin[r]); s1 = max(s1, ymin[r] + yn[r]); }
        }
#pragma unroll
        for (int c = 0; c < INGEST_CHANNELS; ++c) acc[r][c] = RS_HALF;
    }

    if (col_in && s0 < s1) {
        int xmin, xn;
        resize_bounds(a.xb, rx, a.Wi, a.xks, xmin, xn);
        const int32_t* __restrict__ xk = a.xkk + (size_t)rx * a.xks;
        const size_t plane = (size_t)a.Hi * a.Wi;
        resize_accumulate<HWC, XREG>(a.x + b * INGEST_CHANNELS * plane, plane, a.Wi, xmin, xn, xk, s0, s1, ymin, yn, yk, acc);
    }

    resize_store<HWC, NORM>(a.y, tab, b, a.Ho, a.Wo, x, y0, col_in, row_in, acc, a.fill);
}

template <bool HWC, bool NORM>
static void launch_frame_resize(const ResizeArgs& a, dim3 grid, hipStream_t s) {
    const dim3 block(RS_COLS * RS_GROUPS);
    if (a.xks <= RS_XREG) hipLaunchKernelGGL((frame_resize_kernel<HWC, NORM, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((frame_resize_kernel<HWC, NORM, false>), grid, block, 0, s, a);
}

// labels: a gather through the two nearest tables; one thread per output pixel.  CODEC (hs_label_codec.h): the source pixel is a raw
// label -- an id, or 3 colour bytes -- and is encoded on the way; the fill is stored as given (the reference pads after its dataset
// has encoded, with a class value)
template <typename TI, typename TO, int CODEC, typename... CA>
__global__ __launch_bounds__(256)
void label_resize_kernel(const TI* __restrict__ x, const int32_t* __restrict__ iy, const int32_t* __restrict__ ix, TO* __restrict__ y,
                         int Hi, int Wi, int Hr, int Wr, int Ho, int Wo, int oy, int ox, int hflip, int fill, CA... ca) {
    __shared__ uint32_t codec[codec_lds_words<CODEC>()];
    const auto c = codec_args(ca...);
    codec_stage<CODEC>(codec, c, (int)threadIdx.x);
    const long item = (long)blockIdx.x * 256 + threadIdx.x;
    if (item >= (long)Ho * Wo) return;
    const int yy = (int)(item / Wo), xx = (int)(item - (long)yy * Wo);
    const int ry = oy + yy, rx = ox + (hflip ? Wo - 1 - xx : xx);
    const size_t b = blockIdx.y;
    TO v = (TO)fill;
    if (ry >= 0 && ry < Hr && rx >= 0 && rx < Wr) {
        const int sy = min(max(iy[ry], 0), Hi - 1), sx = min(max(ix[rx], 0), Wi - 1);
        if constexpr (CODEC == CODEC_NONE) v = (TO)x[(b * Hi + sy) * (size_t)Wi + sx];
        else v = (TO)codec_gather<CODEC>(x, (b * Hi + sy) * (size_t)Wi + sx, codec, c);
    }
    y[b * (size_t)Ho * Wo + (size_t)item] = v;
}

}  // namespace hs

using namespace hs;

static bool resize_dims_ok(int32_t a, int32_t b, int32_t c, int32_t d, int32_t e, int32_t f) {
    return a <= RS_MAX_DIM && b <= RS_MAX_DIM && c <= RS_MAX_DIM && d <= RS_MAX_DIM && e <= RS_MAX_DIM && f <= RS_MAX_DIM;
}

extern "C" int hs_frame_resize_fwd(const uint8_t* x, int32_t layout, int32_t batch, int32_t Hi, int32_t Wi,
                                   const int32_t* y_bounds, const int32_t* y_kk, int32_t y_ksize, int32_t Hr,
                                   const int32_t* x_bounds, const int32_t* x_kk, int32_t x_ksize, int32_t Wr,
                                   int32_t Ho, int32_t Wo, int32_t oy, int32_t ox, int32_t hflip, uint32_t fill_rgb,
                                   const float* norm_table, void* y, void* stream) {
    if (!x || !y || !y_bounds || !y_kk || !x_bounds || !x_kk) return HS_ERR_BAD_ARG;
    if (batch <= 0 || Hi <= 0 || Wi <= 0 || Hr <= 0 || Wr <= 0 || Ho <= 0 || Wo <= 0 || y_ksize <= 0 || x_ksize <= 0) return HS_ERR_BAD_ARG;
    if (layout != HS_LAYOUT_HWC && layout != HS_LAYOUT_CHW) return HS_ERR_BAD_ARG;
    if (batch > 65535 || !resize_dims_ok(Hi, Wi, Hr, Wr, Ho, Wo)) return HS_ERR_UNSUPPORTED;
    if (oy < -RS_MAX_DIM || oy > RS_MAX_DIM || ox < -RS_MAX_DIM || ox > RS_MAX_DIM) return HS_ERR_UNSUPPORTED;
    ResizeArgs a;
    a.x = x; a.y = y; a.table = norm_table;
    a.yb = y_bounds; a.ykk = y_kk; a.xb = x_bounds; a.xkk = x_kk;
    a.Hi = Hi; a.Wi = Wi; a.Hr = Hr; a.Wr = Wr; a.Ho = Ho; a.Wo = Wo; a.oy = oy; a.ox = ox; a.yks = y_ksize; a.xks = x_ksize;
    a.hflip = hflip != 0; a.fill = fill_rgb & 0xffffffu;
    const dim3 grid((unsigned)((Wo + RS_COLS - 1) / RS_COLS), (unsigned)((Ho + RS_GROUPS * RS_TY - 1) / (RS_GROUPS * RS_TY)), (unsigned)batch);
    hipStream_t s = (hipStream_t)stream;
    const bool hwc = layout == HS_LAYOUT_HWC;
    if (norm_table) { if (hwc) launch_frame_resize<true, true>(a, grid, s); else launch_frame_resize<false, true>(a, grid, s); }
    else { if (hwc) launch_frame_resize<true, false>(a, grid, s); else launch_frame_resize<false, false>(a, grid, s); }
    return launch_status();
}

struct LabelResizeArgs {
    const void* x; const int32_t* iy; const int32_t* ix; void* y;
    int in_dtype, out_dtype, batch, Hi, Wi, Hr, Wr, Ho, Wo, oy, ox, hflip, fill;
};

static int label_resize_checks(const LabelResizeArgs& a) {
    if (!a.x || !a.y || !a.iy || !a.ix) return HS_ERR_BAD_ARG;
    if (a.batch <= 0 || a.Hi <= 0 || a.Wi <= 0 || a.Hr <= 0 || a.Wr <= 0 || a.Ho <= 0 || a.Wo <= 0) return HS_ERR_BAD_ARG;
    if ((a.in_dtype != HS_EVAL_U8 && a.in_dtype != HS_EVAL_I64) || (a.out_dtype != HS_EVAL_U8 && a.out_dtype != HS_EVAL_I64)) return HS_ERR_BAD_ARG;
    if (a.batch > 65535 || !resize_dims_ok(a.Hi, a.Wi, a.Hr, a.Wr, a.Ho, a.Wo)) return HS_ERR_UNSUPPORTED;
    if (a.oy < -RS_MAX_DIM || a.oy > RS_MAX_DIM || a.ox < -RS_MAX_DIM || a.ox > RS_MAX_DIM) return HS_ERR_UNSUPPORTED;
    if (((long)a.Ho * a.Wo + 255) / 256 > 0x7fffffffL) return HS_ERR_UNSUPPORTED;
    return HS_OK;
}

template <typename TI, typename TO, int CODEC, typename... CA>
static void launch_label_resize(const LabelResizeArgs& a, hipStream_t s, CA... ca) {
    const dim3 grid((unsigned)(((long)a.Ho * a.Wo + 255) / 256), (unsigned)a.batch), block(256);
    hipLaunchKernelGGL((label_resize_kernel<TI, TO, CODEC, CA...>), grid, block, 0, s, static_cast<const TI*>(a.x), a.iy, a.ix,
                       static_cast<TO*>(a.y), a.Hi, a.Wi, a.Hr, a.Wr, a.Ho, a.Wo, a.oy, a.ox, a.hflip, a.fill, ca...);
}

// the storage types of a checked launch; a colour image is bytes
template <int CODEC, typename... CA>
static void label_resize_typed(const LabelResizeArgs& a, hipStream_t s, CA... ca) {
    const bool u8_out = a.out_dtype == HS_EVAL_U8;
    if (CODEC == CODEC_COLORS || a.in_dtype == HS_EVAL_U8) {
        if (u8_out) launch_label_resize<uint8_t, uint8_t, CODEC>(a, s, ca...);
        else launch_label_resize<uint8_t, int64_t, CODEC>(a, s, ca...);
    } else if constexpr (CODEC != CODEC_COLORS) {
        if (u8_out) launch_label_resize<int64_t, uint8_t, CODEC>(a, s, ca...);
        else launch_label_resize<int64_t, int64_t, CODEC>(a, s, ca...);
    }
}

extern "C" int hs_label_resize_fwd(const void* x, int32_t in_dtype, int32_t batch, int32_t Hi, int32_t Wi,
                                   const int32_t* y_index, int32_t Hr, const int32_t* x_index, int32_t Wr,
                                   int32_t Ho, int32_t Wo, int32_t oy, int32_t ox, int32_t hflip, int32_t fill,
                                   void* y, int32_t out_dtype, void* stream) {
    const LabelResizeArgs a{x, y_index, x_index, y, in_dtype, out_dtype, batch, Hi, Wi, Hr, Wr, Ho, Wo, oy, ox, (int)(hflip != 0), fill};
    if (const int st = label_resize_checks(a)) return st;
    label_resize_typed<CODEC_NONE>(a, (hipStream_t)stream);
    return launch_status();
}

extern "C" int hs_label_resize_coded_fwd(const void* x, int32_t in_dtype, int32_t batch, int32_t Hi, int32_t Wi,
                                         const int32_t* y_index, int32_t Hr, const int32_t* x_index, int32_t Wr,
                                         int32_t Ho, int32_t Wo, int32_t oy, int32_t ox, int32_t hflip, int32_t fill,
                                         const int32_t* codec_words, int32_t codec_kind, int32_t n, int32_t unmatched,
                                         void* y, int32_t out_dtype, void* stream) {
    const LabelResizeArgs a{x, y_index, x_index, y, in_dtype, out_dtype, batch, Hi, Wi, Hr, Wr, Ho, Wo, oy, ox, (int)(hflip != 0), fill};
    if (const int st = label_resize_checks(a)) return st;
    if (const int st = codec_check(codec_words, codec_kind, in_dtype, n, unmatched)) return st;
    if (codec_kind == HS_CODEC_COLORS) label_resize_typed<CODEC_COLORS>(a, (hipStream_t)stream, codec_words, (int)n, (int)unmatched);
    else label_resize_typed<CODEC_TABLE>(a, (hipStream_t)stream, codec_words, (int)n, (int)unmatched);
    return launch_status();
}

