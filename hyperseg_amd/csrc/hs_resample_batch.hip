// The train chain's resize for a whole batch, every sample with a geometry of its own (RandomResize draws a continuous scale, so
// nearly every sample has a new (in, out) pair on both axes): the tables of hs_resample.hip built ON THE DEVICE, and the two resize
// kernels reading them per sample.  Three launches per batch, nothing built or kept on the host, every per-sample parameter in one
// small device tensor that is read when the kernels RUN -- a captured graph replays with what the caller last copied into it.
//
//   params int32 (B, 6) = Hr, Wr, oy, ox, hflip, reserved: the resized size, the signed offset of the (Ho, Wo) window in the resized
//   image, the flip of the window.  Window position j of an axis is resized index r = o + j.
//
// hs_resize_tables_fwd, ONE launch, the tables of the WINDOW only (O(crop), not O(resized image)), in a caller-owned workspace,
// M = max(Ho, Wo) rows per (sample, axis), axis 0 = y:
//   * bounds (B, 2, M, 2) and kk (B, 2, M, ks_max), one thread per (sample, axis, j): utils/resample.py::resample_coeffs restated in
//     its operation order (hs_resample_tables.h, shared with the ragged launch of hs_augment_ragged.hip), so the integers are the host's;
//   * nearest (B, 2, M): Pillow's table is the ACCUMULATION xo = 0.5 a; idx = (int)xo; xo += a, not a closed form, so it is serial
//     from index 0 to the window's end: one lane per (sample, axis), in a workgroup of its own in the same launch, walks the chain and
//     stores only the window, clamped to in - 1;
//   * status (B,): 0, or a sum of the RT_* codes below.  Such a sample's tables are all-empty and the consumers write fill.
//   Rows with r outside [0, size_r), and rows j past the axis's extent, are (0, 0), zeros and 0.
// hs_frame_resize_batch_fwd / hs_label_resize_batch_fwd: hs_frame_resize_fwd / hs_label_resize_fwd with blockIdx.z / blockIdx.y's
// geometry from params and its tables from the workspace, indexed by window position; the per-pixel code is hs_resample_px.h's.  The
// register-resident-taps path is a wave-uniform run-time choice (the tap count differs per sample and per column).
// Safety: tap counts are clamped to ks_max and first indices to the source, table rows are addressed by window position only, resized
// sizes above 2^19 are declined by status (which also bounds the serial chain): no parameter value can make an access leave the
// workspace or the frame.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <climits>
#include "hyperseg_hip.h"
#include "hs_common.h"
#include "hs_ingest.h"
#include "hs_resample_px.h"
#include "hs_resample_tables.h"
#include "hs_label_codec.h"

namespace hs {

struct AxisGeometry { int in, out, o, extent; };

__device__ __forceinline__ AxisGeometry axis_geometry(const int32_t* __restrict__ p, int axis, int Hi, int Wi, int Ho, int Wo) {
    AxisGeometry g;
    g.in = axis ? Wi : Hi; g.out = p[axis]; g.o = p[2 + axis]; g.extent = axis ? Wo : Ho;
    return g;
}

// HS_RESIZE_STATUS_* of a sample; 0 = its tables are built
__device__ __forceinline__ int sample_status(const int32_t* __restrict__ p, int Hi, int Wi, double filter_support, int ks_max) {
    const int Hr = p[0], Wr = p[1];
    int st = 0;
    if (Hr < 1) st |= HS_RESIZE_STATUS_HR;
    if (Wr < 1) st |= HS_RESIZE_STATUS_WR;
    if (Hr > RS_MAX_DIM || Wr > RS_MAX_DIM) st |= HS_RESIZE_STATUS_SIZE;
    if (st) return st;
    if (Hr != Hi && axis_scale(Hi, Hr, filter_support).ksize > ks_max) st |= HS_RESIZE_STATUS_Y_TAPS;
    if (Wr != Wi && axis_scale(Wi, Wr, filter_support).ksize > ks_max) st |= HS_RESIZE_STATUS_X_TAPS;
    return st;
}

template <bool BICUBIC>
__global__ __launch_bounds__(RT_THREADS)
void resize_tables_kernel(const int32_t* __restrict__ params, int Hi, int Wi, int Ho, int Wo, int M, int ks_max,
                          int32_t* __restrict__ bounds, int32_t* __restrict__ kk, int32_t* __restrict__ nearest,
                          int32_t* __restrict__ status) {
    const int axis = blockIdx.y;
    const size_t b = blockIdx.z;
    const int32_t* __restrict__ p = params + 6 * b;
    constexpr double filter_support = BICUBIC ? 2.0 : 1.0;
    const int st = sample_status(p, Hi, Wi, filter_support, ks_max);
    const AxisGeometry g = axis_geometry(p, axis, Hi, Wi, Ho, Wo);
    const size_t row0 = (b * 2 + axis) * (size_t)M;

    if (blockIdx.x == gridDim.x - 1) {         // the workgroup of the serial chain: one lane
        if (threadIdx.x != 0) return;
        if (axis == 0) status[b] = st;
        int32_t* __restrict__ idx = nearest + row0;
        // the window's rows inside the resized axis are j in [j0, j1)
        const long lo = -(long)g.o, hi = (long)g.out - g.o;
        const int j0 = st ? 0 : (int)min(max(lo, 0L), (long)g.extent), j1 = st ? 0 : (int)min(max(hi, 0L), (long)g.extent);
        for (int j = 0; j < j0; ++j) idx[j] = 0;
        if (j1 > j0) {
            const double a = __ddiv_rn((double)g.in, (double)g.out);
            double xo = __dmul_rn(0.5, a);
            const int first = g.o + j0;        // >= 0; = 0 when the window starts before the image
            for (int r = 0; r < first; ++r) xo = __dadd_rn(xo, a);
            for (int j = j0; j < j1; ++j) {
                idx[j] = min(max((int)xo, 0), g.in - 1);
                xo = __dadd_rn(xo, a);
            }
        }
        for (int j = max(j1, j0); j < M; ++j) idx[j] = 0;
        return;
    }

    const int j = blockIdx.x * RT_THREADS + threadIdx.x;
    if (j >= M) return;
    int32_t* __restrict__ bd = bounds + (row0 + j) * 2;
    int32_t* __restrict__ k_row = kk + (row0 + j) * (size_t)ks_max;
    const long r = (long)g.o + j;
    int xmin = 0, n = 0;
    if (st == 0 && j < g.extent && r >= 0 && r < g.out) {
        resize_table_row<BICUBIC>(g.in, g.out, (int)r, ks_max, k_row, xmin, n);
    }
    bd[0] = xmin; bd[1] = n;
    for (int k = n; k < ks_max; ++k) k_row[k] = 0;
}

struct BatchResizeArgs {
    const uint8_t* x; void* y; const float* table;
    const int32_t* params; const int32_t* bounds; const int32_t* kk; const int32_t* status;
    int Hi, Wi, Ho, Wo, M, ks;
    unsigned fill;                             // r | g << 8 | b << 16
};

template <bool HWC, bool NORM>
__global__ __launch_bounds__(RS_COLS * RS_GROUPS)
void frame_resize_batch_kernel(const BatchResizeArgs a) {
    __shared__ float tab[NORM ? INGEST_TABLE_FLOATS : 1];
    if constexpr (NORM) {
        ingest_table_to_lds(a.table, tab, (int)threadIdx.x);
        __syncthreads();
    }
    const int x = blockIdx.x * RS_COLS + (threadIdx.x & (RS_COLS - 1));
    const int y0 = (blockIdx.y * RS_GROUPS + (threadIdx.x / RS_COLS)) * RS_TY;
    if (x >= a.Wo || y0 >= a.Ho) return;
    const size_t b = blockIdx.z;
    const int32_t* __restrict__ p = a.params + 6 * b;
    const bool ok = a.status[b] == 0;          // a declined sample is fill everywhere
    const int Hr = ok ? p[0] : 0, Wr = ok ? p[1] : 0, oy = p[2], ox = p[3];
    const int jx = p[4] ? a.Wo - 1 - x : x;    // the column's window position
    const long rx = (long)ox + jx;
    const bool col_in = rx >= 0 && rx < Wr;
    const int32_t* __restrict__ yb = a.bounds + (b * 2 + 0) * (size_t)a.M * 2;
    const int32_t* __restrict__ xb = a.bounds + (b * 2 + 1) * (size_t)a.M * 2;
    const int32_t* __restrict__ ykk = a.kk + (b * 2 + 0) * (size_t)a.M * a.ks;
    const int32_t* __restrict__ xkk = a.kk + (b * 2 + 1) * (size_t)a.M * a.ks;

    int ymin[RS_TY], yn[RS_TY], acc[RS_TY][INGEST_CHANNELS];
    const int32_t* yk[RS_TY];
    bool row_in[RS_TY];
    int s0 = INT_MAX, s1 = 0;
#pragma unroll
    for (int r = 0; r < RS_TY; ++r) {
        const int jy = y0 + r;
        const long ry = (long)oy + jy;
        row_in[r] = jy < a.Ho && ry >= 0 && ry < Hr;
        ymin[r] = 0; yn[r] = 0; yk[r] = ykk;
        if (row_in[r]) {
            resize_bounds(yb, jy, a.Hi, a.ks, ymin[r], yn[r]);
            yk[r] = ykk + (size_t)jy * a.ks;
            if (yn[r] > 0) { s0 = min(s0, ymin[r]); s1 = max(s1, ymin[r] + yn[r]); }
        }
#pragma unroll
        for (int c = 0; c < INGEST_CHANNELS; ++c) acc[r][c] = RS_HALF;
    }

    if (col_in && s0 < s1) {
        int xmin, xn;
        resize_bounds(xb, jx, a.Wi, a.ks, xmin, xn);
        const int32_t* __restrict__ xk = xkk + (size_t)jx * a.ks;
        const size_t plane = (size_t)a.Hi * a.Wi;
        const uint8_t* __restrict__ src = a.x + b * INGEST_CHANNELS * plane;
        if (__all(xn <= RS_XREG)) resize_accumulate<HWC, true>(src, plane, a.Wi, xmin, xn, xk, s0, s1, ymin, yn, yk, acc);
        else resize_accumulate<HWC, false>(src, plane, a.Wi, xmin, xn, xk, s0, s1, ymin, yn, yk, acc);
    }

    resize_store<HWC, NORM>(a.y, tab, b, a.Ho, a.Wo, x, y0, col_in, row_in, acc, a.fill);
}

// labels: a gather through the sample's two nearest tables; one thread per output pixel.  CODEC as in hs_resample.hip's label kernel: the
// source pixel is encoded, the fill is stored as given
template <typename TI, typename TO, int CODEC, typename... CA>
__global__ __launch_bounds__(256)
void label_resize_batch_kernel(const TI* __restrict__ x, const int32_t* __restrict__ params, const int32_t* __restrict__ nearest,
                               const int32_t* __restrict__ status, TO* __restrict__ y, int Hi, int Wi, int Ho, int Wo, int M, int fill,
                               CA... ca) {
    __shared__ uint32_t codec[codec_lds_words<CODEC>()];
    const auto c = codec_args(ca...);
    codec_stage<CODEC>(codec, c, (int)threadIdx.x);
    const long item = (long)blockIdx.x * 256 + threadIdx.x;
    if (item >= (long)Ho * Wo) return;
    const size_t b = blockIdx.y;
    const int32_t* __restrict__ p = params + 6 * b;
    const bool ok = status[b] == 0;
    const int Hr = ok ? p[0] : 0, Wr = ok ? p[1] : 0;
    const int jy = (int)(item / Wo), xx = (int)(item - (long)jy * Wo);
    const int jx = p[4] ? Wo - 1 - xx : xx;
    const long ry = (long)p[2] + jy, rx = (long)p[3] + jx;
    TO v = (TO)fill;
    if (ry >= 0 && ry < Hr && rx >= 0 && rx < Wr) {
        const int32_t* __restrict__ iy = nearest + (b * 2 + 0) * (size_t)M;
        const int32_t* __restrict__ ix = nearest + (b * 2 + 1) * (size_t)M;
        const int sy = min(max(iy[jy], 0), Hi - 1), sx = min(max(ix[jx], 0), Wi - 1);
        if constexpr (CODEC == CODEC_NONE) v = (TO)x[(b * Hi + sy) * (size_t)Wi + sx];
        else v = (TO)codec_gather<CODEC>(x, (b * Hi + sy) * (size_t)Wi + sx, codec, c);
    }
    y[b * (size_t)Ho * Wo + (size_t)item] = v;
}

}  // namespace hs

using namespace hs;

static bool batch_dims_ok(int32_t batch, int32_t Hi, int32_t Wi, int32_t Ho, int32_t Wo) {
    return batch <= 65535 && Hi <= RS_MAX_DIM && Wi <= RS_MAX_DIM && Ho <= RS_MAX_DIM && Wo <= RS_MAX_DIM;
}

extern "C" int hs_resize_tables_fwd(const int32_t* params, int32_t batch, int32_t Hi, int32_t Wi, int32_t Ho, int32_t Wo,
                                    int32_t filter, int32_t ks_max, int32_t* bounds, int32_t* kk, int32_t* nearest, int32_t* status,
                                    void* stream) {
    if (!params || !bounds || !kk || !nearest || !status) return HS_ERR_BAD_ARG;
    if (batch <= 0 || Hi <= 0 || Wi <= 0 || Ho <= 0 || Wo <= 0 || ks_max <= 0) return HS_ERR_BAD_ARG;
    if (filter != HS_RESIZE_BILINEAR && filter != HS_RESIZE_BICUBIC) return HS_ERR_BAD_ARG;
    if (!batch_dims_ok(batch, Hi, Wi, Ho, Wo) || ks_max > RT_MAX_KS) return HS_ERR_UNSUPPORTED;
    const int M = Ho > Wo ? Ho : Wo;
    const dim3 grid((unsigned)((M + RT_THREADS - 1) / RT_THREADS) + 1, 2, (unsigned)batch), block(RT_THREADS);
    hipStream_t s = (hipStream_t)stream;
    if (filter == HS_RESIZE_BICUBIC)
        hipLaunchKernelGGL((resize_tables_kernel<true>), grid, block, 0, s, params, Hi, Wi, Ho, Wo, M, ks_max, bounds, kk, nearest, status);
    else
        hipLaunchKernelGGL((resize_tables_kernel<false>), grid, block, 0, s, params, Hi, Wi, Ho, Wo, M, ks_max, bounds, kk, nearest, status);
    return launch_status();
}

extern "C" int hs_frame_resize_batch_fwd(const uint8_t* x, int32_t layout, int32_t batch, int32_t Hi, int32_t Wi, const int32_t* params,
                                         const int32_t* bounds, const int32_t* kk, const int32_t* status, int32_t ks_max,
                                         int32_t Ho, int32_t Wo, uint32_t fill_rgb, const float* norm_table, void* y, void* stream) {
    if (!x || !y || !params || !bounds || !kk || !status) return HS_ERR_BAD_ARG;
    if (batch <= 0 || Hi <= 0 || Wi <= 0 || Ho <= 0 || Wo <= 0 || ks_max <= 0) return HS_ERR_BAD_ARG;
    if (layout != HS_LAYOUT_HWC && layout != HS_LAYOUT_CHW) return HS_ERR_BAD_ARG;
    if (!batch_dims_ok(batch, Hi, Wi, Ho, Wo) || ks_max > RT_MAX_KS) return HS_ERR_UNSUPPORTED;
    BatchResizeArgs a;
    a.x = x; a.y = y; a.table = norm_table;
    a.params = params; a.bounds = bounds; a.kk = kk; a.status = status;
    a.Hi = Hi; a.Wi = Wi; a.Ho = Ho; a.Wo = Wo; a.M = Ho > Wo ? Ho : Wo; a.ks = ks_max;
    a.fill = fill_rgb & 0xffffffu;
    const dim3 grid((unsigned)((Wo + RS_COLS - 1) / RS_COLS), (unsigned)((Ho + RS_GROUPS * RS_TY - 1) / (RS_GROUPS * RS_TY)), (unsigned)batch);
    const dim3 block(RS_COLS * RS_GROUPS);
    hipStream_t s = (hipStream_t)stream;
    const bool hwc = layout == HS_LAYOUT_HWC;
    if (norm_table) {
        if (hwc) hipLaunchKernelGGL((frame_resize_batch_kernel<true, true>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((frame_resize_batch_kernel<false, true>), grid, block, 0, s, a);
    } else {
        if (hwc) hipLaunchKernelGGL((frame_resize_batch_kernel<true, false>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((frame_resize_batch_kernel<false, false>), grid, block, 0, s, a);
    }
    return launch_status();
}

struct LabelBatchArgs {
    const void* x; const int32_t* params; const int32_t* nearest; const int32_t* status; void* y;
    int in_dtype, out_dtype, batch, Hi, Wi, Ho, Wo, fill;
};

static int label_batch_checks(const LabelBatchArgs& a) {
    if (!a.x || !a.y || !a.params || !a.nearest || !a.status) return HS_ERR_BAD_ARG;
    if (a.batch <= 0 || a.Hi <= 0 || a.Wi <= 0 || a.Ho <= 0 || a.Wo <= 0) return HS_ERR_BAD_ARG;
    if ((a.in_dtype != HS_EVAL_U8 && a.in_dtype != HS_EVAL_I64) || (a.out_dtype != HS_EVAL_U8 && a.out_dtype != HS_EVAL_I64)) return HS_ERR_BAD_ARG;
    if (!batch_dims_ok(a.batch, a.Hi, a.Wi, a.Ho, a.Wo)) return HS_ERR_UNSUPPORTED;
    if (((long)a.Ho * a.Wo + 255) / 256 > 0x7fffffffL) return HS_ERR_UNSUPPORTED;
    return HS_OK;
}

template <typename TI, typename TO, int CODEC, typename... CA>
static void launch_label_batch(const LabelBatchArgs& a, hipStream_t s, CA... ca) {
    const dim3 grid((unsigned)(((long)a.Ho * a.Wo + 255) / 256), (unsigned)a.batch), block(256);
    hipLaunchKernelGGL((label_resize_batch_kernel<TI, TO, CODEC, CA...>), grid, block, 0, s, static_cast<const TI*>(a.x), a.params, a.nearest,
                       a.status, static_cast<TO*>(a.y), a.Hi, a.Wi, a.Ho, a.Wo, a.Ho > a.Wo ? a.Ho : a.Wo, a.fill, ca...);
}

// the storage types of a checked launch; a colour image is bytes
template <int CODEC, typename... CA>
static void label_batch_typed(const LabelBatchArgs& a, hipStream_t s, CA... ca) {
    const bool u8_out = a.out_dtype == HS_EVAL_U8;
    if (CODEC == CODEC_COLORS || a.in_dtype == HS_EVAL_U8) {
        if (u8_out) launch_label_batch<uint8_t, uint8_t, CODEC>(a, s, ca...);
        else launch_label_batch<uint8_t, int64_t, CODEC>(a, s, ca...);
    } else if constexpr (CODEC != CODEC_COLORS) {
        if (u8_out) launch_label_batch<int64_t, uint8_t, CODEC>(a, s, ca...);
        else launch_label_batch<int64_t, int64_t, CODEC>(a, s, ca...);
    }
}

extern "C" int hs_label_resize_batch_fwd(const void* x, int32_t in_dtype, int32_t batch, int32_t Hi, int32_t Wi, const int32_t* params,
                                         const int32_t* nearest, const int32_t* status, int32_t Ho, int32_t Wo, int32_t fill,
                                         void* y, int32_t out_dtype, void* stream) {
    const LabelBatchArgs a{x, params, nearest, status, y, in_dtype, out_dtype, batch, Hi, Wi, Ho, Wo, fill};
    if (const int st = label_batch_checks(a)) return st;
    label_batch_typed<CODEC_NONE>(a, (hipStream_t)stream);
    return launch_status();
}

extern "C" int hs_label_resize_batch_coded_fwd(const void* x, int32_t in_dtype, int32_t batch, int32_t Hi, int32_t Wi, const int32_t* params,
                                               const int32_t* nearest, const int32_t* status, int32_t Ho, int32_t Wo, int32_t fill,
                                               const int32_t* codec_words, int32_t codec_kind, int32_t n, int32_t unmatched,
                                               void* y, int32_t out_dtype, void* stream) {
    const LabelBatchArgs a{x, params, nearest, status, y, in_dtype, out_dtype, batch, Hi, Wi, Ho, Wo, fill};
    if (const int st = label_batch_checks(a)) return st;
    if (const int st = codec_check(codec_words, codec_kind, in_dtype, n, unmatched)) return st;
    if (codec_kind == HS_CODEC_COLORS) label_batch_typed<CODEC_COLORS>(a, (hipStream_t)stream, codec_words, (int)n, (int)unmatched);
    else label_batch_typed<CODEC_TABLE>(a, (hipStream_t)stream, codec_words, (int)n, (int)unmatched);
    return launch_status();
}
