// The VOC-SBD train chain RandomHorizontalFlip -> ColorJitter -> RandomResize -> RandomRotation -> ConstantPad -> ToTensor -> Normalize
// for a batch whose samples differ in SIZE, in a fixed number of launches per batch.  A ragged batch is a canvas plus extents: frames
// uint8 (B, Hm, Wm, 3) | (B, 3, Hm, Wm), labels (B, Hm, Wm), and per sample the (h, w) of the top-left region that is the image.  What
// lies outside that region is never read into a result.
//
//   params int32 (B, HS_RAGGED_PARAM_WORDS) = h, w, Hr, Wr, hflip, 3 reserved words: the sample's extent in the canvas, its resized size,
//   the flip of the SOURCE.  Read when the kernels RUN -- a captured graph replays with what the caller last copied into it.
//
// The launches, in the order a batch takes them (the per-pixel code is that of the one-size launches, through headers):
//   hs_resize_tables_ragged_fwd   hs_resize_tables_fwd with (Hi, Wi) = (h, w) per sample and the window = the whole resized image
//                                 (offset 0, extent (Hr, Wr)); M = max(Hc, Wc) rows per (sample, axis); the NEAREST chain serial, one
//                                 lane per (sample, axis), at most M long; the per-sample status word (hs_resample_tables.h);
//   hs_color_jitter_ragged_fwd    hs_color_jitter_fwd's clear, mean and apply passes over the sample's h x w region only: the contrast
//                                 mean is that region's, the canvas padding is neither read nor written (hs_jitter_px.h);
//   hs_frame_resize_ragged_fwd,   hs_frame_resize_batch_fwd / hs_label_resize_batch_fwd reading the canvas with its pitch; with hflip
//   hs_label_resize_ragged_fwd    source column s is column w - 1 - s -- flip-then-resize, the reference's order; Pillow's NEAREST table
//                                 is not mirror-symmetric, so flipping the window instead gives another label.  They write the uint8
//                                 intermediate canvas (B, Hc, Wc, ..), the resized image at its top left (hs_resample_px.h);
//   hs_frame_rotate_ragged_fwd,   hs_frame_rotate_fwd / hs_label_rotate_fwd with (H, W) = (Hr, Wr) per sample, reading the intermediate
//   hs_label_rotate_ragged_fwd    canvas with its pitch, writing the sample's (Ho, Wo) slice of the padded batch (hs_rotate_px.h).
// Safety: every consumer clamps the extents to its canvas and the table rows to the extents, tap counts to ks_max; a sample whose status
// is not 0 is read by nobody and comes out as pad fill everywhere; no value in params or in a table can make an access leave a canvas
// or the workspace.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <climits>
#include "hyperseg_hip.h"
#include "hs_common.h"
#include "hs_ingest.h"
#include "hs_resample_px.h"
#include "hs_resample_tables.h"
#include "hs_jitter_px.h"
#include "hs_rotate_px.h"

namespace hs {

constexpr int RG_WORDS = HS_RAGGED_PARAM_WORDS;

// a sample's geometry as a consumer uses it: all zero for a declined sample, else clamped to the two canvases
struct RaggedGeometry { int h, w, Hr, Wr; bool flip; };

__device__ __forceinline__ RaggedGeometry ragged_geometry(const int32_t* __restrict__ params, const int32_t* __restrict__ status, size_t b,
                                                          int Hm, int Wm, int Hc, int Wc) {
    const int32_t* __restrict__ p = params + RG_WORDS * b;
    RaggedGeometry g;
    const bool ok = status[b] == 0 && p[0] >= 1 && p[1] >= 1;
    g.h = ok ? min(p[0], Hm) : 0; g.w = ok ? min(p[1], Wm) : 0;
    g.Hr = ok ? min(max(p[2], 0), Hc) : 0; g.Wr = ok ? min(max(p[3], 0), Wc) : 0;
    g.flip = p[4] != 0;
    return g;
}

// HS_RESIZE_STATUS_* of a sample; 0 = its tables are built.  An axis of `in` pixels has at most min(ksize, in) taps in a row.
__device__ __forceinline__ int ragged_status(const int32_t* __restrict__ p, int Hm, int Wm, int Hc, int Wc, double filter_support, int ks_max) {
    const int h = p[0], w = p[1], Hr = p[2], Wr = p[3];
    int st = 0;
    if (h < 1 || h > Hm || w < 1 || w > Wm) st |= HS_RESIZE_STATUS_EXTENT;
    if (Hr < 1) st |= HS_RESIZE_STATUS_HR;
    if (Wr < 1) st |= HS_RESIZE_STATUS_WR;
    if (Hr > Hc || Wr > Wc) st |= HS_RESIZE_STATUS_CANVAS;
    if (st) return st;
    if (Hr != h && min(axis_scale(h, Hr, filter_support).ksize, h) > ks_max) st |= HS_RESIZE_STATUS_Y_TAPS;
    if (Wr != w && min(axis_scale(w, Wr, filter_support).ksize, w) > ks_max) st |= HS_RESIZE_STATUS_X_TAPS;
    return st;
}

template <bool BICUBIC>
__global__ __launch_bounds__(RT_THREADS)
void resize_tables_ragged_kernel(const int32_t* __restrict__ params, int Hm, int Wm, int Hc, int Wc, int M, int ks_max,
                                 int32_t* __restrict__ bounds, int32_t* __restrict__ kk, int32_t* __restrict__ nearest,
                                 int32_t* __restrict__ status) {
    const int axis = blockIdx.y;
    const size_t b = blockIdx.z;
    const int32_t* __restrict__ p = params + RG_WORDS * b;
    constexpr double filter_support = BICUBIC ? 2.0 : 1.0;
    const int st = ragged_status(p, Hm, Wm, Hc, Wc, filter_support, ks_max);
    const int in = p[axis];
    const int out = st ? 0 : p[2 + axis];      // st == 0: 1 <= out <= (Hc | Wc) <= M and 1 <= in
    const size_t row0 = (b * 2 + axis) * (size_t)M;

    if (blockIdx.x == gridDim.x - 1) {         // the workgroup of the serial chain: one lane
        if (threadIdx.x != 0) return;
        if (axis == 0) status[b] = st;
        int32_t* __restrict__ idx = nearest + row0;
        if (out > 0) {
            const double a = __ddiv_rn((double)in, (double)out);
            double xo = __dmul_rn(0.5, a);
            for (int j = 0; j < out; ++j) {
                idx[j] = min(max((int)xo, 0), in - 1);
                xo = __dadd_rn(xo, a);
            }
        }
        for (int j = out; j < M; ++j) idx[j] = 0;
        return;
    }

    const int j = blockIdx.x * RT_THREADS + threadIdx.x;
    if (j >= M) return;
    int32_t* __restrict__ bd = bounds + (row0 + j) * 2;
    int32_t* __restrict__ k_row = kk + (row0 + j) * (size_t)ks_max;
    int xmin = 0, n = 0;
    if (j < out) resize_table_row<BICUBIC>(in, out, j, ks_max, k_row, xmin, n);
    bd[0] = xmin; bd[1] = n;
    for (int k = n; k < ks_max; ++k) k_row[k] = 0;
}

struct RaggedResizeArgs {
    const uint8_t* x; uint8_t* y;
    const int32_t* params; const int32_t* bounds; const int32_t* kk; const int32_t* status;
    int Hm, Wm, Hc, Wc, M, ks;
};

template <bool HWC>
__global__ __launch_bounds__(RS_COLS * RS_GROUPS)
void frame_resize_ragged_kernel(const RaggedResizeArgs a) {
    const int x = blockIdx.x * RS_COLS + (threadIdx.x & (RS_COLS - 1));
    const int y0 = (blockIdx.y * RS_GROUPS + (threadIdx.x / RS_COLS)) * RS_TY;
    const size_t b = blockIdx.z;
    const RaggedGeometry g = ragged_geometry(a.params, a.status, b, a.Hm, a.Wm, a.Hc, a.Wc);
    if (x >= g.Wr || y0 >= g.Hr) return;       // what lies outside the resized image is read by nobody
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
        row_in[r] = jy < g.Hr;
        ymin[r] = 0; yn[r] = 0; yk[r] = ykk;
        if (row_in[r]) {
            resize_bounds(yb, jy, g.h, a.ks, ymin[r], yn[r]);
            yk[r] = ykk + (size_t)jy * a.ks;
            if (yn[r] > 0) { s0 = min(s0, ymin[r]); s1 = max(s1, ymin[r] + yn[r]); }
        }
#pragma unroll
        for (int c = 0; c < INGEST_CHANNELS; ++c) acc[r][c] = RS_HALF;
    }

    if (s0 < s1) {
        int xmin, xn;
        resize_bounds(xb, x, g.w, a.ks, xmin, xn);           // 0 <= xmin, xmin + xn <= w
        const int32_t* __restrict__ xk = xkk + (size_t)x * a.ks;
        const size_t plane = (size_t)a.Hm * a.Wm;
        const uint8_t* __restrict__ src = a.x + b * INGEST_CHANNELS * plane;
        const bool xreg = __all(xn <= RS_XREG);
        if (g.flip) {                          // uniform over the workgroup: tap k is source column (w - 1 - xmin) - k >= 0
            const int xfirst = g.w - 1 - xmin;
            if (xreg) resize_accumulate<HWC, true, -1>(src, plane, a.Wm, xfirst, xn, xk, s0, s1, ymin, yn, yk, acc);
            else resize_accumulate<HWC, false, -1>(src, plane, a.Wm, xfirst, xn, xk, s0, s1, ymin, yn, yk, acc);
        } else {
            if (xreg) resize_accumulate<HWC, true>(src, plane, a.Wm, xmin, xn, xk, s0, s1, ymin, yn, yk, acc);
            else resize_accumulate<HWC, false>(src, plane, a.Wm, xmin, xn, xk, s0, s1, ymin, yn, yk, acc);
        }
    }

    resize_store<HWC, false>(a.y, nullptr, b, a.Hc, a.Wc, x, y0, true, row_in, acc, 0u);
}

// labels: a gather through the sample's two nearest tables into the uint8 intermediate canvas; one thread per pixel of it
template <typename TI>
__global__ __launch_bounds__(256)
void label_resize_ragged_kernel(const TI* __restrict__ x, const int32_t* __restrict__ params, const int32_t* __restrict__ nearest,
                                const int32_t* __restrict__ status, uint8_t* __restrict__ y, int Hm, int Wm, int Hc, int Wc, int M) {
    const long item = (long)blockIdx.x * 256 + threadIdx.x;
    if (item >= (long)Hc * Wc) return;
    const size_t b = blockIdx.y;
    const RaggedGeometry g = ragged_geometry(params, status, b, Hm, Wm, Hc, Wc);
    const int jy = (int)(item / Wc), jx = (int)(item - (long)jy * Wc);
    if (jy >= g.Hr || jx >= g.Wr) return;
    const int32_t* __restrict__ iy = nearest + (b * 2 + 0) * (size_t)M;
    const int32_t* __restrict__ ix = nearest + (b * 2 + 1) * (size_t)M;
    const int sy = min(max(iy[jy], 0), g.h - 1);
    int sx = min(max(ix[jx], 0), g.w - 1);
    if (g.flip) sx = g.w - 1 - sx;
    y[b * (size_t)Hc * Wc + (size_t)item] = (uint8_t)x[(b * Hm + sy) * (size_t)Wm + sx];
}

// ---------------------------------------------------------------------------------------------------------------- colour jitter

struct RaggedJitterArgs {
    const uint8_t* x; uint8_t* y; const int32_t* params; const int32_t* table; unsigned long long* sums;
    int Hm, Wm;
};

// the sample's region; (0, 0) where the extent does not lie in the canvas (its status says so; the sample is then left alone)
__device__ __forceinline__ void ragged_region(const int32_t* __restrict__ params, size_t b, int Hm, int Wm, int& h, int& w) {
    h = params[RG_WORDS * b]; w = params[RG_WORDS * b + 1];
    if (h < 1 || h > Hm || w < 1 || w > Wm) h = w = 0;
}

// region pixels q0 .. q0 + cnt - 1 (cnt in 1..4, row-major in the h x w region) of one sample -> v[channel][i] and their canvas pixel
// indices; entries past cnt repeat pixel q0
template <bool HWC>
__device__ __forceinline__ void ragged_load4(const uint8_t* __restrict__ img, size_t plane, int Wm, int w, unsigned q0, int cnt,
                                             int (&v)[3][4], unsigned (&pix)[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const unsigned q = q0 + (i < cnt ? i : 0);
        const unsigned row = q / (unsigned)w;
        pix[i] = row * (unsigned)Wm + (q - row * (unsigned)w);           // < Hm Wm <= 2^26
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c][i] = HWC ? img[3 * (size_t)pix[i] + c] : img[c * plane + pix[i]];
    }
}

template <bool HWC>
__global__ __launch_bounds__(256)
void jitter_mean_ragged_kernel(const RaggedJitterArgs a) {
    __shared__ HueTabs tabs;
    __shared__ unsigned long long wave_sum[4];
    const size_t b = blockIdx.y;
    const JitterRec rec = jitter_record(a.table, b);
    int h, w;
    ragged_region(a.params, b, a.Hm, a.Wm, h, w);
    if (!jitter_has(rec, JT_CONTRAST) || h == 0) return;           // uniform: the whole workgroup leaves
    const int tid = (int)threadIdx.x;
    if (jitter_has(rec, JT_HUE)) hue_tabs_fill(tabs, tid);
    __syncthreads();
    const size_t plane = (size_t)a.Hm * a.Wm;
    const uint8_t* __restrict__ img = a.x + b * 3 * plane;
    const unsigned n = (unsigned)h * (unsigned)w, groups = (n + 3) >> 2;
    unsigned acc = 0;                                              // a thread sees at most 4 * 2^24 / 2^18 pixels of <= 255 each
    for (unsigned grp = blockIdx.x * 256u + tid; grp < groups; grp += gridDim.x * 256u) {
        const unsigned q0 = grp << 2;
        const int cnt = (int)min(4u, n - q0);
        int v[3][4];
        unsigned pix[4];
        ragged_load4<HWC>(img, plane, a.Wm, w, q0, cnt, v, pix);
        jitter_ops<true>(rec, tabs, 0, v);
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (i < cnt) acc += (unsigned)jitter_gray(v[0][i], v[1][i], v[2][i]);
    }
    unsigned long long sum = acc;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_down(sum, off, 64);
    if ((tid & 63) == 0) wave_sum[tid >> 6] = sum;
    __syncthreads();
    if (tid == 0) atomicAdd(a.sums + b, wave_sum[0] + wave_sum[1] + wave_sum[2] + wave_sum[3]);
}

template <bool HWC>
__global__ __launch_bounds__(256)
void jitter_apply_ragged_kernel(const RaggedJitterArgs a) {
    __shared__ HueTabs tabs;
    const size_t b = blockIdx.y;
    const JitterRec rec = jitter_record(a.table, b);
    int h, w;
    ragged_region(a.params, b, a.Hm, a.Wm, h, w);
    const unsigned n = (unsigned)h * (unsigned)w;
    if ((blockIdx.x * 256u) << 2 >= n) return;                     // uniform; also leaves when the extent was declined (n = 0)
    const int tid = (int)threadIdx.x;
    if (jitter_has(rec, JT_HUE)) hue_tabs_fill(tabs, tid);
    __syncthreads();
    int m = 0;
    if (a.sums && jitter_has(rec, JT_CONTRAST)) m = jitter_clip8((int)((double)a.sums[b] / (double)n + 0.5));
    const unsigned q0 = (blockIdx.x * 256u + tid) << 2;
    if (q0 >= n) return;
    const int cnt = (int)min(4u, n - q0);
    const size_t plane = (size_t)a.Hm * a.Wm;
    const uint8_t* __restrict__ img = a.x + b * 3 * plane;
    int v[3][4];
    unsigned pix[4];
    ragged_load4<HWC>(img, plane, a.Wm, w, q0, cnt, v, pix);
    jitter_ops<false>(rec, tabs, m, v);
    uint8_t* __restrict__ out = a.y + b * 3 * plane;
    for (int i = 0; i < cnt; ++i) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if constexpr (HWC) out[3 * (size_t)pix[i] + c] = (uint8_t)v[c][i];
            else out[c * plane + pix[i]] = (uint8_t)v[c][i];
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- rotate + pad

struct RaggedRotateArgs {
    const uint8_t* x; void* y; const float* table; const double* m; const int32_t* params; const int32_t* status;
    int Hc, Wc, Ho, Wo;
    unsigned fill, pad_fill;                   // r | g << 8 | b << 16
};

template <bool HWC, bool NORM>
__global__ __launch_bounds__(RT_COLS * RT_ROWS)
void frame_rotate_ragged_kernel(const RaggedRotateArgs a) {
    __shared__ float tab[NORM ? INGEST_TABLE_FLOATS : 1];
    if constexpr (NORM) {
        ingest_table_to_lds(a.table, tab, (int)threadIdx.x);
        __syncthreads();
    }
    const int x = blockIdx.x * RT_COLS + (threadIdx.x & (RT_COLS - 1));
    const int y = blockIdx.y * RT_ROWS + (threadIdx.x / RT_COLS);
    if (x >= a.Wo || y >= a.Ho) return;
    const size_t b = blockIdx.z;
    const int32_t* __restrict__ p = a.params + RG_WORDS * b;
    const bool ok = a.status[b] == 0;
    const int H = ok ? min(max(p[2], 0), a.Hc) : 0, W = ok ? min(max(p[3], 0), a.Wc) : 0;      // the image inside the intermediate canvas
    unsigned out[INGEST_CHANNELS];
#pragma unroll
    for (int c = 0; c < INGEST_CHANNELS; ++c) out[c] = (a.pad_fill >> (8 * c)) & 255u;
    if (x < W && y < H) {
        const size_t plane = (size_t)a.Hc * a.Wc;
        rotate_frame_pixel<HWC>(a.x + b * INGEST_CHANNELS * plane, plane, a.Wc, H, W, a.m + 6 * b, x, y, a.fill, out);
    }
    rotate_store<HWC, NORM>(a.y, tab, b, a.Ho, a.Wo, x, y, out);
}

template <typename TO>
__global__ __launch_bounds__(256)
void label_rotate_ragged_kernel(const uint8_t* __restrict__ x, const int32_t* __restrict__ params, const int32_t* __restrict__ status,
                                const int32_t* __restrict__ fixed, TO* __restrict__ y, int Hc, int Wc, int Ho, int Wo, int fill,
                                int pad_fill) {
    const long item = (long)blockIdx.x * 256 + threadIdx.x;
    if (item >= (long)Ho * Wo) return;
    const int yy = (int)(item / Wo), xx = (int)(item - (long)yy * Wo);
    const size_t b = blockIdx.y;
    const int32_t* __restrict__ p = params + RG_WORDS * b;
    const bool ok = status[b] == 0;
    const int H = ok ? min(max(p[2], 0), Hc) : 0, W = ok ? min(max(p[3], 0), Wc) : 0;
    TO v = (TO)pad_fill;
    if (yy < H && xx < W) {
        int xs, ys;
        rotate_label_source(fixed + 6 * b, xx, yy, xs, ys);
        v = (TO)fill;
        if (xs >= 0 && xs < W && ys >= 0 && ys < H) v = (TO)x[(b * Hc + ys) * (size_t)Wc + xs];
    }
    y[b * (size_t)Ho * Wo + (size_t)item] = v;
}

}  // namespace hs

using namespace hs;

// every canvas dimension: the rotation's limit (Pillow's 32-bit label arithmetic), which also keeps a canvas below 2^26 pixels
static bool ragged_dims_ok(int32_t batch, int32_t a, int32_t b, int32_t c, int32_t d) {
    return batch <= 65535 && a <= RT_MAX_DIM && b <= RT_MAX_DIM && c <= RT_MAX_DIM && d <= RT_MAX_DIM;
}

extern "C" int hs_resize_tables_ragged_fwd(const int32_t* params, int32_t batch, int32_t Hm, int32_t Wm, int32_t Hc, int32_t Wc,
                                           int32_t filter, int32_t ks_max, int32_t* bounds, int32_t* kk, int32_t* nearest,
                                           int32_t* status, void* stream) {
    if (!params || !bounds || !kk || !nearest || !status) return HS_ERR_BAD_ARG;
    if (batch <= 0 || Hm <= 0 || Wm <= 0 || Hc <= 0 || Wc <= 0 || ks_max <= 0) return HS_ERR_BAD_ARG;
    if (filter != HS_RESIZE_BILINEAR && filter != HS_RESIZE_BICUBIC) return HS_ERR_BAD_ARG;
    if (!ragged_dims_ok(batch, Hm, Wm, Hc, Wc) || ks_max > RT_MAX_KS) return HS_ERR_UNSUPPORTED;
    const int M = Hc > Wc ? Hc : Wc;
    const dim3 grid((unsigned)((M + RT_THREADS - 1) / RT_THREADS) + 1, 2, (unsigned)batch), block(RT_THREADS);
    hipStream_t s = (hipStream_t)stream;
    if (filter == HS_RESIZE_BICUBIC)
        hipLaunchKernelGGL((resize_tables_ragged_kernel<true>), grid, block, 0, s, params, Hm, Wm, Hc, Wc, M, ks_max, bounds, kk, nearest, status);
    else
        hipLaunchKernelGGL((resize_tables_ragged_kernel<false>), grid, block, 0, s, params, Hm, Wm, Hc, Wc, M, ks_max, bounds, kk, nearest, status);
    return launch_status();
}

extern "C" int hs_frame_resize_ragged_fwd(const uint8_t* x, int32_t layout, int32_t batch, int32_t Hm, int32_t Wm, const int32_t* params,
                                          const int32_t* bounds, const int32_t* kk, const int32_t* status, int32_t ks_max,
                                          int32_t Hc, int32_t Wc, uint8_t* y, void* stream) {
    if (!x || !y || !params || !bounds || !kk || !status) return HS_ERR_BAD_ARG;
    if (batch <= 0 || Hm <= 0 || Wm <= 0 || Hc <= 0 || Wc <= 0 || ks_max <= 0) return HS_ERR_BAD_ARG;
    if (layout != HS_LAYOUT_HWC && layout != HS_LAYOUT_CHW) return HS_ERR_BAD_ARG;
    if (!ragged_dims_ok(batch, Hm, Wm, Hc, Wc) || ks_max > RT_MAX_KS) return HS_ERR_UNSUPPORTED;
    RaggedResizeArgs a;
    a.x = x; a.y = y; a.params = params; a.bounds = bounds; a.kk = kk; a.status = status;
    a.Hm = Hm; a.Wm = Wm; a.Hc = Hc; a.Wc = Wc; a.M = Hc > Wc ? Hc : Wc; a.ks = ks_max;
    const dim3 grid((unsigned)((Wc + RS_COLS - 1) / RS_COLS), (unsigned)((Hc + RS_GROUPS * RS_TY - 1) / (RS_GROUPS * RS_TY)), (unsigned)batch);
    const dim3 block(RS_COLS * RS_GROUPS);
    hipStream_t s = (hipStream_t)stream;
    if (layout == HS_LAYOUT_HWC) hipLaunchKernelGGL(frame_resize_ragged_kernel<true>, grid, block, 0, s, a);
    else hipLaunchKernelGGL(frame_resize_ragged_kernel<false>, grid, block, 0, s, a);
    return launch_status();
}

extern "C" int hs_label_resize_ragged_fwd(const void* x, int32_t in_dtype, int32_t batch, int32_t Hm, int32_t Wm, const int32_t* params,
                                          const int32_t* nearest, const int32_t* status, int32_t Hc, int32_t Wc, uint8_t* y,
                                          void* stream) {
    if (!x || !y || !params || !nearest || !status) return HS_ERR_BAD_ARG;
    if (batch <= 0 || Hm <= 0 || Wm <= 0 || Hc <= 0 || Wc <= 0) return HS_ERR_BAD_ARG;
    if (in_dtype != HS_EVAL_U8 && in_dtype != HS_EVAL_I64) return HS_ERR_BAD_ARG;
    if (!ragged_dims_ok(batch, Hm, Wm, Hc, Wc)) return HS_ERR_UNSUPPORTED;
    const long blocks = ((long)Hc * Wc + 255) / 256;
    const int M = Hc > Wc ? Hc : Wc;
    const dim3 grid((unsigned)blocks, (unsigned)batch), block(256);
    hipStream_t s = (hipStream_t)stream;
    if (in_dtype == HS_EVAL_U8)
        hipLaunchKernelGGL(label_resize_ragged_kernel<uint8_t>, grid, block, 0, s, static_cast<const uint8_t*>(x), params, nearest, status, y, Hm, Wm, Hc, Wc, M);
    else
        hipLaunchKernelGGL(label_resize_ragged_kernel<int64_t>, grid, block, 0, s, static_cast<const int64_t*>(x), params, nearest, status, y, Hm, Wm, Hc, Wc, M);
    return launch_status();
}

extern "C" int hs_color_jitter_ragged_fwd(const uint8_t* x, int32_t layout, int32_t batch, int32_t Hm, int32_t Wm, const int32_t* params,
                                          const int32_t* table, uint64_t* sums, uint8_t* y, void* stream) {
    if (!x || !y || !params || !table || batch <= 0 || Hm <= 0 || Wm <= 0) return HS_ERR_BAD_ARG;
    if (layout != HS_LAYOUT_HWC && layout != HS_LAYOUT_CHW) return HS_ERR_BAD_ARG;
    if (!ragged_dims_ok(batch, Hm, Wm, 1, 1)) return HS_ERR_UNSUPPORTED;
    RaggedJitterArgs a;
    a.x = x; a.y = y; a.params = params; a.table = table; a.sums = reinterpret_cast<unsigned long long*>(sums);
    a.Hm = Hm; a.Wm = Wm;
    const long blocks = (((long)Hm * Wm + 3) / 4 + 255) / 256;      // <= 2^16
    hipStream_t s = (hipStream_t)stream;
    const bool hwc = layout == HS_LAYOUT_HWC;
    const dim3 block(256);
    if (sums) {
        hipError_t e = hipMemsetAsync(sums, 0, sizeof(uint64_t) * (size_t)batch, s);
        if (e != hipSuccess) return (int)e;
        const dim3 grid((unsigned)(blocks < JT_MEAN_BLOCKS ? blocks : JT_MEAN_BLOCKS), (unsigned)batch);
        if (hwc) hipLaunchKernelGGL(jitter_mean_ragged_kernel<true>, grid, block, 0, s, a);
        else hipLaunchKernelGGL(jitter_mean_ragged_kernel<false>, grid, block, 0, s, a);
    }
    const dim3 grid((unsigned)blocks, (unsigned)batch);
    if (hwc) hipLaunchKernelGGL(jitter_apply_ragged_kernel<true>, grid, block, 0, s, a);
    else hipLaunchKernelGGL(jitter_apply_ragged_kernel<false>, grid, block, 0, s, a);
    return launch_status();
}

extern "C" int hs_frame_rotate_ragged_fwd(const uint8_t* x, int32_t layout, int32_t batch, int32_t Hc, int32_t Wc, const int32_t* params,
                                          const int32_t* status, const double* matrices, int32_t Ho, int32_t Wo, uint32_t fill_rgb,
                                          uint32_t pad_fill_rgb, const float* norm_table, void* y, void* stream) {
    if (!x || !y || !params || !status || !matrices) return HS_ERR_BAD_ARG;
    if (batch <= 0 || Hc <= 0 || Wc <= 0 || Ho <= 0 || Wo <= 0) return HS_ERR_BAD_ARG;
    if (layout != HS_LAYOUT_HWC && layout != HS_LAYOUT_CHW) return HS_ERR_BAD_ARG;
    if (!ragged_dims_ok(batch, Hc, Wc, Ho, Wo)) return HS_ERR_UNSUPPORTED;
    RaggedRotateArgs a;
    a.x = x; a.y = y; a.table = norm_table; a.m = matrices; a.params = params; a.status = status;
    a.Hc = Hc; a.Wc = Wc; a.Ho = Ho; a.Wo = Wo;
    a.fill = fill_rgb & 0xffffffu; a.pad_fill = pad_fill_rgb & 0xffffffu;
    const dim3 grid((unsigned)((Wo + RT_COLS - 1) / RT_COLS), (unsigned)((Ho + RT_ROWS - 1) / RT_ROWS), (unsigned)batch);
    const dim3 block(RT_COLS * RT_ROWS);
    hipStream_t s = (hipStream_t)stream;
    const bool hwc = layout == HS_LAYOUT_HWC;
    if (norm_table) {
        if (hwc) hipLaunchKernelGGL((frame_rotate_ragged_kernel<true, true>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((frame_rotate_ragged_kernel<false, true>), grid, block, 0, s, a);
    } else {
        if (hwc) hipLaunchKernelGGL((frame_rotate_ragged_kernel<true, false>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((frame_rotate_ragged_kernel<false, false>), grid, block, 0, s, a);
    }
    return launch_status();
}

extern "C" int hs_label_rotate_ragged_fwd(const uint8_t* x, int32_t batch, int32_t Hc, int32_t Wc, const int32_t* params,
                                          const int32_t* status, const int32_t* fixed, int32_t Ho, int32_t Wo, int32_t fill,
                                          int32_t pad_fill, void* y, int32_t out_dtype, void* stream) {
    if (!x || !y || !params || !status || !fixed) return HS_ERR_BAD_ARG;
    if (batch <= 0 || Hc <= 0 || Wc <= 0 || Ho <= 0 || Wo <= 0) return HS_ERR_BAD_ARG;
    if (out_dtype != HS_EVAL_U8 && out_dtype != HS_EVAL_I64) return HS_ERR_BAD_ARG;
    if (!ragged_dims_ok(batch, Hc, Wc, Ho, Wo)) return HS_ERR_UNSUPPORTED;
    const long blocks = ((long)Ho * Wo + 255) / 256;
    const dim3 grid((unsigned)blocks, (unsigned)batch), block(256);
    hipStream_t s = (hipStream_t)stream;
    if (out_dtype == HS_EVAL_U8)
        hipLaunchKernelGGL(label_rotate_ragged_kernel<uint8_t>, grid, block, 0, s, x, params, status, fixed, static_cast<uint8_t*>(y), Hc, Wc, Ho, Wo, fill, pad_fill);
    else
        hipLaunchKernelGGL(label_rotate_ragged_kernel<int64_t>, grid, block, 0, s, x, params, status, fixed, static_cast<int64_t*>(y), Hc, Wc, Ho, Wo, fill, pad_fill);
    return launch_status();
}
