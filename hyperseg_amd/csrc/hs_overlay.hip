// Served overlays: the class map coloured and alpha-blended over the uint8 input frame, returned as uint8 RGB -- the reference's display
// chain tensor2rgb(blend_seg(img, pred, color_map, alpha, ignore_index)) (hyperseg/test.py:230-292, utils/seg_utils.py:82-103,
// utils/img_utils.py:62-75) for a frame normalised with mean = std = 0.5 -- either from finished masks (hs_overlay_fwd) or as the epilogue
// of the final upsample + arg-max launch, where every output pixel's class index already sits in a register (hs_upsample_overlay_fwd).
// An overlay served at ANOTHER size than the model's frame -- the camera frame's, when the model sees a down-scaled copy of it -- takes
// hs_upsample2_overlay_fwd: the decoder's final resize composed with the one to that size (test.py:167-168: the logits are resized before
// the arg-max), the class indices of hs_upsample2_confusion_fwd's masks-only call, blended over the frames at that size in the same
// launch; neither resized logits tensor nor a frame-size mask ever exists in memory.
//
// The arithmetic is data (hyperseg_amd.utils.inference.Overlay builds it on the host, in float32, by the reference's own operations):
//   tables = [ A (256) | A1 (256) | S (n x 3) ],  A[v] = img(v) * am,  A1[v] = img(v),  S[c][ch] = (color[c][ch] / 128 - 1) * (1 - am)
//   blended pixel:      out = uint8(rint(((A[v]  + S[c][ch]) * 0.5 + 0.5) * 255))
//   pixel left alone:   out = uint8(rint(( A1[v]             * 0.5 + 0.5) * 255))  == v for all 256 bytes
// (class == ignore_index or class >= n: left alone).  The kernels look up, add, scale and round (rint: half to even, as np.round);
// x * 0.5 is exact, so it does not matter whether the compiler contracts `* 0.5 + 0.5`.
//
// Shape: the tables live in LDS (2 KB + 12 bytes per colour: 5 KB at 256 colours); one thread owns 4 consecutive pixels of a row -- for
// 'hwc' frames 12 contiguous bytes in and 12 out, three dwords each way where both addresses are 4-byte aligned and the 4 pixels exist,
// bytes otherwise (any base pointer, any width); for 'chw' one dword per plane.  Ordinary vector stores only: no atomics, nothing waits
// on another workgroup, nothing is read back by the host.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "hyperseg_hip.h"
#include "hs_common.h"
#include "hs_upsample_taps.h"

namespace hs {

constexpr int OVL_A = 0, OVL_A1 = 256, OVL_S = 512;
constexpr int OVL_MAX_COLORS = 256;
constexpr int OVL_TABLE_FLOATS = OVL_S + 3 * OVL_MAX_COLORS;       // 5 KB
constexpr int OVL_THREADS = 256;
constexpr int OVL_MAX_BLOCKS = 2048;                               // the standalone kernel grid-strides beyond this many workgroups

// every thread of the workgroup: global tables -> LDS (the caller puts a barrier between this and the first lookup)
__device__ __forceinline__ void overlay_tables_to_lds(const float* __restrict__ tables, float* __restrict__ tab, int ncol) {
    for (int i = threadIdx.x; i < OVL_S + 3 * ncol; i += OVL_THREADS) tab[i] = tables[i];
}

// 3 * class for a pixel that is blended, -1 for one that is left alone
__device__ __forceinline__ int overlay_key(int cls, int ncol, int ignore) { return (cls < ncol && cls != ignore) ? 3 * cls : -1; }

__device__ __forceinline__ unsigned overlay_value(const float* __restrict__ tab, unsigned v, int key, int ch) {
    const float t = key >= 0 ? tab[OVL_A + (int)v] + tab[OVL_S + key + ch] : tab[OVL_A1 + (int)v];
    return (unsigned)rintf((t * 0.5f + 0.5f) * 255.0f);
}

// Pixels pix .. pix + n - 1 (1 <= n <= 4, one row) of the frame at `fb` blended into the overlay at `ob` (both: image b's first byte),
// `plane` = H * W, cls: their class indices.
template <bool HWC>
__device__ __forceinline__ void overlay_row4(const float* __restrict__ tab, const uint8_t* __restrict__ fb, uint8_t* __restrict__ ob,
                                             size_t plane, size_t pix, int n, const int (&cls)[4], int ncol, int ignore) {
    int key[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) key[i] = overlay_key(cls[i], ncol, ignore);
    if constexpr (HWC) {
        const uint8_t* __restrict__ p = fb + pix * 3;
        uint8_t* __restrict__ d = ob + pix * 3;
        if (n == 4 && aligned_to(p, 4) && aligned_to(d, 4)) {
            // r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3: byte j is channel j % 3 of pixel j / 3
            unsigned w[3], o[3] = {0u, 0u, 0u};
#pragma unroll
            for (int k = 0; k < 3; ++k) w[k] = reinterpret_cast<const unsigned*>(p)[k];
#pragma unroll
            for (int j = 0; j < 12; ++j) {
                const unsigned v = (w[j >> 2] >> (8 * (j & 3))) & 255u;
                o[j >> 2] |= overlay_value(tab, v, key[j / 3], j % 3) << (8 * (j & 3));
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) reinterpret_cast<unsigned*>(d)[k] = o[k];
        } else {
            for (int i = 0; i < n; ++i)
#pragma unroll
                for (int c = 0; c < 3; ++c) d[3 * i + c] = (uint8_t)overlay_value(tab, p[3 * i + c], key[i], c);
        }
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const uint8_t* __restrict__ p = fb + c * plane + pix;
            uint8_t* __restrict__ d = ob + c * plane + pix;
            if (n == 4 && aligned_to(p, 4) && aligned_to(d, 4)) {
                const unsigned w = *reinterpret_cast<const unsigned*>(p);
                unsigned o = 0u;
#pragma unroll
                for (int i = 0; i < 4; ++i) o |= overlay_value(tab, (w >> (8 * i)) & 255u, key[i], c) << (8 * i);
                *reinterpret_cast<unsigned*>(d) = o;
            } else {
                for (int i = 0; i < n; ++i) d[i] = (uint8_t)overlay_value(tab, p[i], key[i], c);
            }
        }
    }
}

// Finished masks: blockIdx.y = frame, blockIdx.x grid-strides over H * ceil(W / 4) items.
template <bool HWC>
__global__ __launch_bounds__(OVL_THREADS)
void overlay_kernel(const uint8_t* __restrict__ mask, const uint8_t* __restrict__ frames, const float* __restrict__ tables,
                    uint8_t* __restrict__ out, int H, int W, int wq, int ncol, int ignore) {
    __shared__ float tab[OVL_TABLE_FLOATS];
    overlay_tables_to_lds(tables, tab, ncol);
    __syncthreads();
    const long items = (long)H * wq;
    const size_t b = blockIdx.y, plane = (size_t)H * W;
    for (long item = (long)blockIdx.x * OVL_THREADS + threadIdx.x; item < items; item += (long)gridDim.x * OVL_THREADS) {
        const int yy = (int)(item / wq), x0 = 4 * (int)(item - (long)yy * wq);
        const int n = min(4, W - x0);                               // >= 1
        const size_t pix = (size_t)yy * W + x0;
        const uint8_t* __restrict__ mp = mask + b * plane + pix;
        int cls[4];
        if (n == 4 && aligned_to(mp, 4)) {
            const unsigned w = *reinterpret_cast<const unsigned*>(mp);
#pragma unroll
            for (int i = 0; i < 4; ++i) cls[i] = (int)((w >> (8 * i)) & 255u);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) cls[i] = (int)mp[i < n ? i : 0];
        }
        overlay_row4<HWC>(tab, frames + b * plane * 3, out + b * plane * 3, plane, pix, n, cls, ncol, ignore);
    }
}

// Exact 2x: argmax2x_block (hs_upsample_taps.h), four consecutive lanes per 2 x 4 output block, after which all four lanes hold the
// block's eight class indices: lane 0 stores the masks, lanes 0 and 1 blend one row of four pixels each.
template <bool HWC>
__global__ __launch_bounds__(OVL_THREADS)
void upsample2x_overlay_kernel(const float* __restrict__ x, int B, int C, int Hi, int Wi, const uint8_t* __restrict__ frames,
                               const float* __restrict__ tables, int ncol, int ignore, uint8_t* __restrict__ mask,
                               uint8_t* __restrict__ out) {
    __shared__ float tab[OVL_TABLE_FLOATS];
    overlay_tables_to_lds(tables, tab, ncol);
    __syncthreads();
    const int wq = Wi >> 1;
    const size_t n = (size_t)B * Hi * wq;
    const int Wo = 2 * Wi;
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int sub = (int)(t & 3);
    const size_t e0 = t >> 2;
    const size_t e = e0 < n ? e0 : n - 1;                    // surplus lanes shadow the last block (argmax2x_block: convergent)
    const int q = e % wq; size_t r = e / wq;
    const int yi = r % Hi; const size_t b = r / Hi;
    const float* __restrict__ xb = x + b * C * Hi * Wi;
    int idx0[4], idx1[4];
    argmax2x_block(xb, C, Hi, Wi, yi, q, sub, idx0, idx1);
    if (e0 >= n) return;
    const size_t plane = (size_t)2 * Hi * Wo;
    const size_t pix = (size_t)(2 * yi) * Wo + 4 * q;        // of the block's upper row, inside image b
    if (sub == 0) {
        uint8_t* dst = mask + b * plane + pix;
        *reinterpret_cast<uchar4*>(dst) = make_uchar4(idx0[0], idx0[1], idx0[2], idx0[3]);
        *reinterpret_cast<uchar4*>(dst + Wo) = make_uchar4(idx1[0], idx1[1], idx1[2], idx1[3]);
    }
    if (sub < 2) {
        int cls[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) cls[i] = sub ? idx1[i] : idx0[i];
        overlay_row4<HWC>(tab, frames + b * plane * 3, out + b * plane * 3, plane, pix + (sub ? Wo : 0), 4, cls, ncol, ignore);
    }
}

// General resize (any ratio, the identity included): argmax_row4 (hs_upsample_taps.h), one thread = 4 consecutive output pixels of a
// row, which it then blends.
template <bool HWC>
__global__ __launch_bounds__(OVL_THREADS)
void upsample_overlay_kernel(const float* __restrict__ x, int B, int C, int Hi, int Wi, int Ho, int Wo, float scale_y, float scale_x,
                             const uint8_t* __restrict__ frames, const float* __restrict__ tables, int ncol, int ignore,
                             uint8_t* __restrict__ mask, uint8_t* __restrict__ out) {
    __shared__ float tab[OVL_TABLE_FLOATS];
    overlay_tables_to_lds(tables, tab, ncol);
    __syncthreads();
    const int wq = (Wo + 3) / 4;
    const size_t n = (size_t)B * Ho * wq;
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    const int q = e % wq; size_t r = e / wq;
    const int yo = r % Ho; const size_t b = r / Ho;
    const Row4 t = row4_taps(yo, q, Hi, Wi, Wo, scale_y, scale_x);
    const float* __restrict__ xb = x + b * C * Hi * Wi;
    int idx[4];
    argmax_row4(xb, C, Hi, Wi, t, idx);
    const size_t plane = (size_t)Ho * Wo, pix = (size_t)yo * Wo + 4 * q;
    const int live = min(4, Wo - 4 * q);
    uint8_t* dst = mask + b * plane + pix;
    if (live == 4 && aligned_to(dst, 4)) {
        *reinterpret_cast<uchar4*>(dst) = make_uchar4(idx[0], idx[1], idx[2], idx[3]);
    } else {
        for (int i = 0; i < live; ++i) dst[i] = (uint8_t)idx[i];
    }
    overlay_row4<HWC>(tab, frames + b * plane * 3, out + b * plane * 3, plane, pix, live, idx, ncol, ignore);
}

// Two resizes composed in registers (x -> mid -> frame: the decoder's final resize, then the one to the camera frame's size), both stages
// exact 2x: argmax2x2x_block (hs_upsample_taps.h), four consecutive lanes per x block (yi, q) = 4 x 8 output block, after which all four
// lanes hold the block's 32 class indices; lane `sub` takes output row 4 yi + sub: two dword stores of masks, two rows of four blended.
template <bool HWC>
__global__ __launch_bounds__(OVL_THREADS)
void upsample2x2x_overlay_kernel(const float* __restrict__ x, int B, int C, int Hi, int Wi, const uint8_t* __restrict__ frames,
                                 const float* __restrict__ tables, int ncol, int ignore, uint8_t* __restrict__ mask,
                                 uint8_t* __restrict__ out) {
    __shared__ float tab[OVL_TABLE_FLOATS];
    overlay_tables_to_lds(tables, tab, ncol);
    __syncthreads();
    const int wq = Wi >> 1;
    const size_t n = (size_t)B * Hi * wq;
    const int Wo = 4 * Wi;
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int sub = (int)(t & 3);
    const size_t e0 = t >> 2;
    const size_t e = e0 < n ? e0 : n - 1;                    // surplus lanes shadow the last block (argmax2x2x_block: convergent)
    const int q = e % wq; size_t r = e / wq;
    const int yi = r % Hi; const size_t b = r / Hi;
    const float* __restrict__ xb = x + b * C * Hi * Wi;
    int idx[4][8];
    argmax2x2x_block(xb, C, Hi, Wi, yi, q, sub, idx);
    if (e0 >= n) return;
    int lo[4], hi[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        lo[k] = sub == 0 ? idx[0][k] : sub == 1 ? idx[1][k] : sub == 2 ? idx[2][k] : idx[3][k];
        hi[k] = sub == 0 ? idx[0][4 + k] : sub == 1 ? idx[1][4 + k] : sub == 2 ? idx[2][4 + k] : idx[3][4 + k];
    }
    const size_t plane = (size_t)4 * Hi * Wo;
    const size_t pix = (size_t)(4 * yi + sub) * Wo + 8 * q;  // of the lane's row, inside image b
    uint8_t* dst = mask + b * plane + pix;
    *reinterpret_cast<uchar4*>(dst) = make_uchar4(lo[0], lo[1], lo[2], lo[3]);
    *reinterpret_cast<uchar4*>(dst + 4) = make_uchar4(hi[0], hi[1], hi[2], hi[3]);
    overlay_row4<HWC>(tab, frames + b * plane * 3, out + b * plane * 3, plane, pix, 4, lo, ncol, ignore);
    overlay_row4<HWC>(tab, frames + b * plane * 3, out + b * plane * 3, plane, pix + 4, 4, hi, ncol, ignore);
}

// Two resizes composed, any first and any second stage (down-sampling and identity stages included): argmax2_row4 (hs_upsample_taps.h),
// otherwise upsample_overlay_kernel.
template <bool HWC>
__global__ __launch_bounds__(OVL_THREADS)
void upsample2_overlay_kernel(const float* __restrict__ x, int B, int C, Stages2 s, const uint8_t* __restrict__ frames,
                              const float* __restrict__ tables, int ncol, int ignore, uint8_t* __restrict__ mask,
                              uint8_t* __restrict__ out) {
    __shared__ float tab[OVL_TABLE_FLOATS];
    overlay_tables_to_lds(tables, tab, ncol);
    __syncthreads();
    const int Ho = s.Ho, Wo = s.Wo, wq = (Wo + 3) / 4;
    const size_t n = (size_t)B * Ho * wq;
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    const int q = e % wq; size_t r = e / wq;
    const int yo = r % Ho; const size_t b = r / Ho;
    const Row4x2 t = row4x2_taps(yo, q, s);
    const float* __restrict__ xb = x + b * C * s.Hi * s.Wi;
    int idx[4];
    argmax2_row4(xb, C, s.Hi, s.Wi, t, idx);
    const size_t plane = (size_t)Ho * Wo, pix = (size_t)yo * Wo + 4 * q;
    const int live = min(4, Wo - 4 * q);
    uint8_t* dst = mask + b * plane + pix;
    if (live == 4 && aligned_to(dst, 4)) {
        *reinterpret_cast<uchar4*>(dst) = make_uchar4(idx[0], idx[1], idx[2], idx[3]);
    } else {
        for (int i = 0; i < live; ++i) dst[i] = (uint8_t)idx[i];
    }
    overlay_row4<HWC>(tab, frames + b * plane * 3, out + b * plane * 3, plane, pix, live, idx, ncol, ignore);
}

static bool overlay_args_ok(int layout, const float* tables, int num_colors) {
    return tables && (layout == HS_LAYOUT_HWC || layout == HS_LAYOUT_CHW) && num_colors >= 1 && num_colors <= OVL_MAX_COLORS;
}

}  // namespace hs

using namespace hs;

extern "C" int hs_overlay_fwd(const uint8_t* masks, const uint8_t* frames, int32_t layout, int32_t batch, int32_t H, int32_t W,
                              const float* tables, int32_t num_colors, int32_t ignore_index, uint8_t* overlay, void* stream) {
    if (!masks || !frames || !overlay || batch <= 0 || H <= 0 || W <= 0 || !overlay_args_ok(layout, tables, num_colors)) return HS_ERR_BAD_ARG;
    if (batch > 65535) return HS_ERR_UNSUPPORTED;
    const int wq = (W + 3) / 4;
    long blocks = ((long)H * wq + OVL_THREADS - 1) / OVL_THREADS;
    if (blocks > OVL_MAX_BLOCKS) blocks = OVL_MAX_BLOCKS;
    const dim3 grid((unsigned)blocks, (unsigned)batch), block(OVL_THREADS);
    hipStream_t s = (hipStream_t)stream;
    if (layout == HS_LAYOUT_HWC)
        hipLaunchKernelGGL(overlay_kernel<true>, grid, block, 0, s, masks, frames, tables, overlay, H, W, wq, num_colors, ignore_index);
    else
        hipLaunchKernelGGL(overlay_kernel<false>, grid, block, 0, s, masks, frames, tables, overlay, H, W, wq, num_colors, ignore_index);
    return launch_status();
}

extern "C" int hs_upsample_overlay_fwd(const float* x, int32_t batch, int32_t channels, int32_t Hi, int32_t Wi, int32_t Ho, int32_t Wo,
                                       const uint8_t* frames, int32_t layout, const float* tables, int32_t num_colors,
                                       int32_t ignore_index, uint8_t* mask, uint8_t* overlay, void* stream) {
    if (!x || !frames || !mask || !overlay || batch <= 0 || channels <= 0 || Hi <= 0 || Wi <= 0 || Ho <= 0 || Wo <= 0) return HS_ERR_BAD_ARG;
    if (!overlay_args_ok(layout, tables, num_colors)) return HS_ERR_BAD_ARG;
    if (channels > 256) return HS_ERR_UNSUPPORTED;           // uint8 class indices
    hipStream_t s = (hipStream_t)stream;
    const bool hwc = layout == HS_LAYOUT_HWC;
    if (is_exact2x(Hi, Wi, Ho, Wo)) {            // the form hs_upsample_argmax_fwd takes for this shape: same masks
        if ((reinterpret_cast<uintptr_t>(mask) & 3) != 0) return HS_ERR_UNSUPPORTED;      // it stores the masks as dwords
        const size_t n2 = (size_t)batch * Hi * (Wi / 2) * 4;         // 4 lanes per 2x4 output block
        const dim3 grid((unsigned)((n2 + OVL_THREADS - 1) / OVL_THREADS)), block(OVL_THREADS);
        if (hwc) hipLaunchKernelGGL(upsample2x_overlay_kernel<true>, grid, block, 0, s, x, batch, channels, Hi, Wi, frames, tables, num_colors, ignore_index, mask, overlay);
        else hipLaunchKernelGGL(upsample2x_overlay_kernel<false>, grid, block, 0, s, x, batch, channels, Hi, Wi, frames, tables, num_colors, ignore_index, mask, overlay);
        return launch_status();
    }
    const size_t n = (size_t)batch * Ho * ((Wo + 3) / 4);
    const dim3 grid((unsigned)((n + OVL_THREADS - 1) / OVL_THREADS)), block(OVL_THREADS);
    const float sy = (float)Hi / (float)Ho, sx = (float)Wi / (float)Wo;
    if (hwc) hipLaunchKernelGGL(upsample_overlay_kernel<true>, grid, block, 0, s, x, batch, channels, Hi, Wi, Ho, Wo, sy, sx, frames, tables, num_colors, ignore_index, mask, overlay);
    else hipLaunchKernelGGL(upsample_overlay_kernel<false>, grid, block, 0, s, x, batch, channels, Hi, Wi, Ho, Wo, sy, sx, frames, tables, num_colors, ignore_index, mask, overlay);
    return launch_status();
}

extern "C" int hs_upsample2_overlay_fwd(const float* x, int32_t batch, int32_t channels, int32_t Hi, int32_t Wi, int32_t Hm, int32_t Wm,
                                        int32_t Ho, int32_t Wo, const uint8_t* frames, int32_t layout, const float* tables,
                                        int32_t num_colors, int32_t ignore_index, uint8_t* mask, uint8_t* overlay, void* stream) {
    if (!x || !frames || !mask || !overlay || batch <= 0 || channels <= 0 || Hi <= 0 || Wi <= 0 || Hm <= 0 || Wm <= 0 || Ho <= 0 || Wo <= 0)
        return HS_ERR_BAD_ARG;
    if (!overlay_args_ok(layout, tables, num_colors)) return HS_ERR_BAD_ARG;
    if (channels > 256) return HS_ERR_UNSUPPORTED;           // uint8 class indices
    // int pixel indices inside a plane (the taps), an unsigned grid
    if ((long)Hi * Wi > 0x7fffffffL - 4096 || (long)Hm * Wm > 0x7fffffffL - 4096 || (long)Ho * Wo > 0x7fffffffL - 4096) return HS_ERR_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    const bool hwc = layout == HS_LAYOUT_HWC;
    if (is_exact2x(Hi, Wi, Hm, Wm) && is_exact2x(Hm, Wm, Ho, Wo)) {       // the form hs_upsample2_confusion_fwd takes for this pair: same masks
        if ((reinterpret_cast<uintptr_t>(mask) & 3) != 0) return HS_ERR_UNSUPPORTED;      // it stores the masks as dwords
        const size_t n2 = (size_t)batch * Hi * (Wi / 2) * 4;         // 4 lanes per 4x8 output block
        const size_t nb = (n2 + OVL_THREADS - 1) / OVL_THREADS;
        if (nb > 0x7fffffffu) return HS_ERR_UNSUPPORTED;
        const dim3 grid((unsigned)nb), block(OVL_THREADS);
        if (hwc) hipLaunchKernelGGL(upsample2x2x_overlay_kernel<true>, grid, block, 0, s, x, batch, channels, Hi, Wi, frames, tables, num_colors, ignore_index, mask, overlay);
        else hipLaunchKernelGGL(upsample2x2x_overlay_kernel<false>, grid, block, 0, s, x, batch, channels, Hi, Wi, frames, tables, num_colors, ignore_index, mask, overlay);
        return launch_status();
    }
    const size_t n = (size_t)batch * Ho * ((Wo + 3) / 4);
    const size_t nb = (n + OVL_THREADS - 1) / OVL_THREADS;
    if (nb > 0x7fffffffu) return HS_ERR_UNSUPPORTED;
    const dim3 grid((unsigned)nb), block(OVL_THREADS);
    const Stages2 st = stages2(Hi, Wi, Hm, Wm, Ho, Wo);
    if (hwc) hipLaunchKernelGGL(upsample2_overlay_kernel<true>, grid, block, 0, s, x, batch, channels, st, frames, tables, num_colors, ignore_index, mask, overlay);
    else hipLaunchKernelGGL(upsample2_overlay_kernel<false>, grid, block, 0, s, x, batch, channels, st, frames, tables, num_colors, ignore_index, mask, overlay);
    return launch_status();
}
