// uint8 frames -> the float32 (B, 3, H, W) image the encoder reads: the reference's ToTensor + Normalize
// (hyperseg/datasets/seg_transforms.py -> torchvision to_tensor / normalize, defaults test.py:62-63) and, for 'hwc' frames, the
// transpose to planar layout, as ONE launch on the device.  A pure memory mover -- 1 byte in, 4 bytes out per value:
//   * one thread owns 4 consecutive pixels of a row: for HWC that is 12 contiguous bytes (three dword loads when the row's address is
//     4-byte aligned), for CHW one dword per plane; byte loads otherwise (any base pointer, any width);
//   * the (3, 256) table (hs_ingest.h) lives in LDS; the value IS the table entry, so the result is bit-identical to the host transform;
//   * one 16-byte store per output plane where the destination is aligned and the 4 pixels exist, element stores on the tail.
// blockIdx.y = frame (batch <= 65535), blockIdx.x over H * ceil(W / 4) items.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "hyperseg_hip.h"
#include "hs_common.h"
#include "hs_ingest.h"

namespace hs {

using f32x4 = __attribute__((ext_vector_type(4))) float;

// 4 consecutive bytes at p (n of them exist): one dword when aligned and whole, byte loads otherwise
__device__ __forceinline__ void ingest_load4(const uint8_t* __restrict__ p, int n, unsigned (&v)[4]) {
    if (n == 4 && (reinterpret_cast<uintptr_t>(p) & 3) == 0) {
        const unsigned w = *reinterpret_cast<const unsigned*>(p);
        v[0] = w & 255u; v[1] = (w >> 8) & 255u; v[2] = (w >> 16) & 255u; v[3] = w >> 24;
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = p[i < n ? i : 0];
    }
}

template <bool HWC>
__global__ __launch_bounds__(256)
void image_ingest_kernel(const uint8_t* __restrict__ x, const float* __restrict__ table, float* __restrict__ y, int H, int W, int wq) {
    __shared__ float tab[INGEST_TABLE_FLOATS];
    ingest_table_to_lds(table, tab, (int)threadIdx.x);
    __syncthreads();
    const long item = (long)blockIdx.x * 256 + threadIdx.x;
    if (item >= (long)H * wq) return;
    const int yy = (int)(item / wq), x0 = 4 * (int)(item - (long)yy * wq);
    const int n = min(4, W - x0);                               // >= 1
    const size_t b = blockIdx.y, plane = (size_t)H * W, pix = (size_t)yy * W + x0;
    unsigned v[INGEST_CHANNELS][4];
    if constexpr (HWC) {
        const uint8_t* __restrict__ p = x + (b * plane + pix) * 3;
        if (n == 4 && (reinterpret_cast<uintptr_t>(p) & 3) == 0) {
            // r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3
            const unsigned w0 = reinterpret_cast<const unsigned*>(p)[0], w1 = reinterpret_cast<const unsigned*>(p)[1],
                           w2 = reinterpret_cast<const unsigned*>(p)[2];
            v[0][0] = w0 & 255u; v[1][0] = (w0 >> 8) & 255u; v[2][0] = (w0 >> 16) & 255u; v[0][1] = w0 >> 24;
            v[1][1] = w1 & 255u; v[2][1] = (w1 >> 8) & 255u; v[0][2] = (w1 >> 16) & 255u; v[1][2] = w1 >> 24;
            v[2][2] = w2 & 255u; v[0][3] = (w2 >> 8) & 255u; v[1][3] = (w2 >> 16) & 255u; v[2][3] = w2 >> 24;
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int c = 0; c < INGEST_CHANNELS; ++c) v[c][i] = p[3 * (i < n ? i : 0) + c];
        }
    } else {
#pragma unroll
        for (int c = 0; c < INGEST_CHANNELS; ++c) ingest_load4(x + (b * INGEST_CHANNELS + c) * plane + pix, n, v[c]);
    }
#pragma unroll
    for (int c = 0; c < INGEST_CHANNELS; ++c) {
        float o[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] = ingest_dequant(tab, c, v[c][i]);
        float* __restrict__ d = y + (b * INGEST_CHANNELS + c) * plane + pix;
        if (n == 4 && (reinterpret_cast<uintptr_t>(d) & 15) == 0) {
            *reinterpret_cast<f32x4*>(d) = f32x4{o[0], o[1], o[2], o[3]};
        } else {
            for (int i = 0; i < n; ++i) d[i] = o[i];
        }
    }
}

}  // namespace hs

using namespace hs;

extern "C" int hs_image_ingest_fwd(const uint8_t* x, int32_t layout, int32_t batch, int32_t channels, int32_t H, int32_t W,
                                   const float* table, float* y, void* stream) {
    if (!x || !table || !y || batch <= 0 || channels <= 0 || H <= 0 || W <= 0) return HS_ERR_BAD_ARG;
    if (layout != HS_LAYOUT_HWC && layout != HS_LAYOUT_CHW) return HS_ERR_BAD_ARG;
    if (channels != INGEST_CHANNELS || batch > 65535) return HS_ERR_UNSUPPORTED;
    const int wq = (W + 3) / 4;
    const long blocks = ((long)H * wq + 255) / 256;
    if (blocks > 0x7fffffffL) return HS_ERR_UNSUPPORTED;
    const dim3 grid((unsigned)blocks, (unsigned)batch), block(256);
    hipStream_t s = (hipStream_t)stream;
    if (layout == HS_LAYOUT_HWC) hipLaunchKernelGGL(image_ingest_kernel<true>, grid, block, 0, s, x, table, y, H, W, wq);
    else hipLaunchKernelGGL(image_ingest_kernel<false>, grid, block, 0, s, x, table, y, H, W, wq);
    return launch_status();
}
