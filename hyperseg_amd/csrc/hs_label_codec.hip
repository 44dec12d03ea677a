// A dataset's label encoding on whole label images, one launch (the rules and the codec's layout: hs_label_codec.h): the last per-pixel
// step the reference's loaders do on the host before anything of this package starts -- Cityscapes' id table
// (hyperseg/datasets/cityscapes.py:210-211) and CamVid's twelve full-image colour compares (hyperseg/datasets/camvid.py:93-100).
//
// hs_label_encode_fwd: blockIdx.y = image, a workgroup of 256 threads stages the codec into LDS once and streams its pixels:
//   * table, uint8 in: 16 consecutive pixels per thread -- one 16-byte load where the address is 16-aligned, byte loads otherwise and
//     for the image's last partial run;
//   * table, int64 in: the same 16 pixels as eight 16-byte loads (8-byte loads where the address is not 16-aligned);
//   * colours: 4 consecutive pixels = 12 bytes per thread, three 4-byte loads where the address is 4-aligned, else byte by byte; the
//     compare loop walks the list in LDS from the last entry down and leaves at the first hit;
//   * stores: one 4-byte store per 4 uint8 results (bytes where the address is not 4-aligned), 16-byte stores for int64 results (8-byte
//     where it is not 16-aligned).
// A stream: every input byte is read once and every output byte written once; neighbouring lanes cover neighbouring 16- / 12-byte runs.
// No atomics, no status word, nothing read back: capturable.  Every access is guarded by the image's pixel count.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "hyperseg_hip.h"
#include "hs_common.h"
#include "hs_label_codec.h"

namespace hs {

constexpr int LE_THREADS = 256;

using le_u32x4 = __attribute__((ext_vector_type(4))) uint32_t;
using le_i64x2 = __attribute__((ext_vector_type(2))) long long;

// N results (a multiple of 4) to consecutive labels
template <int N>
__device__ __forceinline__ void store_run(uint8_t* __restrict__ dst, const int (&v)[N]) {
    if (aligned_to(dst, 4)) {
#pragma unroll
        for (int k = 0; k < N; k += 4)
            *reinterpret_cast<uint32_t*>(dst + k) = (uint32_t)v[k] | (uint32_t)v[k + 1] << 8 | (uint32_t)v[k + 2] << 16 | (uint32_t)v[k + 3] << 24;
    } else {
#pragma unroll
        for (int k = 0; k < N; ++k) dst[k] = (uint8_t)v[k];
    }
}
template <int N>
__device__ __forceinline__ void store_run(int64_t* __restrict__ dst, const int (&v)[N]) {
    if (aligned_to(dst, 16)) {
#pragma unroll
        for (int k = 0; k < N; k += 2) *reinterpret_cast<le_i64x2*>(dst + k) = le_i64x2{v[k], v[k + 1]};
    } else {
#pragma unroll
        for (int k = 0; k < N; ++k) dst[k] = v[k];
    }
}

constexpr int LE_TABLE_PX = 16, LE_COLOR_PX = 4;

// 16 raw ids -> 16 table bytes
__device__ __forceinline__ void table_run(const uint8_t* __restrict__ src, const uint32_t* lds, int (&v)[LE_TABLE_PX]) {
    if (aligned_to(src, 16)) {
        const le_u32x4 q = *reinterpret_cast<const le_u32x4*>(src);
#pragma unroll
        for (int k = 0; k < LE_TABLE_PX; ++k) v[k] = codec_table(lds, (int)(q[k >> 2] >> (8 * (k & 3)) & 255u));
    } else {
#pragma unroll
        for (int k = 0; k < LE_TABLE_PX; ++k) v[k] = codec_table(lds, (int)src[k]);
    }
}
__device__ __forceinline__ void table_run(const int64_t* __restrict__ src, const uint32_t* lds, int (&v)[LE_TABLE_PX]) {
    if (aligned_to(src, 16)) {
#pragma unroll
        for (int k = 0; k < LE_TABLE_PX; k += 2) {
            const le_i64x2 q = *reinterpret_cast<const le_i64x2*>(src + k);
            v[k] = codec_table(lds, q[0]); v[k + 1] = codec_table(lds, q[1]);
        }
    } else {
#pragma unroll
        for (int k = 0; k < LE_TABLE_PX; ++k) v[k] = codec_table(lds, (long long)src[k]);
    }
}

template <typename TI, typename TO>
__global__ __launch_bounds__(LE_THREADS)
void label_encode_table_kernel(const TI* __restrict__ x, const int32_t* __restrict__ words, TO* __restrict__ y, long pixels) {
    __shared__ uint32_t codec[codec_lds_words<CODEC_TABLE>()];
    codec_stage<CODEC_TABLE>(codec, CodecArgs{words, 256, 0}, (int)threadIdx.x);
    const long first = ((long)blockIdx.x * LE_THREADS + threadIdx.x) * LE_TABLE_PX;
    if (first >= pixels) return;
    const TI* __restrict__ src = x + (size_t)blockIdx.y * pixels + first;
    TO* __restrict__ dst = y + (size_t)blockIdx.y * pixels + first;
    if (first + LE_TABLE_PX <= pixels) {
        int v[LE_TABLE_PX];
        table_run(src, codec, v);
        store_run(dst, v);
    } else {
        for (int k = 0; k < (int)(pixels - first); ++k) {
            if constexpr (sizeof(TI) == 1) dst[k] = (TO)codec_table(codec, (int)src[k]);
            else dst[k] = (TO)codec_table(codec, (long long)src[k]);
        }
    }
}

template <typename TO>
__global__ __launch_bounds__(LE_THREADS)
void label_encode_colors_kernel(const uint8_t* __restrict__ x, const int32_t* __restrict__ words, int n, int unmatched, TO* __restrict__ y,
                                long pixels) {
    __shared__ uint32_t codec[codec_lds_words<CODEC_COLORS>()];
    codec_stage<CODEC_COLORS>(codec, CodecArgs{words, n, unmatched}, (int)threadIdx.x);
    const long first = ((long)blockIdx.x * LE_THREADS + threadIdx.x) * LE_COLOR_PX;
    if (first >= pixels) return;
    const uint8_t* __restrict__ src = x + ((size_t)blockIdx.y * pixels + first) * 3;
    TO* __restrict__ dst = y + (size_t)blockIdx.y * pixels + first;
    if (first + LE_COLOR_PX <= pixels) {
        uint32_t rgb[LE_COLOR_PX];
        if (aligned_to(src, 4)) {
            const uint32_t w0 = reinterpret_cast<const uint32_t*>(src)[0], w1 = reinterpret_cast<const uint32_t*>(src)[1],
                           w2 = reinterpret_cast<const uint32_t*>(src)[2];
            rgb[0] = w0 & 0xffffffu;
            rgb[1] = (w0 >> 24 | w1 << 8) & 0xffffffu;
            rgb[2] = (w1 >> 16 | w2 << 16) & 0xffffffu;
            rgb[3] = w2 >> 8;
        } else {
#pragma unroll
            for (int k = 0; k < LE_COLOR_PX; ++k) rgb[k] = (uint32_t)src[3 * k] | (uint32_t)src[3 * k + 1] << 8 | (uint32_t)src[3 * k + 2] << 16;
        }
        int v[LE_COLOR_PX];
#pragma unroll
        for (int k = 0; k < LE_COLOR_PX; ++k) v[k] = codec_color(codec, n, unmatched, rgb[k]);
        store_run(dst, v);
    } else {
        for (int k = 0; k < (int)(pixels - first); ++k)
            dst[k] = (TO)codec_color(codec, n, unmatched, (uint32_t)src[3 * k] | (uint32_t)src[3 * k + 1] << 8 | (uint32_t)src[3 * k + 2] << 16);
    }
}

}  // namespace hs

using namespace hs;

extern "C" int hs_label_encode_fwd(const void* x, int32_t in_kind, int32_t batch, int32_t H, int32_t W, const int32_t* codec_words,
                                   int32_t codec_kind, int32_t n, int32_t unmatched, void* y, int32_t out_dtype, void* stream) {
    if (!x || !y || batch <= 0 || H <= 0 || W <= 0) return HS_ERR_BAD_ARG;
    if (out_dtype != HS_EVAL_U8 && out_dtype != HS_EVAL_I64) return HS_ERR_BAD_ARG;
    if (const int st = codec_check(codec_words, codec_kind, in_kind, n, unmatched)) return st;
    if (batch > 65535) return HS_ERR_UNSUPPORTED;
    const long pixels = (long)H * W;
    const int per_thread = codec_kind == HS_CODEC_TABLE ? LE_TABLE_PX : LE_COLOR_PX;
    const long per_group = (long)LE_THREADS * per_thread;
    const long groups = (pixels + per_group - 1) / per_group;
    if (groups > 0x7fffffffL) return HS_ERR_UNSUPPORTED;
    const dim3 grid((unsigned)groups, (unsigned)batch), block(LE_THREADS);
    hipStream_t s = (hipStream_t)stream;
    const bool u8_out = out_dtype == HS_EVAL_U8;
#define HS_ENCODE_TABLE(TI, TO) hipLaunchKernelGGL((label_encode_table_kernel<TI, TO>), grid, block, 0, s, static_cast<const TI*>(x), codec_words, \
                                                   static_cast<TO*>(y), pixels)
#define HS_ENCODE_COLORS(TO) hipLaunchKernelGGL((label_encode_colors_kernel<TO>), grid, block, 0, s, static_cast<const uint8_t*>(x), codec_words, \
                                                (int)n, (int)unmatched, static_cast<TO*>(y), pixels)
    if (codec_kind == HS_CODEC_COLORS) { if (u8_out) HS_ENCODE_COLORS(uint8_t); else HS_ENCODE_COLORS(int64_t); }
    else if (in_kind == HS_EVAL_U8) { if (u8_out) HS_ENCODE_TABLE(uint8_t, uint8_t); else HS_ENCODE_TABLE(uint8_t, int64_t); }
    else { if (u8_out) HS_ENCODE_TABLE(int64_t, uint8_t); else HS_ENCODE_TABLE(int64_t, int64_t); }
#undef HS_ENCODE_TABLE
#undef HS_ENCODE_COLORS
    return launch_status();
}
