// torchvision's ColorJitter on uint8 RGB frames, on the device, with Pillow's bytes: what the reference's HyperSeg-S and VOC train
// configs run on a host thread at the end of their image chain (configs/train/cityscapes_efficientnet_b1_hyperseg-s.py:22-24).  On a
// PIL image ColorJitter is a drawn order of up to four Pillow operations, each reading and writing a uint8 RGB image; the arithmetic
// of each is restated in hyperseg_amd/utils/jitter.py, which is the specification and the CPU implementation this file is held to:
//   blend(a, b, alpha) = clip(float32(a) + float32(alpha * float32(b - a)), 0, 255) truncated -- two roundings, never an FMA (the
//   library is built with -ffp-contract=off, and the two operations are spelt __fmul_rn / __fadd_rn here);
//   brightness: blend(0, x, f);  saturation: blend(L(pixel), x, f);  contrast: blend(m, x, f) with ONE m per image, int(sum L / count
//   + 0.5) in float64 over the image as it stands when contrast runs;  L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16;
//   hue: RGB -> HSV (float32 with two float64 steps), H += shift mod 256, HSV -> RGB (float64) -- also when the shift is 0.
// What varies per sample is data: one 8-word record per sample in a device table (hyperseg_hip.h), so a captured graph replays with
// whatever the table holds at that moment.  Every branch on the record is uniform over a workgroup (blockIdx.y = sample).
//
// hs_color_jitter_fwd, per call: a clear of the per-sample sums (8 bytes each), the mean pass, the apply pass -- or the apply pass
// alone when the caller passes no sums (no record names contrast).
//   * mean pass: workgroups of samples without contrast leave at once.  The others apply the operations that precede contrast in
//     registers, form L and add it up as INTEGERS: 32 bits per thread (at most 2^20 pixels of <= 255 each), 64 bits from the wave
//     reduction on, one 64-bit atomic add per workgroup.  Integer addition commutes: the sum is the same in every run whatever order
//     the workgroups arrive in.  The host never reads it.
//   * apply pass: every pixel is read once, all operations run in registers (m from the sum, in float64), and the byte is stored in
//     the input's layout or -- through InputNorm's table in LDS (hs_ingest.h) -- as float32 planar.
// The operations know nothing of rows, so an image is a flat run of H W pixels: a thread owns 4 consecutive ones -- 'hwc': 12 bytes
// as three dwords, 'chw': one dword per plane, where the image's base is 4-byte aligned ('chw': and H W a multiple of 4, so that the
// planes are too); byte accesses otherwise and on the last H W mod 4 pixels.  Stores mirror the loads; the float form stores 16 bytes
// per plane where the destination is 16-byte aligned.  The hue route's per-H and per-S float64 divisions are tabulated in LDS by the
// workgroup itself (256 entries each, the same expressions as the specification's), which leaves one float64 division per pixel.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "hyperseg_hip.h"
#include "hs_common.h"
#include "hs_ingest.h"
#include "hs_jitter_px.h"

namespace hs {

struct JitterArgs {
    const uint8_t* x; void* y; const float* norm; const int32_t* table; unsigned long long* sums;
    long n;                                    // pixels per image
};

template <bool HWC>
__global__ __launch_bounds__(256)
void jitter_mean_kernel(const JitterArgs a) {
    __shared__ HueTabs tabs;
    __shared__ unsigned long long wave_sum[4];
    const size_t b = blockIdx.y;
    const JitterRec rec = jitter_record(a.table, b);
    if (!jitter_has(rec, JT_CONTRAST)) return;                     // uniform: the whole workgroup leaves
    const int tid = (int)threadIdx.x;
    if (jitter_has(rec, JT_HUE)) hue_tabs_fill(tabs, tid);
    __syncthreads();
    const uint8_t* __restrict__ img = a.x + b * 3 * (size_t)a.n;
    const bool vec = jitter_u8_vec<HWC>(img, a.n);
    const long groups = (a.n + 3) >> 2;
    unsigned acc = 0;                                              // < 2^20 pixels of <= 255 each
    for (long grp = (long)blockIdx.x * 256 + tid; grp < groups; grp += (long)gridDim.x * 256) {
        const long p0 = grp << 2;
        const int cnt = (int)min(4L, a.n - p0);
        int v[3][4];
        jitter_load4<HWC>(img, a.n, p0, cnt, vec, v);
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

template <bool HWC, bool NORM>
__global__ __launch_bounds__(256)
void jitter_apply_kernel(const JitterArgs a) {
    __shared__ HueTabs tabs;
    __shared__ float tab[NORM ? INGEST_TABLE_FLOATS : 1];
    const size_t b = blockIdx.y;
    const JitterRec rec = jitter_record(a.table, b);
    const int tid = (int)threadIdx.x;
    if constexpr (NORM) ingest_table_to_lds(a.norm, tab, tid);
    if (jitter_has(rec, JT_HUE)) hue_tabs_fill(tabs, tid);
    __syncthreads();
    int m = 0;
    if (a.sums && jitter_has(rec, JT_CONTRAST)) m = jitter_clip8((int)((double)a.sums[b] / (double)a.n + 0.5));
    const long p0 = ((long)blockIdx.x * 256 + tid) << 2;
    if (p0 >= a.n) return;
    const int cnt = (int)min(4L, a.n - p0);
    const uint8_t* __restrict__ img = a.x + b * 3 * (size_t)a.n;
    int v[3][4];
    jitter_load4<HWC>(img, a.n, p0, cnt, jitter_u8_vec<HWC>(img, a.n), v);
    jitter_ops<false>(rec, tabs, m, v);

    if constexpr (NORM) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float* __restrict__ d = static_cast<float*>(a.y) + (b * 3 + c) * (size_t)a.n + p0;
            float o[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) o[i] = ingest_dequant(tab, c, (unsigned)v[c][i]);
            if (cnt == 4 && (reinterpret_cast<uintptr_t>(d) & 15) == 0) {
                *reinterpret_cast<f32x4*>(d) = f32x4{o[0], o[1], o[2], o[3]};
            } else {
                for (int i = 0; i < cnt; ++i) d[i] = o[i];
            }
        }
    } else {
        uint8_t* __restrict__ out = static_cast<uint8_t*>(a.y) + b * 3 * (size_t)a.n;
        const bool vec = cnt == 4 && jitter_u8_vec<HWC>(out, a.n);
        if constexpr (HWC) {
            if (vec) {
                unsigned* __restrict__ w = reinterpret_cast<unsigned*>(out + 3 * p0);
                w[0] = (unsigned)v[0][0] | (unsigned)v[1][0] << 8 | (unsigned)v[2][0] << 16 | (unsigned)v[0][1] << 24;
                w[1] = (unsigned)v[1][1] | (unsigned)v[2][1] << 8 | (unsigned)v[0][2] << 16 | (unsigned)v[1][2] << 24;
                w[2] = (unsigned)v[2][2] | (unsigned)v[0][3] << 8 | (unsigned)v[1][3] << 16 | (unsigned)v[2][3] << 24;
            } else {
                for (int i = 0; i < cnt; ++i)
#pragma unroll
                    for (int c = 0; c < 3; ++c) out[3 * (p0 + i) + c] = (uint8_t)v[c][i];
            }
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                uint8_t* __restrict__ d = out + c * a.n + p0;
                if (vec) {
                    *reinterpret_cast<unsigned*>(d) = (unsigned)v[c][0] | (unsigned)v[c][1] << 8 | (unsigned)v[c][2] << 16 | (unsigned)v[c][3] << 24;
                } else {
                    for (int i = 0; i < cnt; ++i) d[i] = (uint8_t)v[c][i];
                }
            }
        }
    }
}

}  // namespace hs

using namespace hs;

extern "C" int hs_color_jitter_fwd(const uint8_t* x, int32_t layout, int32_t batch, int32_t H, int32_t W, const int32_t* table,
                                   uint64_t* sums, const float* norm_table, void* y, void* stream) {
    if (!x || !y || !table || batch <= 0 || H <= 0 || W <= 0) return HS_ERR_BAD_ARG;
    if (layout != HS_LAYOUT_HWC && layout != HS_LAYOUT_CHW) return HS_ERR_BAD_ARG;
    if (batch > 65535 || H > JT_MAX_DIM || W > JT_MAX_DIM) return HS_ERR_UNSUPPORTED;
    JitterArgs a;
    a.x = x; a.y = y; a.norm = norm_table; a.table = table; a.sums = reinterpret_cast<unsigned long long*>(sums);
    a.n = (long)H * W;
    const long blocks = ((a.n + 3) / 4 + 255) / 256;               // <= 2^28
    hipStream_t s = (hipStream_t)stream;
    const bool hwc = layout == HS_LAYOUT_HWC;
    const dim3 block(256);
    if (sums) {
        hipError_t e = hipMemsetAsync(sums, 0, sizeof(uint64_t) * (size_t)batch, s);
        if (e != hipSuccess) return (int)e;
        const dim3 grid((unsigned)(blocks < JT_MEAN_BLOCKS ? blocks : JT_MEAN_BLOCKS), (unsigned)batch);
        if (hwc) hipLaunchKernelGGL(jitter_mean_kernel<true>, grid, block, 0, s, a);
        else hipLaunchKernelGGL(jitter_mean_kernel<false>, grid, block, 0, s, a);
    }
    const dim3 grid((unsigned)blocks, (unsigned)batch);
    if (norm_table) {
        if (hwc) hipLaunchKernelGGL((jitter_apply_kernel<true, true>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((jitter_apply_kernel<false, true>), grid, block, 0, s, a);
    } else {
        if (hwc) hipLaunchKernelGGL((jitter_apply_kernel<true, false>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((jitter_apply_kernel<false, false>), grid, block, 0, s, a);
    }
    return launch_status();
}
