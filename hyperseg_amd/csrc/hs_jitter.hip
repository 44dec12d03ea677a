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

namespace hs {

constexpr int JT_BRIGHTNESS = 1, JT_CONTRAST = 2, JT_SATURATION = 3, JT_HUE = 4;      // operation codes of a record's order
constexpr int JT_WORDS = HS_JITTER_TABLE_WORDS;
constexpr int JT_MEAN_BLOCKS = 1024;           // workgroups per image of the mean pass, at most (grid-stride beyond)
constexpr int JT_MAX_DIM = 1 << 19;            // H and W; keeps a mean-pass thread below 2^20 pixels

using f32x4 = __attribute__((ext_vector_type(4))) float;

struct JitterArgs {
    const uint8_t* x; void* y; const float* norm; const int32_t* table; unsigned long long* sums;
    long n;                                    // pixels per image
};

struct JitterRec { unsigned order; float alpha[3]; unsigned shift, present; };

struct HueTabs {
    double s255[256];                          // double(S) / 255.0
    float frac[256];                           // float32(hd - floor(hd)), hd = double(H) * 6.0 / 255.0
    int sector[256];                           // floor(hd) mod 6
};

__device__ __forceinline__ JitterRec jitter_record(const int32_t* __restrict__ table, size_t b) {
    const int32_t* __restrict__ t = table + b * JT_WORDS;
    JitterRec r;
    r.order = (unsigned)t[0];
    r.alpha[0] = __int_as_float(t[1]); r.alpha[1] = __int_as_float(t[2]); r.alpha[2] = __int_as_float(t[3]);
    r.shift = (unsigned)t[4] & 255u;
    r.present = (unsigned)t[5];
    return r;
}

__device__ __forceinline__ bool jitter_has(const JitterRec& r, int op) { return (r.present >> op) & 1u; }

// every thread of a 256-thread workgroup fills its entry; the caller puts a barrier behind it
__device__ __forceinline__ void hue_tabs_fill(HueTabs& tabs, int tid) {
    const double hd = (double)tid * 6.0 / 255.0, i = floor(hd);
    tabs.frac[tid] = (float)(hd - i);
    tabs.sector[tid] = (int)i % 6;             // H = 255: hd = 6.0, sector 0 with a zero fraction
    tabs.s255[tid] = (double)tid / 255.0;
}

__device__ __forceinline__ int jitter_gray(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16; }

// Image.blend: fmaxf / fminf also turn a NaN (only a caller's own table can hold one) into a byte
__device__ __forceinline__ int jitter_blend(int a, int b, float alpha) {
    const float t = __fadd_rn((float)a, __fmul_rn(alpha, (float)(b - a)));
    return (int)fminf(fmaxf(t, 0.0f), 255.0f);
}

__device__ __forceinline__ int jitter_clip8(int v) { return min(max(v, 0), 255); }

// C's round() of x >= 0, then clip8
__device__ __forceinline__ int jitter_round8(double x) {
    const double fl = floor(x);
    return jitter_clip8((int)fl + (x - fl >= 0.5 ? 1 : 0));
}

__device__ __forceinline__ void jitter_rgb_to_hsv(int r, int g, int b, int& H, int& S, int& V) {
    const int maxc = max(r, max(g, b)), minc = min(r, min(g, b));
    V = maxc; H = 0; S = 0;
    if (maxc != minc) {
        const float cr = (float)(maxc - minc);
        const float s = __fdiv_rn(cr, (float)maxc);
        const float rc = __fdiv_rn((float)(maxc - r), cr), gc = __fdiv_rn((float)(maxc - g), cr), bc = __fdiv_rn((float)(maxc - b), cr);
        float h;
        if (r == maxc) h = __fsub_rn(bc, gc);
        else if (g == maxc) h = (float)((2.0 + (double)rc) - (double)bc);
        else h = (float)((4.0 + (double)gc) - (double)rc);
        const double hd = (double)h / 6.0 + 1.0;                   // in [5/6, 7/6]: fmod(hd, 1.0) is hd - floor(hd), exactly
        h = (float)(hd - floor(hd));
        H = jitter_clip8((int)((double)h * 255.0));
        S = jitter_clip8((int)((double)s * 255.0));
    }
}

__device__ __forceinline__ void jitter_hsv_to_rgb(int H, int S, int V, const HueTabs& tabs, int& r, int& g, int& b) {
    r = g = b = V;
    if (S != 0) {
        const double sd = tabs.s255[S], vd = (double)V;
        const double fs = (double)(float)(sd * (double)tabs.frac[H]);
        const int p = jitter_round8(vd * (1.0 - sd)), q = jitter_round8(vd * (1.0 - fs)), t = jitter_round8(vd * ((1.0 - sd) + fs));
        switch (tabs.sector[H]) {
            case 0: g = t; b = p; break;
            case 1: r = q; b = p; break;
            case 2: r = p; b = t; break;
            case 3: r = p; g = q; break;
            case 4: r = t; g = p; break;
            default: g = p; b = q; break;
        }
    }
}

// The record's operations on a thread's 4 pixels, in order: the operation is chosen once (uniform), its 4 pixels are independent work.
// UNTIL_CONTRAST: stop in front of contrast (the mean pass; the caller has checked that the record names it); otherwise contrast
// blends against m.
template <bool UNTIL_CONTRAST>
__device__ __forceinline__ void jitter_ops(const JitterRec& rec, const HueTabs& tabs, int m, int (&v)[3][4]) {
#pragma unroll 1
    for (int k = 0; k < 4; ++k) {
        const int op = (int)((rec.order >> (4 * k)) & 15u);
        if (op == JT_BRIGHTNESS || (op == JT_CONTRAST && !UNTIL_CONTRAST)) {
            const int a = op == JT_CONTRAST ? m : 0;
            const float alpha = op == JT_CONTRAST ? rec.alpha[1] : rec.alpha[0];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int c = 0; c < 3; ++c) v[c][i] = jitter_blend(a, v[c][i], alpha);
        } else if (op == JT_SATURATION) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int l = jitter_gray(v[0][i], v[1][i], v[2][i]);
#pragma unroll
                for (int c = 0; c < 3; ++c) v[c][i] = jitter_blend(l, v[c][i], rec.alpha[2]);
            }
        } else if (op == JT_HUE) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                int H, S, V;
                jitter_rgb_to_hsv(v[0][i], v[1][i], v[2][i], H, S, V);
                jitter_hsv_to_rgb((H + (int)rec.shift) & 255, S, V, tabs, v[0][i], v[1][i], v[2][i]);
            }
        } else {
            return;                                                // contrast in the mean pass; 0 ends the order; so does any other code
        }
    }
}

// are an image's rows of 4 pixels dword-aligned?  img: the image's first byte (its first plane's for 'chw')
template <bool HWC>
__device__ __forceinline__ bool jitter_u8_vec(const uint8_t* img, long n) {
    return (reinterpret_cast<uintptr_t>(img) & 3) == 0 && (HWC || (n & 3) == 0);
}

// pixels p0 .. p0 + cnt - 1 (cnt in 1..4) of one image -> v[channel][i]; entries past cnt repeat pixel p0
template <bool HWC>
__device__ __forceinline__ void jitter_load4(const uint8_t* __restrict__ img, long n, long p0, int cnt, bool vec, int (&v)[3][4]) {
    if (vec && cnt == 4) {
        if constexpr (HWC) {
            const unsigned* __restrict__ w = reinterpret_cast<const unsigned*>(img + 3 * p0);      // r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3
            const unsigned w0 = w[0], w1 = w[1], w2 = w[2];
            v[0][0] = w0 & 255u; v[1][0] = (w0 >> 8) & 255u; v[2][0] = (w0 >> 16) & 255u; v[0][1] = w0 >> 24;
            v[1][1] = w1 & 255u; v[2][1] = (w1 >> 8) & 255u; v[0][2] = (w1 >> 16) & 255u; v[1][2] = w1 >> 24;
            v[2][2] = w2 & 255u; v[0][3] = (w2 >> 8) & 255u; v[1][3] = (w2 >> 16) & 255u; v[2][3] = w2 >> 24;
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const unsigned w = *reinterpret_cast<const unsigned*>(img + c * n + p0);
                v[c][0] = w & 255u; v[c][1] = (w >> 8) & 255u; v[c][2] = (w >> 16) & 255u; v[c][3] = w >> 24;
            }
        }
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const long p = p0 + (i < cnt ? i : 0);
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c][i] = HWC ? img[3 * p + c] : img[c * n + p];
        }
    }
}

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
