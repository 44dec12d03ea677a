// The per-pixel code of torchvision's ColorJitter with Pillow's bytes, shared by the launch over whole frames (hs_jitter.hip) and the
// launch over the top-left (h, w) region of each sample of a canvas (hs_augment_ragged.hip): the record of a sample, the four
// operations on a thread's 4 pixels in registers, the hue route's LDS tables.  The arithmetic is specified in
// hyperseg_amd/utils/jitter.py and described at the top of hs_jitter.hip; what the launches differ in -- which pixels a thread owns and
// how many pixels the contrast mean is taken over -- stays with each kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "hyperseg_hip.h"

namespace hs {

constexpr int JT_BRIGHTNESS = 1, JT_CONTRAST = 2, JT_SATURATION = 3, JT_HUE = 4;      // operation codes of a record's order
constexpr int JT_WORDS = HS_JITTER_TABLE_WORDS;
constexpr int JT_MEAN_BLOCKS = 1024;           // workgroups per image of the mean pass, at most (grid-stride beyond)
constexpr int JT_MAX_DIM = 1 << 19;            // H and W; keeps a mean-pass thread below 2^20 pixels

using f32x4 = __attribute__((ext_vector_type(4))) float;

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

}  // namespace hs
