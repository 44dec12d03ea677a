// Served confidence maps: beside the uint8 arg-max mask, the soft-max probability of the winning class of every output pixel --
// softmax(v)[argmax] = 1 / sum_c exp(v_c - v_max) -- either from finished fp32 logits (hs_confidence_fwd: the composed route's kernel and
// the yardstick) or as the epilogue of the final upsample + arg-max launch, where every class score of a pixel passes through a register
// anyway (hs_upsample_confidence_fwd; hs_upsample2_confidence_fwd over two composed resizes).  The full-resolution logits are never
// written by the fused entries.
//
// Shape: one thread owns 4 consecutive output pixels of a row and walks the classes in ascending order, one Conf (m, s, idx:
// hs_confidence.h) per pixel -- 12 registers beside the taps.  The class scores come from hs_upsample_taps.h and nothing of the resize is
// restated here: a stage in the exact-2x form takes up2x_tap, whose taps bilinear_row4 / bilinear2_row4 combine in up2x_block's operation
// order, so a score is what hs_upsample_bilinear_fwd stores for that shape, in either of its forms.  The sum is taken in ONE order by
// ONE function (confidence_step) in all three kernels: that is why they agree to the bit, and why the classes are not split among
// lanes the way argmax2x_block splits them (a split sum is another rounding).
// Stores: the mask and a uint8 confidence as one dword, an fp32 confidence as one 16-byte store, where the thread's 4 pixels exist and the
// address is aligned; single elements otherwise -- any base pointer, any width.  Ordinary vector stores only: no atomics, nothing waits
// on another workgroup, nothing is read back by the host.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "hyperseg_hip.h"
#include "hs_common.h"
#include "hs_upsample_taps.h"
#include "hs_confidence.h"

namespace hs {

constexpr int CONF_THREADS = 256;

// ---- where a thread's four class scores come from: operator()(c, o) fills o[0..3] with class c's scores of the thread's pixels
// (a pixel past the row's end repeats the row's last one: computed, never stored)

// finished logits (B, C, H, W): `off` = the first pixel's offset inside a class plane, step[i] = pixel i's distance from it
struct ScoresMem {
    const float* __restrict__ xb; size_t plane, off; int step[4]; bool vec;
    __device__ __forceinline__ void operator()(int c, float (&o)[4]) const {
        const float* __restrict__ p = xb + (size_t)c * plane + off;
        if (vec) {
            const float4 v = *reinterpret_cast<const float4*>(p);
            o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) o[i] = p[step[i]];
        }
    }
};
// one resize, either form
struct ScoresRow4 {
    const float* __restrict__ xb; int Hi, Wi; Row4 t;
    __device__ __forceinline__ void operator()(int c, float (&o)[4]) const { bilinear_row4(xb + (size_t)c * Hi * Wi, Wi, t, o); }
};
// two composed resizes, each in either form
struct ScoresRow4x2 {
    const float* __restrict__ xb; int Hi, Wi; Row4x2 t;
    __device__ __forceinline__ void operator()(int c, float (&o)[4]) const { bilinear2_row4(xb + (size_t)c * Hi * Wi, Wi, t, o); }
};

// Row4 of one stage in the form hs_upsample_bilinear_fwd takes for it (row4_taps is the general form's).
__device__ __forceinline__ Row4 row4_stage_taps(int yo, int q, int Hi, int Wi, int Wo, bool exact2x, float scale_y, float scale_x) {
    Row4 t;
    t.ty = stage_tap(yo, exact2x, scale_y, Hi);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int xo = 4 * q + i;
        t.tx[i] = stage_tap(xo < Wo ? xo : Wo - 1, exact2x, scale_x, Wi);
    }
    return t;
}

// The ascending pass over the classes: UNROLL class trips in flight.
template <int UNROLL, typename Scores>
__device__ __forceinline__ void confidence_row4(const Scores& scores, int C, bool floor_start, Conf (&st)[4]) {
    float o[4];
    scores(0, o);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (floor_start) { st[i] = conf_floor(); confidence_step(st[i], o[i], 0); }
        else st[i] = conf_first(o[i]);
    }
#pragma unroll UNROLL
    for (int c = 1; c < C; ++c) {
        scores(c, o);
#pragma unroll
        for (int i = 0; i < 4; ++i) confidence_step(st[i], o[i], c);
    }
}

// Pixels pix .. pix + live - 1 (1 <= live <= 4) of image-major (B, Ho, Wo) outputs: mask and confidence.  OUT: float | uint8_t.
template <typename OUT>
__device__ __forceinline__ void confidence_store4(const Conf (&st)[4], int live, uint8_t* __restrict__ mdst, OUT* __restrict__ cdst,
                                                  float threshold, int fill) {
    float conf[4];
    uint8_t lab[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        conf[i] = confidence_value(st[i]);
        lab[i] = confidence_label(st[i].idx, conf[i], threshold, fill);
    }
    if (live == 4 && aligned_to(mdst, 4)) {
        *reinterpret_cast<uchar4*>(mdst) = make_uchar4(lab[0], lab[1], lab[2], lab[3]);
    } else {
        for (int i = 0; i < live; ++i) mdst[i] = lab[i];
    }
    if constexpr (sizeof(OUT) == 4) {
        if (live == 4 && aligned_to(cdst, 16)) {
            *reinterpret_cast<float4*>(cdst) = make_float4(conf[0], conf[1], conf[2], conf[3]);
        } else {
            for (int i = 0; i < live; ++i) cdst[i] = conf[i];
        }
    } else {
        if (live == 4 && aligned_to(cdst, 4)) {
            *reinterpret_cast<uchar4*>(cdst) = make_uchar4(confidence_u8(conf[0]), confidence_u8(conf[1]), confidence_u8(conf[2]), confidence_u8(conf[3]));
        } else {
            for (int i = 0; i < live; ++i) cdst[i] = confidence_u8(conf[i]);
        }
    }
}

// thread e of the launch -> (image b, row yo, quad q) of (B, Ho, ceil(Wo / 4)); false: a surplus thread
__device__ __forceinline__ bool conf_item(int B, int Ho, int Wo, size_t& b, int& yo, int& q) {
    const int wq = (Wo + 3) / 4;
    const size_t n = (size_t)B * Ho * wq;
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return false;
    q = (int)(e % wq);
    const size_t r = e / wq;
    yo = (int)(r % Ho);
    b = r / Ho;
    return true;
}

template <typename OUT>
__global__ __launch_bounds__(CONF_THREADS)
void confidence_kernel(const float* __restrict__ x, int B, int C, int H, int W, int vec, float threshold, int fill,
                       uint8_t* __restrict__ mask, OUT* __restrict__ conf) {
    size_t b; int yo, q;
    if (!conf_item(B, H, W, b, yo, q)) return;
    const size_t plane = (size_t)H * W, pix = (size_t)yo * W + 4 * q;
    const int live = min(4, W - 4 * q);
    ScoresMem sc;
    sc.xb = x + b * C * plane; sc.plane = plane; sc.off = pix; sc.vec = vec != 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) sc.step[i] = i < live ? i : live - 1;
    Conf st[4];
    confidence_row4<4>(sc, C, false, st);
    confidence_store4<OUT>(st, live, mask + b * plane + pix, conf + b * plane + pix, threshold, fill);
}

template <typename OUT>
__global__ __launch_bounds__(CONF_THREADS)
void upsample_confidence_kernel(const float* __restrict__ x, int B, int C, int Hi, int Wi, int Ho, int Wo, int exact2x, float scale_y,
                                float scale_x, float threshold, int fill, uint8_t* __restrict__ mask, OUT* __restrict__ conf) {
    size_t b; int yo, q;
    if (!conf_item(B, Ho, Wo, b, yo, q)) return;
    ScoresRow4 sc;
    sc.xb = x + b * C * Hi * Wi; sc.Hi = Hi; sc.Wi = Wi;
    sc.t = row4_stage_taps(yo, q, Hi, Wi, Wo, exact2x != 0, scale_y, scale_x);
    Conf st[4];
    confidence_row4<4>(sc, C, exact2x != 0, st);             // the start of the arg-max form this shape takes (hs_confidence.h)
    const size_t plane = (size_t)Ho * Wo, pix = (size_t)yo * Wo + 4 * q;
    confidence_store4<OUT>(st, min(4, Wo - 4 * q), mask + b * plane + pix, conf + b * plane + pix, threshold, fill);
}

template <typename OUT>
__global__ __launch_bounds__(CONF_THREADS)
void upsample2_confidence_kernel(const float* __restrict__ x, int B, int C, Stages2 s, float threshold, int fill,
                                 uint8_t* __restrict__ mask, OUT* __restrict__ conf) {
    size_t b; int yo, q;
    if (!conf_item(B, s.Ho, s.Wo, b, yo, q)) return;
    ScoresRow4x2 sc;
    sc.xb = x + b * C * s.Hi * s.Wi; sc.Hi = s.Hi; sc.Wi = s.Wi;
    sc.t = row4x2_taps(yo, q, s);
    Conf st[4];
    confidence_row4<1>(sc, C, s.exact1 != 0 && s.exact2 != 0, st);
    const size_t plane = (size_t)s.Ho * s.Wo, pix = (size_t)yo * s.Wo + 4 * q;
    confidence_store4<OUT>(st, min(4, s.Wo - 4 * q), mask + b * plane + pix, conf + b * plane + pix, threshold, fill);
}

// What the three entries ask of their common operands; the grid of one thread per 4 pixels of a row.
static int confidence_args(const void* x, int batch, int channels, int H0, int W0, int H1, int W1, int H2, int W2, int conf_dtype, int fill,
                           const void* mask, const void* conf, unsigned& blocks) {
    if (!x || !mask || !conf || batch <= 0 || channels <= 0 || H0 <= 0 || W0 <= 0 || H1 <= 0 || W1 <= 0 || H2 <= 0 || W2 <= 0) return HS_ERR_BAD_ARG;
    if ((conf_dtype != HS_CONF_F32 && conf_dtype != HS_CONF_U8) || fill < 0 || fill > 255) return HS_ERR_BAD_ARG;
    if (channels > 256) return HS_ERR_UNSUPPORTED;                          // uint8 class indices
    if ((long)H2 * W2 > 0x7fffffffL - 4096 || (long)H1 * W1 > 0x7fffffffL - 4096 || (long)H0 * W0 > 0x7fffffffL - 4096) return HS_ERR_UNSUPPORTED;
    const size_t n = (size_t)batch * H2 * ((W2 + 3) / 4);
    const size_t nb = (n + CONF_THREADS - 1) / CONF_THREADS;
    if (nb > 0x7fffffffu) return HS_ERR_UNSUPPORTED;
    blocks = (unsigned)nb;
    return HS_OK;
}

// calls f with `conf` as a pointer of its storage type (`using OUT = pointee<decltype(c)>;`)
template <typename F> __attribute__((always_inline)) inline void with_conf(int conf_dtype, void* conf, F&& f) {
    if (conf_dtype == HS_CONF_F32) f((float*)conf); else f((uint8_t*)conf);
}

}  // namespace hs

using namespace hs;

extern "C" int hs_confidence_fwd(const float* logits, int32_t batch, int32_t channels, int32_t H, int32_t W, int32_t conf_dtype,
                                 float threshold, int32_t fill, uint8_t* mask, void* conf, void* stream) {
    unsigned blocks = 0;
    const int st = confidence_args(logits, batch, channels, H, W, H, W, H, W, conf_dtype, fill, mask, conf, blocks);
    if (st != HS_OK) return st;
    const int vec = (W & 3) == 0 && (reinterpret_cast<uintptr_t>(logits) & 15) == 0;
    with_conf(conf_dtype, conf, [&](auto c) {
        hipLaunchKernelGGL(confidence_kernel<pointee<decltype(c)>>, dim3(blocks), dim3(CONF_THREADS), 0, (hipStream_t)stream, logits, batch,
                           channels, H, W, vec, threshold, fill, mask, c);
    });
    return launch_status();
}

extern "C" int hs_upsample_confidence_fwd(const float* x, int32_t batch, int32_t channels, int32_t Hi, int32_t Wi, int32_t Ho, int32_t Wo,
                                          int32_t conf_dtype, float threshold, int32_t fill, uint8_t* mask, void* conf, void* stream) {
    unsigned blocks = 0;
    const int st = confidence_args(x, batch, channels, Hi, Wi, Ho, Wo, Ho, Wo, conf_dtype, fill, mask, conf, blocks);
    if (st != HS_OK) return st;
    const int exact = is_exact2x(Hi, Wi, Ho, Wo);
    with_conf(conf_dtype, conf, [&](auto c) {
        hipLaunchKernelGGL(upsample_confidence_kernel<pointee<decltype(c)>>, dim3(blocks), dim3(CONF_THREADS), 0, (hipStream_t)stream, x, batch,
                           channels, Hi, Wi, Ho, Wo, exact, (float)Hi / (float)Ho, (float)Wi / (float)Wo, threshold, fill, mask, c);
    });
    return launch_status();
}

extern "C" int hs_upsample2_confidence_fwd(const float* x, int32_t batch, int32_t channels, int32_t Hi, int32_t Wi, int32_t Hm, int32_t Wm,
                                           int32_t Ho, int32_t Wo, int32_t conf_dtype, float threshold, int32_t fill, uint8_t* mask,
                                           void* conf, void* stream) {
    unsigned blocks = 0;
    const int st = confidence_args(x, batch, channels, Hi, Wi, Hm, Wm, Ho, Wo, conf_dtype, fill, mask, conf, blocks);
    if (st != HS_OK) return st;
    const Stages2 s = stages2(Hi, Wi, Hm, Wm, Ho, Wo);
    with_conf(conf_dtype, conf, [&](auto c) {
        hipLaunchKernelGGL(upsample2_confidence_kernel<pointee<decltype(c)>>, dim3(blocks), dim3(CONF_THREADS), 0, (hipStream_t)stream, x, batch,
                           channels, s, threshold, fill, mask, c);
    });
    return launch_status();
}
