// Flip and pyramid inference merged in the forward's last launch (the reference's HyperGen.forward for a list input,
// hyperseg_v1_0.py:71-91): every pass of the decoder hands over the INPUT of its final resize, and one launch makes, per output pixel and
// class, what the composed route makes with one resize per pass, one flip and one max per entry, one resize per smaller entry and the fold:
//   value of a pass at (ym, xm) of its entry = hs_upsample_bilinear_fwd(x -> (Hm, Wm)) there (stage_tap / tap_value of hs_upsample_taps.h:
//       that entry's bits), a flipped pass read at column Wm - 1 - xm (what torch.flip of the resized map holds), x itself where Hi == Hm;
//   value of an entry = the max over its passes, at the entry's resolution;
//   an entry of another size than (Ho, Wo) is resized to it: the max is taken at each of the four mid taps BEFORE this second interpolation
//       (it is not linear), then the second stage in bilinear2_row4's operation order, its indices clamped in mid space;
//   fold in list order: out = (p + out) * 0.5, or max(p, out).
// Inputs are finite (max is fmaxf: a NaN would not propagate as torch.max's does).
// Mapping: rows of four (hs::item_rows4), one workgroup of 512 threads per CU grid-striding over its image as the scoring kernels do; the class
// loop sits inside the thread in chunks of TTA_CC classes with a running arg-max.  Registers: the taps of a pass depend on the pixel and the
// pass, not on the class, and 8 passes x 15 taps do not fit; what is live instead is ONE mid point of ONE pass at a time -- its two taps, made
// once per chunk and used by the chunk's TTA_CC classes (4 loads each, TTA_CC x 4 in flight) -- beside the chunk's fold (TTA_CC x 4), the entry's
// values (TTA_CC x 4) and the four mid maxima of a pixel (TTA_CC x 4).  The pass and entry loops are wave-uniform (the table is a kernel argument).
// Sinks, any of: fp32 logits, uint8 masks (lowest index wins a tie), (target, prediction) counts by hs_eval_count.h's LDS histogram.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "hyperseg_hip.h"
#include "hs_common.h"
#include "hs_upsample_taps.h"
#include "hs_eval_count.h"

namespace hs {

constexpr int TTA_MAX_PASSES = HS_TTA_MAX_PASSES;
constexpr int TTA_CC = 5;                        // classes per chunk: 19 classes = 4 chunks

// One pass as the kernel reads it; `same`: its entry lives at (Ho, Wo) (no second stage), `identity`: x is at (Hm, Wm) already.
struct TtaPass {
    const float* x;
    int Hi, Wi, Hm, Wm;
    int flipped, identity, same, exact1, exact2;
    float sy1, sx1, sy2, sx2;
};
// Passes sorted by entry: entry e = passes [begin[e], begin[e + 1]).
struct TtaTable {
    TtaPass pass[TTA_MAX_PASSES];
    int begin[TTA_MAX_PASSES + 1];
    int entries;
};

// m[u] = value of the entry (passes [p0, p1) of `tab`) at (ym, xm) of its own resolution, for classes c0 + u (clamped to C - 1) of image b.
__device__ __forceinline__ void entry_at(const TtaTable& tab, int p0, int p1, size_t b, int C, int c0, int ym, int xm, float (&m)[TTA_CC]) {
#pragma unroll 1
    for (int pi = p0; pi < p1; ++pi) {                          // (uniform)
        const TtaPass& p = tab.pass[pi];
        const int xe = p.flipped ? p.Wm - 1 - xm : xm;
        const size_t plane = (size_t)p.Hi * p.Wi;
        const float* __restrict__ xb = p.x + b * C * plane;
        float v[TTA_CC];
        if (p.identity) {
#pragma unroll
            for (int u = 0; u < TTA_CC; ++u) v[u] = xb[(size_t)min(c0 + u, C - 1) * plane + (size_t)ym * p.Wi + xe];
        } else {
            const Tap ty = stage_tap(ym, p.exact1 != 0, p.sy1, p.Hi);
            const Tap tx = stage_tap(xe, p.exact1 != 0, p.sx1, p.Wi);
#pragma unroll
            for (int u = 0; u < TTA_CC; ++u) v[u] = tap_value(xb + (size_t)min(c0 + u, C - 1) * plane, p.Wi, ty, tx);
        }
#pragma unroll
        for (int u = 0; u < TTA_CC; ++u) m[u] = pi == p0 ? v[u] : fmaxf(m[u], v[u]);
    }
}

template <typename TT>
__global__ __launch_bounds__(EVAL_THREADS)
void tta_merge_kernel(TtaTable tab, int C, int Ho, int Wo, int gather_max, const TT* __restrict__ target, int n,
                      unsigned long long* __restrict__ out, long out_image_stride, uint8_t* __restrict__ mask, float* __restrict__ logits,
                      int vec, int vec_logits) {
    extern __shared__ unsigned hist[];
    const int nn = n * n, lane = threadIdx.x & 63;
    const bool count = target != nullptr;                        // (uniform)
    if (count) hist_zero(hist, nn);
    const size_t b = blockIdx.y;
    const int wq = (Wo + 3) / 4;
    const int items = Ho * wq;
    for (int base = blockIdx.x * EVAL_THREADS; base < items; base += gridDim.x * EVAL_THREADS) {      // wave-uniform trip count
        const Item it = item_rows4(base, items, wq);
        const bool live = it.live;
        const int q = it.q, yo = it.y;
        float best[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        int idx[4] = {0, 0, 0, 0};
#pragma unroll 1
        for (int c0 = 0; c0 < C; c0 += TTA_CC) {
            float acc[TTA_CC][4];
#pragma unroll 1
            for (int e = 0; e < tab.entries; ++e) {              // (uniform)
                const int p0 = tab.begin[e], p1 = tab.begin[e + 1];
                const TtaPass& lead = tab.pass[p0];
                float ev[TTA_CC][4];
                if (lead.same) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        float m[TTA_CC];
                        entry_at(tab, p0, p1, b, C, c0, yo, min(4 * q + i, Wo - 1), m);
#pragma unroll
                        for (int u = 0; u < TTA_CC; ++u) ev[u][i] = m[u];
                    }
                } else {
                    const Tap ty2 = stage_tap(yo, lead.exact2 != 0, lead.sy2, lead.Hm);
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const Tap tx2 = stage_tap(min(4 * q + i, Wo - 1), lead.exact2 != 0, lead.sx2, lead.Wm);
                        float m00[TTA_CC], m01[TTA_CC], m10[TTA_CC], m11[TTA_CC];
                        entry_at(tab, p0, p1, b, C, c0, ty2.i0, tx2.i0, m00);
                        entry_at(tab, p0, p1, b, C, c0, ty2.i0, tx2.i1, m01);
                        entry_at(tab, p0, p1, b, C, c0, ty2.i1, tx2.i0, m10);
                        entry_at(tab, p0, p1, b, C, c0, ty2.i1, tx2.i1, m11);
#pragma unroll
                        for (int u = 0; u < TTA_CC; ++u) {       // bilinear2_row4's order
                            const float top = tx2.l0 * m00[u] + tx2.l1 * m01[u];
                            const float bot = tx2.l0 * m10[u] + tx2.l1 * m11[u];
                            ev[u][i] = ty2.l0 * top + ty2.l1 * bot;
                        }
                    }
                }
#pragma unroll
                for (int u = 0; u < TTA_CC; ++u)
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        acc[u][i] = e == 0 ? ev[u][i] : gather_max ? fmaxf(ev[u][i], acc[u][i]) : (ev[u][i] + acc[u][i]) * 0.5f;
            }
#pragma unroll
            for (int u = 0; u < TTA_CC; ++u) {
                const int c = c0 + u;
                if (c < C) {                                     // (uniform)
                    if (logits != nullptr && live) {
                        float* dst = logits + ((b * C + c) * Ho + yo) * Wo + 4 * q;
                        if (vec_logits) {
                            *reinterpret_cast<float4*>(dst) = make_float4(acc[u][0], acc[u][1], acc[u][2], acc[u][3]);
                        } else {
                            for (int i = 0; i < 4 && 4 * q + i < Wo; ++i) dst[i] = acc[u][i];
                        }
                    }
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        if (c == 0 || acc[u][i] > best[i]) { best[i] = acc[u][i]; idx[i] = c; }      // strictly greater: the first maximum
                }
            }
        }
        const size_t at = (b * Ho + yo) * Wo + 4 * q;
        if (mask != nullptr && live) {
            if (vec) {
                *reinterpret_cast<uchar4*>(mask + at) = make_uchar4(idx[0], idx[1], idx[2], idx[3]);
            } else {
                for (int i = 0; i < 4 && 4 * q + i < Wo; ++i) mask[at + i] = (uint8_t)idx[i];
            }
        }
        if (count) {
            TT tv[4];
            if (vec) {
                load4(target + at, tv);
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) tv[i] = target[at + (4 * q + i < Wo ? i : 0)];
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
                count_key(hist, (live && 4 * q + i < Wo) ? pair_key<TT>(tv[i], idx[i], n) : -1, lane);
        }
    }
    if (count) hist_flush(hist, nn, out + b * out_image_stride);
}

}  // namespace hs

using namespace hs;

extern "C" int hs_tta_merge_fwd(const hs_tta_pass* passes, int32_t n_passes, int32_t batch, int32_t channels, int32_t gather_max,
                                const void* target, int32_t target_dtype, int32_t target_h, int32_t target_w, int32_t num_classes,
                                int32_t per_image, int64_t* confusion, uint8_t* mask, float* logits, void* stream) {
    if (!passes || n_passes <= 0 || batch <= 0 || channels <= 0) return HS_ERR_BAD_ARG;
    if (n_passes > TTA_MAX_PASSES) return HS_ERR_UNSUPPORTED;
    const bool count = target != nullptr;
    if (count != (confusion != nullptr) || (!count && !mask && !logits)) return HS_ERR_BAD_ARG;      // a sink to write
    TtaTable tab = {};
    const int Ho = passes[0].Hm, Wo = passes[0].Wm;
    int entries = 0;
    for (int i = 0; i < n_passes; ++i) {
        const hs_tta_pass& p = passes[i];
        if (!eval_shape_given(p.x, batch, channels, p.Hi, p.Wi, p.Hm, p.Wm, Ho, Wo)) return HS_ERR_BAD_ARG;
        // sorted by entry, entries 0, 1, ... without a gap, one size per entry
        if (p.entry != entries - 1) {
            if (p.entry != entries) return HS_ERR_BAD_ARG;
            tab.begin[entries++] = i;
        } else if (p.Hm != passes[i - 1].Hm || p.Wm != passes[i - 1].Wm) {
            return HS_ERR_BAD_ARG;
        }
    }
    tab.begin[entries] = n_passes;
    tab.entries = entries;
    if (count) {
        if (!eval_storage_ok(target_dtype) || num_classes <= 0 || channels > num_classes) return HS_ERR_BAD_ARG;
        if (num_classes > 256) return HS_ERR_BAD_ARG;                                         // uint8 class indices
        if (num_classes > EVAL_MAX_CLASSES) return HS_ERR_UNSUPPORTED;
        if (target_h != Ho || target_w != Wo) return HS_ERR_UNSUPPORTED;                      // scored at entry 0's size only
    }
    if (channels > 256) return HS_ERR_UNSUPPORTED;                                            // as hs_upsample_argmax_fwd
    for (int i = 0; i < n_passes; ++i) {
        const hs_tta_pass& p = passes[i];
        if (!eval_shape_fits(batch, p.Hm, p.Wm, Ho, Wo) || (long)p.Hi * p.Wi > 0x7fffffffL - 4096) return HS_ERR_UNSUPPORTED;
        const Stages2 s = stages2(p.Hi, p.Wi, p.Hm, p.Wm, Ho, Wo);
        tab.pass[i] = {p.x, p.Hi, p.Wi, p.Hm, p.Wm, p.flipped != 0, p.Hi == p.Hm && p.Wi == p.Wm, p.Hm == Ho && p.Wm == Wo,
                       s.exact1, s.exact2, s.sy1, s.sx1, s.sy2, s.sx2};
    }
    const Hist h = eval_hist(num_classes, per_image, confusion);
    const int dtype = count ? target_dtype : HS_EVAL_U8;                                      // nothing counted: the uint8 instantiation, a null pointer
    const int vec = (Wo & 3) == 0 && (!count || aligned_to(target, dtype == HS_EVAL_U8 ? 4 : 16)) && (!mask || aligned_to(mask, 4));
    const int vec_logits = (Wo & 3) == 0 && logits && aligned_to(logits, 16);
    with_target(dtype, target, [&](auto t) {
        hipLaunchKernelGGL(tta_merge_kernel<pointee<decltype(t)>>, eval_grid_rows4(Ho, Wo, batch), dim3(EVAL_THREADS), h.lds, (hipStream_t)stream,
                           tab, channels, Ho, Wo, gather_max != 0, t, h.n, h.out, h.stride, mask, logits, vec, vec_logits);
    });
    return launch_status();
}
