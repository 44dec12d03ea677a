// The validation step's middle (hyperseg/train.py:118-126: loss = criterion(pred, target), then running_metrics.update(target,
// pred.argmax(1))) in ONE pass over each pixel's class scores: the per-pixel cross entropy that BootstrappedCrossEntropyLoss ranks, the
// class arg-max, and the (target, prediction) pair counted into the confusion matrix.
//   * hs_cross_entropy_score_fwd: from logits that exist in memory (training: backward needs them anyway);
//   * hs_upsample_ce_confusion_fwd: from the decoder's last-level output, resized in registers (validation, no_grad): the resized logits
//     never exist in memory.
// Loss bits are hs_cross_entropy_typed_fwd's (cross_entropy_kernel, hs_train_aux.hip): per pixel, in f32, fmaxf over the classes
// ascending, sum += expf(v - m) ascending, (logf(sum) + m) - x[t]; 0 where t == ignore_index or t is outside [0, C).  The build has
// -ffp-contract=off and no fast-math, so the restated arithmetic gives the same bits.  Masks are hs_upsample_argmax_fwd's / argmax(1)'s (the
// first maximum), counts hs_confusion_fwd's: every target in [0, n) is counted -- an in-range ignore_index too, with loss 0, as the
// reference's runningScore does not know ignore_index.
// Counting is hs_eval.hip's (hs_eval_count.h): a workgroup of 512 threads per CU grid-striding over its image (blockIdx.y), a per-workgroup
// n x n LDS histogram fed by count_key's ballot aggregation (wave-uniform trip counts), one flush of the non-zero bins per workgroup.  Not
// the loss launch's workgroup per 256 pixels: thousands of workgroups flushing a histogram each meet on a few bins (the note above
// cross_entropy_kernel: 38.5 us against 17).  No cross-workgroup waiting, no float atomics: the losses are plain stores.
// confusion == nullptr: nothing is counted (loss and masks only).
// The item of a thread in a pass of the resizing kernels' loops is hs_eval.hip's: item_rows4 / item_quad (hs_last_launch.h).
// Host side: three template fronts (one per entry and its weighted twin) over hs_eval.hip's launch front (hs_eval_count.h).
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdlib>
#include "hyperseg_hip.h"
#include "hs_common.h"
#include "hs_upsample_taps.h"
#include "hs_eval_count.h"

namespace hs {

// cross_entropy_kernel's live rule and result
__device__ __forceinline__ bool ce_live(long long t, long long ignore_index, int C) { return t != ignore_index && t >= 0 && t < C; }

// Logits in memory: one thread = one pixel per trip, its C logits HW elements apart (a wave reads C coalesced rows).  CF: the class count
// at compile time (the pixel's logits loaded once, all in flight together), 0 = any count (three passes), as cross_entropy_kernel.
// CW (W; here and in the two kernels below): class weights, nothing or the table (class_weight, hs_common.h) -- loss = w[t] * (the unweighted loss), cross_entropy_kernel<.., W>'s
// bits.  The table is gathered from memory per pixel, right after the target (a few cached lines): nothing is staged, no barrier is added.
template <typename T, int CF, typename... CW>
__global__ __launch_bounds__(EVAL_THREADS)
void ce_score_kernel(const T* __restrict__ x, const long long* __restrict__ target, int C, long hw, long long ignore_index,
                     float* __restrict__ loss, int n, unsigned long long* __restrict__ out, long out_image_stride, uint8_t* __restrict__ mask,
                     CW... cw) {
    constexpr bool W = sizeof...(CW) != 0;
    extern __shared__ unsigned hist[];
    const int nn = n * n, lane = threadIdx.x & 63;
    const bool count = out != nullptr;                           // (uniform)
    if (count) hist_zero(hist, nn);
    const long b = blockIdx.y;
    const T* __restrict__ xb = x + b * C * hw;
    for (long base = (long)blockIdx.x * EVAL_THREADS; base < hw; base += (long)gridDim.x * EVAL_THREADS) {      // wave-uniform trip count
        const long p0 = base + threadIdx.x;
        const bool here = p0 < hw;
        const long p = here ? p0 : hw - 1;                       // surplus lanes shadow the last pixel and store nothing
        const T* __restrict__ xp = xb + p;
        const long long t = target[b * hw + p];
        const bool live = ce_live(t, ignore_index, C);
        const float wt = class_weight(t, live, cw...);
        float value;
        int best_c = 0;
        if constexpr (CF > 0) {
            float v[CF];
#pragma unroll
            for (int c = 0; c < CF; ++c) v[c] = Store<T>::ld(xp, (long)c * hw);
            float m = v[0], best = v[0];
#pragma unroll
            for (int c = 1; c < CF; ++c) {
                m = fmaxf(m, v[c]);
                if (v[c] > best) { best = v[c]; best_c = c; }
            }
            float sum = 0.0f, xt = 0.0f;
#pragma unroll
            for (int c = 0; c < CF; ++c) {
                sum += expf(v[c] - m);
                xt = (c == (int)t) ? v[c] : xt;
            }
            value = live ? weighted<W>(wt, (logf(sum) + m) - xt) : 0.0f;
        } else {
            float m = Store<T>::ld(xp, 0), best = m;
            for (int c = 1; c < C; ++c) {
                const float v = Store<T>::ld(xp, (long)c * hw);
                m = fmaxf(m, v);
                if (v > best) { best = v; best_c = c; }
            }
            float sum = 0.0f;
            for (int c = 0; c < C; ++c) sum += expf(Store<T>::ld(xp, (long)c * hw) - m);
            value = live ? weighted<W>(wt, (logf(sum) + m) - Store<T>::ld(xp, (long)(live ? t : 0) * hw)) : 0.0f;
        }
        if (here) {
            loss[b * hw + p] = value;
            if (mask != nullptr) mask[b * hw + p] = (uint8_t)best_c;
        }
        if (count) count_key(hist, here ? pair_key<long long>(t, best_c, n) : -1, lane);
    }
    if (count) hist_flush(hist, nn, out + b * out_image_stride);
}

// argmax_row4 (hs_upsample_taps.h) handing out the maxima as well: the same loads, the same comparisons, so the same indices.  The
// strict maximum IS cross_entropy_kernel's fmaxf chain for finite scores (they differ in the sign of a zero maximum at most, which
// neither expf(v - m) nor logf(sum) + m shows).  Restated here, not factored out of argmax_row4.  Tried once with the three *_best
// functions moved to hs_upsample_taps.h (argmax_row4_best<UNROLL>) and the index-only forms calling them with a local array for the
// maxima: this file's 40 kernels and every argmax_row4 kernel came out instruction for instruction as before, but the index-only quad
// kernels did not (VGPRs / SGPRs, scratch 0 throughout; before -> after): upsample2x_confusion_kernel<u8> 138 / 79 -> 138 / 73,
// <i64> 136 / 79 -> 138 / 73; upsample2x2x_confusion_kernel<u8> 211 -> 199 VGPRs with 4909 -> 5015 instructions, <i64> 210 -> 199 with
// 4915 -> 5014; upsample2x_argmax_kernel 120 / 46 -> 120 / 40; upsample2x_overlay_kernel: same registers, 5 instructions fewer.  No
// occupancy step either way, but not the same figures, so the copies stay (profiles/last_launch_helpers_isa.txt).
__device__ __forceinline__ void argmax_row4_best(const float* __restrict__ xb, int C, int Hi, int Wi, const Row4& t, int (&idx)[4],
                                                 float (&best)[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) idx[i] = 0;
    bilinear_row4(xb, Wi, t, best);
#pragma unroll 4
    for (int c = 1; c < C; ++c) {
        float o[4];
        bilinear_row4(xb + (size_t)c * Hi * Wi, Wi, t, o);
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (o[i] > best[i]) { best[i] = o[i]; idx[i] = c; }
    }
}

// ... and argmax2x_block likewise: on return all four lanes of the quad hold the block's eight indices AND maxima.
__device__ __forceinline__ void argmax2x_block_best(const float* __restrict__ xb, int C, int Hi, int Wi, int yi, int q, int sub,
                                                    int (&idx0)[4], int (&idx1)[4], float (&best0)[4], float (&best1)[4]) {
    constexpr float NEG = -3.402823466e38f;
#pragma unroll
    for (int i = 0; i < 4; ++i) { best0[i] = best1[i] = NEG; idx0[i] = idx1[i] = sub; }
    for (int c0 = sub; c0 < C; c0 += 20) {
        float o0[5][4], o1[5][4];
#pragma unroll
        for (int u = 0; u < 5; ++u) {                        // 5 classes = 60 loads in flight
            const int c = min(c0 + 4 * u, C - 1);
            up2x_block(xb + (size_t)c * Hi * Wi, Hi, Wi, yi, q, o0[u], o1[u]);
        }
#pragma unroll
        for (int u = 0; u < 5; ++u) {
            const int c = c0 + 4 * u;
            if (c < C) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    if (o0[u][i] > best0[i]) { best0[i] = o0[u][i]; idx0[i] = c; }
                    if (o1[u][i] > best1[i]) { best1[i] = o1[u][i]; idx1[i] = c; }
                }
            }
        }
    }
#pragma unroll
    for (int m = 1; m <= 2; m <<= 1) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float v0 = __shfl_xor(best0[i], m, 64), v1 = __shfl_xor(best1[i], m, 64);
            const int j0 = __shfl_xor(idx0[i], m, 64), j1 = __shfl_xor(idx1[i], m, 64);
            if (v0 > best0[i] || (v0 == best0[i] && j0 < idx0[i])) { best0[i] = v0; idx0[i] = j0; }
            if (v1 > best1[i] || (v1 == best1[i] && j1 < idx1[i])) { best1[i] = v1; idx1[i] = j1; }
        }
    }
}

// General resize (any ratio, the identity included): upsample_confusion_kernel's mapping, one thread = 4 consecutive output pixels of a row,
// all C classes of them its own.  Two passes over the classes: the arg-max and the maxima, then -- the scores recomputed by the same
// operations, so the same bits; the loads hit the cache -- the exp-sum ascending and the target's score.
template <typename TT, typename... CW>
__global__ __launch_bounds__(EVAL_THREADS)
void upsample_ce_confusion_kernel(const float* __restrict__ x, int C, int Hi, int Wi, int Ho, int Wo, float scale_y, float scale_x,
                                  const TT* __restrict__ target, long long ignore_index, float* __restrict__ loss, int n,
                                  unsigned long long* __restrict__ out, long out_image_stride, uint8_t* __restrict__ mask, int vec,
                                  CW... cw) {
    constexpr bool W = sizeof...(CW) != 0;
    extern __shared__ unsigned hist[];
    const int nn = n * n, lane = threadIdx.x & 63;
    const bool count = out != nullptr;                           // (uniform)
    if (count) hist_zero(hist, nn);
    const size_t b = blockIdx.y;
    const int wq = (Wo + 3) / 4;
    const int items = Ho * wq;
    const size_t plane = (size_t)Hi * Wi;
    const float* __restrict__ xb = x + b * C * plane;
    for (int base = blockIdx.x * EVAL_THREADS; base < items; base += gridDim.x * EVAL_THREADS) {      // wave-uniform trip count
        const Item it = item_rows4(base, items, wq);
        const bool live = it.live;
        const int q = it.q, yo = it.y;
        const Row4 t = row4_taps(yo, q, Hi, Wi, Wo, scale_y, scale_x);
        int idx[4];
        float m[4];
        argmax_row4_best(xb, C, Hi, Wi, t, idx, m);
        const size_t at = (b * Ho + yo) * Wo + 4 * q;
        TT tv[4];
        if (vec) {
            load4(target + at, tv);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) tv[i] = target[at + (4 * q + i < Wo ? i : 0)];
        }
        float wt[4];
#pragma unroll
        for (int i = 0; i < 4; ++i)                              // (W: in flight with the second pass' loads)
            wt[i] = class_weight((long long)tv[i], ce_live((long long)tv[i], ignore_index, C), cw...);
        float sum[4] = {0.0f, 0.0f, 0.0f, 0.0f}, xt[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 2
        for (int c = 0; c < C; ++c) {
            float o[4];
            bilinear_row4(xb + (size_t)c * plane, Wi, t, o);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                sum[i] += expf(o[i] - m[i]);
                xt[i] = ((long long)tv[i] == (long long)c) ? o[i] : xt[i];
            }
        }
        float v[4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
            v[i] = ce_live((long long)tv[i], ignore_index, C) ? weighted<W>(wt[i], (logf(sum[i]) + m[i]) - xt[i]) : 0.0f;
        if (live) {
            if (vec) {
                *reinterpret_cast<float4*>(loss + at) = make_float4(v[0], v[1], v[2], v[3]);
                if (mask != nullptr) *reinterpret_cast<uchar4*>(mask + at) = make_uchar4(idx[0], idx[1], idx[2], idx[3]);
            } else {
                for (int i = 0; i < 4 && 4 * q + i < Wo; ++i) {
                    loss[at + i] = v[i];
                    if (mask != nullptr) mask[at + i] = (uint8_t)idx[i];
                }
            }
        }
        if (count) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                count_key(hist, (live && 4 * q + i < Wo) ? pair_key<TT>(tv[i], idx[i], n) : -1, lane);
        }
    }
    if (count) hist_flush(hist, nn, out + b * out_image_stride);
}

// argmax2_row4 (hs_upsample_taps.h) handing out the maxima as well, as argmax_row4_best does for the one-stage form -- for pixels I0 and
// I0 + 1 of the thread's four: the same loads, the same comparisons per pixel, so hs_upsample2_confusion_fwd's indices.  Two pixels per
// class loop, not four: the compiler hoists every load's 64-bit offset out of the loop (16 loads per pixel: argmax2_row4 alone takes 236
// VGPRs), and with the targets, weights, sums and target scores of this kernel beside them the four-pixel loops spill (13 to 32 VGPRs to
// scratch at the 256 that 512 threads allow).  Two loops of two pixels make each load once all the same.
template <int I0>
__device__ __forceinline__ void argmax2_row4_best(const float* __restrict__ xb, int C, size_t plane, int Wi, const Row4x2& t, int (&idx)[4],
                                                  float (&best)[4]) {
#pragma unroll
    for (int i = I0; i < I0 + 2; ++i) { idx[i] = 0; best[i] = bilinear2_at(xb, Wi, t, i); }
#pragma unroll 1
    for (int c = 1; c < C; ++c) {
        const float* __restrict__ pc = xb + (size_t)c * plane;
#pragma unroll
        for (int i = I0; i < I0 + 2; ++i) {
            const float o = bilinear2_at(pc, Wi, t, i);
            if (o > best[i]) { best[i] = o; idx[i] = c; }
        }
    }
}

// ... and the second pass for the same two pixels: the ascending exp-sum and the target's score, the scores recomputed by the same operations.
template <int I0, typename TT>
__device__ __forceinline__ void ce2_row4_sums(const float* __restrict__ xb, int C, size_t plane, int Wi, const Row4x2& t, const TT (&tv)[4],
                                              const float (&m)[4], float (&sum)[4], float (&xt)[4]) {
#pragma unroll 1
    for (int c = 0; c < C; ++c) {
        const float* __restrict__ pc = xb + (size_t)c * plane;
#pragma unroll
        for (int i = I0; i < I0 + 2; ++i) {
            const float o = bilinear2_at(pc, Wi, t, i);
            sum[i] += expf(o - m[i]);
            xt[i] = ((long long)tv[i] == (long long)c) ? o : xt[i];
        }
    }
}

// Two resizes composed in registers (x -> mid -> label: the decoder's final resize, then train.py:119-120's to the label's size), any
// first and any second stage: upsample2_confusion_kernel's mapping (hs_eval.hip), one thread = 4 consecutive label pixels of a row over a
// Row4x2, and upsample_ce_confusion_kernel's two passes over the classes -- bilinear2_row4 recomputed by the same operations in the second,
// so the same bits.  Neither the mid nor the label-size logits exist in memory.
template <typename TT, typename... CW>
__global__ __launch_bounds__(EVAL_THREADS)
void upsample2_ce_confusion_kernel(const float* __restrict__ x, int C, Stages2 s, const TT* __restrict__ target, long long ignore_index,
                                   float* __restrict__ loss, int n, unsigned long long* __restrict__ out, long out_image_stride,
                                   uint8_t* __restrict__ mask, int vec, CW... cw) {
    constexpr bool W = sizeof...(CW) != 0;
    extern __shared__ unsigned hist[];
    const int nn = n * n, lane = threadIdx.x & 63;
    const bool count = out != nullptr;                           // (uniform)
    if (count) hist_zero(hist, nn);
    const size_t b = blockIdx.y;
    const int Ho = s.Ho, Wo = s.Wo, wq = (Wo + 3) / 4;
    const int items = Ho * wq;
    const size_t plane = (size_t)s.Hi * s.Wi;
    const float* __restrict__ xb = x + b * C * plane;
    for (int base = blockIdx.x * EVAL_THREADS; base < items; base += gridDim.x * EVAL_THREADS) {      // wave-uniform trip count
        const Item it = item_rows4(base, items, wq);
        const bool live = it.live;
        const int q = it.q, yo = it.y;
        const Row4x2 t = row4x2_taps(yo, q, s);
        const size_t at = (b * Ho + yo) * Wo + 4 * q;
        TT tv[4];
        if (vec) {
            load4(target + at, tv);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) tv[i] = target[at + (4 * q + i < Wo ? i : 0)];
        }
        float wt[4];
#pragma unroll
        for (int i = 0; i < 4; ++i)                              // (W: in flight with the class loops' loads)
            wt[i] = class_weight((long long)tv[i], ce_live((long long)tv[i], ignore_index, C), cw...);
        int idx[4];
        float m[4], sum[4] = {0.0f, 0.0f, 0.0f, 0.0f}, xt[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        argmax2_row4_best<0>(xb, C, plane, s.Wi, t, idx, m);     // both passes of one pair, then the other's: its load offsets die in between
        ce2_row4_sums<0>(xb, C, plane, s.Wi, t, tv, m, sum, xt);
        argmax2_row4_best<2>(xb, C, plane, s.Wi, t, idx, m);
        ce2_row4_sums<2>(xb, C, plane, s.Wi, t, tv, m, sum, xt);
        float v[4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
            v[i] = ce_live((long long)tv[i], ignore_index, C) ? weighted<W>(wt[i], (logf(sum[i]) + m[i]) - xt[i]) : 0.0f;
        if (live) {
            if (vec) {
                *reinterpret_cast<float4*>(loss + at) = make_float4(v[0], v[1], v[2], v[3]);
                if (mask != nullptr) *reinterpret_cast<uchar4*>(mask + at) = make_uchar4(idx[0], idx[1], idx[2], idx[3]);
            } else {
                for (int i = 0; i < 4 && 4 * q + i < Wo; ++i) {
                    loss[at + i] = v[i];
                    if (mask != nullptr) mask[at + i] = (uint8_t)idx[i];
                }
            }
        }
        if (count) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                count_key(hist, (live && 4 * q + i < Wo) ? pair_key<TT>(tv[i], idx[i], n) : -1, lane);
        }
    }
    if (count) hist_flush(hist, nn, out + b * out_image_stride);
}

// lane J of every quad's value in all four of its lanes, on the DPP path (quad_perm [J, J, J, J]); all lanes present
template <int J>
__device__ __forceinline__ float quad_bcast(float v) {
    const int x = __float_as_int(v);
    return __int_as_float(__builtin_amdgcn_update_dpp(x, x, J * 0x55, 0xf, 0xf, false));
}

// One class of the exact-2x second pass: lane J of the quad made its block values (o0: upper row, o1: lower row); every lane takes the two
// it accounts for -- lane `sub`: row sub >> 1, columns 2 (sub & 1) and + 1 -- and adds class c to their sums.
template <int J>
__device__ __forceinline__ void ce2x_take(const float (&o0)[4], const float (&o1)[4], bool row1, bool right, int c, long long ta, long long tb,
                                          float ma, float mb, float& sa, float& sb, float& xa, float& xb) {
    float r0[4], r1[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) { r0[i] = quad_bcast<J>(o0[i]); r1[i] = quad_bcast<J>(o1[i]); }
    const float va = row1 ? (right ? r1[2] : r1[0]) : (right ? r0[2] : r0[0]);
    const float vb = row1 ? (right ? r1[3] : r1[1]) : (right ? r0[3] : r0[1]);
    sa += expf(va - ma);
    sb += expf(vb - mb);
    xa = (ta == (long long)c) ? va : xa;
    xb = (tb == (long long)c) ? vb : xb;
}

// Exact 2x: upsample2x_confusion_kernel's mapping, four consecutive lanes per 2 x 4 output block.  First pass: argmax2x_block's split of the
// classes over the quad, after which all four lanes hold the block's indices and maxima.  Second pass: a quad-tree sum would not be the
// sequential one, so the quad again makes four classes at a time (lane `sub`: class 4 g + sub, the same up2x_block), the values are
// exchanged within the quad (ce2x_take) and each lane runs the ascending exp-sum of the two pixels it also counts.
template <typename TT, typename... CW>
__global__ __launch_bounds__(EVAL_THREADS)
void upsample2x_ce_confusion_kernel(const float* __restrict__ x, int C, int Hi, int Wi, const TT* __restrict__ target, long long ignore_index,
                                    float* __restrict__ loss, int n, unsigned long long* __restrict__ out, long out_image_stride,
                                    uint8_t* __restrict__ mask, int vec, CW... cw) {
    constexpr bool W = sizeof...(CW) != 0;
    extern __shared__ unsigned hist[];
    const int nn = n * n, lane = threadIdx.x & 63;
    const bool count = out != nullptr;                           // (uniform)
    if (count) hist_zero(hist, nn);
    const size_t b = blockIdx.y;
    const int wq = Wi >> 1, Wo = 2 * Wi;
    const int items = Hi * wq;                                  // 2 x 4 output blocks of this image
    const int sub = (int)(threadIdx.x & 3);
    const bool row1 = (sub & 2) != 0, right = (sub & 1) != 0;
    const size_t plane = (size_t)Hi * Wi;
    const float* __restrict__ xb = x + b * C * plane;
    for (int base = blockIdx.x * (EVAL_THREADS / 4); base < items; base += gridDim.x * (EVAL_THREADS / 4)) {
        const Item it = item_quad(base, items, wq);             // (the quad exchanges: convergent)
        const bool live = it.live;
        const int q = it.q, yi = it.y;
        int idx0[4], idx1[4];
        float best0[4], best1[4];
        argmax2x_block_best(xb, C, Hi, Wi, yi, q, sub, idx0, idx1, best0, best1);
        const size_t at = (b * 2 * Hi + 2 * yi) * Wo + 4 * q;
        if (mask != nullptr && sub == 0 && live) {
            if (vec) {
                *reinterpret_cast<uchar4*>(mask + at) = make_uchar4(idx0[0], idx0[1], idx0[2], idx0[3]);
                *reinterpret_cast<uchar4*>(mask + at + Wo) = make_uchar4(idx1[0], idx1[1], idx1[2], idx1[3]);
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) { mask[at + i] = (uint8_t)idx0[i]; mask[at + Wo + i] = (uint8_t)idx1[i]; }
            }
        }
        const int pa = row1 ? (right ? idx1[2] : idx1[0]) : (right ? idx0[2] : idx0[0]);
        const int pb = row1 ? (right ? idx1[3] : idx1[1]) : (right ? idx0[3] : idx0[1]);
        const float ma = row1 ? (right ? best1[2] : best1[0]) : (right ? best0[2] : best0[0]);
        const float mb = row1 ? (right ? best1[3] : best1[1]) : (right ? best0[3] : best0[1]);
        const size_t mine = at + (row1 ? Wo : 0) + (right ? 2 : 0);
        TT tv[2];
        load2(target + mine, vec != 0, tv);
        const long long ta = (long long)tv[0], tb = (long long)tv[1];
        float wa = 1.0f, wb = 1.0f;
        if constexpr (W) {                                      // in flight with the second pass' loads
            wa = class_weight(ta, ce_live(ta, ignore_index, C), cw...);
            wb = class_weight(tb, ce_live(tb, ignore_index, C), cw...);
        }
        float sa = 0.0f, sb = 0.0f, xa = 0.0f, xb2 = 0.0f;
        for (int c0 = 0; c0 < C; c0 += 4) {                      // (uniform: every lane of the wave takes every trip and every branch below)
            float o0[4], o1[4];
            up2x_block(xb + (size_t)min(c0 + sub, C - 1) * plane, Hi, Wi, yi, q, o0, o1);
            ce2x_take<0>(o0, o1, row1, right, c0, ta, tb, ma, mb, sa, sb, xa, xb2);
            if (c0 + 1 < C) ce2x_take<1>(o0, o1, row1, right, c0 + 1, ta, tb, ma, mb, sa, sb, xa, xb2);
            if (c0 + 2 < C) ce2x_take<2>(o0, o1, row1, right, c0 + 2, ta, tb, ma, mb, sa, sb, xa, xb2);
            if (c0 + 3 < C) ce2x_take<3>(o0, o1, row1, right, c0 + 3, ta, tb, ma, mb, sa, sb, xa, xb2);
        }
        if (live) {
            loss[mine] = ce_live(ta, ignore_index, C) ? weighted<W>(wa, (logf(sa) + ma) - xa) : 0.0f;
            loss[mine + 1] = ce_live(tb, ignore_index, C) ? weighted<W>(wb, (logf(sb) + mb) - xb2) : 0.0f;
        }
        if (count) {
            count_key(hist, live ? pair_key<TT>(tv[0], pa, n) : -1, lane);
            count_key(hist, live ? pair_key<TT>(tv[1], pb, n) : -1, lane);
        }
    }
    if (count) hist_flush(hist, nn, out + b * out_image_stride);
}

// argmax2x2x_block (hs_upsample_taps.h) handing out the maxima as well: on return all four lanes of the quad hold the 4 x 8 label block's
// indices AND maxima.  Restated, as the two copies above are.
__device__ __forceinline__ void argmax2x2x_block_best(const float* __restrict__ xb, int C, int Hi, int Wi, int yi, int q, int sub,
                                                      int (&idx)[4][8], float (&best)[4][8]) {
    constexpr float NEG = -3.402823466e38f;
    const bool top = yi == 0, bottom = yi == Hi - 1, left = q == 0, right = 2 * q + 2 >= Wi;
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int k = 0; k < 8; ++k) { best[r][k] = NEG; idx[r][k] = sub; }
    for (int c0 = sub; c0 < C; c0 += 20) {
        float in[5][3][4];
#pragma unroll
        for (int u = 0; u < 5; ++u) {
            const int c = min(c0 + 4 * u, C - 1);
            load2x_block(xb + (size_t)c * Hi * Wi, Hi, Wi, yi, q, in[u]);
        }
#pragma unroll
        for (int u = 0; u < 5; ++u) {
            const int c = c0 + 4 * u;
            if (c < C) {
                float o[4][8];
                up2x2x_block(in[u], top, bottom, left, right, o);
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int k = 0; k < 8; ++k)
                        if (o[r][k] > best[r][k]) { best[r][k] = o[r][k]; idx[r][k] = c; }
            }
        }
    }
#pragma unroll
    for (int m = 1; m <= 2; m <<= 1) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const float v = __shfl_xor(best[r][k], m, 64);
                const int j = __shfl_xor(idx[r][k], m, 64);
                if (v > best[r][k] || (v == best[r][k] && j < idx[r][k])) { best[r][k] = v; idx[r][k] = j; }
            }
    }
}

// One class of the composed exact-2x second pass: lane J of the quad made the class' 4 x 8 label block; every lane takes the label row it
// accounts for (row `sub`) and adds class c to its eight sums.
template <int J, typename TT>
__device__ __forceinline__ void ce2x2x_take(const float (&o)[4][8], int sub, int c, const TT (&t)[8], const float (&m)[8], float (&s)[8],
                                            float (&xt)[8]) {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const float r0 = quad_bcast<J>(o[0][k]), r1 = quad_bcast<J>(o[1][k]), r2 = quad_bcast<J>(o[2][k]), r3 = quad_bcast<J>(o[3][k]);
        const float v = sub == 0 ? r0 : sub == 1 ? r1 : sub == 2 ? r2 : r3;
        s[k] += expf(v - m[k]);
        xt[k] = ((long long)t[k] == (long long)c) ? v : xt[k];
    }
}

// Both stages exact 2x: upsample2x2x_confusion_kernel's mapping (hs_eval.hip), four consecutive lanes per x block (yi, q) = 4 x 8 label
// block, lane `sub` accounting for label row 4 yi + sub.  First pass: argmax2x2x_block's split of the classes over the quad.  Second pass,
// as upsample2x_ce_confusion_kernel's: the quad makes four classes at a time (lane `sub`: class c0 + sub, the same load2x_block +
// up2x2x_block), the values are exchanged within the quad (ce2x2x_take) and each lane runs the ascending exp-sums of its row's eight pixels.
template <typename TT, typename... CW>
__global__ __launch_bounds__(EVAL_THREADS)
void upsample2x2x_ce_confusion_kernel(const float* __restrict__ x, int C, int Hi, int Wi, const TT* __restrict__ target, long long ignore_index,
                                      float* __restrict__ loss, int n, unsigned long long* __restrict__ out, long out_image_stride,
                                      uint8_t* __restrict__ mask, int vec, CW... cw) {
    constexpr bool W = sizeof...(CW) != 0;
    extern __shared__ unsigned hist[];
    const int nn = n * n, lane = threadIdx.x & 63;
    const bool count = out != nullptr;                           // (uniform)
    if (count) hist_zero(hist, nn);
    const size_t b = blockIdx.y;
    const int wq = Wi >> 1, Wo = 4 * Wi;
    const int items = Hi * wq;                                  // 4 x 8 label blocks of this image
    const int sub = (int)(threadIdx.x & 3);
    const size_t plane = (size_t)Hi * Wi;
    const float* __restrict__ xb = x + b * C * plane;
    for (int base = blockIdx.x * (EVAL_THREADS / 4); base < items; base += gridDim.x * (EVAL_THREADS / 4)) {
        const Item it = item_quad(base, items, wq);             // (the quad exchanges: convergent)
        const bool live = it.live;
        const int q = it.q, yi = it.y;
        const bool top = yi == 0, bottom = yi == Hi - 1, left = q == 0, right = 2 * q + 2 >= Wi;
        int p[8];
        float m[8];
        {
            int idx[4][8];
            float best[4][8];
            argmax2x2x_block_best(xb, C, Hi, Wi, yi, q, sub, idx, best);
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                p[k] = sub == 0 ? idx[0][k] : sub == 1 ? idx[1][k] : sub == 2 ? idx[2][k] : idx[3][k];
                m[k] = sub == 0 ? best[0][k] : sub == 1 ? best[1][k] : sub == 2 ? best[2][k] : best[3][k];
            }
        }
        const size_t at = (b * 4 * Hi + 4 * yi + sub) * Wo + 8 * q;
        TT tv[8];
        if (vec) {
            TT ta[4], tb[4];
            load4(target + at, ta);
            load4(target + at + 4, tb);
#pragma unroll
            for (int k = 0; k < 4; ++k) { tv[k] = ta[k]; tv[4 + k] = tb[k]; }
        } else {
#pragma unroll
            for (int k = 0; k < 8; ++k) tv[k] = target[at + k];
        }
        float wt[8];
#pragma unroll
        for (int k = 0; k < 8; ++k)                              // (W: in flight with the second pass' loads)
            wt[k] = class_weight((long long)tv[k], ce_live((long long)tv[k], ignore_index, C), cw...);
        float s[8], xt[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) s[k] = xt[k] = 0.0f;
        for (int c0 = 0; c0 < C; c0 += 4) {                      // (uniform: every lane of the wave takes every trip and every branch below)
            float in[3][4], o[4][8];
            load2x_block(xb + (size_t)min(c0 + sub, C - 1) * plane, Hi, Wi, yi, q, in);
            up2x2x_block(in, top, bottom, left, right, o);
            ce2x2x_take<0>(o, sub, c0, tv, m, s, xt);
            if (c0 + 1 < C) ce2x2x_take<1>(o, sub, c0 + 1, tv, m, s, xt);
            if (c0 + 2 < C) ce2x2x_take<2>(o, sub, c0 + 2, tv, m, s, xt);
            if (c0 + 3 < C) ce2x2x_take<3>(o, sub, c0 + 3, tv, m, s, xt);
        }
        float v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k)
            v[k] = ce_live((long long)tv[k], ignore_index, C) ? weighted<W>(wt[k], (logf(s[k]) + m[k]) - xt[k]) : 0.0f;
        if (live) {
            if (vec) {
                *reinterpret_cast<float4*>(loss + at) = make_float4(v[0], v[1], v[2], v[3]);
                *reinterpret_cast<float4*>(loss + at + 4) = make_float4(v[4], v[5], v[6], v[7]);
                if (mask != nullptr) {
                    *reinterpret_cast<uchar4*>(mask + at) = make_uchar4(p[0], p[1], p[2], p[3]);
                    *reinterpret_cast<uchar4*>(mask + at + 4) = make_uchar4(p[4], p[5], p[6], p[7]);
                }
            } else {
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    loss[at + k] = v[k];
                    if (mask != nullptr) mask[at + k] = (uint8_t)p[k];
                }
            }
        }
        if (count) {
#pragma unroll
            for (int k = 0; k < 8; ++k) count_key(hist, live ? pair_key<TT>(tv[k], p[k], n) : -1, lane);
        }
    }
    if (count) hist_flush(hist, nn, out + b * out_image_stride);
}

// ---- The launch fronts: one per entry and its weighted twin (CW: nothing, or the table), each kernel form launched from
// one line.  Histogram operands, target-type dispatcher, grids and the shape check: hs_eval_count.h.

template <typename T, typename... CW>
static void launch_ce_score(dim3 grid, const Hist& h, hipStream_t s, const T* x, const long long* target, int C, long hw, long long ignore_index,
                            float* loss, uint8_t* mask, CW... cw) {
    const dim3 block(EVAL_THREADS);
    if (C == 12) hipLaunchKernelGGL((ce_score_kernel<T, 12, CW...>), grid, block, h.lds, s, x, target, C, hw, ignore_index, loss, h.n, h.out, h.stride, mask, cw...);
    else if (C == 19) hipLaunchKernelGGL((ce_score_kernel<T, 19, CW...>), grid, block, h.lds, s, x, target, C, hw, ignore_index, loss, h.n, h.out, h.stride, mask, cw...);
    else if (C == 21) hipLaunchKernelGGL((ce_score_kernel<T, 21, CW...>), grid, block, h.lds, s, x, target, C, hw, ignore_index, loss, h.n, h.out, h.stride, mask, cw...);
    else hipLaunchKernelGGL((ce_score_kernel<T, 0, CW...>), grid, block, h.lds, s, x, target, C, hw, ignore_index, loss, h.n, h.out, h.stride, mask, cw...);
}

// what the loss entries ask of (classes, num_classes, confusion): nothing of num_classes where nothing is counted.  The LDS limit is asked first,
// so 257 classes are HS_ERR_UNSUPPORTED here and HS_ERR_BAD_ARG from hs_eval.hip's entries (kept as it is: DESIGN.md 3.11.3).
static int score_args(int classes, int num_classes, const void* confusion) {
    if (!confusion) return HS_OK;
    if (num_classes > EVAL_MAX_CLASSES) return HS_ERR_UNSUPPORTED;                                   // the LDS histogram (<= 256: uint8 class indices)
    if (num_classes <= 0 || classes > num_classes) return HS_ERR_BAD_ARG;
    return HS_OK;
}

// hs_cross_entropy_score_fwd: logits in memory, one pixel per thread
template <typename... CW>
static int ce_score(int32_t dtype, const void* logits, const int64_t* target, int32_t batch, int32_t classes, int64_t pixels, int64_t ignore_index,
                    float* loss, int32_t num_classes, int32_t per_image, int64_t* confusion, uint8_t* mask, void* stream, CW... cw) {
    if (!logits || !target || !loss || batch <= 0 || classes <= 0 || pixels <= 0) return HS_ERR_BAD_ARG;
    if (!storage_known(dtype)) return HS_ERR_BAD_ARG;
    if (classes > 256) return HS_ERR_BAD_ARG;                                                 // uint8 class indices
    const int status = score_args(classes, num_classes, confusion);
    if (status != HS_OK) return status;
    if (batch > 65535 || pixels > 0x7fffffffL - 4096) return HS_ERR_UNSUPPORTED;
    const Hist h = eval_hist(num_classes, per_image, confusion);
    const dim3 grid(eval_grid_x(((long)pixels + EVAL_THREADS - 1) / EVAL_THREADS, batch), (unsigned)batch);
    with_storage(dtype, [&](auto tag) {
        using T = decltype(tag);
        launch_ce_score<T>(grid, h, (hipStream_t)stream, (const T*)logits, (const long long*)target, classes, (long)pixels, ignore_index, loss, mask, cw...);
    });
    return launch_status();
}

// hs_upsample_ce_confusion_fwd: hs_upsample_confusion_fwd's choice of form (hs_eval.hip)
template <typename... CW>
static int upsample_ce_confusion(const float* x, int32_t batch, int32_t channels, int32_t Hi, int32_t Wi, int32_t Ho, int32_t Wo, const void* target,
                                 int32_t target_dtype, int64_t ignore_index, float* loss, int32_t num_classes, int32_t per_image,
                                 int64_t* confusion, uint8_t* mask, void* stream, CW... cw) {
    if (!target || !loss || !eval_shape_given(x, batch, channels, Hi, Wi, Ho, Wo, Ho, Wo)) return HS_ERR_BAD_ARG;
    if (!eval_storage_ok(target_dtype) || channels > 256) return HS_ERR_BAD_ARG;               // uint8 class indices
    const int status = score_args(channels, num_classes, confusion);
    if (status != HS_OK) return status;
    if (!eval_shape_fits(batch, Ho, Wo, Ho, Wo)) return HS_ERR_UNSUPPORTED;
    const Hist h = eval_hist(num_classes, per_image, confusion);
    const size_t tsz = target_dtype == HS_EVAL_U8 ? 1 : 8;
    const long long ii = (long long)ignore_index;
    const dim3 block(EVAL_THREADS);
    hipStream_t s = (hipStream_t)stream;
    if (is_exact2x(Hi, Wi, Ho, Wo)) {
        const int vec = aligned_to(target, 2 * tsz) && (!mask || aligned_to(mask, 4));
        with_target(target_dtype, target, [&](auto t) {
            hipLaunchKernelGGL((upsample2x_ce_confusion_kernel<pointee<decltype(t)>, CW...>), eval_grid_quads(Hi, Wi, batch), block, h.lds, s, x, channels,
                               Hi, Wi, t, ii, loss, h.n, h.out, h.stride, mask, vec, cw...);
        });
        return launch_status();
    }
    const int vec = (Wo & 3) == 0 && aligned_to(target, tsz == 1 ? 4 : 16) && aligned_to(loss, 16) && (!mask || aligned_to(mask, 4));
    const float sy = (float)Hi / (float)Ho, sx = (float)Wi / (float)Wo;
    with_target(target_dtype, target, [&](auto t) {
        hipLaunchKernelGGL((upsample_ce_confusion_kernel<pointee<decltype(t)>, CW...>), eval_grid_rows4(Ho, Wo, batch), block, h.lds, s, x, channels,
                           Hi, Wi, Ho, Wo, sy, sx, t, ii, loss, h.n, h.out, h.stride, mask, vec, cw...);
    });
    return launch_status();
}

// hs_upsample2_ce_confusion_fwd: hs_upsample2_confusion_fwd's choice of form (hs_eval.hip)
template <typename... CW>
static int upsample2_ce_confusion(const float* x, int32_t batch, int32_t channels, int32_t Hi, int32_t Wi, int32_t Hm, int32_t Wm, int32_t Ho,
                                  int32_t Wo, const void* target, int32_t target_dtype, int64_t ignore_index, float* loss, int32_t num_classes,
                                  int32_t per_image, int64_t* confusion, uint8_t* mask, void* stream, CW... cw) {
    if (!target || !loss || !eval_shape_given(x, batch, channels, Hi, Wi, Hm, Wm, Ho, Wo)) return HS_ERR_BAD_ARG;
    if (!eval_storage_ok(target_dtype) || channels > 256) return HS_ERR_BAD_ARG;               // uint8 class indices
    const int status = score_args(channels, num_classes, confusion);
    if (status != HS_OK) return status;
    if (!eval_shape_fits(batch, Hm, Wm, Ho, Wo)) return HS_ERR_UNSUPPORTED;
    const Hist h = eval_hist(num_classes, per_image, confusion);
    const bool aligned = aligned_to(target, target_dtype == HS_EVAL_U8 ? 4 : 16) && aligned_to(loss, 16) && (!mask || aligned_to(mask, 4));
    const long long ii = (long long)ignore_index;
    const dim3 block(EVAL_THREADS);
    hipStream_t s = (hipStream_t)stream;
    // dev A/B knob (tools/validate_label_time.py): HS_VALIDATE_2X2X=0 sends 2x o 2x shapes to the general form; read per call, so that one
    // process can capture both
    const char* knob = getenv("HS_VALIDATE_2X2X");
    if (is_exact2x(Hi, Wi, Hm, Wm) && is_exact2x(Hm, Wm, Ho, Wo) && !(knob && atoi(knob) == 0)) {
        const int vec = aligned;                                                              // rows of 8 k label pixels
        with_target(target_dtype, target, [&](auto t) {
            hipLaunchKernelGGL((upsample2x2x_ce_confusion_kernel<pointee<decltype(t)>, CW...>), eval_grid_quads(Hi, Wi, batch), block, h.lds, s, x, channels,
                               Hi, Wi, t, ii, loss, h.n, h.out, h.stride, mask, vec, cw...);
        });
        return launch_status();
    }
    const int vec = (Wo & 3) == 0 && aligned;
    with_target(target_dtype, target, [&](auto t) {
        hipLaunchKernelGGL((upsample2_ce_confusion_kernel<pointee<decltype(t)>, CW...>), eval_grid_rows4(Ho, Wo, batch), block, h.lds, s, x, channels,
                           stages2(Hi, Wi, Hm, Wm, Ho, Wo), t, ii, loss, h.n, h.out, h.stride, mask, vec, cw...);
    });
    return launch_status();
}

}  // namespace hs

using namespace hs;

extern "C" int hs_cross_entropy_score_fwd(int32_t dtype, const void* logits, const int64_t* target, int32_t batch, int32_t classes,
                                          int64_t pixels, int64_t ignore_index, float* loss, int32_t num_classes, int32_t per_image,
                                          int64_t* confusion, uint8_t* mask, void* stream) {
    return ce_score(dtype, logits, target, batch, classes, pixels, ignore_index, loss, num_classes, per_image, confusion, mask, stream);
}

extern "C" int hs_upsample_ce_confusion_fwd(const float* x, int32_t batch, int32_t channels, int32_t Hi, int32_t Wi, int32_t Ho, int32_t Wo,
                                            const void* target, int32_t target_dtype, int64_t ignore_index, float* loss, int32_t num_classes,
                                            int32_t per_image, int64_t* confusion, uint8_t* mask, void* stream) {
    return upsample_ce_confusion(x, batch, channels, Hi, Wi, Ho, Wo, target, target_dtype, ignore_index, loss, num_classes, per_image,
                                 confusion, mask, stream);
}

// The weighted twins: `weight` is the (classes,) / (channels,) fp32 table on the device, finite and >= 0 by the caller's word (it is not read on
// the host).  Masks and counts are the unweighted entries'; loss = weight[t] * theirs.
extern "C" int hs_cross_entropy_score_weighted_fwd(int32_t dtype, const void* logits, const int64_t* target, const float* weight, int32_t batch,
                                                   int32_t classes, int64_t pixels, int64_t ignore_index, float* loss, int32_t num_classes,
                                                   int32_t per_image, int64_t* confusion, uint8_t* mask, void* stream) {
    if (!weight) return HS_ERR_BAD_ARG;
    return ce_score(dtype, logits, target, batch, classes, pixels, ignore_index, loss, num_classes, per_image, confusion, mask, stream, weight);
}

extern "C" int hs_upsample_ce_confusion_weighted_fwd(const float* x, int32_t batch, int32_t channels, int32_t Hi, int32_t Wi, int32_t Ho, int32_t Wo,
                                                     const void* target, int32_t target_dtype, const float* weight, int64_t ignore_index,
                                                     float* loss, int32_t num_classes, int32_t per_image, int64_t* confusion, uint8_t* mask,
                                                     void* stream) {
    if (!weight) return HS_ERR_BAD_ARG;
    return upsample_ce_confusion(x, batch, channels, Hi, Wi, Ho, Wo, target, target_dtype, ignore_index, loss, num_classes, per_image,
                                 confusion, mask, stream, weight);
}

// The same at the LABEL's resolution: two resizes composed in registers, x (Hi, Wi) -> mid (Hm, Wm) -> (Ho, Wo).
extern "C" int hs_upsample2_ce_confusion_fwd(const float* x, int32_t batch, int32_t channels, int32_t Hi, int32_t Wi, int32_t Hm, int32_t Wm,
                                             int32_t Ho, int32_t Wo, const void* target, int32_t target_dtype, int64_t ignore_index, float* loss,
                                             int32_t num_classes, int32_t per_image, int64_t* confusion, uint8_t* mask, void* stream) {
    return upsample2_ce_confusion(x, batch, channels, Hi, Wi, Hm, Wm, Ho, Wo, target, target_dtype, ignore_index, loss, num_classes, per_image,
                                  confusion, mask, stream);
}

extern "C" int hs_upsample2_ce_confusion_weighted_fwd(const float* x, int32_t batch, int32_t channels, int32_t Hi, int32_t Wi, int32_t Hm,
                                                      int32_t Wm, int32_t Ho, int32_t Wo, const void* target, int32_t target_dtype,
                                                      const float* weight, int64_t ignore_index, float* loss, int32_t num_classes,
                                                      int32_t per_image, int64_t* confusion, uint8_t* mask, void* stream) {
    if (!weight) return HS_ERR_BAD_ARG;
    return upsample2_ce_confusion(x, batch, channels, Hi, Wi, Hm, Wm, Ho, Wo, target, target_dtype, ignore_index, loss, num_classes, per_image,
                                  confusion, mask, stream, weight);
}
