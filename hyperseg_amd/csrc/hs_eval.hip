// On-device evaluation epilogue: the (target, prediction) confusion matrix of the reference's evaluation loop
// (hyperseg/utils/seg_utils.py:5-36, fed by test.py:166-175 / test_fps.py:184-194) counted on the GPU, either from finished
// masks (hs_confusion_fwd) or inside the final upsample + arg-max launch, where every output pixel's class index already sits in
// a register (hs_upsample_confusion_fwd).  Integer counts only: the result does not depend on arrival order.
//
// Shape of both kernels ("On-device evaluation"):
//   * one workgroup of 512 threads per CU (the arg-max bodies hold 136-256 VGPRs: 1024 threads spill), grid-striding over its image's pixels (blockIdx.y = image), counting into a
//     per-workgroup n x n histogram of 32-bit bins in LDS;
//   * in the wave, label maps are spatially coherent -- most lanes hold the SAME (t, p) key and a per-lane LDS atomic would
//     serialise on one bin.  count_key() walks the distinct keys present in the wave (__ballot / __popcll: one LDS add per
//     distinct key) for a few rounds and only then lets the remaining lanes add for themselves (the uniform-random case);
//   * across workgroups the whole matrix is a few cache lines, so each workgroup flushes once, at its end: non-zero bins only,
//     consecutive lanes on consecutive bins, one 64-bit global atomic add each (global_atomic_add_x2, no compare-and-swap).
// No cross-workgroup waiting of any kind.
// Which item a thread works on in a pass of its grid-stride loop -- item_rows4 / item_quad, surplus lanes shadowing the last item -- is
// stated once for these kernels and hs_validate.hip's (hs_last_launch.h); the loads, stores and counting tails stay written out here.
// Host side: the entries at the end of the file share one launch front with hs_validate.hip's (hs_eval_count.h: histogram operands,
// target-type dispatcher, grids, shape check; Stages2's constructor: hs_upsample_taps.h); refusal order and `vec` stay each entry's own.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "hyperseg_hip.h"
#include "hs_common.h"
#include "hs_upsample_taps.h"
#include "hs_eval_count.h"

namespace hs {

// General resize (any ratio, the identity included): argmax_row4 (hs_upsample_taps.h), one thread = 4 consecutive output pixels of
// a row, then the four pairs are counted.
template <typename TT>
__global__ __launch_bounds__(EVAL_THREADS)
void upsample_confusion_kernel(const float* __restrict__ x, int C, int Hi, int Wi, int Ho, int Wo, float scale_y, float scale_x,
                               const TT* __restrict__ target, int n, unsigned long long* __restrict__ out, long out_image_stride,
                               uint8_t* __restrict__ mask, int vec) {
    extern __shared__ unsigned hist[];
    const int nn = n * n, lane = threadIdx.x & 63;
    hist_zero(hist, nn);
    const size_t b = blockIdx.y;
    const int wq = (Wo + 3) / 4;
    const int items = Ho * wq;
    const float* __restrict__ xb = x + b * C * Hi * Wi;
    for (int base = blockIdx.x * EVAL_THREADS; base < items; base += gridDim.x * EVAL_THREADS) {      // wave-uniform trip count
        const Item it = item_rows4(base, items, wq);
        const bool live = it.live;
        const int q = it.q, yo = it.y;
        const Row4 t = row4_taps(yo, q, Hi, Wi, Wo, scale_y, scale_x);
        int idx[4];
        argmax_row4(xb, C, Hi, Wi, t, idx);
        const size_t at = (b * Ho + yo) * Wo + 4 * q;
        TT tv[4];
        if (vec) {
            load4(target + at, tv);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) tv[i] = target[at + (4 * q + i < Wo ? i : 0)];
        }
        if (mask != nullptr && live) {
            if (vec) {
                *reinterpret_cast<uchar4*>(mask + at) = make_uchar4(idx[0], idx[1], idx[2], idx[3]);
            } else {
                for (int i = 0; i < 4 && 4 * q + i < Wo; ++i) mask[at + i] = (uint8_t)idx[i];
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
            count_key(hist, (live && 4 * q + i < Wo) ? pair_key<TT>(tv[i], idx[i], n) : -1, lane);
    }
    hist_flush(hist, nn, out + b * out_image_stride);
}

// Exact 2x: argmax2x_block (hs_upsample_taps.h), four consecutive lanes per 2 x 4 output block, after which all four lanes hold the
// block's eight class indices and each counts two of them: lane `sub` takes row sub >> 1, columns 2 (sub & 1) and + 1.
template <typename TT>
__global__ __launch_bounds__(EVAL_THREADS)
void upsample2x_confusion_kernel(const float* __restrict__ x, int C, int Hi, int Wi, const TT* __restrict__ target, int n,
                                 unsigned long long* __restrict__ out, long out_image_stride, uint8_t* __restrict__ mask, int vec) {
    extern __shared__ unsigned hist[];
    const int nn = n * n, lane = threadIdx.x & 63;
    hist_zero(hist, nn);
    const size_t b = blockIdx.y;
    const int wq = Wi >> 1, Wo = 2 * Wi;
    const int items = Hi * wq;                                  // 2 x 4 output blocks of this image
    const int sub = (int)(threadIdx.x & 3);
    const float* __restrict__ xb = x + b * C * Hi * Wi;
    for (int base = blockIdx.x * (EVAL_THREADS / 4); base < items; base += gridDim.x * (EVAL_THREADS / 4)) {
        const Item it = item_quad(base, items, wq);             // (argmax2x_block: convergent)
        const bool live = it.live;
        const int q = it.q, yi = it.y;
        int idx0[4], idx1[4];
        argmax2x_block(xb, C, Hi, Wi, yi, q, sub, idx0, idx1);
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
        const bool row1 = (sub & 2) != 0, right = (sub & 1) != 0;
        const int pa = row1 ? (right ? idx1[2] : idx1[0]) : (right ? idx0[2] : idx0[0]);
        const int pb = row1 ? (right ? idx1[3] : idx1[1]) : (right ? idx0[3] : idx0[1]);
        TT tv[2];
        load2(target + at + (row1 ? Wo : 0) + (right ? 2 : 0), vec != 0, tv);
        count_key(hist, live ? pair_key<TT>(tv[0], pa, n) : -1, lane);
        count_key(hist, live ? pair_key<TT>(tv[1], pb, n) : -1, lane);
    }
    hist_flush(hist, nn, out + b * out_image_stride);
}

// Two resizes composed in registers (x -> mid -> label: the decoder's final resize, then test.py:167-168's to the label's size), the
// general form: argmax2_row4 (hs_upsample_taps.h), otherwise upsample_confusion_kernel.  target == nullptr: masks only, nothing counted.
template <typename TT>
__global__ __launch_bounds__(EVAL_THREADS)
void upsample2_confusion_kernel(const float* __restrict__ x, int C, Stages2 s, const TT* __restrict__ target, int n,
                                unsigned long long* __restrict__ out, long out_image_stride, uint8_t* __restrict__ mask, int vec) {
    extern __shared__ unsigned hist[];
    const int nn = n * n, lane = threadIdx.x & 63;
    const bool count = target != nullptr;                        // (uniform)
    if (count) hist_zero(hist, nn);
    const size_t b = blockIdx.y;
    const int Ho = s.Ho, Wo = s.Wo, wq = (Wo + 3) / 4;
    const int items = Ho * wq;
    const float* __restrict__ xb = x + b * C * s.Hi * s.Wi;
    for (int base = blockIdx.x * EVAL_THREADS; base < items; base += gridDim.x * EVAL_THREADS) {      // wave-uniform trip count
        const Item it = item_rows4(base, items, wq);
        const bool live = it.live;
        const int q = it.q, yo = it.y;
        const Row4x2 t = row4x2_taps(yo, q, s);
        int idx[4];
        argmax2_row4(xb, C, s.Hi, s.Wi, t, idx);
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

// Both stages exact 2x: argmax2x2x_block (hs_upsample_taps.h), four consecutive lanes per x block (yi, q) = 4 x 8 label block, after
// which all four lanes hold the block's 32 class indices; lane `sub` takes label row 4 yi + sub: its eight indices are stored with
// two 4-byte stores and counted against eight targets from two vector loads.
template <typename TT>
__global__ __launch_bounds__(EVAL_THREADS)
void upsample2x2x_confusion_kernel(const float* __restrict__ x, int C, int Hi, int Wi, const TT* __restrict__ target, int n,
                                   unsigned long long* __restrict__ out, long out_image_stride, uint8_t* __restrict__ mask, int vec) {
    extern __shared__ unsigned hist[];
    const int nn = n * n, lane = threadIdx.x & 63;
    const bool count = target != nullptr;                        // (uniform)
    if (count) hist_zero(hist, nn);
    const size_t b = blockIdx.y;
    const int wq = Wi >> 1, Wo = 4 * Wi;
    const int items = Hi * wq;                                  // 4 x 8 label blocks of this image
    const int sub = (int)(threadIdx.x & 3);
    const float* __restrict__ xb = x + b * C * Hi * Wi;
    for (int base = blockIdx.x * (EVAL_THREADS / 4); base < items; base += gridDim.x * (EVAL_THREADS / 4)) {
        const Item it = item_quad(base, items, wq);             // (argmax2x2x_block: convergent)
        const bool live = it.live;
        const int q = it.q, yi = it.y;
        int idx[4][8];
        argmax2x2x_block(xb, C, Hi, Wi, yi, q, sub, idx);
        int p[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) p[k] = sub == 0 ? idx[0][k] : sub == 1 ? idx[1][k] : sub == 2 ? idx[2][k] : idx[3][k];
        const size_t at = (b * 4 * Hi + 4 * yi + sub) * Wo + 8 * q;
        if (mask != nullptr && live) {
            if (vec) {
                *reinterpret_cast<uchar4*>(mask + at) = make_uchar4(p[0], p[1], p[2], p[3]);
                *reinterpret_cast<uchar4*>(mask + at + 4) = make_uchar4(p[4], p[5], p[6], p[7]);
            } else {
#pragma unroll
                for (int k = 0; k < 8; ++k) mask[at + k] = (uint8_t)p[k];
            }
        }
        if (count) {
            TT ta[4], tb[4];
            if (vec) {
                load4(target + at, ta);
                load4(target + at + 4, tb);
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) { ta[k] = target[at + k]; tb[k] = target[at + 4 + k]; }
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) count_key(hist, live ? pair_key<TT>(ta[k], p[k], n) : -1, lane);
#pragma unroll
            for (int k = 0; k < 4; ++k) count_key(hist, live ? pair_key<TT>(tb[k], p[4 + k], n) : -1, lane);
        }
    }
    if (count) hist_flush(hist, nn, out + b * out_image_stride);
}

// Finished predictions: one thread = 4 consecutive elements of its image's row of N.  A prediction outside [0, n) is not
// counted either (the stock route miscounts or fails there).
template <typename TP, typename TT>
__global__ __launch_bounds__(EVAL_THREADS)
void confusion_kernel(const TP* __restrict__ pred, const TT* __restrict__ target, long N, int n,
                      unsigned long long* __restrict__ out, long out_image_stride, int vec) {
    extern __shared__ unsigned hist[];
    const int nn = n * n, lane = threadIdx.x & 63;
    hist_zero(hist, nn);
    const size_t b = blockIdx.y;
    const TP* __restrict__ pb = pred + b * N;
    const TT* __restrict__ tb = target + b * N;
    const long groups = (N + 3) / 4;
    for (long base = (long)blockIdx.x * EVAL_THREADS; base < groups; base += (long)gridDim.x * EVAL_THREADS) {
        const long g = base + threadIdx.x;
        const bool live = g < groups;
        const long at = 4 * (live ? g : groups - 1);
        TP pv[4];
        TT tv[4];
        if (vec) {
            load4(pb + at, pv);
            load4(tb + at, tv);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const long j = at + i < N ? at + i : N - 1;
                pv[i] = pb[j]; tv[i] = tb[j];
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const bool ok = live && at + i < N && pv[i] >= (TP)0 && (long long)pv[i] < (long long)n;
            count_key(hist, ok ? pair_key<TT>(tv[i], (int)pv[i], n) : -1, lane);
        }
    }
    hist_flush(hist, nn, out + b * out_image_stride);
}

}  // namespace hs

using namespace hs;

extern "C" int hs_eval_max_classes(void) { return EVAL_MAX_CLASSES; }

// The entries below are fronts in the shape DESIGN.md 3.11.3 describes: the entry's own refusals in its own order, eval_hist's operands, its own
// `vec` predicate per form, and each kernel form launched from one line under with_target.

extern "C" int hs_upsample_confusion_fwd(const float* x, int32_t batch, int32_t channels, int32_t Hi, int32_t Wi, int32_t Ho, int32_t Wo,
                                         const void* target, int32_t target_dtype, int32_t num_classes, int32_t per_image,
                                         int64_t* confusion, uint8_t* mask, void* stream) {
    if (!target || !confusion || !eval_shape_given(x, batch, channels, Hi, Wi, Ho, Wo, Ho, Wo)) return HS_ERR_BAD_ARG;
    if (!eval_storage_ok(target_dtype) || num_classes <= 0 || channels > num_classes) return HS_ERR_BAD_ARG;
    if (num_classes > 256) return HS_ERR_BAD_ARG;                                            // uint8 class indices
    if (num_classes > EVAL_MAX_CLASSES || !eval_shape_fits(batch, Ho, Wo, Ho, Wo)) return HS_ERR_UNSUPPORTED;
    const Hist h = eval_hist(num_classes, per_image, confusion);
    const size_t tsz = target_dtype == HS_EVAL_U8 ? 1 : 8;
    const dim3 block(EVAL_THREADS);
    hipStream_t s = (hipStream_t)stream;
    if (is_exact2x(Hi, Wi, Ho, Wo)) {
        const int vec = aligned_to(target, 2 * tsz) && (!mask || aligned_to(mask, 4));
        with_target(target_dtype, target, [&](auto t) {
            hipLaunchKernelGGL(upsample2x_confusion_kernel<pointee<decltype(t)>>, eval_grid_quads(Hi, Wi, batch), block, h.lds, s, x, channels, Hi, Wi,
                               t, h.n, h.out, h.stride, mask, vec);
        });
        return launch_status();
    }
    const int vec = (Wo & 3) == 0 && aligned_to(target, tsz == 1 ? 4 : 16) && (!mask || aligned_to(mask, 4));
    const float sy = (float)Hi / (float)Ho, sx = (float)Wi / (float)Wo;
    with_target(target_dtype, target, [&](auto t) {
        hipLaunchKernelGGL(upsample_confusion_kernel<pointee<decltype(t)>>, eval_grid_rows4(Ho, Wo, batch), block, h.lds, s, x, channels, Hi, Wi, Ho, Wo,
                           sy, sx, t, h.n, h.out, h.stride, mask, vec);
    });
    return launch_status();
}

extern "C" int hs_upsample2_confusion_fwd(const float* x, int32_t batch, int32_t channels, int32_t Hi, int32_t Wi, int32_t Hm, int32_t Wm,
                                          int32_t Ho, int32_t Wo, const void* target, int32_t target_dtype, int32_t num_classes,
                                          int32_t per_image, int64_t* confusion, uint8_t* mask, void* stream) {
    if (!eval_shape_given(x, batch, channels, Hi, Wi, Hm, Wm, Ho, Wo)) return HS_ERR_BAD_ARG;
    const bool count = target != nullptr;
    if (count != (confusion != nullptr) || (!count && !mask)) return HS_ERR_BAD_ARG;          // masks only: neither, and a mask to write
    if (count) {
        if (!eval_storage_ok(target_dtype) || num_classes <= 0 || channels > num_classes) return HS_ERR_BAD_ARG;
        if (num_classes > 256) return HS_ERR_BAD_ARG;                                         // uint8 class indices
        if (num_classes > EVAL_MAX_CLASSES) return HS_ERR_UNSUPPORTED;
    } else if (channels > 256) {
        return HS_ERR_UNSUPPORTED;                                                            // as hs_upsample_argmax_fwd
    }
    if (!eval_shape_fits(batch, Hm, Wm, Ho, Wo)) return HS_ERR_UNSUPPORTED;
    const Hist h = eval_hist(num_classes, per_image, confusion);
    const int dtype = count ? target_dtype : HS_EVAL_U8;                                      // masks only: the uint8 instantiation, a null pointer
    const bool aligned = (!count || aligned_to(target, dtype == HS_EVAL_U8 ? 4 : 16)) && (!mask || aligned_to(mask, 4));
    const dim3 block(EVAL_THREADS);
    hipStream_t s = (hipStream_t)stream;
    if (is_exact2x(Hi, Wi, Hm, Wm) && is_exact2x(Hm, Wm, Ho, Wo)) {
        const int vec = aligned;                                                              // rows of 8 k label pixels
        with_target(dtype, target, [&](auto t) {
            hipLaunchKernelGGL(upsample2x2x_confusion_kernel<pointee<decltype(t)>>, eval_grid_quads(Hi, Wi, batch), block, h.lds, s, x, channels, Hi, Wi,
                               t, h.n, h.out, h.stride, mask, vec);
        });
        return launch_status();
    }
    const int vec = (Wo & 3) == 0 && aligned;
    with_target(dtype, target, [&](auto t) {
        hipLaunchKernelGGL(upsample2_confusion_kernel<pointee<decltype(t)>>, eval_grid_rows4(Ho, Wo, batch), block, h.lds, s, x, channels,
                           stages2(Hi, Wi, Hm, Wm, Ho, Wo), t, h.n, h.out, h.stride, mask, vec);
    });
    return launch_status();
}

extern "C" int hs_confusion_fwd(const void* pred, int32_t pred_dtype, const void* target, int32_t target_dtype, int32_t batch,
                                int64_t elements, int32_t num_classes, int32_t per_image, int64_t* confusion, void* stream) {
    if (!pred || !target || !confusion || batch <= 0 || elements <= 0 || num_classes <= 0) return HS_ERR_BAD_ARG;
    if (!eval_storage_ok(pred_dtype) || !eval_storage_ok(target_dtype)) return HS_ERR_BAD_ARG;
    if (num_classes > EVAL_MAX_CLASSES || batch > 65535 || elements > 0x7fffffffL - 4096) return HS_ERR_UNSUPPORTED;
    const Hist h = eval_hist(num_classes, per_image, confusion);
    const size_t psz = pred_dtype == HS_EVAL_U8 ? 1 : 8, tsz = target_dtype == HS_EVAL_U8 ? 1 : 8;
    const int vec = (elements & 3) == 0 && aligned_to(pred, psz == 1 ? 4 : 16) && aligned_to(target, tsz == 1 ? 4 : 16);
    hipStream_t s = (hipStream_t)stream;
    with_target(pred_dtype, pred, [&](auto p) {
        with_target(target_dtype, target, [&](auto t) {
            hipLaunchKernelGGL((confusion_kernel<pointee<decltype(p)>, pointee<decltype(t)>>), eval_grid_rows4(1, elements, batch), dim3(EVAL_THREADS),
                               h.lds, s, p, t, (long)elements, h.n, h.out, h.stride, vec);
        });
    });
    return launch_status();
}

