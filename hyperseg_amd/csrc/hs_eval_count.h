// Counting core of the on-device evaluation kernels (hs_eval.hip, hs_validate.hip): the per-workgroup n x n LDS histogram, the wave's
// ballot aggregation into it, its one flush per workgroup, the label loads and the grid cap.  Shape and reasons: hs_eval.hip's header.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "hs_common.h"

namespace hs {

constexpr int EVAL_THREADS = 512;
constexpr int EVAL_MAX_CLASSES = 128;          // n * n * 4 bytes = 64 KB of LDS at most
constexpr int EVAL_AGG_ROUNDS = 4;             // distinct keys handled by ballot before lanes add for themselves

// One key per lane (key < 0: nothing to count), all lanes of the wave present.
__device__ __forceinline__ void count_key(unsigned* __restrict__ hist, int key, int lane) {
    unsigned long long todo = __ballot(key >= 0);
#pragma unroll 1
    for (int it = 0; it < EVAL_AGG_ROUNDS && todo != 0; ++it) {
        const int leader = __ffsll((long long)todo) - 1;
        const int k = __builtin_amdgcn_readlane(key, leader);
        const unsigned long long same = __ballot(key == k);
        if (lane == leader) atomicAdd(&hist[k], (unsigned)__popcll(same));
        todo &= ~same;
    }
    if ((todo >> lane) & 1ull) atomicAdd(&hist[key], 1u);
}

// n * t + p, or -1 where the pair is not counted: targets outside [0, n) are ignored (seg_utils.py:15-17).
template <typename T>
__device__ __forceinline__ int pair_key(T t, int p, int n) {
    return (t >= (T)0 && (long long)t < (long long)n) ? n * (int)t + p : -1;
}

__device__ __forceinline__ void hist_zero(unsigned* hist, int nn) {
    for (int i = threadIdx.x; i < nn; i += EVAL_THREADS) hist[i] = 0u;
    __syncthreads();
}
__device__ __forceinline__ void hist_flush(const unsigned* hist, int nn, unsigned long long* __restrict__ out) {
    __syncthreads();
    for (int i = threadIdx.x; i < nn; i += EVAL_THREADS) {
        const unsigned v = hist[i];
        if (v != 0u) atomicAdd(out + i, (unsigned long long)v);
    }
}

// 2 consecutive targets / 4 consecutive targets; `vec`: the address is a multiple of the vector's size
template <typename T> struct Vec2;
template <> struct Vec2<uint8_t> { typedef uchar2 type; };
template <> struct Vec2<int64_t> { typedef longlong2 type; };
template <typename T>
__device__ __forceinline__ void load2(const T* __restrict__ p, bool vec, T (&t)[2]) {
    if (vec) {
        const typename Vec2<T>::type v = *reinterpret_cast<const typename Vec2<T>::type*>(p);
        t[0] = (T)v.x; t[1] = (T)v.y;
    } else {
        t[0] = p[0]; t[1] = p[1];
    }
}
__device__ __forceinline__ void load4(const uint8_t* __restrict__ p, uint8_t (&t)[4]) {
    const uchar4 v = *reinterpret_cast<const uchar4*>(p);
    t[0] = v.x; t[1] = v.y; t[2] = v.z; t[3] = v.w;
}
__device__ __forceinline__ void load4(const int64_t* __restrict__ p, int64_t (&t)[4]) {
    const longlong2 a = reinterpret_cast<const longlong2*>(p)[0], b = reinterpret_cast<const longlong2*>(p)[1];
    t[0] = a.x; t[1] = a.y; t[2] = b.x; t[3] = b.y;
}

static int eval_cus() {
    static const int cus = [] {                                  // (one process per GPU: every visible device is the same part)
        int dev = 0, c = 0;
        return (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && c > 0) ? c : 256;
    }();
    return cus;
}
// workgroups per image: about one per CU over the whole batch, never more than there are passes of work
static unsigned eval_grid_x(long passes, int batch) {
    long per_image = (eval_cus() + batch - 1) / batch;
    if (per_image > passes) per_image = passes;
    return (unsigned)(per_image < 1 ? 1 : per_image);
}
static bool eval_storage_ok(int dtype) { return dtype == HS_EVAL_U8 || dtype == HS_EVAL_I64; }
static bool aligned_to(const void* p, size_t a) { return ((uintptr_t)p % a) == 0; }

}  // namespace hs
