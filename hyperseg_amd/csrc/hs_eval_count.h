// Counting core of the on-device evaluation kernels (hs_eval.hip, hs_validate.hip): the per-workgroup n x n LDS histogram, the wave's
// ballot aggregation into it, its one flush per workgroup, the label loads and the grid cap.  Shape and reasons: hs_eval.hip's header; which
// item a thread of those kernels works on: hs_last_launch.h.
// Below the device code, the host front of their entries: histogram operands, target-type dispatcher, grids and the shape check.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "hs_common.h"
#include "hs_last_launch.h"

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

// ---- The launch front the scoring entries share.  Host code only.  Each entry keeps its own `vec` predicate and its own
// order of refusals; what it takes from here is how the operands of a launch are made once the call is accepted.

// The LDS histogram's operands: nothing is counted (n = 0, no LDS) where there is no matrix to count into.
struct Hist { int n; size_t lds; long stride; unsigned long long* out; };
static Hist eval_hist(int num_classes, int per_image, int64_t* confusion) {
    const int n = confusion ? num_classes : 0;
    return {n, (size_t)n * n * sizeof(unsigned), per_image ? (long)n * n : 0, reinterpret_cast<unsigned long long*>(confusion)};
}

// The ONE place an HS_EVAL_* code picks a kernel instantiation, as with_storage (hs_common.h) is for HS_DTYPE_*: calls f with `p` as a typed
// pointer (`using TT = pointee<decltype(t)>;` ... kernel<TT>, t) and returns true; for any other code it calls nothing and returns false (the
// entries refuse such a code with eval_storage_ok, at the place in their order where they always did).
template <typename F> __attribute__((always_inline)) inline bool with_target(int dtype, const void* p, F&& f) {
    if (dtype == HS_EVAL_U8) { f((const uint8_t*)p); return true; }
    if (dtype == HS_EVAL_I64) { f((const int64_t*)p); return true; }
    return false;
}

// Grids of the two mappings: one thread = 4 consecutive pixels of a row of (Ho, Wo); four lanes = one 2 x 4 block of pairs of (Hi, Wi)'s columns.
static dim3 eval_grid_rows4(long Ho, long Wo, int batch) {
    return dim3(eval_grid_x((Ho * ((Wo + 3) / 4) + EVAL_THREADS - 1) / EVAL_THREADS, batch), (unsigned)batch);
}
static dim3 eval_grid_quads(int Hi, int Wi, int batch) {
    return dim3(eval_grid_x(((long)Hi * (Wi / 2) + EVAL_THREADS / 4 - 1) / (EVAL_THREADS / 4), batch), (unsigned)batch);
}

// The shape check of the resizing entries, x (batch, channels, Hi, Wi) -> mid (Hm, Wm) -> (Ho, Wo); a one-stage entry names its output as its
// mid.  Two halves, because every entry refuses its class counts between them: given (else HS_ERR_BAD_ARG), fits (else HS_ERR_UNSUPPORTED:
// blockIdx.y, and int pixel indices with room for a grid stride).
static bool eval_shape_given(const void* x, int batch, int channels, int Hi, int Wi, int Hm, int Wm, int Ho, int Wo) {
    return x && batch > 0 && channels > 0 && Hi > 0 && Wi > 0 && Hm > 0 && Wm > 0 && Ho > 0 && Wo > 0;
}
static bool eval_shape_fits(int batch, int Hm, int Wm, int Ho, int Wo) {
    return batch <= 65535 && (long)Ho * Wo <= 0x7fffffffL - 4096 && (long)Hm * Wm <= 0x7fffffffL - 4096;
}

}  // namespace hs
