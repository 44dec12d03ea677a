// One row of Pillow's resize tables built on the device, shared by the launch that builds a crop window of one input size
// (hs_resample_batch.hip) and the launch whose input size differs per sample (hs_augment_ragged.hip):
// utils/resample.py::resample_coeffs restated in its operation order, every float64 operation spelt __ddiv_rn / __dmul_rn / __dadd_rn
// (and the library is built with -ffp-contract=off), so the integers are the host's.  A tap is evaluated twice, for the sum and for the
// quotient: same bits.  What the two launches differ in -- where a sample's sizes come from, which rows exist -- stays with each kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "hs_resample_px.h"

namespace hs {

constexpr int RT_THREADS = 256;
constexpr int RT_MAX_KS = 1 << 12;             // ks_max the entries accept (a table row of 16 KB)

// resample_coeffs' scalars of one axis
struct AxisScale { double scale, support, ss; int ksize; };

__device__ __forceinline__ AxisScale axis_scale(int in, int out, double filter_support) {
    AxisScale s;
    s.scale = __ddiv_rn((double)in, (double)out);
    const double filterscale = s.scale > 1.0 ? s.scale : 1.0;
    s.support = __dmul_rn(filter_support, filterscale);
    s.ksize = (int)ceil(s.support) * 2 + 1;
    s.ss = __ddiv_rn(1.0, filterscale);
    return s;
}

template <bool BICUBIC>
__device__ __forceinline__ double resize_filter(double x) {
    x = fabs(x);
    if constexpr (BICUBIC) {                   // utils/resample.py::_bicubic, a = -0.5, in its parenthesisation
        if (x < 1.0) return __dadd_rn(__dmul_rn(__dmul_rn(__dadd_rn(__dmul_rn(1.5, x), -2.5), x), x), 1.0);
        if (x < 2.0) return __dmul_rn(__dadd_rn(__dmul_rn(__dadd_rn(__dmul_rn(__dadd_rn(x, -5.0), x), 8.0), x), -4.0), -0.5);
        return 0.0;
    } else {
        return x < 1.0 ? __dadd_rn(1.0, -x) : 0.0;
    }
}

template <bool BICUBIC>
__device__ __forceinline__ double resize_tap(int k, int xmin, double center, double ss) {
    return resize_filter<BICUBIC>(__dmul_rn(__dadd_rn(__dadd_rn((double)(k + xmin), -center), 0.5), ss));
}

// Row r (0 <= r < out) of resample_coeffs(in, out): the first source index and the tap count, the weights into k_row[0 .. n).  The
// caller zeroes k_row[n .. ks_max).  n never exceeds ks_max.
template <bool BICUBIC>
__device__ __forceinline__ void resize_table_row(int in, int out, int r, int ks_max, int32_t* __restrict__ k_row, int& xmin, int& n) {
    constexpr double filter_support = BICUBIC ? 2.0 : 1.0;
    if (in == out) {                           // the pass Pillow skips: one tap of 2^22
        xmin = r; n = 1;
        k_row[0] = 1 << RS_BITS;
        return;
    }
    const AxisScale s = axis_scale(in, out, filter_support);
    const double center = __dmul_rn(__dadd_rn((double)r, 0.5), s.scale);
    xmin = max((int)__dadd_rn(__dadd_rn(center, -s.support), 0.5), 0);         // C's (int): truncation
    n = min((int)__dadd_rn(__dadd_rn(center, s.support), 0.5), in) - xmin;
    n = max(min(min(n, s.ksize), ks_max), 0);
    double ww = 0.0;
    for (int k = 0; k < n; ++k) ww = __dadd_rn(ww, resize_tap<BICUBIC>(k, xmin, center, s.ss));      // the sequential sum
    for (int k = 0; k < n; ++k) {
        double w = resize_tap<BICUBIC>(k, xmin, center, s.ss);
        if (ww != 0.0) w = __ddiv_rn(w, ww);
        const double q = __dmul_rn(w, (double)(1 << RS_BITS));
        k_row[k] = (int)(w < 0.0 ? __dadd_rn(-0.5, q) : __dadd_rn(0.5, q));
    }
}

}  // namespace hs
