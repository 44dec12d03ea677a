// Confidence core of the served confidence maps (hs_confidence.hip): the soft-max probability of a pixel's arg-max class,
// softmax(v)[argmax] = 1 / sum_c exp(v_c - v_max), taken in fp32 in ONE ascending pass over the classes with a running maximum and a
// rescaled running sum.  The recurrence lives in confidence_step and nowhere else: every kernel of hs_confidence.hip walks its classes
// through it in the same order, so the composed route (finished logits) and the fused ones (scores from the taps) give the same bits.
// hyperseg_amd/utils/confidence.py states the same recurrence, quantisation and threshold rule on the CPU.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace hs {

// m: the largest score so far, idx: its class (the first one on ties), s: sum of exp(v_c - m) over the classes seen.
struct Conf { float m, s; int idx; };

// The two starts, which differ only where a score is not finite (for finite scores the first step from conf_floor is
// s = 0 * expf(..) + 1 = 1, m = v_0: conf_first's state, bit for bit).  They are the starts of the two arg-max forms, so that the
// mask byte of a pixel with a non-finite score is what the arg-max entry of the same shape writes:
//   conf_first: argmax_row4 / argmax2_row4 -- class 0 holds until a strictly larger score comes (a NaN in class 0 stays);
//   conf_floor: argmax2x_block / argmax2x2x_block -- from -FLT_MAX, a score wins only by being strictly larger (a NaN never wins).
__device__ __forceinline__ Conf conf_first(float v0) { return {v0, 1.0f, 0}; }
__device__ __forceinline__ Conf conf_floor() { return {-3.402823466e38f, 0.0f, 0}; }

// One class: v > m moves the maximum and rescales the sum, s = s * expf(m - v) + 1; otherwise s += expf(v - m).  One expf either way.
__device__ __forceinline__ void confidence_step(Conf& st, float v, int c) {
    const bool up = v > st.m;
    const float e = expf(up ? st.m - v : v - st.m);
    st.s = up ? st.s * e + 1.0f : st.s + e;
    st.m = up ? v : st.m;
    st.idx = up ? c : st.idx;
}

__device__ __forceinline__ float confidence_value(const Conf& st) { return 1.0f / st.s; }

// The served form: (uint8)(conf * 255 + 0.5), 255 for conf = 1.
__device__ __forceinline__ uint8_t confidence_u8(float conf) { return (uint8_t)(conf * 255.0f + 0.5f); }

// Pseudo-labels: a pixel whose fp32 confidence is strictly below the threshold takes the fill byte.
__device__ __forceinline__ uint8_t confidence_label(int idx, float conf, float threshold, int fill) {
    return (uint8_t)(conf < threshold ? fill : idx);
}

}  // namespace hs
