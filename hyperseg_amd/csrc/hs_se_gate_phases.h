// The three phases of the one-launch squeeze-excite gate (se_gate_fused_kernel<8, 3>, hs_encoder.hip) as device helpers for a
// workgroup of ANY number of waves: the project GEMM's workgroups (hs_gemm_split.hip, the SEG form of gemm_split_kernel: 128 / 256 / 512 threads)
// derive the gate for themselves with these, and their gate equals hs_se_gate_fwd's FUSED form bit for bit, because the summation
// order of every output value is fixed by the value alone, never by the thread or the wave that forms it:
//   A  mean[c]  = (0 + u_0 + u_1 + ... + u_{qn-1}) * inv_hw, u_i = the channel's i-th unit: (p0 + p1) + (p2 + p3) of four partial sums
//                 (nblk % 4 == 0), else one partial sum; units pass through LDS in per-channel runs with one pad word
//   B  z[j]     = swish(wave_sum64(a) + b1[j]), lane l's a = the fma chain over columns 4 (l + 64 u) .. + 3, u ascending, from +0 -- a
//                 wave owns WHOLE reduce rows, so a row is summed the same way whichever wave takes it (a u whose columns do not
//                 exist is skipped: fma(0, 0, a) == a, the chain starts at +0 and can never reach -0)
//   C  gate[c]  = sigmoid(((q0 + q1) + (q2 + q3)) + b2[c]), q_i = the fma chain from +0 over j in [i jq, min((i + 1) jq, Csq)), jq = ceil(Csq / 4)
// se_gate_fused_kernel itself keeps its own text (its instantiations and tests are untouched); tests/test_hip_gemm_split_se.py holds
// the two to torch.equal.  Limits, as the FUSED route's: C % 4 == 0, C <= 768, Csq <= 32, units = C * (nblk % 4 ? nblk : nblk / 4) <= 2048.
#pragma once
#include "hs_common.h"

namespace hs {

constexpr int SEP_MAX_C = 768, SEP_MAX_CSQ = 32, SEP_MAX_UNITS = 2048;
// LDS of the phases in floats: mean | squeezed | gate | unit runs (one pad word per channel)
constexpr int SEP_MEAN = 0, SEP_ZS = SEP_MEAN + SEP_MAX_C, SEP_GATE = SEP_ZS + SEP_MAX_CSQ, SEP_PART = SEP_GATE + SEP_MAX_C;
constexpr int SEP_LDS_FLOATS = SEP_PART + SEP_MAX_UNITS + SEP_MAX_C;

// ---- A.  loads: PV units per thread, NTHR PV >= SEP_MAX_UNITS; pb = this frame's partial sums (C, nblk), 16-byte aligned when nblk % 4 == 0
template <int NTHR, int PV>
__device__ __forceinline__ void se_load_units(const float* __restrict__ pb, int nblk, int C, int tid, float4 (&pv)[PV]) {
    const bool vec = (nblk & 3) == 0;
    const int units = C * (vec ? nblk >> 2 : nblk);
    if (vec) {
#pragma unroll
        for (int k = 0; k < PV; ++k) pv[k] = reinterpret_cast<const float4*>(pb)[min(tid + NTHR * k, units - 1)];
    } else {
#pragma unroll
        for (int k = 0; k < PV; ++k) pv[k] = make_float4(pb[min(tid + NTHR * k, units - 1)], 0.0f, 0.0f, 0.0f);
    }
}

// units -> part (LDS) -> mean (LDS); two barriers, the second leaves mean[0..C) visible to every thread
template <int NTHR, int PV>
__device__ __forceinline__ void se_channel_means(const float4 (&pv)[PV], int nblk, int C, float inv_hw, int tid, float* part, float* mean) {
    const int qn = (nblk & 3) == 0 ? nblk >> 2 : nblk, units = C * qn;
#pragma unroll
    for (int k = 0; k < PV; ++k) {
        const int e = tid + NTHR * k;
        if (e < units) {
            const int ch = e / qn;
            part[ch * (qn + 1) + (e - ch * qn)] = (pv[k].x + pv[k].y) + (pv[k].z + pv[k].w);
        }
    }
    __syncthreads();
    for (int ch = tid; ch < C; ch += NTHR) {
        const float* run = part + ch * (qn + 1);
        float t = 0.0f;
        for (int i = 0; i < qn; ++i) t += run[i];
        mean[ch] = t * inv_hw;
    }
    __syncthreads();
}

// ---- B.  wave w of NWV owns reduce rows w, w + NWV, ...: RW NWV >= Csq; W1U: 256 W1U >= C
template <int NWV, int RW, int W1U>
__device__ __forceinline__ void se_load_reduce(const float* __restrict__ w1, const float* __restrict__ b1, int C, int Csq, int wave, int lane,
                                               float4 (&w1v)[RW][W1U], float (&b1v)[RW]) {
    const int c4 = C >> 2;
#pragma unroll
    for (int r = 0; r < RW; ++r) {
        const int j = min(wave + NWV * r, Csq - 1);
        b1v[r] = b1[j];
#pragma unroll
        for (int u = 0; u < W1U; ++u) {
            w1v[r][u] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (NWV * r < Csq && 64 * u < c4)                                       // uniform: rows / columns that exist
                w1v[r][u] = reinterpret_cast<const float4*>(w1 + (size_t)j * C)[min(lane + 64 * u, c4 - 1)];
        }
    }
}

// mean (LDS) -> zs (LDS); the caller's barrier makes zs visible
template <int NWV, int RW, int W1U>
__device__ __forceinline__ void se_squeeze_rows(const float4 (&w1v)[RW][W1U], const float (&b1v)[RW], const float* mean, int C, int Csq,
                                                int wave, int lane, float* zs) {
    const int c4 = C >> 2;
    float4 mv[W1U];
#pragma unroll
    for (int u = 0; u < W1U; ++u) {
        const int k = lane + 64 * u;
        mv[u] = *reinterpret_cast<const float4*>(mean + 4 * min(k, c4 - 1));
        if (k >= c4) mv[u] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
#pragma unroll
    for (int r = 0; r < RW; ++r) {
        if (NWV * r < Csq) {                                                        // uniform
            float a = 0.0f;
#pragma unroll
            for (int u = 0; u < W1U; ++u) {
                a = fmaf(w1v[r][u].x, mv[u].x, a); a = fmaf(w1v[r][u].y, mv[u].y, a);
                a = fmaf(w1v[r][u].z, mv[u].z, a); a = fmaf(w1v[r][u].w, mv[u].w, a);
            }
            a = wave_sum64(a);
            const int j = wave + NWV * r;
            if (lane == 0 && j < Csq) zs[j] = swishf(a + b1v[r]);
        }
    }
}

// ---- C.  one channel's gate from its four quarter sums; w2q[i][u] = w2t[min(i jq + u, Csq - 1)][c]
__device__ __forceinline__ void se_load_expand(const float* __restrict__ w2t, const float* __restrict__ b2, int C, int Csq, int c,
                                               float (&w2q)[4][8], float& b2v) {
    const int jq = (Csq + 3) >> 2;                                                  // <= 8
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int u = 0; u < 8; ++u) w2q[i][u] = w2t[(size_t)min(i * jq + u, Csq - 1) * C + c];
    b2v = b2[c];
}

__device__ __forceinline__ float se_channel_gate(const float (&w2q)[4][8], float b2v, const float* zs, int Csq) {
    const int jq = (Csq + 3) >> 2;
    float q[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int j0 = i * jq, j1 = min(j0 + jq, Csq);
        float acc = 0.0f;
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (j0 + u < j1) acc = fmaf(w2q[i][u], zs[min(j0 + u, SEP_MAX_CSQ - 1)], acc);
        q[i] = acc;
    }
    return sigmoidf_fast(((q[0] + q[1]) + (q[2] + q[3])) + b2v);
}

}  // namespace hs
