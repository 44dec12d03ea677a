// A dataset's label encoding as a compile-time variant of the label kernels (hyperseg_amd/utils/labels.py holds the rules and their CPU
// twin): CODEC_TABLE -- hyperseg/datasets/cityscapes.py:210-211, a raw id outside [0, len) becomes values[0], every other id v becomes
// values[v] -- and CODEC_COLORS -- hyperseg/datasets/camvid.py:96-98, the index of the LAST entry of a colour list equal to the pixel,
// `unmatched` where none is.  Both results are bytes.
//
// The kernels that take a codec end in a parameter pack `CA... ca` (as the loss kernels end in `CW... cw`): empty for CODEC_NONE, whose
// instantiations keep the arguments and the code they had, or (const int32_t* words, int n, int unmatched).
//   words, table:   64 words = the 256 table bytes, little-endian, entries from len on holding values[0] -- so a uint8 id is looked up as
//                   it is and an int64 id outside [0, 256) takes entry 0;
//   words, colours: word 0 the count, words 1..n the colours r | g << 8 | b << 16.
// The codec sits in LDS, staged once per workgroup: 256 bytes (one bank row: every bank holds one dword, so a gather by 64 lanes never
// meets two dwords on one bank), or up to 255 words that every lane walks in the same order (one address per step: a broadcast).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "hyperseg_hip.h"

namespace hs {

constexpr int CODEC_NONE = HS_CODEC_NONE, CODEC_TABLE = HS_CODEC_TABLE, CODEC_COLORS = HS_CODEC_COLORS;
constexpr int CODEC_TABLE_WORDS = 64;       // 256 bytes
constexpr int CODEC_MAX_COLORS = 255;

template <int CODEC> constexpr int codec_lds_words() { return CODEC == CODEC_TABLE ? CODEC_TABLE_WORDS : CODEC == CODEC_COLORS ? 256 : 1; }

struct CodecNone {};
struct CodecArgs { const int32_t* words; int n, unmatched; };
inline __device__ CodecNone codec_args() { return {}; }
inline __device__ CodecArgs codec_args(const int32_t* words, int n, int unmatched) { return {words, n, unmatched}; }

// the codec into LDS, by the first threads of the workgroup (at least 256), and the barrier; nothing for CODEC_NONE
template <int CODEC, typename A>
__device__ __forceinline__ void codec_stage(uint32_t* lds, const A& a, int tid) {
    if constexpr (CODEC == CODEC_TABLE) {
        if (tid < CODEC_TABLE_WORDS) lds[tid] = (uint32_t)a.words[tid];
        __syncthreads();
    } else if constexpr (CODEC == CODEC_COLORS) {
        if (tid < min(a.n, CODEC_MAX_COLORS)) lds[tid] = (uint32_t)a.words[1 + tid] & 0xffffffu;
        __syncthreads();
    }
}

__device__ __forceinline__ int codec_table(const uint32_t* lds, int v) { return reinterpret_cast<const uint8_t*>(lds)[v & 255]; }
__device__ __forceinline__ int codec_table(const uint32_t* lds, long long v) {
    return reinterpret_cast<const uint8_t*>(lds)[(unsigned long long)v < 256ull ? (int)v : 0];
}

// from the last entry down, out at the first hit: camvid.py's later entry overwrites an earlier one
__device__ __forceinline__ int codec_color(const uint32_t* lds, int n, int unmatched, uint32_t rgb) {
    for (int i = min(n, CODEC_MAX_COLORS) - 1; i >= 0; --i)
        if (lds[i] == rgb) return i;
    return unmatched;
}

// the raw label at element `at` of a (.., H, W) / (.., H, W, 3) image, encoded
template <int CODEC, typename TI, typename A>
__device__ __forceinline__ int codec_gather(const TI* __restrict__ x, size_t at, const uint32_t* lds, const A& a) {
    if constexpr (CODEC == CODEC_TABLE) {
        if constexpr (sizeof(TI) == 1) return codec_table(lds, (int)x[at]);
        else return codec_table(lds, (long long)x[at]);
    } else {
        static_assert(CODEC == CODEC_COLORS && sizeof(TI) == 1, "colours are uint8 (.., H, W, 3)");
        const uint8_t* __restrict__ p = reinterpret_cast<const uint8_t*>(x) + 3 * at;
        return codec_color(lds, a.n, a.unmatched, (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16);
    }
}

// host side: what every entry that takes a codec checks before its first launch
inline int codec_check(const int32_t* words, int32_t kind, int32_t in_dtype, int32_t n, int32_t unmatched) {
    if (!words || (kind != HS_CODEC_TABLE && kind != HS_CODEC_COLORS)) return HS_ERR_BAD_ARG;
    if (kind == HS_CODEC_TABLE && (n < 1 || n > 256 || (in_dtype != HS_EVAL_U8 && in_dtype != HS_EVAL_I64))) return HS_ERR_BAD_ARG;
    if (kind == HS_CODEC_COLORS && (n < 1 || n > CODEC_MAX_COLORS || in_dtype != HS_EVAL_U8 || unmatched < 0 || unmatched > 255)) return HS_ERR_BAD_ARG;
    return HS_OK;
}

}  // namespace hs
