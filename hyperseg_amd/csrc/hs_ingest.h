// uint8 frames on the device: the ONE dequantisation shared by hs_image_ingest_fwd (hs_ingest.hip) and the uint8 form of the stem +
// depthwise launch (hs_mbconv_lean.hip).  The transform is data: a (3, 256) float32 table built on the host by the arithmetic of the
// reference's ToTensor + Normalize, table[c][v] = (float(v) / 255 - mean[c]) / std[c] (hyperseg_amd.utils.inference.InputNorm), so
// looking a byte up IS the transform, bit for bit -- no device arithmetic whose rounding would have to be argued about.
#pragma once
#include <hip/hip_runtime.h>

namespace hs {

constexpr int INGEST_CHANNELS = 3;
constexpr int INGEST_TABLE_FLOATS = INGEST_CHANNELS * 256;      // 3 KB: kept in LDS by both kernels

// every thread of a 256-thread workgroup: global table -> LDS (the caller puts a barrier between this and the first lookup)
__device__ __forceinline__ void ingest_table_to_lds(const float* __restrict__ table, float* __restrict__ tab, int tid) {
#pragma unroll
    for (int i = 0; i < INGEST_TABLE_FLOATS / 256; ++i) tab[i * 256 + tid] = table[i * 256 + tid];
}

// the normalised value of byte v (0..255) of channel c
__device__ __forceinline__ float ingest_dequant(const float* __restrict__ tab, int c, unsigned v) { return tab[c * 256 + (int)v]; }

}  // namespace hs
