// The per-line code of Pillow's GaussianBlur (an extended box blur) on bytes held in LDS, shared by the row launch and the column launch
// of hs_blur.hip: a sample's record, the tile geometry, and ONE box pass over a tile.  The arithmetic is specified in
// hyperseg_amd/utils/blur.py and described at the top of hs_blur.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "hyperseg_hip.h"

namespace hs {

constexpr int BLUR_WORDS = HS_BLUR_TABLE_WORDS;
constexpr int BLUR_PASSES = 3;                                         // box passes per direction
constexpr int BLUR_HALO = BLUR_PASSES * (HS_BLUR_MAX_RADIUS + 1);      // pixels a tile reads beyond each of its ends, at most
constexpr int BLUR_RUN = 4;                                            // consecutive outputs of one line a thread slides its window over
constexpr int BLUR_MAX_DIM = HS_BLUR_MAX_DIM;

constexpr int BLUR_ROW_TILE = 128;                                     // row launch: pixels of a line per workgroup ...
constexpr int BLUR_ROW_BYTES = 48;                                     // ... and rows x bytes per pixel: 16 rows of 'hwc', 48 of a plane
constexpr int BLUR_COL_TILE = 64;                                      // column launch: rows per workgroup ...
constexpr int BLUR_COL_BYTES_HWC = 144, BLUR_COL_BYTES_CHW = 128;      // ... and byte columns: 48 'hwc' pixels, 128 of a plane

struct BlurRec {
    int r;                                     // 0 <= r <= HS_BLUR_MAX_RADIUS whatever the table holds
    unsigned ww, fw;
    bool blur, declined;                       // the passes run; the record asks for a radius this file does not take
};

// ww and fw are used as they are: no value of theirs moves an address, and (anything) >> 24 is a byte
__device__ __forceinline__ BlurRec blur_record(const int32_t* __restrict__ table, size_t b) {
    const int32_t* __restrict__ t = table + b * BLUR_WORDS;
    BlurRec rec;
    const bool apply = t[0] != 0;
    const int r = t[1];
    rec.declined = apply && (r < 0 || r > HS_BLUR_MAX_RADIUS);
    rec.blur = apply && !rec.declined;
    rec.r = rec.blur ? r : 0;
    rec.ww = (unsigned)t[2];
    rec.fw = (unsigned)t[3];
    return rec;
}

// A tile's extent along the blurred axis of n pixels, for the tile's own pixels [t0, t1]: what pass k = 1..3 must produce is the tile
// widened by (3 - k)(r + 1) and cut to the line; pass 0 is what is loaded.
struct BlurSpan { int lo, hi; };
__device__ __forceinline__ BlurSpan blur_span(int t0, int t1, int n, int r, bool blur, int k) {
    const int reach = blur ? (BLUR_PASSES - k) * (r + 1) : 0;
    return BlurSpan{max(t0 - reach, 0), min(t1 + reach, n - 1)};
}

// One box pass of a 256-thread workgroup over an LDS tile.  A LINE is the bytes src[off + (p - e0) * pstride] for the pixels p of
// [valid.lo, valid.hi] -- what the pass before produced (or the load), e0 <= valid.lo the pixel at offset 0 -- with
// off = slow * slow_pitch + fast, fast < FAST, slow < n_slow.  The outputs [want.lo, want.hi] of every line go to dst at the same
// offsets.  Lanes run over `fast` first, then over runs of BLUR_RUN outputs, then over `slow`.  Every read index is clamped into
// `valid`: for the taps an output needs that IS the clamp to the line (valid covers want widened by r + 1, cut to the line), and a tap
// no output needs reads a byte of the tile all the same.  n_slow == 1 (ONE_SLOW) saves the division.
template <int FAST, bool ONE_SLOW>
__device__ __forceinline__ void blur_pass(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int n_slow, int slow_pitch, int pstride,
                                          int e0, BlurSpan want, BlurSpan valid, int r, unsigned ww, unsigned fw, int tid) {
    const int n_runs = (want.hi - want.lo + BLUR_RUN) / BLUR_RUN;
    const int total = FAST * n_runs * n_slow;
    for (int id = tid; id < total; id += 256) {
        const int fast = id % FAST, t = id / FAST;
        const int slow = ONE_SLOW ? 0 : t / n_runs;
        const int run = ONE_SLOW ? t : t - slow * n_runs;
        const int off = slow * slow_pitch + fast;
        const int g = want.lo + run * BLUR_RUN;
        auto at = [&](int p) -> unsigned { return src[off + (min(max(p, valid.lo), valid.hi) - e0) * pstride]; };
        unsigned sum = 0;
        for (int d = -r; d <= r; ++d) sum += at(g + d);
        unsigned left = at(g - r - 1), right = at(g + r + 1);
#pragma unroll
        for (int i = 0; i < BLUR_RUN; ++i) {
            if (g + i <= want.hi) dst[off + (g + i - e0) * pstride] = (uint8_t)((ww * sum + fw * (left + right) + (1u << 23)) >> 24);
            const unsigned next_left = at(g + i - r);                  // leaves the window of g + i + 1 and is its left outer tap
            sum += right - next_left;                                  // its right end is the outer tap of g + i
            left = next_left;
            right = at(g + i + r + 2);
        }
    }
}

}  // namespace hs
