// Pillow's ImageFilter.GaussianBlur on uint8 RGB frames, on the device, with Pillow's bytes: what the reference's RandomGaussianBlur
// (hyperseg/datasets/seg_transforms.py:361-378) runs on a host thread.  Pillow's filter is an extended box blur -- three box passes
// along the rows, then three along the columns, each reading and writing BYTES; the arithmetic is restated in
// hyperseg_amd/utils/blur.py, which is the specification and the CPU implementation this file is held to:
//   one pass along a line of n pixels: out[x] = (ww * sum(in[clamp(x + d)], |d| <= r) + fw * (in[clamp(x - r - 1)] + in[clamp(x + r + 1)])
//   + 2^23) >> 24 in 32 unsigned bits, the clamp to [0, n - 1] applied to the pass's own input.  r, ww and fw follow from the Gaussian's
//   sigma on the host (float32 steps, utils/blur.py) and are DATA here: one 4-word record per sample in a device table
//   (hyperseg_hip.h), so a captured graph replays with whatever the table holds at that moment.  Every branch on the record is uniform
//   over a workgroup (blockIdx.y = sample).
//
// hs_gaussian_blur_fwd, per call: TWO launches, rows then columns, a uint8 intermediate of the frames' size between them.
//   * Both launches tile the image; a workgroup loads its tile plus 3 (r + 1) pixels beyond each end along the blurred axis (cut to the
//     line) into LDS as bytes, runs the three dependent passes there -- two LDS buffers, a barrier after each pass, pass k producing
//     the tile widened by (3 - k)(r + 1) so that the next finds every tap (hs_blur_px.h) -- and stores the tile.  A tap index is clamped
//     into what the pass before produced, which for every tap an output needs is the clamp to the line: the passes see the line's own
//     ends exactly where the tile reaches them and nowhere else, whatever the radius, also one that exceeds the line.
//   * A thread slides one window over 4 consecutive outputs of a line: 2 r + 3 byte reads for the first, 2 for each further one.
//   * rows: a line is (row, channel); 'hwc' tiles are 16 rows x 128 pixels of 3 interleaved bytes, a 'chw' plane's 48 rows x 128.
//     columns: a line is a byte column; tiles are 64 rows x 144 bytes ('hwc': 48 pixels) or x 128 (a plane).  The column launch ends the
//     call: it stores bytes in the input's layout or -- through InputNorm's table in LDS (hs_ingest.h) -- float32 planar, 16 bytes per
//     lane where W and the destination allow it.
//   * A sample whose record says "not applied" skips the passes (both launches copy its tiles, the second through the table); one
//     whose record asks for r outside [0, HS_BLUR_MAX_RADIUS] is treated the same and the row launch sets its status word.  r is the
//     only word of a record that moves an address, and it is checked before it does.
// LDS: rows 2 x 16 x 672 = 21 KB, columns 2 x 160 x 144 = 45 KB (+ 3 KB table).
#include <hip/hip_runtime.h>
#include <cstdint>
#include "hyperseg_hip.h"
#include "hs_common.h"
#include "hs_ingest.h"
#include "hs_blur_px.h"

namespace hs {

using blur_f32x4 = __attribute__((ext_vector_type(4))) float;

struct BlurArgs {
    const uint8_t* x; uint8_t* tmp; void* y; const float* norm; const int32_t* table; int32_t* status;
    int H, W, tiles_x;
};

// bytes [j0, j0 + nb) of `rows` rows: global (pitch row_bytes) <-> LDS (pitch lds_pitch); a wave per row, lanes along it
__device__ __forceinline__ void blur_tile_in(const uint8_t* __restrict__ src, size_t row_bytes, uint8_t* __restrict__ lds, int lds_pitch,
                                             int rows, int nb, int tid) {
    for (int s = tid >> 6; s < rows; s += 4)
        for (int j = tid & 63; j < nb; j += 64) lds[s * lds_pitch + j] = src[s * row_bytes + j];
}

__device__ __forceinline__ void blur_tile_out(const uint8_t* __restrict__ lds, int lds_pitch, uint8_t* __restrict__ dst, size_t row_bytes,
                                              int rows, int nb, int tid) {
    for (int s = tid >> 6; s < rows; s += 4)
        for (int j = tid & 63; j < nb; j += 64) dst[s * row_bytes + j] = lds[s * lds_pitch + j];
}

// x -> tmp, blurred along W.  CH bytes per pixel: 3 = 'hwc' (gridDim.z 1), 1 = one plane of 'chw' (gridDim.z 3).
template <int CH>
__global__ __launch_bounds__(256)
void blur_rows_kernel(const BlurArgs a) {
    constexpr int ROWS = BLUR_ROW_BYTES / CH;
    constexpr int PITCH = (BLUR_ROW_TILE + 2 * BLUR_HALO) * CH;
    __shared__ __attribute__((aligned(16))) uint8_t buf[2][ROWS * PITCH];
    const int tid = (int)threadIdx.x;
    const size_t b = blockIdx.y;
    const BlurRec rec = blur_record(a.table, b);
    if (blockIdx.x == 0 && blockIdx.z == 0 && tid == 0) a.status[b] = rec.declined ? HS_BLUR_STATUS_RADIUS : 0;
    const int tx = (int)(blockIdx.x % (unsigned)a.tiles_x), ty = (int)(blockIdx.x / (unsigned)a.tiles_x);
    const int t0 = tx * BLUR_ROW_TILE, t1 = min(t0 + BLUR_ROW_TILE, a.W) - 1;
    const int y0 = ty * ROWS, rows = min(ROWS, a.H - y0);
    const size_t row_bytes = (size_t)CH * a.W;
    const size_t base = ((b * gridDim.z + blockIdx.z) * a.H + y0) * row_bytes;
    BlurSpan valid = blur_span(t0, t1, a.W, rec.r, rec.blur, 0);
    const int e0 = valid.lo;
    blur_tile_in(a.x + base + (size_t)e0 * CH, row_bytes, buf[0], PITCH, rows, (valid.hi - e0 + 1) * CH, tid);
    __syncthreads();
    int cur = 0;
    if (rec.blur) {
        for (int k = 1; k <= BLUR_PASSES; ++k) {
            const BlurSpan want = blur_span(t0, t1, a.W, rec.r, true, k);
            blur_pass<CH, false>(buf[cur], buf[cur ^ 1], rows, PITCH, CH, e0, want, valid, rec.r, rec.ww, rec.fw, tid);
            __syncthreads();
            cur ^= 1;
            valid = want;
        }
    }
    blur_tile_out(buf[cur] + (t0 - e0) * CH, PITCH, a.tmp + base + (size_t)t0 * CH, row_bytes, rows, (t1 - t0 + 1) * CH, tid);
}

// tmp -> y, blurred along H; y uint8 in the input's layout or (NORM) float32 (B, 3, H, W) through the table
template <int CH, bool NORM>
__global__ __launch_bounds__(256)
void blur_cols_kernel(const BlurArgs a) {
    constexpr int TWB = CH == 3 ? BLUR_COL_BYTES_HWC : BLUR_COL_BYTES_CHW;
    __shared__ __attribute__((aligned(16))) uint8_t buf[2][(BLUR_COL_TILE + 2 * BLUR_HALO) * TWB];
    __shared__ float tab[NORM ? INGEST_TABLE_FLOATS : 1];
    const int tid = (int)threadIdx.x;
    const size_t b = blockIdx.y;
    const BlurRec rec = blur_record(a.table, b);
    if constexpr (NORM) ingest_table_to_lds(a.norm, tab, tid);
    const int tx = (int)(blockIdx.x % (unsigned)a.tiles_x), ty = (int)(blockIdx.x / (unsigned)a.tiles_x);
    const size_t row_bytes = (size_t)CH * a.W;
    const int j0 = tx * TWB, nb = (int)min((size_t)TWB, row_bytes - j0);
    const int t0 = ty * BLUR_COL_TILE, t1 = min(t0 + BLUR_COL_TILE, a.H) - 1;
    const size_t plane = (b * gridDim.z + blockIdx.z) * a.H * row_bytes;
    BlurSpan valid = blur_span(t0, t1, a.H, rec.r, rec.blur, 0);
    const int e0 = valid.lo;
    blur_tile_in(a.tmp + plane + (size_t)e0 * row_bytes + j0, row_bytes, buf[0], TWB, valid.hi - e0 + 1, nb, tid);
    __syncthreads();
    int cur = 0;
    if (rec.blur) {
        for (int k = 1; k <= BLUR_PASSES; ++k) {
            const BlurSpan want = blur_span(t0, t1, a.H, rec.r, true, k);
            blur_pass<TWB, true>(buf[cur], buf[cur ^ 1], 1, 0, TWB, e0, want, valid, rec.r, rec.ww, rec.fw, tid);
            __syncthreads();
            cur ^= 1;
            valid = want;
        }
    }
    const uint8_t* __restrict__ done = buf[cur] + (t0 - e0) * TWB;
    const int rows = t1 - t0 + 1;
    if constexpr (!NORM) {
        blur_tile_out(done, TWB, static_cast<uint8_t*>(a.y) + plane + (size_t)t0 * row_bytes + j0, row_bytes, rows, nb, tid);
    } else {
        // groups of 4 pixels of one (row, channel): 16 bytes of floats per lane
        constexpr int NX4 = TWB / CH / 4;
        const int x0 = j0 / CH, npx = nb / CH;
        float* __restrict__ y = static_cast<float*>(a.y);
        const bool vec = (a.W & 3) == 0 && (reinterpret_cast<uintptr_t>(y) & 15) == 0;
        const int total = rows * CH * NX4;
        for (int id = tid; id < total; id += 256) {
            const int x = (id % NX4) * 4, q = id / NX4;
            const int c = CH == 3 ? q % 3 : (int)blockIdx.z, row = CH == 3 ? q / 3 : q;
            const int cnt = min(4, npx - x);
            if (cnt <= 0) continue;
            const uint8_t* __restrict__ s = done + row * TWB + x * CH + (CH == 3 ? c : 0);
            float* __restrict__ d = y + ((b * 3 + c) * a.H + (t0 + row)) * (size_t)a.W + x0 + x;
            if (vec && cnt == 4) {
                *reinterpret_cast<blur_f32x4*>(d) = blur_f32x4{ingest_dequant(tab, c, s[0]), ingest_dequant(tab, c, s[CH]),
                                                               ingest_dequant(tab, c, s[2 * CH]), ingest_dequant(tab, c, s[3 * CH])};
            } else {
                for (int i = 0; i < cnt; ++i) d[i] = ingest_dequant(tab, c, s[i * CH]);
            }
        }
    }
}

}  // namespace hs

using namespace hs;

extern "C" int hs_gaussian_blur_fwd(const uint8_t* x, int32_t layout, int32_t batch, int32_t H, int32_t W, const int32_t* table,
                                    uint8_t* tmp, const float* norm_table, void* y, int32_t* status, void* stream) {
    if (!x || !y || !tmp || !table || !status || batch <= 0 || H <= 0 || W <= 0) return HS_ERR_BAD_ARG;
    if (layout != HS_LAYOUT_HWC && layout != HS_LAYOUT_CHW) return HS_ERR_BAD_ARG;
    if (batch > 65535 || H > BLUR_MAX_DIM || W > BLUR_MAX_DIM) return HS_ERR_UNSUPPORTED;
    const bool hwc = layout == HS_LAYOUT_HWC;
    const int ch = hwc ? 3 : 1;
    BlurArgs a;
    a.x = x; a.tmp = tmp; a.y = y; a.norm = norm_table; a.table = table; a.status = status; a.H = H; a.W = W;
    hipStream_t s = (hipStream_t)stream;
    const dim3 block(256);
    // tiles per image: at most 256 x 2048 (rows) and 683 x 512 (columns), far inside a grid dimension
    a.tiles_x = (W + BLUR_ROW_TILE - 1) / BLUR_ROW_TILE;
    const int row_tiles_y = (H + BLUR_ROW_BYTES / ch - 1) / (BLUR_ROW_BYTES / ch);
    const dim3 row_grid((unsigned)(a.tiles_x * row_tiles_y), (unsigned)batch, hwc ? 1u : 3u);
    if (hwc) hipLaunchKernelGGL(blur_rows_kernel<3>, row_grid, block, 0, s, a);
    else hipLaunchKernelGGL(blur_rows_kernel<1>, row_grid, block, 0, s, a);
    const int twb = hwc ? BLUR_COL_BYTES_HWC : BLUR_COL_BYTES_CHW;
    a.tiles_x = (ch * W + twb - 1) / twb;
    const int col_tiles_y = (H + BLUR_COL_TILE - 1) / BLUR_COL_TILE;
    const dim3 col_grid((unsigned)(a.tiles_x * col_tiles_y), (unsigned)batch, hwc ? 1u : 3u);
    if (norm_table) {
        if (hwc) hipLaunchKernelGGL((blur_cols_kernel<3, true>), col_grid, block, 0, s, a);
        else hipLaunchKernelGGL((blur_cols_kernel<1, true>), col_grid, block, 0, s, a);
    } else {
        if (hwc) hipLaunchKernelGGL((blur_cols_kernel<3, false>), col_grid, block, 0, s, a);
        else hipLaunchKernelGGL((blur_cols_kernel<1, false>), col_grid, block, 0, s, a);
    }
    return launch_status();
}
