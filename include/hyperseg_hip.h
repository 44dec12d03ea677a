/*
 * hyperseg_hip.h -- C ABI of libhyperseg_hip.so: the MI355X (gfx950) kernels of the HyperSeg
 * decoder hot path (dynamic patch-wise convolution + inter-stage glue).
 *
 * The reference (YuvalNirkin/hyperseg) has no FFI layer: its boundary for this path is the
 * nn.Module API of hyperseg/models/layers/{meta_sequential,meta_conv,meta_patch}.py and the
 * HyperPatch* classes of hyperseg/models/hyperseg_v*.py.  The host-side mirror of that API
 * lives in hyperseg_amd/models/ and binds exactly these entry points with ctypes
 * (hyperseg_amd/_hip.py); INTEGRATION.md shows the stub a reference maintainer would add.
 *
 * Conventions
 *  - All tensors are fp32, NCHW, contiguous, device pointers BORROWED for the duration of the
 *    call; the library allocates nothing, keeps no global mutable state, never synchronises the
 *    device, and enqueues on the caller's stream (hipStream_t passed as void*).  Re-entrant.
 *  - Every function returns 0 on success, a negative hs_status on rejected arguments (nothing
 *    enqueued), or a positive hipError_t if the launch itself failed.
 *  - "grid" = the (fh, fw) weight grid; a level of resolution (H, W) has patches of
 *    ph = H/fh by pw = W/fw pixels; patch (b, i, j) has linear index p = (b*fh + i)*fw + j.
 *  - A *bank* is the per-patch filter bank in PATCH-MAJOR layout: bank[p*ld + m], m < rows.
 *    Row order is chosen by the producer (hs_signal2weights_fwd / hs_bank_pack_fwd) through a
 *    row map; the consumers document the order they expect.
 *  - A *stage input* is the channel concatenation the reference builds with torch.cat
 *    (hyperseg_v1_0.py:231-240): [2 coord channels | skip feature | previous level output,
 *    optionally bilinearly resized]; it is generated on the fly, never materialised.
 */
#ifndef HYPERSEG_HIP_H
#define HYPERSEG_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HS_ABI_VERSION 1

typedef enum {
    HS_OK = 0,
    HS_ERR_BAD_ARG = -1,       /* null pointer / non-positive size / inconsistent shapes */
    HS_ERR_NOT_DIVISIBLE = -2, /* H % fh != 0 or W % fw != 0 (hyperseg_v1_0.py:490-494 view error) */
    HS_ERR_UNSUPPORTED = -3,   /* shape outside what the kernels were instantiated for */
    HS_ERR_LDS = -4            /* tile does not fit the 160 KiB LDS */
} hs_status;

/* Epilogue activation.  The reference's decoder uses ReLU / ReLU6 only (hyperseg_v1_0.py:115, 283, 729); SWISH (x * sigmoid(x),
 * efficientnet_utils.py:58-79) is what the encoder-side entry points take, and the patch-convolution epilogues accept it too. */
typedef enum { HS_ACT_NONE = 0, HS_ACT_RELU = 1, HS_ACT_RELU6 = 2, HS_ACT_SWISH = 3 } hs_act;
typedef enum { HS_PAD_ZEROS = 0, HS_PAD_REFLECT = 1, HS_PAD_REPLICATE = 2, HS_PAD_CIRCULAR = 3 } hs_pad_mode;
typedef enum { HS_PREV_NONE = 0, HS_PREV_SAME = 1, HS_PREV_BILINEAR = 2 } hs_prev_mode;

/* Stage input: replaces F.interpolate + 2x torch.cat + get_image_coordinates
 * (hyperseg_v1_0.py:203-240; v0_1: hyperseg_v0_1.py:186-198, 240-246). */
typedef struct {
    const float* skip;   /* (B, c_skip, H, W) */
    const float* prev;   /* (B, c_prev, Hp, Wp) or NULL */
    int32_t batch, H, W;
    int32_t c_skip, c_prev;
    int32_t Hp, Wp;      /* resolution of prev; bilinear (align_corners=False) to (H, W) if prev_mode == 2 */
    int32_t coords;      /* 1: prepend x in [-1,1] over W (ch 0) and y over H (ch 1), linspace endpoints inclusive */
    int32_t prev_mode;   /* hs_prev_mode */
} hs_stage_input;

/* Per-channel affine applied after a convolution: y = act(conv * scale + shift).  Inference
 * BatchNorm folded by hs_bn_fold_fwd; scale == NULL means identity. */
typedef struct {
    const float* scale;
    const float* shift;
    int32_t act;         /* hs_act */
} hs_epilogue;

/* ABI version / build info (sanity check for the ctypes binding). */
int hs_version(void);
const char* hs_build_info(void);

/* a9: "hypernetwork head emits per-patch weights" -- grouped 1x1 conv, bias-free.
 * Replaces signal2weights(...)[:, :hp] (hyperseg_v1_0.py:479-484, 321-326;
 * hyperseg_v1_0_unify.py:302-309) AND the permute/reshape copy that follows it.
 *   bank[p*ld + n] = sum_k wsw_t[k*wc + n] * signal[b, signal_index + g(n)*cs_g + k, i, j],
 *   n < rows <= wc,  g(n) = n / (wc / groups).  Runs on the f32 matrix cores (v_mfma_f32_16x16x4_f32).
 * wsw_t is the Conv2d weight (wc, cs_g, 1, 1) TRANSPOSED to (cs_g, wc) (done once by the host). */
typedef struct hs_s2w_layer hs_s2w_layer;
int hs_signal2weights_fwd(const float* signal, int32_t batch, int32_t c_signal, int32_t fh, int32_t fw,
                          int32_t signal_index, int32_t signal_channels, int32_t groups,
                          const float* wsw_t, int32_t wc, int32_t rows,
                          float* bank, int64_t ld, void* stream);

/* The same for up to 8 signal2weights layers (all levels of a decoder) in ONE launch: every layer reads its own
 * slice of the same signal and writes its own bank. */
struct hs_s2w_layer {
    int32_t signal_index, signal_channels, groups;
    const float* wsw_t;        /* (signal_channels/groups, wc) */
    int32_t wc;
    int32_t rows;
    float* bank;
    int64_t ld;
    const float* wsw_blk;      /* optional: the same weight packed by hs_s2w_pack_fwd (hs_s2w_pack_floats floats).  When EVERY
                                * layer brings one and fh * fw is a multiple of 4, the launch takes the blocked form: operands
                                * staged through LDS by DMA, 64-row x 64-patch blocks; results are bit-identical. */
};
/* Packs the transposed conv weight of one signal2weights layer into the blocked kernel's operand images (once per parameter
 * version; wsw_t as above).  hs_s2w_pack_floats = the size of `out` in floats. */
int64_t hs_s2w_pack_floats(int32_t signal_channels, int32_t groups, int32_t wc);
int hs_s2w_pack_fwd(const float* wsw_t, int32_t signal_channels, int32_t groups, int32_t wc, float* out, void* stream);
int hs_signal2weights_multi_fwd(const float* signal, int32_t batch, int32_t c_signal, int32_t fh, int32_t fw,
                                const hs_s2w_layer* layers, int32_t n_layers, void* stream);

/* Re-layout of a reference-layout weight tensor (B, hp_total, fh, fw) (channel-major, as
 * MetaPatch.forward / HyperPatchInvertedResidual receive it: meta_patch.py:49,
 * hyperseg_v1_0_unify.py:335-349) into a patch-major bank:
 *   bank[p*ld + m] = w[b, ch_offset + m, i, j]. */
int hs_bank_pack_fwd(const float* w, int32_t batch, int32_t hp_total, int32_t fh, int32_t fw,
                     int32_t ch_offset, int32_t rows, float* bank, int64_t ld, void* stream);

/* Inference BatchNorm folding: scale = gamma / sqrt(var + eps), shift = beta - mean * scale,
 * for n channels (nn.BatchNorm2d eval semantics; eps 1e-5 in every reference module). */
int hs_bn_fold_fwd(const float* gamma, const float* beta, const float* mean, const float* var, float eps,
                   int32_t n, float* scale, float* shift, void* stream);

/* Op A / Op B: dynamic patch-wise k x k convolution with image-level padding, stride 1,
 * dilation 1.  Replaces MetaPatch.forward + MetaConv2d.forward (meta_patch.py:35-57,
 * meta_conv.py:163-186), HyperPatchNoPadding.forward (hyperseg_v1_0.py:486-498) and
 * HyperPatch.forward (hyperseg_v1_0.py:543-557), plus the BatchNorm/activation modules that
 * follow them in make_*_patch_conv2d_block.  With fh = fw = 1 it is MetaConv2d itself.
 * Bank row order (natural): m = ((o*cin_g + c)*k + ky)*k + kx, cin_g = cin/groups.
 *   y[b,o,y,x] = act(scale[o] * sum W[m] * in_pad[b, grp(o)*cin_g + c, y+ky-pad, x+kx-pad] + shift[o]) */
int hs_patch_conv_fwd(const hs_stage_input* in, int32_t fh, int32_t fw,
                      const float* bank, int64_t ld,
                      int32_t c_out, int32_t k, int32_t pad, int32_t pad_mode, int32_t groups,
                      const hs_epilogue* ep, float* y, void* stream);

/* hs_patch_conv_fwd with k = 1 (no padding) AND hs_signal2weights_multi_fwd for `layers` as ONE heterogeneous launch: the
 * first batch*fh*fw workgroups are the patch convolution's (one per patch), the rest are signal2weights blocks writing the
 * banks of LATER decoder levels (they depend on the signal only).  The k = 1 levels (hyperseg_v1_0.py:486-498) are
 * latency-bound launches that leave most of the chip idle; the bank producer (hyperseg_v1_0.py:473-484) fills that time
 * instead of preceding level 0 as its own launch.  Results are bit-identical to the two separate calls.
 * Returns HS_ERR_UNSUPPORTED -- nothing launched -- when either half would not take the form this launch is built from
 * (large patches, a layer without wsw_blk, unaligned operands, >= 1024 two-pixel patches): issue the two calls instead.
 * signal (batch, c_signal, sfh, sfw); every layer's bank must be distinct from `bank` and `y`. */
int hs_patch_conv_s2w_fwd(const hs_stage_input* in, int32_t fh, int32_t fw, const float* bank, int64_t ld,
                          int32_t c_out, int32_t groups, const hs_epilogue* ep, float* y,
                          const float* signal, int32_t batch, int32_t c_signal, int32_t sfh, int32_t sfw,
                          const hs_s2w_layer* layers, int32_t n_layers, void* stream);

/* The decoder's three coarse k = 1 levels (patches of 1 x 1, 2 x 2 and 4 x 4 pixels: MultiScaleDecoder.forward's first three
 * iterations, hyperseg_v1_0.py:221-253, each `cat(coords, skip, bilinear2x(prev))` -> HyperPatchNoPadding (:486-498) -> BatchNorm ->
 * ReLU, :728-760) as ONE launch: one workgroup per grid cell walks level 0 -> 1 -> 2, every bank / skip pixel / BatchNorm row of
 * all three levels requested at the top of the kernel, and a level's outputs handed to the NEIGHBOURING cells' workgroups inside
 * the launch (the 2x bilinear upsample reads a one-pixel ring around a cell) as 8-byte {value, generation} granules -- one
 * agent-scope store each, polled by the consumer until the generation matches.  Same values as three hs_patch_conv_fwd calls
 * (same operations per output; the dot products' summation order differs at rounding level).
 *   levels[l]: skip (batch, c_skip, fh << l, fw << l); bank of the level, patch-major, rows o * c_in + c with
 *              c_in = 2 + c_skip + c_out of the previous level (0 for l = 0), row stride ld (multiple of 4, 16-byte aligned);
 *              scale / shift / act: the epilogue (scale null: none).   y (batch, levels[2].c_out, 4 fh, 4 fw).
 *   workspace: hs_k1_chain_workspace() bytes, 16-byte aligned, ZERO-FILLED ONCE by the caller and then left alone: it carries the
 *              generation counter between calls (kernel arguments are frozen under graph replay, so the state lives in memory the
 *              kernel owns).  One workspace per (batch, fh, fw) and per stream: two launches must not share it concurrently.
 *              Its first 32-bit word is an error flag: non-zero after a launch whose workgroups gave up waiting for a neighbour
 *              (bounded spins: ~0.2 s) -- the results of that launch are invalid.
 * HS_ERR_UNSUPPORTED -- nothing launched -- unless n_levels == 3, every bank fits its LDS-DMA budget (24 / 12 / 4 KB),
 * c_out <= 64, c_skip * pixels <= 256 per level, AND the whole grid (batch * fh * fw workgroups) is resident at once on the
 * current device (workgroups wait for their neighbours): the caller then issues the three hs_patch_conv_fwd calls. */
typedef struct hs_k1_level {
    const float* skip; int32_t c_skip;
    const float* bank; int64_t ld;
    int32_t c_out;
    const float* scale; const float* shift; int32_t act;
} hs_k1_level;
int64_t hs_k1_chain_workspace(int32_t batch, int32_t fh, int32_t fw, const hs_k1_level* levels, int32_t n_levels);   /* bytes, or a negative hs_status */
int hs_k1_chain_fwd(int32_t batch, int32_t fh, int32_t fw, const hs_k1_level* levels, int32_t n_levels, void* workspace,
                    float* y, void* stream);

/* The same launch carrying the decoder's FIRST INVERTED-RESIDUAL level as well (HyperPatchInvertedResidual on 8 x 8-pixel patches,
 * hyperseg_v1_0.py:281-376; Op C of hs_patch_ir_fwd): behind level 2 every workgroup hands its 4 x 4 outputs to the neighbouring
 * cells, assembles the reflect halo tile of ITS patch (coords, skip, bilinear 2x of level 2) and runs pw1 -> BN1 -> ReLU6 ->
 * depthwise 3 x 3 -> BN2 -> ReLU6 -> pw3 -> BN3 with the hidden activations in LDS -- exact f32 (v_mfma_f32_16x16x4_f32 for the two
 * 1 x 1 layers, v_fma_f32 for the depthwise one).  ir == NULL: hs_k1_chain_fwd.
 *   ir: skip (batch, c_skip, 8 fh, 8 fw); bank rows [pw1: hidden x c_in | depthwise: hidden x 9 | pw3: c_out x hidden] with
 *       c_in = 2 + c_skip + levels[2].c_out, row stride ld; s1 / b1 ... s3 / b3: the three folded BatchNorms (a null scale: none).
 *       No residual connection (the reference adds one only when c_in == c_out, which no decoder level has).
 *   y (batch, ir->c_out, 8 fh, 8 fw).  workspace: hs_decoder_chain_workspace() bytes, otherwise as for hs_k1_chain_fwd.
 * HS_ERR_UNSUPPORTED in addition when hidden > 64 or not a multiple of 4, c_out > 64, c_skip x 100 > 768, levels[2].c_out > 21,
 * the bank is larger than 12 KB, or the workgroup's LDS (~63 KB at HyperSeg-M) would pass 64 KB. */
typedef struct hs_chain_ir_level {
    const float* skip; int32_t c_skip;
    const float* bank; int64_t ld;
    int32_t hidden, c_out;
    const float* s1; const float* b1; const float* s2; const float* b2; const float* s3; const float* b3;
} hs_chain_ir_level;
int64_t hs_decoder_chain_workspace(int32_t batch, int32_t fh, int32_t fw, const hs_k1_level* levels, int32_t n_levels,
                                   const hs_chain_ir_level* ir);
int hs_decoder_chain_fwd(int32_t batch, int32_t fh, int32_t fw, const hs_k1_level* levels, int32_t n_levels,
                         const hs_chain_ir_level* ir, void* workspace, float* y, void* stream);

/* MetaConv2d.forward with the reference's FULL argument set (meta_conv.py:141-186): per-sample weights w (B, rows >=
 * c_out * c_in/groups * kh * kw, row stride ldw; natural order ((o*cin_g + c)*kh + ky)*kw + kx), non-square kernels, stride,
 * dilation, any padding amounts per side and mode (F.pad semantics for reflect / replicate / circular, zero padding
 * otherwise), groups; optional BatchNorm affine + activation.  y (B, c_out, Ho, Wo),
 * Ho = (H + pad_top + pad_bottom - dil_h (kh - 1) - 1) / stride_h + 1.  The four pad amounts are explicit because the
 * reference pads asymmetrically in its non-zero modes (it hands (ph, pw, ph, pw) to F.pad, i.e. left = top = ph, right =
 * bottom = pw: meta_conv.py:159, 175-176); the host mirror passes exactly that.  The "same"-padded, stride-1 convolutions
 * every reference configuration uses run faster through hs_patch_conv_fwd (fh = fw = 1); this one covers the rest. */
int hs_meta_conv_fwd(const float* x, int32_t batch, int32_t c_in, int32_t H, int32_t W, const float* w, int64_t ldw,
                     int32_t c_out, int32_t kh, int32_t kw, int32_t stride_h, int32_t stride_w, int32_t pad_top,
                     int32_t pad_bottom, int32_t pad_left, int32_t pad_right, int32_t dil_h, int32_t dil_w,
                     int32_t pad_mode, int32_t groups, const hs_epilogue* ep, float* y, void* stream);

/* Backward of hs_meta_conv_fwd for ZERO padding (MetaConv2d is differentiable in the reference through ATen's conv2d,
 * meta_conv.py:163-186; the other padding modes pad explicitly first, and that pad's adjoint is the caller's): dx (B, c_in, H, W)
 * and / or dw (B, rows, row stride lddw), either may be null.  Gather forms, deterministic. */
int hs_meta_conv_bwd(const float* x, int32_t batch, int32_t c_in, int32_t H, int32_t W, const float* w, int64_t ldw,
                     int32_t c_out, int32_t kh, int32_t kw, int32_t stride_h, int32_t stride_w, int32_t pad_top,
                     int32_t pad_bottom, int32_t pad_left, int32_t pad_right, int32_t dil_h, int32_t dil_w, int32_t groups,
                     const float* dy, float* dx, float* dw, int64_t lddw, void* stream);

/* Op A with the bank generated inside the consumer: signal2weights (grouped 1x1 conv of the signal, hs_s2w_layer minus its
 * bank / ld fields, which are ignored) + k = 1 dynamic patch convolution + BatchNorm affine + activation in ONE launch --
 * HyperPatchNoPadding.forward and the norm / activation modules behind it (hyperseg_v1_0.py:473-498, 728-760; unify:
 * WeightLayer hyperseg_v1_0_unify.py:287-309 + 483-494).  The filter bank is never written to HBM.  Conv groups == 1,
 * patches of at most 64 pixels (the coarse levels, where the bank is the level's whole traffic); otherwise
 * HS_ERR_UNSUPPORTED and the caller uses hs_signal2weights_*_fwd + hs_patch_conv_fwd. */
int hs_patch_conv_gen_fwd(const hs_stage_input* in, int32_t fh, int32_t fw, const float* signal, int32_t c_signal,
                          const hs_s2w_layer* layer, int32_t c_out, const hs_epilogue* ep, float* y, void* stream);

/* Op C: fused per-patch inverted residual of hyperseg_v1_0.py:328-376 (and its unify twin
 * hyperseg_v1_0_unify.py:330-389): reflect halo tile -> pw1 -> BN1 -> ReLU6 -> dw3x3 ->
 * BN2 -> ReLU6 -> pw3 -> BN3 (+ the stage input itself if residual != 0, which requires
 * cin == c_out: use_res_connect, hyperseg_v1_0.py:295, 372-376), one launch, hidden activations
 * never leave the CU.  Bank rows in the reference's flat order (hyperseg_v1_0.py:302-309):
 *   [0, cin*hid)               W1[h][c]
 *   [cin*hid, +9*hid)          K[h][ky][kx]
 *   [.., +hid*c_out)           W3[o][h]
 * bn1/bn2/bn3 are folded scale/shift pairs (activation fields ignored). */
int hs_patch_ir_fwd(const hs_stage_input* in, int32_t fh, int32_t fw,
                    const float* bank, int64_t ld, int32_t hidden, int32_t c_out,
                    const hs_epilogue* bn1, const hs_epilogue* bn2, const hs_epilogue* bn3,
                    int32_t residual, int32_t math /* hs_ir_math, below */, float* y, void* stream);

/* Op D: the inverted residual of hyperseg_v0_1.py:205-237 (HyperSeg-L) as ONE launch.  The reference runs it as three
 * IMAGE-level patch convolutions -- pw1 (MetaPatchConv2d k=1) + BN + ReLU6, depthwise 3x3 with reflect padding of the
 * hidden activation (MetaPatchConv2d k=3, groups=hidden) + BN + ReLU6, pw3 (k=1) + BN -- so the depthwise taps that
 * cross a patch border read hidden activations produced with the NEIGHBOURING patch's pw1 weights (unlike Op C, which
 * applies a patch's own weights to its whole halo tile).  The kernel recomputes that one-pixel ring with the
 * neighbours' weights instead of exchanging it through HBM.  Bank rows as for hs_patch_ir_fwd (the nested
 * MetaSequential's cumulative ranges, hyperseg_v0_1.py:226-237: pw1 | depthwise | pw3).  Only the decoder's fused form
 * (coords + skip + 2x-bilinear previous level) at the instantiated shapes; otherwise HS_ERR_UNSUPPORTED, and the caller
 * runs the block as three hs_patch_conv_fwd launches. */
int hs_patch_ir_v0_fwd(const hs_stage_input* in, int32_t fh, int32_t fw,
                       const float* bank, int64_t ld, int32_t hidden, int32_t c_out,
                       const hs_epilogue* bn1, const hs_epilogue* bn2, const hs_epilogue* bn3,
                       int32_t math /* hs_ir_math */, float* y, void* stream);
/* The same operator with a caller-owned workspace: where patches are 4 x 4 or 8 x 8 pixels (HyperSeg-L levels 2 and 3: every 16 x 16
 * region would span 4-16 patches plus a ring of 12-20 more owners) it runs exactly as the reference states it -- pw1 + BN + ReLU6
 * written once to the workspace (channels-last, hidden rounded up to 16), then depthwise + BN + ReLU6 + pw3 + BN -- two launches of
 * per-patch matrix-core GEMMs whose 16-pixel N dimension is the patch (hs_patch_ir_d2.hip).  hs_patch_ir_v0_workspace: the bytes that
 * form needs for this shape, 0 if the shape is not covered (then, or with workspace = NULL, this call equals hs_patch_ir_v0_fwd).
 * The workspace is scratch: nothing is kept in it between calls, and the library holds no state of its own. */
int64_t hs_patch_ir_v0_workspace(const hs_stage_input* in, int32_t fh, int32_t fw, int32_t hidden, int32_t c_out);
int hs_patch_ir_v0_ws_fwd(const hs_stage_input* in, int32_t fh, int32_t fw,
                          const float* bank, int64_t ld, int32_t hidden, int32_t c_out,
                          const hs_epilogue* bn1, const hs_epilogue* bn2, const hs_epilogue* bn3,
                          int32_t math /* hs_ir_math */, float* workspace, int64_t workspace_bytes, float* y, void* stream);

/* Arithmetic of the fused inverted-residual levels -- the `math` ARGUMENT of hs_patch_ir_fwd / hs_patch_ir_v0_fwd (chosen by
 * the caller per launch: the library keeps no mode, or any other mutable state, of its own):
 *   HS_IR_MATH_F32    v_mfma_f32_16x16x4_f32: bit-exact f32 fma chains (csrc/hs_patch_ir_fused.hip, hs_patch_ir_px.hip).
 *   HS_IR_MATH_SPLIT  f16 matrix cores on split operands wherever that form exists (Op C on patches >= 8 rows x 16 columns,
 *       <= 16 skip and <= 16 previous-level channels: csrc/hs_patch_irc.hip): every f32 operand is scaled by a power of two
 *       and split into two f16 pieces, a product is ah*bh + al*bh + ah*bl accumulated in f32.  f32-class: the measured
 *       error of a dot product is BELOW an f32 fmaf chain's (tools/ubench/f16_probe.hip: 1.3e-7 vs 2.2e-7 of sum|a||b|).
 *       The scales are taken from the data -- the exact maximum of each weight MATRIX of the patch (pw1, pw3; even channel
 *       counts, round 4: the f16 pieces hold 2^15 of range below that maximum, so a row keeps f32-class accuracy as long as
 *       its own maximum is within 2^15 of the matrix's; odd channel counts keep one scale per row) and of every halo
 *       position's input column -- so any overall magnitude is carried; what is not is a dynamic range beyond ~2^18 INSIDE
 *       one reduction (an input 2^20 above its position's other channels meeting a weight 2^-20 of its matrix's maximum).
 *   HS_IR_MATH_AUTO   SPLIT where it is the faster form, F32 elsewhere: SPLIT wherever it applies, except narrow blocks (<= 4 skip
 *       channels) in launches of more than 512 16 x 16 regions, where the exact-f32 kernel measured faster (CamVid HyperSeg-L levels 4-5).
 * The reference runs these layers as fp32 torch convolutions (which cuDNN may run in TF32 there); all modes are held to the
 * same parity tolerance (tests/test_hip_parity.py).  The nn.Module mirror defaults to F32; serving / bench.py opt into AUTO
 * (hyperseg_amd.utils.inference.prepare_for_inference(ir_math='auto')). */
typedef enum { HS_IR_MATH_AUTO = 0, HS_IR_MATH_F32 = 1, HS_IR_MATH_SPLIT = 2 } hs_ir_math;

/* Which kernel hs_patch_ir_fwd would run for a call of this shape (host only: nothing is launched, pointers in `in` may be
 * null): the generic kernel (vector ALU, any channel counts), the exact-f32 matrix-core kernel (the decoder's own shapes) or
 * the f16-split matrix-core kernel (any channel split up to 16 + 16 -> 32 on patches >= 8 x 16).  Negative = error code.
 * For callers that want to know what a configuration gets before they run it, and for the tests that pin the coverage. */
typedef enum { HS_IR_ROUTE_GENERIC = 0, HS_IR_ROUTE_F32_MFMA = 1, HS_IR_ROUTE_SPLIT_MFMA = 2 } hs_ir_route;
int hs_patch_ir_route(const hs_stage_input* in, int32_t fh, int32_t fw, int32_t hidden, int32_t c_out,
                      int32_t residual, int32_t math);

/* hs_patch_ir_route plus the FORM inside the route (host only, as above; form: 4 words, may be null).  bank_aligned16 / y_aligned16:
 * the facts the launcher reads off the bank and output pointers (the split kernel's bank DMA and 16-byte stores; a bank view at a
 * 4-byte offset takes the direct kernels).  ld: the bank's row stride, 0 = the packed row rounded up to 4.
 *   HS_IR_ROUTE_GENERIC     form[0] = HS_IR_GENERIC(cin, c_skip, c_out) of the instantiation -- the five exact ones (24, 6, 16),
 *                           (34, 16, 19), (14, 4, 8), (26, 16, 19), (22, 4, 12), or a width class (16, 0, 16), (32, 0, 32), (64, 0, 32),
 *                           (128, 0, 64); form[1] = 1 for an exact one; form[2], form[3] = tiles_y, tiles_x per patch
 *   HS_IR_ROUTE_SPLIT_MFMA  form[0] = RH (8 | 16 region rows), form[1] = NW (waves per region), form[2] = regions per patch,
 *                           form[3] = SPL << 8 | PPL << 4 | MT3 (quads of skip / previous-level channels, 16-channel output tiles)
 *   HS_IR_ROUTE_F32_MFMA    form[0] = REG (region edge 8 | 16), form[1] = PWR (patch edge inside the region),
 *                           form[2] = HS_IR_GENERIC(cin, c_skip, c_out) of the instantiation, form[3] = regions in the launch
 * A negative answer is the launcher's error code (HS_ERR_UNSUPPORTED beyond the widest class). */
#define HS_IR_GENERIC(cin, c_skip, c_out) (((cin) << 16) | ((c_skip) << 8) | (c_out))
int hs_patch_ir_form(const hs_stage_input* in, int32_t fh, int32_t fw, int64_t ld, int32_t hidden, int32_t c_out, int32_t residual,
                     int32_t math, int32_t bank_aligned16, int32_t y_aligned16, int32_t* form);

/* Which form hs_patch_ir_v0_ws_fwd takes (host only; form: 4 words, may be null), or HS_ERR_UNSUPPORTED where it answers that:
 *   HS_IR_V0_ROUTE_D2     two launches through the workspace (4 x 4 / 8 x 8 patches; with_workspace: the caller passes one of
 *                         hs_patch_ir_v0_workspace() bytes, 16-byte aligned): form[0] = patch edge, form[1] = RT (3 | 6), form[2] = AL
 *                         (4 | 2), form[3] = 16-channel hidden steps of the second launch
 *   HS_IR_V0_ROUTE_PX     one launch, one lane per pixel (hs_patch_ir_px.hip): form[0] = 16, form[2] = HS_IR_GENERIC(...)
 *   HS_IR_V0_ROUTE_FUSED  one launch on the f32 matrix cores (hs_patch_ir_fused.hip): form as for HS_IR_ROUTE_F32_MFMA */
#define HS_IR_V0_ROUTE_D2 0
#define HS_IR_V0_ROUTE_PX 1
#define HS_IR_V0_ROUTE_FUSED 2
int hs_patch_ir_v0_route(const hs_stage_input* in, int32_t fh, int32_t fw, int64_t ld, int32_t hidden, int32_t c_out,
                         int32_t with_workspace, int32_t bank_aligned16, int32_t* form);

/* Which of its five forms hs_patch_conv_fwd takes (host only; pointers in `in` may be null; form: 4 words, may be null).  The forms are
 * tried in this order; every predicate is the one the launcher dispatches on.  aligned16: the bank is 16-byte aligned; aligned8: x and y
 * are 8-byte aligned (plain inputs: the pair forms).  with_scale / with_shift / act: the epilogue's fields.
 *   HS_CONV_ROUTE_PLAIN_DW3  plain input, depthwise 3 x 3 with zero padding, no epilogue: image-level kernel; form[0] = 1 for the
 *                            two-pixels-per-lane form (even patch and image widths, aligned8)
 *   HS_CONV_ROUTE_PLAIN_K1M  plain input, k = 1, groups = 1, patches >= 64 pixels, c_out <= 64, c_in <= 64 (not both > 48): f32 matrix
 *                            cores; form = {MT, KQ (16-channel tiles of c_out / c_in), pixels per lane (1 | 2), affine}
 *   HS_CONV_ROUTE_K1M        k = 1, groups = 1, >= 1024 patches of 2 x 2 pixels, even 4 <= cin <= 144, c_out <= 96: the weight stream
 *                            (hs_patch_conv_k1m.hip); form = {RT (3 | 6), AL (4 | 2), PREV (0 | 1)}
 *   HS_CONV_ROUTE_K1         k = 1: one workgroup per patch; form = {PWL (log2 of the patch edge for 1, 2, 4, 8; -1 otherwise), split}
 *   HS_CONV_ROUTE_TILED      the generic kernel; form = {TH, TW, tiles_y, tiles_x} */
#define HS_CONV_ROUTE_PLAIN_DW3 0
#define HS_CONV_ROUTE_PLAIN_K1M 1
#define HS_CONV_ROUTE_K1M 2
#define HS_CONV_ROUTE_K1 3
#define HS_CONV_ROUTE_TILED 4
int hs_patch_conv_route(const hs_stage_input* in, int32_t fh, int32_t fw, int64_t ld, int32_t c_out, int32_t k, int32_t pad,
                        int32_t pad_mode, int32_t groups, int32_t with_scale, int32_t with_shift, int32_t act, int32_t aligned16,
                        int32_t aligned8, int32_t* form);

/* Introspection for the tests (host only, no GPU): the matrix-core tile map of the fused inverted-residual kernel for a
 * region edge `reg` (8|16), mode (0 = Op C, 1 = Op D) and patch edge inside the region `pwr`.  out[(t*16+n)*3 + {0,1,2}]
 * = halo coordinates (u, v) and liveness of column n of pw1 tile t (csrc/hs_ir_tiles.h). */
int hs_ir_tile_map(int32_t reg, int32_t mode, int32_t pwr, int32_t* n_tiles, int32_t* n_pixel_tiles,
                   int32_t* out, int32_t capacity);

/* Final logits resize: F.interpolate(p, size, mode='bilinear', align_corners=False)
 * (hyperseg_v1_0.py:250-251).  x (B,C,Hi,Wi) -> y (B,C,Ho,Wo). */
int hs_upsample_bilinear_fwd(const float* x, int32_t batch, int32_t channels, int32_t Hi, int32_t Wi,
                             int32_t Ho, int32_t Wo, float* y, void* stream);
/* ... on bf16 storage (x and y bf16, same taps, f32 arithmetic, one rounding on store): the training path's final logits under
 * torch.autocast(bfloat16) (autograd.UpsampleBilinear). */
int hs_upsample_bilinear_bf16_fwd(const void* x, int32_t batch, int32_t channels, int32_t Hi, int32_t Wi, int32_t Ho, int32_t Wo,
                                  void* y, void* stream);
/* ... on fp16 storage (IEEE binary16 x and y; the same taps and arithmetic, one round-to-nearest-even on store): the final logits under
 * torch.autocast(float16). */
int hs_upsample_bilinear_f16_fwd(const void* x, int32_t batch, int32_t channels, int32_t Hi, int32_t Wi, int32_t Ho, int32_t Wo,
                                 void* y, void* stream);

/* The same resize with the class argmax taken in registers: mask (B, Ho, Wo) uint8 = argmax_c of the upsampled logits,
 * bit-identical to argmax over hs_upsample_bilinear_fwd's output (shared arithmetic), ties -> lowest class; channels
 * <= 256.  Replaces F.interpolate + pred.argmax(1) (hyperseg_v1_0.py:250-251 + test.py:171, test_fps.py:194) for callers
 * that only need masks: 0.5 MB written instead of 39.8 MB at HyperSeg-M 1024x512. */
int hs_upsample_argmax_fwd(const float* x, int32_t batch, int32_t channels, int32_t Hi, int32_t Wi,
                           int32_t Ho, int32_t Wo, uint8_t* mask, void* stream);

/* On-device evaluation (csrc/hs_eval.hip): the (target, prediction) confusion matrix of the reference's evaluation loop
 * (hyperseg/utils/seg_utils.py:5-36: mat[t][p] += 1 for every pixel whose target t is in [0, num_classes); every other target
 * value -- 255, negatives -- is ignored).  Both entries ACCUMULATE into `confusion` (int64, (n, n), or (batch, n, n) with
 * per_image != 0: image b's counts in slab b -- test.py:174-175 without a host read per image); they never zero it.  Integer
 * sums: the result does not depend on arrival order.  Label storage: HS_EVAL_U8 or HS_EVAL_I64 (what the reference's loaders
 * produce).  num_classes <= hs_eval_max_classes() (the per-workgroup LDS histogram; >= 64), else HS_ERR_UNSUPPORTED and the
 * caller counts some other way.
 *   hs_upsample_confusion_fwd: hs_upsample_argmax_fwd (same taps, same arg-max rule, the identity resize included) with every
 *     output pixel counted against target (batch, Ho, Wo) in the same launch.  mask (optional): the uint8 masks, bit-identical
 *     to hs_upsample_argmax_fwd's.  channels <= num_classes <= 256, else HS_ERR_BAD_ARG.
 *   hs_confusion_fwd: the same counting from finished predictions, pred and target (batch, elements); a prediction outside
 *     [0, num_classes) is not counted. */
typedef enum { HS_EVAL_U8 = 0, HS_EVAL_I64 = 1 } hs_eval_dtype;
int hs_eval_max_classes(void);
int hs_upsample_confusion_fwd(const float* x, int32_t batch, int32_t channels, int32_t Hi, int32_t Wi, int32_t Ho, int32_t Wo,
                              const void* target, int32_t target_dtype, int32_t num_classes, int32_t per_image,
                              int64_t* confusion, uint8_t* mask, void* stream);
int hs_confusion_fwd(const void* pred, int32_t pred_dtype, const void* target, int32_t target_dtype, int32_t batch,
                     int64_t elements, int32_t num_classes, int32_t per_image, int64_t* confusion, void* stream);
/* Scoring at the label's resolution (test.py:167-168: the model's logits, at the frame's size, are resized once more to the label's
 * before the arg-max): hs_upsample_confusion_fwd over TWO resizes composed in registers, x (Hi, Wi) -> mid (Hm, Wm) -> (Ho, Wo).
 * The class score of a label pixel is exactly what hs_upsample_bilinear_fwd(hs_upsample_bilinear_fwd(x -> Hm, Wm) -> Ho, Wo) stores
 * (each stage in the form that entry takes for its shape; the second stage clamps in mid index space), so mask and counts are
 * bit-identical to arg-max + hs_confusion_fwd over those logits -- neither the mid nor the label-size logits are ever in memory.
 * Two forms: both stages exact 2x (one 3 x 4 neighbourhood of x per 4 x 8 label block), and any other pair of stages (down-sampling
 * and identity second stages included).  target and confusion may BOTH be NULL: masks only (then mask is required and num_classes,
 * target_dtype and per_image are not read; channels <= 256).  Otherwise hs_upsample_confusion_fwd's contract. */
int hs_upsample2_confusion_fwd(const float* x, int32_t batch, int32_t channels, int32_t Hi, int32_t Wi, int32_t Hm, int32_t Wm,
                               int32_t Ho, int32_t Wo, const void* target, int32_t target_dtype, int32_t num_classes, int32_t per_image,
                               int64_t* confusion, uint8_t* mask, void* stream);

/* Flip and pyramid inference merged in one launch (csrc/hs_tta_merge.hip; the reference's list-input mode, hyperseg_v1_0.py:71-91).
 * passes: a HOST array of n_passes <= HS_TTA_MAX_PASSES records, copied into the launch's arguments (no device-side table, nothing
 * allocated), sorted by entry, entries 0, 1, ... without a gap, one (Hm, Wm) per entry.  Each pass: x f32 (batch, channels, Hi, Wi), what
 * the decoder hands to its final resize; (Hm, Wm) its frame's size, where the reference's logits live; flipped: it ran on the mirrored
 * frame; entry: the pyramid entry it belongs to.  The output size (Ho, Wo) is entry 0's (Hm, Wm).  Per output pixel and class:
 *   a pass at (ym, xm) of its entry is what hs_upsample_bilinear_fwd(x -> Hm, Wm) stores there (x itself where (Hi, Wi) == (Hm, Wm)), a
 *     flipped pass read at column Wm - 1 - xm;
 *   an entry is the max over its passes at its own resolution; an entry of another size than (Ho, Wo) is then resized to it as
 *     hs_upsample_bilinear_fwd would resize that max map (the max taken at each mid tap before the second interpolation);
 *   entries are folded in order: out = (p + out) * 0.5, or max(p, out) with gather_max != 0.
 * Bit-identical to that composition of launches for finite inputs.  Sinks, selected by non-null pointers (at least one): logits f32
 * (batch, channels, Ho, Wo); mask uint8 (batch, Ho, Wo), the first maximum; confusion together with target (batch, target_h, target_w):
 * hs_confusion_fwd's counts of (target, arg-max), accumulated, per_image slabs, HS_EVAL_U8 or HS_EVAL_I64 targets, channels <=
 * num_classes <= 256 else HS_ERR_BAD_ARG.  HS_ERR_UNSUPPORTED -- nothing launched -- for n_passes > HS_TTA_MAX_PASSES, channels > 256,
 * num_classes > hs_eval_max_classes() when counting, or a target of another size than (Ho, Wo).  Nothing is read back: capturable. */
#define HS_TTA_MAX_PASSES 8
typedef struct {
    const float* x;
    int32_t Hi, Wi, Hm, Wm;
    int32_t flipped, entry;
} hs_tta_pass;
int hs_tta_merge_fwd(const hs_tta_pass* passes, int32_t n_passes, int32_t batch, int32_t channels, int32_t gather_max,
                     const void* target, int32_t target_dtype, int32_t target_h, int32_t target_w, int32_t num_classes,
                     int32_t per_image, int64_t* confusion, uint8_t* mask, float* logits, void* stream);

/* The validation step's middle (csrc/hs_validate.hip; hyperseg/train.py:118-126: the loss of a batch and its running score): the
 * per-pixel cross entropy, the class arg-max and the (target, prediction) count from ONE pass over each pixel's class scores.
 *   loss (batch, pixels) f32: hs_cross_entropy_typed_fwd's values bit for bit (0 where the target is ignore_index or outside
 *     [0, channels)) -- what hs_bootstrap_mean_of_batch_fwd reduces to BootstrappedCrossEntropyLoss' value;
 *   mask (optional) uint8: argmax(1) of the scores widened to f32, the first maximum;
 *   confusion int64 (n, n) / (batch, n, n) with per_image: ACCUMULATED into, never zeroed, hs_confusion_fwd's rule -- every target in
 *     [0, num_classes) is counted, an in-range ignore_index included (the reference's runningScore does not know it), everything else
 *     ignored.  NULL: nothing is counted and num_classes / per_image are not read.
 * channels <= num_classes <= 256 else HS_ERR_BAD_ARG; num_classes > hs_eval_max_classes(): HS_ERR_UNSUPPORTED, nothing launched.
 *   hs_cross_entropy_score_fwd: from logits in memory (dtype: f32 / bf16 / f16 storage, (batch, classes, pixels)), int64 targets.
 *   hs_upsample_ce_confusion_fwd: from x f32 (batch, channels, Hi, Wi) resized to (Ho, Wo) in registers, targets HS_EVAL_U8 or
 *     HS_EVAL_I64 at (batch, Ho, Wo): loss, mask and counts bit-identical to hs_upsample_bilinear_fwd + hs_cross_entropy_typed_fwd and
 *     hs_upsample_argmax_fwd + hs_confusion_fwd; the resized logits never exist in memory.  Both forms of the final upsample (exact 2x;
 *     any other ratio, the identity and down-sampling included).
 * Nothing is read back: capturable. */
int hs_cross_entropy_score_fwd(int32_t dtype, const void* logits, const int64_t* target, int32_t batch, int32_t classes, int64_t pixels,
                               int64_t ignore_index, float* loss, int32_t num_classes, int32_t per_image, int64_t* confusion,
                               uint8_t* mask, void* stream);
int hs_upsample_ce_confusion_fwd(const float* x, int32_t batch, int32_t channels, int32_t Hi, int32_t Wi, int32_t Ho, int32_t Wo,
                                 const void* target, int32_t target_dtype, int64_t ignore_index, float* loss, int32_t num_classes,
                                 int32_t per_image, int64_t* confusion, uint8_t* mask, void* stream);
/* ... with class weights (nn.CrossEntropyLoss(weight=...)): `weight` f32 (classes,) / (channels,) on the device, non-NULL else
 * HS_ERR_BAD_ARG.  loss = weight[t] * (the unweighted entry's loss), one more f32 multiply, hs_cross_entropy_weighted_fwd's bits; masks
 * and counts are the unweighted entries'.  The table is read by the launch only (capturable: the graph holds its address). */
int hs_cross_entropy_score_weighted_fwd(int32_t dtype, const void* logits, const int64_t* target, const float* weight, int32_t batch,
                                        int32_t classes, int64_t pixels, int64_t ignore_index, float* loss, int32_t num_classes,
                                        int32_t per_image, int64_t* confusion, uint8_t* mask, void* stream);
int hs_upsample_ce_confusion_weighted_fwd(const float* x, int32_t batch, int32_t channels, int32_t Hi, int32_t Wi, int32_t Ho, int32_t Wo,
                                          const void* target, int32_t target_dtype, const float* weight, int64_t ignore_index, float* loss,
                                          int32_t num_classes, int32_t per_image, int64_t* confusion, uint8_t* mask, void* stream);
/* The validation step at the LABEL's resolution (train.py:119-120: the logits, at the frame's size, are resized to a label of another size
 * before the criterion and the arg-max): hs_upsample_ce_confusion_fwd over TWO resizes composed in registers, x (Hi, Wi) -> mid (Hm, Wm) ->
 * (Ho, Wo), targets at (batch, Ho, Wo).  A label pixel's class scores are exactly what hs_upsample_bilinear_fwd(hs_upsample_bilinear_fwd(x
 * -> Hm, Wm) -> Ho, Wo) stores (each stage in the form that entry takes for its shape, the second clamping in mid index space), so
 *   loss (batch, Ho, Wo) f32 is hs_cross_entropy_typed_fwd's on those logits bit for bit (times weight[t] in the twin),
 *   mask (optional) and the counts are hs_upsample2_confusion_fwd's,
 * and neither the mid nor the label-size logits are ever in memory.  Two forms, chosen as hs_upsample2_confusion_fwd chooses: both stages
 * exact 2x, and any other pair of stages (down-sampling and identity stages included).  confusion, num_classes, per_image, ignore_index,
 * the limits (channels <= 256, num_classes <= hs_eval_max_classes(), batch <= 65535, Ho * Wo and Hm * Wm < 2^31 - 4096) and the status
 * codes: hs_upsample_ce_confusion_fwd's.  Nothing is read back: capturable. */
int hs_upsample2_ce_confusion_fwd(const float* x, int32_t batch, int32_t channels, int32_t Hi, int32_t Wi, int32_t Hm, int32_t Wm, int32_t Ho,
                                  int32_t Wo, const void* target, int32_t target_dtype, int64_t ignore_index, float* loss, int32_t num_classes,
                                  int32_t per_image, int64_t* confusion, uint8_t* mask, void* stream);
int hs_upsample2_ce_confusion_weighted_fwd(const float* x, int32_t batch, int32_t channels, int32_t Hi, int32_t Wi, int32_t Hm, int32_t Wm,
                                           int32_t Ho, int32_t Wo, const void* target, int32_t target_dtype, const float* weight,
                                           int64_t ignore_index, float* loss, int32_t num_classes, int32_t per_image, int64_t* confusion,
                                           uint8_t* mask, void* stream);

/* Backward of hs_patch_conv_fwd (plain input x, no fused prologue / epilogue), fp32 -- SURVEY.md Appendix E.
 * The reference has no backward of its own (autograd over F.pad/unfold/grouped conv2d/fold: meta_patch.py:35-57);
 * these are the adjoints the training path (BASELINE config 5) needs:
 *   hs_patch_conv_bwd_weight: dbank[p, n] = sum over the patch's pixels of dy * padded x  ("per-patch weight-grad kernel")
 *   hs_patch_conv_bwd_input : dx = transposed patch-wise correlation of dy with each output pixel's own patch filters,
 *                             halo gradients folded back through the padding (adjoint of F.pad). */
int hs_patch_conv_bwd_input(const float* dy, const float* bank, int64_t ld, int32_t batch, int32_t c_in,
                            int32_t H, int32_t W, int32_t fh, int32_t fw, int32_t c_out, int32_t k, int32_t pad,
                            int32_t pad_mode, int32_t groups, float* dx, void* stream);
int hs_patch_conv_bwd_weight(const float* x, const float* dy, int32_t batch, int32_t c_in, int32_t H, int32_t W,
                             int32_t fh, int32_t fw, int32_t c_out, int32_t k, int32_t pad, int32_t pad_mode,
                             int32_t groups, float* dbank, int64_t ld, void* stream);

/* Which kernel the two launchers above take (which = 0: input gradient, 1: weight gradient), and hs_patch_conv_plain_bwd_in / _bwd_w
 * below for the first three routes (host only, nothing launched; every predicate is the one the launcher dispatches on).  dtype: an
 * hs_dtype; align_a / align_b: the addresses of the two tensors the alignment conditions read, modulo 16 (dy and dx for the input
 * gradient, x and dy for the weight gradient: 0 for an allocator's tensor).  Writes *route and form[4]:
 *   HS_BWD_ROUTE_DW3      depthwise 3 x 3 with zero padding: form[0] = 1 for the two-pixels-per-lane form (even patch and image widths,
 *                         8-byte aligned tensors)
 *   HS_BWD_ROUTE_TINY     k = 1, groups = 1, patches of fewer than 16 pixels (input gradient: c_out <= 1024; weight gradient:
 *                         (c_out + c_in) * 17 * 4 bytes of LDS <= 64 KB)
 *   HS_BWD_ROUTE_K1M      k = 1, groups = 1, patches of >= 16 pixels, f32 matrix cores.  Input gradient: form = {CT, KQ (16-channel tiles
 *                         of c_in / c_out), pixels per lane (1 | 2)}; weight gradient: form = {MT, NT (tiles of c_out / c_in), loads
 *                         (1 = four elements, 2 = pairs, 0 = scalar)}
 *   HS_BWD_ROUTE_GENERIC  everything else.  Weight gradient: form = {ob = output channels per block, blocks, 1 where the LDS request
 *                         exceeds 64 KB} of the fp32 kernel; HS_ERR_LDS where not one block fits. */
#define HS_BWD_ROUTE_DW3 0
#define HS_BWD_ROUTE_TINY 1
#define HS_BWD_ROUTE_K1M 2
#define HS_BWD_ROUTE_GENERIC 3
int hs_patch_conv_bwd_route(int32_t which, int32_t dtype, int32_t align_a, int32_t align_b, int64_t ld, int32_t batch, int32_t c_in,
                            int32_t H, int32_t W, int32_t fh, int32_t fw, int32_t c_out, int32_t k, int32_t pad, int32_t pad_mode,
                            int32_t groups, int32_t* route, int32_t* form);

/* Training-path twins with a storage type: HS_DTYPE_F32, or HS_DTYPE_BF16 = bf16 storage of the ACTIVATIONS and their gradients
 * (x, y, dy, dx read and written as bf16: half the HBM bytes) with fp32 accumulation (BASELINE config 5; the reference has no
 * reduced-precision path: SURVEY 8d).  `bank` and `dbank` are fp32 (const float* / float*) for either dtype: the bank comes out of
 * signal2weights and its gradient goes into that layer's adjoint, both fp32.  Plain (B, C, H, W) tensors, no fused prologue /
 * epilogue -- the training route composes the stage input, BatchNorm and activations with its own differentiable ops
 * (hyperseg_amd/autograd.py).  Same math as hs_patch_conv_fwd / hs_patch_conv_bwd_input / hs_patch_conv_bwd_weight above.
 * HS_DTYPE_F16 = IEEE binary16 storage under the same contract (torch.autocast's default dtype; rounding to nearest-even on store,
 * overflow to +-inf as torch's .half()): every entry point that takes an hs_dtype accepts all three. */
typedef enum { HS_DTYPE_F32 = 0, HS_DTYPE_BF16 = 1, HS_DTYPE_F16 = 2 } hs_dtype;
int hs_patch_conv_plain_fwd(int32_t dtype, const void* x, const void* bank, int64_t ld, int32_t batch, int32_t c_in,
                            int32_t H, int32_t W, int32_t fh, int32_t fw, int32_t c_out, int32_t k, int32_t pad,
                            int32_t pad_mode, int32_t groups, void* y, void* stream);
int hs_patch_conv_plain_bwd_in(int32_t dtype, const void* dy, const void* bank, int64_t ld, int32_t batch, int32_t c_in,
                               int32_t H, int32_t W, int32_t fh, int32_t fw, int32_t c_out, int32_t k, int32_t pad,
                               int32_t pad_mode, int32_t groups, void* dx, void* stream);
int hs_patch_conv_plain_bwd_w(int32_t dtype, const void* x, const void* dy, int32_t batch, int32_t c_in, int32_t H, int32_t W,
                              int32_t fh, int32_t fw, int32_t c_out, int32_t k, int32_t pad, int32_t pad_mode,
                              int32_t groups, void* dbank, int64_t ld, void* stream);

/* Encoder-side helper ("next" row of SURVEY.md section 8f; opt-in via hyperseg_amd.utils.inference): depthwise k x k
 * convolution (k in {3,5}, stride in {1,2}) with arbitrary top/left zero padding (TF-"SAME"), + per-channel affine
 * (folded BatchNorm) + activation (hs_act) in one launch.  x (B,C,H,W), w (C,1,k,k) -> y (B,C,Ho,Wo).
 * Replaces F.pad + F.conv2d(groups=C) + BatchNorm2d + swish of the reference's MBConvBlock
 * (hyperseg/models/backbones/efficientnet.py:59-66, 101-103). */
int hs_depthwise_conv_fwd(const float* x, int32_t batch, int32_t channels, int32_t H, int32_t W,
                          const float* w, int32_t k, int32_t stride, int32_t pad_t, int32_t pad_l,
                          int32_t Ho, int32_t Wo, const float* scale, const float* shift, int32_t act,
                          float* y, float* pool_partial, const float* in_scale, const float* in_shift, void* stream);
/* in_scale / in_shift (optional, both or neither, (C)): the taps become swish(in_scale[c]*x + in_shift[c]) -- the folded
 * BatchNorm + swish of the 1x1 expand convolution that produced x (efficientnet.py:101-103), applied on load so that the
 * raw GEMM output is consumed directly; zero padding stays zero.
 * pool_partial (optional): (B*C, hs_depthwise_pool_blocks(Ho, Wo)) per-workgroup sums of the outputs, the squeeze-excite
 * pooling for free.  hs_se_gate_fwd turns them into the SE gate (pool -> 1x1 reduce + swish -> 1x1 expand -> sigmoid;
 * efficientnet.py:106-111): squeezed (B, c_squeezed) = swish(reduce(pool)), then gate (B, channels) -- one launch when the
 * reduce weights are small (channels <= 768, c_squeezed <= 32: every workgroup re-derives the squeezed vector), two otherwise; if
 * w_proj (c_out, channels) is given it also folds the gate -- and, with out_scale (c_out), the project convolution's folded
 * BatchNorm scale -- into the project weights: w_scaled[b, o, c] = w_proj[o, c] * gate[b, c] * out_scale[o].
 * w_reduce is (c_squeezed, channels); w_expand is passed TRANSPOSED, (c_squeezed, channels): both are read coalesced. */
int hs_depthwise_pool_blocks(int32_t Ho, int32_t Wo);

/* The squeeze-excite gate finished by the LAST workgroups of the pooling launch itself (round 5, csrc/hs_se_tail.h) instead of by
 * hs_se_gate_fwd: hs_depthwise_conv_se_fwd / hs_mbconv_expand_dw_se_fwd are the launches above without pool_partial and with this
 * descriptor; gate (B, channels) and, optionally, squeezed (B, c_squeezed) come back.  Same sums in the same order per channel; the
 * two matrix-vector products are split over <= 32 workgroups and re-assembled in slice order (deterministic).
 * workspace: hs_se_tail_workspace(batch, channels, c_squeezed, nblk, wgs_per_batch) bytes (nblk = hs_depthwise_pool_blocks /
 * hs_mbconv_tiles; wgs_per_batch = channels * nblk for the depthwise launch, hs_mbconv_se_workgroups for the fused one), 8-byte
 * aligned, ZERO before its first use and owned by one launch at a time (two streams need two); the launches keep it consistent.
 * Its word [batch] is an error flag: nonzero after a launch whose bounded waits gave up (the gate is then NaN).
 * hs_se_tail_workspace returns 0 -- and the launches HS_ERR_UNSUPPORTED -- for shapes the tail does not cover
 * (c_squeezed > 96, > 512 partials per channel, more than 32 tails of <= 64 channels, fewer workgroups than tails). */
typedef struct hs_se_tail {
    const float* w_reduce;    /* (c_squeezed, channels)            efficientnet.py:107 _se_reduce */
    const float* b_reduce;    /* (c_squeezed) */
    const float* w_expand_t;  /* (c_squeezed, channels): _se_expand's weight TRANSPOSED */
    const float* b_expand;    /* (channels) */
    int32_t c_squeezed;
    float* gate;              /* out (B, channels) = sigmoid(expand(swish(reduce(mean)))) */
    float* squeezed;          /* out (B, c_squeezed), optional */
    void* workspace;
} hs_se_tail;
int64_t hs_se_tail_workspace(int32_t batch, int32_t channels, int32_t c_squeezed, int32_t nblk, int64_t wgs_per_batch);
int hs_se_tail_tails(int32_t channels, int32_t c_squeezed, int32_t nblk, int64_t wgs_per_batch);   /* workgroups that finish the gate; 0: not covered */
int hs_depthwise_conv_se_fwd(const float* x, int32_t batch, int32_t channels, int32_t H, int32_t W,
                             const float* w, int32_t k, int32_t stride, int32_t pad_t, int32_t pad_l,
                             int32_t Ho, int32_t Wo, const float* scale, const float* shift, int32_t act,
                             float* y, const float* in_scale, const float* in_shift, const hs_se_tail* se, void* stream);
int hs_se_gate_fwd(const float* partial, int32_t batch, int32_t channels, int32_t nblk, float inv_hw,
                   const float* w_reduce, const float* b_reduce, int32_t c_squeezed, const float* w_expand,
                   const float* b_expand, float* squeezed, float* gate, const float* w_proj, int32_t c_out,
                   const float* out_scale, float* w_scaled, void* stream);


/* Encoder-side helper: the stem -- dense 3x3 stride-2 convolution of the 3-channel image (zero padding by top/left
 * offsets, TF-"SAME") + folded BatchNorm + swish in one launch.  x (B,3,H,W), w (c_out,3,3,3) -> y (B,c_out,Ho,Wo).
 * Replaces F.pad + conv + BatchNorm2d + swish of efficientnet.py:321-322. */
int hs_stem_conv_fwd(const float* x, int32_t batch, int32_t c_in, int32_t H, int32_t W, const float* w, int32_t c_out,
                     int32_t pad_t, int32_t pad_l, int32_t Ho, int32_t Wo, const float* scale, const float* shift,
                     float* y, void* stream);

/* Encoder-side helper: the first half of an MBConv block in ONE launch,
 *   y = swish(BN1(depthwise_kxk_stride(zero-pad(swish(BN0(w_expand . x))))))   (+ per-tile sums of y for the SE pool)
 * x (B,c_in,H,W), w_expand (c_mid,c_in), w_dw (c_mid,1,k,k), scale/shift = folded BatchNorms, y (B,c_mid,Ho,Wo),
 * pool_partial (optional) (B*c_mid, hs_mbconv_tiles(k, stride, Ho, Wo)).  k in {3,5}, stride in {1,2}, c_in <= 80.
 * The expanded activation lives in LDS only.  Replaces efficientnet.py:101-106 of the reference's MBConvBlock. */
int hs_mbconv_tiles(int32_t k, int32_t stride, int32_t Ho, int32_t Wo);
/* The stem and the first block's depthwise half in one launch (that block has no expand conv):
 *   y = swish(BN1(depthwise_3x3(zero-pad(swish(BN0(conv3x3/s2(zero-pad(x))))))))   (+ per-tile sums of y for the SE pool)
 * x (B,3,H,W); w_stem28 (c_mid, 28): the stem weight (c_mid,3,3,3) flattened to (c_mid, 27) plus one zero column; (Hs, Ws) = the
 * stem's output size = y's (B,c_mid,Hs,Ws); pool_partial (optional) (B*c_mid, hs_mbconv_tiles(3, 1, Hs, Ws)).  The stem's output
 * map never reaches HBM.  HS_ERR_UNSUPPORTED outside k = 3, c_mid % 16 == 0, Ws % 16 == 0 (the caller then runs
 * hs_stem_conv_fwd + hs_depthwise_conv_fwd).  Replaces efficientnet.py:321-322 and 59-66 / 101-103 of MBConvBlock 0. */
int hs_stem_dw_fwd(const float* x, int32_t batch, int32_t H, int32_t W, const float* w_stem28, int32_t c_mid,
                   const float* scale0, const float* shift0, int32_t stem_pad_t, int32_t stem_pad_l, int32_t Hs, int32_t Ws,
                   const float* w_dw, int32_t k, int32_t pad_t, int32_t pad_l, const float* scale1, const float* shift1,
                   float* y, float* pool_partial, void* stream);
/* uint8 frames (what cameras and decoders deliver) normalised on the device.  layout: HS_LAYOUT_HWC = (B, H, W, 3), HS_LAYOUT_CHW =
 * (B, 3, H, W).  table: (3, 256) floats, table[c][v] = (float(v) / 255 - mean[c]) / std[c] computed on the host in float32 -- the
 * arithmetic of the reference's ToTensor + Normalize (hyperseg/datasets/seg_transforms.py, defaults test.py:62-63); the kernels look
 * values up, so their output is bit-identical to the host transform.
 *   hs_image_ingest_fwd: x -> y (B, 3, H, W) float32 in one launch; any H, W >= 1, any alignment of x (y: a float's 4 bytes), batch <= 65535;
 *     HS_ERR_UNSUPPORTED for channels != 3.
 *   hs_stem_dw_u8_fwd: hs_stem_dw_fwd reading x itself (the float image is never written): the other arguments, the outputs (bit for
 *     bit, against hs_stem_dw_fwd on hs_image_ingest_fwd's result) and the shapes answered with HS_ERR_UNSUPPORTED are hs_stem_dw_fwd's;
 *     zero padding is applied after the lookup, i.e. in the normalised domain. */
#define HS_LAYOUT_HWC 0
#define HS_LAYOUT_CHW 1
int hs_image_ingest_fwd(const uint8_t* x, int32_t layout, int32_t batch, int32_t channels, int32_t H, int32_t W, const float* table,
                        float* y, void* stream);
int hs_stem_dw_u8_fwd(const uint8_t* x, int32_t layout, const float* table, int32_t batch, int32_t H, int32_t W,
                      const float* w_stem28, int32_t c_mid, const float* scale0, const float* shift0, int32_t stem_pad_t,
                      int32_t stem_pad_l, int32_t Hs, int32_t Ws, const float* w_dw, int32_t k, int32_t pad_t, int32_t pad_l,
                      const float* scale1, const float* shift1, float* y, float* pool_partial, void* stream);
/* Served overlays (csrc/hs_overlay.hip): the class map coloured and alpha-blended over the uint8 frame, as uint8 RGB in the frame's
 * layout -- the reference's tensor2rgb(blend_seg(img, pred, color_map, alpha, ignore_index)) (hyperseg/test.py:230-292,
 * utils/seg_utils.py:82-103, utils/img_utils.py:62-75) for img = (frame / 255 - 0.5) / 0.5.  tables: 512 + 3 * num_colors floats built on
 * the host in float32 (hyperseg_amd.utils.inference.Overlay): A[256] = img * am, A1[256] = img, S[num_colors][3] =
 * (color / 128 - 1) * (1 - am) with am = 1 - alpha.  A pixel whose class is ignore_index or >= num_colors keeps the frame's byte; every
 * other pixel is uint8(rint(((A[v] + S[c][ch]) * 0.5 + 0.5) * 255)).  1 <= num_colors <= 256; overlay must not alias frames.  Any H, W >= 1
 * and any alignment of frames / overlay.  Neither entry reads anything back: both are capturable.
 *   hs_overlay_fwd: from finished masks (batch, H, W) uint8; batch <= 65535.
 *   hs_upsample_overlay_fwd: hs_upsample_argmax_fwd (same taps, same arg-max rule, both of its forms) with the blend as the launch's
 *     epilogue: writes mask (batch, Ho, Wo), bit-identical to hs_upsample_argmax_fwd's, and overlay; frames are (batch, Ho, Wo) frames.
 *     mask 4-byte aligned where the exact-2x form applies, else HS_ERR_UNSUPPORTED.
 *   hs_upsample2_overlay_fwd: the overlay at another size than the model's frame (the camera frame's): the same over two composed resizes
 *     x (Hi, Wi) -> (Hm, Wm) -> (Ho, Wo), in both forms of hs_upsample2_confusion_fwd (both stages exact 2x: one 3 x 4 neighbourhood of x
 *     per 4 x 8 output block; any other pair, down-sampling and identity stages included): mask (batch, Ho, Wo) bit-identical to that
 *     entry's masks-only call, overlay byte-identical to hs_overlay_fwd(mask, frames); frames are (batch, Ho, Wo) frames.  mask 4-byte
 *     aligned where the 2x o 2x form applies, else HS_ERR_UNSUPPORTED; channels <= 256 and each plane below 2^31 - 4096 pixels, else
 *     HS_ERR_UNSUPPORTED.  Neither resized logits tensor exists in memory; nothing is read back: capturable. */
int hs_overlay_fwd(const uint8_t* masks, const uint8_t* frames, int32_t layout, int32_t batch, int32_t H, int32_t W,
                   const float* tables, int32_t num_colors, int32_t ignore_index, uint8_t* overlay, void* stream);
int hs_upsample_overlay_fwd(const float* x, int32_t batch, int32_t channels, int32_t Hi, int32_t Wi, int32_t Ho, int32_t Wo,
                            const uint8_t* frames, int32_t layout, const float* tables, int32_t num_colors, int32_t ignore_index,
                            uint8_t* mask, uint8_t* overlay, void* stream);
int hs_upsample2_overlay_fwd(const float* x, int32_t batch, int32_t channels, int32_t Hi, int32_t Wi, int32_t Hm, int32_t Wm, int32_t Ho,
                             int32_t Wo, const uint8_t* frames, int32_t layout, const float* tables, int32_t num_colors,
                             int32_t ignore_index, uint8_t* mask, uint8_t* overlay, void* stream);
/* Served confidence maps (csrc/hs_confidence.hip): beside the uint8 arg-max mask, the soft-max probability of the winning class of every
 * output pixel.  For the class scores v_0 .. v_{C-1} of a pixel -- exactly what hs_upsample_bilinear_fwd stores for it -- the mask is the
 * arg-max (strictly greater wins: the lowest class on ties) and the confidence is softmax(v)[argmax] = 1 / sum_c exp(v_c - v_max), taken in
 * fp32 in one ascending pass over the classes with a running maximum m and a rescaled running sum s (csrc/hs_confidence.h: v_c > m gives
 * s = s * expf(m - v_c) + 1, m = v_c; otherwise s += expf(v_c - m)), by the same device function in all three entries, so their
 * confidences agree to the bit.  channels == 1 gives 1.0.  A pixel with a non-finite score has an unspecified confidence, changes no other
 * pixel, and keeps the mask byte the arg-max entry of the same shape writes.
 *   conf (batch, Ho, Wo), conf_dtype: HS_CONF_F32 (float) or HS_CONF_U8 (the served form: (uint8)(conf * 255.0f + 0.5f));
 *   mask (batch, Ho, Wo) uint8; a pixel whose fp32 confidence is < threshold gets the byte `fill` (0..255) there instead of its class
 *     (pseudo-labels with an ignore value); conf is not changed by it.  threshold <= 0 fills nothing.
 * channels <= 256 else HS_ERR_UNSUPPORTED; any H, W >= 1 (each plane below 2^31 - 4096 pixels) and any alignment of logits / mask / conf
 * (wide loads and stores are taken where the addresses allow, single elements otherwise).  Nothing is read back: capturable.
 *   hs_confidence_fwd: from finished fp32 logits (batch, channels, H, W) -- the composed route's kernel.
 *   hs_upsample_confidence_fwd: hs_upsample_argmax_fwd (same taps, same arg-max rule, both of its forms, the identity included) with the
 *     confidence as the launch's epilogue: mask bit-identical to hs_upsample_argmax_fwd's (before the threshold), conf bit-identical to
 *     hs_upsample_bilinear_fwd + hs_confidence_fwd; the resized logits never exist in memory.
 *   hs_upsample2_confidence_fwd: the same over two composed resizes x (Hi, Wi) -> (Hm, Wm) -> (Ho, Wo), in both forms of
 *     hs_upsample2_confusion_fwd (both stages exact 2x; any other pair, down-sampling and identity stages included): mask bit-identical to
 *     that entry's, conf to two hs_upsample_bilinear_fwd + hs_confidence_fwd. */
typedef enum { HS_CONF_F32 = 0, HS_CONF_U8 = 1 } hs_conf_dtype;
int hs_confidence_fwd(const float* logits, int32_t batch, int32_t channels, int32_t H, int32_t W, int32_t conf_dtype, float threshold,
                      int32_t fill, uint8_t* mask, void* conf, void* stream);
int hs_upsample_confidence_fwd(const float* x, int32_t batch, int32_t channels, int32_t Hi, int32_t Wi, int32_t Ho, int32_t Wo,
                               int32_t conf_dtype, float threshold, int32_t fill, uint8_t* mask, void* conf, void* stream);
int hs_upsample2_confidence_fwd(const float* x, int32_t batch, int32_t channels, int32_t Hi, int32_t Wi, int32_t Hm, int32_t Wm, int32_t Ho,
                                int32_t Wo, int32_t conf_dtype, float threshold, int32_t fill, uint8_t* mask, void* conf, void* stream);
/* Camera-size uint8 frames and their labels resized on the device with Pillow's arithmetic (csrc/hs_resample.hip): what the reference's
 * torchvision Resize / RandomResize compute on PIL images (hyperseg/datasets/seg_transforms.py:224-246), plus the crop, pad and flip that
 * follow them (:249-334) as a VIEW, so that only what the crop keeps is resampled.  One geometry per launch, shared by the batch.
 * Tables (built on the host in float64, hyperseg_amd/utils/resample.py; int32, on the device), per axis, for source size S -> resized R:
 *   bounds (R, 2) = (first source index, taps) and kk (R, ksize) 22-bit fixed-point weights, zero-padded (frames);  index (R,) (labels).
 * View: output pixel (y, x) of (Ho, Wo) is resized pixel (oy + y, ox + (hflip ? Wo - 1 - x : x)) of (Hr, Wr), or the fill where that lies
 * outside; the identity view is Ho = Hr, Wo = Wr, oy = ox = 0, hflip = 0.
 *   hs_frame_resize_fwd: x uint8 (B, Hi, Wi, 3) | (B, 3, Hi, Wi) by layout.  A pixel is clip8((2^21 + sum px kk) >> 22) along the width
 *     first, into Pillow's uint8 intermediate (kept in registers, never written), then along the height.  norm_table null: y uint8 in the
 *     input's layout; else y float32 (B, 3, Ho, Wo), every byte -- the fill included (fill_rgb = r | g << 8 | b << 16) -- looked up in
 *     the (3, 256) table of hs_image_ingest_fwd.  Any ksize >= 1 on either axis, any sizes >= 1, any alignment of x and y (a float's 4
 *     bytes for the float form).  Table bounds are clamped to the source.  The caller guarantees 255 * sum |kk| + 2^21 < 2^31 per table row
 *     (true for both filters at every scale; utils/resample.py asserts it).
 *   hs_label_resize_fwd: x (B, Hi, Wi) and y (B, Ho, Wo), each HS_EVAL_U8 or HS_EVAL_I64: a gather through the two index tables.
 * HS_ERR_UNSUPPORTED -- nothing launched -- for batch > 65535, any of Hi, Wi, Hr, Wr, Ho, Wo above 2^19, or |oy|, |ox| above 2^19.
 * Neither entry reads anything back: both are capturable. */
int hs_frame_resize_fwd(const uint8_t* x, int32_t layout, int32_t batch, int32_t Hi, int32_t Wi,
                        const int32_t* y_bounds, const int32_t* y_kk, int32_t y_ksize, int32_t Hr,
                        const int32_t* x_bounds, const int32_t* x_kk, int32_t x_ksize, int32_t Wr,
                        int32_t Ho, int32_t Wo, int32_t oy, int32_t ox, int32_t hflip, uint32_t fill_rgb,
                        const float* norm_table, void* y, void* stream);
int hs_label_resize_fwd(const void* x, int32_t in_dtype, int32_t batch, int32_t Hi, int32_t Wi,
                        const int32_t* y_index, int32_t Hr, const int32_t* x_index, int32_t Wr,
                        int32_t Ho, int32_t Wo, int32_t oy, int32_t ox, int32_t hflip, int32_t fill,
                        void* y, int32_t out_dtype, void* stream);
/* The same two resizes for a batch whose samples each have a geometry of their own (RandomResize draws a continuous scale), the
 * tables built on the device (csrc/hs_resample_batch.hip): three launches per batch, nothing built or cached on the host.
 * params: int32 (batch, 6) on the device = Hr, Wr, oy, ox, hflip, reserved -- the resized size, the signed offset of the (Ho, Wo)
 * window in the resized image, the flip of the window; read when the kernels RUN, so a captured graph replays with what it holds then.
 * Workspace, caller-owned int32, M = max(Ho, Wo), axis 0 = y, row j = window position, resized index r = o + j:
 *   bounds (batch, 2, M, 2), kk (batch, 2, M, ks_max) zero-padded, nearest (batch, 2, M), status (batch).
 *   hs_resize_tables_fwd: fills all four.  filter: HS_RESIZE_BILINEAR | HS_RESIZE_BICUBIC.  The integers equal
 *     utils/resample.py's resample_coeffs / nearest_index rows o .. o + extent - 1 (float64 in the host's operation order; the
 *     nearest table by Pillow's serial accumulation, one lane per sample and axis).  Rows with r outside [0, size_r), and rows past
 *     the axis's extent, are (0, 0), zeros and 0.  status[b]: 0, or the sum of the HS_RESIZE_STATUS_* codes that apply -- Hr < 1,
 *     Wr < 1, a resized size above 2^19, more taps than ks_max on an axis; such a sample's tables are all-empty.
 *   hs_frame_resize_batch_fwd / hs_label_resize_batch_fwd: hs_frame_resize_fwd / hs_label_resize_fwd per sample, same bytes, one
 *     launch for the batch; a sample with a non-zero status is fill everywhere, the others are not affected by it.
 * Tap counts are clamped to ks_max and first indices to the source, table rows are addressed by window position only: no value in
 * params can make an access leave the workspace or the frames.  HS_ERR_UNSUPPORTED -- nothing launched -- for batch > 65535, any of
 * Hi, Wi, Ho, Wo above 2^19 or ks_max above 4096.  Nothing is read back: capturable. */
#define HS_RESIZE_BILINEAR 0
#define HS_RESIZE_BICUBIC 1
#define HS_RESIZE_STATUS_HR 1
#define HS_RESIZE_STATUS_WR 2
#define HS_RESIZE_STATUS_Y_TAPS 4
#define HS_RESIZE_STATUS_X_TAPS 8
#define HS_RESIZE_STATUS_SIZE 16
int hs_resize_tables_fwd(const int32_t* params, int32_t batch, int32_t Hi, int32_t Wi, int32_t Ho, int32_t Wo, int32_t filter,
                         int32_t ks_max, int32_t* bounds, int32_t* kk, int32_t* nearest, int32_t* status, void* stream);
int hs_frame_resize_batch_fwd(const uint8_t* x, int32_t layout, int32_t batch, int32_t Hi, int32_t Wi, const int32_t* params,
                              const int32_t* bounds, const int32_t* kk, const int32_t* status, int32_t ks_max,
                              int32_t Ho, int32_t Wo, uint32_t fill_rgb, const float* norm_table, void* y, void* stream);
int hs_label_resize_batch_fwd(const void* x, int32_t in_dtype, int32_t batch, int32_t Hi, int32_t Wi, const int32_t* params,
                              const int32_t* nearest, const int32_t* status, int32_t Ho, int32_t Wo, int32_t fill,
                              void* y, int32_t out_dtype, void* stream);
/* A dataset's label encoding on the device (csrc/hs_label_codec.hip, csrc/hs_label_codec.h; the rules and their CPU twin:
 * hyperseg_amd/utils/labels.py), the per-pixel step the reference's loaders do on the host before their transforms see a label.
 * codec_kind HS_CODEC_TABLE (hyperseg/datasets/cityscapes.py:210-211): a raw id outside [0, n) becomes values[0], every other id v
 *   becomes values[v]; 1 <= n <= 256.  codec_words: int32 (64), on the device = the 256 table bytes, little-endian, entries from n on
 *   holding values[0].  x (B, H, W), HS_EVAL_U8 or HS_EVAL_I64 (in_kind / in_dtype).  unmatched is not read.
 * codec_kind HS_CODEC_COLORS (hyperseg/datasets/camvid.py:96-98): the index of the LAST of the n colours equal to the pixel, or
 *   unmatched (0..255) where none is; 1 <= n <= 255.  codec_words: int32 (1 + n) = n, then the colours r | g << 8 | b << 16.
 *   x uint8 (B, H, W, 3): in_kind / in_dtype must be HS_EVAL_U8.
 * y (B, ., .) is HS_EVAL_U8 or HS_EVAL_I64 (out_dtype); every result is a byte value.
 *   hs_label_encode_fwd: whole images, one launch.  Any alignment of x and y; the wide loads and stores are taken where the addresses
 *     allow them.  HS_ERR_UNSUPPORTED -- nothing launched -- for batch > 65535.
 *   hs_label_resize_coded_fwd / hs_label_resize_batch_coded_fwd: hs_label_resize_fwd / hs_label_resize_batch_fwd reading RAW labels: the
 *     source pixel is gathered (3 bytes of a colour image), encoded and stored.  fill is stored AS GIVEN, never encoded: the reference
 *     pads and crops after its dataset has encoded, with a class value.  Everything else as the un-coded entries, their limits included.
 * Anything else in codec_kind, n, unmatched or the input type: HS_ERR_BAD_ARG.  Nothing is read back: capturable. */
#define HS_CODEC_NONE 0
#define HS_CODEC_TABLE 1
#define HS_CODEC_COLORS 2
int hs_label_encode_fwd(const void* x, int32_t in_kind, int32_t batch, int32_t H, int32_t W, const int32_t* codec_words,
                        int32_t codec_kind, int32_t n, int32_t unmatched, void* y, int32_t out_dtype, void* stream);
int hs_label_resize_coded_fwd(const void* x, int32_t in_dtype, int32_t batch, int32_t Hi, int32_t Wi,
                              const int32_t* y_index, int32_t Hr, const int32_t* x_index, int32_t Wr,
                              int32_t Ho, int32_t Wo, int32_t oy, int32_t ox, int32_t hflip, int32_t fill,
                              const int32_t* codec_words, int32_t codec_kind, int32_t n, int32_t unmatched,
                              void* y, int32_t out_dtype, void* stream);
int hs_label_resize_batch_coded_fwd(const void* x, int32_t in_dtype, int32_t batch, int32_t Hi, int32_t Wi, const int32_t* params,
                                    const int32_t* nearest, const int32_t* status, int32_t Ho, int32_t Wo, int32_t fill,
                                    const int32_t* codec_words, int32_t codec_kind, int32_t n, int32_t unmatched,
                                    void* y, int32_t out_dtype, void* stream);
/* torchvision's ColorJitter on uint8 RGB frames with Pillow's bytes (csrc/hs_jitter.hip; the arithmetic: hyperseg_amd/utils/jitter.py):
 * up to four operations per sample, each on the uint8 result of the one before, in the order its record gives.
 * table: int32 (B, HS_JITTER_TABLE_WORDS), on the device, one record per sample -- word 0 the order, 4 bits per operation from the lowest
 *   (1 brightness, 2 contrast, 3 saturation, 4 hue; 0 ends it); words 1-3 the float32 bits of the brightness, contrast and saturation
 *   factors; word 4 the hue shift, a byte added to H mod 256; word 5 the operations present, bit `code` each; words 6-7 unused.  The
 *   kernels read it when they RUN: a captured graph replays with what the table holds then.  No record can make an access leave the
 *   frame; an unknown code ends the order.
 * x uint8 (B, H, W, 3) | (B, 3, H, W) by layout.  norm_table null: y uint8 in the input's layout; else y float32 (B, 3, H, W), every
 *   byte looked up in the (3, 256) table of hs_image_ingest_fwd.  Any alignment of x and y (a float's 4 bytes for the float form).
 * sums: B 64-bit words of workspace for the contrast mean (cleared, filled and read by the call: a clear, the mean pass over the
 *   samples that name contrast, the apply pass).  Null -- the caller's promise that no record names contrast -- launches the apply
 *   pass alone; a record that names contrast all the same blends against 0.
 * HS_ERR_UNSUPPORTED -- nothing launched -- for batch > 65535 or H or W above 2^19.  Nothing is read back: capturable. */
#define HS_JITTER_TABLE_WORDS 8
int hs_color_jitter_fwd(const uint8_t* x, int32_t layout, int32_t batch, int32_t H, int32_t W, const int32_t* table,
                        uint64_t* sums, const float* norm_table, void* y, void* stream);
/* Pillow's ImageFilter.GaussianBlur on uint8 RGB frames with Pillow's bytes (csrc/hs_blur.hip; the arithmetic: hyperseg_amd/utils/blur.py):
 * an extended box blur, three box passes along the rows and three along the columns, each on the uint8 result of the one before.
 * table: int32 (B, HS_BLUR_TABLE_WORDS), on the device, one record per sample -- word 0 the apply flag (0: the sample comes out as it
 *   went in), word 1 the box radius r, words 2-3 the 8.24 weights ww and fw of one pass,
 *   out[x] = (ww * sum(in[clamp(x + d)], |d| <= r) + fw * (in[clamp(x - r - 1)] + in[clamp(x + r + 1)]) + 2^23) >> 24 in 32 unsigned bits.
 *   The kernels read it when they RUN: a captured graph replays with what the table holds then.  No record can make an access leave the
 *   frame or the LDS: r is the only word that moves an address, and a record with r outside [0, HS_BLUR_MAX_RADIUS] leaves its sample
 *   unblurred (as apply 0 does) and sets status[b] = HS_BLUR_STATUS_RADIUS; ww and fw are used as they are.
 * status: int32 (B), on the device; every call writes all B words (0 where the record was taken).
 * x uint8 (B, H, W, 3) | (B, 3, H, W) by layout.  tmp: uint8 workspace of x's size, the row launch's result.  norm_table null: y uint8
 *   in the input's layout; else y float32 (B, 3, H, W), every byte -- of an unblurred sample too -- looked up in the (3, 256) table of
 *   hs_image_ingest_fwd by the column launch.  Any alignment of x, tmp and y (a float's 4 bytes for the float form).  Two launches.
 * HS_ERR_UNSUPPORTED -- nothing launched -- for batch > 65535 or H or W above HS_BLUR_MAX_DIM = 2^15 (3 H W then fits 32 unsigned bits
 *   and a launch's tiles one grid dimension; offsets are 64-bit all the same).  Nothing is read back: capturable. */
#define HS_BLUR_TABLE_WORDS 4
#define HS_BLUR_MAX_RADIUS 15
#define HS_BLUR_MAX_DIM 32768
#define HS_BLUR_STATUS_RADIUS 1
int hs_gaussian_blur_fwd(const uint8_t* x, int32_t layout, int32_t batch, int32_t H, int32_t W, const int32_t* table,
                         uint8_t* tmp, const float* norm_table, void* y, int32_t* status, void* stream);
/* uint8 frames and labels rotated on the device with Pillow's arithmetic (csrc/hs_rotate.hip; the arithmetic: hyperseg_amd/utils/rotate.py):
 * PIL.Image.rotate(angle, expand=False) about the centre, what the reference's RandomRotation runs (hyperseg/datasets/seg_transforms.py:
 * 384-426), and the ConstantPad after it (:181-217) as a VIEW: the output is (Ho, Wo), the rotated (H, W) image at its top-left corner, a
 * pad fill right of and below it (Ho < H or Wo < W simply shows less of the rotated image).  One size per launch, one transform per sample.
 *   hs_frame_rotate_fwd: x uint8 (B, H, W, 3) | (B, 3, H, W) by layout; matrices float64 (B, 6), on the device: output pixel (x, y) reads
 *     the source at ((m0 xi + m1 yi) + m2, (m3 xi + m4 yi) + m5), xi = x + 0.5, yi = y + 0.5 -- BICUBIC, Pillow's float64 4 x 4 filter
 *     with truncation to the byte; outside the source the rotation fill (fill_rgb = r | g << 8 | b << 16).  norm_table null: y uint8 in
 *     the input's layout; else y float32 (B, 3, Ho, Wo), every byte -- both fills included -- looked up in the (3, 256) table of
 *     hs_image_ingest_fwd.  Any alignment of x and y (a float's 4 bytes for the float form).
 *   hs_label_rotate_fwd: x (B, H, W) and y (B, Ho, Wo), each HS_EVAL_U8 or HS_EVAL_I64; fixed int32 (B, 6), on the device, Pillow's 16.16
 *     coefficients: NEAREST, source (xs, ys) = ((a2 + y a1 + x a0) >> 16, (a5 + y a4 + x a3) >> 16), the fill outside.
 * Both read their table when they RUN: a captured graph replays with what the table holds then.  No table can make an access leave the
 * frame.  HS_ERR_UNSUPPORTED -- nothing launched -- for batch > 65535 or any of H, W, Ho, Wo above 8192 (up to there no intermediate of
 * Pillow's 32-bit label arithmetic overflows).  Nothing is read back: capturable. */
int hs_frame_rotate_fwd(const uint8_t* x, int32_t layout, int32_t batch, int32_t H, int32_t W, const double* matrices,
                        int32_t Ho, int32_t Wo, uint32_t fill_rgb, uint32_t pad_fill_rgb, const float* norm_table,
                        void* y, void* stream);
int hs_label_rotate_fwd(const void* x, int32_t in_dtype, int32_t batch, int32_t H, int32_t W, const int32_t* fixed,
                        int32_t Ho, int32_t Wo, int32_t fill, int32_t pad_fill, void* y, int32_t out_dtype, void* stream);
/* The VOC-SBD train chain (flip -> ColorJitter -> RandomResize -> RandomRotation -> ConstantPad -> ToTensor -> Normalize) for a batch
 * whose samples differ in SIZE, a fixed number of launches per batch (csrc/hs_augment_ragged.hip).  A ragged batch is a canvas plus
 * extents: frames uint8 (batch, Hm, Wm, 3) | (batch, 3, Hm, Wm) by layout, labels (batch, Hm, Wm), and per sample the (h, w) of the
 * top-left region that is the image; what lies outside it is never read into a result.
 * params: int32 (batch, HS_RAGGED_PARAM_WORDS) on the device = h, w, Hr, Wr, hflip, 3 reserved words -- the extent, the resized size, the
 *   flip of the SOURCE (source column s is column w - 1 - s: flip-then-resize, the reference's order).  Read when the kernels RUN, as are
 *   the jitter records, the matrices and the 16.16 integers: a captured graph replays with what they hold then.
 * Workspace, caller-owned int32, M = max(Hc, Wc), axis 0 = y, row j = resized index j:
 *   bounds (batch, 2, M, 2), kk (batch, 2, M, ks_max) zero-padded, nearest (batch, 2, M), status (batch).
 *   hs_resize_tables_ragged_fwd: hs_resize_tables_fwd with the input size (h, w) per sample and the window the whole resized image; the
 *     same integers (utils/resample.py's resample_coeffs / nearest_index of (h -> Hr) and (w -> Wr); in == out is one tap of 2^22 and
 *     the identity index); rows j >= the resized size are (0, 0), zeros and 0.  status[b]: 0, or the sum of the HS_RESIZE_STATUS_* codes
 *     that apply -- those of hs_resize_tables_fwd, HS_RESIZE_STATUS_EXTENT for an extent outside [1, Hm] x [1, Wm], HS_RESIZE_STATUS_CANVAS
 *     for a resized size above (Hc, Wc); an axis has more taps than ks_max when min(ksize, its input size) does.  Such a sample's tables
 *     are all-empty, every consumer below leaves it alone and its slice of the rotate outputs is the PAD fill; the others are not
 *     affected.
 *   hs_color_jitter_ragged_fwd: hs_color_jitter_fwd over each sample's h x w region, the contrast mean that region's; y is a uint8 canvas
 *     of x's shape whose pixels outside the regions are not written.  sums as there: non-null launches a clear, the mean pass and the
 *     apply pass (three launches), null the apply pass alone.
 *   hs_frame_resize_ragged_fwd / hs_label_resize_ragged_fwd: the bytes of hs_frame_resize_fwd / hs_label_resize_fwd of the flipped
 *     region to (Hr, Wr), written to the top-left of the sample's slice of the uint8 intermediate canvas y (batch, Hc, Wc, 3) |
 *     (batch, 3, Hc, Wc) | (batch, Hc, Wc); labels (HS_EVAL_U8 or HS_EVAL_I64 in) are stored as bytes.  Pixels outside the resized image
 *     are not specified.
 *   hs_frame_rotate_ragged_fwd / hs_label_rotate_ragged_fwd: hs_frame_rotate_fwd / hs_label_rotate_fwd with (H, W) = (Hr, Wr) per sample,
 *     reading the intermediate canvas, writing (batch, 3 | -, Ho, Wo) as they do (norm_table, fills, out_dtype).
 * Every consumer clamps the extents to its canvas, table rows to the extents and tap counts to ks_max: no value in params or in a table
 * can make an access leave a canvas or the workspace.  HS_ERR_UNSUPPORTED -- nothing launched -- for batch > 65535, a canvas or output
 * dimension above 8192 or ks_max above 4096.  Nothing is read back: capturable. */
#define HS_RAGGED_PARAM_WORDS 8
#define HS_RESIZE_STATUS_EXTENT 32
#define HS_RESIZE_STATUS_CANVAS 64
int hs_resize_tables_ragged_fwd(const int32_t* params, int32_t batch, int32_t Hm, int32_t Wm, int32_t Hc, int32_t Wc, int32_t filter,
                                int32_t ks_max, int32_t* bounds, int32_t* kk, int32_t* nearest, int32_t* status, void* stream);
int hs_color_jitter_ragged_fwd(const uint8_t* x, int32_t layout, int32_t batch, int32_t Hm, int32_t Wm, const int32_t* params,
                               const int32_t* table, uint64_t* sums, uint8_t* y, void* stream);
int hs_frame_resize_ragged_fwd(const uint8_t* x, int32_t layout, int32_t batch, int32_t Hm, int32_t Wm, const int32_t* params,
                               const int32_t* bounds, const int32_t* kk, const int32_t* status, int32_t ks_max,
                               int32_t Hc, int32_t Wc, uint8_t* y, void* stream);
int hs_label_resize_ragged_fwd(const void* x, int32_t in_dtype, int32_t batch, int32_t Hm, int32_t Wm, const int32_t* params,
                               const int32_t* nearest, const int32_t* status, int32_t Hc, int32_t Wc, uint8_t* y, void* stream);
int hs_frame_rotate_ragged_fwd(const uint8_t* x, int32_t layout, int32_t batch, int32_t Hc, int32_t Wc, const int32_t* params,
                               const int32_t* status, const double* matrices, int32_t Ho, int32_t Wo, uint32_t fill_rgb,
                               uint32_t pad_fill_rgb, const float* norm_table, void* y, void* stream);
int hs_label_rotate_ragged_fwd(const uint8_t* x, int32_t batch, int32_t Hc, int32_t Wc, const int32_t* params, const int32_t* status,
                               const int32_t* fixed, int32_t Ho, int32_t Wo, int32_t fill, int32_t pad_fill, void* y, int32_t out_dtype,
                               void* stream);
int hs_mbconv_expand_dw_fwd(const float* x, int32_t batch, int32_t c_in, int32_t H, int32_t W,
                            const float* w_expand, int32_t c_mid, const float* scale0, const float* shift0,
                            const float* w_dw, int32_t k, int32_t stride, int32_t pad_t, int32_t pad_l,
                            int32_t Ho, int32_t Wo, const float* scale1, const float* shift1, float* y,
                            float* pool_partial, void* stream);
int64_t hs_mbconv_se_workgroups(int32_t batch, int32_t c_mid, int32_t k, int32_t stride, int32_t Ho, int32_t Wo);   /* per batch element */
int hs_mbconv_expand_dw_se_fwd(const float* x, int32_t batch, int32_t c_in, int32_t H, int32_t W,
                               const float* w_expand, int32_t c_mid, const float* scale0, const float* shift0,
                               const float* w_dw, int32_t k, int32_t stride, int32_t pad_t, int32_t pad_l,
                               int32_t Ho, int32_t Wo, const float* scale1, const float* shift1, float* y,
                               const hs_se_tail* se, void* stream);

/* Encoder-side helper: 1x1 convolution as an fp32 MFMA GEMM with its surroundings fused,
 *   y[b,o,p] = act(scale[o] * sum_c w[o,c] * (gate[b,c] * x[b,c,p]) + shift[o]) + residual[b,o,p]
 * (gate, scale/shift, residual optional; act = hs_act).  x (B,Cin,P), w (Cout,Cin), y (B,Cout,P), P = H*W.
 * Replaces {SE multiply, 1x1 conv, BatchNorm2d, swish, skip add} of an MBConv block (efficientnet.py:101-103, 110-124). */
int hs_pointwise_conv_fwd(const float* x, int32_t batch, int32_t c_in, int32_t pixels, const float* w, int32_t c_out,
                          const float* gate, const float* scale, const float* shift, int32_t act, const float* residual,
                          float* y, void* stream);

/* y = act(scale[c]*x + shift[c]) + residual over (B, C, P), P % 4 == 0, y may alias x: folded BatchNorm + swish (+ skip
 * add) after a stock 1x1 convolution in one launch. */
int hs_affine_act_fwd(const float* x, int32_t batch, int32_t channels, int32_t pixels, const float* scale,
                      const float* shift, int32_t act, const float* residual, float* y, void* stream);

/* Route queries of the encoder helpers (host only: nothing is launched, no pointer is read).  Each answers with the ONE static
 * predicate its launcher dispatches on -- under the current environment, the dev A/B knobs HS_SE_EARLY, HS_PW_VEC, HS_MBX_LEAN and
 * HS_MBX_OTH1 / HS_MBX_OTH2 included -- from the shape and pointer-alignment facts the launcher looks at.  Negative: the HS_ERR_* the
 * launcher would return for the shape.  For the tests that pin which kernel a case runs (tests/test_hip_encoder_f64.py).
 *
 * hs_depthwise_route -> HS_DW_ROUTE(form, k, stride, pl):
 *   HS_DW_FORM_TILED    BN0 + swish prologue, k in {3,5}, >= 256 output quads, Wo % 4 == 0, Wo / 4 divides 256, the input band of a
 *                       workgroup <= 64 KB of LDS, and (k == 5 or >= 8192 planes): whole output rows per workgroup through LDS; pl = 0
 *   HS_DW_FORM_VECTOR   W % 4 == 0, x 16-byte aligned and pad_l one of the compiled constants pl -- (k3,s1): 1; (k3,s2): 0, 1;
 *                       (k5,s1): 2; (k5,s2): 1, 2 -- tap rows as aligned 16-byte loads
 *   HS_DW_FORM_GENERIC  everything else: any pad_l / W, 4-byte loads; pl = 0
 * pad_t never enters the choice.  x_aligned16 / prologue: x is 16-byte aligned / in_scale is given. */
#define HS_DW_FORM_GENERIC 0
#define HS_DW_FORM_VECTOR 1
#define HS_DW_FORM_TILED 2
#define HS_DW_ROUTE(form, k, stride, pl) (((form) << 8) | ((k) << 4) | ((stride) << 2) | (pl))
int hs_depthwise_route(int32_t batch, int32_t channels, int32_t H, int32_t W, int32_t k, int32_t stride, int32_t pad_l,
                       int32_t Ho, int32_t Wo, int32_t x_aligned16, int32_t prologue);
/* hs_stem_route -> the form of hs_stem_conv_fwd: the vector forms need W % 4 == 0, x 16-byte aligned and pad_l 0 or 1. */
#define HS_STEM_ROUTE_GENERIC 0
#define HS_STEM_ROUTE_VECTOR_PL0 1
#define HS_STEM_ROUTE_VECTOR_PL1 2
int hs_stem_route(int32_t W, int32_t pad_l, int32_t x_aligned16);
/* hs_mbconv_route -> HS_MB_ROUTE(form, k, stride) for hs_mbconv_expand_dw_fwd (with_se_tail: hs_mbconv_expand_dw_se_fwd):
 *   HS_MB_FORM_LEAN  no SE tail, c_in in {16, 24, 32, 40} (not 32 / 40 at k 5, stride 2), c_mid % 16 == 0, Wo % 16 == 0, y / scale0 /
 *                    shift0 16-byte aligned (aligned16), c_in H W < 2^30: hs_mbconv_lean.hip
 *   HS_MB_FORM_FULL  every other shape with c_in <= 80: the general kernel (ragged tile columns, any channel counts)
 * hs_stem_dw_route -> HS_MB_ROUTE(HS_MB_FORM_STEM, 3, 1) where hs_stem_dw_fwd / hs_stem_dw_u8_fwd launch, HS_ERR_UNSUPPORTED where
 * they return it (k != 3, c_mid % 16, Ws % 16, an output window that starts outside the image, misaligned y / scale0 / shift0).
 * The instantiation's input width (KS) follows from c_in alone and the tile height from the stride; neither is part of the code. */
#define HS_MB_FORM_FULL 0
#define HS_MB_FORM_LEAN 1
#define HS_MB_FORM_STEM 2
#define HS_MB_ROUTE(form, k, stride) (((form) << 8) | ((k) << 4) | (stride))
int hs_mbconv_route(int32_t batch, int32_t c_in, int32_t H, int32_t W, int32_t c_mid, int32_t k, int32_t stride,
                    int32_t Ho, int32_t Wo, int32_t aligned16, int32_t with_se_tail);
int hs_stem_dw_route(int32_t H, int32_t W, int32_t c_mid, int32_t stem_pad_t, int32_t stem_pad_l, int32_t Hs, int32_t Ws,
                     int32_t k, int32_t aligned16);
/* hs_se_gate_route -> the form hs_se_gate_fwd takes, tried in this order (units = channels * (nblk % 4 == 0 ? nblk / 4 : nblk)):
 *   HS_SE_ROUTE_FUSED       channels % 4 == 0, channels <= 768, c_squeezed <= 32, units <= 2048: one launch, se_gate_fused_kernel<8, 3>
 *   HS_SE_ROUTE_EARLY       no w_proj, channels % 4 == 0, channels * fold <= 144 (fold = 1 / 2 / 4 for nblk <= 256 / 512 / 1024),
 *                           c_squeezed <= 8, nblk <= 1024, nblk % (4 fold) == 0, partial and w_reduce 16-byte aligned (aligned16): one workgroup
 *   HS_SE_ROUTE_FUSED_WIDE  se_gate_fused_kernel<24, 1>; compiled only with -DHS_SE_FUSED_WIDE=1 (measured negative, hs_encoder.hip): the
 *                           product build never returns this code
 *   HS_SE_ROUTE_TWO_LAUNCH  everything else: squeeze + excite
 * (The gate finished by the pooling launch's last workgroups is another ENTRY, hs_depthwise_conv_se_fwd / hs_mbconv_expand_dw_se_fwd, not
 * a route of this one; hs_se_tail_tails is its query.) */
#define HS_SE_ROUTE_FUSED 0
#define HS_SE_ROUTE_EARLY 1
#define HS_SE_ROUTE_FUSED_WIDE 2
#define HS_SE_ROUTE_TWO_LAUNCH 3
int hs_se_gate_route(int32_t channels, int32_t nblk, int32_t c_squeezed, int32_t with_w_proj, int32_t aligned16);
/* hs_pointwise_route -> HS_PW_ROUTE(nb, nt, vec): nb = ceil(c_in / 16) 16-channel K batches (1..8), nt = 16-pixel tiles per wave (4,
 * halved while the launch would have fewer than 512 workgroups), vec = 1: the interleaved 16-byte form (nt == 4, pixels % 64 == 0, x, y
 * and the residual 16-byte aligned (aligned16)).  HS_ERR_UNSUPPORTED for c_in > 128. */
#define HS_PW_ROUTE(nb, nt, vec) (((nb) << 8) | ((nt) << 4) | (vec))
int hs_pointwise_route(int32_t batch, int32_t c_in, int32_t c_out, int32_t pixels, int32_t aligned16);

/* Encoder-side helper (opt-in: prepare_for_inference(split_gemm=True); off by default): a 1x1 convolution as a GEMM on the
 * f16 matrix cores with split operands, f32 storage and accumulation,
 *   y[b,o,p] = act(sum_c w[o,c] * gate[b,c] * x[b,c,p] + shift[o]) + residual[b,o,p]
 * x (B,Cin,P), y (B,Cout,P); gate (B,Cin), shift (Cout), residual (B,Cout,P) optional, residual may be y itself (in-place
 * accumulation onto a skip tensor); act = hs_act.
 * w_frag / w_inv: the STATIC weight split once on the host into two f16 pieces of every row scaled by a power of two to
 * < 2^15, in MFMA-fragment order [ceil(Cout/16)][kp/32][piece][64 lanes][8] (lane = row % 16 + 16 * kgroup holds
 * w[16 R + row % 16][32 S + 8 kgroup + j]), and the inverse row scales padded to a multiple of 16 rows
 * (hyperseg_amd.functional.gemm_split_weights builds both).  Accuracy: per element within a few 2^-22 of sum_c |w||gate x| plus
 * the f32 summation (the derived bound: tests/util_split_ref.py).  Range: finite inputs give finite results while
 * 2^15 * sum_c |w[o,c] / R_o| |gate x| < 2^127, R_o = the power of two above row o's maximum (partial sums are kept in row-scaled
 * units); beyond that y is inf / NaN although the exact value may fit.  Magnitudes below 2^-100 (f32 subnormals included) are
 * accepted with an absolute error floor.  A non-finite x[b,c,p] makes y[b,:,p] non-finite and changes no other pixel.  kp = hs_gemm_split_kp(Cin): Cin rounded up to the workgroup's
 * K split (HS_ERR_UNSUPPORTED for Cin > 2560; hs_gemm_split_fwd itself takes Cin <= 1280, the deeper K is the 2x2 form's).  Replaces the library GEMM of an MBConv block's expand / project convolution
 * (efficientnet.py:101, 115) and, through `gate`, the SE multiply (:110-111). */
int hs_gemm_split_kp(int32_t c_in);
int hs_gemm_split_fwd(const void* w_frag, const float* w_inv, const float* gate, const float* x, const float* shift,
                      int32_t act, const float* residual, float* y, int32_t batch, int32_t c_out, int32_t c_in, int32_t kp,
                      int32_t pixels, void* stream);
/* The same launch deriving the block's squeeze-excite gate itself: the operands are those of the entry above with `gate` replaced by
 * the operands of the gate's own entry above (partial (B c_in, nblk), inv_hw, w_reduce (c_squeezed, c_in), b_reduce, w_expand_t
 * (c_squeezed, c_in), b_expand).  Every workgroup runs the three phases of csrc/hs_se_gate_phases.h before its first product; the
 * gate it uses equals the FUSED form's bit for bit, hence so does y.  gate_out (B, c_in) / squeezed_out (B, c_squeezed): optional,
 * written by one workgroup per frame.  Covered exactly where the gate's own query answers HS_SE_ROUTE_FUSED (no w_proj) AND the
 * launch above takes a FAST single-chunk form (c_in % 8 == 0, pixels % 2 == 0), with partial and w_reduce 16-byte aligned:
 * c_in <= 768, c_squeezed <= 32, units <= 2048.  Anything else: HS_ERR_UNSUPPORTED, nothing launched.  Waves, 16-pixel strips and
 * row tiles per workgroup are the launch above's for the same shape.
 * The route query -> HS_GSE_ROUTE(ks, nwv): k-steps per wave (1..3) and waves per workgroup (2, 4, 8). */
#define HS_GSE_ROUTE(ks, nwv) (((ks) << 4) | (nwv))
int hs_gemm_split_se_fwd(const void* w_frag, const float* w_inv, const float* partial, int32_t nblk, float inv_hw,
                         const float* w_reduce, const float* b_reduce, int32_t c_squeezed, const float* w_expand_t,
                         const float* b_expand, const float* x, const float* shift, int32_t act, const float* residual,
                         float* y, int32_t batch, int32_t c_out, int32_t c_in, int32_t kp, int32_t pixels,
                         float* gate_out, float* squeezed_out, void* stream);
int hs_gemm_split_se_route(int32_t channels, int32_t nblk, int32_t c_squeezed, int32_t c_out, int32_t pixels, int32_t aligned16);
/* Conv2d(c_in, c_out, kernel 2, stride 2, no padding, no bias) + shift + act with the same arithmetic: x (B,c_in,2Ho,2Wo) ->
 * y (B,c_out,Ho,Wo), the window read on load (K = 4 c_in, k = 4 c + 2 dy + dx: the conv weight's own flatten order; no im2col
 * copy).  w_frag / w_inv from the (c_out, 4 c_in) weight, kp = hs_gemm_split_kp(4 c_in); 34 <= c_in <= 640, c_in and Wo even,
 * x 16-byte aligned, else HS_ERR_UNSUPPORTED.  pool_partial (optional): (B, c_out, ceil(Ho Wo / 16)) sums of y over blocks of 16
 * consecutive pixels -- the global average pool that follows, without a launch of its own (hs_pooled_shift_fwd reads it).
 * Replaces F.conv2d + BatchNorm + ReLU of the context head's down blocks (hyperseg_v1_0.py:396-401). */
int hs_gemm_split_conv2x2_fwd(const void* w_frag, const float* w_inv, const float* x, const float* shift, int32_t act, float* y,
                              float* pool_partial, int32_t batch, int32_t c_out, int32_t c_in, int32_t kp, int32_t Ho,
                              int32_t Wo, void* stream);
/* hs_gemm_split_fwd without gate / residual, its (B,c_out,Ho,Wo) result stored nearest-2x upsampled: y (B,c_out,2Ho,2Wo), 8-byte
 * aligned.  The context head's last merge writes straight into the right half of the signal (hyperseg_v1_0.py:409-410: neither
 * the upsampled tensor nor the concatenation is built). */
int hs_gemm_split_up2_fwd(const void* w_frag, const float* w_inv, const float* x, const float* shift, int32_t act, float* y,
                          int32_t batch, int32_t c_out, int32_t c_in, int32_t kp, int32_t Ho, int32_t Wo, void* stream);
/* shift_out[m] = shift[m] + sum_c wb[m][c] * (inv_pixels * sum_j partial[c][j]), partial (channels, nblk) as written by
 * hs_gemm_split_conv2x2_fwd for ONE frame, wb (rows, channels): where the context head concatenates a feature map with its own
 * global average (hyperseg_v1_0.py:404-409) the pooled half contributes a per-row constant to the following 1x1 convolution --
 * this is that constant folded into the BatchNorm shift (mean + mat-vec in one launch).  channels <= 8192. */
int hs_pooled_shift_fwd(const float* partial, int32_t nblk, float inv_pixels, const float* wb, const float* shift,
                        float* shift_out, int32_t rows, int32_t channels, void* stream);

/* Training-path re-layouts and loss reduction (hs_train_aux.hip; dtype = hs_dtype, plain contiguous tensors).
 * Halo tiles: a train-mode v1_0 inverted residual (hyperseg_v1_0.py:328-376) applies each patch's weights to the patch's own
 * reflect-padded (ph+2) x (pw+2) tile; the tiles are laid side by side as one image (B, C, fh (ph+2), fw (pw+2)) so that the three layers
 * are ordinary patch convolutions.  hs_halo_tiles_fwd builds that image from x (B, C, H, W) in one gather (stock ops: F.pad(reflect) ->
 * unfold -> unfold -> permute -> reshape), hs_halo_tiles_bwd is its adjoint (a gather too: per image pixel the <= 16 tile positions that
 * map onto it); hs_tile_interior_fwd drops the halos again, hs_tile_interior_bwd is its adjoint (zeros on the halos). */
int hs_halo_tiles_fwd(int32_t dtype, const void* x, int32_t batch, int32_t channels, int32_t H, int32_t W, int32_t fh, int32_t fw,
                      void* tiled, int32_t patch_major, void* stream);
int hs_halo_tiles_bwd(int32_t dtype, const void* dtiled, int32_t batch, int32_t channels, int32_t H, int32_t W, int32_t fh, int32_t fw,
                      void* dx, int32_t patch_major, void* stream);
/* patch_major (hs_halo_tiles_*, hs_dw_tiles_*): 0 = the tiles side by side as one image (B, C, fh (ph+2), fw (pw+2)); 1 = one tile after the
 * other, (B fh fw, C, ph+2, pw+2) -- every operand of a patch is then one contiguous run and the block's 1x1 layers are patch convolutions
 * with a (1, 1) grid over B fh fw "frames" (same kernels, same bank rows).  hs_tile_interior_* take the image form only. */
int hs_tile_interior_fwd(int32_t dtype, const void* tiled, int32_t batch, int32_t channels, int32_t H, int32_t W, int32_t fh,
                         int32_t fw, void* y, void* stream);
int hs_tile_interior_bwd(int32_t dtype, const void* dy, int32_t batch, int32_t channels, int32_t H, int32_t W, int32_t fh, int32_t fw,
                         void* dtiled, void* stream);
/* The middle layer of that block as the reference states it -- a VALID depthwise 3 x 3 of every halo tile with the patch's own taps
 * (hyperseg_v1_0.py:352-360: F.conv2d on the unfolded, padded patches with padding 0): tile image (B, C, fh (ph+2), fw (pw+2)) -> (B, C, H, W)
 * in one launch, its two adjoints in one launch each.  Replaces hs_patch_conv_plain_* (k = 3, zero padding, on the whole tile image) +
 * hs_tile_interior_*: no ring outputs, no intermediate.  bank / dbank: fp32 (P, ld) with the taps of channel c at columns [9 c, 9 c + 9)
 * (the depthwise range of the block's bank: pass bank + r1); dtype = hs_dtype of the activations.  Even patch widths only
 * (HS_ERR_UNSUPPORTED otherwise: the caller keeps the two-launch route).  autograd.DwTilesValid. */
int hs_dw_tiles_fwd(int32_t dtype, const void* tiled, const float* bank, int64_t ld, int32_t batch, int32_t channels, int32_t H, int32_t W,
                    int32_t fh, int32_t fw, void* y, int32_t patch_major, void* stream);
int hs_dw_tiles_bwd_in(int32_t dtype, const void* dy, const float* bank, int64_t ld, int32_t batch, int32_t channels, int32_t H, int32_t W,
                       int32_t fh, int32_t fw, void* dtiled, int32_t patch_major, void* stream);
int hs_dw_tiles_bwd_w(int32_t dtype, const void* tiled, const void* dy, int32_t batch, int32_t channels, int32_t H, int32_t W, int32_t fh,
                      int32_t fw, float* dbank, int64_t ld, int32_t patch_major, void* stream);
/* The per-image reduction of hyperseg/losses/bootstrapped_ce_loss.py:19-25 over n non-negative f32 losses, with no sort and no host
 * read: if more than k losses exceed thresh, their mean; otherwise the mean of the k largest (the k-th largest found by a three-level
 * radix histogram of the bit patterns; ties at it share the remaining weight).  out5 = {loss, branch, 1/count, t, tie weight}: the
 * state hs_bootstrap_mean_bwd turns into d loss / d values.  workspace: hs_bootstrap_mean_workspace() bytes, scratch.  n > k. */
int64_t hs_bootstrap_mean_workspace(void);
/* The batch form the loss module uses: the batched reduction + the mean of the per-image losses (bootstrapped_ce_loss.py:33, loss / batch)
 * in mean_out (one float), and the adjoint from the ONE upstream gradient of that mean. */
int hs_bootstrap_mean_of_batch_fwd(const float* values, int32_t images, int32_t n, int32_t k, float thresh, void* workspace,
                                   float* out8, float* mean_out, void* stream);
int hs_bootstrap_mean_of_batch_bwd(const float* values, int32_t images, int32_t n, const float* state8, const float* grad_mean,
                                   float* grad_values, void* stream);
/* Adam (torch.optim.Adam / AdamW arithmetic, no amsgrad) for up to 48 fp32 tensors in ONE launch of 1024-element workgroups: the
 * training loop's optimizer step (hyperseg/train.py:185-188) without torch's 65 536-element chunking.  The arrays are HOST arrays of device
 * pointers; `steps`: hs_adam_blocks(numel, n) floats on the device, zero before the first step, owned by this parameter list (one step
 * count per workgroup: graph replay freezes kernel arguments); lr_device (optional) overrides lr.  decoupled: AdamW's weight decay. */
int64_t hs_adam_blocks(const int64_t* numel, int32_t n);
int hs_adam_step(float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq, const int64_t* numel,
                 int32_t n, const float* lr_device, float lr, double beta1, double beta2, float eps, float weight_decay, int32_t decoupled,
                 int32_t maximize, float* steps, void* stream);
/* ... under a GradScaler (torch.optim.Adam(fused=True)'s protocol, no host read): grad_scale (device float, may be null) and found_inf
 * (device float) are what torch.amp.GradScaler.step hands the optimizer.  *found_inf != 0: nothing is written -- no parameter, no moment,
 * no step word.  Otherwise every gradient is divided by *grad_scale (if given), written back to `grads` unscaled, and the step is taken. */
int hs_adam_step_amp(float* const* params, float* const* grads, float* const* exp_avg, float* const* exp_avg_sq, const int64_t* numel,
                     int32_t n, const float* lr_device, float lr, double beta1, double beta2, float eps, float weight_decay, int32_t decoupled,
                     int32_t maximize, float* steps, const float* grad_scale, const float* found_inf, void* stream);
int hs_bootstrap_mean_fwd(const float* values, int32_t n, int32_t k, float thresh, void* workspace, float* out5, void* stream);
int hs_bootstrap_mean_bwd(const float* values, int32_t n, const float* state5, const float* grad_out, float* grad_values, void* stream);
/* The same for `images` images at once (one set of launches, grid.y = image): values (images, n), workspace images x
 * hs_bootstrap_mean_workspace() bytes, out8 / state8 (images, 8) floats whose first five are out5 / state5 above, grad_out (images). */
int hs_bootstrap_mean_batched_fwd(const float* values, int32_t images, int32_t n, int32_t k, float thresh, void* workspace, float* out8,
                                  void* stream);
int hs_bootstrap_mean_batched_bwd(const float* values, int32_t images, int32_t n, const float* state8, const float* grad_out,
                                  float* grad_values, void* stream);

/* Adjoint of hs_bank_pack_fwd: patch-major bank (B fh fw, ld) -> channel-major weights (B, hp_total, fh, fw): channels
 * [ch_offset, ch_offset + rows) from the bank's columns [0, rows), exact zeros elsewhere.  Training path (autograd.BankPack). */
int hs_bank_unpack_fwd(const float* bank, int64_t ld, int32_t batch, int32_t hp_total, int32_t fh, int32_t fw, int32_t ch_offset,
                       int32_t rows, float* w, void* stream);

/* Adjoint of hs_upsample_bilinear_fwd (F.interpolate(..., mode='bilinear', align_corners=False), Ho >= Hi, Wo >= Wi): dy (B,C,Ho,Wo) ->
 * dx (B,C,Hi,Wi), a gather over the outputs whose taps touch each input pixel.  dy_batch_stride (floats; 0 = packed C*Ho*Wo): dy may be a
 * channel range of a wider (B, C_total, Ho, Wo) tensor -- the previous level's slice of a stage input's gradient -- read in place.
 * Training path (autograd.UpsampleBilinear, StageMaterialize). */
int hs_upsample_bilinear_bwd(const float* dy, int64_t dy_batch_stride, int32_t batch, int32_t channels, int32_t Hi, int32_t Wi,
                             int32_t Ho, int32_t Wo, float* dx, void* stream);
/* ... with a storage type (hs_dtype; dy and dx alike, dy_batch_stride in ELEMENTS, f32 arithmetic, one rounding on store): the bf16
 * training step keeps the stage inputs and their gradients in bf16 (autograd.StageMaterialize under torch.autocast). */
int hs_upsample_bilinear_typed_bwd(int32_t dtype, const void* dy, int64_t dy_batch_stride, int32_t batch, int32_t channels, int32_t Hi,
                                   int32_t Wi, int32_t Ho, int32_t Wo, void* dx, void* stream);

/* BatchNorm2d in TRAINING mode (torch.nn.functional.batch_norm semantics: batch statistics, biased variance for the normalisation,
 * unbiased for the running estimate, running = (1 - momentum) running + momentum batch) fused with the activation that follows it
 * (act = HS_ACT_NONE | HS_ACT_RELU | HS_ACT_RELU6), x / y / dy / dx (B, C, pixels) in `dtype` storage, parameters and statistics f32.
 * Two launches per direction.  save_mean / save_invstd (C): written by fwd, read by bwd.  gamma / beta / running_* may be NULL.
 * workspace: hs_bn_train_workspace(C) bytes, scratch; num_batches_tracked (optional): the module's int64 step counter, incremented by one.
 * Replaces BatchNorm2d + ReLU6 of hyperseg_v1_0.py:349-376 in train mode. */
int64_t hs_bn_train_workspace(int32_t channels);
/* The statistics pass of hs_bn_act_train_fwd alone: {sum, sum of squares} around the channel's first element, per channel and slice,
 * into `workspace` (hs_bn_train_workspace(C) bytes) -- for consumers that normalise on load instead of reading a normalised copy. */
int hs_bn_train_stats_fwd(int32_t dtype, const void* x, int32_t batch, int32_t channels, int64_t pixels, void* workspace, void* stream);
/* The train-mode inverted residual's BatchNorm1 + ReLU6 + depthwise 3 x 3 (hyperseg_v1_0.py:346-360) without the normalised copy of the
 * halo tiles: hs_dw_tiles_fwd / _bwd_w reading the RAW output of the first 1 x 1 layer and applying act(gamma invstd (x - mean) + beta)
 * on load.  _fwd: `bn_partial` = hs_bn_train_stats_fwd's workspace for the tile tensor viewed as (B', C, pixels) (patch-major: B' =
 * batch fh fw, pixels = (ph + 2)(pw + 2)); writes save_mean / save_invstd (C floats each), updates running_mean / running_var
 * (optional) and num_batches_tracked (optional) exactly as hs_bn_act_train_fwd.  _bwd_w: the tap gradient from the raw tiles and the
 * saved statistics.  The BatchNorm's own adjoint stays hs_bn_act_train_bwd on (raw tiles, hs_dw_tiles_bwd_in's result). */
int hs_dw_tiles_bn_fwd(int32_t dtype, const void* tiled, const float* bn_partial, const float* gamma, const float* beta,
                       float* running_mean, float* running_var, float momentum, float eps, int32_t act, float* save_mean,
                       float* save_invstd, int64_t* num_batches_tracked, const float* bank, int64_t ld, int32_t batch,
                       int32_t channels, int32_t H, int32_t W, int32_t fh, int32_t fw, void* y, int32_t patch_major, void* stream);
int hs_dw_tiles_bn_bwd_w(int32_t dtype, const void* tiled, const void* dy, const float* gamma, const float* beta, const float* save_mean,
                         const float* save_invstd, int32_t act, int32_t batch, int32_t channels, int32_t H, int32_t W, int32_t fh,
                         int32_t fw, float* dbank, int64_t ld, int32_t patch_major, void* stream);
/* The same move at the block's second cut (round 5): BatchNorm2 + ReLU6 normalised on load by the LAST 1 x 1 layer (hyperseg_v1_0.py:361-370),
 * x (B, c_in, H, W) RAW, bank rows = this layer's (c_out, c_in) weights per patch, k = 1.  _fwd: bn_partial = hs_bn_train_stats_fwd's
 * workspace for x; save_mean / save_invstd / running_* / num_batches_tracked as hs_bn_act_train_fwd.  _bwd_w: the weight gradient on the raw
 * input + saved statistics.  The input gradient is hs_patch_conv_plain_bwd_in unchanged (it yields the gradient of the normalised map),
 * BatchNorm's adjoint hs_bn_act_train_bwd on (x, that).  c_out <= 32, c_in <= 64, patches >= 64 pixels; else HS_ERR_UNSUPPORTED. */
int hs_patch_conv_bn_fwd(int32_t dtype, const void* x, const float* bn_partial, const float* gamma, const float* beta,
                         float* running_mean, float* running_var, float momentum, float eps, int32_t act, float* save_mean,
                         float* save_invstd, int64_t* num_batches_tracked, const float* bank, int64_t ld, int32_t batch,
                         int32_t c_in, int32_t H, int32_t W, int32_t fh, int32_t fw, int32_t c_out, void* y, void* stream);
int hs_patch_conv_bn_bwd_w(int32_t dtype, const void* x, const void* dy, const float* gamma, const float* beta, const float* save_mean,
                           const float* save_invstd, int32_t act, int32_t batch, int32_t c_in, int32_t H, int32_t W, int32_t fh,
                           int32_t fw, int32_t c_out, float* dbank, int64_t ld, void* stream);
int hs_bn_act_train_fwd(int32_t dtype, const void* x, int32_t batch, int32_t channels, int64_t pixels, const float* gamma,
                        const float* beta, float* running_mean, float* running_var, float momentum, float eps, int32_t act,
                        float* save_mean, float* save_invstd, void* workspace, void* y, int64_t* num_batches_tracked, void* stream);
int hs_bn_act_train_bwd(int32_t dtype, const void* x, const void* dy, int32_t batch, int32_t channels, int64_t pixels,
                        const float* gamma, const float* beta, const float* save_mean, const float* save_invstd, float eps, int32_t act,
                        void* workspace, void* dx, float* dgamma, float* dbeta, void* stream);
/* BatchNorm1's adjoint of a train-mode inverted residual WITHOUT its statistics launch (round 6; hyperseg_v1_0.py:352-360 under autograd): the
 * valid depthwise adjoint hs_dw_tiles_bwd_in, given the RAW tiles `tiled` and the statistics hs_dw_tiles_bn_fwd saved, also leaves the adjoint's two
 * per-channel sums over the tile tensor (sum of d, sum of d x_hat; d = dtiled act'(bn(tiled))) as one pair per workgroup: partial holds
 * channels x hs_dw_tiles_bn_bwd_in_partials(batch, H, W, fh, fw) pairs of floats.  hs_bn_act_train_bwd_apply = the second launch of
 * hs_bn_act_train_bwd from such pairs (n_partials per channel, combined in order): dx, dgamma, dbeta.  Same values as the two-launch adjoint up to
 * the association of the sums. */
int64_t hs_dw_tiles_bn_bwd_in_partials(int32_t batch, int32_t H, int32_t W, int32_t fh, int32_t fw);
int hs_dw_tiles_bn_bwd_in(int32_t dtype, const void* dy, const float* bank, int64_t ld, const void* tiled, const float* gamma, const float* beta,
                          const float* save_mean, const float* save_invstd, int32_t act, int32_t batch, int32_t channels, int32_t H, int32_t W,
                          int32_t fh, int32_t fw, void* dtiled, float* partial, int32_t patch_major, void* stream);
int hs_bn_act_train_bwd_apply(int32_t dtype, const void* x, const void* dy, int32_t batch, int32_t channels, int64_t pixels, const float* gamma,
                              const float* beta, const float* save_mean, const float* save_invstd, int32_t act, const float* partial,
                              int64_t n_partials, void* dx, float* dgamma, float* dbeta, void* stream);

/* signal2weights on the TRAINING path, every level of a decoder per launch (hyperseg_v1_0.py:473-484 + the permute / reshape of
 * :334-337, 491, and their autograd): the weights are the Conv2d parameters in their OWN layout (wc, signal_channels / groups) --
 * they change every step, so no transposed or packed copy exists -- and banks / bank gradients are patch-major (P, ld), P = batch*fh*fw.
 *   hs_s2w_train_fwd   bank[p, n] = sum_k w[n, k] * signal[b, signal_index + g(n) * K + k, i, j],  n < rows        (one launch)
 *   hs_s2w_train_bwd   dw[n, k] = sum_p dbank[p, n] * signal[...]  (rows in [rows, wc): exact zeros; dbank NULL = zero gradient),
 *                      dsignal[b, c, i, j] = sum over the layers whose channel range holds c of sum_n dbank[p, n] * w[n, k]
 *                      (channels no layer reads: zeros); `ds` is each layer's private (batch, signal_channels, fh, fw) scratch.
 *                      dw / dsignal may be NULL (not wanted).  workspace (hs_s2w_train_workspace bytes, scratch, optional): the
 *                      reduction of dw over the patches is then cut into slices of 64 patches across workgroups and a fourth launch
 *                      adds the slices in order; without it one workgroup walks all patches of its tile.  No atomics. */
typedef struct hs_s2w_train_layer {
    int32_t signal_index, signal_channels, groups;
    const float* w;            /* (wc, signal_channels / groups) */
    int32_t wc, rows;
    float* bank;               /* forward: (P, ld) out */
    int64_t ld;
    const float* dbank;        /* backward: (P, ld) or NULL */
    float* dw;                 /* backward: (wc, signal_channels / groups) out or NULL */
    float* ds;                 /* backward: scratch, see above */
} hs_s2w_train_layer;
int hs_s2w_train_fwd(const float* signal, int32_t batch, int32_t c_signal, int32_t fh, int32_t fw,
                     const hs_s2w_train_layer* layers, int32_t n_layers, void* stream);
int64_t hs_s2w_train_workspace(int32_t batch, int32_t fh, int32_t fw, const hs_s2w_train_layer* layers, int32_t n_layers);
int hs_s2w_train_bwd(const float* signal, int32_t batch, int32_t c_signal, int32_t fh, int32_t fw,
                     const hs_s2w_train_layer* layers, int32_t n_layers, float* dsignal, void* workspace, int64_t workspace_bytes,
                     void* stream);

/* Per-pixel cross entropy, F.cross_entropy(logits (N,C,H,W), target (N,H,W) int64, ignore_index, reduction='none') without class
 * weights -- what BootstrappedCrossEntropyLoss.forward computes before its top-k rule (hyperseg/losses/bootstrapped_ce_loss.py:20-23) --
 * and its adjoint, one launch each: loss (N,H,W) (0 at ignored pixels); grad_logits (N,C,H,W) = (softmax - onehot) * grad_loss. */
int hs_cross_entropy_fwd(const float* logits, const int64_t* target, int32_t batch, int32_t classes, int64_t pixels,
                         int64_t ignore_index, float* loss, void* stream);
int hs_cross_entropy_bwd(const float* logits, const int64_t* target, int32_t batch, int32_t classes, int64_t pixels,
                         int64_t ignore_index, const float* grad_loss, float* grad_logits, void* stream);
/* ... with the logits' storage type (hs_dtype; the logits' gradient alike; loss and grad_loss fp32; f32 arithmetic): bf16 logits straight
 * from the decoder under torch.autocast(bfloat16), where the stock op widens them with a cast launch first. */
int hs_cross_entropy_typed_fwd(int32_t dtype, const void* logits, const int64_t* target, int32_t batch, int32_t classes, int64_t pixels,
                               int64_t ignore_index, float* loss, void* stream);
int hs_cross_entropy_typed_bwd(int32_t dtype, const void* logits, const int64_t* target, int32_t batch, int32_t classes, int64_t pixels,
                               int64_t ignore_index, const float* grad_loss, void* grad_logits, void* stream);
/* BootstrappedCrossEntropyLoss.forward / backward as one entry each (hyperseg/losses/bootstrapped_ce_loss.py:15-27: per-pixel cross entropy, then per
 * image the mean of the losses above `thresh` if more than k exceed it, else of the k largest; the batch's mean of those).  Forward:
 * hs_cross_entropy_typed_fwd + hs_bootstrap_mean_of_batch_fwd; loss (N, pixels) fp32 = the per-pixel losses (kept for the adjoint),
 * out8 (N, 8) = the per-image selection state of hs_bootstrap_mean_batched_fwd, mean_out[0] = the loss.  workspace: N x hs_bootstrap_mean_workspace()
 * bytes, any contents.  pixels > k (the reference indexes ranked[k]).  Backward: ONE launch (the pixel weights are formed inside the cross entropy's
 * adjoint: no hs_bootstrap_mean_of_batch_bwd launch, no (N, pixels) gradient tensor), grad_logits (N, C, pixels) in the logits' type from the saved
 * `loss`, `out8` and the one upstream gradient grad_mean[0].  Values identical to the separate entries'. */
int hs_bootstrapped_ce_fwd(int32_t dtype, const void* logits, const int64_t* target, int32_t batch, int32_t classes, int64_t pixels,
                           int64_t ignore_index, int32_t k, float thresh, void* workspace, float* loss, float* out8, float* mean_out, void* stream);
int hs_bootstrapped_ce_bwd(int32_t dtype, const void* logits, const int64_t* target, int32_t batch, int32_t classes, int64_t pixels,
                           int64_t ignore_index, const float* loss, const float* state8, const float* grad_mean, void* grad_logits, void* stream);
/* The four entries above with class weights (nn.CrossEntropyLoss(weight, ignore_index, reduction='none') under the top-k rule): `weight` f32
 * (classes,) on the device, non-NULL else HS_ERR_BAD_ARG; everything else is the unweighted twin's contract.
 *   forward: loss = weight[t] * u, u the unweighted entry's loss -- one more f32 multiply; 0 where the target is ignore_index or outside
 *     [0, classes).
 *   adjoint: grad_logits = (softmax - onehot) * (weight[t] * upstream), upstream = grad_loss[e], or -- bootstrapped form -- the selection's
 *     weight formed from the saved (weighted) loss as in hs_bootstrapped_ce_bwd; 0 where the target is not live.
 * The selection ranks the weighted losses and relies on losses >= 0: the caller passes finite weights >= 0 (the table is never read on the
 * host; a captured graph holds its address). */
int hs_cross_entropy_weighted_fwd(int32_t dtype, const void* logits, const int64_t* target, const float* weight, int32_t batch, int32_t classes,
                                  int64_t pixels, int64_t ignore_index, float* loss, void* stream);
int hs_cross_entropy_weighted_bwd(int32_t dtype, const void* logits, const int64_t* target, const float* weight, int32_t batch, int32_t classes,
                                  int64_t pixels, int64_t ignore_index, const float* grad_loss, void* grad_logits, void* stream);
int hs_bootstrapped_ce_weighted_fwd(int32_t dtype, const void* logits, const int64_t* target, const float* weight, int32_t batch,
                                    int32_t classes, int64_t pixels, int64_t ignore_index, int32_t k, float thresh, void* workspace, float* loss,
                                    float* out8, float* mean_out, void* stream);
int hs_bootstrapped_ce_weighted_bwd(int32_t dtype, const void* logits, const int64_t* target, const float* weight, int32_t batch,
                                    int32_t classes, int64_t pixels, int64_t ignore_index, const float* loss, const float* state8,
                                    const float* grad_mean, void* grad_logits, void* stream);

/* Materialises a stage input (B, 2*coords + c_skip + c_prev, H, W); test/diagnostic twin of the
 * fused prologue (the product path never calls it). */
int hs_stage_input_fwd(const hs_stage_input* in, float* y, void* stream);
/* ... with storage types (hs_dtype): in->prev points at prev_dtype elements, y at out_dtype elements; in->skip is fp32.  The training
 * path's stage input under bf16 autocast (autograd.StageMaterialize): the previous level is read as it is stored and the result is
 * written in the type the first convolution reads, instead of a cast launch on either side. */
int hs_stage_input_typed_fwd(const hs_stage_input* in, int32_t prev_dtype, int32_t out_dtype, void* y, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HYPERSEG_HIP_H */
