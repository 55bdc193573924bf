/* scouter_hip.h -- C ABI of libscouter_hip.so, the MI355X (gfx950 / CDNA4) implementation of SCOUTER's xSlot
 * training hot path.
 *
 * The reference (wbw520/scouter) is pure Python over PyTorch; it has NO native plugin / FFI interface to copy
 * (SURVEY.md section 8b).  Each entry point below therefore replaces a PyTorch op *call site* of the reference
 * (cited as file:line under /root/reference) and is what a binding for that call site would bind to.
 *
 * Conventions
 *   - plain C types only: device pointers, sizes, a `void* stream` (hipStream_t); no torch types;
 *   - every function is asynchronous on `stream`, re-entrant, keeps no global mutable state besides the routing
 *     switches below, never allocates device memory (callers pass workspaces sized by the *_workspace_bytes
 *     helpers), never throws or exits;
 *   - return 0 on success, <0 on error (SC_ERR_* below); the message is in scouter_last_error() (thread-local);
 *   - tensors are caller-owned, dense, 16-byte aligned fp32 unless stated;
 *   - activations are NHWC ("[M = B*H*W][C]"), convolution weights are HWIO ([kh][kw][Cin/groups][Cout]).
 *
 * Beyond the training path the library holds what an explanation is drawn and scored with, each in a section of its own below:
 * the input pipeline, Grad-CAM, RISE, insertion / deletion scores, Score-CAM, path and noise batches (Integrated Gradients,
 * SmoothGrad), Grad-CAM++, the infidelity / max-sensitivity scores, the mask sides of Extremal Perturbation and of
 * information-bottleneck attribution, and the superpixel surrogates LIME and KernelSHAP.  The reference
 * computes none of the scores itself; where
 * no program exists to copy, the section's comment is the specification.
 */
#ifndef SCOUTER_HIP_H
#define SCOUTER_HIP_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

#define SC_OK 0
#define SC_ERR_ARG (-1)
#define SC_ERR_LAUNCH (-2)
#define SC_ERR_UNSUPPORTED (-3)
#define SC_ERR_WORKSPACE (-4)

int scouter_abi_version(void);
const char* scouter_last_error(void);

/* routing switches: each is read from its environment variable once, when the library first needs one, and changed
 * afterwards only here.  Names (variable, default): "xwt" (SCOUTER_XWT, 1), "bwt" (SCOUTER_BWT, 1), "bhalo"
 * (SCOUTER_BHALO, 1), "xslot_small" (SCOUTER_XSLOT_SMALL, 1), "xslot_bwd_halves" (SCOUTER_XSLOT_BWD_HALVES, 1),
 * "xslot_bwd_scratch" (SCOUTER_XSLOT_BWD_SCRATCH, 0), "pwp_bn" / "pwp_resident" (SCOUTER_PWP_PLAN_DEV="bn,resident",
 * 0 = the library's own plan).  Values are >= 0.  scouter_set_switch returns SC_ERR_ARG for an unknown name or a negative
 * value; scouter_get_switch returns the value, or SC_ERR_ARG for an unknown name.  A launch already enqueued keeps the
 * route it took. */
int scouter_set_switch(const char* name, int value);
int scouter_get_switch(const char* name);

/* ---- input pipeline on the GPU: the reference's make_transform
 * (dataset/transform_func.py:101-124) = Resize((S,S)) [:19-31, torchvision F.resize -> PIL Image.resize BILINEAR with
 * antialiasing] -> ToTensor [:51-66] -> Normalize [:91-99], for a batch of decoded uint8 HWC images of different sizes.
 * The resize is bit-identical to Pillow's 8-bit resampler (Resample.c); ToTensor+Normalize is a [C][256] float table
 * the caller fills exactly as the reference computes it (float64, then float32).
 * srcs: device array of B image pointers; hw: device [B][2] (height, width); tmp: device scratch for the horizontal
 * pass, image b at tmp + tmp_off[b], size h_b*out_w*C bytes; max_h/max_w: largest height/width in the batch (grid
 * sizing); out: float32 [B][C][out_h][out_w].  Down-scaling factors above 47 are refused. */
int scouter_resize_normalize_u8_f32(const unsigned char* const* srcs, const int* hw, unsigned char* tmp,
                                    const long* tmp_off, const float* lut, float* out, int B, int C, int max_h, int max_w,
                                    int out_h, int out_w, void* stream);
/* the same resize with the bytes stored as they are: out uint8 [B][C][out_h][out_w] -- the input of the augmentation
 * stages below (the float entry point above is unchanged). */
int scouter_resize_u8(const unsigned char* const* srcs, const int* hw, unsigned char* tmp, const long* tmp_off,
                      unsigned char* out, int B, int C, int max_h, int max_w, int out_h, int out_w, void* stream);

/* ---- training augmentation on the GPU (`--aug true`): the reference's tools/image_aug.py (imgaug Fliplr, Flipud, Affine,
 * GaussianBlur in random order, per image on a CPU worker, dataset/transform_func.py:112-118) between the resize and the
 * table lookup, on planar bytes [B][C][S][S] (C in {1, 3, 4}, 5 <= S <= 32768, B * C <= 65535).  No reference program runs
 * here (imgaug / OpenCV are third-party), so the definition -- and its departures from them: own random stream, float
 * bilinear warp, float blur, unrounded translation -- is the docstring of scouter_amd/dataset/augment.py, whose
 * `augment_host` is the yardstick.  A drawn sequence reduces to blur, warp, blur; which of them an image takes is read by
 * the kernels from per-image tables ON THE DEVICE (row b at table + b * stride, strides in 4-byte words), so a stage is
 * one launch per batch.  src and dst must differ.
 *   blur    klen[b] (0: copy; else odd, <= 9) and taps[b][0 .. klen) float32: row pass then column pass in float32, border
 *           reflect-101, products summed in ascending tap order, no rounding between the passes (the intermediate stays
 *           in LDS), one round-half-to-even to a byte.
 *   warp    identity[b] != 0: copy; else minv[b][0 .. 6) = top two rows of the inverse matrix: output (x, y) reads
 *           u = m0 x + m1 y + m2, v = m3 x + m4 y + m5 (float32: two rounded products, their rounded sum, plus the
 *           constant, no fma), bilinear over the four taps around (floor u, floor v), a tap outside counts as 0, along x
 *           then along y, round half to even, clamp, byte.
 *   finish  out float32 [B][C][S][S] = lut[c][byte], lut the [C][256] table of scouter_resize_normalize_u8_f32. */
int scouter_aug_blur_u8(const unsigned char* src, unsigned char* dst, const int* klen, int klen_stride, const float* taps,
                        int taps_stride, int B, int C, int S, void* stream);
int scouter_aug_warp_u8(const unsigned char* src, unsigned char* dst, const float* minv, int minv_stride,
                        const int* identity, int identity_stride, int B, int C, int S, void* stream);
int scouter_aug_finish_u8_f32(const unsigned char* src, const float* lut, float* out, int B, int C, int S, void* stream);

/* optional per-kernel hipEvent timing used by bench.py's roofline leg: when enabled, every launch of the conv / BN /
 * xSlot kernels is bracketed by two hipEvents on ITS stream and aggregated by kernel-instance name.
 * scouter_prof_collect writes "name\tlaunches\ttotal_ms\talgorithmic_flops\talgorithmic_bytes\n" lines into buf
 * (returns the byte count) and clears the log. */
void scouter_prof_enable(int on);
int scouter_prof_collect(char* buf, int cap);

/* ---- convolution = nn.Conv2d call sites: timm/models/resnet.py:491-501 (stem, blocks), resnest.py:111-143,
 * layers/split_attn.py:54-60 (grouped 3x3, fc1, fc2), sloter/slot_model.py:108 (conv1x1) and their autograd
 * backward (engine.py:33).  fp32 implicit GEMM on v_mfma_f32_32x32x2_f32.  Per-group channels must be multiples
 * of 32.  `bias` (per Cout), `addend` (same shape as the output) may be NULL; relu applies last.
 * bn_partial (may be NULL): the epilogue also writes per-M-tile fp64 (sum, sum of squares) of every output channel,
 * [scouter_conv2d_fwd_bn_partial_rows(...)][Cout][2], which scouter_bn_fwd_f32 accepts instead of re-reading y.
 * tile_hint: -1 = built-in heuristic, 0..3 = block tile 128x128 / 128x64 / 64x64 / 128x32 (ignored if illegal for the
 * shape).  Results are bit-identical for every tile (same K order per output element), so callers may autotune it. */
int scouter_conv2d_fwd_bn_partial_rows(int B, int H, int W, int Cin, int Cout, int kh, int kw, int stride, int pad,
                                       int groups, int tile_hint);
int scouter_conv2d_fwd_f32(const float* x, const float* w, const float* bias, const float* addend, float* y,
                           double* bn_partial, int B, int H, int W, int Cin, int Cout, int kh, int kw, int stride,
                           int pad, int groups, int relu, int tile_hint, void* stream);
int scouter_conv2d_dgrad_f32(const float* dy, const float* w, const float* addend, float* dx, int B, int H, int W,
                             int Cin, int Cout, int kh, int kw, int stride, int pad, int groups, int tile_hint,
                             void* stream);
/* Input gradient with the BatchNorm-BACKWARD reductions of its consumer fused into the epilogue.  The tensor being
 * produced is d(out) of a block output out = relu(bn(x1) [+ bn(x2) | + shortcut]) (resnet.py:404-412, resnest.py:128-143;
 * the shortcut / downsample gradient arrives through `addend`).  The epilogue applies the ReLU sign (relu_mask: the bit
 * mask scouter_bn_fwd_f32 wrote, NULL = no ReLU), stores g = d(out) * [out > 0] into dx, and writes per M tile and
 * input channel the fp64 pairs (sum g, sum g * xhat1) to part1 [rows][Cin][2] -- and (sum g, sum g * xhat2) to part2 for
 * a second BatchNorm fed by the same gradient (downsample branch; may be NULL).  x1 / x2: the BatchNorm inputs
 * [B][H][W][Cin]; saved1 / saved2: their [4][Cin] blocks {mean, rstd, scale, shift}.  rows =
 * scouter_conv2d_dgrad_bn_partial_rows(...) (fp32 / bf16-input kernels: ceil(B*H*W / 64) for tile 2, / 128 otherwise;
 * plane kernels: / 128, 128, 128, 64, 256, 256 for tile 0..5, 4 * ceil(B*H*W / 256) for tile 6).  scouter_bn_bwd_f32(ext_partial = part, ext_rows = rows) then
 * runs without its own reduction pass.  part1 == NULL: exactly scouter_conv2d_dgrad_f32.
 * tile_hint 5 (round 5; csrc/conv_pw_persist_x3.h): the PERSISTENT kernel on the bf16 matrix cores (three-way operand split:
 * fp32-grade products, another summation order) -- 1x1 / stride 1 / groups 1 with GEMM-K of 64 / 128 / 256 and 64-multiples of
 * output columns: the input gradient WITH the fused epilogue (one partial row per workgroup row:
 * scouter_conv2d_dgrad_bn_partial_rows(..., 5)), and the forward without bias / addend / ReLU
 * (scouter_conv2d_fwd_bn_partial_rows(..., 5)); named where it does not apply: SC_ERR_UNSUPPORTED, never re-routed. */
int scouter_conv2d_dgrad_bn_partial_rows(int B, int H, int W, int Cin, int Cout, int kh, int kw, int stride, int pad,
                                         int groups, int tile_hint);
int scouter_conv2d_dgrad_bnbwd_f32(const float* dy, const float* w, const float* addend, float* dx, int B, int H, int W,
                                   int Cin, int Cout, int kh, int kw, int stride, int pad, int groups, int tile_hint,
                                   const void* relu_mask, const float* x1, const float* saved1, double* part1,
                                   const float* x2, const float* saved2, double* part2, void* stream);
/* ---- bf16 matrix inputs, fp32 accumulation (mixed-precision mode of BASELINE configs[4]): same tensors (fp32 in HBM),
 * same semantics and fused epilogues as the fp32 entry points; operands are rounded to bf16 (RNE) on their way into
 * LDS and multiplied on v_mfma_f32_32x32x16_bf16.  The forward takes the weights pre-transposed to bf16
 * [kh*kw][Cout][Cin/groups] (scouter_conv2d_weight_bf16t, 2*kh*kw*Cin/groups*Cout bytes); dgrad reads the fp32 HWIO
 * weights directly (stride 1 only: strided input gradients stay on the fp32 kernel).  wgrad_bf16 covers same-size
 * stride-1 convolutions with per-group channels that are multiples of 32 (32-channel groups on ragged 64-wide tiles) and
 * returns SC_ERR_UNSUPPORTED otherwise (callers then use scouter_conv2d_wgrad_f32); it shares that function's workspace.
 *
 * ACTIVATION STORAGE (`*_io` entry points, round 4): under --precision bf16 the widest tensors of a bottleneck -- the conv3 /
 * downsample-convolution outputs and the block outputs (timm/models/resnest.py:128-143: `out = self.bn3(self.conv3(out))`,
 * `out += residual`, `out = self.act3(out)`) -- may be STORED as bf16.  The typed entry points take untyped pointers plus
 * an `io` bit set: SCOUTER_IO_X_BF16 (1) the main input, SCOUTER_IO_Y_BF16 (2) the output, SCOUTER_IO_R_BF16 (4) the
 * residual; values are widened on load and rounded RNE on store, all arithmetic (and every gradient tensor) stays fp32;
 * a bf16-stored convolution input holds exactly the values the kernel rounds an fp32 input to, so the product is the
 * same bits.  io = 0 is the fp32 entry point. */
#define SCOUTER_IO_X_BF16 1
#define SCOUTER_IO_Y_BF16 2
#define SCOUTER_IO_R_BF16 4
int scouter_conv2d_weight_bf16t(const float* w, void* wt, int kh, int kw, int Cin, int Cout, int groups, void* stream);
int scouter_conv2d_fwd_bf16(const float* x, const void* wt_bf16, const float* bias, const float* addend, float* y,
                            double* bn_partial, int B, int H, int W, int Cin, int Cout, int kh, int kw, int stride,
                            int pad, int groups, int relu, int tile_hint, void* stream);
int scouter_conv2d_fwd_bf16_io(const void* x, const void* wt_bf16, const float* bias, const float* addend, void* y,
                               double* bn_partial, int B, int H, int W, int Cin, int Cout, int kh, int kw, int stride,
                               int pad, int groups, int relu, int tile_hint, int io, void* stream);
int scouter_conv2d_dgrad_bf16(const float* dy, const float* w, const float* addend, float* dx, int B, int H, int W,
                              int Cin, int Cout, int kh, int kw, int stride, int pad, int groups, int tile_hint,
                              void* stream);
int scouter_conv2d_dgrad_bnbwd_bf16(const float* dy, const float* w, const float* addend, float* dx, int B, int H, int W,
                                    int Cin, int Cout, int kh, int kw, int stride, int pad, int groups, int tile_hint,
                                    const void* relu_mask, const float* x1, const float* saved1, double* part1,
                                    const float* x2, const float* saved2, double* part2, void* stream);
/* io bits of the typed input gradient: 1 -- x1 is stored as bf16, 2 -- x2 is (the BatchNorm inputs the fused epilogue
 * reads), 4 -- the addend is, 8 -- dy is (the values the kernel rounds an fp32 dy to: same result), 16 -- dx is */
#define SCOUTER_DGRAD_IO_X1 1
#define SCOUTER_DGRAD_IO_X2 2
#define SCOUTER_DGRAD_IO_ADDEND 4
#define SCOUTER_DGRAD_IO_DY 8
#define SCOUTER_DGRAD_IO_DX 16
int scouter_conv2d_dgrad_bnbwd_bf16_io(const void* dy, const float* w, const void* addend, void* dx, int B, int H,
                                       int W, int Cin, int Cout, int kh, int kw, int stride, int pad, int groups,
                                       int tile_hint, const void* relu_mask, const void* x1, const float* saved1,
                                       double* part1, const void* x2, const float* saved2, double* part2, int io,
                                       void* stream);
/* tile_hint 4 of the typed FORWARD (round 5): the persistent pointwise kernel (csrc/conv_pw_persist_bf16.h pwb_fwd_kernel) --
 * 1x1 / stride 1 / groups 1, 64 / 128 / 256 / 512 input channels STORED as bf16 (SCOUTER_IO_X_BF16), 128-multiples of output
 * channels, no bias / addend / ReLU; y bf16 or fp32; bn_partial rows = scouter_conv2d_fwd_bn_partial_rows_bf16(..., 4)
 * (tile_hint 0-3: as scouter_conv2d_fwd_bn_partial_rows).  Named where it does not apply: SC_ERR_UNSUPPORTED. */
int scouter_conv2d_fwd_bn_partial_rows_bf16(int B, int H, int W, int Cin, int Cout, int kh, int kw, int stride, int pad,
                                            int groups, int tile_hint);
/* tile_hint 4 of the typed input gradient (round 5): the PERSISTENT pointwise kernel (csrc/conv_pw_persist_bf16.h) -- 1x1 /
 * stride 1 / groups 1, Cout of 64 / 128 / 256 / 512, 128-multiples of Cin, the fused BatchNorm-backward epilogue present
 * (part1 != NULL) and EVERY tensor stored as bf16 (io = DY | DX | X1 [| X2] [| ADDEND]); anything else named with tile 4 is
 * SC_ERR_UNSUPPORTED, never re-routed.  WITHOUT the fused epilogue (part1 == NULL) tile 4 is the plain persistent kernel:
 * Cout of 64 ... 1024, 64-multiples of Cin, dy stored as bf16 (DY), dx fp32, optional addend (fp32 or bf16).
 * The fused kernel writes ONE partial row per workgroup row: rows =
 * scouter_conv2d_dgrad_bn_partial_rows_bf16(..., 4, part2 != NULL) (tile_hint 0-3: the rows of the bf16-input tiles, as
 * scouter_conv2d_dgrad_bn_partial_rows). */
int scouter_conv2d_dgrad_bn_partial_rows_bf16(int B, int H, int W, int Cin, int Cout, int kh, int kw, int stride, int pad,
                                              int groups, int tile_hint, int two_batchnorms);
int scouter_conv2d_wgrad_bf16(const float* x, const float* dy, float* dw, int B, int H, int W, int Cin, int Cout, int kh,
                              int kw, int stride, int pad, int groups, int plan_hint, void* ws, size_t ws_bytes,
                              void* stream);
/* io: SCOUTER_IO_X_BF16 -- x is stored as bf16, SCOUTER_IO_R_BF16 -- dy is.  plan_hint < 0 (the library's own plan) with BOTH
 * operands stored as bf16 on a 3x3 / stride 1 / pad 1 layer with 32 input channels per group and rows of at most 112 pixels: the
 * tap-fused kernel (every x row fetched once per workgroup, not once per tap; csrc/conv_wgrad_taps_bf16.h; SCOUTER_BWT=0: off).
 * Same workspace bound (scouter_conv2d_wgrad_workspace_bytes with the same plan_hint) and deterministic slab sum. */
int scouter_conv2d_wgrad_bf16_io(const void* x, const void* dy, float* dw, int B, int H, int W, int Cin, int Cout,
                                 int kh, int kw, int stride, int pad, int groups, int plan_hint, void* ws,
                                 size_t ws_bytes, int io, void* stream);
/* plan_hint: -1 = built-in plan; otherwise bits 0-1 = block budget {512,1024,2048,4096} (sets the split-K count),
 * bit 4 / bit 5 = halve the ci / co tile edge.  Every plan is deterministic; different plans sum the pixels in a
 * different order (results differ in the last bits), so a caller that autotunes keeps its choice for the whole run. */
size_t scouter_conv2d_wgrad_workspace_bytes(int B, int H, int W, int Cin, int Cout, int kh, int kw, int stride, int pad,
                                            int groups, int plan_hint);
int scouter_conv2d_wgrad_f32(const float* x, const float* dy, float* dw, int B, int H, int W, int Cin, int Cout, int kh,
                             int kw, int stride, int pad, int groups, int plan_hint, void* ws, size_t ws_bytes,
                             void* stream);
/* ---- ROUTE QUERIES: what a convolution entry point answers to a shape, asked without calling it.  Each returns 1 or 0 and is
 * a pure function of its integer arguments -- no HIP call, no routing switch, no error text -- so it can be called before a
 * device exists and on a machine without one.  Each is defined next to its entry point and evaluates the SAME host predicate
 * that entry point rejects through (csrc/conv_common.h): a wrapper that routes on a query cannot drift from the kernel.
 * *_tile_ok(shape, tile, epilogue[, io]): naming `tile` runs that tile's kernel for a call with this shape, epilogue and
 * storage.  Tiles that are HINTS answer 0 where the library runs another tile instead (SC_OK): tiles 0-3 of the fp32 /
 * bf16-input kernels and the register-split family, plane tiles 0-5, and fp32 tile 4 on a SHAPE it does not cover (its
 * partial rows come from the same choice: scouter_conv2d_*_bn_partial_rows).  Tiles that are REFUSED answer 0 exactly where
 * the call returns SC_ERR_UNSUPPORTED: fp32 tile 4 on a covered shape with an epilogue that is not its own (forward: bias /
 * addend / ReLU), fp32 tile 5, tile 4 of the typed kernels, tile 7 of the register-split family, plane tile 6.  Arguments no
 * tensor reaches (2^36 pixels, 2^20 channels) answer 0.  Shape arguments are those of the entry point (B, H, W: the INPUT map).
 * TWO LIMITS every pixel-walking kernel shares (csrc/conv_common.h sc_tap_mask_ok / sc_pixel_walk_ok), answered 0 here and
 * refused with SC_ERR_UNSUPPORTED by the entry points: a filter of more than 32 taps (kh * kw; the tap validity of a GEMM row
 * is one 32-bit word: fp32 / bf16-input / register-split / plane forward and input gradient), and more than 2^22 - 256 pixels
 * in one image of the GEMM-row map (the forward's OUTPUT map, the input gradient's and weight gradient's INPUT map; the fp32
 * pixel unflattening is exact below 2^22: all of the above and the weight-gradient kernels).  Pointwise layers on the kernels that
 * walk no pixels there (fp32 tiles 0-5, the register-split pointwise kernel, the pointwise weight gradients) have neither limit.
 * tests/test_conv_tiles_cpu.py proves the domain and asks every family's query on both sides of it.
 * epilogue: SCOUTER_EPI_* bits of the call; io: SCOUTER_IO_* (forward) / SCOUTER_DGRAD_IO_* (typed input gradient). */
#define SCOUTER_EPI_BIAS 1      /* bias != NULL */
#define SCOUTER_EPI_ADDEND 2    /* addend != NULL */
#define SCOUTER_EPI_RELU 4
#define SCOUTER_EPI_BN_STATS 8  /* forward: bn_partial != NULL */
#define SCOUTER_EPI_BN_BWD 16   /* input gradient: part1 != NULL (one fused BatchNorm backward) */
#define SCOUTER_EPI_BN_BWD2 32  /* part2 != NULL too */
int scouter_conv2d_fwd_tile_ok(int B, int H, int W, int Cin, int Cout, int kh, int kw, int stride, int pad, int groups,
                               int tile, int epilogue);
int scouter_conv2d_dgrad_tile_ok(int B, int H, int W, int Cin, int Cout, int kh, int kw, int stride, int pad, int groups,
                                 int tile, int epilogue);
/* resident_rows != 0 asks instead: with switch bhalo on, the resident-rows kernel (csrc/conv_halo_dgrad_bf16.h) runs BEHIND
 * `tile` (forward: tile 1 / 3 by the columns per group, x stored as bf16; input gradient: tile 3, dy stored as bf16) */
int scouter_conv2d_fwd_bf16_tile_ok(int B, int H, int W, int Cin, int Cout, int kh, int kw, int stride, int pad, int groups,
                                    int tile, int epilogue, int io, int resident_rows);
int scouter_conv2d_dgrad_bf16_tile_ok(int B, int H, int W, int Cin, int Cout, int kh, int kw, int stride, int pad,
                                      int groups, int tile, int epilogue, int io, int resident_rows);
/* tile < 0: the entry point takes this shape at all (its own choice of tile) */
int scouter_conv2d_fwd_x3_tile_ok(int B, int H, int W, int Cin, int Cout, int kh, int kw, int stride, int pad, int groups,
                                  int tile, int epilogue);
int scouter_conv2d_dgrad_x3_tile_ok(int B, int H, int W, int Cin, int Cout, int kh, int kw, int stride, int pad, int groups,
                                    int tile, int epilogue);
int scouter_conv2d_wgrad_x3_ok(int B, int H, int W, int Cin, int Cout);
/* the launch of scouter_conv2d_wgrad_x3 for plan_hint, by its own plan function.  field 0: CI_TILES, 1: CO_TILES (128-channel
 * tiles), 2: SPLITS (above 1: the slab sum runs), 3: PIX_PER_SPLIT.  -1 where scouter_conv2d_wgrad_x3_ok answers 0 */
long scouter_conv2d_wgrad_x3_plan(int B, int H, int W, int Cin, int Cout, int plan_hint, int field);
int scouter_conv2d_fwd_planes_tile_ok(int B, int H, int W, int Cin, int Cout, int kh, int kw, int stride, int pad, int groups,
                                      int nplanes, int tile, int epilogue, int io);
int scouter_conv2d_dgrad_planes_tile_ok(int B, int H, int W, int Cin, int Cout, int kh, int kw, int stride, int pad,
                                        int groups, int nplanes, int tile, int epilogue);
/* the plane weight gradient takes this shape with this plan (bit 6: the tap-fused plans) */
int scouter_conv2d_wgrad_planes_plan_ok(int B, int H, int W, int Cin, int Cout, int kh, int kw, int pad, int groups,
                                        int nplanes, int plan);
/* the launch of scouter_conv2d_wgrad_planes for plan_hint, by its own plan function.  field 0: BM, 1: BN (channel edges of the
 * block tile, 64 or 128), 2: SPLITS, 3: PIX_PER_SPLIT, 4: FUSED (1: the tap-fused kernel, 64 x 64 tiles that carry all nine taps).
 * -1 where scouter_conv2d_wgrad_planes_plan_ok answers 0 */
long scouter_conv2d_wgrad_planes_plan(int B, int H, int W, int Cin, int Cout, int kh, int kw, int pad, int groups,
                                      int nplanes, int plan_hint, int field);
/* rows of fused BatchNorm partials plane tile 0..6 writes for M GEMM rows */
int scouter_conv2d_planes_partial_rows(long M, int tile);
/* which weight-gradient kernels take this shape: F32 / BF16 -- the entry point does; TAPS / XWT -- scouter_conv2d_wgrad_f32's
 * own plan (plan_hint < 0) is the tap-fused fp32 kernel / behind switch xwt the register-split one; BWT -- with both operands
 * stored as bf16 and switch bwt on, scouter_conv2d_wgrad_bf16_io's own plan is the tap-fused one-plane kernel.  Otherwise the
 * own plan runs one workgroup per tap.  ROWS32 -- the layer shape XWT and BWT share (3x3 / stride 1 / pad 1, 32 input channels
 * per group, a map at most 112 wide and two rows high), without their map-size and byte guards. */
#define SCOUTER_WGRAD_F32 0
#define SCOUTER_WGRAD_BF16 1
#define SCOUTER_WGRAD_TAPS 2
#define SCOUTER_WGRAD_XWT 3
#define SCOUTER_WGRAD_BWT 4
#define SCOUTER_WGRAD_ROWS32 5
int scouter_conv2d_wgrad_kernel_ok(int B, int H, int W, int Cin, int Cout, int kh, int kw, int stride, int pad, int groups,
                                   int kernel);
/* the launch of a weight-gradient kernel of scouter_conv2d_wgrad_f32 / _bf16_io for this shape, one integer per call.
 * kernel = SCOUTER_WGRAD_F32 / SCOUTER_WGRAD_BF16: the per-tap kernel (one workgroup per tap) under plan_hint.  BM / BN -- the input /
 * output channel edge of the block tile; SPLITS -- split-K slabs (above 1: the slab sum runs); PIX_PER_SPLIT -- pixels of one
 * split (the last split holds the rest); MODE -- the addressing mode, 0 = general, 1 = same-size padded taps, 2 = pointwise.
 * With plan_hint < 0 the entry points run a tap-fused kernel instead where scouter_conv2d_wgrad_kernel_ok says TAPS / XWT / BWT;
 * kernel 0 / 1 describe the per-tap launch they fall back to.
 * kernel = SCOUTER_WGRAD_TAPS / SCOUTER_WGRAD_XWT / SCOUTER_WGRAD_BWT: that tap-fused launch (plan_hint is not read).  BM -- 32; BN --
 * the column tile, 32 or 64; SPLITS, PIX_PER_SPLIT as above; field 4 (CHUNK) -- the pixels a workgroup stages per turn, 32 for TAPS,
 * 64 for XWT and BWT.
 * Evaluated by the launchers' own plan and mode functions.  -1: scouter_conv2d_wgrad_kernel_ok answers 0 for this kernel (or an
 * unknown kernel / field). */
#define SCOUTER_WGRAD_PLAN_BM 0
#define SCOUTER_WGRAD_PLAN_BN 1
#define SCOUTER_WGRAD_PLAN_SPLITS 2
#define SCOUTER_WGRAD_PLAN_PIX_PER_SPLIT 3
#define SCOUTER_WGRAD_PLAN_MODE 4
#define SCOUTER_WGRAD_PLAN_CHUNK 4
long scouter_conv2d_wgrad_plan(int B, int H, int W, int Cin, int Cout, int kh, int kw, int stride, int pad, int groups,
                               int kernel, int plan_hint, int field);
/* stem (Cin < 32): im2col of the NCHW image into [M][Kpad] rows so the stem runs as a 1x1 conv on the same path */
int scouter_im2col_nchw_f32(const float* x, float* col, int B, int Cin, int H, int W, int k, int stride, int pad,
                            int Kpad, void* stream);
int scouter_pad_rows_f32(const float* w, float* wpad, long nvalid, long ntotal, void* stream);
/* stem input gradient, d output / d image (train.py --grad / --grad_min_level, captum_vis.py: `image.requires_grad_()` and the
 * attribution methods that read the gradient of the image; sloter/slot_model.py:23-24, timm/models/resnet.py stems):
 * dx NCHW [B][Cin][H][W] = conv_transpose(dy NHWC [B][Ho][Wo][Cout], w HWIO [k][k][Cin][Cout]).  Gather form, no atomics:
 * bit-identical run to run.  Cin < 32, stride 1 or 2, k <= 11, pad < k; the three stems of the project (7x7 / 2 / 3 with
 * Cin 3, 3x3 / 2 / 1 with Cin 1 or 3; Cout a multiple of 16) run on the tiled kernel, the rest on a generic one.  Anything
 * else, or a tensor past the 32-bit offset guards: SC_ERR_UNSUPPORTED, nothing is launched. */
int scouter_stem_dgrad_f32(const float* dy, const float* w, float* dx, int B, int Cin, int H, int W, int Cout, int k, int stride,
                           int pad, void* stream);

/* ---- Grad-CAM at the backbone's output (reference captum_vis.py: LayerGradCam(model, layer=model.layer4) with
 * relu_attributions=False; sloter/utils/grad_cam.py).  feat / dfeat NHWC fp32 [B][N = h*w][C], 16-byte aligned:
 * wbar[b][c] = (1/N) sum_p dfeat[b][p][c], out[b * out_stride + p] = sum_c wbar[b][c] * feat[b][p][c] (relu != 0: clamped at
 * 0) -- out is fp32 [B][N] written through a batch stride in elements, e.g. one column of a [B][K][N] tensor.  One workgroup
 * per image, the channel means in LDS, each input read once, one fixed summation order per element and no atomics:
 * bit-identical run to run.  Any N >= 1 and 1 <= C <= 8192.  A null or misaligned pointer, B, N or C below 1, or a batch
 * stride below N: SC_ERR_ARG; C above 8192 or an image past 32-bit offsets: SC_ERR_UNSUPPORTED; nothing is launched then. */
int scouter_gradcam_f32(const float* feat, const float* dfeat, float* out, int B, int N, int C, long out_stride, int relu,
                        void* stream);
/* The heat map the reference draws from an attribution (captum_vis.py:51-59, show_cam_on_image), for M maps in one launch:
 * cam fp32 [M][h][w] -> out uint8 [M][H][W].  Per map: bilinear resize to H x W (F.interpolate align_corners=False:
 * src = (dst + 0.5) * in / out - 0.5 clamped at 0, i0 = floor(src), i1 = min(i0 + 1, in - 1)), max(., 0), min-max scaling to
 * [0, 1], max(., min_level), min-max scaling again, uint8(255 * v) truncating.  A map that is constant at either scaling step
 * (where the reference divides 0 / 0) is all zeros.  One workgroup per map with the source in LDS (h * w <= 32768); the
 * resized float map is recomputed, never stored.  Up- and down-sampling. */
int scouter_cam_maps_u8(const float* cam, unsigned char* out, int M, int h, int w, int H, int W, float min_level,
                        void* stream);

/* ---- RISE (Petsiuk et al. 2018; reference torchcam_vis.py: torchray.attribution.rise): saliency from N random masks.
 * Mask n is a grid of bytes in {0, 1}, grids u8 [N][s][s], and a shift, shifts i32 [N][2] = (dy, dx).  With
 * cell = ceil(size / s) and U = (s + 1) * cell per axis, mask_n(y, x) is the bilinear upsampling of the grid to U_h x U_w
 * (F.interpolate align_corners=False, the convention of scouter_cam_maps_u8) read at (y + dy, x + dx), 0 <= dy < cell_h,
 * 0 <= dx < cell_w.  Both calls form it by the same expression and never store it; every index is clamped, so a shift outside
 * its range (the callers check it on the host) reads nothing outside the grid.  1 <= s <= 16 and s <= min(H, W), else
 * SC_ERR_ARG, like a null or misaligned pointer or a count below 1; nothing is launched then.
 * out fp32 [N][C][H][W] = image [C][H][W] * mask_n, the mask value formed once per pixel for all C channels; 16-byte accesses
 * when W is a multiple of 4 and image / out are 16-byte aligned, one pixel per thread otherwise.  Any N >= 1. */
int scouter_rise_mask_images_f32(const float* image, const unsigned char* grids, const int* shifts, float* out, int N, int C,
                                 int H, int W, int s, void* stream);
/* acc fp32 [K][H][W] += sum_n (scale * expf(logp[n][cols[k]])) * mask_n(y, x), logp fp32 [N][n_classes], cols i32 [K] in
 * [0, n_classes) (checked by the caller; clamped here).  Every output element belongs to one thread, which starts from the
 * value in acc and adds the N terms one fma at a time in n order: no atomics, no partial sums -- splitting the masks over
 * several calls at any point gives the bits of one call.  Any N >= 1 (staged through LDS in pieces), any K >= 1. */
int scouter_rise_accumulate_f32(const float* logp, const int* cols, const unsigned char* grids, const int* shifts, float* acc,
                                int N, int n_classes, int K, int H, int W, int s, float scale, void* stream);
/* The drawing steps of scouter_cam_maps_u8 without the resize, for maps of any size H * W < 2^31: maps fp32 [M][H][W] -> out
 * uint8 [M][H][W]; per map max(., 0), min-max scaling, max(., min_level), min-max scaling again, uint8(255 * v) truncating; a
 * map constant at either step is all zeros.  One workgroup per map, two passes over it.  The same bytes as
 * scouter_cam_maps_u8 with H x W = h x w. */
int scouter_heat_maps_u8(const float* maps, unsigned char* out, int M, int H, int W, float min_level, void* stream);

/* ---- Insertion / deletion scores of a saliency map (Petsiuk et al. 2018, section 4.1; the IAUC / DAUC columns of the SCOUTER
 * paper; csrc/causal.hip, tools/attribution.py causal_metrics).  For an image x [C][H][W], a class c and a map m [H][W]: the
 * pixels are ordered by saliency, most salient first, equal values by ascending flat index y * W + x, -0 equal to +0, a NaN
 * less salient than every number (NaNs among themselves by index); rank[p] in [0, HW) is the position of pixel p.  `step`
 * pixels change per point, a curve has n_points = ceil(HW / step) + 1 points and point j has the min(j * step, HW) first-ranked
 * pixels changed: DELETION = x with the changed pixels set to 0 in every channel, INSERTION = blur(x) with the changed pixels
 * taken from x.  p_j = exp(log_prob_j[c]); the score is the trapezoid area (p_0 / 2 + p_1 + ... + p_{n-1} + p_n / 2) / n with
 * n = n_points - 1.  Every call has one fixed order per output element and no atomics: bit-identical run to run.  A null or
 * misaligned (4-byte) pointer or a count below 1 is SC_ERR_ARG in every call; nothing is launched after an error.
 *
 * in fp32 [M][h][w] -> out fp32 [M][H][W], F.interpolate(mode = "bilinear", align_corners = False): the source coordinate of
 * scouter_cam_maps_u8 (src = (dst + 0.5) * in / out - 0.5 clamped at 0, i0 = floor(src), i1 = min(i0 + 1, in - 1)) and three
 * fmas for the blend; up- and down-sampling; h x w = H x W copies the map bit for bit.  M above 65535 or a map past 32-bit
 * offsets: SC_ERR_UNSUPPORTED. */
int scouter_resize_bilinear_f32(const float* in, float* out, int M, int h, int w, int H, int W, void* stream);
/* maps fp32 [M][HW] -> ranks i32 [M][HW], the rank of the definition above.  One workgroup per map: a stable least-significant-
 * digit radix sort (4-bit digits, 8 passes) of (key, index) pairs, every thread scattering a contiguous run from offsets
 * scanned in LDS -- the same bits for the same input.  The pairs ping-pong through `ws`, at least
 * scouter_saliency_ranks_workspace_bytes(M, HW) = 16 * M * HW bytes (less: SC_ERR_WORKSPACE).  1 <= HW <= 2^20; above:
 * SC_ERR_UNSUPPORTED. */
size_t scouter_saliency_ranks_workspace_bytes(int M, long HW);
int scouter_saliency_ranks_i32(const float* maps, int* ranks, int M, long HW, void* ws, size_t ws_bytes, void* stream);
/* x fp32 [C][H][W], taps fp32 [klen] on the device -> out fp32 [C][H][W]: the klen-tap filter along rows (into tmp fp32
 * [C][H][W], a buffer of the caller's that is neither x nor out), then along columns; zeros outside the image; per pass klen
 * fmas in tap order starting from 0, centre tap klen / 2.  Two launches.  klen even, below 1 or above 31, or tmp == x / out:
 * SC_ERR_ARG; C above 65535 or a plane past 32-bit offsets: SC_ERR_UNSUPPORTED. */
int scouter_separable_filter_f32(const float* x, const float* taps, float* tmp, float* out, int C, int H, int W, int klen,
                                 void* stream);
/* A chunk of the edit stream of ONE image: image / blurred fp32 [C][H][W], ranks i32 [K][HW] -> out fp32 [n][C][H][W].  Stream
 * index g = first + i, 0 <= i < n, decodes as k = g / (2 * n_points), mode = (g / n_points) % 2 (0 deletion, 1 insertion),
 * j = g % n_points; out[i] is that point: a select by ranks[k][p] < j * step, made once per pixel for all C channels, so every
 * value is an exact copy (or 0).  A chunk may start and end anywhere in [0, 2 * K * n_points).  16-byte accesses when W is a
 * multiple of 4 and all four pointers are 16-byte aligned, one pixel per thread otherwise.  n_points < 2, step < 1, n_points
 * other than ceil(HW / step) + 1, or a chunk outside the stream: SC_ERR_ARG; an image past 32-bit offsets: SC_ERR_UNSUPPORTED. */
int scouter_causal_step_images_f32(const float* image, const float* blurred, const int* ranks, float* out, long first, int n,
                                   int K, int n_points, int step, int C, int H, int W, void* stream);
/* curve_flat[first + i] = expf(logp[i][cols[(first + i) / (2 * n_points)]]) for the same chunk: logp fp32 [n][n_classes], cols
 * i32 [K] in [0, n_classes) (checked by the caller; clamped here), curve_flat fp32 [K][2][n_points].  n_points < 2, n_classes
 * below 1 or a chunk outside the stream: SC_ERR_ARG. */
int scouter_causal_curve_f32(const float* logp, const int* cols, float* curve_flat, long first, int n, int K, int n_points,
                             int n_classes, void* stream);
/* curves fp32 [R][n_points] -> scores fp32 [R], the trapezoid area above: one thread per curve adds the points in j order, the
 * two ends halved, and divides by n_points - 1.  n_points < 2: SC_ERR_ARG; R above 65535 * 256: SC_ERR_UNSUPPORTED. */
int scouter_causal_auc_f32(const float* curves, float* scores, long R, int n_points, void* stream);

/* ---- The Score-CAM family: Score-CAM (Wang et al., CVPR-W 2020), SS-CAM (Wang et al. 2020) and IS-CAM (Naidu et al. 2020), the
 * gradient-free CAMs of the reference's torchcam_vis.py (csrc/scorecam.hip, tools/attribution.py scorecam / sscam / iscam).  For
 * ONE image's backbone output feat NHWC fp32 [h][w][C] and channel c:
 * U_c = the bilinear resize of feat[:, :, c] to H x W (F.interpolate align_corners=False, the source coordinate and the three
 * fmas of scouter_resize_bilinear_f32), lo_c / hi_c = the minimum / maximum of the fp32 values U_c(y, x) over the H * W pixels
 * (NOT the extrema of the h * w source values), span_c = hi_c - lo_c.  The channel is LIVE when span_c > 0 and its mask is
 * mask_c(y, x) = (U_c(y, x) - lo_c) / span_c -- one subtraction, then one correctly rounded division -- which attains exactly
 * 0 and exactly 1; otherwise (a constant channel, or a NaN / infinity in its range) it is DEAD: its mask is 0 everywhere and its
 * weight 0.  U and the mask are formed by the same inlined expressions wherever they are needed and never stored; every index is
 * clamped, so no feature value moves an address.  A channel's h * w source values live in LDS: h * w <= 1024, above that (or
 * features past 32-bit offsets) SC_ERR_UNSUPPORTED.  A null or misaligned (4-byte) pointer or a count below 1 is SC_ERR_ARG;
 * nothing is launched after an error.
 *
 * Every channel's mask goes through the model n_samples = N times (Score-CAM: N = 1, no noise, no ramp); the N * C rows of an
 * image form ONE flat stream, row r = sample j = r / C, channel c = r % C, and a call takes n <= C consecutive rows from
 * first_row, which may straddle a sample boundary but never hold a channel twice.  One fixed order per output element and no
 * atomics: bit-identical run to run and for any split of the stream into chunks.
 *
 * ranges fp32 [C][2] = (lo_c, hi_c) for every channel, one launch: a workgroup reads 8 channels for all positions coalesced along
 * C into LDS, each wave walks the H * W pixels of one channel and ends in a butterfly min / max. */
int scouter_scorecam_ranges_f32(const float* feat, float* ranges, int h, int w, int C, int H, int W, void* stream);
/* out fp32 [n][Cin][H][W], row first_row + i: out[i][ch][y][x] = image[ch][y][x] * g, g = a + nz, a = scale_j * mask_c(y, x),
 * nz = sigma * z(seed, j, e), e = ch * H * W + y * W + x -- two products, then ONE sum fused with neither, then the product with
 * the image, all fp32 with no contraction.  scale_j = 1, or with ramp != 0 (IS-CAM) (float)((double)(j + 1) * (j + 2) / (2 * N)),
 * the partial sum of (t + 1) / N over t <= j.  z is the standard normal scouter_noise_images_f32 gives for (seed, sample j,
 * element e): it depends on the sample and the image element, not on the channel c.  sigma == 0: no noise is formed and
 * out = image * a, which with ramp == 0 is image * mask_c exactly (Score-CAM's masked image).  The mask value is formed once
 * per pixel for all Cin channels; a dead channel writes zeros, noise or not.  16-byte accesses when W is a multiple of 4 and
 * image / out are 16-byte aligned, one pixel per thread otherwise; both give the same bits.  n < 1, n > C, n_samples < 1, rows
 * outside [0, N * C), sigma negative, NaN or infinite: SC_ERR_ARG; N * C of 2^31 or more: SC_ERR_UNSUPPORTED. */
int scouter_sscam_mask_images_f32(const float* image, const float* feat, const float* ranges, float* out, int first_row, int n,
                                  int n_samples, int ramp, float sigma, int seed_lo, int seed_hi, int Cin, int H, int W, int h,
                                  int w, int C, void* stream);
/* wsum fp64 [C][K], wsum[c][k] += (double)expf(logp[i][cols[k]]) with c = (first_row + i) % C, for logp fp32 [n][n_classes] (the
 * model's output for the n rows scouter_sscam_mask_images_f32 wrote at the same first_row) and cols i32 [K] in [0, n_classes)
 * (checked by the caller, who holds them on the host; clamped here).  One thread per (i, k) and n <= C (above: SC_ERR_ARG), so
 * no two threads meet: the sum of a (channel, class) runs in stream order whatever the chunking.  wsum is 8-byte aligned. */
int scouter_sscam_weights_f64(const float* logp, const int* cols, double* wsum, int first_row, int n, int n_classes, int K, int C,
                              void* stream);
/* out fp32 [K][h][w] = sum_c live_c * (float)(wsum[c][k] * norm) * feat[p][c]: the weight is rounded from fp64 ONCE (after one
 * sample and with norm = 1 it is expf(logp) exactly), then every output element belongs to one thread, which starts from 0 and
 * adds one fma per live channel in ascending order (a dead channel is skipped): no atomics, no partial sums.  The weights are
 * staged through LDS in pieces: any C, any K >= 1.  out is overwritten.  norm must be finite. */
int scouter_sscam_contract_f32(const double* wsum, const float* feat, const float* ranges, float* out, double norm, int K, int h,
                               int w, int C, void* stream);

/* ---- Path and noise batches for the gradient methods that need many gradients per image: Integrated Gradients (Sundararajan
 * et al., ICML 2017) and SmoothGrad / VarGrad (Smilkov et al. 2017; Adebayo et al. 2018), captum's IntegratedGradients and
 * NoiseTunnel of the reference's captum_vis.py (csrc/pathgrad.hip, tools/attribution.py integrated_gradients / smoothgrad).
 * E = C * H * W is the flat element count of ONE image and e the flat index; every image is dense.  The images of a chunk are
 * written into a batch buffer, the model's own forward and backward turn them into gradients, and the gradients are summed in
 * fp64.  One thread owns an output element (or four consecutive ones), one fixed order per element and no atomics:
 * bit-identical run to run.  Each call has a 16-byte form (E, or H * W, a multiple of 4 and every pointer 16-byte aligned) and a
 * one-element form that give the same bits.  A null or misaligned pointer (fp32: 4 bytes, fp64: 8), a size below 1 or a range
 * outside [0, N) is SC_ERR_ARG; n * E (or E, or M * C * HW) of 2^31 or more is SC_ERR_UNSUPPORTED; nothing is launched after an
 * error.
 *
 * out fp32 [n][E], out[j][e] = fmaf(alphas[first + j], image[e] - base[e], base[e]): one fp32 subtraction, formed once per
 * element and reused for the thread's values of j, then one fma.  alphas fp32 [N], 0 <= first and first + n <= N.  base may be
 * null: all zeros.  A dense leading slice of a longer out is fine. */
int scouter_path_images_f32(const float* image, const float* base, const float* alphas, float* out, int first, int n, int N,
                            long E, void* stream);
/* out fp32 [n][E], out[j][e] = fmaf(sigma, z(seed, first + j, e), image[e]), sigma >= 0 and finite.  z is standard normal:
 * Philox4x32-10 (multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85) with the key (seed_lo, seed_hi)
 * -- the two ints are taken as 32-bit patterns -- and the counter (e / 4, first + j, 0, 0); its words r0 .. r3 serve the elements
 * 4q .. 4q + 3: u_i = (float)(2 * (r_i >> 9) + 1) * 2^-24 (exact, inside (0, 1)), (z0, z1) = rad(u0) * (cosf, sinf)(
 * 6.283185307179586f * u1), (z2, z3) the same from (u2, u3), rad(u) = sqrtf(-2 * logf(u)), with the accurate device functions.
 * A partial last group (E not a multiple of 4) uses its leading words.  The value of an element depends on (seed, first + j, e)
 * alone: not on the chunking and not on the form that wrote it. */
int scouter_noise_images_f32(const float* image, float* out, float sigma, int seed_lo, int seed_hi, int first, int n, long E,
                             void* stream);
/* acc fp64 [E] += sum_j w_j * g[j][e] and, when acc_sq (fp64 [E]) is not null, acc_sq[e] += sum_j w_j * g[j][e]^2, for grads
 * fp32 [n][E] and w_j = weights[first + j] (fp32 [N]; null: every w_j is 1), 0 <= first and first + n <= N.  The sums run in
 * ascending j in fp64 and start from the values in acc / acc_sq; w_j * g is exact, (w_j * g) * g takes one rounding inside the
 * fma that adds it.  No partial sums: splitting the N terms over calls at any point gives the bits of one call. */
int scouter_grad_accumulate_f64(const float* grads, const float* weights, double* acc, double* acc_sq, int first, int n, int N,
                                long E, void* stream);
/* out fp32 [E] by mode -- SCOUTER_ATTR_IG 0: (float)((double)(image[e] - base[e]) * acc[e]), the fp32 difference
 * scouter_path_images_f32 forms (base null: zeros); SCOUTER_ATTR_MEAN 1: (float)(acc[e] * inv_n); SCOUTER_ATTR_MEAN_SQ 2:
 * (float)(acc_sq[e] * inv_n); SCOUTER_ATTR_VAR 3: (float)(acc_sq[e] * inv_n - (acc[e] * inv_n)^2), the biased variance of
 * captum's vargrad (one fma).  Only the inputs a mode reads must be non-null; another mode is SC_ERR_ARG.  When total (fp64 [1])
 * is not null it receives sum_e (double)out[e]: one partial sum per workgroup into ws (at least
 * scouter_attr_finish_workspace_bytes() bytes, else SC_ERR_WORKSPACE), added by a second launch in a fixed order -- the grid
 * depends on E alone, so two calls give the same bits.  ws may be null when total is. */
#define SCOUTER_ATTR_IG 0
#define SCOUTER_ATTR_MEAN 1
#define SCOUTER_ATTR_MEAN_SQ 2
#define SCOUTER_ATTR_VAR 3
size_t scouter_attr_finish_workspace_bytes(void);
int scouter_attr_finish_f32(int mode, const double* acc, const double* acc_sq, const float* image, const float* base,
                            double inv_n, float* out, double* total, long E, void* ws, size_t ws_bytes, void* stream);
/* out fp32 [M][HW], out[m][p] = (float)(sum_c v(x[m][c][p]) / C) for x fp32 [M][C][HW]: v the identity, or fabs when `absolute`
 * is not 0; the sum runs over ascending c in fp64 and is divided by C in fp64. */
int scouter_channel_mean_f32(const float* x, float* out, long M, int C, long HW, int absolute, void* stream);

/* ---- Grad-CAM++ (Chattopadhay et al., WACV 2018) and Smooth Grad-CAM++ (Omeiza et al. 2019) at the backbone's output: torchcam's
 * GradCAMpp / SmoothGradCAMpp of the reference's torchcam_vis.py (torchcam/cams/gradcam.py:104-272; csrc/gradcampp.hip,
 * tools/attribution.py gradcampp / smooth_gradcampp).  feat = A and dfeat = g NHWC fp32 [B][N = h*w][C], 16-byte aligned.  Per
 * image: S[c] = sum_p g[p][c]^3 * A[p][c], den[p][c] = 2 * g[p][c]^2 + S[c], alpha[p][c] = g[p][c]^2 / den[p][c] and 0 where
 * den == 0 (the reference divides 0 / 0 there and later replaces the NaN product by 1), w[c] = sum_p alpha[p][c] * max(g[p][c], 0),
 * out[b * out_stride + p] = sum_c w[c] * A[p][c] (relu != 0: clamped at 0) -- out is fp32 [B][N] written through a batch stride
 * in elements, as in scouter_gradcam_f32.  All in fp32.  One workgroup per image and three passes: S and w by column (dfeat is
 * read twice, feat twice), then one wave per position; S and w live in LDS.  One fixed summation order per element and no
 * atomics: bit-identical run to run.  Any N >= 1 and 1 <= C <= 8192.  A null or misaligned pointer, B, N or C below 1, or a batch
 * stride below N: SC_ERR_ARG; C above 8192 or an image past 32-bit offsets: SC_ERR_UNSUPPORTED; nothing is launched then. */
int scouter_gradcampp_f32(const float* feat, const float* dfeat, float* out, int B, int N, int C, long out_stride, int relu,
                          void* stream);
/* acc2 fp64 [E] += sum_j g[j][e]^2 and acc3 fp64 [E] += sum_j g[j][e]^3 for grads fp32 [n][E]: the sums run in ascending j in
 * fp64 and start from the values in acc2 / acc3; g^2 is exact, g^2 * g takes one rounding inside the fma that adds it.  No
 * partial sums: splitting the terms over calls at any point gives the bits of one call (the contract of
 * scouter_grad_accumulate_f64).  A null or misaligned pointer (fp32: 4 bytes, fp64: 8), acc2 == acc3, n or E below 1:
 * SC_ERR_ARG; n * E of 2^31 or more: SC_ERR_UNSUPPORTED. */
int scouter_grad_powers_accumulate(const float* grads, double* acc2, double* acc3, int n, long E, void* stream);
/* Smooth Grad-CAM++ from the sums of scouter_grad_powers_accumulate over the n_samples noisy copies of an image: q = acc2 /
 * n_samples and t = acc3 / n_samples (fp64 [B][N][C]; 16-byte aligned when C is a multiple of 4, like glast), S[c] = sum_p t[p][c] * A[p][c], alpha = q / (2 * q + S[c])
 * and 0 where the denominator is 0, w[c] = sum_p alpha[p][c] * max(glast[p][c], 0) -- glast fp32 [B][N][C] is the gradient of the
 * LAST sample, as the reference has it (gradcam.py:272) -- all in fp64, w rounded to fp32 once; out as above from the clean
 * image's features feat, in fp32.  The same kernel plan, argument rules and errors as scouter_gradcampp_f32; n_samples below 1:
 * SC_ERR_ARG. */
int scouter_gradcampp_smooth_f32(const float* feat, const double* acc2, const double* acc3, const float* glast, float* out,
                                 int n_samples, int B, int N, int C, long out_stride, int relu, void* stream);

/* ---- CAM of the FC baseline (Zhou et al., CVPR 2016; torchcam's CAM(model, 'layer4', 'fc'), the first extractor of the
 * reference's torchcam_vis.py: CAM._get_weights followed by compute_cams; csrc/fccam.hip, tools/attribution.py fccam).
 * feat NHWC fp32 [B][N = h*w][C], w fp32 [n_classes][C] (the fc weight as it is stored), both 16-byte aligned; cols i32 on the
 * device -- per_image == 0: [K] columns shared by all images; per_image != 0: [B], each image its own class, K = 1 -- in
 * [0, n_classes) (checked by the caller, clamped here); out fp32 [B][K][N]:
 * out[b][k][p] = sum_c w[col][c] * feat[b][p][c] (relu != 0: clamped at 0).  No bias and no 1 / N.  One workgroup per image and
 * tile of 8 positions, the tile staged in LDS 2048 channels at a time and walked by the K classes: the features cross HBM once
 * (every class re-reads the tile from LDS, a wave per class: for large K the LDS traffic sets the time, not HBM).
 * fp32, one fixed summation order per element that depends on C alone and no atomics: two calls, a per-image call and the
 * matching columns of an all-classes call, and an image at another batch position give the same bits.  Any N, C, K >= 1.  A
 * null or misaligned pointer, a count below 1, or per_image with K != 1: SC_ERR_ARG; a tensor past 32-bit offsets:
 * SC_ERR_UNSUPPORTED; nothing is launched then. */
int scouter_cam_fc_f32(const float* feat, const float* w, const int* cols, float* out, int B, int N, int C, int n_classes, int K,
                       int per_image, int relu, void* stream);

/* ---- Localisation scores of uint8 maps: the area size and the precision of the SCOUTER paper's comparison and the pointing
 * game (Zhang et al., ECCV 2016) from one pass (csrc/localization.hip, tools/attribution.py localization).  maps u8
 * [B][K][H][W] (what scouter_cam_maps_u8 / scouter_heat_maps_u8 write), boxes i32 [B][max_boxes][4] = (x0, y0, x1, y1), half-open
 * pixel ranges of the map's own grid, n_boxes i32 [B] in [0, max_boxes] (clamped); boxes and n_boxes may both be null: no image
 * has a box.  A pixel is inside when it lies in any of its image's first n_boxes[b] boxes (a union: a pixel under two boxes
 * counts once); boxes are clipped to the map and a box with x1 <= x0 or y1 <= y0 holds nothing.  sums i64 [B][K][4] =
 * (S, the sum of the map's bytes; S_in, the sum of the bytes inside; arg, the flat index y * W + x of the largest byte, the
 * smallest index among equals; hit, 1 if that pixel is inside, else 0).  Integers only, so every value is exact.  One
 * workgroup per map, no atomics.  1 <= max_boxes <= 32 and H * W < 2^31, else SC_ERR_UNSUPPORTED. */
int scouter_map_localization_u8(const unsigned char* maps, const int* boxes, const int* n_boxes, long* sums, int B, int K, int H,
                                int W, int max_boxes, void* stream);
/* The bytes SlotAttention.vis_maps draws (reference slot_attention.py:74) for every image of a batch: maps fp32 [M][G][N] ->
 * out u8 [M][G][N]; per group m, lo and hi over all G * N values, span = hi - lo,
 * out = (unsigned char)((v - lo) / span * 255.f) -- these fp32 operations in this order, truncating; span == 0: all zeros.
 * One workgroup per group.  G * N < 2^31. */
int scouter_group_maps_u8(const float* maps, unsigned char* out, int M, int G, long N, void* stream);

/* ---- Infidelity and max-sensitivity of an explanation (Yeh et al., NeurIPS 2019, "On the (In)fidelity and Sensitivity of
 * Explanations"; captum's infidelity and sensitivity_max, two columns of the SCOUTER paper's comparison of explanations;
 * csrc/fidelity.hip, tools/attribution.py infidelity / sensitivity_max).  No reference program computes either here: the
 * definitions below are the specification.  One image x of E = C * H * W elements, e the flat index, HW = H * W; a stream of N
 * perturbed copies of x goes through the model (or the explanation method) in chunks [first, first + n), every forward with the
 * clean image in row 0, and the chunks fill per-sample fp64 arrays [K][N].  One fixed order per output element and no atomics:
 * bit-identical run to run, and no value depends on the chunking.  A null or misaligned pointer (fp32 / i32: 4 bytes, fp64: 8),
 * a size below 1 or a chunk outside [0, N) is SC_ERR_ARG; sizes past 32-bit offsets or the grid are SC_ERR_UNSUPPORTED; nothing
 * is launched after an error.
 *
 * INFIDELITY of K attributions a_k for the class columns c_k: z_j[e] = the standard normal of scouter_noise_images_f32 (the key
 * (seed_lo, seed_hi), the counter (e / 4, j, 0, 0)), the perturbed image x_j = fmaf(sigma, z_j[e], x[e]) written by that call, the
 * perturbation DEFINED as I_j[e] = -sigma * z_j[e] (the exact product of the two fp32 values: x - x_j up to the fma's rounding),
 * dot[k][j] = sum_e a_k[e] * I_j[e] in fp64, delta[k][j] = F(out[0][c_k]) - F(out[1 + i][c_k]) for the sample j in row 1 + i of a
 * forward (F the identity on the log-probabilities, or exp), and over ascending j in fp64
 *   raw[k] = (1 / N) sum_j (dot - delta)^2,  beta[k] = sum_j dot * delta / sum_j dot^2 (0 when the denominator is 0),
 *   normalized[k] = (1 / N) sum_j (beta * dot - delta)^2   (captum's normalize = True).
 *
 * dots fp64 [K][N], dots[k][first + j] = sum_e a_k[e] * I_{first + j}[e] for j < n.  attrs fp32 [K][A]: A == E is the FULL form
 * (a_k = attrs[k]), A < E with E % A == 0 is the MAP form, A = HW, a map that counts for every channel (a_k[e] = attrs[k][e % A]);
 * anything else is SC_ERR_ARG.  z is regenerated from Philox, no image buffer is read.  A thread owns groups of four elements
 * 4q .. 4q + 3 (ascending q); per group it loads a tile of 4 attributions once and, per sample of a tile of 4 samples, forms the four
 * p = -(double)sigma * (double)z and adds fma((double)a_k[e], p, .) in e order; then a butterfly over the wave, the waves of the
 * workgroup in order through LDS, and a second launch that adds the workgroups' partial sums in workgroup order.  The grid
 * along the elements is min(ceil(ceil(E / 4) / 256), 256) workgroups, a function of E alone.  16-byte loads when A is a multiple
 * of 4 and attrs is 16-byte aligned, one element per load otherwise: the same bits.  sigma >= 0 and finite (0: every dot is 0).
 * ws: at least scouter_perturb_dots_workspace_bytes(n, K, E) bytes, 8-byte aligned (less: SC_ERR_WORKSPACE). */
size_t scouter_perturb_dots_workspace_bytes(int n, int K, long E);
int scouter_perturb_dots_f64(const float* attrs, double* dots, float sigma, int seed_lo, int seed_hi, int first, int n, int N,
                             int K, long E, long A, void* ws, size_t ws_bytes, void* stream);
/* deltas fp64 [K][N], deltas[k][first + j] = F((double)out[0][cols[k]]) - F((double)out[1 + j][cols[k]]) for j < n: out fp32
 * [1 + n][n_classes] is ONE forward's output with the clean image in row 0, cols i32 [K] in [0, n_classes) (checked by the caller;
 * clamped here), of = SCOUTER_DELTA_LOG_PROB 0: F the identity, SCOUTER_DELTA_PROB 1: F = exp in fp64; another value is
 * SC_ERR_ARG. */
#define SCOUTER_DELTA_LOG_PROB 0
#define SCOUTER_DELTA_PROB 1
int scouter_output_deltas_f64(const float* out, const int* cols, double* deltas, int first, int n, int N, int K, int n_classes,
                              int of, void* stream);
/* One thread per row r < R of dots / deltas fp64 [R][N], the samples in ascending j, every product-and-add one fp64 fma:
 * raw[r] = sum_j (dot - delta)^2 / N, beta[r] = sum_j dot * delta / sum_j dot^2 (0 when sum_j dot^2 == 0),
 * normalized[r] = sum_j (fma(beta, dot, -delta))^2 / N.  raw, beta, normalized fp64 [R]. */
int scouter_infidelity_finish_f64(const double* dots, const double* deltas, double* raw, double* beta, double* normalized,
                                  long R, int N, void* stream);
/* MAX-SENSITIVITY of an explanation method: d_j[e] = 2 * u - 1 with u = (float)(2 * (r >> 9) + 1) * 2^-24 from the Philox word
 * r = word e % 4 of the counter (e / 4, j, 1, 0) under the same key -- the third counter word sets this stream apart from the
 * noise -- so d_j[e] = ((2 * (r >> 9) + 1) - 2^23) * 2^-23 exactly, never 0 and inside (-1, 1); x_j = fmaf(radius, d_j[e], x[e]);
 * the method explains [x, x_first, ...] as A fp32 [1 + n][K][M]; term[k][j] = sqrt(sum_m (A_j[k][m] - A_0[k][m])^2 / den_k) with
 * den_k = sum_m A_0[k][m]^2, or 1 when that sum is 0 (captum's choice for a zero explanation); score[k] = max_j term[k][j], NaN if
 * any term is NaN.
 *
 * out fp32 [n][E], out[j][e] = fmaf(radius, d_{first + j}[e], image[e]), radius >= 0 and finite: the twin of
 * scouter_noise_images_f32 with its forms, its refusals and its rule that an element's value depends on (seed, first + j, e) alone.
 * A thread writes a tile of 8 samples of its four elements; n above 65535 * 8: SC_ERR_UNSUPPORTED. */
int scouter_uniform_images_f32(const float* image, float* out, float radius, int seed_lo, int seed_hi, int first, int n, long E,
                               void* stream);
/* terms fp64 [K][N], terms[k][first + j] = the term above for j < n, from maps fp32 [1 + n][K][M] of ONE call of the method (den_k
 * comes from row 0 of the same call).  One workgroup of 256 threads per (j, k): a thread adds (A_j[m] - A_0[m])^2, the difference
 * formed in fp64, and A_0[m]^2, one fma each, for m = t, t + 256, ... in ascending m; then a butterfly over the wave and the waves
 * in order.  K above 65535: SC_ERR_UNSUPPORTED. */
int scouter_map_distances_f64(const float* maps, double* terms, int first, int n, int N, int K, long M, void* stream);
/* score fp64 [R], score[r] = max_j terms[r][j] over terms fp64 [R][N], one thread per row in ascending j; a NaN term makes the
 * score NaN. */
int scouter_sensitivity_finish_f64(const double* terms, double* score, long R, int N, void* stream);

/* ---- Extremal perturbation (Fong, Patrick, Vedaldi, ICCV 2019; torchray.attribution.extremal_perturbation, which the
 * reference's torchcam_vis.py runs after RISE; csrc/extremal.hip, tools/attribution.py extremal_perturbation): the mask side of
 * one step of the optimisation.  No reference program runs here: the definitions below are the specification.  n coarse masks
 * pmask fp32 [n][hm][wm] in [0, 1] on a grid of `step` pixels, hm = ceil(H / step), wm = ceil(W / step); full masks [n][H][W];
 * one image's blur pyramid P fp32 [L][C][H][W] (level L - 1 the image, level 0 the most blurred).  One launch each, no atomics,
 * every cross-thread sum in one fixed order: bit-identical run to run, and a mask's values do not depend on n.  A null or
 * misaligned (4 bytes) pointer, a size below 1, L < 2, a variant or flag outside {0, 1} is SC_ERR_ARG; sizes past 32-bit
 * offsets, n above 65535 or a kernel table above 16384 floats are SC_ERR_UNSUPPORTED; nothing is launched after an error.
 *
 * SMOOTH-MAX UPSAMPLING.  r = 1 + ceil(sigma / step), D = 2 r + 1, beta = 20.  Cell (i, j) has its centre at pixel coordinates
 * ((i + 0.5) step - 0.5, (j + 0.5) step - 0.5).  Pixel u = (y, x) sees the D * D cells c = (y / step + a, x / step + b), a, b in
 * [-r, r]: v_c = k_c * p_c with k_c = exp(-2 * max(|u - centre_c| / sigma - 0.5, 0)^2), v_c = 0 for a cell outside the grid;
 * out[u] = sum_c v_c * e_c / sum_c e_c, e_c = exp(beta * (v_c - vmax)), vmax = max_c v_c, the window in (a, b) order.  k depends on
 * (y % step, x % step, a, b) alone: a table of step^2 * D^2 floats per workgroup in LDS.  stats (may be NULL) fp32 [n][H * W][2]
 * receives (vmax, sum_c e_c) per pixel, what scouter_extremal_step_f32 reads. */
int scouter_extremal_mask_f32(const float* pmask, float* out, float* stats, int n, int H, int W, int step, float sigma,
                              void* stream);
/* THE BLEND.  m' = mask (variant 0, preserve) or 1 - mask (variant 1, delete), t = m' * (L - 1), k = min(floor(t), L - 2),
 * w = t - k: out[j][c][y][x] = fma(w, P[k + 1][c][q], (1 - w) * P[k][c][q]) with q = (y, x), or (y, W - 1 - x) when flip is set -- the
 * mirrored image.  Exact at the ends: w = 0 gives P[k], m' = 1 gives the image.  At an interior knot the right-hand piece is
 * used.  16-byte accesses when W is a multiple of 4 and every pointer is 16-byte aligned, one element otherwise: the same
 * bits.  out may be a leading slice of a longer buffer. */
int scouter_extremal_blend_f32(const float* pyramid, const float* mask, float* out, int n, int L, int C, int H, int W, int variant,
                               int flip, void* stream);
/* THE SEED of the backward and the reward: p_j = exp(logp[j][cols[j]]) for logp fp32 [n][n_out] and cols i32 [n] in [0, n_out)
 * (checked by the caller; clamped here); seed[j][cols[j]] = -p_j (variant 0: the loss is -p) or +p_j (variant 1), every other
 * entry of seed fp32 [n][n_out] is written 0; rewards fp32 [n_iters][n]: rewards[it][j] = p_j, 0 <= it < n_iters. */
int scouter_extremal_seed_f32(const float* logp, const int* cols, float* seed, float* rewards, int n, int n_out, int n_iters,
                              int it, int variant, void* stream);
/* THE MASK GRADIENT.  dmask[j][q] = fma(+-(L - 1), sum_c dx[j][c][q'] * (P[k + 1][c][q] - P[k][c][q]), c2 * (mask[j][q] - tau)), + for
 * variant 0 and - for variant 1, the sum one fma per channel in ascending c, k from mask[j][q] by the expression of the blend
 * (the same bits), q' = q mirrored in x when flip is set (dx fp32 [n][C][H][W] is the gradient of the loss at the image the blend
 * wrote), tau = 1 where ranks[j][q] < targets[j] and 0 elsewhere (ranks i32 [n][H * W] of scouter_saliency_ranks_i32 on the
 * mask, targets i32 [n] the number of pixels of each mask's area), c2 = (float)(2 * lam / (H * W)) formed in fp64: the gradient of
 * lam * mean_q (mask - tau)^2.  lam >= 0 and finite. */
int scouter_extremal_mask_grad_f32(const float* pyramid, const float* mask, const float* dx, const int* ranks, const int* targets,
                                   float* dmask, float lam, int n, int L, int C, int H, int W, int variant, int flip, void* stream);
/* THE STEP, in place.  Per cell c of mask j: g = sum_u dmask[j][u] * k_uc * w_uc * (1 + beta * (v_uc - mask[j][u])) over the at most
 * (D * step)^2 pixels u that see the cell, v_uc = k_uc * pmask[j][c], w_uc = exp(beta * (v_uc - vmax_u)) / den_u with (vmax_u, den_u)
 * from stats as scouter_extremal_mask_f32 wrote them for THIS pmask (g is then d sum_u dmask * out / d pmask[j][c]); mom = g
 * (first) or fma(momentum, mom, (1 - momentum) * g) -- SGD with dampening = momentum --; pmask = clamp(fma(-lr, mom, pmask), 0, 1).
 * One wave per cell: a lane adds the pixels lane, lane + 64, ... of the cell's window (row-major) by one fma each, then a
 * butterfly.  A cell's terms read its own pmask value and per-pixel arrays nothing here writes: no race. */
int scouter_extremal_step_f32(float* pmask, float* mom, const float* mask, const float* dmask, const float* stats, int n, int H,
                              int W, int step, float sigma, float lr, float momentum, int first, void* stream);

/* ---- Information-bottleneck attribution (Schulz, Sixt, Tombari, Landgraf, ICLR 2020; the reference's torchcam/IBA/pytorch.py,
 * attached to model.layer4 by torchcam_vis.py; csrc/iba.hip, tools/attribution.py information_bottleneck): the mask side of one
 * Adam step and the estimator of the feature distribution.  x, mean, std, active fp32 [h][w][C] (one image's features NHWC, the
 * fitted mean, std and 0 / 1 activity); alpha fp32 [K][h][w][C], one mask per class; rows j = k * S + s; N = h * w, E = N * C.
 * One launch each, no atomics, fixed summation orders: bit-identical run to run, and a class's values do not depend on K.
 * A null or misaligned (4 bytes; 8 for fp64) pointer, a size below 1, a window radius not below h and w, a flag outside {0, 1}
 * is SC_ERR_ARG; sigma above 3.25, h * w above 120, K above 65535 or sizes past 32-bit offsets are SC_ERR_UNSUPPORTED.
 *
 * SMOOTHING G: the depthwise window of side D = 2 * r + 1, r = round(2 * sigma) (to even at a tie), values
 * exp(-d^2 / (2 * sigma^2)) normalised to sum 1 (formed in fp64, rounded once), over (h, w) with reflection padding that does
 * not repeat the edge; sigma = 0: no smoothing.  lambda = G(sigmoid(alpha)), kappa = G(sigmoid(-alpha)) = 1 - lambda without the
 * cancellation.  sd = max(std, min_std), r = (x - mean) / sd.
 * NOISE: eps[j][e] is the stream of scouter_noise_images_f32: Philox4x32-10 under the key (seed_lo, seed_hi) and the counter
 * (e / 4, first + j, 0, 0), e = p * C + c, Box-Muller on the word pairs.  The caller passes first = t * (all rows of the image) +
 * the first row of this call.
 * SAMPLE: z_out[j] = active ? fma(lambda_k, x, kappa_k * fma(sd, eps[j], mean)) : 0, clamped at 0 when relu is set;
 * cap_out (may be NULL) fp32 [K][h][w][C] = active ? -0.5 * (1 + 2 * ln(kappa) - (r * lambda)^2 - kappa^2) : 0, in nats. */
int scouter_iba_sample_f32(const float* x, const float* mean, const float* std, const float* active, const float* alpha,
                           float* z_out, float* cap_out, int K, int S, int h, int w, int C, float sigma, float min_std, int seed_lo,
                           int seed_hi, int first, int relu, void* stream);
/* THE STEP, in place.  dz fp32 [K * S][h][w][C] = d loss / d z_out.  G_lambda[k] = active ? sum_s dz[k * S + s] * (x - fma(sd, eps, mean))
 * * [z > 0 if relu] + (beta / E) * (1 / kappa + r^2 * lambda - kappa) : 0, one fma per sample in ascending s, eps and z regenerated by
 * the expressions of the sample; G_alpha[k] = sigmoid(alpha) * sigmoid(-alpha) * G^T(G_lambda[k]), G^T the adjoint of the reflecting
 * window; then Adam as torch.optim.Adam (betas 0.9 / 0.999, eps 1e-8, no weight decay) at iteration t >= 0 on alpha, adam_m, adam_v
 * (zeros before t = 0): m = fma(0.9, m, 0.1 * g), v = fma(0.999, v, 0.001 * g * g), alpha -= lr / (1 - 0.9^(t + 1)) * m /
 * (sqrt(v) / sqrt(1 - 0.999^(t + 1)) + 1e-8), the two corrections formed in fp64. */
int scouter_iba_step_f32(const float* x, const float* mean, const float* std, const float* active, float* alpha, const float* dz,
                         float* adam_m, float* adam_v, int K, int S, int h, int w, int C, float sigma, float min_std, int seed_lo,
                         int seed_hi, int first, float beta, float lr, int t, int relu, void* stream);
/* THE ESTIMATOR.  Welford per element over the B rows of feat fp32 [B][E] in order, continuing from n0 earlier rows:
 * d = x - mean; mean += d / n; m2 += d * (x - mean); nonzero += (x != 0); mean, m2 fp64 [E] and nonzero i32 [E] start at 0.  Any
 * chunking of the same rows gives the same bits. */
int scouter_iba_estimate_f64(const float* feat, double* mean, double* m2, int* nonzero, long n0, int B, long E, void* stream);
/* mean_out = mean, std_out = sqrt(m2 / (n - 1)), active_out = (nonzero / n > threshold) ? 1 : 0, fp32 [E]; n < 2: SC_ERR_ARG. */
int scouter_iba_estimate_finish_f32(const double* mean, const double* m2, const int* nonzero, float* mean_out, float* std_out,
                                    float* active_out, long n, double threshold, long E, void* stream);
/* out[i] = (sum_c cap[i][c]) / ln 2 for cap fp32 [rows][C]: fp64, ascending c, one thread per row. */
int scouter_iba_bits_f32(const float* cap, float* out, long rows, int C, void* stream);

/* ---- I-GOS (Qi, Khorram, Fuxin, AAAI 2020: integrated-gradient optimised saliency, which the reference's torchcam_vis.py runs
 * first of all; csrc/igos.hip, tools/attribution.py igos): the mask side of one iteration.  No reference program runs here: the
 * definitions below are the specification.  R coarse masks pmask fp32 [R][hm][wm] in [0, 1] of ONE image fp32 [C][H][W] and its
 * baseline `base` of the same shape (NULL: zeros), one mask per class; d = image - base, the fp32 difference.  S = n_steps points
 * on the path, T1 = T + 1 entries of the step ladder.  No atomics, every sum in one fixed order that depends on the shapes
 * alone: bit-identical run to run, and a mask's values do not depend on R.  A null or misaligned (4 bytes; 8 for fp64) pointer,
 * R, C, n or n_steps below 1, H or W below 2, hm outside [2, H], wm outside [2, W], a chunk outside its stream, T1 < 2, tv_beta
 * outside [1, 64], a negative or non-finite sigma, tv_coeff or alpha, a flag outside {0, 1} is SC_ERR_ARG; hm * wm above 16384,
 * T1 above 64, R, n_steps or the rows of a trial chunk above 65535 or sizes past 32-bit offsets are SC_ERR_UNSUPPORTED; nothing
 * is launched after an error.
 *
 * THE UPSAMPLER U (torch.nn.UpsamplingBilinear2d, align_corners = True): sy = (float)(hm - 1) / (float)(H - 1); for pixel row y:
 * s = (float)y * sy, i0 = min((int)s, hm - 1), i1 = min(i0 + 1, hm - 1), t = s - i0; the columns likewise; U(p)[y][x] =
 * fma(ty, bot - top, top) with top = fma(tx, p[i0][j1] - p[i0][j0], p[i0][j0]) and bot the same on row i1.  16-byte stores when W
 * is a multiple of 4 and the image-sized pointers are 16-byte aligned, one element otherwise, in every kernel below: the same
 * bits. */
int scouter_igos_upsample_f32(const float* pmask, float* out, int R, int H, int W, int hm, int wm, void* stream);
/* THE PATH.  Stream row g = r * S + j, a = (float)(j + 1) / (float)S: out[g - first][c][q] = fma(sigma, z, fma(a * U(p_r)[q], d[c][q],
 * base[c][q])) for the n rows from `first`, z the value scouter_noise_images_f32 gives for (seed, sample0 + j, e = c * H * W + q):
 * Philox4x32-10 under the key (seed_lo, seed_hi) and the counter (e / 4, sample0 + j, 0, 0), Box-Muller on the word pairs.  Every
 * mask row sees the same noise.  sigma == 0: no noise is formed and out = fma(a * U, d, base).  out may be a leading slice of a
 * longer buffer. */
int scouter_igos_path_images_f32(const float* image, const float* base, const float* pmask, float* out, int first, int n, int R,
                                 int n_steps, int C, int H, int W, int hm, int wm, float sigma, int seed_lo, int seed_hi, int sample0,
                                 void* stream);
/* THE CONTRACTION.  dx fp32 [n][C][H][W], the input gradients of stream rows first .. first + n - 1; acc fp64 [R][H][W]:
 * acc[r][q] = fma(w_j, sum_c (double)dx[g][c][q] * (double)d[c][q], acc[r][q]) for the rows g = r * S + j of the chunk in ascending j,
 * the channel sum from 0 in ascending c, w_j = ((j + 1) / S) / S in fp64: calls over consecutive pieces give the bits of one. */
int scouter_igos_accumulate_f64(const float* image, const float* base, const float* dx, double* acc, int first, int n, int R,
                                int n_steps, int C, int H, int W, void* stream);
/* THE MASK GRADIENT.  loss1(p) = l1 * mean|1 - p| + tv_coeff * (mean_{i < hm - 1, j} |p[i][j] - p[i + 1][j]|^beta +
 * mean_{i, j < wm - 1} |p[i][j] - p[i][j + 1]|^beta), l1 = l1[r] (fp32 [R] on the device), beta = tv_beta; the derivative of |.| and of
 * |.|^beta at 0 is 0.  dmask[r][cell] = (float)(sum_u acc[r][u] * wy_u * wx_u + d loss1 / d p[cell]) in fp64: the adjoint of U as a gather
 * over the pixels u whose i0 / i1 (weights 1 - t / t) and j0 / j1 touch the cell, one wave per cell, a lane adding the pixels
 * lane, lane + 64, ... of the cell's window in row-major order by one fma each, then a butterfly.  stats fp64 [R][2] =
 * (loss1(p_r), sum over the cells of (double)dmask^2, the stored fp32 values), one workgroup of 1024 threads per row: a thread adds
 * its cells t, t + 1024, ... in order, the lanes meet by a butterfly and the waves in order.  Two launches. */
int scouter_igos_mask_grad_f32(const float* pmask, const double* acc, const float* l1, float* dmask, double* stats, float tv_coeff,
                               float tv_beta, int R, int H, int W, int hm, int wm, void* stream);
/* THE TRIALS of the line search.  steps fp32 [T1] on the device, steps[0] = 0.  Stream row g = r * T1 + k: cand_k[cell] =
 * min(max(fma(-steps[k], dmask[r][cell], p_r[cell]), 0), 1) (a NaN goes to 0), out[g - first][c][q] = fma(U(cand_k)[q], d[c][q],
 * base[c][q]).  No noise. */
int scouter_igos_trial_images_f32(const float* image, const float* base, const float* pmask, const float* dmask, const float* steps,
                                  float* out, int first, int n, int R, int T1, int C, int H, int W, int hm, int wm, void* stream);
/* THE STEP, in place.  logp fp32 [R * T1][n_out], the outputs for the trial stream; cols i32 [R] in [0, n_out) (checked by the
 * caller; clamped here).  Per row r in fp64: tot_k = loss1(cand_k) + exp(logp[r * T1 + k][cols[r]]), thr_k = tot_0 - alpha * steps[k] *
 * stats[r][1]; chosen = the first k in 1 .. T with NOT (tot_k > thr_k) -- a NaN accepts -- and T when none passes; p_r = cand_chosen,
 * the bits of the trial stream.  curves fp64 [R][n_iters][4]: curves[r][it] = (loss1(p_r) before, exp(logp[r * T1][cols[r]]),
 * steps[chosen], chosen).  adapt = 1 and n_iters > 3: at it == n_iters / 2, l1[r] /= 10 when |curves[r][it][1] - curves[r][0][1]| <=
 * 1e-3; otherwise at it == (int)(n_iters / 1.25), l1[r] /= 5 when that difference is <= 1e-2 (fp32 divisions, after this
 * iteration's totals).  One workgroup of 1024 threads per row, the sums of loss1 as in scouter_igos_mask_grad_f32. */
int scouter_igos_step_f32(float* pmask, const float* dmask, const float* steps, const float* logp, const int* cols, const double* stats,
                          float* l1, double* curves, int R, int T1, int n_out, int hm, int wm, int it, int n_iters, double alpha,
                          float tv_coeff, float tv_beta, int adapt, void* stream);

/* ---- LIME (Ribeiro et al., KDD 2016) and KernelSHAP (Lundberg & Lee, NeurIPS 2017): a linear surrogate over d superpixels,
 * fitted to the class probabilities of N perturbed copies of an image (csrc/surrogate.hip, tools/attribution.py superpixels /
 * lime / kernelshap).  No reference program runs either; this comment is the specification.  Images are fp32 [B][C][H][W],
 * labels i32 [B][H][W] in [0, d), 1 <= d <= 128, C <= 30.  Every call has one fixed order per output element and no atomics:
 * bit-identical run to run.  A null or misaligned pointer, a count below 1, d outside [1, 128], a grid larger than the image or
 * K = 0 is SC_ERR_ARG, with a message that names the call; nothing is launched after an error.  Every label a kernel indexes
 * with is clamped to [0, d - 1].
 *
 * SEGMENTATION: SLIC (Achanta et al. 2012) on the image as it is given (the normalised tensor, not Lab) and without the
 * connectivity pass.  The grid: pixel (y, x) lies in cell (y * gy / H, x * gx / W) (integer division) and cell (i, j) has label
 * i * gx + j, d = gy * gx.  labels_0 is the grid; for t = 1 .. iters: centres = update(x, labels_{t-1}), labels_t = assign(x,
 * centres).
 *
 * UPDATE.  centres fp32 [B][d][C + 2] = (the C mean colours, mean y, mean x) and means fp32 [B][d][C] = the mean colours, of the
 * pixels that carry the segment's label: float64 sums in a fixed order, one division, rounded once to fp32.  A segment without a
 * pixel keeps the centre it had (centres is read and written) and gets means 0.  window = 1: a segment's pixels are looked for
 * in the 3 x 3 cells around its own cell only, where `assign` puts them (gy <= H and gx <= W); window = 0: in the whole image,
 * for labels of any origin (then only d = gy * gx counts).  One workgroup per (segment, image). */
int scouter_slic_update_f32(const float* images, const int* labels, float* centres, float* means, int B, int C, int H, int W,
                            int gy, int gx, int window, void* stream);
/* ASSIGN.  Each pixel compares the centres of the 3 x 3 cells around its home cell, clipped to the grid, in ascending label
 * order: D^2 = sum_c (x_c - mu_c)^2 (one fma per channel from 0) and then fma(lambda, fma(dy, dy, dx * dx), .), dy = y - c_y,
 * dx = x - c_x, all fp32.  A strictly smaller D^2 wins, so a tie goes to the smallest label; when every D^2 is a NaN the pixel
 * keeps its home cell.  lambda = (compactness / S)^2 with S = sqrt(H * W / d), formed by the caller in double. */
int scouter_slic_assign_f32(const float* images, const float* centres, int* labels, int B, int C, int H, int W, int gy, int gx,
                            float lambda, void* stream);
/* THE PERTURBED BATCH of ONE image: image fp32 [C][H][W], labels i32 [H][W], z u8 [N][d] -> out fp32 [N][C][H][W],
 * out[n][c][p] = z[n][labels[p]] != 0 ? image[c][p] : hide[c][p], with hide[c][p] = means[labels[p]][c] (means fp32 [d][C]) or,
 * when means is null, the constant `fill`.  A select: every value is an exact copy.  16-byte accesses when W is a multiple of 4
 * and image / labels / out are 16-byte aligned, one pixel per thread otherwise.  Any N >= 1. */
int scouter_segment_images_f32(const float* image, const int* labels, const unsigned char* z, const float* means, float fill,
                               float* out, int N, int d, int C, int H, int W, void* stream);
/* THE MOMENTS of one image, a chunk of N sample rows at a time: z u8 [N][d], logp fp32 [N][n_classes], cols i32 [K] in
 * [0, n_classes) (checked by the caller; clamped here).  With z^ = (1, z != 0) and y[n][k] = exp((double) logp[n][cols[k]]):
 * S f64 [d + 1][d + 1] += sum_n pi_n z^ z^T and T f64 [d + 1][K] += sum_n pi_n z^ y^T.  mode 0 (LIME): pi_n = sqrt(exp(-D^2 /
 * kernel_width^2)), D = 1 - sqrt(|z_n| / d) and D = 1 when |z_n| = 0, in double; mode 1 (KernelSHAP): pi_n = 1.  Every entry
 * belongs to one thread, which starts from the stored value and adds the rows in ascending n: chunks of any length give the
 * bits of one call.  `first` is the chunk's first row in the whole sample matrix: when the chunk holds rows 0 (all ones) and 1
 * (all zeros) of it, their targets go to yref f64 [2][K] (yref may be null). */
int scouter_surrogate_accumulate_f64(const float* logp, const int* cols, const unsigned char* z, double* S, double* T, double* yref,
                                     long first, int N, int n_classes, int K, int d, int mode, double kernel_width, void* stream);
/* THE FIT of B images in one launch, one workgroup each: S f64 [B][d + 1][d + 1], T f64 [B][d + 1][K], yref f64 [B][2][K] ->
 * coef f64 [B][K][d], icpt f64 [B][K].  With S2 = S[1:, 1:], S1 = S[1:, 0], T1 = T[1:], T0 = T[0], S00 = S[0][0]:
 *   mode 0, LIME (ridge alpha on the coefficients, free intercept):  G = S2 - S1 S1^T / S00 + alpha I,  R = T1 - S1 T0 / S00,
 *     w = G^-1 R,  icpt = (T0 - S1^T w) / S00;
 *   mode 1, KernelSHAP (intercept y_0 = yref[1], efficiency sum(phi) = Delta = yref[0] - yref[1] enforced by eliminating the last
 *     feature e = d - 1):  G[a][c] = S2[a][c] - S2[a][e] - S2[e][c] + S2[e][e] + alpha delta_ac,  R[a][k] = T1[a][k] - T1[e][k] -
 *     y_0[k] (S1[a] - S1[e]) - Delta_k (S2[a][e] - S2[e][e]) for a, c < e,  phi = G^-1 R,  phi_e = Delta - sum(phi); d = 1: phi_0 = Delta.
 * G | R is written to ws (at least scouter_surrogate_solve_workspace_bytes(B, d, K) = 8 B d (d + K) bytes; less:
 * SC_ERR_WORKSPACE), factored in place by a Cholesky factorisation and solved by substitution, all float64.  A pivot that is not
 * positive (a NaN included) writes NaN coefficients for that image (and a NaN LIME intercept) and faults nothing. */
size_t scouter_surrogate_solve_workspace_bytes(int B, int d, int K);
int scouter_surrogate_solve_f64(const double* S, const double* T, const double* yref, double* coef, double* icpt, int B, int d,
                                int K, int mode, double alpha, void* ws, size_t ws_bytes, void* stream);
/* THE MAP: out fp32 [B][K][H][W], out[b][k][p] = (float) coef[b][k][labels[b][p]] -- a gather.  B * K <= 65535. */
int scouter_segment_paint_f32(const double* coef, const int* labels, float* out, int B, int K, int d, int H, int W, void* stream);

/* ---- Occlusion sensitivity (Zeiler & Fergus, ECCV 2014; captum's Occlusion) and Ablation-CAM (Desai & Ramaswamy, WACV 2020): take
 * a part away -- a window of the image, a channel of the backbone's output -- and see what the class loses (csrc/occlusion.hip,
 * csrc/ablation.hip, tools/attribution.py occlusion / ablationcam).  No reference program runs either; this comment is the
 * specification.  Both loops put the untouched input in row 0 of every batch and read the loss with scouter_output_deltas_f64.  Every
 * call has one fixed order per output element and no atomics: bit-identical run to run.  A null or misaligned pointer, a count
 * below 1, rows outside the stream or a geometry outside the rule below is SC_ERR_ARG, with a message that names the call; nothing
 * is launched after an error.
 *
 * THE WINDOWS, per axis of `size` pixels with window `win` and stride `str`, 1 <= str <= win <= size: n = 1 + ceil((size - win) / str)
 * windows; window i covers [i * str, min(i * str + win, size)) -- the last one may be partial; the windows that cover pixel y are
 * exactly i in [max(0, ceil((y - win + 1) / str)), min(n - 1, floor(y / str))], a range that is never empty.  With (wh, sy) for the
 * rows and (ww, sx) for the columns there are ny and nx of them, window n = iy * nx + ix, N = ny * nx.
 *
 * THE OCCLUDED BATCH: image fp32 [C][H][W] -> out fp32 [1 + n][C][H][W].  Row 0 is the image; row 1 + j is the image with window
 * first + j set to `fill` (not a NaN) in every channel and a bit-exact copy elsewhere; first >= 0, first + n <= N.  16-byte accesses
 * when W is a multiple of 4 and image / out are 16-byte aligned, one pixel per thread otherwise: the same bits. */
int scouter_occlude_images_f32(const float* image, float* out, int first, int n, int C, int H, int W, int wh, int ww, int sy, int sx,
                               float fill, void* stream);
/* THE MAP: deltas fp64 [K][N] (what scouter_output_deltas_f64 wrote for the N windows) -> out fp32 [K][H][W], overwritten:
 * out[k][y][x] = (float)((sum_iy sum_ix deltas[k][iy * nx + ix]) / count) over the windows that cover (y, x), iy ascending, then ix
 * ascending, in fp64; count is their number.  One thread per output element: no atomics and no partial sums. */
int scouter_occlusion_finish_f32(const double* deltas, float* out, int K, int H, int W, int wh, int ww, int sy, int sx, void* stream);
/* THE ABLATED BATCH: feat fp32 NHWC [P = h * w][C] -> out fp32 [1 + n][P][C].  Row 0 is feat; row 1 + j is feat with channel first + j
 * set to 0.0f at every position and a bit-exact copy elsewhere; first >= 0, first + n <= C.  16-byte accesses when C is a multiple
 * of 4 and feat / out are 16-byte aligned, one element per thread otherwise: the same bits. */
int scouter_ablate_channels_f32(const float* feat, float* out, int first, int n, int P, int C, void* stream);
/* THE CLASS MAP: deltas fp64 [K][C] (the drop of the class probability per ablated channel), clean fp32 [n_classes] (the clean
 * log-probabilities), cols i32 [K] in [0, n_classes) (checked by the caller; clamped here), feat as above -> out fp32 [K][P],
 * overwritten.  w[k][c] = (float)(deltas[k][c] / exp((double)clean[cols[k]])), rounded from fp64 once (a clean probability of 0
 * gives the infinity or NaN the division gives); out[k][p] starts from 0 and adds fmaf(w[k][c], feat[p][c], .) for c ascending,
 * then is clamped at 0 (fmaxf: a NaN becomes 0) when relu != 0.  One thread per output element, the weights staged through LDS in
 * pieces.  Any C >= 1, any K >= 1. */
int scouter_ablation_contract_f32(const double* deltas, const float* clean, const int* cols, const float* feat, float* out, int K,
                                  int n_classes, int P, int C, int relu, void* stream);

/* ---- Layer attributions that keep the gradient per position of the backbone's output (the reference's captum_vis.py attributes
 * to model.layer4 with captum's layer methods): Layer Integrated Gradients, Layer Conductance (Dhamdhere et al. 2018), HiResCAM
 * (Draelos & Carin 2020) and LayerCAM (Jiang et al. 2021) (csrc/layerattr.hip, tools/attribution.py layer_integrated_gradients /
 * layer_conductance / layer_gradxact).  No reference program runs them; this comment is the specification.  Features and
 * gradients are fp32 NHWC, one image [P = h * w][C]; every product and sum is formed in fp64.  Every call has one fixed order per
 * output element and no atomics: bit-identical run to run.  A null or misaligned pointer (fp32: 4 bytes, fp64: 8), a count below
 * 1, r below 2 or an unknown mode is SC_ERR_ARG; a tensor past the 32-bit offsets is SC_ERR_UNSUPPORTED; each with a message that
 * names the call, and nothing is launched after an error.  16-byte accesses when C is a multiple of 4 and the pointers are
 * 16-byte aligned, one element at a time otherwise.
 *
 * A POSITION'S CHANNEL SUM, shared by the map of scouter_layer_attr_finish_f32 and by scouter_layer_gxa_f32: one wave per
 * position; lane l adds the terms of the channel groups q = l, l + 64, ... (V = 4 channels on the 16-byte path, else 1; within a
 * group and from group to group in ascending c) onto 0.0, then the 64 partial sums meet in a butterfly.  The order depends on C
 * and V alone; the error is inside the (C + 2) * 2^-53 * sum|terms| of any summation order, and a sum of zeros is exactly 0.
 *
 * CONDUCTANCE STEPS: feats, grads fp32 [r][P][C] (r >= 2 consecutive points of a path and the gradients there), acc fp64 [P][C]:
 * acc[e] = fma((double)grads[j][e], (double)feats[j + 1][e] - (double)feats[j][e], acc[e]) for j = 0 .. r - 2 ascending, onto what
 * acc holds.  grads[r - 1] is not read.  Calls over the rows [0 .. m] and [m .. n], which share row m, give the bits of one call
 * over [0 .. n]. */
int scouter_conductance_accumulate_f64(const float* feats, const float* grads, double* acc, int r, int P, int C, void* stream);
/* THE MAPS: acc fp64 [K][P][C] -> map fp32 [K][P], overwritten.  mode SCOUTER_LAYER_PATH: term[k][p][c] = ((double)feat[p][c] -
 * (double)base[p][c]) * acc[k][p][c] with feat, base fp32 [P][C] (base null: zeros); SCOUTER_LAYER_SUM: term = acc, feat and base
 * are ignored and may be null.  map[k][p] = (float)(the channel sum of the terms, above).  attr (may be null) fp32 [K][P][C]
 * receives (float)term.  total (may be null) fp64 [K] receives the sum over p of the UNROUNDED fp64 channel sums: one workgroup
 * of 16 waves per class, wave v adds its positions v, v + 16, ... in ascending order, then the 16 sums are added in wave order. */
int scouter_layer_attr_finish_f32(const float* feat, const float* base, const double* acc, float* map, float* attr, double* total,
                                  int K, int P, int C, int mode, void* stream);
#define SCOUTER_LAYER_PATH 0
#define SCOUTER_LAYER_SUM 1
/* GRADIENT TIMES ACTIVATION: feat, dfeat fp32 [B][P][C] -> out[b * out_stride + p] = (float)(the channel sum of
 * (double)(rectify != 0 ? fmaxf(dfeat, 0) : dfeat) * (double)feat), clamped at 0 in fp64 when relu != 0 (a NaN becomes 0).  out is
 * fp32 [B][P] written through a batch stride in elements, as in scouter_gradcam_f32: one column of a [B][K][P] tensor; a stride
 * below P with B > 1 is SC_ERR_ARG.  rectify = relu = 0 is HiResCAM (captum's LayerGradientXActivation summed over the
 * channels), rectify = relu = 1 LayerCAM. */
int scouter_layer_gxa_f32(const float* feat, const float* dfeat, float* out, int B, int P, int C, long out_stride, int rectify,
                          int relu, void* stream);

/* ---- GradientSHAP / expected gradients (Lundberg & Lee 2017; Erion et al. 2019; captum's GradientShap and LayerGradientShap of
 * the reference's captum_vis.py) (csrc/gradshap.hip, tools/attribution.py gradient_shap / layer_gradient_shap): a path method
 * whose every row walks from its own randomly drawn baseline of a BANK by its own random fraction.  No reference program runs it
 * with this stream; this comment is the specification.  E is the flat element count of one image (or of one image's features),
 * e the flat index, image fp32 [E], bank fp32 [R][E], every tensor dense.
 *
 * THE DRAWS of sample s: (r0, r1, ., .) = Philox4x32-10 (as in scouter_noise_images_f32) of the counter (0, s, 2, 0) under the
 * key (seed_lo, seed_hi); pick_s = ((uint64) r0 * R) >> 32 in [0, R), alpha_s = (float)(2 * (r1 >> 9) + 1) * 2^-24, exact and
 * inside (0, 1).  They depend on (seed, s, R) alone.  The third counter word names the stream: 0 is the normal stream of
 * scouter_noise_images_f32, 1 the uniform stream of scouter_uniform_images_f32, 2 this one; nothing else uses 2.
 * THE NOISY IMAGE: sigma == 0: x~_s = image exactly (no Philox call; a -0.0 stays -0.0); sigma > 0: x~_s[e] is the value
 * scouter_noise_images_f32 writes for (seed, sample s, element e): fmaf(sigma, z(seed, s, e), image[e]), counter (e / 4, s, 0, 0).
 * THE ROW: d_s[e] = x~_s[e] - bank[pick_s][e], one fp32 subtraction; row_s[e] = fmaf(alpha_s, d_s[e], bank[pick_s][e]), the
 * expression of scouter_path_images_f32.
 *
 * One thread owns four consecutive elements (one Philox call serves them), one fixed order per output element, no atomics:
 * bit-identical run to run.  Each call has a 16-byte form (E a multiple of 4 and every pointer 16-byte aligned) and a one-element
 * form that give the same bits.  R < 1, n < 0, first < 0, first + n above 2^31 - 1, E < 0, a sigma that is negative or not finite,
 * an inv_n that is not finite, a null pointer where one is required or a misaligned one (fp32 / int32: 4 bytes, fp64: 8) is
 * SC_ERR_ARG; n * E or R * E of 2^31 or more is SC_ERR_UNSUPPORTED; each with a message that names the call, and nothing is
 * launched after an error.  n == 0 or E == 0 is SC_OK without a launch, after the scalar arguments have been checked all the same
 * (an empty tensor's pointer may be null).
 *
 * picks int32 [n], alphas fp32 [n]: the draws of the samples first .. first + n - 1.  Either may be null (both: no launch). */
int scouter_gradshap_draws(int* picks, float* alphas, int seed_lo, int seed_hi, int first, int n, int R, void* stream);
/* out fp32 [n][E], out[j] = row_{first + j}.  A row's value depends on (seed, first + j, e) alone, so chunks written by separate
 * calls equal one call.  A dense leading slice of a longer out is fine.  At most 65535 * 8 rows per call (SC_ERR_UNSUPPORTED). */
int scouter_gradshap_images_f32(const float* image, const float* bank, float* out, float sigma, int seed_lo, int seed_hi, int first,
                                int n, int R, long E, void* stream);
/* grads fp32 [n][E] (the gradients at the rows first .. first + n - 1), acc fp64 [E]: for j ascending t = (double)grads[j][e] *
 * (double)d_{first + j}[e], exact in fp64, then acc[e] = fma(t, inv_n, acc[e]), onto what acc holds.  d is formed again from the
 * draws, the noise included, as scouter_perturb_dots_f64 forms its noise again; it is never stored.  The accumulator stays in
 * registers over the j loop: calls over consecutive pieces give the bits of one call. */
int scouter_gradshap_accumulate_f64(const float* grads, const float* image, const float* bank, double* acc, float sigma,
                                    double inv_n, int seed_lo, int seed_hi, int first, int n, int R, long E, void* stream);

/* ---- BatchNorm2d (+ReLU, +residual add): timm/models/resnet.py:383 (norm_layer), BasicBlock :172-199,
 * ResNestBottleneck resnest.py:111-143.  Training mode: batch statistics (fp64 accumulation), running stats
 * updated with `momentum` and the unbiased variance; eval mode: running stats.
 * y = (x - mean) * scale + shift with scale = gamma*rstd, shift = beta; mean/rstd/scale are saved for the backward.
 * relu_mask_out (optional, needs relu): sign bitmask of y, scouter_relu_mask_words(M*C) 64-bit words (1 bit/element);
 * handing it to scouter_bn_bwd_f32 as relu_mask replaces the 4-byte-per-element read of ymask in both backward passes.
 * planes_out (optional): the output ALSO as nplanes (1 or 3) bf16 operand planes for scouter_conv2d_fwd_planes
 * (likewise dx_planes of scouter_sa_bn_bwd_f32 for scouter_conv2d_dgrad_planes).
 * residual_bn_saved (optional, with residual): `residual` is the RAW output of the downsample convolution and this is
 * its BatchNorm's saved block [4][C] (statistics finalised by a y == NULL call): y = relu(bn(x) + bn_ds(residual)) in
 * one pass -- the downsample BatchNorm's output is never stored (resnet.py:404-412 `x += residual` with
 * residual = downsample(x)). */
size_t scouter_relu_mask_words(long n);
size_t scouter_colreduce_workspace_bytes(long M, int C);
int scouter_bn_fwd_f32(const float* x, float* y, const float* residual, long M, int C, const float* gamma,
                       const float* beta, float* running_mean, float* running_var, float momentum, float eps,
                       int training, int relu, float* mean_out, float* rstd_out, float* scale_out, float* shift_out,
                       const double* ext_partial, int ext_rows, unsigned long long* relu_mask_out, void* planes_out,
                       int nplanes, const float* residual_bn_saved, void* ws, size_t ws_bytes, void* stream);
/* typed storage (see ACTIVATION STORAGE above): x / y / residual per `io`; a bf16 x needs ext_partial in training mode
 * (its batch statistics are those of the producing convolution's fp32 accumulators) */
int scouter_bn_fwd_io(const void* x, void* y, const void* residual, long M, int C, const float* gamma,
                      const float* beta, float* running_mean, float* running_var, float momentum, float eps,
                      int training, int relu, float* mean_out, float* rstd_out, float* scale_out, float* shift_out,
                      const double* ext_partial, int ext_rows, unsigned long long* relu_mask_out, void* planes_out,
                      int nplanes, const float* residual_bn_saved, int io, void* ws, size_t ws_bytes, void* stream);
/* y == NULL in scouter_bn_fwd_f32: with planes_out the apply pass writes the planes only (every consumer reads planes: 6
 * instead of 10 bytes per element); without, statistics / running-stat update only.  scouter_bn_apply_f32: the apply pass alone
 * from a saved block [4][C] = {mean, rstd, scale, shift} (contiguous rows, as written through the four *_out pointers). */
int scouter_bn_apply_f32(const float* x, const float* bn_saved, float* y, long M, int C, int relu, void* stream);
/* g = dy * (y > 0), the sign taken from relu_mask if given, else from ymask (both may be NULL: no ReLU);
 * dgamma/dbeta may be NULL (frozen); gout (may be NULL) receives g.
 * ext_partial (may be NULL): [ext_rows][C][2] fp64 (sum g, sum g * xhat) already reduced by the epilogue of the
 * input-gradient kernel that produced dy (scouter_conv2d_dgrad_bnbwd_*): dy then IS g (ymask / relu_mask / gout must be
 * NULL) and the reduction pass over (dy, x) is skipped. */
int scouter_bn_bwd_f32(const float* dy, const float* ymask, const float* x, const float* mean, const float* rstd,
                       const float* scale, const unsigned long long* relu_mask, long M, int C, int training,
                       float* dgamma, float* dbeta, float* dx, float* gout, const double* ext_partial, int ext_rows,
                       void* ws, size_t ws_bytes, void* stream);
/* io: SCOUTER_IO_X_BF16 -- the BatchNorm input x is stored as bf16; SCOUTER_IO_Y_BF16 -- dx is stored as bf16 (for a dx
 * read only by bf16-input convolution kernels, which round it the same way: same results); SCOUTER_IO_R_BF16 -- dy is
 * stored as bf16 (the masked block-output gradient of scouter_conv2d_dgrad_bnbwd_bf16_io; gout must be NULL) */
int scouter_bn_bwd_io(const void* dy, const float* ymask, const void* x, const float* mean, const float* rstd,
                      const float* scale, const unsigned long long* relu_mask, long M, int C, int training,
                      float* dgamma, float* dbeta, void* dx, float* gout, const double* ext_partial, int ext_rows,
                      int io, void* ws, size_t ws_bytes, void* stream);
/* out[c] = alpha * sum_m a[m][c] * (b ? b[m][c] : 1)  -- bias gradients, d(initial_slots) */
int scouter_colsum_f32(const float* a, const float* b, float* out, long M, int C, float alpha, void* ws,
                       size_t ws_bytes, void* stream);
int scouter_relu_bwd_f32(const float* dy, const float* y, float* dx, long n, void* stream);
int scouter_axpby_f32(const float* a, const float* b, float* y, float alpha, float beta, long n, void* stream);

/* ---- pooling: MaxPool2d(3,2,1) resnet.py:412; AvgPool2d(3,s,1) resnest.py:93 (avd); AvgPool2d(2,s,ceil,
 * count_include_pad=False) resnet.py:300 (downsample_avg) */
int scouter_pool_out_size(int in, int k, int stride, int pad, int ceil_mode);
int scouter_maxpool_fwd_f32(const float* x, float* y, unsigned char* argmax, int B, int H, int W, int C, int k,
                            int stride, int pad, void* stream);
int scouter_maxpool_bwd_f32(const float* dy, const unsigned char* argmax, float* dx, int B, int H, int W, int C, int k,
                            int stride, int pad, void* stream);
/* BatchNorm + ReLU + MaxPool2d fused in both directions (the stem: bn1, act1, maxpool -- timm/models/resnet.py:404-412,
 * 494-496).  bn_saved = the [4][C] block {mean, rstd, scale, shift} finalised by scouter_bn_fwd_f32(y = NULL).
 * fwd: y = maxpool(relu(bn(x))) and the arg-max taps; the activation and its sign mask are never stored.
 * bwd: dy = gradient of the pooled tensor -> dx = gradient of the BatchNorm INPUT, dgamma / dbeta (may be NULL);
 * workspace scouter_colreduce_workspace_bytes(B*Ho*Wo, C) + 2*C*4 bytes; stride 1 / 2. */
int scouter_bn_maxpool_fwd_f32(const float* x, const float* bn_saved, float* y, unsigned char* argmax, int B, int H, int W,
                               int C, int k, int stride, int pad, void* stream);
int scouter_bn_maxpool_bwd_f32(const float* dy, const unsigned char* argmax, const float* x, const float* bn_saved, int B,
                               int H, int W, int C, int k, int stride, int pad, int training, float* dgamma,
                               float* dbeta, float* dx, void* ws, size_t ws_bytes, void* stream);
/* io & SCOUTER_IO_Y_BF16: dx is stored as bf16 */
int scouter_bn_maxpool_bwd_io(const float* dy, const unsigned char* argmax, const float* x, const float* bn_saved, int B,
                              int H, int W, int C, int k, int stride, int pad, int training, float* dgamma,
                              float* dbeta, void* dx, int io, void* ws, size_t ws_bytes, void* stream);
int scouter_avgpool_fwd_f32(const float* x, float* y, int B, int H, int W, int C, int k, int stride, int pad,
                            int ceil_mode, int count_include_pad, void* stream);
int scouter_avgpool_fwd_io(const void* x, float* y, int B, int H, int W, int C, int k, int stride, int pad,
                           int ceil_mode, int count_include_pad, int io, void* stream);    /* io: SCOUTER_IO_X_BF16 */
int scouter_avgpool_bwd_f32(const float* dy, float* dx, int B, int H, int W, int C, int k, int stride, int pad,
                            int ceil_mode, int count_include_pad, void* stream);
int scouter_transpose_f32(const float* in, float* out, int batch, int rows, int cols, void* stream);

/* ---- split attention glue: timm/models/layers/split_attn.py:62-80 (radix 2, cardinality 1).
 * bn_saved (may be NULL) = the [4][2Cp] block {mean, rstd, scale, shift} scouter_bn_fwd_f32 wrote for bn0: x is then the
 * RAW output of the radix convolution and relu(bn0(x)) is evaluated on the fly -- the activation is never stored
 * (scouter_bn_fwd_f32 with y == NULL only finalises the statistics).  scouter_sa_bn_bwd_f32 is the matching backward:
 * gradient w.r.t. the split-attention input h0 (from dout, the attention weights a and d(gap)), ReLU mask recomputed from
 * x0, BatchNorm backward of bn0 (dgamma / dbeta may be NULL) -> dx = gradient w.r.t. the convolution output.  * bn_sums (optional): the per-image statistics [B][2C'][4] (fp64) that scouter_sa_reduce_f32(mode 1, bn_sums_out) produced
 * in the d(attention) pass -- g = (dout * a + dgap / HW) * [bn0(x0) > 0] is affine in (a, dgap), constants of an image,
 * so its BatchNorm-backward sums follow from them and the reduction pass over (dout, x0) is skipped. */
size_t scouter_sa_workspace_bytes(int B, int HW, int C2);
/* typed storage of the radix convolution's raw output x / x0 (SCOUTER_IO_X_BF16) and of the attention-weighted sum `out`
 * (SCOUTER_IO_Y_BF16) -- see ACTIVATION STORAGE above */
int scouter_sa_reduce_io(const void* x, const float* dout, const float* bn_saved, float* out, double* bn_sums_out, int B,
                         int HW, int Cp, int mode, int io, void* ws, size_t ws_bytes, void* stream);
int scouter_sa_bn_bwd_io(const float* dout, const float* a, const float* dgap, const void* x0, const float* bn_saved,
                         const double* bn_sums, int B, int HW, int Cp, int training, float* dgamma, float* dbeta,
                         float* dx, void* dx_planes, int nplanes, int io, void* ws, size_t ws_bytes, void* stream);
int scouter_sa_apply_fwd_io(const void* x, const float* a, const float* bn_saved, void* out, int B, int HW, int Cp, int io,
                            void* stream);
int scouter_sa_reduce_f32(const float* x, const float* dout, const float* bn_saved, float* out, double* bn_sums_out,
                          int B, int HW, int Cp, int mode, void* ws, size_t ws_bytes, void* stream);
int scouter_sa_bn_bwd_f32(const float* dout, const float* a, const float* dgap, const float* x0, const float* bn_saved,
                          const double* bn_sums, int B, int HW, int Cp, int training, float* dgamma, float* dbeta,
                          float* dx, void* dx_planes, int nplanes, void* ws, size_t ws_bytes, void* stream);
int scouter_radix_softmax_fwd_f32(const float* z, float* a, int B, int Cp, void* stream);
int scouter_radix_softmax_bwd_f32(const float* a, const float* da, float* dz, int B, int Cp, void* stream);
int scouter_sa_apply_fwd_f32(const float* x, const float* a, const float* bn_saved, float* out, int B, int HW, int Cp,
                             void* stream);
int scouter_sa_apply_bwd_f32(const float* dout, const float* a, const float* dgap, float* dx, int B, int HW, int Cp,
                             void* stream);

/* ---- xSlot head: sloter/utils/position_encode.py:26-46; sloter/utils/slot_attention.py:44-96;
 * sloter/slot_model.py:117-121; tools/calculate_tool.py:4-7 */
int scouter_posenc_sine_f32(float* pe /* [h*w][d] token-major */, int h, int w, int d, void* stream);
/* X: [B][N][d] tokens after conv1x1+ReLU; PE: [N][d]; tok_w / tok_b: HOST arrays of L device pointers, one
 * [d][d] (out,in) weight / [d] bias per to_k Linear; slots0: [S][d];
 * GRU weights in nn.GRU layout (gate order r,z,n).  Outputs: logits [B][S/spc], attn [B][S][N] (last iteration),
 * area_part [B] (per-image sum of attn).  Saved for backward: Ksave [B][N][d], Hsave [L][B][N][d] (the INPUT of
 * every to_k layer: Hsave[0] = X+PE), states [T-1][B][S][d] (slots entering iterations 2..T). */
int scouter_xslot_fwd_f32(const float* X, const float* PE, const float* const* tok_w, const float* const* tok_b,
                          const float* slots0,
                          const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh, int B, int N,
                          int d, int S, int spc, int T, int L, float loss_status, float* logits, float* attn,
                          float* area_part, float* Ksave, float* Hsave, float* states, void* stream);
size_t scouter_xslot_bwd_workspace_bytes(int B, int N, int d, int S, int T);
/* dlogits: [B][S/spc]; g_area_sum: device scalar dL/d(sum attn_T).  Outputs: dX [B][N][d]; dgi, dgh
 * [T-1][B][S][3d] and Usave [T-1][B][S][d] (operands of the GRU weight-gradient GEMMs); ds0 [B][S][d];
 * dZ [L][B][N][d] (pre-activation gradients of the to_k layers). */
int scouter_xslot_bwd_f32(const float* X, const float* PE, const float* const* tok_w, const float* slots0,
                          const float* w_ih,
                          const float* w_hh, const float* b_ih, const float* b_hh, const float* Ksave,
                          const float* Hsave, const float* states, const float* dlogits, const float* g_area_sum,
                          int B, int N, int d, int S, int spc, int T, int L, float loss_status, float* dX, float* dgi,
                          float* dgh, float* Usave, float* ds0, float* dZ, void* ws, size_t ws_bytes, void* stream);
/* ---- HEAD INSTANCES: which kernel instantiation scouter_xslot_fwd_f32 / scouter_xslot_bwd_f32 take for a head of N tokens,
 * S slots, T iterations and L to_k layers under the CURRENT switches xslot_small / xslot_bwd_halves / xslot_bwd_scratch, asked
 * without calling them: no HIP call, so it answers before a device exists and on a machine without one.  Returns 1 and fills
 * inst[SCOUTER_XSLOT_INST_WORDS], or 0 when the entry points refuse the shape (N > 96, S > 512, T > 8, L > 8, a size < 1).  Both
 * entry points select their kernel through the same rule (csrc/xslot_common.h, xs_instance), and the tile backward derives
 * its walk from the inline that fills words 6 and 7.  attn_align16: whether the `attn` pointer is 16-byte aligned.
 *   [0] small      1: the 16-slot kernels (S <= 16 with xslot_small on), else the 32-slot tile kernels
 *   [1] NJT        token tiles of 32, 1..3 (small: the token-width parameter, 1 for N <= 64, else 2)
 *   [2] GX         forward: live 8-token groups of the token contraction -- 4 NJT, or 11 for 65 <= N <= 88 (small: 0)
 *   [3] TPW        forward: slot tiles per wave, ceil(ceil(S / 32) / 4) = 1..4 (small: 0)
 *   [4] attn form  forward: 1 = 16-byte stores of the attention map (S * N % 4 == 0 and the pointer aligned), 0 = scalar
 *   [5] backward   SCOUTER_XSLOT_BWD_* family
 *   [6] nfull, [7] nhalf   backward walk: slot tiles walked 32 wide, then live 16-slot half tiles (small: 0, 0)
 *   [8] backward dynamic-LDS bytes
 *   [9] ceil(S / 32),  [10] forward: the leftover tiles (ceil(S / 32) % 4 = 1, 2) are shared by wave pairs */
#define SCOUTER_XSLOT_BWD_TILE 0     /* xslot_bwd_kernel<1 | 2> */
#define SCOUTER_XSLOT_BWD_TILE_WG 1  /* xslot_bwd_kernel<3, true>: 64 < N <= 96, W_ih read from global memory */
#define SCOUTER_XSLOT_BWD_SCRATCH 2  /* xslot_bwd_scratch_kernel<3>: 64 < N <= 96 with xslot_bwd_scratch on */
#define SCOUTER_XSLOT_BWD_SMALL 3    /* xslot_small_bwd_kernel<1 | 2> */
#define SCOUTER_XSLOT_INST_WORDS 11
int scouter_xslot_instance(int N, int S, int T, int L, int attn_align16, int* inst);
/* stats[0..4] = loss, nll, area**power, top-1 accuracy, area.  labels: int64 (may be NULL -> log_softmax only). */
int scouter_slot_loss_fwd_f32(const float* logits, const long* labels, const float* area_part, int n_area_part, int B,
                              int C, double area_count, float lambda, float power, float* logp, float* stats,
                              void* stream);
int scouter_slot_loss_bwd_f32(const float* logp, const long* labels, const float* stats, const float* g_loss,
                              const float* g_nll, const float* g_term, const float* g_logp, int B, int C,
                              double area_count, float lambda, float power, float* dlogits, float* g_area_sum,
                              void* stream);

/* ---- FC baseline head (`use_slot=False`): global average pool = scouter_avgpool_*_f32 with k = H, then
 * nn.Linear (weight [C][K], sloter/slot_model.py:116-125, timm/models/resnet.py:503-509).  Each of dx, dw, db may be NULL
 * independently of the other two: an output that is given is written, whichever of the others are left out. */
int scouter_linear_small_fwd_f32(const float* x, const float* w, const float* bias, float* y, int B, int K, int C,
                                 void* stream);
int scouter_linear_small_bwd_f32(const float* dy, const float* x, const float* w, float* dx, float* dw, float* db,
                                 int B, int K, int C, void* stream);

/* ---- convolution on pre-split bf16 operand planes (scouter_amd/csrc/conv_planes.hip; same reference call sites as
 * scouter_conv2d_*_f32).  nplanes = 3: x = hi + mid + lo exactly, six bf16 MFMA products per fp32 product -> fp32
 * accuracy at 2.7x the fp32-MFMA rate;  nplanes = 1: plain bf16 inputs (BASELINE configs[4]).
 * planes: [nplanes][elements] bf16, every plane laid out like the fp32 tensor.  Weight planes (k contiguous):
 * w_fwd [nplanes][tap][Cout][Cin/groups], w_dgrad [nplanes][tap][Cin][Cout/groups]; either may be NULL.
 * tile (block tile, callers autotune it): nplanes = 3: 0 = 128x128, 2 = 128x64 (two workgroups per CU), 3 = 64x64,
 * 4 = 256x128 (eight waves), 5 = 256 x (128 | 64) with the input rows resident in LDS for all nine taps (same-size 3x3
 * layers on maps up to 63 pixels wide; falls back to tile 0 / 1 otherwise); nplanes = 1: 0 = 128x128, 1 = 128x64;
 * 6 (1 or 3 planes) = PERSISTENT 256 x (128 | 64): one workgroup per CU walks the tile list, the LDS-DMA stream runs on into
 * the next tile, register epilogue (csrc/conv_planes_persist.h; needs >= 2 K-tiles of 32 channels x taps).
 * Fused BatchNorm-statistics rows = ceil(M / BM) with BM = 128, 128, 128, 64, 256, 256 for tile 0..5; tile 6 writes one row
 * per 64-row wave row of its 256-row tiles: 4 * ceil(M / 256).  scouter_conv2d_fwd_planes_bn_partial_rows returns the
 * largest count any tile writes (4 * ceil(M / 256)).  Tile 6 with bn_partial AND bias / addend, or with fewer than two
 * K-tiles, is refused with SC_ERR_UNSUPPORTED (no silent re-routing: the row layout depends on the tile).  Tiles 0-4 and 6
 * sum every output ELEMENT in the same K order (bit-identical convolution outputs); the fused BatchNorm statistics are
 * per-tile partial sums, grouped differently per tile, so batch statistics -- and everything downstream -- agree between
 * tiles to fp64 rounding of the partial sums, not bit for bit; tile 5 sums 16-channel chunks outer / taps inner. */
int scouter_planes_split_f32(const float* x, void* planes, long n, int nplanes, void* stream);
int scouter_planes_split_weight_f32(const float* w_hwio, void* w_fwd, void* w_dgrad, int kh, int kw, int Cin, int Cout,
                                    int groups, int nplanes, void* stream);
/* The weight split of EVERY plane convolution of a model in one launch (the weights change with every optimizer step):
 * `table` = nrows device-resident rows of scouter_planes_split_weights_row_bytes() bytes each, laid out as
 * { const float* w_hwio; void* w_fwd; void* w_dgrad; int taps, cin_per_group, cout, groups; long first; } with `first` the
 * running element count and total = sum of taps * cin_per_group * cout. */
size_t scouter_planes_split_weights_row_bytes(void);
int scouter_planes_split_weights_multi(const void* table, int nrows, long total, int nplanes, void* stream);
int scouter_conv2d_fwd_planes_bn_partial_rows(int B, int H, int W, int kh, int kw, int stride, int pad);
/* io & SCOUTER_IO_Y_BF16: y is stored as bf16 (tiles 0-5; the persistent tile 6 writes fp32 only) */
int scouter_conv2d_fwd_planes_io(const void* x_planes, const void* w_planes, const float* bias, const float* addend,
                                 void* y, double* bn_partial, int B, int H, int W, int Cin, int Cout, int kh, int kw,
                                 int stride, int pad, int groups, int relu, int nplanes, int tile, int io, void* stream);
int scouter_conv2d_fwd_planes(const void* x_planes, const void* w_planes, const float* bias, const float* addend,
                              float* y, double* bn_partial, int B, int H, int W, int Cin, int Cout, int kh, int kw,
                              int stride, int pad, int groups, int relu, int nplanes, int tile, void* stream);
int scouter_conv2d_dgrad_planes(const void* dy_planes, const void* w_planes, const float* addend, float* dx, int B, int H,
                                int W, int Cin, int Cout, int kh, int kw, int stride, int pad, int groups, int nplanes,
                                int tile, void* stream);
int scouter_conv2d_dgrad_planes_bnbwd(const void* dy_planes, const void* w_planes, const float* addend, float* dx, int B,
                                      int H, int W, int Cin, int Cout, int kh, int kw, int stride, int pad, int groups,
                                      int nplanes, int tile, const void* relu_mask, const float* x1,
                                      const float* saved1, double* part1, const float* x2, const float* saved2,
                                      double* part2, void* stream);

/* weight gradient on planes: same-size stride-1 convolutions (2 * pad == k - 1), 64-multiples of channels per group;
 * x_planes [nplanes][B*H*W][Cin], dy_planes [nplanes][B*H*W][Cout]; dw HWIO fp32; split-K slabs in ws, summed in a
 * fixed order.  plan_hint: -1 = static plan; else bits 0-1 = workgroup budget {512, 1024, 2048, 4096}, bit 4 / bit 5 = 64
 * instead of 128 input / output channels per tile; bit 6 (3x3, pad 1, maps up to 63 wide) = the TAP-FUSED kernel
 * (csrc/conv_planes_wgrad_taps.h: one workgroup accumulates all nine taps of a 64 x 64 tile from an LDS-resident ring of X
 * rows), bits 0-1 then = budget {256, 512, 1024, 2048} workgroups (callers autotune it; every plan is deterministic,
 * different plans sum the pixels in a different order). */
size_t scouter_conv2d_wgrad_planes_workspace_bytes(int B, int H, int W, int Cin, int Cout, int kh, int kw, int groups,
                                                   int plan_hint);
int scouter_conv2d_wgrad_planes(const void* x_planes, const void* dy_planes, float* dw, int B, int H, int W, int Cin,
                                int Cout, int kh, int kw, int pad, int groups, int nplanes, int plan_hint,
                                void* ws, size_t ws_bytes, void* stream);

/* ---- Convolutions at fp32 accuracy on the bf16 matrix cores with the three-way operand split done in registers
 * (csrc/conv_x3.hip, round 5): the deep 1x1 layers of the bottlenecks -- conv1 / conv3 (timm/models/resnest.py:111-143),
 * the downsample convolution (resnet.py:292-306) -- and the stride-1 3x3 layers with 32 channels per group (the deep stem,
 * resnet.py:471-489, and the first radix convolution, layers/split_attn.py:54-60).  The ACTIVATION / GRADIENT is a plain fp32
 * NHWC tensor (no producer writes planes); only the WEIGHT arrives as three bf16 planes (scouter_planes_split_weight_f32 /
 * _weights_multi: forward layout [3][taps][Cout][Cin/groups], input-gradient layout [3][taps][Cin][Cout/groups]).  Results are
 * bit-identical to scouter_conv2d_fwd_planes / _dgrad_planes (nplanes = 3) on the split activation.  kh x kw: 1x1 (pad 0) or
 * an odd same-size filter (2 * pad == kh - 1), stride 1; 32-multiples of channels per group, at least two 32-channel K-tiles.
 * tile_hint: 0 = 256x128 (eight waves), 1 = 128x128, 2 = 128x64, 3 = 64x64, 4 = 256x64 (eight waves), 5 = 256x32, 6 = 128x32 (two waves), else the
 * library's choice (scouter_conv2d_x3_tile tells which for N = output columns per group; every tile gives the same bits).
 * bn_partial: as scouter_conv2d_fwd_f32, one row per M tile = scouter_conv2d_x3_partial_rows(M, N, tile_hint).  The input
 * gradient takes the optional fused BatchNorm-backward epilogue of scouter_conv2d_dgrad_bnbwd_f32 (relu_mask .. part2).
 * tile_hint 7 (round 6, csrc/conv_xhalo.hip; only on request, never the library's choice): the 3x3 / pad 1 layers whose GEMM
 * is 32 columns wide per group -- forward with Cout / groups == 32, input gradient with Cin / groups == 32 (the deep stem's
 * 32 -> 32 and 32 -> 64 convolutions, resnet.py:471-489; the input gradient of layer1's radix convolution,
 * layers/split_attn.py:54-60), 16-multiples of GEMM-K channels per group (its own channel rule: 16 and 48 run, which tiles 0-6
 * refuse), maps up to 126 pixels wide, no bias / forward addend -- on a PERSISTENT kernel that splits
 * every input element once and keeps the split rows resident in LDS for all nine taps.  Same error bound as the other
 * tiles, another summation order (16-channel chunk outer, tap inner): equal to fp32 rounding, not bit for bit.  Its
 * bn_partial / part1 / part2 have scouter_conv2d_x3_halo_partial_rows(groups) rows (one per workgroup of a group). */
int scouter_conv2d_x3_tile(long M, int N, int tile_hint);
int scouter_conv2d_x3_partial_rows(long M, int N, int tile_hint);
int scouter_conv2d_x3_halo_partial_rows(int groups);
int scouter_conv2d_fwd_x3(const float* x, const void* w_planes_fwd, const float* bias, const float* addend, float* y,
                          double* bn_partial, int B, int H, int W, int Cin, int Cout, int kh, int kw, int pad, int groups,
                          int relu, int tile_hint, void* stream);
int scouter_conv2d_dgrad_x3_bnbwd(const float* dy, const void* w_planes_dgrad, const float* addend, float* dx, int B,
                                  int H, int W, int Cin, int Cout, int kh, int kw, int pad, int groups, int tile_hint,
                                  const void* relu_mask, const float* x1, const float* saved1, double* part1,
                                  const float* x2, const float* saved2, double* part2, void* stream);

/* Weight gradient of the same layers, dw[Cin][Cout] = x^T dy over the B*H*W pixels (the HWIO gradient of a 1x1 layer), both
 * fp32 operands transposed (4x4 register patches) and split three-way on their way into LDS; 128-multiples of Cin and Cout.
 * Split-K over the pixels into `ws` slabs summed in slab order (deterministic).  plan_hint: -1 / bits 0-1 = workgroup budget
 * 256 << hint (callers take it from the static table; different plans sum the pixels in another order). */
size_t scouter_conv2d_wgrad_x3_workspace_bytes(int B, int H, int W, int Cin, int Cout, int plan_hint);
int scouter_conv2d_wgrad_x3(const float* x, const float* dy, float* dw, int B, int H, int W, int Cin, int Cout,
                            int plan_hint, void* ws, size_t ws_bytes, void* stream);

/* ---- BatchNorm-folded inference (eval mode: nn.BatchNorm2d is the fixed per-channel map y = (x - running_mean) * gamma /
 * sqrt(running_var + eps) + beta, timm/models/resnet.py:383; SlotModel.set_inference_fold).
 * scouter_bn_fold_multi folds EVERY (convolution, BatchNorm) pair of a model in one launch: with s[co] = gamma[co] /
 * sqrt(running_var[co] + eps), w_out[r][co] = w[r][co] * s[co] and bias_out[co] = beta[co] - running_mean[co] * s[co]
 * (+ conv_bias[co] * s[co]); every product is formed in fp64 and rounded once to fp32.  `table` = nrows device-resident rows
 * of scouter_bn_fold_row_bytes() bytes each, laid out as { const float* w, *conv_bias (may be NULL), *gamma, *beta,
 * *running_mean, *running_var; double eps; float* w_out, *bias_out; int rows, cout; long first; } with the HWIO weight seen as
 * [rows = taps * Cin / groups][cout], cout a multiple of 4, `first` the running element count and total = sum of rows * cout.
 * The kernel moves four output channels per access: w, w_out and bias_out must be 16-byte aligned and EVERY row's cout a
 * multiple of 4 (the table lives on the device, so the entry point can only check the total: the caller checks each row).
 * w_out / bias_out are caller-owned persistent buffers; the convolution entry points above then run on
 * them unchanged (scouter_conv2d_weight_bf16t / scouter_planes_split_weights_multi for the bf16 and bf16x3 kernels). */
size_t scouter_bn_fold_row_bytes(void);
int scouter_bn_fold_multi(const void* table, int nrows, long total, void* stream);
/* The split-attention gate of one block in one launch (timm/models/layers/split_attn.py:68-75 with bn1 folded into fc1):
 * a[B][2Cp] = radix_softmax(fc2(relu(gap . w1 + b1)) + b2), gap [B][Cp] (scouter_sa_reduce_f32 mode 0), w1 HWIO [Cp][A] and
 * b1 [A] the folded fc1, w2 HWIO [A][2Cp] and b2 [2Cp] fc2's own.  fp32 FMA; one workgroup per image and one fixed summation
 * order per output element, no atomics: an image's row of `a` does not depend on B.  Covers A = 32 / 64 / 128 / 256 with
 * Cp <= 512 a multiple of 8 * (256 / A) -- resnest26d / 50d: (Cp, A) = (64, 32), (128, 64), (256, 128), (512, 256); anything
 * else is SC_ERR_UNSUPPORTED (callers keep the convolution / softmax entry points). */
int scouter_sa_gate_fwd_f32(const float* gap, const float* w1, const float* b1, const float* w2, const float* b2, float* a,
                            int B, int Cp, int A, void* stream);

/* ---- Backward of the folded path: what a gradient with respect to the IMAGE needs next to the convolution input gradients
 * (SlotModel.image_pass).  Deterministic, no atomics; bad arguments are refused before any launch.
 * scouter_sa_gate_bwd_f32: the backward of scouter_sa_gate_fwd_f32 in one launch, one workgroup per image.  With a [B][2Cp] the
 * forward's output and da [B][2Cp] its gradient: dz = radix softmax backward (the expression of scouter_radix_softmax_bwd_f32),
 * h = relu(gap . w1 + b1) re-formed by the forward's own device function (the same bits), dh = (dz . w2^T) * [h > 0],
 * dgap [B][Cp] = dh . w1^T.  h_out [B][A] (may be NULL) receives h.  fc2's bias is not needed.  One summation order per output
 * element, a function of (Cp, A) alone: a row does not depend on B.  w1 and w2 are read as 16-byte vectors (16-byte aligned).
 * Covers the shapes of scouter_sa_gate_fwd_f32; anything else is SC_ERR_UNSUPPORTED. */
int scouter_sa_gate_bwd_f32(const float* gap, const float* w1, const float* b1, const float* w2, const float* a,
                            const float* da, float* dgap, float* h_out, int B, int Cp, int A, void* stream);
/* dx[b][p][r Cp + c] = x0[b][p][r Cp + c] > 0 ? dout[b][p][c] * a[b][r Cp + c] + dgap[b][c] * (1 / HW) : +0, r = 0, 1:
 * scouter_sa_apply_bwd_f32 and the ReLU backward of the folded radix convolution (whose output x0 [B][HW][2Cp] is stored after its
 * ReLU) in one pass.  Cp a multiple of 4. */
int scouter_sa_apply_relu_bwd_f32(const float* dout, const float* a, const float* dgap, const float* x0, float* dx, int B,
                                  int HW, int Cp, void* stream);
/* scouter_maxpool_bwd_f32 followed by scouter_relu_bwd_f32 with y = h [B][H][W][C], the pool's input, in one pass -- the same
 * windows added in the same order, so the same bits. */
int scouter_maxpool_relu_bwd_f32(const float* dy, const unsigned char* argmax, const float* h, float* dx, int B, int H, int W,
                                 int C, int k, int stride, int pad, void* stream);

/* ---- The rule a ReLU's backward applies in that backward (ImagePass.grad_from `rule`): with g the gradient arriving at the
 * ReLU's output and y that output,
 *   0 gradient    y > 0 ? g : +0                 the derivative: what the four entry points without `rule` compute
 *   1 guided      (y > 0 && g > 0) ? g : +0      guided backpropagation (Springenberg et al. 2015)
 *   2 deconvnet   g > 0 ? g : +0                 the deconvnet rule (Zeiler & Fergus 2014)
 * in plain fp32 comparisons: a NaN or a -0 in g gives +0 under rules 1 and 2.  g is the value the kernel forms in front of its
 * mask: dy (relu_bwd), the row dot sum_n dz[n] w2[j][n] (sa_gate_bwd; h is re-formed and h_out written under every rule),
 * dout * a_r + dgap / HW with the roundings of rule 0 (sa_apply_relu_bwd), the gathered sum of the windows that chose the pixel in
 * the order of rule 0 (maxpool_relu_bwd; the gather itself is the ordinary one).  The rule is a compile-time argument of the
 * kernels: rule 0 runs the code and gives the bits of the entry point without `rule`; rule 2 issues no load of the activation
 * (y / x0 / h; 12 instead of 20 bytes per dout element in sa_apply_relu_bwd), whose pointer is still checked like the others.
 * Any other rule is SC_ERR_ARG before any launch; every other argument and refusal is that of the entry point without `rule`. */
#define SCOUTER_RULE_GRADIENT 0
#define SCOUTER_RULE_GUIDED 1
#define SCOUTER_RULE_DECONVNET 2
int scouter_relu_bwd_rule_f32(const float* dy, const float* y, float* dx, long n, int rule, void* stream);
int scouter_sa_gate_bwd_rule_f32(const float* gap, const float* w1, const float* b1, const float* w2, const float* a,
                                 const float* da, float* dgap, float* h_out, int B, int Cp, int A, int rule, void* stream);
int scouter_sa_apply_relu_bwd_rule_f32(const float* dout, const float* a, const float* dgap, const float* x0, float* dx, int B,
                                       int HW, int Cp, int rule, void* stream);
int scouter_maxpool_relu_bwd_rule_f32(const float* dy, const unsigned char* argmax, const float* h, float* dx, int B, int H,
                                      int W, int C, int k, int stride, int pad, int rule, void* stream);

/* Guided Grad-CAM's product: out[b][c][y][x] = grad[b][c][y][x] * up(cam[b])[y][x], one fp32 multiplication per element.  grad /
 * out dense NCHW fp32 [B][C][H][W] (out == grad allowed; any other overlap is refused), cam [h][w] dense per image, image b at
 * cam + b * cam_stride_b (any stride >= h * w: a column of a [B][K][h][w] tensor).  mode 0: nearest, source index (y h) / H and
 * (x w) / W in integer arithmetic (F.interpolate(mode = "nearest") whenever H % h == 0 and W % w == 0); mode 1: bilinear,
 * align_corners = False, the expressions and the bits of scouter_resize_bilinear_f32.  16-byte accesses when W % 4 == 0 and grad
 * and out are 16-byte aligned, one element at a time otherwise.  Deterministic, no atomics.  Pointers 4-byte aligned; C * H * W and
 * h * w below 2^31. */
int scouter_guided_cam_f32(const float* grad, const float* cam, float* out, int B, int C, int H, int W, int h, int w,
                           long cam_stride_b, int mode, void* stream);

/* p[i] += v for n 64-bit counters (the num_batches_tracked buffers of a model as views of one flat buffer: one launch per
 * training forward instead of one ATen launch; torch.nn.BatchNorm2d increments them one by one) */
int scouter_iadd_i64(long* p, long n, long v, void* stream);

/* ---- optimizer: torch.optim.AdamW defaults (train.py:146).  chunk table = array of {float* param; long offset
 * into the flat grad/moment arenas; int n; int pad} built by the host (scouter_adamw_chunk_bytes() each). */
int scouter_adamw_chunk_bytes(void);
int scouter_adamw_step_f32(const void* chunk_table, int nchunks, const float* grads, float* exp_avg,
                           float* exp_avg_sq, float lr, float beta1, float beta2, float eps, float weight_decay,
                           int step, void* stream);
/* The same update with the step-dependent scalars read from DEVICE memory, so that the launch can live in a captured
 * hipGraph (scouter_amd/graph.py): dyn[0] = learning rate, dyn[1] = step count t >= 1 (as a float, exact below 2^24);
 * the bias corrections 1 - beta^t are formed in the kernel.  The host advances dyn[1] before each launch. */
int scouter_adamw_step_dev_f32(const void* chunk_table, int nchunks, const float* grads, float* exp_avg,
                               float* exp_avg_sq, const float* dyn, float beta1, float beta2, float eps,
                               float weight_decay, void* stream);

#ifdef __cplusplus
}
#endif
#endif
