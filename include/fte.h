/*
 * fte.h -- C ABI of libfte.so, the MI355X (gfx950) kernel library behind
 * tf_face_toolbox_amd's data-parallel training step.
 *
 * The reference (medivhna/TF_Face_Toolbox) has NO native boundary of its own:
 * its hot path is a TensorFlow-1.x graph whose arithmetic lives in stock TF
 * ops.  Each entry point below therefore replaces one TF op
 * (or one fused group of them) at the reference call site cited beside it.
 * A maintainer binds them with ctypes; nothing here takes or
 * returns a torch type.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller; nothing is
 *     allocated, freed or retained by the library; scratch comes in through
 *     (ws, ws_bytes) and fte_*_ws_bytes() says how much a call needs;
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued on it
 *     and the call returns without synchronising;
 *   - return value: 0 = ok, otherwise a negative FTE_E* code or a positive
 *     hipError_t; no C++ exception crosses the boundary;
 *   - every tensor pointer is 16-byte aligned and every tensor smaller than 2 GiB (the kernels move 16 bytes per lane
 *     through range-checked buffer loads); a violation is an error code, never an out-of-bounds access;
 *   - activations are NHWC fp32 (the layout data.py:275-279 hands over; the
 *     reference's NHWC->NCHW transpose, nets/sphere.py:53-54, is folded away),
 *     conv weights are TF HWIO [3,3,Cin,Cout], dense weights are [in,out].
 *   - TF 'SAME' padding (pad_before = pad_total/2) -- asymmetric (0,1) for
 *     stride 2 on even sizes.
 *   - all arithmetic is fp32 with fp32 accumulation (v_mfma_f32_32x32x2_f32
 *     for the GEMM-shaped work), the reference's dtype (nets/sphere.py:35).
 */
#ifndef FTE_H_
#define FTE_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FTE_OK 0
#define FTE_EINVAL (-1)      /* unsupported shape / null pointer */
#define FTE_EWORKSPACE (-2)  /* ws_bytes too small */

/* Library / build identification: "fte <version> gfx950". */
const char* fte_version(void);

/* ---------------------------------------------------------------------------
 * Operand precision of every MFMA product of the library (convolutions and dense GEMMs; process-wide, not per stream).
 *   FTE_MFMA_F32  (default): v_mfma_f32_32x32x2_f32, exact fp32 -- the reference's arithmetic (dtype=tf.float32,
 *                 nets/sphere.py:35).
 *   FTE_MFMA_BF16: operand tiles are rounded to bf16 (round-to-nearest-even) on their way into LDS and multiplied by
 *                 v_mfma_f32_32x32x16_bf16 with fp32 accumulation (16x the fp32 MFMA rate).  Tensors in HBM, epilogues,
 *                 reductions, losses and the optimizer stay fp32 -- mixed precision as in BASELINE.json config 3.
 * Returns FTE_EINVAL for any other value.
 * ------------------------------------------------------------------------- */
#define FTE_MFMA_F32 0
#define FTE_MFMA_BF16 1
int fte_set_mfma_dtype(int dtype);
int fte_get_mfma_dtype(void);

/* ---------------------------------------------------------------------------
 * Convolution algorithm of the stride-1 3x3 layers in the fp32, BN-free entry points (fte_conv3x3_* / fte_conv2d_*): the reference
 * runs them on cuDNN's Winograd algorithm (train.py:260 sets TF_ENABLE_WINOGRAD_NONFUSED=1 for every run; the layers are
 * nets/sphere.py:41-42).  Process-wide; initialised from the environment variable FTE_CONV_ALGO = direct | winograd | auto.
 *   FTE_CONV_DIRECT   implicit GEMM over the nine taps (csrc/igemm.hip)
 *   FTE_CONV_WINOGRAD F(2x2,3x3) -- and F(3x3,2x2) for the filter gradient -- wherever the kernels exist (channels % 64 == 0)
 *   FTE_CONV_AUTO     (default) Winograd for the layers where it measured faster, direct elsewhere: all three products of the layers
 *                     with >= 128 channels (min(cin, cout); FTE_WINO_MIN_C, ops by the bit mask FTE_WINO_OPS, default 7), and the
 *                     forward pass and filter gradient -- not the data gradient -- of 64-channel layers (FTE_WINO_OPS64, default 5:
 *                     bit op of fte_conv3x3_algo).  The 64-channel packs are the large ones: 1.6 GB at 512 images of 56x56
 * Winograd needs the workspace fte_*_ws_bytes reports UNDER THE CURRENT SETTING (transformed tiles: 64 bytes per tile and channel);
 * with less the call runs the direct algorithm.  Same results to fp32 rounding (tests/test_gpu_wino.py: <= 2e-5 of max|ref|).
 * ------------------------------------------------------------------------- */
#define FTE_CONV_DIRECT 0
#define FTE_CONV_WINOGRAD 1
#define FTE_CONV_AUTO 2
int fte_set_conv_algo(int algo);
int fte_get_conv_algo(void);
/* The algorithm the CURRENT switch selects for a 3x3 layer in the fp32 mode, op = 0 forward, 1 data gradient, 2 filter gradient:
 * FTE_CONV_DIRECT or FTE_CONV_WINOGRAD (given the workspace of the matching *_ws_bytes query). */
int fte_conv3x3_algo(int n, int h, int wd, int cin, int cout, int stride, int op);
/* Bytes of the transformed-tile pack V = B^T d B of an [n, h, wd, c] tensor (16 floats per 2x2 tile and channel, row blocks of 64
 * tiles); 0 for shapes the Winograd kernels do not take. */
size_t fte_wino_pack_bytes(int n, int h, int wd, int c);

/* Measurement hook (bench.py's roofline leg; no reference counterpart).  While enabled, every
 * launch of the MFMA kernel family is bracketed by a HIP event pair ON THE LAUNCH STREAM and its
 * algorithmic FLOPs (2*rows*N*K of that launch) are recorded.  fte_prof_enable(1) clears and starts,
 * fte_prof_enable(0) pauses, fte_prof_enable(2) resumes without clearing (sampled recording: the event pair costs a
 * queue barrier per launch, ~5 % of a step at 64 images per GPU); after a device synchronise, fte_prof_get returns record i:
 * sig = {A layout, B layout, epilogue, tile id, split count} (identifies the kernel symbol:
 * igemm_kernel<BM,BN,WM,WN,sig[0],sig[1],sig[2]>; tile 0=128x128 1=256x64 2=128x64 3=64x64),
 * flops, and the launch's duration in milliseconds. */
int fte_prof_enable(int on);
int fte_prof_count(void);
int fte_prof_get(int i, int* sig, double* flops, float* ms);
/* the GEMM shape of record i, mnk = {rows, N, K} (conv forward: rows = n*ho*wo, N = cout, K = 9*cin), and its ALGORITHMIC
 * bytes: every operand and result tensor of that launch once -- what bench.py's per-shape roofline divides by. */
int fte_prof_get_shape(int i, int* mnk, double* bytes);
/* the kernel symbol record i was dispatched to, with its template arguments as `rocprofv3 --kernel-trace` prints them minus
 * blanks (e.g. "igemm_kernel<128,128,2,2,1,0,0,0>", "igemm16_kernel<128,128,4,2,0,2,4,0>"): bench.py's per-symbol table and
 * scripts/pmc_summary.py join the launch records with the profiler's rows on this string -- no name is rebuilt by hand. */
int fte_prof_get_name(int i, char* buf, int buflen);

/* ---------------------------------------------------------------------------
 * 3x3 convolution, TF-SAME, stride 1 or 2, Cin % 32 == 0, Cout % 64 == 0
 * (every conv of nets/sphere.py:41-42,61,65,69 except the first).
 * Implicit GEMM on fp32 MFMA: M = n*ho*wo, K = 9*cin, N = cout.
 * ------------------------------------------------------------------------- */

/* Replaces Conv2D + BiasAdd + the 6-op PReLU (nets/sphere.py:29-36) + residual
 * Add (nets/sphere.py:43):   z = conv(x,w) + bias ;  y = prelu(z, alpha) + res.
 * bias, alpha, res, z may be NULL (no bias / identity / no residual / do not
 * keep the pre-activation).  z is what backward needs (sign of z, min(z,0)). */
int fte_conv3x3_fwd(const float* x, const float* w, const float* bias, const float* alpha,
                    const float* res, float* z, float* y,
                    int n, int h, int wd, int cin, int cout, int stride,
                    void* ws, size_t ws_bytes, void* stream);
/* ws is optional (NULL/0 allowed): with it, leftover or too-few output tiles run as split-K big tiles
 * plus a fused fix-up instead of small tiles (faster tails and small per-GPU shards). */
size_t fte_conv3x3_fwd_ws_bytes(int n, int h, int wd, int cin, int cout, int stride);
/* fte_conv3x3_fwd that LEAVES the transformed input tiles in `vpack` (caller-owned, fte_wino_pack_bytes(n, h, wd, cin) bytes) for the
 * filter gradient of the same layer: the forward pass and Conv2DBackpropFilter read the same B^T d B of x (one transform instead of
 * two).  Only for layers fte_conv3x3_algo reports FTE_CONV_WINOGRAD for (op 0 and op 2); with vpack != NULL the call either runs the
 * Winograd algorithm or fails (FTE_EWORKSPACE) -- it never falls back silently.  vpack = NULL: exactly fte_conv3x3_fwd. */
int fte_conv3x3_fwd_keep(const float* x, const float* w, const float* bias, const float* alpha,
                         const float* res, float* z, float* y,
                         int n, int h, int wd, int cin, int cout, int stride, float* vpack,
                         void* ws, size_t ws_bytes, void* stream);
/* fte_conv3x3_fwd_keep for the two convs of a residual block that both run the Winograd algorithm, so that the first conv's
 * y = prelu(z) -- read by the second conv's tile transform and by nothing else -- never goes to memory:
 *   xalpha != NULL: x is the PRE-activation z of the producing layer and xalpha its PReLU slopes [cin]; the tile transform forms
 *                   x > 0 ? x : xalpha[c] * x itself (the forward epilogue's own expression: V equals the pack of that layer's y);
 *                   xalpha = NULL: x is taken as it is
 *   y = NULL:       only z is written (z must not be NULL then), by an epilogue that issues nothing for y and res
 * vpack is required.  The call runs the Winograd algorithm or fails (FTE_EWORKSPACE; FTE_EINVAL without vpack): the direct and the bf16
 * paths need the activated input and write y, and are never entered from here. */
int fte_conv3x3_fwd_keep_act(const float* x, const float* xalpha, const float* w, const float* bias, const float* alpha,
                             const float* res, float* z, float* y,
                             int n, int h, int wd, int cin, int cout, int stride, float* vpack,
                             void* ws, size_t ws_bytes, void* stream);

/* Replaces Conv2DBackpropInput fused with the PReLU gradient of the PRODUCING
 * layer (tf.gradients, data_parallel.py:33):
 *     g      = conv_transpose(dz, w) + addin          (gradient wrt the input x of this conv)
 *     raw    = g                                      (optional: x is also a residual shortcut)
 *     dzprev = g * prelu'(zprev, alpha_prev)          (zprev NULL: dzprev = g)
 *     dalpha_prev[c] = sum g*min(zprev,0) ; dbias_prev[c] = sum dzprev
 * x has shape [n,h,wd,cin]; dz has the conv's output shape.  addin, raw,
 * zprev, dalpha_prev, dbias_prev may be NULL. */
int fte_conv3x3_dgrad(const float* dz, const float* w, const float* addin,
                      const float* zprev, const float* alpha_prev,
                      float* raw, float* dzprev, float* dalpha_prev, float* dbias_prev,
                      int n, int h, int wd, int cin, int cout, int stride,
                      void* ws, size_t ws_bytes, void* stream);
size_t fte_conv3x3_dgrad_ws_bytes(int n, int h, int wd, int cin, int cout, int stride);

/* Replaces Conv2DBackpropFilter:  dw[3,3,cin,cout] = sum_pixels x (*) dz
 * (deterministic split-K: partial slabs in ws, then an ordered reduction). */
int fte_conv3x3_wgrad(const float* x, const float* dz, float* dw,
                      int n, int h, int wd, int cin, int cout, int stride,
                      void* ws, size_t ws_bytes, void* stream);
size_t fte_conv3x3_wgrad_ws_bytes(int n, int h, int wd, int cin, int cout, int stride);
/* fte_conv3x3_wgrad reading the V pack fte_conv3x3_fwd_keep left for this layer instead of transforming x again.  With vpack != NULL
 * the call runs the Winograd algorithm or fails and x is never read (it may be NULL: fte_conv3x3_fwd_keep_act leaves no activated
 * input behind); vpack = NULL: exactly fte_conv3x3_wgrad. */
int fte_conv3x3_wgrad_kept(const float* x, const float* dz, float* dw,
                           int n, int h, int wd, int cin, int cout, int stride, const float* vpack,
                           void* ws, size_t ws_bytes, void* stream);


/* ---------------------------------------------------------------------------
 * Generic SAME convolution (kernel 1x1 or 3x3, stride 1 or 2, no dilation) on the same MFMA kernel
 * family: the convs of nets/resnet.py:47-61 (`conv_bn_relu`), nets/resnext.py:56-62 and the pointwise
 * convs of nets/shufflenet_v2.py:100-105.  Arguments as fte_conv3x3_*, plus `ksize`.
 * ------------------------------------------------------------------------- */
int fte_conv2d_fwd(const float* x, const float* w, const float* bias, const float* alpha, const float* res,
                   float* z, float* y, int n, int h, int wd, int cin, int cout, int ksize, int stride,
                   void* ws, size_t ws_bytes, void* stream);
size_t fte_conv2d_fwd_ws_bytes(int n, int h, int wd, int cin, int cout, int ksize, int stride);
int fte_conv2d_dgrad(const float* dz, const float* w, const float* addin, const float* zprev,
                     const float* alpha_prev, float* raw, float* dzprev, float* dalpha_prev, float* dbias_prev,
                     int n, int h, int wd, int cin, int cout, int ksize, int stride,
                     void* ws, size_t ws_bytes, void* stream);
size_t fte_conv2d_dgrad_ws_bytes(int n, int h, int wd, int cin, int cout, int ksize, int stride);
int fte_conv2d_wgrad(const float* x, const float* dz, float* dw, int n, int h, int wd, int cin, int cout,
                     int ksize, int stride, void* ws, size_t ws_bytes, void* stream);
size_t fte_conv2d_wgrad_ws_bytes(int n, int h, int wd, int cin, int cout, int ksize, int stride);

/* First layer of the BN nets (7x7 stride 2, Cin = 3; nets/resnet.py:109): cols[n*ho*wo, kpad] with k ordered
 * (r, s, c) like the HWIO weight rows and zero columns from ksize*ksize*cin to kpad (kpad % 32 == 0); the
 * stem is then fte_gemm_nn / fte_gemm_tn on cols. */
int fte_im2col_first(const float* x, float* cols, int n, int h, int wd, int cin, int ksize, int stride,
                     int kpad, void* stream);
/* the same with bf16 columns (bf16 STORAGE: the stem then runs as a 1x1 conv of `kpad` input channels on the bf16-source kernels --
 * fte_conv2d_bn_fwd / fte_conv2d_fwd_s16 / fte_conv2d_wgrad16 with cin = kpad, ksize = 1 -- and its output is stored as bf16) */
int fte_im2col_first_s16(const float* x, uint16_t* cols16, int n, int h, int wd, int cin, int ksize, int stride, int kpad, void* stream);

/* The loader's image transform on DECODED uint8 images (data.py:206-223 of the reference: convert_image_dtype, resize_images
 * to in_h x in_w -- TF-1.x bilinear, align_corners = False --, random_crop to crop_h x crop_w, random_flip_left_right,
 * (x - 0.5) / 0.5; the evaluation transform of data.py:153-191 is the same with the full window and no flip).  `slots` holds
 * n slots of slot_stride bytes (a multiple of 64): a 64-byte header of int32 {mode, h0, w0, y0, x0, flip, 0...} followed by
 * the h0 x w0 x channels bytes of the image (mode 0; y0 / x0 = the crop's corner in the RESIZED image) or by the finished
 * float32 crop (mode 1: copied from byte 64; a crop that does not fit the slot reads 0).  out is [n, crop_h, crop_w, channels]
 * float32; every value is bit-equal to the host transform (tf_face_toolbox_amd/_decode_worker.py).  The random draws stay on the
 * host (they are the workers' seeded draws).  This entry and the three below are csrc/loader.hip: one header decode (SlotHeader),
 * one bilinear tap, one colour tail and one mode-1 copy serve the 64-byte-header entries; the aligned entry shares the colour tail. */
int fte_preprocess_u8(const uint8_t* slots, float* out, int n, long slot_stride, int channels, int in_h, int in_w, int crop_h, int crop_w,
                      void* stream);
/* The same transform followed by the colour augmentation of preprocessing.py:22-38 of the reference (train.py --augmentation 1)
 * before the final (x - 0.5) / 0.5.  Same arguments, same refusals, same slots; the header words that fte_preprocess_u8 ignores
 * carry the worker's draws:
 *   hd[0..5]  {mode, h0, w0, y0, x0, flip}, as above
 *   hd[6]     flag bits: 1 = brightness, 2 = hue, 4 = saturation (the host's `draw < 0.1 / 0.2 / 1.0` decisions, taken in float64)
 *   hd[7]     float32 bits of the brightness delta   (x - delta; no clip of its own)
 *   hd[8]     float32 bits of the hue delta          (clip to [0, 1], RGB -> HSV, h = (h - delta) mod 1, HSV -> RGB)
 *   hd[9]     float32 bits of the saturation factor  (clip to [0, 1], RGB -> HSV, s = clip(s * factor, 0, 1), HSV -> RGB)
 *   hd[10..15] 0
 * Words 6..9 steer arithmetic only, never an address.  channels == 1: bits 2 and 4 are ignored.  Mode 1 slots hold the crop the
 * worker finished, augmentation included, and are copied.  With hd[6] == 0 the output is fte_preprocess_u8's; every value is
 * bit-equal to the host transform with augmentation = 1 (tf_face_toolbox_amd/preprocessing.py, float32 element by element). */
int fte_preprocess_u8_aug(const uint8_t* slots, float* out, int n, long slot_stride, int channels, int in_h, int in_w, int crop_h,
                          int crop_w, void* stream);
/* The same transform with the geometric pair of preprocessing.py:41-71 of the reference (train.py --augmentation 2 | 3) between
 * the crop and the flip: resize + crop, ZOOM, AFFINE, flip, colour (words 6..9, as above), (x - 0.5) / 0.5.  Same slots, same
 * arguments and refusals as fte_preprocess_u8_aug, plus FTE_EINVAL for a null affine_table and FTE_EWORKSPACE for a workspace
 * smaller than fte_preprocess_u8_geo_ws_bytes() (0 when an image's two float planes fit in LDS).  Further header words:
 *   hd[6]     bit 8 = zoom applied ((th, tw) != (crop_h, crop_w)), bit 16 = affine
 *   hd[10..11] th, tw: the zoom's target shape     hd[12] rnd: row of affine_table     hd[13..15] 0
 * affine_table: device copy of preprocessing.AFFINE_TABLE, float32 [729][6] = (a0, a1, a2, b0, b1, b2).
 *   ZOOM    I = resize(resize(I, th, tw), crop_h, crop_w), both the TF-1.x bilinear of fte_preprocess_u8 on floats:
 *           in = out * (n_in / n_out), lo = floor(in), hi = min(lo + 1, n_in - 1), blended along x, then along y.
 *   AFFINE  output pixel (x, y), coordinates of the crop BEFORE the flip, reads
 *           sx = (a0 x + a1 y) + a2, sy = (b0 x + b1 y) + b2;  fx = floor(sx), fy = floor(sy), cx = fx + 1, cy = fy + 1;
 *           top = (cx - sx) R(fy, fx) + (sx - fx) R(fy, cx);  bot = (cx - sx) R(cy, fx) + (sx - fx) R(cy, cx);
 *           out = (cy - sy) top + (sy - fy) bot;  R = 0 outside the image  (tf.contrib.image.transform, 'BILINEAR').
 * Every operation is float32 and rounds on its own.  Words 10..12 steer addresses and are NOT trusted: th outside [1, crop_h] or
 * tw outside [1, crop_w] -> bit 8 is taken as clear; rnd outside [0, 728] -> bit 16 is taken as clear; every tap of the two
 * resizes is clamped into its plane and the warp's zero fill is decided on the float coordinates (a NaN reads 0).  Mode 1 slots
 * are copied.  With neither bit the output is fte_preprocess_u8_aug's; every value is bit-equal to the host transform with
 * augmentation = 2 | 3 (tf_face_toolbox_amd/preprocessing.py: zoom_in_out, affine_warp). */
size_t fte_preprocess_u8_geo_ws_bytes(int n, int channels, int crop_h, int crop_w);
int fte_preprocess_u8_geo(const uint8_t* slots, float* out, int n, long slot_stride, int channels, int in_h, int in_w, int crop_h,
                          int crop_w, const float* affine_table, void* ws, size_t ws_bytes, void* stream);
/* Five-point face alignment in place of the resize (train.py / evaluate.py --landmark_list_path): the aligned in_h x in_w image
 * is a similarity warp of the decoded image, and the stages are warp over the crop window, flip, colour (words 6..9, as
 * fte_preprocess_u8_aug; hd[6] == 0 is the identity, bits 8 and 16 are ignored), (x - 0.5) / 0.5.  Same arguments and refusals
 * as fte_preprocess_u8_aug (FTE_EINVAL: channels not 1 / 3, a crop larger than the input, a slot stride that is not a multiple
 * of 64 or smaller than the header).  An aligned slot has a 128-byte header:
 *   hd[0..15]  as fte_preprocess_u8_aug, with h0, w0 = the shape of the WINDOW of the decoded image that the slot carries
 *              (preprocessing.align_window: the bounding box of the aligned image's corners in the source, padded by 2 pixels
 *              and clamped to the image); y0 / x0 = the crop's corner in the ALIGNED image
 *   hd[16..21] float32 bits of m6 = (a0, a1, a2, b0, b1, b2): the inverse similarity, translation relative to the window's corner
 *   hd[22..31] 0
 * followed by the window's h0 x w0 x channels bytes (mode 0) or the finished float32 crop (mode 1: copied from byte 128; a crop
 * that does not fit the slot reads 0).  Output pixel (x, y), coordinates of the aligned image BEFORE the flip, reads
 *   sx = (a0 x + a1 y) + a2, sy = (b0 x + b1 y) + b2;  fx = floor(sx), fy = floor(sy), cx = fx + 1, cy = fy + 1;
 *   top = (cx - sx) R(fy, fx) + (sx - fx) R(fy, cx);  bot = (cx - sx) R(cy, fx) + (sx - fx) R(cy, cx);
 *   out = (cy - sy) top + (sy - fy) bot;  R = byte * (1 / 255) inside the window, 0 outside;
 *   a pixel NONE of whose four taps lies inside the window is 0 (the formula's own value for finite coordinates).
 * Every operation is float32 and rounds on its own.  Words 16..21, h0 and w0 steer addresses and are NOT trusted: whether a tap
 * lies inside [0, w0 - 1] x [0, h0 - 1] is decided on the float coordinates before any conversion to int (a NaN, an infinity or
 * an out-of-range value reads 0, so such a pixel is 0 and the output -1), the converted index is clamped into the window, and
 * with h0 < 1, w0 < 1 or h0 * w0 * channels > slot_stride - 128 every tap reads 0.  y0, x0 and flip only enter arithmetic.
 * Every value is bit-equal to the host aligned transform (tf_face_toolbox_amd/preprocessing.py: align_window, align_warp). */
int fte_preprocess_u8_align(const uint8_t* slots, float* out, int n, long slot_stride, int channels, int in_h, int in_w, int crop_h,
                            int crop_w, void* stream);

/* Raw slots from a pre-decoded image pack that is RESIDENT in device memory (tf_face_toolbox_amd/packs.py; train.py / evaluate.py
 * --packed_data_path P --pack_on_gpu 1).  `rows` holds num_rows rows of row_stride bytes (the pack's uint8 images, zero padded to
 * a multiple of 64), `headers` n slot headers of 64 bytes (the workers' draws, mode 0, h0 x w0 = the pack's image shape),
 * `index` n int64 pack rows.  For i < n:
 *   slots[i * slot_stride .. + 64)              = headers[64 i .. + 64)
 *   slots[i * slot_stride + 64 .. + row_stride) = rows[r * row_stride .. + row_stride),  r = clamp(index[i], 0, num_rows - 1)
 * -- the slots fte_preprocess_u8 / _aug / _geo read (csrc/loader.hip: pack_gather_slots_kernel).  The index is device data and is NOT trusted: it is clamped, never used raw
 * (the loader validates its own indices on the host as well).  Bytes of a slot beyond 64 + row_stride are not written.  Every
 * byte offset is 64-bit: r * row_stride passes 2^32 for real packs.  A plain copy in 16-byte chunks by a bounded grid; no
 * workspace, no atomics, two calls write identical bytes.  FTE_EINVAL, with nothing launched: a null pointer, n < 1,
 * num_rows < 1, row_stride < 64 or not a multiple of 64, slot_stride not a multiple of 64 or below 64 + row_stride, rows /
 * headers / slots not 16-byte aligned (index: 8). */
int fte_pack_gather_slots(const uint8_t* rows, long num_rows, long row_stride, const int64_t* index, const uint8_t* headers,
                          uint8_t* slots, int n, long slot_stride, void* stream);

/* ---------------------------------------------------------------------------
 * layers.batch_norm(scale=True, center=True, fused=True, decay=0.999, epsilon=1e-3) in TRAINING mode
 * (nets/resnet.py:97-99; FusedBatchNorm / FusedBatchNormGrad).  z is [rows, c] (NHWC flattened).
 *   fwd: mean/var over the rows of THIS shard (biased var normalises; the moving variance gets the unbiased
 *        one), y = [relu](gamma*(z-mean)*rstd + beta [+ res]);  mean, rstd, scale, shift are kept for backward;
 *        moving_mean / moving_var may be NULL (replicas other than tower 0, data_parallel.py:242-243).
 *   bwd: g = dy * (ymask > 0) when ymask != NULL (the ReLU that followed), dgamma = sum g*xhat, dbeta = sum g,
 *        dz = gamma*rstd*(g - dbeta/rows - xhat*dgamma/rows).
 * ws >= fte_bn_ws_bytes(c).
 * ------------------------------------------------------------------------- */
size_t fte_bn_ws_bytes(int c);
int fte_bn_train_fwd(const float* z, const float* gamma, const float* beta, const float* res, float* y,
                     float* mean, float* rstd, float* scale, float* shift, float* moving_mean, float* moving_var,
                     long rows, int c, float eps, float decay, int relu, void* ws, size_t ws_bytes, void* stream);
int fte_bn_infer_fwd(const float* z, const float* gamma, const float* beta, const float* moving_mean,
                     const float* moving_var, const float* res, float* y, float* scale, float* shift,
                     long rows, int c, float eps, int relu, void* stream);
int fte_bn_train_bwd(const float* dy, const float* ymask, const float* z, const float* gamma, const float* mean,
                     const float* rstd, float* dz, float* dgamma, float* dbeta, long rows, int c,
                     void* ws, size_t ws_bytes, void* stream);
/* The same backward pass with the ReLU mask recomputed from z: g = dy * (fma(z, scale, shift) > 0) with the scale / shift
 * the forward pass kept -- the expression the forward kernels evaluate, so the mask is the forward's bit for bit and
 * the normalised activation is not read (nor need it exist: fte_channel_gather_affine). */
int fte_bn_train_bwd_zmask(const float* dy, const float* z, const float* gamma, const float* mean, const float* rstd,
                           const float* scale, const float* shift, float* dz, float* dgamma, float* dbeta, long rows, int c,
                           void* ws, size_t ws_bytes, void* stream);
/* Residual blocks (BN -> add shortcut -> ReLU, nets/resnet.py:97-112): g = dy * (y > 0) is needed twice, by the shortcut and by
 * this BN's backward.  The reduce pass writes it to g_out as a by-product and the apply pass reads it back -- no separate
 * fte_relu_bwd launch (3 tensor passes).  Bit-identical to fte_relu_bwd followed by fte_bn_train_bwd without a mask. */
int fte_bn_train_bwd_res(const float* dy, const float* y, const float* z, const float* gamma, const float* mean, const float* rstd,
                         float* g_out, float* dz, float* dgamma, float* dbeta, long rows, int c,
                         void* ws, size_t ws_bytes, void* stream);
/* The two halves of fte_bn_train_fwd / fte_bn_infer_fwd without the apply pass: batch statistics -> mean, rstd,
 * scale = gamma*rstd, shift = beta - mean*scale (+ the moving statistics), and the inference coefficients from the
 * moving statistics.  For consumers that apply scale / shift themselves (fte_channel_gather_affine). */
int fte_bn_train_stats(const float* z, const float* gamma, const float* beta, float* mean, float* rstd, float* scale, float* shift,
                       float* moving_mean, float* moving_var, long rows, int c, float eps, float decay,
                       void* ws, size_t ws_bytes, void* stream);
int fte_bn_infer_coef(const float* gamma, const float* beta, const float* moving_mean, const float* moving_var,
                      float* scale, float* shift, int c, float eps, void* stream);
/* ---------------------------------------------------------------------------
 * BN + PReLU: batch norm followed by a per-channel PReLU in one pass (the IResNet block, nets/iresnet.py).  fp32 tensors only,
 * z / y / dy / dz are [rows, c], c % 4 == 0; alpha / dalpha are [c].  With u = fma(z, scale[c], shift[c]) -- the expression
 * fte_bn_apply evaluates, scale / shift from fte_bn_train_stats, fte_conv2d_bn_fwd or fte_bn_infer_coef:
 *   fte_bn_prelu_apply      y = u > 0 ? u : alpha[c] * u  (the PReLU of the conv epilogues; the product is rounded on its own, so
 *                           alpha = 1 gives the bytes of fte_bn_apply(relu = 0) and alpha = 0 the values of fte_bn_apply(relu = 1)).
 *   fte_bn_prelu_infer_fwd  fte_bn_infer_coef (scale / shift from the moving statistics, written for the caller) followed by
 *                           fte_bn_prelu_apply: two launches.
 *   fte_bn_prelu_train_bwd  the sign of u is recomputed from z exactly as the forward evaluated it (the activated tensor is not read):
 *                           g = dy * (u > 0 ? 1 : alpha[c]),  dalpha[c] = sum_{u <= 0} dy * u,  dgamma = sum g * xhat,  dbeta = sum g,
 *                           dz = gamma * rstd * (g - dbeta / rows - xhat * dgamma / rows).
 *                           Two passes over (dy, z): a split reduce with three sums per channel, then the apply.  The sums are fp32,
 *                           merged in a fixed order without float atomics: two calls write identical bytes.
 *                           ws >= fte_bn_prelu_ws_bytes(c).
 * FTE_EINVAL: a null pointer, rows < 1, c < 4 or c % 4, ws NULL or shorter than fte_bn_prelu_ws_bytes(c).  Nothing is launched then.
 * ------------------------------------------------------------------------- */
size_t fte_bn_prelu_ws_bytes(int c);
int fte_bn_prelu_apply(const float* z, const float* scale, const float* shift, const float* alpha, float* y, long rows, int c,
                       void* stream);
int fte_bn_prelu_infer_fwd(const float* z, const float* gamma, const float* beta, const float* moving_mean, const float* moving_var,
                           const float* alpha, float* y, float* scale, float* shift, long rows, int c, float eps, void* stream);
int fte_bn_prelu_train_bwd(const float* dy, const float* z, const float* gamma, const float* mean, const float* rstd,
                           const float* scale, const float* shift, const float* alpha, float* dz, float* dgamma, float* dbeta,
                           float* dalpha, long rows, int c, void* ws, size_t ws_bytes, void* stream);
/* ---------------------------------------------------------------------------
 * BN + SE + shortcut, no activation: the tail of an SE-IResNet block (nets/iresnet.py with se=True),
 *   z -> u = BN(z) -> out = u * gate(mean_hw u) + shortcut.
 * fp32 tensors only: z / shortcut / out / dy are [n, hw, c], c % 4 == 0, c >= 4; sq / xm / gate / s1 / s2 / dgate are [n, c].  scale /
 * shift / mean / rstd are the BN layer's (fte_bn_train_stats, fte_conv2d_bn_fwd or fte_bn_infer_coef); u = fma(z, scale[c], shift[c]) as
 * fte_bn_apply evaluates it, xhat = (z - mean) * rstd.
 *   fte_se_lin_squeeze    sq = scale * mean_hw(z) + shift; xm (optional) = (mean_hw(z) - mean) * rstd: the values of fte_se_squeeze.
 *   fte_se_lin_apply_fwd  out = u * gate[n, c] + shortcut, no clamp.  Product and sum are rounded on their own: gate = 1 gives the
 *                         bytes of fte_bn_apply(res = shortcut, relu = 0).
 *   fte_se_lin_bwd_sums   s1 = sum_hw dy, s2 = sum_hw dy * xhat, dgate = (gamma * s2 + beta * s1) * gate * (1 - gate) (the gradient of
 *                         the gate's pre-sigmoid).  Reads dy and z only: no output tensor is read, no masked gradient is written.
 * The rest of the backward is fte_se_bn_bwd_coef and fte_se_bn_bwd_apply with g = dy and flags = 0; dy itself is the shortcut's gradient.
 * The two reductions split the pixels of an image over S blocks when ceil(c / 64) * n blocks cannot give every compute unit of the
 * device one (S from the device's CU count, at most 64); the partial sums go to ws and are added in split order by a small second
 * launch.  S = 1 writes the results from the one launch.  Sums are fp32 and merged in a fixed order without float atomics: two calls
 * write identical bytes.  ws >= fte_se_lin_ws_bytes(n, hw, c) (0 for a shape the entry points refuse).
 * FTE_EINVAL: a null pointer (xm excepted; mean / rstd may be NULL without xm), n < 1, hw < 1, c < 4 or c % 4, ws NULL or shorter than
 * fte_se_lin_ws_bytes(n, hw, c), n > 65535 or hw * c >= 2^32.  Nothing is launched then.
 * ------------------------------------------------------------------------- */
size_t fte_se_lin_ws_bytes(int n, int hw, int c);
int fte_se_lin_squeeze(const float* z, const float* scale, const float* shift, const float* mean, const float* rstd, float* sq, float* xm,
                       int n, int hw, int c, void* ws, size_t ws_bytes, void* stream);
int fte_se_lin_apply_fwd(const float* z, const float* scale, const float* shift, const float* gate, const float* shortcut, float* out,
                         int n, int hw, int c, void* stream);
int fte_se_lin_bwd_sums(const float* dy, const float* z, const float* gamma, const float* beta, const float* mean, const float* rstd,
                        const float* gate, float* s1, float* s2, float* dgate, int n, int hw, int c, void* ws, size_t ws_bytes, void* stream);
/* g = dy * (y > 0)  (tf.nn.relu gradient, materialised where a residual shortcut needs it) */
int fte_relu_bwd(const float* dy, const float* y, float* g, long n, void* stream);

/* layers.max_pool2d(kernel 3, stride 2, 'SAME') (nets/resnet.py:115); idx keeps the window position of
 * the first maximum (uint8 per element) for the gradient. */
int fte_maxpool3x3s2_fwd(const float* x, float* y, uint8_t* idx, int n, int h, int wd, int c, void* stream);
int fte_maxpool3x3s2_bwd(const float* dy, const uint8_t* idx, float* dx, int n, int h, int wd, int c, void* stream);
/* tf.reduce_mean over the spatial axes (nets/resnet.py:142) */
int fte_gap_fwd(const float* x, float* y, int n, int hw, int c, void* stream);
int fte_gap_bwd(const float* dy, float* dx, int n, int hw, int c, void* stream);
/* layers.dropout(keep_prob) (nets/resnet.py:152): mask = U(seed, i) < keep, y = x*mask/keep */
int fte_dropout_fwd(const float* x, float* mask, float* y, long n, float keep_prob, uint64_t seed, void* stream);
int fte_dropout_bwd(const float* dy, const float* mask, float* dx, long n, float keep_prob, void* stream);

/* ---------------------------------------------------------------------------
 * Grouped 3x3 convolution: ONE kernel for the tf.split / 32 x layers.conv2d / tf.concat of
 * nets/resnext.py:41-51.  x [n,h,wd,c], w [groups][3][3][c/groups][c/groups] (the reference's 32 HWIO
 * variables `conv2_3x3_group_<i>/weights` stacked), c/groups in {4,8,16,32}, TF-SAME, stride 1 or 2.
 * ------------------------------------------------------------------------- */
int fte_gconv3x3_fwd(const float* x, const float* w, float* y, int n, int h, int wd, int c, int groups,
                     int stride, void* stream);
/* bf16 MFMA mode: the grouped 3x3 on the matrix cores.  A 32-channel slice (32 / gw whole groups) is a dense 3x3 conv 32 -> 32
 * with a block-diagonal filter; fte_gconv3x3_pack_bf16 builds that filter (bf16, k-contiguous) for the forward pass and --
 * mirrored and transposed -- for the data gradient.  fte_gconv3x3_bf16(x, wpk_fwd, y, ..., dgrad = 0) = forward,
 * fte_gconv3x3_bf16(dz, wpk_dgrad, dx, ..., dgrad = 1) = data gradient; n, h, wd are the FORWARD layer's input size in both,
 * TF-SAME, stride 1 or 2.  Operands rounded to bf16 (RNE), fp32 accumulate, fp32 tensors.
 * wpk_*: (c / 32) * 9 * 1024 uint16.  gw = c / groups in {4, 8, 16, 32}, c % 32 == 0. */
int fte_gconv3x3_pack_bf16(const float* w, uint16_t* wpk_fwd, uint16_t* wpk_dgrad, int c, int groups, void* stream);
int fte_gconv3x3_bf16(const float* x, const uint16_t* wpk, float* y, int n, int h, int wd, int c, int stride, int dgrad, void* stream);
/* ... and the filter gradient of those layers: per slice and tap a [32 ic] x [32 oc] product over the pixels (operands rounded to
 * bf16, fragments transposed out of LDS by ds_read_b64_tr_b16), ordered partials in ws, the groups' diagonal blocks summed into
 * dw [groups][3][3][gw][gw]. */
size_t fte_gconv3x3_wgrad_bf16_ws_bytes(int n, int h, int wd, int c, int groups, int stride);
int fte_gconv3x3_wgrad_bf16(const float* x, const float* dz, float* dw, int n, int h, int wd, int c, int groups, int stride,
                            void* ws, size_t ws_bytes, void* stream);
int fte_gconv3x3_dgrad(const float* dz, const float* w, float* dx, int n, int h, int wd, int c, int groups,
                       int stride, void* stream);
int fte_gconv3x3_wgrad(const float* x, const float* dz, float* dw, int n, int h, int wd, int c, int groups,
                       int stride, void* ws, size_t ws_bytes, void* stream);
size_t fte_gconv3x3_wgrad_ws_bytes(int n, int h, int wd, int c, int groups, int stride);

/* Squeeze-excitation gate pieces (nets/shufflenet_v2.py:79-85): activations kind 0 = ReLU, 1 = sigmoid
 * (bwd takes the OUTPUT y), and the per-(image, channel) scale y = x * gate[n,c] with its gradients
 * dx = dy*gate, dgate[n,c] = sum_hw dy*x.  The two 1x1 convs on the pooled vector are fte_gemm_*. */
/* dx[n,hw,c] += v[n,c]*scale: the squeeze (spatial mean) gradient broadcast back over the map */
int fte_bcast_add(float* dx, const float* v, int n, int hw, int c, float scale, void* stream);
/* The gate's dense layers in ONE launch each (fte_gemm_* make two: split-K + reduction, 12-15 us for these sizes):
 * out[m, n] = act(a[m, k] * op(w) + bias) [* (mask > 0)], op(w) = w[k][n] (trans_w = 0: layers.fully_connected forward) or w[n][k]^T
 * (trans_w = 1: the gradient w.r.t. the layer's input); act 0 none, 1 ReLU, 2 sigmoid; bias [n] and mask [m, n] optional (mask: the ReLU
 * gradient of the layer below, tf.nn.relu's grad).  n % 32 == 0, k % 128 == 0.  Operand precision follows fte_set_mfma_dtype. */
int fte_dense_small(const float* a, const float* w, const float* bias, const float* mask, float* out, int m, int n, int k,
                    int trans_w, int act, void* stream);
int fte_act_fwd(const float* x, float* y, long n, int kind, void* stream);
int fte_act_bwd(const float* dy, const float* y, float* dx, long n, int kind, void* stream);
int fte_channel_scale_fwd(const float* x, const float* gate, float* y, int n, int hw, int c, void* stream);
/* pre_sigmoid != 0: dgate is multiplied by gate * (1 - gate), i.e. it is the gradient w.r.t. the pre-sigmoid value */
int fte_channel_scale_bwd(const float* dy, const float* x, const float* gate, float* dx, float* dgate,
                          int n, int hw, int c, int pre_sigmoid, void* stream);

/* ---------------------------------------------------------------------------
 * bf16 OPERAND COPIES (mixed precision with bf16 storage of what the MFMAs read; BASELINE.json config 3).
 * The *16 convolutions read bf16 copies of their two operands -- half the bytes per K-step through the load path, no
 * conversion in the loop -- and can write a bf16 copy of their result for the next consumer; everything else (fp32
 * accumulation, bias / PReLU / residual / PReLU-gradient epilogues, the fp32 result tensors, reductions) is unchanged.
 * Results are bit-identical to the FTE_MFMA_BF16 mode of the fp32-source entry points (same rounding, same order).
 *   fte_to_bf16            y16[i] = bf16(x[i]) (round to nearest even), n % 4 == 0
 *   fte_pack_weights_bf16  w [k*k][cin][cout] (HWIO) -> w16 (same layout: dgrad's operand) and / or w16t [k*k][cout][cin]
 *                          (forward's operand); once per optimizer step
 *   fte_conv2d_fwd16       = fte_conv2d_fwd with x16, w16t; y16 (optional) receives bf16(y)
 *   fte_conv2d_dgrad16     = fte_conv2d_dgrad with dz16, w16; dzprev16 (optional) receives bf16(dzprev)
 *   fte_conv2d_wgrad16     = fte_conv2d_wgrad with x16, dz16 (cin % 8 == 0)
 * Workspace sizes are those of the fp32-source functions.
 * ------------------------------------------------------------------------- */
int fte_to_bf16(const float* x, uint16_t* y16, long n, void* stream);
int fte_pack_weights_bf16(const float* w, uint16_t* w16, uint16_t* w16t, int ksize, int cin, int cout, void* stream);
/* every filter of a net in ONE launch per layout (a step of a 50-layer net made 36-53 pack launches of ~7 us otherwise): `table` is a
 * DEVICE array of nconv <= 64 rows {source offset in `params` (floats), destination offset in `dst` (bf16 elements, a multiple of 8),
 * taps, cin, cout, first index of this conv in the flattened walk / 4}, cin % 4 == 0 and cout % 4 == 0, total = sum of
 * taps*cin*cout.  transposed = 1 writes the [tap][cout][cin] packs (forward), 0 the HWIO packs (data gradient). */
int fte_pack_weights_bf16_table(const float* params, uint16_t* dst, const int32_t* table, int nconv, long total, int transposed, void* stream);
int fte_conv2d_fwd16(const uint16_t* x16, const uint16_t* w16t, const float* bias, const float* alpha, const float* res,
                     float* z, float* y, uint16_t* y16, int n, int h, int wd, int cin, int cout, int ksize, int stride,
                     void* ws, size_t ws_bytes, void* stream);
int fte_conv2d_dgrad16(const uint16_t* dz16, const uint16_t* w16, const float* addin, const float* zprev,
                       const float* alpha_prev, float* raw, float* dzprev, uint16_t* dzprev16, float* dalpha_prev,
                       float* dbias_prev, int n, int h, int wd, int cin, int cout, int ksize, int stride,
                       void* ws, size_t ws_bytes, void* stream);
int fte_conv2d_wgrad16(const uint16_t* x16, const uint16_t* dz16, float* dw, int n, int h, int wd, int cin, int cout,
                       int ksize, int stride, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------
 * bf16 STORAGE (the third precision contract, next to fp32 and "bf16 operands, fp32 tensors"; BASELINE.json config 3's
 * precision, SURVEY.md section 7 step 8 "bf16 storage path, fp32 master weights").  The activations the backward pass keeps -- z, y -- and the
 * gradients that travel between layers -- dz, and the skip-path gradient `raw` -- live in HBM as bf16 ONLY: the epilogues
 * move 6-8 bytes per output element instead of 10-18.  Arithmetic is unchanged: fp32 accumulation, fp32 bias / PReLU /
 * residual / PReLU-gradient math, fp32 dalpha / dbias / filter gradients, fp32 master weights and optimizer.  Every stored
 * value is rounded exactly once, to nearest even, where it is written; every consumer sees the rounded value:
 *   y16  = bf16( prelu(acc + bias) + float(res16) )       z16 = bf16( acc + bias )
 *   g    = acc + float(addin16)        raw16 = bf16(g)     dz = g * prelu'(float(zprev16))      dzprev16 = bf16(dz)
 *   dalpha = sum g * min(float(zprev16), 0)                dbias = sum dz                       (fp32 sums of unrounded terms)
 * oracle/ops.py storage_rounding('bf16') rounds at the same points (tests/test_gpu_bf16_storage.py).
 *   fte_conv2d_fwd_s16          as fte_conv2d_fwd16 with a bf16 shortcut, bf16 z / y outputs; z32 / y32 (optional) also
 *                               receive the unrounded fp32 values (the last conv layer, whose consumer is the dense layer)
 *   fte_conv2d_dgrad_s16        as fte_conv2d_dgrad16 with bf16 skip gradient / z inputs and bf16 raw / dz outputs
 *   fte_conv3x3_first_fwd_s16   the first layer (fp32 images in, bf16 z / y out)
 *   fte_conv3x3_first_wgrad_s16 its filter gradient from a bf16 dz
 * The filter gradient of every other layer is fte_conv2d_wgrad16 (bf16 x and dz in, fp32 dw out).
 * ------------------------------------------------------------------------- */
int fte_conv2d_fwd_s16(const uint16_t* x16, const uint16_t* w16t, const float* bias, const float* alpha, const uint16_t* res16,
                       uint16_t* z16, uint16_t* y16, float* z32, float* y32, int n, int h, int wd, int cin, int cout,
                       int ksize, int stride, void* ws, size_t ws_bytes, void* stream);
int fte_conv2d_dgrad_s16(const uint16_t* dz16, const uint16_t* w16, const uint16_t* addin16, const uint16_t* zprev16,
                         const float* alpha_prev, uint16_t* raw16, uint16_t* dzprev16, float* dalpha_prev, float* dbias_prev,
                         int n, int h, int wd, int cin, int cout, int ksize, int stride, void* ws, size_t ws_bytes, void* stream);
int fte_conv3x3_first_fwd_s16(const float* x, const float* w, const float* bias, const float* alpha, uint16_t* z16, uint16_t* y16,
                              int n, int h, int wd, int cin, int cout, int stride, void* stream);
int fte_conv3x3_first_wgrad_s16(const float* x, const uint16_t* dz16, float* dw, int n, int h, int wd, int cin, int cout, int stride,
                                void* ws, size_t ws_bytes, void* stream);

/* bf16 STORAGE for the BN nets (nets/resnet.py, nets/resnext.py: BASELINE.json configs[2] "bf16").  Same contract as above: the
 * tensors between the layers are bf16 in HBM, every kernel computes in fp32 and rounds once where it stores.  `flags` says which
 * tensors of a call are bf16: FTE_S16_Z = the pre-activation side (z, and dz in backward), FTE_S16_A = the activation side (y, the
 * shortcut `res`, dy, the masked gradient g_out); the other side is fp32 (the stem, whose conv output comes from an fp32 GEMM).
 * Pointers are void*: bf16 (uint16_t) or float elements per the flags.  c % 4 == 0 and c >= 32.
 *   fte_bn_train_fwd_s16 / fte_bn_infer_fwd_s16   = fte_bn_train_fwd / fte_bn_infer_fwd
 *   fte_bn_train_bwd_s16   the three backward forms in one: g_out + y given = the residual form (fte_bn_train_bwd_res), scale + shift
 *                          given = the ReLU mask recomputed from z (fte_bn_train_bwd_zmask), neither = fte_bn_train_bwd (y = optional mask)
 *   fte_relu_bwd_s16, fte_maxpool3x3s2_{fwd,bwd}_s16, fte_gap_{fwd,bwd}_s16 (features / their gradient stay fp32)
 *   fte_gconv3x3_bf16_s16, fte_gconv3x3_wgrad_bf16_s16   the grouped 3x3 on the bf16 MFMA with bf16 x / y / dz in HBM (dw fp32) */
#define FTE_S16_Z 1
#define FTE_S16_A 2
int fte_bn_train_fwd_s16(const void* z, const float* gamma, const float* beta, const void* res, void* y,
                         float* mean, float* rstd, float* scale, float* shift, float* moving_mean, float* moving_var,
                         long rows, int c, float eps, float decay, int relu, int flags, void* ws, size_t ws_bytes, void* stream);
int fte_bn_infer_fwd_s16(const void* z, const float* gamma, const float* beta, const float* moving_mean, const float* moving_var,
                         const void* res, void* y, float* scale, float* shift, long rows, int c, float eps, int relu, int flags, void* stream);
int fte_bn_train_bwd_s16(const void* dy, const void* y, const void* z, const float* gamma, const float* mean, const float* rstd,
                         const float* scale, const float* shift, void* g_out, void* dz, float* dgamma, float* dbeta,
                         long rows, int c, int flags, void* ws, size_t ws_bytes, void* stream);
int fte_relu_bwd_s16(const uint16_t* dy16, const uint16_t* y16, uint16_t* g16, long n, void* stream);
int fte_maxpool3x3s2_fwd_s16(const uint16_t* x16, uint16_t* y16, uint8_t* idx, int n, int h, int wd, int c, void* stream);
int fte_maxpool3x3s2_bwd_s16(const uint16_t* dy16, const uint8_t* idx, uint16_t* dx16, int n, int h, int wd, int c, void* stream);
int fte_gap_fwd_s16(const uint16_t* x16, float* y, int n, int hw, int c, void* stream);
int fte_gap_bwd_s16(const float* dy, uint16_t* dx16, int n, int hw, int c, void* stream);
int fte_gconv3x3_bf16_s16(const uint16_t* x16, const uint16_t* wpk, uint16_t* y16, int n, int h, int wd, int c, int stride, int dgrad, void* stream);
int fte_gconv3x3_wgrad_bf16_s16(const uint16_t* x16, const uint16_t* dz16, float* dw, int n, int h, int wd, int c, int groups, int stride,
                                void* ws, size_t ws_bytes, void* stream);
/* ---------------------------------------------------------------------------
 * BN FUSION: the conv -> batch_norm (-> ReLU) pairs of nets/resnet.py:47-61 (`conv_bn_relu`), nets/resnext.py:34-67,
 * nets/shufflenet_v2.py:120-135.  TF runs Conv2D, FusedBatchNorm (statistics pass + normalise pass) and Relu as separate
 * kernels, and FusedBatchNormGrad re-reads dy and x for its two sums; here the PRODUCING kernel leaves those per-channel
 * sums behind, so each BN tensor makes one HBM round trip less in each direction:
 *   forward   the conv epilogue keeps (n, mean, M2) of the values it stores -- per tile row and channel, Chan-merged, no
 *             E[x^2] - E[x]^2 -- in `ws`; one finalize launch merges the tile rows in a fixed order -> mean, rstd (biased batch
 *             variance, eps inside the root), scale = gamma * rstd, shift = beta - mean * scale, moving statistics (decay, unbiased
 *             variance) exactly as fte_bn_train_stats.  The caller normalises with fte_bn_apply (or the consumer folds it in).
 *   backward  the data gradient that lands on the BN layer's OUTPUT applies the ReLU mask in its epilogue, stores the masked gradient
 *             g and leaves sum g, sum g * xhat per tile row; one finalize launch -> dgamma, dbeta and coef[3 c] = (A, B, C0) of
 *             dz = A g + B z + C0, which fte_bn_bwd_apply evaluates (one read of g and z, one write of dz).
 *             mask:  bn_scale / bn_shift given -> fma(zbn, scale, shift) > 0, the expression the forward pass evaluated (BN + ReLU);
 *                    ybn given -> ybn > 0, ybn = the stored output of BN + add + ReLU (g is then also the shortcut's gradient);
 *                    neither -> no mask (BN without activation).
 * s16 = 0: fp32 tensors (w: HWIO fp32);  s16 = 1: bf16 storage -- x / dz / addin / zbn / ybn / z / g are bf16, w is the bf16 pack
 * (forward: [tap][cout][cin], data gradient: HWIO; fte_pack_weights_bf16), and statistics / sums are taken of the ROUNDED values that
 * are stored.  Sums are fp32, deterministic (fixed merge order, no atomics).  Shapes as fte_conv2d_fwd / fte_conv2d_dgrad.
 * The grouped 3x3 twins run on the bf16 MFMA with bf16 tensors (4 / 8 / 16 / 32 channels per group, c % 32 == 0).
 * ------------------------------------------------------------------------- */
size_t fte_conv2d_bn_fwd_ws_bytes(int n, int h, int wd, int cin, int cout, int ksize, int stride);
/* in_scale / in_shift / y_side (all three or none): `x` is then the PRE-normalisation tensor of the batch norm IN FRONT of this conv
 * (conv -> BN -> ReLU -> conv chains); the operand loader applies y = relu(in_scale[k] * x + in_shift[k]) -- the expression and the
 * bf16 rounding of fte_bn_apply -- on the way to the matrix cores and writes the normalised rows to y_side, which only the filter
 * gradient reads: the fte_bn_apply launch between the two convs and its pass over the tensor disappear.  Taken by the streaming
 * pointwise kernel only: fte_conv2d_bn_fwd_folds() says whether a shape qualifies (bf16 storage, 1x1, stride 1, cin 64 / 128 / 256). */
int fte_conv2d_bn_fwd_folds(int n, int h, int wd, int cin, int cout, int ksize, int stride, int s16);
int fte_conv2d_bn_fwd(const void* x, const void* w, void* z, const float* gamma, const float* beta, float* mean, float* rstd,
                      float* scale, float* shift, float* moving_mean, float* moving_var, float eps, float decay,
                      const float* in_scale, const float* in_shift, void* y_side,
                      int n, int h, int wd, int cin, int cout, int ksize, int stride, int s16, void* ws, size_t ws_bytes, void* stream);
size_t fte_conv2d_dgrad_bn_ws_bytes(int n, int h, int wd, int cin, int cout, int ksize, int stride);
int fte_conv2d_dgrad_bn(const void* dz, const void* w, const void* addin, const void* zbn, const void* ybn,
                        const float* gamma, const float* mean, const float* rstd, const float* bn_scale, const float* bn_shift,
                        void* g, float* dgamma, float* dbeta, float* coef,
                        int n, int h, int wd, int cin, int cout, int ksize, int stride, int s16, void* ws, size_t ws_bytes, void* stream);
/* y = [relu](scale[c] * z + shift[c] [+ res]) with given coefficients; flags: FTE_S16_Z (z bf16), FTE_S16_A (res, y bf16) */
int fte_bn_apply(const void* z, const float* scale, const float* shift, const void* res, void* y, long rows, int c, int relu, int flags, void* stream);
/* dz = coef[c] * g + coef[C + c] * z + coef[2C + c], g already masked; flags: FTE_S16_Z (z, dz bf16), FTE_S16_A (g bf16) */
int fte_bn_bwd_apply(const void* g, const void* z, const float* coef, void* dz, long rows, int c, int flags, void* stream);
size_t fte_gconv3x3_bn_ws_bytes(int n, int h, int wd, int c, int stride);
/* (in_scale / in_shift / y_side as above; stride 1 only) */
int fte_gconv3x3_bn_fwd_bf16_s16(const uint16_t* x16, const uint16_t* wpk, uint16_t* z16, const float* gamma, const float* beta,
                                 float* mean, float* rstd, float* scale, float* shift, float* moving_mean, float* moving_var,
                                 float eps, float decay, const float* in_scale, const float* in_shift, uint16_t* y_side,
                                 int n, int h, int wd, int c, int stride, void* ws, size_t ws_bytes, void* stream);
int fte_gconv3x3_dgrad_bn_bf16_s16(const uint16_t* dz16, const uint16_t* wpk_dgrad, const uint16_t* zbn16, const float* gamma, const float* mean,
                                   const float* rstd, const float* bn_scale, const float* bn_shift, uint16_t* g16, float* dgamma, float* dbeta,
                                   float* coef, int n, int h, int wd, int c, int stride, void* ws, size_t ws_bytes, void* stream);

/* ShuffleNet-v2's layers on bf16 tensors (nets/shufflenet_v2.py): depthwise 3x3 forward / data gradient / filter gradient (fp32 filter
 * and dw), the channel gather and the gather with batch norm folded in (sources and results bf16, tables / scale / shift unchanged),
 * and the statistics-only pass of a folded batch norm (`flags` as above: FTE_S16_Z = z is bf16). */
/* the SE gate on bf16 tensors: y = x * gate; dgate = sum_hw dy * x (reduction only); dx = dy * gate + dsq * scale in ONE pass -- written
 * once, rounded once (gate, dgate, dsq are [n, c] fp32) */
int fte_channel_scale_fwd_s16(const uint16_t* x16, const float* gate, uint16_t* y16, int n, int hw, int c, void* stream);
int fte_channel_scale_bwd_s16(const uint16_t* dy16, const uint16_t* x16, const float* gate, float* dgate, int n, int hw, int c,
                              int pre_sigmoid, void* stream);
int fte_channel_scale_bwd_apply_s16(const uint16_t* dy16, const float* gate, const float* dsq, uint16_t* dx16, int n, int hw, int c,
                                    float scale, void* stream);
/* The SE residual block  z -> BN (no activation) -> y * gate(mean_hw y) -> + shortcut -> ReLU  (nets/resnet.py:63-92 with the gate of
 * nets/shufflenet_v2.py:79-85) in ONE pass over the tensor forward and TWO backward; the BN output and the gated tensor never exist
 * in HBM.  flags: bit 0 (FTE_S16_Z) z / dz are bf16, bit 1 (FTE_S16_A) shortcut / out / dy / g are bf16; gate, sq, xm, s1, s2, dgate, dsq
 * are [n, c] fp32; scale / shift / mean / rstd are the BN layer's (fte_conv2d_bn_fwd, fte_bn_train_stats, fte_bn_infer_coef).
 *   fte_se_squeeze       sq = scale * mean_hw(z) + shift (= mean_hw of the BN output); xm (optional) = (mean_hw(z) - mean) * rstd
 *   fte_se_apply_fwd     out = relu(fma(z, scale, shift) * gate + shortcut)
 *   fte_se_bwd_gate      g = dy * (out > 0) (the shortcut's gradient; stored, and the stored value is what is summed);
 *                        s1 = sum_hw g, s2 = sum_hw g * xhat, dgate = (gamma * s2 + beta * s1) * gate * (1 - gate) (w.r.t. the pre-sigmoid)
 *   fte_se_bn_bwd_coef   dsq = gradient of the squeeze (from the gate's dense layers): the batch-norm backward of
 *                        dy_bn = g * gate + dsq / hw from the per-image sums -- dbeta = sum_n (gate * s1 + dsq), dgamma = sum_n (gate * s2 +
 *                        dsq * xm), coef[3][c] of dz = A dy_bn + B z + C0 (FusedBatchNormGrad, nets/resnet.py:97-99)
 *   fte_se_bn_bwd_apply  dz = A * (g * gate + dsq / hw) + B * z + C0 */
int fte_se_squeeze(const void* z, const float* scale, const float* shift, const float* mean, const float* rstd, float* sq, float* xm,
                   int n, int hw, int c, int flags, void* stream);
int fte_se_apply_fwd(const void* z, const float* scale, const float* shift, const float* gate, const void* shortcut, void* out,
                     int n, int hw, int c, int flags, void* stream);
int fte_se_bwd_gate(const void* dy, const void* out, const void* z, const float* gamma, const float* beta, const float* mean,
                    const float* rstd, const float* gate, void* g, float* s1, float* s2, float* dgate, int n, int hw, int c, int flags, void* stream);
int fte_se_bn_bwd_coef(const float* s1, const float* s2, const float* gate, const float* dsq, const float* xm, const float* gamma,
                       const float* mean, const float* rstd, float* dgamma, float* dbeta, float* coef, int n, int hw, int c, void* stream);
int fte_se_bn_bwd_apply(const void* g, const void* z, const float* coef, const float* gate, const float* dsq, void* dz,
                        int n, int hw, int c, int flags, void* stream);
int fte_dwconv3x3_fwd_s16(const uint16_t* x16, const float* w, uint16_t* y16, int n, int h, int wd, int c, int stride, void* stream);
int fte_dwconv3x3_dgrad_s16(const uint16_t* dy16, const float* w, uint16_t* dx16, int n, int h, int wd, int c, int stride, void* stream);
int fte_dwconv3x3_wgrad_s16(const uint16_t* x16, const uint16_t* dy16, float* dw, int n, int h, int wd, int c, int stride,
                            void* ws, size_t ws_bytes, void* stream);
int fte_channel_gather_s16(const uint16_t* a, const uint16_t* b, uint16_t* out, const int32_t* table, long rows, int ca, int cb, int co, void* stream);
int fte_channel_gather_affine_s16(const uint16_t* a, const uint16_t* b, uint16_t* out, const int32_t* table, int co,
                                  uint16_t* out1, const int32_t* table1, int co1, long rows, int ca, int cb,
                                  const float* scale_a, const float* shift_a, int relu_a,
                                  const float* scale_b, const float* shift_b, int relu_b, void* stream);
int fte_bn_train_stats_s16(const void* z, const float* gamma, const float* beta, float* mean, float* rstd, float* scale, float* shift,
                           float* moving_mean, float* moving_var, long rows, int c, float eps, float decay, int flags,
                           void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------
 * ShuffleNet-v2 (nets/shufflenet_v2.py).  Depthwise 3x3, TF-SAME, stride 1 or 2: the DepthwiseConv2dNative half of
 * layers.separable_conv2d (:98,104; the pointwise half is fte_conv2d_* with ksize 1).  x [n,h,wd,c], w [3,3,c].
 * HBM-bound (9 MAC per element).
 * fte_channel_gather: out[row,k] = table[k] < 0 ? 0 : (table[k]>>16 ? b : a)[row, table[k] & 0xffff] -- one kernel
 * for _channel_split (:60-64), tf.concat + _channel_shuffle (:66-77,112-113) and their gradients; the
 * concatenated tensor is never materialised.  table is a device int32[co].
 * ------------------------------------------------------------------------- */
int fte_dwconv3x3_fwd(const float* x, const float* w, float* y, int n, int h, int wd, int c, int stride, void* stream);
int fte_dwconv3x3_dgrad(const float* dy, const float* w, float* dx, int n, int h, int wd, int c, int stride, void* stream);
int fte_dwconv3x3_wgrad(const float* x, const float* dy, float* dw, int n, int h, int wd, int c, int stride,
                        void* ws, size_t ws_bytes, void* stream);
size_t fte_dwconv3x3_wgrad_ws_bytes(int n, int h, int wd, int c, int stride);
int fte_channel_gather(const float* a, const float* b, float* out, const int32_t* table, long rows,
                       int ca, int cb, int co, void* stream);
/* The gather with batch norm applied to a source on the way: a source whose scale is not NULL contributes
 * [relu](fma(src[row,ch], scale[ch], shift[ch])).  conv3_1x1's BN + ReLU output (:110) and the stride-2 shortcut's (:96-101)
 * feed only the concat / shuffle / split: they are normalised inside the gather and never written to HBM.
 * out1 / table1 / co1 (optional, NULL / NULL / 0): a second output of the same two sources in the same launch -- the two
 * halves a block hands to the next one (forward), the gradients of the two sources (backward). */
int fte_channel_gather_affine(const float* a, const float* b, float* out, const int32_t* table, int co,
                              float* out1, const int32_t* table1, int co1, long rows, int ca, int cb,
                              const float* scale_a, const float* shift_a, int relu_a,
                              const float* scale_b, const float* shift_b, int relu_b, void* stream);

/* ---------------------------------------------------------------------------
 * First conv of the net (Cin = 1 or 3; nets/sphere.py:57, nets/shufflenet_v2.py:148-149): K = 9*Cin
 * is too short for a GEMM -- HBM-bound direct convolution, fused bias+PReLU (both optional).
 * cout = 64, or 32 for the 24-wide ShuffleNet-v2 stem stored 32 channels wide (w is [3,3,cin,cout]).
 * ------------------------------------------------------------------------- */
int fte_conv3x3_first_fwd(const float* x, const float* w, const float* bias, const float* alpha,
                          float* z, float* y, int n, int h, int wd, int cin, int cout,
                          int stride, void* stream);
int fte_conv3x3_first_wgrad(const float* x, const float* dz, float* dw,
                            int n, int h, int wd, int cin, int cout, int stride,
                            void* ws, size_t ws_bytes, void* stream);
size_t fte_conv3x3_first_wgrad_ws_bytes(int n, int h, int wd, int cin, int cout, int stride);

/* ---------------------------------------------------------------------------
 * Dense layers (MatMul + BiasAdd and their gradients: nets/sphere.py:73-74,
 * 86-90).  Row-major fp32; k % 32 == 0 for nn/nt, n % 64 == 0 everywhere.
 * ------------------------------------------------------------------------- */

/* y[m,n] = x[m,k] @ w[k,n] (+ bias[n]) */
int fte_gemm_nn(const float* x, const float* w, const float* bias, float* y,
                int m, int n, int k, void* ws, size_t ws_bytes, void* stream);
/* the same followed by an activation in the same pass over y: act 0 none, 1 ReLU, 2 sigmoid (the squeeze-excitation gate's two dense
 * layers, nets/shufflenet_v2.py:79-85; y = act(x @ w + bias)) */
int fte_gemm_nn_act(const float* x, const float* w, const float* bias, float* y,
                    int m, int n, int k, int act, void* ws, size_t ws_bytes, void* stream);
/* dx[m,k] = dy[m,n] @ w[k,n]^T, with the same fused PReLU-gradient epilogue as
 * fte_conv3x3_dgrad (zprev has dx's shape; alpha_prev has `amod` entries and
 * column j uses alpha_prev[j % amod] -- the flattened H*W*C feature map that
 * feeds nets/sphere.py:72-74). */
int fte_gemm_nt(const float* dy, const float* w, const float* zprev, const float* alpha_prev,
                int amod, float* raw, float* dx, float* dalpha_prev,
                int m, int n, int k, void* ws, size_t ws_bytes, void* stream);
/* dw[k,n] = x[m,k]^T @ dy[m,n] */
int fte_gemm_tn(const float* x, const float* dy, float* dw,
                int m, int n, int k, void* ws, size_t ws_bytes, void* stream);
size_t fte_gemm_ws_bytes(int m, int n, int k);

/* ---------------------------------------------------------------------------
 * Loss heads
 * ------------------------------------------------------------------------- */

/* Replaces SparseSoftmaxCrossEntropyWithLogits + mean + its gradient
 * (tf.losses.sparse_softmax_cross_entropy, nets/sphere.py:109):
 *   loss_rows[i] = -log softmax(logits[i,:c])[labels[i]]
 *   dlogits[i,j] = (softmax - onehot) * grad_scale   (columns c..ld-1 get 0)
 * logits/dlogits are [n, ld] with ld >= c (padded classifier width); pad columns of `logits` are never read.
 * Bad labels, the rule of every head of this section (softmax-CE, focal, A-softmax, additive margin): a label outside
 * [0, c) -- negative, >= c, a pad column c <= y < ld included -- gives a NaN row: loss_rows[i] and the row's gradient
 * (dlogits / G, and f, rowcoef where the head has them) are NaN in columns 0..c-1 and 0 in the pad columns c..ld-1, exactly as a
 * good row's pads.  Nothing is read or written out of bounds, the other rows are bitwise what they are without the bad
 * row, and the caller's non-finite-loss check trips (TF's sparse_softmax_cross_entropy gives NaN loss rows on GPU too).
 * Which kernel runs is decided by ld alone (row in registers up to ld = 2048 and up to 12288, three passes over the row
 * above); the three give bit-identical results for the same [n, c] logits.
 * FTE_EINVAL: a null pointer, n < 1, c < 1, ld < c. */
int fte_softmax_ce_fwd_bwd(const float* logits, const int32_t* labels, float* loss_rows,
                           float* dlogits, int n, int c, int ld, float grad_scale, void* stream);

/* focal_loss (loss.py:18-27; note the reference's swapped-looking defaults gamma = 1.0, alpha = 2.0 are kept as named):
 * loss_rows[i] = gamma * (1 - p_y)^alpha * CE_i, dlogits = grad_scale * d(loss_rows[i])/dlogits (through BOTH the
 * cross-entropy and the softmax-score factor, as tf.gradients does).  Same layout, pad and bad-label rules as above.
 * alpha >= 1 (FTE_EINVAL otherwise, nothing written): below 1 the factor (1 - p_y)^(alpha - 1) of the gradient is unbounded
 * as p_y -> 1.  A saturated row (1 - p_y rounds to 0 in fp32) has loss 0 and gradient 0, never NaN: (1 - p_y)^(alpha - 1) is
 * taken as 1 at alpha == 1 and the factor log p_y next to it is 0 there. */
int fte_focal_loss_fwd_bwd(const float* logits, const int32_t* labels, float* loss_rows, float* dlogits,
                           int n, int c, int ld, float gamma, float alpha, float grad_scale, void* stream);

/* A-softmax (SphereFace, m = 4; README.md:14,19 claims it, the code is not in
 * the reference tree -- SURVEY.md Appendix A.9).  s = x @ w is the raw dot
 * product [n, ld]; xn = |x_i| (n), wn = |W_j| (c).  Produces the margin logits
 * f (optional), the per-row loss, G = dLoss/ds (the matrix that feeds the two
 * gradient GEMMs), rowcoef (dx += rowcoef_i * x_i) and, via
 * fte_asoftmax_colcoef, colcoef (dw[:,j] += colcoef_j * w[:,j]).  f may be NULL (G, loss_rows and rowcoef do not
 * depend on it).  Columns c..ld-1 of f and G get 0; the bad-label rule of fte_softmax_ce_fwd_bwd holds (NaN loss, rowcoef, and
 * f / G below c).  psi is continuous in cos(theta_y) but its derivative is not at the branch thresholds 0, +-sqrt(1/2): a
 * target cosine within fp32 rounding of a threshold may take either neighbouring branch.
 * FTE_EINVAL: a null pointer (f excepted), n < 1, c < 1, ld < c. */
int fte_asoftmax_fwd_bwd(const float* s, const float* xn, const float* wn, const int32_t* labels,
                         float lambda, float* f, float* loss_rows, float* G, float* rowcoef,
                         int n, int c, int ld, float grad_scale, void* stream);
/* colcoef_j = -sum_i G[i,j] * s[i,j] / wn_j^2 (columns c..ld-1 get 0): the norm-correction term of a head on the
 * normalised weight columns, dw[:,j] += colcoef_j * w[:,j].  Serves both the A-softmax head and the additive-margin
 * head below (whatever the loss, G = dLoss/ds and s = x @ w). */
int fte_asoftmax_colcoef(const float* G, const float* s, const float* wn, float* colcoef,
                         int n, int c, int ld, void* stream);
/* Additive-margin softmax: ArcFace (angular margin m, cos(theta + m)) and CosFace (cosine margin m3, cos(theta) - m3),
 * InsightFace's combined margin with m1 = 1.  Scale S = `scale`.  For row i with label y, column j < c, eps = 1e-12:
 *   c_ij = clamp(s_ij / (max(xn_i, eps) * wn_j), -1, 1)      (the clamp only absorbs rounding: identity in the derivative)
 *   z_ij = S * c_ij (j != y);  z_iy = S * t(c_iy) with
 *     m == 0:                      t = c - m3,                                 t' = 1                          (CosFace)
 *     m > 0, c > cos(pi - m):      t = c cos m - sin_t sin m - m3,            t' = cos m + sin m * c / max(sin_t, 1e-6),
 *                                  sin_t = sqrt(max((1 - c)(1 + c), 0))                                        (ArcFace)
 *     m > 0, otherwise:            t = c - m sin m - m3,                       t' = 1       (theta + m > pi, easy_margin = False)
 *   loss_rows[i] = logsumexp_j z_ij - z_iy
 *   dL/dc_ij = grad_scale * S * (p_ij - [j = y]) * (j = y ? t' : 1),  p = softmax(z_i)
 *   G_ij = dL/dc_ij / (max(xn_i, eps) * wn_j)                  (dLoss/ds: feeds the two classifier GEMMs)
 *   rowcoef_i = xn_i > eps ? -sum_j G_ij s_ij / xn_i^2 : 0
 *   f (optional, may be NULL) = z, the margin logits.
 * With colcoef from fte_asoftmax_colcoef, dx = G W^T + rowcoef (.) x and dW = x^T G + colcoef (.) W: the exact gradient through
 * both normalisations (not the straight-through variant that applies the margin under no_grad).  s / f / G are [n, ld],
 * ld >= c; columns c..ld-1 get G = 0 and f = 0 and wn[j] is never read for j >= c.  An out-of-range label gives a NaN row
 * (loss, rowcoef, G and f below c), never an out-of-bounds access.  Zero-norm weight columns are outside the contract.
 * Presets: ArcFace S = 64, m = 0.5, m3 = 0; CosFace S = 64, m = 0, m3 = 0.35.
 * FTE_EINVAL: a null pointer (f excepted), n < 1, c < 1, ld < c, scale <= 0 or m < 0 (or either NaN). */
int fte_margin_softmax_fwd_bwd(const float* s, const float* xn, const float* wn, const int32_t* labels,
                               float scale, float m, float m3, float* f, float* loss_rows, float* G, float* rowcoef,
                               int n, int c, int ld, float grad_scale, void* stream);
/* Sharded margin head: fte_margin_softmax_fwd_bwd with the classes split over R ranks (model parallelism).
 * Global batch of N = R * n_local rows in rank order (the `n` below is N), C = num_classes classes, Cs = ceil(C / R).  Rank r owns
 * classes [lo_r, hi_r) = [r * Cs, min(C, (r + 1) * Cs)), c_r = hi_r - lo_r >= 1, stored as columns [D, ld_r] with ld_r = c_r rounded
 * up to 128 and zero padding columns.  c_ij, t, t', eps, the clamp and the presets are those of fte_margin_softmax_fwd_bwd.  Labels
 * are GLOBAL class ids: row i's target column lives on the one shard with lo <= y_i < hi, at local column y_i - lo.
 *
 * fte_margin_shard_stats -- for row i over this shard's live columns j < c, z_ij carrying the margin on the target column iff this
 * shard owns it; stats is [3][n]:
 *   stats[0][i] = max_j z_ij,   stats[1][i] = sum_j exp(z_ij - stats[0][i]),   stats[2][i] = z_iy if the shard owns y_i, else 0.0f
 * A label outside [0, num_classes) gives NaN in all three on EVERY shard, never an out-of-bounds access.
 *
 * fte_margin_shard_fwd_bwd -- all_stats is [R][3][n], the shards' stats in rank order.  Per row, every sum over r in rank order (so
 * every rank computes the same bits from the same all_stats):
 *   M = max_r m_r,   Z = sum_r e_r * expf(m_r - M),   T = sum_r t_r,   loss_rows[i] = logf(Z) + M - T   (the same on every shard)
 *   p_ij = exp(z_ij - M) / Z
 *   G_ij = grad_scale * S * (p_ij - [j owns y]) * (t' or 1) / (max(xn_i, eps) * wn_j) on this shard's columns, 0 in c..ld-1
 *   rowcoef_part[i] = xn_i > eps ? -sum_{j<c} G_ij s_ij / xn_i^2 : 0     (the shard's share: the shares add up to the dense rowcoef)
 *   f (optional, may be NULL) = this shard's margin logits, 0 in the pads.
 * A NaN statistic (or an out-of-range label) gives the NaN row of the dense contract; the other rows are bitwise unaffected.
 * colcoef is the unchanged fte_asoftmax_colcoef over all N rows of the shard's G: complete on the owning rank.  With X [N, D] the
 * gathered features, dW_r = X^T G + colcoef (.) W_r is FINAL (no all-reduce), dX = sum_r (G W_r^T + rowcoef_part (.) X).
 * Both: 16-byte aligned s / wn / G / f and ld % 4 == 0 take the vector path, anything else the scalar one.  All sums are fp32 in a
 * fixed order, no float atomics: two calls write identical bytes.
 * FTE_EINVAL (nothing is launched): the cases of fte_margin_softmax_fwd_bwd, a null stats / all_stats, R < 1, class_lo < 0,
 * class_lo + c > num_classes. */
int fte_margin_shard_stats(const float* s, const float* xn, const float* wn, const int32_t* labels,
                           int class_lo, int num_classes, float scale, float m, float m3,
                           float* stats, int n, int c, int ld, void* stream);
int fte_margin_shard_fwd_bwd(const float* s, const float* xn, const float* wn, const int32_t* labels,
                             int class_lo, int num_classes, float scale, float m, float m3,
                             const float* all_stats, int R,
                             float* f, float* loss_rows, float* G, float* rowcoef_part,
                             int n, int c, int ld, float grad_scale, void* stream);
/* Additive-margin softmax with a margin per row (the AdaFace head; Kim et al., CVPR 2022).  The contract is that of
 * fte_margin_softmax_fwd_bwd above -- c_ij, z_ij for j != y, loss_rows, G, rowcoef, the optional f, columns c..ld-1, the NaN row
 * of an out-of-range label -- with the target term of row i taken from a = a_rows[i], b = b_rows[i] (c = c_iy, E = 1e-3):
 *   theta = acos(c),  theta' = min(max(theta + a, E), pi - E),  z_iy = S * t,  t = cos(theta') - b
 *   t' = sin(theta') / max(sin_t, 1e-6), sin_t = sqrt(max((1 - c)(1 + c), 0)), where the clip of theta' does not bind
 *   t' = 0 where it binds (the logit is the constant cos(E) - b or -cos(E) - b there: AdaFace's clip under autograd)
 * a may be negative.  A NaN or infinite a or b gives a NaN row like an out-of-range label.  a_i = 0, b_i = m3 is CosFace and
 * a_i = m, b_i = 0 is ArcFace on the rows with c_iy > cos(pi - m) whose theta' stays inside the clip.
 * FTE_EINVAL: a null pointer (f excepted), n < 1, c < 1, ld < c, scale <= 0 (or NaN). */
int fte_margin_softmax_rows_fwd_bwd(const float* s, const float* xn, const float* wn, const int32_t* labels, float scale,
                                    const float* a_rows, const float* b_rows, float* f, float* loss_rows, float* G, float* rowcoef,
                                    int n, int c, int ld, float grad_scale, void* stream);
/* AdaFace's margins from the embedding norms xn [n] (fte_row_norms) and the running statistics stats = [mean, std]:
 *   q_i = min(max(xn_i, 1e-3), 100),  mean_b = sum q / n,  std_b = sqrt(sum (q - mean_b)^2 / (n - 1))   (two passes)
 *   mu = t_alpha * mean_b + (1 - t_alpha) * stats[0],  sd = t_alpha * std_b + (1 - t_alpha) * stats[1]
 *   k_i = min(max((q_i - mu) / (sd + 1e-3) * h, -1), 1),  a_rows[i] = -m * k_i,  b_rows[i] = m + m * k_i
 * update != 0: stats is overwritten with (mu, sd); update == 0: stats is left alone (the margins use (mu, sd) either way).
 * One block, one launch, no host read-back; the sums run in a fixed order: two calls on the same data are bit-identical.  The
 * norm enters the margins as a constant (no gradient flows through k_i), as in the paper.
 * FTE_EINVAL: a null pointer, n < 2, m < 0, h <= 0, t_alpha outside [0, 1] (or any of them NaN). */
int fte_adaface_margins(const float* xn, int n, float m, float h, float t_alpha, int update, float* stats,
                        float* a_rows, float* b_rows, void* stream);
/* CurricularFace (Huang et al., CVPR 2020): ArcFace's target column, and the NEGATIVE columns whose cosine exceeds the margined
 * target cosine are re-weighted by a running mean t of the batch's target cosines; DESIGN.md 4.21.  c_ij, eps, the clamp (identity
 * derivative, NaN stays NaN), loss_rows, rowcoef, the optional f, columns c..ld-1 and the NaN row of an out-of-range label are
 * those of fte_margin_softmax_fwd_bwd.  With c = c_iy, sin_t = sqrt(max((1 - c)(1 + c), 0)):
 *   u_i = c cos m - sin_t sin m                               (the mask threshold, on both sides of the fallback below)
 *   target:  c > -cos m:  z_iy = S u_i,              t' = cos m + sin m * c / max(sin_t, 1e-6)
 *            otherwise:   z_iy = S (c - m sin m),    t' = 1                        (the target column of fte_margin_softmax_fwd_bwd, m3 = 0)
 *   j != y:  c_ij > u_i (HARD; strict, a NaN is never hard):  z_ij = S c_ij (t + c_ij),  dz/dc = S (t + 2 c_ij)
 *            otherwise:                                       z_ij = S c_ij,             dz/dc = S
 *   G_ij = grad_scale * (p_ij - [j = y]) * (dz/dc)_ij / (max(xn_i, eps) * wn_j);  the mask and t are constants of the gradient.
 * The logit is DISCONTINUOUS in c_ij at c_ij = u_i: it jumps by S c (t + c - 1).
 * t = t_used[0] is read on the device, once per block.  colcoef is the unchanged fte_asoftmax_colcoef.  Preset: S = 64, m = 0.5.
 *
 * fte_curricular_t -- before the logits:  c_iy as above over the rows with 0 <= labels[i] < c (V of them);
 *   update != 0 and V > 0:  t_used[0] = t_state[0] = alpha * (sum c_iy / V) + (1 - alpha) * t_state[0]
 *   otherwise:              t_used[0] = t_state[0], t_state is not written
 * One block, sums in a fixed order, no float atomics, no host read-back: two calls on the same data write identical bytes.
 * FTE_EINVAL (nothing is launched or written), both: a null pointer (f excepted), n < 1, c < 1, ld < c, scale <= 0, m outside
 * [0, pi/2), alpha outside [0, 1] (or any of them NaN). */
int fte_curricular_t(const float* s, const float* xn, const float* wn, const int32_t* labels, float alpha, int update,
                     float* t_state, float* t_used, int n, int c, int ld, void* stream);
int fte_curricular_softmax_fwd_bwd(const float* s, const float* xn, const float* wn, const int32_t* labels, float scale, float m,
                                   const float* t_used, float* f, float* loss_rows, float* G, float* rowcoef,
                                   int n, int c, int ld, float grad_scale, void* stream);
/* MagFace (Meng et al., CVPR 2021): ArcFace's target column with the margin of each row a function of the NORM of its embedding,
 * and a regulariser g on that norm; the one head whose margin is NOT a constant of the gradient; DESIGN.md 4.22.  c_ij, eps, the
 * clamp (identity derivative, NaN stays NaN), loss_rows, G, the optional f, columns c..ld-1 and the NaN row of an out-of-range
 * label (NaN in reg_rows too) are those of fte_margin_softmax_fwd_bwd.  With a_raw = xn_i, a = min(max(a_raw, l_a), u_a),
 * k_m = (u_m - l_m) / (u_a - l_a), c = c_iy, sin_t = sqrt(max((1 - c)(1 + c), 0)):
 *   mu_i = l_m + k_m (a - l_a)                                 (the row's margin)
 *   reg_rows[i] = g_i = a / u_a^2 + 1 / a                      (the regulariser)
 *   c > -cos mu:  t = c cos mu - sin_t sin mu,  t' = cos mu + sin mu * c / max(sin_t, 1e-6),  dt/dmu = -(sin_t cos mu + c sin mu)
 *   otherwise:    t = c - mu sin mu,            t' = 1,                                      dt/dmu = -(sin mu + mu cos mu)
 *   z_iy = S t;  z_ij = S c_ij (j != y);  loss_rows[i] = logsumexp_j z_ij - z_iy
 *   G_ij = grad_scale * S (p_ij - [j = y]) (j = y ? t' : 1) / (max(xn_i, eps) * wn_j)
 *   in_i = [l_a <= a_raw <= u_a]                               (the derivative of the clamp, bounds included)
 *   dL/da_i = in_i * grad_scale * (S (p_iy - 1) * dt/dmu * k_m + lambda_g (1 / u_a^2 - 1 / a^2))
 *   rowcoef_i = xn_i > eps ? -sum_j G_ij s_ij / xn_i^2 + (dL/da_i) / xn_i : 0
 * The whole of the gradient through the norm is in rowcoef: dx = G W^T + rowcoef (.) x and dW = x^T G + colcoef (.) W keep their
 * form, colcoef is the unchanged fte_asoftmax_colcoef.  The total loss the gradient belongs to is
 * grad_scale * sum_i (loss_rows[i] + lambda_g reg_rows[i]).  The target logit is DISCONTINUOUS in c at c = -cos mu_i.
 * One launch (mu needs no batch statistic); mu, cos mu, sin mu once per block; sums in fp32 in a fixed order, no float atomics: two
 * calls write identical bytes.  Preset (the paper's MS1M-V2 values): S = 64, l_a = 10, u_a = 110, l_m = 0.45, u_m = 0.8, lambda_g = 35.
 * FTE_EINVAL (nothing is launched or written): a null pointer (f excepted), n < 1, c < 1, ld < c, scale <= 0, l_a <= 0, u_a <= l_a,
 * l_m < 0, u_m < l_m, u_m >= pi/2, lambda_g < 0 (or any of them NaN). */
int fte_magface_softmax_fwd_bwd(const float* s, const float* xn, const float* wn, const int32_t* labels, float scale,
                                float l_a, float u_a, float l_m, float u_m, float lambda_g,
                                float* f, float* loss_rows, float* reg_rows, float* G, float* rowcoef,
                                int n, int c, int ld, float grad_scale, void* stream);
/* Sub-center ArcFace (Deng et al., ECCV 2020): K centres per class, the class cosine the max over them; DESIGN.md 4.16.
 * LAYOUT -- planar: with ld the padded class count of ONE plane, the classifier W [d, K*ld], the raw product s = x @ W [n, K*ld],
 * G [n, K*ld], wn [K*ld] and colcoef [K*ld] hold centre k of class j at column k*ld + j; columns c..ld-1 of every plane are
 * padding.  (A 16-byte chunk of a plane is four classes, so the pool is an element-wise max of K aligned loads; plane k of W is
 * W + k*ld with row stride K*ld, which a per-plane gather / scatter of sampled classes can address without a new kernel.)
 * The contract is that of fte_margin_softmax_fwd_bwd -- eps, clamp, t, t', the presets -- on the pooled cosine:
 *   c_ijk = clamp(s[i, k*ld+j] / (max(xn_i, eps) * wn[k*ld+j]), -1, 1),   c_ij = max_k c_ijk,
 *   k*(i,j) = the LOWEST k that attains the max (a fixed rule: two calls give the same bits)
 *   z, loss_rows and dL/dc_ij as above on c_ij (the margin applies to the pooled target cosine)
 *   G[i, k*ld+j] = dL/dc_ij / (max(xn_i, eps) * wn[k*ld+j]) for k = k*(i,j), exactly 0.0f for the other centres and in the pad
 *   columns of every plane;  rowcoef_i = xn_i > eps ? -sum_{j,k} G s / xn_i^2 : 0;  f (optional, [n, ld]) = the pooled z, 0 in pads.
 * wn is read only at k*ld + j, j < c.  An out-of-range label gives a NaN row: loss, rowcoef, f and G below c in EVERY plane are
 * NaN, the pads 0, the other rows bitwise unaffected.  With K = 1 every output is bit-identical to fte_margin_softmax_fwd_bwd on
 * the same inputs.  16-byte aligned s / wn / G / f and ld % 4 == 0 take the vector path, anything else the scalar one.
 * FTE_EINVAL: the cases of fte_margin_softmax_fwd_bwd, and K outside 1..8. */
int fte_subcenter_margin_softmax_fwd_bwd(const float* s, const float* xn, const float* wn, const int32_t* labels, int K,
                                         float scale, float m, float m3, float* f, float* loss_rows, float* G, float* rowcoef,
                                         int n, int c, int ld, float grad_scale, void* stream);
/* colcoef [K*ld] of the planar layout: colcoef[k*ld+j] = -sum_i G[i, k*ld+j] * s[i, k*ld+j] / wn[k*ld+j]^2 for j < c and 0 for
 * the pad columns c..ld-1 of EVERY plane (fte_asoftmax_colcoef over one width K*ld would divide by wn = 0 in the pads of the
 * interior planes).  With K = 1 bit-identical to fte_asoftmax_colcoef.  FTE_EINVAL: its cases, and K outside 1..8. */
int fte_subcenter_colcoef(const float* G, const float* s, const float* wn, float* colcoef, int K, int n, int c, int ld, void* stream);
/* The assignment of the cleaning pass: for sample i with label y, cosv[k*n + i] = clamp(x_i . w_k / (max(|x_i|, eps) *
 * max(|w_k|, eps)), -1, 1) for the K centres w_k = Wt[k*c + y, :] of its OWN class, and sel[i] = arg max_k, the lowest k on a tie.
 * x [n, d]; Wt [K*c, d] is the classifier transposed once by the caller, row k*c + j = centre k of class j (no padding);
 * sel [n] int32, cosv [K*n].  Only K rows of Wt are read per sample -- the [n, K*c] product is never formed.  A label outside
 * [0, c) gives sel = -1 and cosv = NaN for every k.  One wave per sample; lane l sums elements l, l+64, ... in index order and the
 * lanes merge in a fixed butterfly, so the order of every sum depends on d ONLY: a sample's result is the same bits wherever it
 * sits in the batch and whatever n is.  FTE_EINVAL: a null pointer, n, d or c < 1, K outside 1..8. */
int fte_subcenter_assign(const float* x, const float* Wt, const int32_t* labels, int K, int32_t* sel, float* cosv,
                         int n, int d, int c, void* stream);
/* out[i] = sqrt(sum_j a[i,j]^2) over rows of [rows, ld] (cols used) */
int fte_row_norms(const float* a, float* out, int rows, int cols, int ld, void* stream);
/* out[j] = sqrt(sum_i a[i,j]^2) over columns */
int fte_col_norms(const float* a, float* out, int rows, int cols, int ld, void* stream);
/* The flip-averaged inference path (nets/sphere.py:97-101, evaluate.py:62-63): y[n,h,w',c] = x[n,h,wd-1-w',c] replaces
 * tf.reverse(images, axis=[2]) (x != y; 16-byte aligned when c % 4 == 0) and out = a*x + b*y the mean of the two embeddings
 * (a = b = 0.5; out may alias x or y; n >= 1). */
int fte_flip_width(const float* x, float* y, int n, int h, int wd, int c, void* stream);
int fte_axpby(float a, const float* x, float b, const float* y, float* out, long n, void* stream);
/* a[i,j] += rc[i] * b[i,j]   (rc NULL -> skip) ;  a[i,j] += cc[j] * b[i,j]  (cc NULL -> skip), a and b [rows, ld], ld >= cols;
 * columns cols..ld-1 are neither read nor written. */
int fte_add_scaled_rows_cols(float* a, const float* b, const float* rc, const float* cc,
                             int rows, int cols, int ld, void* stream);

/* center loss (loss.py:29-45): loss_rows[i] = sum_j (f_ij - c_{y_i} j)^2 (caller takes the mean over n*d);
 * dfeat = 2(f - c_y)*grad_scale; then centers[y] -= (1-alpha)(c_y - f), duplicates accumulating
 * (scatter_sub).  Every gather is served from the centers as they were BEFORE the update
 * (loss.py:37 before :39).  In place on `centers` [num_classes, d]; ws >= n*d floats, and after the call
 * ws[0 : n*d] holds diff = f - c_y (what fte_center_scatter_update consumes).  alpha == 1 evaluates loss and gradient
 * only (no update launch).  A label outside [0, num_classes) gives a NaN loss / gradient row, a zero diff row and no
 * update -- never an out-of-bounds access; such a sample is skipped by the update as if it were not in the batch (it
 * does not own a row of the table either).  The update is deterministic: rows of one label are summed in sample order.
 * FTE_EINVAL: a null pointer, n, d or num_classes < 1; FTE_EWORKSPACE: ws NULL or ws_bytes < n*d*sizeof(float). */
int fte_center_loss_fwd_bwd_update(const float* feat, const int32_t* labels, float* centers,
                                   float* loss_rows, float* dfeat, int n, int d, int num_classes, float alpha,
                                   float grad_scale, void* ws, size_t ws_bytes, void* stream);
/* the scatter_sub half of loss.py:38-39 on its own: centers[labels[i]] += (1 - alpha) * diff[i] for i < n, duplicates
 * accumulating.  Used by the opt-in replica reconciliation (DataParallel(sync_centers=True)): every rank evaluates the loss
 * with alpha = 1, the ranks all-gather their (labels, diff) rows and each applies ALL of them, so the replicas keep ONE
 * table equal to the single-tower update of the global batch; the default reproduces the reference's per-tower tables. */
int fte_center_scatter_update(const float* diff, const int32_t* labels, float* centers, int n, int d, int num_classes,
                              float alpha, void* stream);

/* batch-hard triplet (loss.py:47-78): per-sample loss [n] and d(sum w_i*loss_i)/dfeat.
 * soft_margin != 0 selects softplus(pos - neg) (margin=None in the reference, loss.py:74-75) and `margin` is ignored; otherwise
 * max(0, pos - neg + margin) for ANY margin, negative ones included (loss.py:76-77).
 * ws >= 2*n*n floats (the distance and the coefficient matrix; FTE_EWORKSPACE below that).  1 <= n <= 8192 (a coefficient
 * row lives in LDS) and d >= 1, FTE_EINVAL otherwise, before anything is launched.
 * As in the reference, an anchor without a positive takes pos = 0 and one without a negative neg = 1e6, and neither
 * contributes a gradient; distances are sqrt(|f_i - f_j|^2 + 1e-12).
 * Ties: of several equidistant hardest positives (or negatives) the one with the LOWEST index takes the whole gradient
 * (numpy argmax / argmin).  The reference's tf.reduce_max / reduce_min divide the gradient evenly among tied entries; only
 * exact ties differ, i.e. duplicated images in one batch, and the loss values are the same either way. */
int fte_batch_hard_triplet_fwd_bwd(const float* feat, const int32_t* labels, float margin, int soft_margin,
                                   float loss_weight, float* loss_rows, float* dfeat,
                                   int n, int d, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------
 * Flat-arena reductions and optimizers (ApplyMomentum / ApplyAdam per variable,
 * data_parallel.py:65-69,191-196; L2Loss + AddN, nets/net_base.py:105).
 * ------------------------------------------------------------------------- */

/* out[j] = scale * sum_{r<rows} in[r*cols + j]  (+ bias[j % bmod] when bias != NULL).
 * If fold > 1, column j of `out` (cols/fold of them) sums in[r, j + t*(cols/fold)] over t too. */
int fte_reduce_rows(const float* in, float* out, const float* bias, int bmod,
                    long rows, long cols, int fold, float scale, void* stream);
/* out[0] = scale * sum_i a[i]^2   (ws >= 1024 floats; a 16-byte aligned, n >= 1, any remainder n % 4) */
int fte_sumsq(const float* a, long n, float scale, float* out, void* ws, size_t ws_bytes, void* stream);
/* out[0] = scale * sum_i a[i]     (ws >= 1024 floats; a 16-byte aligned, n >= 1, any remainder n % 4) */
int fte_sum(const float* a, long n, float scale, float* out, void* ws, size_t ws_bytes, void* stream);

/* acc = mom*acc + (gscale*g + wd*w) ; w -= lr*acc      (MomentumOptimizer, Appendix A.7); w, acc, g 16-byte aligned, n >= 1,
 * any remainder n % 4 */
int fte_momentum_update(float* w, float* acc, const float* g, long n,
                        float lr, float mom, float wd, float gscale, void* stream);
/* TF AdamOptimizer (epsilon outside the bias correction) on gscale*g + wd*w; t = 1-based step (t < 1: FTE_EINVAL) */
int fte_adam_update(float* w, float* m, float* v, const float* g, long n,
                    float lr, float b1, float b2, float eps, float wd, float gscale, int t, void* stream);

/* ---------------------------------------------------------------------------
 * Evaluation: similarity search and score statistics (verify.py).
 * Scoring of extracted embeddings: LFW-style listed pairs, all-pairs TAR@FAR through genuine / impostor score histograms, and
 * 1:N identification through a fused product + top-k.  All arithmetic is fp32 and the products run on v_mfma_f32_32x32x2_f32
 * (an exact fp32 fma chain in a k order fixed by d alone, so a score does not depend on the tile, slice or chunk that computed
 * it); these entry points IGNORE fte_set_mfma_dtype.  Rows are row-major [rows, d].  Like every entry point they neither allocate
 * nor synchronise, and every tensor must stay below 2 GiB: a larger gallery or set is passed in chunks (fte_topk_merge combines
 * the chunks' top-k lists; the histogram call accumulates, so the host walks the chunk pairs I <= J).
 * ------------------------------------------------------------------------- */

/* y[i,:] = x[i,:] / max(|x_i|, 1e-12) with |x_i| = sqrt(sum_c x[i,c]^2) reduced in a fixed order; norms[i] = |x_i| when
 * norms != NULL.  x and y may alias.  FTE_EINVAL: x or y NULL, n < 1, d < 1, or a tensor of 2 GiB or more. */
int fte_l2_normalize_rows(const float* x, float* y, float* norms, int n, int d, void* stream);
/* out[p] = dot(x[ia[p],:], x[ib[p],:]) for p < npairs (the LFW protocol's listed pairs, on normalised rows).  An index outside
 * [0, n) gives out[p] = NaN, never an out-of-bounds read.  FTE_EINVAL: a NULL pointer, n < 1, d < 1, npairs < 1, >= 2 GiB. */
int fte_pair_scores(const float* x, const int32_t* ia, const int32_t* ib, float* out, int n, int d, int npairs, void* stream);
/* Fused similarity + top-k.  probes [m, d] and gallery [n, d], both normalised, d % 32 == 0, 1 <= k <= 64, k <= n.
 * scores [m, k] (fp32) and index [m, k] (int32): row i holds the k best gallery rows j by s = dot(probe_i, gallery_j), sorted by
 * score descending; equal scores are ordered by the smaller gallery index, so the result is fully deterministic.  Every returned
 * index is gallery_base + j.  exclude_self != 0 drops the pairs with probe_base + i == gallery_base + j (leave-one-out
 * identification when probes and gallery are one set); a row then left with fewer than k candidates ends in (-inf, -1) slots.
 * Two passes: a partial pass over (32-probe block, gallery slice) pairs, the slice count chosen from the CU count, writes each
 * (row, slice) top-k list to ws; fte_topk_merge then merges the slices.  ws >= fte_topk_search_ws_bytes(m, n, d, k).
 * FTE_EINVAL: a NULL pointer (ws excepted), m < 1, n < 1, d % 32, k outside 1..min(64, n), a base < 0, or a tensor >= 2 GiB.
 * FTE_EWORKSPACE: ws NULL or short. */
size_t fte_topk_search_ws_bytes(int m, int n, int d, int k);
int fte_topk_search(const float* probes, const float* gallery, int m, int n, int d, int k, int gallery_base, int exclude_self,
                    int probe_base, float* scores, int32_t* index, void* ws, size_t ws_bytes, void* stream);
/* Merge of `lists` sorted top-k lists per row: in_scores / in_index [m, lists, k], each list in the order above (index < 0 marks
 * an empty slot, after every real one) -> scores / index [m, k] in the same order.  The host merges the results of several
 * gallery chunks with it (stack the chunks' [m, k] outputs into [m, lists, k]).  Indices are taken as they are (no base added).
 * FTE_EINVAL: a NULL pointer, m < 1, lists outside 1..64, k outside 1..64, or a tensor >= 2 GiB. */
int fte_topk_merge(const float* in_scores, const int32_t* in_index, int m, int lists, int k, float* scores, int32_t* index,
                   void* stream);
/* Fused similarity + score histograms.  a [na, d] with labels la [na], b [nb, d] with labels lb [nb], all normalised,
 * d % 32 == 0.  same == 0: every pair (i of a, j of b) counts; same != 0: a and b are the same rows (na == nb) and only the
 * pairs i < j count.  A pair's score s = dot(a_i, b_j) goes to bin
 *     bin = clamp((int)((s + 1.0f) * (0.5f * nbins)), 0, nbins - 1)        (exactly this fp32 expression)
 * of hist_genuine when la[i] == lb[j], else of hist_impostor.  Both are uint64 [nbins] and the call ACCUMULATES (+=) into them,
 * so the host can stream chunk pairs of a set of any size; the counts are integer and independent of execution order.  Bin b
 * covers scores [2b / nbins - 1, 2(b + 1) / nbins - 1).  nbins is a power of two in 256..8192.
 * FTE_EINVAL: a NULL pointer, na < 1, nb < 1, d % 32, a bad nbins, same with na != nb, or a tensor >= 2 GiB. */
int fte_score_histograms(const float* a, const int32_t* la, int na, const float* b, const int32_t* lb, int nb, int d, int same,
                         int nbins, uint64_t* hist_genuine, uint64_t* hist_impostor, void* stream);

/* ---- Templates (IJB-style set-to-set comparison; verify.py --protocol templates / template_search) ----
 * A template is a set of image rows of one subject, grouped into media (one still image, or the frames of one video).  Both
 * entry points take the grouping as int32 CSR lists over the feature rows x [n, d]:
 *     members   [n_members]        feature row of each member, template-major (template 0's media first, each media's members
 *                                  in listed order);
 *     media_off [n_media + 1]      media m has members[media_off[m] .. media_off[m + 1]);
 *     tmpl_off  [n_templates + 1]  template t has media tmpl_off[t] .. tmpl_off[t + 1] - 1.
 * The offsets are read on the device and never trusted: an offset outside its list or a decreasing pair, like a member row
 * outside [0, n), makes that template's result NaN and is never an out-of-bounds read. */

/* Media-aware template pooling.  For each template t, with w[r] = 1 when w == NULL:
 *     v = sum over media m of t, in listed order, of  ( sum over members i of m, in listed order: w[r_i] * x[r_i,:] ) / W_m,
 *         W_m = sum of those w[r_i] in the same order (fp32); a media with W_m == 0 (or no members) contributes nothing;
 *     out[t,:] = v / max(|v|, 1e-12)      (exactly the fte_l2_normalize_rows rule and reduction order: the pooled row is
 *                                           bitwise what fte_l2_normalize_rows gives on the unnormalised v)
 * Every column's sum is one sequential chain in list order, so out depends on the lists alone, not on the launch geometry.  A
 * template with no media (or only zero-weight media) gives a zero row; one with a member row outside [0, n) or bad offsets gives
 * a NaN row.  x [n, d], w [n] (optional), out [n_templates, d], any d >= 1.  HBM / L2 bound: a gather with a fixed-order sum.
 * FTE_EINVAL: a NULL pointer (w excepted), n, d, n_members, n_media or n_templates < 1, or a tensor of 2 GiB or more. */
int fte_template_pool(const float* x, const float* w, int n, int d, const int32_t* members, int n_members, const int32_t* media_off,
                      int n_media, const int32_t* tmpl_off, int n_templates, float* out, void* stream);
/* Set-to-set softmax score fusion (the IJB-A "SoftMax" template comparison).  x [n, d] normalised rows, d % 32 == 0; media are
 * ignored: template t is the member rows members[media_off[tmpl_off[t]] .. media_off[tmpl_off[t + 1]]).  For each listed pair
 * p < npairs with A = ta[p], B = tb[p] and betas[0 .. nbetas) (a HOST array, 1 <= nbetas <= 32, each beta in [0, 40]):
 *     out[p] = (1 / nbetas) sum over b of  N_b / D_b,   N_b = sum_{i in A, j in B} s_ij e_ijb,  D_b = sum_{i in A, j in B} e_ijb,
 *     s_ij = dot(x_i, x_j) (fp32 on v_mfma_f32_16x16x4_f32, a k order fixed by d alone),
 *     e_ijb = exp2(c_b * s_ij - c_b) with c_b = (float)(beta_b * log2(e)) (hardware exp2; fp32 fma for the argument).
 * Shifting the exponent by the bound |s| <= 1 cancels in N_b / D_b and keeps e in [2^-116, 1]: a normal float for beta <= 40,
 * so no sum can overflow and D_b > 0.  beta = 0 gives the plain mean of the |A| |B| scores.  No score matrix is materialised.
 * The sums run over 16 x 16 tiles of the pair in an order, and are reduced over the lanes in an order, fixed by (|A|, |B|,
 * nbetas): a pair's result depends only on its two member lists, x and betas -- not on its position, npairs or the grid -- so
 * the host may reorder pairs (largest first, for load balance) without changing a bit.  An out-of-range template id, an empty
 * template, bad offsets or a member row outside [0, n) gives out[p] = NaN.
 * FTE_EINVAL: a NULL pointer, n, n_members, n_media, n_templates or npairs < 1, d < 32 or d % 32, nbetas outside 1..32, a beta
 * outside [0, 40] (or NaN), or a tensor of 2 GiB or more. */
int fte_set_pair_scores(const float* x, int n, int d, const int32_t* members, int n_members, const int32_t* media_off, int n_media,
                        const int32_t* tmpl_off, int n_templates, const int32_t* ta, const int32_t* tb, int npairs, const float* betas,
                        int nbetas, float* out, void* stream);

/* ---- MegaFace (challenge 1 style million-distractor identification and verification; verify.py --protocol megaface,
 * DESIGN.md 4.12) ----
 * The protocol, which the host side (verification.py megaface_*) implements on these two calls:
 *   probe set: the FaceScrub rows with labels; distractors: rows of a path-only list, row i = line i.  Noise removal drops a
 *   distractor whose path equals a listed path or ends with "/" + that path, before anything else.  Size N: the first N kept
 *   distractor rows in list order (a size above the kept count is capped to it).
 *   genuine pairs: every ordered pair (p, g) of distinct FaceScrub rows with the same label.
 *   rank of (p, g) at size N: 1 + #{d < N : s(p, d) >= s(p, g)}: TIES COUNT AGAINST THE GENUINE PAIR.  CMC(k) at size N: the
 *   fraction of pairs with rank <= k.
 *   verification at size N: genuine = unordered same-label FaceScrub pairs, impostor = every (FaceScrub row, distractor d < N)
 *   pair, TAR at FAR from fte_score_histograms-binned histograms.
 * Scores are fp32 cosines of normalised rows on v_mfma_f32_32x32x2_f32 with the probe on the lane side and the other row on the
 * register side, in the k order of the other evaluation products (fixed by d alone).  s(p, g) from fte_megaface_pair_scores and
 * s(p, d) inside fte_megaface_scan are the same arithmetic: a distractor that is a bitwise copy of g ties exactly and counts,
 * wherever it falls. */

/* out[j] = s(probes[ip[j]], rows[ig[j]]) for j < npairs, in the scan's arithmetic (above).  probes [m, d] and rows [n, d]
 * normalised, d % 32 == 0.  An index outside [0, m) or [0, n) gives out[j] = NaN, never an out-of-bounds read.
 * FTE_EINVAL: a NULL pointer, m, n or npairs < 1, d < 32 or d % 32, or a tensor of 2 GiB or more. */
int fte_megaface_pair_scores(const float* probes, int m, const float* rows, int n, int d, const int32_t* ip, const int32_t* ig,
                             int npairs, float* out, void* stream);
/* Fused rank count + impostor histogram of probes [m, d] against one range of distractor rows [n, d] (both normalised,
 * d % 32 == 0), with no score matrix.  Each probe's genuine scores, sorted DESCENDING, are an int32 CSR list: probe p has
 * thresholds thr[thr_off[p] .. thr_off[p + 1]) (thr_off [m + 1], thr [nthr], fp32).  The call ACCUMULATES (+=):
 *     counts[j] += #{rows r of the range : s(p, r) >= thr[j]}       for every threshold j of every probe p   (uint64 [nthr])
 *     hist[bin(s(p, r))] += 1                                       for every probe p and row r              (uint64 [nbins])
 * with bin() the fte_score_histograms formula, nbins a power of two in 256..8192.  The host scans each size bucket
 * [N_{b-1}, N_b) as its own range (or several chunks of it) and sums; every count is an integer, so the result does not depend
 * on order, chunking or the launch geometry.  A probe whose list is bad (thr_off[p] > thr_off[p + 1], or outside 0..nthr) or
 * empty is SKIPPED for the counts (its slots are left as they are) but its scores still enter hist; a list that is not sorted
 * descending gives wrong counts for that probe, never an out-of-bounds access.  ws (>= fte_megaface_scan_ws_bytes) holds a
 * uint64 per threshold: survivors of a fast reject against the probe's smallest threshold are counted at the first threshold
 * they reach, and a second kernel turns those into the prefix sums.  ws is cleared by the call (hipMemsetAsync on the stream).
 * FTE_EINVAL: a NULL pointer (ws excepted), m, n or nthr < 1, d < 32 or d % 32, a bad nbins, or a tensor of 2 GiB or more.
 * FTE_EWORKSPACE: ws NULL or short. */
size_t fte_megaface_scan_ws_bytes(int m, int nthr);
int fte_megaface_scan(const float* probes, int m, const float* rows, int n, int d, const int32_t* thr_off, const float* thr, int nthr,
                      int nbins, uint64_t* counts, uint64_t* hist, void* ws, size_t ws_bytes, void* stream);

/* ---- Partial FC: the additive-margin head over a per-step sample of the classes (An et al., "Partial FC: Training 10 Million
 * Identities on a Single Machine"; loss.py partial_fc_margin_loss, SphereNet-ArcFace / -CosFace with a sample rate) ----
 * The sample of a step.  With seed `seed`, step number `step`, labels y[0..n), C classes and a fixed sample size S (n <= S <= C):
 *   fmix32(h): h ^= h >> 16; h *= 0x85ebca6b; h ^= h >> 13; h *= 0xc2b2ae35; h ^= h >> 16       (uint32, wrap-around)
 *   base = fmix32(fmix32(seed) + step);  class j gets h_j = fmix32(j + base)
 *   order all classes by the triple (j is not a label of this batch, h_j, j), ascending; the sample is the first S classes: every
 *   class present in the batch, then the other classes with the smallest hashes.  The triple is a total order (and fmix32 a
 *   bijection, so the h_j alone are distinct): the set is unique, whatever the thread scheduling.
 *   index[0..S) = the sample sorted by class id; index[S..Spad) = -1, Spad = S rounded up to 64.
 *   inverse[j] (j < C) = the position of class j in index, -1 for a class outside the sample.
 *   labels_out[i] = inverse[y[i]]; a label outside [0, C) takes no part in the sample and gives labels_out[i] = -1, which the head
 *   kernel answers with a NaN row as for any out-of-range label.
 * The head is fte_margin_softmax_fwd_bwd, unchanged, over the S gathered columns (c = S, ld = Spad) with labels_out: loss_i =
 * logsumexp_{k < S} z_ik - z_i,labels_out[i].  The gradient with respect to x and to the sampled columns of W is the exact one
 * (rowcoef / colcoef as for the dense head); with respect to every other column it is exactly 0.0.
 *
 * fte_pfc_sample: index [Spad], inverse [C], labels_out [n], all int32 and 16-byte aligned; ws >= fte_pfc_sample_ws_bytes(C),
 * cleared by the call (hipMemsetAsync on the stream).  Integer histograms and a compaction in class order: two calls with the same
 * arguments write the same bytes.  Nothing is read back to the host.
 * FTE_EINVAL: a NULL pointer, n < 1, C < 1, S < n or S > C, or a misaligned pointer.  FTE_EWORKSPACE: ws NULL or short. */
size_t fte_pfc_sample_ws_bytes(int C);
int fte_pfc_sample(const int32_t* labels, int n, int C, int S, uint32_t seed, uint32_t step, int32_t* index, int32_t* inverse,
                   int32_t* labels_out, void* ws, size_t ws_bytes, void* stream);
/* Ws[d, k] = W[d, index[k]] for k < S, 0 for S <= k < Spad (and for an index outside [0, C)).  W [D, cpad], Ws [D, Spad], row-major.
 * The sampled column norms are fte_col_norms of Ws.
 * FTE_EINVAL: a NULL pointer, D < 1, C < 1, cpad < C, S < 1, Spad < S, Spad % 4, or index / Ws not 16-byte aligned. */
int fte_pfc_gather_cols(const float* W, const int32_t* index, float* Ws, int D, int C, int cpad, int S, int Spad, void* stream);
/* dW[d, j] = dWs[d, inverse[j]] where 0 <= inverse[j] < S, else 0.0 (j >= C: 0.0), for every j < cpad: one pass that writes each
 * element of dW exactly once, so whatever dW held before (NaNs included) is gone.  dWs [D, Spad], dW [D, cpad].
 * FTE_EINVAL: a NULL pointer, D < 1, C < 1, cpad < C, cpad % 4, S < 1, Spad < S, or dW not 16-byte aligned. */
int fte_pfc_scatter_cols(const float* dWs, const int32_t* inverse, float* dW, int D, int C, int cpad, int S, int Spad, void* stream);
/* The optimizer update of the classifier straight from the compact gradient: fte_pfc_scatter_cols followed by fte_momentum_update /
 * fte_adam_update over the D * cpad range, in one pass that never forms the dense dW.  For every d < D, j < cpad:
 *   g = dWs[d, inverse[j]] where j < C and 0 <= inverse[j] < S, else 0.0 (the padding columns j >= C: 0.0; the padding columns
 *   S <= k < Spad of dWs are never read), then fte_momentum_update's / fte_adam_update's arithmetic on W[d, j] and its slots with
 *   the same scalars (Adam: the same double-precision lr_t computed on the host from lr, b1, b2, t).
 * The bytes of W and of the slots after the call equal those after the two-call sequence (NaN and signed-zero patterns included):
 * dense-optimizer semantics, so the unsampled columns still decay and still move by their momentum; only the traffic of the dense
 * dW (one write, one read) is gone.  W, acc / m, v [D, cpad]; dWs [D, Spad]; inverse [C] as fte_pfc_sample writes it.
 * FTE_EINVAL: a NULL pointer, D < 1, C < 1, cpad < C, cpad % 4, S < 1, Spad < S, t < 1 (Adam), or W, a slot or inverse not
 * 16-byte aligned. */
int fte_pfc_momentum_update_cols(float* W, float* acc, const float* dWs, const int32_t* inverse, int D, int C, int cpad, int S, int Spad,
                                 float lr, float mom, float wd, float gscale, void* stream);
int fte_pfc_adam_update_cols(float* W, float* m, float* v, const float* dWs, const int32_t* inverse, int D, int C, int cpad, int S,
                             int Spad, float lr, float b1, float b2, float eps, float wd, float gscale, int t, void* stream);

/* ---------------------------------------------------------------------------
 * Clustering: link rules over kNN lists and connected components (cluster.py, verification.py).
 * Grouping the embeddings of an unlabelled or badly labelled list into identities.  The input is the neighbour lists exactly as
 * fte_topk_search writes them for a leave-one-out search of a set against itself: scores [n, k] fp32 and index [n, k] int32 with
 * 1 <= k <= 64, n * k < 2^29, index values global row numbers.  A slot (a, t) is VALID iff 0 <= index[a,t] < n and
 * index[a,t] != a; every other slot is a hole (the (-inf, -1) tails, garbage, self): a hole never links, is never a member of a
 * list, and is never followed, so bad indices cannot cause an out-of-bounds access.  Both link rules write a keep mask
 * uint8 [n, k] (1 or 0 in every slot); fte_components turns either mask into labels.  Everything after the fp32 scores is
 * integer logic: the results are exact and do not depend on execution order.  Like the evaluation entry points these neither
 * allocate nor synchronise, and no host loop waits on the device.
 * FTE_EINVAL (all three): a NULL pointer, n < 1, k outside 1..64, n * k >= 2^29.
 * ------------------------------------------------------------------------- */

/* Cosine threshold on the (mutual) kNN graph.  With b = index[a,t]: keep[a,t] = 1 iff the slot is valid, scores[a,t] >= min_score,
 * and, when mutual != 0, some slot u of row b has index[b,u] == a and scores[b,u] >= min_score.  A NaN score compares false. */
int fte_knn_links_threshold(const float* scores, const int32_t* index, int n, int k, float min_score, int mutual, uint8_t* keep,
                            void* stream);
/* Approximate rank-order links (Otto, Wang, Jain, "Clustering Millions of Faces by Identity", TPAMI 2018).  L_a is the list
 * (a, index[a,0], ..., index[a,k-1]) at positions 0..k; its members are a and its valid entries (an entry repeated in a row
 * counts at its first position only; fte_topk_search never writes one).
 *     r(a,b) = 1 + the smallest t with index[a,t] == b, or k + 1 if there is none;
 *     m(a,b) = the number of positions p in 0..min(r(a,b), k) of L_a whose entry is a member of L_a and not a member of L_b.
 * With b = index[a,t]: keep[a,t] = 1 iff the slot is valid, scores[a,t] >= min_score (min_score = -inf turns the floor off), and
 *     (float)(m(a,b) + m(b,a)) < theta * (float)min(r(a,b), r(b,a))        (exactly this fp32 expression: one rounded product)
 * The distance is symmetric in (a, b): a pair listed from both sides gets the same answer from both.
 * FTE_EINVAL also: theta not finite or <= 0. */
int fte_knn_links_rank_order(const float* scores, const int32_t* index, int n, int k, float theta, float min_score, uint8_t* keep,
                             void* stream);
/* Connected components of the graph whose edges are the slots with keep[a,t] != 0 that are valid (a -- index[a,t]; a link from
 * either side is enough).  label[i] = the smallest row number of i's component, int32 [n].  parent: int32 [n] workspace, fully
 * rewritten by the call.  A lock-free union-find in three launches on the stream (init, link, flatten): links hook the larger
 * root under the smaller with a compare-and-swap and retry from the new roots when the swap loses, so the root of a tree is always
 * its smallest member; no thread waits for another's progress and nothing is driven from the host.  Two calls write identical
 * bytes. */
int fte_components(const int32_t* index, const uint8_t* keep, int n, int k, int32_t* parent /* workspace [n] */, int32_t* label /* [n] */,
                   void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FTE_H_ */
