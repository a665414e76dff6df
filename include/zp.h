/*
 * zp.h -- C ABI of libzp.so, the MI355X (gfx950) implementation of ZebraPose's
 * data-parallel hot path.
 *
 * Plain C: pointers, sizes and POD structs only; no torch types.  Every pointer
 * argument named x / y / w / res / ... is a DEVICE pointer (caller-owned memory,
 * e.g. the PyTorch caching allocator); `stream` is a hipStream_t (NULL = legacy
 * default stream).  All calls are stream-ordered and never synchronise the host.
 * Return value: 0 (ZP_OK) or an error code; zp_last_error() describes the last
 * failure of the calling thread.
 *
 * Layouts.  Activations are NHWC ("channels last") with a row stride `ld*`
 * (elements per pixel) and a channel offset `c*0`, so a producer can write
 * straight into a channel slice of a concat buffer (the reference's torch.cat,
 * aspp.py:101-112).  Packed conv weights are [rows_pad][k_pad] with
 * k = tap * Cin + cin ("tap-major implicit GEMM").
 *
 * Reference interfaces replaced (file:line in lyltc1/ZebraPose):
 *   zp_conv2d          nn.Conv2d / nn.ConvTranspose2d + BatchNorm2d + ReLU (+ residual add)
 *                      as called at model/resnet.py:41-51, torchvision resnet children
 *                      (resnet.py:191-199), model/aspp.py:60-80, 89-112
 *   zp_conv2d_wgrad    their weight gradients (autograd of the same modules, train_v6.py:337)
 *   zp_bn_*            BatchNorm2d train/eval semantics (resnet.py:29, aspp.py:12..)
 *   zp_maxpool3s2      torchvision maxpool (resnet.py:197), and its backward
 *   zp_global_avgpool  aspp.py:94  AdaptiveAvgPool2d(1)   (+ zp_broadcast_hw = aspp.py:96 bilinear 1x1->HxW)
 *   zp_code_loss       BinaryCodeLoss / HammingLoss / BinaryLossWeighted (model/BinaryCodeNet.py:8-81,
 *                      96-109) as driven at train_v6.py:325-327;  zp_mask_loss  MaskLoss (:84-93)
 *   zp_threshold       common_ops.py:5-19 (sigmoid > 0.5 -> {0,1})
 *   zp_decode          binary_code_helper/CNN_output_to_pose.py:34-64, 100-130 and
 *                      class_id_encoder_decoder.py:17-28 (bits -> id -> LUT -> 2D/3D)
 *   zp_decode_unique   binary_code_helper/CNN_output_to_pose.py:67-91 (one 2D-3D pair per class id)
 *   zp_lut_coarsen     binary_code_helper/generate_new_dict.py:4-33 (ignore_bit LUT)
 *   zp_ce_loss, zp_code_digits, zp_decode_radix, zp_pack_digits
 *                      the d-ary code ablation (config_ablation/exp_lmo_ablation_*: 'CE' loss,
 *                      common_ops.py:21-28, class_id_encoder_decoder.py:17-28, 43-63)
 *   zp_augment         apply_augmentation (bop_dataset_pytorch.py:349-355): the imgaug colour chain of
 *                      GDR_Net_Augmentation.py:161-178 ahead of the is_train crop (:267-277)
 *   zp_crop_image_m, zp_crop_gt_m, zp_augment_m
 *                      the crops with resize_method "crop_square_resize" (bop_dataset_pytorch.py:36-72) or
 *                      "crop_resize" (:74-88, the paper and ablation configs)
 *   zp_adam            torch.optim.Adam step used by train_v6.py:268-269, 338
 *   zp_render          the OpenGL GT renderer Binary_Code_GT_Generator/Render_GT_Color_Mesh_to_GT_Img
 *                      (render_related_source/opengl_render.cpp:164-206, camera.hpp:29-59,
 *                      shader_groundtruth.vs / .fs) driven by generate_training_labels_for_BOP_v2.py:77-85
 *   zp_mesh_code       the offline coder Binary_Code_GT_Generator/Generate_Mesh_with_GT_Color
 *                      (Generate_Mesh_with_GT_Color.cpp:61-218 balanced 2-means split, :322-455 vertex /
 *                      face ids and the class -> 3D-point LUT), binary splits
 *   zp_mesh_code_radix the same tool run with divide_number_each_itration = 4 / 16 / 256 (the code-radix
 *                      ablation): a balanced d-way split per level, restated (the reference balances
 *                      classes 0 and 1 only)
 *   zp_mesh_subdivide  step 1 of Binary_Code_GT_Generator/Generate_GT.md (:90-92): Meshlab's 'subdivision
 *                      surface: mid point' filter, run by hand there until the mesh has > 2^16 vertices
 *   zp_mask_contour    the visible contour handed to the refinement (test.py:300-307: cv2.findContours
 *                      of the entire mask, the visible-mask filter, mapping_pixel_position_to_original_position)
 *   zp_edge_refine_step  one iteration of py_edge_refine (edge_refine/examples/edge_refine.cpp:68-173:
 *                      cv::findContours of the rendered silhouette, the nearest-contour match, the
 *                      6 x 6 normal equations and the pose update), on zp_render's depth
 *   zp_scene_depth, zp_gt_info
 *                      the files the loader reads beside the GT code images: the mask_visib PNGs and
 *                      scene_gt_info.json (bbox_visib: bop_dataset_pytorch.py:249, 411; visib_fract:
 *                      tools_for_BOP/bop_io.py:71-72, 269-270), with the visibility test of
 *                      lib/pysixd/visibility.py:29-36 ('bop19' and 'bop18')
 *   zp_scene_compose   no program of the reference: whole cluttered frames (the BlenderProc 'pbr' frames
 *                      train_v6.py:138-178 mixes in through second_dataset_ratio) composed from
 *                      zp_render_shaded's per-instance renders, with exact visible masks
 */
#ifndef ZP_H_
#define ZP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ZP_ABI_VERSION 4

#define ZP_OK 0
#define ZP_ERR_ARG 1
#define ZP_ERR_HIP 2

/* element types of activations / packed weights */
#define ZP_F32 0
#define ZP_BF16 1
#define ZP_F16 2 /* IEEE fp16 storage + v_mfma_f32_16x16x32_f16; inference (forward) kernels only */
/* fp32 in split form (eval-mode inference): a tensor is THREE contiguous bf16 planes [3][...], the
 * pointer names plane 0, plane p starts p plane-sizes later (plane size = the tensor's element
 * count: N*H*W*ld for an activation, rows_pad*k_pad for packed weights, N*C for a pooled vector).
 * v = hi + mid + lo exactly (hi = bf16(v), mid = bf16(v - hi), lo = bf16(v - hi - mid)).  zp_conv2d
 * forms every product a*b from the six terms of magnitude >= 2^-16 |a b| (hi*hi, hi*mid, mid*hi,
 * hi*lo, mid*mid, lo*hi) on bf16 MFMAs with f32 accumulation: the dropped terms are below
 * 2^-23 |a b| (f32's own product rounding is 2^-24), i.e. f32-accurate convolutions at 6/16 of the
 * f32-MFMA cost.  Forward (eval) kernels only. */
#define ZP_F32X3 3
/* fp32 in the two-plane fp16 split form (eval-mode inference), laid out like ZP_F32X3 with TWO
 * planes [2][...] of IEEE fp16: hi = fp16(v), lo = fp16((v - hi) * 2^11), v = hi + lo * 2^-11 to
 * 22 significant bits (|error| <= 2^-23 |v| for |v| >= 2^-13, 2^-36 below; |v| must stay below 65504).
 * zp_conv2d forms a*b from hi*hi + (hi*lo + lo*hi) * 2^-11 on fp16 MFMAs (the dropped lo*lo term is
 * below 2^-22 |a b|): 3 MFMAs and 2 staged planes per product instead of ZP_F32X3's 6 and 3.
 * Forward (eval) kernels only. */
#define ZP_F32H2 4

/* Range guard of ZP_F32H2.  A finite value at or above 65520 in magnitude has no two-plane form
 * (hi rounds to fp16 infinity); a WEIGHT at or above 32 (65504 / 2^11) has none for the wide-tile
 * conv, which forms 2^11 * hi in fp16.  Every ZP_F32H2 store -- the zp_conv2d epilogues (split-K's
 * included), zp_im2col_split, the f32 stem writing ZP_OUT_NHWC_H2 and zp_pack_weight(_multi), the
 * latter with the weight bound -- sets *flag = 1 (a device word) when it meets one; nothing clears it.  The flag is per device
 * (the calling thread's current device at registration; launches read it at enqueue time, so a
 * captured hipGraph keeps the word of its capture).  NULL unregisters.  The max / average pools and
 * broadcasts of split tensors cannot leave the range of their inputs and do not check.  The Python
 * engine registers one word, reads it once per fp32 eval forward and re-runs an overflowing forward
 * on the full-range ZP_F32X3 form (reference forward: model/BinaryCodeNet.py:161-174, plain f32). */
int zp_split_range_flag(unsigned int* flag);

/* zp_conv_args.out_mode */
#define ZP_OUT_NHWC 0       /* y[n, oy, ox, cy0 + c] (ldy elements per pixel), dtype of the call */
#define ZP_OUT_HEAD_NCHW 1  /* c == 0 -> y (f32 [N,1,OH,OW]); c >= 1 -> y2 (f32 [N,Cout-1,OH,OW]) */
#define ZP_OUT_NHWC_F32 2   /* y f32 NHWC regardless of dtype (raw conv output for train-mode BN) */
#define ZP_OUT_NHWC_X3 3    /* y = plane 0 of a ZP_F32X3 NHWC tensor (an f32 call writing split output) */
#define ZP_OUT_NHWC_H2 4    /* y = plane 0 of a ZP_F32H2 NHWC tensor (an f32 call writing split output) */

#define ZP_MAX_TAPS 64
#define ZP_MAX_SUB 4

/* One implicit-GEMM sub-problem.  Grid point (n, gy, gx), tap t reads input pixel
 * (gy*sy + ty[t], gx*sx + tx[t]) (zero outside) and writes output pixel
 * (gy*oys + oyo, gx*oxs + oxo).  This covers strided/dilated convs, the four
 * sub-pixel phases of ConvTranspose2d(3, s2, p1, op1), and the data-gradient
 * convs of both. */
typedef struct zp_conv_sub {
  const void* w;        /* packed weights [rows_pad][k_pad], dtype of the call */
  const float* scale;   /* per-output-channel multiplier (folded BN) or NULL (=1) */
  const float* shift;   /* per-output-channel addend (folded BN + bias) or NULL (=0) */
  void* y;              /* output (see out_mode) */
  void* y2;             /* second output (ZP_OUT_HEAD_NCHW) */
  int ldy, cy0, OH, OW;
  int oys, oyo, oxs, oxo;
  int ntaps;            /* taps in ty/tx (general path) */
  int kw, dil, pad;     /* arithmetic taps for the small-Cin path: t -> ((t/kw)*dil-pad, (t%kw)*dil-pad) */
  signed char ty[ZP_MAX_TAPS];
  signed char tx[ZP_MAX_TAPS];
} zp_conv_sub;

typedef struct zp_conv_args {
  int dtype;            /* ZP_F32 (exact-f32 MFMA path), ZP_BF16 or ZP_F16 (16-bit MFMA, fp32 accumulate),
                           ZP_F32X3 (split fp32: x / w / res in 3 planes, Cin a multiple of 32) */
  const void* x;        /* input NHWC */
  int ldx, cx0, IH, IW, Cin;   /* Cin: multiple of 64 (bf16) / 32 (f32), or 8 (small-Cin path) */
  int N, GH, GW, sy, sx;       /* GEMM grid (pixels) and input stride */
  int Cout, k_pad;             /* k_pad: weight row length (elements) */
  int w_rows;                  /* packed weight rows (>= Cout, multiple of the cout tile: use
                                  zp_conv_rows_pad(Cout)) */
  const void* res;             /* residual NHWC (same pixel as y) or NULL */
  int ldr, cr0;
  int relu, out_mode;
  float* stats;                /* if non-NULL (raw output only: no scale/shift/res/relu): per-channel
                                  partial statistics of the stored value, [3][parts][Cout] =
                                  (count, mean, centred M2), parts = zp_conv2d_stat_parts() */
  int nsub;
  zp_conv_sub sub[ZP_MAX_SUB];
  /* ABI 3.  Data-gradient launches (ZP_F32 / ZP_BF16, NHWC, no scale / shift / residual / ReLU / stats):
   * if bnr_part is non-NULL the launch also takes the reduce of zp_bn_bwd_reduce (relu mode 2) for the
   * train-mode BatchNorm whose OUTPUT gradient it writes -- g = the stored value, masked by
   * fma(x, save scale, save shift) > 0, xhat = (x - mean) * invstd -- per stat part:
   * partials[0][k][c] = sum g, partials[1][k][c] = sum g * xhat over stat part k, in the
   * [2][parts + 1][Cout] layout of zp_bn_bwd_reduce with parts = zp_conv2d_bnr_parts(); finish with
   * zp_bn_bwd_totals.
   * Valid only when this launch is the gradient's only writer (it overwrites every pixel).
   * Replaces the separate reduce pass of the BN backward (reference model/resnet.py:41-51, autograd
   * of nn.BatchNorm2d + ReLU) */
  const void* bnr_x;       /* that BN's raw conv output x [P][Cout] (dtype) */
  const float* bnr_save;   /* its zp_bn_train_finalize save: mean, invstd, scale, shift ([4][Cout]) */
  float* bnr_part;
} zp_conv_args;

int zp_abi_version(void);
const char* zp_last_error(void);

/* ---- convolution (forward and data-gradient) ---------------------------------------- */
int zp_conv2d(const zp_conv_args* a, void* stream);
/* packed weight row count zp_conv2d expects for Cout output channels */
int zp_conv_rows_pad(int Cout);
/* number of pixel tiles (grid_x) a zp_conv2d launch with these args uses */
int zp_conv2d_grid(const zp_conv_args* a);
/* number of partial-sum slots `stats` needs: one per pixel tile and sub-problem (round 5: the conv
 * kernels merge their wave halves in LDS first; the split-fp32 forms and k_conv_strip, ZP_CONV_FLAGS
 * without 64, keep one per wave half: (pixel tile / 64) * grid_x * nsub) */
int zp_conv2d_stat_parts(const zp_conv_args* a);
/* number of partial-sum slots a launch with bnr_part emits: zp_conv2d_stat_parts, or one per
 * 256-pixel tile where the strip kernel sums its wave halves first (ABI 3) */
int zp_conv2d_bnr_parts(const zp_conv_args* a);
/* launch configuration zp_conv2d picks: cout tile, pixel tile, LDS ring depth, kernel variant
 * (0 = k_conv, 1 = k_conv_strip: 3x3 stride-1 convs with activation-strip reuse, 2 = k_conv_strip2:
 * the same with the lean main loop, 3 = k_conv_quad: the four phases of a stride-2 transposed
 * structure in one tile, 4 = k_conv3: the split-fp32 (ZP_F32X3) kernel, 5 = k_conv3s: its 3x3
 * stride-1 form with activation-strip reuse, 6 = k_conv3w: the 256 x 256 two-plane tile, 7 = k_conv1x1n: a
 * 1x1 with 32 / 64 input channels and a wide output, the weights held in LDS) */
int zp_conv2d_config(const zp_conv_args* a, int* tc, int* tp, int* stages, int* variant);
/* Split-fp32 forms (ZP_F32X3 / ZP_F32H2) only: a launch whose grid would leave most CUs idle (an
 * NHWC conv -- one sub-problem or several: ConvT phases, merged ASPP branches -- with under 256
 * workgroups, e.g. bs = 1) is cut along K into slices whose f32
 * sums are finished (summed in slice order, then BN / residual / ReLU / split store) by a second
 * kernel, when zp_conv_args.stats points to an f32 workspace of this many bytes (0: not split;
 * stats NULL: not split).  Deterministic. */
long long zp_conv2d_split_ws(const zp_conv_args* a);
/* runtime tuning knobs (tests / sweeps): key 0 = minimum workgroup count for the 256-channel
 * tile (default 1024); key 1 = conv schedule flags (-1 = ZP_CONV_FLAGS or the default); key 2 =
 * 64-channel layers on the strip kernel (default 1); key 3 = the lean weight-gradient kernel
 * (default 1); key 4 = its workgroup rounds over the CUs (default 1); key 5 = the general
 * weight-gradient kernel's workgroup rounds (default 1; 0 = a ~1024-workgroup target); key 6 = the
 * fewest workgroups the four-phase kernel (k_conv_quad) runs with (default 256); key 7 = the
 * split-fp32 strip kernel k_conv3s (0 off, 1 64-channel tiles, 2 also 128-channel tiles; -1 =
 * ZP_CONV3_STRIP or the default 1); key 8 = the fewest workgroups a split-fp32 launch runs
 * 128-channel tiles with (fewer: 64-channel tiles); key 9 = split-K of small split-fp32 launches
 * (default 1, 0 off); keys 10-12 = the 256 x 256 two-plane tile (on / fewest workgroups / split-K);
 * key 13 = its accumulation form (0 the flushed correction accumulator, default; 1 one scaled
 * accumulator; 2 per-step partial sums; 3 flushed on the 2^11 scale; 4 a persistent second
 * accumulator); key 14 = its 256 x 128 tile (default 0); key 15 = zp_bn_train_finalize's merge in
 * one launch (1, default) or two (0); key 16 = k_conv3's multi-sub launches with a tile's subs
 * adjacent on one XCD (default 0); key 17 = k_conv3w's multi-sub launches (ConvT phases) with a
 * pixel tile's phases adjacent on one XCD (default 0); key 18
 * = the 256 x 256 two-plane tile on 32x32x16 MFMAs (default 0); key 19 = the ring depth (2, 3, 4) of
 * the register-pipelined two-plane 64-channel tile (default 2); key 20 = persistent workgroups per CU
 * of the two-plane stem (1 or 2, default 1); key 21 = the wide strip tile's next-step pixel fragments
 * read before the step's barrier (1, default) or after it (0); key 22 = the wide strip tile's two
 * wave groups half a K step apart (the ping-pong K loop: 1 on, 0 off; the default decides per
 * geometry; launches that are not one-sub strip launches keep the lock-step loop).  Keys 7, 10 and
 * 13-22 hold -1 until set: the environment (ZP_CONV3_STRIP, ZP_CONV3W, ZP_CONV3W_ACC, ZP_CONV3W_TP128,
 * ZP_BN_FUSED, ZP_CONV3_SUBINT, ZP_CONV3W_SUBINT, ZP_CONV3W_MF32, ZP_CONV3_PIPE_ST, ZP_STEM_WGS,
 * ZP_CONV3W_PFB, ZP_CONV3W_PP) or the default then decides.  Returns the previous value, -1 for an unknown key. */
int zp_conv_tuning(int key, int value);

/* Fused 1x1 head (the reference's conv_1x1_4 over torch.cat([x, x_128]) and the mask / code split,
 * model/aspp.py:112 + model/BinaryCodeNet.py:172).  The conv of *a (one sub, NHWC, BN scale / shift,
 * bias, residual and ReLU applied as by zp_conv2d) is NOT stored: each output pixel's Cout channels,
 * followed by the C2 channels of x2 at the same pixel (NHWC of a's dtype, [N][OH][OW][ldx2], channels
 * cx20..), feed a 1x1 conv with hcout <= 32 outputs: weights w packed by zp_pack_weight(a's dtype,
 * rows_pad 32, k = channel, k_pad >= Cout + C2), bias (f32 [hcout] or NULL).  Output f32 NCHW:
 * channel 0 -> mask [N][1][OH][OW], channels 1.. -> code [N][hcout-1][OH][OW].
 *   ZP_F32H2: the 256 x 256 two-plane tile runs the conv and the whole head (one launch).
 *   ZP_BF16 / ZP_F16 (eval, ABI 2): the 3x3 conv runs on the strip tile (two 128-channel cout tiles);
 *   each tile's head sums over its channels (the first tile's also over x2) go to ws, f32
 *   [2][32][N*OH*OW] (zp_conv2d_head_ws bytes), and a second launch adds the two in a fixed order,
 *   plus the bias: deterministic.
 * zp_conv2d_head_ok: 1 if *a has a geometry the fused kernels take (e.g. not at bs = 1 for
 * ZP_F32H2, where the unfused path runs). */
typedef struct zp_head_args {
  const void* w;
  int k_pad;
  const float* bias;
  int cout;
  const void* x2;
  int ldx2, cx20, C2;
  float* mask;
  float* code;
  float* ws;  /* ABI 2: the 16-bit path's partial sums (zp_conv2d_head_ws bytes); ignored by ZP_F32H2 */
} zp_head_args;
int zp_conv2d_head_ok(const zp_conv_args* a);
long long zp_conv2d_head_ws(const zp_conv_args* a);
int zp_conv2d_head(const zp_conv_args* a, const zp_head_args* h, void* stream);

/* Pack an f32 weight tensor src[d0][d1][kh][kw] into dst[rows_pad][k_pad] (dtype), taps
 * (ky[t], kx[t]), t < ntaps:
 *   transposed == 0: dst[r][t*cstride + c] = src[r][c][ky[t]][kx[t]]   (conv forward: OIHW)
 *   transposed == 1: dst[r][t*cstride + c] = src[c][r][ky[t]][kx[t]]   (ConvT forward, conv dgrad)
 * ky/kx are HOST arrays (<= ZP_MAX_TAPS).  Padding rows / columns / channels are zeroed. */
int zp_pack_weight(const float* src, int d0, int d1, int kh, int kw, int transposed, int ntaps,
                   const int* ky, const int* kx, int cstride, int dtype, void* dst, int rows_pad,
                   int k_pad, void* stream);

/* Many zp_pack_weight jobs in one launch (training repacks every conv's weights once per
 * optimizer step).  `jobs` and `prefix` are DEVICE arrays: prefix[i] = sum of rows_pad*k_pad of
 * jobs before i (prefix[n] = total elements; validated, the kernel maps one grid row per job,
 * n <= 65535).  Same element mapping as zp_pack_weight. */
typedef struct zp_pack_job {
  const float* src;
  void* dst;
  int d0, d1, kh, kw, transposed, ntaps, cstride, rows_pad, k_pad, dtype;
  signed char ky[ZP_MAX_TAPS], kx[ZP_MAX_TAPS];
} zp_pack_job;
int zp_pack_weight_multi(int n, const zp_pack_job* jobs, const long long* prefix, long long total,
                         void* stream);

/* ---- weight gradient ------------------------------------------------------------------
 * dw[co][ci][ky][kx] (f32, layout of the conv's own weight; transposed_w=1 for ConvT's
 * [ci][co][kh][kw]) = sum over grid points and taps of dy[out pixel][co] * x[in pixel][ci],
 * with the same sub/tap geometry as the forward zp_conv_args (sub[].y = dy, dtype = act dtype).
 * `ws` is a device workspace of zp_conv2d_wgrad_ws_bytes() bytes. accumulate != 0 adds to dw. */
typedef struct zp_wgrad_args {
  int dtype;
  const void* x; int ldx, cx0, IH, IW, Cin;
  int N, GH, GW, sy, sx;
  int Cout;
  int Cw;                      /* input channels of the weight tensor (<= Cin; Cin may be padded) */
  int kh, kw, transposed_w;
  int nsub;
  struct {
    const void* dy; int lddy, cdy0, OH, OW, oys, oyo, oxs, oxo;
    int ntaps;
    signed char ky[ZP_MAX_TAPS], kx[ZP_MAX_TAPS];   /* weight tap of each geometric tap */
    signed char ty[ZP_MAX_TAPS], tx[ZP_MAX_TAPS];
  } sub[ZP_MAX_SUB];
  float* dw;
  int accumulate;
} zp_wgrad_args;
long long zp_conv2d_wgrad_ws_bytes(const zp_wgrad_args* a);
int zp_conv2d_wgrad(const zp_wgrad_args* a, void* ws, void* stream);

/* ---- batch norm ---------------------------------------------------------------------- */
/* eval: scale = gamma / sqrt(var + eps); shift = beta + (bias - mean) * scale (bias may be NULL) */
int zp_bn_fold(const float* gamma, const float* beta, const float* mean, const float* var,
               const float* conv_bias, float eps, int C, float* scale, float* shift, void* stream);
/* train: merge the [3][parts][C] partial statistics of zp_conv2d(stats); the merged count is the sum
 * of the parts' own counts (parts of count 0 add nothing).  `count` is the caller's pixel count P: it
 * must be positive and is NOT compared with that sum (the parts live on the device; a check would
 * put a synchronisation into the training step).  Then
 * update running stats (momentum, unbiased var; the conv bias, if any, is added to the mean)
 * and emit scale/shift for the apply pass, plus save[4][C] = (mean, invstd, scale, shift) of the
 * raw values (shift = fma(-mean, scale, beta)).
 * partials is scratch: a first merge level overwrites it in place (every 64th part).
 * ABI 4: partials holds zp_bn_finalize_floats(parts, C) floats -- the [3][parts][C] statistics and,
 * past them, the one-launch merge's per-launch hand-off counters (zeroed on `stream` by this call),
 * so concurrent finalizes on different streams or hipGraphs never share counters. */
int zp_bn_train_finalize(float* partials, int parts, int C, long long count, float eps,
                         float momentum, const float* gamma, const float* beta, const float* conv_bias,
                         float* running_mean, float* running_var, int64_t* num_batches_tracked,
                         float* scale, float* shift, float* save, void* stream);
/* size in floats of zp_bn_train_finalize's partials buffer for (parts, C) (ABI 4) */
long long zp_bn_finalize_floats(int parts, int C);
/* y[p, cy0+c] = act(fma(x[p, c], scale[c], shift[c]) (+ res[p, cr0+c])), x: raw conv output [P][C] */
int zp_bn_apply(const void* x, int P, int C, const float* scale, const float* shift,
                const void* res, int ldr, int cr0, int relu, int dtype, void* y, int ldy, int cy0,
                void* stream);
/* number of partial slots zp_bn_bwd_reduce uses for P pixels (partials needs [2][parts+1][C]) */
int zp_bn_bwd_parts(int P, int C);
/* backward of y = act(bn(x) (+res)):  g = dy * mask;  xhat = (x - mean) * invstd;
 * relu 0: no mask; 1: mask = y > 0 (y read); 2: mask = fma(x, save scale, save shift) > 0, recomputed
 * from the raw x exactly as zp_bn_apply formed y (no residual) -- y is not read and may be NULL;
 * partials[0][k][c] = sum g, partials[1][k][c] = sum g*xhat over pixel block k (x == NULL: only sum g);
 * then totals into partials[.][parts][c] and (optional) dgamma = sum g*xhat, dbeta = sum g
 * (written, or added if accumulate).
 * C, lddy, cdy0 (and ldy, cy0 for relu 1) are multiples of the 16-byte vector (8 elements, f32: 4): checked. */
int zp_bn_bwd_reduce(const void* dy, int lddy, int cdy0, const void* y, int ldy, int cy0,
                     const void* x, int P, int C, const float* save, int relu, int dtype,
                     float* partials, float* dgamma, float* dbeta, int accumulate, void* stream);
/* totals of partials [2][parts + 1][C] filled by a zp_conv2d launch with bnr_part (parts =
 * zp_conv2d_bnr_parts) -> partials[0][out_parts][c], partials[1][out_parts][c] of the [2][out_parts
 * + 1][C] layout zp_bn_bwd_apply reads (out_parts = zp_bn_bwd_parts(P, C); the buffer holds
 * [2][max(parts, out_parts) + 1][C]); dgamma / dbeta as zp_bn_bwd_reduce */
int zp_bn_bwd_totals(float* partials, int parts, int C, int out_parts, float* dgamma, float* dbeta,
                     int accumulate, void* stream);
/* dx[p][c] = gamma*invstd*(g - sum_g/P - xhat*sum_gx/P)  (dx dtype, [P][C]); relu as for the
 * reduce (mode 2 needs dx);
 * dres (optional) [p, cdres0+c] = g, or += g if res_accumulate; alignment as for the reduce, lddres and
 * cdres0 included (checked) */
int zp_bn_bwd_apply(const void* dy, int lddy, int cdy0, const void* y, int ldy, int cy0,
                    const void* x, int P, int C, const float* save, const float* partials,
                    const float* gamma, int relu, int dtype, void* dx, void* dres, int lddres,
                    int cdres0, int res_accumulate, void* stream);

/* ---- layout / pooling ---------------------------------------------------------------- */
/* x f32 NCHW [B][C][H][W] -> y NHWC [B][H][W][cpad] (dtype), channels C..cpad-1 zero */
int zp_nchw_to_nhwc(const float* x, int B, int C, int H, int W, int cpad, int dtype, void* y,
                    void* stream);
/* Split-fp32 stem input (ZP_F32X3 / ZP_F32H2): the im2col of an f32 NHWC image x [B][H][W][ldx]
 * (C real channels) for a k x k / stride s / padding p conv -- y [NPL][B][OH][OW][kpad] with
 * element kk = (ky * k + kx) * C + c (kk >= k*k*C and out-of-image taps zero), stored split.  The
 * stem conv (torchvision ResNet conv1 7x7/s2/p3, reference model/resnet.py:195) then runs as a 1x1
 * split-fp32 conv over kpad channels, weights packed with zp_pack_weight(..., cstride = C, ...). */
int zp_im2col_split(const float* x, int B, int H, int W, int ldx, int C, int k, int s, int p, int OH, int OW,
                    int kpad, int dtype, void* y, void* stream);
/* The stem conv of the two-plane engine in one launch (ZP_F32H2 only): torchvision conv1 (7x7,
 * stride 2, pad 3, 3 -> 64 channels; reference model/resnet.py:195) + folded BN (scale, shift) +
 * ReLU, from the f32 image x -- ldx == 0: NCHW [B][3][H][W], the reference's input tensor
 * (bop_dataset_pytorch.py:345; no zp_nchw_to_nhwc copy); else NHWC [B][H][W][ldx] (channels 0..2, ldx a
 * multiple of 4) -- to a ZP_F32H2 NHWC slice y [2][B][OH][OW][ldy] at channel cy0.  Weights:
 * zp_pack_weight of the 7x7 kernel in the zp_im2col_split order (taps row-major, cstride 3, k_pad 160,
 * dtype ZP_F32H2, w_rows >= 64).  Replaces zp_im2col_split + the 1x1 split GEMM (no patch tensor).
 * OW must divide 256 and be <= 128. */
int zp_stem_split(const float* x, int B, int H, int W, int ldx, const void* w, int w_rows, int k_pad,
                  const float* scale, const float* shift, int dtype, void* y, int ldy, int cy0, int OH, int OW,
                  void* stream);
/* 3x3 / stride 2 / pad 1 max pool, NHWC slices; C multiple of 8 */
int zp_maxpool3s2(const void* x, int B, int IH, int IW, int ldx, int cx0, int C, int dtype,
                  void* y, int OH, int OW, int ldy, int cy0, void* stream);
int zp_maxpool3s2_bwd(const void* x, int ldx, int cx0, const void* dy, int lddy, int cdy0,
                      int B, int IH, int IW, int C, int OH, int OW, int dtype,
                      void* dx, int lddx, int cdx0, int accumulate, void* stream);
/* y[b][c] = mean over H*W of x (f32 accumulate), y dtype */
int zp_global_avgpool(const void* x, int B, int H, int W, int ldx, int cx0, int C, int dtype,
                      void* y, void* stream);
/* y[b, :, :, cy0 + c] = src[b][c] */
int zp_broadcast_hw(const void* src, int B, int C, int dtype, void* y, int H, int W, int ldy, int cy0,
                    void* stream);
/* backward of zp_broadcast_hw: out[b][c] (dtype) = sum over H*W of dy[b, h, w, cdy0 + c] */
int zp_sum_hw(const void* dy, int B, int H, int W, int lddy, int cdy0, int C, int dtype, void* out,
              void* stream);
/* backward of zp_global_avgpool: y[b, h, w, cy0 + c] (+)= src[b][c] * mul  (src dtype) */
int zp_add_broadcast_hw(const void* src, float mul, int B, int C, int dtype, void* y, int H, int W,
                        int ldy, int cy0, int accumulate, void* stream);
/* generic NHWC slice copy / add / cast: y[p, cy0+c] (+)= x[p, cx0+c]  */
int zp_copy_slice(const void* x, int ldx, int cx0, int xdtype, void* y, int ldy, int cy0, int ydtype,
                  int P, int C, int accumulate, void* stream);
/* F.interpolate(mask, (OH, OW), mode="bilinear", align_corners=False) of a one-channel f32 NCHW
 * map into channel cy0 of an NHWC concat buffer (BinaryCodeNet_Deeplab_v3: aspp_v3.py:89, 96-101),
 * and its backward (gather form, deterministic) into f32 NCHW dx (accumulate: dx += ...). */
int zp_mask_interp(const float* x, int B, int H, int W, int OH, int OW, int dtype, void* y, int ldy, int cy0,
                   void* stream);
int zp_mask_interp_bwd(const void* dy, int lddy, int cdy0, int B, int OH, int OW, int H, int W, int dtype, float* dx,
                       int accumulate, void* stream);
/* head gradient f32 NCHW (dmask [B][1][H][W], dcode [B][L][H][W]) -> y NHWC [B][H][W][ldy]
 * (dtype), channel 0 = mask, 1..L = code, channels L+1..ldy-1 zeroed */
int zp_head_grad_to_nhwc(const float* dmask, const float* dcode, int B, int L, int H, int W, int ldy,
                         int dtype, void* y, void* stream);

/* ---- loss ---------------------------------------------------------------------------- */
/* loss_b of BinaryCodeLoss('BCE', mask_binary_code_loss=mask_code, 2, use_hist)
 * (model/BinaryCodeNet.py:34-81 with HammingLoss :100-109), f64 like the reference:
 *   code_logits f32 [B][L][H][W];
 *   mask: mask01 (f64 [B][1][H][W], rounded and clamped to {0,1} as HammingLoss does) or, if
 *         mask01 == NULL, mask_logits (f32 [B][1][H][W]) thresholded like train_v6.py:325-326;
 *   gt [B][L][H][W]: f64 if gt_f64 else u8 (0/1);
 *   hist_state f64[L+1]: [0..L) the histogram EMA (module state), [L] = 0 before the first call;
 *   out f64[2] = (loss_b, mean hamming loss); coef f64[L] = w_i / sum(w) / (B*H*W), kept for the
 *   backward.  ws: zp_code_loss_ws_bytes(B, L, H, W) bytes. */
long long zp_code_loss_ws_bytes(int B, int L, int H, int W);
int zp_code_loss(const float* code_logits, const double* mask01, const float* mask_logits, const void* gt,
                 int gt_f64, int B, int L, int H, int W, int use_hist, int mask_code, double* hist_state,
                 double* out, double* coef, void* ws, void* stream);
/* dcode[b][i][p] = gscale * coef[i] * (sigmoid(z) - t) * (mask_code ? m : 1), z = (mask_code ? m : 1) * code;
 * gscale = *grad_scale (f64 device scalar) or 1 if NULL */
int zp_code_loss_bwd(const float* code_logits, const double* mask01, const float* mask_logits, const void* gt,
                     int gt_f64, int B, int L, int H, int W, int mask_code, const double* coef,
                     const double* grad_scale, float* dcode, void* stream);
/* loss_b of BinaryCodeLoss('CE', mask_binary_code_loss=mask_code, d, False) -- the d-ary code
 * ablation (model/BinaryCodeNet.py:23-24, 47-48, 57-60, 65; config_ablation/exp_lmo_ablation_*), f64
 * like the reference (its mask is f64, so z and the cross-entropy are):
 *   code_logits f32 [B][L*d][H][W] (step i's d class logits are channels i*d .. i*d+d-1);
 *   mask: as zp_code_loss (mask01's raw f64 value multiplies the logits, :48);
 *   gt [B][L][H][W]: the digit planes, f64 if gt_f64 else u8, each in [0, d);
 *   z[b][i*d+k][p] = (mask_code ? m[b][p] : 1) * code[b][i*d+k][p];
 *   out f64[1] = mean over (b, i, p) of logsumexp_k z - z[gt]: masked-out pixels count, with log d.
 * Per-block partial sums in a grid fixed by B*L*H*W, then one block in a fixed order:
 * deterministic.  2 <= d <= 256.  ws: zp_ce_loss_ws_bytes(B, L, H, W) bytes. */
long long zp_ce_loss_ws_bytes(int B, int L, int H, int W);
int zp_ce_loss(const float* code_logits, const double* mask01, const float* mask_logits, const void* gt,
               int gt_f64, int B, int L, int d, int H, int W, int mask_code, double* out, void* ws, void* stream);
/* dcode[b][i*d+k][p] = gscale * m * (softmax_k(z) - [k == gt]) / (B*L*H*W) (m = 1 unless mask_code),
 * computed in f64 and rounded once to f32; gscale = *grad_scale (f64 device scalar) or 1 if NULL */
int zp_ce_loss_bwd(const float* code_logits, const double* mask01, const float* mask_logits, const void* gt,
                   int gt_f64, int B, int L, int d, int H, int W, int mask_code, const double* grad_scale,
                   float* dcode, void* stream);
/* MaskLoss (BinaryCodeNet.py:89-93): out f32[1] = mean |sigmoid(x) - g| over n elements
 * (x = mask logits [B][1][H][W] viewed as [B][H][W]); ws: zp_mask_loss_ws_bytes(n) bytes */
long long zp_mask_loss_ws_bytes(long long n);
int zp_mask_loss(const float* mask_logits, const float* gt_mask, long long n, float* out, void* ws, void* stream);
/* dmask = gscale * sign(sigmoid(x) - g) * sigmoid(x) * (1 - sigmoid(x)) / n  (gscale f32 device scalar or NULL) */
int zp_mask_loss_bwd(const float* mask_logits, const float* gt_mask, long long n, const float* grad_scale,
                     float* dmask, void* stream);

/* ---- decode -------------------------------------------------------------------------- */
/* bits (u8, or f64 if out_f64) = logits > 8.940696716308594e-08f  (CPU fp32 sigmoid(x) > 0.5) */
int zp_threshold(const float* logits, long long n, int out_f64, void* bits, void* stream);
/* Per crop b (lut_index[b] selects the LUT when several objects are batched, NULL = 0):
 *   mask = threshold(mask_logits), id = sum_i bit_i << (L-1-i) over code channels 0..L-1,
 *   in row-major order of the mask pixels: xy = (int)(bbox[2]/bbox_size * x + bbox[0]),
 *   (int)(bbox[3]/bbox_size * y + bbox[1]) (truncation toward zero), xyz = lut[id] or 0 if any
 *   component is NaN; counts[b] = number of mask pixels.  ids (optional) = id image [B][H][W].
 *   mask_logits f32 [B][1][H][W], code_logits f32 [B][Lfull][H][W], lut f32 [n_lut][2^L][3],
 *   bbox int32 [B][4], xy int32 [B][H*W][2], xyz f32 [B][H*W][3].  The f64 map is a division, a
 *   multiply and an add, each rounded on its own (numpy's).  L <= 24, B <= 65535.
 *   ws: zp_decode_ws_bytes(B, H, W) bytes. */
long long zp_decode_ws_bytes(int B, int H, int W);
int zp_decode(const float* mask_logits, const float* code_logits, int B, int H, int W, int Lfull,
              int L, const float* lut, const int* lut_index, const int* bbox, int bbox_size,
              int* ids, int* counts, int* xy, float* xyz, void* ws, void* stream);
/* d-ary codes (common_ops.py:21-28, the 'CE' branch): digits [B][L][H][W] (u8, or f64 if out_f64)
 * = argmax_k code_logits[b][i*d+k][p], the lowest k on a tie (np.argmax); code_logits f32
 * [B][L*d][H][W], 2 <= d <= 256 */
int zp_code_digits(const float* code_logits, int B, int L, int d, int H, int W, int out_f64, void* digits,
                   void* stream);
/* zp_decode for d-ary codes (CNN_output_to_pose.py:100-130 with class_base = d): id = sum_i
 * digit_i * d^(L-1-i) (class_id_encoder_decoder.py:17-28) with zp_code_digits' digits over all L
 * steps; lut f32 [n_lut][d^L][3], d^L <= 2^24.  Mask threshold, row-major compaction, truncating
 * bbox map, NaN class -> (0, 0, 0), optional ids, lut_index and ws: as zp_decode. */
int zp_decode_radix(const float* mask_logits, const float* code_logits, int B, int H, int W, int L, int d,
                    const float* lut, const int* lut_index, const int* bbox, int bbox_size, int* ids,
                    int* counts, int* xy, float* xyz, void* ws, void* stream);
/* Unique correspondences (build_unique_2D_3D_correspondence, CNN_output_to_pose.py:67-91): one row
 * per distinct class id under crop b's mask, in the row-major order of each class's first pixel.
 *   d == 2: bit logits as zp_decode (Lfull channels, the top L used); d > 2: L steps of d class
 *   logits as zp_decode_radix (Lfull == L * d); at most 2^24 class ids either way.
 *   mean = (sum x / n, sum y / n) over the class's pixels: exact integer sums, one correctly
 *   rounded f64 division per axis; xy = (int)(bbox[2]/bbox_size * mean_x + bbox[0]), likewise y
 *   (f64 multiply, then add, truncation toward zero); xyz = lut[id] or 0 if any component is NaN.
 *   counts[b] = number of distinct ids; rows at or past counts[b] are unspecified.  Optional:
 *   ids [B][H][W], mult int32 [B][H*W] (pixels per row), mean_xy f64 [B][H*W][2] (crop-space mean).
 *   H * W * max(H, W) < 2^31 (the int32 coordinate sums); B <= 65535.
 *   ws: zp_decode_unique_ws_bytes(B, H, W) bytes (< 48 per pixel plus the tile counts, whatever the
 *   number of classes), filled on `stream` inside the call.  Results are bitwise reproducible. */
long long zp_decode_unique_ws_bytes(int B, int H, int W);
int zp_decode_unique(const float* mask_logits, const float* code_logits, int B, int H, int W, int Lfull,
                     int L, int d, const float* lut, const int* lut_index, const int* bbox, int bbox_size,
                     int* ids, int* counts, int* xy, float* xyz, int* mult, double* mean_xy, void* ws,
                     void* stream);
/* out[n][3] (f32) = mean over the 2^(old-new) children of lut64 (f64, summed in order) */
int zp_lut_coarsen(const double* lut64, int old_bits, int new_bits, float* out, void* stream);

/* ---- pose ---------------------------------------------------------
 * Batched RANSAC-EPnP, replacing cv2.solvePnPRansac(P3D, P2D, K, None, reprojectionError,
 * iterationsCount, flags=SOLVEPNP_EPNP) at binary_code_helper/CNN_output_to_pose.py:152-156.
 * Inputs are zp_decode's outputs: counts[B], xy int32 [B][HW][2] (original-image pixels),
 * xyz f32 [B][HW][3]; K f64 [B][4] = (fx, fy, cx, cy).  Outputs R f64 [B][9] (row-major),
 * T f64 [B][3], success[B] (RANSAC found a model), inliers[B].  ws: zp_pnp_ws_bytes(B, iters). */
long long zp_pnp_ws_bytes(int B, int iters);
int zp_pnp_ransac(int B, int HW, const int* counts, const int* xy, const float* xyz, const double* K,
                  int iters, double reproj_err, double confidence, double* R, double* T, int* success,
                  int* inliers, void* ws, void* stream);

/* ---- PnP local optimisation -----------------------------------------------------------------
 * The reference's default solver is Progressive-X (binary_code_helper/CNN_output_to_pose.py:132-144),
 * a locally optimised RANSAC; zp_pnp_ransac is its fallback, which ends with one algebraic EPnP fit over
 * the inliers of the best minimal-sample pose.  zp_pnp_lo adds what a local optimisation adds to that:
 * the consensus set is re-selected from the fitted pose, and the pose becomes the least-squares minimiser
 * of the reprojection error over that set.  It does not restate Progressive-X: no graph cuts, no spatial
 * coherence term, no multi-model proposals; parity with pyprogressivex is not pinned.  The semantics
 * are restated, in numpy, in tests/pnp_lo_ref.py.
 *
 * counts, xy, xyz, K as for zp_pnp_ransac; pose b uses its first n = min(counts[b], HW) rows (a negative
 * count is 0) and rows past that are never read.  R f64 [B][9] row-major, t f64 [B][3]: zp_pnp_ransac's
 * outputs.  active i32 [B] or NULL: 0 skips the crop.  One workgroup per crop, the whole loop in one
 * launch, no host synchronisation, no atomics; all real arithmetic is f64, each step below one IEEE
 * operation (no fused multiply-add), every sum over a fixed partition and a fixed tree: two runs give
 * the same bits, and a crop's result does not depend on its place in the batch or on its neighbours.
 *   projection: p = f64(xyz), (u, v) = f64(xy);
 *               X = ((R00 p.x + R01 p.y) + R02 p.z) + t.x, likewise Y and Z;
 *               e.x = u - ((fx X) / Z + cx), e.y = v - ((fy Y) / Z + cy);  r2 = e.x e.x + e.y e.y.
 *   selection:  S = { i < n : Z > 0, r2 finite and r2 <= thr2 }, thr2 = reproj_err reproj_err, in f64.
 *               zp_pnp_ransac tests in f32 (its projection stored as f32, thr2 an f32), so the two
 *               counts may differ by points on the threshold.  The membership mask lives in ws.
 *   rounds:     for r = 0 .. rounds - 1: select S_r under the current pose; stop if |S_r| < 6 (at r = 0:
 *               status 2); stop if r > 0 and S_r = S_(r-1) as sets (masks compared exactly); else run
 *               Levenberg-Marquardt on S_r.
 *   LM:         lambda = 1e-3.  At most `steps` iterations, each: with a = fx / Z, b = fy / Z,
 *               c = -((fx X) / (Z Z)), d = -((fy Y) / (Z Z)) the rows of J = Jp [-[Xc]x | I] are
 *               J0 = (c Y, a Z - c X, -(a Y), a, 0, c), J1 = (d Y - b Z, -(d X), b X, 0, b, d);
 *               H = sum_S (J0 J0^T + J1 J1^T), each entry's term J0r J0c + J1r J1c; g = sum_S (J0 e.x +
 *               J1 e.y); C = sum_S r2.  Solve (H + lambda diag(H)) theta = g by Cholesky (column by
 *               column; a pivot that is not positive and finite is a rejection, never an error).
 *               Trial pose: E = exp([theta_r]x) by Rodrigues (the series below |theta_r| = 1e-8, as
 *               zp_edge_refine_step), R' = E R, t' = E t + theta_t.  C' = sum of r2 under the trial pose
 *               over the same S, +infinity if a point of S has Z <= 0 there.  Accepted iff the
 *               factorisation succeeded, C' is finite and C' < C: the pose is replaced, lambda =
 *               max(0.1 lambda, 1e-9), and LM ends if C - C' <= 1e-10 C.  Rejected: lambda = 10 lambda,
 *               and LM ends if lambda > 1e6 (H, g and C are unchanged and not summed again).
 *   monotone:   the truncated cost M(pose) = sum_(i<n) min(r2_i, thr2), a point that fails the inlier
 *               test counting thr2, never rises: selection does not change M, and an accepted step
 *               lowers sum_S r2 with S fixed and every point of S still in front of the camera, so it
 *               lowers M.  M(R_out, t_out) <= M(R, t) up to the rounding of the sums.
 *   outputs:    R_out, t_out: the final pose.  inliers i32 [B]: the size of the set selected under it;
 *               cost f64 [B]: sum of r2 over that set.
 *   status i32 [B]: 0 refined; 1 skipped (active[b] = 0, n < 6, or a non-finite entry in R or t);
 *               2 fewer than 6 inliers under the input pose.  With 1 and 2 the pose is copied through
 *               bit for bit, cost is 0 and inliers is the count under the input pose (0 with status 1).
 *   Optional outputs (NULL: not written): trace i32 [B][rounds][2] = (|S_r|, LM iterations run; 0 for a
 *   round that stopped after its selection), (-1, -1) for rounds not started (all of them with status
 *   1); Hb f64 [B][28]: for the first LM iteration of round 0 the upper triangle of H by rows (21
 *   values), then g (6), then C; zeros with status 1 and 2.
 *   1 <= rounds, steps <= 64; reproj_err > 0 and finite; 1 <= B <= 65535; 1 <= HW <= 2^24; R_out / t_out
 *   must not be R / t; anything else, or a NULL pointer that is not optional, is ZP_ERR_ARG before any
 *   device call.  ws: zp_pnp_lo_ws_bytes bytes (-1: bad sizes). */
long long zp_pnp_lo_ws_bytes(int B, int HW);
int zp_pnp_lo(int B, int HW, const int* counts, const int* xy, const float* xyz, const double* K, const double* R,
              const double* t, const int* active, double reproj_err, int rounds, int steps, double* R_out,
              double* t_out, int* inliers, double* cost, int* status, int* trace, double* Hb, void* ws, void* stream);

/* ---- pose error ----------------------------------------------------
 * ADD / ADI of B pose pairs over one model's points pts f32 [n][3], replacing
 * metric.py:8-18 (bop_toolkit pose_error.add / adi; lib/pysixd/pose_error.py:297-336).
 * R f64 [B][9] row-major, t f64 [B][3]; out f64 [B].  ADI is an exact nearest-neighbour search. */
#define ZP_METRIC_ADD 0
#define ZP_METRIC_ADI 1
long long zp_pose_error_ws_bytes(int B, int n, int mode);
int zp_pose_error(int B, const float* pts, int n, const double* R_est, const double* t_est,
                  const double* R_gt, const double* t_gt, int mode, double* out, void* ws, void* stream);

/* ---- BOP pose errors: MSSD, MSPD, VSD ----------------------------------------------------------
 * The three errors behind BOP's average recalls (lib/pysixd/pose_error.py:22-179; defaults in
 * lib/pysixd/scripts/eval_calc_errors.py:37-53), batched over B pose pairs of one model.
 * tests/bop_ref.py restates the semantics below in numpy.
 *
 * zp_pose_error_sym: MSSD (pose_error.py:131-153) and MSPD (:156-179) over a set of S symmetry
 * transformations (misc.py:206-254; zebrapose_amd.metric.symmetry_transformations builds it).
 *   pts f32 [n][3]; R_* f64 [B][9] row-major, t_* f64 [B][3]; sym_R f64 [S][9] row-major, sym_t f64
 *   [S][3]; K f64 [B][4] = (fx, fy, cx, cy), read by ZP_METRIC_MSPD only (else it may be NULL);
 *   out f64 [B].  All arithmetic is f64, as in the reference.
 *   Per symmetry s: R_s = R_gt sym_R[s], t_s = R_gt sym_t[s] + t_gt.
 *   MSSD: e_s = max_i || (R_est p_i + t_est) - (R_s p_i + t_s) ||.
 *   MSPD: the same over the projections u = fx X / Z + cx, v = fy Y / Z + cy (misc.py:511-525); there
 *         is no special case for Z <= 0: the reference divides too.
 *   out[b] = min_s e_s.  Squared distances are compared and one square root is taken at the end;
 *   max and min are exact, so the result is bitwise reproducible and independent of how the points
 *   are partitioned.  A NaN distance (possible only with non-finite input or Z = 0) is ignored.
 * 1 <= S <= 4096, n >= 1, B >= 1; anything else, or a NULL pointer, is ZP_ERR_ARG before any device
 * call.  ws: zp_pose_error_sym_ws_bytes bytes (-1: bad sizes or mode).
 *
 * zp_vsd: the pixel stage of VSD (pose_error.py:84-128) on depth images that are already rendered
 * (zebrapose_amd.metric.vsd_errors renders them with zp_render: this rasteriser's depth, not OpenGL's).
 *   depth_est, depth_gt f32 [B][H][W] and depth_test f32 [n_test][H][W], 0 = no surface; pose b reads
 *   test image test_index[b] (i32 [B] on the device; an index outside [0, n_test) is read as the
 *   nearest valid one), or image b when test_index is NULL (then n_test >= B).  K f64 [B][4] as
 *   above.  taus is a HOST array of ntau tolerances (copied at the call); diameter f64 [B] on the
 *   device, or NULL for distances that are not normalised.  out f64 [B][ntau]; counts i32
 *   [B][2 + ntau] = (union, inter, cost_0 ..), or NULL.
 *   Distance image (misc.py:565-588), per pixel (x, y) and image d, every step one IEEE f64
 *   operation: pX = (x - cx) / fx, pY = (y - cy) / fy, z = f64(d),
 *   dist = sqrt(((pX z)^2 + (pY z)^2) + z^2).
 *   Visibility, visib_mode 'bop19' (visibility.py:34-36, 72-73):
 *     visib(m) = (f32(dist_m) - f32(dist_test) <= f32(delta) || dist_test == 0) && dist_m > 0
 *     visib_gt = visib(gt); visib_est = visib(est) || (visib_gt && dist_est > 0).
 *   union / inter = pixel counts of visib_gt | visib_est and visib_gt & visib_est; on the inter
 *   pixels dists = |dist_gt - dist_est|, divided by diameter[b] when given; cost_k = #(dists >=
 *   taus[k]), the 'step' cost (pose_error.py:117-118).
 *   out[b][k] = f64(cost_k + (union - inter)) / f64(union), or 1.0 when union == 0.
 *   Every counter is an integer, so the result is exact and independent of the order of the pixels.
 * Left out: the 'tlinear' cost (pose_error.py:119-121) and visib_mode 'bop18' (visibility.py:29-32).
 * 1 <= ntau <= 32, 1 <= B <= 65535, H, W >= 1, H * W < 2^31 - 1024, n_test >= 1; anything else, or a
 * NULL pointer other than test_index, diameter and counts, is ZP_ERR_ARG before any device call.
 * ws: zp_vsd_ws_bytes bytes (-1: bad sizes). */
#define ZP_METRIC_MSSD 2
#define ZP_METRIC_MSPD 3
long long zp_pose_error_sym_ws_bytes(int B, int n, int S, int mode);
int zp_pose_error_sym(int B, const float* pts, int n, const double* R_est, const double* t_est,
                      const double* R_gt, const double* t_gt, const double* K, const double* sym_R,
                      const double* sym_t, int S, int mode, double* out, void* ws, void* stream);
long long zp_vsd_ws_bytes(int B, int H, int W, int ntau);
int zp_vsd(int B, const float* depth_est, const float* depth_gt, const float* depth_test, int n_test,
           const int* test_index, int H, int W, const double* K, double delta, const double* taus, int ntau,
           const double* diameter, double* out, int* counts, void* ws, void* stream);

/* ---- BOP GT masks and info -----------------------------------------------------------------
 * The visible mask of every instance (the mask_visib PNGs) and the entries of scene_gt_info.json, which
 * the reference's loader reads (bop_dataset_pytorch.py:249, 411: bbox_visib; tools_for_BOP/bop_io.py:
 * 71-72, 269-270 and lib/pysixd/scripts/eval_calc_scores.py:215: visib_fract) and which in a BOP
 * dataset come from the BOP toolkit's calc_gt_masks.py / calc_gt_info.py.  The toolkit is not part
 * of the reference: for px_count_all, the large render and the empty-box rule the text below is the
 * specification.  tests/gtinfo_ref.py restates both functions in numpy; the outputs match it exactly.
 *
 * zp_scene_depth: the depth image of each of n_img synthetic scenes from its instances' renders.
 *   depth f32 [B][H][W]: zp_render's camera Z, 0 = no surface; img_index i32 [B] (device): the image
 *   instance b belongs to, in any order, several instances per image; an index outside [0, n_img)
 *   contributes nothing.
 *   scene f32 [n_img][H][W] = the smallest depth > 0 over the image's instances, 0 where there is none;
 *   instance i32 [n_img][H][W] (may be NULL) = the b that supplied it, the lowest b on a tie, -1 for
 *   background.  A gather over the instances in ascending b: no atomics and no workspace, bitwise
 *   reproducible, independent of the order the instances are listed in (up to the names b).
 *   1 <= B, n_img <= 65535, H, W >= 1, H * W < 2^31 - 1024.
 *
 * zp_gt_info: per-instance masks, pixel counts and boxes.
 *   depth_gt f32 [B][Hg][Wg]: instance b rendered alone.  The window [oy, oy + H) x [ox, ox + W) of it
 *   is the image; the rest is the part of the object outside the frame (the toolkit renders at 3 H x
 *   3 W with the principal point moved by (W, H); Hg x Wg = H x W with a zero origin is allowed).
 *   depth_test f32 [n_test][H][W]: the scene's depth, measured or from zp_scene_depth, in the unit of
 *   the poses; test_index i32 [B] or NULL, as in zp_vsd (out-of-range entries are read as the nearest
 *   valid one; NULL: image b, then n_test >= B).  K f64 [B][4] = (fx, fy, cx, cy) of the IMAGE, not
 *   the shifted ones of the large render.
 *   Outputs (each may be NULL): mask u8 [B][H][W] (255 / 0) = depth_gt > 0 in the window; mask_visib
 *   u8 [B][H][W] (255 / 0); info i32 [B][11] = px_count_all, px_count_valid, px_count_visib, obj_x0,
 *   obj_y0, obj_x1, obj_y1, vis_x0, vis_y0, vis_x1, vis_y1.
 *   Distance image (misc.py:571-590) of the window of depth_gt and of depth_test at window pixel
 *   (x, y), exactly zp_vsd's: pX = (x - cx) / fx, pY = (y - cy) / fy, z = f64(d),
 *   dist = sqrt(((pX z)^2 + (pY z)^2) + z^2), every step one IEEE f64 operation.
 *   Visibility (visibility.py:29-36), diff = f32(dist_gt) - f32(dist_test):
 *     ZP_VISIB_BOP19: (diff <= f32(delta) || dist_test == 0) && dist_gt > 0
 *     ZP_VISIB_BOP18:  diff <= f32(delta) && dist_test > 0 && dist_gt > 0
 *   px_count_all   = #(depth_gt > 0) over the WHOLE Hg x Wg render (the truncated part counts, which
 *                    is why visib_fract falls for an object that leaves the frame);
 *   px_count_valid = #(dist_gt > 0 && dist_test > 0) over the window;
 *   px_count_visib = #(visible) over the window.
 *   obj_* = inclusive min / max corners of depth_gt > 0 over the whole render in image coordinates
 *   (render coordinate minus (ox, oy): they can be negative or exceed the frame); vis_* = the same of
 *   the visible mask.  A box with no pixels is (-1, -1, -1, -1).
 *   Every counter and corner is an integer merged with integer add / min / max (registers -> wave ->
 *   LDS -> one atomic per workgroup and counter), so the output is exact and independent of the order
 *   of the pixels.
 * 1 <= B <= 65535, Hg * Wg < 2^31 - 1024, 0 <= ox, ox + W <= Wg, 0 <= oy, oy + H <= Hg, n_test >= 1;
 * anything else, an unknown visib_mode, or a NULL depth_gt / depth_test / K is ZP_ERR_ARG before any
 * device call. */
#define ZP_VISIB_BOP19 0
#define ZP_VISIB_BOP18 1
int zp_scene_depth(int B, const float* depth, const int* img_index, int n_img, int H, int W, float* scene,
                   int* instance, void* stream);
int zp_gt_info(int B, const float* depth_gt, int Hg, int Wg, int ox, int oy, int H, int W, const float* depth_test,
               int n_test, const int* test_index, const double* K, double delta, int visib_mode, uint8_t* mask,
               uint8_t* mask_visib, int* info, void* stream);

/* ---- device crop pipeline --------------------------------------------
 * Replaces the DataLoader worker's crop_square_resize (bop_dataset_pytorch.py:36-72) of the image
 * (cv2.INTER_LINEAR -> S px) + transform_pre (:333-347: ToTensor + ImageNet Normalize on the BGR
 * array), and of the GT code image / visible mask / entire mask (cv2.INTER_NEAREST -> S px)
 * + RGB_image_to_class_id_image / class_id_image_to_class_code_images
 * (class_id_encoder_decoder.py:6-15, 43-63).  Images stay on the device as one stack
 * u8 [n_img][H][W][3] (masks [n_img][H][W]); crop b reads image img_index[b] with the padded box
 * bbox[b] = (x, y, w, h) int32 (padding_Bbox output).  A box with w <= 0 and h <= 0 gives the
 * reference's all-zero dummy crop.
 *   zp_crop_image: out f32 [B][3][S][S] (normalised, BGR channel order as the reference feeds it)
 *   zp_crop_gt:    code u8 [B][L][S][S] (0/1, channel 0 = MSB), mask_out / entire_out f32
 *                  [B][S][S] = v / 255; any of the three outputs may be NULL */
int zp_crop_image(const uint8_t* imgs, int n_img, int H, int W, const int* img_index, const int* bbox, int B, int S,
                  float* out, void* stream);
int zp_crop_gt(const uint8_t* gts, const uint8_t* masks, const uint8_t* entire_masks, int n_img, int H, int W,
               const int* img_index, const int* bbox, int B, int S, int L, uint8_t* code, float* mask_out,
               float* entire_out, void* stream);
/* The same with the reference's resize_method as an argument (zp_crop_image / zp_crop_gt / zp_augment are
 * the ZP_CROP_SQUARE case, bit for bit):
 *   ZP_CROP_SQUARE  "crop_square_resize" (bop_dataset_pytorch.py:36-72; the config_BOP files): as above.
 *   ZP_CROP_RECT    "crop_resize" (:74-88; the paper and ablation configs): the ROI is the box clipped to
 *                   the image, x1 = max(0, x), x2 = min(W, x + w), y1 = max(0, y), y2 = min(H, y + h), an
 *                   sw x sh = (x2 - x1) x (y2 - y1) slice with no squaring and no zero fill, resized to
 *                   S x S with one scale per axis (1 / (S / sw), 1 / (S / sh)): INTER_LINEAR's taps with
 *                   n = sw for x and n = sh for y; the 2 x 2 box filter only when both scales are exactly
 *                   2, a copy only when sw == sh == S; INTER_NEAREST per axis.  get_final_Bbox(..,
 *                   "crop_resize") (:183-192) returns that clipped box.
 * Deviation from the reference: an empty ROI under ZP_CROP_RECT (sw <= 0 or sh <= 0: w <= 0, h <= 0 or a box
 * wholly outside the image), on which cv2.resize raises (and for x + w < 0 the reference's slice wraps
 * around), gives the all-zero dummy crop (x = 0.0, code = 0, masks = 0), and zp_augment_m writes nothing.
 * Parity of the resize with OpenCV itself is unpinned for both methods (tests/crop_rect_ref.py,
 * oracle/crop_ref.py restate it).  Any other method is ZP_ERR_ARG before any device call. */
#define ZP_CROP_SQUARE 0
#define ZP_CROP_RECT 1
int zp_crop_image_m(const uint8_t* imgs, int n_img, int H, int W, const int* img_index, const int* bbox, int B, int S,
                    float* out, int method, void* stream);
int zp_crop_gt_m(const uint8_t* gts, const uint8_t* masks, const uint8_t* entire_masks, int n_img, int H, int W,
                 const int* img_index, const int* bbox, int B, int S, int L, uint8_t* code, float* mask_out,
                 float* entire_out, int method, void* stream);
/* GT digit planes of a d-ary code, d = 2^s: bits u8 [B][nbits][H][W] (zp_crop_gt's planes, channel 0 =
 * MSB) -> digits u8 [B][nbits/s][H][W], digit_i = planes [s*i, s*i+s) read MSB first -- with nbits = 16
 * the reference's class_id_image_to_class_code_images(id, d, 16/s, 65536)
 * (class_id_encoder_decoder.py:43-63): digit_i = (id >> s*(L-1-i)) & (d-1).  nbits % s == 0, s <= 8 */
int zp_pack_digits(const uint8_t* bits, int B, int nbits, int H, int W, int s, uint8_t* digits, void* stream);

/* ---- training-branch colour augmentation on the device -------------------------------------
 * Replaces apply_augmentation (bop_dataset_pytorch.py:349-355): the imgaug chain of
 * GDR_Net_Augmentation.build_augmentations (GDR_Net_Augmentation.py:161-178), Sequential in fixed
 * order, run over the image before the is_train crop (bop_dataset_pytorch.py:267-277).  The host
 * samples every random choice (zebrapose_amd/augment.py); the device does exact integer pixel work,
 * u8 -> u8 per stage, one flag bit per stage:
 *   ZP_AUG_SP       SaltAndPepper: h1 = fmix(sp_seed ^ ((y W + x) 0x9E3779B9)) (uint32, fmix = murmur3's
 *                   finaliser); when h1 < sp_thresh all three channels become
 *                   beta_tab[fmix(h1 ^ 0x68bc21eb) >> 24]
 *   ZP_AUG_STENCIL_A  MotionBlur: out = min(255, (sum kA[i][j] in[y+i-2][x+j-2] + 32768) >> 16), kA >= 0 with
 *                   sum 65536, BORDER_REFLECT_101 on the full image
 *   ZP_AUG_DROPOUT  CoarseDropout: keep-mask masks[b][mh][mw] nearest-upsampled (my = min(floor(y (1 /
 *                   (H / mh))), mh - 1)); a dropped pixel becomes 0 in all channels
 *   ZP_AUG_STENCIL_B  GaussianBlur: the same stencil with kB, its reflected border reading the dropout
 *                   stage's output at the in-image position
 *   ZP_AUG_LUT      Add / Invert / Multiply x 2 / LinearContrast composed: c = luts[b][c][v]
 * imgs u8 [n_img][H][W][3]; crop b reads image img_index[b]; out u8 [B][H][W][3].  flags == 0 copies.
 * bbox NULL: every pixel of out is written.  bbox int32 [B][4] (the box handed to zp_crop_image):
 * only the 32 x 32 tiles meeting the region crop_square_resize copies, [max(x1, 0), xe) x [max(y1, 0), ye),
 * are written (a zero box writes nothing); the rest of out keeps its contents.
 * H, W >= 8; 1 <= mh <= H, 1 <= mw <= W; all of masks, luts, beta_tab are required. */
#define ZP_AUG_SP 1
#define ZP_AUG_STENCIL_A 2
#define ZP_AUG_DROPOUT 4
#define ZP_AUG_STENCIL_B 8
#define ZP_AUG_LUT 16
typedef struct {
  uint32_t flags;
  uint32_t sp_seed, sp_thresh;
  int32_t kA[25], kB[25]; /* [5][5], Q16 */
} zp_aug_desc;
int zp_augment(const uint8_t* imgs, int n_img, int H, int W, const int* img_index, const zp_aug_desc* desc,
               const uint8_t* masks, int mh, int mw, const uint8_t* luts, const uint8_t* beta_tab, const int* bbox,
               int B, uint8_t* out, void* stream);
/* zp_augment with the crop method the box is read with (ZP_CROP_SQUARE / ZP_CROP_RECT above).  Under
 * ZP_CROP_RECT the written tiles are those meeting the clipped box [x1, x2) x [y1, y2); an empty one
 * writes nothing. */
int zp_augment_m(const uint8_t* imgs, int n_img, int H, int W, const int* img_index, const zp_aug_desc* desc,
                 const uint8_t* masks, int mh, int mw, const uint8_t* luts, const uint8_t* beta_tab, const int* bbox,
                 int B, uint8_t* out, int method, void* stream);

/* ---- GT renderer ------------------------------------------------------------------------
 * B renders of one mesh (GT code images, depth, masks), replacing the reference's OpenGL program
 * Render_GT_Color_Mesh_to_GT_Img: rendering_GT_once / render_3D_GT_Model
 * (render_related_source/opengl_render.cpp:164-206: black clear, GL_LESS, no culling, no
 * antialiasing), the projection of camera.hpp:29-59 (u = fx X / Z + cx, pixel centres at
 * half-integers) and the pass-through shaders shader_groundtruth.vs / .fs.
 *   verts f32 [nv][3], faces i32 [nf][3], face_bgr u8 [nf][3]: one colour per face in the byte order
 *   zp_crop_gt reads (id = B << 16 | G << 8 | R); needed only when color is asked for.
 *   Per render b: R f64 [B][9] row-major, t f64 [B][3], K f64 [B][4] = (fx, fy, cx, cy), as zp_pnp_ransac.
 *   Outputs (each may be NULL): color u8 [B][H][W][3], depth f32 [B][H][W] (camera Z), mask u8
 *   [B][H][W] (255 / 0), face_out i32 [B][H][W] (-1 = background); background is 0 in color, depth, mask.
 * Semantics (tests/render_ref.py restates them in numpy; the outputs match it bit for bit):
 *   vertex:   Xc = ((r0 x + r1 y) + r2 z) + tx in f64 (likewise Yc, Zc); u = (fx Xc) / Zc + cx,
 *             v = (fy Yc) / Zc + cy; snapped to 1/256 px, xi = rint(256 u) (half to even), saturated
 *             to +-2^28 so the edge functions fit int64.
 *   triangle: discarded whole when any vertex has Zc < z_near or a NaN projection, when its snapped
 *             area is 0, or when an index is outside [0, nv).  No back-face culling.
 *   coverage: pixel (x, y) is sampled at (x + 1/2, y + 1/2); exact int64 edge functions; a sample
 *             exactly on an edge belongs to the triangle for which that edge is a top or a left edge
 *             in image coordinates, so triangles sharing an edge cover its samples exactly once.
 *   depth:    q = (E12 (1/Z0) + E20 (1/Z1)) + E01 (1/Z2), invz = f32(q / A) (perspective-correct);
 *             depth = f32(1 / f64(invz)).
 *   visible:  the largest invz, ties to the lowest face index (GL_LESS under draw order), as one
 *             64-bit key per pixel merged with an unsigned atomic max: independent of the order
 *             triangles arrive in, bitwise reproducible.
 *   colour:   the winning face's face_bgr (flat).
 * Deviations from GL: no near / far clipping (the whole-triangle discard above; GT poses lie in
 * front of the camera); flat per-face instead of interpolated per-vertex colour (equal on the GT
 * meshes, whose faces are uniform); GL's choice for samples exactly on an edge is not pinned.
 * H, W <= 32768; B * nv, B * nf, B * H * W < 2^31 - 1024.  ws: zp_render_ws_bytes bytes (-1: bad sizes). */
long long zp_render_ws_bytes(int B, int nv, int nf, int H, int W);
int zp_render(int B, const float* verts, int nv, const int* faces, int nf, const uint8_t* face_bgr,
              const double* R, const double* t, const double* K, int H, int W, double z_near,
              uint8_t* color, float* depth, uint8_t* mask, int* face_out, void* ws, void* stream);

/* ---- shaded renderer ------------------------------------------------------------------------
 * zp_render plus a Phong-shaded colour image of a vertex-coloured mesh, replacing the reference's
 * OpenGL renderer lib/meshrenderer/meshrenderer_phong.py with shader/depth_shader_phong.vs / .frag
 * (synthetic frames of the train_render kind, the debug renders of test.py:316-327).
 *   zp_render's inputs, plus vert_normals f32 [nv][3], vert_rgb u8 [nv][3] (red, green, blue) and
 *   light f64 [B][6] = (lx, ly, lz, ambient, diffuse, specular) (device), the light's position in
 *   this project's camera coordinates (X right, Y down, Z forward); all three needed only for shaded.
 *   Outputs (each may be NULL): shaded u8 [B][H][W][3] in B, G, R order as zp_crop_image takes images,
 *   background 0; color, depth, mask, face_out as zp_render's, from the same visibility pass.
 * Visibility is zp_render's own device code (snapping, discards, exact int64 coverage, top-left rule,
 * 64-bit atomic-max key): the four common outputs equal zp_render's bit for bit.
 * Shading (tests/shade_ref.py restates it in numpy; shaded matches it bit for bit): all f64, every
 * step one IEEE operation in the order written, only + - * / and sqrt.  unit(v) = v / sqrt((x x +
 * y y) + z z), and a vector whose length is not > 0 stays zero.
 *   vertex:   P = (Xc, Yc, Zc) as zp_render's; n_e = unit(((r0 nx + r1 ny) + r2 nz) per row of R);
 *             L_v = unit(light - P); V_v = -P.
 *   pixel:    f = the face in the pixel's key; E12, E20, E01 its exact int64 edge values at the
 *             sample; b_i = f64(E_i) (1/Z_i); q = (b0 + b1) + b2 (the q of the depth rule); every
 *             attribute a (colour / 255, n_e, L_v, V_v) interpolates as ((b0 a0 + b1 a1) + b2 a2) / q.
 *   Phong:    N, Ld, Vd = unit of the interpolated n_e, L_v, V_v; nl = (N0 Ld0 + N1 Ld1) + N2 Ld2;
 *             d = nl > 0 ? nl : 0; Rv = (2 nl) N - Ld; s = max(Rv . Vd, 0) likewise (no shininess
 *             exponent: the reference has none); per channel o = (ka c + kd (d c)) + ks (s c), clamped
 *             to <= 1; byte = rint(255 o), half to even (a negative or NaN o gives 0).
 *   No culling: a back face gets d = 0 and shows its ambient term, as under GL (and whatever specular
 *   the formula above gives it: as in the reference's shader, s is not gated by d).
 * Deviations from the reference: its vertex shader normalises the 4-vector transpose(inverse(view)) *
 * vec4(normal, 1) and takes xyz, which scales the interpolated normal by a per-vertex factor; here
 * R n is normalised in 3-space.  The light is given in this project's camera frame: gl_utils/camera.py
 * realCamera builds view = diag(1, 1, -1) [R | t], so GL's eye frame is (Xc, Yc, -Zc) and the
 * reference's default light (400, 400, 400) is (400, 400, -400) here (zebrapose_amd.render's default).
 * f64 instead of GL's f32, and zp_render's deviations (no near / far clipping, 1/256 px snapping);
 * parity with a GL implementation is unpinned, as for zp_render.
 * Sizes as zp_render.  ws: zp_render_shaded_ws_bytes bytes (-1: bad sizes). */
long long zp_render_shaded_ws_bytes(int B, int nv, int nf, int H, int W);
int zp_render_shaded(int B, const float* verts, const float* vert_normals, const uint8_t* vert_rgb, int nv,
                     const int* faces, int nf, const uint8_t* face_bgr, const double* R, const double* t,
                     const double* K, const double* light, int H, int W, double z_near, uint8_t* shaded,
                     uint8_t* color, float* depth, uint8_t* mask, int* face_out, void* ws, void* stream);

/* ---- compositor -----------------------------------------------------------------------------
 * A rendered object over a background, replacing GDR_Net_Augmentation.py:78-153 (get_bg_image,
 * replace_bg with resize_short_edge :37-74) with no host round trip.
 * zp_mask_bbox: mask u8 [B][H][W] -> bbox i32 [B][4] = (r1, c1, r2, c2), the inclusive row / column
 * bounds of the nonzero pixels; an empty mask gives (0, 0, -1, -1).
 * zp_composite: fg u8 [B][H][W][3], mask u8 [B][H][W], bbox as above; bgs u8 [n_bg][Hb][Wb][3];
 * per sample (device arrays) bg_index i32 [B], bg_geo i32 [B][4] = (crop_w, crop_h, out_w, out_h),
 * bg_f f64 [B] = the factor f that resize_short_edge passes as fx = fy (zebrapose_amd.synth.bg_geometry
 * computes geo and f), trunc f64 [B][2] = (rnd, u).  Outputs (each may be NULL): out u8 [B][H][W][3],
 * mask_out u8 [B][H][W] (255 / 0).  tests/synth_ref.py restates both in numpy; the outputs match it
 * bit for bit.
 *   truncation (replace_bg:128-149, rows r, columns c; uniform(a, b) = a + (b - a) u in f64, int()
 *   truncates; mid_r = 0.5 (r1 + r2), mid_c = 0.5 (c1 + c2)):
 *     rnd < 0 off; rnd < 0.2 clears rows below int(uniform(r1, mid_r)); rnd < 0.4 rows from
 *     int(uniform(mid_r, r2)) on; rnd < 0.6 columns below int(uniform(c1, mid_c)); rnd < 0.8 columns
 *     from int(uniform(mid_c, c2)) on; otherwise (a NaN included) nothing.
 *   pixel: fg where the truncated mask is set, else the background pixel: the top-left crop_w x crop_h
 *     of bgs[bg_index] resized to out_w x out_h and pasted at the top-left of a zero image.
 *   resize: cv2.resize(crop, None, fx=f, fy=f, INTER_LINEAR) for u8 as OpenCV 4.x's generic path
 *     (the arithmetic of oracle/crop_ref.py): the sampling scale is 1 / f (not crop / out); source
 *     position f32((i + 1/2) scale - 1/2), floor and fraction in f32, clamped to the first / last
 *     sample; weights rint(w 2048); horizontal pass exact; vertical pass ((h0 >> 4) b0 >> 16) +
 *     ((h1 >> 4) b1 >> 16), then (v + 2) >> 2.  out == crop sizes: a copy.  |scale - 2| < DBL_EPSILON:
 *     OpenCV's INTER_AREA fast path, (a + b + c + d + 2) >> 2; a 2 x 2 block cut by the crop's last
 *     row or column averages the 1 or 2 samples inside, half to even.
 * Deviations from the reference: an empty mask clears nothing (np.min of nothing raises there); rows
 * or columns of the resized background beyond H or W are dropped (the reference's paste raises);
 * a bg_index, crop or factor that does not fit the stack (crop_w > Wb, f <= 0, ...) shows a zero
 * background; u is expected in [0, 1] (cuts are kept inside [0, 65536]).  Parity with OpenCV itself
 * is unpinned, as for zp_crop_image.
 * H, W, Hb, Wb <= 32768; B * H * W < 2^31 - 1024. */
int zp_mask_bbox(const uint8_t* mask, int B, int H, int W, int* bbox, void* stream);
int zp_composite(const uint8_t* fg, const uint8_t* mask, const int* bbox, int B, int H, int W, const uint8_t* bgs,
                 int n_bg, int Hb, int Wb, const int* bg_index, const int* bg_geo, const double* bg_f,
                 const double* trunc, uint8_t* out, uint8_t* mask_out, void* stream);

/* ---- scene compositor -----------------------------------------------------------------------
 * Whole synthetic scenes from per-instance renders: the colour image, foreground, depth and instance
 * map of each of n_img images, and every instance's exact visible mask, pixel counts and visible box,
 * in one pass that reads each depth once.  The reference has no such program (its cluttered training
 * frames are BlenderProc renders made outside it); tests/scene_ref.py restates the text below in
 * numpy and every output matches it bit for bit.
 *   depth f32 [B][H][W]: instance b rendered alone, as zp_render / zp_render_shaded write it; shaded u8
 *   [B][H][W][3] (B, G, R), needed only for image; img_index i32 [B] (device): the image of instance b,
 *   in any order.  An instance whose img_index lies outside [0, n_img) belongs to no image, exactly
 *   as zp_scene_depth ignores it: it is never used as an index, takes part in no image, its mask_visib
 *   is all 0 and its info is (px_all, 0, 0, 0, -1, -1).  It is not an error.
 *   winner:  of pixel (i, y, x), among the instances b with img_index[b] == i, by zp_scene_depth's rule:
 *            a surface is depth > 0 (so 0, a negative value and NaN are none, +inf and a subnormal are
 *            one), the smallest depth wins, the lowest b on a tie.
 *   Outputs (each may be NULL): image u8 [n_img][H][W][3] = the winner's shaded pixel, 0 without one
 *   (needs shaded); fg u8 [n_img][H][W] = 255 with a winner, else 0; scene f32 [n_img][H][W] and
 *   instance i32 [n_img][H][W] = zp_scene_depth's outputs bit for bit (the winner's depth or 0, the
 *   winner or -1); mask_visib u8 [B][H][W] = 255 exactly where instance[img_index[b]] == b -- exact
 *   occupancy, NOT zp_gt_info's delta-tolerance test: it marks precisely the pixels of image that
 *   show b's colour; info i32 [B][6] = px_all (#depth[b] > 0, the in-frame count), px_visib (#pixels
 *   won), r1, c1, r2, c2 = the inclusive row / column bounds of mask_visib[b], (0, 0, -1, -1) when
 *   it is empty, as zp_mask_bbox.
 *   Every byte of every output asked for is written.  Counters and corners are integers merged with
 *   integer add / min / max (registers -> wave shuffles -> one atomic per wave), so the output is
 *   exact, independent of the order of the pixels and bitwise reproducible.  The instances of an
 *   image are found as zp_scene_depth finds them, by a scan of img_index over all B per workgroup.
 * 1 <= B, n_img <= 65535 (zp_scene_depth's bound); sizes otherwise as zp_render: H, W <= 32768,
 * B * H * W and n_img * H * W < 2^31 - 1024.  ws: zp_scene_compose_ws_bytes bytes (-1: bad sizes),
 * needed only with info.  Bad sizes, a NULL depth or img_index, image without shaded or info without
 * ws are ZP_ERR_ARG before any device call. */
long long zp_scene_compose_ws_bytes(int B, int n_img, int H, int W);
int zp_scene_compose(int B, int n_img, int H, int W, const float* depth, const uint8_t* shaded, const int* img_index,
                     uint8_t* image, uint8_t* fg, float* scene, int* instance, uint8_t* mask_visib, int* info,
                     void* ws, void* stream);

/* ---- mesh coder --------------------------------------------------------------------------
 * Surface codes of a raw triangle mesh: per-vertex class id, per-face class id and the class ->
 * 3D-point LUT, replacing the reference's offline tool Generate_Mesh_with_GT_Color (PCL + OpenCV):
 * `bits` levels of a balanced 2-means split of the vertices (Generate_Mesh_with_GT_Color.cpp:61-218),
 * ids with the first split as the MSB (:322-353), the face rule (:356-393) and the LUT (:396-455).
 * Binary splits here (the reference's balancing and bit assembly are 2-way); divide_number > 2 is
 * zp_mesh_code_radix below.  OpenCV's k-means++ draws cannot be reproduced, so the semantics are restated in
 * exact integer arithmetic (tests/meshcode_ref.py restates them in numpy; the outputs match it bit
 * for bit and do not depend on the order of any summation):
 *   grid:     q = rint(f64(v) * 2^grid_log2) per coordinate, saturated to +-(2^19 - 1).  The host
 *             passes the largest grid_log2 for which no coordinate saturates.  From here on all
 *             clustering arithmetic is int64: |delta| <= 2^20, d^2 < 2^42, sums over <= 2^21 vertices.
 *   level l:  (l = 0 .. bits - 1) 2^l groups, the root group being all vertices; a group's vertices
 *             are taken in ascending vertex index wherever an order matters; n >= 2^(bits - l) each.
 *   2-means:  per group, `attempts` tries.  Seeds from one uint32 draw r per (attempt, group),
 *             draws[attempt][(2^l - 1) + g]: c0 = the vertex at rank (r * n) >> 32, c1 = the group's
 *             vertex with the largest d^2 to c0 (ties: lowest index).  Up to `iterations` Lloyd steps:
 *             label = nearer centre (ties: class 0); each non-empty class's centre becomes
 *             floor((2 S + n_j) / (2 n_j)) per axis, an empty class keeps its centre; the group
 *             stops after the step in which the larger of the two centre shifts^2 is <= eps2_q
 *             (= floor((eps * 2^grid_log2)^2)).  Compactness = sum of d^2 to the own centre under one
 *             more labelling; the attempt with the lowest compactness wins (ties: lowest attempt).
 *   balance:  with the winning centres' labels and m = floor(n / 2): a class with more than m
 *             vertices keeps the m with the largest d^2 to the OTHER centre (ties: lower index), the
 *             rest change class.  Children of group g: 2g (bit 0) and 2g + 1 (bit 1).
 *   ids:      vertex id = sum_l bit_l * 2^(bits - 1 - l); face id, from its vertices' ids i0, i1, i2:
 *             i0 if i0 == i1 or i0 == i2, else i1 if i1 == i2, else i0.
 *   LUT:      per class the f64 mean of the f32 positions of the three vertices of each of its
 *             faces (with multiplicity), summed in ascending face index, vertex 0, 1, 2 as single
 *             IEEE additions; a class without a face is NaN (bits 0x7FF8000000000000).
 * verts f32 [nv][3] (finite), faces i32 [nf][3] (indices in [0, nv); an index outside is read as the
 * nearest valid one), draws u32 [attempts][2^bits - 1] (device memory, like every pointer here);
 * outputs vertex_ids i32 [nv], face_ids i32 [nf], lut f64 [2^bits][3].
 * 1 <= bits <= 16, 2^bits <= nv <= 2^21, 1 <= nf <= 2^24, 1 <= attempts <= 64, 1 <= iterations <= 1000,
 * |grid_log2| <= 40, eps2_q >= 0; anything else, or a NULL pointer, is ZP_ERR_ARG before any device
 * call.  ws: zp_mesh_code_ws_bytes bytes (-1: bad sizes). */
long long zp_mesh_code_ws_bytes(int nv, int nf, int bits);
int zp_mesh_code(const float* verts, int nv, const int* faces, int nf, int bits, int attempts, int iterations,
                 int grid_log2, long long eps2_q, const uint32_t* draws, int* vertex_ids, int* face_ids, double* lut,
                 void* ws, void* stream);

/* d-ary surface codes of a raw mesh: `levels` levels of a balanced d-way split, d = divide a power of
 * two in [4, 256] (the reference's code-radix ablation, divide_number_each_itration = 4 / 16 / 256).
 * The reference's Divide_PointCloud_Opencv_Samesize (:61-218) calls cv::kmeans with d centres, but its
 * "same size" step only ever moves points between classes 0 and 1 towards n / 2 (:148-214): for d > 2
 * it is an unbalanced k-means, and cv::kmeans throws once a group holds fewer than d points.  The
 * split is therefore restated with a real d-way balance, in exact int64 arithmetic
 * (tests/meshcode_radix_ref.py restates it in numpy; the outputs match it bit for bit and depend on
 * the order of no summation and of no atomic).  Grid, group order, faces and LUT are zp_mesh_code's:
 *   level l:  (l = 0 .. levels - 1) d^l groups, the root group being all vertices, each taken in
 *             ascending vertex index wherever an order matters; n >= d^(levels - l) vertices each.
 *   seeds:    one uint32 draw r per (attempt, group), draws[attempt][(d^l - 1) / (d - 1) + g]: c_0 = the
 *             group's vertex at rank (r * n) >> 32; for j = 1 .. d - 1, c_j = the group's vertex with
 *             the largest (minimum d^2 to c_0 .. c_(j-1)), ties to the lowest vertex index
 *             (farthest-point seeding; coincident seeds are possible among identical points).
 *   Lloyd:    up to `iterations` steps: label = nearest centre (ties: lowest class); a non-empty
 *             class's centre becomes floor((2 S + n_j) / (2 n_j)) per axis, an empty class keeps its
 *             centre; the group stops after the step in which the largest of its d centre shifts^2
 *             is <= eps2_q.  Compactness = sum of d^2 to the own centre under one more labelling;
 *             the attempt with the lowest compactness wins (ties: lowest attempt).
 *   balance:  (the peel) with the winning centres, D[p][j] = d^2 of vertex p to centre j and U_0 = the
 *             group: for j = 0 .. d - 2, class j takes the k_j = floor(|U_j| / (d - j)) vertices of U_j
 *             with the lowest D[p][j] - min_{i > j} D[p][i] (ties: lower vertex index), U_(j+1) is the
 *             rest; class d - 1 takes U_(d-1).  Every class ends with floor(n / d) or ceil(n / d)
 *             vertices, so no child group starves.  Children of group g: d * g + digit.
 *   ids:      vertex id = sum_l digit_l * d^(levels - 1 - l) (the fold of zp_decode_radix and of
 *             zp_pack_digits' planes); face ids and the LUT over d^levels classes as in zp_mesh_code.
 * verts, faces as zp_mesh_code; draws u32 [attempts][(d^levels - 1) / (d - 1)]; outputs vertex_ids
 * i32 [nv], face_ids i32 [nf], lut f64 [d^levels][3].  divide a power of two in [4, 256] (divide == 2
 * is ZP_ERR_ARG: that is zp_mesh_code), levels >= 1, d^levels <= 65536, d^levels <= nv <= 2^21, nf,
 * attempts, iterations, grid_log2 and eps2_q as zp_mesh_code; anything else, or a NULL pointer, is
 * ZP_ERR_ARG before any device call.  ws: zp_mesh_code_radix_ws_bytes bytes (-1: bad sizes); the
 * distances of the peel are recomputed per class, so the workspace is O(nv + nf + d^levels). */
long long zp_mesh_code_radix_ws_bytes(int nv, int nf, int divide, int levels);
int zp_mesh_code_radix(const float* verts, int nv, const int* faces, int nf, int divide, int levels, int attempts,
                       int iterations, int grid_log2, long long eps2_q, const uint32_t* draws, int* vertex_ids,
                       int* face_ids, double* lut, void* ws, void* stream);

/* Mesh upsampling: one pass of midpoint subdivision with an edge-length threshold.  Step 1 of the
 * reference's label-generation recipe (Binary_Code_GT_Generator/Generate_GT.md:90-92) upsamples a model
 * "until it has more than 2^16 vertices" by hand, with Meshlab's 'subdivision surface: mid point'
 * filter; zp_mesh_code needs that many vertices too.  The filter is restated with exact semantics
 * (tests/subdiv_ref.py restates them in numpy; the outputs match it bit for bit and depend on the
 * order of no summation and of no atomic).  One call is one pass:
 *   edges:    face (v0, v1, v2) has edge slots 0: (v0, v1), 1: (v1, v2), 2: (v2, v0).  An edge is the
 *             unordered pair of indices, its key (min << 32) | max; unique edges are taken in ascending
 *             key order.  An index outside [0, nv) is read as the nearest valid one.
 *   length:   d = f64(a) - f64(b) per axis (exact), len2 = (dx * dx + dy * dy) + dz * dz, every
 *             operation rounded once (no FMA).  max_len2 = the maximum over the unique edges; len2 >= 0,
 *             so any reduction order gives the same bits.
 *   split:    an edge qualifies iff len2 > abs2 and len2 > rel2 * max_len2 (one IEEE multiply).  If more
 *             than max_split qualify, only the max_split with the largest len2 split (ties: lower key).
 *             An edge of length 0 never splits; that covers a face with a repeated index.
 *   vertices: old vertices keep their indices; the split edges, in ascending key order, get nv, nv + 1,
 *             ...; position per axis f32((f64(a) + f64(b)) * 0.5): sum and halving are exact, one
 *             round-to-nearest-even to f32.  parents[i] = (i, i) for i < nv, (min, max) for a new vertex.
 *   faces:    the children of face i are consecutive, from the exclusive prefix sum of 1 + (number of
 *             its split edges), orientation kept; mij is the midpoint of edge (vi, vj):
 *               0 split: (v0, v1, v2)
 *               3 split: (v0, m01, m20), (m01, v1, m12), (m20, m12, v2), (m01, m12, m20)
 *               1 split: the face rotated so that the split edge is (v0, v1): (v0, m01, v2), (m01, v1, v2)
 *               2 split: rotated so that the unsplit edge is (v2, v0): (m01, v1, m12), then the quad
 *                        (v0, m01, m12, v2) cut by its shorter diagonal: if len2(m01, v2) < len2(v0, m12)
 *                        strictly (both as above, from the f32 output positions), (v0, m01, v2),
 *                        (m01, m12, v2); otherwise (v0, m01, m12), (v0, m12, v2).
 *   counts:   {n_unique_edges, n_split, nv_out, nf_out}.  If nv_out > cap_v or nf_out > cap_f nothing is
 *             written to out_verts, out_faces and parents; counts and max_len2 are still filled, so the
 *             caller can size a retry.
 * verts f32 [nv][3] (finite), faces i32 [nf][3]; outputs out_verts f32 [cap_v][3], out_faces i32
 * [cap_f][3], parents i32 [cap_v][2], counts i64 [4], max_len2 f64 [1] (device memory, like every
 * pointer here; the outputs may not overlap the inputs).  1 <= nv <= 2^21, 1 <= nf <= 2^24, abs2 >= 0,
 * 0 <= rel2 < 1, max_split >= 0, cap_v >= 0, cap_f >= 0; anything else, or a NULL pointer, is ZP_ERR_ARG
 * before any device call.  ws: zp_mesh_subdivide_ws_bytes bytes (-1: bad sizes). */
long long zp_mesh_subdivide_ws_bytes(int nv, int nf);
int zp_mesh_subdivide(const float* verts, int nv, const int* faces, int nf, double abs2, double rel2, int max_split,
                      float* out_verts, int cap_v, int* out_faces, int cap_f, int* parents, long long* counts,
                      double* max_len2, void* ws, void* stream);

/* ---- edge refinement -----------------------------------------------------------------------
 * The refine = True branch of the reference's inference (test.py:276-313): the visible contour of the
 * object's mask (zp_mask_contour) and py_edge_refine's Gauss-Newton iteration against it
 * (zp_edge_refine_step, edge_refine/examples/edge_refine.cpp:68-173), batched over B crops / poses.
 * The reference needs OpenGL, Eigen and OpenCV for it; the semantics are restated here and, in numpy,
 * in tests/refine_ref.py.  R f64 [B][9] row-major, t f64 [B][3], K f64 [B][4] = (fx, fy, cx, cy), as
 * zp_render and zp_pnp_ransac; all arithmetic on reals is f64 (the reference: f32 Eigen).
 *
 * Outer border of a binary image (both functions): pad the image with one ring of unset pixels; the
 * OUTSIDE is the 4-connected component of unset pixels containing the ring; a set pixel is an
 * outer-border pixel iff one of its four neighbours is in the outside.  This is the pixel set of
 * cv2.findContours(RETR_EXTERNAL, CHAIN_APPROX_NONE) over all 8-connected components; borders of
 * holes, and components lying inside a hole, are not part of it.  Order: row-major (y, then x).
 * A pixel the tracer visits twice appears once.
 * The outside is found by row and column sweeps repeated until nothing changes, at most 4 (H + W)
 * times; an image that needs more (no rendered silhouette does) is reported, never waited for.
 * Images: 1 <= H, W <= 32768 and H * 32 ceil(W / 32) <= 2^19 (640 x 480 and 720 x 540 fit), 1 <= B <=
 * 65535; anything else, or a NULL pointer that is not optional, is ZP_ERR_ARG before any device call.
 *
 * zp_mask_contour (test.py:300-307): entire u8 [B][S][S] (non-zero = set), visible u8 [B][S][S] or
 * NULL, bbox i32 [B][4] = (x, y, w, h) -> counts i32 [B], xy i32 [B][cap][2].
 *   An outer-border pixel (x, y) of `entire` is kept iff x > 0, y > 0 and any of visible[y-1 .. y]
 *   [x-1 .. x] is non-zero (visible NULL: iff x > 0 and y > 0).  It is written as
 *   X = trunc(f64(w) / S * x + bx), Y = trunc(f64(h) / S * y + by)
 *   (mapping_pixel_position_to_original_position: f64 divide, multiply, add, truncation toward zero);
 *   duplicates after truncation are kept.  counts[b] is the true count, entries past cap are dropped;
 *   counts[b] = -1 when the sweep cap was hit.
 *
 * zp_edge_refine_step: one iteration for B poses, on the depth images f32 [B][H][W] (0 = background)
 * that zp_render produced at those poses with K' = (fx, fy, cx + 1/2, cy + 1/2): the reference's
 * renderer has its pixel centres at integers (renderer.cpp:115-118), zp_render samples at
 * half-integers.  The step itself takes the unshifted K.
 *   counts i32 [B], xy i32 [B][cap][2]: the observed contour, as zp_mask_contour writes it; pose b
 *   uses its first min(counts[b], cap) points, each coordinate saturated to +-2^20.  1 <= cap <= 2^20.
 *   silhouette: depth > 0; border list: its outer border.
 *   match:    per observed point (x, y) the border pixel (xc, yc) with the smallest integer squared
 *             distance, ties to the lowest row-major index.
 *   residual: e = (x - xc, y - yc);  cost[b] = sum |e|^2, an exact integer.
 *   geometry: d = f64(depth[yc][xc]); Xc = (d (xc - cx) / fx, d (yc - cy) / fy, d); Xb = R^T (Xc - t);
 *             Jc = [[-fx / d, 0, fx Xc.x / d^2], [0, -fy / d, fy Xc.y / d^2]]; Jt = Jc R;
 *             Jr = -Jt [Xb]x; J = [Jr | Jt] (2 x 6);  H = sum J^T J;  b = -sum J^T e.
 *             The sums run over a fixed partition and a fixed tree, without floating-point atomics:
 *             two runs give the same bits.
 *   solve:    (diag(lambda_rot x 3, lambda_trans x 3) + H) theta = b (Cholesky); both lambdas > 0.
 *   update:   E = exp([theta_r]x) by Rodrigues (the series below |theta_r| = 1e-8);
 *             R_out = R E; t_out = t + R_out theta_t (Eigen's rotate, then translate, :163-166).
 *   status i32 [B]: 0 stepped; 1 fewer than 20 border pixels, or no observed point (:96-100);
 *             2 the sweep cap was hit.  With 1 and 2 the pose is copied through bit for bit, cost is 0.
 *   units:    those of depth and t.  The reference works in metres with lambda_rot = 5000,
 *             lambda_trans = 500000; for millimetres pass lambda_trans * 0.001^2 = 0.5 and the same
 *             lambda_rot: the problem is then the same one.
 *   Optional outputs (NULL: not written): border_n i32 [B]; border_xy i32 [B][bcap][2] (the first bcap
 *   border pixels); match i32 [B][cap] (index into the border list, -1 past the points used); Hb f64
 *   [B][27]: the upper triangle of H by rows (21 values), then b.
 *   R_out / t_out must not be R / t.  ws: zp_edge_refine_ws_bytes bytes (-1: bad sizes); it holds the
 *   border pixels past the 4096 kept on chip.
 * Deviations from the reference: f64 for f32; the exact f32 depth for SRT3D's 16-bit depth buffer, and
 * no 0.001 - 50 m clip; contours as sets (row-major, no repeats) for traces; the tie rule (the reference
 * takes the first in trace order); the border of all components, where the reference drops contours
 * shorter than 20 and matches against contours[0] alone; e from the pixel itself, where the
 * reference re-projects the back-projected point (the same up to rounding). */
int zp_mask_contour(int B, int S, const uint8_t* entire, const uint8_t* visible, const int* bbox, int cap,
                    int* counts, int* xy, void* stream);
long long zp_edge_refine_ws_bytes(int B, int H, int W);
int zp_edge_refine_step(int B, int H, int W, const float* depth, const int* counts, const int* xy, int cap,
                        const double* R, const double* t, const double* K, double lambda_rot, double lambda_trans,
                        double* R_out, double* t_out, long long* cost, int* status, int* border_n, int* border_xy,
                        int bcap, int* match, double* Hb, void* ws, void* stream);

/* ---- ICP refinement -------------------------------------------------------------------------
 * The reference's depth-based refiner (zebrapose/icp/icp_utils.py:7-176): render the model's depth at
 * the estimated pose, back-project it and the measured depth to point clouds (zp_depth_points, called
 * once for each), and run point-to-point ICP from the rendered cloud to the measured one (zp_icp),
 * batched over B poses.  The reference needs OpenGL and sklearn for it and takes one pose at a time;
 * the semantics are restated here and, in numpy, in tests/icp_ref.py.  All reals are f64; R f64 [B][9]
 * row-major, t f64 [B][3], K f64 [B][4] = (fx, fy, cx, cy).  Neither function synchronises the host or
 * uses atomics; two runs give the same bits.  Bad sizes or values, or a NULL pointer that is not
 * optional, are ZP_ERR_ARG before any device call.  The *_ws_bytes functions return -1 for sizes out
 * of range and otherwise the workspace the call needs, which is 0 for both today (ws may then be NULL):
 * everything lives in registers and LDS.
 *
 * zp_depth_points (rgbd_to_point_cloud, :7-13): depth f32 [B][H][W] -> counts i32 [B], pts f64 [B][cap][3].
 *   A pixel (u, v) counts iff its depth is finite and > 0 (the reference's nonzero() would also take
 *   negative values and NaN).  Its point is z = f64(depth), x = ((u - cx) * z) / fx,
 *   y = ((v - cy) * z) / fy, each step one f64 operation, u and v the integer pixel indices.
 *   filter (optional) f64 [B][4] = (centre x, y, z, radius), device memory, with the host scalar factor
 *   >= 0 (:147-148): with lim = factor * radius a point is kept iff (dx dx + dy dy) + dz dz < lim * lim,
 *   d = point - centre.  Kept points are written in row-major pixel order; counts[b] is the true count,
 *   entries past cap are dropped.
 *   stats (optional) f64 [B][4]: the centroid of ALL kept points (sum / count) and the largest distance
 *   sqrt((dx dx + dy dy) + dz dz) of one from it (:139-141); zeros when nothing is kept.  It has the
 *   filter's layout: the call for the measured depth reads the stats of the call for the rendered one.
 *   1 <= B <= 65535, 1 <= H, W <= 16384, H W <= 2^24, 1 <= cap <= 2^24, B cap <= 2^28; stats != filter.
 *
 * zp_icp (ICPRefiner.refine from :149 on, icp :83-126, best_fit_transform :35-80): source = the rendered
 * cloud (src_pts f64 [B][src_cap][3], src_counts i32 [B]), destination = the measured one, both as
 * zp_depth_points writes them; counts are clamped to [0, cap].  One workgroup per pose, one launch.
 *   status 1: n_src = 0.  status 2: n_dst < n_src * min_fraction (the reference: 1/20), or n_dst = 0.
 *   subsample: n = min(n_src, n_dst, N); entry i < n of each side is point floor(draw[i] * count) of its
 *             list, draws_src / draws_dst f64 [B][N] uniform in [0, 1) (sampling with replacement, as
 *             np.random.choice, from the caller's generator, not numpy's stream).  1 <= N <= 4096.  A draw
 *             outside [0, 1) still gives an index: count - 1 from draw * count >= count on, 0 for a
 *             negative product and for NaN.
 *   iterate:  at most max_iterations (>= 1) times: per source point the destination point with the
 *             smallest (dx dx + dy dy) + dz dz, ties to the lowest index; the best-fit transform from
 *             the source points to their neighbours; the source points moved by it; stop after the move
 *             when |prev_error - mean distance| < tolerance (distances Euclidean, prev_error starts at
 *             0 and follows the mean).
 *   fit:      centroids cA, cB; mode 1 (depth_only): R = I, t = cB - cA.  Otherwise H = sum (a - cA)
 *             (b - cB)^T = U S V^T, R = V U^T with the last singular pair's sign chosen so that det R = 1,
 *             t = cB - R cA, and in mode 2 (no_depth) t_z = 0.  The solver is a 3 x 3 Jacobi iteration on
 *             H^T H, its v2 and v3 polished against H itself where s2 <= 1e-3 s1 (the reference: LAPACK's
 *             SVD).  Where the rotation is not unique (H of rank 0 or 1) it is the identity, or one of the
 *             best rotations.
 *   result:   T = the fit from the original subsample to the final source points (:119); in mode 2 a T
 *             whose rotation angle atan2(|sin|, cos) exceeds angle_limit (the reference: 20 degrees in
 *             radians) is dropped, status 3.  R_out = T_R R, t_out = T_R t + T_t.
 *   With status 1, 2 and 3 the pose is copied through bit for bit; iterations is 0 and mean_error 0 for
 *   1 and 2.  iterations i32 [B]: iterations run (the reference's i + 1); mean_error f64 [B]: the mean
 *   distance of the last one.
 *   Optional outputs (NULL: not written): nn i32 [B][N], the neighbour of each source point in the last
 *   iteration run as an index into the destination subsample, -1 from n on; T f64 [B][16] row-major,
 *   the fitted transform (also with status 3; the identity with 1 and 2).
 *   R_out / t_out must not be R / t.  tolerance must not be NaN, max_iterations <= 100000. */
long long zp_depth_points_ws_bytes(int B, int H, int W, int cap);
int zp_depth_points(int B, int H, int W, const float* depth, const double* K, int cap, const double* filter,
                    double factor, int* counts, double* pts, double* stats, void* ws, void* stream);
long long zp_icp_ws_bytes(int B, int N);
int zp_icp(int B, int N, const double* src_pts, const int* src_counts, int src_cap, const double* dst_pts,
           const int* dst_counts, int dst_cap, const double* draws_src, const double* draws_dst, int max_iterations,
           double tolerance, int mode, double min_fraction, double angle_limit, const double* R, const double* t,
           double* R_out, double* t_out, int* status, int* iterations, double* mean_error, int* nn, double* T,
           void* ws, void* stream);

/* ---- model info -----------------------------------------------------------------------------
 * The diameter and the box of one entry of BOP's models_info.json, from the model's points.  The
 * reference reads them from the file that ships with a dataset (test.py:136, train_v6.py:118); its own
 * routine for the diameter is lib/pysixd/misc.py:952-966 (calc_pts_diameter), n numpy passes over all
 * n (n + 1) / 2 pairs.  The semantics are restated here and, in numpy, in tests/modelinfo_ref.py.  Each
 * f64 operation below is rounded on its own (no fused multiply-add), so the result is defined bit for
 * bit; nothing depends on how the pairs are split over the device, there are no atomics, and two runs
 * give the same bits.
 *
 * zp_model_info: pts f32 [n][3] (as zp_pose_error takes them) -> out f64 [8], pair i32 [2], status i32 [1].
 *   d2(i, j), i <= j: dx = f64(x_i) - f64(x_j), likewise dy, dz; d2 = (dx dx + dy dy) + dz dz: what
 *             (pts_diff * pts_diff).sum(axis=1) gives on the f64 copies BOP's load_ply makes of f32 files.
 *   out[7]    d2max = the largest d2(i, j) over all i <= j.  The pairs include i = j, as the reference's
 *             pts[pt_id:] does: one point, or n equal points, give 0.
 *   out[6]    diameter = sqrt(d2max) as the device's f64 square root gives it.  That it is the correctly
 *             rounded one is not established here: a caller that needs the bits of the host's
 *             sqrt(d2max) takes that root itself from out[7] (zebrapose_amd.modelinfo does).
 *   pair      the lexicographically lowest (i, j), i <= j, with d2(i, j) == d2max; may be NULL.
 *   out[0..2] min x, y, z: the f32 minimum widened to f64;  out[3..5] size x, y, z = f64(max) - f64(min).
 *             -0 orders below +0 in both.
 *   status    0, or 1 when any coordinate is not finite; the other outputs are then unspecified.
 *   n >= 1 and 3 n < 2^31 - 1024; anything else, or a NULL pts / out / status / ws, is ZP_ERR_ARG before
 *   any device call.  ws: zp_model_info_ws_bytes(n) bytes (-1: bad n), one 16-byte partial per
 *   workgroup of a fixed grid: it does not grow with n. */
long long zp_model_info_ws_bytes(int n);
int zp_model_info(const float* pts, int n, double* out, int* pair, int* status, void* ws, void* stream);

/* ---- optimizer ----------------------------------------------------------------------- */
/* torch.optim.Adam (no weight decay, amsgrad off) over one flat f32 buffer; step >= 1 */
int zp_adam(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long long n,
            double lr, double beta1, double beta2, double eps, long long step, void* stream);
/* the same update for `count` tensors in ceil(count / 40) launches (host arrays of device
 * pointers; every tensor at the same step), bitwise identical to zp_adam per tensor */
int zp_adam_multi(int count, float* const* params, const float* const* grads, float* const* exp_avg,
                  float* const* exp_avg_sq, const long long* numel, double lr, double beta1, double beta2,
                  double eps, long long step, void* stream);
/* the same with the step count read on the device (f32 scalar, already advanced to this step):
 * capturable in a hipGraph, whose replays then use the current count (GraphedTrainStep) */
int zp_adam_multi_dev(int count, float* const* params, const float* const* grads, float* const* exp_avg,
                      float* const* exp_avg_sq, const long long* numel, double lr, double beta1, double beta2,
                      double eps, const float* step_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ZP_H_ */
