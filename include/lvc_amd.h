/*
 * lvc_amd.h -- C ABI of liblvc_amd.so: the MI355X (gfx950) kernels of the lvc hot path.
 *
 * The reference (prannaykaul/lvc) has no C ABI for this path: it sits behind Python registries and
 * nn.Module call signatures, with exactly one native op of its own
 * (detectron2/layers/csrc/vision.cpp:96-97, roi_align_forward/backward) and torchvision's nms.  This header
 * is the drop-in boundary a maintainer binds instead (INTEGRATION.md shows the ctypes / torch.library
 * stubs).  Conventions:
 *   - extern "C", plain pointers and sizes; no torch types.  All data pointers are DEVICE pointers unless
 *     marked [host]; tensors are dense fp32 / int32 / int64 as stated.
 *   - every function enqueues work on `stream` (a hipStream_t passed as void*; NULL = default stream) and
 *     returns immediately; nothing here synchronises the device (the reference's ROIAlign does:
 *     ROIAlign_cuda.cu:364, a defect we do not reproduce).
 *   - return value: 0 = LVC_OK, 1 = LVC_ERR_INVALID (bad argument), 2 = LVC_ERR_HIP (launch failed);
 *     lvc_last_error() gives the message for the calling thread.  Data-dependent conditions that the
 *     reference asserts on the host (negative RoI size, ROIAlign_cpu.cpp:149-152) are reported
 *     asynchronously through a device status word (`d_status`, bit 0 = negative RoI size, bit 1 =
 *     detection candidate overflow) which the host reads together with the results.
 *   - ownership: the caller owns every buffer, including workspaces (sizes from the *_workspace_bytes
 *     queries); the library allocates nothing and keeps no state between calls.
 *   - threading: one host thread per stream; functions are re-entrant.
 */
#ifndef LVC_AMD_H
#define LVC_AMD_H

#ifdef __cplusplus
extern "C" {
#endif

#define LVC_OK 0
#define LVC_ERR_INVALID 1
#define LVC_ERR_HIP 2

int lvc_abi_version(void);
const char* lvc_last_error(void);
void lvc_set_error(const char* fmt, ...);

/* ---------------------------------------------------------------------------------------------------
 * Convolution / linear layers: NHWC fp32 implicit GEMM with the per-channel affine (FrozenBN and/or bias),
 * optional residual and ReLU fused into the epilogue.  This entry point is the exact-fp32 engine
 * (v_mfma_f32_32x32x2_f32); the default engines of the detector are the fp32-accurate operand-split forms
 * further down (lvc_conv*_f16x2: two-way fp16 split, 3 fp16 MFMAs per block; lvc_conv*_bf16x3: three-way
 * bf16 split, 6 bf16 MFMAs per block), which take the same tensors and the same epilogue arguments.
 * Replaces: detectron2/layers/wrappers.py:41-99 (Conv2d+norm+activation), batch_norm.py:45-65 (FrozenBN),
 *   backbone/resnet.py:195-211 (residual add + ReLU), backbone/fpn.py:131-133 (nearest x2 upsample + add),
 *   lvc/modeling/roi_heads/box_head.py:82-91 and fast_rcnn.py:583-598 (Linear = 1x1 conv on [M,1,1,K]).
 *   x        [N,H,W,C]        C = physical channels (mode 0: C % 32 == 0; mode 1: C == 4, the RGB0 stem)
 *   w_packed [Kpad,Kg]        rows = out channel, zero rows up to a multiple of 128;
 *                             mode 0: k = (c/32, r, s, c%32), Kg = R*S*C
 *                             mode 1: k = (r, 8 pixels x 4 ch), Kg = R*32 (7x7 stem: pixel 7 / ch 3 zero)
 *   scale, shift [K] or NULL  y = acc*scale + shift
 *   residual                  res_mode 0 none | 1: [M,ldr] same rows as y | 2: [N,Ho/2,Wo/2,ldr], upsampled x2
 *   y        [N*Ho*Wo, ldy]   ldy/ldr = row strides in floats (<=0: K)
 *   workspace                 lvc_conv_workspace_bytes() bytes, zero-initialised ONCE by the caller and then
 *                             reused by every launch on the same stream (split-tile partials + flags of the
 *                             stream-K decomposition); launches on different streams need different workspaces
 */
long long lvc_conv_workspace_bytes(void);
/* Byte offset, inside that workspace, of the range / error words described next (behind the partial tiles and the worker
 * flags; the layout is csrc/conv_common.h's).  Hosts read the words at this offset instead of restating the layout. */
long long lvc_conv_range_words_offset(void);
/* Per-layer range words.  The workspace ends in lvc_range_slots() int32 words behind the worker flags (byte offset
 * lvc_conv_range_words_offset()).  Word 0 is the shared error word (bit 0: a stream-K worker timed out; bit 1: an operand left a
 * two-way fp16 split kernel's range).  lvc_set_range_slot(s), 0 < s < lvc_range_slots(), makes the fp16-split conv/GEMM
 * launches that follow ON THE CALLING THREAD raise their bits in word s instead, so the host can re-route exactly the layer
 * that overflowed (lvc_amd.kernels.check_conv_error_word); 0 restores the shared word. */
void lvc_set_range_slot(int slot);
int lvc_range_slot(void);
int lvc_range_slots(void);
int lvc_conv2d_nhwc_f32(const float* x, const float* w_packed, const float* scale, const float* shift,
                        const float* residual, float* y, int N, int H, int W, int C, int K, int R, int S,
                        int stride, int pad, int Kg, int relu, int res_mode, int ldy, int ldr, int mode,
                        void* workspace, void* stream);

/* Same layer contract on the bf16 matrix cores with fp32-level accuracy (csrc/conv_bf16x3.hip): every fp32 operand is
 * split exactly into three bf16 values and the product assembled from six v_mfma_f32_32x32x16_bf16 (fp32 accumulate).
 * w_split: [3][Kpad][Kg] bf16 planes (hi, mid, lo) of the packed weights of lvc_conv2d_nhwc_f32 mode 0.
 * Requires C % 32 == 0, K % 4 == 0, ldy % 4 == 0, ldr % 4 == 0.  Same workspace as lvc_conv2d_nhwc_f32. */
int lvc_conv2d_nhwc_bf16x3(const float* x, const unsigned short* w_split, const float* scale, const float* shift,
                           const float* residual, float* y, int N, int H, int W, int C, int K, int R, int S,
                           int stride, int pad, int Kg, int relu, int res_mode, int ldy, int ldr, void* workspace,
                           void* stream);

/* 3x3 / stride 1 / pad 1 specialisation of lvc_conv2d_nhwc_bf16x3 (csrc/conv3x3_halo.hip): identical arguments minus
 * (R, S, stride, pad), identical packed weights, workspace and result contract -- the layers it serves are conv2 of
 * every BottleneckBlock (detectron2/modeling/backbone/resnet.py:178-187 with STRIDE_IN_1X1), the FPN output convs
 * (fpn.py:88-96) and the RPN head conv (rpn.py:83).  The output is tiled as 2-D pixel patches x 128 channels and the
 * (PH+2) x (PW+2) activation window of a 32-channel chunk is staged once in LDS for all nine taps. */
int lvc_conv3x3_nhwc_bf16x3(const float* x, const unsigned short* w_split, const float* scale, const float* shift,
                            const float* residual, float* y, int N, int H, int W, int C, int K, int Kg, int relu,
                            int res_mode, int ldy, int ldr, void* workspace, void* stream);

/* Two-way fp16 operand split (Ootomo & Yokota 2022) form of lvc_conv3x3_nhwc_bf16x3 (csrc/conv3x3_halo_h2.hip):
 * a = a1 + 2^-11 a2 with a1 = fp16(a), a2 = fp16((a - a1) * 2048); products a1 b1 (main accumulator) and a1 b2 + a2 b1
 * (cross accumulator, folded in as cross / 2048): three fp16 MFMAs per block instead of six bf16 ones, two operand planes
 * instead of three, fp32-level accuracy.  w_split: [2][Kpad][Kg] fp16 planes (w1, (w - w1) * 2048), same k order and
 * padding as the bf16 planes.  Operands beyond fp16's range (|a| > 65504, NaN) set bit 1 of the workspace error word
 * (the word after the LVC worker flags; lvc_amd.kernels.conv_error_word reads it).  No small-map fallback. */
int lvc_conv3x3_nhwc_f16x2(const float* x, const unsigned short* w_split, const float* scale, const float* shift,
                           const float* residual, float* y, int N, int H, int W, int C, int K, int Kg, int relu,
                           int res_mode, int ldy, int ldr, void* workspace, void* stream);
/* Single-accumulator, software-pipelined form of lvc_conv3x3_nhwc_f16x2 (csrc/conv3x3_halo_s1.hip; the forward 3x3 layers of
 * detectron2/modeling/backbone/resnet.py:195-211, fpn.py:101-113 and proposal_generator/rpn.py:108-127).  Same arguments and
 * results except the weights: w_split = the [2][Kpad][Kg] fp16 planes of lvc_split_weights_rowscaled (row k times 2^e_k, the
 * residual plane unscaled), and `scale` (never NULL) = (the layer's per-channel scale or 1) x row_factor[k] of that call.
 * Activations are multiplied by 2^4 before their split: |a| > 4094 (or NaN) sets bit 1 of the workspace error word. */
int lvc_conv3x3_nhwc_f16s1(const float* x, const unsigned short* w_split, const float* scale, const float* shift,
                           const float* residual, float* y, int N, int H, int W, int C, int K, int Kg, int relu,
                           int res_mode, int ldy, int ldr, void* workspace, void* stream);
/* lvc_conv3x3_nhwc_f16x2 -- same arguments, weight planes, numerics (main + cross accumulators, |a| <= 65504) and results up to
 * the fp32 summation order -- on the software-pipelined tap loop of csrc/conv3x3_halo_s1.hip (LDS-DMA weight ring, rotating
 * fragment registers, barrier in the middle of a tap, double-buffered halo window). */
int lvc_conv3x3_nhwc_f16x2_pipe(const float* x, const unsigned short* w_split, const float* scale, const float* shift,
                                const float* residual, float* y, int N, int H, int W, int C, int K, int Kg, int relu,
                                int res_mode, int ldy, int ldr, void* workspace, void* stream);
/* L <= 6 maps [N,Hs[l],Ws[l],C] through the SAME 3x3 / stride 1 / pad 1 layer in ONE launch of that kernel (ys[l] [N,Hs[l],Ws[l],K]; xs / ys /
 * Hs / Ws are [host] arrays): one stream-K split over the row tiles of all maps -- StandardRPNHead.conv over the pyramid levels
 * (detectron2/modeling/proposal_generator/rpn.py:112-120 calls it once per level).  oneacc: 1 = the arguments of lvc_conv3x3_nhwc_f16s1,
 * 0 = those of lvc_conv3x3_nhwc_f16x2_pipe.  No residual.  Per output pixel the arithmetic is the single-map launch's. */
int lvc_conv3x3_nhwc_f16_levels(int oneacc, const float* const* xs, float* const* ys, const int* Hs, const int* Ws, int L,
                                const unsigned short* w_split, const float* scale, const float* shift, int N, int C, int K, int Kg,
                                int relu, void* workspace, void* stream);
/* ... with a POINTWISE layer on top of act(conv), the hidden maps never written: StandardRPNHead.forward of the reference
 * (detectron2/modeling/proposal_generator/rpn.py:112-120: t = relu(conv(x)); objectness_logits(t), anchor_deltas(t)) as one launch over
 * the levels.  ys[l] [N,Hs[l],Ws[l],pred_ld] are the POINTWISE layer's outputs and must be ZEROED by the caller (every workgroup adds
 * its 128-channel slice of the contraction atomically: K = 128 or 256 hidden channels -> at most two addends per element, the sum does
 * not depend on their order).  oneacc must be 0 (w_split / scale / shift as for lvc_conv3x3_nhwc_f16x2_pipe).  pred_w: the
 * [2][pred_rows >= 32][K] fp16 planes lvc_split_weights writes for the pointwise weights [pred_rows][K] (rows >= pred_K zero), pred_scale /
 * pred_shift [pred_K] or NULL, 1 <= pred_K <= 32 <= pred_rows, pred_ld >= pred_K.  pred_slot: the pointwise layer's range word (a hidden
 * value beyond 65504 raises it; the 3x3 layer's own word is the slot set by lvc_set_range_slot). */
int lvc_conv3x3_nhwc_f16_levels_pred(int oneacc, const float* const* xs, float* const* ys, const int* Hs, const int* Ws, int L,
                                     const unsigned short* w_split, const float* scale, const float* shift, int N, int C, int K, int Kg,
                                     int relu, const unsigned short* pred_w, const float* pred_scale, const float* pred_shift, int pred_K,
                                     int pred_rows, int pred_ld, int pred_slot, void* workspace, void* stream);
/* The same with a LAYER per map (L layers of one shape and form: the FPN output convs, detectron2/modeling/backbone/fpn.py:128-141): ws /
 * scales / shifts are [host] arrays of L device pointers (shift entries may be NULL). */
int lvc_conv3x3_nhwc_f16_layers(int oneacc, const float* const* xs, float* const* ys, const int* Hs, const int* Ws, int L,
                                const unsigned short* const* ws, const float* const* scales, const float* const* shifts, int N, int C,
                                int K, int Kg, int relu, void* workspace, void* stream);
/* Work distribution of the two entries below: 0 (default) = one workgroup per tile; 1 = stream-K (one resident workgroup per CU takes an
 * equal share of the (tile, 16-channel chunk) list; split tiles are completed through `workspace` as in the other conv kernels, in worker
 * order: deterministic); 2 = persistent workgroups on whole tiles.  Measured: neither beats 0 on the detector's layers (conv3x3_wino.hip). */
void lvc_set_wino_streamk(int mode);
/* Patch decomposition of the 3x3 / stride 1 kernels.  0 = one patch shape per map (per launch for the grouped entries).  1 (default) =
 * lvc_conv3x3_nhwc_wino* cut every map into at most two regions, each with the patch shape that wastes the fewest 256-pixel tiles on it
 * (csrc/patch_plan.h); their outputs are bit-identical to 0.  2 = the direct kernel (lvc_conv3x3_nhwc_f16s1*, _f16x2_pipe, _f16_levels*,
 * _f16_layers) does the same; its outputs then differ in the last bits where the stream-K worker boundaries fall, which move with the
 * tile count -- not the default.  The library reads LVC_PATCH_PLAN (0 / 1 / 2) from the environment once, at the first launch or
 * question; the setter overrides it. */
void lvc_set_patch_plan(int mode);
int lvc_patch_plan(void);
/* Process-wide A/B and test switches (no environment lookups inside the library): the NMS ordered reduce of short lists from global
 * memory instead of LDS (same keep lists); the bf16x3 3x3 halo kernel with a fixed patch shape / without its small-map fallback. */
void lvc_set_nms_reduce_global(int on);
/* The selections after the convs, or (0) as they were before their short forms: the parity witness and A/B arm.  Bit 0: lvc_rpn_proposals
 * runs the per-level top-k as one wide launch (keys + histogram of their top 12 bits) and ONE workgroup per (image, level) for every
 * other radix pass, the take and the sort, instead of five phase launches and two finishing kernels; with bit 2 also set that workgroup
 * does the key pass too (the whole selection in one launch; measured slower on the detector's p2).  Bit 1: lvc_batched_nms's head-block
 * form puts only its head rows in order (radix select + sort of the head; the rest is sorted on the device only for an image whose head
 * block did not yield max_keep boxes).  Default 3; same outputs for every value. */
void lvc_set_select_onelaunch(int mode);
int lvc_select_onelaunch(void);
void lvc_set_halo_test_hooks(int ph, int pw, int force);
/* 3x3 / stride 1 / pad 1 as Winograd F(2,3) along x (round 5, csrc/conv3x3_wino.hip; the 256-channel layers of
 * detectron2/modeling/backbone/fpn.py:141-144 and proposal_generator/rpn.py:92-94 on the large maps): two thirds of the MFMAs of
 * lvc_conv3x3_nhwc_f16s1 at the same operand precision and the direct evaluation's fp32 error.  u = transformed row-scaled weight planes
 * [3][C/16][4][2][Kpad][16] fp16 (Kpad % 128 == 0), scale [K] = their row factors x the layer's scale (lvc_amd.kernels.pack_wino);
 * C % 16 == 0; |window value| <= 4094 or the layer's range word in `workspace` is raised. */
int lvc_conv3x3_nhwc_wino(const float* x, const unsigned short* u, const float* scale, const float* shift, float* y, int N, int H, int W,
                          int C, int K, int Kpad, int relu, int ldy, void* workspace, void* stream);
/* ... with a pointwise layer (<= 32 outputs; the RPN predictor, rpn.py:95-106) on top of act(conv): y [N,H,W,ldy] = its outputs, ZEROED
 * by the caller, the hidden map is never written; K in {128, 256} (at most two atomically added slices per element: order-free).  pred_*
 * as for lvc_conv3x3_nhwc_f16_levels_pred. */
int lvc_conv3x3_nhwc_wino_pred(const float* x, const unsigned short* u, const float* scale, const float* shift, float* y, int N, int H,
                               int W, int C, int K, int Kpad, int relu, int ldy, const unsigned short* pred_w, const float* pred_scale,
                               const float* pred_shift, int pred_K, int pred_rows, int pred_slot, void* workspace, void* stream);
/* Pointwise (R = S = 1, pad 0) layers with a long contraction on the pipelined loop of the 3x3 kernel (csrc/conv_pw_s1.hip; the conv1
 * / FC layers of detectron2/modeling/backbone/resnet.py:195-211, roi_heads/box_head.py:80-93 and the ViT linears): y = act(conv(x,
 * w) * scale + shift (+ residual)), x [N,H,W,C] fp32 NHWC with C % 32 == 0, stride >= 1, relu: 0 none / 1 ReLU / 2 exact GELU,
 * res_mode / ldy / ldr / workspace as lvc_conv2d_nhwc_f16x2.  _f16x2_pipe: the numerics and weight planes of
 * lvc_conv2d_nhwc_f16x2 (|a| <= 65504).  _f16s1: the single-accumulator form, w_split / scale as for lvc_conv3x3_nhwc_f16s1
 * (|a| <= 4094). */
int lvc_conv1x1_nhwc_f16x2_pipe(const float* x, const unsigned short* w_split, const float* scale, const float* shift,
                                const float* residual, float* y, int N, int H, int W, int C, int K, int stride, int relu,
                                int res_mode, int ldy, int ldr, void* workspace, void* stream);
int lvc_conv1x1_nhwc_f16s1(const float* x, const unsigned short* w_split, const float* scale, const float* shift,
                           const float* residual, float* y, int N, int H, int W, int C, int K, int stride, int relu,
                           int res_mode, int ldy, int ldr, void* workspace, void* stream);
/* A bottleneck's conv2 -> conv3 hand-over without the consumer's operand split (round 6; reference resnet.py:200-212).
 * lvc_conv3x3_nhwc_f16s1_presplit = lvc_conv3x3_nhwc_f16s1 with ReLU and no residual whose output y [N,H,W,K] (K % 32 == 0; same bytes as
 * the fp32 tensor) holds, per pixel and 32-channel chunk, the 32 hi halves then the 32 lo halves of the two-way fp16 split of the result
 * x 2^4 -- the planes lvc_conv1x1_nhwc_f16s1's own split would form; a value beyond |a| <= 4094 raises range word `next_slot` (the
 * consumer's).  lvc_conv1x1_nhwc_f16s1_presplit = lvc_conv1x1_nhwc_f16s1 (stride 1, K > 64) reading such planes: the same products in
 * the same order, results bit-identical to the fp32 hand-over. */
int lvc_conv3x3_nhwc_f16s1_presplit(const float* x, const unsigned short* w_split, const float* scale, const float* shift, void* y,
                                    int N, int H, int W, int C, int K, int Kg, int next_slot, void* workspace, void* stream);
int lvc_conv1x1_nhwc_f16s1_presplit(const void* x, const unsigned short* w_split, const float* scale, const float* shift,
                                    const float* residual, float* y, int N, int H, int W, int C, int K, int relu,
                                    int res_mode, int ldy, int ldr, void* workspace, void* stream);
/* _f16s1_w2 (round 5, csrc/conv_pw_w2.hip): the single-accumulator form on a 256-row x 256-channel workgroup tile (wave tile 64 x
 * 128, 16-deep stages) for layers with >= 256 input and output channels -- res4 / res5 conv1 and conv3, the FPN laterals
 * (detectron2/modeling/backbone/fpn.py:128-140), box-head fc1 / fc2: 0.67 x the operand bytes per MFMA of the 256 x 128 tile.  Same
 * operands and results as lvc_conv1x1_nhwc_f16s1 up to the fp32 summation order; C % 16 == 0; Kpad = rows of a weight plane
 * (>= K rounded up to 256). */
int lvc_conv1x1_nhwc_f16s1_w2(const float* x, const unsigned short* w_split, const float* scale, const float* shift,
                              const float* residual, float* y, int N, int H, int W, int C, int K, int Kpad, int stride, int relu,
                              int res_mode, int ldy, int ldr, void* workspace, void* stream);
/* Two chained pointwise layers in one launch, the second fed from the first one's accumulators (csrc/conv_pw_chain.hip):
 *   y1 = act1(x Wa^T * sa + ta (+ residual))   -- a bottleneck's conv3 + FrozenBN + shortcut add + ReLU,
 *   y2 = act2(y1 Wb^T * sb + tb)               -- the next bottleneck's conv1 + FrozenBN + ReLU,
 * detectron2/modeling/backbone/resnet.py:205-211 of block i followed by :195-197 of block i+1; both results are stored, y1 is never
 * read back.  x [M][ldx] (K1 channels), residual [M][ldr] or NULL, y1 [M][ldy1] (N1), y2 [M][ldy2] (N2).  wa [2][wa_rows][K1] /
 * wb [2][wb_rows][N1]: fp16 planes of lvc_split_weights_rowscaled over weights whose contraction index is permuted within every
 * 16 entries (0-3, 8-11, 4-7, 12-15); sa / sb = (per-channel scale or 1) x that call's row factors (never NULL); ta / tb shifts
 * or NULL; relu1 / relu2: 0 none, 1 ReLU.  (K1, N1, N2) in {(64,256,64), (128,256,64), (128,512,128)}.  |x| or |y1| > 4094 (or
 * NaN) sets bit 1 of the workspace error word. */
int lvc_conv1x1_chain_nhwc_f16s1(const float* x, int ldx, const unsigned short* wa, int wa_rows, const float* sa, const float* ta,
                                 const float* residual, int ldr, float* y1, int ldy1, int relu1, const unsigned short* wb,
                                 int wb_rows, const float* sb, const float* tb, float* y2, int ldy2, int relu2, int M, int K1,
                                 int N1, int N2, void* workspace, void* stream);
/* A whole bottleneck block in one launch (round 6, csrc/conv_bneck.hip), replacing the three conv + FrozenBN launches and the shortcut
 * add of detectron2/modeling/backbone/resnet.py:195-211 for the 64-mid / 256-output-channel blocks of res2 (stride 1):
 *   y = relu(bn3(conv3(relu(bn2(conv2(relu(bn1(conv1(x)))))))) + shortcut(x)).
 * conv1's output lives in LDS (output tile + one-pixel halo, fp16 planes), conv2's in registers; x is read once, y written once.
 * x [N][H][W][ldx] (cin channels used), y [N][H][W][ldy].  proj = 0: cin = 256, shortcut = x.  proj = 1: cin = 64, the projection
 * shortcut's weights are the last 64 contraction columns of the third layer.  w: stage images built by
 * lvc_amd.kernels.pack_bottleneck (row-scaled fp16 planes of lvc_split_weights_rowscaled in fragment order: (cin/32) x 8 KB,
 * 18 x 8 KB, 8 or 16 x 8 KB: 34 or 36 stages of eight 1 KB fragments); s1/t1, s2/t2 (64 entries), s3/t3 (256): epilogue scales (x row factors) and shifts, never NULL.
 * |x|, |conv1 out| or |conv2 out| > 4094 (or non-finite) sets bit 1 / 2 of the launch's range word. */
int lvc_bottleneck_nhwc_f16s1(const float* x, int ldx, float* y, int ldy, int N, int H, int W, int cin, int proj,
                              const unsigned short* w, const float* s1, const float* t1, const float* s2, const float* t2,
                              const float* s3, const float* t3, void* workspace, void* stream);
/* wp [rows][Kg] fp32 (lvc_pack_conv_weights) -> planes_out [2][rows][Kg] fp16: w1 = fp16(wp 2^e), w2 = fp16(wp 2^e - w1) with
 * e = 13 - floor(log2(max |wp[row][:]|)) per row (0 for an all-zero row); row_factor[row] = 2^-(e + 4). */
int lvc_split_weights_rowscaled(const float* wp, int rows, int Kg, void* planes_out, float* row_factor, void* stream);

/* Two-way fp16 split form of the POINTWISE shapes of lvc_conv2d_nhwc_bf16x3 (csrc/conv_f16x2.hip): R = S = 1, pad 0
 * and (C <= 512 or N*Ho*Wo >= 2048); anything else returns LVC_ERR_INVALID.  w_split as lvc_conv3x3_nhwc_f16x2. */
int lvc_conv2d_nhwc_f16x2(const float* x, const unsigned short* w_split, const float* scale, const float* shift,
                          const float* residual, float* y, int N, int H, int W, int C, int K, int R, int S,
                          int stride, int pad, int Kg, int relu, int res_mode, int ldy, int ldr, void* workspace,
                          void* stream);
/* The same contract for pointwise layers (R = S = 1, pad 0, C % 32 == 0; y and residual below 2 GiB), operands streamed by
 * LDS-DMA (csrc/conv_pw_dma.hip: raw fp32 activation rows and the fp16 weight planes go HBM/L2 -> LDS by
 * global_load_lds_dwordx4 in a three-stage ring that runs across tile boundaries, the fp16 split happens in registers at
 * fragment time, the epilogue stores from the accumulators).  Results equal lvc_conv2d_nhwc_f16x2's to fp32 rounding
 * (same products, same accumulation order per tile).  LVC_ERR_INVALID for non-pointwise shapes. */
int lvc_conv2d_nhwc_f16x2_dma(const float* x, const unsigned short* w_split, const float* scale, const float* shift,
                          const float* residual, float* y, int N, int H, int W, int C, int K, int R, int S,
                          int stride, int pad, int Kg, int relu, int res_mode, int ldy, int ldr, void* workspace,
                          void* stream);

/* BasicStem in one launch (detectron2/modeling/backbone/resnet.py:588-592): conv 7x7 s2 p3 (3 -> 64) -> FrozenBN fold
 * (scale/shift, NULL = identity) -> ReLU -> max_pool2d 3x3 s2 p1, with the two-way fp16 operand split (csrc/stem_pool_h2.hip).
 * x [N,H,W,4] NHWC4 (the layout lvc_preprocess_nhwc4 writes), w_split = the [2][Kpad][224] fp16 planes of the mode-1 packed
 * stem weights of lvc_conv2d_nhwc_f32 (k = r*32 + s*4 + c), Kpad >= 64 rows per plane; y [N,Hp,Wp,64] with Ho = (H-1)/2+1,
 * Hp = (Ho-1)/2+1 (same for W).  d_error_word: device int whose bit 1 is set when an input beyond fp16's range is met (may be
 * NULL).  (The three-way bf16 form of this kernel was removed in round 4: under the range-free split the stem runs as conv +
 * max-pool, two launches.) */
int lvc_stem_conv_pool_nhwc4_f16x2(const float* x, const unsigned short* w_split, const float* scale, const float* shift,
                                   float* y, int N, int H, int W, int Kpad, int relu, int* d_error_word,
                                   float* y2 /* optional second copy of y, rows of ldy2 floats */, int ldy2, void* stream);

/* GeneralizedRCNN.preprocess_image (lvc/modeling/meta_arch/rcnn.py:324-333) + ImageList.from_tensors
 * padding (detectron2/structures/image_list.py:95-119): out[y,x,:] = ((img[:,y,x]-mean)/std, 0), zero
 * outside h x w.  image: CHW, dtype 0 = fp32, 1 = uint8.  mean3/std3 are [host] arrays of 3 floats. */
int lvc_preprocess_nhwc4(const void* image, int dtype, int h, int w, const float* mean3, const float* std3,
                         float* out, int Hp, int Wp, void* stream);
/* The same for B images in one launch (16 per launch): images[i] -> out[i] ([B,Hp,Wp,4]); all float32 or all uint8. */
int lvc_preprocess_batch_nhwc4(const void* const* images, int dtype, const int* hs, const int* ws, int B, const float* mean3,
                               const float* std3, float* out, int Hp, int Wp, void* stream);

/* Test-time input pipeline: ResizeShortestEdge's Pillow bilinear resize of a uint8 HWC image
 * (detectron2/data/transforms/transform.py:101-109), bit-exact with Pillow's ImagingResample (22-bit fixed point,
 * horizontal then vertical pass, uint8 intermediate), optionally fused with preprocess_image's normalise + zero-pad
 * (lvc/modeling/meta_arch/rcnn.py:324-333) into the batch's NHWC4 slot.
 *   image [H,W,3] u8; xb [new_w,2] / xk [new_w,kxs] int32 = (first source column, count) and coefficients of each
 *   output column (NULL when new_w == W; host: lvc_amd/data/transforms.py resample_coeffs = Pillow's
 *   precompute_coeffs + normalize_coeffs_8bpc); yb / yk / kys likewise for rows; tmp: H*new_w*3 bytes of scratch;
 *   out_u8 [new_h,new_w,3] and out_nhwc4 [Hp,Wp,4] fp32 are each optional; mean3 / std3: host float[3]. */
int lvc_resize_bilinear_u8(const unsigned char* image, int H, int W, int new_h, int new_w, const int* xb, const int* xk,
                           int kxs, const int* yb, const int* yk, int kys, unsigned char* tmp, unsigned char* out_u8,
                           float* out_nhwc4, int Hp, int Wp, const float* mean3, const float* std3, void* stream);
/* Test-time augmentation (lvc_amd/csrc/tta.hip; reference detectron2/modeling/test_time_augmentation.py).
 * lvc_tta_resize_u8: every ResizeShortestEdge size (+ its horizontal mirror) of one uint8 image, Pillow-exact as
 *   lvc_resize_bilinear_u8, in two launches for up to 16 sizes: image element (y,x,c) at image[y*sy + x*sx + c*sc];
 *   hjobs host int64 [n_h][5] = (xb, xk, kxs, new_w, tmp) per distinct output width != W; vjobs host int64 [n_v][14] =
 *   (source hjob or -1, yb, yk or 0, kys, new_h, new_w, u8, u8 mirrored, slot, Hp, Wp, mirrored slot, Hpm, Wpm), each output
 *   optional (u8 [new_h,new_w,3]; slots [Hp,Wp,4] fp32 = (v - mean) / std, zero padded, as preprocess_image).
 * lvc_tta_merge: union of B images' augmentation detections (boxes [A,topk_in,4], scores, classes int32, counts [A]) through
 *   the inverse transforms (params [A][16] fp32 device), finite filter, clip, score > score_thresh, per-class NMS, first topk_out;
 *   tab [B][4] int32 device = (first augmentation, end, height, width).  Outputs [B,topk_out] + count [B]; no host sync. */
int lvc_tta_resize_u8(const unsigned char* image, int H, int W, long long sy, long long sx, long long sc, const long long* hjobs,
                      int n_h, const long long* vjobs, int n_v, const float* mean3, const float* std3, void* stream);
long long lvc_tta_merge_workspace_bytes(int B, int Nmax);
int lvc_tta_merge(const float* boxes, const float* scores, const int* classes, const int* counts, int topk_in, const float* params,
                  const int* tab, int B, int Nmax, float score_thresh, double nms_thresh, int topk_out, float* ob, float* osc, int* ocl,
                  int* ocount, void* workspace, long long workspace_bytes, void* stream);
/* Training input of a whole batch (lvc_amd/csrc/train_input.hip; reference lvc/data/dataset_mapper.py:90-209): RandomCrop ->
 * ResizeShortestEdge (Pillow-exact, as lvc_resize_bilinear_u8, coefficients for the CROPPED size -> the output size) -> RandomFlip
 * -> normalise + zero-pad, for B uint8 images of different sizes in two launches whatever B is.
 *   h_blob (host) / d_blob (its device copy), blob_bytes: int64 jobs [B][24] first, the int32 bounds / coefficient tables behind
 *   them at the byte offsets the jobs name.  Job words: 0 source pointer (element (y,x,c) at src[y*sy + x*sx + c*sc]), 1 H, 2 W,
 *   3 sy, 4 sx, 5 sc, 6 x0, 7 y0, 8 crop w, 9 crop h, 10 new_h, 11 new_w, 12 xb offset (-1: width unchanged), 13 xk offset,
 *   14 kxs, 15 yb offset (-1: height unchanged), 16 yk offset, 17 kys, 18 flip, 19 slot, 20 optional uint8 output pointer
 *   [new_h,new_w,3] (0: none), 21 byte offset of the job's [crop h,new_w,3] intermediate in tmp; 22-23 reserved.
 *   out [n_slots,Hp,Wp,4] fp32 = (v - mean) / std, zero padded; mean3 / std3: host float[3].  The host blob is validated (windows
 *   inside their images, taps inside their crops, outputs inside their buffers) before anything is launched.  launches: optional,
 *   receives the number of kernel launches issued (at most two). */
int lvc_train_input_u8(const void* h_blob, const void* d_blob, long long blob_bytes, int B, unsigned char* tmp, long long tmp_bytes,
                       float* out, int n_slots, int Hp, int Wp, const float* mean3, const float* std3, int* launches, void* stream);
/* The same for images that are mosaics of 1 to 9 tiles (reference lvc/data/mosaic.py get_mosaic / get_mosaic9; a plain image is a
 * job with one tile), read in place: neither the canvas nor the composite is written to memory; two launches whatever B and the mix.
 *   A job's source is a canvas: tile t covers the canvas rectangle [x1a,x2a) x [y1a,y2a) with its pixels from (x1b,y1b) on, tiles
 *   are painted in order (the later one wins where rectangles overlap), what no tile covers is 114.  Arguments as
 *   lvc_train_input_u8, with int64 jobs [B][128] first in the blob.  Job words: 0 X0, 1 Y0, 2 crop w, 3 crop h (the crop window in
 *   canvas coordinates), 4 new_h, 5 new_w, 6 xb offset (-1: width unchanged), 7 xk offset, 8 kxs, 9 yb offset (-1: height
 *   unchanged), 10 yk offset, 11 kys, 12 flip, 13 slot, 14 optional uint8 output pointer [new_h,new_w,3] (0: none), 15 byte offset
 *   of the job's [crop h,new_w,3] intermediate in tmp (always used: the horizontal pass always runs, as a copy when the width
 *   stays), 16 number of tiles (1..9), 17-19 reserved; tile t at words 20 + 12 t: 0 source pointer (element (y,x,c) at
 *   src[y*sy + x*sx + c*sc]), 1 H, 2 W, 3 sy, 4 sx, 5 sc, 6 x1a, 7 y1a, 8 x2a, 9 y2a, 10 x1b, 11 y1b.
 *   Refused before anything is launched: a tile count outside 1..9, a null tile pointer, non-positive strides, a rectangle with
 *   negative extent, any pixel of a rectangle inside the window that maps outside its tile, taps outside the window, an output
 *   outside the padded batch, two jobs on one slot, an intermediate outside tmp. */
int lvc_train_input_tiles_u8(const void* h_blob, const void* d_blob, long long blob_bytes, int B, unsigned char* tmp,
                             long long tmp_bytes, float* out, int n_slots, int Hp, int Wp, const float* mean3, const float* std3,
                             int* launches, void* stream);
/* INPUT.LSJ (reference ResizeScale -> FixedSizeCrop -> RandomFlip, detectron2/data/transforms/augmentation_impl.py:123-161, 391-431)
 * of a whole batch in two launches (lvc_amd/csrc/train_input.hip): the crop window of a tiled job (tiles and painting rule of
 * lvc_train_input_tiles_u8; a plain image or a jittered crop is one tile) is resized WHOLE to sh x sw with Pillow's tables for the
 * full resize, of which only the output window (ox, oy, ow, oh) is computed -- the scaled image is never written -- and placed at
 * the top left of a th x tw canvas whose right and bottom are `fill`; a flipped job mirrors the canvas (fill on the left).
 *   Arguments as lvc_train_input_tiles_u8, with int64 jobs [B][140] first in the blob.  Job words: 0 X0, 1 Y0, 2 crop w, 3 crop h,
 *   4 sh, 5 sw (the whole scaled image), 6 xb offset (-1: width unchanged), 7 xk offset, 8 kxs, 9 yb offset (-1: height unchanged),
 *   10 yk offset, 11 kys (tables of the full crop -> scaled resize), 12 flip, 13 slot, 14 optional uint8 output pointer [th,tw,3]
 *   (0: none), 15 byte offset of the job's [bh,ow,3] intermediate in tmp, 16 number of tiles (1..9), 17 ox, 18 oy, 19 ow, 20 oh,
 *   21 th, 22 tw, 23 fill byte, 24 by0, 25 bh (the band of crop-window rows the vertical taps of rows [oy, oy + oh) touch; the rows
 *   themselves where the height stays), 26-31 reserved; tile t at words 32 + 12 t as in lvc_train_input_tiles_u8.
 *   out [n_slots,Hp,Wp,4] fp32 = (v - mean) / std on the canvas, zero outside it.  Refused before anything is launched: what
 *   lvc_train_input_tiles_u8 refuses of a window and its tiles, an output window outside the scaled image or larger than the canvas,
 *   a canvas outside the padded batch, a fill that is no byte, a band outside the crop window, column taps outside the crop window,
 *   row taps outside the band, two jobs on one slot, an intermediate outside tmp or over another job's. */
int lvc_train_input_lsj_u8(const void* h_blob, const void* d_blob, long long blob_bytes, int B, unsigned char* tmp,
                           long long tmp_bytes, float* out, int n_slots, int Hp, int Wp, const float* mean3, const float* std3,
                           int* launches, void* stream);
/* INPUT.COLOR_JITTER (reference ColorJitterPIL: torchvision's ColorJitter on a PIL image, i.e. Pillow's ImageEnhance blends,
 * convert("L") and RGB <-> HSV conversion) of a whole batch (csrc/color_jitter.hip): per job the crop window of a canvas painted
 * from 1 to 9 tiles (tiles and painting rule of lvc_train_input_tiles_u8) goes through up to four steps in the job's own order and
 * leaves as a packed uint8 [crop h][crop w][3] image at the job's byte offset in `out`, which lvc_train_input_u8 then reads as a
 * plain image.  Two launches whatever B and the mix: the sum of grey levels the contrast step needs (64-bit integer atomics into
 * word 19 of the job's row in d_blob, which is therefore written), then the pixels.  Bytes equal Pillow's.
 *   h_blob / d_blob / blob_bytes: int64 jobs [B][128], host copy and device copy.  Job words: 0 X0, 1 Y0, 2 crop w, 3 crop h (canvas
 *   coordinates), 4 byte offset of the output in `out` (a multiple of 4), 5 n_ops (0..4), 6-9 step ids in the order applied (0
 *   brightness, 1 contrast, 2 saturation, 3 hue; at most one contrast step), 10-13 their factors (the bits of an fp32 in the low
 *   half; hue: the hue factor in [-0.5, 0.5]), 14 number of tiles (1..9), 15-18 reserved, 19 zero (the sum); tile t at words
 *   20 + 12 t as in lvc_train_input_tiles_u8.
 *   Refused before anything is launched: what lvc_train_input_tiles_u8 refuses of a window and its tiles, a step count outside
 *   0..4, a step id outside 0..3, a second contrast step, a factor outside its range, a non-zero sum word, an output outside `out`
 *   or over another job's.  launches: optional, the number of kernel launches issued (two). */
int lvc_color_jitter_tiles_u8(const void* h_blob, void* d_blob, long long blob_bytes, int B, unsigned char* out, long long out_bytes,
                              int* launches, void* stream);
/* F.max_pool2d on NHWC (BasicStem resnet.py:591: k3 s2 p1; LastLevelMaxPool fpn.py:176: k1 s2 p0). */
int lvc_maxpool2d_nhwc(const float* x, float* y, int N, int H, int W, int C, int k, int stride, int pad,
                       void* stream);

/* Descriptor crops (lvc/data/utils.py:485-519 get_crops_qe): zero-pad the box window to a square and resize to
 * out_size x out_size with F.interpolate(mode='nearest').  image [C,H,W]; d_windows [K,8] int32 =
 * (x1,y1,x2,y2 inclusive, l_pad, t_pad, side_w, side_h) (integer bookkeeping done by the host); out [K,C,out,out]. */
int lvc_crop_resize_nearest(const float* image_chw, int C, int H, int W, const int* d_windows, int K, int out_size,
                            float* out, void* stream);

/* Row-wise (x - mu) / den; den = |x-mu| + eps (mode 0, CosineSimOutputLayers fast_rcnn.py:822-833) or
 * max(|x-mu|, eps) (mode 1, F.cosine_similarity as used by tools/run_nearest_neighbours.py:150-153). */
int lvc_rownorm(const float* x, const float* mu, float* y, int M, int D, int ldx, int ldy, float eps, int mode,
                void* stream);
/* Backward of lvc_rownorm mode 0 without mu (CosineSimOutputLayers training, lvc/modeling/roi_heads/fast_rcnn.py:
 * 823-825): dx = dy/(n+eps) - x (dy.x)/((n+eps)^2 n), n = |x| per row; accumulate != 0 adds to dx. */
int lvc_rownorm_backward(const float* x, const float* dy, float* dx, int M, int D, float eps, int accumulate, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * ROIAlign forward.  Same arithmetic as ROIAlign_cpu.cpp:20-218 / ROIAlign_cuda.cu:65-139 (and the same operation order in the NCHW form).
 * lvc_roi_align_forward_nchw has the reference op's shape contract (csrc/vision.cpp:96):
 *   input [B,C,H,W], rois [K,5] = (batch index, x1, y1, x2, y2), output [K,C,pooled_h,pooled_w].
 * lvc_roi_align_fpn_nhwc is the engine form: L pyramid levels [B,H_l,W_l,C] (feats/Hs/Ws/scales are [host]
 * arrays of L entries), per-RoI level ids [K] int32 (NULL if L == 1), output [K,pooled_h,pooled_w,C];
 * replaces the per-level gather/ROIAlign/scatter loop of detectron2/modeling/poolers.py:236-246.
 *   The engine form sums a bin in the separable order (weights of a row and of a column pre-summed, every window pixel read once:
 *   csrc/roi_align.hip): the reference's value to fp32 rounding (1e-6 of the output scale in the tests), not its bits; the NCHW
 *   form keeps the reference's order.
 * d_num_valid (device int, may be NULL): rows >= *d_num_valid are zero-filled.
 * lvc_roi_work_order writes d_order [K], a permutation of the RoIs with the largest windows first; lvc_roi_align_fpn_nhwc_ordered
 *   lets workgroup i pool RoI d_order[i] (output row k is RoI k either way; NULL = RoI order): the launch no longer ends on a few
 *   large RoIs that started last.
 */
int lvc_roi_align_forward_nchw(const float* input, const float* rois, float* output, int B, int C, int H, int W,
                               int K, int pooled_h, int pooled_w, float spatial_scale, int sampling_ratio,
                               int aligned, int* d_status, void* stream);
int lvc_roi_align_fpn_nhwc(const float* const* feats, const int* Hs, const int* Ws, const float* scales, int L,
                           int B, int C, const float* rois, const int* levels, const int* d_num_valid, int K,
                           int pooled_h, int pooled_w, int sampling_ratio, int aligned, float* output,
                           int* d_status, void* stream);
int lvc_roi_work_order(const float* rois, const int* levels, const float* scales, int L, int K, int pooled_h, int* d_order,
                       void* stream);
/* XCD-local order for B <= 16 images: position i holds a RoI of image i % B (workgroup i runs on XCD i % 8), inside an image by
 * (level, 16-pixel band of the box centre's row) -- the windows an XCD reads next to each other in time share its L2. */
int lvc_roi_work_order_xcd(const float* rois, const int* levels, int K, int B, int* d_order, void* stream);
int lvc_roi_align_fpn_nhwc_ordered(const float* const* feats, const int* Hs, const int* Ws, const float* scales, int L,
                                   int B, int C, const float* rois, const int* levels, const int* d_num_valid, int K,
                                   int pooled_h, int pooled_w, int sampling_ratio, int aligned, float* output,
                                   int* d_status, const int* d_order, void* stream);

/* ROIAlign backward (csrc/vision.cpp:97 roi_align_backward; ROIAlign_cuda.cu:142-306 / ROIAlign_cpu.cpp:219-406):
 *   grad [K,C,pooled_h,pooled_w] contiguous -> grad_input [B,C,H,W], zeroed by the call (the reference returns a
 *   fresh at::zeros tensor).  Scatter by fp32 atomic adds like the reference CUDA kernel: equal to the reference CPU
 *   kernel up to summation order.  The _fpn_ form is the gradient of lvc_roi_align_fpn_nhwc: grad
 *   [K,pooled_h,pooled_w,C] -> grad_feats[l] [B,H_l,W_l,C] (grad_feats/Hs/Ws/scales are [host] arrays of L entries). */
int lvc_roi_align_backward_nchw(const float* grad, const float* rois, float* grad_input, int B, int C, int H, int W,
                                int K, int pooled_h, int pooled_w, float spatial_scale, int sampling_ratio,
                                int aligned, int* d_status, void* stream);
int lvc_roi_align_fpn_backward_nhwc(const float* grad, float* const* grad_feats, const int* Hs, const int* Ws,
                                    const float* scales, int L, int B, int C, const float* rois, const int* levels,
                                    const int* d_num_valid, int K, int pooled_h, int pooled_w, int sampling_ratio,
                                    int aligned, int* d_status, void* stream);
/* The kernel a ROIAlign call of these shapes runs, on plain numbers ([host] only, no launch): the one dispatch both directions use.
 *   forward (backward = 0): 0 scalar (NCHW, C % 4 != 0 or d_num_valid given), 1 one wave per output bin (dwordx4 taps), 2 one wave
 *   per output row (separable sums; pooled_h <= 8, pooled_w == 7); backward: 0 per-sample scatter, 1 separable rows (NHWC, 7 x 7).
 *   largest_level_elems: max over the levels of H_l * W_l * C (the row form keeps 32-bit offsets inside one image of a level). */
int lvc_roi_align_route(int backward, int nhwc, int C, int pooled_h, int pooled_w, int has_num_valid,
                        long long largest_level_elems);

/* ---------------------------------------------------------------------------------------------------
 * Batched NMS, B images per call.  Replaces torchvision.ops.boxes.batched_nms / nms as called from
 * detectron2/layers/nms.py:10-29 (consumers proposal_utils.py:104, lvc fast_rcnn.py:128).  Keep indices are
 * bit-exact w.r.t. the CPU algorithm (offset trick in fp32, IoU in fp32 compared against the double
 * threshold, score ties -> lower index).
 *   boxes [B,Nmax,4], scores [B,Nmax], idxs [B,Nmax] int32 or NULL, d_counts [B] int32 or NULL (= Nmax)
 *   keep [B,Nmax] int32 (indices into the image's rows, score-descending), d_num_keep [B] int32
 *   max_keep <= 0: unlimited.  Any Nmax: up to 16384 rows per image run as one LDS sort + one mask + one reduce launch;
 *   beyond that (the reference switches to a per-class loop at 40000 boxes, nms.py:22-29, same result) a global bitonic
 *   sort and the greedy pass in blocks of 16384 sorted rows.
 */
long long lvc_batched_nms_workspace_bytes(int B, int Nmax);
int lvc_batched_nms(const float* boxes, const float* scores, const int* idxs, const int* d_counts, int B,
                    int Nmax, double iou_threshold, int max_keep, int* keep, int* d_num_keep, void* workspace,
                    long long workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * RPN.predict_proposals + find_top_rpn_proposals (detectron2/modeling/proposal_generator/rpn.py:455-508,
 * proposal_utils.py:13-118, anchor_generator.py:157-178, box_regression.py:73-110), inference branch.
 *   per level l (arrays of L [host] entries):
 *     logits[l]  device ptr: objectness of anchor a at pixel p of image b = logits[l][(b*H*W + p)*ld_logit[l] + a]
 *     deltas[l]  device ptr: delta c of anchor a                          = deltas[l][(b*H*W + p)*ld_delta[l] + a*4 + c]
 *     cell_anchors[l] device ptr [A,4]; Hs, Ws, strides
 *   d_image_sizes [B,2] int32 (h, w).  Outputs: out_boxes [B,post,4], out_logits [B,post] (zero rows past
 *   d_out_count[b]).  pre_nms_topk <= 2048.
 */
long long lvc_rpn_proposals_workspace_bytes(int B, int L, int A, const int* Hs, const int* Ws, int pre_nms_topk);
int lvc_rpn_proposals(const float* const* logits, const int* ld_logit, const float* const* deltas,
                      const int* ld_delta, const float* const* cell_anchors, const int* Hs, const int* Ws,
                      const int* strides, int L, int A, int B, const int* d_image_sizes, int pre_nms_topk,
                      int post_nms_topk, double nms_thresh, float min_box_size, float scale_clamp,
                      float* out_boxes, float* out_logits, int* d_out_count, void* workspace,
                      long long workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * RetinaNet.inference_single_image, the loop over the levels (detectron2/modeling/meta_arch/retinanet.py:327-353,
 * anchor_generator.py:157-178, box_regression.py:73-110), for all images and levels in one call (csrc/retinanet.hip).
 *   per level l (arrays of L [host] entries):
 *     logits[l]  device ptr: logit of class k of anchor a at pixel p of image b = logits[l][(b*H*W + p)*ld_logit[l] + a*K + k]
 *     deltas[l]  device ptr: delta c of anchor a                                = deltas[l][(b*H*W + p)*ld_delta[l] + a*4 + c]
 *       (ld_logit[l] >= A*K, ld_delta[l] >= 4*A: rows may carry padding channels, which are never read as entries)
 *     cell_anchors[l] device ptr [A,4]; Hs, Ws, strides; anchor_offset = MODEL.ANCHOR_GENERATOR.OFFSET
 *   Per (image, level), with flat index i = (p*A + a)*K + k: the min(topk, H*W*A) entries with the largest logit (equal logits:
 *   lower i first), of those the ones with sigmoid(logit) > score_thresh in fp32; class = i % K, anchor = i / K,
 *   box = apply_deltas(deltas[anchor], grid anchor; weights wx..wh, scale_clamp), not clipped.
 *   Outputs (rows = L*topk per image): out_boxes [B,rows,4], out_scores [B,rows], out_classes [B,rows] int32, out_index [B,rows]
 *   int32 (= i) -- an image's candidates level after level, densely, inside a level in selection order; d_count[b] = their
 *   number; rows past it are zero.  Bit-identical between runs.  topk <= 2048; H*W*A*K < 2^31 per level.
 *   max_survivors: capacity of the per-(image, level) list of entries above the threshold (H*W*A*K cannot overflow); an overflow
 *   ORs 4 into *d_status [1] int32 (never cleared here) and leaves the outputs of the call unspecified.
 *   One pass over the logits; no host read.
 */
long long lvc_retinanet_select_workspace_bytes(int B, int L, int A, int K, const int* Hs, const int* Ws, int topk,
                                               int max_survivors);
int lvc_retinanet_select(const float* const* logits, const int* ld_logit, const float* const* deltas, const int* ld_delta,
                         const float* const* cell_anchors, const int* Hs, const int* Ws, const int* strides,
                         float anchor_offset, int L, int A, int K, int B, int topk, float score_thresh, float wx, float wy,
                         float ww, float wh, float scale_clamp, int max_survivors, float* out_boxes, float* out_scores,
                         int* out_classes, int* out_index, int* d_count, int* d_status, void* workspace,
                         long long workspace_bytes, void* stream);

/* Gather of the rows an NMS kept, with detector_postprocess (detectron2/modeling/postprocessing.py:10-79, box fields):
 *   boxes [B,Nmax,4], scores / classes / rows [B,Nmax] (rows: any int32 carried along, e.g. out_index of lvc_retinanet_select),
 *   keep [B,Nmax] int32 + d_num_keep [B] as lvc_batched_nms writes them; the first min(d_num_keep[b], topk) kept rows, in order.
 *   d_post NULL or [B,4] fp32 = (scale_x, scale_y, out_h, out_w): scale, clip to the output size, drop empty boxes.
 *   Outputs [B,topk,...], zero past d_out_count[b]. */
int lvc_gather_detections(const float* boxes, const float* scores, const int* classes, const int* rows, const int* keep,
                          const int* d_num_keep, int B, int Nmax, int topk, const float* d_post, float* out_boxes,
                          float* out_scores, int* out_classes, int* out_rows, int* d_out_count, void* stream);

/* RetinaNet's training loss (detectron2/modeling/meta_arch/retinanet.py:184-236 `losses`: fvcore sigmoid_focal_loss "sum" over the
 * valid anchors' K entries, smooth_l1_loss "sum" of the deltas against Box2BoxTransform.get_deltas(anchor, matched gt) over the positive
 * anchors, both divided by the EMA loss normaliser) on the head's per-level NHWC outputs (csrc/retinanet_loss.hip).
 *   logits[l] / deltas[l], ld_logit / ld_delta, Hs, Ws, L (1..8), A, K, B: as for lvc_retinanet_select; padding channels are never read.
 *   anchors [R,4] (R = sum_l H_l W_l A, level after level, p*A + a inside a level), matches int32 [B,R] and labels int8 [B,R] as
 *   lvc_match_boxes_batched writes them (1: the class of the matched gt box is the target; 0: every target 0; -1: no loss, zero
 *   gradient; an image without gt is background everywhere), gt [Gtot,4], gt_classes int64 [Gtot], gt_off int32 [B+1]: all DEVICE.
 *   alpha < 0: no alpha weighting; gamma 0 or >= 1 (2, 0 and 1 do not go through powf); beta < 1e-5: pure L1.
 * lvc_retinanet_loss (two launches: the streaming pass, and a one-workgroup finish that adds the workgroups' fp64 partial sums in index
 *   order): *num_pos = the number of positive anchors, *normalizer_out = momentum * *normalizer_in + one_minus_momentum *
 *   max(num_pos, 1) in fp64 with a separately rounded multiply and add (the reference's Python float, bit for bit; the two slots must
 *   differ), out_losses [2] = (loss_cls, loss_box_reg) = the two sums / *normalizer_out, out_sums [2] (may be NULL) = the two sums
 *   themselves in fp64.  The loss terms are evaluated in fp64 (alpha, gamma, beta and the weights are doubles: the reference's Python
 *   floats), the gradient entries in fp32.  Bit-identical between runs; no host read.
 * lvc_retinanet_loss_grad (one launch): dlogits[l] [B,H_l,W_l,ld_dlogit[l]] = *g_cls / *normalizer * d(focal sum)/d(logits) and
 *   ddeltas[l] [B,H_l,W_l,ld_ddelta[l]] = *g_box / *normalizer * d(smooth-L1 sum)/d(deltas); zero on ignored anchors (dlogits), on
 *   every anchor that is not positive (ddeltas) and on the padding channels.  normalizer, g_cls, g_box: device scalars.
 * 16-byte accesses where a level's ld is a multiple of 4 and its base pointer is 16-byte aligned; scalar accesses otherwise. */
long long lvc_retinanet_loss_workspace_bytes(int B, int L, int A, int K, const int* Hs, const int* Ws);
int lvc_retinanet_loss(const float* const* logits, const int* ld_logit, const float* const* deltas, const int* ld_delta,
                       const int* Hs, const int* Ws, int L, int A, int K, int B, const float* anchors, const int* matches,
                       const signed char* labels, const float* gt, const long long* gt_classes, const int* gt_off, double alpha,
                       double gamma, double beta, double wx, double wy, double ww, double wh, double momentum,
                       double one_minus_momentum, const double* normalizer_in, double* normalizer_out, float* out_losses,
                       double* out_sums /* [2] or NULL */, int* num_pos, void* workspace, long long workspace_bytes, void* stream);
int lvc_retinanet_loss_grad(const float* const* logits, const int* ld_logit, const float* const* deltas, const int* ld_delta,
                            const int* Hs, const int* Ws, int L, int A, int K, int B, const float* anchors, const int* matches,
                            const signed char* labels, const float* gt, const long long* gt_classes, const int* gt_off, double alpha,
                            double gamma, double beta, double wx, double wy, double ww, double wh, const double* normalizer,
                            const float* g_cls, const float* g_box, float* const* dlogits, const int* ld_dlogit,
                            float* const* ddeltas, const int* ld_ddelta, void* stream);

/* assign_boxes_to_levels + convert_boxes_to_pooler_format (detectron2/modeling/poolers.py:23-59, 69-96).
 * boxes [B,R,4] -> levels [B*R] int32 (offset from min_level), rois [B*R,5] (may be NULL). */
int lvc_assign_levels_rois(const float* boxes, int B, int R, int min_level, int max_level, int canonical_box_size,
                           int canonical_level, int* levels, float* rois, void* stream);

/* FastRCNNOutputs.predict_boxes / predict_probs + fast_rcnn_inference (lvc/modeling/roi_heads/fast_rcnn.py:95-137,
 * 440-468) + optional detector_postprocess (detectron2/modeling/postprocessing.py:10-79).
 *   cls_logits [B*R, ld_cls] (K+1 used), deltas [B*R, ld_delta] (4K, or 4 when cls_agnostic), proposals [B,R,4],
 *   d_prop_count [B] or NULL, d_image_sizes [B,2] (h,w), (wx,wy,ww,wh) = ROI_BOX_HEAD.BBOX_REG_WEIGHTS,
 *   d_post [B,4] = (scale_x, scale_y, out_h, out_w) or NULL.
 *   Outputs [B,topk,*] + d_out_count [B]; out_rows = index of the proposal each detection came from.
 *   max_candidates: capacity of the (roi,class) candidate list per image (pairs above score_thresh); R*K can never
 *   overflow; a smaller capacity that does overflow sets d_status bit 1 (value 2) and the host re-runs with R*K.
 */
long long lvc_fast_rcnn_inference_workspace_bytes(int B, int max_candidates);
int lvc_fast_rcnn_inference(const float* cls_logits, int ld_cls, const float* deltas, int ld_delta, int K,
                            int cls_agnostic, const float* proposals, const int* d_prop_count, int B, int R,
                            const int* d_image_sizes, float wx, float wy, float ww, float wh, float scale_clamp,
                            float score_thresh, double nms_thresh, int topk, int max_candidates,
                            const float* d_post, float* out_boxes, float* out_scores, int* out_classes,
                            int* out_rows, int* d_out_count, int* d_status, void* workspace,
                            long long workspace_bytes, void* stream);

/* One class-agnostic cascade stage of the box corrector: BoxOnlyLayersCascade.predict_boxes
 * (lvc/modeling/roi_heads/roi_heads_cascade.py:197-211) + the clip of _create_proposals_from_boxes
 * (cascade_rcnn.py:348-369).  deltas [M, ld] (4 used), boxes [M,4] = B images x R rows, d_image_sizes [B,2] or NULL. */
int lvc_decode_boxes(const float* deltas, int ld, const float* boxes, int M, int R, const int* d_image_sizes,
                     float wx, float wy, float ww, float wh, float scale_clamp, float* out, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Training-time kernels of the fine-tune step (BASELINE config 3; only the box predictor trains).
 * lvc_match_boxes: pairwise_iou (detectron2/structures/boxes.py:315-347) + Matcher (modeling/matcher.py:61-126)
 *   without materialising the G x N matrix.  gt [G,4] (1..512), boxes [N,4]; thresholds t0 (,t1), labels l0,l1(,l2);
 *   outputs matches [N] int64 (first arg-max), labels [N] int8, matched_vals [N]; d_gt_best [G] uint32 scratch.
 * lvc_fast_rcnn_losses: FastRCNNOutputs.losses (lvc/modeling/roi_heads/fast_rcnn.py:267-279, 296-359): mean softmax CE
 *   and smooth-L1(sum)/R, plus d(loss)/d(logits) [R,K+1] and d(loss)/d(deltas) [R,4K|4].  gt_classes int64, K = bg.
 *   One wave per row; the per-row terms are added in a fixed order from the fp64 scratch row_terms [2R].
 * lvc_rpn_losses: RPN.losses (proposal_generator/rpn.py:328-400) over S sampled anchors, forward only:
 *   out = (BCE-with-logits sum, smooth-L1 sum over positives) / normalizer.
 */
int lvc_match_boxes(const float* gt, int G, const float* boxes, int N, float t0, float t1, int nthr, int l0, int l1,
                    int l2, int allow_low_quality, long long* matches, signed char* labels, float* matched_vals,
                    unsigned int* d_gt_best, void* stream);
/* The label-and-sample steps of a training forward for the whole batch (round 5, csrc/train_targets.hip; RPN.label_and_sample_anchors,
 * detectron2/modeling/proposal_generator/rpn.py:269-325, and ROIHeads.label_and_sample_proposals, lvc/modeling/roi_heads/roi_heads.py:
 * 173-278, without their per-image loops and device->host reads).
 * lvc_match_boxes_batched: lvc_match_boxes for B images in two launches.  gt [Gtot,4] = the images' boxes one after the other, gt_off
 *   [B+1] int32 DEVICE prefix of the per-image counts (0..512 each; an image without gt gets label l0, match 0 everywhere);
 *   box_img_stride 0: boxes [N,4] shared (anchors), else [B][N][4] with nbox [B] rows in use (NULL: N; rows behind: label -1).
 * lvc_subsample_batched: subsample_labels (sampling.py:10-54) per row of labels int8 [B,N] (1 positive, 0 negative, else ignored): the
 *   min(#pos, cap_pos) positives and min(#neg, bs - num_pos) negatives with the smallest keys (int64 [B,N], distinct, < 2^nbits; or NULL:
 *   keys = a pseudo-random bijection of b N + i generated from `seed` by a 4-round Feistel network, nothing to sort or read) ->
 *   sel int32 [B,bs] (positives first, each group by increasing key, -1 padded), counts int32 [B,2].  bs <= 1024.
 * lvc_rpn_gather_sampled: for sel / counts over the R = sum_l H_l W_l A anchors: logits [B bs], deltas / anchors / matched gt boxes
 *   [B bs,4], labels int8 (1 / 0 / -1 padding) read from the head's per-level outputs fused[l] [B,H_l,W_l,ld_l] (channel a objectness,
 *   A + 4a + c delta c); grid anchors = shift + cell anchor (anchor_generator.py:161-185).  Feeds lvc_rpn_losses.
 * lvc_roi_build_table: add_ground_truth_to_proposals (proposal_utils.py:121-162) into a padded table boxes [B,Wt,4], logits [B,Wt],
 *   nrow [B]; lvc_roi_gather_sampled: its sampled rows with classes (gt class of the match / K for background and padding rows). */
int lvc_match_boxes_batched(const float* gt, const int* gt_off, int Gtot, int B, const float* boxes, long long box_img_stride,
                            const int* nbox, int N, float t0, float t1, int nthr, int l0, int l1, int l2, int allow_low_quality,
                            int* matches, signed char* labels, float* vals, unsigned int* gt_best, void* stream);
long long lvc_subsample_workspace_bytes(int B);   /* zeroed by the caller before the first use; the launches leave it zeroed */
int lvc_subsample_batched(const signed char* labels, const long long* keys /* NULL: generated from seed */, unsigned long long seed,
                          int B, int N, int nbits, int cap_pos, int bs, int* sel, int* counts, void* workspace, void* stream);
int lvc_rpn_gather_sampled(const void* const* fused, const int* ld, const void* const* cell_anchors, const int* H, const int* W,
                           const int* strides, int L, int A, int B, int bs, const int* sel, const int* counts, const int* matches,
                           const float* gt, const int* gt_off, float* logits, float* deltas, float* anchors, float* gt_boxes,
                           signed char* labels, void* stream);
int lvc_roi_build_table(const float* pboxes, const float* plogits, const int* pcount, int B, int P, const float* gt, const int* gt_off,
                        float gt_logit, int Wt, float* boxes, float* logits, int* nrow, void* stream);
int lvc_roi_gather_sampled(const float* boxes, const float* logits, const int* matches, const int* sel, const int* counts,
                           const long long* gt_classes, const int* gt_off, int B, int Wt, int bs, int K, float* s_boxes, float* s_logits,
                           long long* s_cls, long long* s_match, void* stream);
int lvc_fast_rcnn_losses(const float* logits, int ld_cls, const float* deltas, int ld_delta, int K, int cls_agnostic,
                         const float* proposals, const float* gt_boxes, const long long* gt_classes, int R, float wx,
                         float wy, float ww, float wh, float smooth_l1_beta, float* out_losses, float* dlogits,
                         float* ddeltas, double* row_terms /* [2R] scratch */, void* stream);
int lvc_rpn_losses(const float* logits, const float* deltas, const float* anchors, const float* gt_boxes,
                   const signed char* labels, int S, float smooth_l1_beta, float normalizer, float* out_losses,
                   void* stream);
/* lvc_rpn_losses plus the gradients the RPN head trains on (faster_rcnn_R_50_FPN_base.yaml, ft_all yaml):
 * dlogits [S] = (sigmoid(x) - label) / normalizer, ddeltas [S,4] = smooth-L1' / normalizer on positive rows, else 0. */
int lvc_rpn_losses_grad(const float* logits, const float* deltas, const float* anchors, const float* gt_boxes,
                        const signed char* labels, int S, float smooth_l1_beta, float normalizer, float* out_losses,
                        float* dlogits, float* ddeltas, void* stream);

/* Box-corrector training (BASELINE config 5; the shipped fine-tune yaml freezes the backbone).
 * lvc_giou_box_loss: BoxOnlyLayersCascade.box_reg_loss / BoxOnlyLayers.box_reg_loss
 *   (lvc/modeling/roi_heads/roi_heads_cascade.py:165-195): apply_deltas (box_regression.py:73-110, weights wx..wh,
 *   clamp) on the foreground rows (gt_classes in [0,K)) -> GIoU loss (fvcore.nn.giou_loss, eps 1e-7) -> mean; with
 *   iterate != 0: mean(max(loss_after - lambda * loss_before, 0)).  out_loss [1] (NaN when no row is foreground, as the
 *   reference's mean of an empty tensor), ddeltas [R,4] = d(loss)/d(deltas).
 * lvc_relu_backward: out = y > 0 ? dy : 0 (backward of the fused Linear+ReLU of FastRCNNConvFCHead, box_head.py:82-91).
 * lvc_colsum: out[n] = sum_m x[m*ldx + n], rows added in order (bias gradients). */
int lvc_giou_box_loss(const float* deltas, int ld_delta, const float* proposals, const float* gt_boxes,
                      const long long* gt_classes, int R, int K, float wx, float wy, float ww, float wh,
                      float scale_clamp, int iterate, float lambda, float* out_loss, float* ddeltas, void* stream);
int lvc_relu_backward(const float* dy, const float* y, long long n, float* out, void* stream);
int lvc_colsum(const float* x, int M, int N, int ldx, float* out, void* stream);

/* Backward into the trunk (BASELINE config 5 with `cascade_ubbr_R_50_FPN_base.yaml`: `BACKBONE.FREEZE_AT 2`, and the
 * base / ft_all detector yamls): the reference trains through ATen's conv2d backward for BottleneckBlock
 * (detectron2/modeling/backbone/resnet.py:195-211), FPN (backbone/fpn.py:109-144) and StandardRPNHead
 * (proposal_generator/rpn.py:120-139).
 * lvc_conv_wgrad_nhwc: dw[k][r][s][c] = scale[k] * sum_{n,oy,ox} dy[n,oy,ox,k] * x[n, oy*stride+r-pad, ox*stride+s-pad, c]
 *   (x zero outside the map).  x [N,H,W,C], dy [N,Ho,Wo,*] with row pitch lddy floats, scale [K] or NULL (the
 *   FrozenBatchNorm2d scale that follows the conv, batch_norm.py:45-65), dw [K,R,S,C] zeroed by the call.  Exact fp32
 *   MFMA; partial sums over pixel ranges are combined with fp32 atomics (not run-to-run deterministic).
 *   The data gradient needs no entry point of its own: it is lvc_conv2d_nhwc_* / lvc_conv3x3_nhwc_bf16x3 on dy with the
 *   weights flipped and transposed (host: kernels.pack_conv_dgrad), followed for a stride-2 1x1 by lvc_scatter_stride2_nhwc
 *   (a stride-2 3x3 / pad 1: dy is zero-stuffed onto the input grid by lvc_scatter_stride2_nhwc first, then the stride-1 product).
 * lvc_scatter_stride2_nhwc: y[n,2i,2j,:] = x[n,i,j,:], 0 elsewhere; x [N,(H-1)/2+1,(W-1)/2+1,C] -> y [N,H,W,C]
 *   (input gradient of a stride-2 1x1 conv and of LastLevelMaxPool, fpn.py:165-177).
 * lvc_downsum2x2_nhwc: y[n,i,j,:] = sum of x[n,2i..2i+1,2j..2j+1,:]; x [N,2Hs,2Ws,C] (backward of the nearest x2
 *   upsample of the FPN top-down path, fpn.py:131-133).
 * lvc_colsum_atomic: lvc_colsum for 10^5-row operands (conv bias gradients): row slabs combined with fp32 atomics. */
/* Device-side packing of the reference's OIHW parameters (detectron2/layers/wrappers.py:41-99 keeps `weight` as
 * [K,C,R,S]) into the conv kernels' operand: wp [rows_pad][R*S*cin_pad] fp32, k = (c/32, r, s, c%32).
 *   mode 0 (forward): rows = K output channels, cin = C.   mode 1 (data gradient): rows = C, contraction over the K
 *   output channels, taps flipped, times scale[k] (FrozenBatchNorm2d scale or NULL).  Padding rows/channels are zero.
 * lvc_split_weights: planes == 3 -> out = 3 x n bf16 (hi, mid, lo), planes == 2 -> 2 x n fp16 (w1, (w - w1) * 2048);
 *   |w| > 65504 in the fp16 split raises bit 1 of *err_word (the conv error word of lvc_conv_workspace). */
int lvc_pack_conv_weights(const float* w, const float* scale, float* wp, int K, int C, int R, int S, int rows_pad,
                          int cin_pad, int mode, void* stream);
int lvc_split_weights(const float* wp, long long n, int planes, void* out, int* err_word, void* stream);
/* lvc_pack_conv_weights and lvc_split_weights in one launch: planes_out [planes][rows_pad][R*S*cin_pad], planes = 2
 * (fp16) or 3 (bf16); err_word as lvc_split_weights. */
int lvc_pack_split_conv_weights(const float* w, const float* scale, float* wp, void* planes_out, int planes, int* err_word,
                                int K, int C, int R, int S, int rows_pad, int cin_pad, int mode, void* stream);
/* lvc_pack_split_conv_weights (+ lvc_split_weights_rowscaled) for `njobs` layers in one launch per 24 jobs (round 5: an optimizer
 * step invalidates the packed operands of every trainable layer -- the reference has no such step, ATen reads OIHW directly).
 * ptrs: host array, 6 device pointers per job = w (OIHW), scale (mode 1: folded into the operand, or NULL), fac_scale (fmt 4:
 * multiplied into the row factors, or NULL), wp ([rows_pad][R*S*cin_pad] fp32), planes, fac ([rows_pad] fp32, fmt 4);
 * shapes: 8 ints per job = K, C, R, S, rows_pad, cin_pad, mode (as lvc_pack_conv_weights), fmt -- 0: wp only, 2: fp16 planes
 * (lvc_split_weights), 3: bf16 planes, 4: row-scaled fp16 planes + fac[row] = 2^-e / 16 (* fac_scale[row]) (lvc_split_weights_rowscaled). */
int lvc_pack_group(int njobs, const void* const* ptrs, const int* shapes, int* err_word, void* stream);
int lvc_conv_wgrad_nhwc(const float* x, const float* dy, const float* scale, float* dw, int N, int H, int W, int C,
                        int K, int R, int S, int stride, int pad, int lddy, void* stream);
/* lvc_conv_wgrad_nhwc on the three-way bf16 split MFMA path (six bf16 MFMAs per fp32-accurate product, one fp32
 * accumulator; gfx950 LDS transpose reads for the pixel-major operands).  No range restriction: the default. */
int lvc_conv_wgrad_nhwc_bf16x3(const float* x, const float* dy, const float* scale, float* dw, int N, int H, int W, int C,
                               int K, int R, int S, int stride, int pad, int lddy, void* stream);
/* lvc_conv_wgrad_nhwc on the two-way fp16 split MFMA path (gfx950 LDS transpose reads for the pixel-major operands).
 * dy and x must lie inside fp16's range -- gradients scaled by a power of two (lvc_amd.solver.LossScaler); a value beyond
 * 65504 raises bit 1 (value 2) of *err_word (the conv error word of lvc_conv_workspace; may be NULL).  A layer with fewer than 16
 * output pixels (less than one k-step of the fp16 MFMA) runs on lvc_conv_wgrad_nhwc instead: exact products, no range restriction. */
int lvc_conv_wgrad_nhwc_f16x2(const float* x, const float* dy, const float* scale, float* dw, int N, int H, int W, int C,
                              int K, int R, int S, int stride, int pad, int lddy, int* err_word, void* stream);
/* The weight gradients of `njobs` layers in one launch of the bf16x3 kernel (round 5): ATen's conv2d backward runs one wgrad per
 * layer (resnet.py:195-211, fpn.py:109-144 under autograd); at 2 images per GPU (cascade_ubbr_R_101_FPN_base.yaml) a res4 layer's
 * 16-36 tiles cannot fill the chip, and the weight gradient is off the backward's critical path, so the host queues the (x, dy)
 * pairs (lvc_amd.kernels.defer_wgrad) and launches them together.  x / dy / scale / dw: host arrays of njobs device pointers
 * (scale[j] may be NULL); shapes: host array, 10 ints per job = N, H, W, C, K, R, S, stride, pad, lddy (as lvc_conv_wgrad_nhwc).
 * dw[j] ([K][R][S][C]) must be ZERO on entry: partial sums over pixel slices are added with fp32 atomics. */
int lvc_conv_wgrad_group_bf16x3(int njobs, const float* const* x, const float* const* dy, const float* const* scale,
                                float* const* dw, const int* shapes, void* stream);
/* dst[j] (the parameter's OIHW layout [K][C][R*S]) = (beta ? dst[j] : 0) + src[j] ([K][R*S][C], what the wgrad kernels write), all
 * jobs in one launch; shapes: 4 ints per job = K, C, R*S, beta.  (AccumulateGrad's `grad += dw` / first assignment.) */
int lvc_wgrad_finalize_group(int njobs, const float* const* src, float* const* dst, const int* shapes, void* stream);
int lvc_scatter_stride2_nhwc(const float* x, float* y, int N, int H, int W, int C, void* stream);
/* Grouped 3x3 convolution of a ResNeXt bottleneck (reference detectron2/modeling/backbone/resnet.py BottleneckBlock with
 * num_groups > 1), csrc/conv_grouped.hip: NHWC fp32, pad 1, stride 1 or 2, `groups` groups of cg = C / groups input AND output
 * channels (C == K), cg in {4, 8, 16, 32, 64}, C a multiple of 64; any other shape returns LVC_ERR_INVALID.  Exact fp32 MFMA
 * (range-free: no range word is raised).
 * lvc_conv3x3_grouped_nhwc: y = act(conv(x) * scale + shift (+ residual)); the argument order of the dense entry points, wp from
 *   lvc_pack_conv3x3_grouped; res_mode 0 or 1 (a residual of the output's shape).  With a mode-1 operand it is the data
 *   gradient of a stride-1 layer; a stride-2 layer's gradient is zero-stuffed first (lvc_scatter_stride2_nhwc), then the same call.
 * lvc_pack_conv3x3_grouped: w [K][cg][3][3] (the reference's state_dict layout) -> wp, lvc_conv3x3_grouped_packed_floats(K,
 *   groups) floats.  mode 0: forward; mode 1: data gradient (taps flipped, per-group transpose, times scale[k] or 1).
 * lvc_conv3x3_grouped_wgrad_nhwc: dw [K][cg][3][3] = scale[k] * sum dy[n,oy,ox,k] * x[n, oy*stride+r-1, ox*stride+s-1, c] from x
 *   [N,H,W,C] and dy [N,Ho,Wo,*] (row pitch lddy); scratch: lvc_conv3x3_grouped_wgrad_workspace_bytes(...) bytes.  Partial sums
 *   over pixel chunks are added in chunk order (no atomics): two runs are bit-identical. */
int lvc_conv3x3_grouped_nhwc(const float* x, const float* wp, const float* scale, const float* shift, const float* residual,
                             float* y, int N, int H, int W, int C, int K, int groups, int stride, int relu, int res_mode, int ldy,
                             int ldr, void* workspace, void* stream);
long long lvc_conv3x3_grouped_packed_floats(int K, int groups);
int lvc_pack_conv3x3_grouped(const float* w, const float* scale, float* wp, int K, int groups, int mode, void* stream);
long long lvc_conv3x3_grouped_wgrad_workspace_bytes(int N, int H, int W, int K, int groups, int stride);
int lvc_conv3x3_grouped_wgrad_nhwc(const float* x, const float* dy, const float* scale, float* dw, int N, int H, int W, int C,
                                   int groups, int stride, int lddy, void* scratch, void* stream);
/* y[n, i, j, 0..C) = x[n, 2i, 2j, :], rows of ldy floats in y (0 = C): the sampling of a stride-2 1x1 convolution as a copy (the
 * block input of res3.0 / res4.0 / res5.0 next to conv2's output: conv3 + projection shortcut as one GEMM, resnet.py:117-160). */
int lvc_subsample2_nhwc(const float* x, float* y, int N, int H, int W, int C, int ldy, void* stream);
int lvc_downsum2x2_nhwc(const float* x, float* y, int N, int Hs, int Ws, int C, void* stream);
/* nn.AvgPool2d(2) of the ResNet-D trunk (RESNETS.D: the pools of a BottleneckBlockCLIP, reference resnet.py:359, :399), csrc/avgpool.hip,
 * NHWC fp32, C % 4 == 0, H >= 2, W >= 2, 16-byte aligned pointers; anything else returns LVC_ERR_INVALID.
 * lvc_avgpool2_nhwc: y[n, i, j, 0..C) = (((x[2i,2j] + x[2i,2j+1]) + x[2i+1,2j]) + x[2i+1,2j+1]) * 0.25f in exactly that order, no
 *   contraction; [N, H/2, W/2] outputs (floor: an odd last row / column is dropped); rows of ldo floats in y (0 = C; ldo % 4 == 0):
 *   y may point at a channel slice of a wider buffer, whose other channels are not touched.
 * lvc_avgpool2_bwd_nhwc: dx [N,H,W,C] = 0.25f * dy[n, h/2, w/2, :], zeros in a dropped odd row / column; dy [N,H/2,W/2,*] with rows of
 *   ldi floats (0 = C). */
int lvc_avgpool2_nhwc(const float* x, float* y, int N, int H, int W, int C, int ldo, void* stream);
int lvc_avgpool2_bwd_nhwc(const float* dy, float* dx, int N, int H, int W, int C, int ldi, void* stream);
int lvc_colsum_atomic(const float* x, int M, int N, int ldx, float* out, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Label-verification kNN (tools/run_nearest_neighbours.py:142-162, 214-227).
 * lvc_colmean: mu[d] = mean_m x[m,d], summed in a fixed order (run-to-run deterministic).  lvc_knn_topk_vote: per query row, class ids of the 10 most similar
 * shots (ties -> lower shot index) and keep = (mode of the first kvote ids, ties -> smallest id, == detector class).
 *   sims [Q,ld] fp32 (S columns used, S <= 4096), shot_classes [S] int64, det_classes [Q] int64 or NULL,
 *   top_classes [Q,10] int64, keep [Q] int64 or NULL.
 */
int lvc_colmean(const float* x, float* mu, int M, int D, int ld, void* stream);
/* Shot sets of any size (tools/run_nearest_neighbours.py:146-160 ranks any S): lvc_knn_topk_candidates writes, for ONE block of
 * S <= 4096 columns of sims [Q,ld], the ten best (similarity, idx_base + column) pairs per row (cand_val / cand_idx [Q,10];
 * value descending, ties -> lower index, padded with (-inf, INT_MAX)); lvc_knn_merge_vote ranks nlists <= 64 such lists
 * ([nlists][Q][10]) against each other, gathers the classes and votes: outputs as lvc_knn_topk_vote.
 * lvc_max_f32: out[0] = max of x[0..n). */
int lvc_knn_topk_candidates(const float* sims, int ld, int Q, int S, int idx_base, float* cand_val, int* cand_idx, void* stream);
int lvc_knn_merge_vote(const float* cand_val, const int* cand_idx, int nlists, int Q, const long long* shot_classes,
                       const long long* det_classes, int kvote, long long* top_classes, long long* keep, void* stream);
int lvc_max_f32(const float* x, long long n, float* out, void* stream);
int lvc_knn_topk_vote(const float* sims, int ld, int Q, int S, const long long* shot_classes,
                      const long long* det_classes, int kvote, long long* top_classes, long long* keep,
                      void* stream);
/* Two-stage form of the same sweep (cosine branch; the similarities of run_nearest_neighbours.py:146-151 are never
 * materialised in full precision).
 * lvc_rownorm_h: lvc_rownorm that writes the rows rounded to fp16 (yh [M,D]), the denominators (den [M] or NULL), the
 *   2-norm of each row's rounding residual row - fp16(row) (resid [M] or NULL) and, if y is not NULL, the fp32 rows
 *   (contiguous, bit-identical to lvc_rownorm).
 * lvc_gemm_f16: y [M,ldy] fp32 = a [M,C] . b [N,ldb]^T on fp16 operands (csrc/gemm_h.hip; C % 32 == 0, ldb = elements
 *   between rows of b, 0 = C; y below 2 GiB) -- for unit-norm rows |y - exact| < 2^-10.
 * lvc_knn_verify_topk_vote: per query row, the shots whose approximate similarity is within `margin` (>= 2 x that bound)
 *   of the 10th largest approximate value provably contain the exact ten best; those of them that have a shot of another
 *   class within margin are re-evaluated in fp32 from q [Q,ldq] (raw descriptors; (q - mu) / den[row] is redone exactly as
 *   lvc_rownorm_h did it; mu / den may be NULL: q then already holds the rows) and sn [S,D] (normalised shots), and the
 *   candidates are ranked so that the class sequence equals the exact ranking's (ties -> lower shot index; csrc/knn.hip
 *   states the argument).  margins [Q] (or NULL): a margin per row that replaces `margin` -- 2 x the row's own error bound
 *   |resid_q| max|s_h| + |q| max resid_s + D 2^-24 (Cauchy-Schwarz on the two rounding residuals + fp32 accumulation), about
 *   half the worst case.  D % 4 == 0, D <= 2048.  Outputs as lvc_knn_topk_vote. */
int lvc_rownorm_h(const float* x, const float* mu, float* y, unsigned short* yh, float* den, float* resid, int M, int D, int ldx,
                  float eps, int mode, void* stream);
int lvc_gemm_f16(const unsigned short* a, const unsigned short* b, int ldb, float* y, int M, int N, int C, int ldy,
                 void* stream);
int lvc_knn_verify_topk_vote(const float* approx, int ld, int Q, int S, const float* q, int ldq, const float* mu,
                             const float* den, const float* sn, int D, float margin, const float* margins,
                             const long long* shot_classes, const long long* det_classes, int kvote, long long* top_classes,
                             long long* keep, void* stream);
/* 16-bit fixed-point form of the two-stage sweep's similarity matrix (tools/run_nearest_neighbours.py:146-151 keeps it in fp32; here
 * it only pre-filters): lvc_gemm_f16_q15 writes y[m][n] = rint(32766 * dot) clamped to +-32766 as int16 (NaN -> 32767; ldy even), and
 * lvc_knn_verify_topk_vote_q15 reads it (ld % 8 == 0, rows 16-byte aligned) -- half the bytes of the matrix round trip; the margin
 * handed in must include 2 x 1.6e-5 for the quantisation. */
/* The sweep's per-row margins in one launch: margins[i] = 2 (1 + 1e-4) (qres[i] (1 + 1e-6 + *d_sres_max) + *d_sres_max (1 + 1e-5) + acc) + extra
 * (qres: the queries' rounding-residual norms from lvc_rownorm_h, d_sres_max: device scalar = lvc_max_f32 over the shots' residual
 * norms, acc: the accumulation term, extra: the 16-bit matrix's quantisation margin or 0). */
int lvc_knn_margins(const float* qres, const float* d_sres_max, float acc, float extra, int Q, float* margins, void* stream);
int lvc_gemm_f16_q15(const unsigned short* a, const unsigned short* b, int ldb, short* y, int M, int N, int C, int ldy, void* stream);
int lvc_knn_verify_topk_vote_q15(const short* approx, int ld, int Q, int S, const float* q, int ldq, const float* mu,
                             const float* den, const float* sn, int D, float margin, const float* margins,
                             const long long* shot_classes, const long long* det_classes, int kvote, long long* top_classes,
                             long long* keep, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Descriptor network of the label-verification step: DINO ViT-S/8 as loaded by
 * tools/run_nearest_neighbours.py:292-293 (torch.hub 'facebookresearch/dino', a third-party model: published
 * architecture, restated for the tests in oracle/vit.py).  The linear layers run on the conv/GEMM entry points
 * above; these are the remaining pieces.  All tensors fp32, row-major.
 *   lvc_vit_patchify : img [B,C,H,W] -> [B*(H/ps)*(W/ps), C*ps*ps], column = c*ps*ps + r*ps + s (so that the ps x ps
 *                      stride-ps convolution of patch_embed is one GEMM with proj.weight.reshape(D, C*ps*ps))
 *   lvc_vit_tokens   : out[b][0] = cls + pos[0], out[b][1+p] = emb[b*P+p] + pos[1+p]   (out [B*(P+1), D], D % 4 == 0)
 *   lvc_layernorm    : torch.nn.LayerNorm over rows of D <= 2048 elements (biased variance, eps inside the sqrt)
 *   lvc_gelu         : torch.nn.GELU() exact (erf) form, n % 4 == 0
 *   lvc_mha          : qkv [B*N, 3*H*64] (column = which*H*64 + h*64 + d) -> out [B*N, H*64] =
 *                      softmax(q k^T * scale) v per (image, head); head_dim must be 64 (one thread per query, fp32 VALU)
 *   lvc_mha_mfma     : the same result on the matrix cores (csrc/vit.hip: both products as fp32-accurate two-way fp16 splits, the
 *                      probabilities stay in registers between them); workspace = lvc_mha_workspace_bytes(B, N, H) bytes,
 *                      16-byte aligned (fp16 operand planes of q, k, v); d_error_word (may be NULL): device int whose bit 1 is
 *                      set when q * scale * log2(e), k or v leaves fp16's range (|x| > 65504) or is NaN -- the result is
 *                      then invalid and the caller falls back to lvc_mha */
int lvc_vit_patchify(const float* img, float* out, int B, int C, int H, int W, int ps, void* stream);
/* lvc_vit_patchify of (img - mean[c]) / std[c] (tools/run_nearest_neighbours.py:95-99 preprocess_crops fused into the gather);
 * mean / std: HOST arrays of C <= 8 floats. */
int lvc_vit_patchify_norm(const float* img, const float* mean, const float* std, float* out, int B, int C, int H, int W, int ps,
                          void* stream);
int lvc_vit_tokens(const float* emb, const float* cls, const float* pos, float* out, int B, int P, int D, void* stream);
int lvc_layernorm(const float* x, int ldx, const float* w, const float* b, float* y, int ldy, int M, int D, float eps,
                  void* stream);
int lvc_gelu(const float* x, float* y, long long n, void* stream);
int lvc_mha(const float* qkv, float* out, int B, int N, int H, int head_dim, float scale, void* stream);
/* The attention output of token 0 (the class token) of every image only: qkv [B*N, 3*H*64] -> out [B, H*64] (N <= 1024).  The last block
 * of the descriptor network: its output is read at the class rows (tools/run_nearest_neighbours.py:102-128). */
int lvc_mha_cls(const float* qkv, float* out, int B, int N, int H, float scale, void* stream);
long long lvc_mha_workspace_bytes(int B, int N, int H);
int lvc_mha_mfma(const float* qkv, float* out, void* workspace, int B, int N, int H, float scale, int* d_error_word, void* stream);
/* The qkv layer of a ViT block written straight into lvc_mha_mfma's operand planes (round 5; the DINO ViT's `attention.qkv` + the first
 * pass of the attention, tools/run_nearest_neighbours.py:102-128): lvc_conv1x1_nhwc_f16s1 on x [B*N][C] (w_split / scale / shift as there,
 * K = 3 * H * 64 columns = (q | k | v, head, d)); planes [6][B*H][Npad][64] fp16 (lvc_mha_workspace_bytes), q multiplied by softmax_scale *
 * log2(e) (as lvc_mha_mfma does); rows N..Npad-1 are not written (the caller keeps them zero).  Bit-identical to the two launches it replaces.
 * An operand beyond fp16's range raises bit 1 (value 2) of *err_word.  lvc_mha_mfma_planes: the attention on such planes. */
int lvc_conv1x1_qkv_planes_f16s1(const float* x, const unsigned short* w_split, const float* scale, const float* shift, void* planes,
                                 int B, int N, int C, int H, float softmax_scale, int* err_word, void* workspace, void* stream);
int lvc_mha_mfma_planes(const void* planes, float* out, int B, int N, int H, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * GroupNorm on NHWC fp32 maps (csrc/group_norm.hip; reference detectron2/layers/batch_norm.py:127-150, NORM "GN" =
 * nn.GroupNorm(32, C) after the FPN convs and the convs of FastRCNNConvFCHead).
 * lvc_group_norm_fwd_nhwc: y = act(((x - mean) * rstd) * gamma + beta) (+ residual), mean / rstd [N,G] per (sample, group) over
 *   H * W * C/G values (biased variance, eps inside the sqrt), written for the backward.  x, y [N,H,W,C]; x_sn..x_sc: the element
 *   strides of x, which must be those of a contiguous tensor (anything else is an error); C % G == 0 (16-byte accesses where C/G is a
 *   multiple of 4 and the pointers are 16-byte aligned, scalar ones otherwise).  relu: 0 | 1.  res_mode 0: none; 1: residual
 *   [N,H,W,C]; 2: residual [N,(H+1)/2,(W+1)/2,C], nearest-x2-upsampled (pixel (h,w) adds residual (h/2,w/2): the conv epilogue's
 *   res_mode 2, odd sizes included).  relu with a residual is an error.
 *   tile_rows 0: one workgroup owns whole samples (x held in LDS when a sample fits 64 KB); > 0: statistics over tiles of
 *   tile_rows image rows, partials in `workspace`, combined in tile order in the prologue of the second launch.
 *   No float atomics anywhere: repeated calls are bit-identical.
 * lvc_group_norm_bwd_nhwc: dx [N,H,W,C], dgamma [C], dbeta [C] from dy and the forward's x / mean / rstd; relu 1 rebuilds the
 *   mask from x, gamma, beta (beta may be NULL when relu == 0).  The gradient of a residual is dy itself (res_mode 1) or its 2x2
 *   down-sum (res_mode 2, lvc_downsum2x2_nhwc) and is not computed here.  Same two regimes; per-channel partial sums go through
 *   workspace slabs added in a fixed order.
 * lvc_upsample2_add_grad_nhwc: the res_mode-2 residual's gradient at ANY fine size: dres [N,(H+1)/2,(W+1)/2,C], dres[n,i,j,:] = sum of
 *   g[n,2i..2i+1,2j..2j+1,:] inside the map (g [N,H,W,C] contiguous; an even H and W gives lvc_downsum2x2_nhwc's values).
 * lvc_group_norm_workspace_bytes: bytes of `workspace` for one call (backward != 0: of the backward); 0 = none needed. */
long long lvc_group_norm_workspace_bytes(int N, int H, int W, int C, int G, int tile_rows, int backward);
int lvc_group_norm_fwd_nhwc(const float* x, const float* gamma, const float* beta, const float* residual, float* y, float* mean,
                            float* rstd, int N, int H, int W, int C, int G, long long x_sn, long long x_sh, long long x_sw,
                            long long x_sc, float eps, int relu, int res_mode, int tile_rows, void* workspace,
                            long long workspace_bytes, void* stream);
int lvc_upsample2_add_grad_nhwc(const float* g, float* dres, int N, int H, int W, int C, void* stream);
int lvc_group_norm_bwd_nhwc(const float* dy, const float* x, const float* mean, const float* rstd, const float* gamma,
                            const float* beta, float* dx, float* dgamma, float* dbeta, int N, int H, int W, int C, int G,
                            long long x_sn, long long x_sh, long long x_sw, long long x_sc, int relu, int tile_rows,
                            void* workspace, long long workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Mask R-CNN inference: the mask head's tail and the paste of the predicted masks into the image.
 * lvc_mask_deconv_predict (csrc/mask_deconv.hip): ConvTranspose2d(Cin, Cmid, 2, stride 2) + bias -> ReLU -> Conv2d(Cmid, K, 1) + bias ->
 *   the plane of ONE class per RoI -> sigmoid, one launch (detectron2/modeling/roi_heads/mask_head.py `layers` + mask_rcnn_inference):
 *     prob[m, 2y+dy, 2x+dx] = sigmoid(b_pred[c] + sum_co relu(b_deconv[co] + sum_ci x[m,y,x,ci] * Wd[ci,co,dy,dx]) * w_pred[c,co])
 *   x [M,S,S,Cin] NHWC fp32; w_deconv [4*Cmid, Cin], row (dy*2+dx)*Cmid + co (from the parameter [Cin,Cmid,2,2]); w_pred [K,Cmid];
 *   b_deconv [Cmid], b_pred [K] (NULL = zeros); classes [M] int32, c = classes[m] (NULL: class 0 for every row, CLS_AGNOSTIC_MASK);
 *   d_num_valid (device int, may be NULL): rows >= *d_num_valid are neither read nor written; prob [M,2S,2S].
 *   Cin, Cmid multiples of 64 up to 256, K >= 1, S >= 1, any M; anything else returns LVC_ERR_INVALID.  Exact fp32 MFMA (range-free).
 *   A class outside [0, K) sets bit 3 (value 8) of *d_status and is computed as class 0.  No float atomics: two runs are bit-identical.
 * lvc_paste_masks (csrc/mask_paste.hip): detectron2/layers/mask_ops.py paste_masks_in_image for a batch in one launch.  A job = 8 int64
 *   words: row of prob [num_rows, mask_size, mask_size]; x0, y0, x1, y1 (fp32 bit patterns, output coordinates); out_h; out_w; byte
 *   offset of the job's [out_h, out_w] uint8 plane in `out`.  h_jobs [host] is checked (row and plane inside their buffers, finite
 *   boxes of positive width and height: the non-empty filter runs before the paste), d_jobs is its device copy, read by the kernel.
 *   out: 16-byte aligned, out_bytes a multiple of 16; every byte of every job's plane is written (value >= threshold ? 1 : 0), bytes
 *   outside the planes are not touched.  threshold >= 0 (0 sets every pixel, as in the reference; its threshold < 0 visualisation
 *   branch is not built). */
int lvc_mask_deconv_predict(const float* x, const float* w_deconv, const float* b_deconv, const float* w_pred, const float* b_pred,
                            const int* classes, const int* d_num_valid, float* prob, int M, int S, int Cin, int Cmid, int K,
                            int* d_status, void* stream);
int lvc_paste_masks(const float* prob, int num_rows, int mask_size, const long long* h_jobs, const long long* d_jobs, int num_jobs,
                    unsigned char* out, long long out_bytes, float threshold, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Mask R-CNN training: mask targets, the tail's logits, the mask loss and the tail's backward (detectron2 mask_head.py mask_rcnn_loss,
 * structures/masks.py BitMasks.crop_and_resize).
 * lvc_mask_targets (csrc/mask_targets.hip, no contraction): ROIAlign((T,T), 1.0, 0, aligned=True) of each row's matched 0/1 plane, then
 *   >= 0.5, for the rows [0, count[b * count_stride]) of every image of boxes [B,R,4], one launch.  matched int64 [B,R]: index of the
 *   row's plane among its image's; table: 4 int64 words per image (plane base pointer, number of planes, H, W; planes are bytes,
 *   [n,H,W] contiguous), h_table on the host (checked), d_table its device copy.  out uint8 [B*R,T,T]; rows past the count are not
 *   written; a row whose index is outside [0, n) gets an empty target.  fp32 in the order of ROIAlign_cpu.cpp.
 * lvc_mask_deconv_logits (csrc/mask_deconv.hip): lvc_mask_deconv_predict without the sigmoid (classes: the GROUND-TRUTH class of each
 *   RoI): logits [M,2S,2S]; num_valid, status bit 8 and classes = NULL as there.
 * lvc_mask_loss (csrc/mask_train.hip, two launches): over the rows < *d_num_valid, out_loss = mean of
 *   max(z,0) - z t + log1p(exp(-|z|)) (terms and sum in fp64; 0 when there is no row), out_sum (may be NULL) the fp64 sum, out_counts
 *   (may be NULL) int64 [3] = pixels with (z > 0) != t, pixels with t, pixels with z > 0 and not t.  Partial sums per workgroup, added
 *   in index order by one workgroup: bit-identical between runs.
 * lvc_mask_deconv_grad (csrc/mask_train.hip, three launches): with dz = (sigmoid(z) - t) * *d_upstream / (*d_num_valid (2S)^2) and the
 *   hidden tile recomputed on fp32 MFMA, writes dh [M*S*S, 4*Cmid] = dz w_pred[c,co] [h > 0] (column (dy*2+dx)*Cmid + co: the gradient of
 *   the GEMM x [M*S*S,Cin] x w_deconv^T; the rows of x past num_valid are not read, their dh rows are zero), dw_pred [K,Cmid], db_pred [K] (rows of classes absent from the batch exactly 0) and db_deconv [Cmid].
 *   Per-(RoI, 64-pixel tile) partials in `workspace`, added in a fixed order: no float atomics, bit-identical between runs.
 * lvc_mask_deconv_wgrad (csrc/mask_train.hip, two launches): dw_packed [4*Cmid,Cin] = dh^T x over the rows below *d_num_valid (S*S each; the rows past it are not read) on fp32 MFMA; the rows
 *   are cut into slices fixed by M and S, each slice's partial tile goes to `workspace`, the slices are added in index order:
 *   bit-identical between runs (the conv weight-gradient kernels join their slices with atomics). */
int lvc_mask_targets(const float* boxes, const long long* matched, const int* count, int count_stride, const long long* h_table,
                     const long long* d_table, int B, int R, int T, unsigned char* out, void* stream);
int lvc_mask_deconv_logits(const float* x, const float* w_deconv, const float* b_deconv, const float* w_pred, const float* b_pred,
                           const int* classes, const int* d_num_valid, float* logits, int M, int S, int Cin, int Cmid, int K,
                           int* d_status, void* stream);
long long lvc_mask_loss_workspace_bytes(int M, int S);
int lvc_mask_loss(const float* logits, const unsigned char* targets, const int* d_num_valid, int M, int S, float* out_loss,
                  double* out_sum, long long* out_counts, void* workspace, long long workspace_bytes, void* stream);
long long lvc_mask_deconv_grad_workspace_bytes(int M, int S, int Cmid);
long long lvc_mask_deconv_wgrad_workspace_bytes(int M, int S, int Cin, int Cmid);
int lvc_mask_deconv_wgrad(const float* dh, const float* x, const int* d_num_valid, float* dw_packed, int M, int S, int Cin, int Cmid,
                          void* workspace, long long workspace_bytes, void* stream);
int lvc_mask_deconv_grad(const float* x, const float* w_deconv, const float* b_deconv, const float* w_pred, const int* classes,
                         const float* logits, const unsigned char* targets, const int* d_num_valid, const float* d_upstream, float* dh,
                         float* dw_pred, float* db_pred, float* db_deconv, int M, int S, int Cin, int Cmid, int K,
                         int* d_status, void* workspace, long long workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Keypoint R-CNN inference: the keypoint head's transposed convolution and the heatmap decode (detectron2
 * modeling/roi_heads/keypoint_head.py KRCNNConvDeconvUpsampleHead.layers, structures/keypoints.py heatmaps_to_keypoints).
 * lvc_keypoint_deconv (csrc/keypoint.hip): ConvTranspose2d(Cin, K, 4, stride 2, padding 1) + bias.  x [M,S,S,Cin] NHWC fp32; packed:
 *   the operand lvc_keypoint_deconv_pack writes from the parameter [Cin,K,4,4] -- lvc_keypoint_deconv_packed_rows(K) rows of Cin
 *   floats ([4 parities][4 taps][K rounded up to 32][Cin]); bias [K] (NULL = zeros); out: planes [M,K,2S,2S].  Cin a multiple of 16
 *   (up to 4096), 1 <= K <= 64, any M; anything else returns LVC_ERR_INVALID.  d_num_valid (device int, may be NULL): rows
 *   >= *d_num_valid are neither read nor written.  Exact fp32 MFMA (range-free) in short chains that are joined, with the bias, in
 *   fp64 and rounded once; an output is summed by one lane in a fixed order,
 *   no atomics: two runs are bit-identical.
 * lvc_heatmaps_to_keypoints (csrc/keypoint_decode.hip, no contraction): maps: planes [M,K,P,P]; rois [M,4] (x1, y1, x2, y2); up 1 or
 *   2, up * P <= 64.  With up == 2 the bilinear x2 map (align_corners=False, source index max(0, (dst + 0.5) / 2 - 0.5)) is formed on
 *   chip first.  maps_out (may be NULL): [M,K,up*P,up*P], the map that is decoded.  Per (RoI, keypoint): ATen's bicubic resize
 *   (A = -0.75, align_corners=False) of the map to ceil(max(y2 - y1, 1)) x ceil(max(x2 - x1, 1)), its maximum and the position of the
 *   maximum -- among equal maxima the LOWEST flat index y * w + x wins, as torch.argmax on the CPU --, score = exp(v - max) /
 *   sum over the [up*P, up*P] map of exp(map - max), x = (x_int + 0.5) * (w / ceil w) + x1 and y likewise in fp32 without
 *   contraction.  out [M,K,4] = (x, y, logit, score).  Rows >= *d_num_valid keep their bytes (out and maps_out).  No atomics: two
 *   runs are bit-identical.  A box side is cut at 16384 output pixels. */
int lvc_keypoint_deconv_packed_rows(int K);
int lvc_keypoint_deconv_pack(const float* weight, float* packed, int Cin, int K, void* stream);
int lvc_keypoint_deconv(const float* x, const float* packed, const float* bias, const int* d_num_valid, float* out, int M, int S,
                        int Cin, int K, void* stream);
int lvc_heatmaps_to_keypoints(const float* maps, const float* rois, const int* d_num_valid, float* maps_out, float* out, int M, int K,
                              int P, int up, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Keypoint R-CNN training: heatmap targets, the loss, and the backward of the head's transposed convolution (detectron2
 * structures/keypoints.py _keypoints_to_heatmap, modeling/roi_heads/roi_heads.py select_proposals_with_visible_keypoints,
 * modeling/roi_heads/keypoint_head.py keypoint_rcnn_loss).  Every kernel: rows >= *d_num_valid (device int, may be NULL) are neither
 * read nor written; no float atomics; two runs are bit-identical.
 * lvc_keypoint_targets (csrc/keypoint_targets.hip, no contraction, one launch): boxes [B,R,4]; matched int64 [B,R]: the row's
 *   instance among its image's; count int32 [B] with stride count_stride: rows [0, count_b) of image b are real; h_table / d_table:
 *   B x 2 int64 words per image (device pointer of the image's keypoints [n_b,K,3] fp32 = (x, y, v), n_b) on the host (checked) and on
 *   the device (read by the kernel).  target int32 [B*R,K] = (y * size + x) * valid with x = floor((x - x1) * (size / (x2 - x1))),
 *   x == x2 -> size - 1 (y likewise); valid uint8 [B*R,K] = inside [0, size) and v > 0; selected uint8 [B*R] = any keypoint with
 *   v >= 1 inside the box, both ends inclusive; sel_count int32 [B] = selected rows per image.  apply_selection != 0: valid &=
 *   selected[row].  A box of non-positive width or height, or a matched index outside [0, n_b): invalid, not selected.
 * lvc_keypoint_loss (csrc/keypoint_train.hip, two launches): low: planes [M,K,2S,2S] (lvc_keypoint_deconv), S <= 16; target int32 /
 *   valid uint8 [M,K].  Per valid entry the bilinear x2 map [4S,4S] is formed on chip with the decode's fp32 expression and
 *   term = logsumexp - z[target] in fp64; term fp64 [M,K], plane_max fp32 [M,K] and plane_lse fp64 [M,K] (log of sum exp(z - max))
 *   are written for valid entries only.  out_sum fp64 [1]: the ordered sum of the terms; out_count int64 [1]: the entries summed;
 *   out_loss fp32 [1] = sum / (normalizer > 0 ? normalizer : count) * loss_weight, exactly 0 when count is 0.  A target outside
 *   [0, 16 S^2) on a valid entry sets status bit 16 and the entry is skipped (here and in lvc_keypoint_loss_grad).
 * lvc_keypoint_loss_grad: dlow = the adjoint of the bilinear x2 applied to (softmax - onehot) * *d_upstream / normaliser * loss_weight
 *   (d_count: lvc_keypoint_loss's out_count, on the device), gathered per low-resolution pixel in fp64 in a fixed order and rounded
 *   once; zeros for invalid entries.  dlow is CHANNELS-LAST [M,2S,2S,Kc], Kc = lvc_keypoint_dlow_channels(K) = K rounded up to 4,
 *   padding channels zero.
 * lvc_keypoint_deconv_dx: dx [M,S,S,Cin] = sum_k sum_{ky,kx} dlow[m, 2iy-1+ky, 2ix-1+kx, k] W[ci,k,ky,kx] on fp32 MFMA (exact
 *   products, range-free); packed: [Cin][16*Kc] from lvc_keypoint_deconv_dx_pack (column (ky*4+kx)*Kc + k).  Cin a multiple of 16.
 * lvc_keypoint_deconv_wgrad (four launches): dw_packed [Cin][16*Kc] (the same packing) = sum over rows of x[row,ci] * dlow[tap], and
 *   db [K] = sum dlow, on fp32 MFMA over row slices fixed by M and S, the slices added in index order from `workspace`. */
int lvc_keypoint_targets(const float* boxes, const long long* matched, const int* count, int count_stride, const long long* h_table,
                         const long long* d_table, int B, int R, int K, int size, int apply_selection, int* target,
                         unsigned char* valid, unsigned char* selected, int* sel_count, void* stream);
int lvc_keypoint_dlow_channels(int K);
int lvc_keypoint_loss(const float* low, const int* target, const unsigned char* valid, const int* d_num_valid, int M, int K, int S,
                      double normalizer, double loss_weight, double* term, float* plane_max, double* plane_lse, float* out_loss,
                      double* out_sum, long long* out_count, int* d_status, void* stream);
int lvc_keypoint_loss_grad(const float* low, const int* target, const unsigned char* valid, const float* plane_max,
                           const double* plane_lse, const long long* d_count, const float* d_upstream, const int* d_num_valid, int M,
                           int K, int S, double normalizer, double loss_weight, float* dlow, void* stream);
int lvc_keypoint_deconv_dx_pack(const float* weight, float* packed, int Cin, int K, void* stream);
int lvc_keypoint_deconv_dx(const float* dlow, const float* packed, const int* d_num_valid, float* dx, int M, int S, int Cin, int K,
                           void* stream);
long long lvc_keypoint_deconv_wgrad_workspace_bytes(int M, int S, int Cin, int K);
int lvc_keypoint_deconv_wgrad(const float* x, const float* dlow, const int* d_num_valid, float* dw_packed, float* db, int M, int S,
                              int Cin, int K, void* workspace, long long workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LVC_AMD_H */
