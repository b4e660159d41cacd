/* lvc_amd_segtrain.h -- the entry points of liblvc_amd.so that train the semantic branch (prefix lvcst_; csrc/sem_seg_train.hip).
 *
 * A third statement of the C ABI beside lvc_amd.h and lvc_amd_seg.h, held to the same discipline: csrc/common.h includes it, so every
 * definition is compiled against its declaration; lvc_amd/_lib.py binds restype / argtypes of every lvcst_* function from this text;
 * the exported lvcst_* symbols of the library are exactly the ones declared here (tests/test_host_abi_segtrain.py).  Plain C99 without
 * typedefs, structs or function pointers.  Every int function returns LVC_OK (0) or an error code of lvc_amd.h; the text of the last
 * error is lvc_last_error().  Nothing here allocates, synchronises or reads back: a call validates its host arguments and enqueues its
 * launches on `stream`.  No kernel here uses a floating-point atomic: every sum has one fixed order, two runs give the same bits.
 */
#ifndef LVC_AMD_SEGTRAIN_H
#define LVC_AMD_SEGTRAIN_H

#ifdef __cplusplus
extern "C" {
#endif

/* The adjoint of lvcseg_upsample2_bilinear_nhwc without accumulator: dy [N,2H,2W,C] -> dx [N,H,W,C], fp32, C % 4 == 0, 16-byte aligned.
 * dx[i, j] = sum over the outputs (oy, ox), ascending rows then columns, whose taps touch (i, j), of (l m) dy[oy, ox], where l is the
 * forward's weight of row i at output row oy (w0 where i0 == i, plus w1 where i1 == i: a clamped border output puts both on one
 * pixel) and m the same for columns.  One thread per four channels of one dx pixel gathers; dx is written once.  */
int lvcst_upsample2_bilinear_bwd_nhwc(const float* dy, float* dx, int N, int H, int W, int C, void* stream);

/* int64 words per image of the loss entries' job table:
 *   0 offset (elements) of the image's own label map [label_h, label_w] in `labels`   1 label_h   2 label_w
 * A pixel of the scale*h x scale*w map outside [label_h, label_w] counts as `ignore_value` (ImageList.from_tensors' padding, without
 * the padded copy).  label_h <= scale * h, label_w <= scale * w.  */
#define LVCST_LOSS_FIELDS 3
/* bit of the status word: a label that is neither `ignore_value` nor in [0, K) was met (it adds nothing) */
#define LVCST_STATUS_LABEL_RANGE 1

/* bytes of lvcst_sem_seg_loss_fwd's workspace (the per-workgroup partials: an fp64 sum and an int64 count each); -1 for arguments
 * outside the kernel's range */
long long lvcst_sem_seg_loss_workspace_bytes(int N, int h, int w, int K, int scale);

/* F.cross_entropy(F.interpolate(logits, scale_factor=scale, "bilinear", align_corners=False), labels, reduction="mean",
 * ignore_index=ignore_value) without the interpolated tensor.  logits [N,h,w,ld] fp32 of which the first K channels are read.  Per
 * pixel of the scale*h x scale*w map, fp32 without contraction: z_k by the expression of lvcseg_sem_seg_postprocess' first stage (the
 * same bits), m = max_k z_k, lse = m + logf(sum_k expf(z_k - m)) in class order, loss = lse - z_t.  labels: label_bytes 1 (uint8) or 8
 * (int64), read through the job table (h_jobs: the host's copy, validated here; d_jobs: the device's).  Writes, for every pixel of the
 * [N,scale*h,scale*w] map, mmax = m and lsum = logf(sum) -- the two parts of lse, kept apart for the backward: their fp32 sum has lost,
 * where |m| is large, what the softmax needs -- and lse itself where `lse` is not NULL; per-workgroup (fp64 sum, int64 count) partials
 * into `workspace`; then one workgroup adds the partials in index order and writes *loss = (float)(sum / count) (NaN when
 * count == 0), *sum and *count.  ORs LVCST_STATUS_LABEL_RANGE into *status (which the caller clears).  1 <= scale <= 64,
 * 1 <= K <= 4096, ld >= K; refused where the low-resolution footprint of one output pixel exceeds the LDS budget (60 KB).  */
int lvcst_sem_seg_loss_fwd(const float* logits, int N, int h, int w, int K, int ld, int scale, const void* labels,
                           long long labels_numel, int label_bytes, long long ignore_value, const long long* h_jobs,
                           const long long* d_jobs, float* mmax, float* lsum, float* lse, void* workspace, long long workspace_bytes,
                           float* loss, double* sum, long long* count, int* status, void* stream);

/* dlow [N,h,w,ld]: the gradient of *loss times *g with respect to the logits, i.e. the transposed interpolation of
 * (expf((z_k - mmax) - lsum) - [k == t]) over the valid pixels, times *g / (float)*count; channels K .. ld-1 are written as zeros.
 * z is recomputed from the logits; `mmax`, `lsum` and `count` are the forward's, `g` the upstream scalar on the device.  One thread
 * owns one (low-resolution pixel, class) and adds its outputs in ascending (row, column) order.  */
int lvcst_sem_seg_loss_bwd(const float* logits, int N, int h, int w, int K, int ld, int scale, const void* labels,
                           long long labels_numel, int label_bytes, long long ignore_value, const long long* h_jobs,
                           const long long* d_jobs, const float* mmax, const float* lsum, const float* g, const long long* count,
                           float* dlow, void* stream);

#ifdef __cplusplus
}
#endif
#endif
