/* lvc_amd_seg.h -- the semantic / panoptic entry points of liblvc_amd.so (prefix lvcseg_).
 *
 * A second statement of the C ABI beside lvc_amd.h, held to the same discipline: csrc/common.h includes it, so every definition is
 * compiled against its declaration; lvc_amd/_lib.py binds restype / argtypes of every lvcseg_* function from this text; the exported
 * lvcseg_* symbols of the library are exactly the ones declared here (tests/test_host_abi_seg.py).  Plain C99 without typedefs,
 * structs or function pointers.  Every function returns LVC_OK (0) or an error code of lvc_amd.h; the text of the last error is
 * lvc_last_error().  Nothing here allocates, synchronises or reads back: a call validates its host arguments and enqueues one launch
 * on `stream`.
 */
#ifndef LVC_AMD_SEG_H
#define LVC_AMD_SEG_H

#ifdef __cplusplus
extern "C" {
#endif

/* y = up2(x) (acc == NULL) or y = acc + up2(x): nn.Upsample(scale_factor=2, mode="bilinear", align_corners=False) on NHWC fp32.
 * x [N,H,W,C], acc and y [N,2H,2W,C], C % 4 == 0, all 16-byte aligned; y may be acc.  Per output element, in fp32 without contraction:
 *   s = max(0.5 (d + 0.5) - 0.5, 0), i0 = (int)s, i1 = min(i0 + 1, size - 1), w1 = s - i0, w0 = 1 - w1      (rows: l, columns: m)
 *   v = l0 (m0 a + m1 b) + l1 (m0 c + m1 d),   a = x[y0,x0], b = x[y0,x1], c = x[y1,x0], d = x[y1,x1];   y = v  or  y = acc + v.  */
int lvcseg_upsample2_bilinear_nhwc(const float* x, const float* acc, float* y, int N, int H, int W, int C, void* stream);

/* int64 words per job of lvcseg_sem_seg_postprocess, one job per image:
 *   0 offset (floats) of the image's low-resolution logits [h, w, ld] in `logits`   1 h   2 w
 *   3 image height   4 image width      (the crop of the x`scale` map; <= scale * h, scale * w)
 *   5 output height  6 output width
 *   7 offset (floats) of the image's [K, out_h, out_w] plane in `soft`   8 offset (elements) of its [out_h, out_w] map in `labels` */
#define LVCSEG_POST_FIELDS 9

/* F.interpolate(scale_factor=scale) -> crop to the image size -> F.interpolate(size=(out_h, out_w)) -> argmax over the K classes, per
 * output pixel, without writing the intermediate maps.  Both interpolations are bilinear, align_corners=False, fp32 without
 * contraction, coordinates as ATen's area_pixel_compute_source_index (scale 1 / `scale` for the first stage, (float)in / out for the
 * second); each takes the expression of lvcseg_upsample2_bilinear_nhwc.  Where the output size equals the image size the second stage
 * is the identity and is not evaluated.  The argmax takes the lowest class on equal values.  logits: NHWC rows of `ld` floats of which
 * the first K are read.  soft (fp32, CHW per image) and labels (label_bytes 1: uint8, needs K <= 256; 4: int32) are each optional
 * (NULL), not both.  h_jobs / d_jobs: the same table on the host (validated here) and on the device (read by the kernel).  */
int lvcseg_sem_seg_postprocess(const float* logits, long long logits_numel, const long long* h_jobs, const long long* d_jobs,
                               int num_jobs, int K, int ld, int scale, float* soft, long long soft_numel, void* labels,
                               long long labels_numel, int label_bytes, void* stream);

/* int64 words per image of lvcseg_panoptic_combine:
 *   0 row of the image's first instance in the plane table   1 number of instances
 *   2 height   3 width
 *   4 offset (elements) of its label map in `labels`   5 offset (int32 elements) of its map in `panoptic`
 *   6 first row of its segment table in `segments`     7 rows reserved there (>= instances + num_labels)
 *   8 index of the first instance's score in `scores` and of its class in `classes`  */
#define LVCSEG_COMBINE_FIELDS 9
/* int32 words per row of the segment table: id, isthing, category, instance index (-1 for stuff), score (fp32 bits; 0 for stuff),
 * area (pixels the segment took), 0, 0.  Rows past an image's count are zero. */
#define LVCSEG_SEGMENT_FIELDS 8

/* combine_semantic_and_instance_outputs for a batch, one workgroup per image.  planes: uint8 [h, w] per instance (0 / 1) at the byte
 * offsets of `plane_jobs`, the job table of lvc_paste_masks (LVC paste fields: row, box as four fp32 bit patterns, h, w, byte offset);
 * use_boxes != 0: a plane is zero outside its box (enlarged as the paste kernel enlarges it), so only that rectangle is scanned.
 * Instances in descending score (equal scores: lower index first); stop at the first score < instances_thresh (in double); skip
 * zero area; skip when (double)intersect / (double)area > overlap_thresh; otherwise the instance takes its free pixels.  Then the
 * labels 1 .. num_labels - 1 present in the map, ascending, each taking its free pixels unless (double)area < stuff_area_limit.
 * Writes every pixel of `panoptic` (0: no segment), the segment rows and counts[image].  Integer counts only: two runs give the same
 * bits.  At most 1024 instances per image, num_labels <= 4096.  */
int lvcseg_panoptic_combine(const unsigned char* planes, long long planes_bytes, const long long* h_plane_jobs,
                            const long long* d_plane_jobs, int num_planes, int use_boxes, const float* scores, const int* classes,
                            const void* labels, long long labels_numel, int label_bytes, int num_labels, const long long* h_images,
                            const long long* d_images, int num_images, double overlap_thresh, double stuff_area_limit,
                            double instances_thresh, int* panoptic, long long panoptic_numel, int* segments, long long segment_rows,
                            int* counts, void* stream);

#ifdef __cplusplus
}
#endif
#endif
