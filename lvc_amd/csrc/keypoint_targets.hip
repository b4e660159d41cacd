// keypoint_targets.hip -- the keypoint branch's training targets for every sampled foreground row of a batch in ONE launch (reference
// detectron2/structures/keypoints.py _keypoints_to_heatmap, called from keypoint_rcnn_loss, and modeling/roi_heads/roi_heads.py
// select_proposals_with_visible_keypoints).
//
// A row of the sampled [B, R] table carries the INDEX of its matched ground-truth instance; the instance's keypoints [K, 3] =
// (x, y, v) are read through it from the image's own tensor [n_b, K, 3] (a small per-image table gives base pointer and n_b): nothing
// is gathered on the host.  Per (row, keypoint), in fp32 and in the reference's order (this file is built without contraction, with
// correctly rounded division):
//     x = floor((x - x1) * (size / (x2 - x1))),  y likewise;   x == x2 -> size - 1,  y == y2 -> size - 1
//     valid = 0 <= x < size and 0 <= y < size and v > 0;       target = (y * size + x) * valid
// and per row  selected = any keypoint with v >= 1 and x1 <= x <= x2 and y1 <= y <= y2  (both ends inclusive).  With `apply_selection`
// the written valid is valid & selected: the reference drops the rows that are not selected before it forms the loss, and the two
// rules can disagree by a rounding just past x2.  A box of non-positive width or height makes its row invalid and not selected (the
// reference floors an inf or a NaN there); so does a matched index outside [0, n_b).
// One workgroup owns one image: a thread walks rows tid, tid + 256, ... below the image's count and its K keypoints; the image's
// number of selected rows is a fixed tree over the workgroup's integer counts.  Rows past the count are not written.
#include <stdint.h>

#include "common.h"

#define KT_FIELDS 2     // int64 words per image: keypoint base pointer, number of instances

__global__ __launch_bounds__(256) void keypoint_targets_kernel(const float* __restrict__ boxes, const long long* __restrict__ midx,
                                                               const int* __restrict__ count, int count_stride,
                                                               const long long* __restrict__ table, int* __restrict__ target,
                                                               unsigned char* __restrict__ valid, unsigned char* __restrict__ selected,
                                                               int* __restrict__ sel_count, int R, int K, int size, int apply_selection) {
  __shared__ int red[256];
  const int b = blockIdx.x, tid = threadIdx.x;
  int cnt = count[(size_t)b * count_stride];
  cnt = cnt < 0 ? 0 : (cnt < R ? cnt : R);
  const long long* tb = table + (size_t)b * KT_FIELDS;
  const float* base = reinterpret_cast<const float*>((uintptr_t)tb[0]);
  const long long n = tb[1];
  const float fsize = (float)size;
  int mine = 0;
  for (int r = tid; r < cnt; r += 256) {
    const size_t row = (size_t)b * R + r;
    const float* bx = boxes + row * 4;
    const float x1 = bx[0], y1 = bx[1], x2 = bx[2], y2 = bx[3];
    const long long g = midx[row];
    const bool real = g >= 0 && g < n && x2 - x1 > 0.f && y2 - y1 > 0.f;      // (a NaN side compares false)
    int sel = 0;
    if (real) {
      const float* kp = base + (size_t)g * K * 3;
      for (int k = 0; k < K; ++k) {
        const float kx = kp[k * 3], ky = kp[k * 3 + 1], v = kp[k * 3 + 2];
        sel |= v >= 1.f && kx >= x1 && kx <= x2 && ky >= y1 && ky <= y2;
      }
      const float scale_x = fsize / (x2 - x1), scale_y = fsize / (y2 - y1);
      for (int k = 0; k < K; ++k) {
        const float kx = kp[k * 3], ky = kp[k * 3 + 1], v = kp[k * 3 + 2];
        float fx = floorf((kx - x1) * scale_x), fy = floorf((ky - y1) * scale_y);
        if (kx == x2) fx = fsize - 1.f;
        if (ky == y2) fy = fsize - 1.f;
        // compared as floats: an inf or a NaN is never converted
        bool ok = fx >= 0.f && fx < fsize && fy >= 0.f && fy < fsize && v > 0.f;
        const int t = ok ? (int)fy * size + (int)fx : 0;
        if (apply_selection && !sel) ok = false;
        target[row * K + k] = ok ? t : 0;
        valid[row * K + k] = ok ? 1 : 0;
      }
    } else {
      for (int k = 0; k < K; ++k) {
        target[row * K + k] = 0;
        valid[row * K + k] = 0;
      }
    }
    selected[row] = (unsigned char)sel;
    mine += sel;
  }
  red[tid] = mine;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  if (tid == 0) sel_count[b] = red[0];
}

extern "C" int lvc_keypoint_targets(const float* boxes, const long long* matched, const int* count, int count_stride,
                                    const long long* h_table, const long long* d_table, int B, int R, int K, int size,
                                    int apply_selection, int* target, unsigned char* valid, unsigned char* selected, int* sel_count,
                                    void* stream) {
  LVC_CHECK_ARG(B >= 0 && R >= 0 && K >= 1 && K <= 4096 && count_stride >= 1, "B >= 0, R >= 0, 1 <= K <= 4096, count_stride >= 1");
  LVC_CHECK_ARG(size >= 1 && size <= 4096, "1 <= size <= 4096");      // size^2 and every fp32 bin index are exact
  if (B == 0) return LVC_OK;
  LVC_CHECK_ARG(count && h_table && d_table && sel_count, "null pointer");
  LVC_CHECK_ARG(R == 0 || (boxes && matched && target && valid && selected), "null pointer");
  LVC_CHECK_ARG((long long)B * R * K < (1LL << 31), "too many (row, keypoint) entries");
  for (int b = 0; b < B; ++b) {
    const long long* tb = h_table + (size_t)b * KT_FIELDS;
    LVC_CHECK_ARG(tb[1] >= 0 && tb[1] < (1LL << 31), "keypoint table: instance count out of range");
    LVC_CHECK_ARG(tb[1] == 0 || tb[0] != 0, "keypoint table: null keypoint pointer");
  }
  hipLaunchKernelGGL(keypoint_targets_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, boxes, matched, count, count_stride,
                     d_table, target, valid, selected, sel_count, R, K, size, apply_selection);
  LVC_CHECK_LAUNCH();
  return LVC_OK;
}
