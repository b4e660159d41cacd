// mask_targets.hip -- the mask branch's training targets (reference detectron2/structures/masks.py BitMasks.crop_and_resize, called
// from mask_rcnn_loss): ROIAlign((T, T), 1.0, 0, aligned=True) on each RoI's matched 0/1 ground-truth plane, then >= 0.5, for every
// foreground row of a batch in ONE launch.  One byte per target pixel leaves the chip.
//
// The reference gathers the planes per sampled row (gt_masks[matched_idxs]: 512 x H x W bytes per image) and converts them to fp32
// (4 bytes per image pixel and instance).  Here a row carries the INDEX of its plane, the planes are read as the bytes they are, and
// a small per-image table gives each image's base pointer and size (images of a batch differ in size, and every image's
// BitMasks.tensor is an allocation of its own).
//
// Arithmetic: fp32, in the order of the reference's ROIAlign_cpu.cpp (this file is built without contraction): the adaptive grid is
// ceil(roi_h / T) x ceil(roi_w / T); a sample outside [-1, H] x [-1, W] adds nothing but counts in the divisor; per sample the
// four-term sum w1 v1 + w2 v2 + w3 v3 + w4 v4 with w1 = hy hx ..., samples added iy-major, ONE division by the count.
// A workgroup owns one row of the [B, R] table; rows past the image's count are not written.
#include <stdint.h>

#include "common.h"

#define MT_FIELDS 4     // int64 words per image: plane base pointer, number of planes, H, W

__global__ __launch_bounds__(256) void mask_targets_kernel(const float* __restrict__ boxes, const long long* __restrict__ midx,
                                                           const int* __restrict__ count, int count_stride,
                                                           const long long* __restrict__ table, unsigned char* __restrict__ out, int R,
                                                           int T) {
  const int row = blockIdx.x;
  const int b = row / R, r = row - b * R;
  if (r >= count[(size_t)b * count_stride]) return;
  const long long* tb = table + (size_t)b * MT_FIELDS;
  const unsigned char* base = reinterpret_cast<const unsigned char*>((uintptr_t)tb[0]);
  const long long n = tb[1];
  const int H = (int)tb[2], W = (int)tb[3];
  const long long g = midx[row];
  unsigned char* o = out + (size_t)row * T * T;
  if (g < 0 || g >= n || H < 1 || W < 1) {      // no such plane: an empty target, nothing is read
    for (int i = threadIdx.x; i < T * T; i += 256) o[i] = 0;
    return;
  }
  const unsigned char* in = base + (size_t)g * H * W;
  const float* bx = boxes + (size_t)row * 4;
  const float roi_start_w = bx[0] * 1.0f - 0.5f;
  const float roi_start_h = bx[1] * 1.0f - 0.5f;
  const float roi_end_w = bx[2] * 1.0f - 0.5f;
  const float roi_end_h = bx[3] * 1.0f - 0.5f;
  const float roi_width = roi_end_w - roi_start_w;
  const float roi_height = roi_end_h - roi_start_h;
  const float bin_h = roi_height / (float)T;
  const float bin_w = roi_width / (float)T;
  int gh = (int)ceilf(roi_height / (float)T);
  int gw = (int)ceilf(roi_width / (float)T);
  if (!(roi_height >= 0.f && roi_width >= 0.f)) gh = gw = 0;      // (a malformed or NaN box: an empty grid, value 0)
  const int cnt = gh * gw > 1 ? gh * gw : 1;
  const float fcount = (float)cnt;
  for (int i = threadIdx.x; i < T * T; i += 256) {
    const int ph = i / T, pw = i - ph * T;
    float acc = 0.f;
    for (int iy = 0; iy < gh; ++iy) {
      const float yy = roi_start_h + ph * bin_h + (float)(iy + .5f) * bin_h / (float)gh;
      for (int ix = 0; ix < gw; ++ix) {
        const float xx = roi_start_w + pw * bin_w + (float)(ix + .5f) * bin_w / (float)gw;
        float x = xx, y = yy;
        if (y < -1.0f || y > (float)H || x < -1.0f || x > (float)W) continue;
        if (y <= 0) y = 0;
        if (x <= 0) x = 0;
        int y_low = (int)y, x_low = (int)x, y_high, x_high;
        if (y_low >= H - 1) { y_high = y_low = H - 1; y = (float)y_low; } else y_high = y_low + 1;
        if (x_low >= W - 1) { x_high = x_low = W - 1; x = (float)x_low; } else x_high = x_low + 1;
        const float ly = y - y_low, lx = x - x_low;
        const float hy = 1.f - ly, hx = 1.f - lx;
        const float w1 = hy * hx, w2 = hy * lx, w3 = ly * hx, w4 = ly * lx;
        const float v1 = in[(size_t)y_low * W + x_low] ? 1.f : 0.f;
        const float v2 = in[(size_t)y_low * W + x_high] ? 1.f : 0.f;
        const float v3 = in[(size_t)y_high * W + x_low] ? 1.f : 0.f;
        const float v4 = in[(size_t)y_high * W + x_high] ? 1.f : 0.f;
        acc += w1 * v1 + w2 * v2 + w3 * v3 + w4 * v4;
      }
    }
    o[i] = (acc / fcount) >= 0.5f ? 1 : 0;
  }
}

extern "C" int lvc_mask_targets(const float* boxes, const long long* matched, const int* count, int count_stride,
                                const long long* h_table, const long long* d_table, int B, int R, int T, unsigned char* out,
                                void* stream) {
  LVC_CHECK_ARG(B >= 0 && R >= 0 && T >= 1 && T <= 1024 && count_stride >= 1, "B >= 0, R >= 0, 1 <= T <= 1024, count_stride >= 1");
  if (B == 0 || R == 0) return LVC_OK;
  LVC_CHECK_ARG(boxes && matched && count && h_table && d_table && out, "null pointer");
  LVC_CHECK_ARG((long long)B * R < (1LL << 31), "too many rows");
  for (int b = 0; b < B; ++b) {
    const long long* tb = h_table + (size_t)b * MT_FIELDS;
    LVC_CHECK_ARG(tb[1] >= 0 && tb[2] >= 0 && tb[3] >= 0 && tb[2] < (1 << 24) && tb[3] < (1 << 24), "plane table: sizes out of range");
    LVC_CHECK_ARG(tb[1] == 0 || tb[2] == 0 || tb[3] == 0 || tb[0] != 0, "plane table: null plane pointer");
  }
  hipLaunchKernelGGL(mask_targets_kernel, dim3((unsigned)(B * R)), dim3(256), 0, (hipStream_t)stream, boxes, matched, count, count_stride,
                     d_table, out, R, T);
  LVC_CHECK_LAUNCH();
  return LVC_OK;
}
