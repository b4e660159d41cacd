// seg_bilinear.h -- the one bilinear expression of the semantic branch, shared by sem_seg.hip (inference) and sem_seg_train.hip (loss
// and gradients) so that both see the same bits.  Rows weigh l, columns m:
//   v = l0 (m0 a + m1 b) + l1 (m0 c + m1 d)
// with ATen's coordinates for align_corners=False: s = max(scale (d + 0.5) - 0.5, 0), i0 = (int)s, i1 = i0 + (i0 < size - 1),
// w1 = s - i0, w0 = 1 - w1.  Both objects are EXACT (-ffp-contract=off): every fp32 operation rounds as written.
#pragma once
#include <hip/hip_runtime.h>

struct SegTap {
  int i0, i1;
  float w0, w1;
};

// area_pixel_compute_source_index (cubic = false) and the two taps of upsample_bilinear2d
__host__ __device__ __forceinline__ SegTap seg_tap(float scale, int d, int size) {
  float s = scale * ((float)d + 0.5f) - 0.5f;
  s = s < 0.f ? 0.f : s;
  SegTap t;
  t.i0 = (int)s;
  if (t.i0 > size - 1) t.i0 = size - 1;      // (never for an output inside scale * size; keeps every index in bounds)
  t.i1 = t.i0 + (t.i0 < size - 1 ? 1 : 0);
  t.w1 = s - (float)t.i0;
  t.w0 = 1.f - t.w1;
  return t;
}

__device__ __forceinline__ float seg_bilerp(float l0, float l1, float m0, float m1, float a, float b, float c, float d) {
  return l0 * (m0 * a + m1 * b) + l1 * (m0 * c + m1 * d);
}
