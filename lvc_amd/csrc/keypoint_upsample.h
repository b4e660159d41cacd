// keypoint_upsample.h -- the bilinear x2 upsampling of KRCNNConvDeconvUpsampleHead.layers (align_corners=False) as ONE fp32 expression,
// shared by the decode (keypoint_decode.hip) and the training loss and its gradient (keypoint_train.hip): training and inference see
// the same bits.  Both files are built without contraction.
#pragma once

// ATen's source index of output index `o` at scale 2, max(0, (o + 0.5) / 2 - 0.5), on a source of P samples -> the two taps and
// their weights
__device__ __forceinline__ void kp_up2_taps(int o, int P, int& i0, int& i1, float& l0, float& l1) {
  float s = ((float)o + 0.5f) * 0.5f - 0.5f;
  s = s < 0.f ? 0.f : s;
  i0 = (int)s;
  i1 = i0 + (i0 < P - 1 ? 1 : 0);
  l1 = s - (float)i0;
  l0 = 1.f - l1;
}

// the value at (oy, ox) of the x2 map of the plane src [P, P]
__device__ __forceinline__ float kp_up2(const float* src, int P, int oy, int ox) {
  int y0, y1, x0, x1;
  float ly0, ly1, lx0, lx1;
  kp_up2_taps(oy, P, y0, y1, ly0, ly1);
  kp_up2_taps(ox, P, x0, x1, lx0, lx1);
  const float t0 = src[y0 * P + x0] * lx0 + src[y0 * P + x1] * lx1;
  const float t1 = src[y1 * P + x0] * lx0 + src[y1 * P + x1] * lx1;
  return t0 * ly0 + t1 * ly1;
}

// the weight with which output index `o` reads source sample `a` (0 when it does not): the adjoint's coefficient
__device__ __forceinline__ float kp_up2_weight(int o, int P, int a) {
  int i0, i1;
  float l0, l1;
  kp_up2_taps(o, P, i0, i1, l0, l1);
  return (i0 == a ? l0 : 0.f) + (i1 == a ? l1 : 0.f);
}
