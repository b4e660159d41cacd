// avgpool.hip -- nn.AvgPool2d(2) of the ResNet-D trunk (RESNETS.D: reference detectron2/modeling/backbone/resnet.py:359, :399, the
// pools in front of conv3 and of the projection shortcut of a BottleneckBlockCLIP), NHWC fp32, forward and backward.
//   lvc_avgpool2_nhwc     : y[n, i, j, c] = (((x[2i,2j] + x[2i,2j+1]) + x[2i+1,2j]) + x[2i+1,2j+1]) * 0.25f, H//2 x W//2 outputs (an odd
//                           last row / column is dropped, as AvgPool2d's floor).  That is ATen's CPU summation order; the file is built
//                           with -ffp-contract=off, so the result is bit-reproducible.  y rows are ldo floats wide: a channel slice of a
//                           wider buffer ([pool(conv2 output) | pool(x)] of the one-GEMM conv3 + shortcut), other channels untouched.
//   lvc_avgpool2_bwd_nhwc : dx[n, h, w, c] = 0.25f * dy[n, h/2, w/2, c], zeros in a dropped odd row / column; dy rows ldi floats wide.
// Streaming kernels: one thread per four channels of an output pixel, 16-byte loads and stores along C, no LDS, no atomics.
#include "common.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(256) void avgpool2_kernel(const f32x4* __restrict__ x, float* __restrict__ y, int H, int W, int Ho, int Wo,
                                                       int C4, int ldo, long long total) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int c = (int)(i % C4);
  long long q = i / C4;
  const int ox = (int)(q % Wo); q /= Wo;
  const int oy = (int)(q % Ho);
  const int n = (int)(q / Ho);
  const long long row = (long long)W * C4;
  const f32x4* p = x + (((long long)n * H + 2 * oy) * W + 2 * ox) * C4 + c;      // 2 oy + 1 < H and 2 ox + 1 < W by Ho = H / 2, Wo = W / 2
  const f32x4 a = p[0], b = p[C4], d = p[row], e = p[row + C4];
  const f32x4 v = (((a + b) + d) + e) * 0.25f;
  *reinterpret_cast<f32x4*>(y + (((long long)n * Ho + oy) * Wo + ox) * ldo + c * 4) = v;
}

__global__ __launch_bounds__(256) void avgpool2_bwd_kernel(const float* __restrict__ dy, f32x4* __restrict__ dx, int H, int W, int Ho,
                                                           int Wo, int C4, int ldi, long long total) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int c = (int)(i % C4);
  long long q = i / C4;
  const int ix = (int)(q % W); q /= W;
  const int iy = (int)(q % H);
  const int n = (int)(q / H);
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if ((iy >> 1) < Ho && (ix >> 1) < Wo)
    v = *reinterpret_cast<const f32x4*>(dy + (((long long)n * Ho + (iy >> 1)) * Wo + (ix >> 1)) * ldi + c * 4) * 0.25f;
  dx[i] = v;
}

static int avgpool2_check(const char* fn, const void* a, const void* b, int N, int H, int W, int C, int ld, long long total) {
  if (!(a && b && N > 0 && H >= 2 && W >= 2 && C > 0 && C % 4 == 0)) {
    lvc_set_error("%s: needs N > 0, H >= 2, W >= 2 and C a positive multiple of 4", fn);
    return LVC_ERR_INVALID;
  }
  if (!(ld >= C && ld % 4 == 0 && (((uintptr_t)a | (uintptr_t)b) & 15) == 0)) {
    lvc_set_error("%s: the row pitch must be a multiple of 4 and >= C, the pointers 16-byte aligned", fn);
    return LVC_ERR_INVALID;
  }
  if (!(total > 0 && lvc_cdiv64(total, 256) <= 0x7FFFFFFFLL)) {
    lvc_set_error("%s: tensor too large for one launch", fn);
    return LVC_ERR_INVALID;
  }
  return LVC_OK;
}

extern "C" int lvc_avgpool2_nhwc(const float* x, float* y, int N, int H, int W, int C, int ldo, void* stream) {
  const int ld = ldo > 0 ? ldo : C;
  const int Ho = H / 2, Wo = W / 2;
  const long long total = (long long)N * Ho * Wo * (C / 4);
  const int st = avgpool2_check(__func__, x, y, N, H, W, C, ld, total);
  if (st != LVC_OK) return st;
  hipLaunchKernelGGL(avgpool2_kernel, dim3((unsigned)lvc_cdiv64(total, 256)), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<const f32x4*>(x), y, H, W, Ho, Wo, C / 4, ld, total);
  LVC_CHECK_LAUNCH();
  return LVC_OK;
}

extern "C" int lvc_avgpool2_bwd_nhwc(const float* dy, float* dx, int N, int H, int W, int C, int ldi, void* stream) {
  const int ld = ldi > 0 ? ldi : C;
  const long long total = (long long)N * H * W * (C / 4);
  const int st = avgpool2_check(__func__, dy, dx, N, H, W, C, ld, total);
  if (st != LVC_OK) return st;
  hipLaunchKernelGGL(avgpool2_bwd_kernel, dim3((unsigned)lvc_cdiv64(total, 256)), dim3(256), 0, (hipStream_t)stream, dy,
                     reinterpret_cast<f32x4*>(dx), H, W, H / 2, W / 2, C / 4, ld, total);
  LVC_CHECK_LAUNCH();
  return LVC_OK;
}
