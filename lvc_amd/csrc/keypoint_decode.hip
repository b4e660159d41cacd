// keypoint_decode.hip -- heatmaps_to_keypoints (reference detectron2/structures/keypoints.py:145-212) for every (RoI, keypoint) of a
// batch in one launch, with the bilinear x2 upsampling of KRCNNConvDeconvUpsampleHead.layers in front of it when up == 2.
//
// The reference loops over the RoIs in Python: F.interpolate(bicubic) to the box's ceil(h) x ceil(w), a max and an argmax over that
// map, two exp maps and a sum -- [K, h, w] temporaries per box.  Here one workgroup owns one (RoI, keypoint) plane and nothing of the
// box's size is ever stored:
//   0. the plane [P, P] is read once; with up == 2 the bilinear x2 map (align_corners=False, ATen's source index
//      max(0, (dst + 0.5) / 2 - 0.5)) is formed in LDS, and written to maps_out only when that pointer is given.
//   1. ATen's bicubic resize (A = -0.75; scale = in / out; source = scale (dst + 0.5) - 0.5, NOT clamped; floor; the four taps read at
//      clamped indices), evaluated separably as ATen does: along x first, then along y (coefficients: see kp_taps).  The output is tiled in strips of KP_TW = 64
//      columns: a strip holds the x-interpolated value of EVERY source row for its 64 columns ([side][64] floats of LDS, whatever the
//      box's size), and the four waves walk the output rows (row y belongs to wave y & 3), each output being four LDS reads.
//   2. maximum and position: among equal maxima the LOWEST flat index y * w + x wins (torch.argmax on the CPU).  Every lane keeps
//      (value, index) under that rule, then a fixed tree over the 256 lanes; no atomics.
//   3. score = exp(v - max) / sum over the [side, side] source map of exp(map - max): the reference's mixed normalisation
//      (keypoints.py:184-191), max being the full-resolution maximum.
//   4. x = (x_int + 0.5) * (w / ceil w) + x1, y likewise, in the reference's fp32 order (this file is built without contraction).
// out [M, K, 4] = (x, y, logit, score).  Rows past *d_num_valid keep their bytes.
#include <stdint.h>

#include "common.h"
#include "keypoint_upsample.h"
#include "rows_common.h"

#define KP_TW 64           // output columns per strip
#define KP_MAX_SIDE 64     // up * P at most (LDS: two [side][64] float arrays)

__device__ __forceinline__ double kp_cc1(double x, double A) { return ((A + 2.) * x - (A + 3.)) * x * x + 1.; }
__device__ __forceinline__ double kp_cc2(double x, double A) { return ((A * x - 5. * A) * x + 8. * A) * x - 4. * A; }

// Source index and ATen's get_cubic_upsample_coefficients for output index `dst`: -> floor(source), w[4].  The index and the four
// coefficients are formed in fp64 and rounded once to fp32: in fp32 the source index of a wide box carries an error of an ulp of
// ~50 into t, and the coefficients three more roundings -- measured against the fp64 resize, a maximum formed with fp32 coefficients
// deviated up to 3.2 x as far as ATen's own fp32 result, with these at most as far.  The sums over the taps stay fp32.
__device__ __forceinline__ int kp_taps(int n_in, int n_out, int dst, float w[4]) {
  const double A = -0.75;
  const double src = (double)n_in / (double)n_out * ((double)dst + 0.5) - 0.5;
  const double fl = floor(src);
  const double t = src - fl;
  w[0] = (float)kp_cc2(t + 1., A);
  w[1] = (float)kp_cc1(t, A);
  w[2] = (float)kp_cc1(1. - t, A);
  w[3] = (float)kp_cc2(2. - t, A);
  return (int)fl;
}

__device__ __forceinline__ int kp_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// (value, flat index) under the rule "greater value, or equal value and lower index"
__device__ __forceinline__ void kp_better(float& bv, long long& bi, float v, long long i) {
  if (v > bv || (v == bv && i < bi)) {
    bv = v;
    bi = i;
  }
}

__global__ __launch_bounds__(256) void heatmaps_to_keypoints_kernel(const float* __restrict__ maps, const float* __restrict__ rois,
                                                                    const int* __restrict__ d_num_valid, float* __restrict__ maps_out,
                                                                    float* __restrict__ out, int M, int K, int P, int up) {
  __shared__ float smap[KP_MAX_SIDE * KP_MAX_SIDE];       // the source map [side][side]
  __shared__ float strip[KP_MAX_SIDE * KP_TW];            // x-interpolated source rows of the current strip [side][KP_TW]
  __shared__ float red_v[256];
  __shared__ long long red_i[256];
  __shared__ float red_s[4];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int Mv = lvc_valid_rows(d_num_valid, M);
  const int m = blockIdx.x / K, k = blockIdx.x - m * K;
  if (m >= Mv) return;      // (uniform)
  const int side = up * P;
  const float* src = maps + ((size_t)m * K + k) * P * P;

  // 0. the source map
  if (up == 1) {
    for (int i = tid; i < side * side; i += 256) smap[i] = src[i];
  } else {
    for (int i = tid; i < side * side; i += 256) {
      const int oy = i / side, ox = i - oy * side;
      smap[i] = kp_up2(src, P, oy, ox);      // (keypoint_upsample.h: the expression the training loss uses too)
    }
  }
  __syncthreads();
  if (maps_out) {
    float* dst = maps_out + ((size_t)m * K + k) * side * side;
    for (int i = tid; i < side * side; i += 256) dst[i] = smap[i];
  }

  // the box
  const float bx1 = rois[m * 4 + 0], by1 = rois[m * 4 + 1], bx2 = rois[m * 4 + 2], by2 = rois[m * 4 + 3];
  float bw = bx2 - bx1, bh = by2 - by1;
  bw = bw > 1.f ? bw : 1.f;       // clamp(min=1); a NaN becomes 1
  bh = bh > 1.f ? bh : 1.f;
  const float cw = ceilf(bw), ch = ceilf(bh);
  // (the host has checked the boxes it could see; a box from the device beyond the limit is cut to it: nothing is indexed by it)
  const int ow = cw < 16384.f ? (int)cw : 16384, oh = ch < 16384.f ? (int)ch : 16384;

  float bv = -INFINITY;
  long long bi = 0x7fffffffffffffffLL;
  for (int x0 = 0; x0 < ow; x0 += KP_TW) {
    // 1a. this lane's column: the x-interpolated value of the source rows wave, wave + 4, ...
    const int ox = x0 + lane;
    if (ox < ow) {
      float wx[4];
      const int ix = kp_taps(side, ow, ox, wx);
      const int c0 = kp_clamp(ix - 1, side - 1), c1 = kp_clamp(ix, side - 1), c2 = kp_clamp(ix + 1, side - 1), c3 = kp_clamp(ix + 2, side - 1);
      for (int r = wave; r < side; r += 4) {
        const float* row = smap + r * side;
        float v = row[c0] * wx[0];
        v = fmaf(row[c1], wx[1], v);
        v = fmaf(row[c2], wx[2], v);
        v = fmaf(row[c3], wx[3], v);
        strip[r * KP_TW + lane] = v;
      }
    }
    __syncthreads();
    // 1b + 2. the output rows of this strip
    if (ox < ow) {
      for (int oy = wave; oy < oh; oy += 4) {
        float wy[4];
        const int iy = kp_taps(side, oh, oy, wy);
        float v = strip[kp_clamp(iy - 1, side - 1) * KP_TW + lane] * wy[0];
        v = fmaf(strip[kp_clamp(iy, side - 1) * KP_TW + lane], wy[1], v);
        v = fmaf(strip[kp_clamp(iy + 1, side - 1) * KP_TW + lane], wy[2], v);
        v = fmaf(strip[kp_clamp(iy + 2, side - 1) * KP_TW + lane], wy[3], v);
        kp_better(bv, bi, v, (long long)oy * ow + ox);
      }
    }
    __syncthreads();
  }
  red_v[tid] = bv;
  red_i[tid] = bi;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) {
      float v = red_v[tid];
      long long i = red_i[tid];
      kp_better(v, i, red_v[tid + s], red_i[tid + s]);
      red_v[tid] = v;
      red_i[tid] = i;
    }
    __syncthreads();
  }
  const float vmax = red_v[0];
  long long pos = red_i[0];
  if (pos == 0x7fffffffffffffffLL) pos = 0;      // no value compared greater than -inf (a map of NaN)

  // 3. sum over the source map of exp(map - max): per lane, then the wave's lanes and the four waves in a fixed order
  float s = 0.f;
  for (int i = tid; i < side * side; i += 256) s += expf(smap[i] - vmax);
  for (int d = 32; d > 0; d >>= 1) s += __shfl_xor(s, d);
  if (lane == 0) red_s[wave] = s;
  __syncthreads();
  if (tid == 0) {
    const float total = (red_s[0] + red_s[1]) + (red_s[2] + red_s[3]);
    const int xi = (int)(pos % ow), yi = (int)(pos / ow);
    // 4. the reference's fp32 expressions, one rounding per operation
    const float wc = bw / cw, hc = bh / ch;
    float x = ((float)xi + 0.5f) * wc;
    float y = ((float)yi + 0.5f) * hc;
    x = x + bx1;
    y = y + by1;
    float* o = out + ((size_t)m * K + k) * 4;
    o[0] = x;
    o[1] = y;
    o[2] = vmax;
    o[3] = expf(vmax - vmax) / total;
  }
}

extern "C" int lvc_heatmaps_to_keypoints(const float* maps, const float* rois, const int* d_num_valid, float* maps_out, float* out, int M,
                                         int K, int P, int up, void* stream) {
  LVC_CHECK_ARG(M >= 0 && K >= 1 && P >= 1, "M >= 0, K >= 1, P >= 1");
  LVC_CHECK_ARG(up == 1 || up == 2, "up: 1 or 2");
  LVC_CHECK_ARG(up * P <= KP_MAX_SIDE, "the heatmap side up * P is at most 64");
  if (M == 0) return LVC_OK;
  LVC_CHECK_ARG(maps && rois && out, "null pointer");
  LVC_CHECK_ARG((long long)M * K < (1LL << 31), "too many (RoI, keypoint) planes");
  hipLaunchKernelGGL(heatmaps_to_keypoints_kernel, dim3((unsigned)(M * K)), dim3(256), 0, (hipStream_t)stream, maps, rois, d_num_valid,
                     maps_out, out, M, K, P, up);
  LVC_CHECK_LAUNCH();
  return LVC_OK;
}
