// select_common.h -- what the top-k selections (boxes.hip: RPN proposals; retinanet.hip: per-level candidates) share: the
// order-preserving key, the LDS bitonic sort, the digit search of the radix select, and the box decode.
#pragma once
#include "common.h"

typedef unsigned long long u64;

__device__ __forceinline__ unsigned int desc_key(float f) {
  if (f == 0.f) f = 0.f;
  unsigned int u = __float_as_uint(f);
  u ^= (u >> 31) ? 0xFFFFFFFFu : 0x80000000u;
  return ~u;
}

template <typename T>
__device__ __forceinline__ void bitonic_sort_lds(T* keys, int npad) {
  for (int k = 2; k <= npad; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = threadIdx.x; t < npad / 2; t += blockDim.x) {
        int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1));
        int hi = lo | j;
        bool up = (lo & k) == 0;
        T a = keys[lo], b = keys[hi];
        if ((a > b) == up) { keys[lo] = b; keys[hi] = a; }
      }
      __syncthreads();
    }
  }
}

// first 256 threads: digit d with  sum(h[0..d-1]) < krem <= sum(h[0..d]);  returns through sh[8] = d, sh[9] = sum(h[0..d-1])
__device__ __forceinline__ void find_digit(const int* __restrict__ h, int krem, int* sh) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int x = 0, incl = 0;
  if (tid < 256) {
    x = h[tid];
    incl = x;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int t = __shfl_up(incl, o);
      if (lane >= o) incl += t;
    }
    if (lane == 63) sh[wave] = incl;
  }
  __syncthreads();
  if (tid < 256) {
    int off = 0;
    for (int w = 0; w < wave; ++w) off += sh[w];
    incl += off;
    if (incl - x < krem && krem <= incl) { sh[8] = tid; sh[9] = incl - x; }
  }
  __syncthreads();
}

// =====================================================================================
// shared decode (Box2BoxTransform.apply_deltas, box_regression.py:73-110)
// =====================================================================================
__device__ __forceinline__ void apply_deltas(float bx1, float by1, float bx2, float by2, float d0, float d1,
                                             float d2, float d3, float wx, float wy, float ww, float wh,
                                             float scale_clamp, float* o) {
  const float widths = bx2 - bx1, heights = by2 - by1;
  const float ctr_x = bx1 + 0.5f * widths, ctr_y = by1 + 0.5f * heights;
  const float dx = d0 / wx, dy = d1 / wy;
  float dw = d2 / ww, dh = d3 / wh;
  dw = dw > scale_clamp ? scale_clamp : dw;  // torch.clamp(max=): NaN stays NaN
  dh = dh > scale_clamp ? scale_clamp : dh;
  const float pcx = dx * widths + ctr_x, pcy = dy * heights + ctr_y;
  const float pw = expf(dw) * widths, ph = expf(dh) * heights;
  o[0] = pcx - 0.5f * pw; o[1] = pcy - 0.5f * ph; o[2] = pcx + 0.5f * pw; o[3] = pcy + 0.5f * ph;
}
