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

// The one-workgroup selections (1024 threads, every digit pass inside one launch) search wider digits: up to 4096 bins, four
// per thread.  Bin d with  sum(h[0..d-1]) < krem <= sum(h[0..d]);  returns through sh[18] = d, sh[19] = sum(h[0..d-1]).
// `sh` holds >= 20 ints; nbins is a multiple of 4; 1 <= krem <= sum(h).  Starts with a barrier (the histogram's atomics).
__device__ __forceinline__ void find_bin_1024(const int* __restrict__ h, int nbins, int krem, int* sh) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  __syncthreads();
  int c[4] = {0, 0, 0, 0};
  if (tid * 4 < nbins) {
#pragma unroll
    for (int u = 0; u < 4; ++u) c[u] = h[tid * 4 + u];
  }
  const int s = c[0] + c[1] + c[2] + c[3];
  int incl = s;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(incl, o);
    if (lane >= o) incl += t;
  }
  if (lane == 63) sh[wave] = incl;
  __syncthreads();
  int excl = incl - s;
  for (int w = 0; w < wave; ++w) excl += sh[w];
  if (excl < krem && krem <= excl + s) {   // exactly one thread
    int u = 0;
    while (excl + c[u] < krem) { excl += c[u]; ++u; }
    sh[18] = tid * 4 + u;
    sh[19] = excl;
  }
  __syncthreads();
}

// The radix select of those kernels over keys that one workgroup can re-read cheaply (its own slice of L2, or LDS): the
// k-th smallest 32-bit key in three digit passes (12 + 12 + 8 bits).  `first` true: the 12-bit histogram of the top digit is
// already in hist[0 .. 4096).  Returns the threshold key T and how many keys EQUAL to T belong to the k smallest.
// hist holds >= 4096 ints.  Eight loads in flight per thread.
__device__ __forceinline__ void radix_select_1024(const unsigned int* keys, int n, int k, bool first, int* hist, int* sh,
                                                  unsigned int* T, int* need_eq) {
  const int tid = threadIdx.x;
  unsigned int prefix = 0, pmask = 0;
  int krem = k;
  for (int pass = 0; pass < 3; ++pass) {
    const int shift = pass == 0 ? 20 : pass == 1 ? 8 : 0, nb = pass == 2 ? 256 : 4096;
    if (pass > 0 || !first) {
      __syncthreads();
      for (int t = tid; t < nb; t += 1024) hist[t] = 0;
      __syncthreads();
      for (int i0 = tid; i0 < n; i0 += 8 * 1024) {
        unsigned int kv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) { const int i = i0 + u * 1024; kv[u] = i < n ? keys[i] : 0u; }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int i = i0 + u * 1024;
          if (i < n && (kv[u] & pmask) == prefix) atomicAdd(&hist[(kv[u] >> shift) & (nb - 1)], 1);
        }
      }
    }
    find_bin_1024(hist, nb, krem, sh);
    prefix |= (unsigned int)sh[18] << shift;
    pmask |= (unsigned int)(nb - 1) << shift;
    krem -= sh[19];
  }
  __syncthreads();
  *T = prefix;
  *need_eq = krem;
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
