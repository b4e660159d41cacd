// sem_seg_train.hip -- training the semantic half of Panoptic FPN (reference detectron2/modeling/meta_arch/semantic_seg.py:179-187):
// the adjoint of the scale heads' bilinear x2 upsample, and F.interpolate(x COMMON_STRIDE) + F.cross_entropy(mean, ignore_index) with
// its gradient, neither of which forms the interpolated [N, K, H, W] tensor.  Declarations: include/lvc_amd_segtrain.h.
//
// Built without contraction (EXACT), with seg_bilinear.h's expression: the z of the loss are the bits lvcseg_sem_seg_postprocess writes
// as soft logits in the equal-size case.  No floating-point atomic anywhere: every sum below has one order, fixed by the indices.
#include <stdint.h>

#include "common.h"
#include "seg_bilinear.h"

// ------------------------------------------------------------------------------------------------ x2 upsample, backward
// The weight of input index i in output o of one axis: w0 where the first tap is i, plus w1 where the second is (both at a clamped
// border output).  `hit` is false where neither tap is i.
__device__ __forceinline__ float st_up2_weight(int o, int i, int size, bool* hit) {
  const SegTap t = seg_tap(0.5f, o, size);
  *hit = t.i0 == i || t.i1 == i;
  return (t.i0 == i ? t.w0 : 0.f) + (t.i1 == i ? t.w1 : 0.f);
}

// A thread owns four channels of one input pixel and gathers, rows then columns ascending, the outputs that tap it: 2i-1 .. 2i+2 of
// an axis, and output 0 also for i = 1 (its second tap, at weight 0, as the forward has it).
__global__ __launch_bounds__(256) void st_upsample2_bwd_kernel(const float4* __restrict__ dy, float4* __restrict__ dx, int H, int W, int C4,
                                                               long long total) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int c = (int)(i % C4);
  long long p = i / C4;
  const int ix = (int)(p % W);
  p /= W;
  const int iy = (int)(p % H);
  const long long n = p / H;
  const int OH = 2 * H, OW = 2 * W;
  const int y_lo = iy <= 1 ? 0 : 2 * iy - 1, y_hi = min(2 * iy + 2, OH - 1);
  const int x_lo = ix <= 1 ? 0 : 2 * ix - 1, x_hi = min(2 * ix + 2, OW - 1);
  const float4* dn = dy + n * OH * OW * C4 + c;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int oy = y_lo; oy <= y_hi; ++oy) {
    bool hit_y;
    const float l = st_up2_weight(oy, iy, H, &hit_y);
    if (!hit_y) continue;
    for (int ox = x_lo; ox <= x_hi; ++ox) {
      bool hit_x;
      const float m = st_up2_weight(ox, ix, W, &hit_x);
      if (!hit_x) continue;
      const float wgt = l * m;
      const float4 d = dn[((long long)oy * OW + ox) * C4];
      acc.x += wgt * d.x; acc.y += wgt * d.y; acc.z += wgt * d.z; acc.w += wgt * d.w;
    }
  }
  dx[i] = acc;
}

extern "C" int lvcst_upsample2_bilinear_bwd_nhwc(const float* dy, float* dx, int N, int H, int W, int C, void* stream) {
  LVC_CHECK_ARG(N >= 0 && H >= 1 && W >= 1 && C >= 4 && C % 4 == 0, "N >= 0, H, W >= 1, C a positive multiple of 4");
  LVC_CHECK_ARG(H < (1 << 20) && W < (1 << 20), "H, W below 2^20");
  if (N == 0) return LVC_OK;
  LVC_CHECK_ARG(dy && dx, "null pointer");
  LVC_CHECK_ARG((((uintptr_t)dy | (uintptr_t)dx) & 15) == 0, "16-byte aligned pointers");
  LVC_CHECK_ARG(dy != dx, "in place");
  const long long total = (long long)N * H * W * (C / 4);
  const long long blocks = (total + 255) / 256;
  LVC_CHECK_ARG(blocks < (1LL << 31), "too many workgroups");
  hipLaunchKernelGGL(st_upsample2_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const float4*)dy, (float4*)dx, H,
                     W, C / 4, total);
  LVC_CHECK_LAUNCH();
  return LVC_OK;
}

// ------------------------------------------------------------------------------------------------ loss: shared pieces
#define ST_THREADS 256
#define ST_LDS_BYTES (60 * 1024)

// The class of pixel (y, x) of image `jw`, or -1 where it adds nothing: outside the image's own map, `ignore`, or out of range (which
// raises the status bit where a status word is given).
template <typename LabelT>
__device__ __forceinline__ int st_target(const LabelT* __restrict__ labels, const long long* __restrict__ jw, int y, int x, long long ignore,
                                         int K, int* status) {
  const int lh = (int)jw[1], lw = (int)jw[2];
  if (y >= lh || x >= lw) return -1;
  const long long v = (long long)labels[jw[0] + (long long)y * lw + x];
  if (v == ignore) return -1;
  if (v < 0 || v >= K) {
    if (status) atomicOr(status, LVCST_STATUS_LABEL_RANGE);
    return -1;
  }
  return (int)v;
}

static int st_check_common(const char* fn, int N, int h, int w, int K, int ld, int scale, long long labels_numel, int label_bytes,
                           const long long* h_jobs) {
#define ST_ARG(cond, msg)                  \
  do {                                     \
    if (!(cond)) {                         \
      lvc_set_error("%s: %s", fn, msg);    \
      return LVC_ERR_INVALID;              \
    }                                      \
  } while (0)
  ST_ARG(N >= 0 && K >= 1 && K <= 4096 && ld >= K && scale >= 1 && scale <= 64, "N >= 0, 1 <= K <= 4096, ld >= K, 1 <= scale <= 64");
  ST_ARG(h >= 1 && w >= 1 && (long long)h * scale < (1 << 20) && (long long)w * scale < (1 << 20), "h, w >= 1, scale x h, w below 2^20");
  ST_ARG(label_bytes == 1 || label_bytes == 8, "label_bytes is 1 (uint8) or 8 (int64)");
  if (N == 0) return LVC_OK;
  ST_ARG(h_jobs, "null pointer");
  for (int i = 0; i < N; ++i) {
    const long long* jw = h_jobs + (size_t)i * LVCST_LOSS_FIELDS;
    ST_ARG(jw[1] >= 0 && jw[2] >= 0 && jw[1] <= (long long)h * scale && jw[2] <= (long long)w * scale, "a job's label map exceeds scale x the logits");
    ST_ARG(jw[0] >= 0 && jw[0] + jw[1] * jw[2] <= labels_numel, "a job's label map lies outside the buffer");
  }
#undef ST_ARG
  return LVC_OK;
}

// ------------------------------------------------------------------------------------------------ loss, forward
// A workgroup owns TH x TW pixels of the full-resolution map and stages their low-resolution footprint in LDS, K floats per pixel at
// an odd stride, as the postprocess kernel does (channels K .. ld-1 are never read).  Per pixel: max, sum of exponentials, lse; the
// labelled pixels add (double)(lse - z_t) to the thread's sum.  The workgroup's 256 sums and counts meet in a fixed tree.
// The backward is handed m and logf(sum) apart, not lse: fl(m + logf(sum)) has lost what the softmax needs where |m| is large (at
// |m| = 90 half an ulp is 3.8e-6, relative, in every probability), and (z - m) - logf(sum) has not -- torch's log_softmax forms the same.
template <typename LabelT>
__global__ __launch_bounds__(ST_THREADS) void st_loss_fwd_kernel(const float* __restrict__ logits, const long long* __restrict__ jobs,
                                                                 const LabelT* __restrict__ labels, long long ignore, int h, int w, int K,
                                                                 int ld, int scale, float rscale, int TH, int TW, int tiles_y, int tiles_x,
                                                                 int lds_pixels, float* __restrict__ mmax, float* __restrict__ lsum,
                                                                 float* __restrict__ lse, double* __restrict__ psum,
                                                                 long long* __restrict__ pcnt, int* status) {
  extern __shared__ __align__(16) float st_lds[];
  __shared__ double s_sum[ST_THREADS];
  __shared__ int s_cnt[ST_THREADS];
  const int tiles = tiles_y * tiles_x;
  const int n = blockIdx.x / tiles, blk = blockIdx.x - n * tiles;
  const int H = scale * h, W = scale * w;
  const int ty0 = (blk / tiles_x) * TH, tx0 = (blk % tiles_x) * TW;
  const int ty1 = min(ty0 + TH, H) - 1, tx1 = min(tx0 + TW, W) - 1;
  const int ylo = seg_tap(rscale, ty0, h).i0, yhi = seg_tap(rscale, ty1, h).i1;
  const int xlo = seg_tap(rscale, tx0, w).i0, xhi = seg_tap(rscale, tx1, w).i1;
  const int nrows = yhi - ylo + 1, ncols = xhi - xlo + 1;
  const int Kp = K | 1;
  double sum = 0.0;
  int cnt = 0;
  if (nrows * ncols <= lds_pixels) {      // (always: the host sized the LDS from these same spans)
    const float* low = logits + (long long)n * h * w * ld;
    for (int i = threadIdx.x; i < nrows * ncols * K; i += ST_THREADS) {
      const int k = i % K, pix = i / K;
      const int r = pix / ncols, c = pix - r * ncols;
      st_lds[pix * Kp + k] = low[((long long)(ylo + r) * w + (xlo + c)) * ld + k];
    }
    __syncthreads();
    const long long* jw = jobs + (size_t)n * LVCST_LOSS_FIELDS;
    const long long map_n = (long long)n * H * W;
    for (int p = threadIdx.x; p < TH * TW; p += ST_THREADS) {
      const int oy = ty0 + p / TW, ox = tx0 + p % TW;
      if (oy > ty1 || ox > tx1) continue;
      const SegTap ry = seg_tap(rscale, oy, h), rx = seg_tap(rscale, ox, w);
      const int ya0 = (ry.i0 - ylo) * ncols, ya1 = (ry.i1 - ylo) * ncols, xa0 = rx.i0 - xlo, xa1 = rx.i1 - xlo;
      const float* A = st_lds + (ya0 + xa0) * Kp;
      const float* B = st_lds + (ya0 + xa1) * Kp;
      const float* C = st_lds + (ya1 + xa0) * Kp;
      const float* D = st_lds + (ya1 + xa1) * Kp;
      float m = seg_bilerp(ry.w0, ry.w1, rx.w0, rx.w1, A[0], B[0], C[0], D[0]);
      for (int k = 1; k < K; ++k) {
        const float v = seg_bilerp(ry.w0, ry.w1, rx.w0, rx.w1, A[k], B[k], C[k], D[k]);
        m = v > m ? v : m;
      }
      float s = 0.f;
      for (int k = 0; k < K; ++k) s += expf(seg_bilerp(ry.w0, ry.w1, rx.w0, rx.w1, A[k], B[k], C[k], D[k]) - m);
      const float ls = logf(s), l = m + ls;
      const long long at = map_n + (long long)oy * W + ox;
      mmax[at] = m;
      lsum[at] = ls;
      if (lse) lse[at] = l;
      const int t = st_target(labels, jw, oy, ox, ignore, K, status);
      if (t >= 0) {
        const float zt = seg_bilerp(ry.w0, ry.w1, rx.w0, rx.w1, A[t], B[t], C[t], D[t]);
        sum += (double)(l - zt);
        ++cnt;
      }
    }
  }
  s_sum[threadIdx.x] = sum;
  s_cnt[threadIdx.x] = cnt;
  __syncthreads();
  for (int s = ST_THREADS / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      s_sum[threadIdx.x] += s_sum[threadIdx.x + s];
      s_cnt[threadIdx.x] += s_cnt[threadIdx.x + s];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    psum[blockIdx.x] = s_sum[0];
    pcnt[blockIdx.x] = (long long)s_cnt[0];
  }
}

// One workgroup: thread t adds the partials t, t + 256, .. in that order, then the same tree.
__global__ __launch_bounds__(ST_THREADS) void st_loss_finish_kernel(const double* __restrict__ psum, const long long* __restrict__ pcnt,
                                                                    long long blocks, float* loss, double* sum, long long* count) {
  __shared__ double s_sum[ST_THREADS];
  __shared__ long long s_cnt[ST_THREADS];
  double a = 0.0;
  long long c = 0;
  for (long long i = threadIdx.x; i < blocks; i += ST_THREADS) {
    a += psum[i];
    c += pcnt[i];
  }
  s_sum[threadIdx.x] = a;
  s_cnt[threadIdx.x] = c;
  __syncthreads();
  for (int s = ST_THREADS / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      s_sum[threadIdx.x] += s_sum[threadIdx.x + s];
      s_cnt[threadIdx.x] += s_cnt[threadIdx.x + s];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    *sum = s_sum[0];
    *count = s_cnt[0];
    *loss = (float)(s_sum[0] / (double)s_cnt[0]);      // 0 / 0: NaN, as F.cross_entropy gives with no valid pixel
  }
}

struct StFwdPlan {
  int TH, TW, tiles_y, tiles_x, px;
};

// the largest tile (from 16 x 64 down) whose largest footprint fits the LDS budget; px < 0: not even one pixel's does
static StFwdPlan st_fwd_plan(int h, int w, int K, int scale) {
  const float rscale = (float)(1.0 / (double)scale);      // ATen: static_cast<float>(1.0 / scale_factor)
  const int H = scale * h, W = scale * w, Kp = K | 1;
  StFwdPlan p;
  p.TH = 16;
  p.TW = 64;
  for (;;) {
    int rows = 0, cols = 0;
    for (int y0 = 0; y0 < H; y0 += p.TH) {
      const int y1 = (y0 + p.TH < H ? y0 + p.TH : H) - 1;
      const int n = seg_tap(rscale, y1, h).i1 - seg_tap(rscale, y0, h).i0 + 1;
      if (n > rows) rows = n;
    }
    for (int x0 = 0; x0 < W; x0 += p.TW) {
      const int x1 = (x0 + p.TW < W ? x0 + p.TW : W) - 1;
      const int n = seg_tap(rscale, x1, w).i1 - seg_tap(rscale, x0, w).i0 + 1;
      if (n > cols) cols = n;
    }
    p.px = rows * cols;
    if ((long long)p.px * Kp * 4 <= ST_LDS_BYTES) break;
    if (p.TH * p.TW == 1) {
      p.px = -1;
      break;
    }
    if (p.TW > p.TH) p.TW /= 2; else p.TH /= 2;
  }
  p.tiles_y = (H + p.TH - 1) / p.TH;
  p.tiles_x = (W + p.TW - 1) / p.TW;
  return p;
}

extern "C" long long lvcst_sem_seg_loss_workspace_bytes(int N, int h, int w, int K, int scale) {
  if (N < 0 || h < 1 || w < 1 || K < 1 || K > 4096 || scale < 1 || scale > 64 || (long long)h * scale >= (1 << 20) ||
      (long long)w * scale >= (1 << 20))
    return -1;
  const StFwdPlan p = st_fwd_plan(h, w, K, scale);
  if (p.px < 0) return -1;
  return (long long)N * p.tiles_y * p.tiles_x * 16;
}

extern "C" int lvcst_sem_seg_loss_fwd(const float* logits, int N, int h, int w, int K, int ld, int scale, const void* labels,
                                      long long labels_numel, int label_bytes, long long ignore_value, const long long* h_jobs,
                                      const long long* d_jobs, float* mmax, float* lsum, float* lse, void* workspace,
                                      long long workspace_bytes, float* loss, double* sum, long long* count, int* status, void* stream) {
  const int st = st_check_common(__func__, N, h, w, K, ld, scale, labels_numel, label_bytes, h_jobs);
  if (st != LVC_OK) return st;
  LVC_CHECK_ARG(loss && sum && count && status, "null pointer");
  LVC_CHECK_ARG((((uintptr_t)workspace | (uintptr_t)sum | (uintptr_t)count) & 7) == 0, "8-byte aligned workspace, sum and count");
  const StFwdPlan p = st_fwd_plan(h, w, K, scale);
  LVC_CHECK_ARG(p.px >= 0, "the footprint of one output pixel exceeds the LDS budget");
  const long long blocks = (long long)N * p.tiles_y * p.tiles_x;
  LVC_CHECK_ARG(blocks < (1LL << 31), "too many workgroups");
  LVC_CHECK_ARG(workspace_bytes >= blocks * 16, "workspace too small");
  double* psum = reinterpret_cast<double*>(workspace);
  long long* pcnt = reinterpret_cast<long long*>(psum + blocks);
  if (N > 0) {
    LVC_CHECK_ARG(logits && d_jobs && mmax && lsum && workspace && (labels || labels_numel == 0), "null pointer");
    const float rscale = (float)(1.0 / (double)scale);
    const dim3 grid((unsigned)blocks), block(ST_THREADS);
    const size_t lds = (size_t)p.px * (K | 1) * 4;
    if (label_bytes == 1)
      hipLaunchKernelGGL(st_loss_fwd_kernel<unsigned char>, grid, block, lds, (hipStream_t)stream, logits, d_jobs, (const unsigned char*)labels,
                         ignore_value, h, w, K, ld, scale, rscale, p.TH, p.TW, p.tiles_y, p.tiles_x, p.px, mmax, lsum, lse, psum, pcnt, status);
    else
      hipLaunchKernelGGL(st_loss_fwd_kernel<long long>, grid, block, lds, (hipStream_t)stream, logits, d_jobs, (const long long*)labels,
                         ignore_value, h, w, K, ld, scale, rscale, p.TH, p.TW, p.tiles_y, p.tiles_x, p.px, mmax, lsum, lse, psum, pcnt, status);
    LVC_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(st_loss_finish_kernel, dim3(1), dim3(ST_THREADS), 0, (hipStream_t)stream, psum, pcnt, blocks, loss, sum, count);
  LVC_CHECK_LAUNCH();
  return LVC_OK;
}

// ------------------------------------------------------------------------------------------------ loss, backward
// The full-resolution outputs [*lo, *hi] of one axis whose taps touch the low-resolution indices [i0, i1].  Both taps are non-decreasing
// in the output, so the set is a range; the closed form is the start (at scale 4: 4 i0 - 2 .. 4 i1 + 5) and the taps themselves decide,
// so the range is exact whatever the rounding of (float)(1 / scale).
__host__ __device__ __forceinline__ void st_outputs_of(int i0, int i1, int scale, float rscale, int low, int* lo, int* hi) {
  const int out = scale * low;
  int a = scale * i0 - scale / 2 - 1, b = scale * i1 + (3 * scale) / 2;
  a = a < 0 ? 0 : (a > out - 1 ? out - 1 : a);
  b = b < 0 ? 0 : (b > out - 1 ? out - 1 : b);
  while (a > 0 && seg_tap(rscale, a - 1, low).i1 >= i0) --a;
  while (a < out - 1 && seg_tap(rscale, a, low).i1 < i0) ++a;
  while (b < out - 1 && seg_tap(rscale, b + 1, low).i0 <= i1) ++b;
  while (b > 0 && seg_tap(rscale, b, low).i0 > i1) --b;
  *lo = a;
  *hi = b;
}

// A workgroup owns LH x LW low-resolution pixels.  In LDS: the logits of the pixels its outputs tap (the tile and a halo of one), and,
// where it fits (`staged`), max, log-sum and class of every output that taps the tile.  A thread owns one (pixel, channel): it walks the
// pixel's outputs rows then columns ascending, recomputes z, and adds (l m) (expf((z - max) - logsum) - [k == t]); the sum times
// g / count is written once.
template <typename LabelT>
__global__ __launch_bounds__(ST_THREADS) void st_loss_bwd_kernel(const float* __restrict__ logits, const long long* __restrict__ jobs,
                                                                 const LabelT* __restrict__ labels, long long ignore, int h, int w, int K,
                                                                 int ld, int scale, float rscale, int LH, int LW, int tiles_y, int tiles_x,
                                                                 int lds_pixels, int region_pixels, int staged,
                                                                 const float* __restrict__ mmax, const float* __restrict__ lsum,
                                                                 const float* __restrict__ g, const long long* __restrict__ count,
                                                                 float* __restrict__ dlow) {
  extern __shared__ __align__(16) float st_lds[];
  const int tiles = tiles_y * tiles_x;
  const int n = blockIdx.x / tiles, blk = blockIdx.x - n * tiles;
  const int H = scale * h, W = scale * w;
  const int i0 = (blk / tiles_x) * LH, j0 = (blk % tiles_x) * LW;
  const int i1 = min(i0 + LH, h) - 1, j1 = min(j0 + LW, w) - 1;
  int ylo, yhi, xlo, xhi;
  st_outputs_of(i0, i1, scale, rscale, h, &ylo, &yhi);
  st_outputs_of(j0, j1, scale, rscale, w, &xlo, &xhi);
  const int flo_y = seg_tap(rscale, ylo, h).i0, fhi_y = seg_tap(rscale, yhi, h).i1;
  const int flo_x = seg_tap(rscale, xlo, w).i0, fhi_x = seg_tap(rscale, xhi, w).i1;
  const int frows = fhi_y - flo_y + 1, fcols = fhi_x - flo_x + 1;
  const int ry = yhi - ylo + 1, rx = xhi - xlo + 1;
  const int Kp = K | 1;
  const int th = i1 - i0 + 1, tw = j1 - j0 + 1;
  float* dl = dlow + (long long)n * h * w * ld;
  if (frows * fcols > lds_pixels || (staged && ry * rx > region_pixels)) return;      // (never: the host sized both from these spans)
  const float* low = logits + (long long)n * h * w * ld;
  for (int i = threadIdx.x; i < frows * fcols * K; i += ST_THREADS) {
    const int k = i % K, pix = i / K;
    const int r = pix / fcols, c = pix - r * fcols;
    st_lds[pix * Kp + k] = low[((long long)(flo_y + r) * w + (flo_x + c)) * ld + k];
  }
  const long long* jw = jobs + (size_t)n * LVCST_LOSS_FIELDS;
  const float* max_n = mmax + (long long)n * H * W;
  const float* sum_n = lsum + (long long)n * H * W;
  float* r_max = st_lds + (size_t)lds_pixels * Kp;
  float* r_sum = r_max + region_pixels;
  int* r_t = reinterpret_cast<int*>(r_sum + region_pixels);
  if (staged) {
    for (int p = threadIdx.x; p < ry * rx; p += ST_THREADS) {
      const int y = ylo + p / rx, x = xlo + p % rx;
      r_max[p] = max_n[(long long)y * W + x];
      r_sum[p] = sum_n[(long long)y * W + x];
      r_t[p] = st_target(labels, jw, y, x, ignore, K, (int*)nullptr);
    }
  }
  __syncthreads();
  const float coef = g[0] / (float)count[0];
  for (int it = threadIdx.x; it < th * tw * ld; it += ST_THREADS) {
    const int k = it % ld, pix = it / ld;
    const int i = i0 + pix / tw, j = j0 + pix % tw;
    float acc = 0.f;
    if (k < K) {
      int yl, yh, xl, xh;
      st_outputs_of(i, i, scale, rscale, h, &yl, &yh);
      st_outputs_of(j, j, scale, rscale, w, &xl, &xh);
      for (int y = yl; y <= yh; ++y) {
        const SegTap ty = seg_tap(rscale, y, h);
        const float l = (ty.i0 == i ? ty.w0 : 0.f) + (ty.i1 == i ? ty.w1 : 0.f);
        const float* Ly0 = st_lds + (ty.i0 - flo_y) * fcols * Kp + k;
        const float* Ly1 = st_lds + (ty.i1 - flo_y) * fcols * Kp + k;
        for (int x = xl; x <= xh; ++x) {
          float M, S;
          int t;
          if (staged) {
            const int p = (y - ylo) * rx + (x - xlo);
            M = r_max[p];
            S = r_sum[p];
            t = r_t[p];
          } else {
            M = max_n[(long long)y * W + x];
            S = sum_n[(long long)y * W + x];
            t = st_target(labels, jw, y, x, ignore, K, (int*)nullptr);
          }
          if (t < 0) continue;
          const SegTap tx = seg_tap(rscale, x, w);
          const float m = (tx.i0 == j ? tx.w0 : 0.f) + (tx.i1 == j ? tx.w1 : 0.f);
          const int xa0 = (tx.i0 - flo_x) * Kp, xa1 = (tx.i1 - flo_x) * Kp;
          const float z = seg_bilerp(ty.w0, ty.w1, tx.w0, tx.w1, Ly0[xa0], Ly0[xa1], Ly1[xa0], Ly1[xa1]);
          float e = expf((z - M) - S);
          if (k == t) e -= 1.f;
          acc += (l * m) * e;
        }
      }
      acc *= coef;
    }
    dl[((long long)i * w + j) * ld + k] = acc;
  }
}

struct StBwdPlan {
  int LH, LW, tiles_y, tiles_x, px, region, staged;
};

// the largest tile (from 8 x 8 down) whose logits footprint and output region fit the LDS budget together; at 1 x 1 the region may stay
// in memory (staged = 0); px < 0: not even one pixel's logits footprint fits
static StBwdPlan st_bwd_plan(int h, int w, int K, int scale) {
  const float rscale = (float)(1.0 / (double)scale);
  const int Kp = K | 1;
  StBwdPlan p;
  p.LH = 8;
  p.LW = 8;
  p.staged = 1;
  for (;;) {
    int rows = 0, cols = 0, ry = 0, rx = 0, lo, hi;
    for (int a = 0; a < h; a += p.LH) {
      const int b = (a + p.LH < h ? a + p.LH : h) - 1;
      st_outputs_of(a, b, scale, rscale, h, &lo, &hi);
      const int n = seg_tap(rscale, hi, h).i1 - seg_tap(rscale, lo, h).i0 + 1;
      if (n > rows) rows = n;
      if (hi - lo + 1 > ry) ry = hi - lo + 1;
    }
    for (int a = 0; a < w; a += p.LW) {
      const int b = (a + p.LW < w ? a + p.LW : w) - 1;
      st_outputs_of(a, b, scale, rscale, w, &lo, &hi);
      const int n = seg_tap(rscale, hi, w).i1 - seg_tap(rscale, lo, w).i0 + 1;
      if (n > cols) cols = n;
      if (hi - lo + 1 > rx) rx = hi - lo + 1;
    }
    p.px = rows * cols;
    p.region = ry * rx;
    if ((long long)p.px * Kp * 4 + (long long)p.region * 12 <= ST_LDS_BYTES) break;
    if (p.LH * p.LW == 1) {
      p.staged = 0;
      p.region = 0;
      if ((long long)p.px * Kp * 4 > ST_LDS_BYTES) p.px = -1;
      break;
    }
    if (p.LW > p.LH) p.LW /= 2; else p.LH /= 2;
  }
  p.tiles_y = (h + p.LH - 1) / p.LH;
  p.tiles_x = (w + p.LW - 1) / p.LW;
  return p;
}

extern "C" int lvcst_sem_seg_loss_bwd(const float* logits, int N, int h, int w, int K, int ld, int scale, const void* labels,
                                      long long labels_numel, int label_bytes, long long ignore_value, const long long* h_jobs,
                                      const long long* d_jobs, const float* mmax, const float* lsum, const float* g,
                                      const long long* count, float* dlow, void* stream) {
  const int st = st_check_common(__func__, N, h, w, K, ld, scale, labels_numel, label_bytes, h_jobs);
  if (st != LVC_OK) return st;
  if (N == 0) return LVC_OK;
  LVC_CHECK_ARG(logits && d_jobs && mmax && lsum && g && count && dlow && (labels || labels_numel == 0), "null pointer");
  LVC_CHECK_ARG(logits != dlow, "in place");
  const StBwdPlan p = st_bwd_plan(h, w, K, scale);
  LVC_CHECK_ARG(p.px >= 0, "the footprint of one low-resolution pixel exceeds the LDS budget");
  const long long blocks = (long long)N * p.tiles_y * p.tiles_x;
  LVC_CHECK_ARG(blocks < (1LL << 31), "too many workgroups");
  const float rscale = (float)(1.0 / (double)scale);
  const dim3 grid((unsigned)blocks), block(ST_THREADS);
  const size_t lds = (size_t)p.px * (K | 1) * 4 + (size_t)p.region * 12;
  if (label_bytes == 1)
    hipLaunchKernelGGL(st_loss_bwd_kernel<unsigned char>, grid, block, lds, (hipStream_t)stream, logits, d_jobs, (const unsigned char*)labels,
                       ignore_value, h, w, K, ld, scale, rscale, p.LH, p.LW, p.tiles_y, p.tiles_x, p.px, p.region, p.staged, mmax, lsum, g, count,
                       dlow);
  else
    hipLaunchKernelGGL(st_loss_bwd_kernel<long long>, grid, block, lds, (hipStream_t)stream, logits, d_jobs, (const long long*)labels,
                       ignore_value, h, w, K, ld, scale, rscale, p.LH, p.LW, p.tiles_y, p.tiles_x, p.px, p.region, p.staged, mmax, lsum, g, count,
                       dlow);
  LVC_CHECK_LAUNCH();
  return LVC_OK;
}
