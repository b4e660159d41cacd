// sem_seg.hip -- the semantic half of Panoptic FPN (reference detectron2/modeling/meta_arch/semantic_seg.py, panoptic_fpn.py,
// postprocessing.py:82-105): the bilinear x2 upsample of the scale heads, the head's x`COMMON_STRIDE` upsample + sem_seg_postprocess +
// argmax in one kernel, and combine_semantic_and_instance_outputs for a batch.  Declarations: include/lvc_amd_seg.h.
//
// Built without contraction (EXACT): every fp32 expression below rounds as written, and tests/seg_ref.py restates them bit for bit.
// One bilinear expression serves all three interpolations (rows weigh l, columns m):
//   v = l0 (m0 a + m1 b) + l1 (m0 c + m1 d)
// with ATen's coordinates for align_corners=False: s = max(scale (d + 0.5) - 0.5, 0), i0 = (int)s, i1 = i0 + (i0 < size - 1),
// w1 = s - i0, w0 = 1 - w1.
#include <stdint.h>

#include "common.h"
#include "seg_bilinear.h"      // SegTap, seg_tap, seg_bilerp: shared with sem_seg_train.hip

// ------------------------------------------------------------------------------------------------ x2 upsample (+ accumulator)
// A thread owns four channels of one output pixel: four 16-byte loads (L2 serves the re-reads of the 2x2 neighbourhood), one 16-byte
// load of the accumulator, one 16-byte store.
__global__ __launch_bounds__(256) void seg_upsample2_kernel(const float4* __restrict__ x, const float4* acc, float4* y, int H, int W,
                                                            int C4, long long total) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int c = (int)(i % C4);
  long long p = i / C4;
  const int ox = (int)(p % (2 * W));
  p /= 2 * W;
  const int oy = (int)(p % (2 * H));
  const long long n = p / (2 * H);
  const SegTap ty = seg_tap(0.5f, oy, H), tx = seg_tap(0.5f, ox, W);
  const float4* xn = x + n * H * W * C4 + c;
  const float4 a = xn[((long long)ty.i0 * W + tx.i0) * C4], b = xn[((long long)ty.i0 * W + tx.i1) * C4];
  const float4 cc = xn[((long long)ty.i1 * W + tx.i0) * C4], d = xn[((long long)ty.i1 * W + tx.i1) * C4];
  float4 v;
  v.x = seg_bilerp(ty.w0, ty.w1, tx.w0, tx.w1, a.x, b.x, cc.x, d.x);
  v.y = seg_bilerp(ty.w0, ty.w1, tx.w0, tx.w1, a.y, b.y, cc.y, d.y);
  v.z = seg_bilerp(ty.w0, ty.w1, tx.w0, tx.w1, a.z, b.z, cc.z, d.z);
  v.w = seg_bilerp(ty.w0, ty.w1, tx.w0, tx.w1, a.w, b.w, cc.w, d.w);
  if (acc) {      // added last: ((p2 + p3') + p4') + p5' is the reference's order of the level sum
    const float4 r = acc[i];
    v.x = r.x + v.x; v.y = r.y + v.y; v.z = r.z + v.z; v.w = r.w + v.w;
  }
  y[i] = v;
}

extern "C" int lvcseg_upsample2_bilinear_nhwc(const float* x, const float* acc, float* y, int N, int H, int W, int C, void* stream) {
  LVC_CHECK_ARG(N >= 0 && H >= 1 && W >= 1 && C >= 4 && C % 4 == 0, "N >= 0, H, W >= 1, C a positive multiple of 4");
  LVC_CHECK_ARG(H < (1 << 20) && W < (1 << 20), "H, W below 2^20");
  if (N == 0) return LVC_OK;
  LVC_CHECK_ARG(x && y, "null pointer");
  LVC_CHECK_ARG((((uintptr_t)x | (uintptr_t)acc | (uintptr_t)y) & 15) == 0, "16-byte aligned pointers");
  LVC_CHECK_ARG(x != y, "in place: y may be acc, not x");
  const long long total = (long long)N * 2 * H * 2 * W * (C / 4);
  const long long blocks = (total + 255) / 256;
  LVC_CHECK_ARG(blocks < (1LL << 31), "too many workgroups");
  hipLaunchKernelGGL(seg_upsample2_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const float4*)x, (const float4*)acc,
                     (float4*)y, H, W, C / 4, total);
  LVC_CHECK_LAUNCH();
  return LVC_OK;
}

// ------------------------------------------------------------------------------------------------ postprocess + argmax
// A workgroup of 256 threads owns an output tile of TH rows x TW columns (TW a lane per column where it is 64: a wave stores 256
// contiguous bytes of a soft plane, 64 of the label map).  It stages the low-resolution footprint of the tile -- every low-resolution
// pixel one of its output pixels can tap through both interpolations -- in LDS, K floats per pixel at an odd stride, and never reads
// channels K .. ld-1.  At scale 4 and equal sizes a 16 x 64 tile taps 6 x 18 low-resolution pixels: 108 x 55 floats = 23 KB for 54
// classes.  A strong downscale widens the footprint; the host halves the tile until the largest footprint of the launch fits.
#define SP_THREADS 256
#define SP_LDS_BYTES (60 * 1024)

struct SegJob {
  long long low_off, soft_off, label_off;
  int h, w, ih, iw, oh, ow;
};

__host__ __device__ __forceinline__ SegJob seg_job(const long long* jw) {
  SegJob j;
  j.low_off = jw[0]; j.h = (int)jw[1]; j.w = (int)jw[2]; j.ih = (int)jw[3]; j.iw = (int)jw[4]; j.oh = (int)jw[5]; j.ow = (int)jw[6];
  j.soft_off = jw[7]; j.label_off = jw[8];
  return j;
}

// The low-resolution rows (or columns) [lo, hi] that the outputs d0 .. d1 of one axis tap.  Both source indices are non-decreasing in d
// (a positive scale, rounded monotonically), so the first output gives lo and the last gives hi.
__host__ __device__ __forceinline__ void seg_span(int d0, int d1, int out, int img, int low, float rscale, int* lo, int* hi) {
  int a = d0, b = d1;
  if (out != img) {
    const float s2 = (float)img / (float)out;
    a = seg_tap(s2, d0, img).i0;
    b = seg_tap(s2, d1, img).i1;
  }
  *lo = seg_tap(rscale, a, low).i0;
  *hi = seg_tap(rscale, b, low).i1;
}

template <typename LabelT>
__global__ __launch_bounds__(SP_THREADS) void seg_postprocess_kernel(const float* __restrict__ logits, const long long* __restrict__ jobs,
                                                                     int K, int ld, float rscale, float* __restrict__ soft,
                                                                     LabelT* __restrict__ labels, int TH, int TW, int blocks_per_job,
                                                                     int lds_pixels) {
  extern __shared__ __align__(16) float sp_lds[];
  const int job = blockIdx.x / blocks_per_job;
  const int blk = blockIdx.x - job * blocks_per_job;
  const SegJob jb = seg_job(jobs + (size_t)job * LVCSEG_POST_FIELDS);
  const int tiles_x = (jb.ow + TW - 1) / TW, tiles_y = (jb.oh + TH - 1) / TH;
  if (blk >= tiles_x * tiles_y) return;      // (the whole workgroup: blk is uniform)
  const int ty0 = (blk / tiles_x) * TH, tx0 = (blk % tiles_x) * TW;
  const int ty1 = min(ty0 + TH, jb.oh) - 1, tx1 = min(tx0 + TW, jb.ow) - 1;
  int ylo, yhi, xlo, xhi;
  seg_span(ty0, ty1, jb.oh, jb.ih, jb.h, rscale, &ylo, &yhi);
  seg_span(tx0, tx1, jb.ow, jb.iw, jb.w, rscale, &xlo, &xhi);
  const int nrows = yhi - ylo + 1, ncols = xhi - xlo + 1;
  if (nrows * ncols > lds_pixels) return;      // (the host sized the LDS from these same spans; never taken)
  const int Kp = K | 1;
  const float* low = logits + jb.low_off;
  for (int i = threadIdx.x; i < nrows * ncols * K; i += SP_THREADS) {
    const int k = i % K, pix = i / K;
    const int r = pix / ncols, c = pix - r * ncols;
    sp_lds[pix * Kp + k] = low[((long long)(ylo + r) * jb.w + (xlo + c)) * ld + k];
  }
  __syncthreads();

  const bool ident_y = jb.oh == jb.ih, ident_x = jb.ow == jb.iw;
  const float s2y = (float)jb.ih / (float)jb.oh, s2x = (float)jb.iw / (float)jb.ow;
  const long long plane = (long long)jb.oh * jb.ow;
  for (int p = threadIdx.x; p < TH * TW; p += SP_THREADS) {
    const int oy = ty0 + p / TW, ox = tx0 + p % TW;
    if (oy > ty1 || ox > tx1) continue;
    // second stage (image -> output): two image rows and two image columns, or one of each where the sizes agree
    SegTap qy, qx;
    if (ident_y) { qy.i0 = qy.i1 = oy; qy.w0 = 1.f; qy.w1 = 0.f; } else qy = seg_tap(s2y, oy, jb.ih);
    if (ident_x) { qx.i0 = qx.i1 = ox; qx.w0 = 1.f; qx.w1 = 0.f; } else qx = seg_tap(s2x, ox, jb.iw);
    // first stage (low resolution -> x scale) of those rows and columns; LDS offsets relative to the footprint
    const SegTap ry0 = seg_tap(rscale, qy.i0, jb.h), ry1 = seg_tap(rscale, qy.i1, jb.h);
    const SegTap rx0 = seg_tap(rscale, qx.i0, jb.w), rx1 = seg_tap(rscale, qx.i1, jb.w);
    const int ya0 = (ry0.i0 - ylo) * ncols, ya1 = (ry0.i1 - ylo) * ncols, yb0 = (ry1.i0 - ylo) * ncols, yb1 = (ry1.i1 - ylo) * ncols;
    const int xa0 = rx0.i0 - xlo, xa1 = rx0.i1 - xlo, xb0 = rx1.i0 - xlo, xb1 = rx1.i1 - xlo;
    float best = 0.f;
    int arg = 0;
    const long long at = (long long)oy * jb.ow + ox;
    for (int k = 0; k < K; ++k) {
      const float* L = sp_lds + k;
#define SP_AT(yo, xo) L[((yo) + (xo)) * Kp]
      float v = seg_bilerp(ry0.w0, ry0.w1, rx0.w0, rx0.w1, SP_AT(ya0, xa0), SP_AT(ya0, xa1), SP_AT(ya1, xa0), SP_AT(ya1, xa1));
      if (!(ident_y && ident_x)) {
        const float v01 = seg_bilerp(ry0.w0, ry0.w1, rx1.w0, rx1.w1, SP_AT(ya0, xb0), SP_AT(ya0, xb1), SP_AT(ya1, xb0), SP_AT(ya1, xb1));
        const float v10 = seg_bilerp(ry1.w0, ry1.w1, rx0.w0, rx0.w1, SP_AT(yb0, xa0), SP_AT(yb0, xa1), SP_AT(yb1, xa0), SP_AT(yb1, xa1));
        const float v11 = seg_bilerp(ry1.w0, ry1.w1, rx1.w0, rx1.w1, SP_AT(yb0, xb0), SP_AT(yb0, xb1), SP_AT(yb1, xb0), SP_AT(yb1, xb1));
        v = seg_bilerp(qy.w0, qy.w1, qx.w0, qx.w1, v, v01, v10, v11);
      }
#undef SP_AT
      if (soft) soft[jb.soft_off + k * plane + at] = v;
      if (k == 0 || v > best) { best = v; arg = k; }      // strictly greater: the lowest class wins on equal values
    }
    if (labels) labels[jb.label_off + at] = (LabelT)arg;
  }
}

// (tile, LDS pixels) for one launch: the largest tile whose largest footprint over all jobs fits the LDS budget
static int sp_footprint(const long long* h_jobs, int num_jobs, float rscale, int TH, int TW) {
  int worst = 0;
  for (int i = 0; i < num_jobs; ++i) {
    const SegJob jb = seg_job(h_jobs + (size_t)i * LVCSEG_POST_FIELDS);
    int rows = 0, cols = 0, lo, hi;
    for (int y0 = 0; y0 < jb.oh; y0 += TH) {
      const int y1 = (y0 + TH < jb.oh ? y0 + TH : jb.oh) - 1;
      seg_span(y0, y1, jb.oh, jb.ih, jb.h, rscale, &lo, &hi);
      if (hi - lo + 1 > rows) rows = hi - lo + 1;
    }
    for (int x0 = 0; x0 < jb.ow; x0 += TW) {
      const int x1 = (x0 + TW < jb.ow ? x0 + TW : jb.ow) - 1;
      seg_span(x0, x1, jb.ow, jb.iw, jb.w, rscale, &lo, &hi);
      if (hi - lo + 1 > cols) cols = hi - lo + 1;
    }
    if (rows * cols > worst) worst = rows * cols;
  }
  return worst;
}

extern "C" int lvcseg_sem_seg_postprocess(const float* logits, long long logits_numel, const long long* h_jobs, const long long* d_jobs,
                                          int num_jobs, int K, int ld, int scale, float* soft, long long soft_numel, void* labels,
                                          long long labels_numel, int label_bytes, void* stream) {
  LVC_CHECK_ARG(num_jobs >= 0 && K >= 1 && K <= 4096 && ld >= K && scale >= 1 && scale <= 64, "num_jobs >= 0, 1 <= K <= 4096, ld >= K, 1 <= scale <= 64");
  LVC_CHECK_ARG(label_bytes == 1 || label_bytes == 4, "label_bytes is 1 (uint8) or 4 (int32)");
  LVC_CHECK_ARG(!labels || label_bytes == 4 || K <= 256, "more than 256 classes need int32 labels");
  LVC_CHECK_ARG(soft || labels, "neither output requested");
  if (num_jobs == 0) return LVC_OK;
  LVC_CHECK_ARG(logits && h_jobs && d_jobs, "null pointer");
  long long max_tiles_px = 0;
  for (int i = 0; i < num_jobs; ++i) {
    const long long* jw = h_jobs + (size_t)i * LVCSEG_POST_FIELDS;
    LVC_CHECK_ARG(jw[1] >= 1 && jw[2] >= 1 && jw[1] < (1 << 20) && jw[2] < (1 << 20), "a job's low-resolution size");
    LVC_CHECK_ARG(jw[0] >= 0 && jw[0] + jw[1] * jw[2] * (long long)ld <= logits_numel, "a job's logits lie outside the buffer");
    LVC_CHECK_ARG(jw[3] >= 1 && jw[4] >= 1 && jw[3] <= jw[1] * scale && jw[4] <= jw[2] * scale, "a job's image size exceeds scale x its logits");
    LVC_CHECK_ARG(jw[5] >= 1 && jw[6] >= 1 && jw[5] < (1 << 20) && jw[6] < (1 << 20), "a job's output size");
    const long long hw = jw[5] * jw[6];
    LVC_CHECK_ARG(!soft || (jw[7] >= 0 && jw[7] + (long long)K * hw <= soft_numel), "a job's soft plane lies outside the buffer");
    LVC_CHECK_ARG(!labels || (jw[8] >= 0 && jw[8] + hw <= labels_numel), "a job's label map lies outside the buffer");
    if (hw > max_tiles_px) max_tiles_px = hw;
  }
  const float rscale = (float)(1.0 / (double)scale);      // ATen: static_cast<float>(1.0 / scale_factor)
  const int Kp = K | 1;
  int TH = 16, TW = 64, px;
  while ((long long)(px = sp_footprint(h_jobs, num_jobs, rscale, TH, TW)) * Kp * 4 > SP_LDS_BYTES && TH * TW > 1) {
    if (TW > TH) TW /= 2; else TH /= 2;
  }
  LVC_CHECK_ARG((long long)px * Kp * 4 <= SP_LDS_BYTES, "the footprint of one output pixel exceeds the LDS budget");
  long long bpj = 0;
  for (int i = 0; i < num_jobs; ++i) {
    const long long* jw = h_jobs + (size_t)i * LVCSEG_POST_FIELDS;
    const long long t = ((jw[5] + TH - 1) / TH) * ((jw[6] + TW - 1) / TW);
    if (t > bpj) bpj = t;
  }
  LVC_CHECK_ARG(bpj * num_jobs < (1LL << 31), "too many workgroups");
  const dim3 grid((unsigned)(bpj * num_jobs)), block(SP_THREADS);
  const size_t lds = (size_t)px * Kp * 4;
  if (label_bytes == 1)
    hipLaunchKernelGGL(seg_postprocess_kernel<unsigned char>, grid, block, lds, (hipStream_t)stream, logits, d_jobs, K, ld, rscale, soft,
                       (unsigned char*)labels, TH, TW, (int)bpj, px);
  else
    hipLaunchKernelGGL(seg_postprocess_kernel<int>, grid, block, lds, (hipStream_t)stream, logits, d_jobs, K, ld, rscale, soft,
                       (int*)labels, TH, TW, (int)bpj, px);
  LVC_CHECK_LAUNCH();
  return LVC_OK;
}

// ------------------------------------------------------------------------------------------------ combine
// One workgroup of 1024 threads per image walks that image's instances serially: instance r+1 sees the pixels instance r took because
// both passes of an instance end in a workgroup barrier, and no workgroup waits on another.  Every count is an integer sum (per-thread
// count -> LDS atomic add), so the result does not depend on the order of arrival.
#define CB_THREADS 1024
#define CB_MAX_INST 1024
#define CB_MAX_LABELS 4096
#define CB_PLANE_FIELDS 8      // lvc_paste_masks' job row: prob row, x0, y0, x1, y1 (fp32 bits), h, w, byte offset

__device__ __forceinline__ float cb_bits(long long v) { return __int_as_float((int)(unsigned)(v & 0xffffffffLL)); }

template <typename LabelT>
__global__ __launch_bounds__(CB_THREADS) void seg_combine_kernel(const unsigned char* __restrict__ planes, const long long* __restrict__ plane_jobs,
                                                                 int use_boxes, const float* __restrict__ scores, const int* __restrict__ classes,
                                                                 const LabelT* __restrict__ labels, int num_labels,
                                                                 const long long* __restrict__ images, double overlap_thresh,
                                                                 double stuff_area_limit, double instances_thresh, int* panoptic,
                                                                 int* __restrict__ segments, int* __restrict__ counts) {
  __shared__ int order[CB_MAX_INST];
  __shared__ int hist[CB_MAX_LABELS];       // free pixels per label; then the id the label got (0: none)
  __shared__ int present[CB_MAX_LABELS];    // the label occurs in the map at all (torch.unique)
  __shared__ int s_area, s_inter;
  const long long* iw = images + (size_t)blockIdx.x * LVCSEG_COMBINE_FIELDS;
  const int first = (int)iw[0], n = (int)iw[1], H = (int)iw[2], W = (int)iw[3];
  const LabelT* lab = labels + iw[4];
  int* pan = panoptic + iw[5];
  int* seg = segments + iw[6] * LVCSEG_SEGMENT_FIELDS;
  const int seg_rows = (int)iw[7];
  const float* sc = scores + iw[8];
  const int* cl = classes + iw[8];
  const int HW = H * W, t = threadIdx.x;

  for (int i = t; i < HW; i += CB_THREADS) pan[i] = 0;
  for (int i = t; i < seg_rows * LVCSEG_SEGMENT_FIELDS; i += CB_THREADS) seg[i] = 0;
  for (int i = t; i < CB_MAX_INST; i += CB_THREADS) order[i] = -1;
  for (int i = t; i < num_labels; i += CB_THREADS) hist[i] = present[i] = 0;
  __syncthreads();
  // descending score, equal scores by the lower index: an instance's rank is the number of instances in front of it
  for (int j = t; j < n; j += CB_THREADS) {
    const float sj = sc[j];
    int rank = 0;
    for (int i = 0; i < n; ++i) {
      const float si = sc[i];
      rank += (si > sj || (si == sj && i < j)) ? 1 : 0;
    }
    order[rank] = j;      // (a rank is below n; NaN scores can leave ranks unused: those stay -1 and are passed over)
  }
  __syncthreads();

  int cur = 0;      // segments so far; every thread keeps the same value
  for (int r = 0; r < n; ++r) {
    const int j = order[r];
    if (j < 0) continue;
    if ((double)sc[j] < instances_thresh) break;
    const long long* pw = plane_jobs + (size_t)(first + j) * CB_PLANE_FIELDS;
    const unsigned char* m = planes + pw[7];
    int x0 = 0, x1 = W, y0 = 0, y1 = H;
    if (use_boxes) {
      // the paste kernel's rectangle (mask_paste.hip) widened by one more pixel on every side
      const float bx0 = cb_bits(pw[1]), by0 = cb_bits(pw[2]), bx1 = cb_bits(pw[3]), by1 = cb_bits(pw[4]);
      const float mx = (bx1 - bx0) + 3.f, my = (by1 - by0) + 3.f;      // (>= (x1 - x0) / Sm + 2 for any mask size Sm >= 1, plus one)
      const float fx0 = floorf(bx0 - mx), fx1 = ceilf(bx1 + mx), fy0 = floorf(by0 - my), fy1 = ceilf(by1 + my);
      x0 = fx0 > 0.f ? (fx0 < (float)W ? (int)fx0 : W) : 0;
      x1 = fx1 < (float)W ? (fx1 > 0.f ? (int)fx1 : 0) : W;
      y0 = fy0 > 0.f ? (fy0 < (float)H ? (int)fy0 : H) : 0;
      y1 = fy1 < (float)H ? (fy1 > 0.f ? (int)fy1 : 0) : H;
    }
    const int rw = x1 - x0, rn = rw > 0 && y1 > y0 ? rw * (y1 - y0) : 0;
    if (t == 0) { s_area = 0; s_inter = 0; }
    __syncthreads();
    int area = 0, inter = 0;
    for (int i = t; i < rn; i += CB_THREADS) {
      const int p = (y0 + i / rw) * W + x0 + i % rw;
      if (m[p]) { ++area; inter += pan[p] > 0 ? 1 : 0; }
    }
    if (area) { atomicAdd(&s_area, area); atomicAdd(&s_inter, inter); }
    __syncthreads();
    area = s_area; inter = s_inter;
    __syncthreads();      // every thread has the sums before the next instance resets them
    if (area == 0) continue;                                                    // (uniform: every thread read the same sums)
    if ((double)inter / (double)area > overlap_thresh) continue;
    ++cur;
    for (int i = t; i < rn; i += CB_THREADS) {
      const int p = (y0 + i / rw) * W + x0 + i % rw;
      if (m[p] && pan[p] == 0) pan[p] = cur;
    }
    if (t == 0 && cur <= seg_rows) {
      int* row = seg + (cur - 1) * LVCSEG_SEGMENT_FIELDS;
      row[0] = cur; row[1] = 1; row[2] = cl[j]; row[3] = j; row[4] = __float_as_int(sc[j]); row[5] = area - inter;
    }
    __syncthreads();      // the taken pixels are visible to the next instance's count
  }

  // stuff: free pixels per label
  for (int i = t; i < HW; i += CB_THREADS) {
    const int l = (int)lab[i];
    if (l < 0 || l >= num_labels) continue;
    if (!present[l]) present[l] = 1;      // (a race of equal values)
    if (pan[i] == 0) atomicAdd(&hist[l], 1);
  }
  __syncthreads();
  if (t == 0) {
    int id = cur;
    for (int l = 1; l < num_labels; ++l) {
      const int a = hist[l];
      hist[l] = 0;
      if (!present[l] || (double)a < stuff_area_limit) continue;
      ++id;
      hist[l] = id;
      if (id <= seg_rows) {
        int* row = seg + (id - 1) * LVCSEG_SEGMENT_FIELDS;
        row[0] = id; row[1] = 0; row[2] = l; row[3] = -1; row[4] = 0; row[5] = a;
      }
    }
    hist[0] = 0;
    counts[blockIdx.x] = id;
  }
  __syncthreads();
  for (int i = t; i < HW; i += CB_THREADS) {
    const int l = (int)lab[i];
    if (l < 0 || l >= num_labels) continue;
    const int id = hist[l];
    if (id && pan[i] == 0) pan[i] = id;
  }
}

extern "C" int lvcseg_panoptic_combine(const unsigned char* planes, long long planes_bytes, const long long* h_plane_jobs,
                                       const long long* d_plane_jobs, int num_planes, int use_boxes, const float* scores,
                                       const int* classes, const void* labels, long long labels_numel, int label_bytes, int num_labels,
                                       const long long* h_images, const long long* d_images, int num_images, double overlap_thresh,
                                       double stuff_area_limit, double instances_thresh, int* panoptic, long long panoptic_numel,
                                       int* segments, long long segment_rows, int* counts, void* stream) {
  LVC_CHECK_ARG(num_images >= 0 && num_planes >= 0, "num_images >= 0, num_planes >= 0");
  LVC_CHECK_ARG(label_bytes == 1 || label_bytes == 4, "label_bytes is 1 (uint8) or 4 (int32)");
  LVC_CHECK_ARG(num_labels >= 1 && num_labels <= CB_MAX_LABELS && (label_bytes == 4 || num_labels <= 256), "1 <= num_labels <= 4096 (256 for uint8 labels)");
  if (num_images == 0) return LVC_OK;
  LVC_CHECK_ARG(labels && h_images && d_images && panoptic && segments && counts, "null pointer");
  LVC_CHECK_ARG(num_planes == 0 || (planes && h_plane_jobs && d_plane_jobs && scores && classes), "null pointer");
  for (int i = 0; i < num_images; ++i) {
    const long long* iw = h_images + (size_t)i * LVCSEG_COMBINE_FIELDS;
    LVC_CHECK_ARG(iw[1] >= 0 && iw[1] <= CB_MAX_INST && iw[0] >= 0 && iw[0] + iw[1] <= num_planes, "an image's instances: at most 1024, inside the plane table");
    LVC_CHECK_ARG(iw[2] >= 1 && iw[3] >= 1 && iw[2] * iw[3] < (1LL << 30), "an image's size");
    const long long hw = iw[2] * iw[3];
    LVC_CHECK_ARG(iw[4] >= 0 && iw[4] + hw <= labels_numel, "an image's label map lies outside the buffer");
    LVC_CHECK_ARG(iw[5] >= 0 && iw[5] + hw <= panoptic_numel, "an image's panoptic map lies outside the buffer");
    LVC_CHECK_ARG(iw[7] >= iw[1] + num_labels && iw[6] >= 0 && iw[6] + iw[7] <= segment_rows, "an image's segment rows: >= instances + num_labels, inside the table");
    LVC_CHECK_ARG(iw[8] >= 0, "an image's first score");
    for (long long j = iw[0]; j < iw[0] + iw[1]; ++j) {
      const long long* pw = h_plane_jobs + (size_t)j * CB_PLANE_FIELDS;
      LVC_CHECK_ARG(pw[5] == iw[2] && pw[6] == iw[3], "a plane's size differs from its image's");
      LVC_CHECK_ARG(pw[7] >= 0 && pw[7] + hw <= planes_bytes, "a plane lies outside the buffer");
    }
  }
  const dim3 grid((unsigned)num_images), block(CB_THREADS);
  if (label_bytes == 1)
    hipLaunchKernelGGL(seg_combine_kernel<unsigned char>, grid, block, 0, (hipStream_t)stream, planes, d_plane_jobs, use_boxes, scores, classes,
                       (const unsigned char*)labels, num_labels, d_images, overlap_thresh, stuff_area_limit, instances_thresh, panoptic,
                       segments, counts);
  else
    hipLaunchKernelGGL(seg_combine_kernel<int>, grid, block, 0, (hipStream_t)stream, planes, d_plane_jobs, use_boxes, scores, classes,
                       (const int*)labels, num_labels, d_images, overlap_thresh, stuff_area_limit, instances_thresh, panoptic, segments,
                       counts);
  LVC_CHECK_LAUNCH();
  return LVC_OK;
}
