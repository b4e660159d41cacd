// mask_paste.hip -- paste_masks_in_image (reference detectron2/layers/mask_ops.py:16-135) for a whole batch in one launch.
//
// The reference builds an [N, H, W, 2] fp32 sampling grid and calls F.grid_sample per chunk of detections, then thresholds the
// [N, H, W] fp32 result.  Here a job table with one row per detection drives one kernel that writes the thresholded bytes directly:
// 1 byte per output pixel leaves the chip, nothing else of that size exists.
//
// Per output pixel the arithmetic is the reference's, in fp32 and in its order (this file is built without contraction):
//   gx = (px + 0.5 - x0) / (x1 - x0) * 2 - 1                        (_do_paste_mask)
//   ix = ((gx + 1) * Wm - 1) / 2                                    (grid_sample, align_corners=False)
//   w = ix - floor(ix), e = 1 - w (likewise n, s for y); value = nw_val * (s e) + ne_val * (s w) + sw_val * (n e) + se_val * (n w)
//   with zeros for taps outside the mask; byte = value >= threshold.
// The tap weights take the form of ATen's vectorised CPU grid_sample, whose fp32 bits the tests compare against; ATen's CUDA kernel
// forms them as ix_se - ix etc., which can differ from these in the last bit (far inside the band the tests set aside).
// A thread owns 16 consecutive bytes of the output buffer, aligned to 16 in the BUFFER (detections follow each other without padding,
// so a detection's first and last chunk may be shared with its neighbours: those are written byte by byte, all others with one
// 16-byte store).  Pixels outside a rectangle that conservatively contains every pixel with a tap inside the mask are zero without
// sampling: a detection's bytes far from its box cost a store and nothing else.  (The value there is 0, so the byte is 0 >= threshold:
// 1 only for threshold 0, which sets every pixel, as in the reference.)
#include <stdint.h>

#include "common.h"

#define MP_FIELDS 8      // int64 words per job: prob row, x0, y0, x1, y1 (fp32 bit patterns), out_h, out_w, byte offset of [out_h, out_w]

struct PasteJob {
  const float* mask;
  float x0, y0, x1, y1;
  int H, W, xlo, xhi, ylo, yhi;
  long long off;
};

__device__ __forceinline__ float mp_bits(long long v) { return __int_as_float((int)(unsigned)(v & 0xffffffffLL)); }

__device__ __forceinline__ unsigned mp_pixel(const PasteJob& jb, int Sm, int px, int py, float thr) {
  const unsigned zero_bit = 0.f >= thr ? 1u : 0u;      // a pixel with no tap inside the mask
  if (px < jb.xlo || px >= jb.xhi || py < jb.ylo || py >= jb.yhi) return zero_bit;
  const float fS = (float)Sm;
  const float gx = ((float)px + 0.5f - jb.x0) / (jb.x1 - jb.x0) * 2.f - 1.f;
  const float gy = ((float)py + 0.5f - jb.y0) / (jb.y1 - jb.y0) * 2.f - 1.f;
  const float ix = ((gx + 1.f) * fS - 1.f) / 2.f;
  const float iy = ((gy + 1.f) * fS - 1.f) / 2.f;
  if (!(ix > -1.f && ix < fS && iy > -1.f && iy < fS)) return zero_bit;      // every tap outside the mask
  const float fx = floorf(ix), fy = floorf(iy);
  const int xw = (int)fx, yn = (int)fy;
  const float w = ix - fx, e = 1.f - w, n = iy - fy, s = 1.f - n;
  const bool wi = xw >= 0, ei = xw + 1 < Sm, ni = yn >= 0, si = yn + 1 < Sm;
  const float* m = jb.mask;
  const float nwv = (ni && wi) ? m[yn * Sm + xw] : 0.f;
  const float nev = (ni && ei) ? m[yn * Sm + xw + 1] : 0.f;
  const float swv = (si && wi) ? m[(yn + 1) * Sm + xw] : 0.f;
  const float sev = (si && ei) ? m[(yn + 1) * Sm + xw + 1] : 0.f;
  const float v = nwv * (s * e) + nev * (s * w) + swv * (n * e) + sev * (n * w);
  return v >= thr ? 1u : 0u;
}

__global__ __launch_bounds__(256) void paste_masks_kernel(const float* __restrict__ prob, int Sm, const long long* __restrict__ jobs,
                                                          unsigned char* __restrict__ out, float thr, int blocks_per_job) {
  const int job = blockIdx.x / blocks_per_job;
  const int blk = blockIdx.x - job * blocks_per_job;
  const long long* jw = jobs + (size_t)job * MP_FIELDS;
  PasteJob jb;
  jb.mask = prob + (size_t)jw[0] * Sm * Sm;
  jb.x0 = mp_bits(jw[1]); jb.y0 = mp_bits(jw[2]); jb.x1 = mp_bits(jw[3]); jb.y1 = mp_bits(jw[4]);
  jb.H = (int)jw[5]; jb.W = (int)jw[6]; jb.off = jw[7];
  // pixels that may have a tap inside the mask: |px + 0.5 - centre| < (x1 - x0) (1/2 + 1/(2 Sm)); a margin of a whole mask cell plus
  // two pixels covers the rounding of the expressions above (the exact test per pixel is made inside the rectangle)
  const float mx = (jb.x1 - jb.x0) / (float)Sm + 2.f, my = (jb.y1 - jb.y0) / (float)Sm + 2.f;
  const float fxlo = floorf(jb.x0 - mx), fxhi = ceilf(jb.x1 + mx), fylo = floorf(jb.y0 - my), fyhi = ceilf(jb.y1 + my);
  jb.xlo = fxlo > 0.f ? (fxlo < (float)jb.W ? (int)fxlo : jb.W) : 0;
  jb.xhi = fxhi < (float)jb.W ? (fxhi > 0.f ? (int)fxhi : 0) : jb.W;
  jb.ylo = fylo > 0.f ? (fylo < (float)jb.H ? (int)fylo : jb.H) : 0;
  jb.yhi = fyhi < (float)jb.H ? (fyhi > 0.f ? (int)fyhi : 0) : jb.H;

  const long long HW = (long long)jb.H * jb.W;
  const long long base = jb.off & ~15LL;                                   // first 16-byte chunk of the buffer this job touches
  const long long chunk = (long long)blk * 256 + threadIdx.x;
  const long long g0 = base + chunk * 16;                                  // buffer position of the chunk's first byte
  if (g0 >= jb.off + HW) return;
  long long i0 = g0 - jb.off;                                              // index inside [H, W]; negative in a shared first chunk
  const bool whole = i0 >= 0 && i0 + 16 <= HW;
  const long long ic = i0 < 0 ? 0 : i0;
  int py = (int)(ic / jb.W), px = (int)(ic - (long long)py * jb.W);
  if (whole) {
    const unsigned fill = 0.f >= thr ? 0x01010101u : 0u;
    unsigned wds[4] = {fill, fill, fill, fill};
    // rows wholly outside the rectangle: nothing to sample when the chunk's first and last pixel rows are
    const int pyl = (int)((ic + 15) / jb.W);
    const bool skip = (pyl < jb.ylo || py >= jb.yhi) || (py == pyl && (px >= jb.xhi || px + 15 < jb.xlo));
    if (!skip) {
      wds[0] = wds[1] = wds[2] = wds[3] = 0u;
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        wds[k >> 2] |= mp_pixel(jb, Sm, px, py, thr) << ((k & 3) * 8);
        if (++px == jb.W) { px = 0; ++py; }
      }
    }
    *reinterpret_cast<uint4*>(out + g0) = make_uint4(wds[0], wds[1], wds[2], wds[3]);
  } else {
    for (long long i = ic; i < i0 + 16 && i < HW; ++i) {
      out[jb.off + i] = (unsigned char)mp_pixel(jb, Sm, px, py, thr);
      if (++px == jb.W) { px = 0; ++py; }
    }
  }
}

static float mp_host_bits(long long v) {
  union { unsigned u; float f; } c;
  c.u = (unsigned)(v & 0xffffffffLL);
  return c.f;
}

extern "C" int lvc_paste_masks(const float* prob, int num_rows, int mask_size, const long long* h_jobs, const long long* d_jobs,
                               int num_jobs, unsigned char* out, long long out_bytes, float threshold, void* stream) {
  LVC_CHECK_ARG(num_jobs >= 0 && num_rows >= 0 && mask_size >= 1, "num_jobs >= 0, num_rows >= 0, mask_size >= 1");
  LVC_CHECK_ARG(threshold >= 0.f, "the reference's threshold < 0 visualisation branch is not built");
  if (num_jobs == 0) return LVC_OK;
  LVC_CHECK_ARG(prob && h_jobs && d_jobs && out, "null pointer");
  LVC_CHECK_ARG(((uintptr_t)out & 15) == 0 && out_bytes % 16 == 0, "output buffer: 16-byte aligned, a multiple of 16 bytes");
  long long max_hw = 0;
  for (int i = 0; i < num_jobs; ++i) {
    const long long* jw = h_jobs + (size_t)i * MP_FIELDS;
    LVC_CHECK_ARG(jw[0] >= 0 && jw[0] < num_rows, "a job's source row is outside prob");
    const float x0 = mp_host_bits(jw[1]), y0 = mp_host_bits(jw[2]), x1 = mp_host_bits(jw[3]), y1 = mp_host_bits(jw[4]);
    LVC_CHECK_ARG(x0 - x0 == 0.f && y0 - y0 == 0.f && x1 - x1 == 0.f && y1 - y1 == 0.f, "a job's box is not finite");
    LVC_CHECK_ARG(x1 > x0 && y1 > y0, "a box of zero width or height (the non-empty filter runs before the paste)");
    LVC_CHECK_ARG(jw[5] > 0 && jw[6] > 0 && jw[5] < (1 << 24) && jw[6] < (1 << 24), "a job's image size");
    const long long hw = jw[5] * jw[6];
    LVC_CHECK_ARG(jw[7] >= 0 && jw[7] + hw <= out_bytes, "a job's output lies outside the buffer");
    if (hw > max_hw) max_hw = hw;
  }
  // chunks a job can touch: its HW bytes plus up to 15 bytes in front of them inside the first chunk
  const long long chunks = (max_hw + 15 + 15) / 16;
  const long long bpj = (chunks + 255) / 256;
  LVC_CHECK_ARG(bpj * num_jobs < (1LL << 31), "too many workgroups");
  hipLaunchKernelGGL(paste_masks_kernel, dim3((unsigned)(bpj * num_jobs)), dim3(256), 0, (hipStream_t)stream, prob, mask_size, d_jobs, out,
                     threshold, (int)bpj);
  LVC_CHECK_LAUNCH();
  return LVC_OK;
}
