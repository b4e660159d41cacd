// color_jitter.hip -- INPUT.COLOR_JITTER of a whole batch on the device: torchvision's ColorJitter on a PIL image (reference
// detectron2/data/transforms/augmentation_impl.py:589-617 ColorJitterPIL, detection_utils.py:581-584), which is Pillow's ImageEnhance
// blends (Image.blend against a degenerate image), convert("L"), and the RGB <-> HSV conversions of Convert.c around an 8-bit hue shift.
//
// lvc_color_jitter_tiles_u8: per job a crop window on a canvas painted from 1 to 9 tiles (the tile list and the painting rule of
// lvc_train_input_tiles_u8: later tile wins, 114 where no tile is; a plain image is one tile) and up to four steps in the job's own
// order.  The jittered window leaves as a packed uint8 [ch][cw][3] image in the caller's scratch buffer, which lvc_train_input_u8 then
// reads as a plain image.  TWO launches whatever the batch size and the mix:
//   1. the grey-level sum: the contrast step blends with the rounded MEAN grey level of the whole window as the steps before it left
//      it, so jobs with a contrast step add L of every pixel (after those steps) into a 64-bit word of their job row -- integer
//      atomics: the order of the additions does not change the sum, runs stay bit-identical.  The word is zero in the uploaded blob;
//      jobs without a contrast step leave at once;
//   2. the pixels: m = int(sum / count + 0.5) (fp64, as ImageStat's mean), the steps in order, packed stores.
// A thread owns four consecutive pixels of the packed window (12 bytes: three whole dwords).
//
// The arithmetic is Pillow's, checked exhaustively (tests/color_ref.py, tests/test_host_color_jitter.py): the blend is
// in1 + f * (in2 - in1) in fp32 without contraction; RGB -> HSV mixes fp32 and fp64 as Convert.c does (the fp32 store of the hue
// after the fmod matters); HSV -> RGB is in integers (Pillow rounds v * (1 - s * f) half away from zero; the exact quotient over
// 255 * 255 is never at a half, and the integer form equals Pillow on all 2^24 triples).  Channels are taken by position.
// EXACT flags (-ffp-contract=off -fno-fast-math).
#include "input_common.h"

#define CJ_FIELDS (TL_HEAD + TL_MAX_TILES * TL_WORDS)   // 128 words = 1 KiB per job (lvc_amd.h); the tile list: input_common.h
#define CJ_PIX 4          // pixels per thread
#define CJ_BLOCK 256
#define CJ_MAX_GRID (1 << 18)   // workgroups per job; larger windows are walked in strides

enum { CJ_X0 = 0, CJ_Y0, CJ_CW, CJ_CH, CJ_OUT, CJ_NOPS, CJ_OP0, CJ_F0 = CJ_OP0 + 4, CJ_NT = CJ_F0 + 4, CJ_SUM = 19 };
enum { CJ_BRIGHTNESS = 0, CJ_CONTRAST, CJ_SATURATION, CJ_HUE };

// the tiles of a job in window coordinates, in paint order
struct CjTiles {
  int lo_x[TL_MAX_TILES], hi_x[TL_MAX_TILES], lo_y[TL_MAX_TILES], hi_y[TL_MAX_TILES];
  long long base[TL_MAX_TILES], sy[TL_MAX_TILES], sx[TL_MAX_TILES], sc[TL_MAX_TILES];   // window pixel (y, x): base + y * sy + x * sx
  int n;
};

// the steps of a job
struct CjOps {
  int n, op[4], shift, m;
  float f[4];
};

__device__ __forceinline__ void cj_load_tiles(const long long* jb, CjTiles* tl) {
  const int t = threadIdx.x, nt = (int)jb[CJ_NT];
  if (t < nt) {
    const long long* q = jb + TL_HEAD + (size_t)t * TL_WORDS;
    const long long X0 = jb[CJ_X0], Y0 = jb[CJ_Y0], cw = jb[CJ_CW], ch = jb[CJ_CH];
    const long long lx = q[TL_X1A] - X0, hx = q[TL_X2A] - X0, ly = q[TL_Y1A] - Y0, hy = q[TL_Y2A] - Y0;
    tl->lo_x[t] = (int)(lx > 0 ? lx : 0); tl->hi_x[t] = (int)(hx < cw ? hx : cw);
    tl->lo_y[t] = (int)(ly > 0 ? ly : 0); tl->hi_y[t] = (int)(hy < ch ? hy : ch);
    tl->sy[t] = q[TL_SY]; tl->sx[t] = q[TL_SX]; tl->sc[t] = q[TL_SC];
    tl->base[t] = q[TL_SRC] + (Y0 - q[TL_Y1A] + q[TL_Y1B]) * q[TL_SY] + (X0 - q[TL_X1A] + q[TL_X1B]) * q[TL_SX];
  }
  if (t == 0) tl->n = nt;
}

__device__ __forceinline__ void cj_load_ops(const long long* jb, CjOps& o, int n) {
  o.n = n; o.shift = 0; o.m = 0;
  for (int k = 0; k < 4; ++k) {
    o.op[k] = (int)jb[CJ_OP0 + k];
    o.f[k] = __int_as_float((int)jb[CJ_F0 + k]);
    // adjust_hue: np.uint8(hue_factor * 255), the product in fp64, truncated toward zero, 8-bit wrap-around
    if (k < n && o.op[k] == CJ_HUE) o.shift = (int)((double)o.f[k] * 255.0) & 255;
  }
}

// window pixel (y, x) through the tile list: the last tile that covers it, TL_FILL where none does
__device__ __forceinline__ void cj_fetch(const CjTiles* tl, int y, int x, int& c0, int& c1, int& c2) {
  int own = -1;
  for (int i = 0; i < tl->n; ++i)
    if (tl->lo_x[i] <= x && x < tl->hi_x[i] && tl->lo_y[i] <= y && y < tl->hi_y[i]) own = i;
  c0 = c1 = c2 = TL_FILL;
  if (own >= 0) {
    const long long sc = tl->sc[own];
    const unsigned char* p = reinterpret_cast<const unsigned char*>(tl->base[own] + y * tl->sy[own] + x * tl->sx[own]);
    c0 = p[0]; c1 = p[sc]; c2 = p[2 * sc];
  }
}

__device__ __forceinline__ int cj_grey(int c0, int c1, int c2) { return (c0 * 19595 + c1 * 38470 + c2 * 7471 + 0x8000) >> 16; }

// Image.blend(degenerate, image, f) on one channel
__device__ __forceinline__ int cj_blend(int d, int c, float f) {
  const float t = (float)d + f * ((float)c - (float)d);
  return t <= 0.f ? 0 : (t >= 255.f ? 255 : (int)t);
}

__device__ __forceinline__ int cj_clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// Convert.c rgb2hsv_row, the hue moved by `shift` (8-bit wrap-around), hsv2rgb
__device__ __forceinline__ void cj_hue(int& c0, int& c1, int& c2, int shift) {
  const int mx = max(c0, max(c1, c2)), mn = min(c0, min(c1, c2));
  int H = 0, S = 0;
  const int V = mx;
  if (mx != mn) {
    const float cr = (float)(mx - mn);
    const float s = cr / (float)mx;
    const float rc = (float)(mx - c0) / cr, gc = (float)(mx - c1) / cr, bc = (float)(mx - c2) / cr;
    float h;
    if (c0 == mx) h = bc - gc;
    else if (c1 == mx) h = (float)((2.0 + (double)rc) - (double)bc);
    else h = (float)((4.0 + (double)gc) - (double)rc);
    const double w = (double)h / 6.0 + 1.0;      // in [5/6, 11/6): fmod(w, 1.0) is w or w - 1, both exact
    h = (float)(w >= 1.0 ? w - 1.0 : w);
    H = cj_clip8((int)((double)h * 255.0));
    S = cj_clip8((int)((double)s * 255.0));
  }
  H = (H + shift) & 255;
  if (S == 0) { c0 = c1 = c2 = V; return; }
  const int i = H * 6 / 255, r = H * 6 - 255 * i;      // hue sector and its remainder in 255ths
  const int p = (2 * V * (255 - S) + 255) / 510;
  const int q = (2 * V * (65025 - S * r) + 65025) / 130050;
  const int t = (2 * V * (65025 - S * (255 - r)) + 65025) / 130050;
  switch (i % 6) {
    case 0: c0 = V; c1 = t; c2 = p; break;
    case 1: c0 = q; c1 = V; c2 = p; break;
    case 2: c0 = p; c1 = V; c2 = t; break;
    case 3: c0 = p; c1 = q; c2 = V; break;
    case 4: c0 = t; c1 = p; c2 = V; break;
    default: c0 = V; c1 = p; c2 = q; break;
  }
}

// steps [0, upto) of the job on one pixel
__device__ __forceinline__ void cj_apply(const CjOps& o, int upto, int& c0, int& c1, int& c2) {
  for (int k = 0; k < upto; ++k) {
    const float f = o.f[k];
    if (o.op[k] == CJ_HUE) {
      cj_hue(c0, c1, c2, o.shift);
    } else {
      int d0 = 0, d1 = 0, d2 = 0;      // brightness: black
      if (o.op[k] == CJ_CONTRAST) d0 = d1 = d2 = o.m;
      else if (o.op[k] == CJ_SATURATION) d0 = d1 = d2 = cj_grey(c0, c1, c2);
      c0 = cj_blend(d0, c0, f); c1 = cj_blend(d1, c1, f); c2 = cj_blend(d2, c2, f);
    }
  }
}

__device__ __forceinline__ int cj_contrast_at(const long long* jb, int n) {
  for (int k = 0; k < n; ++k)
    if (jb[CJ_OP0 + k] == CJ_CONTRAST) return k;
  return -1;
}

// launch 1: sum of L over the window after the steps in front of the contrast step -> the job's CJ_SUM word
__global__ __launch_bounds__(CJ_BLOCK) void color_jitter_sum_kernel(char* __restrict__ blob) {
  long long* jb = reinterpret_cast<long long*>(blob) + (size_t)blockIdx.y * CJ_FIELDS;
  const int n_ops = (int)jb[CJ_NOPS];
  const int at = cj_contrast_at(jb, n_ops);
  if (at < 0) return;                                   // no contrast step: the whole workgroup leaves
  const int cw = (int)jb[CJ_CW];
  const long long total = (long long)cw * jb[CJ_CH], per_wg = CJ_BLOCK * CJ_PIX;
  if ((long long)blockIdx.x * per_wg >= total) return;
  __shared__ CjTiles tl;
  __shared__ unsigned long long part[CJ_BLOCK / 64];
  __shared__ CjOps o;                                   // the steps are the same for every thread
  cj_load_tiles(jb, &tl);
  if (threadIdx.x == 64) cj_load_ops(jb, o, n_ops);
  __syncthreads();
  unsigned long long acc = 0;
  for (long long first = ((long long)blockIdx.x * CJ_BLOCK + threadIdx.x) * CJ_PIX; first < total; first += (long long)gridDim.x * per_wg) {
    int y = (int)(first / cw), x = (int)(first - (long long)y * cw);
    for (int k = 0; k < CJ_PIX && first + k < total; ++k) {
      int c0, c1, c2;
      cj_fetch(&tl, y, x, c0, c1, c2);
      cj_apply(o, at, c0, c1, c2);
      acc += (unsigned)cj_grey(c0, c1, c2);
      if (++x == cw) { x = 0; ++y; }
    }
  }
  for (int d = 32; d > 0; d >>= 1) acc += __shfl_down(acc, d, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long s = 0;
    for (int w = 0; w < CJ_BLOCK / 64; ++w) s += part[w];
    atomicAdd(reinterpret_cast<unsigned long long*>(jb + CJ_SUM), s);
  }
}

// launch 2: the steps on every pixel of the window -> out + CJ_OUT, packed [ch][cw][3]
__global__ __launch_bounds__(CJ_BLOCK) void color_jitter_pixels_kernel(const char* __restrict__ blob, unsigned char* __restrict__ out) {
  const long long* jb = reinterpret_cast<const long long*>(blob) + (size_t)blockIdx.y * CJ_FIELDS;
  const int cw = (int)jb[CJ_CW];
  const long long total = (long long)cw * jb[CJ_CH], per_wg = CJ_BLOCK * CJ_PIX;
  if ((long long)blockIdx.x * per_wg >= total) return;
  __shared__ CjTiles tl;
  __shared__ CjOps o;
  cj_load_tiles(jb, &tl);
  if (threadIdx.x == 64) {
    cj_load_ops(jb, o, (int)jb[CJ_NOPS]);
    // ImageEnhance.Contrast: int(ImageStat.Stat(L).mean[0] + 0.5), the mean a float64 division
    o.m = (int)((double)jb[CJ_SUM] / (double)total + 0.5);
  }
  __syncthreads();
  unsigned char* dst = out + jb[CJ_OUT];      // 4-byte aligned (checked on the host)
  for (long long first = ((long long)blockIdx.x * CJ_BLOCK + threadIdx.x) * CJ_PIX; first < total; first += (long long)gridDim.x * per_wg) {
    int y = (int)(first / cw), x = (int)(first - (long long)y * cw);
    unsigned w[3] = {0u, 0u, 0u};              // the packed bytes of this thread's pixels
    int n = 0;
#pragma unroll
    for (int k = 0; k < CJ_PIX; ++k) {
      if (first + k < total) {
        int c0, c1, c2;
        cj_fetch(&tl, y, x, c0, c1, c2);
        cj_apply(o, o.n, c0, c1, c2);
        w[(3 * k) >> 2] |= (unsigned)c0 << (((3 * k) & 3) * 8);
        w[(3 * k + 1) >> 2] |= (unsigned)c1 << (((3 * k + 1) & 3) * 8);
        w[(3 * k + 2) >> 2] |= (unsigned)c2 << (((3 * k + 2) & 3) * 8);
        n = k + 1;
        if (++x == cw) { x = 0; ++y; }
      }
    }
    if (n == CJ_PIX) {
      unsigned* d = reinterpret_cast<unsigned*>(dst + first * 3);
      d[0] = w[0]; d[1] = w[1]; d[2] = w[2];
    } else {                                   // the last pixels of the window
#pragma unroll
      for (int j = 0; j < 3 * (CJ_PIX - 1); ++j)
        if (j < 3 * n) dst[first * 3 + j] = (unsigned char)(w[j >> 2] >> ((j & 3) * 8));
    }
  }
}

// Job words and arguments: include/lvc_amd.h.  d_blob is WRITTEN: word 19 receives the grey-level sum.  Checked on the host copy
// before anything is launched: every pixel of a rectangle that the window sees lies inside its tile, outputs inside `out`.
// launches: optional, the number of kernel launches issued (two).
extern "C" int lvc_color_jitter_tiles_u8(const void* h_blob, void* d_blob, long long blob_bytes, int B, unsigned char* out,
                                         long long out_bytes, int* launches, void* stream) {
  if (launches) *launches = 0;
  LVC_CHECK_ARG(B >= 0 && B <= 65535, "bad batch size");
  if (B == 0) return LVC_OK;
  LVC_CHECK_ARG(h_blob && d_blob && out, "null argument");
  LVC_CHECK_ARG(((uintptr_t)h_blob & 7) == 0 && ((uintptr_t)d_blob & 7) == 0 && ((uintptr_t)out & 3) == 0, "the blob must be 8-byte, the output 4-byte aligned");
  LVC_CHECK_MSG(check_blob(h_blob, d_blob, blob_bytes, B, CJ_FIELDS));
  const long long* jobs = reinterpret_cast<const long long*>(h_blob);
  long long most = 0;
  for (int i = 0; i < B; ++i) {
    const long long* j = jobs + (size_t)i * CJ_FIELDS;
    const long long cw = j[CJ_CW], ch = j[CJ_CH];
    LVC_CHECK_MSG(check_window_tiles(j, j[CJ_NT], j + TL_HEAD));
    LVC_CHECK_ARG(j[CJ_NOPS] >= 0 && j[CJ_NOPS] <= 4, "a job has 0 to 4 steps");
    int contrasts = 0;
    for (int k = 0; k < (int)j[CJ_NOPS]; ++k) {
      LVC_CHECK_ARG(j[CJ_OP0 + k] >= CJ_BRIGHTNESS && j[CJ_OP0 + k] <= CJ_HUE, "bad step id");
      float f;
      const int bits = (int)j[CJ_F0 + k];
      memcpy(&f, &bits, 4);
      LVC_CHECK_ARG(f == f && f >= -1e6f && f <= 1e6f, "bad factor");
      if (j[CJ_OP0 + k] == CJ_HUE) LVC_CHECK_ARG(f >= -0.5f && f <= 0.5f, "the hue factor lies in [-0.5, 0.5]");
      else LVC_CHECK_ARG(f >= 0.f, "a blend factor is not negative");
      contrasts += j[CJ_OP0 + k] == CJ_CONTRAST;
    }
    LVC_CHECK_ARG(contrasts <= 1, "at most one contrast step");
    LVC_CHECK_ARG(j[CJ_SUM] == 0, "the sum word must be zero");
    LVC_CHECK_ARG(j[CJ_OUT] >= 0 && (j[CJ_OUT] & 3) == 0 && j[CJ_OUT] <= out_bytes && ch * cw * 3 <= out_bytes - j[CJ_OUT],
                  "output outside the scratch buffer");
    for (int p = 0; p < i; ++p) {
      const long long* q = jobs + (size_t)p * CJ_FIELDS;
      LVC_CHECK_ARG(q[CJ_OUT] + q[CJ_CH] * q[CJ_CW] * 3 <= j[CJ_OUT] || j[CJ_OUT] + ch * cw * 3 <= q[CJ_OUT], "two outputs overlap");
    }
    most = ch * cw > most ? ch * cw : most;
  }
  long long gx = lvc_cdiv64(most, CJ_BLOCK * CJ_PIX);
  gx = gx > CJ_MAX_GRID ? CJ_MAX_GRID : gx;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(color_jitter_sum_kernel, dim3((unsigned)gx, B), dim3(CJ_BLOCK), 0, st,
                     reinterpret_cast<char*>(d_blob));
  LVC_CHECK_LAUNCH();
  if (launches) ++*launches;
  hipLaunchKernelGGL(color_jitter_pixels_kernel, dim3((unsigned)gx, B), dim3(CJ_BLOCK), 0, st, reinterpret_cast<const char*>(d_blob), out);
  LVC_CHECK_LAUNCH();
  if (launches) ++*launches;
  return LVC_OK;
}
