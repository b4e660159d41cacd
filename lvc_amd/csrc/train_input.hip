// train_input.hip -- the training input of a whole batch on the device: RandomCrop -> ResizeShortestEdge -> RandomFlip
// (reference lvc/data/dataset_mapper.py:90-209; detectron2/data/detection_utils.py:563-598; fvcore CropTransform / HFlipTransform)
// fused with GeneralizedRCNN.preprocess_image (lvc/modeling/meta_arch/rcnn.py:324-333) and ImageList.from_tensors.
//
// lvc_train_input_u8: B uint8 images of different sizes, read through strides, go to the B slots of one NHWC4 fp32 batch
// [n_slots][Hp][Wp][4] as (resized - mean) / std, mirrored along the width where the job says so, zero padded -- the slot layout
// lvc_resize_bilinear_u8 fills at test time -- in TWO launches whatever B is:
//   1. horizontal pass, grid (x tiles, rows of the largest crop, B): only the rows and columns of each crop window are read;
//      images whose width does not change leave at once;
//   2. vertical pass, grid (x tiles, Hp, B): thread (yo, xo) owns OUTPUT pixel (yo, xo) of its slot: it resamples source column
//      new_w-1-xo when the image is mirrored (HFlipTransform after the resize), xo otherwise, and writes one float4 -- the pixel, or
//      the zero padding outside new_h x new_w -- and optionally the uint8 pixel (the reference's dataset_dict["image"]).
// The resample is resize.hip's, bit for bit: Pillow's 22-bit coefficients for the CROPPED size -> the output size
// (lvc_amd/data/transforms.py resample_coeffs), a uint8 intermediate, an unchanged axis skipped.  Crop and flip are copies.
//
// The per-image job table and every coefficient table travel in ONE blob that the caller uploads once; the host copy of the same
// blob is checked here (windows inside their images, every tap inside its crop, outputs inside their buffers) before anything
// is launched.  EXACT flags (-ffp-contract=off -fno-fast-math): the normaliser rounds as preprocess_image does.
//
// lvc_train_input_tiles_u8 (below, with kernels and a job table of its own): the same for images that are MOSAICS of 1 to 9 tiles
// (reference lvc/data/mosaic.py get_mosaic / get_mosaic9), read in place -- neither the canvas nor the composite exists in memory.
//
// lvc_train_input_lsj_u8 (at the end, with kernels and a job table of its own): INPUT.LSJ -- the window of the scaled image that
// FixedSizeCrop keeps, on its padded canvas, without the scaled image ever being written.
#include "common.h"

#define TI_PREC 22
#define TI_FIELDS 24   // int64 words per job (lvc_amd.h)

enum {
  TI_SRC = 0, TI_H, TI_W, TI_SY, TI_SX, TI_SC, TI_X0, TI_Y0, TI_CW, TI_CH, TI_NEW_H, TI_NEW_W, TI_XB, TI_XK, TI_KXS, TI_YB, TI_YK,
  TI_KYS, TI_FLIP, TI_SLOT, TI_U8, TI_TMP
};

__device__ __forceinline__ unsigned char ti_clip8(int v) {
  v >>= TI_PREC;
  return (unsigned char)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// src crop [ch][cw] (strided) -> tmp [ch][new_w][3]
__global__ __launch_bounds__(256) void train_input_h_kernel(const char* __restrict__ blob, unsigned char* __restrict__ tmp) {
  const long long* jb = reinterpret_cast<const long long*>(blob) + (size_t)blockIdx.z * TI_FIELDS;
  if (jb[TI_XB] < 0) return;   // width unchanged: Pillow skips the horizontal pass
  const int xo = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
  const int new_w = (int)jb[TI_NEW_W];
  if (xo >= new_w || y >= (int)jb[TI_CH]) return;
  const long long sy = jb[TI_SY], sx = jb[TI_SX], sc = jb[TI_SC];
  const int* xb = reinterpret_cast<const int*>(blob + jb[TI_XB]);
  const int kxs = (int)jb[TI_KXS];
  const int* k = reinterpret_cast<const int*>(blob + jb[TI_XK]) + (size_t)xo * kxs;
  const int xmin = xb[2 * xo], cnt = xb[2 * xo + 1];
  const unsigned char* row = reinterpret_cast<const unsigned char*>(jb[TI_SRC]) + (jb[TI_Y0] + y) * sy + (jb[TI_X0] + xmin) * sx;
  int s0 = 1 << (TI_PREC - 1), s1 = s0, s2 = s0;
  for (int x = 0; x < cnt; ++x) {
    const int c = k[x];
    const unsigned char* p = row + x * sx;
    s0 += p[0] * c;
    s1 += p[sc] * c;
    s2 += p[2 * sc] * c;
  }
  unsigned char* o = tmp + jb[TI_TMP] + ((size_t)y * new_w + xo) * 3;
  o[0] = ti_clip8(s0); o[1] = ti_clip8(s1); o[2] = ti_clip8(s2);
}

__global__ __launch_bounds__(256) void train_input_v_kernel(const char* __restrict__ blob, const unsigned char* __restrict__ tmp,
                                                            float* __restrict__ out, int Hp, int Wp, float m0, float m1, float m2,
                                                            float d0, float d1, float d2) {
  const long long* jb = reinterpret_cast<const long long*>(blob) + (size_t)blockIdx.z * TI_FIELDS;
  const int xo = blockIdx.x * 256 + threadIdx.x, yo = blockIdx.y;
  if (xo >= Wp) return;
  const int new_h = (int)jb[TI_NEW_H], new_w = (int)jb[TI_NEW_W];
  float4 v = {0.f, 0.f, 0.f, 0.f};
  if (yo < new_h && xo < new_w) {
    const int xs = jb[TI_FLIP] ? new_w - 1 - xo : xo;   // HFlipTransform(new_w) after the resize
    const unsigned char* col;
    long long sy, sc;
    if (jb[TI_XB] >= 0) {
      col = tmp + jb[TI_TMP] + (size_t)xs * 3; sy = (long long)new_w * 3; sc = 1;
    } else {
      sy = jb[TI_SY]; sc = jb[TI_SC];
      col = reinterpret_cast<const unsigned char*>(jb[TI_SRC]) + jb[TI_Y0] * sy + (jb[TI_X0] + xs) * jb[TI_SX];
    }
    unsigned char r0, r1, r2;
    if (jb[TI_YB] >= 0) {
      const int* yb = reinterpret_cast<const int*>(blob + jb[TI_YB]);
      const int* k = reinterpret_cast<const int*>(blob + jb[TI_YK]) + (size_t)yo * (int)jb[TI_KYS];
      const int ymin = yb[2 * yo], cnt = yb[2 * yo + 1];
      int s0 = 1 << (TI_PREC - 1), s1 = s0, s2 = s0;
      for (int y = 0; y < cnt; ++y) {
        const unsigned char* p = col + (ymin + y) * sy;
        const int c = k[y];
        s0 += p[0] * c; s1 += p[sc] * c; s2 += p[2 * sc] * c;
      }
      r0 = ti_clip8(s0); r1 = ti_clip8(s1); r2 = ti_clip8(s2);
    } else {   // height unchanged: Pillow skips the vertical pass
      const unsigned char* p = col + yo * sy;
      r0 = p[0]; r1 = p[sc]; r2 = p[2 * sc];
    }
    if (jb[TI_U8]) {
      unsigned char* o = reinterpret_cast<unsigned char*>(jb[TI_U8]) + ((size_t)yo * new_w + xo) * 3;
      o[0] = r0; o[1] = r1; o[2] = r2;
    }
    v.x = ((float)r0 - m0) / d0;
    v.y = ((float)r1 - m1) / d1;
    v.z = ((float)r2 - m2) / d2;
  }
  *reinterpret_cast<float4*>(out + (((size_t)jb[TI_SLOT] * Hp + yo) * Wp + xo) * 4) = v;
}

// one resample axis of one job: the tables lie inside the blob and every tap inside [0, in_size)
static bool ti_check_axis(const char* h_blob, long long blob_bytes, long long b_off, long long k_off, long long ks, long long in_size,
                          long long out_size) {
  if (ks <= 0 || b_off < 0 || k_off < 0 || (b_off & 3) || (k_off & 3)) return false;
  if (b_off + out_size * 8 > blob_bytes || k_off + out_size * ks * 4 > blob_bytes) return false;
  const int* b = reinterpret_cast<const int*>(h_blob + b_off);
  for (long long i = 0; i < out_size; ++i) {
    const long long lo = b[2 * i], n = b[2 * i + 1];
    if (lo < 0 || n < 0 || n > ks || lo + n > in_size) return false;
  }
  return true;
}

// h_blob: host, blob_bytes bytes: int64 jobs [B][24] first, the int32 bounds / coefficient tables behind them at the byte offsets the
// jobs name; d_blob: its device copy (uploaded by the caller on `stream` or ordered before it).  Job words: 0 source pointer
// (device uint8, element (y,x,c) at src[y*sy + x*sx + c*sc]), 1 H, 2 W, 3 sy, 4 sx, 5 sc, 6 x0, 7 y0, 8 crop w, 9 crop h, 10 new_h,
// 11 new_w, 12 xb offset (-1: new_w == crop w), 13 xk offset, 14 kxs, 15 yb offset (-1: new_h == crop h), 16 yk offset, 17 kys,
// 18 flip, 19 slot, 20 optional uint8 output pointer [new_h][new_w][3] (0: none), 21 byte offset of this job's [crop h][new_w][3]
// intermediate in tmp.  out [n_slots][Hp][Wp][4] fp32; every job's slot is written completely.  mean3 / std3: host float[3].
// launches: optional, receives the number of kernel launches issued (at most two).
extern "C" int lvc_train_input_u8(const void* h_blob, const void* d_blob, long long blob_bytes, int B, unsigned char* tmp,
                                  long long tmp_bytes, float* out, int n_slots, int Hp, int Wp, const float* mean3,
                                  const float* std3, int* launches, void* stream) {
  if (launches) *launches = 0;
  LVC_CHECK_ARG(B >= 0 && n_slots >= B && Hp > 0 && Wp > 0, "bad batch size");
  if (B == 0) return LVC_OK;
  LVC_CHECK_ARG(h_blob && d_blob && out && mean3 && std3, "null argument");
  LVC_CHECK_ARG(((uintptr_t)h_blob & 7) == 0 && ((uintptr_t)d_blob & 7) == 0, "the blob must be 8-byte aligned");
  LVC_CHECK_ARG(blob_bytes >= (long long)B * TI_FIELDS * 8, "blob smaller than its job table");
  const long long* jobs = reinterpret_cast<const long long*>(h_blob);
  const char* hb = reinterpret_cast<const char*>(h_blob);
  int gw = 0, gh = 0;
  unsigned long long slots_seen = 0;
  for (int i = 0; i < B; ++i) {
    const long long* j = jobs + (size_t)i * TI_FIELDS;
    const long long H = j[TI_H], W = j[TI_W], x0 = j[TI_X0], y0 = j[TI_Y0], cw = j[TI_CW], ch = j[TI_CH];
    const long long nh = j[TI_NEW_H], nw = j[TI_NEW_W];
    LVC_CHECK_ARG(j[TI_SRC] && H > 0 && W > 0, "bad source image");
    LVC_CHECK_ARG(j[TI_SY] > 0 && j[TI_SX] > 0 && j[TI_SC] > 0, "strides must be positive");
    LVC_CHECK_ARG(x0 >= 0 && y0 >= 0 && cw > 0 && ch > 0 && x0 + cw <= W && y0 + ch <= H, "crop window outside the image");
    LVC_CHECK_ARG(nh > 0 && nw > 0 && nh <= Hp && nw <= Wp, "output size outside the padded batch");
    LVC_CHECK_ARG(j[TI_SLOT] >= 0 && j[TI_SLOT] < n_slots, "bad slot");
    if (j[TI_SLOT] < 64) {
      LVC_CHECK_ARG(!(slots_seen >> j[TI_SLOT] & 1ull), "two jobs write one slot");
      slots_seen |= 1ull << j[TI_SLOT];
    }
    LVC_CHECK_ARG((j[TI_XB] >= 0) == (nw != cw) && (j[TI_YB] >= 0) == (nh != ch), "coefficients must match the size change");
    if (j[TI_XB] >= 0) {
      LVC_CHECK_ARG(ti_check_axis(hb, blob_bytes, j[TI_XB], j[TI_XK], j[TI_KXS], cw, nw), "bad column tables");
      LVC_CHECK_ARG(tmp && j[TI_TMP] >= 0 && j[TI_TMP] + ch * nw * 3 <= tmp_bytes, "intermediate outside the scratch buffer");
      gw = nw > gw ? (int)nw : gw;
      gh = ch > gh ? (int)ch : gh;
    }
    if (j[TI_YB] >= 0) LVC_CHECK_ARG(ti_check_axis(hb, blob_bytes, j[TI_YB], j[TI_YK], j[TI_KYS], ch, nh), "bad row tables");
  }
  hipStream_t st = (hipStream_t)stream;
  const char* db = reinterpret_cast<const char*>(d_blob);
  if (gw > 0) {
    hipLaunchKernelGGL(train_input_h_kernel, dim3(lvc_cdiv(gw, 256), gh, B), dim3(256), 0, st, db, tmp);
    LVC_CHECK_LAUNCH();
    if (launches) ++*launches;
  }
  hipLaunchKernelGGL(train_input_v_kernel, dim3(lvc_cdiv(Wp, 256), Hp, B), dim3(256), 0, st, db, tmp, out, Hp, Wp, mean3[0], mean3[1],
                     mean3[2], std3[0], std3[1], std3[2]);
  LVC_CHECK_LAUNCH();
  if (launches) ++*launches;
  return LVC_OK;
}

// ------------------------------------------------------------------------------------------------ tiled sources (mosaic)
// A job's source is a CANVAS painted from 1..9 tiles: tile t covers the canvas rectangle [x1a, x2a) x [y1a, y2a) with its pixels
// from (x1b, y1b) on; tiles are painted in order (where rectangles overlap the later one wins) and what no tile covers is 114.  The
// crop window (X0, Y0, cw, ch) is in canvas coordinates.  Two launches whatever B and whatever the mix of tile counts:
//   1. horizontal pass, grid (x tiles, rows of the largest window, B), ALWAYS run: a workgroup is one canvas row of one job, so the
//      tiles that cross it are the same for all its threads: the first wavefront finds them once (<= 9 tests, kept in paint order in
//      LDS).  A thread walks its taps through contiguous x and keeps the run [.., hi) in which the owner of a pixel does not change,
//      so the tile list is searched again only where a tap leaves that run.  A width that does not change is a copy (one tap of
//      weight 1 << 22: what Pillow's skipping the pass gives, byte for byte);
//   2. vertical pass: train_input_v_kernel's, reading the contiguous [ch][new_w][3] intermediate only.
#define TT_HEAD 20        // int64 words in front of a job's tiles
#define TT_TILE 12        // int64 words per tile
#define TT_MAX_TILES 9
#define TT_FIELDS (TT_HEAD + TT_MAX_TILES * TT_TILE)   // 128 words = 1 KiB per job (lvc_amd.h)
#define TT_FILL 114
#define TT_COORD_MAX (1ll << 30)

enum {
  TT_X0 = 0, TT_Y0, TT_CW, TT_CH, TT_NEW_H, TT_NEW_W, TT_XB, TT_XK, TT_KXS, TT_YB, TT_YK, TT_KYS, TT_FLIP, TT_SLOT, TT_U8, TT_TMP,
  TT_NT
};
enum { TL_SRC = 0, TL_H, TL_W, TL_SY, TL_SX, TL_SC, TL_X1A, TL_Y1A, TL_X2A, TL_Y2A, TL_X1B, TL_Y1B };

// canvas window row [cw] (through the tile list) -> tmp [ch][new_w][3]
__global__ __launch_bounds__(256) void train_input_tiles_h_kernel(const char* __restrict__ blob, unsigned char* __restrict__ tmp) {
  const long long* jb = reinterpret_cast<const long long*>(blob) + (size_t)blockIdx.z * TT_FIELDS;
  const int y = blockIdx.y, new_w = (int)jb[TT_NEW_W], cw = (int)jb[TT_CW];
  if (y >= (int)jb[TT_CH] || (int)(blockIdx.x * 256) >= new_w) return;   // the whole workgroup leaves: nobody waits below
  __shared__ int seg_lo[TT_MAX_TILES], seg_hi[TT_MAX_TILES], n_seg;
  __shared__ long long seg_sx[TT_MAX_TILES], seg_sc[TT_MAX_TILES];
  __shared__ const unsigned char* seg_row[TT_MAX_TILES];      // the tile's pixel under window column 0 of this row
  if (threadIdx.x < 64) {      // the first wavefront: lane t tests tile t; the crossing tiles are compacted in paint order
    const long long X0 = jb[TT_X0], Y = jb[TT_Y0] + y;
    const long long* tl = jb + TT_HEAD + (size_t)(threadIdx.x < TT_MAX_TILES ? threadIdx.x : 0) * TT_TILE;
    long long lo = 0, hi = 0;
    bool cross = false;
    if ((long long)threadIdx.x < jb[TT_NT] && Y >= tl[TL_Y1A] && Y < tl[TL_Y2A]) {
      lo = tl[TL_X1A] > X0 ? tl[TL_X1A] - X0 : 0;
      hi = tl[TL_X2A] < X0 + cw ? tl[TL_X2A] - X0 : cw;
      cross = lo < hi;
    }
    const unsigned long long m = __ballot(cross);
    if (cross) {
      const int p = __popcll(m & ((1ull << threadIdx.x) - 1ull));
      seg_lo[p] = (int)lo; seg_hi[p] = (int)hi; seg_sx[p] = tl[TL_SX]; seg_sc[p] = tl[TL_SC];
      seg_row[p] = reinterpret_cast<const unsigned char*>(tl[TL_SRC]) + (Y - tl[TL_Y1A] + tl[TL_Y1B]) * tl[TL_SY] +
                   (X0 - tl[TL_X1A] + tl[TL_X1B]) * tl[TL_SX];
    }
    if (threadIdx.x == 0) n_seg = __popcll(m);
  }
  __syncthreads();
  const int xo = blockIdx.x * 256 + threadIdx.x;
  if (xo >= new_w) return;
  int xmin = xo, cnt = 1;
  const int* k = nullptr;      // width unchanged: one tap of weight 1
  if (jb[TT_XB] >= 0) {
    const int* xb = reinterpret_cast<const int*>(blob + jb[TT_XB]);
    k = reinterpret_cast<const int*>(blob + jb[TT_XK]) + (size_t)xo * (int)jb[TT_KXS];
    xmin = xb[2 * xo]; cnt = xb[2 * xo + 1];
  }
  const int ns = n_seg;
  int run_hi = -1;                       // taps below run_hi have the owner found last
  const unsigned char* row = nullptr;    // its row (nullptr: no tile, the fill colour)
  long long sx = 0, sc = 0;
  int s0 = 1 << (TI_PREC - 1), s1 = s0, s2 = s0;
  for (int t = 0; t < cnt; ++t) {
    const int x = xmin + t;
    if (x >= run_hi) {      // the last tile that covers x owns it; the run ends where that tile ends or a later one begins
      row = nullptr; run_hi = cw;
      for (int i = 0; i < ns; ++i) {
        const int lo = seg_lo[i], hi = seg_hi[i];
        if (lo <= x && x < hi) { row = seg_row[i]; sx = seg_sx[i]; sc = seg_sc[i]; run_hi = hi; }
        else if (lo > x && lo < run_hi) run_hi = lo;
      }
    }
    int p0 = TT_FILL, p1 = TT_FILL, p2 = TT_FILL;
    if (row) {
      const unsigned char* p = row + x * sx;
      p0 = p[0]; p1 = p[sc]; p2 = p[2 * sc];
    }
    const int c = k ? k[t] : 1 << TI_PREC;
    s0 += p0 * c; s1 += p1 * c; s2 += p2 * c;
  }
  unsigned char* o = tmp + jb[TT_TMP] + ((size_t)y * new_w + xo) * 3;
  o[0] = ti_clip8(s0); o[1] = ti_clip8(s1); o[2] = ti_clip8(s2);
}

// tmp [ch][new_w][3] -> the job's slot (and its optional uint8 output): train_input_v_kernel on the tiled job table
__global__ __launch_bounds__(256) void train_input_tiles_v_kernel(const char* __restrict__ blob, const unsigned char* __restrict__ tmp,
                                                                  float* __restrict__ out, int Hp, int Wp, float m0, float m1,
                                                                  float m2, float d0, float d1, float d2) {
  const long long* jb = reinterpret_cast<const long long*>(blob) + (size_t)blockIdx.z * TT_FIELDS;
  const int xo = blockIdx.x * 256 + threadIdx.x, yo = blockIdx.y;
  if (xo >= Wp) return;
  const int new_h = (int)jb[TT_NEW_H], new_w = (int)jb[TT_NEW_W];
  float4 v = {0.f, 0.f, 0.f, 0.f};
  if (yo < new_h && xo < new_w) {
    const int xs = jb[TT_FLIP] ? new_w - 1 - xo : xo;   // HFlipTransform(new_w) after the resize
    const unsigned char* col = tmp + jb[TT_TMP] + (size_t)xs * 3;
    const long long sy = (long long)new_w * 3;
    unsigned char r0, r1, r2;
    if (jb[TT_YB] >= 0) {
      const int* yb = reinterpret_cast<const int*>(blob + jb[TT_YB]);
      const int* k = reinterpret_cast<const int*>(blob + jb[TT_YK]) + (size_t)yo * (int)jb[TT_KYS];
      const int ymin = yb[2 * yo], cnt = yb[2 * yo + 1];
      int s0 = 1 << (TI_PREC - 1), s1 = s0, s2 = s0;
      for (int y = 0; y < cnt; ++y) {
        const unsigned char* p = col + (ymin + y) * sy;
        const int c = k[y];
        s0 += p[0] * c; s1 += p[1] * c; s2 += p[2] * c;
      }
      r0 = ti_clip8(s0); r1 = ti_clip8(s1); r2 = ti_clip8(s2);
    } else {   // height unchanged: Pillow skips the vertical pass
      const unsigned char* p = col + yo * sy;
      r0 = p[0]; r1 = p[1]; r2 = p[2];
    }
    if (jb[TT_U8]) {
      unsigned char* o = reinterpret_cast<unsigned char*>(jb[TT_U8]) + ((size_t)yo * new_w + xo) * 3;
      o[0] = r0; o[1] = r1; o[2] = r2;
    }
    v.x = ((float)r0 - m0) / d0;
    v.y = ((float)r1 - m1) / d1;
    v.z = ((float)r2 - m2) / d2;
  }
  *reinterpret_cast<float4*>(out + (((size_t)jb[TT_SLOT] * Hp + yo) * Wp + xo) * 4) = v;
}

// h_blob / d_blob / blob_bytes as lvc_train_input_u8, with int64 jobs [B][128] first.  Job words: 0 X0, 1 Y0, 2 cw, 3 ch (the crop
// window in canvas coordinates), 4 new_h, 5 new_w, 6 xb offset (-1: new_w == cw), 7 xk offset, 8 kxs, 9 yb offset (-1: new_h == ch),
// 10 yk offset, 11 kys, 12 flip, 13 slot, 14 optional uint8 output pointer [new_h][new_w][3] (0: none), 15 byte offset of the job's
// [ch][new_w][3] intermediate in tmp (always used), 16 number of tiles (1..9), 17-19 reserved; tile t at words 20 + 12 t: 0 source
// pointer (device uint8, element (y,x,c) at src[y*sy + x*sx + c*sc]), 1 H, 2 W, 3 sy, 4 sx, 5 sc, 6 x1a, 7 y1a, 8 x2a, 9 y2a (its
// canvas rectangle), 10 x1b, 11 y1b (the tile pixel at the rectangle's first corner).  Checked on the host copy before anything is
// launched: every pixel of a rectangle that the window sees lies inside its tile, every tap inside the window, outputs and intermediates inside
// their buffers, no slot written twice.  launches: optional, the number of kernel launches issued (two).
extern "C" int lvc_train_input_tiles_u8(const void* h_blob, const void* d_blob, long long blob_bytes, int B, unsigned char* tmp,
                                        long long tmp_bytes, float* out, int n_slots, int Hp, int Wp, const float* mean3,
                                        const float* std3, int* launches, void* stream) {
  if (launches) *launches = 0;
  LVC_CHECK_ARG(B >= 0 && n_slots >= B && Hp > 0 && Wp > 0, "bad batch size");
  if (B == 0) return LVC_OK;
  LVC_CHECK_ARG(h_blob && d_blob && out && tmp && mean3 && std3, "null argument");
  LVC_CHECK_ARG(((uintptr_t)h_blob & 7) == 0 && ((uintptr_t)d_blob & 7) == 0, "the blob must be 8-byte aligned");
  LVC_CHECK_ARG(blob_bytes >= (long long)B * TT_FIELDS * 8, "blob smaller than its job table");
  const long long* jobs = reinterpret_cast<const long long*>(h_blob);
  const char* hb = reinterpret_cast<const char*>(h_blob);
  int gw = 0, gh = 0;
  unsigned long long slots_seen = 0;
  for (int i = 0; i < B; ++i) {
    const long long* j = jobs + (size_t)i * TT_FIELDS;
    const long long X0 = j[TT_X0], Y0 = j[TT_Y0], cw = j[TT_CW], ch = j[TT_CH], nh = j[TT_NEW_H], nw = j[TT_NEW_W];
    LVC_CHECK_ARG(j[TT_NT] >= 1 && j[TT_NT] <= TT_MAX_TILES, "a job has 1 to 9 tiles");
    LVC_CHECK_ARG(X0 >= 0 && Y0 >= 0 && cw > 0 && ch > 0 && X0 < TT_COORD_MAX && Y0 < TT_COORD_MAX && cw < TT_COORD_MAX &&
                  ch < TT_COORD_MAX, "bad crop window");
    for (int t = 0; t < (int)j[TT_NT]; ++t) {
      const long long* tl = j + TT_HEAD + (size_t)t * TT_TILE;
      LVC_CHECK_ARG(tl[TL_SRC] && tl[TL_H] > 0 && tl[TL_W] > 0 && tl[TL_H] < TT_COORD_MAX && tl[TL_W] < TT_COORD_MAX, "bad tile image");
      LVC_CHECK_ARG(tl[TL_SY] > 0 && tl[TL_SX] > 0 && tl[TL_SC] > 0, "strides must be positive");
      for (int f = TL_X1A; f <= TL_Y1B; ++f) LVC_CHECK_ARG(tl[f] > -TT_COORD_MAX && tl[f] < TT_COORD_MAX, "tile coordinate out of range");
      LVC_CHECK_ARG(tl[TL_X2A] >= tl[TL_X1A] && tl[TL_Y2A] >= tl[TL_Y1A], "canvas rectangle with negative extent");
      const long long lx = tl[TL_X1A] > X0 ? tl[TL_X1A] : X0, hx = tl[TL_X2A] < X0 + cw ? tl[TL_X2A] : X0 + cw;
      const long long ly = tl[TL_Y1A] > Y0 ? tl[TL_Y1A] : Y0, hy = tl[TL_Y2A] < Y0 + ch ? tl[TL_Y2A] : Y0 + ch;
      if (lx < hx && ly < hy)      // the part of the tile's rectangle the window sees: read from inside the tile
        LVC_CHECK_ARG(lx - tl[TL_X1A] + tl[TL_X1B] >= 0 && hx - tl[TL_X1A] + tl[TL_X1B] <= tl[TL_W] &&
                      ly - tl[TL_Y1A] + tl[TL_Y1B] >= 0 && hy - tl[TL_Y1A] + tl[TL_Y1B] <= tl[TL_H], "a tile is read outside its image");
    }
    LVC_CHECK_ARG(nh > 0 && nw > 0 && nh <= Hp && nw <= Wp, "output size outside the padded batch");
    LVC_CHECK_ARG(j[TT_SLOT] >= 0 && j[TT_SLOT] < n_slots, "bad slot");
    if (j[TT_SLOT] < 64) {
      LVC_CHECK_ARG(!(slots_seen >> j[TT_SLOT] & 1ull), "two jobs write one slot");
      slots_seen |= 1ull << j[TT_SLOT];
    }
    LVC_CHECK_ARG((j[TT_XB] >= 0) == (nw != cw) && (j[TT_YB] >= 0) == (nh != ch), "coefficients must match the size change");
    if (j[TT_XB] >= 0) LVC_CHECK_ARG(ti_check_axis(hb, blob_bytes, j[TT_XB], j[TT_XK], j[TT_KXS], cw, nw), "bad column tables");
    if (j[TT_YB] >= 0) LVC_CHECK_ARG(ti_check_axis(hb, blob_bytes, j[TT_YB], j[TT_YK], j[TT_KYS], ch, nh), "bad row tables");
    LVC_CHECK_ARG(j[TT_TMP] >= 0 && j[TT_TMP] <= tmp_bytes && ch * nw * 3 <= tmp_bytes - j[TT_TMP], "intermediate outside the scratch buffer");
    gw = nw > gw ? (int)nw : gw;
    gh = ch > gh ? (int)ch : gh;
  }
  hipStream_t st = (hipStream_t)stream;
  const char* db = reinterpret_cast<const char*>(d_blob);
  hipLaunchKernelGGL(train_input_tiles_h_kernel, dim3(lvc_cdiv(gw, 256), gh, B), dim3(256), 0, st, db, tmp);
  LVC_CHECK_LAUNCH();
  if (launches) ++*launches;
  hipLaunchKernelGGL(train_input_tiles_v_kernel, dim3(lvc_cdiv(Wp, 256), Hp, B), dim3(256), 0, st, db, tmp, out, Hp, Wp, mean3[0],
                     mean3[1], mean3[2], std3[0], std3[1], std3[2]);
  LVC_CHECK_LAUNCH();
  if (launches) ++*launches;
  return LVC_OK;
}

// ------------------------------------------------------------------------------------------------ large-scale jitter (INPUT.LSJ)
// ResizeScale -> FixedSizeCrop -> RandomFlip (reference detectron2/data/transforms/augmentation_impl.py:123-161, 391-431): the crop
// window of a tiled job is resized WHOLE to sh x sw (Pillow's tables for the full cw -> sw / ch -> sh resize: support and weights
// depend on the full sizes), the window (ox, oy, ow, oh) of that scaled image lands at the top left of a th x tw canvas filled with
// `fill` at its right and bottom, and the canvas is mirrored where the job says so.  The scaled image never exists: the window only
// selects columns and rows of the tables.  Two launches whatever B and the mix:
//   1. horizontal pass, grid (x tiles, rows of the largest band, B), always run (a copy where the width stays): output columns
//      [ox, ox + ow) of the source rows [by0, by0 + bh) of the crop window -- the band the vertical taps of rows [oy, oy + oh) touch
//      (those rows themselves where the height stays) -- through the tile list, as train_input_tiles_h_kernel -> tmp [bh][ow][3];
//   2. vertical pass, grid (x tiles, Hp, B): thread (yo, xo) owns OUTPUT pixel (yo, xo) of its slot; its canvas column before the
//      flip is xc = flip ? tw-1-xo : xo; inside oh x ow it resamples column xc of tmp with the taps of scaled row oy + yo, elsewhere
//      inside the canvas it is the fill; both are normalised as above; outside the canvas it is the batch's zero padding.
#define LJ_HEAD 32        // int64 words in front of a job's tiles
#define LJ_FIELDS (LJ_HEAD + TT_MAX_TILES * TT_TILE)   // 140 words per job (lvc_amd.h)

enum {
  LJ_X0 = 0, LJ_Y0, LJ_CW, LJ_CH, LJ_SH, LJ_SW, LJ_XB, LJ_XK, LJ_KXS, LJ_YB, LJ_YK, LJ_KYS, LJ_FLIP, LJ_SLOT, LJ_U8, LJ_TMP, LJ_NT,
  LJ_OX, LJ_OY, LJ_OW, LJ_OH, LJ_TH, LJ_TW, LJ_FILL, LJ_BY0, LJ_BH
};

// rows [by0, by0 + bh) of the crop window (through the tile list), scaled columns [ox, ox + ow) -> tmp [bh][ow][3]
__global__ __launch_bounds__(256) void train_input_lsj_h_kernel(const char* __restrict__ blob, unsigned char* __restrict__ tmp) {
  const long long* jb = reinterpret_cast<const long long*>(blob) + (size_t)blockIdx.z * LJ_FIELDS;
  const int y = blockIdx.y, ow = (int)jb[LJ_OW], cw = (int)jb[LJ_CW];
  if (y >= (int)jb[LJ_BH] || (int)(blockIdx.x * 256) >= ow) return;   // the whole workgroup leaves: nobody waits below
  __shared__ int seg_lo[TT_MAX_TILES], seg_hi[TT_MAX_TILES], n_seg;
  __shared__ long long seg_sx[TT_MAX_TILES], seg_sc[TT_MAX_TILES];
  __shared__ const unsigned char* seg_row[TT_MAX_TILES];      // the tile's pixel under window column 0 of this row
  if (threadIdx.x < 64) {      // the first wavefront: lane t tests tile t; the crossing tiles are compacted in paint order
    const long long X0 = jb[LJ_X0], Y = jb[LJ_Y0] + jb[LJ_BY0] + y;
    const long long* tl = jb + LJ_HEAD + (size_t)(threadIdx.x < TT_MAX_TILES ? threadIdx.x : 0) * TT_TILE;
    long long lo = 0, hi = 0;
    bool cross = false;
    if ((long long)threadIdx.x < jb[LJ_NT] && Y >= tl[TL_Y1A] && Y < tl[TL_Y2A]) {
      lo = tl[TL_X1A] > X0 ? tl[TL_X1A] - X0 : 0;
      hi = tl[TL_X2A] < X0 + cw ? tl[TL_X2A] - X0 : cw;
      cross = lo < hi;
    }
    const unsigned long long m = __ballot(cross);
    if (cross) {
      const int p = __popcll(m & ((1ull << threadIdx.x) - 1ull));
      seg_lo[p] = (int)lo; seg_hi[p] = (int)hi; seg_sx[p] = tl[TL_SX]; seg_sc[p] = tl[TL_SC];
      seg_row[p] = reinterpret_cast<const unsigned char*>(tl[TL_SRC]) + (Y - tl[TL_Y1A] + tl[TL_Y1B]) * tl[TL_SY] +
                   (X0 - tl[TL_X1A] + tl[TL_X1B]) * tl[TL_SX];
    }
    if (threadIdx.x == 0) n_seg = __popcll(m);
  }
  __syncthreads();
  const int xo = blockIdx.x * 256 + threadIdx.x;
  if (xo >= ow) return;
  const int xs = (int)jb[LJ_OX] + xo;      // the column of the scaled image
  int xmin = xs, cnt = 1;
  const int* k = nullptr;      // width unchanged: one tap of weight 1
  if (jb[LJ_XB] >= 0) {
    const int* xb = reinterpret_cast<const int*>(blob + jb[LJ_XB]);
    k = reinterpret_cast<const int*>(blob + jb[LJ_XK]) + (size_t)xs * (int)jb[LJ_KXS];
    xmin = xb[2 * xs]; cnt = xb[2 * xs + 1];
  }
  const int ns = n_seg;
  int run_hi = -1;                       // taps below run_hi have the owner found last
  const unsigned char* row = nullptr;    // its row (nullptr: no tile, the mosaic's fill colour)
  long long sx = 0, sc = 0;
  int s0 = 1 << (TI_PREC - 1), s1 = s0, s2 = s0;
  for (int t = 0; t < cnt; ++t) {
    const int x = xmin + t;
    if (x >= run_hi) {      // the last tile that covers x owns it; the run ends where that tile ends or a later one begins
      row = nullptr; run_hi = cw;
      for (int i = 0; i < ns; ++i) {
        const int lo = seg_lo[i], hi = seg_hi[i];
        if (lo <= x && x < hi) { row = seg_row[i]; sx = seg_sx[i]; sc = seg_sc[i]; run_hi = hi; }
        else if (lo > x && lo < run_hi) run_hi = lo;
      }
    }
    int p0 = TT_FILL, p1 = TT_FILL, p2 = TT_FILL;
    if (row) {
      const unsigned char* p = row + x * sx;
      p0 = p[0]; p1 = p[sc]; p2 = p[2 * sc];
    }
    const int c = k ? k[t] : 1 << TI_PREC;
    s0 += p0 * c; s1 += p1 * c; s2 += p2 * c;
  }
  unsigned char* o = tmp + jb[LJ_TMP] + ((size_t)y * ow + xo) * 3;
  o[0] = ti_clip8(s0); o[1] = ti_clip8(s1); o[2] = ti_clip8(s2);
}

// tmp [bh][ow][3] -> the job's slot (and its optional uint8 canvas [th][tw][3])
__global__ __launch_bounds__(256) void train_input_lsj_v_kernel(const char* __restrict__ blob, const unsigned char* __restrict__ tmp,
                                                                float* __restrict__ out, int Hp, int Wp, float m0, float m1, float m2,
                                                                float d0, float d1, float d2) {
  const long long* jb = reinterpret_cast<const long long*>(blob) + (size_t)blockIdx.z * LJ_FIELDS;
  const int xo = blockIdx.x * 256 + threadIdx.x, yo = blockIdx.y;
  if (xo >= Wp) return;
  const int th = (int)jb[LJ_TH], tw = (int)jb[LJ_TW];
  float4 v = {0.f, 0.f, 0.f, 0.f};
  if (yo < th && xo < tw) {
    const int xc = jb[LJ_FLIP] ? tw - 1 - xo : xo;   // HFlipTransform(tw) on the padded canvas: the fill moves to the left
    const int ow = (int)jb[LJ_OW];
    unsigned char r0, r1, r2;
    r0 = r1 = r2 = (unsigned char)jb[LJ_FILL];
    if (yo < (int)jb[LJ_OH] && xc < ow) {
      const unsigned char* col = tmp + jb[LJ_TMP] + (size_t)xc * 3;
      const long long sy = (long long)ow * 3;
      const int ys = (int)jb[LJ_OY] + yo, by0 = (int)jb[LJ_BY0];      // the row of the scaled image; the band's first source row
      if (jb[LJ_YB] >= 0) {
        const int* yb = reinterpret_cast<const int*>(blob + jb[LJ_YB]);
        const int* k = reinterpret_cast<const int*>(blob + jb[LJ_YK]) + (size_t)ys * (int)jb[LJ_KYS];
        const int ymin = yb[2 * ys] - by0, cnt = yb[2 * ys + 1];
        int s0 = 1 << (TI_PREC - 1), s1 = s0, s2 = s0;
        for (int y = 0; y < cnt; ++y) {
          const unsigned char* p = col + (ymin + y) * sy;
          const int c = k[y];
          s0 += p[0] * c; s1 += p[1] * c; s2 += p[2] * c;
        }
        r0 = ti_clip8(s0); r1 = ti_clip8(s1); r2 = ti_clip8(s2);
      } else {   // height unchanged: Pillow skips the vertical pass
        const unsigned char* p = col + (ys - by0) * sy;
        r0 = p[0]; r1 = p[1]; r2 = p[2];
      }
    }
    if (jb[LJ_U8]) {
      unsigned char* o = reinterpret_cast<unsigned char*>(jb[LJ_U8]) + ((size_t)yo * tw + xo) * 3;
      o[0] = r0; o[1] = r1; o[2] = r2;
    }
    v.x = ((float)r0 - m0) / d0;
    v.y = ((float)r1 - m1) / d1;
    v.z = ((float)r2 - m2) / d2;
  }
  *reinterpret_cast<float4*>(out + (((size_t)jb[LJ_SLOT] * Hp + yo) * Wp + xo) * 4) = v;
}

// h_blob / d_blob / blob_bytes as lvc_train_input_tiles_u8, with int64 jobs [B][140] first.  Job words: 0 X0, 1 Y0, 2 cw, 3 ch (the
// crop window in canvas coordinates: what is resized), 4 sh, 5 sw (the size of the WHOLE scaled image), 6 xb offset (-1: sw == cw),
// 7 xk offset, 8 kxs, 9 yb offset (-1: sh == ch), 10 yk offset, 11 kys (the tables of the full cw -> sw / ch -> sh resize), 12 flip,
// 13 slot, 14 optional uint8 output pointer [th][tw][3] (0: none), 15 byte offset of the job's [bh][ow][3] intermediate in tmp,
// 16 number of tiles (1..9), 17 ox, 18 oy, 19 ow, 20 oh (the output window inside the scaled image), 21 th, 22 tw (the canvas),
// 23 fill byte, 24 by0, 25 bh (the band of crop-window rows the horizontal pass produces), 26-31 reserved; tile t at words
// 32 + 12 t as in lvc_train_input_tiles_u8.  Checked on the host copy before anything is launched: what lvc_train_input_tiles_u8
// checks of a window and its tiles, the output window inside the scaled image and not larger than the canvas, the canvas inside the
// padded batch, the band inside the crop window, every tap of the window's columns inside the crop window and of its rows inside the
// band, the intermediate inside tmp and apart from every other job's, no slot written twice.  launches: optional, the number of kernel launches issued (two).
extern "C" int lvc_train_input_lsj_u8(const void* h_blob, const void* d_blob, long long blob_bytes, int B, unsigned char* tmp,
                                      long long tmp_bytes, float* out, int n_slots, int Hp, int Wp, const float* mean3,
                                      const float* std3, int* launches, void* stream) {
  if (launches) *launches = 0;
  LVC_CHECK_ARG(B >= 0 && n_slots >= B && Hp > 0 && Wp > 0, "bad batch size");
  if (B == 0) return LVC_OK;
  LVC_CHECK_ARG(h_blob && d_blob && out && tmp && mean3 && std3, "null argument");
  LVC_CHECK_ARG(((uintptr_t)h_blob & 7) == 0 && ((uintptr_t)d_blob & 7) == 0, "the blob must be 8-byte aligned");
  LVC_CHECK_ARG(blob_bytes >= (long long)B * LJ_FIELDS * 8, "blob smaller than its job table");
  const long long* jobs = reinterpret_cast<const long long*>(h_blob);
  const char* hb = reinterpret_cast<const char*>(h_blob);
  int gw = 0, gh = 0;
  unsigned long long slots_seen = 0;
  for (int i = 0; i < B; ++i) {
    const long long* j = jobs + (size_t)i * LJ_FIELDS;
    const long long X0 = j[LJ_X0], Y0 = j[LJ_Y0], cw = j[LJ_CW], ch = j[LJ_CH], sh = j[LJ_SH], sw = j[LJ_SW];
    const long long ox = j[LJ_OX], oy = j[LJ_OY], ow = j[LJ_OW], oh = j[LJ_OH], th = j[LJ_TH], tw = j[LJ_TW];
    const long long by0 = j[LJ_BY0], bh = j[LJ_BH];
    LVC_CHECK_ARG(j[LJ_NT] >= 1 && j[LJ_NT] <= TT_MAX_TILES, "a job has 1 to 9 tiles");
    LVC_CHECK_ARG(X0 >= 0 && Y0 >= 0 && cw > 0 && ch > 0 && X0 < TT_COORD_MAX && Y0 < TT_COORD_MAX && cw < TT_COORD_MAX &&
                  ch < TT_COORD_MAX, "bad crop window");
    for (int t = 0; t < (int)j[LJ_NT]; ++t) {
      const long long* tl = j + LJ_HEAD + (size_t)t * TT_TILE;
      LVC_CHECK_ARG(tl[TL_SRC] && tl[TL_H] > 0 && tl[TL_W] > 0 && tl[TL_H] < TT_COORD_MAX && tl[TL_W] < TT_COORD_MAX, "bad tile image");
      LVC_CHECK_ARG(tl[TL_SY] > 0 && tl[TL_SX] > 0 && tl[TL_SC] > 0, "strides must be positive");
      for (int f = TL_X1A; f <= TL_Y1B; ++f) LVC_CHECK_ARG(tl[f] > -TT_COORD_MAX && tl[f] < TT_COORD_MAX, "tile coordinate out of range");
      LVC_CHECK_ARG(tl[TL_X2A] >= tl[TL_X1A] && tl[TL_Y2A] >= tl[TL_Y1A], "canvas rectangle with negative extent");
      const long long lx = tl[TL_X1A] > X0 ? tl[TL_X1A] : X0, hx = tl[TL_X2A] < X0 + cw ? tl[TL_X2A] : X0 + cw;
      const long long ly = tl[TL_Y1A] > Y0 ? tl[TL_Y1A] : Y0, hy = tl[TL_Y2A] < Y0 + ch ? tl[TL_Y2A] : Y0 + ch;
      if (lx < hx && ly < hy)      // the part of the tile's rectangle the crop window sees: read from inside the tile
        LVC_CHECK_ARG(lx - tl[TL_X1A] + tl[TL_X1B] >= 0 && hx - tl[TL_X1A] + tl[TL_X1B] <= tl[TL_W] &&
                      ly - tl[TL_Y1A] + tl[TL_Y1B] >= 0 && hy - tl[TL_Y1A] + tl[TL_Y1B] <= tl[TL_H], "a tile is read outside its image");
    }
    LVC_CHECK_ARG(sh > 0 && sw > 0 && sh < TT_COORD_MAX && sw < TT_COORD_MAX, "bad scaled size");
    LVC_CHECK_ARG(ox >= 0 && oy >= 0 && ow > 0 && oh > 0 && ox <= sw - ow && oy <= sh - oh, "output window outside the scaled image");
    LVC_CHECK_ARG(th > 0 && tw > 0 && ow <= tw && oh <= th && th <= Hp && tw <= Wp, "canvas outside the padded batch or smaller than its window");
    LVC_CHECK_ARG(j[LJ_FILL] >= 0 && j[LJ_FILL] <= 255, "the fill is a byte");
    LVC_CHECK_ARG(j[LJ_SLOT] >= 0 && j[LJ_SLOT] < n_slots, "bad slot");
    if (j[LJ_SLOT] < 64) {
      LVC_CHECK_ARG(!(slots_seen >> j[LJ_SLOT] & 1ull), "two jobs write one slot");
      slots_seen |= 1ull << j[LJ_SLOT];
    }
    LVC_CHECK_ARG((j[LJ_XB] >= 0) == (sw != cw) && (j[LJ_YB] >= 0) == (sh != ch), "coefficients must match the size change");
    LVC_CHECK_ARG(by0 >= 0 && bh > 0 && by0 <= ch - bh, "band outside the crop window");
    if (j[LJ_XB] >= 0) LVC_CHECK_ARG(ti_check_axis(hb, blob_bytes, j[LJ_XB], j[LJ_XK], j[LJ_KXS], cw, sw), "bad column tables");
    if (j[LJ_YB] >= 0) {
      LVC_CHECK_ARG(ti_check_axis(hb, blob_bytes, j[LJ_YB], j[LJ_YK], j[LJ_KYS], ch, sh), "bad row tables");
      const int* b = reinterpret_cast<const int*>(hb + j[LJ_YB]);
      for (long long r = oy; r < oy + oh; ++r)
        LVC_CHECK_ARG(b[2 * r] >= by0 && (long long)b[2 * r] + b[2 * r + 1] <= by0 + bh, "row taps outside the band");
    } else {
      LVC_CHECK_ARG(by0 <= oy && oy + oh <= by0 + bh, "output rows outside the band");
    }
    LVC_CHECK_ARG(j[LJ_TMP] >= 0 && j[LJ_TMP] <= tmp_bytes && bh * ow * 3 <= tmp_bytes - j[LJ_TMP], "intermediate outside the scratch buffer");
    for (int k = 0; k < i; ++k) {      // both passes of all jobs run side by side: no two intermediates may share a byte
      const long long* o = jobs + (size_t)k * LJ_FIELDS;
      LVC_CHECK_ARG(j[LJ_TMP] + bh * ow * 3 <= o[LJ_TMP] || o[LJ_TMP] + o[LJ_BH] * o[LJ_OW] * 3 <= j[LJ_TMP],
                    "two jobs share bytes of the intermediate");
    }
    gw = ow > gw ? (int)ow : gw;
    gh = bh > gh ? (int)bh : gh;
  }
  hipStream_t st = (hipStream_t)stream;
  const char* db = reinterpret_cast<const char*>(d_blob);
  hipLaunchKernelGGL(train_input_lsj_h_kernel, dim3(lvc_cdiv(gw, 256), gh, B), dim3(256), 0, st, db, tmp);
  LVC_CHECK_LAUNCH();
  if (launches) ++*launches;
  hipLaunchKernelGGL(train_input_lsj_v_kernel, dim3(lvc_cdiv(Wp, 256), Hp, B), dim3(256), 0, st, db, tmp, out, Hp, Wp, mean3[0],
                     mean3[1], mean3[2], std3[0], std3[1], std3[2]);
  LVC_CHECK_LAUNCH();
  if (launches) ++*launches;
  return LVC_OK;
}
