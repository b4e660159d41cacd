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
