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
// The resample is resize.hip's (input_common.h), bit for bit: Pillow's 22-bit coefficients for the CROPPED size -> the output size
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
#include "input_common.h"

#define TI_FIELDS 24   // int64 words per job (lvc_amd.h)
#define TT_FIELDS (TL_HEAD + TL_MAX_TILES * TL_WORDS)       // 128 words = 1 KiB per tiles job (lvc_amd.h)
#define LJ_FIELDS (TL_HEAD_LSJ + TL_MAX_TILES * TL_WORDS)   // 140 words per LSJ job (lvc_amd.h)

enum {
  TI_SRC = 0, TI_H, TI_W, TI_SY, TI_SX, TI_SC, TI_X0, TI_Y0, TI_CW, TI_CH, TI_NEW_H, TI_NEW_W, TI_XB, TI_XK, TI_KXS, TI_YB, TI_YK,
  TI_KYS, TI_FLIP, TI_SLOT, TI_U8, TI_TMP
};

// resample_v_pixel with the row tables of a blob job: yw[0..2] = the job's words (yb offset, -1 where the height does not change;
// yk offset; kys)
template <typename T, typename C>
__device__ __forceinline__ void ti_v_pixel(const unsigned char* col, T sy, C sc, const char* blob, const long long* yw, int ys,
                                           int y_first, unsigned char& r0, unsigned char& r1, unsigned char& r2) {
  const bool rows = yw[0] >= 0;
  resample_v_pixel(col, sy, sc, rows ? reinterpret_cast<const int*>(blob + yw[0]) : nullptr,
                   rows ? reinterpret_cast<const int*>(blob + yw[1]) : nullptr, (int)yw[2], ys, y_first, r0, r1, r2);
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
  const int* k = reinterpret_cast<const int*>(blob + jb[TI_XK]) + (size_t)xo * (int)jb[TI_KXS];
  const unsigned char* row = reinterpret_cast<const unsigned char*>(jb[TI_SRC]) + (jb[TI_Y0] + y) * sy + (jb[TI_X0] + xb[2 * xo]) * sx;
  unsigned char* o = tmp + jb[TI_TMP] + ((size_t)y * new_w + xo) * 3;
  resample_taps(row, 0, sx, sc, k, xb[2 * xo + 1], o[0], o[1], o[2]);
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
    } else {      // width unchanged: the strided source is read in place
      sy = jb[TI_SY]; sc = jb[TI_SC];
      col = reinterpret_cast<const unsigned char*>(jb[TI_SRC]) + jb[TI_Y0] * sy + (jb[TI_X0] + xs) * jb[TI_SX];
    }
    unsigned char r0, r1, r2;
    ti_v_pixel(col, sy, sc, blob, jb + TI_YB, yo, 0, r0, r1, r2);
    if (jb[TI_U8]) {
      unsigned char* o = reinterpret_cast<unsigned char*>(jb[TI_U8]) + ((size_t)yo * new_w + xo) * 3;
      o[0] = r0; o[1] = r1; o[2] = r2;
    }
    v = normalise4(r0, r1, r2, m0, m1, m2, d0, d1, d2);
  }
  *reinterpret_cast<float4*>(out + (((size_t)jb[TI_SLOT] * Hp + yo) * Wp + xo) * 4) = v;
}

// Job words and arguments: include/lvc_amd.h.  The host copy of the blob is checked before anything is launched; every job's slot
// is written completely.  launches: optional, receives the number of kernel launches issued (at most two).
extern "C" int lvc_train_input_u8(const void* h_blob, const void* d_blob, long long blob_bytes, int B, unsigned char* tmp,
                                  long long tmp_bytes, float* out, int n_slots, int Hp, int Wp, const float* mean3,
                                  const float* std3, int* launches, void* stream) {
  if (launches) *launches = 0;
  LVC_CHECK_ARG(B >= 0 && n_slots >= B && Hp > 0 && Wp > 0, "bad batch size");
  if (B == 0) return LVC_OK;
  LVC_CHECK_ARG(out && mean3 && std3, "null argument");
  LVC_CHECK_MSG(check_blob(h_blob, d_blob, blob_bytes, B, TI_FIELDS));
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
    LVC_CHECK_MSG(check_slot(j[TI_SLOT], n_slots, slots_seen));
    LVC_CHECK_ARG((j[TI_XB] >= 0) == (nw != cw) && (j[TI_YB] >= 0) == (nh != ch), "coefficients must match the size change");
    if (j[TI_XB] >= 0) {
      LVC_CHECK_ARG(check_axis(hb, blob_bytes, j[TI_XB], j[TI_XK], j[TI_KXS], cw, nw), "bad column tables");
      LVC_CHECK_ARG(tmp && j[TI_TMP] >= 0 && j[TI_TMP] + ch * nw * 3 <= tmp_bytes, "intermediate outside the scratch buffer");
      gw = nw > gw ? (int)nw : gw;
      gh = ch > gh ? (int)ch : gh;
    }
    if (j[TI_YB] >= 0) LVC_CHECK_ARG(check_axis(hb, blob_bytes, j[TI_YB], j[TI_YK], j[TI_KYS], ch, nh), "bad row tables");
  }
  hipStream_t st = (hipStream_t)stream;
  const char* db = reinterpret_cast<const char*>(d_blob);
  if (gw > 0) {      // no width changes: no horizontal launch
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
// The crop window (X0, Y0, cw, ch) of a job lies on a canvas painted from 1..9 tiles (input_common.h).  Two launches whatever B and
// whatever the mix of tile counts:
//   1. horizontal pass, grid (x tiles, rows of the largest window, B), ALWAYS run: tiles_h_pass over the whole window;
//   2. vertical pass: train_input_v_kernel's, reading the contiguous [ch][new_w][3] intermediate only.
__global__ __launch_bounds__(256) void train_input_tiles_h_kernel(const char* __restrict__ blob, unsigned char* __restrict__ tmp) {
  const long long* jb = reinterpret_cast<const long long*>(blob) + (size_t)blockIdx.z * TT_FIELDS;
  tiles_h_pass(blob, jb, jb + TL_HEAD, tmp, 0, (int)jb[TJ_CH], 0, (int)jb[TJ_NEW_W]);
}

// tmp [ch][new_w][3] -> the job's slot (and its optional uint8 output)
__global__ __launch_bounds__(256) void train_input_tiles_v_kernel(const char* __restrict__ blob, const unsigned char* __restrict__ tmp,
                                                                  float* __restrict__ out, int Hp, int Wp, float m0, float m1,
                                                                  float m2, float d0, float d1, float d2) {
  const long long* jb = reinterpret_cast<const long long*>(blob) + (size_t)blockIdx.z * TT_FIELDS;
  const int xo = blockIdx.x * 256 + threadIdx.x, yo = blockIdx.y;
  if (xo >= Wp) return;
  const int new_h = (int)jb[TJ_NEW_H], new_w = (int)jb[TJ_NEW_W];
  float4 v = {0.f, 0.f, 0.f, 0.f};
  if (yo < new_h && xo < new_w) {
    const int xs = jb[TJ_FLIP] ? new_w - 1 - xo : xo;   // HFlipTransform(new_w) after the resize
    unsigned char r0, r1, r2;
    ti_v_pixel(tmp + jb[TJ_TMP] + (size_t)xs * 3, (long long)new_w * 3, 1, blob, jb + TJ_YB, yo, 0, r0, r1, r2);
    if (jb[TJ_U8]) {
      unsigned char* o = reinterpret_cast<unsigned char*>(jb[TJ_U8]) + ((size_t)yo * new_w + xo) * 3;
      o[0] = r0; o[1] = r1; o[2] = r2;
    }
    v = normalise4(r0, r1, r2, m0, m1, m2, d0, d1, d2);
  }
  *reinterpret_cast<float4*>(out + (((size_t)jb[TJ_SLOT] * Hp + yo) * Wp + xo) * 4) = v;
}

// Job words and arguments: include/lvc_amd.h.  Checked on the host copy before anything is launched: every pixel of a rectangle
// that the window sees lies inside its tile, every tap inside the window, outputs and intermediates inside their buffers, no slot
// written twice.  launches: optional, the number of kernel launches issued (two).
extern "C" int lvc_train_input_tiles_u8(const void* h_blob, const void* d_blob, long long blob_bytes, int B, unsigned char* tmp,
                                        long long tmp_bytes, float* out, int n_slots, int Hp, int Wp, const float* mean3,
                                        const float* std3, int* launches, void* stream) {
  if (launches) *launches = 0;
  LVC_CHECK_ARG(B >= 0 && n_slots >= B && Hp > 0 && Wp > 0, "bad batch size");
  if (B == 0) return LVC_OK;
  LVC_CHECK_ARG(out && tmp && mean3 && std3, "null argument");
  LVC_CHECK_MSG(check_blob(h_blob, d_blob, blob_bytes, B, TT_FIELDS));
  const long long* jobs = reinterpret_cast<const long long*>(h_blob);
  const char* hb = reinterpret_cast<const char*>(h_blob);
  int gw = 0, gh = 0;
  unsigned long long slots_seen = 0;
  for (int i = 0; i < B; ++i) {
    const long long* j = jobs + (size_t)i * TT_FIELDS;
    const long long cw = j[TJ_CW], ch = j[TJ_CH], nh = j[TJ_NEW_H], nw = j[TJ_NEW_W];
    LVC_CHECK_MSG(check_window_tiles(j, j[TJ_NT], j + TL_HEAD));
    LVC_CHECK_ARG(nh > 0 && nw > 0 && nh <= Hp && nw <= Wp, "output size outside the padded batch");
    LVC_CHECK_MSG(check_slot(j[TJ_SLOT], n_slots, slots_seen));
    LVC_CHECK_ARG((j[TJ_XB] >= 0) == (nw != cw) && (j[TJ_YB] >= 0) == (nh != ch), "coefficients must match the size change");
    if (j[TJ_XB] >= 0) LVC_CHECK_ARG(check_axis(hb, blob_bytes, j[TJ_XB], j[TJ_XK], j[TJ_KXS], cw, nw), "bad column tables");
    if (j[TJ_YB] >= 0) LVC_CHECK_ARG(check_axis(hb, blob_bytes, j[TJ_YB], j[TJ_YK], j[TJ_KYS], ch, nh), "bad row tables");
    LVC_CHECK_ARG(j[TJ_TMP] >= 0 && j[TJ_TMP] <= tmp_bytes && ch * nw * 3 <= tmp_bytes - j[TJ_TMP], "intermediate outside the scratch buffer");
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
//      (those rows themselves where the height stays) -- through the tile list (tiles_h_pass) -> tmp [bh][ow][3];
//   2. vertical pass, grid (x tiles, Hp, B): thread (yo, xo) owns OUTPUT pixel (yo, xo) of its slot; its canvas column before the
//      flip is xc = flip ? tw-1-xo : xo; inside oh x ow it resamples column xc of tmp with the taps of scaled row oy + yo, elsewhere
//      inside the canvas it is the fill; both are normalised as above; outside the canvas it is the batch's zero padding.
__global__ __launch_bounds__(256) void train_input_lsj_h_kernel(const char* __restrict__ blob, unsigned char* __restrict__ tmp) {
  const long long* jb = reinterpret_cast<const long long*>(blob) + (size_t)blockIdx.z * LJ_FIELDS;
  tiles_h_pass(blob, jb, jb + TL_HEAD_LSJ, tmp, jb[TJ_BY0], (int)jb[TJ_BH], (int)jb[TJ_OX], (int)jb[TJ_OW]);
}

// tmp [bh][ow][3] -> the job's slot (and its optional uint8 canvas [th][tw][3])
__global__ __launch_bounds__(256) void train_input_lsj_v_kernel(const char* __restrict__ blob, const unsigned char* __restrict__ tmp,
                                                                float* __restrict__ out, int Hp, int Wp, float m0, float m1, float m2,
                                                                float d0, float d1, float d2) {
  const long long* jb = reinterpret_cast<const long long*>(blob) + (size_t)blockIdx.z * LJ_FIELDS;
  const int xo = blockIdx.x * 256 + threadIdx.x, yo = blockIdx.y;
  if (xo >= Wp) return;
  const int th = (int)jb[TJ_TH], tw = (int)jb[TJ_TW];
  float4 v = {0.f, 0.f, 0.f, 0.f};
  if (yo < th && xo < tw) {
    const int xc = jb[TJ_FLIP] ? tw - 1 - xo : xo;   // HFlipTransform(tw) on the padded canvas: the fill moves to the left
    const int ow = (int)jb[TJ_OW];
    unsigned char r0, r1, r2;
    r0 = r1 = r2 = (unsigned char)jb[TJ_FILL];
    if (yo < (int)jb[TJ_OH] && xc < ow)      // row oy + yo of the scaled image; tmp begins at the band's first source row
      ti_v_pixel(tmp + jb[TJ_TMP] + (size_t)xc * 3, (long long)ow * 3, 1, blob, jb + TJ_YB, (int)jb[TJ_OY] + yo, (int)jb[TJ_BY0], r0, r1, r2);
    if (jb[TJ_U8]) {
      unsigned char* o = reinterpret_cast<unsigned char*>(jb[TJ_U8]) + ((size_t)yo * tw + xo) * 3;
      o[0] = r0; o[1] = r1; o[2] = r2;
    }
    v = normalise4(r0, r1, r2, m0, m1, m2, d0, d1, d2);
  }
  *reinterpret_cast<float4*>(out + (((size_t)jb[TJ_SLOT] * Hp + yo) * Wp + xo) * 4) = v;
}

// Job words and arguments: include/lvc_amd.h.  Checked on the host copy before anything is launched: what lvc_train_input_tiles_u8
// checks of a window and its tiles, the output window inside the scaled image and not larger than the canvas, the canvas inside the
// padded batch, the band inside the crop window, every tap of the window's columns inside the crop window and of its rows inside the
// band, the intermediate inside tmp and apart from every other job's, no slot written twice.  launches: optional, the number of
// kernel launches issued (two).
extern "C" int lvc_train_input_lsj_u8(const void* h_blob, const void* d_blob, long long blob_bytes, int B, unsigned char* tmp,
                                      long long tmp_bytes, float* out, int n_slots, int Hp, int Wp, const float* mean3,
                                      const float* std3, int* launches, void* stream) {
  if (launches) *launches = 0;
  LVC_CHECK_ARG(B >= 0 && n_slots >= B && Hp > 0 && Wp > 0, "bad batch size");
  if (B == 0) return LVC_OK;
  LVC_CHECK_ARG(out && tmp && mean3 && std3, "null argument");
  LVC_CHECK_MSG(check_blob(h_blob, d_blob, blob_bytes, B, LJ_FIELDS));
  const long long* jobs = reinterpret_cast<const long long*>(h_blob);
  const char* hb = reinterpret_cast<const char*>(h_blob);
  int gw = 0, gh = 0;
  unsigned long long slots_seen = 0;
  for (int i = 0; i < B; ++i) {
    const long long* j = jobs + (size_t)i * LJ_FIELDS;
    const long long cw = j[TJ_CW], ch = j[TJ_CH], sh = j[TJ_NEW_H], sw = j[TJ_NEW_W];
    const long long ox = j[TJ_OX], oy = j[TJ_OY], ow = j[TJ_OW], oh = j[TJ_OH], th = j[TJ_TH], tw = j[TJ_TW];
    const long long by0 = j[TJ_BY0], bh = j[TJ_BH];
    LVC_CHECK_MSG(check_window_tiles(j, j[TJ_NT], j + TL_HEAD_LSJ));
    LVC_CHECK_ARG(sh > 0 && sw > 0 && sh < TL_COORD_MAX && sw < TL_COORD_MAX, "bad scaled size");
    LVC_CHECK_ARG(ox >= 0 && oy >= 0 && ow > 0 && oh > 0 && ox <= sw - ow && oy <= sh - oh, "output window outside the scaled image");
    LVC_CHECK_ARG(th > 0 && tw > 0 && ow <= tw && oh <= th && th <= Hp && tw <= Wp, "canvas outside the padded batch or smaller than its window");
    LVC_CHECK_ARG(j[TJ_FILL] >= 0 && j[TJ_FILL] <= 255, "the fill is a byte");
    LVC_CHECK_MSG(check_slot(j[TJ_SLOT], n_slots, slots_seen));
    LVC_CHECK_ARG((j[TJ_XB] >= 0) == (sw != cw) && (j[TJ_YB] >= 0) == (sh != ch), "coefficients must match the size change");
    LVC_CHECK_ARG(by0 >= 0 && bh > 0 && by0 <= ch - bh, "band outside the crop window");
    if (j[TJ_XB] >= 0) LVC_CHECK_ARG(check_axis(hb, blob_bytes, j[TJ_XB], j[TJ_XK], j[TJ_KXS], cw, sw), "bad column tables");
    if (j[TJ_YB] >= 0) {
      LVC_CHECK_ARG(check_axis(hb, blob_bytes, j[TJ_YB], j[TJ_YK], j[TJ_KYS], ch, sh), "bad row tables");
      const int* b = reinterpret_cast<const int*>(hb + j[TJ_YB]);
      for (long long r = oy; r < oy + oh; ++r)
        LVC_CHECK_ARG(b[2 * r] >= by0 && (long long)b[2 * r] + b[2 * r + 1] <= by0 + bh, "row taps outside the band");
    } else {
      LVC_CHECK_ARG(by0 <= oy && oy + oh <= by0 + bh, "output rows outside the band");
    }
    LVC_CHECK_ARG(j[TJ_TMP] >= 0 && j[TJ_TMP] <= tmp_bytes && bh * ow * 3 <= tmp_bytes - j[TJ_TMP], "intermediate outside the scratch buffer");
    for (int k = 0; k < i; ++k) {      // both passes of all jobs run side by side: no two intermediates may share a byte
      const long long* o = jobs + (size_t)k * LJ_FIELDS;
      LVC_CHECK_ARG(j[TJ_TMP] + bh * ow * 3 <= o[TJ_TMP] || o[TJ_TMP] + o[TJ_BH] * o[TJ_OW] * 3 <= j[TJ_TMP],
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
