// input_common.h -- what the device-side input pipeline shares (resize.hip, tta.hip, train_input.hip, color_jitter.hip): Pillow's 8-bit
// resample, the tile list of a mosaic canvas with its row walk, and the host checks of a job blob.  The job layouts are described
// once, in include/lvc_amd.h.
#pragma once
#include "common.h"

// ------------------------------------------------------------------------------------------------ Pillow's 8-bit resample
// src/libImaging/Resample.c ImagingResampleHorizontal_8bpc / Vertical_8bpc: 22-bit fixed-point coefficients, each output =
// clip8((2^21 + sum k * pixel) >> 22) in int32.  Strides given as literals at the call site stay constants: everything is inlined.
#define RS_PREC 22

__device__ __forceinline__ unsigned char clip8(int v) {
  v >>= RS_PREC;
  return (unsigned char)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// cnt taps of weights k on the three channels of the pixels p + first * step, p + (first + 1) * step, ...; a pixel's channels lie
// sc apart
template <typename T, typename C>
__device__ __forceinline__ void resample_taps(const unsigned char* p, int first, T step, C sc, const int* k, int cnt, unsigned char& r0,
                                              unsigned char& r1, unsigned char& r2) {
  int s0 = 1 << (RS_PREC - 1), s1 = s0, s2 = s0;
  for (int t = 0; t < cnt; ++t) {
    const unsigned char* q = p + (first + t) * step;
    const int c = k[t];
    s0 += q[0] * c; s1 += q[sc] * c; s2 += q[2 * sc] * c;
  }
  r0 = clip8(s0); r1 = clip8(s1); r2 = clip8(s2);
}

// one pixel of the vertical pass: row ys of the tables yb [.][2] / yk [.][kys] applied down the column `col` (rows sy apart) of an
// intermediate whose first row is source row y_first; yk == nullptr: height unchanged, Pillow skips the pass and row ys is copied
template <typename T, typename C>
__device__ __forceinline__ void resample_v_pixel(const unsigned char* col, T sy, C sc, const int* yb, const int* yk, int kys, int ys,
                                                 int y_first, unsigned char& r0, unsigned char& r1, unsigned char& r2) {
  if (yk) {
    const int ymin = yb[2 * ys] - y_first, cnt = yb[2 * ys + 1];
    resample_taps(col, ymin, sy, sc, yk + (size_t)ys * kys, cnt, r0, r1, r2);
  } else {
    const unsigned char* p = col + (ys - y_first) * sy;
    r0 = p[0]; r1 = p[sc]; r2 = p[2 * sc];
  }
}

// GeneralizedRCNN.preprocess_image on one pixel, 4th channel zero
__device__ __forceinline__ float4 normalise4(unsigned char r0, unsigned char r1, unsigned char r2, float m0, float m1, float m2,
                                             float d0, float d1, float d2) {
  return make_float4(((float)r0 - m0) / d0, ((float)r1 - m1) / d1, ((float)r2 - m2) / d2, 0.f);
}

// ------------------------------------------------------------------------------------------------ tiled sources (mosaic canvas)
// A job's source is a CANVAS painted from 1..9 tiles: tile t covers the canvas rectangle [x1a, x2a) x [y1a, y2a) with its pixels
// from (x1b, y1b) on; tiles are painted in order (where rectangles overlap the later one wins) and what no tile covers is TL_FILL.
#define TL_WORDS 12       // int64 words per tile
#define TL_MAX_TILES 9
#define TL_FILL 114
#define TL_COORD_MAX (1ll << 30)
#define TL_HEAD 20        // int64 words in front of the tiles of a tiles job and of a colour-jitter job
#define TL_HEAD_LSJ 32    // ... of an LSJ job

enum { TL_SRC = 0, TL_H, TL_W, TL_SY, TL_SX, TL_SC, TL_X1A, TL_Y1A, TL_X2A, TL_Y2A, TL_X1B, TL_Y1B };
// the head of a tiles job and, from TJ_OX on, of an LSJ job (whose TJ_NEW_H / TJ_NEW_W are the size of the WHOLE scaled image)
enum {
  TJ_X0 = 0, TJ_Y0, TJ_CW, TJ_CH, TJ_NEW_H, TJ_NEW_W, TJ_XB, TJ_XK, TJ_KXS, TJ_YB, TJ_YK, TJ_KYS, TJ_FLIP, TJ_SLOT, TJ_U8, TJ_TMP,
  TJ_NT, TJ_OX, TJ_OY, TJ_OW, TJ_OH, TJ_TH, TJ_TW, TJ_FILL, TJ_BY0, TJ_BH
};

// the tiles that cross one canvas row, clipped to the crop window, in paint order
struct TileSegs {
  int lo[TL_MAX_TILES], hi[TL_MAX_TILES], n;      // window columns [lo, hi)
  long long sx[TL_MAX_TILES], sc[TL_MAX_TILES];
  const unsigned char* row[TL_MAX_TILES];         // the tile's pixel under window column 0 of this row
};

// A workgroup is one canvas row Y of one job, so the crossing tiles are the same for all its threads: the first wavefront finds them
// once (lane t tests tile t) and compacts them into LDS.  The whole workgroup must call this.
__device__ __forceinline__ void tile_segs_load(const long long* jb, const long long* tiles, long long Y, TileSegs& sg) {
  if (threadIdx.x < 64) {
    const long long X0 = jb[TJ_X0], cw = jb[TJ_CW];
    const long long* tl = tiles + (size_t)(threadIdx.x < TL_MAX_TILES ? threadIdx.x : 0) * TL_WORDS;
    long long lo = 0, hi = 0;
    bool cross = false;
    if ((long long)threadIdx.x < jb[TJ_NT] && Y >= tl[TL_Y1A] && Y < tl[TL_Y2A]) {
      lo = tl[TL_X1A] > X0 ? tl[TL_X1A] - X0 : 0;
      hi = tl[TL_X2A] < X0 + cw ? tl[TL_X2A] - X0 : cw;
      cross = lo < hi;
    }
    const unsigned long long m = __ballot(cross);
    if (cross) {
      const int p = __popcll(m & ((1ull << threadIdx.x) - 1ull));
      sg.lo[p] = (int)lo; sg.hi[p] = (int)hi; sg.sx[p] = tl[TL_SX]; sg.sc[p] = tl[TL_SC];
      sg.row[p] = reinterpret_cast<const unsigned char*>(tl[TL_SRC]) + (Y - tl[TL_Y1A] + tl[TL_Y1B]) * tl[TL_SY] +
                  (X0 - tl[TL_X1A] + tl[TL_X1B]) * tl[TL_SX];
    }
    if (threadIdx.x == 0) sg.n = __popcll(m);
  }
  __syncthreads();
}

// The horizontal pass of a tiled job (head at jb, tiles at `tiles`), grid (x tiles, rows, jobs): row row0 + blockIdx.y of the crop
// window, columns [col0, col0 + out_w) of the resized width -> tmp [rows][out_w][3] at the job's TJ_TMP.  A thread walks its taps
// through contiguous x and keeps the run [.., run_hi) in which the owner of a pixel does not change, so the tile list is searched
// again only where a tap leaves that run.  A width that does not change is a copy (one tap of weight 1 << 22: what Pillow's
// skipping the pass gives, byte for byte).
__device__ __forceinline__ void tiles_h_pass(const char* blob, const long long* jb, const long long* tiles, unsigned char* tmp,
                                             long long row0, int rows, int col0, int out_w) {
  const int y = blockIdx.y, cw = (int)jb[TJ_CW];
  if (y >= rows || (int)(blockIdx.x * 256) >= out_w) return;   // the whole workgroup leaves: nobody waits below
  __shared__ TileSegs sg;
  tile_segs_load(jb, tiles, jb[TJ_Y0] + row0 + y, sg);
  const int xo = blockIdx.x * 256 + threadIdx.x;
  if (xo >= out_w) return;
  const int xs = col0 + xo;      // the column of the resized image
  int xmin = xs, cnt = 1;
  const int* k = nullptr;      // width unchanged: one tap of weight 1
  if (jb[TJ_XB] >= 0) {
    const int* xb = reinterpret_cast<const int*>(blob + jb[TJ_XB]);
    k = reinterpret_cast<const int*>(blob + jb[TJ_XK]) + (size_t)xs * (int)jb[TJ_KXS];
    xmin = xb[2 * xs]; cnt = xb[2 * xs + 1];
  }
  const int ns = sg.n;
  int run_hi = -1;                       // taps below run_hi have the owner found last
  const unsigned char* row = nullptr;    // its row (nullptr: no tile, the fill colour)
  long long sx = 0, sc = 0;
  int s0 = 1 << (RS_PREC - 1), s1 = s0, s2 = s0;
  for (int t = 0; t < cnt; ++t) {
    const int x = xmin + t;
    if (x >= run_hi) {      // the last tile that covers x owns it; the run ends where that tile ends or a later one begins
      row = nullptr; run_hi = cw;
      for (int i = 0; i < ns; ++i) {
        const int lo = sg.lo[i], hi = sg.hi[i];
        if (lo <= x && x < hi) { row = sg.row[i]; sx = sg.sx[i]; sc = sg.sc[i]; run_hi = hi; }
        else if (lo > x && lo < run_hi) run_hi = lo;
      }
    }
    int p0 = TL_FILL, p1 = TL_FILL, p2 = TL_FILL;
    if (row) {
      const unsigned char* p = row + x * sx;
      p0 = p[0]; p1 = p[sc]; p2 = p[2 * sc];
    }
    const int c = k ? k[t] : 1 << RS_PREC;
    s0 += p0 * c; s1 += p1 * c; s2 += p2 * c;
  }
  unsigned char* o = tmp + jb[TJ_TMP] + ((size_t)y * out_w + xo) * 3;
  o[0] = clip8(s0); o[1] = clip8(s1); o[2] = clip8(s2);
}

// ------------------------------------------------------------------------------------------------ host checks of a job blob
// Each returns the message of the first check that fails, or nullptr; the entry point raises it under its own name.
#define LVC_CHECK_MSG(expr)       \
  do {                            \
    const char* m_ = (expr);      \
    LVC_CHECK_ARG(!m_, m_);       \
  } while (0)

// the host and device copies of a blob of B jobs of `fields` int64 words
static const char* check_blob(const void* h_blob, const void* d_blob, long long blob_bytes, long long B, long long fields) {
  if (!h_blob || !d_blob) return "null argument";
  if (((uintptr_t)h_blob & 7) || ((uintptr_t)d_blob & 7)) return "the blob must be 8-byte aligned";
  if (blob_bytes < B * fields * 8) return "blob smaller than its job table";
  return nullptr;
}

// a job's slot lies in the batch and no earlier job writes it (seen: the slots below 64 met so far)
static const char* check_slot(long long slot, long long n_slots, unsigned long long& seen) {
  if (slot < 0 || slot >= n_slots) return "bad slot";
  if (slot < 64) {
    if (seen >> slot & 1ull) return "two jobs write one slot";
    seen |= 1ull << slot;
  }
  return nullptr;
}

// one resample axis of one job: the tables lie inside the blob and every tap inside [0, in_size)
static bool check_axis(const char* h_blob, long long blob_bytes, long long b_off, long long k_off, long long ks, long long in_size,
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

// the crop window at words 0-3 of a job (X0, Y0, cw, ch in canvas coordinates) and its nt tiles: every pixel of a rectangle that
// the window sees lies inside its tile
static const char* check_window_tiles(const long long* j, long long nt, const long long* tiles) {
  const long long X0 = j[TJ_X0], Y0 = j[TJ_Y0], cw = j[TJ_CW], ch = j[TJ_CH];
  if (nt < 1 || nt > TL_MAX_TILES) return "a job has 1 to 9 tiles";
  if (X0 < 0 || Y0 < 0 || cw <= 0 || ch <= 0 || X0 >= TL_COORD_MAX || Y0 >= TL_COORD_MAX || cw >= TL_COORD_MAX || ch >= TL_COORD_MAX)
    return "bad crop window";
  for (const long long* tl = tiles; tl < tiles + nt * TL_WORDS; tl += TL_WORDS) {
    if (!tl[TL_SRC] || tl[TL_H] <= 0 || tl[TL_W] <= 0 || tl[TL_H] >= TL_COORD_MAX || tl[TL_W] >= TL_COORD_MAX) return "bad tile image";
    if (tl[TL_SY] <= 0 || tl[TL_SX] <= 0 || tl[TL_SC] <= 0) return "strides must be positive";
    for (int f = TL_X1A; f <= TL_Y1B; ++f)
      if (tl[f] <= -TL_COORD_MAX || tl[f] >= TL_COORD_MAX) return "tile coordinate out of range";
    if (tl[TL_X2A] < tl[TL_X1A] || tl[TL_Y2A] < tl[TL_Y1A]) return "canvas rectangle with negative extent";
    const long long lx = tl[TL_X1A] > X0 ? tl[TL_X1A] : X0, hx = tl[TL_X2A] < X0 + cw ? tl[TL_X2A] : X0 + cw;
    const long long ly = tl[TL_Y1A] > Y0 ? tl[TL_Y1A] : Y0, hy = tl[TL_Y2A] < Y0 + ch ? tl[TL_Y2A] : Y0 + ch;
    if (lx < hx && ly < hy &&      // the part of the tile's rectangle the window sees: read from inside the tile
        (lx - tl[TL_X1A] + tl[TL_X1B] < 0 || hx - tl[TL_X1A] + tl[TL_X1B] > tl[TL_W] || ly - tl[TL_Y1A] + tl[TL_Y1B] < 0 ||
         hy - tl[TL_Y1A] + tl[TL_Y1B] > tl[TL_H]))
      return "a tile is read outside its image";
  }
  return nullptr;
}
