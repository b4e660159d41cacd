// tta.hip -- test-time augmentation on the device (reference detectron2/modeling/test_time_augmentation.py:27-291).
//
// 1. lvc_tta_resize_u8: DatasetMapperTTA (:42-81) + GeneralizedRCNN.preprocess_image for every augmentation of one uint8 image in
//    two launches: a horizontal pass over a table of the distinct output widths, then a vertical pass over a table of the output
//    sizes.  The vertical pass writes each resized pixel into up to two NHWC4 fp32 batch slots -- the plain one and the horizontally
//    mirrored one (RandomFlip(prob=1) -> HFlipTransform(new_w) after the resize: column x -> new_w - 1 - x) -- as (v - mean) / std,
//    zero-padded to each slot's own padded size with the 4th channel zero, and optionally the uint8 [new_h,new_w,3] images.
//    The resample is resize.hip's (input_common.h), bit for bit: Pillow's 22-bit coefficients (lvc_amd/data/transforms.py
//    resample_coeffs), a uint8 intermediate, an unchanged axis skipped.  The source is read through strides (CHW `image` or HWC
//    `raw` without a copy).
// 2. lvc_tta_merge: _get_augmented_boxes (:228-244) + _merge_detections (:246-264) -> fast_rcnn_inference_single_image
//    (detectron2/modeling/roi_heads/fast_rcnn.py:111-158) for B images at once from the device-resident per-augmentation outputs.
//    One workgroup per image walks its augmentations in order and gathers the union in the reference's order (augmentation, then
//    detection), applying the inverse transforms as fvcore's TransformList.apply_box does in fp32 numpy -- one rounding per step
//    (un-flip x -> W - x, then x * fp32(sx) per resize), min/max of the corners -- then the finite filter, Boxes.clip and
//    `score > 1e-8` (the one-hot score matrix has one entry per row, so its row-major nonzero order is the union order).  Then
//    lvc_batched_nms (per class, bit-exact keep order) with max_keep = DETECTIONS_PER_IMAGE, and a gather into [B, topk] outputs.
//
// Byte streams and latency-bound bookkeeping: built with the EXACT flags (-ffp-contract=off -fno-fast-math): the fp32 steps of the
// inverse transforms and the normaliser must round exactly as numpy / preprocess_image do.
#include "input_common.h"   // lvc_batched_nms (nms.hip) comes with the public header

#define TTA_MAX_JOBS 16
#define TTA_MAX_STEPS 4
#define TTA_PARAM_STRIDE 16

struct TtaHJob {
  const int* xb;
  const int* xk;
  unsigned char* tmp;   // [H][new_w][3]
  int kxs, new_w;
};

struct TtaHTable {
  TtaHJob j[TTA_MAX_JOBS];
};

struct TtaVJob {
  const unsigned char* src;   // the horizontal pass's output of this width, or the image itself (width unchanged)
  long long sy, sx, sc;       // element strides of src
  const int* yb;
  const int* yk;              // NULL: height unchanged
  unsigned char* u8;          // optional [new_h][new_w][3]
  unsigned char* u8m;         // optional, mirrored
  float* f;                   // optional plain slot [Hp][Wp][4]
  float* fm;                  // optional mirrored slot [Hpm][Wpm][4]
  int kys, new_h, new_w, Hp, Wp, Hpm, Wpm, rows, cols;   // rows / cols: the extent this job covers
};

struct TtaVTable {
  TtaVJob j[TTA_MAX_JOBS];
};

// one launch for every distinct output width: grid (x tiles, H rows, jobs)
__global__ __launch_bounds__(256) void tta_resize_h_kernel(const unsigned char* __restrict__ src, int H, long long sy, long long sx,
                                                           long long sc, TtaHTable tab) {
  const TtaHJob& jb = tab.j[blockIdx.z];
  const int xo = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
  if (xo >= jb.new_w) return;
  unsigned char* o = jb.tmp + ((size_t)y * jb.new_w + xo) * 3;
  resample_taps(src + (size_t)y * sy + (size_t)jb.xb[2 * xo] * sx, 0, sx, sc, jb.xk + (size_t)xo * jb.kxs, jb.xb[2 * xo + 1], o[0], o[1], o[2]);
}

// one launch for every output size: grid (x tiles, rows, jobs).  Thread (yo, xo) resamples pixel (yo, xo) of its job (when inside
// new_h x new_w), stores it at (yo, xo) of the plain slot and at (yo, new_w-1-xo) of the mirrored one, and writes the zero padding of
// both slots at (yo, xo) where that lies outside the image.
__global__ __launch_bounds__(256) void tta_resize_v_kernel(TtaVTable tab, float m0, float m1, float m2, float d0, float d1, float d2) {
  const TtaVJob& jb = tab.j[blockIdx.z];
  const int xo = blockIdx.x * 256 + threadIdx.x, yo = blockIdx.y;
  if (xo >= jb.cols || yo >= jb.rows) return;
  const bool inside = yo < jb.new_h && xo < jb.new_w;
  float4 v = {0.f, 0.f, 0.f, 0.f};
  if (inside) {
    unsigned char r0, r1, r2;
    resample_v_pixel(jb.src + (size_t)xo * jb.sx, jb.sy, jb.sc, jb.yb, jb.yk, jb.kys, yo, 0, r0, r1, r2);
    const int xm = jb.new_w - 1 - xo;
    if (jb.u8) {
      unsigned char* o = jb.u8 + ((size_t)yo * jb.new_w + xo) * 3;
      o[0] = r0; o[1] = r1; o[2] = r2;
    }
    if (jb.u8m) {
      unsigned char* o = jb.u8m + ((size_t)yo * jb.new_w + xm) * 3;
      o[0] = r0; o[1] = r1; o[2] = r2;
    }
    v = normalise4(r0, r1, r2, m0, m1, m2, d0, d1, d2);
    if (jb.fm) *reinterpret_cast<float4*>(jb.fm + ((size_t)yo * jb.Wpm + xm) * 4) = v;
  } else if (jb.fm && yo < jb.Hpm && xo < jb.Wpm) {
    *reinterpret_cast<float4*>(jb.fm + ((size_t)yo * jb.Wpm + xo) * 4) = v;
  }
  if (jb.f && yo < jb.Hp && xo < jb.Wp) *reinterpret_cast<float4*>(jb.f + ((size_t)yo * jb.Wp + xo) * 4) = v;
}

// image: uint8, element (y, x, c) at image[y*sy + x*sx + c*sc] (device).  hjobs: host int64 [n_h][5] = (xb, xk, kxs, new_w, tmp):
// the horizontal pass for each distinct output width != W (tmp: H*new_w*3 bytes).  vjobs: host int64 [n_v][14] = (src_hjob (-1: the
// image itself, width unchanged), yb, yk (0: height unchanged), kys, new_h, new_w, u8, u8m, f, Hp, Wp, fm, Hpm, Wpm).  mean3 / std3:
// host float[3].  Up to TTA_MAX_JOBS jobs per launch: at most two launches for <= 16 output sizes.
extern "C" int lvc_tta_resize_u8(const unsigned char* image, int H, int W, long long sy, long long sx, long long sc,
                                 const long long* hjobs, int n_h, const long long* vjobs, int n_v, const float* mean3,
                                 const float* std3, void* stream) {
  LVC_CHECK_ARG(image && H > 0 && W > 0 && n_h >= 0 && n_v > 0, "bad image / job count");
  LVC_CHECK_ARG(n_h == 0 || hjobs, "missing horizontal jobs");
  LVC_CHECK_ARG(vjobs && mean3 && std3, "null argument");
  hipStream_t st = (hipStream_t)stream;
  for (int j0 = 0; j0 < n_h; j0 += TTA_MAX_JOBS) {
    TtaHTable tab = {};
    const int n = n_h - j0 < TTA_MAX_JOBS ? n_h - j0 : TTA_MAX_JOBS;
    int gw = 0;
    for (int i = 0; i < n; ++i) {
      const long long* r = hjobs + (size_t)(j0 + i) * 5;
      TtaHJob& jb = tab.j[i];
      jb.xb = (const int*)r[0]; jb.xk = (const int*)r[1]; jb.kxs = (int)r[2]; jb.new_w = (int)r[3]; jb.tmp = (unsigned char*)r[4];
      LVC_CHECK_ARG(jb.xb && jb.xk && jb.tmp && jb.kxs > 0 && jb.new_w > 0 && jb.new_w != W, "bad horizontal job");
      gw = jb.new_w > gw ? jb.new_w : gw;
    }
    hipLaunchKernelGGL(tta_resize_h_kernel, dim3(lvc_cdiv(gw, 256), H, n), dim3(256), 0, st, image, H, sy, sx, sc, tab);
    LVC_CHECK_LAUNCH();
  }
  for (int j0 = 0; j0 < n_v; j0 += TTA_MAX_JOBS) {
    TtaVTable tab = {};
    const int n = n_v - j0 < TTA_MAX_JOBS ? n_v - j0 : TTA_MAX_JOBS;
    int gw = 0, gh = 0;
    for (int i = 0; i < n; ++i) {
      const long long* r = vjobs + (size_t)(j0 + i) * 14;
      TtaVJob& jb = tab.j[i];
      const int hj = (int)r[0];
      LVC_CHECK_ARG(hj >= -1 && hj < n_h, "bad source job");
      jb.yb = (const int*)r[1]; jb.yk = (const int*)r[2]; jb.kys = (int)r[3];
      jb.new_h = (int)r[4]; jb.new_w = (int)r[5];
      jb.u8 = (unsigned char*)r[6]; jb.u8m = (unsigned char*)r[7];
      jb.f = (float*)r[8]; jb.Hp = (int)r[9]; jb.Wp = (int)r[10];
      jb.fm = (float*)r[11]; jb.Hpm = (int)r[12]; jb.Wpm = (int)r[13];
      LVC_CHECK_ARG(jb.new_h > 0 && jb.new_w > 0, "bad output size");
      LVC_CHECK_ARG((jb.yk != nullptr) == (jb.new_h != H) && (!jb.yk || (jb.yb && jb.kys > 0)), "row coefficients must match the size change");
      if (hj < 0) {
        LVC_CHECK_ARG(jb.new_w == W, "width changes but no horizontal job is given");
        jb.src = image; jb.sy = sy; jb.sx = sx; jb.sc = sc;
      } else {
        const long long* hr = hjobs + (size_t)hj * 5;
        LVC_CHECK_ARG((int)hr[3] == jb.new_w, "horizontal job of another width");
        jb.src = (const unsigned char*)hr[4]; jb.sy = (long long)jb.new_w * 3; jb.sx = 3; jb.sc = 1;
      }
      LVC_CHECK_ARG(jb.u8 || jb.u8m || jb.f || jb.fm, "no output requested");
      LVC_CHECK_ARG(!jb.f || (jb.Hp >= jb.new_h && jb.Wp >= jb.new_w), "plain slot smaller than the image");
      LVC_CHECK_ARG(!jb.fm || (jb.Hpm >= jb.new_h && jb.Wpm >= jb.new_w), "mirrored slot smaller than the image");
      jb.rows = jb.new_h; jb.cols = jb.new_w;
      if (jb.f) { jb.rows = jb.Hp > jb.rows ? jb.Hp : jb.rows; jb.cols = jb.Wp > jb.cols ? jb.Wp : jb.cols; }
      if (jb.fm) { jb.rows = jb.Hpm > jb.rows ? jb.Hpm : jb.rows; jb.cols = jb.Wpm > jb.cols ? jb.Wpm : jb.cols; }
      gw = jb.cols > gw ? jb.cols : gw;
      gh = jb.rows > gh ? jb.rows : gh;
    }
    hipLaunchKernelGGL(tta_resize_v_kernel, dim3(lvc_cdiv(gw, 256), gh, n), dim3(256), 0, st, tab, mean3[0], mean3[1], mean3[2],
                       std3[0], std3[1], std3[2]);
    LVC_CHECK_LAUNCH();
  }
  return LVC_OK;
}

// ---------------------------------------------------------------------------------------------------------------- merge
// Inverse transform of one augmentation: params[0] = number of steps (<= TTA_MAX_STEPS), then (kind, a, b) per step -- kind 1:
// hflip, x -> a - x (HFlipTransform(width = a)); kind 2: resize, x -> x * a, y -> y * b (a, b = fp32(new_w / w), fp32(new_h / h) of
// the inverse).  Every step maps the corners and takes their min / max, as fvcore's Transform.apply_box does.  Returns false when a
// coordinate is not finite after some step: numpy's min / max propagate a NaN, which the ternaries here would hide, so the finite
// filter is decided per coordinate before them.
__device__ __forceinline__ bool tta_inverse_box(const float* __restrict__ p, float& x0, float& y0, float& x1, float& y1) {
  int n = (int)p[0];
  n = n < TTA_MAX_STEPS ? n : TTA_MAX_STEPS;
  bool fin = isfinite(x0) && isfinite(y0) && isfinite(x1) && isfinite(y1);
  for (int s = 0; s < n; ++s) {
    const int kind = (int)p[1 + 3 * s];
    const float a = p[2 + 3 * s], b = p[3 + 3 * s];
    float u0, u1, v0 = y0, v1 = y1;
    if (kind == 1) {
      u0 = a - x0; u1 = a - x1;
    } else {
      u0 = x0 * a; u1 = x1 * a; v0 = y0 * b; v1 = y1 * b;
    }
    fin = fin && isfinite(u0) && isfinite(u1) && isfinite(v0) && isfinite(v1);
    x0 = u0 < u1 ? u0 : u1; x1 = u0 < u1 ? u1 : u0;
    y0 = v0 < v1 ? v0 : v1; y1 = v0 < v1 ? v1 : v0;
  }
  return fin;
}

// one workgroup per image: the union of its augmentations' detections, inverse-transformed, filtered, clipped, in union order.
// tab [B][4] = (first augmentation, end, clip height, clip width).
__global__ __launch_bounds__(256) void tta_union_kernel(const float* __restrict__ boxes, const float* __restrict__ scores,
                                                        const int* __restrict__ classes, const int* __restrict__ counts, int topk_in,
                                                        const float* __restrict__ params, const int* __restrict__ tab, int Nmax,
                                                        float score_thresh, float* __restrict__ cboxes, float* __restrict__ cscores,
                                                        int* __restrict__ cclasses, int* __restrict__ ccount) {
  __shared__ int wsum[4];
  const int img = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int a0 = tab[4 * img], a1 = tab[4 * img + 1];
  const float ch = (float)tab[4 * img + 2], cw = (float)tab[4 * img + 3];
  float* cb = cboxes + (size_t)img * Nmax * 4;
  float* cs = cscores + (size_t)img * Nmax;
  int* cc = cclasses + (size_t)img * Nmax;
  int base = 0;
  for (int a = a0; a < a1; ++a) {
    int n = counts[a];
    n = n < 0 ? 0 : (n > topk_in ? topk_in : n);
    const float* p = params + (size_t)a * TTA_PARAM_STRIDE;
    for (int r0 = 0; r0 < n; r0 += 256) {
      const int r = r0 + tid;
      bool keep = false;
      float x0 = 0.f, y0 = 0.f, x1 = 0.f, y1 = 0.f, s = 0.f;
      int c = 0;
      if (r < n) {
        const float* b = boxes + ((size_t)a * topk_in + r) * 4;
        x0 = b[0]; y0 = b[1]; x1 = b[2]; y1 = b[3];
        s = scores[(size_t)a * topk_in + r];
        c = classes[(size_t)a * topk_in + r];
        keep = tta_inverse_box(p, x0, y0, x1, y1) && isfinite(s) && s > score_thresh;
        // Boxes.clip: clamp(min=0, max=w / h)
        x0 = fminf(fmaxf(x0, 0.f), cw); x1 = fminf(fmaxf(x1, 0.f), cw);
        y0 = fminf(fmaxf(y0, 0.f), ch); y1 = fminf(fmaxf(y1, 0.f), ch);
      }
      const unsigned long long m = __ballot(keep);
      const int below = __popcll(m & ((1ull << lane) - 1ull));
      if (lane == 0) wsum[wave] = __popcll(m);
      __syncthreads();
      int off = base, tot = 0;
      for (int w = 0; w < 4; ++w) {
        if (w < wave) off += wsum[w];
        tot += wsum[w];
      }
      if (keep) {
        const int pos = off + below;
        if (pos < Nmax) {
          cb[(size_t)pos * 4 + 0] = x0; cb[(size_t)pos * 4 + 1] = y0; cb[(size_t)pos * 4 + 2] = x1; cb[(size_t)pos * 4 + 3] = y1;
          cs[pos] = s;
          cc[pos] = c;
        }
      }
      base += tot;
      __syncthreads();
    }
  }
  if (tid == 0) ccount[img] = base < Nmax ? base : Nmax;
}

__global__ __launch_bounds__(256) void tta_gather_kernel(const float* __restrict__ cboxes, const float* __restrict__ cscores,
                                                         const int* __restrict__ cclasses, const int* __restrict__ keep,
                                                         const int* __restrict__ num_keep, int Nmax, int topk_out,
                                                         float* __restrict__ ob, float* __restrict__ osc, int* __restrict__ ocl,
                                                         int* __restrict__ ocount) {
  const int img = blockIdx.x;
  int n = num_keep[img];
  n = n < topk_out ? n : topk_out;
  for (int j = threadIdx.x; j < n; j += 256) {
    const int i = keep[(size_t)img * Nmax + j];
    const float* b = cboxes + ((size_t)img * Nmax + i) * 4;
    float* o = ob + ((size_t)img * topk_out + j) * 4;
    o[0] = b[0]; o[1] = b[1]; o[2] = b[2]; o[3] = b[3];
    osc[(size_t)img * topk_out + j] = cscores[(size_t)img * Nmax + i];
    ocl[(size_t)img * topk_out + j] = cclasses[(size_t)img * Nmax + i];
  }
  if (threadIdx.x == 0) ocount[img] = n;
}

static long long tta_align(long long n) { return (n + 255) & ~255ll; }

extern "C" long long lvc_tta_merge_workspace_bytes(int B, int Nmax) {
  return tta_align((long long)B * Nmax * 16) + tta_align((long long)B * Nmax * 4) * 3 + tta_align((long long)B * 4) * 2 +
         tta_align(lvc_batched_nms_workspace_bytes(B, Nmax));
}

// boxes [A][topk_in][4] fp32, scores [A][topk_in], classes [A][topk_in] int32, counts [A] int32: every augmentation's detections in
// its own image's coordinates (the fast path's outputs without detector_postprocess), A = all augmentations of the B images, those of
// image b at [tab[4b], tab[4b+1]).  params [A][16] fp32 (device): the inverse transform of each augmentation (tta_inverse_box).
// tab [B][4] int32 (device): (first, end, height, width).  Nmax >= the largest union (augmentations of one image x topk_in).
// Outputs: ob [B][topk_out][4], osc [B][topk_out], ocl [B][topk_out] int32, ocount [B] int32 (rows beyond the count unwritten).
// topk_out = DETECTIONS_PER_IMAGE (>= 1; the caller maps a negative value to Nmax).  No host synchronisation.
extern "C" int lvc_tta_merge(const float* boxes, const float* scores, const int* classes, const int* counts, int topk_in,
                             const float* params, const int* tab, int B, int Nmax, float score_thresh, double nms_thresh, int topk_out,
                             float* ob, float* osc, int* ocl, int* ocount, void* workspace, long long workspace_bytes, void* stream) {
  LVC_CHECK_ARG(B >= 0 && Nmax > 0 && topk_in > 0 && topk_out > 0, "bad size");
  if (B == 0) return LVC_OK;
  LVC_CHECK_ARG(boxes && scores && classes && counts && params && tab && ob && osc && ocl && ocount && workspace, "null pointer");
  LVC_CHECK_ARG(workspace_bytes >= lvc_tta_merge_workspace_bytes(B, Nmax), "workspace too small");
  LVC_CHECK_ARG(((uintptr_t)workspace & 255) == 0, "workspace must be 256-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  float* cboxes = (float*)ws; ws += tta_align((long long)B * Nmax * 16);
  float* cscores = (float*)ws; ws += tta_align((long long)B * Nmax * 4);
  int* cclasses = (int*)ws; ws += tta_align((long long)B * Nmax * 4);
  int* keep = (int*)ws; ws += tta_align((long long)B * Nmax * 4);
  int* ccount = (int*)ws; ws += tta_align((long long)B * 4);
  int* num_keep = (int*)ws; ws += tta_align((long long)B * 4);
  const long long nms_bytes = lvc_batched_nms_workspace_bytes(B, Nmax);
  hipLaunchKernelGGL(tta_union_kernel, dim3(B), dim3(256), 0, st, boxes, scores, classes, counts, topk_in, params, tab, Nmax,
                     score_thresh, cboxes, cscores, cclasses, ccount);
  LVC_CHECK_LAUNCH();
  const int rc = lvc_batched_nms(cboxes, cscores, cclasses, ccount, B, Nmax, nms_thresh, topk_out < Nmax ? topk_out : Nmax, keep,
                                 num_keep, ws, nms_bytes, stream);
  if (rc != LVC_OK) return rc;
  hipLaunchKernelGGL(tta_gather_kernel, dim3(B), dim3(256), 0, st, cboxes, cscores, cclasses, keep, num_keep, Nmax, topk_out, ob, osc,
                     ocl, ocount);
  LVC_CHECK_LAUNCH();
  return LVC_OK;
}
