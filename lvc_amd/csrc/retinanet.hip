// retinanet.hip -- lvc_retinanet_select: the per-level candidate selection of RetinaNet's inference for all images and levels in
// one call, on the device, no host read.
//   reference detectron2/modeling/meta_arch/retinanet.py:327-353 (inference_single_image, the loop over the levels),
//             detectron2/modeling/anchor_generator.py:157-178 (grid anchors = shift + cell anchor),
//             detectron2/modeling/box_regression.py:73-110 (apply_deltas)
// The reference sorts all H*W*A*K probabilities of an (image, level) (129 M per batch at 8 x 800x1333, 80 classes).  Here:
//   1. rn_compact_kernel   ONE pass over the logits.  An entry survives when its fp32 sigmoid is above the score threshold; survivors
//                          are appended to the (image, level)'s list as 64-bit keys (order-preserving logit key << 32 | flat index).
//                          The slot comes from an integer atomic: the ORDER of a list varies between runs, its CONTENT does not.
//   2. rn_select_kernel    one workgroup per (image, level): the min(topk, H*W*A) smallest keys of the list -- the keys are unique, so
//                          "larger logit first, equal logits: lower flat index first" is a total order and the result does not depend
//                          on the list's order -- sorted (LDS bitonic sort), decoded against their grid anchors, written behind the
//                          image's lower levels.  Lists of up to 2048 survivors are sorted whole; longer ones go through a radix
//                          select (up to 8 x 8 bit, stopped once the remaining candidates fit the sort) first.
// The select key is the logit, not the probability: no transcendental decides an order.  It refines the reference's sort and can
// differ from it only inside groups of entries whose fp32 probabilities are equal.  The top-k of all entries that pass the threshold
// are the first min(k, count) survivors by logit as long as the device's fp32 sigmoid is monotonic around the threshold; entries
// whose probability lies within rounding of the threshold may fall on either side, as in any fp32 evaluation.  NaN logits never
// survive.  A list that overflows its capacity sets bit 2 (value 4) of *d_status; the outputs of that call are then unspecified
// (in bounds) and the caller repeats it with max_survivors = H*W*A*K.
// Integer atomics only; every value that reaches an output is computed by exactly one thread.  Built with -ffp-contract=off.
#include "common.h"
#include "select_common.h"

#define RN_MAXL 8
#define RN_TOPK_PAD 2048
#define RN_OVERFLOW_BIT 4
#define RN_CT 256              // threads of the compaction kernel
#define RN_CU 8                // loads in flight per thread

struct RnLevels {
  const float* logits[RN_MAXL];        // [B, HW, ld_logit]: logit of (pixel p, anchor a, class k) = base[(b*HW + p)*ld + a*K + k]
  const float* deltas[RN_MAXL];        // [B, HW, ld_delta]: delta c of anchor a = base[(b*HW + p)*ld + a*4 + c]
  const float* cell_anchors[RN_MAXL];  // [A,4]
  int ld_logit[RN_MAXL], ld_delta[RN_MAXL], H[RN_MAXL], W[RN_MAXL], stride[RN_MAXL];
  int cap[RN_MAXL];                    // list capacity of a level = min(max_survivors, H*W*A*K)
  long long list_off[RN_MAXL + 1];     // prefix of cap (entries per image)
  int L, A, K;
};

__device__ __forceinline__ float rn_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

// V = 4: rows are float4-aligned (ld % 4 == 0, A*K % 4 == 0, 16-byte aligned base); V = 1: any layout
template <int V>
__global__ __launch_bounds__(RN_CT) void rn_compact_kernel(RnLevels lv, float t_lo, float score_thresh, u64* __restrict__ lists,
                                                           int* __restrict__ counts) {
  const int l = blockIdx.y, b = blockIdx.z, tid = threadIdx.x, lane = tid & 63;
  const int HW = lv.H[l] * lv.W[l], AK = lv.A * lv.K, ld = lv.ld_logit[l];
  const int nunits = (int)(((long long)HW * ld) / V);          // units of V consecutive floats (host: HW * ld < 2^31)
  const int u0 = blockIdx.x * (RN_CT * RN_CU);
  if (u0 >= nunits) return;
  const float* lg = lv.logits[l] + (size_t)b * HW * ld;
  const int cap = lv.cap[l];
  u64* list = lists + (size_t)b * lv.list_off[lv.L] + lv.list_off[l];
  int* cnt = counts + b * lv.L + l;

  // all loads first (RN_CU in flight per thread), then the tests.  Only units inside the A*K used columns are loaded: the rows may be a
  // channel slice of a wider tensor, whose last row ends before base + HW * ld.
  float x[RN_CU][V];
  int flat_of[RN_CU];
#pragma unroll
  for (int j = 0; j < RN_CU; ++j) {
    const int u = u0 + j * RN_CT + tid;
    flat_of[j] = -1;
#pragma unroll
    for (int e = 0; e < V; ++e) x[j][e] = -INFINITY;
    if (u < nunits) {
      const int e0 = u * V, row = e0 / ld, col = e0 - row * ld;
      if (col < AK) {                                            // the columns past A*K are padding (V == 4: AK % 4 == 0)
        flat_of[j] = row * AK + col;
        if (V == 4) {
          const float4 q = *reinterpret_cast<const float4*>(lg + (size_t)u * 4);
          x[j][0] = q.x; x[j][1 % V] = q.y; x[j][2 % V] = q.z; x[j][3 % V] = q.w;
        } else {
          x[j][0] = lg[u];
        }
      }
    }
  }
  unsigned int okmask = 0;                                       // bit j*V + e: entry e of unit j survives (RN_CU * V <= 32)
#pragma unroll
  for (int j = 0; j < RN_CU; ++j) {
#pragma unroll
    for (int e = 0; e < V; ++e) {
      const float v = x[j][e];
      // (v > t_lo: far below the threshold no sigmoid is evaluated)
      if (flat_of[j] >= 0 && v > t_lo && rn_sigmoid(v) > score_thresh) okmask |= 1u << (j * V + e);
    }
  }
  // ONE atomic per workgroup (8192 entries at V = 4): the survivors of a workgroup take consecutive slots, in thread order.  (One
  // atomic per wave and unit, all of an (image, level) on one address, cost more than the pass over the logits.)
  __shared__ int wsum[RN_CT / 64];
  __shared__ int s_base;
  const int mine = __popc(okmask), wave = tid >> 6;
  int incl = mine;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(incl, o);
    if (lane >= o) incl += t;
  }
  if (lane == 63) wsum[wave] = incl;
  __syncthreads();
  int wbase = 0, total = 0;
#pragma unroll
  for (int w = 0; w < RN_CT / 64; ++w) {
    if (w < wave) wbase += wsum[w];
    total += wsum[w];
  }
  if (total == 0) return;                                        // (uniform) the usual case: nothing in this workgroup's entries survives
  if (tid == 0) s_base = atomicAdd(cnt, total);                  // the count goes on past the capacity: the select sees the overflow
  __syncthreads();
  int pos = s_base + wbase + incl - mine;
#pragma unroll
  for (int j = 0; j < RN_CU; ++j) {
#pragma unroll
    for (int e = 0; e < V; ++e) {
      if (okmask & (1u << (j * V + e))) {
        if (pos < cap) list[pos] = ((u64)desc_key(x[j][e]) << 32) | (unsigned int)(flat_of[j] + e);
        ++pos;
      }
    }
  }
}

__global__ __launch_bounds__(1024) void rn_select_kernel(RnLevels lv, int topk, float anchor_offset, float wx, float wy, float ww,
                                                         float wh, float scale_clamp, const u64* __restrict__ lists,
                                                         const int* __restrict__ counts, int* __restrict__ d_status, int rows,
                                                         float* __restrict__ out_boxes, float* __restrict__ out_scores,
                                                         int* __restrict__ out_classes, int* __restrict__ out_index,
                                                         int* __restrict__ d_count) {
  __shared__ u64 sortbuf[RN_TOPK_PAD];
  __shared__ int hist[256];
  __shared__ int sh[20];
  __shared__ int s_n;
  const int l = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
  const int A = lv.A, K = lv.K, AK = A * K, W = lv.W[l], HW = lv.H[l] * W;
  // rows of the image's lower levels, and this level's: min(k, survivors) each
  int out_off = 0, m = 0, k = 0;
  for (int q = 0; q <= l; ++q) {
    const int na = lv.H[q] * lv.W[q] * A;
    const int kq = topk < na ? topk : na;
    const int cq = counts[b * lv.L + q];
    const int mq = cq < lv.cap[q] ? cq : lv.cap[q];
    if (q < l) out_off += kq < mq ? kq : mq;
    else { m = mq; k = kq; if (cq > lv.cap[q] && tid == 0) atomicOr(d_status, RN_OVERFLOW_BIT); }
  }
  const int kept = k < m ? k : m;
  const u64* list = lists + (size_t)b * lv.list_off[lv.L] + lv.list_off[l];
  int npad = 2;
  while (npad < kept) npad <<= 1;                                // <= RN_TOPK_PAD (host: topk <= 2048)

  if (m <= RN_TOPK_PAD) {
    npad = 2;
    while (npad < m) npad <<= 1;
    for (int i = tid; i < npad; i += 1024) sortbuf[i] = i < m ? list[i] : ~0ull;
    __syncthreads();
  } else {
    // radix select towards the k-th smallest key (k <= 2048 < m), most significant byte first; the keys are unique.  It stops as soon
    // as the keys below the prefix found so far plus those inside its bin fit the sort buffer (usually after two or three bytes: the
    // cut lies far out in the tail of the list); they are sorted whole and the first k taken.
    u64 prefix = 0, pmask = 0;
    int krem = k, ncand = 0;
    for (int pass = 0; pass < 8; ++pass) {
      const int shift = 56 - 8 * pass;
      if (tid < 256) hist[tid] = 0;
      __syncthreads();
      for (int i0 = 0; i0 < m; i0 += 1024) {
        const int i = i0 + tid;
        u64 key = 0;
        bool act = false;
        if (i < m) {
          key = list[i];
          act = (key & pmask) == prefix;
        }
        // LDS histogram: the digits most lanes of a wave share (constant logits, the sign / exponent byte) are added once per wave
        // -- up to four of them --, what is left goes one atomic per lane (a byte of mantissa or index: few lanes per address)
        const unsigned int d = (unsigned int)(key >> shift) & 255u;
        u64 mm = __ballot(act);
        for (int it = 0; it < 4 && mm; ++it) {
          const int first = __ffsll((long long)mm) - 1;
          const unsigned int dd = (unsigned int)__shfl((int)d, first);
          const u64 same = __ballot(act && d == dd);
          if (lane == first) atomicAdd(&hist[dd], __popcll(same));
          if (d == dd) act = false;
          mm &= ~same;
        }
        if (act) atomicAdd(&hist[d], 1);
      }
      __syncthreads();
      find_digit(hist, krem, sh);
      const int dsel = sh[8];
      prefix |= (u64)(unsigned int)dsel << shift;
      pmask |= 255ull << shift;
      krem -= sh[9];
      ncand = (k - krem) + hist[dsel];                           // keys below the prefix + keys inside its bin
      __syncthreads();
      if (ncand <= RN_TOPK_PAD) break;                           // (uniform; after the last byte the bin holds one key: ncand = k)
    }
    npad = 2;
    while (npad < ncand) npad <<= 1;
    for (int i = tid; i < npad; i += 1024) sortbuf[i] = ~0ull;
    if (tid == 0) s_n = 0;
    __syncthreads();
    for (int i = tid; i < m; i += 1024) {
      const u64 key = list[i];
      if ((key & pmask) <= prefix) {
        const int slot = atomicAdd(&s_n, 1);                     // any order: sorted below
        if (slot < npad) sortbuf[slot] = key;
      }
    }
    __syncthreads();
  }
  if (kept > 0) bitonic_sort_lds(sortbuf, npad);

  const float* lg = lv.logits[l] + (size_t)b * HW * lv.ld_logit[l];
  const float* dl = lv.deltas[l] + (size_t)b * HW * lv.ld_delta[l];
  const int stride = lv.stride[l];
  for (int r = tid; r < kept; r += 1024) {
    const int i = (int)(sortbuf[r] & 0xFFFFFFFFull);
    const int p = i / AK, col = i - p * AK;
    const int a = col / K, c = col - a * K;
    const int y = p / W, x = p - y * W;
    // torch.arange(offset * stride, size * stride, stride, dtype=float32): start + i * step, rounded once
    const float sx = (float)((double)anchor_offset * stride + (double)x * stride);
    const float sy = (float)((double)anchor_offset * stride + (double)y * stride);
    const float* ca = lv.cell_anchors[l] + a * 4;
    const float* d = dl + (size_t)p * lv.ld_delta[l] + a * 4;
    float box[4];
    apply_deltas(sx + ca[0], sy + ca[1], sx + ca[2], sy + ca[3], d[0], d[1], d[2], d[3], wx, wy, ww, wh, scale_clamp, box);
    const size_t o = (size_t)b * rows + out_off + r;
    *reinterpret_cast<float4*>(out_boxes + o * 4) = float4{box[0], box[1], box[2], box[3]};
    out_scores[o] = rn_sigmoid(lg[(size_t)p * lv.ld_logit[l] + col]);
    out_classes[o] = c;
    out_index[o] = i;
  }
  if (l == lv.L - 1) {                                           // the last level's workgroup: rows past the count = 0
    const int total = out_off + kept;
    for (int r = total + tid; r < rows; r += 1024) {
      const size_t o = (size_t)b * rows + r;
      *reinterpret_cast<float4*>(out_boxes + o * 4) = float4{0.f, 0.f, 0.f, 0.f};
      out_scores[o] = 0.f;
      out_classes[o] = 0;
      out_index[o] = 0;
    }
    if (tid == 0) d_count[b] = total;
  }
}

struct RnPlan {
  long long entries;      // list entries per image
  long long off_counts, off_lists, total;
  int cap[RN_MAXL];
};
static RnPlan rn_plan(int B, int L, int A, int K, const int* Hs, const int* Ws, int max_survivors) {
  RnPlan p;
  p.entries = 0;
  for (int l = 0; l < L; ++l) {
    const long long n = (long long)Hs[l] * Ws[l] * A * K;
    p.cap[l] = (int)(n < max_survivors ? n : max_survivors);
    p.entries += p.cap[l];
  }
  p.off_counts = 0;
  p.off_lists = ((long long)B * L * 4 + 255) & ~255ll;
  p.total = p.off_lists + (long long)B * p.entries * 8;
  return p;
}
static bool rn_shapes_ok(int B, int L, int A, int K, const int* Hs, const int* Ws, int topk, int max_survivors) {
  if (!(L >= 1 && L <= RN_MAXL && B > 0 && A > 0 && K > 0 && Hs && Ws && topk > 0 && topk <= RN_TOPK_PAD && max_survivors > 0))
    return false;
  for (int l = 0; l < L; ++l)
    if (Hs[l] <= 0 || Ws[l] <= 0 || (long long)Hs[l] * Ws[l] * A * K >= (1ll << 31)) return false;
  return true;
}

extern "C" long long lvc_retinanet_select_workspace_bytes(int B, int L, int A, int K, const int* Hs, const int* Ws, int topk,
                                                          int max_survivors) {
  if (!rn_shapes_ok(B, L, A, K, Hs, Ws, topk, max_survivors)) return -1;
  return rn_plan(B, L, A, K, Hs, Ws, max_survivors).total;
}

extern "C" int lvc_retinanet_select(const float* const* logits, const int* ld_logit, const float* const* deltas,
                                    const int* ld_delta, const float* const* cell_anchors, const int* Hs, const int* Ws,
                                    const int* strides, float anchor_offset, int L, int A, int K, int B, int topk,
                                    float score_thresh, float wx, float wy, float ww, float wh, float scale_clamp,
                                    int max_survivors, float* out_boxes, float* out_scores, int* out_classes, int* out_index,
                                    int* d_count, int* d_status, void* workspace, long long workspace_bytes, void* stream) {
  LVC_CHECK_ARG(rn_shapes_ok(B, L, A, K, Hs, Ws, topk, max_survivors),
                "needs 1..8 levels, positive B / A / K / H / W / max_survivors, topk in 1..2048, H*W*A*K < 2^31 per level");
  LVC_CHECK_ARG(logits && ld_logit && deltas && ld_delta && cell_anchors && strides && out_boxes && out_scores && out_classes &&
                    out_index && d_count && d_status && workspace, "null pointer");
  LVC_CHECK_ARG(wx > 0.f && wy > 0.f && ww > 0.f && wh > 0.f, "box weights must be positive");
  LVC_CHECK_ARG(((uintptr_t)out_boxes & 15) == 0 && ((uintptr_t)workspace & 15) == 0, "out_boxes / workspace must be 16-byte aligned");
  RnPlan p = rn_plan(B, L, A, K, Hs, Ws, max_survivors);
  LVC_CHECK_ARG(workspace_bytes >= p.total, "workspace too small");
  RnLevels lv;
  memset(&lv, 0, sizeof lv);
  lv.L = L; lv.A = A; lv.K = K;
  bool vec = (A * K) % 4 == 0;
  long long max_units = 0;
  for (int l = 0; l < L; ++l) {
    LVC_CHECK_ARG(logits[l] && deltas[l] && cell_anchors[l], "null level pointer");
    LVC_CHECK_ARG(ld_logit[l] >= A * K && ld_delta[l] >= 4 * A, "row strides must cover A*K logits / 4*A deltas");
    LVC_CHECK_ARG((long long)Hs[l] * Ws[l] * ld_logit[l] < (1ll << 31), "a level's logit rows must stay below 2^31 floats per image");
    LVC_CHECK_ARG(((uintptr_t)logits[l] & 3) == 0 && ((uintptr_t)deltas[l] & 3) == 0, "pointers must be 4-byte aligned");
    lv.logits[l] = logits[l]; lv.deltas[l] = deltas[l]; lv.cell_anchors[l] = cell_anchors[l];
    lv.ld_logit[l] = ld_logit[l]; lv.ld_delta[l] = ld_delta[l];
    lv.H[l] = Hs[l]; lv.W[l] = Ws[l]; lv.stride[l] = strides[l];
    lv.cap[l] = p.cap[l];
    lv.list_off[l + 1] = lv.list_off[l] + p.cap[l];
    vec = vec && ld_logit[l] % 4 == 0 && ((uintptr_t)logits[l] & 15) == 0;
    const long long e = (long long)Hs[l] * Ws[l] * ld_logit[l];
    if (e > max_units) max_units = e;
  }
  char* ws = (char*)workspace;
  hipStream_t st = (hipStream_t)stream;
  int* counts = (int*)(ws + p.off_counts);
  u64* lists = (u64*)(ws + p.off_lists);
  if (hipMemsetAsync(counts, 0, (size_t)B * L * 4, st) != hipSuccess) {
    lvc_set_error("%s: hipMemsetAsync failed", __func__);
    return LVC_ERR_HIP;
  }
  // the logit below which no sigmoid is evaluated: well under the threshold's own logit (the margin covers the fp32 evaluation)
  float t_lo;
  if (!(score_thresh > 0.f)) {
    t_lo = -INFINITY;
  } else if (score_thresh >= 1.f) {
    t_lo = INFINITY;
  } else {
    const double th = (double)score_thresh;
    t_lo = (float)(log(th / (1.0 - th)) - (1e-3 + 1e-6 / (th * (1.0 - th))));
  }
  const int per_block = RN_CT * RN_CU;
  if (vec) {
    const int gx = (int)((max_units / 4 + per_block - 1) / per_block);
    hipLaunchKernelGGL(rn_compact_kernel<4>, dim3(gx > 0 ? gx : 1, L, B), dim3(RN_CT), 0, st, lv, t_lo, score_thresh, lists, counts);
  } else {
    const int gx = (int)((max_units + per_block - 1) / per_block);
    hipLaunchKernelGGL(rn_compact_kernel<1>, dim3(gx > 0 ? gx : 1, L, B), dim3(RN_CT), 0, st, lv, t_lo, score_thresh, lists, counts);
  }
  LVC_CHECK_LAUNCH();
  hipLaunchKernelGGL(rn_select_kernel, dim3(L, B), dim3(1024), 0, st, lv, topk, anchor_offset, wx, wy, ww, wh, scale_clamp, lists,
                     counts, d_status, L * topk, out_boxes, out_scores, out_classes, out_index, d_count);
  LVC_CHECK_LAUNCH();
  return LVC_OK;
}
