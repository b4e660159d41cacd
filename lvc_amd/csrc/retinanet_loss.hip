// retinanet_loss.hip -- the training loss of RetinaNet (reference detectron2/modeling/meta_arch/retinanet.py:184-236 `losses`, with
// fvcore's sigmoid_focal_loss and smooth_l1_loss, Box2BoxTransform.get_deltas and the loss-normaliser EMA) on the head's own outputs.
//
//   lvc_retinanet_loss        one streaming pass over the per-level NHWC logits [B,H_l,W_l,ld] and deltas + a one-workgroup finish:
//                             focal-loss sum over the valid anchors' K entries, smooth-L1 sum over the positive anchors, the number of
//                             positives, the EMA normaliser (device double) and the two losses divided by it
//   lvc_retinanet_loss_grad   one pass that writes d(loss)/d(logits) and d(loss)/d(deltas) in the layout the predictors' backward
//                             consumes, already times the upstream scalars / the normaliser; padding channels are written as zero
//
// The target of an entry is derived here from the outputs of lvc_match_boxes_batched (labels int8 [B,R]: 1 positive, 0 background,
// -1 ignored; matches int32 [B,R]) and gt_classes: no [B,R] class tensor, no one-hot, no gather, no concatenation.  R runs level after
// level, p*A + a inside a level (`Boxes.cat(anchors)`); entry (p*A + a)*K + k of a level is channel a*K + k of pixel p.
//
// Work is cut into 2L segments -- the logits and the deltas of each level -- and every workgroup belongs to one segment, so the level's
// pointers and strides are wave-uniform.  A lane handles SLOTS of four consecutive channels of a pixel row (one 16-byte access where the
// row width, the stride and the base pointer allow it, scalar accesses otherwise) and maps each of the four entries to its anchor by
// itself: K may be smaller than a slot, and a slot may straddle two anchors.
//
// Sums: the loss terms are evaluated in fp64 (the gradient entries in fp32); every lane adds its terms in a fixed order, a workgroup's lanes are added by a fixed shuffle tree, its three totals
// go to the workgroup's own slot of the workspace, and the finish adds the slots in index order -- no float atomics, bit-identical runs.
// Built with -ffp-contract=off like the other loss files.
#include "common.h"

#define RL_MAXL 8
#define RL_NT 256

struct RlArgs {
  const float* logits[RL_MAXL];
  const float* deltas[RL_MAXL];
  float* dlogits[RL_MAXL];
  float* ddeltas[RL_MAXL];
  int ld_logit[RL_MAXL], ld_delta[RL_MAXL], ld_dlogit[RL_MAXL], ld_ddelta[RL_MAXL];
  int HW[RL_MAXL];
  int r_off[RL_MAXL];            // first anchor of the level inside R
  int vec[RL_MAXL];              // bit 0: 16-byte loads of the logits, bit 1: 16-byte stores of dlogits, bit 2: loads of the deltas, bit 3: stores of ddeltas
  int blk_off[2 * RL_MAXL + 1];  // first workgroup of segment s (s < L: logits of level s; else deltas of level s - L)
  int L, A, K, B, R, per_thread;
  const float* anchors;          // [R,4]
  const int* matches;            // [B,R]
  const signed char* labels;     // [B,R]
  const float* gt;               // [Gtot,4]
  const long long* gt_classes;   // [Gtot]
  const int* gt_off;             // [B+1]
  double alpha, gamma, beta, wx, wy, ww, wh;      // doubles: 0.1 as a float is 1.5e-8 away from the reference's Python 0.1
};

// Box2BoxTransform.get_deltas (box_regression.py:40-71), evaluated in fp64 (as csrc/train.hip: in fp32 the two centres are rounded at the
// size of the coordinates before they are subtracted, and smooth-L1's 1 / beta multiplies that error in the gradient).  Four values per
// positive anchor: the cost is nothing next to the pass over the logits.
__device__ __forceinline__ void rl_get_deltas(const float4 s, const float4 t, double wx, double wy, double ww, double wh, double* d) {
  const double sw = (double)s.z - s.x, sh = (double)s.w - s.y, scx = s.x + 0.5 * sw, scy = s.y + 0.5 * sh;
  const double tw = (double)t.z - t.x, th = (double)t.w - t.y, tcx = t.x + 0.5 * tw, tcy = t.y + 0.5 * th;
  d[0] = wx * (tcx - scx) / sw;
  d[1] = wy * (tcy - scy) / sh;
  d[2] = ww * log(tw / sw);
  d[3] = wh * log(th / sh);
}

// fvcore smooth_l1_loss: beta < 1e-5 is pure L1
__device__ __forceinline__ double rl_smooth_l1(double x, double t, double beta, double* grad) {
  const double n = fabs(x - t);
  if (beta < 1e-5) { *grad = x > t ? 1.0 : (x < t ? -1.0 : 0.0); return n; }
  if (n < beta) { *grad = (x - t) / beta; return 0.5 * n * n / beta; }
  *grad = x > t ? 1.0 : -1.0;
  return n - 0.5 * beta;
}

// One entry of fvcore's sigmoid_focal_loss.  With z = x for t = 1 and z = -x for t = 0: p_t = sigmoid(z), ce = -log p_t = softplus(-z)
// = max(-z, 0) + log1p(exp(-|z|)), q = 1 - p_t = sigmoid(-z) formed from e = exp(-|z|) directly (no 1 - p cancellation, finite and
// correct at |x| = 90: ce = max(-z, 0) + ~0, q in {~0, 1}).
//   loss = alpha_t * ce * q^gamma,     dloss/dz = alpha_t * q^gamma * (gamma * p_t * log p_t - q)
// (1 - p_t)^gamma never goes through pow for gamma = 2, 0 and 1.
//
// The LOSS terms are evaluated in fp64: the sums are held to 3 x the deviation of an fp32 evaluation from an fp64 one, and an fp32
// evaluation here would be that fp32 evaluation -- inside its own noise, not a third of it.  The GRADIENT (an fp32 tensor, one rounding
// of each entry is the floor anyway) is evaluated in fp32.
__device__ __forceinline__ double rl_focal_loss(float x, bool t, double alpha, double gamma) {
  const double z = t ? (double)x : -(double)x;
  const double e = exp(-fabs(z));
  const double inv = 1.0 / (1.0 + e);
  const double q = z >= 0.0 ? e * inv : inv;
  const double ce = fmax(-z, 0.0) + log1p(e);
  const double at = alpha >= 0.0 ? (t ? alpha : 1.0 - alpha) : 1.0;
  const double m = gamma == 2.0 ? q * q : (gamma == 0.0 ? 1.0 : (gamma == 1.0 ? q : pow(q, gamma)));
  return at * (ce * m);
}

__device__ __forceinline__ float rl_focal_grad(float x, bool t, float alpha, float gamma) {
  const float z = t ? x : -x;
  const float e = expf(-fabsf(z));
  const float inv = 1.f / (1.f + e);
  const float pt = z >= 0.f ? inv : e * inv;
  const float q = z >= 0.f ? e * inv : inv;
  const float ce = fmaxf(-z, 0.f) + log1pf(e);
  const float at = alpha >= 0.f ? (t ? alpha : 1.f - alpha) : 1.f;
  const float m = gamma == 2.f ? q * q : (gamma == 0.f ? 1.f : (gamma == 1.f ? q : powf(q, gamma)));
  const float dz = at * (m * (-(gamma * pt) * ce - q));
  return t ? dz : -dz;
}

// class of the gt box that anchor (b, r) is matched to, or -1 (background: every target 0), or -2 (ignored)
__device__ __forceinline__ int rl_anchor_class(const RlArgs& a, int b, int r, int g0, int G) {
  const int lab = a.labels[(size_t)b * a.R + r];
  if (lab < 0) return -2;
  if (lab == 0 || G <= 0) return -1;
  const int m = a.matches[(size_t)b * a.R + r];
  if (m < 0 || m >= G) return -1;
  const long long c = a.gt_classes[g0 + m];
  return (c >= 0 && c < a.K) ? (int)c : -1;
}

// Position of a lane inside its segment: item i = (b*HW + p) * nslot + s.  One set of 32-bit divisions for the first item; every
// further item is 256 items on, reached by additions with carries (the steps are wave-uniform).
struct RlCursor {
  unsigned i, row, s, b, p;
  unsigned d_row, d_s, d_b, d_p, nslot, HW;
  __device__ __forceinline__ void init(unsigned first, unsigned nslot_, unsigned HW_) {
    nslot = nslot_; HW = HW_;
    i = first; row = first / nslot; s = first - row * nslot; b = row / HW; p = row - b * HW;
    d_row = RL_NT / nslot; d_s = RL_NT - d_row * nslot; d_b = d_row / HW; d_p = d_row - d_b * HW;
  }
  __device__ __forceinline__ void next() {
    i += RL_NT; s += d_s; row += d_row; p += d_p; b += d_b;
    if (s >= nslot) { s -= nslot; ++row; ++p; }
    if (p >= HW) { p -= HW; ++b; }
  }
};

// GRAD = false: partial sums of this workgroup -> part[blockIdx.x * 2 + {0,1}], cnt[blockIdx.x].
// GRAD = true:  dlogits / ddeltas = derivative * scale, scale = upstream scalar / normaliser.
template <bool GRAD>
__global__ __launch_bounds__(RL_NT) void retinanet_loss_kernel(const RlArgs a, double* __restrict__ part, int* __restrict__ cnt,
                                                               const double* __restrict__ normalizer,
                                                               const float* __restrict__ g_cls, const float* __restrict__ g_box) {
  int seg = 0;
  while (seg + 1 < 2 * a.L && (int)blockIdx.x >= a.blk_off[seg + 1]) ++seg;
  const bool is_cls = seg < a.L;
  const int l = is_cls ? seg : seg - a.L;
  const int HW = a.HW[l], A = a.A, K = a.K;
  // (fewer than 2^31 items per segment: checked by the host)
  const unsigned first = (unsigned)(blockIdx.x - a.blk_off[seg]) * (unsigned)(RL_NT * a.per_thread) + threadIdx.x;
  RlCursor cur;
  double s_cls = 0.0, s_box = 0.0;
  int npos = 0;
  float sc_cls = 0.f;
  double sc_box = 0.0;
  if (GRAD) {
    const double nz = normalizer[0];
    sc_cls = (float)((double)g_cls[0] / nz);
    sc_box = (double)g_box[0] / nz;
  }
  const float alpha_f = (float)a.alpha, gamma_f = (float)a.gamma;
  if (is_cls) {
    const int AK = A * K;
    const int width = GRAD ? a.ld_dlogit[l] : AK;       // the gradient pass also covers the padding channels (zeros)
    const int nslot = (width + 3) >> 2;
    const unsigned nitem = (unsigned)a.B * HW * nslot;
    const int ld = a.ld_logit[l];
    const bool vin = a.vec[l] & 1, vout = a.vec[l] & 2;
    const float* __restrict__ src = a.logits[l];
    cur.init(first, nslot, HW);
    for (int it = 0; it < a.per_thread; ++it, cur.next()) {
      if (cur.i >= nitem) break;
      const int row = (int)cur.row;                     // b*HW + p
      const int c0 = (int)cur.s << 2;
      const int b = (int)cur.b, p = (int)cur.p;
      const int nv = min(4, AK - c0);                   // entries of the slot (<= 0: padding only)
      float x[4] = {0.f, 0.f, 0.f, 0.f}, o[4] = {0.f, 0.f, 0.f, 0.f};
      if (nv > 0) {
        const float* ps = src + (size_t)row * ld + c0;
        if (vin && nv == 4) {
          const float4 v = *reinterpret_cast<const float4*>(ps);
          x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
        } else {
          for (int j = 0; j < 4; ++j)
            if (j < nv) x[j] = ps[j];
        }
        const int g0 = a.gt_off[b], G = a.gt_off[b + 1] - g0;
        int an = (int)((unsigned)c0 / (unsigned)K), k = c0 - an * K;
        int cls = rl_anchor_class(a, b, a.r_off[l] + p * A + an, g0, G);
        for (int j = 0; j < 4; ++j) {
          if (j < nv) {
            if (cls != -2) {
              if (GRAD) o[j] = rl_focal_grad(x[j], k == cls, alpha_f, gamma_f) * sc_cls;
              else s_cls += rl_focal_loss(x[j], k == cls, a.alpha, a.gamma);
            }
            if (++k == K && j + 1 < nv) {
              k = 0;
              ++an;
              cls = rl_anchor_class(a, b, a.r_off[l] + p * A + an, g0, G);
            }
          }
        }
      }
      if (GRAD) {
        float* pd = a.dlogits[l] + (size_t)row * width + c0;
        if (vout) {
          *reinterpret_cast<float4*>(pd) = make_float4(o[0], o[1], o[2], o[3]);
        } else {
          for (int j = 0; j < 4; ++j)
            if (c0 + j < width) pd[j] = o[j];
        }
      }
    }
  } else {
    const int width = GRAD ? a.ld_ddelta[l] : 4 * A;
    const int nslot = (width + 3) >> 2;
    const unsigned nitem = (unsigned)a.B * HW * nslot;
    const int ld = a.ld_delta[l];
    const bool vin = a.vec[l] & 4, vout = a.vec[l] & 8;
    const float* __restrict__ src = a.deltas[l];
    cur.init(first, nslot, HW);
    for (int it = 0; it < a.per_thread; ++it, cur.next()) {
      if (cur.i >= nitem) break;
      const int row = (int)cur.row;
      const int an = (int)cur.s;
      const int b = (int)cur.b, p = (int)cur.p;
      float o[4] = {0.f, 0.f, 0.f, 0.f};
      if (an < A) {
        const int r = a.r_off[l] + p * A + an;
        const int g0 = a.gt_off[b], G = a.gt_off[b + 1] - g0;
        const int m = a.matches ? a.matches[(size_t)b * a.R + r] : 0;
        if (a.labels[(size_t)b * a.R + r] == 1 && G > 0 && m >= 0 && m < G) {
          const float* ps = src + (size_t)row * ld + an * 4;
          float x[4];
          if (vin) {
            const float4 v = *reinterpret_cast<const float4*>(ps);
            x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
          } else {
            for (int j = 0; j < 4; ++j) x[j] = ps[j];
          }
          const float4 anc = *reinterpret_cast<const float4*>(a.anchors + (size_t)r * 4);
          const float4 gb = *reinterpret_cast<const float4*>(a.gt + (size_t)(g0 + m) * 4);
          double t[4], gr;
          rl_get_deltas(anc, gb, a.wx, a.wy, a.ww, a.wh, t);
          for (int j = 0; j < 4; ++j) {
            const double v = rl_smooth_l1((double)x[j], t[j], a.beta, &gr);
            if (GRAD) o[j] = (float)(gr * sc_box);
            else s_box += v;
          }
          ++npos;
        }
      }
      if (GRAD) {
        float* pd = a.ddeltas[l] + (size_t)row * width + an * 4;
        if (vout) {
          *reinterpret_cast<float4*>(pd) = make_float4(o[0], o[1], o[2], o[3]);
        } else {
          for (int j = 0; j < 4; ++j)
            if (an * 4 + j < width) pd[j] = o[j];
        }
      }
    }
  }
  if (!GRAD) {
    __shared__ double red[2][RL_NT / 64];
    __shared__ int redn[RL_NT / 64];
    for (int o = 32; o > 0; o >>= 1) {
      s_cls += __shfl_xor(s_cls, o);
      s_box += __shfl_xor(s_box, o);
      npos += __shfl_xor(npos, o);
    }
    if ((threadIdx.x & 63) == 0) {
      red[0][threadIdx.x >> 6] = s_cls;
      red[1][threadIdx.x >> 6] = s_box;
      redn[threadIdx.x >> 6] = npos;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      double c = 0.0, x = 0.0;
      int n = 0;
      for (int w = 0; w < RL_NT / 64; ++w) { c += red[0][w]; x += red[1][w]; n += redn[w]; }
      part[(size_t)blockIdx.x * 2] = c;
      part[(size_t)blockIdx.x * 2 + 1] = x;
      cnt[blockIdx.x] = n;
    }
  }
}

// The workgroups' slots in index order: lane t adds the slots of its contiguous range one after the other, then the 256 range totals are
// added one after the other.  normalizer_out = momentum * normalizer_in + one_minus_momentum * max(num_pos, 1) with an uncontracted
// multiply and add each, as the reference's Python float arithmetic.
__global__ __launch_bounds__(RL_NT) void retinanet_loss_finish_kernel(const double* __restrict__ part, const int* __restrict__ cnt,
                                                                      int nblk, double momentum, double one_minus_momentum,
                                                                      const double* __restrict__ normalizer_in,
                                                                      double* __restrict__ normalizer_out,
                                                                      float* __restrict__ out_losses, double* __restrict__ out_sums,
                                                                      int* __restrict__ num_pos) {
  __shared__ double red[2][RL_NT];
  __shared__ int redn[RL_NT];
  const int per = (nblk + RL_NT - 1) / RL_NT;
  const int lo = threadIdx.x * per, hi = min(nblk, lo + per);
  double c = 0.0, x = 0.0;
  int n = 0;
  for (int i = lo; i < hi; ++i) { c += part[(size_t)i * 2]; x += part[(size_t)i * 2 + 1]; n += cnt[i]; }
  red[0][threadIdx.x] = c;
  red[1][threadIdx.x] = x;
  redn[threadIdx.x] = n;
  __syncthreads();
  if (threadIdx.x == 0) {
    c = 0.0; x = 0.0; n = 0;
    for (int t = 0; t < RL_NT; ++t) { c += red[0][t]; x += red[1][t]; n += redn[t]; }
    const double nz = __dadd_rn(__dmul_rn(momentum, normalizer_in[0]), __dmul_rn(one_minus_momentum, (double)max(n, 1)));
    normalizer_out[0] = nz;
    out_losses[0] = (float)(c / nz);
    out_losses[1] = (float)(x / nz);
    if (out_sums) { out_sums[0] = c; out_sums[1] = x; }
    num_pos[0] = n;
  }
}

static bool rl_aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

// Fills the launch arguments; returns the number of workgroups or -1.
static long long rl_plan(RlArgs& a, bool grad, const float* const* logits, const int* ld_logit, const float* const* deltas,
                         const int* ld_delta, float* const* dlogits, const int* ld_dlogit, float* const* ddeltas,
                         const int* ld_ddelta, const int* Hs, const int* Ws, int L, int A, int K, int B) {
  if (!(L >= 1 && L <= RL_MAXL && A >= 1 && K >= 1 && B >= 1)) return -1;
  long long R = 0, slots = 0;
  for (int l = 0; l < L; ++l) {
    if (!(Hs[l] > 0 && Ws[l] > 0 && logits[l] && deltas[l] && ld_logit[l] >= A * K && ld_delta[l] >= 4 * A)) return -1;
    if (grad && !(dlogits[l] && ddeltas[l] && ld_dlogit[l] >= A * K && ld_ddelta[l] >= 4 * A)) return -1;
    const long long hw = (long long)Hs[l] * Ws[l];
    const long long wl = grad ? ld_dlogit[l] : A * K, wd = grad ? ld_ddelta[l] : 4 * A;
    if (B * hw * (ld_logit[l] > wl ? ld_logit[l] : wl) >= (1ll << 31) || B * hw * (ld_delta[l] > wd ? ld_delta[l] : wd) >= (1ll << 31)) return -1;
    a.logits[l] = logits[l]; a.deltas[l] = deltas[l];
    a.ld_logit[l] = ld_logit[l]; a.ld_delta[l] = ld_delta[l];
    a.dlogits[l] = grad ? dlogits[l] : nullptr; a.ddeltas[l] = grad ? ddeltas[l] : nullptr;
    a.ld_dlogit[l] = grad ? ld_dlogit[l] : 0; a.ld_ddelta[l] = grad ? ld_ddelta[l] : 0;
    a.HW[l] = (int)hw;
    a.r_off[l] = (int)R;
    int v = 0;
    if (ld_logit[l] % 4 == 0 && rl_aligned16(logits[l])) v |= 1;
    if (grad && ld_dlogit[l] % 4 == 0 && rl_aligned16(dlogits[l])) v |= 2;
    if (ld_delta[l] % 4 == 0 && rl_aligned16(deltas[l])) v |= 4;
    if (grad && ld_ddelta[l] % 4 == 0 && rl_aligned16(ddeltas[l])) v |= 8;
    a.vec[l] = v;
    R += hw * A;
    slots += B * hw * ((wl + 3) / 4) + B * hw * ((wd + 3) / 4);
  }
  if (R * B >= (1ll << 31)) return -1;
  // slots per lane: enough that the partial-sum list stays a few thousand entries long at the largest inputs
  int per = (int)((slots + (long long)RL_NT * 4096 - 1) / ((long long)RL_NT * 4096));
  per = per < 1 ? 1 : (per > 64 ? 64 : per);
  a.per_thread = per;
  long long blk = 0;
  for (int s = 0; s < 2 * L; ++s) {
    const int l = s < L ? s : s - L;
    const long long w = s < L ? (grad ? ld_dlogit[l] : A * K) : (grad ? ld_ddelta[l] : 4 * A);
    const long long n = (long long)B * a.HW[l] * ((w + 3) / 4);
    a.blk_off[s] = (int)blk;
    blk += (n + (long long)RL_NT * per - 1) / ((long long)RL_NT * per);
  }
  a.blk_off[2 * L] = (int)blk;
  if (blk >= (1ll << 31)) return -1;
  a.L = L; a.A = A; a.K = K; a.B = B; a.R = (int)R;
  return blk;
}

extern "C" long long lvc_retinanet_loss_workspace_bytes(int B, int L, int A, int K, const int* Hs, const int* Ws) {
  RlArgs a;
  const float* dummy[RL_MAXL];
  int ldl[RL_MAXL], ldd[RL_MAXL];
  if (!(L >= 1 && L <= RL_MAXL && A >= 1 && K >= 1 && Hs && Ws)) return -1;
  for (int l = 0; l < L; ++l) { dummy[l] = (const float*)16; ldl[l] = A * K; ldd[l] = 4 * A; }
  const long long blk = rl_plan(a, false, dummy, ldl, dummy, ldd, nullptr, nullptr, nullptr, nullptr, Hs, Ws, L, A, K, B);
  return blk < 0 ? -1 : blk * (2 * (long long)sizeof(double) + (long long)sizeof(int)) + 16;
}

static bool rl_gamma_ok(double gamma) { return gamma == 0.0 || gamma >= 1.0; }

extern "C" int lvc_retinanet_loss(const float* const* logits, const int* ld_logit, const float* const* deltas, const int* ld_delta,
                                  const int* Hs, const int* Ws, int L, int A, int K, int B, const float* anchors, const int* matches,
                                  const signed char* labels, const float* gt, const long long* gt_classes, const int* gt_off,
                                  double alpha, double gamma, double beta, double wx, double wy, double ww, double wh, double momentum,
                                  double one_minus_momentum, const double* normalizer_in, double* normalizer_out, float* out_losses,
                                  double* out_sums, int* num_pos, void* workspace, long long workspace_bytes, void* stream) {
  LVC_CHECK_ARG(logits && ld_logit && deltas && ld_delta && Hs && Ws, "null pointer");
  LVC_CHECK_ARG(anchors && matches && labels && gt_off && normalizer_in && normalizer_out && out_losses && num_pos && workspace, "null pointer");
  LVC_CHECK_ARG(rl_aligned16(anchors) && (!gt || rl_aligned16(gt)), "anchors / gt must be 16-byte aligned");
  LVC_CHECK_ARG(rl_gamma_ok(gamma), "FOCAL_LOSS_GAMMA in (0,1) (unbounded derivative at saturation) or negative");
  RlArgs a;
  const long long blk = rl_plan(a, false, logits, ld_logit, deltas, ld_delta, nullptr, nullptr, nullptr, nullptr, Hs, Ws, L, A, K, B);
  LVC_CHECK_ARG(blk > 0, "shapes outside the kernel's range (1..8 levels, ld >= A*K / 4A, < 2^31 entries per level)");
  LVC_CHECK_ARG(workspace_bytes >= blk * (2 * (long long)sizeof(double) + (long long)sizeof(int)) + 16 && rl_aligned16(workspace), "workspace too small or misaligned");
  a.anchors = anchors; a.matches = matches; a.labels = labels; a.gt = gt; a.gt_classes = gt_classes; a.gt_off = gt_off;
  a.alpha = alpha; a.gamma = gamma; a.beta = beta; a.wx = wx; a.wy = wy; a.ww = ww; a.wh = wh;
  double* part = (double*)workspace;
  int* cnt = (int*)(part + blk * 2);
  hipLaunchKernelGGL(retinanet_loss_kernel<false>, dim3((unsigned)blk), dim3(RL_NT), 0, (hipStream_t)stream, a, part, cnt,
                     (const double*)nullptr, (const float*)nullptr, (const float*)nullptr);
  LVC_CHECK_LAUNCH();
  hipLaunchKernelGGL(retinanet_loss_finish_kernel, dim3(1), dim3(RL_NT), 0, (hipStream_t)stream, part, cnt, (int)blk, momentum,
                     one_minus_momentum, normalizer_in, normalizer_out, out_losses, out_sums, num_pos);
  LVC_CHECK_LAUNCH();
  return LVC_OK;
}

extern "C" int lvc_retinanet_loss_grad(const float* const* logits, const int* ld_logit, const float* const* deltas,
                                       const int* ld_delta, const int* Hs, const int* Ws, int L, int A, int K, int B,
                                       const float* anchors, const int* matches, const signed char* labels, const float* gt,
                                       const long long* gt_classes, const int* gt_off, double alpha, double gamma, double beta, double wx,
                                       double wy, double ww, double wh, const double* normalizer, const float* g_cls, const float* g_box,
                                       float* const* dlogits, const int* ld_dlogit, float* const* ddeltas, const int* ld_ddelta,
                                       void* stream) {
  LVC_CHECK_ARG(logits && ld_logit && deltas && ld_delta && Hs && Ws && dlogits && ld_dlogit && ddeltas && ld_ddelta, "null pointer");
  LVC_CHECK_ARG(anchors && matches && labels && gt_off && normalizer && g_cls && g_box, "null pointer");
  LVC_CHECK_ARG(rl_aligned16(anchors) && (!gt || rl_aligned16(gt)), "anchors / gt must be 16-byte aligned");
  LVC_CHECK_ARG(rl_gamma_ok(gamma), "FOCAL_LOSS_GAMMA in (0,1) (unbounded derivative at saturation) or negative");
  RlArgs a;
  const long long blk = rl_plan(a, true, logits, ld_logit, deltas, ld_delta, dlogits, ld_dlogit, ddeltas, ld_ddelta, Hs, Ws, L, A, K, B);
  LVC_CHECK_ARG(blk > 0, "shapes outside the kernel's range (1..8 levels, ld >= A*K / 4A, < 2^31 entries per level)");
  a.anchors = anchors; a.matches = matches; a.labels = labels; a.gt = gt; a.gt_classes = gt_classes; a.gt_off = gt_off;
  a.alpha = alpha; a.gamma = gamma; a.beta = beta; a.wx = wx; a.wy = wy; a.ww = ww; a.wh = wh;
  hipLaunchKernelGGL(retinanet_loss_kernel<true>, dim3((unsigned)blk), dim3(RL_NT), 0, (hipStream_t)stream, a, (double*)nullptr,
                     (int*)nullptr, normalizer, g_cls, g_box);
  LVC_CHECK_LAUNCH();
  return LVC_OK;
}
