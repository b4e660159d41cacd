// GroupNorm on NHWC fp32 maps (reference detectron2/layers/batch_norm.py:127-150, "GN" -> nn.GroupNorm(32, C)): the norm of the
// FPN convs (MODEL.FPN.NORM) and of the 4conv1fc box head (MODEL.ROI_BOX_HEAD.NORM).
//
//   forward   y = act(((x - mean) * rstd) * gamma + beta) [+ residual | + up2(residual)],  mean / rstd per (sample, group)
//   backward  g = relu mask of dy;  dgamma[c] = sum g * xhat,  dbeta[c] = sum g,
//             dx = rstd * (g * gamma - (A * xhat + B)),  A / B = the group means of g * gamma * xhat and g * gamma
//
// Two regimes, chosen by the caller through `tile_rows`:
//   tile_rows == 0  one workgroup owns whole samples (box head, [M,7,7,256]: 392 values per group).  A sample that fits the 64 KB
//                   of LDS is read from HBM once, kept there for the statistics and the apply pass, and written once.
//   tile_rows  > 0  a sample is cut into tiles of `tile_rows` image rows (pyramid maps: p2 has 537 600 values per group and only
//                   N * G (sample, group) pairs).  Tile partials go to a workspace slab and are combined in tile order.
//
// Statistics are never formed as E[x^2] - E[x]^2: a tile's sums are taken about a shift K (the tile's first value of the group,
// so |mean - K| is of the order of the deviation) in double-precision accumulators (the kernels are bound by memory: the fp64 adds
// are free), and tiles are combined with Chan's (count, mean, M2) update, in double.  Channel sums of the backward are accumulated,
// kept in the slabs and added up in double as well; results are rounded to fp32 once.  Every sum has a fixed order and there are no float atomics: repeated runs are bit-identical.
// This file is built with -ffp-contract=off (csrc/Makefile, EXACT_SRCS): the backward recomputes the forward's pre-activation value
// for the ReLU mask and must round as the forward did.
//
// Thread map of every kernel: a workgroup is PP pixel rows x CT channel units (a unit = VEC consecutive channels, one 16-byte
// access at VEC = 4, where C / G is a multiple of 4; at C = 256 one wave covers a pixel's 1 KB).  A thread keeps its channel unit and
// walks pixels, so a unit never leaves its group and gamma / beta / mean / rstd stay in registers.
#include "common.h"

namespace {

constexpr int GN_THREADS = 256;
constexpr int GN_LDS_BYTES = 64 * 1024;
constexpr int GN_SMALL_GRID = 1024;    // workgroups of the whole-sample kernels (each walks samples wg, wg + grid, ...)
constexpr int GN_REDUCE_ROWS = 128;    // slab rows per workgroup of the first channel-sum reduction

struct GnDims {
  int N, H, W, C, G, cpg, HW;
  int CV, CT, PP, nthr;     // channel units, units per workgroup row, pixel rows per workgroup, threads
  int rows, T;              // tile height in image rows, tiles per sample (split regime)
};

struct GnFwdArgs {
  const float *x, *gamma, *beta, *res;
  float *y, *mean, *rstd;
  double* ws;
  GnDims d;
  float eps;
  int relu, res_mode;
};

struct GnBwdArgs {
  const float *dy, *x, *mean, *rstd, *gamma, *beta;
  float *dx, *gstat;
  double *slab, *persample;
  GnDims d;
  int relu;
};

__host__ __device__ inline size_t gn_align16(size_t b) { return (b + 15) & ~(size_t)15; }

template <int VEC>
__device__ __forceinline__ void ldv(const float* p, float (&v)[VEC]) {
  if constexpr (VEC == 4) {
    const float4 q = *reinterpret_cast<const float4*>(p);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else {
    v[0] = *p;
  }
}

template <int VEC>
__device__ __forceinline__ void stv(float* p, const float (&v)[VEC]) {
  if constexpr (VEC == 4) {
    *reinterpret_cast<float4*>(p) = float4{v[0], v[1], v[2], v[3]};
  } else {
    *p = v[0];
  }
}

template <int VEC>
__device__ __forceinline__ double lanesum(const double (&a)[VEC]) {
  if constexpr (VEC == 4) return (a[0] + a[1]) + (a[2] + a[3]);
  else return a[0];
}

// the one expression of the normalised value: forward output and the backward's ReLU mask
__device__ __forceinline__ float gn_affine(float x, float mean, float rstd, float gam, float bet) {
  return ((x - mean) * rstd) * gam + bet;
}

// Per group: s1 = sum (x - K), s2 = sum (x - K)^2 over pixels [p0, p1) of the sample at `src`, K = src[p0][first channel of the
// group].  gsum [G][2].  red: 2 doubles per thread.
template <int VEC>
__device__ void gn_group_sums(const float* src, int p0, int p1, const GnDims& d, double* red, double* gsum) {
  const int t = threadIdx.x, py = t / d.CT, ct = t - py * d.CT;
  const int cu = d.cpg / VEC;
  for (int g = t; g < d.G; g += d.nthr) { gsum[2 * g] = 0.0; gsum[2 * g + 1] = 0.0; }
  for (int c0 = 0; c0 < d.CV; c0 += d.CT) {
    const int cv = c0 + ct;
    double s1[VEC] = {}, s2[VEC] = {};
    if (cv < d.CV) {
      const int c = cv * VEC, g = c / d.cpg;
      const double K = (double)src[(size_t)p0 * d.C + g * d.cpg];
      for (int p = p0 + py; p < p1; p += d.PP) {
        float v[VEC];
        ldv<VEC>(src + (size_t)p * d.C + c, v);
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
          const double dl = (double)v[j] - K;
          s1[j] += dl;
          s2[j] += dl * dl;
        }
      }
    }
    __syncthreads();
    red[2 * t] = lanesum<VEC>(s1);
    red[2 * t + 1] = lanesum<VEC>(s2);
    __syncthreads();
    const int cend = min(c0 + d.CT, d.CV);
    const int gfirst = c0 / cu, glast = (cend - 1) / cu;
    for (int g = gfirst + t; g <= glast; g += d.nthr) {
      const int u0 = max(g * cu, c0) - c0, u1 = min((g + 1) * cu, cend) - c0;
      double a = 0.0, b = 0.0;
      for (int q = 0; q < d.PP; ++q)
        for (int u = u0; u < u1; ++u) {
          a += red[2 * (q * d.CT + u)];
          b += red[2 * (q * d.CT + u) + 1];
        }
      gsum[2 * g] += a;
      gsum[2 * g + 1] += b;
    }
  }
  __syncthreads();
}

__device__ __forceinline__ void chan(double& na, double& ma, double& Ma, double nb, double mb, double Mb) {
  if (nb == 0.0) return;
  if (na == 0.0) { na = nb; ma = mb; Ma = Mb; return; }
  const double n = na + nb, dl = mb - ma;
  ma = ma + dl * (nb / n);
  Ma = (Ma + Mb) + (dl * dl) * (na * (nb / n));
  na = n;
}

// y over pixels [p0, p1) of sample n.  src: the sample's x (HBM or its LDS copy).  stat [G][2] = mean, rstd.
template <int VEC>
__device__ void gn_apply(const float* src, int n, int p0, int p1, const float* stat, const GnFwdArgs& a) {
  const GnDims& d = a.d;
  const int t = threadIdx.x, py = t / d.CT, ct = t - py * d.CT;
  const size_t base = (size_t)n * d.HW;
  const int Hc = (d.H + 1) >> 1, Wc = (d.W + 1) >> 1;
  for (int c0 = 0; c0 < d.CV; c0 += d.CT) {
    const int cv = c0 + ct;
    if (cv >= d.CV) continue;
    const int c = cv * VEC, g = c / d.cpg;
    const float m = stat[2 * g], r = stat[2 * g + 1];
    float gam[VEC], bet[VEC];
    ldv<VEC>(a.gamma + c, gam);
    ldv<VEC>(a.beta + c, bet);
    for (int p = p0 + py; p < p1; p += d.PP) {
      float v[VEC], o[VEC];
      ldv<VEC>(src + (size_t)p * d.C + c, v);
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        o[j] = gn_affine(v[j], m, r, gam[j], bet[j]);
        if (a.relu) o[j] = o[j] > 0.f ? o[j] : 0.f;
      }
      if (a.res_mode) {
        size_t ro = base + p;
        if (a.res_mode == 2) {
          const int h = p / d.W, w = p - h * d.W;
          ro = ((size_t)n * Hc + (h >> 1)) * Wc + (w >> 1);
        }
        float rv[VEC];
        ldv<VEC>(a.res + ro * d.C + c, rv);
#pragma unroll
        for (int j = 0; j < VEC; ++j) o[j] += rv[j];
      }
      stv<VEC>(a.y + (base + p) * d.C + c, o);
    }
  }
}

// ---------------------------------------------------------------------------------------------- forward, whole samples
__device__ __forceinline__ void gn_finish(double mean, double M2, double cnt, float eps, float& mean_f, float& rstd_f) {
  const double var = M2 > 0.0 ? M2 / cnt : 0.0;
  mean_f = (float)mean;
  rstd_f = (float)(1.0 / sqrt(var + (double)eps));
}

// LDS (bytes): red double[2*GN_THREADS] | gsum double[2G] | stat float[2G] | (16-byte aligned, CACHED) x float[HW*C]
__host__ __device__ inline size_t gn_fwd_small_head_bytes(int G) {
  return (size_t)2 * GN_THREADS * 8 + (size_t)2 * G * 8 + (size_t)2 * G * 4;
}

template <int VEC, bool CACHED>
__global__ __launch_bounds__(GN_THREADS) void gn_fwd_small_kernel(GnFwdArgs a) {
  extern __shared__ __align__(16) unsigned char gn_smem[];
  const GnDims& d = a.d;
  double* red = reinterpret_cast<double*>(gn_smem);
  double* gsum = red + 2 * GN_THREADS;
  float* stat = reinterpret_cast<float*>(gsum + 2 * d.G);
  float* xl = reinterpret_cast<float*>(gn_smem + gn_align16(gn_fwd_small_head_bytes(d.G)));
  const int t = threadIdx.x;
  for (int n = blockIdx.x; n < d.N; n += gridDim.x) {
    const float* xs = a.x + (size_t)n * d.HW * d.C;
    const float* src = xs;
    if constexpr (CACHED) {
      for (int u = t; u < d.HW * d.CV; u += d.nthr) {
        float v[VEC];
        ldv<VEC>(xs + (size_t)u * VEC, v);
        stv<VEC>(xl + (size_t)u * VEC, v);
      }
      __syncthreads();
      src = xl;
    }
    gn_group_sums<VEC>(src, 0, d.HW, d, red, gsum);
    const double cnt = (double)d.HW * (double)d.cpg;
    for (int g = t; g < d.G; g += d.nthr) {
      const double K = (double)src[g * d.cpg], s1 = gsum[2 * g], s2 = gsum[2 * g + 1];
      float mean, rstd;
      gn_finish(K + s1 / cnt, s2 - s1 * (s1 / cnt), cnt, a.eps, mean, rstd);
      stat[2 * g] = mean;
      stat[2 * g + 1] = rstd;
      a.mean[(size_t)n * d.G + g] = mean;
      a.rstd[(size_t)n * d.G + g] = rstd;
    }
    __syncthreads();
    gn_apply<VEC>(src, n, 0, d.HW, stat, a);
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------- forward, row tiles
// grid (T, N).  ws double [N][T][G][2] = the tile's mean and M2 (its count follows from the tile's rows).
// LDS: red double[2*GN_THREADS] | gsum double[2G]
template <int VEC>
__global__ __launch_bounds__(GN_THREADS) void gn_fwd_stats_kernel(GnFwdArgs a) {
  extern __shared__ __align__(16) unsigned char gn_smem[];
  const GnDims& d = a.d;
  double* red = reinterpret_cast<double*>(gn_smem);
  double* gsum = red + 2 * GN_THREADS;
  const int tile = blockIdx.x, n = blockIdx.y;
  const int p0 = tile * d.rows * d.W, p1 = min(d.H, (tile + 1) * d.rows) * d.W;
  const float* xs = a.x + (size_t)n * d.HW * d.C;
  gn_group_sums<VEC>(xs, p0, p1, d, red, gsum);
  const double cnt = (double)(p1 - p0) * (double)d.cpg;
  double* out = a.ws + ((size_t)n * d.T + tile) * d.G * 2;
  for (int g = threadIdx.x; g < d.G; g += d.nthr) {
    const double K = (double)xs[(size_t)p0 * d.C + g * d.cpg], s1 = gsum[2 * g], s2 = gsum[2 * g + 1];
    const double M2 = s2 - s1 * (s1 / cnt);
    out[2 * g] = K + s1 / cnt;
    out[2 * g + 1] = M2 > 0.0 ? M2 : 0.0;
  }
}

// grid (T, N).  Prologue: the sample's tile partials combined in a fixed order (every workgroup of the sample computes the same
// values; tile 0 writes them out).  LDS: scratch double[3 * (GN_THREADS + G)] | stat float[2G]
template <int VEC>
__global__ __launch_bounds__(GN_THREADS) void gn_fwd_apply_kernel(GnFwdArgs a) {
  extern __shared__ __align__(16) unsigned char gn_smem[];
  const GnDims& d = a.d;
  double* scratch = reinterpret_cast<double*>(gn_smem);
  float* stat = reinterpret_cast<float*>(scratch + 3 * (GN_THREADS + d.G));
  const int t = threadIdx.x, tile = blockIdx.x, n = blockIdx.y;
  const double* part = a.ws + (size_t)n * d.T * d.G * 2;
  const int L = d.nthr >= d.G ? d.nthr / d.G : 1;
  for (int item = t; item < d.G * L; item += d.nthr) {
    const int g = item % d.G, l = item / d.G;
    double cn = 0.0, cm = 0.0, cM = 0.0;
    for (int q = l; q < d.T; q += L) {
      const double nb = (double)((min(d.H, (q + 1) * d.rows) - q * d.rows) * d.W) * (double)d.cpg;
      chan(cn, cm, cM, nb, part[((size_t)q * d.G + g) * 2], part[((size_t)q * d.G + g) * 2 + 1]);
    }
    scratch[3 * item] = cn; scratch[3 * item + 1] = cm; scratch[3 * item + 2] = cM;
  }
  __syncthreads();
  for (int g = t; g < d.G; g += d.nthr) {
    double cn = 0.0, cm = 0.0, cM = 0.0;
    for (int l = 0; l < L; ++l) chan(cn, cm, cM, scratch[3 * (l * d.G + g)], scratch[3 * (l * d.G + g) + 1], scratch[3 * (l * d.G + g) + 2]);
    float mean, rstd;
    gn_finish(cm, cM, cn, a.eps, mean, rstd);
    stat[2 * g] = mean;
    stat[2 * g + 1] = rstd;
    if (tile == 0) {
      a.mean[(size_t)n * d.G + g] = mean;
      a.rstd[(size_t)n * d.G + g] = rstd;
    }
  }
  __syncthreads();
  const int p0 = tile * d.rows * d.W, p1 = min(d.H, (tile + 1) * d.rows) * d.W;
  gn_apply<VEC>(a.x + (size_t)n * d.HW * d.C, n, p0, p1, stat, a);
}

// ---------------------------------------------------------------------------------------------- backward
// Channel sums over pixels [p0, p1) of sample n: dst[c] = sum g * xhat, dst[C + c] = sum g (dst: LDS floats, or a slab row of doubles).
// gl (CACHED): the masked gradient is kept in LDS for the dx pass.  red: 2 * VEC floats per thread.
template <int VEC, bool CACHED, typename D>
__device__ void gn_bwd_sums(const GnBwdArgs& a, int n, int p0, int p1, float* red, D* dst, float* gl) {
  const GnDims& d = a.d;
  const int t = threadIdx.x, py = t / d.CT, ct = t - py * d.CT;
  const size_t base = (size_t)n * d.HW;
  for (int c0 = 0; c0 < d.CV; c0 += d.CT) {
    const int cv = c0 + ct, c = cv * VEC;
    double sg[VEC] = {}, sgx[VEC] = {};
    if (cv < d.CV) {
      const int g = c / d.cpg;
      const float m = a.mean[(size_t)n * d.G + g], r = a.rstd[(size_t)n * d.G + g];
      float gam[VEC], bet[VEC];
      ldv<VEC>(a.gamma + c, gam);
      ldv<VEC>(a.beta + c, bet);
      for (int p = p0 + py; p < p1; p += d.PP) {
        float xv[VEC], gv[VEC];
        ldv<VEC>(a.x + (base + p) * d.C + c, xv);
        ldv<VEC>(a.dy + (base + p) * d.C + c, gv);
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
          if (a.relu && !(gn_affine(xv[j], m, r, gam[j], bet[j]) > 0.f)) gv[j] = 0.f;
          sg[j] += (double)gv[j];
          sgx[j] += (double)gv[j] * (double)((xv[j] - m) * r);
        }
        if constexpr (CACHED) stv<VEC>(gl + (size_t)p * d.C + c, gv);
      }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      red[t * 2 * VEC + j] = (float)sgx[j];
      red[t * 2 * VEC + VEC + j] = (float)sg[j];
    }
    __syncthreads();
    if (py == 0 && cv < d.CV) {
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        double sa = 0.0, sb = 0.0;
        for (int q = 0; q < d.PP; ++q) {
          sa += (double)red[(q * d.CT + ct) * 2 * VEC + j];
          sb += (double)red[(q * d.CT + ct) * 2 * VEC + VEC + j];
        }
        dst[c + j] = (D)sa;
        dst[d.C + c + j] = (D)sb;
      }
    }
  }
  __syncthreads();
}

// A = mean over the group of g*gamma*xhat, B = mean of g*gamma, from the sample's channel sums cs [2C]
template <typename D>
__device__ __forceinline__ void gn_group_ab(const D* cs, const float* gamma, int g, const GnDims& d, float& A, float& B) {
  double sa = 0.0, sb = 0.0;
  for (int c = g * d.cpg; c < (g + 1) * d.cpg; ++c) {
    sa += (double)gamma[c] * (double)cs[c];
    sb += (double)gamma[c] * (double)cs[d.C + c];
  }
  const double cnt = (double)d.HW * (double)d.cpg;
  A = (float)(sa / cnt);
  B = (float)(sb / cnt);
}

// dx over pixels [p0, p1) of sample n.  gstat [G][2] = A, B (LDS or HBM).
template <int VEC, bool CACHED>
__device__ void gn_bwd_dx(const GnBwdArgs& a, int n, int p0, int p1, const float* gstat, const float* gl) {
  const GnDims& d = a.d;
  const int t = threadIdx.x, py = t / d.CT, ct = t - py * d.CT;
  const size_t base = (size_t)n * d.HW;
  for (int c0 = 0; c0 < d.CV; c0 += d.CT) {
    const int cv = c0 + ct;
    if (cv >= d.CV) continue;
    const int c = cv * VEC, g = c / d.cpg;
    const float m = a.mean[(size_t)n * d.G + g], r = a.rstd[(size_t)n * d.G + g];
    const float A = gstat[2 * g], B = gstat[2 * g + 1];
    float gam[VEC], bet[VEC];
    ldv<VEC>(a.gamma + c, gam);
    ldv<VEC>(a.beta + c, bet);
    for (int p = p0 + py; p < p1; p += d.PP) {
      float xv[VEC], gv[VEC], o[VEC];
      ldv<VEC>(a.x + (base + p) * d.C + c, xv);
      if constexpr (CACHED) ldv<VEC>(gl + (size_t)p * d.C + c, gv);
      else ldv<VEC>(a.dy + (base + p) * d.C + c, gv);
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        if (!CACHED && a.relu && !(gn_affine(xv[j], m, r, gam[j], bet[j]) > 0.f)) gv[j] = 0.f;
        const float xh = (xv[j] - m) * r;
        o[j] = r * (gv[j] * gam[j] - (A * xh + B));
      }
      stv<VEC>(a.dx + (base + p) * d.C + c, o);
    }
  }
}

// whole samples.  slab double [gridDim.x][2C] = this workgroup's channel sums over its samples (added in sample order).
// LDS (bytes): tot double[2C] | red float[2*VEC*GN_THREADS] | cs float[2C] | gstat float[2G] | (16-byte aligned, CACHED) g float[HW*C]
__host__ __device__ inline size_t gn_bwd_small_head_bytes(int C, int G, int vec) {
  return (size_t)2 * C * 8 + (size_t)2 * vec * GN_THREADS * 4 + (size_t)2 * C * 4 + (size_t)2 * G * 4;
}

template <int VEC, bool CACHED>
__global__ __launch_bounds__(GN_THREADS) void gn_bwd_small_kernel(GnBwdArgs a) {
  extern __shared__ __align__(16) unsigned char gn_smem[];
  const GnDims& d = a.d;
  double* tot = reinterpret_cast<double*>(gn_smem);
  float* red = reinterpret_cast<float*>(tot + 2 * d.C);
  float* cs = red + 2 * VEC * GN_THREADS;
  float* gstat = cs + 2 * d.C;
  float* gl = reinterpret_cast<float*>(gn_smem + gn_align16(gn_bwd_small_head_bytes(d.C, d.G, VEC)));
  const int t = threadIdx.x;
  for (int i = t; i < 2 * d.C; i += d.nthr) tot[i] = 0.0;
  for (int n = blockIdx.x; n < d.N; n += gridDim.x) {
    gn_bwd_sums<VEC, CACHED, float>(a, n, 0, d.HW, red, cs, gl);
    for (int i = t; i < 2 * d.C; i += d.nthr) tot[i] += (double)cs[i];
    for (int g = t; g < d.G; g += d.nthr) gn_group_ab<float>(cs, a.gamma, g, d, gstat[2 * g], gstat[2 * g + 1]);
    __syncthreads();
    gn_bwd_dx<VEC, CACHED>(a, n, 0, d.HW, gstat, gl);
    __syncthreads();
  }
  for (int i = t; i < 2 * d.C; i += d.nthr) a.slab[(size_t)blockIdx.x * 2 * d.C + i] = tot[i];
}

// row tiles, grid (T, N): slab double [N][T][2C].  LDS: red float[2*VEC*GN_THREADS]
template <int VEC>
__global__ __launch_bounds__(GN_THREADS) void gn_bwd_tile_sums_kernel(GnBwdArgs a) {
  extern __shared__ __align__(16) unsigned char gn_smem[];
  const GnDims& d = a.d;
  const int tile = blockIdx.x, n = blockIdx.y;
  const int p0 = tile * d.rows * d.W, p1 = min(d.H, (tile + 1) * d.rows) * d.W;
  gn_bwd_sums<VEC, false, double>(a, n, p0, p1, reinterpret_cast<float*>(gn_smem), a.slab + ((size_t)n * d.T + tile) * 2 * d.C,
                                  nullptr);
}

// grid (N): the sample's tile sums added in tile order -> persample double [N][2C], gstat [N][G][2].  LDS: cs double[2C]
__global__ __launch_bounds__(GN_THREADS) void gn_bwd_sample_kernel(GnBwdArgs a) {
  extern __shared__ __align__(16) unsigned char gn_smem[];
  double* cs = reinterpret_cast<double*>(gn_smem);
  const GnDims& d = a.d;
  const int n = blockIdx.x, t = threadIdx.x;
  const double* rows = a.slab + (size_t)n * d.T * 2 * d.C;
  for (int i = t; i < 2 * d.C; i += GN_THREADS) {
    double s = 0.0;
    for (int q = 0; q < d.T; ++q) s += rows[(size_t)q * 2 * d.C + i];
    cs[i] = s;
    a.persample[(size_t)n * 2 * d.C + i] = s;
  }
  __syncthreads();
  for (int g = t; g < d.G; g += GN_THREADS) {
    float A, B;
    gn_group_ab<double>(cs, a.gamma, g, d, A, B);
    a.gstat[((size_t)n * d.G + g) * 2] = A;
    a.gstat[((size_t)n * d.G + g) * 2 + 1] = B;
  }
}

template <int VEC>
__global__ __launch_bounds__(GN_THREADS) void gn_bwd_tile_dx_kernel(GnBwdArgs a) {
  const GnDims& d = a.d;
  const int tile = blockIdx.x, n = blockIdx.y;
  const int p0 = tile * d.rows * d.W, p1 = min(d.H, (tile + 1) * d.rows) * d.W;
  gn_bwd_dx<VEC, false>(a, n, p0, p1, a.gstat + (size_t)n * d.G * 2, nullptr);
}

// out row (blockIdx.y) = sum of rows [blockIdx.y * rpw, +rpw) of in [R][C2], four row phases added as (p0 + p1) + (p2 + p3);
// columns < half go to out0, the rest to out1 (row pitch ldo in both).  O: double (an intermediate slab) or float (dgamma / dbeta).
template <typename O>
__global__ __launch_bounds__(256) void gn_reduce_rows_kernel(const double* __restrict__ in, int R, int C2, int rpw, O* out0, O* out1,
                                                             int half, int ldo) {
  __shared__ double part[4][64];
  const int col = blockIdx.x * 64 + (threadIdx.x & 63), ph = threadIdx.x >> 6;
  const int r0 = blockIdx.y * rpw, r1 = min(R, r0 + rpw);
  double s = 0.0;
  if (col < C2)
    for (int r = r0 + ph; r < r1; r += 4) s += in[(size_t)r * C2 + col];
  part[ph][threadIdx.x & 63] = s;
  __syncthreads();
  if (ph == 0 && col < C2) {
    const int l = threadIdx.x;
    const double v = (part[0][l] + part[1][l]) + (part[2][l] + part[3][l]);
    if (col < half) out0[(size_t)blockIdx.y * ldo + col] = (O)v;
    else out1[(size_t)blockIdx.y * ldo + col - half] = (O)v;
  }
}

// Gradient of the coarser map of a res_mode-2 add at any fine size: out[n,i,j,c] = sum of g[n,2i..2i+1,2j..2j+1,c] inside the map
// (an odd H / W: the last coarse row / column was added to one fine row / column only).  One thread per output element.
__global__ __launch_bounds__(256) void gn_upsample2_grad_kernel(const float* __restrict__ g, float* __restrict__ out, int H, int W,
                                                                int C, long long total) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int Hc = (H + 1) >> 1, Wc = (W + 1) >> 1;
  const int c = (int)(i % C);
  long long q = i / C;
  const int jx = (int)(q % Wc); q /= Wc;
  const int jy = (int)(q % Hc);
  const long long n = q / Hc;
  const int h0 = 2 * jy, w0 = 2 * jx;
  const float* p = g + ((n * H + h0) * W + w0) * C + c;
  const bool right = w0 + 1 < W, below = h0 + 1 < H;
  float top = p[0], bot = 0.f;
  if (right) top += p[C];
  if (below) {
    bot = p[(long long)W * C];
    if (right) bot += p[(long long)W * C + C];
  }
  out[i] = top + bot;
}

// ---------------------------------------------------------------------------------------------- host
void gn_dims(GnDims& d, int N, int H, int W, int C, int G, int tile_rows, int vec) {
  d.N = N; d.H = H; d.W = W; d.C = C; d.G = G; d.cpg = C / G; d.HW = H * W;
  d.CV = C / vec;
  d.CT = d.CV < GN_THREADS ? d.CV : GN_THREADS;
  d.PP = GN_THREADS / d.CT;
  d.nthr = d.CT * d.PP;
  d.rows = tile_rows;
  d.T = tile_rows > 0 ? lvc_cdiv(H, tile_rows) : 1;
}

inline bool aligned16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

// bytes of the backward's workspace regions, in their order (the doubles first)
struct GnBwdWs { long long slab, persample, stage, gstat; };
GnBwdWs gn_bwd_ws(int N, int C, int G, int T, int split) {
  GnBwdWs w;
  const long long rows = split ? (long long)N * T : (N < GN_SMALL_GRID ? N : GN_SMALL_GRID);
  const long long final_rows = split ? N : rows;
  w.slab = rows * 2 * C * 8;
  w.persample = split ? (long long)N * 2 * C * 8 : 0;
  w.stage = lvc_cdiv64(final_rows, GN_REDUCE_ROWS) * 2 * C * 8;
  w.gstat = split ? (long long)N * 2 * G * 4 : 0;
  return w;
}

int gn_check_common(const char* fn, int N, int H, int W, int C, int G, int tile_rows) {
  if (!(N > 0 && H > 0 && W > 0 && C > 0 && G > 0)) { lvc_set_error("%s: non-positive dimension", fn); return LVC_ERR_INVALID; }
  if (C % G != 0) { lvc_set_error("%s: C (%d) must be divisible by the number of groups (%d)", fn, C, G); return LVC_ERR_INVALID; }
  if (tile_rows < 0) { lvc_set_error("%s: tile_rows must be >= 0", fn); return LVC_ERR_INVALID; }
  if ((long long)H * W * C >= (1ll << 31)) { lvc_set_error("%s: a sample must stay below 2^31 elements", fn); return LVC_ERR_INVALID; }
  if (tile_rows > 0 && lvc_cdiv(H, tile_rows) > 65535) { lvc_set_error("%s: more than 65535 row tiles", fn); return LVC_ERR_INVALID; }
  if (tile_rows > 0 && N > 65535) { lvc_set_error("%s: the row-tile regime takes at most 65535 samples", fn); return LVC_ERR_INVALID; }
  return LVC_OK;
}

}  // namespace

extern "C" long long lvc_group_norm_workspace_bytes(int N, int H, int W, int C, int G, int tile_rows, int backward) {
  if (N <= 0 || H <= 0 || W <= 0 || C <= 0 || G <= 0 || tile_rows < 0) return 0;
  const int T = tile_rows > 0 ? lvc_cdiv(H, tile_rows) : 1;
  long long bytes;
  if (!backward) {
    bytes = tile_rows > 0 ? (long long)N * T * G * 2 * 8 : 0;
  } else {
    const GnBwdWs w = gn_bwd_ws(N, C, G, T, tile_rows > 0);
    bytes = w.slab + w.persample + w.stage + w.gstat;
  }
  return bytes ? bytes + 16 : 0;
}

extern "C" int lvc_group_norm_fwd_nhwc(const float* x, const float* gamma, const float* beta, const float* residual, float* y,
                                       float* mean, float* rstd, int N, int H, int W, int C, int G, long long x_sn,
                                       long long x_sh, long long x_sw, long long x_sc, float eps, int relu, int res_mode,
                                       int tile_rows, void* workspace, long long workspace_bytes, void* stream) {
  LVC_CHECK_ARG(x && gamma && beta && y && mean && rstd, "null pointer");
  if (int rc = gn_check_common(__func__, N, H, W, C, G, tile_rows)) return rc;
  LVC_CHECK_ARG(x_sc == 1 && x_sw == C && x_sh == (long long)W * C && x_sn == (long long)H * W * C, "x must be contiguous NHWC");
  LVC_CHECK_ARG(eps > 0.f, "eps must be positive");
  LVC_CHECK_ARG(relu == 0 || relu == 1, "relu must be 0 or 1");
  LVC_CHECK_ARG(res_mode >= 0 && res_mode <= 2, "res_mode must be 0..2");
  LVC_CHECK_ARG(res_mode == 0 || residual, "residual pointer missing");
  LVC_CHECK_ARG(!(relu && res_mode), "ReLU together with a residual is not implemented (no caller has it)");
  LVC_CHECK_ARG(workspace_bytes >= lvc_group_norm_workspace_bytes(N, H, W, C, G, tile_rows, 0) && (tile_rows == 0 || workspace),
                "workspace too small (lvc_group_norm_workspace_bytes)");
  const bool vec4 = (C / G) % 4 == 0 && aligned16(x) && aligned16(y) && aligned16(gamma) && aligned16(beta) &&
                    (!res_mode || aligned16(residual));
  GnFwdArgs a;
  a.x = x; a.gamma = gamma; a.beta = beta; a.res = residual; a.y = y; a.mean = mean; a.rstd = rstd;
  a.ws = reinterpret_cast<double*>(((uintptr_t)workspace + 15) & ~(uintptr_t)15);
  a.eps = eps; a.relu = relu; a.res_mode = res_mode;
  gn_dims(a.d, N, H, W, C, G, tile_rows, vec4 ? 4 : 1);
  const GnDims& d = a.d;
  hipStream_t st = (hipStream_t)stream;
  if (tile_rows == 0) {
    const size_t head = gn_align16(gn_fwd_small_head_bytes(G));
    LVC_CHECK_ARG(head <= (size_t)GN_LDS_BYTES, "too many groups");
    const bool cached = head + (size_t)d.HW * C * 4 <= (size_t)GN_LDS_BYTES;
    const size_t lds = head + (cached ? (size_t)d.HW * C * 4 : 0);
    const dim3 grid((unsigned)(N < GN_SMALL_GRID ? N : GN_SMALL_GRID)), block((unsigned)d.nthr);
    if (vec4 && cached) hipLaunchKernelGGL((gn_fwd_small_kernel<4, true>), grid, block, lds, st, a);
    else if (vec4) hipLaunchKernelGGL((gn_fwd_small_kernel<4, false>), grid, block, lds, st, a);
    else if (cached) hipLaunchKernelGGL((gn_fwd_small_kernel<1, true>), grid, block, lds, st, a);
    else hipLaunchKernelGGL((gn_fwd_small_kernel<1, false>), grid, block, lds, st, a);
    LVC_CHECK_LAUNCH();
    return LVC_OK;
  }
  const size_t lds_stats = (size_t)(2 * GN_THREADS + 2 * G) * 8;
  const size_t lds_apply = (size_t)3 * (GN_THREADS + G) * 8 + (size_t)2 * G * 4;
  LVC_CHECK_ARG(lds_stats <= (size_t)GN_LDS_BYTES && lds_apply <= (size_t)GN_LDS_BYTES, "too many groups");
  const dim3 grid((unsigned)d.T, (unsigned)N), block((unsigned)d.nthr);
  if (vec4) hipLaunchKernelGGL((gn_fwd_stats_kernel<4>), grid, block, lds_stats, st, a);
  else hipLaunchKernelGGL((gn_fwd_stats_kernel<1>), grid, block, lds_stats, st, a);
  LVC_CHECK_LAUNCH();
  if (vec4) hipLaunchKernelGGL((gn_fwd_apply_kernel<4>), grid, block, lds_apply, st, a);
  else hipLaunchKernelGGL((gn_fwd_apply_kernel<1>), grid, block, lds_apply, st, a);
  LVC_CHECK_LAUNCH();
  return LVC_OK;
}

extern "C" int lvc_group_norm_bwd_nhwc(const float* dy, const float* x, const float* mean, const float* rstd, const float* gamma,
                                       const float* beta, float* dx, float* dgamma, float* dbeta, int N, int H, int W, int C,
                                       int G, long long x_sn, long long x_sh, long long x_sw, long long x_sc, int relu,
                                       int tile_rows, void* workspace, long long workspace_bytes, void* stream) {
  LVC_CHECK_ARG(dy && x && mean && rstd && gamma && dx && dgamma && dbeta && workspace, "null pointer");
  LVC_CHECK_ARG(relu == 0 || relu == 1, "relu must be 0 or 1");
  LVC_CHECK_ARG(!relu || beta, "the ReLU mask needs beta");
  if (int rc = gn_check_common(__func__, N, H, W, C, G, tile_rows)) return rc;
  LVC_CHECK_ARG(x_sc == 1 && x_sw == C && x_sh == (long long)W * C && x_sn == (long long)H * W * C,
                "x and dy must be contiguous NHWC");
  LVC_CHECK_ARG(workspace_bytes >= lvc_group_norm_workspace_bytes(N, H, W, C, G, tile_rows, 1),
                "workspace too small (lvc_group_norm_workspace_bytes)");
  if (!beta) beta = gamma;     // never read for a value without the mask; keeps the vector loads on valid memory
  const bool vec4 = (C / G) % 4 == 0 && aligned16(x) && aligned16(dy) && aligned16(dx) && aligned16(gamma) && aligned16(beta);
  const int split = tile_rows > 0;
  GnBwdArgs a;
  a.dy = dy; a.x = x; a.mean = mean; a.rstd = rstd; a.gamma = gamma; a.beta = beta; a.dx = dx; a.relu = relu;
  gn_dims(a.d, N, H, W, C, G, tile_rows, vec4 ? 4 : 1);
  const GnDims& d = a.d;
  const GnBwdWs w = gn_bwd_ws(N, C, G, d.T, split);
  unsigned char* base = reinterpret_cast<unsigned char*>(((uintptr_t)workspace + 15) & ~(uintptr_t)15);
  a.slab = reinterpret_cast<double*>(base);
  a.persample = reinterpret_cast<double*>(base + w.slab);
  double* stage = reinterpret_cast<double*>(base + w.slab + w.persample);
  a.gstat = reinterpret_cast<float*>(base + w.slab + w.persample + w.stage);
  hipStream_t st = (hipStream_t)stream;
  const int vec = vec4 ? 4 : 1;
  const double* rows_in;
  int R;
  if (!split) {
    const size_t head = gn_align16(gn_bwd_small_head_bytes(C, G, vec));
    LVC_CHECK_ARG(head <= (size_t)GN_LDS_BYTES, "too many channels for the whole-sample regime");
    const bool cached = head + (size_t)d.HW * C * 4 <= (size_t)GN_LDS_BYTES;
    const size_t lds = head + (cached ? (size_t)d.HW * C * 4 : 0);
    R = N < GN_SMALL_GRID ? N : GN_SMALL_GRID;
    const dim3 grid((unsigned)R), block((unsigned)d.nthr);
    if (vec4 && cached) hipLaunchKernelGGL((gn_bwd_small_kernel<4, true>), grid, block, lds, st, a);
    else if (vec4) hipLaunchKernelGGL((gn_bwd_small_kernel<4, false>), grid, block, lds, st, a);
    else if (cached) hipLaunchKernelGGL((gn_bwd_small_kernel<1, true>), grid, block, lds, st, a);
    else hipLaunchKernelGGL((gn_bwd_small_kernel<1, false>), grid, block, lds, st, a);
    LVC_CHECK_LAUNCH();
    rows_in = a.slab;
  } else {
    LVC_CHECK_ARG((size_t)C * 16 <= (size_t)GN_LDS_BYTES, "too many channels");
    const dim3 grid((unsigned)d.T, (unsigned)N), block((unsigned)d.nthr);
    const size_t lds = (size_t)2 * vec * GN_THREADS * 4;
    if (vec4) hipLaunchKernelGGL((gn_bwd_tile_sums_kernel<4>), grid, block, lds, st, a);
    else hipLaunchKernelGGL((gn_bwd_tile_sums_kernel<1>), grid, block, lds, st, a);
    LVC_CHECK_LAUNCH();
    hipLaunchKernelGGL(gn_bwd_sample_kernel, dim3((unsigned)N), dim3(GN_THREADS), (size_t)C * 16, st, a);
    LVC_CHECK_LAUNCH();
    if (vec4) hipLaunchKernelGGL((gn_bwd_tile_dx_kernel<4>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((gn_bwd_tile_dx_kernel<1>), grid, block, 0, st, a);
    LVC_CHECK_LAUNCH();
    rows_in = a.persample;
    R = N;
  }
  // dgamma / dbeta: the slab rows added in row order, in one launch up to GN_REDUCE_ROWS rows and in two above
  const int C2 = 2 * C;
  const unsigned gx = (unsigned)lvc_cdiv(C2, 64);
  if (R > GN_REDUCE_ROWS) {
    const int R1 = lvc_cdiv(R, GN_REDUCE_ROWS);
    hipLaunchKernelGGL((gn_reduce_rows_kernel<double>), dim3(gx, (unsigned)R1), dim3(256), 0, st, rows_in, R, C2, GN_REDUCE_ROWS,
                       stage, stage + C, C, C2);
    LVC_CHECK_LAUNCH();
    rows_in = stage;
    R = R1;
  }
  hipLaunchKernelGGL((gn_reduce_rows_kernel<float>), dim3(gx, 1), dim3(256), 0, st, rows_in, R, C2, R, dgamma, dbeta, C, 0);
  LVC_CHECK_LAUNCH();
  return LVC_OK;
}

extern "C" int lvc_upsample2_add_grad_nhwc(const float* g, float* dres, int N, int H, int W, int C, void* stream) {
  LVC_CHECK_ARG(g && dres && N > 0 && H > 0 && W > 0 && C > 0, "bad arguments");
  const long long total = (long long)N * ((H + 1) / 2) * ((W + 1) / 2) * C;
  LVC_CHECK_ARG(lvc_cdiv64(total, 256) < (1ll << 31), "tensor too large");
  hipLaunchKernelGGL(gn_upsample2_grad_kernel, dim3((unsigned)lvc_cdiv64(total, 256)), dim3(256), 0, (hipStream_t)stream, g, dres, H, W,
                     C, total);
  LVC_CHECK_LAUNCH();
  return LVC_OK;
}
