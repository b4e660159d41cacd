// mask_train.hip -- the mask branch's training loss and the backward of the head's fused tail (reference
// detectron2/modeling/roi_heads/mask_head.py mask_rcnn_loss: binary_cross_entropy_with_logits(mean) of the ground-truth class's logits
// against the cropped ground-truth masks, and autograd through predictor, ReLU and ConvTranspose2d).
//
// lvc_mask_loss: one streaming pass over the logits z [M, 2S, 2S] (lvc_mask_deconv_logits) and the target bytes of the real rows.
//   Each term max(z, 0) - z t + log1p(exp(-|z|)) is evaluated in fp64 (as retinanet_loss.hip); a workgroup owns a contiguous slice and
//   leaves one fp64 partial sum and three integer counts; ONE finishing workgroup adds the partials in index order.  No float atomics:
//   two runs give the same bits.  num_valid = 0 gives a loss of 0.
//
// lvc_mask_deconv_grad: dz = (sigmoid(z) - t) g / N is formed in the kernel (g: the upstream scalar ON THE DEVICE, N = num_valid (2S)^2).
//   The hidden map [M, Cmid, 2S, 2S] is not kept by the forward, so the kernel recomputes its tile with the forward's MFMA pass
//   (v_mfma_f32_16x16x4_f32 on fp32 operands: exact products, range-free) and, in registers,
//     dh = dz Wp[c, co] [h > 0]                    -> written as [M S^2, 4 Cmid], the operand of the two GEMMs that give dx and dWd
//     u[m, tile, co] = sum dz h,  v[m, tile] = sum dz,  w[m, tile, co] = sum dh      (fixed lane and tap order, per-(RoI, tile) partials)
//   A training tile holds rows of ONE RoI (grid M x ceil(S^2 / 64)): the partials of a RoI belong to one class, and a finishing launch
//   with workgroups per class adds the partials of its RoIs in a fixed order into dWp[k, :] and dbp[k] -- a class absent from the batch
//   gets exact zeros -- and a third small launch adds every w into dbd.  No all-class tensor, no float atomics on data.
//   Rows past num_valid are not read; their dh rows are written as zeros.
//
// lvc_mask_deconv_wgrad: dWd (packed [4 Cmid, Cin]) = dh^T x, the contraction over the M S^2 rows.  The project's conv_wgrad joins its
//   pixel slices with float atomics (order not deterministic), so this product has a kernel of its own: fp32 MFMA (exact products), the
//   rows cut into a number of slices fixed by M alone, a workgroup per (256 x 64 output tile, slice) that writes its partial tile, and a
//   second launch that adds the slices in index order.  Rows of x and dh past num_valid are not read: slices past it add exact zeros.
#include "conv_common.h"
#include "rows_common.h"

#define MG_TM 64            // rows (pixels of one RoI) per workgroup
#define MG_PAD 4            // floats of padding per LDS row
#define MG_STATUS_CLASS 8   // status bit: a class index outside [0, K)
#define ML_MAX_GROUPS 1024  // workgroups (partials) of the loss pass

// ------------------------------------------------------------------------------------------------- loss
__global__ __launch_bounds__(256) void mask_loss_kernel(const float* __restrict__ z, const unsigned char* __restrict__ t,
                                                        const int* __restrict__ d_num_valid, int M, long long P, long long chunk,
                                                        double* __restrict__ psum, long long* __restrict__ pcnt) {
  __shared__ double ssum[4];
  __shared__ long long scnt[4][3];
  const int Mv = lvc_valid_rows(d_num_valid, M);
  const long long total = (long long)Mv * P;
  const long long i0 = (long long)blockIdx.x * chunk;
  long long i1 = i0 + chunk;
  if (i1 > total) i1 = total;
  double s = 0.0;
  long long bad = 0, pos = 0, fp = 0;
  for (long long i = i0 + threadIdx.x; i < i1; i += 256) {
    const float zf = z[i];
    const bool tt = t[i] != 0;
    const double zd = (double)zf;
    s += (zd > 0.0 ? zd : 0.0) - (tt ? zd : 0.0) + log1p(exp(-fabs(zd)));
    const bool pred = zf > 0.f;
    bad += pred != tt;
    pos += tt;
    fp += pred && !tt;
  }
  for (int off = 32; off >= 1; off >>= 1) {
    s += __shfl_xor(s, off);
    bad += __shfl_xor(bad, off);
    pos += __shfl_xor(pos, off);
    fp += __shfl_xor(fp, off);
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    ssum[wave] = s;
    scnt[wave][0] = bad;
    scnt[wave][1] = pos;
    scnt[wave][2] = fp;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    psum[blockIdx.x] = (ssum[0] + ssum[1]) + (ssum[2] + ssum[3]);
    for (int k = 0; k < 3; ++k) pcnt[(size_t)blockIdx.x * 3 + k] = (scnt[0][k] + scnt[1][k]) + (scnt[2][k] + scnt[3][k]);
  }
}

__global__ __launch_bounds__(64) void mask_loss_finish_kernel(const double* __restrict__ psum, const long long* __restrict__ pcnt, int G,
                                                              const int* __restrict__ d_num_valid, int M, long long P,
                                                              float* __restrict__ out_loss, double* __restrict__ out_sum,
                                                              long long* __restrict__ out_counts) {
  if (threadIdx.x != 0) return;
  const int Mv = lvc_valid_rows(d_num_valid, M);
  double s = 0.0;
  long long c[3] = {0, 0, 0};
  for (int g = 0; g < G; ++g) {
    s += psum[g];
    for (int k = 0; k < 3; ++k) c[k] += pcnt[(size_t)g * 3 + k];
  }
  const double n = (double)Mv * (double)P;
  *out_loss = Mv > 0 ? (float)(s / n) : 0.f;
  if (out_sum) *out_sum = s;
  if (out_counts)
    for (int k = 0; k < 3; ++k) out_counts[k] = c[k];
}

static int mask_loss_groups(int M, int S) {
  const long long total = (long long)M * 4 * S * S;
  long long g = (total + 2047) / 2048;
  if (g < 1) g = 1;
  if (g > ML_MAX_GROUPS) g = ML_MAX_GROUPS;
  return (int)g;
}

extern "C" long long lvc_mask_loss_workspace_bytes(int M, int S) {
  if (M < 0 || S < 1) return -1;
  return (long long)mask_loss_groups(M, S) * 32;
}

extern "C" int lvc_mask_loss(const float* logits, const unsigned char* targets, const int* d_num_valid, int M, int S, float* out_loss,
                             double* out_sum, long long* out_counts, void* workspace, long long workspace_bytes, void* stream) {
  LVC_CHECK_ARG(M >= 0 && S >= 1 && S <= 4096, "M >= 0, 1 <= S <= 4096");
  LVC_CHECK_ARG(out_loss && workspace && (M == 0 || (logits && targets)), "null pointer");
  LVC_CHECK_ARG(workspace_bytes >= lvc_mask_loss_workspace_bytes(M, S) && ((uintptr_t)workspace & 7) == 0, "workspace too small or unaligned");
  const int G = mask_loss_groups(M, S);
  const long long P = 4LL * S * S, total = (long long)M * P;
  const long long chunk = (total + G - 1) / G;
  double* psum = reinterpret_cast<double*>(workspace);
  long long* pcnt = reinterpret_cast<long long*>(psum + G);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(mask_loss_kernel, dim3(G), dim3(256), 0, st, logits, targets, d_num_valid, M, P, chunk, psum, pcnt);
  hipLaunchKernelGGL(mask_loss_finish_kernel, dim3(1), dim3(64), 0, st, psum, pcnt, G, d_num_valid, M, P, out_loss, out_sum, out_counts);
  LVC_CHECK_LAUNCH();
  return LVC_OK;
}

// ------------------------------------------------------------------------------------------------- tail backward
template <int NBC>      // Cmid / 64
__global__ __launch_bounds__(256) void mask_deconv_grad_kernel(const float* __restrict__ x, const float* __restrict__ wd,
                                                               const float* __restrict__ bd, const float* __restrict__ wp,
                                                               const int* __restrict__ classes, const float* __restrict__ z,
                                                               const unsigned char* __restrict__ tg, const int* __restrict__ d_num_valid,
                                                               const float* __restrict__ d_g, int* __restrict__ d_status,
                                                               float* __restrict__ dh, float* __restrict__ pu,
                                                               float* __restrict__ pv, float* __restrict__ pw, int M, int S, int Cin, int K,
                                                               int tiles) {
  constexpr int Cmid = 64 * NBC;
  extern __shared__ __attribute__((aligned(16))) unsigned char mg_smem[];
  const int LDP = Cin + MG_PAD;
  float* sx = reinterpret_cast<float*>(mg_smem);      // [MG_TM][LDP]
  float* sdz = sx + MG_TM * LDP;                      // [4 taps][MG_TM]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = lane & 15, kq = lane >> 4;
  const int S2 = S * S;
  const int Mv = lvc_valid_rows(d_num_valid, M);
  const int m = blockIdx.x / tiles, tile = blockIdx.x - m * tiles;
  const int p0 = tile * MG_TM;
  const int rows = S2 - p0 < MG_TM ? S2 - p0 : MG_TM;
  const size_t r0 = (size_t)m * S2 + p0;
  const int c4n = Cin >> 2;
  if (m >= Mv) {      // (uniform) a row past num_valid: nothing is read, its rows of dh are zeros
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    for (int idx = tid; idx < rows * Cmid; idx += 256) *reinterpret_cast<f32x4*>(dh + r0 * 4 * Cmid + (size_t)idx * 4) = zero;
    return;
  }
  for (int idx = tid; idx < MG_TM * c4n; idx += 256) {
    const int p = idx / c4n, c4 = idx - p * c4n;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (p < rows) v = *reinterpret_cast<const f32x4*>(x + (r0 + p) * Cin + c4 * 4);
    *reinterpret_cast<f32x4*>(sx + p * LDP + c4 * 4) = v;
  }
  int c = 0;
  if (classes) {
    c = classes[m];
    if (c < 0 || c >= K) {
      if (d_status && tid == 0) atomicOr(d_status, MG_STATUS_CLASS);
      c = 0;
    }
  }
  {
    const int p = tid & 63, q = tid >> 6;
    float dz = 0.f;
    if (p < rows) {
      const int pix = p0 + p;
      const int yy = pix / S, xx = pix - yy * S;
      const int S_2 = 2 * S;
      const size_t i = ((size_t)m * S_2 + 2 * yy + (q >> 1)) * S_2 + 2 * xx + (q & 1);
      const float zf = z[i];
      const float t = tg[i] ? 1.f : 0.f;
      const float scale = *d_g / ((float)Mv * (float)(4 * S2));
      dz = (1.f / (1.f + expf(-zf)) - t) * scale;
    }
    sdz[q * MG_TM + p] = dz;
  }
  __syncthreads();
  if (wave == 0) {      // v: the four taps of a pixel, then the 64 pixels by halving -- always the same order
    float s = (sdz[lane] + sdz[MG_TM + lane]) + (sdz[2 * MG_TM + lane] + sdz[3 * MG_TM + lane]);
    for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off);
    if (lane == 0) pv[blockIdx.x] = s;
  }

  f32x4 uacc[NBC], wacc[NBC];
#pragma unroll
  for (int nb = 0; nb < NBC; ++nb) uacc[nb] = wacc[nb] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int kcn = Cin >> 4;
#pragma unroll 1
  for (int q = 0; q < 4; ++q) {
    f32x4 acc[4][NBC];
#pragma unroll
    for (int pb = 0; pb < 4; ++pb)
#pragma unroll
      for (int nb = 0; nb < NBC; ++nb) acc[pb][nb] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float* wrow = wd + (size_t)(q * Cmid + wave * NBC * 16 + j) * Cin + kq * 4;
    const float* brow = sx + j * LDP + kq * 4;
    for (int kc = 0; kc < kcn; ++kc) {
      f32x4 a[NBC], b[4];
#pragma unroll
      for (int nb = 0; nb < NBC; ++nb) a[nb] = *reinterpret_cast<const f32x4*>(wrow + (size_t)nb * 16 * Cin + kc * 16);
#pragma unroll
      for (int pb = 0; pb < 4; ++pb) b[pb] = *reinterpret_cast<const f32x4*>(brow + pb * 16 * LDP + kc * 16);
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int nb = 0; nb < NBC; ++nb)
#pragma unroll
          for (int pb = 0; pb < 4; ++pb) acc[pb][nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[nb][t], b[pb][t], acc[pb][nb], 0, 0, 0);
    }
    // the lane holds co = (wave NBC + nb) 16 + 4 kq + e of pixel pb 16 + j
#pragma unroll
    for (int pb = 0; pb < 4; ++pb) {
      const int p = pb * 16 + j;
      const float dz = sdz[q * MG_TM + p];      // 0 for the rows past the RoI's last pixel
#pragma unroll
      for (int nb = 0; nb < NBC; ++nb) {
        const int co = (wave * NBC + nb) * 16 + kq * 4;
        f32x4 b4 = {0.f, 0.f, 0.f, 0.f};
        if (bd) b4 = *reinterpret_cast<const f32x4*>(bd + co);
        const f32x4 w4 = *reinterpret_cast<const f32x4*>(wp + (size_t)c * Cmid + co);
        f32x4 g4;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float v = acc[pb][nb][e] + b4[e];
          const bool on = v > 0.f;
          g4[e] = on ? dz * w4[e] : 0.f;
          uacc[nb][e] = fmaf(dz, on ? v : 0.f, uacc[nb][e]);
          wacc[nb][e] += g4[e];
        }
        if (p < rows) *reinterpret_cast<f32x4*>(dh + ((r0 + p) * 4 + q) * Cmid + co) = g4;
      }
    }
  }
#pragma unroll
  for (int nb = 0; nb < NBC; ++nb) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float u = uacc[nb][e], w = wacc[nb][e];
      for (int off = 1; off <= 8; off <<= 1) {
        u += __shfl_xor(u, off);
        w += __shfl_xor(w, off);
      }
      uacc[nb][e] = u;
      wacc[nb][e] = w;
    }
    if (j == 0) {
      const int co = (wave * NBC + nb) * 16 + kq * 4;
      *reinterpret_cast<f32x4*>(pu + (size_t)blockIdx.x * Cmid + co) = uacc[nb];
      *reinterpret_cast<f32x4*>(pw + (size_t)blockIdx.x * Cmid + co) = wacc[nb];
    }
  }
}

// Workgroup (k, 64-channel slice): dWp[k, slice] and dbp[k] from the partials of the RoIs of class k.  Four phases of threads walk the RoIs
// m = phase, phase + 4, ... in index order (a single walk over 1024 RoIs is a chain of a thousand dependent load latencies), and the four
// phase sums are added in a fixed order: the same bits in every run; a class without RoIs gets exact zeros.
__global__ __launch_bounds__(256) void mask_deconv_grad_finish_kernel(const float* __restrict__ pu, const float* __restrict__ pv,
                                                                      const int* __restrict__ classes, const int* __restrict__ d_num_valid,
                                                                      int M, int tiles, int Cmid, int K, float* __restrict__ dwp,
                                                                      float* __restrict__ dbp) {
  __shared__ float sa[4][64];
  __shared__ float sb[4];
  const int Mv = lvc_valid_rows(d_num_valid, M);
  const int k = blockIdx.x, col = threadIdx.x & 63, ph = threadIdx.x >> 6;
  const int co = blockIdx.y * 64 + col;
  float a = 0.f, b = 0.f;
  for (int m = ph; m < Mv; m += 4) {
    int c = classes ? classes[m] : 0;
    if (c < 0 || c >= K) c = 0;
    if (c != k) continue;
    for (int t = 0; t < tiles; ++t) {
      const size_t i = (size_t)m * tiles + t;
      a += pu[i * Cmid + co];
      b += pv[i];
    }
  }
  sa[ph][col] = a;
  if (col == 0) sb[ph] = b;
  __syncthreads();
  if (ph == 0) {
    dwp[(size_t)k * Cmid + co] = (sa[0][col] + sa[1][col]) + (sa[2][col] + sa[3][col]);
    if (col == 0 && blockIdx.y == 0) dbp[k] = (sb[0] + sb[1]) + (sb[2] + sb[3]);
  }
}

// dbd: workgroup = 16 channels x 16 phases over all (RoI, tile) partials of dh's column sums, the phase sums added in a fixed order
__global__ __launch_bounds__(256) void mask_deconv_grad_dbd_kernel(const float* __restrict__ pw, const int* __restrict__ d_num_valid, int M,
                                                                   int tiles, int Cmid, float* __restrict__ dbd) {
  __shared__ float sa[16][16];
  const int Mv = lvc_valid_rows(d_num_valid, M);
  const int col = threadIdx.x & 15, ph = threadIdx.x >> 4;
  const int co = blockIdx.x * 16 + col;
  const long long parts = (long long)Mv * tiles;
  float a = 0.f;
#pragma unroll 4
  for (long long i = ph; i < parts; i += 16) a += pw[(size_t)i * Cmid + co];
  sa[ph][col] = a;
  __syncthreads();
  if (ph == 0) {
    float s = 0.f;
    for (int q = 0; q < 16; ++q) s += sa[q][col];
    dbd[co] = s;
  }
}

static long long mask_grad_tiles(int S) { return ((long long)S * S + MG_TM - 1) / MG_TM; }

extern "C" long long lvc_mask_deconv_grad_workspace_bytes(int M, int S, int Cmid) {
  if (M < 0 || S < 1 || Cmid < 1) return -1;
  const long long parts = (long long)M * mask_grad_tiles(S);
  return parts * (2LL * Cmid + 1) * 4 + 16;
}

template <int NBC>
static int launch_mask_deconv_grad(const float* x, const float* wd, const float* bd, const float* wp, const int* classes, const float* z,
                                   const unsigned char* tg, const int* d_num_valid, const float* d_g, int* d_status, float* dh,
                                   float* pu, float* pv, float* pw, int M, int S, int Cin, int K, int tiles, hipStream_t st) {
  const size_t lds = (size_t)MG_TM * (Cin + MG_PAD) * 4 + 4 * MG_TM * 4;
  static bool lds_set[64] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = -1;
  if (dev < 0 || !lds_set[dev]) {
    const size_t lds_max = (size_t)MG_TM * (256 + MG_PAD) * 4 + 4 * MG_TM * 4;
    if (hipFuncSetAttribute((const void*)mask_deconv_grad_kernel<NBC>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_max) != hipSuccess) {
      (void)hipGetLastError();
      lvc_set_error("lvc_mask_deconv_grad: %zu bytes of LDS refused", lds_max);
      return LVC_ERR_HIP;
    }
    if (dev >= 0) lds_set[dev] = true;
  }
  hipLaunchKernelGGL((mask_deconv_grad_kernel<NBC>), dim3((unsigned)(M * tiles)), dim3(256), lds, st, x, wd, bd, wp, classes, z, tg,
                     d_num_valid, d_g, d_status, dh, pu, pv, pw, M, S, Cin, K, tiles);
  return LVC_OK;
}

extern "C" int lvc_mask_deconv_grad(const float* x, const float* w_deconv, const float* b_deconv, const float* w_pred, const int* classes,
                                    const float* logits, const unsigned char* targets, const int* d_num_valid, const float* d_upstream,
                                    float* dh, float* dw_pred, float* db_pred, float* db_deconv, int M, int S, int Cin,
                                    int Cmid, int K, int* d_status, void* workspace, long long workspace_bytes, void* stream) {
  LVC_CHECK_ARG(M >= 0 && S >= 1 && K >= 1, "M >= 0, S >= 1, K >= 1");
  LVC_CHECK_ARG(Cin >= 64 && Cin <= 256 && Cin % 64 == 0 && Cmid >= 64 && Cmid <= 256 && Cmid % 64 == 0,
                "channels of the deconvolution: multiples of 64 up to 256 (MODEL.ROI_MASK_HEAD.CONV_DIM)");
  LVC_CHECK_ARG(dw_pred && db_pred && db_deconv && workspace, "null pointer");
  LVC_CHECK_ARG(M == 0 || (x && w_deconv && w_pred && logits && targets && d_upstream && dh), "null pointer");
  LVC_CHECK_ARG((((uintptr_t)x | (uintptr_t)w_deconv | (uintptr_t)w_pred | (uintptr_t)b_deconv | (uintptr_t)dh |
                  (uintptr_t)workspace) & 15) == 0, "16-byte aligned operands");
  const long long tiles = mask_grad_tiles(S);
  LVC_CHECK_ARG((long long)M * tiles < (1LL << 31) && (long long)M * S * S < (1LL << 31) - MG_TM, "too many rows");
  LVC_CHECK_ARG(workspace_bytes >= lvc_mask_deconv_grad_workspace_bytes(M, S, Cmid), "workspace too small");
  hipStream_t st = (hipStream_t)stream;
  const long long parts = (long long)M * tiles;
  float* pu = reinterpret_cast<float*>(workspace);
  float* pw = pu + parts * Cmid;
  float* pv = pw + parts * Cmid;
  if (M > 0) {
    int rc;
    switch (Cmid / 64) {
      case 1: rc = launch_mask_deconv_grad<1>(x, w_deconv, b_deconv, w_pred, classes, logits, targets, d_num_valid, d_upstream, d_status, dh, pu, pv, pw, M, S, Cin, K, (int)tiles, st); break;
      case 2: rc = launch_mask_deconv_grad<2>(x, w_deconv, b_deconv, w_pred, classes, logits, targets, d_num_valid, d_upstream, d_status, dh, pu, pv, pw, M, S, Cin, K, (int)tiles, st); break;
      case 3: rc = launch_mask_deconv_grad<3>(x, w_deconv, b_deconv, w_pred, classes, logits, targets, d_num_valid, d_upstream, d_status, dh, pu, pv, pw, M, S, Cin, K, (int)tiles, st); break;
      default: rc = launch_mask_deconv_grad<4>(x, w_deconv, b_deconv, w_pred, classes, logits, targets, d_num_valid, d_upstream, d_status, dh, pu, pv, pw, M, S, Cin, K, (int)tiles, st); break;
    }
    if (rc != LVC_OK) return rc;
  }
  hipLaunchKernelGGL(mask_deconv_grad_finish_kernel, dim3((unsigned)K, (unsigned)(Cmid / 64)), dim3(256), 0, st, pu, pv, classes, d_num_valid, M,
                     (int)tiles, Cmid, K, dw_pred, db_pred);
  hipLaunchKernelGGL(mask_deconv_grad_dbd_kernel, dim3((unsigned)(Cmid / 16)), dim3(256), 0, st, pw, d_num_valid, M, (int)tiles, Cmid, db_deconv);
  LVC_CHECK_LAUNCH();
  return LVC_OK;
}

// ------------------------------------------------------------------------------------------------- dWd = dh^T x
#define MW_TN 256           // output rows (columns of dh) per workgroup: 64 per wave
#define MW_TC 64            // output columns (columns of x) per workgroup
#define MW_KC 16            // rows of dh / x per LDS chunk
#define MW_LDA (MW_TN + 16) // LDS row strides: the four k rows a wave reads at once fall on different banks
#define MW_LDB (MW_TC + 16)
#define MW_SLICE_ROWS 2048  // rows per slice (a multiple of MW_KC) ...
#define MW_MAX_SLICES 64    // ... unless that would make more slices than this

static LvcSliceCut mask_wgrad_cut(int M, int S) { return lvc_slice_cut((long long)M * S * S, MW_SLICE_ROWS, MW_MAX_SLICES, MW_KC); }

__global__ __launch_bounds__(256) void mask_wgrad_kernel(const float* __restrict__ dh, const float* __restrict__ x,
                                                         const int* __restrict__ d_num_valid, float* __restrict__ part, int M, int S2,
                                                         int N4, int Cin, long long slice_rows) {
  __shared__ __attribute__((aligned(16))) float sA[MW_KC * MW_LDA];
  __shared__ __attribute__((aligned(16))) float sB[MW_KC * MW_LDB];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = lane & 15, kq = lane >> 4;
  const int Mv = lvc_valid_rows(d_num_valid, M);
  const long long R = (long long)Mv * S2;      // the rows past it are never read (x may hold anything there)
  const int nt = N4 / MW_TN;
  const int tn = blockIdx.x % nt, tc = blockIdx.x / nt;
  const int n0 = tn * MW_TN, c0 = tc * MW_TC;
  const long long rb = (long long)blockIdx.y * slice_rows;
  long long re = rb + slice_rows;
  if (re > R) re = R;

  f32x4 acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  f32x4 ga[4], gb;
  const int brow = tid >> 4, bc4 = tid & 15;
  auto fetch = [&](long long r) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int idx = tid + i * 256, row = idx >> 6, c4 = idx & 63;
      ga[i] = r + row < re ? *reinterpret_cast<const f32x4*>(dh + (size_t)(r + row) * N4 + n0 + c4 * 4) : zero;
    }
    gb = r + brow < re ? *reinterpret_cast<const f32x4*>(x + (size_t)(r + brow) * Cin + c0 + bc4 * 4) : zero;
  };
  if (rb < re) fetch(rb);
  for (long long r = rb; r < re; r += MW_KC) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int idx = tid + i * 256, row = idx >> 6, c4 = idx & 63;
      *reinterpret_cast<f32x4*>(sA + row * MW_LDA + c4 * 4) = ga[i];
    }
    *reinterpret_cast<f32x4*>(sB + brow * MW_LDB + bc4 * 4) = gb;
    __syncthreads();
    if (r + MW_KC < re) fetch(r + MW_KC);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int k = 4 * t + kq;
      float a[4], b[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        a[i] = sA[k * MW_LDA + wave * 64 + i * 16 + j];
        b[i] = sB[k * MW_LDB + i * 16 + j];
      }
#pragma unroll
      for (int ia = 0; ia < 4; ++ia)
#pragma unroll
        for (int ib = 0; ib < 4; ++ib) acc[ia][ib] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[ia], b[ib], acc[ia][ib], 0, 0, 0);
    }
    __syncthreads();
  }
  // the lane holds rows n0 + wave 64 + ia 16 + 4 kq + e, column c0 + ib 16 + j
  float* out = part + (size_t)blockIdx.y * N4 * Cin;
#pragma unroll
  for (int ia = 0; ia < 4; ++ia)
#pragma unroll
    for (int ib = 0; ib < 4; ++ib)
#pragma unroll
      for (int e = 0; e < 4; ++e) out[(size_t)(n0 + wave * 64 + ia * 16 + 4 * kq + e) * Cin + c0 + ib * 16 + j] = acc[ia][ib][e];
}

__global__ __launch_bounds__(256) void mask_wgrad_finish_kernel(const float* __restrict__ part, int slices, long long n, float* __restrict__ dw) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float s = 0.f;
  for (int k = 0; k < slices; ++k) s += part[(size_t)k * n + i];
  dw[i] = s;
}

extern "C" long long lvc_mask_deconv_wgrad_workspace_bytes(int M, int S, int Cin, int Cmid) {
  if (M < 0 || S < 1 || Cin < 1 || Cmid < 1) return -1;
  return (long long)mask_wgrad_cut(M, S).slices * 4 * Cmid * Cin * 4;
}

extern "C" int lvc_mask_deconv_wgrad(const float* dh, const float* x, const int* d_num_valid, float* dw_packed, int M, int S, int Cin,
                                     int Cmid, void* workspace, long long workspace_bytes, void* stream) {
  LVC_CHECK_ARG(M >= 0 && S >= 1, "M >= 0, S >= 1");
  LVC_CHECK_ARG(Cin >= 64 && Cin <= 256 && Cin % 64 == 0 && Cmid >= 64 && Cmid <= 256 && Cmid % 64 == 0,
                "channels of the deconvolution: multiples of 64 up to 256 (MODEL.ROI_MASK_HEAD.CONV_DIM)");
  LVC_CHECK_ARG(dw_packed && workspace && (M == 0 || (dh && x)), "null pointer");
  LVC_CHECK_ARG((((uintptr_t)dh | (uintptr_t)workspace) & 15) == 0, "16-byte aligned operands");
  LVC_CHECK_ARG((long long)M * S * S < (1LL << 31), "too many rows");
  LVC_CHECK_ARG(workspace_bytes >= lvc_mask_deconv_wgrad_workspace_bytes(M, S, Cin, Cmid), "workspace too small");
  const LvcSliceCut cut = mask_wgrad_cut(M, S);
  const int N4 = 4 * Cmid, slices = cut.slices;
  const long long n = (long long)N4 * Cin;
  hipStream_t st = (hipStream_t)stream;
  float* part = reinterpret_cast<float*>(workspace);
  hipLaunchKernelGGL(mask_wgrad_kernel, dim3((unsigned)((N4 / MW_TN) * (Cin / MW_TC)), (unsigned)slices), dim3(256), 0, st, dh, x, d_num_valid,
                     part, M, S * S, N4, Cin, cut.rows);
  hipLaunchKernelGGL(mask_wgrad_finish_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, part, slices, n, dw_packed);
  LVC_CHECK_LAUNCH();
  return LVC_OK;
}
