// keypoint_train.hip -- the keypoint branch's training loss and the backward of `score_lowres` (reference
// detectron2/modeling/roi_heads/keypoint_head.py keypoint_rcnn_loss: cross_entropy(sum) over the (4S)^2 positions of the bilinear x2
// map of every valid (row, keypoint), and autograd through interpolate and ConvTranspose2d(Cin, K, 4, stride 2, padding 1)).
// Built without contraction: the x2 map is keypoint_upsample.h's expression, the bits keypoint_decode.hip decodes.
//
// lvc_keypoint_loss: one workgroup per (row, keypoint).  An entry with valid == 0 returns at once.  The low-resolution plane [2S, 2S]
//   is read once, the x2 map [4S, 4S] is formed in LDS (the [M, K, 4S, 4S] tensor is never written), its maximum is taken in fp32
//   (exact) and sum exp(z - max) and the term  max + log(sum) - z[target]  in fp64.  The term, the maximum and the log-sum are kept
//   for the backward.  A target outside [0, 16 S^2) on a valid entry sets KEYPOINT_BAD_TARGET; the entry is skipped by every kernel.
//   A finishing workgroup adds the terms: lane t walks entries t, t + 256, ... in order, then a fixed tree.  loss = sum / normaliser
//   x LOSS_WEIGHT with the normaliser either the counted valid entries (normalizer <= 0) or the given number; count 0 gives exactly 0.
//
// lvc_keypoint_loss_grad: one workgroup per (row, keypoint): g = (softmax - onehot) x upstream / normaliser x LOSS_WEIGHT on the x2
//   map in LDS (fp64), then the ADJOINT of the bilinear x2 as a gather: a low-resolution pixel (a, b) sums the up-to 4x4 upsampled
//   pixels oy in [2a - 1, 2a + 2], ox in [2b - 1, 2b + 2] that read it, each with the product of its two clamped-edge weights, in fp64,
//   oy-major, and is rounded once.  Invalid entries and rows that were not selected get zeros.
//   LAYOUT of dlow: channels-last [M, 2S, 2S, Kc], Kc = K rounded up to 4, the padding channels zero.  The two kernels below gather
//   a tap's K channels of one pixel as consecutive floats (16-byte reads in dx); with planes [M, K, 2S, 2S] every one of their
//   reads would be a lone float.  The loss-grad kernel pays for it with strided 4-byte stores, 4 S^2 per workgroup.
//
// lvc_keypoint_deconv_dx: dx[m, iy, ix, ci] = sum_k sum_{ky,kx} dlow[m, 2iy-1+ky, 2ix-1+kx, k] W[ci, k, ky, kx]: a gathered
//   [M S^2, 16 Kc] x [16 Kc, Cin] product on v_mfma_f32_16x16x4_f32 (fp32 operands: exact products, range-free, no tier, no range
//   word).  No im2col tensor: a lane reads its pixel's taps from dlow.  The contraction index is e = (ky 4 + kx) Kc + k; Kc is a
//   multiple of 4, so a lane's 16-byte read lies in one tap.  The weight operand is its own packing [Cin][16 Kc]
//   (lvc_keypoint_deconv_dx_pack).  The four MFMA steps of a 16-wide chunk go to four accumulators, added in a fixed order at the end.
//
// lvc_keypoint_deconv_wgrad: dW[ci, e] = sum_rows x[row, ci] dlow[tap e of row, k of e] on fp32 MFMA, and db[k] = sum dlow.  The rows
//   are cut into slices fixed by M and S alone; a workgroup owns a (64 e x 64 ci) tile of one slice and writes its partial; a
//   finishing launch adds the slices in index order (in fp64, rounded once).  db: fp64 partials of 512-pixel chunks, added by one
//   workgroup per keypoint in a fixed order.  No float atomics: conv_wgrad joins its slices with them
//   and cannot give the same bits twice.  dW comes out in the dx packing [Cin][16 Kc].
//
// Every kernel: rows past *d_num_valid are neither read nor written; no float atomics; two runs give the same bits.
#include "conv_common.h"
#include "keypoint_upsample.h"
#include "rows_common.h"

#define KL_MAX_P 32               // 2S at most (the x2 map's side is at most 64, as in keypoint_decode.hip)
#define KL_STATUS_TARGET 16       // status bit: a target outside [0, 16 S^2) on a valid entry
#define KX_TM 64                  // dx: rows (input pixels) per workgroup, 16 per wave
#define KW_KC 32                  // wgrad: rows per LDS chunk (a multiple of 16: four rows per MFMA step, steps dealt to four accumulators)
#define KW_LD (64 + 16)           // wgrad: LDS row stride
#define KW_SLICE_ROWS 2048        // wgrad: rows per slice (a multiple of KW_KC) ...
#define KW_MAX_SLICES 64          // ... unless that would make more slices than this
#define KB_PIXELS 512             // db: low-resolution pixels per workgroup

static int kl_channels(int K) { return (K + 3) / 4 * 4; }

extern "C" int lvc_keypoint_dlow_channels(int K) { return K < 1 ? 0 : kl_channels(K); }

// ------------------------------------------------------------------------------------------------- loss
__global__ __launch_bounds__(256) void keypoint_loss_kernel(const float* __restrict__ low, const int* __restrict__ target,
                                                            const unsigned char* __restrict__ valid, const int* __restrict__ d_num_valid,
                                                            int* __restrict__ d_status, double* __restrict__ term,
                                                            float* __restrict__ pmax, double* __restrict__ plse, int M, int K, int P) {
  __shared__ float slow[KL_MAX_P * KL_MAX_P];
  __shared__ float smap[4 * KL_MAX_P * KL_MAX_P];
  __shared__ float redf[4];
  __shared__ double redd[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int Mv = lvc_valid_rows(d_num_valid, M);
  const int e = blockIdx.x, m = e / K;
  if (m >= Mv) return;            // (uniform)
  if (!valid[e]) return;          // (uniform)
  const int side = 2 * P, n = side * side;
  const int t = target[e];
  if (t < 0 || t >= n) {          // (uniform) nothing is read out of range
    if (d_status && tid == 0) atomicOr(d_status, KL_STATUS_TARGET);
    return;
  }
  const float* src = low + (size_t)e * P * P;
  for (int i = tid; i < P * P; i += 256) slow[i] = src[i];
  __syncthreads();
  float mx = -INFINITY;
  for (int i = tid; i < n; i += 256) {
    const int oy = i / side, ox = i - oy * side;
    const float v = kp_up2(slow, P, oy, ox);
    smap[i] = v;
    mx = fmaxf(mx, v);
  }
  for (int d = 32; d > 0; d >>= 1) mx = fmaxf(mx, __shfl_xor(mx, d));
  if (lane == 0) redf[wave] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(redf[0], redf[1]), fmaxf(redf[2], redf[3]));
  double s = 0.0;
  for (int i = tid; i < n; i += 256) s += exp((double)smap[i] - (double)mx);
  for (int d = 32; d > 0; d >>= 1) s += __shfl_xor(s, d);
  if (lane == 0) redd[wave] = s;
  __syncthreads();
  if (tid == 0) {
    const double lse = log((redd[0] + redd[1]) + (redd[2] + redd[3]));
    term[e] = ((double)mx + lse) - (double)smap[t];
    pmax[e] = mx;
    plse[e] = lse;
  }
}

__global__ __launch_bounds__(256) void keypoint_loss_finish_kernel(const double* __restrict__ term, const int* __restrict__ target,
                                                                   const unsigned char* __restrict__ valid,
                                                                   const int* __restrict__ d_num_valid, int M, int K, int n,
                                                                   double normalizer, double weight, float* __restrict__ out_loss,
                                                                   double* __restrict__ out_sum, long long* __restrict__ out_count) {
  __shared__ double ss[256];
  __shared__ long long sc[256];
  const int tid = threadIdx.x;
  const long long N = (long long)lvc_valid_rows(d_num_valid, M) * K;
  double s = 0.0;
  long long c = 0;
  for (long long e = tid; e < N; e += 256) {
    if (!valid[e]) continue;
    const int t = target[e];
    if (t < 0 || t >= n) continue;
    s += term[e];
    ++c;
  }
  ss[tid] = s;
  sc[tid] = c;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (tid < h) {
      ss[tid] += ss[tid + h];
      sc[tid] += sc[tid + h];
    }
    __syncthreads();
  }
  if (tid == 0) {
    const double norm = normalizer > 0.0 ? normalizer : (double)sc[0];
    *out_loss = sc[0] > 0 ? (float)(ss[0] / norm * weight) : 0.f;
    *out_sum = ss[0];
    *out_count = sc[0];
  }
}

static int kl_check(int M, int K, int S) { return M >= 0 && K >= 1 && K <= 64 && S >= 1 && 2 * S <= KL_MAX_P; }

extern "C" int lvc_keypoint_loss(const float* low, const int* target, const unsigned char* valid, const int* d_num_valid, int M, int K,
                                 int S, double normalizer, double loss_weight, double* term, float* plane_max, double* plane_lse,
                                 float* out_loss, double* out_sum, long long* out_count, int* d_status, void* stream) {
  LVC_CHECK_ARG(kl_check(M, K, S), "M >= 0, 1 <= K <= 64, 1 <= S <= 16");
  LVC_CHECK_ARG(out_loss && out_sum && out_count, "null pointer");
  LVC_CHECK_ARG(M == 0 || (low && target && valid && term && plane_max && plane_lse), "null pointer");
  LVC_CHECK_ARG((long long)M * K < (1LL << 31), "too many (row, keypoint) planes");
  hipStream_t st = (hipStream_t)stream;
  if (M > 0)
    hipLaunchKernelGGL(keypoint_loss_kernel, dim3((unsigned)(M * K)), dim3(256), 0, st, low, target, valid, d_num_valid, d_status, term,
                       plane_max, plane_lse, M, K, 2 * S);
  hipLaunchKernelGGL(keypoint_loss_finish_kernel, dim3(1), dim3(256), 0, st, term, target, valid, d_num_valid, M, K, 16 * S * S,
                     normalizer, loss_weight, out_loss, out_sum, out_count);
  LVC_CHECK_LAUNCH();
  return LVC_OK;
}

// ------------------------------------------------------------------------------------------------- loss gradient -> dlow
__global__ __launch_bounds__(256) void keypoint_loss_grad_kernel(const float* __restrict__ low, const int* __restrict__ target,
                                                                 const unsigned char* __restrict__ valid, const float* __restrict__ pmax,
                                                                 const double* __restrict__ plse, const long long* __restrict__ d_count,
                                                                 const float* __restrict__ d_up, const int* __restrict__ d_num_valid,
                                                                 float* __restrict__ dlow, int M, int K, int Kc, int P, double normalizer,
                                                                 double weight) {
  __shared__ float slow[KL_MAX_P * KL_MAX_P];
  __shared__ double sg[4 * KL_MAX_P * KL_MAX_P];
  const int tid = threadIdx.x;
  const int Mv = lvc_valid_rows(d_num_valid, M);
  const int e = blockIdx.x, m = e / K, k = e - m * K;
  if (m >= Mv) return;            // (uniform)
  const int side = 2 * P, n = side * side, PP = P * P;
  const int t = target[e];
  const bool ok = valid[e] && t >= 0 && t < n;
  float* o = dlow + (size_t)m * PP * Kc;
  const int kend = k == K - 1 ? Kc : k + 1;      // the last keypoint's workgroup also clears the padding channels
  if (!ok) {                      // (uniform)
    for (int q = tid; q < PP; q += 256)
      for (int c = k; c < kend; ++c) o[(size_t)q * Kc + c] = 0.f;
    return;
  }
  const long long cnt = *d_count;
  const double norm = normalizer > 0.0 ? normalizer : (double)cnt;
  const double scale = cnt > 0 ? (double)*d_up / norm * weight : 0.0;
  const float* src = low + (size_t)e * PP;
  for (int i = tid; i < PP; i += 256) slow[i] = src[i];
  __syncthreads();
  const double shift = (double)pmax[e] + plse[e];
  for (int i = tid; i < n; i += 256) {
    const int oy = i / side, ox = i - oy * side;
    const double p = exp((double)kp_up2(slow, P, oy, ox) - shift);
    sg[i] = (p - (i == t ? 1.0 : 0.0)) * scale;
  }
  __syncthreads();
  for (int q = tid; q < PP; q += 256) {
    const int a = q / P, b = q - a * P;
    const int oy0 = 2 * a - 1 < 0 ? 0 : 2 * a - 1, oy1 = 2 * a + 2 > side - 1 ? side - 1 : 2 * a + 2;
    const int ox0 = 2 * b - 1 < 0 ? 0 : 2 * b - 1, ox1 = 2 * b + 2 > side - 1 ? side - 1 : 2 * b + 2;
    double acc = 0.0;
    for (int oy = oy0; oy <= oy1; ++oy) {
      const double wy = (double)kp_up2_weight(oy, P, a);
      for (int ox = ox0; ox <= ox1; ++ox) acc += sg[oy * side + ox] * (wy * (double)kp_up2_weight(ox, P, b));
    }
    o[(size_t)q * Kc + k] = (float)acc;
    for (int c = k + 1; c < kend; ++c) o[(size_t)q * Kc + c] = 0.f;
  }
}

extern "C" int lvc_keypoint_loss_grad(const float* low, const int* target, const unsigned char* valid, const float* plane_max,
                                      const double* plane_lse, const long long* d_count, const float* d_upstream, const int* d_num_valid,
                                      int M, int K, int S, double normalizer, double loss_weight, float* dlow, void* stream) {
  LVC_CHECK_ARG(kl_check(M, K, S), "M >= 0, 1 <= K <= 64, 1 <= S <= 16");
  if (M == 0) return LVC_OK;
  LVC_CHECK_ARG(low && target && valid && plane_max && plane_lse && d_count && d_upstream && dlow, "null pointer");
  LVC_CHECK_ARG((long long)M * K < (1LL << 31), "too many (row, keypoint) planes");
  hipLaunchKernelGGL(keypoint_loss_grad_kernel, dim3((unsigned)(M * K)), dim3(256), 0, (hipStream_t)stream, low, target, valid, plane_max,
                     plane_lse, d_count, d_upstream, d_num_valid, dlow, M, K, kl_channels(K), 2 * S, normalizer, loss_weight);
  LVC_CHECK_LAUNCH();
  return LVC_OK;
}

// ------------------------------------------------------------------------------------------------- dx
// ConvTranspose2d weight [Cin, K, 4, 4] -> [Cin][16 Kc]: column (ky 4 + kx) Kc + k, zeros for k >= K
__global__ void keypoint_dx_pack_kernel(const float* __restrict__ w, float* __restrict__ wp, int Cin, int K, int Kc) {
  const long long n = 16LL * Kc * Cin;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const int k = (int)(i % Kc);
    const long long rest = i / Kc;
    const int tap = (int)(rest % 16), ci = (int)(rest / 16);
    wp[i] = k < K ? w[((size_t)ci * K + k) * 16 + tap] : 0.f;
  }
}

static int kx_check(int Cin, int K) { return Cin >= 16 && Cin % 16 == 0 && Cin <= 4096 && K >= 1 && K <= 64; }

extern "C" int lvc_keypoint_deconv_dx_pack(const float* weight, float* packed, int Cin, int K, void* stream) {
  LVC_CHECK_ARG(kx_check(Cin, K), "Cin: a multiple of 16 up to 4096; 1 <= K <= 64");
  LVC_CHECK_ARG(weight && packed, "null pointer");
  const long long n = 16LL * kl_channels(K) * Cin;
  const unsigned blocks = (unsigned)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
  hipLaunchKernelGGL(keypoint_dx_pack_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, weight, packed, Cin, K, kl_channels(K));
  LVC_CHECK_LAUNCH();
  return LVC_OK;
}

// D[16 ci][16 pixels] += A[16 ci][4 e] B[4 e][16 pixels]: lane (j, kq) gives A[ci j][e 16c + 4kq + t] and B[the same e][pixel j] in
// step t, and holds ci 4 kq + i of pixel j.  A wave owns 16 rows and four 16-channel blocks of ci.
__global__ __launch_bounds__(256) void keypoint_dx_kernel(const float* __restrict__ dlow, const float* __restrict__ wp,
                                                          const int* __restrict__ d_num_valid, float* __restrict__ dx, int M, int S,
                                                          int Cin, int Kc) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = lane & 15, kq = lane >> 4;
  const int S2 = S * S, P = 2 * S, E = 16 * Kc;
  const long long R = (long long)lvc_valid_rows(d_num_valid, M) * S2;
  const long long r0 = (long long)blockIdx.x * KX_TM;
  if (r0 >= R) return;      // (uniform) rows past num_valid are neither read nor written
  const int cb0 = blockIdx.y * 4, ncb = Cin >> 4;
  const long long r = r0 + wave * 16 + j;
  const bool live = r < R;
  const long long m = r / S2;
  const int rem = (int)(r - m * S2);
  const int iy = rem / S, ix = rem - iy * S;
  const float* plane = dlow + (size_t)m * P * P * Kc;      // (not dereferenced unless live)

  f32x4 acc[4][4];      // [MFMA step t][channel block]
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int nb = 0; nb < 4; ++nb) acc[t][nb] = f32x4{0.f, 0.f, 0.f, 0.f};
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  int tap = (4 * kq) / Kc, k = 4 * kq - tap * Kc;      // of e = 16 c + 4 kq; advanced by 16 per chunk with a carry
  for (int c = 0; c < Kc; ++c) {      // E / 16 chunks
    const int e = 16 * c + 4 * kq;
    const int oy = 2 * iy - 1 + (tap >> 2), ox = 2 * ix - 1 + (tap & 3);
    f32x4 b = zero;
    if (live && oy >= 0 && oy < P && ox >= 0 && ox < P) b = *reinterpret_cast<const f32x4*>(plane + ((size_t)oy * P + ox) * Kc + k);
    f32x4 a[4];
#pragma unroll
    for (int nb = 0; nb < 4; ++nb) {
      a[nb] = zero;
      if (cb0 + nb < ncb) a[nb] = *reinterpret_cast<const f32x4*>(wp + ((size_t)(cb0 + nb) * 16 + j) * E + e);      // (uniform guard)
    }
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int nb = 0; nb < 4; ++nb) acc[t][nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[nb][t], b[t], acc[t][nb], 0, 0, 0);
    k += 16;
    while (k >= Kc) {
      k -= Kc;
      ++tap;
    }
  }
  if (!live) return;
#pragma unroll
  for (int nb = 0; nb < 4; ++nb) {
    if (cb0 + nb >= ncb) continue;
    f32x4 v;
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = (acc[0][nb][i] + acc[1][nb][i]) + (acc[2][nb][i] + acc[3][nb][i]);
    *reinterpret_cast<f32x4*>(dx + (size_t)r * Cin + (cb0 + nb) * 16 + 4 * kq) = v;
  }
}

extern "C" int lvc_keypoint_deconv_dx(const float* dlow, const float* packed, const int* d_num_valid, float* dx, int M, int S, int Cin,
                                      int K, void* stream) {
  LVC_CHECK_ARG(M >= 0 && S >= 1 && S <= 1024, "M >= 0, 1 <= S <= 1024");
  LVC_CHECK_ARG(kx_check(Cin, K), "Cin: a multiple of 16 up to 4096; 1 <= K <= 64");
  if (M == 0) return LVC_OK;
  LVC_CHECK_ARG(dlow && packed && dx, "null pointer");
  LVC_CHECK_ARG((((uintptr_t)dlow | (uintptr_t)packed | (uintptr_t)dx) & 15) == 0, "16-byte aligned operands");
  LVC_CHECK_ARG((long long)M * S * S < (1LL << 31) - KX_TM, "too many rows");
  const long long rows = (long long)M * S * S;
  hipLaunchKernelGGL(keypoint_dx_kernel, dim3((unsigned)((rows + KX_TM - 1) / KX_TM), (unsigned)((Cin / 16 + 3) / 4)), dim3(256), 0,
                     (hipStream_t)stream, dlow, packed, d_num_valid, dx, M, S, Cin, kl_channels(K));
  LVC_CHECK_LAUNCH();
  return LVC_OK;
}

// ------------------------------------------------------------------------------------------------- dW, db
static LvcSliceCut kw_cut(int M, int S) { return lvc_slice_cut((long long)M * S * S, KW_SLICE_ROWS, KW_MAX_SLICES, KW_KC); }

// D[16 e][16 ci] += A[16 e][4 rows] B[4 rows][16 ci]; the workgroup's (64 e x 64 ci) tile: wave w owns e block w and the four ci blocks
__global__ __launch_bounds__(256) void keypoint_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ dlow,
                                                             const int* __restrict__ d_num_valid, float* __restrict__ part, int M, int S,
                                                             int Cin, int Kc, long long slice_rows) {
  __shared__ float sA[KW_KC * KW_LD];
  __shared__ float sB[KW_KC * KW_LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = lane & 15, kq = lane >> 4;
  const int S2 = S * S, P = 2 * S, E = 16 * Kc;
  const long long R = (long long)lvc_valid_rows(d_num_valid, M) * S2;      // rows past it are never read
  const int ne = E / 64;
  const int e0 = (blockIdx.x % ne) * 64, c0 = (blockIdx.x / ne) * 64;
  const long long rb = (long long)blockIdx.y * slice_rows;
  long long re = rb + slice_rows;
  if (re > R) re = R;
  const int el = tid & 63, rq = tid >> 6;
  const int e = e0 + el, tap = e / Kc, k = e - tap * Kc;
  const int ky = tap >> 2, kx = tap & 3;
  const int ci = c0 + el;
  const bool ci_ok = ci < Cin;

  f32x4 acc[4][4];      // [MFMA step t][ci block]
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int ib = 0; ib < 4; ++ib) acc[t][ib] = f32x4{0.f, 0.f, 0.f, 0.f};
  float ga[KW_KC / 4], gb[KW_KC / 4];
  auto fetch = [&](long long r) {
    // the thread's rows r + rq, r + rq + 4, ...: one division for the first, then (m, iy, ix) advance by four pixels with carries
    // (a division per row made the kernel wait on its index arithmetic, not on its MFMAs)
    long long m = (r + rq) / S2;
    const int rem = (int)(r + rq - m * S2);
    int iy = rem / S, ix = rem - iy * S;
#pragma unroll
    for (int i = 0; i < KW_KC / 4; ++i) {
      const long long row = r + rq + 4 * i;
      ga[i] = gb[i] = 0.f;
      if (row < re) {
        const int oy = 2 * iy - 1 + ky, ox = 2 * ix - 1 + kx;
        if (oy >= 0 && oy < P && ox >= 0 && ox < P) ga[i] = dlow[(((size_t)m * P + oy) * P + ox) * Kc + k];
        if (ci_ok) gb[i] = x[(size_t)row * Cin + ci];
      }
      ix += 4;
      while (ix >= S) {
        ix -= S;
        if (++iy == S) {
          iy = 0;
          ++m;
        }
      }
    }
  };
  if (rb < re) fetch(rb);
  for (long long r = rb; r < re; r += KW_KC) {
#pragma unroll
    for (int i = 0; i < KW_KC / 4; ++i) {
      sA[(rq + 4 * i) * KW_LD + el] = ga[i];
      sB[(rq + 4 * i) * KW_LD + el] = gb[i];
    }
    __syncthreads();
    if (r + KW_KC < re) fetch(r + KW_KC);
#pragma unroll
    for (int t = 0; t < KW_KC / 4; ++t) {
      const int kk = 4 * t + kq;
      const float a = sA[kk * KW_LD + wave * 16 + j];
#pragma unroll
      for (int ib = 0; ib < 4; ++ib)
        acc[t & 3][ib] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, sB[kk * KW_LD + ib * 16 + j], acc[t & 3][ib], 0, 0, 0);
    }
    __syncthreads();
  }
  // the lane holds e = e0 + wave 16 + 4 kq + i of ci = c0 + ib 16 + j
  float* out = part + (size_t)blockIdx.y * Cin * E;
#pragma unroll
  for (int ib = 0; ib < 4; ++ib) {
    const int co = c0 + ib * 16 + j;
    if (co >= Cin) continue;
    f32x4 v;
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = (acc[0][ib][i] + acc[1][ib][i]) + (acc[2][ib][i] + acc[3][ib][i]);
    *reinterpret_cast<f32x4*>(out + (size_t)co * E + e0 + wave * 16 + 4 * kq) = v;
  }
}

// db partials: workgroup = KB_PIXELS consecutive low-resolution pixels of the flat [M 4 S^2] list (the cut depends on M and S alone);
// thread (channel c = tid & 63, phase = tid >> 6) walks the chunk's pixels phase, phase + 4, ... in fp64; the four phases are added in
// a fixed order.  (One workgroup per row slice -- 25 workgroups of 2048 dependent loads each at M = 256 -- took longer than the MFMA
// kernel beside it.)
__global__ __launch_bounds__(256) void keypoint_dbias_kernel(const float* __restrict__ dlow, const int* __restrict__ d_num_valid,
                                                             double* __restrict__ pb, int M, int S, int Kc) {
  __shared__ double sa[4][64];
  const int c = threadIdx.x & 63, ph = threadIdx.x >> 6;
  const long long N = (long long)lvc_valid_rows(d_num_valid, M) * 4 * S * S;
  const long long p0 = (long long)blockIdx.x * KB_PIXELS;
  long long p1 = p0 + KB_PIXELS;
  if (p1 > N) p1 = N;
  double a = 0.0;
  if (c < Kc) {
#pragma unroll 4
    for (long long p = p0 + ph; p < p1; p += 4) a += (double)dlow[(size_t)p * Kc + c];
  }
  sa[ph][c] = a;
  __syncthreads();
  if (ph == 0 && c < Kc) pb[(size_t)blockIdx.x * Kc + c] = (sa[0][c] + sa[1][c]) + (sa[2][c] + sa[3][c]);
}

// db[k]: workgroup k adds the chunk partials -- thread t those of chunks t, t + 256, ... in order, then a fixed tree
__global__ __launch_bounds__(256) void keypoint_dbias_finish_kernel(const double* __restrict__ pb, int chunks, int Kc, float* __restrict__ db) {
  __shared__ double ss[256];
  const int k = blockIdx.x, tid = threadIdx.x;
  double s = 0.0;
  for (int q = tid; q < chunks; q += 256) s += pb[(size_t)q * Kc + k];
  ss[tid] = s;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (tid < h) ss[tid] += ss[tid + h];
    __syncthreads();
  }
  if (tid == 0) db[k] = (float)ss[0];
}

__global__ __launch_bounds__(256) void keypoint_wgrad_finish_kernel(const float* __restrict__ part, int slices, long long n,
                                                                    float* __restrict__ dw) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double s = 0.0;
  for (int q = 0; q < slices; ++q) s += (double)part[(size_t)q * n + i];
  dw[i] = (float)s;
}

static long long kb_chunks(int M, int S) {
  const long long n = ((long long)M * 4 * S * S + KB_PIXELS - 1) / KB_PIXELS;
  return n < 1 ? 1 : n;
}

extern "C" long long lvc_keypoint_deconv_wgrad_workspace_bytes(int M, int S, int Cin, int K) {
  if (M < 0 || S < 1 || Cin < 1 || K < 1) return -1;
  const long long Kc = kl_channels(K);
  return (long long)kw_cut(M, S).slices * 16LL * Kc * Cin * 4 + kb_chunks(M, S) * Kc * 8;
}

extern "C" int lvc_keypoint_deconv_wgrad(const float* x, const float* dlow, const int* d_num_valid, float* dw_packed, float* db, int M,
                                         int S, int Cin, int K, void* workspace, long long workspace_bytes, void* stream) {
  LVC_CHECK_ARG(M >= 0 && S >= 1 && S <= 1024, "M >= 0, 1 <= S <= 1024");
  LVC_CHECK_ARG(kx_check(Cin, K), "Cin: a multiple of 16 up to 4096; 1 <= K <= 64");
  LVC_CHECK_ARG(dw_packed && db && workspace && (M == 0 || (x && dlow)), "null pointer");
  LVC_CHECK_ARG((((uintptr_t)workspace | (uintptr_t)dw_packed) & 15) == 0, "16-byte aligned operands");
  LVC_CHECK_ARG((long long)M * S * S < (1LL << 31) - KX_TM, "too many rows");
  LVC_CHECK_ARG(workspace_bytes >= lvc_keypoint_deconv_wgrad_workspace_bytes(M, S, Cin, K), "workspace too small");
  const LvcSliceCut cut = kw_cut(M, S);
  const int Kc = kl_channels(K), E = 16 * Kc, slices = cut.slices;
  const long long n = (long long)E * Cin, per = cut.rows;
  hipStream_t st = (hipStream_t)stream;
  const long long chunks = kb_chunks(M, S);
  LVC_CHECK_ARG(chunks < (1LL << 31), "too many rows");
  double* pb = reinterpret_cast<double*>(workspace);      // [chunks][Kc], then the tile partials [slices][Cin][E]
  float* part = reinterpret_cast<float*>(pb + (size_t)chunks * Kc);
  hipLaunchKernelGGL(keypoint_wgrad_kernel, dim3((unsigned)((E / 64) * ((Cin + 63) / 64)), (unsigned)slices), dim3(256), 0, st, x, dlow,
                     d_num_valid, part, M, S, Cin, Kc, per);
  hipLaunchKernelGGL(keypoint_wgrad_finish_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, part, slices, n, dw_packed);
  hipLaunchKernelGGL(keypoint_dbias_kernel, dim3((unsigned)chunks), dim3(256), 0, st, dlow, d_num_valid, pb, M, S, Kc);
  hipLaunchKernelGGL(keypoint_dbias_finish_kernel, dim3((unsigned)K), dim3(256), 0, st, pb, (int)chunks, Kc, db);
  LVC_CHECK_LAUNCH();
  return LVC_OK;
}
