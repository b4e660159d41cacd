// mask_deconv.hip -- the tail of detectron2's MaskRCNNConvUpsampleHead at inference (reference detectron2/modeling/roi_heads/mask_head.py
// `layers` + `mask_rcnn_inference`): ConvTranspose2d(Cin, Cmid, 2, stride 2) + bias -> ReLU -> Conv2d(Cmid, K, 1) + bias -> the predicted
// class's plane -> sigmoid, in ONE launch:
//
//   prob[m, 2y+dy, 2x+dx] = sigmoid(bp[c] + sum_co relu(bd[co] + sum_ci x[m,y,x,ci] * Wd[ci,co,dy,dx]) * Wp[c,co]),   c = classes[m]
//
// The reference writes the deconvolution's [M, Cmid, 2S, 2S] map (800 KB per RoI at S = 14, Cmid = 256) and all K logit planes, then
// keeps one plane.  A stride-2 2x2 transposed convolution has no overlap between taps: it is the GEMM [M S^2, Cin] x [Cin, 4 Cmid]
// (column (dy*2+dx)*Cmid + co), and the predictor for ONE class is a dot product of a row's Cmid values of one tap with Wp[c, :].
//
// What was chosen
//   * Arithmetic: v_mfma_f32_16x16x4_f32 on fp32 operands, as conv_grouped.hip: exact products, fp32 accumulation, range-free (no
//     range word, no tier).
//   * Tiling: a workgroup (4 waves) owns 64 rows (pixels of consecutive RoIs: a tile may straddle RoIs, each row carries its class).
//     The 64 x Cin activations sit in LDS once.  D[16 co][16 pixels] += A[16 co][4 ci] * B[4 ci][16 pixels]; a wave owns Cmid/64
//     16-channel blocks of every tap and walks the four taps one after another: 4 pixel blocks x Cmid/64 channel blocks of accumulators
//     live through one pass over Cin.  The k index of an MFMA step is free as long as A and B agree: lane group kq takes channels
//     16 kc + 4 kq + t in step t, so one 16-byte read per operand feeds four steps (weights from the packed [4 Cmid, Cin] rows in
//     L2, activations from LDS).
//   * Epilogue in registers: a lane ends a pass with 4 consecutive co of one pixel per block: + bd, ReLU, times Wp[c, co..co+3],
//     summed over its blocks; the four lane groups are added by two cross-lane steps, the four waves through 4 KB of LDS, always in
//     the same order.  Nothing of size Cmid (2S)^2 leaves the workgroup; no atomics on data: two runs are bit-identical.
//   * A class outside [0, K) sets bit 3 (value 8) of the status word and is computed as class 0: nothing is read out of bounds.
#include "conv_common.h"
#include "rows_common.h"

#define MD_TM 64            // rows (pixels) per workgroup
#define MD_PAD 4            // floats of padding per LDS row
#define MD_STATUS_CLASS 8   // status bit: a class index outside [0, K)

template <int NBC, bool SIGMOID>      // Cmid / 64: 16-channel blocks per wave and tap; SIGMOID false: the logits leave (training)
__global__ __launch_bounds__(256) void mask_deconv_kernel(const float* __restrict__ x, const float* __restrict__ wd,
                                                          const float* __restrict__ bd, const float* __restrict__ wp,
                                                          const float* __restrict__ bp, const int* __restrict__ classes,
                                                          const int* __restrict__ d_num_valid, int* __restrict__ d_status,
                                                          float* __restrict__ prob, int M, int S, int Cin, int K) {
  constexpr int Cmid = 64 * NBC;
  extern __shared__ __attribute__((aligned(16))) unsigned char md_smem[];
  const int LDP = Cin + MD_PAD;
  float* sx = reinterpret_cast<float*>(md_smem);                  // [MD_TM][LDP]
  float* red = sx + MD_TM * LDP;                                  // [4 waves][4 taps][MD_TM]
  int* scls = reinterpret_cast<int*>(red + 4 * 4 * MD_TM);        // [MD_TM]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = lane & 15, kq = lane >> 4;
  const int S2 = S * S;
  const int Mv = lvc_valid_rows(d_num_valid, M);
  const long long R = (long long)Mv * S2;
  const long long r0 = (long long)blockIdx.x * MD_TM;
  if (r0 >= R) return;      // (uniform) rows past num_valid are neither read nor written

  const int c4n = Cin >> 2;
  for (int idx = tid; idx < MD_TM * c4n; idx += 256) {
    const int p = idx / c4n, c4 = idx - p * c4n;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (r0 + p < R) v = *reinterpret_cast<const f32x4*>(x + (size_t)(r0 + p) * Cin + c4 * 4);
    *reinterpret_cast<f32x4*>(sx + p * LDP + c4 * 4) = v;
  }
  if (tid < MD_TM) {
    int c = 0;
    if (r0 + tid < R && classes) {
      c = classes[(r0 + tid) / S2];
      if (c < 0 || c >= K) {
        if (d_status) atomicOr(d_status, MD_STATUS_CLASS);
        c = 0;
      }
    }
    scls[tid] = c;
  }
  __syncthreads();

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
      const int c = scls[pb * 16 + j];
      float s = 0.f;
#pragma unroll
      for (int nb = 0; nb < NBC; ++nb) {
        const int co = (wave * NBC + nb) * 16 + kq * 4;
        f32x4 b4 = {0.f, 0.f, 0.f, 0.f};
        if (bd) b4 = *reinterpret_cast<const f32x4*>(bd + co);
        const f32x4 w4 = *reinterpret_cast<const f32x4*>(wp + (size_t)c * Cmid + co);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float v = acc[pb][nb][e] + b4[e];
          v = v > 0.f ? v : 0.f;
          s = fmaf(v, w4[e], s);
        }
      }
      s += __shfl_xor(s, 16);
      s += __shfl_xor(s, 32);
      if (kq == 0) red[(wave * 4 + q) * MD_TM + pb * 16 + j] = s;
    }
  }
  __syncthreads();
  {
    const int p = tid & 63, q = tid >> 6;
    const long long r = r0 + p;
    if (r < R) {
      float z = (red[(0 * 4 + q) * MD_TM + p] + red[(1 * 4 + q) * MD_TM + p]) + (red[(2 * 4 + q) * MD_TM + p] + red[(3 * 4 + q) * MD_TM + p]);
      if (bp) z += bp[scls[p]];
      const float pr = SIGMOID ? 1.f / (1.f + expf(-z)) : z;
      const int m = (int)(r / S2), rem = (int)(r - (long long)m * S2);
      const int yy = rem / S, xx = rem - yy * S;
      const int S_2 = 2 * S;
      prob[((size_t)m * S_2 + 2 * yy + (q >> 1)) * S_2 + 2 * xx + (q & 1)] = pr;
    }
  }
}

template <int NBC, bool SIGMOID>
static int launch_mask_deconv(const float* x, const float* wd, const float* bd, const float* wp, const float* bp, const int* classes,
                              const int* d_num_valid, int* d_status, float* prob, int M, int S, int Cin, int K, hipStream_t st) {
  const size_t lds = (size_t)MD_TM * (Cin + MD_PAD) * 4 + 4 * 4 * MD_TM * 4 + MD_TM * 4;
  // the attribute is set once per template instance and device, for the largest Cin (the per-batch path makes no runtime call for it)
  static bool lds_set[64] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = -1;
  if (dev < 0 || !lds_set[dev]) {
    const size_t lds_max = (size_t)MD_TM * (256 + MD_PAD) * 4 + 4 * 4 * MD_TM * 4 + MD_TM * 4;
    if (hipFuncSetAttribute((const void*)mask_deconv_kernel<NBC, SIGMOID>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_max) != hipSuccess) {
      (void)hipGetLastError();
      lvc_set_error("lvc_mask_deconv_%s: %zu bytes of LDS refused", SIGMOID ? "predict" : "logits", lds_max);
      return LVC_ERR_HIP;
    }
    if (dev >= 0) lds_set[dev] = true;
  }
  const long long rows = (long long)M * S * S;
  const unsigned blocks = (unsigned)((rows + MD_TM - 1) / MD_TM);
  hipLaunchKernelGGL((mask_deconv_kernel<NBC, SIGMOID>), dim3(blocks), dim3(256), lds, st, x, wd, bd, wp, bp, classes, d_num_valid, d_status, prob, M,
                     S, Cin, K);
  return LVC_OK;
}

template <bool SIGMOID>
static int mask_deconv_entry(const float* x, const float* w_deconv, const float* b_deconv, const float* w_pred, const float* b_pred,
                             const int* classes, const int* d_num_valid, float* prob, int M, int S, int Cin, int Cmid, int K, int* d_status,
                             void* stream) {
  LVC_CHECK_ARG(M >= 0 && S >= 1 && K >= 1, "M >= 0, S >= 1, K >= 1");
  LVC_CHECK_ARG(Cin >= 64 && Cin <= 256 && Cin % 64 == 0 && Cmid >= 64 && Cmid <= 256 && Cmid % 64 == 0,
                "channels of the deconvolution: multiples of 64 up to 256 (MODEL.ROI_MASK_HEAD.CONV_DIM)");
  if (M == 0) return LVC_OK;
  LVC_CHECK_ARG(x && w_deconv && w_pred && prob, "null pointer");
  LVC_CHECK_ARG((((uintptr_t)x | (uintptr_t)w_deconv | (uintptr_t)w_pred | (uintptr_t)b_deconv) & 15) == 0, "16-byte aligned operands");
  LVC_CHECK_ARG((long long)M * S * S < (1LL << 31) - MD_TM && (long long)M * 4 * S * S < (1LL << 40), "too many rows");
  hipStream_t st = (hipStream_t)stream;
  int rc;
  switch (Cmid / 64) {
    case 1: rc = launch_mask_deconv<1, SIGMOID>(x, w_deconv, b_deconv, w_pred, b_pred, classes, d_num_valid, d_status, prob, M, S, Cin, K, st); break;
    case 2: rc = launch_mask_deconv<2, SIGMOID>(x, w_deconv, b_deconv, w_pred, b_pred, classes, d_num_valid, d_status, prob, M, S, Cin, K, st); break;
    case 3: rc = launch_mask_deconv<3, SIGMOID>(x, w_deconv, b_deconv, w_pred, b_pred, classes, d_num_valid, d_status, prob, M, S, Cin, K, st); break;
    default: rc = launch_mask_deconv<4, SIGMOID>(x, w_deconv, b_deconv, w_pred, b_pred, classes, d_num_valid, d_status, prob, M, S, Cin, K, st); break;
  }
  if (rc != LVC_OK) return rc;
  LVC_CHECK_LAUNCH();
  return LVC_OK;
}

extern "C" int lvc_mask_deconv_predict(const float* x, const float* w_deconv, const float* b_deconv, const float* w_pred,
                                       const float* b_pred, const int* classes, const int* d_num_valid, float* prob, int M, int S,
                                       int Cin, int Cmid, int K, int* d_status, void* stream) {
  return mask_deconv_entry<true>(x, w_deconv, b_deconv, w_pred, b_pred, classes, d_num_valid, prob, M, S, Cin, Cmid, K, d_status, stream);
}

// The training tail: the same launch with the RoI's GROUND-TRUTH class and without the sigmoid -- logits [M, 2S, 2S] for lvc_mask_loss
// and lvc_mask_deconv_grad (csrc/mask_train.hip).
extern "C" int lvc_mask_deconv_logits(const float* x, const float* w_deconv, const float* b_deconv, const float* w_pred,
                                      const float* b_pred, const int* classes, const int* d_num_valid, float* logits, int M, int S,
                                      int Cin, int Cmid, int K, int* d_status, void* stream) {
  return mask_deconv_entry<false>(x, w_deconv, b_deconv, w_pred, b_pred, classes, d_num_valid, logits, M, S, Cin, Cmid, K, d_status, stream);
}
