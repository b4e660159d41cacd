// keypoint.hip -- `score_lowres` of detectron2's KRCNNConvDeconvUpsampleHead (reference detectron2/modeling/roi_heads/keypoint_head.py
// `layers`): ConvTranspose2d(Cin, K, 4, stride 2, padding 1) + bias on channels-last RoI maps,
//
//   out[m, k, oy, ox] = b[k] + sum_ci sum_{ky,kx} x[m, iy, ix, ci] * W[ci, k, ky, kx],   oy = 2 iy - 1 + ky,  ox = 2 ix - 1 + kx
//
// written as planes [M, K, 2S, 2S]: the layout lvc_heatmaps_to_keypoints (csrc/keypoint_decode.hip) reads.
//
// What was chosen
//   * Four gathered products, one per output parity q = (oy & 1, ox & 1): an output pixel (2a + py, 2b + px) sums exactly four input
//     pixels, (a, b), (a + dy, b), (a, b + dx), (a + dy, b + dx) with dy = py ? +1 : -1 (dx likewise), each with ONE kernel tap, so the
//     layer is four [M S^2, 4 Cin] x [4 Cin, K] products.  The other form -- one [M S^2, Cin] x [Cin, 16 K] product and an overlap-add
//     of its 16 K columns -- has the same multiply count but every output would be the sum of four partial results of different
//     input pixels, across tile borders too; here a lane owns an output from the first product to the store, nothing is added between
//     lanes or workgroups and there are no atomics: two runs are bit-identical.
//   * Arithmetic: v_mfma_f32_16x16x4_f32 on fp32 operands, as mask_deconv.hip: exact products, fp32 accumulation, range-free (no
//     range word, no tier).  The outputs decide an argmax, so the fp32 accumulation chains are kept short and are joined in fp64:
//     the four MFMA steps of a 16-channel chunk go to four accumulators (step t takes channels 16 kc + 4 kq + t, so a chain holds a
//     quarter of a tap's channels), and after each tap the four chains are added, in a fixed order, to an fp64 running total; the
//     bias joins it in fp64 and the total is rounded to fp32 once, at the store.  (An MFMA is a chain of fused multiply-adds in k
//     order -- restated on the CPU, its fp32 bits are reproduced --, so one accumulator for a 16-channel map rounds 16 times at
//     the result's magnitude and once more for the bias: up to 0.9 ulp measured where this form stays within 0.25.)
//   * Tiling: a workgroup (8 waves) owns 64 rows (input pixels of consecutive RoIs; a tile may straddle RoIs) and one tile of 32
//     output channels; waves q and q + 4 compute parity q for 32 rows each (with all 64 rows a wave needs 366 registers and runs
//     alone on its SIMD: 1.83 ms for 800 RoIs).  D[16 k][16 pixels] += A[16 k][4 ci] * B[4 ci][16 pixels]; lane
//     group kq takes channels 16 kc + 4 kq + t in step t, so one 16-byte read per operand feeds four steps.  Activations are read
//     from global memory (the waves of a workgroup read the same 3x3 neighbourhoods, and the two waves of a parity the same weights: L1 / L2 hits); weights from the packed
//     operand [4 parities][4 taps][Kp][Cin], Kp = K rounded up to 32 with zero rows, so no weight read needs a bound.
//   * Rows past *d_num_valid are neither read nor written; a neighbour of a real pixel lies in the same RoI, so it is real too.
#include "conv_common.h"
#include "rows_common.h"

#define KD_TM 64      // rows (input pixels) per workgroup
#define KD_TN 32      // output channels per workgroup (two 16-channel blocks)
#define KD_G 4        // 16-channel chunks per loop iteration (and per prefetch)
#define KD_PB 2       // 16-pixel blocks per wave: eight waves, two per parity, each with half of the workgroup's rows

__global__ __launch_bounds__(512) void keypoint_deconv_kernel(const float* __restrict__ x, const float* __restrict__ wpk,
                                                              const float* __restrict__ bias, const int* __restrict__ d_num_valid,
                                                              float* __restrict__ out, int M, int S, int Cin, int K, int Kp) {
  const int tid = threadIdx.x, lane = tid & 63, q = (tid >> 6) & 3, half = tid >> 8;
  const int j = lane & 15, kq = lane >> 4;
  const int py = q >> 1, px = q & 1;
  const int S2 = S * S;
  const int Mv = lvc_valid_rows(d_num_valid, M);
  const long long R = (long long)Mv * S2;
  const long long r0 = (long long)blockIdx.x * KD_TM;
  if (r0 >= R) return;      // (uniform) rows past num_valid are neither read nor written
  const int k0 = blockIdx.y * KD_TN;

  // the input pixel of every (pixel block, tap) this lane feeds: a row index (the entry keeps M S^2 below 2^31), or -1 for a tap
  // outside the map or a row past R
  int pix[KD_PB][4];
#pragma unroll
  for (int pb = 0; pb < KD_PB; ++pb) {
    const long long r = r0 + (half * KD_PB + pb) * 16 + j;
    const long long m = r / S2;
    const int rem = (int)(r - m * S2);
    const int a = rem / S, b = rem - a * S;
#pragma unroll
    for (int tap = 0; tap < 4; ++tap) {
      const int iy = a + ((tap >> 1) ? (py ? 1 : -1) : 0);
      const int ix = b + ((tap & 1) ? (px ? 1 : -1) : 0);
      const bool in = r < R && iy >= 0 && iy < S && ix >= 0 && ix < S;
      pix[pb][tap] = in ? (int)(m * S2 + (long long)iy * S + ix) : -1;
    }
  }

  double tot[KD_PB][2][4];
#pragma unroll
  for (int pb = 0; pb < KD_PB; ++pb)
#pragma unroll
    for (int nb = 0; nb < 2; ++nb)
#pragma unroll
      for (int e = 0; e < 4; ++e) tot[pb][nb][e] = 0.;

  const int kcn = Cin >> 4;
#pragma unroll 1
  for (int tap = 0; tap < 4; ++tap) {
    f32x4 acc[4][KD_PB][2];      // [MFMA step t][pixel block][channel block]
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int pb = 0; pb < KD_PB; ++pb)
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) acc[t][pb][nb] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float* wrow = wpk + ((size_t)(q * 4 + tap) * Kp + k0 + j) * Cin + kq * 4;
    const float* xrow[KD_PB];
#pragma unroll
    for (int pb = 0; pb < KD_PB; ++pb) {
      int p = 0;
#pragma unroll
      for (int t = 0; t < 4; ++t) p = tap == t ? pix[pb][t] : p;
      xrow[pb] = p >= 0 ? x + (size_t)p * Cin + kq * 4 : nullptr;
    }
    // KD_G chunks per iteration; the NEXT group's operands are requested before this group's 64 MFMAs are issued: the loads'
    // latency (L2 and beyond) hides behind them.  One chunk ahead, 16 MFMAs, did not cover it: 1.72 ms for 800 RoIs
    f32x4 a[KD_G][2], b[KD_G][KD_PB];
    auto load_group = [&](int kc0, f32x4 (&ra)[KD_G][2], f32x4 (&rb)[KD_G][KD_PB]) {
#pragma unroll
      for (int g = 0; g < KD_G; ++g) {
        const int kc = kc0 + g;
        const bool live = kc < kcn;      // (uniform) past the end nothing is read: zeros, which add nothing
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) {
          ra[g][nb] = f32x4{0.f, 0.f, 0.f, 0.f};
          if (live) ra[g][nb] = *reinterpret_cast<const f32x4*>(wrow + (size_t)nb * 16 * Cin + kc * 16);
        }
#pragma unroll
        for (int pb = 0; pb < KD_PB; ++pb) {
          rb[g][pb] = f32x4{0.f, 0.f, 0.f, 0.f};
          if (live && xrow[pb]) rb[g][pb] = *reinterpret_cast<const f32x4*>(xrow[pb] + kc * 16);
        }
      }
    };
    load_group(0, a, b);
    for (int kc = 0; kc < kcn; kc += KD_G) {
      f32x4 an[KD_G][2], bn[KD_G][KD_PB];
      load_group(kc + KD_G, an, bn);
#pragma unroll
      for (int g = 0; g < KD_G; ++g)
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
          for (int nb = 0; nb < 2; ++nb)
#pragma unroll
            for (int pb = 0; pb < KD_PB; ++pb)
              acc[t][pb][nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[g][nb][t], b[g][pb][t], acc[t][pb][nb], 0, 0, 0);
#pragma unroll
      for (int g = 0; g < KD_G; ++g) {
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) a[g][nb] = an[g][nb];
#pragma unroll
        for (int pb = 0; pb < KD_PB; ++pb) b[g][pb] = bn[g][pb];
      }
    }
#pragma unroll
    for (int pb = 0; pb < KD_PB; ++pb)
#pragma unroll
      for (int nb = 0; nb < 2; ++nb)
#pragma unroll
        for (int e = 0; e < 4; ++e)
          tot[pb][nb][e] += ((double)acc[0][pb][nb][e] + (double)acc[1][pb][nb][e]) + ((double)acc[2][pb][nb][e] + (double)acc[3][pb][nb][e]);
  }

  // the lane holds k = k0 + nb 16 + 4 kq + e of input pixel (half KD_PB + pb) 16 + j
  const int S_2 = 2 * S;
#pragma unroll
  for (int pb = 0; pb < KD_PB; ++pb) {
    const long long r = r0 + (half * KD_PB + pb) * 16 + j;
    if (r >= R) continue;
    const long long m = r / S2;
    const int rem = (int)(r - m * S2);
    const int a = rem / S, b = rem - a * S;
    const size_t pos = (size_t)(2 * a + py) * S_2 + 2 * b + px;
#pragma unroll
    for (int nb = 0; nb < 2; ++nb)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int k = k0 + nb * 16 + kq * 4 + e;
        if (k < K) out[((size_t)m * K + k) * S_2 * S_2 + pos] = (float)(tot[pb][nb][e] + (bias ? (double)bias[k] : 0.));
      }
  }
}

// ConvTranspose2d weight [Cin, K, 4, 4] -> [4 parities][4 taps][Kp][Cin] (zero rows for k >= K): parity q = py*2 + px, tap = ty*2 + tx;
// the kernel row of tap ty under parity py is ky = py ? (ty ? 0 : 2) : (ty ? 3 : 1) (kx likewise)
__global__ void keypoint_deconv_pack_kernel(const float* __restrict__ w, float* __restrict__ wpk, int Cin, int K, int Kp) {
  const long long n = 16LL * Kp * Cin;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const int ci = (int)(i % Cin);
    const long long rest = i / Cin;
    const int k = (int)(rest % Kp), qt = (int)(rest / Kp);
    const int q = qt >> 2, tap = qt & 3;
    const int py = q >> 1, px = q & 1, ty = tap >> 1, tx = tap & 1;
    const int ky = py ? (ty ? 0 : 2) : (ty ? 3 : 1);
    const int kx = px ? (tx ? 0 : 2) : (tx ? 3 : 1);
    wpk[i] = k < K ? w[(((size_t)ci * K + k) * 4 + ky) * 4 + kx] : 0.f;
  }
}

static int kd_check(int Cin, int K) { return Cin >= 16 && Cin % 16 == 0 && Cin <= 4096 && K >= 1 && K <= 64; }

extern "C" int lvc_keypoint_deconv_packed_rows(int K) { return K < 1 ? 0 : 16 * ((K + KD_TN - 1) / KD_TN * KD_TN); }

extern "C" int lvc_keypoint_deconv_pack(const float* weight, float* packed, int Cin, int K, void* stream) {
  LVC_CHECK_ARG(kd_check(Cin, K), "Cin: a multiple of 16 up to 4096; 1 <= K <= 64");
  LVC_CHECK_ARG(weight && packed, "null pointer");
  const int Kp = (K + KD_TN - 1) / KD_TN * KD_TN;
  const long long n = 16LL * Kp * Cin;
  const unsigned blocks = (unsigned)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
  hipLaunchKernelGGL(keypoint_deconv_pack_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, weight, packed, Cin, K, Kp);
  LVC_CHECK_LAUNCH();
  return LVC_OK;
}

extern "C" int lvc_keypoint_deconv(const float* x, const float* packed, const float* bias, const int* d_num_valid, float* out, int M,
                                   int S, int Cin, int K, void* stream) {
  LVC_CHECK_ARG(M >= 0 && S >= 1 && S <= 1024, "M >= 0, 1 <= S <= 1024");
  LVC_CHECK_ARG(kd_check(Cin, K), "Cin: a multiple of 16 up to 4096; 1 <= K <= 64");
  if (M == 0) return LVC_OK;
  LVC_CHECK_ARG(x && packed && out, "null pointer");
  LVC_CHECK_ARG((((uintptr_t)x | (uintptr_t)packed) & 15) == 0, "16-byte aligned operands");
  LVC_CHECK_ARG((long long)M * S * S < (1LL << 31) - KD_TM, "too many rows");
  const int Kp = (K + KD_TN - 1) / KD_TN * KD_TN;
  const long long rows = (long long)M * S * S;
  hipLaunchKernelGGL(keypoint_deconv_kernel, dim3((unsigned)((rows + KD_TM - 1) / KD_TM), (unsigned)(Kp / KD_TN)), dim3(512), 0,
                     (hipStream_t)stream, x, packed, bias, d_num_valid, out, M, S, Cin, K, Kp);
  LVC_CHECK_LAUNCH();
  return LVC_OK;
}
