// conv_grouped.hip -- the grouped 3x3 convolution of a ResNeXt bottleneck's conv2 (reference detectron2/modeling/backbone/resnet.py
// BottleneckBlock: Conv2d(groups=num_groups)), NHWC fp32, pad 1, stride 1 or 2, with its data- and weight-gradient operands.
//
// Shapes: G groups of cg input and cg output channels each (every ResNeXt conv2 has cg == kg), cg in {4, 8, 16, 32, 64},
// C = K = G * cg a multiple of 64.  Anything else is LVC_ERR_INVALID (the host names RESNETS.NUM_GROUPS / WIDTH_PER_GROUP).
//
// What was chosen
//   * Arithmetic: v_mfma_f32_16x16x4_f32 on fp32 operands -- exact fp32 products, fp32 accumulation.  The kernel is range-free
//     (an activation of 1e5 is an ordinary fp32 number), so it has no range word and takes no part in the tier re-routing: there
//     is no narrower tier to leave.  The layer has 1/32 of the dense layer's flops; at the trunk's shapes the fp32 matrix rate
//     (157 TF) puts it next to the time its bytes take, so the fp16x2 / bf16x3 splits (3 or 6 MFMAs and a VALU split per operand)
//     would trade exactness for nothing the memory system can use.
//   * GEMM shape: D[16 output channels][16 pixels] += A[16 oc][4 ic] * B[4 ic][16 pixels].  With cg >= 16 a 16-channel output
//     block contracts over its group's cg channels; with cg = 8 / 4 the block spans 2 / 4 groups and contracts over its own 16
//     channels with a block-diagonal A (zeros between groups, written by the packing kernel): one code path, at the cost of
//     2x / 4x idle multiplies on the two smallest widths, where the layer is furthest from the matrix pipe's limit.
//   * Memory: a workgroup owns a 64-channel slab (whole groups) and walks output tiles of 16 x 8 (stride 2: 16 x 3) pixels.  The
//     input tile with its halo is loaded ONCE into LDS with 16-byte loads along C (x is read once but for the halo ring, which
//     neighbouring tiles find in L2) and serves all nine taps; the whole weight set of a wave's output block sits in registers for
//     the life of the workgroup (9 * max(cg,16) / 4 floats per lane: 36 .. 144 VGPRs), so the tile loop reads only activations.
//     Each lane ends with 4 consecutive output channels of one pixel: scale / shift / residual / ReLU on float4, one 16-byte store.
//   * Data gradient: the SAME kernel on an operand packed with mode 1 (taps flipped, per-group transpose, times the FrozenBN
//     scale).  For a stride-2 layer the gradient is zero-stuffed onto the input grid first (lvc_scatter_stride2_nhwc) and the
//     stride-1 kernel runs on that: one extra pass over a tensor a quarter of x's size, no second kernel to keep exact.
//   * Weight gradient: D[16 oc][16 ic] += dy[4 pixels][16 oc]^T * x[4 pixels][16 ic] per tap, accumulators in registers across a
//     workgroup's pixel chunk; each chunk writes its partial [K][max(cg,16)][9] to the caller's scratch and a second kernel adds
//     the chunks in index order, applies the scale and writes OIHW.  No float atomics: two runs are bit-identical.
// Measured against it: PyTorch-ROCm's F.conv2d(groups=) in fp32, NCHW and channels_last, alternated in one process
// (scripts/bench_grouped_conv.py -> profiles/grouped_conv_bench.json), X-101-32x8d's shapes at 8 x 800 x 1333, forward ms ours / torch:
// res2 cg 8 0.661 / 1.474, res3 cg 16 0.404 / 0.523, res4 cg 32 0.346 / 0.221, res5 cg 64 0.354 / 0.222.  The two narrow-map shapes miss
// the yardstick: the time stops falling at ~0.35 ms (57 TF, 36 % of the fp32 matrix peak) -- one 4-byte LDS read per MFMA and a barrier
// pair per tile at one or two waves per SIMD bound it, not memory; a kernel trace (profiles/grouped_conv_kernel_trace.txt) shows the
// yardstick there to be MIOpen's assembly Winograd F(2,3), 2.25x fewer multiplies.  Next: 16-byte fragment reads, a double-buffered tile,
// Winograd along x for cg >= 32.
#include "conv_common.h"

#define GC_SLAB 64          // channels per workgroup: whole groups for every supported cg
#define GC_TW 16            // output pixels per tile row = the MFMA's 16 columns
#define GC_LDP 68           // floats per LDS pixel (forward): 64 + 4 -> the 16 pixels x 4 channels of a B fragment hit 64 banks
#define GC_LDW 80           // floats per LDS pixel (weight gradient): 64 + 16 -> 4 pixels x 16 channels of a fragment likewise

// ---------------------------------------------------------------------------------------------------------------- forward / dgrad
template <int KC, int STRIDE>      // KC = max(cg, 16): contraction channels of a 16-channel output block
__global__ __launch_bounds__(256) void conv3x3_grouped_kernel(const float* __restrict__ x, const float* __restrict__ wp,
                                                              const float* __restrict__ scale, const float* __restrict__ shift,
                                                              const float* __restrict__ res, float* __restrict__ y, int N, int H, int W,
                                                              int C, int Ho, int Wo, int relu, int ldo, int ldr, int tiles_x,
                                                              int tiles_y) {
  constexpr int TH = STRIDE == 1 ? 8 : 3;
  constexpr int IH = (TH - 1) * STRIDE + 3, IW = (GC_TW - 1) * STRIDE + 3;
  constexpr int KS = KC / 4;
  __shared__ __attribute__((aligned(16))) float sx[IH * IW * GC_LDP];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c0 = blockIdx.y * GC_SLAB;
  const int cb = ((wave * 16) / KC) * KC;      // first contraction channel of this wave's block, within the slab
  const int j = lane & 15, kq = lane >> 4;

  // this wave's whole operand: [tap][k-step] fragments of 64 floats, lane-major (lvc_pack_conv3x3_grouped)
  float wr[9 * KS];
  {
    const float* wsrc = wp + (size_t)((c0 >> 4) + wave) * (9 * KS * 64) + lane;
#pragma unroll
    for (int i = 0; i < 9 * KS; ++i) wr[i] = wsrc[i * 64];
  }
  const int oc = c0 + wave * 16 + kq * 4;      // the lane's 4 output channels
  f32x4 sc = {1.f, 1.f, 1.f, 1.f}, sh = {0.f, 0.f, 0.f, 0.f};
  if (scale) sc = *reinterpret_cast<const f32x4*>(scale + oc);
  if (shift) sh = *reinterpret_cast<const f32x4*>(shift + oc);

  const int per_image = tiles_x * tiles_y;
  const int ntiles = N * per_image;
  for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int n = t / per_image, rem = t - n * per_image;
    const int ty = rem / tiles_x, tx = rem - ty * tiles_x;
    const int oy0 = ty * TH, ox0 = tx * GC_TW;
    const int iy0 = oy0 * STRIDE - 1, ix0 = ox0 * STRIDE - 1;
    __syncthreads();      // the previous tile's fragment reads are done
    for (int idx = tid; idx < IH * IW * 16; idx += 256) {
      const int p = idx >> 4, c4 = idx & 15;
      const int py = p / IW, px = p - py * IW;
      const int iy = iy0 + py, ix = ix0 + px;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if ((unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W)
        v = *reinterpret_cast<const f32x4*>(x + (((size_t)n * H + iy) * W + ix) * C + c0 + c4 * 4);
      *reinterpret_cast<f32x4*>(sx + p * GC_LDP + c4 * 4) = v;
    }
    __syncthreads();
    f32x4 acc[TH];
#pragma unroll
    for (int m = 0; m < TH; ++m) acc[m] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float* sb = sx + (j * STRIDE) * GC_LDP + cb + kq;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int r = tap / 3, s = tap - r * 3;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
#pragma unroll
        for (int m = 0; m < TH; ++m) {
          const float b = sb[((m * STRIDE + r) * IW + s) * GC_LDP + ks * 4];
          acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(wr[tap * KS + ks], b, acc[m], 0, 0, 0);
        }
        // keep the scheduler from hoisting every fragment read of the tile above the first MFMA (it spilled the weights to do so)
        if ((ks & 3) == 3) __builtin_amdgcn_sched_barrier(0);
      }
    }
    const int ox = ox0 + j;
    if (ox < Wo) {
#pragma unroll
      for (int m = 0; m < TH; ++m) {
        const int oy = oy0 + m;
        if (oy < Ho) {
          const size_t pix = ((size_t)n * Ho + oy) * Wo + ox;
          f32x4 v = acc[m] * sc + sh;
          if (res) v += *reinterpret_cast<const f32x4*>(res + pix * ldr + oc);
          if (relu) {
            v[0] = v[0] > 0.f ? v[0] : 0.f; v[1] = v[1] > 0.f ? v[1] : 0.f;
            v[2] = v[2] > 0.f ? v[2] : 0.f; v[3] = v[3] > 0.f ? v[3] : 0.f;
          }
          *reinterpret_cast<f32x4*>(y + pix * ldo + oc) = v;
        }
      }
    }
  }
}

static bool grouped_cg_ok(int cg) { return cg == 4 || cg == 8 || cg == 16 || cg == 32 || cg == 64; }

template <int KC, int STRIDE>
static void launch_grouped(const float* x, const float* wp, const float* scale, const float* shift, const float* res, float* y, int N,
                           int H, int W, int C, int Ho, int Wo, int relu, int ldo, int ldr, hipStream_t st) {
  constexpr int TH = STRIDE == 1 ? 8 : 3;
  const int tiles_x = lvc_cdiv(Wo, GC_TW), tiles_y = lvc_cdiv(Ho, TH);
  const long long ntiles = (long long)N * tiles_x * tiles_y;
  const int slabs = C / GC_SLAB;
  // three workgroups per compute unit over all slabs; every workgroup keeps its weights and walks its share of the tiles
  long long gx = (3LL * lvc_cu_count() + slabs - 1) / slabs;
  if (gx > ntiles) gx = ntiles;
  if (gx < 1) gx = 1;
  hipLaunchKernelGGL((conv3x3_grouped_kernel<KC, STRIDE>), dim3((unsigned)gx, (unsigned)slabs), dim3(256), 0, st, x, wp, scale, shift, res, y,
                     N, H, W, C, Ho, Wo, relu, ldo, ldr, tiles_x, tiles_y);
}

extern "C" int lvc_conv3x3_grouped_nhwc(const float* x, const float* wp, const float* scale, const float* shift, const float* residual,
                                        float* y, int N, int H, int W, int C, int K, int groups, int stride, int relu, int res_mode,
                                        int ldy, int ldr, void* workspace, void* stream) {
  (void)workspace;      // range-free: no range word, no partial tiles
  LVC_CHECK_ARG(x && wp && y, "null pointer");
  LVC_CHECK_ARG(N > 0 && H > 0 && W > 0, "empty tensor (the host returns before a launch)");
  LVC_CHECK_ARG(groups > 0 && C == K && C % groups == 0, "grouped 3x3: in_channels == out_channels, divisible by groups");
  const int cg = C / groups;
  LVC_CHECK_ARG(grouped_cg_ok(cg) && C % GC_SLAB == 0, "grouped 3x3: channels per group must be 4, 8, 16, 32 or 64 and C a multiple of 64");
  LVC_CHECK_ARG(stride == 1 || stride == 2, "stride 1 or 2");
  LVC_CHECK_ARG(res_mode == 0 || (res_mode == 1 && residual), "residual of the output's shape only");
  if (ldy <= 0) ldy = K;
  if (ldr <= 0) ldr = K;
  LVC_CHECK_ARG((ldy & 3) == 0 && (ldr & 3) == 0 && ldy >= K && ldr >= K, "ldy, ldr: multiples of 4, at least K");
  const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
  LVC_CHECK_ARG((long long)N * lvc_cdiv(Wo, GC_TW) * lvc_cdiv(Ho, 3) < (1LL << 31), "too many tiles");
  const float* res = res_mode ? residual : nullptr;
  hipStream_t st = (hipStream_t)stream;
  const int kc = cg < 16 ? 16 : cg;
#define GC_GO(KC_)                                                                                              \
  do {                                                                                                          \
    if (stride == 1) launch_grouped<KC_, 1>(x, wp, scale, shift, res, y, N, H, W, C, Ho, Wo, relu, ldy, ldr, st); \
    else launch_grouped<KC_, 2>(x, wp, scale, shift, res, y, N, H, W, C, Ho, Wo, relu, ldy, ldr, st);             \
  } while (0)
  if (kc == 16) GC_GO(16); else if (kc == 32) GC_GO(32); else GC_GO(64);
#undef GC_GO
  LVC_CHECK_LAUNCH();
  return LVC_OK;
}

// ---------------------------------------------------------------------------------------------------------------- packing
// wp[((nb * 9 + tap) * KS + ks) * 64 + l]: the A fragment of output block nb (channels 16 nb ..), tap, k-step ks: lane l holds
// A[oc = 16 nb + l % 16][ic = cbase + 4 ks + l / 16], cbase = (16 nb / KC) KC; zero where oc and ic are in different groups.
//   mode 0: A = w[oc][ic % cg][tap]                       (forward)
//   mode 1: A = scale[ic] * w[ic][oc % cg][8 - tap]       (data gradient: oc is an INPUT channel of the layer, ic an output channel)
__global__ void pack_grouped_kernel(const float* __restrict__ w, const float* __restrict__ scale, float* __restrict__ wp, int K, int cg,
                                    int KC, int mode) {
  const long long total = (long long)K * 9 * KC;
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int KS = KC / 4;
  const int l = (int)(i & 63);
  long long f = i >> 6;
  const int ks = (int)(f % KS); f /= KS;
  const int tap = (int)(f % 9);
  const int nb = (int)(f / 9);
  const int oc = nb * 16 + (l & 15);
  const int ic = (nb * 16 / KC) * KC + ks * 4 + (l >> 4);
  float v = 0.f;
  if (oc / cg == ic / cg) {
    if (mode == 0) v = w[((size_t)oc * cg + ic % cg) * 9 + tap];
    else v = w[((size_t)ic * cg + oc % cg) * 9 + (8 - tap)] * (scale ? scale[ic] : 1.f);
  }
  wp[i] = v;
}

extern "C" long long lvc_conv3x3_grouped_packed_floats(int K, int groups) {
  if (groups <= 0 || K <= 0 || K % groups) return 0;
  const int cg = K / groups;
  return (long long)K * 9 * (cg < 16 ? 16 : cg);
}

extern "C" int lvc_pack_conv3x3_grouped(const float* w, const float* scale, float* wp, int K, int groups, int mode, void* stream) {
  LVC_CHECK_ARG(w && wp, "null pointer");
  LVC_CHECK_ARG(groups > 0 && K > 0 && K % groups == 0, "out_channels divisible by groups");
  const int cg = K / groups;
  LVC_CHECK_ARG(grouped_cg_ok(cg) && K % GC_SLAB == 0, "grouped 3x3: channels per group must be 4, 8, 16, 32 or 64 and K a multiple of 64");
  LVC_CHECK_ARG(mode == 0 || mode == 1, "mode 0 (forward) or 1 (data gradient)");
  const int KC = cg < 16 ? 16 : cg;
  const long long total = (long long)K * 9 * KC;
  hipLaunchKernelGGL(pack_grouped_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w, scale, wp, K, cg, KC,
                     mode);
  LVC_CHECK_LAUNCH();
  return LVC_OK;
}

// ---------------------------------------------------------------------------------------------------------------- weight gradient
// part[chunk][oc][icl][tap], icl = ic - cbase(oc) in [0, KC): the chunk's sum over its tiles of dy[.., oc] * x[.. + tap, ic]
template <int KC, int STRIDE>
__global__ __launch_bounds__(256) void conv3x3_grouped_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                                    float* __restrict__ part, int N, int H, int W, int C, int Ho, int Wo,
                                                                    int lddy, int tiles_x, int tiles_y) {
  constexpr int TH = STRIDE == 1 ? 4 : 2;
  constexpr int IH = (TH - 1) * STRIDE + 3, IW = (GC_TW - 1) * STRIDE + 3;
  constexpr int NI = KC / 16;      // 16-channel input blocks of this wave's contraction range
  __shared__ __attribute__((aligned(16))) float sx[IH * IW * GC_LDW];
  __shared__ __attribute__((aligned(16))) float sd[TH * GC_TW * GC_LDW];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c0 = blockIdx.y * GC_SLAB;
  const int cb = ((wave * 16) / KC) * KC;
  const int j = lane & 15, kq = lane >> 4;
  f32x4 acc[NI][9];
#pragma unroll
  for (int i = 0; i < NI; ++i)
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) acc[i][tap] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int per_image = tiles_x * tiles_y;
  const int ntiles = N * per_image;
  for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int n = t / per_image, rem = t - n * per_image;
    const int ty = rem / tiles_x, tx = rem - ty * tiles_x;
    const int oy0 = ty * TH, ox0 = tx * GC_TW;
    const int iy0 = oy0 * STRIDE - 1, ix0 = ox0 * STRIDE - 1;
    __syncthreads();
    for (int idx = tid; idx < IH * IW * 16; idx += 256) {
      const int p = idx >> 4, c4 = idx & 15;
      const int py = p / IW, px = p - py * IW;
      const int iy = iy0 + py, ix = ix0 + px;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if ((unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W)
        v = *reinterpret_cast<const f32x4*>(x + (((size_t)n * H + iy) * W + ix) * C + c0 + c4 * 4);
      *reinterpret_cast<f32x4*>(sx + p * GC_LDW + c4 * 4) = v;
    }
    for (int idx = tid; idx < TH * GC_TW * 16; idx += 256) {
      const int p = idx >> 4, c4 = idx & 15;
      const int py = p / GC_TW, px = p - py * GC_TW;
      const int oy = oy0 + py, ox = ox0 + px;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (oy < Ho && ox < Wo) v = *reinterpret_cast<const f32x4*>(dy + (((size_t)n * Ho + oy) * Wo + ox) * lddy + c0 + c4 * 4);
      *reinterpret_cast<f32x4*>(sd + p * GC_LDW + c4 * 4) = v;
    }
    __syncthreads();
    // k-steps of 4 consecutive output pixels of one tile row: A[oc = j][pixel kq] from sd, B[pixel kq][ic = j] from sx at the tap
#pragma unroll
    for (int m = 0; m < TH; ++m) {
#pragma unroll
      for (int q = 0; q < GC_TW / 4; ++q) {
        const int px = q * 4 + kq;
        const float a = sd[(m * GC_TW + px) * GC_LDW + wave * 16 + j];
#pragma unroll
        for (int i = 0; i < NI; ++i) {
#pragma unroll
          for (int tap = 0; tap < 9; ++tap) {
            const int r = tap / 3, s = tap - r * 3;
            const float b = sx[((m * STRIDE + r) * IW + px * STRIDE + s) * GC_LDW + cb + i * 16 + j];
            acc[i][tap] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc[i][tap], 0, 0, 0);
          }
        }
      }
    }
  }
  // D[oc = 4 kq + e][ic = j]
  const int K = C;
  float* dst = part + (size_t)blockIdx.x * K * KC * 9;
#pragma unroll
  for (int i = 0; i < NI; ++i)
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int oc = c0 + wave * 16 + kq * 4 + e;
        dst[((size_t)oc * KC + i * 16 + j) * 9 + tap] = acc[i][tap][e];
      }
}

// dw[oc][i][tap] = scale[oc] * sum over chunks, in chunk order, of part[chunk][oc][group base - cbase + i][tap]
__global__ void grouped_wgrad_reduce_kernel(const float* __restrict__ part, const float* __restrict__ scale, float* __restrict__ dw, int K,
                                            int cg, int KC, int chunks) {
  const long long total = (long long)K * cg * 9;
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int tap = (int)(idx % 9);
  const int i = (int)((idx / 9) % cg);
  const int oc = (int)(idx / (9 * cg));
  const int icl = (oc / cg) * cg - (oc / KC) * KC + i;
  const size_t per = (size_t)K * KC * 9;
  const float* src = part + ((size_t)oc * KC + icl) * 9 + tap;
  float s = 0.f;
  for (int c = 0; c < chunks; ++c) s += src[c * per];
  dw[idx] = scale ? s * scale[oc] : s;
}

static int grouped_wgrad_chunks(int N, int Ho, int Wo, int K, int cg, int stride) {
  const int KC = cg < 16 ? 16 : cg;
  const int TH = stride == 1 ? 4 : 2;
  const long long ntiles = (long long)N * lvc_cdiv(Wo, GC_TW) * lvc_cdiv(Ho, TH);
  // from the shape alone (the result does not depend on the device): at most 256 chunks, at most 64 MiB of partial sums
  long long chunks = (64LL << 20) / ((long long)K * KC * 9 * 4);
  if (chunks > 256) chunks = 256;
  if (chunks > ntiles) chunks = ntiles;
  if (chunks < 1) chunks = 1;
  return (int)chunks;
}

extern "C" long long lvc_conv3x3_grouped_wgrad_workspace_bytes(int N, int H, int W, int K, int groups, int stride) {
  if (groups <= 0 || K <= 0 || K % groups || N <= 0 || H <= 0 || W <= 0 || (stride != 1 && stride != 2)) return 0;
  const int cg = K / groups;
  const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
  return (long long)grouped_wgrad_chunks(N, Ho, Wo, K, cg, stride) * K * (cg < 16 ? 16 : cg) * 9 * 4;
}

template <int KC, int STRIDE>
static void launch_grouped_wgrad(const float* x, const float* dy, float* part, int N, int H, int W, int C, int Ho, int Wo, int lddy,
                                 int chunks, hipStream_t st) {
  constexpr int TH = STRIDE == 1 ? 4 : 2;
  hipLaunchKernelGGL((conv3x3_grouped_wgrad_kernel<KC, STRIDE>), dim3((unsigned)chunks, (unsigned)(C / GC_SLAB)), dim3(256), 0, st, x, dy, part,
                     N, H, W, C, Ho, Wo, lddy, lvc_cdiv(Wo, GC_TW), lvc_cdiv(Ho, TH));
}

extern "C" int lvc_conv3x3_grouped_wgrad_nhwc(const float* x, const float* dy, const float* scale, float* dw, int N, int H, int W, int C,
                                              int groups, int stride, int lddy, void* scratch, void* stream) {
  LVC_CHECK_ARG(x && dy && dw && scratch, "null pointer");
  LVC_CHECK_ARG(N > 0 && H > 0 && W > 0, "empty tensor (the host returns before a launch)");
  LVC_CHECK_ARG(groups > 0 && C % groups == 0, "channels divisible by groups");
  const int cg = C / groups;
  LVC_CHECK_ARG(grouped_cg_ok(cg) && C % GC_SLAB == 0, "grouped 3x3: channels per group must be 4, 8, 16, 32 or 64 and C a multiple of 64");
  LVC_CHECK_ARG(stride == 1 || stride == 2, "stride 1 or 2");
  if (lddy <= 0) lddy = C;
  LVC_CHECK_ARG((lddy & 3) == 0 && lddy >= C, "lddy: a multiple of 4, at least K");
  const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
  LVC_CHECK_ARG((long long)N * lvc_cdiv(Wo, GC_TW) * lvc_cdiv(Ho, 2) < (1LL << 31), "too many tiles");
  const int chunks = grouped_wgrad_chunks(N, Ho, Wo, C, cg, stride);
  const int kc = cg < 16 ? 16 : cg;
  hipStream_t st = (hipStream_t)stream;
  float* part = (float*)scratch;
#define GC_GO(KC_)                                                                                        \
  do {                                                                                                    \
    if (stride == 1) launch_grouped_wgrad<KC_, 1>(x, dy, part, N, H, W, C, Ho, Wo, lddy, chunks, st);       \
    else launch_grouped_wgrad<KC_, 2>(x, dy, part, N, H, W, C, Ho, Wo, lddy, chunks, st);                   \
  } while (0)
  if (kc == 16) GC_GO(16); else if (kc == 32) GC_GO(32); else GC_GO(64);
#undef GC_GO
  LVC_CHECK_LAUNCH();
  const long long total = (long long)C * cg * 9;
  hipLaunchKernelGGL(grouped_wgrad_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, part, scale, dw, C, cg, kc, chunks);
  LVC_CHECK_LAUNCH();
  return LVC_OK;
}
