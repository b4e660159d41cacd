// gemm_h.hip -- y [M, N] (fp32) = A [M, C] . B [N, C]^T on fp16 operands: the pre-filter GEMM of the two-stage kNN sweep
// (tools/run_nearest_neighbours.py:146-151 computes these similarities in fp32; here they only select the shots whose exact
// fp32 similarity lvc_knn_verify_topk_vote re-evaluates, see knn.hip).
//
// Shape of the kernel (one workgroup of 8 waves per CU, persistent over its tile list):
//   * 256 x 256 output tiles, wave grid 4 x 2, a wave owns 64 rows x 128 columns = 2 x 4 MFMA blocks of 32 x 32 (128
//     accumulator registers): per 32-deep chunk a wave reads 4 KB of A and 8 KB of B fragments for 16 MFMAs -- 96 KB of LDS
//     reads per chunk and workgroup against 2 x 512 matrix-pipe cycles per SIMD, the LDS port and the matrix pipe are about
//     level (the 8 x 1 wave grid of conv_pw_dma.hip reads 160 KB for the same work and is LDS-bound with one MFMA per block);
//   * operands arrive by `global_load_lds_dwordx4` into a ring of four 32 KB stages (A rows 0..255 then B rows 0..255, 64 bytes
//     per row and chunk), two to three chunks ahead, across tile boundaries; one s_barrier per chunk; fragments are read one
//     k16 step ahead of the MFMAs that use them;
//   * LDS images are lane-linear; the four 16-byte granules of a row are permuted with slot = G ^ ((row >> 2) & 3) on the
//     source side and on the fragment-read side, so that a 16-lane group of a ds_read_b128 covers the 64 banks once;
//   * row tiles are dealt to XCDs (tile_m % 8 == blockIdx % 8) and a workgroup walks (row tile, column tile) pairs of its XCD
//     with the column tile fastest: an A tile leaves HBM once and is shared through that XCD's L2;
//   * the epilogue stores from the accumulators through a buffer descriptor (rows >= M, columns >= N dropped by the bounds
//     check) while the ring keeps the next tile's first chunks in flight.
#include "conv_common.h"
#include <stdlib.h>

#ifndef GH_NS
#define GH_NS 4
#endif
#define GH_A_BYTES (256 * 64)
#define GH_STAGE (2 * GH_A_BYTES)

struct GemmHArgs {
  const unsigned short* a;
  const unsigned short* b;
  float* y;
  int M, N, C, ldb, ldy, nk, tiles_m, tiles_n, nworkers, ngroup;
  unsigned y_bytes;
  int q15;      // 1: y is int16, y[m][n] = rint(32766 * value) clamped to +-32766 (cosine similarities), NaN -> 32767
};

__global__ __launch_bounds__(512, 1) void gemm_f16_dma_kernel(GemmHArgs p) {
  __shared__ __attribute__((aligned(1024))) unsigned char smem[GH_NS * GH_STAGE];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int fi = lane & 31, fh = lane >> 5;
  const int fx3 = (fi >> 2) & 3;

  const int xcd = blockIdx.x & 7, local = blockIdx.x >> 3, per_xcd = p.nworkers >> 3;
  const int ntl = ((p.tiles_m - xcd + 7) >> 3) * p.tiles_n;   // tiles of this XCD: row tiles xcd, xcd + 8, ... x all column tiles
  if (local >= ntl) return;

  // ---- loader: this wave DMAs rows [wave*32, wave*32 + 32) of the A image and of the B image of every chunk (2 + 2 instructions
  // of 16 rows x 64 bytes); lane -> row lane / 4, LDS slot lane % 4, source granule slot ^ ((row >> 2) & 3)
  const unsigned short* asrc[2];
  const unsigned short* bsrc[2];
  int l_u = local, l_kc = 0;
  bool l_done = false;
  // tile u of this XCD's list -> (row tile, column tile).  The column tiles are taken in groups of p.ngroup: within a group the
  // row tiles of the XCD go by with the group's columns fastest, so the workgroups of an XCD that run side by side share
  // p.ngroup B tiles (resident in that XCD's L2) and 32 / p.ngroup A tiles; A crosses the fabric once per group
  const int mx = (p.tiles_m - xcd + 7) >> 3;
  auto tile_of = [&](int u, int& tm, int& tn) {
    const int full = mx * p.ngroup;
    const int ng = (p.tiles_n + p.ngroup - 1) / p.ngroup;
    int g = u / full;
    g = g < ng - 1 ? g : ng - 1;
    const int r = u - g * full;
    const int w = min(p.ngroup, p.tiles_n - g * p.ngroup);
    const int ml = r / w;
    tm = ml * 8 + xcd;
    tn = g * p.ngroup + (r - ml * w);
  };
  auto loader_enter = [&](int u) {
    int tm, tn;
    tile_of(u, tm, tn);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int r = wave * 32 + j * 16 + (lane >> 2);
      const int G = (lane & 3) ^ ((r >> 2) & 3);
      int ra = tm * 256 + r, rb = tn * 256 + r;
      ra = ra < p.M ? ra : p.M - 1;      // rows past the end read a valid row; their outputs are never stored
      rb = rb < p.N ? rb : p.N - 1;
      asrc[j] = p.a + (size_t)ra * p.C + G * 8;
      bsrc[j] = p.b + (size_t)rb * p.ldb + G * 8;
    }
  };
  int issued = 0, landed = 0;   // chunks [0, landed) are known to have landed (a full drain happened after their issue)
  auto issue_chunk = [&]() {
    if (l_done) return;
    unsigned char* st = smem + (issued % GH_NS) * GH_STAGE;
    {
#pragma unroll
      for (int j = 0; j < 2; ++j) glds16(asrc[j] + l_kc * 32, st + (wave * 32 + j * 16) * 64);
#pragma unroll
      for (int j = 0; j < 2; ++j) glds16(bsrc[j] + l_kc * 32, st + GH_A_BYTES + (wave * 32 + j * 16) * 64);
    }
    ++issued;
    if (++l_kc == p.nk) {
      l_kc = 0;
      l_u += per_xcd;
      if (l_u < ntl) loader_enter(l_u);
      else l_done = true;
    }
  };
  // this wave's pieces of chunk g have landed: loads retire in order, only the 4 pieces of each younger chunk may be outstanding
  auto wait_landed = [&](int g) {
    if (g < landed) return;
    const int younger = issued - g - 1;
    if (younger >= 4) asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
    else if (younger == 3) asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
    else if (younger == 2) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    else if (younger == 1) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  };
  // the six fragments of a k16 step (2 row blocks of A + 4 column blocks of B).  They are read from LDS one step AHEAD of the
  // MFMAs that use them: after a barrier every wave of the workgroup is at the same point, so reading and multiplying the same
  // data would alternate "all waves on the LDS port" with "all waves on the matrix pipe"; one step ahead, the reads of the next
  // step travel under the eight MFMAs of this one.  Written as asm so that the scheduler cannot move the reads; a wait carries
  // the fragments (and the accumulator the preceding MFMAs end on) as operands, which pins the MFMAs on either side of it.
  // (Measured on the 120k x 2400 x 1024 sweep, round 2: the same 0.85 ms as the compiler-scheduled read-then-multiply loop; with
  // DMA and stores ablated the loop ran at 1.06 PFLOP/s, operand DMA and the output stores add 0.13 ms each.  Round 3 reading:
  // the kernel is bound by operand ingest -- 1 MB per 256 x 256 x 1024 tile at the ~20 - 25 GB/s a CU takes in -- not by the
  // matrix pipe, which sustains 1.54 PFLOP/s at this fragment-read ratio: profiles/r03_mfma_ceiling.txt)
  struct Half { f16x8 a[2]; f16x8 b[4]; };
  const unsigned a_off = (unsigned)((wm * 64 + fi) * 64), b_off = (unsigned)(GH_A_BYTES + (wn * 128 + fi) * 64);
  const unsigned bo0 = (unsigned)((fh ^ fx3) * 16), bo1 = (unsigned)(((2 + fh) ^ fx3) * 16);
  const unsigned smem_lds = (unsigned)(size_t)(lds_ptr_t)(void*)smem;
  auto read_half = [&](Half& h, int g, unsigned bo) {
    const unsigned st = smem_lds + (unsigned)(g % GH_NS) * GH_STAGE;
    const unsigned a0 = st + a_off + bo, b0 = st + b_off + bo;
#define GH_READ(dst, addr, off) asm volatile("ds_read_b128 %0, %1 offset:" #off : "=v"(dst) : "v"(addr))
    GH_READ(h.a[0], a0, 0); GH_READ(h.a[1], a0, 2048);
    GH_READ(h.b[0], b0, 0); GH_READ(h.b[1], b0, 2048); GH_READ(h.b[2], b0, 4096); GH_READ(h.b[3], b0, 6144);
#undef GH_READ
  };
  auto wait_half = [&](Half& h, f32x16& last) {
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(h.a[0]), "+v"(h.a[1]), "+v"(h.b[0]), "+v"(h.b[1]), "+v"(h.b[2]), "+v"(h.b[3]), "+v"(last));
  };

  const int total = ((ntl - local + per_xcd - 1) / per_xcd) * p.nk;   // chunks of this workgroup
  loader_enter(l_u);
  for (int i = 0; i < GH_NS; ++i) issue_chunk();

  const __amdgpu_buffer_rsrc_t yres = __builtin_amdgcn_make_buffer_rsrc((void*)p.y, 0, p.y_bytes, 0x00020000);
  const unsigned ldy4 = (unsigned)p.ldy * 4u;

  f32x16 acc[2][4];
  auto zero_acc = [&]() {
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[a][b][e] = 0.f;
  };
  zero_acc();
  int u = local, kc = 0;
  auto epilogue = [&]() {
    int tile_m, tile_n;
    tile_of(u, tile_m, tile_n);
    // The chunks prefetched so far are drained first and remembered as landed: the counted waits of the next chunks would
    // otherwise also wait for these stores (one vmcnt queue).  A store writes 2 rows x 32 consecutive columns.
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    landed = issued;
    const int m0 = tile_m * 256 + wm * 64, n0 = tile_n * 256 + wn * 128;
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) {
      const unsigned rbase = (unsigned)(m0 + mi * 32 + 4 * fh) * ldy4;
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) {
        const int col = n0 + ni * 32 + fi;
        if (p.q15) {
          // 16-bit fixed point (step 2^-15: 1.5e-5 of quantisation error against the pre-filter's own ~6e-4): half the bytes of the
          // matrix that this kernel writes and lvc_knn_verify_topk_vote_q15 reads back
          const unsigned cb16 = col < p.N ? (rbase >> 1) + (unsigned)col * 2u : 0x80000000u;
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            const float v = acc[mi][ni][e];
            // rint by the 1.5 x 2^23 trick: the low 16 bits of clamp(v, -1, 1) * 32766 + 12582912 are the rounded value in two's
            // complement (one fma instead of multiply, round, clamp, convert).  NaN takes the largest code so that it sorts first, as
            // in torch.topk; -32768 is never written ("no value" for the reader)
            const float c = __builtin_fminf(__builtin_fmaxf(v, -1.f), 1.f);
            const unsigned qv = v != v ? 32767u : __float_as_uint(__builtin_fmaf(c, 32766.f, 12582912.f));
            __builtin_amdgcn_raw_buffer_store_b16((short)qv, yres, cb16 + (unsigned)((e & 3) + 8 * (e >> 2)) * (ldy4 >> 1), 0, 0);
          }
          continue;
        }
        const unsigned cbase = col < p.N ? rbase + (unsigned)col * 4u : 0x80000000u;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const float v = acc[mi][ni][e];   // a scalar copy: __builtin_bit_cast on the vector element itself reads element 0
          __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), yres, cbase + (unsigned)((e & 3) + 8 * (e >> 2)) * ldy4, 0, 0);
        }
      }
    }
  };
  Half H0, H1;
  auto mfmas = [&](Half& h) {
#pragma unroll
    for (int ni = 0; ni < 4; ++ni)
#pragma unroll
      for (int mi = 0; mi < 2; ++mi) acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_f16(h.a[mi], h.b[ni], acc[mi][ni], 0, 0, 0);
  };
  wait_landed(0);
  __builtin_amdgcn_s_barrier();
  read_half(H0, 0, bo0);
  // step g: H0 holds (or is about to receive) the first k16 step of chunk g.  Before the barrier every wave has finished its
  // LDS reads of chunk g - 1 (so that slot can take chunk g - 1 + GH_NS) and its own DMA pieces of chunk g + 1 have landed.
#pragma unroll 1
  for (int g = 0; g < total; ++g) {
    const bool more = g + 1 < total;
    if (more) wait_landed(g + 1);
    __builtin_amdgcn_s_barrier();
    if (g > 0) issue_chunk();
    {
      wait_half(H0, acc[1][3]);
      read_half(H1, g, bo1);
      mfmas(H0);
      wait_half(H1, acc[1][3]);
      if (more) read_half(H0, g + 1, bo0);
      mfmas(H1);
    }
    if (++kc == p.nk) {
      epilogue();
      zero_acc();
      kc = 0;
      u += per_xcd;
    }
  }
}

static int gemm_f16_launch(const unsigned short* a, const unsigned short* b, int ldb, float* y, int M, int N, int C, int ldy,
                           void* stream, int q15 = 0) {
  LVC_CHECK_ARG(M >= 0 && N > 0 && C > 0, "bad shape");
  if (M == 0) return LVC_OK;
  LVC_CHECK_ARG(a && b && y, "null pointer");
  LVC_CHECK_ARG(C % 32 == 0, "needs C % 32 == 0");
  GemmHArgs g;
  g.a = a; g.b = b; g.y = y; g.M = M; g.N = N; g.C = C;
  g.ldb = ldb > 0 ? ldb : C;
  LVC_CHECK_ARG(g.ldb >= C && g.ldb % 8 == 0 && (((uintptr_t)a | (uintptr_t)b) & 15) == 0, "operands must be 16-byte aligned (ldb % 8 == 0)");
  g.ldy = ldy > 0 ? ldy : N;
  LVC_CHECK_ARG(g.ldy >= N, "ldy < N");
  const long long yb = (long long)M * g.ldy * (q15 ? 2 : 4);
  LVC_CHECK_ARG(yb < (1ll << 31), "output must be smaller than 2 GiB");
  LVC_CHECK_ARG(!q15 || g.ldy % 2 == 0, "16-bit rows must be 4-byte aligned");
  g.y_bytes = (unsigned)yb;
  g.q15 = q15;
  g.nk = C / 32;
  g.tiles_m = lvc_cdiv(M, 256);
  g.tiles_n = lvc_cdiv(N, 256);
  // measured on 120000 x 2400 x 1024 (scripts/probe_gemm_h_pmc.sh): all ten column tiles in one sweep 1.89 GB of fabric reads per
  // launch, groups of five 1.11 GB at the same speed (0.855 vs 0.861 ms), narrower groups no less traffic and 4 - 6 % slower
  g.ngroup = 5;
  if (g.ngroup > g.tiles_n) g.ngroup = g.tiles_n;
  g.nworkers = lvc_cu_count() / 8 * 8;
  if (g.nworkers < 8) g.nworkers = 8;
  hipLaunchKernelGGL(gemm_f16_dma_kernel, dim3(g.nworkers), dim3(512), 0, (hipStream_t)stream, g);
  LVC_CHECK_LAUNCH();
  return LVC_OK;
}

// a [M, C], b [N, ldb] (ldb >= C elements between rows; 0 = C): fp16 bit patterns, 16-byte aligned rows, C % 32 == 0;
// y [M, ldy] fp32 (ldy >= N), smaller than 2 GiB.  y[m][n] = sum_c a[m][c] * b[n][c] accumulated in fp32 (chunks of 32 in
// order, 16-wide MFMA steps inside).
extern "C" int lvc_gemm_f16(const unsigned short* a, const unsigned short* b, int ldb, float* y, int M, int N, int C, int ldy,
                            void* stream) {
  return gemm_f16_launch(a, b, ldb, y, M, N, C, ldy, stream);
}

// lvc_gemm_f16 with a 16-bit fixed-point result: y [M, ldy] int16, y[m][n] = rint(32766 * sum_c a[m][c] b[n][c]) clamped to +-32766,
// NaN -> 32767.  For operands with |dot product| <= 1 (unit-norm rows: the kNN pre-filter): |y / 32766 - dot| <= 1.6e-5 (a dot product
// that rounding pushed beyond +-1 is clamped TOWARDS the true value).  ldy even.
extern "C" int lvc_gemm_f16_q15(const unsigned short* a, const unsigned short* b, int ldb, short* y, int M, int N, int C, int ldy,
                                void* stream) {
  return gemm_f16_launch(a, b, ldb, (float*)y, M, N, C, ldy, stream, 1);
}
