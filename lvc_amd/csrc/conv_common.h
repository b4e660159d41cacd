// conv_common.h -- what the convolution / GEMM kernels (conv_*.hip, conv3x3_*.hip, stem_pool_h2.hip, gemm_h.hip) share: vector types,
// the inline-asm load / wait helpers, the range check, the split-tile hand-off, the workspace layout and the worker split of the
// launchers.  Only what more than one file uses lives here; a kernel's own helpers stay in its file.
#pragma once
#include "common.h"

// ---------------------------------------------------------------------------------------------------------------- types
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16;
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) void* lds_ptr_t;
typedef const __attribute__((address_space(1))) void* glb_ptr_t;

// ---------------------------------------------------------------------------------------------------------------- workspace layout
// One caller-owned, once-zeroed workspace per stream (include/lvc_amd.h):
//   [LVC_MAX_WORKERS] partial accumulator tiles of LVC_WS_PARTIAL_BYTES (a kernel whose partial tile is twice that caps its workers
//                     at LVC_MAX_WORKERS / 2), then
//   [LVC_MAX_WORKERS] int32 worker flags (`flags`; 1 = that worker's partial tile is published), then
//   [LVC_RANGE_SLOTS] int32 range / error words: flags[LVC_MAX_WORKERS + slot], slot 0 = the shared word (lvc_set_range_slot).
#define LVC_MAX_WORKERS 1024
#define LVC_RANGE_SLOTS 1024
#define LVC_WS_PARTIAL_BYTES (256 * 128 * 4)
#define LVC_WS_FLAGS_OFFSET ((size_t)LVC_MAX_WORKERS * LVC_WS_PARTIAL_BYTES)
#define LVC_WS_RANGE_OFFSET (LVC_WS_FLAGS_OFFSET + (size_t)LVC_MAX_WORKERS * 4)
#define LVC_WS_BYTES (LVC_WS_RANGE_OFFSET + (size_t)LVC_RANGE_SLOTS * 4 + 256)
// diagnostics builds (*_TIMELINE) write their samples into the upper half of the partial tiles
#define LVC_WS_DIAG_OFFSET ((size_t)(LVC_MAX_WORKERS / 2) * LVC_WS_PARTIAL_BYTES)
static inline int* lvc_ws_flags(void* workspace) { return (int*)((char*)workspace + LVC_WS_FLAGS_OFFSET); }
static inline int lvc_ws_range_index(int slot) { return LVC_MAX_WORKERS + slot; }   // index into `flags` of range word `slot`

// ---------------------------------------------------------------------------------------------------------------- host launch helpers
extern "C" int lvc_cu_count(void);   // compute units of the current device, read once (256 if the query fails); common.cpp
// (lvc_patch_plan(), the patch decomposition switch of the 3x3 kernels, is public: include/lvc_amd.h states its values; common.cpp)

// Stream-K split of `units` equal work items over at most `cap` workers, none with fewer than `min_units` (except when there are
// fewer units than that): every worker gets units_per_worker contiguous units, the last one the remainder.
static inline void lvc_plan_workers(long long units, int cap, int min_units, int* units_per_worker, int* nworkers) {
  long long workers = (units + min_units - 1) / min_units;
  if (workers > cap) workers = cap;
  if (workers < 1) workers = 1;
  *units_per_worker = (int)((units + workers - 1) / workers);
  *nworkers = (int)((units + *units_per_worker - 1) / *units_per_worker);
}

// ---------------------------------------------------------------------------------------------------------------- range check
// The fp16-split kernels track the largest |activation| they split.  Single-accumulator forms scale activations by 2^4 before the
// split, so their limit is LVC_ACT_MAX; the two-accumulator forms take fp16's whole range.  Bits of a range / error word:
//   bit 0 (1): a stream-K worker timed out waiting for a partial tile (lvc_wait_partial);
//   bit 1 (2): a FINITE activation beyond the form's range;
//   bit 2 (4): a non-finite one (usually what an upstream layer that left ITS range in this pass handed down:
//              kernels.check_conv_error_word does not move this layer for it while another layer reports bit 1).
#define LVC_ACT_SCALE 16.f    // activations x 2^4 before the split
#define LVC_ACT_MAX 4094.f    // 65504 / 16
#define LVC_F16_MAX 65504.f
// lvc_report_range(flags, index, big, limit): a macro so that `flags` and `index` (kernel-argument fields at every call) are read
// only when the report fires, as in the hand-written form; as an inline function their loads move ahead of the branch and the
// generated code of conv_pw_w2 and of the stream-K Winograd kernels changes (scripts/kernel_isa_digest.sh).
#define lvc_report_range(flags, index, big, limit)                                             \
  do {                                                                                         \
    if (!((big) <= (limit))) atomicOr((flags) + (index), (big) < INFINITY ? 2 : 4);            \
  } while (0)

// ---------------------------------------------------------------------------------------------------------------- split-tile hand-off
// A tile whose k-range is split over several workers is finished by the worker that holds its k = 0 piece.  The others store
// their accumulators to their partial tile, then ALL threads `s_waitcnt vmcnt(0)` + barrier, then ONE thread publishes; the finisher
// has ONE thread wait, then a barrier, all threads add the tile, a barrier, and ONE thread hands the flag back.  The stores and adds
// themselves differ per kernel and live there.
#define LVC_SPIN_LIMIT (1 << 24)
__device__ __forceinline__ void lvc_publish_partial(int* flags, int worker) {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __hip_atomic_store(flags + worker, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// polls relaxed, acquires once; a worker that never publishes raises bit 0 of the launch's error word instead of hanging the device
__device__ __forceinline__ void lvc_wait_partial(int* flags, int worker, int err_index) {
  int spins = 0;
  while (__hip_atomic_load(flags + worker, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) {
    __builtin_amdgcn_s_sleep(4);
    if (++spins > LVC_SPIN_LIMIT) { atomicOr(flags + err_index, 1); break; }
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
}
__device__ __forceinline__ void lvc_release_partial(int* flags, int worker) {
  __hip_atomic_store(flags + worker, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---------------------------------------------------------------------------------------------------------------- asm / intrinsic helpers
// 16 bytes per lane global -> LDS without passing through registers (global_load_lds_dwordx4)
__device__ __forceinline__ void glds16(const void* g, void* l) {
  __builtin_amdgcn_global_load_lds((glb_ptr_t)g, (lds_ptr_t)l, 16, 0, 0);
}
template <int N> __device__ __forceinline__ void wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
// behind it: at most N vector-memory operations outstanding and every LDS operation of this wave complete
template <int N> __device__ __forceinline__ void wait_vm_lds() { asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(N) : "memory"); }

// buffer_load_dwordx4 the compiler does not track (it would wait for everything in flight, LDS-DMA and stores included, at the first
// use): out-of-range offsets return zeros.  THE RULE: such a load completes only through a COUNTED wait that is TIED to its
// destination registers (wait_tied, or wait_vm followed by an empty asm with "+v" on them), and the registers are used only behind
// it.  A spill or scratch copy of such a register would save it BEFORE its data has arrived -- silent corruption -- so the files that
// use these loads are under the Makefile's no-spill rule (NOSPILL_SRCS; conv_pw_s1.hip's exception is explained there).
__device__ __forceinline__ f32x4 load_untracked(u32x4 rsrc, unsigned voff, unsigned soff) {
  f32x4 v;
  asm volatile("buffer_load_dwordx4 %0, %1, %2, %3 offen" : "=v"(v) : "v"(voff), "s"(rsrc), "s"(soff) : "memory");
  return v;
}
template <int IMM> __device__ __forceinline__ f32x4 load_untracked(u32x4 rsrc, unsigned voff, unsigned soff) {   // + immediate offset
  f32x4 v;
  asm volatile("buffer_load_dwordx4 %0, %1, %2, %3 offen offset:%4" : "=v"(v) : "v"(voff), "s"(rsrc), "s"(soff), "n"(IMM) : "memory");
  return v;
}
// at most N vector-memory operations outstanding; the registers become usable only behind it
template <int N> __device__ __forceinline__ void wait_tied(f32x4& a, f32x4& b) {
  asm volatile("s_waitcnt vmcnt(%2)" : "+v"(a), "+v"(b) : "n"(N) : "memory");
}
template <int N> __device__ __forceinline__ void wait_tied(f32x4& a, f32x4& b, f32x4& c, f32x4& d) {
  asm volatile("s_waitcnt vmcnt(%4)" : "+v"(a), "+v"(b), "+v"(c), "+v"(d) : "n"(N) : "memory");
}
__device__ __forceinline__ u32x4 make_rsrc(const void* base, unsigned bytes) {
  const unsigned long long b = (unsigned long long)base;
  return u32x4{(unsigned)__builtin_amdgcn_readfirstlane((unsigned)b), (unsigned)__builtin_amdgcn_readfirstlane((unsigned)(b >> 32) & 0xffffu),
               (unsigned)__builtin_amdgcn_readfirstlane(bytes), 0x00020000u};
}
// The scalar offset of a store is ALWAYS the literal 0.  The compiler inserts the wait state a > 64-bit VMEM store needs before its
// data registers are overwritten only when soffset is not an SGPR (GCNHazardRecognizer::createsVALUHazard); gfx950 needs it with an
// SGPR soffset as well: with `buffer_store_dwordx4 v[172:175], .., s93 offen` followed directly by a write of v172, the lanes
// 12-15 of every 16 stored 0 instead of the value (scripts/dbg_chain.py found exactly the registers that were rewritten next).
__device__ __forceinline__ void store_b128(f32x4 v, __amdgpu_buffer_rsrc_t rsrc, unsigned voff) {
  __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), rsrc, voff, 0, 0);
}
// Range tracking pinned in program order (volatile asm): written as plain fmaxf the compiler sank these maxima far below the
// split, kept the raw input rows alive for them and SPILLED those registers right after the untracked loads were issued --
// i.e. before their data had arrived.
__device__ __forceinline__ void track_abs(float& big, float a, float b) {
  asm volatile("v_max3_f32 %0, %0, |%1|, |%2|" : "+v"(big) : "v"(a), "v"(b));
}
// two-way fp16 split of the two-accumulator forms: a = h + m 2^-11 up to fp32 rounding
__device__ __forceinline__ void split2h(float a, f16& h, f16& m) {
  h = (f16)a;
  m = (f16)((a - (float)h) * 2048.f);
}
