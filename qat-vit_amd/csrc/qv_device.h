// Device primitives shared by the hand-written MFMA kernels of libqatvit (gfx950): vector types, LDS fences and barriers, counted waits,
// buffer descriptors and LDS-DMA, the swizzled LDS image offsets and the fragment reads that go with them.  Exactly one definition of each;
// include after qv_common.h.  Everything here is __device__ inline except allow_lds (host).
#pragma once
#include "qv_common.h"

namespace qv {

// ---------------------------------------------------------------- MFMA operand / accumulator vectors
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef int v4i32 __attribute__((ext_vector_type(4)));   // a raw buffer descriptor held in four SGPRs (make_rsrc_v)
typedef __attribute__((address_space(3))) void lds_void;
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;

// ---------------------------------------------------------------- fences, barriers, counted waits
// Workgroup barrier that orders LDS traffic only.  __syncthreads() also drains vmcnt: between epilogue slabs that is a wait for every
// global store of the slab just written to be acknowledged (and for LDS-DMA that was deliberately started early).
__device__ inline void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
// Wave-private hand-off through LDS: LDS is in order per wave, so no barrier is needed; the wait + memory clobber stop the compiler from
// reordering LDS accesses across the hand-off.
__device__ inline void wave_lds_fence() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }
template <int N> __device__ inline void wait_vmcnt() {
    static_assert(N >= 0 && N <= 20, "vmcnt immediate");
#define QV_W(n) if constexpr (N == n) asm volatile("s_waitcnt vmcnt(" #n ")" ::: "memory")
    QV_W(0); QV_W(1); QV_W(2); QV_W(3); QV_W(4); QV_W(5); QV_W(6); QV_W(7); QV_W(8); QV_W(9); QV_W(10);
    QV_W(11); QV_W(12); QV_W(13); QV_W(14); QV_W(15); QV_W(16); QV_W(17); QV_W(18); QV_W(19); QV_W(20);
#undef QV_W
}
// the wait that makes the asm-loaded fragments valid: nothing may be scheduled across it (hipcc moves register-only MFMAs past an asm
// s_waitcnt despite the memory clobber; sched_barrier(0) is the fence - cdna_hip_programming.md rule 18)
template <int N> __device__ inline void wait_vmcnt_b() {
    wait_vmcnt<N>();
    __builtin_amdgcn_sched_barrier(0);
}

// ---------------------------------------------------------------- buffer descriptors, LDS-DMA, asm loads
__device__ inline __amdgpu_buffer_rsrc_t make_rsrc(const void* base, int64_t bytes) {
    // wave-uniform descriptor: raw buffer, out-of-range (>= bytes) lanes load 0
    const uint32_t n = bytes > 0xffffffffll ? 0xffffffffu : (uint32_t)bytes;
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, n, 0x00020000);
}
// LDS-DMA through inline asm.  The TN kernel reads its fragments with the ds_read_tr16_b64 builtin; hipcc 7.2 cannot prove that such a
// read does not alias the LDS destination of a __builtin_amdgcn_raw_ptr_buffer_load_lds still in flight (another ring stage) and puts
// an s_waitcnt vmcnt(0) between every DMA issue and the next fragment read: no prefetch overlap at all.  (The same in front of every
// ordinary LDS read it cannot prove disjoint: the fp16 strip kernel's fragment reads of the next column tile.)  An asm DMA is invisible to
// that bookkeeping; completion is counted by hand (wait_vmcnt + s_barrier), exactly as the ring protocol requires anyway.
__device__ inline v4i32 make_rsrc_v(const void* base, int64_t bytes) {
    const uint64_t b = reinterpret_cast<uint64_t>(base);
    const uint32_t n = bytes > 0xffffffffll ? 0xffffffffu : (uint32_t)bytes;
    return (v4i32){(int)(uint32_t)b, (int)(uint32_t)(b >> 32), (int)n, 0x00020000};
}
// (m0 holds the wave-uniform LDS destination of the DMA; it is saved and restored around the load because the compiler does not see the asm use it)
__device__ inline void dma16_asm(v4i32 rsrc, const char* lds_dst, uint32_t voff) {
    const uint32_t m = __builtin_amdgcn_readfirstlane((uint32_t)reinterpret_cast<uintptr_t>((lds_void*)lds_dst));
    uint32_t keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %3, 0 offen lds\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(voff), "s"(m), "s"(rsrc)
                 : "memory");
}
// register-destination loads beside LDS-DMA: inline asm (hipcc waits vmcnt(0) for every ordinary load result while a DMA is in flight), counted by hand
__device__ inline v4i32 load16_asm(v4i32 rsrc, uint32_t voff) {
    v4i32 v;
    asm volatile("buffer_load_dwordx4 %0, %1, %2, 0 offen" : "=v"(v) : "v"(voff), "s"(rsrc) : "memory");
    return v;
}

// XCD-aware, bijective block-id remap: blocks b and b+8 share an XCD (and its L2), so give each
// XCD a contiguous run of tiles (neighbouring tiles share an A row panel).
__device__ inline int xcd_remap(int bid, int nwg) {
    const int q = nwg >> 3, r = nwg & 7, x = bid & 7;
    return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + (bid >> 3);
}

// ---------------------------------------------------------------- LDS images (byte offset of 16-B chunk `chunk` of row `row`)
// The XOR swizzles are applied on the DMA *source* address (the DMA destination is lane-linear) and on the fragment read, so that
// ds_read_b128 / ds_read_b64_tr_b16 of a whole wave are bank-conflict free.
// NT, BK = 64: [rows][64 bf16] tile, 128-B rows, 16-B chunk index XOR (row & 7).
__device__ inline int nt_off(int row, int chunk) { return row * 128 + ((chunk ^ (row & 7)) << 4); }
// NT, BK = 32: two 64-B tile rows share one 128-B LDS row; chunk index ((row & 1) * 4 + k-chunk) XOR (LDS row & 7).
__device__ inline int nt_off32(int row, int chunk) {
    const int R = row >> 1;
    return R * 128 + (((((row & 1) << 2) | chunk) ^ (R & 7)) << 4);
}
// A-stationary strips (i8strip.hip, f16strip.hip): one [rows][64 B] k-tile of A is the BK = 32 image.
__device__ inline int strip_off(int row, int chunk) { return nt_off32(row, chunk); }
// TN (wgrad): [64 rows (tokens)][128 bf16] tile for ds_read_b64_tr_b16: 256-B rows, chunk XOR.
__device__ inline int tn_sw(int row) { return ((row & 3) << 1) | (((row >> 3) & 1) << 3); }
__device__ inline int tn_off(int row, int chunk) { return row * 256 + ((chunk ^ tn_sw(row)) << 4); }
// attention: [tokens][HD] bf16 tile
template <int HD> __device__ inline int row_off(int row, int chunk) {   // for ds_read_b128 row fragments
    if constexpr (HD == 64) return row * 128 + ((chunk ^ (row & 7)) << 4);
    else return row * (HD * 2) + (chunk << 4);
}
template <int HD> __device__ inline int tr_off(int row, int chunk) {    // for ds_read_b64_tr_b16 blocks of 4 rows
    if constexpr (HD == 64) return row * 128 + ((chunk ^ (((row >> 1) & 3) << 1)) << 4);
    else return row * (HD * 2) + (chunk << 4);
}

// fragment of a tr_off image whose k-slots (g, j) are tokens tokA + 4g + (0..3) [j<4] and tokB + 4g + (0..3) [j>=4],
// and whose row/col index is feature col0 + (lane & 15)
template <int HD> __device__ inline bf16x8 tr_frag2(const char* img, int tokA, int tokB, int col0, int lane) {
    const int g = lane >> 4, idx = lane & 15, q = idx >> 2, pp = idx & 3;
    const int chunk = (col0 >> 3) + (pp >> 1);
    const s16x4 a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(img + tr_off<HD>(tokA + 4 * g + q, chunk) + (pp & 1) * 8));
    const s16x4 b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(img + tr_off<HD>(tokB + 4 * g + q, chunk) + (pp & 1) * 8));
    // whole-vector bit cast: per-element short->__bf16 inserts are miscompiled by hipcc 7.2 (every element becomes a[0])
    const s16x8 v = __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7);
    return __builtin_bit_cast(bf16x8, v);
}

// Re-tile half of one wave's 16 x HD fp32 accumulator block (MFMA layout: column on the lane, 4 rows per register group) through a private
// LDS scratch of 8 x (HD + 4) floats into row-major runs -> 16-B bf16 stores instead of 2-B scatters.  8 token rows at a time (2.1 KiB of
// scratch per wave instead of 4.3 KiB for the whole block): with it the attention forward and dQ kernels fit TWO workgroups per CU
// (LDS <= 80 KiB, <= 128 VGPRs), so one workgroup's staging phase overlaps the other's compute.
// half = 0: rows 0..7 (lanes with g < 2 hold them), half = 1: rows 8..15.  Afterwards lane (row = lane / (HD/8), c8 = lane % (HD/8))
// holds 8 consecutive features of token row 8*half + row.
template <int HD>
__device__ inline bool wave_retile8(float* sO, const f32x4 (&acc)[HD / 16], float scale, int lane, int half, float (&out)[8], int& row, int& c8) {
    constexpr int LDO = HD + 4;
    const int r = lane & 15, g = lane >> 4;
    if ((g >> 1) == half) {
#pragma unroll
        for (int jd = 0; jd < HD / 16; ++jd)
#pragma unroll
            for (int e = 0; e < 4; ++e) sO[(4 * (g & 1) + e) * LDO + 16 * jd + r] = acc[jd][e] * scale;
    }
    wave_lds_fence();
    row = lane / (HD / 8);
    c8 = lane % (HD / 8);
    const bool active = row < 8;
    if (active) {
        const float4 v0 = *reinterpret_cast<const float4*>(sO + row * LDO + 8 * c8), v1 = *reinterpret_cast<const float4*>(sO + row * LDO + 8 * c8 + 4);
        out[0] = v0.x; out[1] = v0.y; out[2] = v0.z; out[3] = v0.w; out[4] = v1.x; out[5] = v1.y; out[6] = v1.z; out[7] = v1.w;
    }
    wave_lds_fence();
    return active;
}

// ---------------------------------------------------------------- register pins of a float4
// An empty asm that "uses" loaded values right after a load loop: left alone, LLVM sinks part of the loads below the first conversions
// (or, with one `if (c < D)` region per column group, each group's loads to its uses): several dependent memory round trips instead of one.
// Two forms that do not generate the same code, hence two names: pin4 also "writes" the registers (in/out constraint), pin4_in only reads them.
__device__ inline void pin4(float4& v) { asm volatile("" : "+v"(v.x), "+v"(v.y), "+v"(v.z), "+v"(v.w)); }
__device__ inline void pin4_in(const float4& v) { asm volatile("" ::"v"(v.x), "v"(v.y), "v"(v.z), "v"(v.w)); }

// The weight fake-quant's straight-through rule, for every kernel that recomputes the STE mask from the fp32 weight: the gradient of weight value w is dropped unless
// its grid index rint(w * (1 / scale)) + zero point lies inside [qmin, qmax] (a NaN index is outside).
__device__ inline bool ste_clips(float w, float inv_scale, float fzp, int qmin, int qmax) {
    const float q = rintf(w * inv_scale) + fzp;
    return !(q >= (float)qmin && q <= (float)qmax);
}

// ---------------------------------------------------------------- host
// Raise a kernel's dynamic LDS limit above the 64 KiB default.  Once per kernel instantiation: call it from the initialiser of a function-local
// static next to the launch, `static bool once = (allow_lds(kernel<...>, bytes), true);`.
template <typename K>
static void allow_lds(K kernel, size_t bytes) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

}  // namespace qv
