// The classifier head of the three float (pre-QAT) student steps on MFMA (gfx950), for 128 .. 32768 classes: the second form of k_fs_head_fwd /
// k_fs_head_bwd (float_step.hip, fp32-accurate) and of k_fa_head_fwd / k_fa_head_bwd (float_amp.hip, fp16 / bf16), which walk the classes one
// after the other.  One body per kernel, a template on the element type E: float, _Float16 or __bf16.
//
// The arithmetic contract of the scalar kernels stays; only the summation order differs.
//   E = float      v_mfma_f32_16x16x4_f32: true fp32 products, fp32 accumulate.  No (hi, lo) planes of the head weight (it changes every step: a
//                  split pass would cost a read and a write of [C, D]), no dropped lo.lo term.  This MFMA runs at a fraction of the 16-bit rate: at
//                  21841 classes the kernels are MFMA-bound, not HBM-bound.
//   E = 16 bits    v_mfma_f32_16x16x32_f16 / _bf16.  W is read as fp32 from HBM once and rounded to E in registers while it is staged into LDS:
//                  no cast pass, no E copy of W anywhere.  hn holds E-representable fp32 values and converts exactly on load.
//
// k_fh_rows<E>: hn[b, :] = LN(x[b * T, :]) from the saved row statistics (16-bit forms: rounded to E, kept as fp32 values), as the scalar forward
// forms it.  launch_ln_bwd_fq and the backward read it.
//
// Forward, k_fh_fwd<E, STATS>: one workgroup per tile of classes - 32 in fp32, 64 in 16 bits, so that D = 768 stays under 100 KB of LDS.  It stages
// its [tile, D] slice of W in LDS ONCE (K = D whole, no ring; rows padded by 16 bytes: sixteen rows' 16-byte chunks then cover all banks) and walks
// the batch 64 rows at a time, one 16-row MFMA tile per wave; the A fragments are 16-byte loads of the L2-resident hn, rows clamped at B - 1.
// With fewer class tiles than CUs the row blocks are dealt over gridDim.y.  The fp32 form takes sixteen k as FOUR MFMAs whose k slots are
// {k0 + 4 g + i}: each lane reads four consecutive k of both operands with one 16-byte load (a sum does not care which MFMA a k lands in); the eight
// MFMAs of a 32-k step feed eight accumulators, folded pairwise behind the loop.
// The epilogue adds the bias, rounds once to E in the 16-bit forms, masks ragged class tiles and stores single elements ([B, C] rows have no
// alignment where C is odd).  STATS (the observe-only forward, fp32 form): min / max of acc + bias in registers over the walk, one stat_atomic per wave.
//
// Backward, k_fh_bwd<E, WGRAD>:
//   wgrad  dW[c, d] = sum_b dl[b, c] hn[b, d], dbias[c] = sum_b dl[b, c].  Workgroup = 32 classes, K = B whole in 32-row steps.  dl's k-run is
//          strided in memory, so its LDS image keeps the global [b][c] layout; the 16-bit forms take both fragments through ds_read_b64_tr_b16
//          (lane map as gemm.hip tr_frag), the fp32 form reads single dwords from images whose row strides spread the four k rows of a fragment
//          over the banks.  dbias is summed in fp32 from the staged values, eight fixed row groups folded in order.  Stores are "=".
//   dgrad  dhn[b, d] = sum_c dl[b, c] r(W[c, d]).  K = C is the long dimension: workgroup = (32 batch rows, a range of 32-class chunks), ranges
//          sized for a constant 256 workgroups so that the scratch size needs no device; the [32, D] accumulators stay in registers over the range,
//          the fp32 partial tile goes to scratch and k_fh_dgrad_reduce sums the ranges in range order and, in the 16-bit forms, rounds once to E
//          (fp16: beyond 65504 -> +-inf, as stock).  No atomics anywhere: two calls give the same bits.
// A k-step is staged, synchronised and consumed (no second LDS stage: DESIGN 7zh).  Nothing is read or written past B, C or D: out-of-range rows
// of a staged block are zero-filled, the forward clamps its A rows, the epilogues are masked.
#include <algorithm>
#include <type_traits>

#include "qv_common.h"
#include "qv_device.h"
#include "qv_kernels.h"

namespace qv {
namespace {

// the element type's pieces: the 16x16x32 MFMA and its fragment, two floats packed (one v_cvt_pk, round to nearest even), round and back
template <typename E> struct Fh;
template <> struct Fh<float> {
    static __device__ __attribute__((always_inline)) float r(float v) { return v; }
};
template <> struct Fh<_Float16> {
    typedef f16x8 v8;
    static __device__ __attribute__((always_inline)) f32x4 mfma(v8 a, v8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
    static __device__ __attribute__((always_inline)) uint32_t pk(float a, float b) { return pk_f16(a, b); }
    static __device__ __attribute__((always_inline)) float r(float v) { return (float)(_Float16)v; }
};
template <> struct Fh<__bf16> {
    typedef bf16x8 v8;
    static __device__ __attribute__((always_inline)) f32x4 mfma(v8 a, v8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
    static __device__ __attribute__((always_inline)) uint32_t pk(float a, float b) { return pk_bf16(a, b); }
    static __device__ __attribute__((always_inline)) float r(float v) { return (float)(__bf16)v; }
};
__device__ __attribute__((always_inline)) inline f32x4 mfma4(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
// eight consecutive fp32 values as eight E in 16 bytes (whole-vector bit casts only: qv_device.h tr_frag2)
template <typename E> __device__ inline uint4 pack8(const float4 a, const float4 b) {
    return make_uint4(Fh<E>::pk(a.x, a.y), Fh<E>::pk(a.z, a.w), Fh<E>::pk(b.x, b.y), Fh<E>::pk(b.z, b.w));
}

// [rows, D] fp32 rows r0 .. r0 + rows - 1 of X (zero beyond R) into an LDS image of row stride rowb bytes, as fp32 or rounded to E; D % 8 == 0
template <typename E>
__device__ inline void stage_rows(char* img, int rowb, const float* __restrict__ X, int r0, int R, int rows, int D) {
    if constexpr (std::is_same<E, float>::value) {
        const int cpr = D / 4;
        for (int i = threadIdx.x; i < rows * cpr; i += 256) {
            const int r = i / cpr, ch = i % cpr;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (r0 + r < R) v = *reinterpret_cast<const float4*>(X + (int64_t)(r0 + r) * D + ch * 4);
            *reinterpret_cast<float4*>(img + r * rowb + ch * 16) = v;
        }
    } else {
        const int cpr = D / 8;
        for (int i = threadIdx.x; i < rows * cpr; i += 256) {
            const int r = i / cpr, ch = i % cpr;
            float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
            if (r0 + r < R) {
                const float* src = X + (int64_t)(r0 + r) * D + ch * 8;
                a = *reinterpret_cast<const float4*>(src);
                b = *reinterpret_cast<const float4*>(src + 4);
            }
            *reinterpret_cast<uint4*>(img + r * rowb + ch * 16) = pack8<E>(a, b);
        }
    }
}

// ---------------------------------------------------------------- rows
template <typename E>
__global__ __launch_bounds__(256) void k_fh_rows(const float* __restrict__ x, const float* __restrict__ mean, const float* __restrict__ rstd,
                                                 const float* __restrict__ gamma, const float* __restrict__ beta, float* __restrict__ hn, int D, int T) {
    const int b = blockIdx.x;
    const int64_t row = (int64_t)b * T;
    const float mu = mean[row], rs = rstd[row];
    for (int c = threadIdx.x; c < D; c += 256) hn[(int64_t)b * D + c] = Fh<E>::r((x[row * D + c] - mu) * rs * gamma[c] + beta[c]);
}

// ---------------------------------------------------------------- forward
constexpr int kFwdRows = 64;   // batch rows per step: one 16-row tile per wave
constexpr int kFwdPad = 16;    // bytes behind each LDS row of the weight slice
template <typename E> constexpr int fwd_classes() { return std::is_same<E, float>::value ? 32 : 64; }   // classes per workgroup
template <typename E> constexpr size_t fwd_lds(int D) { return (size_t)fwd_classes<E>() * (D * sizeof(E) + kFwdPad); }

template <typename E, bool STATS>
__global__ __launch_bounds__(256) void k_fh_fwd(const float* __restrict__ hn, const float* __restrict__ W, const float* __restrict__ bias,
                                                E* __restrict__ logits, uint32_t* __restrict__ stats, int B, int D, int C) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr bool F32 = std::is_same<E, float>::value;
    constexpr int TILE = fwd_classes<E>(), NJ = TILE / 16;
    const int rowb = D * (int)sizeof(E) + kFwdPad;
    const int c0 = blockIdx.x * TILE;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, idx = lane & 15, g = lane >> 4;
    stage_rows<E>(smem, rowb, W, c0, C, TILE, D);
    __syncthreads();
    float bi[NJ];
    bool cv[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int c = c0 + 16 * j + idx;
        cv[j] = c < C;
        bi[j] = Fh<E>::r(bias[cv[j] ? c : C - 1]);
    }
    float mn = INFINITY, mx = -INFINITY;
    for (int r0 = blockIdx.y * kFwdRows; r0 < B; r0 += gridDim.y * kFwdRows) {
        const int rw = r0 + wave * 16;
        if (rw >= B) continue;   // (wave-uniform; no barrier below)
        const int ra = min(rw + idx, B - 1);
        f32x4 acc[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        if constexpr (F32) {
            // eight accumulation chains per class tile, folded pairwise at the end: sixteen independent MFMAs in flight, and each chain D / 32 steps long
            // instead of D / 4 (one chain's rounding error against fp64 grew to 4 x that of the scalar kernel's pairwise wave_sum)
            const float* arow = hn + (int64_t)ra * D + g * 4;
            f32x4 part[NJ][8];
#pragma unroll
            for (int j = 0; j < NJ; ++j)
#pragma unroll
                for (int q = 0; q < 8; ++q) part[j][q] = f32x4{0.f, 0.f, 0.f, 0.f};
            for (int kb = 0; kb < D; kb += 32) {
                const float4 a0 = *reinterpret_cast<const float4*>(arow + kb), a1 = *reinterpret_cast<const float4*>(arow + kb + 16);
#pragma unroll
                for (int j = 0; j < NJ; ++j) {
                    const char* wrow = smem + (16 * j + idx) * rowb + (kb + 4 * g) * 4;
                    const float4 w0 = *reinterpret_cast<const float4*>(wrow), w1 = *reinterpret_cast<const float4*>(wrow + 64);
                    part[j][0] = mfma4(a0.x, w0.x, part[j][0]);
                    part[j][1] = mfma4(a0.y, w0.y, part[j][1]);
                    part[j][2] = mfma4(a0.z, w0.z, part[j][2]);
                    part[j][3] = mfma4(a0.w, w0.w, part[j][3]);
                    part[j][4] = mfma4(a1.x, w1.x, part[j][4]);
                    part[j][5] = mfma4(a1.y, w1.y, part[j][5]);
                    part[j][6] = mfma4(a1.z, w1.z, part[j][6]);
                    part[j][7] = mfma4(a1.w, w1.w, part[j][7]);
                }
            }
#pragma unroll
            for (int j = 0; j < NJ; ++j)
                acc[j] = ((part[j][0] + part[j][1]) + (part[j][2] + part[j][3])) + ((part[j][4] + part[j][5]) + (part[j][6] + part[j][7]));
        } else {
            typedef typename Fh<E>::v8 v8;
            const float* arow = hn + (int64_t)ra * D + g * 8;
            for (int kk = 0; kk < D / 32; ++kk) {
                const float4 a0 = *reinterpret_cast<const float4*>(arow + kk * 32), a1 = *reinterpret_cast<const float4*>(arow + kk * 32 + 4);
                const v8 a = __builtin_bit_cast(v8, pack8<E>(a0, a1));   // (E-representable values: exact)
#pragma unroll
                for (int j = 0; j < NJ; ++j) {
                    const v8 w = *reinterpret_cast<const v8*>(smem + (16 * j + idx) * rowb + (kk * 4 + g) * 16);
                    acc[j] = Fh<E>::mfma(a, w, acc[j]);
                }
            }
        }
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int row = rw + 4 * g + e;
                if (row < B && cv[j]) {
                    const float v = acc[j][e] + bi[j];
                    logits[(int64_t)row * C + c0 + 16 * j + idx] = (E)v;
                    if constexpr (STATS) { mn = fminf(mn, v); mx = fmaxf(mx, v); }
                }
            }
        }
    }
    if constexpr (STATS) {
        mn = wave_min(mn);
        mx = wave_max(mx);
        if (lane == 0 && mn <= mx) stat_atomic(stats, kStatSlots, mn, mx);
    }
}

// ---------------------------------------------------------------- backward
constexpr int kBwdTile = 32;      // rows of the output tile (dgrad: batch rows, wgrad: classes) and of a k-step
constexpr int kMaxNT = 12;        // 16-column tiles per wave: D / 64 <= 12
constexpr int kDgradGrid = 256;   // workgroups the dgrad aims at: a constant, so that the scratch size needs no device
// bytes per LDS row of the dl image [32 batch rows][32 classes].  16 bits: 16 bytes of padding.  fp32, single-dword fragment reads: the wgrad reads four
// consecutive rows (k) x sixteen consecutive classes - 48 floats apart they take banks 0-15, 48-63, 32-47, 16-31; the dgrad reads sixteen rows (batch) x
// four consecutive classes (k) - 36 floats apart the rows start at sixteen different multiples of 4.
template <typename E, bool WGRAD> constexpr int a_row() { return std::is_same<E, float>::value ? (WGRAD ? 48 : 36) * 4 : 2 * kBwdTile + 16; }
// bytes per LDS row of the other operand's [32, D] block: 16 bits 32 bytes of padding (the transposed reads), fp32 16 floats (four consecutive k rows x
// sixteen consecutive columns cover all banks, D being a multiple of 64)
template <typename E> constexpr int b_row(int D) { return std::is_same<E, float>::value ? (D + 16) * 4 : 2 * D + 32; }
template <typename E, bool WGRAD> constexpr size_t bwd_lds(int D) {
    return (size_t)kBwdTile * b_row<E>(D) + (size_t)kBwdTile * a_row<E, WGRAD>() + 8 * kBwdTile * sizeof(float);   // fp32 at D = 768: 107520 bytes
}

struct FhBwdArgs {
    const void* dl;        // [B, C] of E
    const float* X;        // the other operand, fp32: dgrad W [C, D], wgrad hn [B, D]
    float* partial;        // dgrad: [splits][row tiles * 32][D]
    int chunks_per_split;
    float* dW; float* dbias;
    int B, D, C;
};

// 16x16x32 operand fragment out of a row-major LDS image of 16-bit elements whose k index runs over rows 8 g + (0..7) and whose row / column index is image
// column col0 + (lane & 15): two transposed 4 x 16 block reads (the lane map gemm.hip tr_frag, qv_device.h tr_frag2 and head_mfma.hip use)
template <typename E>
__device__ inline typename Fh<E>::v8 fh_tr_frag(const char* img, int rowb, int col0, int lane) {
    const int g = lane >> 4, idx = lane & 15, q = idx >> 2, pp = idx & 3;
    const char* p = img + (8 * g + q) * rowb + (col0 + 4 * pp) * 2;
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)p);
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(p + 4 * rowb));
    const s16x8 v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
    return __builtin_bit_cast(typename Fh<E>::v8, v);
}

template <typename E, bool WGRAD>
__global__ __launch_bounds__(256) void k_fh_bwd(const FhBwdArgs p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr bool F32 = std::is_same<E, float>::value;
    constexpr int kARow = a_row<E, WGRAD>();
    const int B = p.B, D = p.D, C = p.C;
    const int browb = b_row<E>(D);
    char* imgB = smem;
    char* imgA = smem + kBwdTile * browb;
    float* sdb = reinterpret_cast<float*>(imgA + kBwdTile * kARow);   // wgrad: [8 row groups][32 classes]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, idx = lane & 15, g = lane >> 4;
    const int ntw = D / 64;
    const E* dlp = reinterpret_cast<const E*>(p.dl);
    const int tile0 = blockIdx.x * kBwdTile;
    int k_lo = 0, k_hi;
    if constexpr (!WGRAD) {
        k_lo = blockIdx.y * p.chunks_per_split;
        k_hi = min((C + kBwdTile - 1) / kBwdTile, k_lo + p.chunks_per_split);
    } else {
        k_hi = (B + kBwdTile - 1) / kBwdTile;
    }
    f32x4 acc[2][kMaxNT];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int j = 0; j < kMaxNT; ++j) acc[mt][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    float db = 0.f;
    const int cl = threadIdx.x & 31, bs = threadIdx.x >> 5;
    for (int kc = k_lo; kc < k_hi; ++kc) {
        const int b0 = WGRAD ? kc * kBwdTile : tile0, c0 = WGRAD ? tile0 : kc * kBwdTile;
        const int c = c0 + cl;
        E gv[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int b = b0 + bs + 8 * i;
            gv[i] = (b < B && c < C) ? dlp[(int64_t)b * C + c] : (E)0.f;
        }
        stage_rows<E>(imgB, browb, p.X, WGRAD ? b0 : c0, WGRAD ? B : C, kBwdTile, D);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if constexpr (WGRAD) db += (float)gv[i];
            *reinterpret_cast<E*>(imgA + (bs + 8 * i) * kARow + cl * (int)sizeof(E)) = gv[i];
        }
        __syncthreads();
        if constexpr (F32) {
            const float* fa = reinterpret_cast<const float*>(imgA);
            const float* fb = reinterpret_cast<const float*>(imgB);
            constexpr int lda = kARow / 4;
            const int ldb = browb / 4;
            float af[2][8];   // k = 4 s + g
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int s = 0; s < 8; ++s) {
                    if constexpr (WGRAD) af[mt][s] = fa[(4 * s + g) * lda + 16 * mt + idx];   // row index = class, k = batch row
                    else af[mt][s] = fa[(16 * mt + idx) * lda + 4 * s + g];                   // row index = batch row, k = class
                }
#pragma unroll
            for (int j = 0; j < kMaxNT; ++j) {
                if (j < ntw) {
                    const int col = (wave * ntw + j) * 16 + idx;
                    float bv[8];
#pragma unroll
                    for (int s = 0; s < 8; ++s) bv[s] = fb[(4 * s + g) * ldb + col];
#pragma unroll
                    for (int s = 0; s < 8; ++s)
#pragma unroll
                        for (int mt = 0; mt < 2; ++mt) acc[mt][j] = mfma4(af[mt][s], bv[s], acc[mt][j]);
                }
            }
        } else {
            typedef typename Fh<E>::v8 v8;
            v8 af[2];
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) {
                if constexpr (WGRAD) af[mt] = fh_tr_frag<E>(imgA, kARow, 16 * mt, lane);                        // row index = class, k = batch row
                else af[mt] = *reinterpret_cast<const v8*>(imgA + (16 * mt + idx) * kARow + g * 16);           // row index = batch row, k = class
            }
#pragma unroll
            for (int j = 0; j < kMaxNT; ++j) {
                if (j < ntw) {
                    const v8 bf = fh_tr_frag<E>(imgB, browb, (wave * ntw + j) * 16, lane);
#pragma unroll
                    for (int mt = 0; mt < 2; ++mt) acc[mt][j] = Fh<E>::mfma(af[mt], bf, acc[mt][j]);
                }
            }
        }
        __syncthreads();
    }
    if constexpr (WGRAD) {
        sdb[bs * kBwdTile + cl] = db;
        __syncthreads();
        if (threadIdx.x < kBwdTile && tile0 + (int)threadIdx.x < C) {
            float s = sdb[threadIdx.x];
#pragma unroll
            for (int k = 1; k < 8; ++k) s += sdb[k * kBwdTile + threadIdx.x];
            p.dbias[tile0 + threadIdx.x] = s;
        }
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int c = tile0 + 16 * mt + 4 * g + e;
                if (c >= C) continue;
#pragma unroll
                for (int j = 0; j < kMaxNT; ++j)
                    if (j < ntw) p.dW[(int64_t)c * D + (wave * ntw + j) * 16 + idx] = acc[mt][j][e];
            }
    } else {
        const int64_t rows = (int64_t)gridDim.x * kBwdTile;
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int b = tile0 + 16 * mt + 4 * g + e;
                if (b >= B) continue;
#pragma unroll
                for (int j = 0; j < kMaxNT; ++j)
                    if (j < ntw) p.partial[((int64_t)blockIdx.y * rows + b) * D + (wave * ntw + j) * 16 + idx] = acc[mt][j][e];
            }
    }
}

// dhn = the class ranges' partial tiles summed in range order, rounded once to E in the 16-bit forms
template <typename E>
__global__ __launch_bounds__(256) void k_fh_dgrad_reduce(const float* __restrict__ partial, int splits, int64_t stride, float* __restrict__ dhn, int64_t n) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    float s = partial[i];
    for (int k = 1; k < splits; ++k) s += partial[k * stride + i];
    dhn[i] = Fh<E>::r(s);
}

struct DgradGeom { int row_tiles, splits, chunks_per_split; };
DgradGeom dgrad_geom(int B, int C) {
    DgradGeom q;
    q.row_tiles = cdiv(B, kBwdTile);
    const int chunks = cdiv(C, kBwdTile), want = std::min(chunks, std::max(1, kDgradGrid / q.row_tiles));
    q.chunks_per_split = cdiv(chunks, want);
    q.splits = cdiv(chunks, q.chunks_per_split);   // (no empty range)
    return q;
}

template <typename E>
void fh_forward(const float* x, const float* mean, const float* rstd, const float* gamma, const float* beta, const float* W, const float* bias, float* hn,
                void* logits, uint32_t* stats, int B, int D, int T, int C, hipStream_t st) {
    k_fh_rows<E><<<B, 256, 0, st>>>(x, mean, rstd, gamma, beta, hn, D, T);
    const int gx = cdiv(C, fwd_classes<E>());
    const dim3 grid(gx, std::min(cdiv(B, kFwdRows), std::max(1, cu_count() / gx)));
    if constexpr (std::is_same<E, float>::value) {
        static bool once = (allow_lds(k_fh_fwd<E, false>, fwd_lds<E>(768)), allow_lds(k_fh_fwd<E, true>, fwd_lds<E>(768)), true);
        (void)once;
        if (stats) {
            k_fh_fwd<E, true><<<grid, 256, fwd_lds<E>(D), st>>>(hn, W, bias, reinterpret_cast<E*>(logits), stats, B, D, C);
            return;
        }
    } else {
        static bool once = (allow_lds(k_fh_fwd<E, false>, fwd_lds<E>(768)), true);
        (void)once;
    }
    k_fh_fwd<E, false><<<grid, 256, fwd_lds<E>(D), st>>>(hn, W, bias, reinterpret_cast<E*>(logits), nullptr, B, D, C);
}

template <typename E>
void fh_backward(const void* dl, const float* hn, const float* W, float* dW, float* dbias, float* dhn, void* scratch, int B, int D, int C, hipStream_t st) {
    static bool once = (allow_lds(k_fh_bwd<E, false>, bwd_lds<E, false>(768)), allow_lds(k_fh_bwd<E, true>, bwd_lds<E, true>(768)), true);
    (void)once;
    const DgradGeom q = dgrad_geom(B, C);
    FhBwdArgs dg{};
    dg.dl = dl; dg.X = W; dg.partial = reinterpret_cast<float*>(scratch); dg.chunks_per_split = q.chunks_per_split; dg.B = B; dg.D = D; dg.C = C;
    k_fh_bwd<E, false><<<dim3(q.row_tiles, q.splits), 256, bwd_lds<E, false>(D), st>>>(dg);
    const int64_t n = (int64_t)B * D;
    k_fh_dgrad_reduce<E><<<cdiv(n, 256), 256, 0, st>>>(dg.partial, q.splits, (int64_t)q.row_tiles * kBwdTile * D, dhn, n);
    FhBwdArgs wg{};
    wg.dl = dl; wg.X = hn; wg.dW = dW; wg.dbias = dbias; wg.B = B; wg.D = D; wg.C = C;
    k_fh_bwd<E, true><<<cdiv(C, kBwdTile), 256, bwd_lds<E, true>(D), st>>>(wg);
}

bool fh_check(const char* fn, int B, int D, int C, int dtype) {
    if (dtype < kFloatHeadF32 || dtype > kFloatHeadBf16) { set_error("%s: dtype %d (0 fp32, 1 fp16, 2 bf16)", fn, dtype); return false; }
    if (!float_head_mfma_covers(D, C) || B < 1) {
        set_error("%s: B %d, D %d, C %d (needs B >= 1, D %% 64 == 0, D <= 768, %d <= C <= %d)", fn, B, D, C, kFloatHeadMinClasses, kFloatHeadMaxClasses);
        return false;
    }
    return true;
}
bool aligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

}  // namespace

bool float_head_mfma_covers(int D, int C) { return C >= kFloatHeadMinClasses && C <= kFloatHeadMaxClasses && D >= 64 && D % 64 == 0 && D <= 768; }

int64_t float_head_scratch_bytes(int B, int D, int C) {
    const DgradGeom q = dgrad_geom(B, C);
    return (int64_t)q.splits * q.row_tiles * kBwdTile * D * 4;
}

int launch_float_head_fwd(const float* x, const float* mean, const float* rstd, const float* gamma, const float* beta, const float* W, const float* bias,
                          float* hn, void* logits, uint32_t* stats, int B, int D, int T, int C, int dtype, hipStream_t st) {
    if (!fh_check("float_head_fwd", B, D, C, dtype)) return 1;
    if (stats && dtype != kFloatHeadF32) { set_error("float_head_fwd: stats belong to the fp32 form (dtype %d)", dtype); return 1; }
    if (!aligned16(W) || !aligned16(hn)) { set_error("float_head_fwd: the MFMA form needs W and hn 16-byte aligned"); return 1; }
    if (dtype == kFloatHeadF32) fh_forward<float>(x, mean, rstd, gamma, beta, W, bias, hn, logits, stats, B, D, T, C, st);
    else if (dtype == kFloatHeadF16) fh_forward<_Float16>(x, mean, rstd, gamma, beta, W, bias, hn, logits, nullptr, B, D, T, C, st);
    else fh_forward<__bf16>(x, mean, rstd, gamma, beta, W, bias, hn, logits, nullptr, B, D, T, C, st);
    return 0;
}

int launch_float_head_bwd(const void* dl, const float* hn, const float* W, float* dW, float* dbias, float* dhn, void* scratch, int B, int D, int C, int dtype,
                          hipStream_t st) {
    if (!fh_check("float_head_bwd", B, D, C, dtype)) return 1;
    if (!aligned16(W) || !aligned16(hn) || !scratch || reinterpret_cast<uintptr_t>(scratch) % 4) {
        set_error("float_head_bwd: the MFMA form needs W and hn 16-byte aligned and a scratch area");
        return 1;
    }
    if (dtype == kFloatHeadF32) fh_backward<float>(dl, hn, W, dW, dbias, dhn, scratch, B, D, C, st);
    else if (dtype == kFloatHeadF16) fh_backward<_Float16>(dl, hn, W, dW, dbias, dhn, scratch, B, D, C, st);
    else fh_backward<__bf16>(dl, hn, W, dW, dbias, dhn, scratch, B, D, C, st);
    return 0;
}

}  // namespace qv
