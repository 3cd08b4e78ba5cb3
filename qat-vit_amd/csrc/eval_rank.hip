// Validation at many classes: a [B, C] batch of logits -> the histogram of the label's RANK (every top-k at once), the label-smoothed cross-entropy
// and optional per-class counts, added to a state block of 74 words (include/qatvit.h, qatvit_eval_accumulate_rank).  The
// class-parallel sibling of eval.hip, laid out like loss_rows.hip:
//   k_eval_rank<T, NT, R, HELD>  NT threads share one row; thread t owns the classes base + t + NT * j, j < R.
//       NT = 64    (2 <= C <= 1024)    one wave per row, 4 rows in flight per 256-thread workgroup; R = 1, 4, 16.  No barrier inside a row.
//       NT = 256   (1024 < C <= 4096)  one workgroup per row, R = 16.
//       NT = 1024  (4096 < C <= 32768) one 16-wave workgroup per row, R = 8: the row passes in chunks of 8192 classes, 32 KB of loads in flight.
//     HELD (C <= NT * R): the row is loaded ONCE, every load issued before the first use, and both sweeps run over the R registers.  Otherwise the
//     second sweep re-reads the chunks (the row sits in L2).  Every read is 64 consecutive elements per wave.
//   Per row: x[label] arrives first as one broadcast load.  Sweep 1 gives each thread its best (value, index) candidate, its count of candidates that
//   beat the label's, and its maximum; sweep 2, after the cross-thread maximum m, gives sum exp(x - m) and sum (x - m) (summed as differences, so
//   a common offset of the logits does not cancel against C * m).  Waves fold by butterflies, workgroups through one LDS record per wave and stage.
//   The workgroup's counters live in LDS (one LDS atomic per row and counter); at the end one device atomic per counter that moved.
// Rows are dealt round-robin to a grid of at most 1024 workgroups.  Plain C++ throughout: vector loads, LDS and device atomics, no inline assembly.
#include <limits.h>

#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>

#include "qv_common.h"
#include "qv_kernels.h"

namespace qv {

static constexpr int kRankWaveMaxC = 1024, kRankRegMaxC = 4096;
// words of the state block (include/qatvit.h lists them)
enum : int { kRkTotal = 0, kRkBadLabels, kRkNonfinite, kRkLossRows, kRkOtherSeen, kRkAgree, kRkBadIndex, kRkLossSum = 8, kRkHist = 10,
             kRkOtherHist = kRkHist + kEvalRankBins };
static_assert(kRkOtherHist + kEvalRankBins == kEvalRankWords, "the state block is 74 words");

// widening to fp32 is exact and monotone for both 16-bit formats, so comparing the widened values compares the stored ones
__device__ __forceinline__ float rk_load(const float* p) { return *p; }
__device__ __forceinline__ float rk_load(const __half* p) { return __half2float(*p); }
__device__ __forceinline__ float rk_load(const __hip_bfloat16* p) { return __builtin_bit_cast(float, (uint32_t)(*reinterpret_cast<const uint16_t*>(p)) << 16); }

// eval.hip's order on (value, index) candidates, torch.argmax's: a NaN beats every number, a larger number beats a smaller one (+0 == -0), and among
// equals (two NaNs included) the lower index wins.  A total order: no candidate beats itself, and of two different candidates exactly one beats the other.
__device__ __forceinline__ bool rk_beats(float v, int i, float bv, int bi) {
    const bool vn = v != v, bn = bv != bv;
    if (vn || bn) return vn && (!bn || i < bi);
    return v > bv || (v == bv && i < bi);
}

struct RankRow {
    int pred;     // the row's argmax in that order
    int rank;     // number of columns whose candidate beats (x[y], y); 0 without a valid label
    float loss;   // the smoothed cross-entropy; 0 where it was not asked for
};

// One row by NT threads (tid = 0 .. NT - 1); every thread returns the same record.  y < 0: no valid label, only pred is formed.  NT > 64: every thread
// of the workgroup must call with the same arguments (two barriers with want_loss, else one).  STAGE gives each call site of a kernel its own LDS
// records; the kernel's barrier at the end of a row keeps the next row's writes behind this row's reads.
template <typename T, int NT, int R, bool HELD, int STAGE>
__device__ __forceinline__ RankRow rank_row(const T* __restrict__ row, int C, int y, bool want_loss, float eps, int tid) {
    constexpr int NW = NT / 64;
    const float xl = y >= 0 ? rk_load(row + y) : 0.f;   // one address for the whole wave: a broadcast load, ahead of the row's
    float v[R];
    auto fetch = [&](int base) {
#pragma unroll
        for (int j = 0; j < R; ++j) {
            const int c = base + tid + NT * j;
            if (c < C) v[j] = rk_load(row + c);
        }
    };
    // sweep 1: best candidate, candidates that beat the label's, maximum (fmaxf drops NaNs: m is the largest number, -inf if there is none)
    float bv = -INFINITY, m = -INFINITY;
    int bi = INT_MAX, cnt = 0;   // INT_MAX = "no column": loses against every real candidate of equal value
    auto sweep1 = [&](int base) {
#pragma unroll
        for (int j = 0; j < R; ++j) {
            const int c = base + tid + NT * j;
            if (c < C) {
                const float x = v[j];
                m = fmaxf(m, x);
                if (rk_beats(x, c, bv, bi)) { bv = x; bi = c; }
                cnt += y >= 0 && rk_beats(x, c, xl, y);
            }
        }
    };
    if constexpr (HELD) {
        fetch(0);
        sweep1(0);
    } else {
        for (int base = 0; base < C; base += NT * R) { fetch(base); sweep1(base); }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (rk_beats(ov, oi, bv, bi)) { bv = ov; bi = oi; }
        // the rank is a sum of per-thread counts of one fixed set of columns: integer addition, the same value in any association
        cnt += __shfl_xor(cnt, o, 64);
    }
    m = wave_max(m);
    if constexpr (NW > 1) {
        __shared__ float s_bv[NW], s_m[NW];
        __shared__ int s_bi[NW], s_cnt[NW];
        const int w = tid >> 6;
        if ((tid & 63) == 0) { s_bv[w] = bv; s_bi[w] = bi; s_cnt[w] = cnt; s_m[w] = m; }
        __syncthreads();
        bv = s_bv[0]; bi = s_bi[0]; cnt = s_cnt[0]; m = s_m[0];
#pragma unroll
        for (int k = 1; k < NW; ++k) {
            if (rk_beats(s_bv[k], s_bi[k], bv, bi)) { bv = s_bv[k]; bi = s_bi[k]; }
            cnt += s_cnt[k];
            m = fmaxf(m, s_m[k]);
        }
    }
    RankRow out = {bi, cnt, 0.f};
    if (!want_loss) return out;
    // sweep 2: z = sum exp(x - m), sd = sum (x - m).  A NaN, a +inf or an all -inf row puts a NaN into z; a -inf element makes sd -inf.
    float z = 0.f, sd = 0.f;
    auto sweep2 = [&](int base) {
#pragma unroll
        for (int j = 0; j < R; ++j) {
            if (base + tid + NT * j < C) {
                const float d = v[j] - m;
                z += expf(d);
                sd += d;
            }
        }
    };
    if constexpr (HELD) {
        sweep2(0);
    } else {
        for (int base = 0; base < C; base += NT * R) { fetch(base); sweep2(base); }
    }
    z = wave_sum(z);
    sd = wave_sum(sd);
    if constexpr (NW > 1) {
        __shared__ float s_z[NW], s_sd[NW];
        const int w = tid >> 6;
        if ((tid & 63) == 0) { s_z[w] = z; s_sd[w] = sd; }
        __syncthreads();
        z = s_z[0]; sd = s_sd[0];
#pragma unroll
        for (int k = 1; k < NW; ++k) { z += s_z[k]; sd += s_sd[k]; }
    }
    // L = log z - (1 - eps) (x[y] - m) - (eps / C) sum (x - m); without smoothing the last term is left out (0 * -inf would be NaN): eval.hip's loss
    float L = logf(z) - (1.0f - eps) * (xl - m);
    if (eps > 0.f) L -= (eps / (float)C) * sd;
    out.loss = L;
    return out;
}

template <typename T, int NT, int R, bool HELD>
__global__ __launch_bounds__(NT < 256 ? 256 : NT) void k_eval_rank(const T* __restrict__ logits, int64_t ld, const int64_t* __restrict__ labels, int B, int C,
                                                                   float eps, const float* __restrict__ other, int64_t other_ld,
                                                                   const int64_t* __restrict__ other_index, int64_t other_rows,
                                                                   unsigned long long* __restrict__ state, int64_t* __restrict__ class_counts) {
    constexpr int RPB = NT == 64 ? 4 : 1;   // rows in flight per workgroup
    const int tid = NT == 64 ? (threadIdx.x & 63) : threadIdx.x;
    const int slot = NT == 64 ? (threadIdx.x >> 6) : 0;
    // the workgroup's counters, in the order of the state block; loss sums per row slot, in double
    __shared__ unsigned int sc[kEvalRankWords];
    __shared__ double sloss[4];
    if (threadIdx.x < kEvalRankWords) sc[threadIdx.x] = 0u;
    if (threadIdx.x < 4) sloss[threadIdx.x] = 0.0;
    __syncthreads();
    double loss = 0.0;
    for (int b = blockIdx.x * RPB + slot; b < B; b += gridDim.x * RPB) {   // NT > 64: b is the same in every thread, so are all branches below
        const int64_t y64 = labels[b];
        const bool y_ok = y64 >= 0 && y64 < C;
        const int y = y_ok ? (int)y64 : -1;
        const RankRow r = rank_row<T, NT, R, HELD, 0>(logits + (int64_t)b * ld, C, y, y_ok, eps, tid);
        int orank = -1, opred = -1;
        bool bad_index = false;
        if (other) {
            const int64_t i = other_index ? other_index[b] : (int64_t)b;
            bad_index = other_index && (i < 0 || i >= other_rows);
            if (!bad_index) {
                const RankRow o = rank_row<float, NT, R, HELD, 1>(other + i * other_ld, C, y, false, 0.f, tid);
                opred = o.pred;
                orank = o.rank;
            }
        }
        if (tid == 0) {
            atomicAdd(&sc[kRkTotal], 1u);
            if (y_ok) {
                atomicAdd(&sc[kRkHist + min(r.rank, kEvalRankBins - 1)], 1u);
                if (isfinite(r.loss)) { loss += (double)r.loss; atomicAdd(&sc[kRkLossRows], 1u); }
                else atomicAdd(&sc[kRkNonfinite], 1u);
                if (class_counts) {
                    atomicAdd(reinterpret_cast<unsigned long long*>(class_counts + y), 1ull);
                    if (r.rank == 0) atomicAdd(reinterpret_cast<unsigned long long*>(class_counts + C + y), 1ull);
                }
            } else {
                atomicAdd(&sc[kRkBadLabels], 1u);
            }
            if (bad_index) atomicAdd(&sc[kRkBadIndex], 1u);
            if (opred >= 0) {
                atomicAdd(&sc[kRkOtherSeen], 1u);
                if (opred == r.pred) atomicAdd(&sc[kRkAgree], 1u);
                if (y_ok) atomicAdd(&sc[kRkOtherHist + min(orank, kEvalRankBins - 1)], 1u);
            }
        }
        if constexpr (NT > 64) __syncthreads();   // the next row rewrites rank_row's LDS records: every wave has read this row's
    }
    if (tid == 0) sloss[slot] = loss;
    __syncthreads();
    // one device atomic per counter that moved
    if (threadIdx.x == kRkLossSum) {
        if (sc[kRkLossRows]) atomicAdd(reinterpret_cast<double*>(state + kRkLossSum), (sloss[0] + sloss[1]) + (sloss[2] + sloss[3]));
    } else if (threadIdx.x < kEvalRankWords && sc[threadIdx.x]) {
        atomicAdd(state + threadIdx.x, (unsigned long long)sc[threadIdx.x]);
    }
}

template <typename T>
static void launch_rank_typed(const void* logits, int64_t ld, const int64_t* labels, int B, int C, float eps, const float* other, int64_t other_ld,
                              const int64_t* other_index, int64_t other_rows, void* state, int64_t* class_counts, hipStream_t st) {
    const int wave_grid = cdiv(B, 4) < 1024 ? cdiv(B, 4) : 1024, row_grid = B < 1024 ? B : 1024;
#define QV_RANK(NT, R, HELD, GRID)                                                                                                                 \
    k_eval_rank<T, NT, R, HELD><<<GRID, NT < 256 ? 256 : NT, 0, st>>>(static_cast<const T*>(logits), ld, labels, B, C, eps, other, other_ld, other_index, \
                                                                      other_rows, static_cast<unsigned long long*>(state), class_counts)
    if (C <= 64) QV_RANK(64, 1, true, wave_grid);
    else if (C <= 256) QV_RANK(64, 4, true, wave_grid);
    else if (C <= kRankWaveMaxC) QV_RANK(64, 16, true, wave_grid);
    else if (C <= kRankRegMaxC) QV_RANK(256, 16, true, row_grid);
    else QV_RANK(1024, 8, false, row_grid);
#undef QV_RANK
}

int launch_eval_rank(const void* logits, int dtype, int64_t ld, const int64_t* labels, int64_t batch, int64_t classes, float label_smoothing,
                     const float* other, int64_t other_ld, const int64_t* other_index, int64_t other_rows, void* state, int64_t* class_counts,
                     hipStream_t st) {
    const int B = (int)batch, C = (int)classes;
    switch (dtype) {
    case 0: launch_rank_typed<float>(logits, ld, labels, B, C, label_smoothing, other, other_ld, other_index, other_rows, state, class_counts, st); return 0;
    case 1: launch_rank_typed<__half>(logits, ld, labels, B, C, label_smoothing, other, other_ld, other_index, other_rows, state, class_counts, st); return 0;
    case 2:
        launch_rank_typed<__hip_bfloat16>(logits, ld, labels, B, C, label_smoothing, other, other_ld, other_index, other_rows, state, class_counts, st);
        return 0;
    }
    return 1;
}

}  // namespace qv
