// Validation counts on the device: a [B, C] batch of logits -> accuracy / cross-entropy / confusion counts, accumulated into one small state
// block, so a whole evaluation needs one device-to-host copy at its end.  Restates the reference's evaluate_fp32 (qat_trainer.py:49-61:
// argmax, ==, sum) without its host round trip per batch; state layout and counting rules: qv_kernels.h (EvalState) and include/qatvit.h.
#include <limits.h>

#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>

#include "qv_common.h"
#include "qv_kernels.h"

namespace qv {

// widening to fp32 is exact and monotone for both 16-bit formats, so comparing the widened values compares the stored ones
__device__ __forceinline__ float ev_load(const float* p) { return *p; }
__device__ __forceinline__ float ev_load(const __half* p) { return __half2float(*p); }
__device__ __forceinline__ float ev_load(const __hip_bfloat16* p) { return __builtin_bit_cast(float, (uint32_t)(*reinterpret_cast<const uint16_t*>(p)) << 16); }

// torch.argmax's order on (value, index) candidates: a NaN beats every number, a larger number beats a smaller one (+0 == -0), and among equals
// (two NaNs included) the lower index wins.  It is a total order, so a reduction in any association gives the same winner.
__device__ __forceinline__ bool ev_better(float v, int i, float bv, int bi) {
    const bool vn = v != v, bn = bv != bv;
    if (vn || bn) return vn && (!bn || i < bi);
    return v > bv || (v == bv && i < bi);
}

// argmax of one row by one wave (lane l holds columns l, l + 64, ...); every lane returns the winner.  mx, when given, receives the row's
// largest non-NaN value (-inf if there is none).
template <typename T>
__device__ __forceinline__ int ev_row_argmax(const T* __restrict__ row, int C, float* mx) {
    const int lane = threadIdx.x & 63;
    float bv = -INFINITY, m = -INFINITY;
    int bi = INT_MAX;   // "no column": loses against every real candidate of equal value
    for (int c = lane; c < C; c += kWave) {
        const float v = ev_load(row + c);
        m = fmaxf(m, v);
        if (ev_better(v, c, bv, bi)) { bv = v; bi = c; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (ev_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
    }
    if (mx) *mx = wave_max(m);
    return bi;
}

template <typename T>
__global__ __launch_bounds__(256) void k_eval_accumulate(const T* __restrict__ logits, int64_t ld, const int64_t* __restrict__ labels, int B, int C,
                                                         const float* __restrict__ other, int64_t other_ld, const int64_t* __restrict__ other_index,
                                                         int64_t other_rows, EvalState* __restrict__ state, int64_t* __restrict__ confusion) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // this wave's counts, in the order of EvalState's int64 words; every lane keeps the same values (all inputs to them are wave-uniform)
    unsigned long long cnt[kEvalCounters] = {};
    double loss = 0.0;
    for (int b = blockIdx.x * 4 + wave; b < B; b += gridDim.x * 4) {
        const T* row = logits + (int64_t)b * ld;
        float m;
        const int pred = ev_row_argmax(row, C, &m);
        const int64_t y = labels[b];
        const bool y_ok = y >= 0 && y < C;
        cnt[0] += 1;
        if (y_ok) {
            cnt[1] += pred == (int)y;
            // CE = logsumexp(row) - row[y] in the max-subtracted form of loss.hip: log(sum exp(x - m)) - (x[y] - m).  A NaN, a +inf or an all -inf
            // row makes it non-finite (x - m is NaN somewhere); such a row is counted, not summed.
            float z = 0.f;
            for (int c = lane; c < C; c += kWave) z += expf(ev_load(row + c) - m);
            z = wave_sum(z);
            const float ce = logf(z) - (ev_load(row + y) - m);
            if (isfinite(ce)) { loss += (double)ce; cnt[8] += 1; }
            else cnt[3] += 1;
            if (confusion && lane == 0) atomicAdd(reinterpret_cast<unsigned long long*>(confusion + y * C + pred), 1ull);
        } else {
            cnt[2] += 1;
        }
        if (other) {
            const int64_t r = other_index ? other_index[b] : (int64_t)b;
            if (other_index && (r < 0 || r >= other_rows)) {
                cnt[7] += 1;
            } else {
                const int op = ev_row_argmax(other + r * other_ld, C, nullptr);
                cnt[4] += 1;
                cnt[5] += op == pred;
                cnt[6] += y_ok && op == (int)y;
            }
        }
    }
    // fold the block's four waves, then one atomic per counter that moved
    __shared__ unsigned long long scnt[4][kEvalCounters];
    __shared__ double sloss[4];
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < kEvalCounters; ++k) scnt[wave][k] = cnt[k];
        sloss[wave] = loss;
    }
    __syncthreads();
    if (threadIdx.x < kEvalCounters) {
        const unsigned long long v = scnt[0][threadIdx.x] + scnt[1][threadIdx.x] + scnt[2][threadIdx.x] + scnt[3][threadIdx.x];
        if (v) atomicAdd(reinterpret_cast<unsigned long long*>(state) + threadIdx.x, v);
    } else if (threadIdx.x == kEvalCounters) {
        const double v = (sloss[0] + sloss[1]) + (sloss[2] + sloss[3]);
        if (scnt[0][8] + scnt[1][8] + scnt[2][8] + scnt[3][8]) atomicAdd(&state->loss_sum, v);
    }
}

int launch_eval_accumulate(const void* logits, int dtype, int64_t ld, const int64_t* labels, int64_t batch, int64_t classes, const float* other,
                           int64_t other_ld, const int64_t* other_index, int64_t other_rows, EvalState* state, int64_t* confusion, hipStream_t st) {
    const int B = (int)batch, C = (int)classes;
    const int grid = cdiv(batch, 4) < 1024 ? cdiv(batch, 4) : 1024;
    switch (dtype) {
    case 0:
        k_eval_accumulate<<<grid, 256, 0, st>>>(static_cast<const float*>(logits), ld, labels, B, C, other, other_ld, other_index, other_rows, state, confusion);
        return 0;
    case 1:
        k_eval_accumulate<<<grid, 256, 0, st>>>(static_cast<const __half*>(logits), ld, labels, B, C, other, other_ld, other_index, other_rows, state, confusion);
        return 0;
    case 2:
        k_eval_accumulate<<<grid, 256, 0, st>>>(static_cast<const __hip_bfloat16*>(logits), ld, labels, B, C, other, other_ld, other_index, other_rows, state,
                                                confusion);
        return 0;
    }
    return 1;
}

}  // namespace qv
