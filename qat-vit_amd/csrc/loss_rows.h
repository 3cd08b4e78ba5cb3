// What the class-parallel loss kernels share (loss_rows.hip: k_kd_ce_rows; teacher_topk.hip: k_kd_ce_topk): the class-count thresholds of the forms,
// the ownership rule c = t + NT * j and the reduction of the threads' values in one fixed order.  Two kernels that use these with the same
// per-element expressions give the same bits.
#pragma once
#include "qv_common.h"

namespace qv {

static constexpr int kRowsWaveMaxC = 1024, kRowsRegMaxC = 4096;

// One value per wave -> the row's value in every thread.  NT = 64: the butterfly alone.  NT = 256: lane 0 of each wave stores its K values, one barrier,
// every thread combines the four in one order.  STAGE names the LDS array: each reduction of a kernel has its own, so one barrier per stage is enough.
template <int NT, int STAGE, bool MAX, int K>
__device__ __forceinline__ void row_reduce(float (&v)[K]) {
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = MAX ? wave_max(v[k]) : wave_sum(v[k]);
    if constexpr (NT > 64) {
        static_assert(NT == 256, "four waves");
        __shared__ float sh[4][K];
        if ((threadIdx.x & 63) == 0) {
#pragma unroll
            for (int k = 0; k < K; ++k) sh[threadIdx.x >> 6][k] = v[k];
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < K; ++k)
            v[k] = MAX ? fmaxf(fmaxf(sh[0][k], sh[1][k]), fmaxf(sh[2][k], sh[3][k])) : (sh[0][k] + sh[1][k]) + (sh[2][k] + sh[3][k]);
    }
}

// f(j, c) for every class c = t + NT * j this thread owns: NPL > 0 unrolled over the register slots, NPL = 0 a loop (j stays 0)
template <int NT, int NPL, class F>
__device__ __forceinline__ void for_owned(int t, int C, F f) {
    if constexpr (NPL > 0) {
#pragma unroll
        for (int j = 0; j < NPL; ++j) {
            const int c = t + NT * j;
            if (c < C) f(j, c);
        }
    } else {
        for (int c = t; c < C; c += NT) f(0, c);
    }
}

}  // namespace qv
