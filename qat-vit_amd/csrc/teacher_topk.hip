// The compressed teacher table (include/qatvit.h, qatvit_teacher_topk_rows and qatvit_kd_ce_loss_topk): a teacher row kept as
// its k largest logits (int16 classes, fp32 values, descending, equal values lower class first) and ONE fp32 logit u for every other class, chosen so
// that at the build temperature the tail keeps its softmax mass, spread uniformly.
//   k_topk_wave<R>   2 <= C <= 1024: one wave per row, 4 rows per workgroup, the row in R = 1, 4, 16 registers per lane (class c = lane + 64 j).  No LDS.
//   k_topk_group     1024 < C <= 32768: one 16-wave workgroup per row, the row in C floats of dynamic LDS (up to 128 KB of the CU's 160 KB).
//     Both read the row from global memory once.  Selection is k rounds of an argmax on the 64-bit key (order-preserving value, ~class): every thread
//     keeps the best key of the classes it owns; a round is one butterfly over the wave (and, for the workgroup, 16 keys through LDS and one barrier, the
//     key slots double-buffered), after which the ONE thread that owns the winner retires it and rescans its own classes.  The tail sum runs over what is
//     left: thread t adds its classes t + NT j in ascending j, a butterfly adds the lanes, the workgroup adds its waves 0 .. 15 in that order.
//   k_kd_ce_topk<NT, NPL>   k_kd_ce_rows<NT, NPL> (loss_rows.hip) with the table row(s) decompressed into LDS by the wave that reads them: every wave
//     fills the classes its lanes own with u and then scatters the entries that fall on them (LDS operations of one wave execute in order; of equal
//     classes the later entry is the one stored), one barrier, and the three sweeps run with k_kd_ce_rows' ownership, expressions and reduction order:
//     dlogits and the partials are bit for bit those of k_kd_ce_rows on the decompressed table.  NPL > 0: once, then the values sit in registers.
//     NPL = 0 (C > 4096): each sweep passes the row in chunks of 4096 classes (32 KB of LDS for a row and its partner).  Where all lanes of a wave
//     hold a tail class, the tail's exp is taken from the one computed per row instead of being evaluated again (the same bits).
//   k_kd_bce_finish (bce.hip, unedited) forms out3.  No atomics, no zeroed state: the same inputs give the same bits.
#include <float.h>

#include "loss_rows.h"
#include "qv_common.h"
#include "qv_kernels.h"

namespace qv {

static constexpr int kTopkGroupThreads = 1024, kTopkGroupWaves = kTopkGroupThreads / 64, kTopkChunk = 4096;

// (value, class) -> a key whose unsigned order is the selection order: a larger value first (-0 == +0), among equal values the lower class.  Every key of
// a finite value is > 0, which stands for "no class".
__device__ __forceinline__ uint64_t tk_key(float v, int c) {
    const float z = v == 0.f ? 0.f : v;
    return ((uint64_t)f2ord(z) << 32) | (uint32_t)~(uint32_t)c;
}
__device__ __forceinline__ int tk_class(uint64_t key) { return (int)~(uint32_t)key; }
__device__ __forceinline__ uint64_t wave_max_u64(uint64_t key) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)key, o, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(key >> 32), o, 64);
        const uint64_t other = ((uint64_t)hi << 32) | lo;
        key = other > key ? other : key;
    }
    return key;
}
// u from the maximum m and the tail's sum S of expf((t - m) / Tb) over n classes: m + Tb (log S - log n), with the two logarithms taken as ONE, of the
// quotient - each of them alone is rounded at a magnitude of 5 .. 10, and Tb times those roundings is 2e-6 .. 4e-6 of a u that is often below 1
__device__ __forceinline__ float tk_tail(float m, float S, float Tb, int n) { return m + Tb * logf(fmaxf(S, FLT_MIN) / (float)n); }

template <int R>
__global__ __launch_bounds__(256) void k_topk_wave(const float* __restrict__ logits, int B, int C, int k, float Tb, int16_t* __restrict__ idx,
                                                   float* __restrict__ val, float* __restrict__ tail) {
    const int lane = threadIdx.x & 63, b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;   // the whole wave: no barrier in this kernel
    const float* row = logits + (int64_t)b * C;
    int16_t* ib = idx + (int64_t)b * k;
    float* vb = val + (int64_t)b * k;
    float v[R];
    bool nan = false;
#pragma unroll
    for (int j = 0; j < R; ++j) {
        const int c = lane + 64 * j;
        if (c < C) { v[j] = row[c]; nan |= v[j] != v[j]; }
    }
    if (__builtin_amdgcn_ballot_w64(nan) != 0) {   // a NaN row: NaN values and tail, classes 0 .. k - 1
        if (lane < k) { ib[lane] = (int16_t)lane; vb[lane] = NAN; }
        if (lane == 0) tail[b] = NAN;
        return;
    }
    unsigned retired = 0;   // bit j: the class in register j is one of the selected
    uint64_t mine;
    float mine_raw;
    auto rescan = [&]() {
        mine = 0;
        mine_raw = 0.f;
#pragma unroll
        for (int j = 0; j < R; ++j) {
            const int c = lane + 64 * j;
            if (c < C && !((retired >> j) & 1u)) {
                const uint64_t key = tk_key(v[j], c);
                if (key > mine) { mine = key; mine_raw = v[j]; }
            }
        }
    };
    rescan();
    int out_c = 0;
    float out_v = 0.f, m = 0.f;
    for (int e = 0; e < k; ++e) {   // k <= C - 1: every round has a winner
        const int c = tk_class(wave_max_u64(mine));
        const float raw = __shfl(mine_raw, c & 63, 64);   // the stored bits, from the lane that owns the class
        if (e == 0) m = raw;
        if (lane == e) { out_c = c; out_v = raw; }
        if (lane == (c & 63)) { retired |= 1u << (c >> 6); rescan(); }
    }
    float S = 0.f;
#pragma unroll
    for (int j = 0; j < R; ++j)
        if (lane + 64 * j < C && !((retired >> j) & 1u)) S += expf((v[j] - m) / Tb);
    S = wave_sum(S);
    if (lane < k) { ib[lane] = (int16_t)out_c; vb[lane] = out_v; }
    if (lane == 0) tail[b] = tk_tail(m, S, Tb, C - k);
}

__global__ __launch_bounds__(kTopkGroupThreads) void k_topk_group(const float* __restrict__ logits, int C, int k, float Tb, int16_t* __restrict__ idx,
                                                                  float* __restrict__ val, float* __restrict__ tail) {
    extern __shared__ float tk_row[];   // C floats; thread t reads and writes the classes t + 1024 j alone, a selected class holds NaN
    __shared__ uint64_t s_key[2][kTopkGroupWaves];
    __shared__ float s_sum[kTopkGroupWaves], s_val[64];
    __shared__ int s_idx[64];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, b = blockIdx.x;
    const float* row = logits + (int64_t)b * C;
    int16_t* ib = idx + (int64_t)b * k;
    float* vb = val + (int64_t)b * k;
    bool nan = false;
    uint64_t mine = 0;
    for (int c = tid; c < C; c += kTopkGroupThreads) {
        const float x = row[c];
        tk_row[c] = x;
        nan |= x != x;
        const uint64_t key = tk_key(x, c);
        mine = key > mine ? key : mine;
    }
    if (__syncthreads_or(nan)) {
        if (tid < k) { ib[tid] = (int16_t)tid; vb[tid] = NAN; }
        if (tid == 0) tail[b] = NAN;
        return;
    }
    for (int e = 0; e < k; ++e) {
        const uint64_t wmax = wave_max_u64(mine);
        if (lane == 0) s_key[e & 1][w] = wmax;
        __syncthreads();   // round e + 1 writes the other buffer; nobody reaches round e + 2 before every wave has read this one
        uint64_t win = s_key[e & 1][0];
#pragma unroll
        for (int i = 1; i < kTopkGroupWaves; ++i) win = s_key[e & 1][i] > win ? s_key[e & 1][i] : win;
        const int c = tk_class(win);
        if (tid == (c & (kTopkGroupThreads - 1))) {
            s_idx[e] = c;
            s_val[e] = tk_row[c];
            tk_row[c] = NAN;
            mine = 0;
            for (int cc = tid; cc < C; cc += kTopkGroupThreads) {
                const float x = tk_row[cc];
                const uint64_t key = tk_key(x, cc);
                if (x == x && key > mine) mine = key;
            }
        }
    }
    __syncthreads();
    const float m = s_val[0];
    float S = 0.f;
    for (int c = tid; c < C; c += kTopkGroupThreads) {
        const float x = tk_row[c];
        if (x == x) S += expf((x - m) / Tb);
    }
    S = wave_sum(S);
    if (lane == 0) s_sum[w] = S;
    __syncthreads();
    if (tid < k) { ib[tid] = (int16_t)s_idx[tid]; vb[tid] = s_val[tid]; }
    if (tid == 0) {
        S = s_sum[0];
#pragma unroll
        for (int i = 1; i < kTopkGroupWaves; ++i) S += s_sum[i];
        tail[b] = tk_tail(m, S, Tb, C - k);
    }
}

int launch_teacher_topk_rows(const float* logits, int64_t batch, int64_t classes, int k, float Tb, int16_t* idx, float* val, float* tail, hipStream_t st) {
    const int B = (int)batch, C = (int)classes;
    if (C <= 64) k_topk_wave<1><<<(B + 3) / 4, 256, 0, st>>>(logits, B, C, k, Tb, idx, val, tail);
    else if (C <= 256) k_topk_wave<4><<<(B + 3) / 4, 256, 0, st>>>(logits, B, C, k, Tb, idx, val, tail);
    else if (C <= kRowsWaveMaxC) k_topk_wave<16><<<(B + 3) / 4, 256, 0, st>>>(logits, B, C, k, Tb, idx, val, tail);
    else {
        // a row of more than 16K classes needs more dynamic LDS than the 64 KB a kernel gets unasked
        static const hipError_t raised = hipFuncSetAttribute(reinterpret_cast<const void*>(k_topk_group), hipFuncAttributeMaxDynamicSharedMemorySize, 32768 * 4);
        if (raised != hipSuccess) {
            set_error("qatvit_teacher_topk_rows: cannot raise the dynamic LDS limit to 128 KB: %s", hipGetErrorString(raised));
            return 2;
        }
        k_topk_group<<<B, kTopkGroupThreads, (size_t)C * 4, st>>>(logits, C, k, Tb, idx, val, tail);
    }
    return 0;
}

template <int NT, int NPL>
__global__ __launch_bounds__(256) void k_kd_ce_topk(const float* __restrict__ s, const int16_t* __restrict__ tidx, const float* __restrict__ tval,
                                                    const float* __restrict__ ttail, int64_t rows, int k, const int64_t* __restrict__ index,
                                                    const int64_t* __restrict__ labels, const int32_t* __restrict__ mix, int B, int C, float T, float alpha,
                                                    float eps, float* __restrict__ partials, float* __restrict__ dlogits) {
    constexpr int R = NPL > 0 ? NPL : 1;
    constexpr int W = NPL > 0 ? NT * NPL : kTopkChunk;   // classes decompressed at a time
    static_assert(W % NT == 0 && kTopkChunk % 256 == 0, "a chunk is whole strides of the threads");
    __shared__ float dense[NT == 64 ? 4 : 1][2][W];       // per row slot: the row and its partner's, at most 32 KB
    const int tid = NT == 64 ? (threadIdx.x & 63) : threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = NT == 64 ? blockIdx.x * 4 + wave : blockIdx.x;
    float (&d0)[W] = dense[NT == 64 ? wave : 0][0];
    float (&d1)[W] = dense[NT == 64 ? wave : 0][1];
    const bool live = b < B;   // NT = 64: a wave past the batch still meets the workgroup's one barrier
    const float w_ce = 1.0f - alpha, w_kd = alpha;
    const float invB = 1.0f / (float)B, invT = 1.0f / T;
    float lam = 1.0f;
    int p = b;
    int64_t i = 0, i2 = 0;
    bool bad = false;
    if (live) {
        if (mix) {
            const int32_t* rec = mix + (int64_t)b * 6;
            lam = __int_as_float(rec[5]);
            if (lam != 1.0f && (unsigned)rec[0] < (unsigned)B) p = rec[0];
        }
        i = index[b];
        i2 = lam != 1.0f ? index[p] : i;
        bad = i < 0 || i >= rows || i2 < 0 || i2 >= rows;
    }
    const float oml = 1.0f - lam;
    float* dr = dlogits + (int64_t)(live ? b : 0) * C;
    auto nan_row = [&]() {
        for (int c = tid; c < C; c += NT) dr[c] = NAN;
        if (tid == 0) { partials[2 * (int64_t)b] = NAN; partials[2 * (int64_t)b + 1] = NAN; }
    };
    if (NT > 64 && bad) { nan_row(); return; }   // the whole workgroup, before any barrier
    const bool use = live && !bad, two = use && lam != 1.0f;
    // the entries: lane e of every wave holds entry e of the row and of the partner's row.  An entry takes part if its class is inside [0, C), no later
    // entry names the same class, and the class is owned by a thread of this wave (class c belongs to thread c % NT)
    int ec[2] = {-1, -1};
    float ev[2] = {0.f, 0.f}, u[2] = {0.f, 0.f};
    if (use) {
        u[0] = ttail[i];
        if (two) u[1] = ttail[i2];
        if (lane < k) {
            ec[0] = tidx[i * k + lane]; ev[0] = tval[i * k + lane];
            if (two) { ec[1] = tidx[i2 * k + lane]; ev[1] = tval[i2 * k + lane]; }
        }
    }
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        bool keep = ec[r] >= 0 && ec[r] < C && (NT == 64 || ((ec[r] & (NT - 1)) >> 6) == wave);
        // (skipped by a whole wave that has nothing to store: no partner row, or no entry on its classes)
        for (int e = 1; e < k && __builtin_amdgcn_ballot_w64(keep) != 0; ++e) {
            const int later = __shfl(ec[r], e, 64);   // every lane takes part: a shuffle reads nothing useful from a lane that sits it out
            keep = keep && !(e > lane && later == ec[r]);
        }
        if (!keep) ec[r] = -1;
    }
    auto decompress = [&](int base) {   // classes base .. base + W - 1 of the row(s); base % NT == 0
#pragma unroll
        for (int j = 0; j < W / NT; ++j) {
            d0[tid + NT * j] = u[0];
            if (two) d1[tid + NT * j] = u[1];
        }
        if (ec[0] >= base && ec[0] < base + W) d0[ec[0] - base] = ev[0];
        if (two && ec[1] >= base && ec[1] < base + W) d1[ec[1] - base] = ev[1];
    };
    float sv[R], tv[R], uv[R];
    if constexpr (NPL > 0) {
        if (use) decompress(0);
        __syncthreads();
        if (!live) return;
        if (bad) { nan_row(); return; }
    }
    const int y = (int)labels[b], y2 = (int)labels[p];
    const float* sr = s + (int64_t)b * C;
    if constexpr (NPL > 0) {
        for_owned<NT, NPL>(tid, C, [&](int j, int c) { sv[j] = sr[c]; tv[j] = d0[c]; uv[j] = two ? d1[c] : 0.f; });
    }
    // f(c, x, q, q2) for every class this thread owns, ascending: the student's logit and the two decompressed teacher logits (q2 is read where `two`)
    auto pass = [&](auto f) {
        if constexpr (NPL > 0) {
            for_owned<NT, NPL>(tid, C, [&](int j, int c) { f(c, sv[j], tv[j], uv[j]); });
        } else {
            for (int base = 0; base < C; base += W) {
                decompress(base);
                __syncthreads();
                const int end = base + W < C ? base + W : C;
                for (int c = base + tid; c < end; c += NT) f(c, sr[c], d0[c - base], two ? d1[c - base] : 0.f);
                __syncthreads();   // the next chunk's scatter follows every thread's reads of this one
            }
        }
    };
    // true where every active lane of the wave holds the tail's logit: its terms are then the row's one tail term
    auto all_tail = [&](float q, float ut) { return __builtin_amdgcn_ballot_w64(__float_as_uint(q) != __float_as_uint(ut)) == 0; };

    // sweep 1: the maxima m1, mt, mt2
    float mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    pass([&](int c, float x, float q, float q2) {
        mx[0] = fmaxf(mx[0], x);
        mx[1] = fmaxf(mx[1], q);
        if (two) mx[2] = fmaxf(mx[2], q2);
    });
    row_reduce<NT, 0, true>(mx);
    const float m1 = mx[0], mt = mx[1], mt2 = mx[2];
    // sweep 2: the partition sums z1, zT, zq, zq2
    const float eu = expf((u[0] - mt) * invT), eu2 = two ? expf((u[1] - mt2) * invT) : 0.f;
    float z[4] = {0.f, 0.f, 0.f, 0.f};
    pass([&](int c, float x, float q, float q2) {
        const float d = x - m1;
        z[0] += expf(d);
        z[1] += expf(d * invT);
        z[2] += all_tail(q, u[0]) ? eu : expf((q - mt) * invT);
        if (two) z[3] += all_tail(q2, u[1]) ? eu2 : expf((q2 - mt2) * invT);
    });
    row_reduce<NT, 1, false>(z);
    const float lz1 = logf(z[0]), lzT = logf(z[1]), lzq = logf(z[2]), lzq2 = two ? logf(z[3]) : 0.f;
    // sweep 3: the terms and the gradient (k_kd_ce_rows, term for term)
    const float qu = expf((u[0] - mt) * invT - lzq), qu2 = two ? expf((u[1] - mt2) * invT - lzq2) : 0.f;
    float acc[2] = {0.f, 0.f};   // ce, kd
    pass([&](int c, float x, float tq, float tq2) {
        const float lp = x - m1 - lz1;                      // log_softmax(s)
        const float ysm = (1.0f - eps) * (lam * (c == y ? 1.0f : 0.0f) + oml * (c == y2 ? 1.0f : 0.0f)) + eps / (float)C;
        acc[0] -= ysm * lp;
        float g = w_ce * (expf(lp) - ysm) * invB;
        const float lpT = (x - m1) * invT - lzT;            // log_softmax(s/T)
        float lq = (tq - mt) * invT - lzq;
        float q = all_tail(tq, u[0]) ? qu : expf(lq);
        if (two) {
            q = lam * q + oml * (all_tail(tq2, u[1]) ? qu2 : expf((tq2 - mt2) * invT - lzq2));
            lq = q > 0.f ? logf(q) : 0.f;                   // 0 * log 0 = 0
        }
        acc[1] += q * (lq - lpT);
        g += w_kd * T * (expf(lpT) - q) * invB;
        dr[c] = g;
    });
    row_reduce<NT, 2, false>(acc);
    if (tid == 0) { partials[2 * (int64_t)b] = acc[0]; partials[2 * (int64_t)b + 1] = acc[1]; }
}

int launch_kd_ce_loss_topk(const float* student, const int16_t* idx, const float* val, const float* tail, int64_t table_rows, int k, const int64_t* index,
                           const int64_t* labels, const int32_t* mix, int64_t batch, int64_t classes, float kd_temp, float kd_alpha,
                           float label_smoothing, float* partials, float* out3, float* dlogits, hipStream_t st) {
    const int B = (int)batch, C = (int)classes;
#define QV_TOPK(NT, NPL, GRID) \
    k_kd_ce_topk<NT, NPL><<<GRID, 256, 0, st>>>(student, idx, val, tail, table_rows, k, index, labels, mix, B, C, kd_temp, kd_alpha, label_smoothing, partials, dlogits)
    if (C <= 64) QV_TOPK(64, 1, (B + 3) / 4);
    else if (C <= 256) QV_TOPK(64, 4, (B + 3) / 4);
    else if (C <= kRowsWaveMaxC) QV_TOPK(64, 16, (B + 3) / 4);
    else if (C <= kRowsRegMaxC) QV_TOPK(256, 16, B);
    else QV_TOPK(256, 0, B);
#undef QV_TOPK
    k_kd_bce_finish<<<1, 256, 0, st>>>(partials, B, kd_temp, kd_alpha, 1, 1.0f / (float)B, out3);
    return 0;
}

}  // namespace qv
