// KD (temperature-scaled KL, batchmean) + label-smoothed softmax CE, forward and d/dlogits, with the classes of a row spread over the lanes
// (include/qatvit.h, qatvit_kd_ce_loss_rows).  Per element the expressions are kd_ce_row<MIX>'s (loss.hip), the record
// handling is k_kd_bce's (bce.hip): only the order of the sums over c and over b differs from the serial CE entries.
//   k_kd_ce_rows<NT, NPL>  NT threads share one row; thread t owns the classes t + NT * j.
//       NT = 64   (2 <= C <= 1024)   one wave per row, 4 rows per 256-thread workgroup, grid ceil(B / 4); NPL = 1, 4, 16 values per lane.  No LDS, no barrier.
//       NT = 256  (1024 < C <= 32768) one workgroup per row; NPL = 16 up to C = 4096, NPL = 0 above.
//     NPL > 0: the student's row and the teacher's row(s) are loaded ONCE into NPL registers per operand, every load issued before the first use, and the
//     three sweeps (maxima; partition sums; terms and gradient) run over registers.  NPL = 0: the sweeps re-read global memory (the row sits in L2).
//     Every read and the dlogits write are 64 consecutive floats per wave.  A workgroup's four waves combine their statistics through 16 floats of LDS per
//     stage in the fixed order (0 + 1) + (2 + 3), so every wave derives the same m and log z.  Writes the row's {sum_c ce terms, KD} to partials[2 * b].
//   k_kd_bce_finish (bce.hip, unedited) then forms out3 from the partials with scale = 1 / B, in double, in one fixed order.
// The form is chosen from C alone: a row's dlogits bits depend on the row, its partner, C and 1 / B only.  Two launches, no atomics, no zeroed state.
#include "loss_rows.h"
#include "qv_common.h"
#include "qv_kernels.h"

namespace qv {

template <int NT, int NPL>
__global__ __launch_bounds__(256) void k_kd_ce_rows(const float* __restrict__ s, const float* __restrict__ t, const float* __restrict__ table,
                                                    int64_t rows, const int64_t* __restrict__ index, const int64_t* __restrict__ labels,
                                                    const int32_t* __restrict__ mix, int B, int C, float T, float alpha, float eps,
                                                    float* __restrict__ partials, float* __restrict__ dlogits) {
    constexpr int R = NPL > 0 ? NPL : 1;
    const int tid = NT == 64 ? (threadIdx.x & 63) : threadIdx.x;
    const int b = NT == 64 ? blockIdx.x * 4 + (threadIdx.x >> 6) : blockIdx.x;
    if (b >= B) return;   // NT = 64 only, the whole wave: no barrier follows
    const bool kd = t || table;
    const float w_ce = kd ? (1.0f - alpha) : 1.0f, w_kd = kd ? alpha : 0.0f;
    const float invB = 1.0f / (float)B, invT = 1.0f / T;
    // the record: a row with lam == 1 (or without a record) is its own partner, so one expression below serves the mixed and the unmixed row
    float lam = 1.0f;
    int p = b;
    if (mix) {
        const int32_t* rec = mix + (int64_t)b * 6;
        lam = __int_as_float(rec[5]);
        if (lam != 1.0f && (unsigned)rec[0] < (unsigned)B) p = rec[0];
    }
    const float oml = 1.0f - lam;
    const int y = (int)labels[b], y2 = (int)labels[p];
    const float* sr = s + (int64_t)b * C;
    float* dr = dlogits + (int64_t)b * C;
    const float *tr = t ? t + (int64_t)b * C : nullptr, *tr2 = nullptr;
    if (table) {
        const int64_t i = index[b], i2 = lam != 1.0f ? index[p] : i;
        if (i < 0 || i >= rows || i2 < 0 || i2 >= rows) {   // the whole row, so (NT = 256) the whole workgroup leaves before any barrier
            for (int c = tid; c < C; c += NT) dr[c] = NAN;
            if (tid == 0) { partials[2 * (int64_t)b] = NAN; partials[2 * (int64_t)b + 1] = NAN; }
            return;
        }
        tr = table + i * C;
        if (lam != 1.0f) tr2 = table + i2 * C;
    }
    // the row(s) into registers: every load is issued here, before the first use
    float sv[R], tv[R], uv[R];
    if constexpr (NPL > 0) {
        for_owned<NT, NPL>(tid, C, [&](int j, int c) { sv[j] = sr[c]; });
        if (tr) for_owned<NT, NPL>(tid, C, [&](int j, int c) { tv[j] = tr[c]; });
        if (tr2) for_owned<NT, NPL>(tid, C, [&](int j, int c) { uv[j] = tr2[c]; });
    }
    auto S = [&](int j, int c) { return NPL > 0 ? sv[j] : sr[c]; };
    auto Q = [&](int j, int c) { return NPL > 0 ? tv[j] : tr[c]; };
    auto Q2 = [&](int j, int c) { return NPL > 0 ? uv[j] : tr2[c]; };

    // sweep 1: the maxima m1, mt, mt2
    float mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for_owned<NT, NPL>(tid, C, [&](int j, int c) { mx[0] = fmaxf(mx[0], S(j, c)); });
    if (tr) for_owned<NT, NPL>(tid, C, [&](int j, int c) { mx[1] = fmaxf(mx[1], Q(j, c)); });
    if (tr2) for_owned<NT, NPL>(tid, C, [&](int j, int c) { mx[2] = fmaxf(mx[2], Q2(j, c)); });
    row_reduce<NT, 0, true>(mx);
    const float m1 = mx[0], mt = mx[1], mt2 = mx[2];
    // sweep 2: the partition sums z1, zT, zq, zq2
    float z[4] = {0.f, 0.f, 0.f, 0.f};
    for_owned<NT, NPL>(tid, C, [&](int j, int c) {
        const float d = S(j, c) - m1;
        z[0] += expf(d);
        if (tr) z[1] += expf(d * invT);
    });
    if (tr) for_owned<NT, NPL>(tid, C, [&](int j, int c) { z[2] += expf((Q(j, c) - mt) * invT); });
    if (tr2) for_owned<NT, NPL>(tid, C, [&](int j, int c) { z[3] += expf((Q2(j, c) - mt2) * invT); });
    row_reduce<NT, 1, false>(z);
    const float lz1 = logf(z[0]), lzT = tr ? logf(z[1]) : 0.f, lzq = tr ? logf(z[2]) : 0.f, lzq2 = tr2 ? logf(z[3]) : 0.f;
    // sweep 3: the terms and the gradient (kd_ce_row<true>, term for term)
    float acc[2] = {0.f, 0.f};   // ce, kd
    for_owned<NT, NPL>(tid, C, [&](int j, int c) {
        const float x = S(j, c);
        const float lp = x - m1 - lz1;                      // log_softmax(s)
        const float ysm = (1.0f - eps) * (lam * (c == y ? 1.0f : 0.0f) + oml * (c == y2 ? 1.0f : 0.0f)) + eps / (float)C;
        acc[0] -= ysm * lp;
        float g = w_ce * (expf(lp) - ysm) * invB;
        if (tr) {
            const float lpT = (x - m1) * invT - lzT;        // log_softmax(s/T)
            float lq = (Q(j, c) - mt) * invT - lzq;
            float q = expf(lq);
            if (tr2) {
                q = lam * q + oml * expf((Q2(j, c) - mt2) * invT - lzq2);
                lq = q > 0.f ? logf(q) : 0.f;               // 0 * log 0 = 0
            }
            acc[1] += q * (lq - lpT);
            g += w_kd * T * (expf(lpT) - q) * invB;
        }
        dr[c] = g;
    });
    row_reduce<NT, 2, false>(acc);
    if (tid == 0) { partials[2 * (int64_t)b] = acc[0]; partials[2 * (int64_t)b + 1] = acc[1]; }
}

int launch_kd_ce_loss_rows(const float* student, const float* teacher, const float* table, int64_t table_rows, const int64_t* index,
                           const int64_t* labels, const int32_t* mix, int64_t batch, int64_t classes, float kd_temp, float kd_alpha,
                           float label_smoothing, float* partials, float* out3, float* dlogits, hipStream_t st) {
    const int B = (int)batch, C = (int)classes;
#define QV_ROWS(NT, NPL, GRID) \
    k_kd_ce_rows<NT, NPL><<<GRID, 256, 0, st>>>(student, teacher, table, table_rows, index, labels, mix, B, C, kd_temp, kd_alpha, label_smoothing, partials, dlogits)
    if (C <= 64) QV_ROWS(64, 1, (B + 3) / 4);
    else if (C <= 256) QV_ROWS(64, 4, (B + 3) / 4);
    else if (C <= kRowsWaveMaxC) QV_ROWS(64, 16, (B + 3) / 4);
    else if (C <= kRowsRegMaxC) QV_ROWS(256, 16, B);
    else QV_ROWS(256, 0, B);
#undef QV_ROWS
    k_kd_bce_finish<<<1, 256, 0, st>>>(partials, B, kd_temp, kd_alpha, teacher || table ? 1 : 0, 1.0f / (float)B, out3);
    return 0;
}

}  // namespace qv
