// KD (temperature-scaled KL, batchmean) + label-smoothed CE, forward and d/dlogits in one
// single-block launch.  Restates /root/reference/src/training/qat_trainer.py:343-349 with the
// criteria of :265-266; closed forms in SURVEY.md section 8(a) row LOSS.
#include "qv_common.h"
#include "qv_kernels.h"

namespace qv {


// One row of the loss: accumulates the row's CE and KD sums and writes its dlogits.  `tr` is the teacher's row (nullptr: CE only).  All kernels below
// run exactly this code on a row, so a teacher row gathered from a table gives what the same row passed in a [B, C] tensor gives, bit for bit.
// MIX adds the second target pair of a mix record: the label y2 with weight 1 - lam next to y with lam, and, where tr2 is given, the KD target
// lam * softmax(tr / T) + (1 - lam) * softmax(tr2 / T).  With lam == 1 and tr2 == nullptr every value is the one MIX = false forms:
// (1 - eps) * 1 is the 1 - eps of the hard label, (1 - eps) * 0 its 0.
template <bool MIX>
__device__ __forceinline__ void kd_ce_row(const float* __restrict__ sr, const float* __restrict__ tr, int y, int C, float T, float invT, float invB,
                                          float w_ce, float w_kd, float eps, float& ce_acc, float& kd_acc, float* __restrict__ dr,
                                          const float* __restrict__ tr2 = nullptr, int y2 = 0, float lam = 1.0f) {
    float m1 = -INFINITY;
    for (int c = 0; c < C; ++c) m1 = fmaxf(m1, sr[c]);
    float z1 = 0.f, zT = 0.f;
    for (int c = 0; c < C; ++c) { z1 += expf(sr[c] - m1); zT += expf((sr[c] - m1) * invT); }
    const float lz1 = logf(z1), lzT = logf(zT);
    float mt = -INFINITY, zq = 0.f;
    if (tr) {
        for (int c = 0; c < C; ++c) mt = fmaxf(mt, tr[c]);
        for (int c = 0; c < C; ++c) zq += expf((tr[c] - mt) * invT);
    }
    const float lzq = tr ? logf(zq) : 0.f;
    float mt2 = -INFINITY, zq2 = 0.f;
    if (MIX && tr2) {
        for (int c = 0; c < C; ++c) mt2 = fmaxf(mt2, tr2[c]);
        for (int c = 0; c < C; ++c) zq2 += expf((tr2[c] - mt2) * invT);
    }
    const float lzq2 = MIX && tr2 ? logf(zq2) : 0.f;
    const float oml = 1.0f - lam;
    for (int c = 0; c < C; ++c) {
        const float lp = sr[c] - m1 - lz1;                  // log_softmax(s)
        const float ysm = MIX ? (1.0f - eps) * (lam * (c == y ? 1.0f : 0.0f) + oml * (c == y2 ? 1.0f : 0.0f)) + eps / (float)C
                              : (c == y ? 1.0f - eps : 0.0f) + eps / (float)C;
        ce_acc -= ysm * lp;
        float g = w_ce * (expf(lp) - ysm) * invB;
        if (tr) {
            const float lpT = (sr[c] - m1) * invT - lzT;    // log_softmax(s/T)
            float lq = (tr[c] - mt) * invT - lzq;
            float q = expf(lq);
            if (MIX && tr2) {
                q = lam * q + oml * expf((tr2[c] - mt2) * invT - lzq2);
                lq = q > 0.f ? logf(q) : 0.f;               // 0 * log 0 = 0
            }
            kd_acc += q * (lq - lpT);
            g += w_kd * T * (expf(lpT) - q) * invB;
        }
        dr[c] = g;
    }
}

// the block's sums -> out3 = {loss, ce, kd * T^2}
__device__ __forceinline__ void kd_ce_finish(float ce_acc, float kd_acc, float invB, float T, float w_ce, float w_kd, float* __restrict__ out3) {
    __shared__ float sce[4], skd[4];
    ce_acc = wave_sum(ce_acc);
    kd_acc = wave_sum(kd_acc);
    if ((threadIdx.x & 63) == 0) { sce[threadIdx.x >> 6] = ce_acc; skd[threadIdx.x >> 6] = kd_acc; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const float ce = (sce[0] + sce[1] + sce[2] + sce[3]) * invB;
        const float kd = (skd[0] + skd[1] + skd[2] + skd[3]) * invB * T * T;
        out3[0] = w_kd * kd + w_ce * ce;
        out3[1] = ce;
        out3[2] = kd;
    }
}

__global__ __launch_bounds__(256) void k_kd_ce(const float* __restrict__ s, const float* __restrict__ t, const int64_t* __restrict__ labels,
                                               int B, int C, float T, float alpha, float eps, float* __restrict__ out3,
                                               float* __restrict__ dlogits) {
    float ce_acc = 0.f, kd_acc = 0.f;
    const float invB = 1.0f / (float)B, invT = 1.0f / T;
    const float w_ce = t ? (1.0f - alpha) : 1.0f, w_kd = t ? alpha : 0.0f;
    for (int b = threadIdx.x; b < B; b += blockDim.x)
        kd_ce_row<false>(s + (int64_t)b * C, t ? t + (int64_t)b * C : nullptr, (int)labels[b], C, T, invT, invB, w_ce, w_kd, eps, ce_acc, kd_acc,
                         dlogits + (int64_t)b * C);
    kd_ce_finish(ce_acc, kd_acc, invB, T, w_ce, w_kd, out3);
}

// The same loss with the teacher's row of sample b read from a table of per-sample logits: tr = table + index[b] * C.  An index outside
// [0, rows) reads nothing: its row of dlogits and (through the sums) all of out3 become NaN, without a fault and without a host synchronisation.
__global__ __launch_bounds__(256) void k_kd_ce_table(const float* __restrict__ s, const float* __restrict__ table, int64_t rows,
                                                     const int64_t* __restrict__ index, const int64_t* __restrict__ labels, int B, int C, float T,
                                                     float alpha, float eps, float* __restrict__ out3, float* __restrict__ dlogits) {
    float ce_acc = 0.f, kd_acc = 0.f;
    const float invB = 1.0f / (float)B, invT = 1.0f / T;
    const float w_ce = 1.0f - alpha, w_kd = alpha;
    for (int b = threadIdx.x; b < B; b += blockDim.x) {
        const int64_t i = index[b];
        float* dr = dlogits + (int64_t)b * C;
        if (i < 0 || i >= rows) {
            for (int c = 0; c < C; ++c) dr[c] = NAN;
            ce_acc = NAN;
            kd_acc = NAN;
            continue;
        }
        kd_ce_row<false>(s + (int64_t)b * C, table + i * C, (int)labels[b], C, T, invT, invB, w_ce, w_kd, eps, ce_acc, kd_acc, dr);
    }
    kd_ce_finish(ce_acc, kd_acc, invB, T, w_ce, w_kd, out3);
}

// Both forms with the targets of a mix record per row (include/qatvit.h): labels y_b and y_p weighted lam and 1 - lam; with a table, the KD target
// mixed from the rows index[b] and index[p] in the same way.  A teacher tensor saw the mixed images: its row stands alone.  The partner's row is
// read only where lam != 1, so an index outside the table makes NaN exactly where its row would have been used.
__global__ __launch_bounds__(256) void k_kd_ce_mix(const float* __restrict__ s, const float* __restrict__ t, const float* __restrict__ table,
                                                   int64_t rows, const int64_t* __restrict__ index, const int64_t* __restrict__ labels,
                                                   const int32_t* __restrict__ mix, int B, int C, float T, float alpha, float eps,
                                                   float* __restrict__ out3, float* __restrict__ dlogits) {
    float ce_acc = 0.f, kd_acc = 0.f;
    const float invB = 1.0f / (float)B, invT = 1.0f / T;
    const bool kd = t || table;
    const float w_ce = kd ? (1.0f - alpha) : 1.0f, w_kd = kd ? alpha : 0.0f;
    for (int b = threadIdx.x; b < B; b += blockDim.x) {
        const int32_t* rec = mix + (int64_t)b * 6;
        const int p = (unsigned)rec[0] < (unsigned)B ? rec[0] : b;
        const float lam = __int_as_float(rec[5]);
        float* dr = dlogits + (int64_t)b * C;
        const float *tr = t ? t + (int64_t)b * C : nullptr, *tr2 = nullptr;
        if (table) {
            const int64_t i = index[b], i2 = lam != 1.0f ? index[p] : i;
            if (i < 0 || i >= rows || i2 < 0 || i2 >= rows) {
                for (int c = 0; c < C; ++c) dr[c] = NAN;
                ce_acc = NAN;
                kd_acc = NAN;
                continue;
            }
            tr = table + i * C;
            if (lam != 1.0f) tr2 = table + i2 * C;
        }
        kd_ce_row<true>(s + (int64_t)b * C, tr, (int)labels[b], C, T, invT, invB, w_ce, w_kd, eps, ce_acc, kd_acc, dr, tr2, (int)labels[p], lam);
    }
    kd_ce_finish(ce_acc, kd_acc, invB, T, w_ce, w_kd, out3);
}

int launch_kd_ce_loss(const float* student, const float* teacher, const int64_t* labels, int64_t batch, int64_t classes, float kd_temp,
                      float kd_alpha, float label_smoothing, float* out3, float* dlogits, hipStream_t st) {
    k_kd_ce<<<1, 256, 0, st>>>(student, teacher, labels, (int)batch, (int)classes, kd_temp, kd_alpha, label_smoothing, out3, dlogits);
    return 0;
}

int launch_kd_ce_loss_table(const float* student, const float* table, int64_t table_rows, const int64_t* index, const int64_t* labels, int64_t batch,
                            int64_t classes, float kd_temp, float kd_alpha, float label_smoothing, float* out3, float* dlogits, hipStream_t st) {
    k_kd_ce_table<<<1, 256, 0, st>>>(student, table, table_rows, index, labels, (int)batch, (int)classes, kd_temp, kd_alpha, label_smoothing, out3,
                                     dlogits);
    return 0;
}

int launch_kd_ce_loss_mix(const float* student, const float* teacher, const float* table, int64_t table_rows, const int64_t* index,
                          const int64_t* labels, const int32_t* mix, int64_t batch, int64_t classes, float kd_temp, float kd_alpha,
                          float label_smoothing, float* out3, float* dlogits, hipStream_t st) {
    if (!mix)
        return table ? launch_kd_ce_loss_table(student, table, table_rows, index, labels, batch, classes, kd_temp, kd_alpha, label_smoothing, out3,
                                               dlogits, st)
                     : launch_kd_ce_loss(student, teacher, labels, batch, classes, kd_temp, kd_alpha, label_smoothing, out3, dlogits, st);
    k_kd_ce_mix<<<1, 256, 0, st>>>(student, teacher, table, table_rows, index, labels, mix, (int)batch, (int)classes, kd_temp, kd_alpha,
                                   label_smoothing, out3, dlogits);
    return 0;
}

}  // namespace qv
