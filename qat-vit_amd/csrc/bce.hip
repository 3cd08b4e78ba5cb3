// KD (temperature-scaled KL, batchmean) + binary cross-entropy with logits on the smoothed, mixed and optionally thresholded targets, forward and
// d/dlogits (include/qatvit.h, qatvit_kd_bce_loss).  The hard targets are the ones loss.hip forms for the CE entries, used
// element-wise as timm's BinaryCrossEntropy uses them; the KD part is kd_ce_row's, term for term.
//   k_kd_bce         one wave per batch row, 4 rows per workgroup: the lanes stride over the classes, so every read of the student's and the teacher's
//                    rows and every write of dlogits is coalesced, and a row's max and sums are one wave butterfly each.  Writes the row's
//                    {bce_sum, kd_sum} to partials[2 * b].
//   k_kd_bce_finish  one workgroup: adds the partials up in double in one fixed order and writes out3.  No atomics, no ticket: the same inputs give
//                    the same bits.
#include "qv_common.h"
#include "qv_kernels.h"

namespace qv {

static constexpr int kBceRowsPerBlock = 4, kBceFinishThreads = 256;

__global__ __launch_bounds__(64 * kBceRowsPerBlock) void k_kd_bce(const float* __restrict__ s, const float* __restrict__ t,
                                                                  const float* __restrict__ table, int64_t rows,
                                                                  const int64_t* __restrict__ index, const int64_t* __restrict__ labels,
                                                                  const int32_t* __restrict__ mix, int B, int C, float T, float alpha, float eps,
                                                                  float thr, float scale, float* __restrict__ partials,
                                                                  float* __restrict__ dlogits) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * kBceRowsPerBlock + (threadIdx.x >> 6);
    if (b >= B) return;   // the whole wave: no barrier follows
    const bool kd = t || table;
    const float w_hard = kd ? (1.0f - alpha) : 1.0f, w_kd = kd ? alpha : 0.0f;
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
        if (i < 0 || i >= rows || i2 < 0 || i2 >= rows) {
            for (int c = lane; c < C; c += 64) dr[c] = NAN;
            if (lane == 0) { partials[2 * (int64_t)b] = NAN; partials[2 * (int64_t)b + 1] = NAN; }
            return;
        }
        tr = table + i * C;
        if (lam != 1.0f) tr2 = table + i2 * C;
    }
    // the KD part's row statistics (kd_ce_row's m1, zT, mt, zq, mt2, zq2), each lane over its classes, then one butterfly
    float m1 = -INFINITY, mt = -INFINITY, mt2 = -INFINITY, lzT = 0.f, lzq = 0.f, lzq2 = 0.f;
    if (tr) {
        for (int c = lane; c < C; c += 64) {
            m1 = fmaxf(m1, sr[c]);
            mt = fmaxf(mt, tr[c]);
            if (tr2) mt2 = fmaxf(mt2, tr2[c]);
        }
        m1 = wave_max(m1);
        mt = wave_max(mt);
        mt2 = wave_max(mt2);
        float zT = 0.f, zq = 0.f, zq2 = 0.f;
        for (int c = lane; c < C; c += 64) {
            zT += expf((sr[c] - m1) * invT);
            zq += expf((tr[c] - mt) * invT);
            if (tr2) zq2 += expf((tr2[c] - mt2) * invT);
        }
        lzT = logf(wave_sum(zT));
        lzq = logf(wave_sum(zq));
        lzq2 = tr2 ? logf(wave_sum(zq2)) : 0.f;
    }
    float bce_acc = 0.f, kd_acc = 0.f;
    for (int c = lane; c < C; c += 64) {
        const float x = sr[c];
        float tg = (1.0f - eps) * (lam * (c == y ? 1.0f : 0.0f) + oml * (c == y2 ? 1.0f : 0.0f)) + eps / (float)C;
        if (thr >= 0.f) tg = tg > thr ? 1.0f : 0.0f;
        const float e = expf(-fabsf(x));                                  // expf(-x) where x >= 0, expf(x) where x < 0
        bce_acc += fmaxf(x, 0.f) - x * tg + log1pf(e);
        const float sg = x >= 0.f ? 1.0f / (1.0f + e) : e / (1.0f + e);   // a NaN logit takes the second branch: NaN
        float g = w_hard * (sg - tg) * scale;
        if (tr) {
            const float lpT = (x - m1) * invT - lzT;    // log_softmax(s/T)
            float lq = (tr[c] - mt) * invT - lzq;
            float q = expf(lq);
            if (tr2) {
                q = lam * q + oml * expf((tr2[c] - mt2) * invT - lzq2);
                lq = q > 0.f ? logf(q) : 0.f;           // 0 * log 0 = 0
            }
            kd_acc += q * (lq - lpT);
            g += w_kd * T * (expf(lpT) - q) * invB;
        }
        dr[c] = g;
    }
    bce_acc = wave_sum(bce_acc);
    kd_acc = wave_sum(kd_acc);
    if (lane == 0) { partials[2 * (int64_t)b] = bce_acc; partials[2 * (int64_t)b + 1] = kd_acc; }
}

__device__ inline double bce_wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// thread i takes rows i, i + 256, ... in double, then one butterfly per wave, then the four waves in one order
__global__ __launch_bounds__(kBceFinishThreads) void k_kd_bce_finish(const float* __restrict__ partials, int B, float T, float alpha, int kd,
                                                                     float scale, float* __restrict__ out3) {
    __shared__ double sh[2][kBceFinishThreads / 64];
    double sb = 0.0, sk = 0.0;
    for (int b = threadIdx.x; b < B; b += kBceFinishThreads) {
        sb += (double)partials[2 * (int64_t)b];
        sk += (double)partials[2 * (int64_t)b + 1];
    }
    sb = bce_wave_sum_f64(sb);
    sk = bce_wave_sum_f64(sk);
    if ((threadIdx.x & 63) == 0) { sh[0][threadIdx.x >> 6] = sb; sh[1][threadIdx.x >> 6] = sk; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double w_hard = kd ? 1.0 - (double)alpha : 1.0, w_kd = kd ? (double)alpha : 0.0;
        const double bce = ((sh[0][0] + sh[0][1]) + (sh[0][2] + sh[0][3])) * (double)scale;
        const double kdv = ((sh[1][0] + sh[1][1]) + (sh[1][2] + sh[1][3])) / (double)B * (double)T * (double)T;
        out3[0] = (float)(w_kd * kdv + w_hard * bce);
        out3[1] = (float)bce;
        out3[2] = (float)kdv;
    }
}

int launch_kd_bce_loss(const float* student, const float* teacher, const float* table, int64_t table_rows, const int64_t* index,
                       const int64_t* labels, const int32_t* mix, int64_t batch, int64_t classes, float kd_temp, float kd_alpha,
                       float label_smoothing, float target_threshold, bool sum_classes, float* partials, float* out3, float* dlogits,
                       hipStream_t st) {
    const int B = (int)batch, C = (int)classes;
    const float scale = sum_classes ? 1.0f / (float)B : 1.0f / ((float)B * (float)C);
    k_kd_bce<<<(B + kBceRowsPerBlock - 1) / kBceRowsPerBlock, 64 * kBceRowsPerBlock, 0, st>>>(
        student, teacher, table, table_rows, index, labels, mix, B, C, kd_temp, kd_alpha, label_smoothing, target_threshold, scale, partials, dlogits);
    k_kd_bce_finish<<<1, kBceFinishThreads, 0, st>>>(partials, B, kd_temp, kd_alpha, teacher || table ? 1 : 0, scale, out3);
    return 0;
}

}  // namespace qv
