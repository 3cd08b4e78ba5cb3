// KD + binary cross-entropy with logits, class-parallel to 32768 classes, with the teacher read from the COMPRESSED table in its sparse form
// (include/qatvit.h, qatvit_kd_bce_loss_topk).  A compressed row is at most 64 explicit classes and ONE logit for all the
// others, so the KD target of a row (and of its partner under a mix record) is at most 128 explicit probabilities and one constant.  The dense
// teacher row never exists, in LDS or anywhere else, and expf / logf of the teacher run once per ENTRY, not once per class.
//   k_kd_bce_topk<NT, NPL>  the class ownership of k_kd_ce_rows (loss_rows.hip): NT threads share a row, thread t owns the classes t + NT * j.
//       NT = 64   (2 <= C <= 1024)   one wave per row, 4 rows per 256-thread workgroup; NPL = 1, 4, 16 student values per lane.  No barrier.
//       NT = 256  (1024 < C <= 32768) one workgroup per row; NPL = 16 up to C = 4096, NPL = 0 above (the sweeps re-read the student's row, in L2).
//     The teacher block of a row slot (4 slots in the wave form, 1 in the workgroup form), in LDS, prepared by ONE wave with lane e holding entry e:
//       bm[ceil(C / 32)]   the class bitmap: bit c set <=> class c has an entry
//       key/q/lq[256]      the entries as an open-addressing hash on the class (multiplicative hash, linear probing, at most 128 of 256 slots in
//                          use): the class, Q and log Q.  Lanes insert in parallel with an LDS compare-and-swap; where an entry lands depends on who
//                          wins, what a lookup returns does not
//       q0, lq0            Q and log Q of every class without an entry
//     An entry is live iff its class is in [0, C) and no later entry of its row names the class (the header's decompression rule); with n live
//     entries  mt = max(live val, u),  zq = sum_live expf((val - mt) / T) + (C - n) * expf((u - mt) / T)  by one butterfly.  Under a live mix record
//     the partner's row is prepared the same way into the same hash (slot defaults: the two tails), and one pass over the 256 slots forms
//     Q = lam * q + oml * q' and log Q once per entry.
//     The student sweeps are k_kd_bce's (bce.hip): maximum; zT; terms and gradient.  In the last one a lane reads its class's bit (the 64 lanes of a
//     wave read two neighbouring words) and takes (q0, lq0) unless it is set; with the bit set it probes the hash - the rare path.
//   k_kd_bce_finish (bce.hip, unedited) forms out3.  Two launches, no global atomics, no zeroed state: the same inputs give the same bits.
#include "bce_topk.h"
#include "loss_rows.h"
#include "qv_common.h"
#include "qv_kernels.h"

namespace qv {

template <int NT, int NPL>
__global__ __launch_bounds__(256) void k_kd_bce_topk(const float* __restrict__ s, const int16_t* __restrict__ tidx, const float* __restrict__ tval,
                                                     const float* __restrict__ ttail, int64_t rows, int k, const int64_t* __restrict__ index,
                                                     const int64_t* __restrict__ labels, const int32_t* __restrict__ mix, int B, int C, float T,
                                                     float alpha, float eps, float thr, float scale, float* __restrict__ partials,
                                                     float* __restrict__ dlogits) {
    constexpr int R = NPL > 0 ? NPL : 1;
    constexpr int BM = NT == 64 ? kRowsWaveMaxC / 32 : 32768 / 32;
    __shared__ TkBlock<BM> blocks[NT == 64 ? 4 : 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int tid = NT == 64 ? lane : threadIdx.x;
    const int b = NT == 64 ? blockIdx.x * 4 + wave : blockIdx.x;
    if (b >= B) return;   // NT = 64 only, the whole wave: the wave form has no barrier
    TkBlock<BM>& blk = blocks[NT == 64 ? wave : 0];
    const bool kd = tidx != nullptr;
    const float w_hard = kd ? (1.0f - alpha) : 1.0f, w_kd = kd ? alpha : 0.0f;
    const float invB = 1.0f / (float)B, invT = 1.0f / T;
    // the record: a row with lam == 1 (or without a record) is its own partner
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
    const bool two = kd && lam != 1.0f;
    int64_t i = 0, i2 = 0;
    if (kd) {
        i = index[b];
        i2 = two ? index[p] : i;
        if (i < 0 || i >= rows || i2 < 0 || i2 >= rows) {   // the whole row, so (NT = 256) the whole workgroup leaves before any barrier
            for (int c = tid; c < C; c += NT) dr[c] = NAN;
            if (tid == 0) { partials[2 * (int64_t)b] = NAN; partials[2 * (int64_t)b + 1] = NAN; }
            return;
        }
    }
    // the student's row into registers: every load is issued here, before the first use and before the teacher block is built
    float sv[R];
    if constexpr (NPL > 0) for_owned<NT, NPL>(tid, C, [&](int j, int c) { sv[j] = sr[c]; });
    auto S = [&](int j, int c) { return NPL > 0 ? sv[j] : sr[c]; };

    // (the block's build below and the lookup in the last sweep have a twin, statement for statement, in bce_topk.h - tk_build, tk_lookup - that
    // k_kd_bce_topk16 calls; this kernel keeps them inline, which keeps its register allocation.  A change to one is a change to both.)
    // the teacher block, by one wave.  NT = 256: the other waves go on to the student sweeps; the barriers of their two reductions, which this wave
    // meets after the block is complete, make it visible to them before the last sweep reads it
    if (kd && (NT == 64 || wave == 0)) {
        const TkRow r0 = tk_row(tidx, tval, ttail, i, k, C, invT, lane);
        TkRow r1 = r0;
        if (two) r1 = tk_row(tidx, tval, ttail, i2, k, C, invT, lane);
        const float t0 = expf(r0.lq0), t1 = expf(r1.lq0);
#pragma unroll
        for (int h = lane; h < kTkSlots; h += 64) { blk.key[h] = -1; blk.q[h] = t0; blk.lq[h] = t1; }
        for (int w = lane; w < (C + 31) / 32; w += 64) blk.bm[w] = 0u;
        wave_lds_sync();
        if (r0.c >= 0) {
            const int h = tk_insert(blk.key, r0.c);
            atomicOr(&blk.bm[r0.c >> 5], 1u << (r0.c & 31));
            blk.q[h] = expf(r0.lq);
            if (!two) blk.lq[h] = r0.lq;   // unmixed: log Q is the log-probability itself, no logarithm at all
        }
        if (two) {
            wave_lds_sync();
            if (r1.c >= 0) {   // joins the row's own entry of the class where there is one
                const int h = tk_insert(blk.key, r1.c);
                atomicOr(&blk.bm[r1.c >> 5], 1u << (r1.c & 31));
                blk.lq[h] = expf(r1.lq);
            }
            wave_lds_sync();
#pragma unroll
            for (int h = lane; h < kTkSlots; h += 64) {   // one logarithm per entry
                if (blk.key[h] >= 0) {
                    const float q = lam * blk.q[h] + oml * blk.lq[h];
                    blk.q[h] = q;
                    blk.lq[h] = q > 0.f ? logf(q) : 0.f;   // 0 * log 0 = 0
                }
            }
        }
        if (lane == 0) {
            const float q = lam * t0 + oml * t1;
            blk.q0 = two ? q : t0;
            blk.lq0 = two ? (q > 0.f ? logf(q) : 0.f) : r0.lq0;
        }
        wave_lds_sync();
    }

    // sweeps 1 and 2 of the student's row: m1 and zT (the KD part alone needs them)
    float m1 = 0.f, lzT = 0.f;
    if (kd) {
        float mx[1] = {-INFINITY};
        for_owned<NT, NPL>(tid, C, [&](int j, int c) { mx[0] = fmaxf(mx[0], S(j, c)); });
        row_reduce<NT, 0, true>(mx);
        m1 = mx[0];
        float z[1] = {0.f};
        for_owned<NT, NPL>(tid, C, [&](int j, int c) { z[0] += expf((S(j, c) - m1) * invT); });
        row_reduce<NT, 1, false>(z);
        lzT = logf(z[0]);
    }
    const float q0 = kd ? blk.q0 : 0.f, lq0 = kd ? blk.lq0 : 0.f;
    // sweep 3: the terms and the gradient (k_kd_bce, term for term)
    float acc[2] = {0.f, 0.f};   // bce, kd
    for_owned<NT, NPL>(tid, C, [&](int j, int c) {
        const float x = S(j, c);
        float tg = (1.0f - eps) * (lam * (c == y ? 1.0f : 0.0f) + oml * (c == y2 ? 1.0f : 0.0f)) + eps / (float)C;
        if (thr >= 0.f) tg = tg > thr ? 1.0f : 0.0f;
        const float e = expf(-fabsf(x));                                  // expf(-x) where x >= 0, expf(x) where x < 0
        acc[0] += fmaxf(x, 0.f) - x * tg + log1pf(e);
        const float sg = x >= 0.f ? 1.0f / (1.0f + e) : e / (1.0f + e);   // a NaN logit takes the second branch: NaN
        float g = w_hard * (sg - tg) * scale;
        if (kd) {
            const float lpT = (x - m1) * invT - lzT;    // log_softmax(s/T)
            float q = q0, lq = lq0;
            if ((blk.bm[c >> 5] >> (c & 31)) & 1u) {    // the class has an entry: it is in the hash
                int h = tk_hash(c);
                for (int n = 0; n < kTkSlots && blk.key[h] != c; ++n) h = (h + 1) & (kTkSlots - 1);
                q = blk.q[h];
                lq = blk.lq[h];
            }
            acc[1] += q * (lq - lpT);
            g += w_kd * T * (expf(lpT) - q) * invB;
        }
        dr[c] = g;
    });
    row_reduce<NT, 2, false>(acc);
    if (tid == 0) { partials[2 * (int64_t)b] = acc[0]; partials[2 * (int64_t)b + 1] = acc[1]; }
}

int launch_kd_bce_loss_topk(const float* student, const int16_t* idx, const float* val, const float* tail, int64_t table_rows, int k,
                            const int64_t* index, const int64_t* labels, const int32_t* mix, int64_t batch, int64_t classes, float kd_temp,
                            float kd_alpha, float label_smoothing, float target_threshold, bool sum_classes, float* partials, float* out3,
                            float* dlogits, hipStream_t st) {
    const int B = (int)batch, C = (int)classes;
    const float scale = sum_classes ? 1.0f / (float)B : 1.0f / ((float)B * (float)C);
#define QV_BCE_TOPK(NT, NPL, GRID)                                                                                                                  \
    k_kd_bce_topk<NT, NPL><<<GRID, 256, 0, st>>>(student, idx, val, tail, table_rows, k, index, labels, mix, B, C, kd_temp, kd_alpha, label_smoothing, \
                                                 target_threshold, scale, partials, dlogits)
    if (C <= 64) QV_BCE_TOPK(64, 1, (B + 3) / 4);
    else if (C <= 256) QV_BCE_TOPK(64, 4, (B + 3) / 4);
    else if (C <= kRowsWaveMaxC) QV_BCE_TOPK(64, 16, (B + 3) / 4);
    else if (C <= kRowsRegMaxC) QV_BCE_TOPK(256, 16, B);
    else QV_BCE_TOPK(256, 0, B);
#undef QV_BCE_TOPK
    k_kd_bce_finish<<<1, 256, 0, st>>>(partials, B, kd_temp, kd_alpha, idx ? 1 : 0, scale, out3);
    return 0;
}

}  // namespace qv
