// The teacher block of the sparse-table BCE kernels (bce_topk.hip: k_kd_bce_topk; loss_rows16.hip: k_kd_bce_topk16): a compressed row, and under a mix
// record its partner's, as a class bitmap, an open-addressing hash of (class, Q, log Q) and one (Q, log Q) for every other class.  bce_topk.hip states
// the layout and the rules.  k_kd_bce_topk keeps its own inline statement of the build and the lookup (its machine code is unchanged); tk_build and
// tk_lookup are those statements, one for one, for k_kd_bce_topk16, so the two kernels' KD targets have the same bits.
#pragma once
#include "qv_common.h"

namespace qv {

static constexpr int kTkSlots = 256;   // hash slots per row slot: twice the 128 entries a row and its partner can hold

template <int BM>
struct TkBlock {
    int key[kTkSlots];     // the class, -1: free
    float q[kTkSlots];     // while the block is built: the row's own probability (default: its tail's); then Q
    float lq[kTkSlots];    // while the block is built: the partner's probability (default: its tail's); then log Q
    unsigned bm[BM];
    float q0, lq0;
};

__device__ __forceinline__ int tk_hash(int c) { return (int)(((unsigned)c * 0x9E3779B1u) >> 24); }

// orders the LDS accesses of the lanes of ONE wave: the hardware executes a wave's LDS operations in order, this keeps the compiler from moving them
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// One compressed row, lane e holding entry e: which entries are live, and the log-probabilities at temperature T of the entry and of the tail.
struct TkRow {
    int c;          // the class of this lane's entry; -1: not live
    float lq, lq0;  // log q of the entry, log q of a tail class
};
__device__ __forceinline__ TkRow tk_row(const int16_t* __restrict__ tidx, const float* __restrict__ tval, const float* __restrict__ ttail, int64_t i,
                                        int k, int C, float invT, int lane) {
    int c = -1;
    float v = 0.f;
    if (lane < k) { c = tidx[i * k + lane]; v = tval[i * k + lane]; }
    const float u = ttail[i];
    bool live = c >= 0 && c < C;
    for (int e = 1; e < k; ++e) {   // every lane takes part in the shuffle
        const int later = __shfl(c, e, 64);
        live = live && !(e > lane && later == c);
    }
    const int n = __builtin_popcountll(__builtin_amdgcn_ballot_w64(live));
    const float mt = fmaxf(wave_max(live ? v : -INFINITY), u);
    const float eu = expf((u - mt) * invT);
    const float zq = wave_sum(live ? expf((v - mt) * invT) : 0.f) + (float)(C - n) * eu;
    const float lzq = logf(zq);
    TkRow r;
    r.c = live ? c : -1;
    r.lq = (v - mt) * invT - lzq;
    r.lq0 = (u - mt) * invT - lzq;
    return r;
}

// the slot of class c, claimed if it has none yet: at most 128 of the 256 slots are ever in use, so the probe ends
__device__ __forceinline__ int tk_insert(int* key, int c) {
    int h = tk_hash(c);
    for (;;) {
        const int old = atomicCAS(&key[h], -1, c);
        if (old == -1 || old == c) return h;
        h = (h + 1) & (kTkSlots - 1);
    }
}

// The block of table row i (and, where `two`, of its partner's row i2 mixed in with lam / oml), built by ONE wave with lane e holding entry e
template <int BM>
__device__ __forceinline__ void tk_build(TkBlock<BM>& blk, const int16_t* __restrict__ tidx, const float* __restrict__ tval,
                                         const float* __restrict__ ttail, int64_t i, int64_t i2, bool two, float lam, float oml, int k, int C, float invT,
                                         int lane) {
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

// (Q, log Q) of class c from a finished block: the tail's pair unless the class's bit is set, then its hash slot - the rare path
template <int BM>
__device__ __forceinline__ void tk_lookup(const TkBlock<BM>& blk, int c, float& q, float& lq) {
    if ((blk.bm[c >> 5] >> (c & 31)) & 1u) {
        int h = tk_hash(c);
        for (int n = 0; n < kTkSlots && blk.key[h] != c; ++n) h = (h + 1) & (kTkSlots - 1);
        q = blk.q[h];
        lq = blk.lq[h];
    }
}

}  // namespace qv
