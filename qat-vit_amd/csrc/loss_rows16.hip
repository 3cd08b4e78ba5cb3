// The class-parallel losses on fp16 / bf16 student logits, with the gradient written in the same 16-bit type (include/qatvit.h,
// qatvit_kd_ce_loss_rows16 / _topk16 / qatvit_kd_bce_loss_topk16).  x = (float)logit is exact and every expression after it is the
// fp32 kernels' (loss_rows.hip, teacher_topk.hip, bce_topk.hip), operation for operation, in fp32; the finished gradient g is rounded ONCE, to
// (E)(g * s) with s = *grad_scale (1 without one).  What is new is how a row is owned and moved:
//   Ownership.  Row b starts at byte 2 b C, so it is 16-byte aligned only where C % 8 == 0.  With h = the elements in front of the row's first 16-byte
//   boundary (0 .. 7, at most C), nb = (C - h) / 8 and ts = h + 8 nb, the row is
//       head   classes [0, h)       thread t < h owns class t                       } the "edge": at most ONE class per thread, h + (C - ts) <= 14,
//       tail   classes [ts, C)      thread t, h <= t < h + C - ts, owns ts + t - h  } moved with 2-byte loads and stores
//       body   classes [h, ts)      group g = classes h + 8 g .. h + 8 g + 7 belongs to thread g % NT, its slot j = g / NT: thread t owns 8 t + 8 NT j + 0 .. 7
//                                   counted from the boundary.  One 16-byte load per group; the 8 logits stay PACKED, 4 VGPRs per group.
//   dlogits is written with one 16-byte store per group where the dlogits row has the student row's phase modulo 16 bytes (always so for two tensors of
//   one allocator), else with eight 2-byte stores.
//   k_kd_ce_rows16<E, NT, NJ, TOPK>, k_kd_bce_topk16<E, NT, NJ>   NT threads share one row.
//       NT = 64   (2 <= C <= 1024)    one wave per row, 4 rows per 256-thread workgroup; NJ = 1 (C <= 512) or 2 groups per lane.  No barrier.
//       NT = 256  (1024 < C <= 32768) one workgroup per row; NJ = 2 (C <= 4096), NJ = 4 (C <= 8192), NJ = 0 above.
//     NJ > 0: the student's row is read ONCE, every load issued before the first use, and the three sweeps run over the packed registers.  The bound of
//     this form is 8 * 256 * NJ classes: NJ = 4 is 16 VGPRs of row (the fp32 form holds 16 for 4096 classes), and the unpacked values of one group, 8
//     more, live only inside a sweep (profiles/loss16_resource_usage.txt: 70 - 79 VGPRs, scratch 0); NJ = 8 (16384 classes) would hold 32 on top of
//     that and was not built.  NJ = 0: the sweeps re-read the row (it sits in L2), still 16 bytes per load.
//     The teacher stays fp32 and is read where it is used: a teacher tensor / dense table row from global memory in every sweep (it would cost four
//     times the student's registers), a compressed row (TOPK) decompressed into LDS one slot at a time - the 8 NT classes of slot j, filled with the
//     tail's logit by the threads of the row and overwritten by the entries that fall into it, each wave scattering onto the words its own lanes
//     filled (a wave's LDS operations execute in order; of entries with the same class only the last takes part) - or bce_topk.h's sparse block.
//   Summation order.  Per thread: the edge class first, then the groups in ascending j, the 8 classes of a group in ascending order; over the threads
//   row_reduce (loss_rows.h): butterflies over a wave, the four waves as (0 + 1) + (2 + 3).  k_kd_bce_finish (bce.hip, unedited) forms out3 in double.
//   Two launches, no atomics, no zeroed state: the same inputs (and the same row phases) give the same bits.
#include "bce_topk.h"
#include "loss_rows.h"
#include "qv_common.h"
#include "qv_kernels.h"

namespace qv {

static constexpr int kRows16WaveOneC = 512, kRows16TwoC = 4096, kRows16RegMaxC = 8192;

template <class E> __device__ __forceinline__ float up16(uint32_t lo16);   // the 16-bit pattern in the low half -> fp32, exact
template <> __device__ __forceinline__ float up16<_Float16>(uint32_t b) { return (float)__builtin_bit_cast(_Float16, (uint16_t)b); }
template <> __device__ __forceinline__ float up16<__bf16>(uint32_t b) { return __uint_as_float(b << 16); }
// one round-to-nearest-even conversion; fp16 overflow gives +-inf
template <class E> __device__ __forceinline__ uint32_t down16(float v) { return (uint32_t)__builtin_bit_cast(uint16_t, (E)v); }

template <int NT> __device__ __forceinline__ void row_sync() {   // orders the LDS traffic of the threads of one row
    if constexpr (NT == 64) wave_lds_sync();
    else __syncthreads();
}

// A thread's share of row b (the header states the ownership).  pass<STORE>(prep, f): prep(j) by every thread of the row before the edge (j = -1) and
// before each slot j that holds a group, then r = f(c, li, x) for every owned class in the summation order, li = the thread index (edge) or the
// class's offset in its slot; STORE: (E)(r * gs) goes to dlogits.
template <class E, int NT, int NJ>
struct Row16 {
    static constexpr int R = NJ > 0 ? NJ : 1;
    const E* sr;
    E* dr;
    int tid, h, nb, ts, C, ec;
    bool same_phase;
    float gs, ex;
    uint4 v[R];

    __device__ __forceinline__ Row16(const E* s, E* d, int64_t b, int C_, int tid_, float gs_) : sr(s + b * C_), dr(d + b * C_), tid(tid_), C(C_), gs(gs_) {
        h = (int)(((16u - (unsigned)((uintptr_t)sr & 15u)) & 15u) >> 1);
        if (h > C) h = C;
        nb = (C - h) >> 3;
        ts = h + 8 * nb;
        ec = tid < h ? tid : (tid - h < C - ts ? ts + tid - h : -1);
        same_phase = (((uintptr_t)sr ^ (uintptr_t)dr) & 15u) == 0;
        ex = 0.f;
    }
    __device__ __forceinline__ const uint4* group(int g) const { return reinterpret_cast<const uint4*>(sr + h + 8 * g); }
    __device__ __forceinline__ void load() {
        if (ec >= 0) ex = (float)sr[ec];
        if constexpr (NJ > 0) {
#pragma unroll
            for (int j = 0; j < NJ; ++j)
                if (tid + NT * j < nb) v[j] = *group(tid + NT * j);
        }
    }
    // the edge slot of class c (what prep(-1) fills), -1: a body class or no class
    __device__ __forceinline__ int edge_slot(int c) const { return c < 0 || c >= C ? -1 : (c < h ? c : (c >= ts ? h + c - ts : -1)); }
    __device__ __forceinline__ void nan_row() const {
        for (int c = tid; c < C; c += NT) dr[c] = (E)NAN;
    }

    template <bool STORE, class P, class F>
    __device__ __forceinline__ void pass(P prep, F f) {
        prep(-1);
        if (ec >= 0) {
            const float r = f(ec, tid, ex);
            if constexpr (STORE) dr[ec] = (E)(r * gs);
        }
        auto slot = [&](int j, const uint4& w) {
            const int cb = h + 8 * (tid + NT * j);
            const uint32_t in[4] = {w.x, w.y, w.z, w.w};
            uint32_t out[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const float x = up16<E>((i & 1) ? in[i >> 1] >> 16 : in[i >> 1] & 0xffffu);
                const float r = f(cb + i, 8 * tid + i, x);
                if constexpr (STORE) out[i >> 1] |= down16<E>(r * gs) << (16 * (i & 1));
            }
            if constexpr (STORE) {
                if (same_phase) {
                    *reinterpret_cast<uint4*>(dr + cb) = make_uint4(out[0], out[1], out[2], out[3]);
                } else {
#pragma unroll
                    for (int i = 0; i < 8; ++i) reinterpret_cast<uint16_t*>(dr)[cb + i] = (uint16_t)(out[i >> 1] >> (16 * (i & 1)));
                }
            }
        };
        if constexpr (NJ > 0) {
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                if (NT * j < nb) {   // the same for every thread of the row
                    prep(j);
                    if (tid + NT * j < nb) slot(j, v[j]);
                }
            }
        } else {
            for (int j = 0; NT * j < nb; ++j) {
                prep(j);
                if (tid + NT * j < nb) slot(j, *group(tid + NT * j));
            }
        }
    }
};

// The CE + KD rows kernel: k_kd_ce_rows' forms (teacher tensor, dense table, mix records, none) and, TOPK, k_kd_ce_topk's compressed table.
template <class E, int NT, int NJ, bool TOPK>
__global__ __launch_bounds__(256) void k_kd_ce_rows16(const E* __restrict__ s, const float* __restrict__ t, const float* __restrict__ table,
                                                      const int16_t* __restrict__ tidx, const float* __restrict__ tval, const float* __restrict__ ttail,
                                                      int64_t rows, int k, const int64_t* __restrict__ index, const int64_t* __restrict__ labels,
                                                      const int32_t* __restrict__ mix, int B, int C, float T, float alpha, float eps,
                                                      const float* __restrict__ gscale, float* __restrict__ partials, E* __restrict__ dlogits) {
    constexpr int W = 8 * NT;   // the classes of one slot
    __shared__ float dense[TOPK ? (NT == 64 ? 4 : 1) : 1][2][TOPK ? W : 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int tid = NT == 64 ? lane : threadIdx.x;
    const int b = NT == 64 ? blockIdx.x * 4 + wave : blockIdx.x;
    if (b >= B) return;   // NT = 64 only, the whole wave: the wave form has no barrier
    float* d0 = dense[NT == 64 && TOPK ? wave : 0][0];
    float* d1 = dense[NT == 64 && TOPK ? wave : 0][1];
    const bool kd = TOPK || t || table;
    const float w_ce = kd ? (1.0f - alpha) : 1.0f, w_kd = kd ? alpha : 0.0f;
    const float invB = 1.0f / (float)B, invT = 1.0f / T;
    float lam = 1.0f;
    int p = b;
    if (mix) {
        const int32_t* rec = mix + (int64_t)b * 6;
        lam = __int_as_float(rec[5]);
        if (lam != 1.0f && (unsigned)rec[0] < (unsigned)B) p = rec[0];
    }
    const float oml = 1.0f - lam;
    const int y = (int)labels[b], y2 = (int)labels[p];
    Row16<E, NT, NJ> row(s, dlogits, b, C, tid, gscale ? *gscale : 1.0f);
    int64_t i = 0, i2 = 0;
    if (TOPK || table) {
        i = index[b];
        i2 = lam != 1.0f ? index[p] : i;
        if (i < 0 || i >= rows || i2 < 0 || i2 >= rows) {   // the whole row, so (NT = 256) the whole workgroup leaves before any barrier
            row.nan_row();
            if (tid == 0) { partials[2 * (int64_t)b] = NAN; partials[2 * (int64_t)b + 1] = NAN; }
            return;
        }
    }
    row.load();
    const float *tr = nullptr, *tr2 = nullptr;
    if (!TOPK) {
        tr = t ? t + (int64_t)b * C : (table ? table + i * C : nullptr);
        if (table && lam != 1.0f) tr2 = table + i2 * C;
    }
    const bool two = TOPK ? lam != 1.0f : tr2 != nullptr;
    // TOPK: lane e of every wave holds entry e of the row and of the partner's row; an entry takes part if its class is in [0, C) and no later entry
    // names the same class
    int ec[2] = {-1, -1};
    float ev[2] = {0.f, 0.f}, u[2] = {0.f, 0.f};
    if constexpr (TOPK) {
        u[0] = ttail[i];
        if (two) u[1] = ttail[i2];
        if (lane < k) {
            ec[0] = tidx[i * k + lane]; ev[0] = tval[i * k + lane];
            if (two) { ec[1] = tidx[i2 * k + lane]; ev[1] = tval[i2 * k + lane]; }
        }
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            bool keep = ec[r] >= 0 && ec[r] < C;
            for (int e = 1; e < k && __builtin_amdgcn_ballot_w64(keep) != 0; ++e) {
                const int later = __shfl(ec[r], e, 64);   // every lane takes part
                keep = keep && !(e > lane && later == ec[r]);
            }
            if (!keep) ec[r] = -1;
        }
    }
    // the teacher's logits of slot j (-1: of the edge) into LDS, between two synchronisations of the row's threads
    auto prep = [&](int j) {
        if constexpr (TOPK) {
            row_sync<NT>();   // every thread has read the slot before
            if (j < 0) {
                if (tid < 16) { d0[tid] = u[0]; if (two) d1[tid] = u[1]; }
                const int s0 = row.edge_slot(ec[0]), s1 = row.edge_slot(ec[1]);
                if (NT == 64 || wave == 0) {
                    if (s0 >= 0) d0[s0] = ev[0];
                    if (two && s1 >= 0) d1[s1] = ev[1];
                }
            } else {
#pragma unroll
                for (int m = 0; m < 8; ++m) { d0[tid + NT * m] = u[0]; if (two) d1[tid + NT * m] = u[1]; }
                const int lo = row.h + W * j, l0 = ec[0] - lo, l1 = ec[1] - lo;
                if (ec[0] >= 0 && ec[0] < row.ts && l0 >= 0 && l0 < W && (NT == 64 || ((l0 & (NT - 1)) >> 6) == wave)) d0[l0] = ev[0];
                if (two && ec[1] >= 0 && ec[1] < row.ts && l1 >= 0 && l1 < W && (NT == 64 || ((l1 & (NT - 1)) >> 6) == wave)) d1[l1] = ev[1];
            }
            row_sync<NT>();
        }
    };
    auto Q = [&](int c, int li) { return TOPK ? d0[li] : tr[c]; };
    auto Q2 = [&](int c, int li) { return TOPK ? d1[li] : tr2[c]; };
    // true where every active lane of the wave holds the tail's logit: its terms are then the row's one tail term (the same bits)
    auto all_tail = [&](float q, float ut) { return TOPK && __builtin_amdgcn_ballot_w64(__float_as_uint(q) != __float_as_uint(ut)) == 0; };

    // sweep 1: the maxima m1, mt, mt2
    float mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    row.template pass<false>(prep, [&](int c, int li, float x) {
        mx[0] = fmaxf(mx[0], x);
        if (kd) mx[1] = fmaxf(mx[1], Q(c, li));
        if (two) mx[2] = fmaxf(mx[2], Q2(c, li));
        return 0.f;
    });
    row_reduce<NT, 0, true>(mx);
    const float m1 = mx[0], mt = mx[1], mt2 = mx[2];
    // sweep 2: the partition sums z1, zT, zq, zq2
    const float eu = TOPK ? expf((u[0] - mt) * invT) : 0.f, eu2 = TOPK && two ? expf((u[1] - mt2) * invT) : 0.f;
    float z[4] = {0.f, 0.f, 0.f, 0.f};
    row.template pass<false>(prep, [&](int c, int li, float x) {
        const float d = x - m1;
        z[0] += expf(d);
        if (kd) {
            z[1] += expf(d * invT);
            const float q = Q(c, li);
            z[2] += all_tail(q, u[0]) ? eu : expf((q - mt) * invT);
        }
        if (two) {
            const float q2 = Q2(c, li);
            z[3] += all_tail(q2, u[1]) ? eu2 : expf((q2 - mt2) * invT);
        }
        return 0.f;
    });
    row_reduce<NT, 1, false>(z);
    const float lz1 = logf(z[0]), lzT = kd ? logf(z[1]) : 0.f, lzq = kd ? logf(z[2]) : 0.f, lzq2 = two ? logf(z[3]) : 0.f;
    // sweep 3: the terms and the gradient (k_kd_ce_rows, term for term)
    const float qu = TOPK ? expf((u[0] - mt) * invT - lzq) : 0.f, qu2 = TOPK && two ? expf((u[1] - mt2) * invT - lzq2) : 0.f;
    float acc[2] = {0.f, 0.f};   // ce, kd
    row.template pass<true>(prep, [&](int c, int li, float x) {
        const float lp = x - m1 - lz1;                      // log_softmax(s)
        const float ysm = (1.0f - eps) * (lam * (c == y ? 1.0f : 0.0f) + oml * (c == y2 ? 1.0f : 0.0f)) + eps / (float)C;
        acc[0] -= ysm * lp;
        float g = w_ce * (expf(lp) - ysm) * invB;
        if (kd) {
            const float lpT = (x - m1) * invT - lzT;        // log_softmax(s/T)
            const float tq = Q(c, li);
            float lq = (tq - mt) * invT - lzq;
            float q = all_tail(tq, u[0]) ? qu : expf(lq);
            if (two) {
                const float tq2 = Q2(c, li);
                q = lam * q + oml * (all_tail(tq2, u[1]) ? qu2 : expf((tq2 - mt2) * invT - lzq2));
                lq = q > 0.f ? logf(q) : 0.f;               // 0 * log 0 = 0
            }
            acc[1] += q * (lq - lpT);
            g += w_kd * T * (expf(lpT) - q) * invB;
        }
        return g;
    });
    row_reduce<NT, 2, false>(acc);
    if (tid == 0) { partials[2 * (int64_t)b] = acc[0]; partials[2 * (int64_t)b + 1] = acc[1]; }
}

// The sparse-table BCE kernel: k_kd_bce_topk's teacher block (bce_topk.h) and expressions on a Row16.
template <class E, int NT, int NJ>
__global__ __launch_bounds__(256) void k_kd_bce_topk16(const E* __restrict__ s, const int16_t* __restrict__ tidx, const float* __restrict__ tval,
                                                       const float* __restrict__ ttail, int64_t rows, int k, const int64_t* __restrict__ index,
                                                       const int64_t* __restrict__ labels, const int32_t* __restrict__ mix, int B, int C, float T,
                                                       float alpha, float eps, float thr, float scale, const float* __restrict__ gscale,
                                                       float* __restrict__ partials, E* __restrict__ dlogits) {
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
    float lam = 1.0f;
    int p = b;
    if (mix) {
        const int32_t* rec = mix + (int64_t)b * 6;
        lam = __int_as_float(rec[5]);
        if (lam != 1.0f && (unsigned)rec[0] < (unsigned)B) p = rec[0];
    }
    const float oml = 1.0f - lam;
    const int y = (int)labels[b], y2 = (int)labels[p];
    Row16<E, NT, NJ> row(s, dlogits, b, C, tid, gscale ? *gscale : 1.0f);
    const bool two = kd && lam != 1.0f;
    int64_t i = 0, i2 = 0;
    if (kd) {
        i = index[b];
        i2 = two ? index[p] : i;
        if (i < 0 || i >= rows || i2 < 0 || i2 >= rows) {   // the whole row, so (NT = 256) the whole workgroup leaves before any barrier
            row.nan_row();
            if (tid == 0) { partials[2 * (int64_t)b] = NAN; partials[2 * (int64_t)b + 1] = NAN; }
            return;
        }
    }
    row.load();   // issued before the teacher block is built
    // the teacher block, by one wave.  NT = 256: the other waves go on to the student sweeps; the barriers of their two reductions, which this wave
    // meets after the block is complete, make it visible to them before the last sweep reads it
    if (kd && (NT == 64 || wave == 0)) tk_build(blk, tidx, tval, ttail, i, i2, two, lam, oml, k, C, invT, lane);

    auto none = [](int) {};
    float m1 = 0.f, lzT = 0.f;
    if (kd) {
        float mx[1] = {-INFINITY};
        row.template pass<false>(none, [&](int, int, float x) { mx[0] = fmaxf(mx[0], x); return 0.f; });
        row_reduce<NT, 0, true>(mx);
        m1 = mx[0];
        float z[1] = {0.f};
        row.template pass<false>(none, [&](int, int, float x) { z[0] += expf((x - m1) * invT); return 0.f; });
        row_reduce<NT, 1, false>(z);
        lzT = logf(z[0]);
    }
    const float q0 = kd ? blk.q0 : 0.f, lq0 = kd ? blk.lq0 : 0.f;
    // sweep 3: the terms and the gradient (k_kd_bce_topk, term for term)
    float acc[2] = {0.f, 0.f};   // bce, kd
    row.template pass<true>(none, [&](int c, int, float x) {
        float tg = (1.0f - eps) * (lam * (c == y ? 1.0f : 0.0f) + oml * (c == y2 ? 1.0f : 0.0f)) + eps / (float)C;
        if (thr >= 0.f) tg = tg > thr ? 1.0f : 0.0f;
        const float e = expf(-fabsf(x));
        acc[0] += fmaxf(x, 0.f) - x * tg + log1pf(e);
        const float sg = x >= 0.f ? 1.0f / (1.0f + e) : e / (1.0f + e);   // a NaN logit takes the second branch: NaN
        float g = w_hard * (sg - tg) * scale;
        if (kd) {
            const float lpT = (x - m1) * invT - lzT;    // log_softmax(s/T)
            float q = q0, lq = lq0;
            tk_lookup(blk, c, q, lq);
            acc[1] += q * (lq - lpT);
            g += w_kd * T * (expf(lpT) - q) * invB;
        }
        return g;
    });
    row_reduce<NT, 2, false>(acc);
    if (tid == 0) { partials[2 * (int64_t)b] = acc[0]; partials[2 * (int64_t)b + 1] = acc[1]; }
}

// the form of a class count: KERNEL<NT, NJ> on its grid
#define QV_ROWS16_FORMS(LAUNCH)                           \
    do {                                                  \
        if (C <= kRows16WaveOneC) LAUNCH(64, 1, (B + 3) / 4);      \
        else if (C <= kRowsWaveMaxC) LAUNCH(64, 2, (B + 3) / 4);   \
        else if (C <= kRows16TwoC) LAUNCH(256, 2, B);     \
        else if (C <= kRows16RegMaxC) LAUNCH(256, 4, B);  \
        else LAUNCH(256, 0, B);                           \
    } while (0)

template <class E, bool TOPK>
static void ce_rows16(const void* student, const float* teacher, const float* table, const int16_t* idx, const float* val, const float* tail,
                      int64_t table_rows, int k, const int64_t* index, const int64_t* labels, const int32_t* mix, int B, int C, float kd_temp,
                      float kd_alpha, float label_smoothing, const float* grad_scale, float* partials, void* dlogits, hipStream_t st) {
#define QV_CE16(NT, NJ, GRID)                                                                                                                        \
    k_kd_ce_rows16<E, NT, NJ, TOPK><<<GRID, 256, 0, st>>>(static_cast<const E*>(student), teacher, table, idx, val, tail, table_rows, k, index, labels, \
                                                          mix, B, C, kd_temp, kd_alpha, label_smoothing, grad_scale, partials, static_cast<E*>(dlogits))
    QV_ROWS16_FORMS(QV_CE16);
#undef QV_CE16
}

template <class E>
static void bce_topk16(const void* student, const int16_t* idx, const float* val, const float* tail, int64_t table_rows, int k, const int64_t* index,
                       const int64_t* labels, const int32_t* mix, int B, int C, float kd_temp, float kd_alpha, float label_smoothing, float thr,
                       float scale, const float* grad_scale, float* partials, void* dlogits, hipStream_t st) {
#define QV_BCE16(NT, NJ, GRID)                                                                                                                      \
    k_kd_bce_topk16<E, NT, NJ><<<GRID, 256, 0, st>>>(static_cast<const E*>(student), idx, val, tail, table_rows, k, index, labels, mix, B, C, kd_temp, \
                                                     kd_alpha, label_smoothing, thr, scale, grad_scale, partials, static_cast<E*>(dlogits))
    QV_ROWS16_FORMS(QV_BCE16);
#undef QV_BCE16
}

int launch_kd_ce_loss_rows16(const void* student, bool bf16, const float* teacher, const float* table, int64_t table_rows, const int64_t* index,
                             const int64_t* labels, const int32_t* mix, int64_t batch, int64_t classes, float kd_temp, float kd_alpha,
                             float label_smoothing, const float* grad_scale, float* partials, float* out3, void* dlogits, hipStream_t st) {
    const int B = (int)batch, C = (int)classes;
    (bf16 ? ce_rows16<__bf16, false> : ce_rows16<_Float16, false>)(student, teacher, table, nullptr, nullptr, nullptr, table_rows, 0, index, labels, mix, B,
                                                                  C, kd_temp, kd_alpha, label_smoothing, grad_scale, partials, dlogits, st);
    k_kd_bce_finish<<<1, 256, 0, st>>>(partials, B, kd_temp, kd_alpha, teacher || table ? 1 : 0, 1.0f / (float)B, out3);
    return 0;
}

int launch_kd_ce_loss_topk16(const void* student, bool bf16, const int16_t* idx, const float* val, const float* tail, int64_t table_rows, int k,
                             const int64_t* index, const int64_t* labels, const int32_t* mix, int64_t batch, int64_t classes, float kd_temp,
                             float kd_alpha, float label_smoothing, const float* grad_scale, float* partials, float* out3, void* dlogits,
                             hipStream_t st) {
    const int B = (int)batch, C = (int)classes;
    (bf16 ? ce_rows16<__bf16, true> : ce_rows16<_Float16, true>)(student, nullptr, nullptr, idx, val, tail, table_rows, k, index, labels, mix, B, C, kd_temp,
                                                                kd_alpha, label_smoothing, grad_scale, partials, dlogits, st);
    k_kd_bce_finish<<<1, 256, 0, st>>>(partials, B, kd_temp, kd_alpha, 1, 1.0f / (float)B, out3);
    return 0;
}

int launch_kd_bce_loss_topk16(const void* student, bool bf16, const int16_t* idx, const float* val, const float* tail, int64_t table_rows, int k,
                              const int64_t* index, const int64_t* labels, const int32_t* mix, int64_t batch, int64_t classes, float kd_temp,
                              float kd_alpha, float label_smoothing, float target_threshold, bool sum_classes, const float* grad_scale, float* partials,
                              float* out3, void* dlogits, hipStream_t st) {
    const int B = (int)batch, C = (int)classes;
    const float scale = sum_classes ? 1.0f / (float)B : 1.0f / ((float)B * (float)C);
    (bf16 ? bce_topk16<__bf16> : bce_topk16<_Float16>)(student, idx, val, tail, table_rows, k, index, labels, mix, B, C, kd_temp, kd_alpha, label_smoothing,
                                                      target_threshold, scale, grad_scale, partials, dlogits, st);
    k_kd_bce_finish<<<1, 256, 0, st>>>(partials, B, kd_temp, kd_alpha, idx ? 1 : 0, scale, out3);
    return 0;
}

}  // namespace qv
