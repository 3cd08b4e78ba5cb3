// What the multi-tensor optimizer kernels (optim.hip: clip + AdamW, weight EMA, swap; lamb.hip: LAMB) and their entries share.
// Device side: one workgroup per row of the host's (tensor, chunk) table - chunk_range says which elements, group_row fetches the tensor's
// param-group row, walk_range runs a float4 body with a scalar tail over them, adamw_range is the AdamW update (with the weight average as an
// optional fifth stream) written that way.  Host side: the argument checks of the nine entries with their texts, and the AdamW prefactors.
// The kernels' names, parameter lists and argument structs are theirs; tools/isa_digest.py holds their machine code to what it was
// (profiles/optim_one_walker_identity.txt).
#pragma once
#include <math.h>

#include "../../include/qatvit.h"
#include "qv_common.h"

namespace qv {

constexpr int kOptThreads = 256;   // workgroup of every kernel here: four waves

// ---------------------------------------------------------------------------------------------------------------- device
// chunk -> tensor -> group -> row: the index of the tensor's row in the kernel's table of group rows, uniform, so that `rows[group_row(...)]` is
// read into scalars, once.  in_group = false (and row 0): a tensor of no group (the host cannot see that table).  It gets an empty range
// (chunk_range) instead of an early exit, so that the row - the last link of the chain - is fetched while the first vector loads are in flight
// rather than in front of them.  (The index and not the row: a pointer to the by-value kernel arguments handed to a function costs the kernels
// of lamb.hip the global address space of their streams.)
__device__ inline int group_row(const int32_t* chunk_tensor, const int32_t* tensor_group, int32_t n_groups, bool& in_group) {
    const int gi = __builtin_amdgcn_readfirstlane(tensor_group[chunk_tensor[blockIdx.x]]);
    in_group = (unsigned)gi < (unsigned)n_groups;
    return in_group ? gi : 0;
}

// the workgroup's row of the host's (tensor, chunk) table: tensor t, its chunk ck = elements [lo, hi) of its n.  chunk_range(..., live = false)
// (a tensor of no group): hi = lo, both loops of walk_range are empty
struct ChunkRange {
    int t, ck;
    int64_t lo, hi, n;
};

__device__ inline ChunkRange chunk_range(const int64_t* numel, const int32_t* chunk_tensor, const int32_t* chunk_index, int64_t chunk, bool live = true) {
    const int t = chunk_tensor[blockIdx.x];
    const int ck = chunk_index[blockIdx.x];
    const int64_t lo = (int64_t)ck * chunk;
    const int64_t n = numel[t];
    return ChunkRange{t, ck, lo, !live ? lo : lo + chunk < n ? lo + chunk : n, n};
}

// every stream of a float4 body on a 16-byte boundary (a null pointer - an absent stream - passes)
template <class... T>
__device__ inline bool aligned16(const T*... p) {
    return ((... | reinterpret_cast<uintptr_t>(p)) & 15) == 0;
}

// f4(i) on four elements at i where the streams allow it, f1(i) on the rest, element by element; a workgroup's threads interleave
template <class F4, class F1>
__device__ inline void walk_range(bool al, const ChunkRange& r, F4 f4, F1 f1) {
    int64_t tail = r.lo;
    if (al) {
        const int64_t hi4 = r.lo + ((r.hi - r.lo) & ~(int64_t)3);
        for (int64_t i = r.lo + 4 * threadIdx.x; i < hi4; i += 4 * kOptThreads) f4(i);
        tail = hi4;
    }
    for (int64_t i = tail + threadIdx.x; i < r.hi; i += kOptThreads) f1(i);
}

// The weight average e <- lerp(e, p, w), w = (float)(1.0 - ema_decay), in its two roundings.  Both are specified behaviour:
// ema_one (ClipAdamW; k_adamw_ema, k_adamw_groups_ema, k_ema): ATen's lerp(e, p, w) in both of its branches with every operation rounded to fp32
// and unfused (-ffp-contract=off), so ema_decay = 0 gives e' = p' exactly.
__device__ inline float ema_one(float e, float p, float w) {
    const float d = p - e;
    return w < 0.5f ? e + w * d : p - d * (1.0f - w);
}
// lamb_ema_one (ClipLamb; k_lamb_apply<true>): the same with each branch's multiply-add as ONE fused operation.  That is how stock torch.lerp
// rounds, on this GPU and on the CPU alike (its kernels are built with contraction on: of 200,000 normal samples at w = 0.1 22,503 differ from the
// two-rounding form and none from this one), and state[p]["ema"] is specified as torch.equal to torch.lerp applied after the step.  The library is
// built with -ffp-contract=off, so the fusion is written out; d and 1 - w are rounded on their own, as there.  Against ema_one's two roundings the
// result differs by at most one rounding of the product; w = 1 gives p exactly in both.
__device__ inline float lamb_ema_one(float e, float p, float w) {
    const float d = p - e;
    return w < 0.5f ? fmaf(w, d, e) : fmaf(-d, 1.0f - w, p);
}

// ---- AdamW
struct AdamGroup {
    float decay;       // 1 - lr * weight_decay
    float w1;          // 1 - beta1
    float beta2, w2;   // beta2, 1 - beta2
    float step_size;   // lr / (1 - beta1^t)
    float bc2_sqrt;    // sqrt(1 - beta2^t)
    float eps;
};

struct AdamArgs {
    float* const* params;
    const float* const* grads;
    float* const* exp_avg;
    float* const* exp_avg_sq;
    const int64_t* numel;
    const int32_t* chunk_tensor;
    const int32_t* chunk_index;
    int64_t chunk;
    float decay, w1, beta2, w2, step_size, bc2_sqrt, eps;   // an AdamGroup, spelt out: the layout is the kernels' argument block
    const float* coef;   // optional device scalar multiplied into every gradient (the clip coefficient)
};

__host__ __device__ inline AdamArgs adam_args(float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                                              const int64_t* numel, const int32_t* chunk_tensor, const int32_t* chunk_index, int64_t chunk,
                                              const AdamGroup& h, const float* coef) {
    return AdamArgs{params, grads, exp_avg, exp_avg_sq, numel, chunk_tensor, chunk_index, chunk,
                    h.decay, h.w1, h.beta2, h.w2, h.step_size, h.bc2_sqrt, h.eps, coef};
}

__device__ inline void adam_one(float& p, float g, float& m, float& v, const AdamArgs& a, float coef) {
    g *= coef;
    p *= a.decay;
    m = m + a.w1 * (g - m);
    v = v * a.beta2 + a.w2 * g * g;   // addcmul_: value * t1 * t2, left to right
    const float denom = sqrtf(v) / a.bc2_sqrt + a.eps;
    p = p - a.step_size * (m / denom);
}

// The update of tensor r.t's elements [r.lo, r.hi): the same adam_one on the same operands in the same order whichever kernel calls it, so p, m, v
// come out with the same bits from all four.  EMA: the weight average e as a fifth stream, written from the register that holds the new p.
template <bool EMA>
__device__ inline void adamw_range(const AdamArgs& a, const ChunkRange& r, float* __restrict__ e, float w) {
    float* p = a.params[r.t];
    const float* g = a.grads[r.t];
    float* m = a.exp_avg[r.t];
    float* v = a.exp_avg_sq[r.t];
    const float coef = a.coef ? a.coef[1] : 1.0f;
    walk_range(
        aligned16(p, g, m, v, e), r,
        [&](int64_t i) {
            float4 P = *reinterpret_cast<float4*>(p + i), M = *reinterpret_cast<float4*>(m + i), V = *reinterpret_cast<float4*>(v + i);
            const float4 G = *reinterpret_cast<const float4*>(g + i);
            float4 E = EMA ? *reinterpret_cast<float4*>(e + i) : float4{};
            adam_one(P.x, G.x, M.x, V.x, a, coef);
            adam_one(P.y, G.y, M.y, V.y, a, coef);
            adam_one(P.z, G.z, M.z, V.z, a, coef);
            adam_one(P.w, G.w, M.w, V.w, a, coef);
            if (EMA) {
                E.x = ema_one(E.x, P.x, w);
                E.y = ema_one(E.y, P.y, w);
                E.z = ema_one(E.z, P.z, w);
                E.w = ema_one(E.w, P.w, w);
            }
            *reinterpret_cast<float4*>(p + i) = P;
            *reinterpret_cast<float4*>(m + i) = M;
            *reinterpret_cast<float4*>(v + i) = V;
            if (EMA) *reinterpret_cast<float4*>(e + i) = E;
        },
        [&](int64_t i) {
            float P = p[i], M = m[i], V = v[i];
            adam_one(P, g[i], M, V, a, coef);
            p[i] = P; m[i] = M; v[i] = V;
            if (EMA) e[i] = ema_one(e[i], P, w);
        });
}

// ---------------------------------------------------------------------------------------------------------------- host
// The argument checks of the entries: each sets the entry's message and returns false; the entry returns 1 before any HIP call.  Their order in
// an entry is: pointers, chunking, n_groups, the rows in ascending order, the decay.

// an operand that is a device table of tensor addresses
template <class T>
inline T* const* ptr_table(const void* p) {
    return reinterpret_cast<T* const*>(p);
}

inline bool tables_ok(const char* fn, bool all_pointers, int32_t n_chunks, int64_t chunk_elems) {
    if (!all_pointers) {
        set_error("%s: null pointer", fn);
        return false;
    }
    if (!(n_chunks > 0 && chunk_elems > 0 && chunk_elems % 4 == 0)) {
        set_error("%s: bad chunking (n_chunks=%d chunk=%lld)", fn, n_chunks, (long long)chunk_elems);
        return false;
    }
    return true;
}

inline bool n_groups_ok(const char* fn, int32_t n_groups) {
    if (n_groups >= 1 && n_groups <= QATVIT_OPTIM_MAX_GROUPS) return true;
    set_error("%s: n_groups %d outside [1, %d]", fn, n_groups, QATVIT_OPTIM_MAX_GROUPS);
    return false;
}

// One row of hyper-parameters (NaN fails every comparison).  group < 0: the one-group AdamW entries, which neither check nor print weight_decay
// (torch.optim.AdamW's own check is the caller's there); that asymmetry is kept as it is.
inline bool hyper_ok(const char* fn, int group, int64_t step, double lr, double beta1, double beta2, double eps, double weight_decay) {
    const bool ok = step >= 1 && lr >= 0. && beta1 >= 0. && beta1 < 1. && beta2 >= 0. && beta2 < 1. && eps >= 0.;
    if (group < 0) {
        if (ok) return true;
        set_error("%s: bad hyper-parameters (step=%lld lr=%g betas=(%g, %g) eps=%g)", fn, (long long)step, lr, beta1, beta2, eps);
        return false;
    }
    if (ok && weight_decay >= 0.) return true;
    set_error("%s: bad hyper-parameters in group %d (step=%lld lr=%g betas=(%g, %g) eps=%g weight_decay=%g)", fn, group, (long long)step, lr, beta1,
              beta2, eps, weight_decay);
    return false;
}

inline bool ema_decay_ok(const char* fn, double ema_decay) {
    if (ema_decay >= 0. && ema_decay < 1.) return true;   // NaN fails both comparisons
    set_error("%s: ema_decay %g outside [0, 1)", fn, ema_decay);
    return false;
}

// The scalar prefactors exactly as torch/optim/adamw.py forms them: python floats = doubles, narrowed once.  (Hyper-parameters arrive as doubles
// for that reason: 1 - float(0.999) is 1.3e-5 away from float(1 - 0.999).)
inline AdamGroup adam_prefactors(double lr, double beta1, double beta2, double eps, double weight_decay, int64_t step) {
    const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
    return AdamGroup{(float)(1.0 - lr * weight_decay), (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2),
                     (float)(lr / bc1), (float)sqrt(bc2), (float)eps};
}

}  // namespace qv
