// LAMB (layer-wise adaptive moments, You et al. 2020) with per-tensor trust ratios as two multi-tensor launches behind the global-norm launch pair of
// optim.hip (qatvit_optim_grad_norm, unchanged: its out2 is the `coef` below).  The arithmetic is the one include/qatvit.h states - timm's Lamb with
// that class's defaults - per tensor, with the row of the tensor's param group:
//     g <- g * coef ; m <- b1 * m + w1 * g ; v <- b2 * v + (1 - b2) * g * g            (w1 = 1 - b1, or 1 without grad_averaging)
//     r  = (m / (1 - b1^t)) / (sqrt(v) / sqrt(1 - b2^t) + eps) + wd * p
//     trust = ||p||_2 / ||r||_2 where the group adapts and both norms are > 0, else 1 ; p <- p - (lr * trust) * r
// every fp32 operation rounded on its own (-ffp-contract=off), in the order written.
// The two norms of a tensor stand between forming r and applying it, so the step is a multi-tensor reduction with a dependent second phase:
//   k_lamb_moments  one workgroup per (tensor, chunk) of optim.hip's chunk table: reads p, g, m, v, writes m, v, forms r in registers and writes the
//                   workgroup's {sum r^2, sum p^2} to partials[chunk][2] (k_grad_sqnorm's reduction order).  p is not written.  16 B + 8 B per parameter.
//   k_lamb_apply    the same table: every workgroup adds up ITS TENSOR's partials (contiguous in the table from tensor_first_chunk[t]) in double, in one
//                   fixed order, each wave for itself - so all workgroups of a tensor hold the same trust without a barrier or a third launch - then
//                   forms r again from the new m, v and the untouched p (lamb_r, the expression of launch 1: the same bits) and writes p, and the
//                   weight average from the register that holds the new p where ema_ptrs is given.  12 B + 4 B per parameter (+ 8 B with the average).
// No atomics, nothing kept per parameter beyond m and v: 40 B of traffic per parameter against AdamW's 28.  (r as a fourth stream would move the same
// 40 B and cost 4 B per parameter of state; it would save launch 2's divisions and square root, which a kernel bound by HBM does not wait for.)
#include "../../include/qatvit.h"
#include "qv_common.h"
#include "qv_kernels.h"

namespace qv {

constexpr int kLambThreads = 256;
constexpr uint32_t kLambAdapt = 1, kLambTrustClip = 2;

struct LambRow {
    float b1, w1, b2, w2;   // beta1, 1 - beta1 (1 without grad_averaging), beta2, 1 - beta2
    float bc1, bc2_sqrt;    // 1 - beta1^t, sqrt(1 - beta2^t)
    float eps, wd, lr;
    uint32_t flags;         // kLambAdapt: weight_decay != 0 or always_adapt; kLambTrustClip
};

struct LambArgs {
    float* const* params;
    const float* const* grads;   // launch 1 only
    float* const* exp_avg;
    float* const* exp_avg_sq;
    float* const* ema;           // launch 2 only, null: no average
    const int64_t* numel;
    const int32_t* tensor_group;
    const int32_t* tensor_first_chunk;   // launch 2 only
    const int32_t* chunk_tensor;
    const int32_t* chunk_index;
    int64_t chunk;
    const float* coef;           // launch 1 only: null or optim.hip's out2
    float* partials;             // [n_chunks][2] = {sum r^2, sum p^2}
    float* trust_out;            // launch 2 only, null or [n_tensors]
    float ema_w;                 // 1 - ema_decay
    int32_t n_groups;
    LambRow group[QATVIT_OPTIM_MAX_GROUPS];
};
static_assert(sizeof(LambArgs) <= 4096, "the rows travel in the kernel-argument block");

// the one expression of r: launch 2 repeats what launch 1 summed
__device__ inline float lamb_r(float p, float m, float v, const LambRow& h) {
    return (m / h.bc1) / (sqrtf(v) / h.bc2_sqrt + h.eps) + h.wd * p;
}

__device__ inline float lamb_moments_one(float p, float g, float& m, float& v, const LambRow& h, float coef) {
    g *= coef;
    m = h.b1 * m + h.w1 * g;
    v = h.b2 * v + h.w2 * g * g;
    return lamb_r(p, m, v, h);
}

// The weight average: optim.hip's ema_one - ATen's lerp(e, p, w), both branches - with each branch's multiply-add as ONE fused operation.  That is
// how stock torch.lerp rounds, on this GPU and on the CPU alike (its kernels are built with contraction on: of 200,000 normal samples at w = 0.1
// 22,503 differ from the two-rounding form and none from this one), and state[p]["ema"] is specified as torch.equal to torch.lerp applied after the
// step.  The library is built with -ffp-contract=off, so the fusion is written out; d and 1 - w are rounded on their own, as there.  Against
// ema_one's two roundings the result differs by at most one rounding of the product; w = 1 gives p exactly in both.
__device__ inline float lamb_ema_one(float e, float p, float w) {
    const float d = p - e;
    return w < 0.5f ? fmaf(w, d, e) : fmaf(-d, 1.0f - w, p);
}

// chunk -> tensor -> group -> row as in k_adamw_groups: the row is read into scalars once, and a tensor of no group gets an empty range (its partials
// are written as zeros, its trust is not written)
__global__ __launch_bounds__(kLambThreads) void k_lamb_moments(const LambArgs a) {
    const int t = a.chunk_tensor[blockIdx.x];
    const int gi = __builtin_amdgcn_readfirstlane(a.tensor_group[t]);
    const bool in_group = (unsigned)gi < (unsigned)a.n_groups;
    const LambRow h = a.group[in_group ? gi : 0];
    const int64_t lo = (int64_t)a.chunk_index[blockIdx.x] * a.chunk;
    const int64_t n = a.numel[t];
    const int64_t hi = !in_group ? lo : lo + a.chunk < n ? lo + a.chunk : n;
    const float* p = a.params[t];
    const float* g = a.grads[t];
    float* m = a.exp_avg[t];
    float* v = a.exp_avg_sq[t];
    const float coef = a.coef ? a.coef[1] : 1.0f;
    const bool al = ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(m) | reinterpret_cast<uintptr_t>(v)) & 15) == 0;
    float sr = 0.f, sp = 0.f;
    int64_t tail = lo;
    if (al) {
        const int64_t hi4 = lo + ((hi - lo) & ~(int64_t)3);
        for (int64_t i = lo + 4 * threadIdx.x; i < hi4; i += 4 * kLambThreads) {
            const float4 P = *reinterpret_cast<const float4*>(p + i), G = *reinterpret_cast<const float4*>(g + i);
            float4 M = *reinterpret_cast<float4*>(m + i), V = *reinterpret_cast<float4*>(v + i);
            const float rx = lamb_moments_one(P.x, G.x, M.x, V.x, h, coef);
            const float ry = lamb_moments_one(P.y, G.y, M.y, V.y, h, coef);
            const float rz = lamb_moments_one(P.z, G.z, M.z, V.z, h, coef);
            const float rw = lamb_moments_one(P.w, G.w, M.w, V.w, h, coef);
            *reinterpret_cast<float4*>(m + i) = M;
            *reinterpret_cast<float4*>(v + i) = V;
            sr += rx * rx + ry * ry + rz * rz + rw * rw;
            sp += P.x * P.x + P.y * P.y + P.z * P.z + P.w * P.w;
        }
        tail = hi4;
    }
    for (int64_t i = tail + threadIdx.x; i < hi; i += kLambThreads) {
        const float P = p[i];
        float M = m[i], V = v[i];
        const float r = lamb_moments_one(P, g[i], M, V, h, coef);
        m[i] = M; v[i] = V;
        sr += r * r;
        sp += P * P;
    }
    __shared__ float sw[2][kLambThreads / 64];
    sr = wave_sum(sr);
    sp = wave_sum(sp);
    if ((threadIdx.x & 63) == 0) { sw[0][threadIdx.x >> 6] = sr; sw[1][threadIdx.x >> 6] = sp; }
    __syncthreads();
    if (threadIdx.x == 0) {
        a.partials[2 * (int64_t)blockIdx.x] = (sw[0][0] + sw[0][1]) + (sw[0][2] + sw[0][3]);
        a.partials[2 * (int64_t)blockIdx.x + 1] = (sw[1][0] + sw[1][1]) + (sw[1][2] + sw[1][3]);
    }
}

__device__ inline double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);   // a + b == b + a: all 64 lanes end with the same bits
    return v;
}

template <bool EMA>
__global__ __launch_bounds__(kLambThreads) void k_lamb_apply(const LambArgs a) {
    const int t = a.chunk_tensor[blockIdx.x];
    const int gi = __builtin_amdgcn_readfirstlane(a.tensor_group[t]);
    const bool in_group = (unsigned)gi < (unsigned)a.n_groups;
    const LambRow h = a.group[in_group ? gi : 0];
    const int ck = a.chunk_index[blockIdx.x];
    const int64_t lo = (int64_t)ck * a.chunk;
    const int64_t n = a.numel[t];
    const int64_t hi = !in_group ? lo : lo + a.chunk < n ? lo + a.chunk : n;
    // the tensor's two norms: lane l of every wave takes partials l, l + 64, ... of the tensor in double, then one butterfly - the same order in every
    // wave of every workgroup of the tensor, so they all apply the same trust
    const int64_t first = a.tensor_first_chunk[t];
    const int64_t nc = in_group ? (n + a.chunk - 1) / a.chunk : 0;
    double sr = 0.0, sp = 0.0;
    for (int64_t c = threadIdx.x & 63; c < nc; c += 64) {
        sr += (double)a.partials[2 * (first + c)];
        sp += (double)a.partials[2 * (first + c) + 1];
    }
    sr = wave_sum_f64(sr);
    sp = wave_sum_f64(sp);
    const float rn = (float)sqrt(sr), pn = (float)sqrt(sp);
    float trust = 1.0f;
    if ((h.flags & kLambAdapt) && pn > 0.f && rn > 0.f) {
        trust = pn / rn;
        if (h.flags & kLambTrustClip) trust = fminf(trust, 1.0f);
    }
    trust = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, trust)));
    if (a.trust_out && in_group && ck == 0 && threadIdx.x == 0) a.trust_out[t] = trust;
    const float step = h.lr * trust;

    float* p = a.params[t];
    const float* m = a.exp_avg[t];
    const float* v = a.exp_avg_sq[t];
    float* e = EMA ? a.ema[t] : nullptr;
    const float w = a.ema_w;
    const bool al = ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(m) | reinterpret_cast<uintptr_t>(v) | reinterpret_cast<uintptr_t>(e)) & 15) == 0;
    int64_t tail = lo;
    if (al) {
        const int64_t hi4 = lo + ((hi - lo) & ~(int64_t)3);
        for (int64_t i = lo + 4 * threadIdx.x; i < hi4; i += 4 * kLambThreads) {
            float4 P = *reinterpret_cast<float4*>(p + i);
            const float4 M = *reinterpret_cast<const float4*>(m + i), V = *reinterpret_cast<const float4*>(v + i);
            P.x = P.x - step * lamb_r(P.x, M.x, V.x, h);
            P.y = P.y - step * lamb_r(P.y, M.y, V.y, h);
            P.z = P.z - step * lamb_r(P.z, M.z, V.z, h);
            P.w = P.w - step * lamb_r(P.w, M.w, V.w, h);
            *reinterpret_cast<float4*>(p + i) = P;
            if (EMA) {
                float4 E = *reinterpret_cast<float4*>(e + i);
                E.x = lamb_ema_one(E.x, P.x, w);
                E.y = lamb_ema_one(E.y, P.y, w);
                E.z = lamb_ema_one(E.z, P.z, w);
                E.w = lamb_ema_one(E.w, P.w, w);
                *reinterpret_cast<float4*>(e + i) = E;
            }
        }
        tail = hi4;
    }
    for (int64_t i = tail + threadIdx.x; i < hi; i += kLambThreads) {
        float P = p[i];
        P = P - step * lamb_r(P, m[i], v[i], h);
        p[i] = P;
        if (EMA) e[i] = lamb_ema_one(e[i], P, w);
    }
}

// the rows of `groups` as the kernels' prefactors: formed in double, narrowed once (as qatvit_optim_adamw_groups forms its own)
static int lamb_rows(const char* fn, const qatvit_lamb_group* groups, int32_t n_groups, LambArgs& a) {
    for (int i = 0; i < n_groups; ++i) {
        const qatvit_lamb_group& g = groups[i];
        if (!(g.step >= 1 && g.lr >= 0. && g.beta1 >= 0. && g.beta1 < 1. && g.beta2 >= 0. && g.beta2 < 1. && g.eps >= 0. && g.weight_decay >= 0.)) {
            set_error("%s: bad hyper-parameters in group %d (step=%lld lr=%g betas=(%g, %g) eps=%g weight_decay=%g)", fn, i, (long long)g.step, g.lr,
                      g.beta1, g.beta2, g.eps, g.weight_decay);
            return 1;
        }
        const double bc1 = 1.0 - pow(g.beta1, (double)g.step), bc2 = 1.0 - pow(g.beta2, (double)g.step);
        a.group[i] = LambRow{(float)g.beta1, g.grad_averaging ? (float)(1.0 - g.beta1) : 1.0f, (float)g.beta2, (float)(1.0 - g.beta2),
                             (float)bc1, (float)sqrt(bc2), (float)g.eps, (float)g.weight_decay, (float)g.lr,
                             ((g.weight_decay != 0. || g.always_adapt) ? kLambAdapt : 0u) | (g.trust_clip ? kLambTrustClip : 0u)};
    }
    a.n_groups = n_groups;
    return 0;
}

}  // namespace qv

using namespace qv;

extern "C" {

int qatvit_optim_lamb_moments(const void* param_ptrs, const void* grad_ptrs, const void* exp_avg_ptrs, const void* exp_avg_sq_ptrs, const int64_t* numel,
                              const int32_t* tensor_group, const int32_t* chunk_tensor, const int32_t* chunk_index, int32_t n_chunks, int64_t chunk_elems,
                              const qatvit_lamb_group* groups, int32_t n_groups, const float* clip_out2, float* partials2, void* stream) {
    QV_CHECK_ARG(param_ptrs && grad_ptrs && exp_avg_ptrs && exp_avg_sq_ptrs && numel && tensor_group && chunk_tensor && chunk_index && groups && partials2,
                 "qatvit_optim_lamb_moments: null pointer");
    QV_CHECK_ARG(n_chunks > 0 && chunk_elems > 0 && chunk_elems % 4 == 0, "qatvit_optim_lamb_moments: bad chunking (n_chunks=%d chunk=%lld)", n_chunks,
                 (long long)chunk_elems);
    QV_CHECK_ARG(n_groups >= 1 && n_groups <= QATVIT_OPTIM_MAX_GROUPS, "qatvit_optim_lamb_moments: n_groups %d outside [1, %d]", n_groups,
                 QATVIT_OPTIM_MAX_GROUPS);
    LambArgs a{};
    a.params = reinterpret_cast<float* const*>(param_ptrs);
    a.grads = reinterpret_cast<const float* const*>(grad_ptrs);
    a.exp_avg = reinterpret_cast<float* const*>(exp_avg_ptrs);
    a.exp_avg_sq = reinterpret_cast<float* const*>(exp_avg_sq_ptrs);
    a.numel = numel;
    a.tensor_group = tensor_group;
    a.chunk_tensor = chunk_tensor;
    a.chunk_index = chunk_index;
    a.chunk = chunk_elems;
    a.coef = clip_out2;
    a.partials = partials2;
    if (lamb_rows("qatvit_optim_lamb_moments", groups, n_groups, a)) return 1;
    k_lamb_moments<<<n_chunks, kLambThreads, 0, reinterpret_cast<hipStream_t>(stream)>>>(a);
    QV_CHECK_LAUNCH("k_lamb_moments");
    return 0;
}

int qatvit_optim_lamb_apply(const void* param_ptrs, const void* exp_avg_ptrs, const void* exp_avg_sq_ptrs, const void* ema_ptrs, const int64_t* numel,
                            const int32_t* tensor_group, const int32_t* tensor_first_chunk, const int32_t* chunk_tensor, const int32_t* chunk_index,
                            int32_t n_chunks, int64_t chunk_elems, const qatvit_lamb_group* groups, int32_t n_groups, double ema_decay,
                            const float* partials2, float* trust_out, void* stream) {
    QV_CHECK_ARG(param_ptrs && exp_avg_ptrs && exp_avg_sq_ptrs && numel && tensor_group && tensor_first_chunk && chunk_tensor && chunk_index && groups &&
                     partials2,
                 "qatvit_optim_lamb_apply: null pointer");
    QV_CHECK_ARG(n_chunks > 0 && chunk_elems > 0 && chunk_elems % 4 == 0, "qatvit_optim_lamb_apply: bad chunking (n_chunks=%d chunk=%lld)", n_chunks,
                 (long long)chunk_elems);
    QV_CHECK_ARG(n_groups >= 1 && n_groups <= QATVIT_OPTIM_MAX_GROUPS, "qatvit_optim_lamb_apply: n_groups %d outside [1, %d]", n_groups,
                 QATVIT_OPTIM_MAX_GROUPS);
    LambArgs a{};
    a.params = reinterpret_cast<float* const*>(param_ptrs);
    a.exp_avg = reinterpret_cast<float* const*>(exp_avg_ptrs);
    a.exp_avg_sq = reinterpret_cast<float* const*>(exp_avg_sq_ptrs);
    a.ema = reinterpret_cast<float* const*>(ema_ptrs);
    a.numel = numel;
    a.tensor_group = tensor_group;
    a.tensor_first_chunk = tensor_first_chunk;
    a.chunk_tensor = chunk_tensor;
    a.chunk_index = chunk_index;
    a.chunk = chunk_elems;
    a.partials = const_cast<float*>(partials2);
    a.trust_out = trust_out;
    if (lamb_rows("qatvit_optim_lamb_apply", groups, n_groups, a)) return 1;
    if (ema_ptrs) {
        QV_CHECK_ARG(ema_decay >= 0. && ema_decay < 1., "qatvit_optim_lamb_apply: ema_decay %g outside [0, 1)", ema_decay);   // NaN fails both comparisons
        a.ema_w = (float)(1.0 - ema_decay);
        k_lamb_apply<true><<<n_chunks, kLambThreads, 0, reinterpret_cast<hipStream_t>(stream)>>>(a);
    } else {
        k_lamb_apply<false><<<n_chunks, kLambThreads, 0, reinterpret_cast<hipStream_t>(stream)>>>(a);
    }
    QV_CHECK_LAUNCH("k_lamb_apply");
    return 0;
}

}  // extern "C"
