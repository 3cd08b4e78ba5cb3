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
#include "qv_kernels.h"
#include "qv_optim.h"

namespace qv {

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

// The row of the tensor's group and the range as in k_adamw_groups (qv_optim.h: group_row, chunk_range); a tensor of no group has its partials written as
// zeros, its trust is not written.  The two kernels keep their float4 body and scalar tail written out instead of calling walk_range: a closure carries
// the stream pointers through memory at the point where the compiler decides that they are global addresses, and both kernels came out with flat
// loads and stores, other scalar-register counts and another schedule ([&] and [=] captures alike; profiles/optim_one_walker_identity.txt).
__global__ __launch_bounds__(kOptThreads) void k_lamb_moments(const LambArgs a) {
    bool in_group;
    const LambRow h = a.group[group_row(a.chunk_tensor, a.tensor_group, a.n_groups, in_group)];
    const ChunkRange r = chunk_range(a.numel, a.chunk_tensor, a.chunk_index, a.chunk, in_group);
    const float* p = a.params[r.t];
    const float* g = a.grads[r.t];
    float* m = a.exp_avg[r.t];
    float* v = a.exp_avg_sq[r.t];
    const float coef = a.coef ? a.coef[1] : 1.0f;
    const bool al = aligned16(p, g, m, v);
    const int64_t lo = r.lo, hi = r.hi;
    float sr = 0.f, sp = 0.f;
    int64_t tail = lo;
    if (al) {
        const int64_t hi4 = lo + ((hi - lo) & ~(int64_t)3);
        for (int64_t i = lo + 4 * threadIdx.x; i < hi4; i += 4 * kOptThreads) {
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
    for (int64_t i = tail + threadIdx.x; i < hi; i += kOptThreads) {
        const float P = p[i];
        float M = m[i], V = v[i];
        const float r = lamb_moments_one(P, g[i], M, V, h, coef);
        m[i] = M; v[i] = V;
        sr += r * r;
        sp += P * P;
    }
    __shared__ float sw[2][kOptThreads / 64];
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
__global__ __launch_bounds__(kOptThreads) void k_lamb_apply(const LambArgs a) {
    bool in_group;
    const LambRow h = a.group[group_row(a.chunk_tensor, a.tensor_group, a.n_groups, in_group)];
    const ChunkRange r = chunk_range(a.numel, a.chunk_tensor, a.chunk_index, a.chunk, in_group);
    // the tensor's two norms: lane l of every wave takes partials l, l + 64, ... of the tensor in double, then one butterfly - the same order in every
    // wave of every workgroup of the tensor, so they all apply the same trust
    const int64_t first = a.tensor_first_chunk[r.t];
    const int64_t nc = in_group ? (r.n + a.chunk - 1) / a.chunk : 0;
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
    if (a.trust_out && in_group && r.ck == 0 && threadIdx.x == 0) a.trust_out[r.t] = trust;
    const float step = h.lr * trust;

    float* p = a.params[r.t];
    const float* m = a.exp_avg[r.t];
    const float* v = a.exp_avg_sq[r.t];
    float* e = EMA ? a.ema[r.t] : nullptr;
    const float w = a.ema_w;
    const bool al = aligned16(p, m, v, e);
    const int64_t lo = r.lo, hi = r.hi;
    int64_t tail = lo;
    if (al) {
        const int64_t hi4 = lo + ((hi - lo) & ~(int64_t)3);
        for (int64_t i = lo + 4 * threadIdx.x; i < hi4; i += 4 * kOptThreads) {
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
    for (int64_t i = tail + threadIdx.x; i < hi; i += kOptThreads) {
        float P = p[i];
        P = P - step * lamb_r(P, m[i], v[i], h);
        p[i] = P;
        if (EMA) e[i] = lamb_ema_one(e[i], P, w);
    }
}

// the rows of `groups` as the kernels' prefactors, checked in ascending order: formed in double, narrowed once (as adam_prefactors forms AdamW's)
static bool lamb_rows(const char* fn, const qatvit_lamb_group* groups, int32_t n_groups, LambArgs& a) {
    for (int i = 0; i < n_groups; ++i) {
        const qatvit_lamb_group& g = groups[i];
        if (!hyper_ok(fn, i, g.step, g.lr, g.beta1, g.beta2, g.eps, g.weight_decay)) return false;
        const double bc1 = 1.0 - pow(g.beta1, (double)g.step), bc2 = 1.0 - pow(g.beta2, (double)g.step);
        a.group[i] = LambRow{(float)g.beta1, g.grad_averaging ? (float)(1.0 - g.beta1) : 1.0f, (float)g.beta2, (float)(1.0 - g.beta2),
                             (float)bc1, (float)sqrt(bc2), (float)g.eps, (float)g.weight_decay, (float)g.lr,
                             ((g.weight_decay != 0. || g.always_adapt) ? kLambAdapt : 0u) | (g.trust_clip ? kLambTrustClip : 0u)};
    }
    a.n_groups = n_groups;
    return true;
}

}  // namespace qv

using namespace qv;

extern "C" {

int qatvit_optim_lamb_moments(const void* param_ptrs, const void* grad_ptrs, const void* exp_avg_ptrs, const void* exp_avg_sq_ptrs, const int64_t* numel,
                              const int32_t* tensor_group, const int32_t* chunk_tensor, const int32_t* chunk_index, int32_t n_chunks, int64_t chunk_elems,
                              const qatvit_lamb_group* groups, int32_t n_groups, const float* clip_out2, float* partials2, void* stream) {
    const char* fn = "qatvit_optim_lamb_moments";
    if (!tables_ok(fn, param_ptrs && grad_ptrs && exp_avg_ptrs && exp_avg_sq_ptrs && numel && tensor_group && chunk_tensor && chunk_index && groups &&
                           partials2,
                   n_chunks, chunk_elems) ||
        !n_groups_ok(fn, n_groups))
        return 1;
    LambArgs a{};
    a.params = ptr_table<float>(param_ptrs);
    a.grads = ptr_table<const float>(grad_ptrs);
    a.exp_avg = ptr_table<float>(exp_avg_ptrs);
    a.exp_avg_sq = ptr_table<float>(exp_avg_sq_ptrs);
    a.numel = numel;
    a.tensor_group = tensor_group;
    a.chunk_tensor = chunk_tensor;
    a.chunk_index = chunk_index;
    a.chunk = chunk_elems;
    a.coef = clip_out2;
    a.partials = partials2;
    if (!lamb_rows(fn, groups, n_groups, a)) return 1;
    k_lamb_moments<<<n_chunks, kOptThreads, 0, reinterpret_cast<hipStream_t>(stream)>>>(a);
    QV_CHECK_LAUNCH("k_lamb_moments");
    return 0;
}

int qatvit_optim_lamb_apply(const void* param_ptrs, const void* exp_avg_ptrs, const void* exp_avg_sq_ptrs, const void* ema_ptrs, const int64_t* numel,
                            const int32_t* tensor_group, const int32_t* tensor_first_chunk, const int32_t* chunk_tensor, const int32_t* chunk_index,
                            int32_t n_chunks, int64_t chunk_elems, const qatvit_lamb_group* groups, int32_t n_groups, double ema_decay,
                            const float* partials2, float* trust_out, void* stream) {
    const char* fn = "qatvit_optim_lamb_apply";
    if (!tables_ok(fn, param_ptrs && exp_avg_ptrs && exp_avg_sq_ptrs && numel && tensor_group && tensor_first_chunk && chunk_tensor && chunk_index &&
                           groups && partials2,
                   n_chunks, chunk_elems) ||
        !n_groups_ok(fn, n_groups))
        return 1;
    LambArgs a{};
    a.params = ptr_table<float>(param_ptrs);
    a.exp_avg = ptr_table<float>(exp_avg_ptrs);
    a.exp_avg_sq = ptr_table<float>(exp_avg_sq_ptrs);
    a.ema = ptr_table<float>(ema_ptrs);
    a.numel = numel;
    a.tensor_group = tensor_group;
    a.tensor_first_chunk = tensor_first_chunk;
    a.chunk_tensor = chunk_tensor;
    a.chunk_index = chunk_index;
    a.chunk = chunk_elems;
    a.partials = const_cast<float*>(partials2);
    a.trust_out = trust_out;
    if (!lamb_rows(fn, groups, n_groups, a)) return 1;
    if (ema_ptrs) {   // the decay is looked at only with averages
        if (!ema_decay_ok(fn, ema_decay)) return 1;
        a.ema_w = (float)(1.0 - ema_decay);
        k_lamb_apply<true><<<n_chunks, kOptThreads, 0, reinterpret_cast<hipStream_t>(stream)>>>(a);
    } else {
        k_lamb_apply<false><<<n_chunks, kOptThreads, 0, reinterpret_cast<hipStream_t>(stream)>>>(a);
    }
    QV_CHECK_LAUNCH("k_lamb_apply");
    return 0;
}

}  // extern "C"
