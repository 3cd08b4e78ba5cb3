// Gradient clipping by global L2 norm + AdamW (decoupled weight decay) as two multi-tensor launches.
// Restates the step that follows the hot path in the reference's loop, /root/reference/src/training/qat_trainer.py:360-361:
//     torch.nn.utils.clip_grad_norm_(ddp_model.parameters(), 1.0); optimizer.step()
// with the optimizer of :271-276 (torch.optim.AdamW, betas (0.9, 0.999), eps 1e-8, amsgrad off).
// Arithmetic follows torch/optim/adamw.py (_single_tensor_adamw) and torch/nn/utils/clip_grad.py:
//     total = || (||g_i||_2)_i ||_2 ; coef = min(1, max_norm / (total + 1e-6)) ; g <- g * coef      (g is NOT written back here)
//     p <- p * (1 - lr*wd) ; m <- m + (1-b1) * (g - m) ; v <- v*b2 + (1-b2) * g*g
//     p <- p - (lr / (1-b1^t)) * m / (sqrt(v) / sqrt(1-b2^t) + eps)
// HBM-bound: 28 B per parameter for the update (p, g, m, v read; p, m, v written), 4 B for the norm.
// Tensors are separate allocations (the parameters belong to torch), so work is dealt in fixed-size chunks through a
// (tensor, chunk) table the host builds once; no atomics: chunk partials are reduced in a fixed order (deterministic).
//
// Weight EMA (k_adamw_ema, k_adamw_groups_ema, k_ema) and the in-place exchange (k_swap): an exponential moving average e of every parameter,
// written by the update launch from the register that holds the new parameter p' - one more read-modify-write stream, 36 B per parameter, no
// extra launch and no second read of p.  With w = (float)(1.0 - ema_decay) (double on the host, narrowed once):
//     d = p' - e ;  e' = (w < 0.5f) ? e + w * d : p' - d * (1.0f - w)
// every operation rounded to fp32 and unfused (-ffp-contract=off): ATen's lerp(e, p', w) in both of its branches, so ema_decay = 0 gives e' = p'
// exactly.  k_ema is the same average as a launch of its own (12 B per element) for tensors that take no update in a step; k_swap exchanges the
// contents of two tensor lists bit for bit (16 B per element), which is how the averaged weights are evaluated without new addresses.
// k_adamw / k_adamw_groups and their entries are not shared with the EMA kernels: their machine code is what it was.
#include "../../include/qatvit.h"
#include "qv_common.h"
#include "qv_kernels.h"

namespace qv {

constexpr int kOptThreads = 256;

__global__ __launch_bounds__(kOptThreads) void k_grad_sqnorm(const float* const* __restrict__ grads, const int64_t* __restrict__ numel,
                                                             const int32_t* __restrict__ chunk_tensor, const int32_t* __restrict__ chunk_index,
                                                             int64_t chunk, float* __restrict__ partials) {
    const int t = chunk_tensor[blockIdx.x];
    const int64_t lo = (int64_t)chunk_index[blockIdx.x] * chunk;
    const int64_t n = numel[t];
    const int64_t hi = lo + chunk < n ? lo + chunk : n;
    const float* g = grads[t];
    float s = 0.f;
    if ((reinterpret_cast<uintptr_t>(g) & 15) == 0) {
        const int64_t hi4 = lo + ((hi - lo) & ~(int64_t)3);
        for (int64_t i = lo + 4 * threadIdx.x; i < hi4; i += 4 * kOptThreads) {
            const float4 v = *reinterpret_cast<const float4*>(g + i);
            s += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
        }
        for (int64_t i = hi4 + threadIdx.x; i < hi; i += kOptThreads) s += g[i] * g[i];
    } else {
        for (int64_t i = lo + threadIdx.x; i < hi; i += kOptThreads) s += g[i] * g[i];
    }
    __shared__ float sw[kOptThreads / 64];
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) sw[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) partials[blockIdx.x] = (sw[0] + sw[1]) + (sw[2] + sw[3]);
}

// one block: total norm from the chunk partials (fixed summation order), clip coefficient; out2 = {total_norm, coef}
__global__ __launch_bounds__(kOptThreads) void k_clip_coef(const float* __restrict__ partials, int n, float max_norm, float* __restrict__ out2) {
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += kOptThreads) s += (double)partials[i];
    __shared__ double sd[kOptThreads];
    sd[threadIdx.x] = s;
    __syncthreads();
    for (int w = kOptThreads / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) sd[threadIdx.x] += sd[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float total = (float)sqrt(sd[0]);
        float coef = 1.0f;
        if (max_norm >= 0.f) coef = fminf(max_norm / (total + 1e-6f), 1.0f);
        out2[0] = total;
        out2[1] = coef;
    }
}

struct AdamArgs {
    float* const* params;
    const float* const* grads;
    float* const* exp_avg;
    float* const* exp_avg_sq;
    const int64_t* numel;
    const int32_t* chunk_tensor;
    const int32_t* chunk_index;
    int64_t chunk;
    float decay;       // 1 - lr * weight_decay
    float w1;          // 1 - beta1
    float beta2, w2;   // beta2, 1 - beta2
    float step_size;   // lr / (1 - beta1^t)
    float bc2_sqrt;    // sqrt(1 - beta2^t)
    float eps;
    const float* coef; // optional device scalar multiplied into every gradient (the clip coefficient)
};

__device__ inline void adam_one(float& p, float g, float& m, float& v, const AdamArgs& a, float coef) {
    g *= coef;
    p *= a.decay;
    m = m + a.w1 * (g - m);
    v = v * a.beta2 + a.w2 * g * g;   // addcmul_: value * t1 * t2, left to right
    const float denom = sqrtf(v) / a.bc2_sqrt + a.eps;
    p = p - a.step_size * (m / denom);
}

__global__ __launch_bounds__(kOptThreads) void k_adamw(const AdamArgs a) {
    const int t = a.chunk_tensor[blockIdx.x];
    const int64_t lo = (int64_t)a.chunk_index[blockIdx.x] * a.chunk;
    const int64_t n = a.numel[t];
    const int64_t hi = lo + a.chunk < n ? lo + a.chunk : n;
    float* p = a.params[t];
    const float* g = a.grads[t];
    float* m = a.exp_avg[t];
    float* v = a.exp_avg_sq[t];
    const float coef = a.coef ? a.coef[1] : 1.0f;
    const bool al = ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(m) | reinterpret_cast<uintptr_t>(v)) & 15) == 0;
    int64_t tail = lo;
    if (al) {
        const int64_t hi4 = lo + ((hi - lo) & ~(int64_t)3);
        for (int64_t i = lo + 4 * threadIdx.x; i < hi4; i += 4 * kOptThreads) {
            float4 P = *reinterpret_cast<float4*>(p + i), M = *reinterpret_cast<float4*>(m + i), V = *reinterpret_cast<float4*>(v + i);
            const float4 G = *reinterpret_cast<const float4*>(g + i);
            adam_one(P.x, G.x, M.x, V.x, a, coef);
            adam_one(P.y, G.y, M.y, V.y, a, coef);
            adam_one(P.z, G.z, M.z, V.z, a, coef);
            adam_one(P.w, G.w, M.w, V.w, a, coef);
            *reinterpret_cast<float4*>(p + i) = P;
            *reinterpret_cast<float4*>(m + i) = M;
            *reinterpret_cast<float4*>(v + i) = V;
        }
        tail = hi4;
    }
    for (int64_t i = tail + threadIdx.x; i < hi; i += kOptThreads) {
        float P = p[i], M = m[i], V = v[i];
        adam_one(P, g[i], M, V, a, coef);
        p[i] = P; m[i] = M; v[i] = V;
    }
}

// ---- several param groups in one launch: the seven prefactors of every group travel by value in the kernel-argument block (no host-to-device
// copy, nothing to keep alive), and a workgroup picks its tensor's row once
struct AdamGroup {
    float decay, w1, beta2, w2, step_size, bc2_sqrt, eps;   // as in AdamArgs
};

struct AdamGroupsArgs {
    float* const* params;
    const float* const* grads;
    float* const* exp_avg;
    float* const* exp_avg_sq;
    const int64_t* numel;
    const int32_t* tensor_group;
    const int32_t* chunk_tensor;
    const int32_t* chunk_index;
    int64_t chunk;
    const float* coef;
    int32_t n_groups;
    AdamGroup group[QATVIT_OPTIM_MAX_GROUPS];
};

// k_adamw with AdamArgs assembled per workgroup: the same adam_one on the same operands in the same order, so a tensor is updated to the same bits
// whichever of the two kernels it goes through (tests/test_gpu_optim_groups.py: identity).  A tensor of no group (the host cannot see that table) gets an
// empty range instead of an early exit, so that the row - the last link of the chain chunk -> tensor -> group -> row - is fetched while the first
// vector loads are in flight rather than in front of them.
__global__ __launch_bounds__(kOptThreads) void k_adamw_groups(const AdamGroupsArgs ga) {
    const int t = ga.chunk_tensor[blockIdx.x];
    const int gi = __builtin_amdgcn_readfirstlane(ga.tensor_group[t]);   // uniform: the row is read into scalars, once
    const bool in_group = (unsigned)gi < (unsigned)ga.n_groups;
    const AdamGroup h = ga.group[in_group ? gi : 0];
    const AdamArgs a{ga.params, ga.grads, ga.exp_avg, ga.exp_avg_sq, ga.numel, ga.chunk_tensor, ga.chunk_index, ga.chunk,
                     h.decay, h.w1, h.beta2, h.w2, h.step_size, h.bc2_sqrt, h.eps, ga.coef};
    const int64_t lo = (int64_t)a.chunk_index[blockIdx.x] * a.chunk;
    const int64_t n = a.numel[t];
    const int64_t hi = !in_group ? lo : lo + a.chunk < n ? lo + a.chunk : n;   // no group: both loops are empty
    float* p = a.params[t];
    const float* g = a.grads[t];
    float* m = a.exp_avg[t];
    float* v = a.exp_avg_sq[t];
    const float coef = a.coef ? a.coef[1] : 1.0f;
    const bool al = ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(m) | reinterpret_cast<uintptr_t>(v)) & 15) == 0;
    int64_t tail = lo;
    if (al) {
        const int64_t hi4 = lo + ((hi - lo) & ~(int64_t)3);
        for (int64_t i = lo + 4 * threadIdx.x; i < hi4; i += 4 * kOptThreads) {
            float4 P = *reinterpret_cast<float4*>(p + i), M = *reinterpret_cast<float4*>(m + i), V = *reinterpret_cast<float4*>(v + i);
            const float4 G = *reinterpret_cast<const float4*>(g + i);
            adam_one(P.x, G.x, M.x, V.x, a, coef);
            adam_one(P.y, G.y, M.y, V.y, a, coef);
            adam_one(P.z, G.z, M.z, V.z, a, coef);
            adam_one(P.w, G.w, M.w, V.w, a, coef);
            *reinterpret_cast<float4*>(p + i) = P;
            *reinterpret_cast<float4*>(m + i) = M;
            *reinterpret_cast<float4*>(v + i) = V;
        }
        tail = hi4;
    }
    for (int64_t i = tail + threadIdx.x; i < hi; i += kOptThreads) {
        float P = p[i], M = m[i], V = v[i];
        adam_one(P, g[i], M, V, a, coef);
        p[i] = P; m[i] = M; v[i] = V;
    }
}

// ---- the same two updates with the weight average as a fifth stream.  The chunk tables, the float4 body with its scalar tail and adam_one are
// those of k_adamw; the 16-byte alignment test includes e.  p, m, v come out with the bits k_adamw / k_adamw_groups give them.
__device__ inline float ema_one(float e, float p, float w) {
    const float d = p - e;
    return w < 0.5f ? e + w * d : p - d * (1.0f - w);   // ATen lerp(e, p, w), both branches
}

__device__ inline void adamw_ema_range(const AdamArgs& a, int t, int64_t lo, int64_t hi, float* __restrict__ e, float w) {
    float* p = a.params[t];
    const float* g = a.grads[t];
    float* m = a.exp_avg[t];
    float* v = a.exp_avg_sq[t];
    const float coef = a.coef ? a.coef[1] : 1.0f;
    const bool al = ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(m) | reinterpret_cast<uintptr_t>(v) |
                      reinterpret_cast<uintptr_t>(e)) & 15) == 0;
    int64_t tail = lo;
    if (al) {
        const int64_t hi4 = lo + ((hi - lo) & ~(int64_t)3);
        for (int64_t i = lo + 4 * threadIdx.x; i < hi4; i += 4 * kOptThreads) {
            float4 P = *reinterpret_cast<float4*>(p + i), M = *reinterpret_cast<float4*>(m + i), V = *reinterpret_cast<float4*>(v + i);
            const float4 G = *reinterpret_cast<const float4*>(g + i);
            float4 E = *reinterpret_cast<float4*>(e + i);
            adam_one(P.x, G.x, M.x, V.x, a, coef);
            adam_one(P.y, G.y, M.y, V.y, a, coef);
            adam_one(P.z, G.z, M.z, V.z, a, coef);
            adam_one(P.w, G.w, M.w, V.w, a, coef);
            E.x = ema_one(E.x, P.x, w);
            E.y = ema_one(E.y, P.y, w);
            E.z = ema_one(E.z, P.z, w);
            E.w = ema_one(E.w, P.w, w);
            *reinterpret_cast<float4*>(p + i) = P;
            *reinterpret_cast<float4*>(m + i) = M;
            *reinterpret_cast<float4*>(v + i) = V;
            *reinterpret_cast<float4*>(e + i) = E;
        }
        tail = hi4;
    }
    for (int64_t i = tail + threadIdx.x; i < hi; i += kOptThreads) {
        float P = p[i], M = m[i], V = v[i];
        adam_one(P, g[i], M, V, a, coef);
        p[i] = P; m[i] = M; v[i] = V;
        e[i] = ema_one(e[i], P, w);
    }
}

struct EmaArgs {
    float* const* ema;
    float w;   // 1 - ema_decay
};

__global__ __launch_bounds__(kOptThreads) void k_adamw_ema(const AdamArgs a, const EmaArgs ea) {
    const int t = a.chunk_tensor[blockIdx.x];
    const int64_t lo = (int64_t)a.chunk_index[blockIdx.x] * a.chunk;
    const int64_t n = a.numel[t];
    const int64_t hi = lo + a.chunk < n ? lo + a.chunk : n;
    adamw_ema_range(a, t, lo, hi, ea.ema[t], ea.w);
}

// the row of the tensor's group as in k_adamw_groups (a tensor of no group: an empty range); one decay for all groups
__global__ __launch_bounds__(kOptThreads) void k_adamw_groups_ema(const AdamGroupsArgs ga, const EmaArgs ea) {
    const int t = ga.chunk_tensor[blockIdx.x];
    const int gi = __builtin_amdgcn_readfirstlane(ga.tensor_group[t]);
    const bool in_group = (unsigned)gi < (unsigned)ga.n_groups;
    const AdamGroup h = ga.group[in_group ? gi : 0];
    const AdamArgs a{ga.params, ga.grads, ga.exp_avg, ga.exp_avg_sq, ga.numel, ga.chunk_tensor, ga.chunk_index, ga.chunk,
                     h.decay, h.w1, h.beta2, h.w2, h.step_size, h.bc2_sqrt, h.eps, ga.coef};
    const int64_t lo = (int64_t)a.chunk_index[blockIdx.x] * a.chunk;
    const int64_t n = a.numel[t];
    const int64_t hi = !in_group ? lo : lo + a.chunk < n ? lo + a.chunk : n;
    adamw_ema_range(a, t, lo, hi, ea.ema[t], ea.w);
}

// e <- lerp(e, p, w) for tensors that take no update: p is read only
__global__ __launch_bounds__(kOptThreads) void k_ema(const float* const* __restrict__ params, float* const* __restrict__ ema,
                                                     const int64_t* __restrict__ numel, const int32_t* __restrict__ chunk_tensor,
                                                     const int32_t* __restrict__ chunk_index, int64_t chunk, float w) {
    const int t = chunk_tensor[blockIdx.x];
    const int64_t lo = (int64_t)chunk_index[blockIdx.x] * chunk;
    const int64_t n = numel[t];
    const int64_t hi = lo + chunk < n ? lo + chunk : n;
    const float* p = params[t];
    float* e = ema[t];
    int64_t tail = lo;
    if (((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(e)) & 15) == 0) {
        const int64_t hi4 = lo + ((hi - lo) & ~(int64_t)3);
        for (int64_t i = lo + 4 * threadIdx.x; i < hi4; i += 4 * kOptThreads) {
            const float4 P = *reinterpret_cast<const float4*>(p + i);
            float4 E = *reinterpret_cast<float4*>(e + i);
            E.x = ema_one(E.x, P.x, w);
            E.y = ema_one(E.y, P.y, w);
            E.z = ema_one(E.z, P.z, w);
            E.w = ema_one(E.w, P.w, w);
            *reinterpret_cast<float4*>(e + i) = E;
        }
        tail = hi4;
    }
    for (int64_t i = tail + threadIdx.x; i < hi; i += kOptThreads) e[i] = ema_one(e[i], p[i], w);
}

// a[t] <-> b[t], as 32-bit words (no float is formed: NaN payloads and signed zeros pass through)
__global__ __launch_bounds__(kOptThreads) void k_swap(uint32_t* const* __restrict__ as, uint32_t* const* __restrict__ bs, const int64_t* __restrict__ numel,
                                                      const int32_t* __restrict__ chunk_tensor, const int32_t* __restrict__ chunk_index, int64_t chunk) {
    const int t = chunk_tensor[blockIdx.x];
    const int64_t lo = (int64_t)chunk_index[blockIdx.x] * chunk;
    const int64_t n = numel[t];
    const int64_t hi = lo + chunk < n ? lo + chunk : n;
    uint32_t* a = as[t];
    uint32_t* b = bs[t];
    int64_t tail = lo;
    if (((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15) == 0) {
        const int64_t hi4 = lo + ((hi - lo) & ~(int64_t)3);
        for (int64_t i = lo + 4 * threadIdx.x; i < hi4; i += 4 * kOptThreads) {
            const uint4 A = *reinterpret_cast<const uint4*>(a + i), B = *reinterpret_cast<const uint4*>(b + i);
            *reinterpret_cast<uint4*>(a + i) = B;
            *reinterpret_cast<uint4*>(b + i) = A;
        }
        tail = hi4;
    }
    for (int64_t i = tail + threadIdx.x; i < hi; i += kOptThreads) {
        const uint32_t A = a[i], B = b[i];
        a[i] = B;
        b[i] = A;
    }
}

}  // namespace qv

using namespace qv;

extern "C" {

int qatvit_optim_grad_norm(const void* grad_ptrs, const int64_t* numel, const int32_t* chunk_tensor, const int32_t* chunk_index,
                           int32_t n_chunks, int64_t chunk_elems, float max_norm, float* partials, float* out2, void* stream) {
    QV_CHECK_ARG(grad_ptrs && numel && chunk_tensor && chunk_index && partials && out2, "qatvit_optim_grad_norm: null pointer");
    QV_CHECK_ARG(n_chunks > 0 && chunk_elems > 0 && chunk_elems % 4 == 0, "qatvit_optim_grad_norm: bad chunking (n_chunks=%d chunk=%lld)", n_chunks,
                 (long long)chunk_elems);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    k_grad_sqnorm<<<n_chunks, kOptThreads, 0, st>>>(reinterpret_cast<const float* const*>(grad_ptrs), numel, chunk_tensor, chunk_index, chunk_elems,
                                                    partials);
    QV_CHECK_LAUNCH("k_grad_sqnorm");
    k_clip_coef<<<1, kOptThreads, 0, st>>>(partials, n_chunks, max_norm, out2);
    QV_CHECK_LAUNCH("k_clip_coef");
    return 0;
}

int qatvit_optim_adamw(const void* param_ptrs, const void* grad_ptrs, const void* exp_avg_ptrs, const void* exp_avg_sq_ptrs, const int64_t* numel,
                       const int32_t* chunk_tensor, const int32_t* chunk_index, int32_t n_chunks, int64_t chunk_elems, double lr, double beta1,
                       double beta2, double eps, double weight_decay, int64_t step, const float* clip_out2, void* stream) {
    QV_CHECK_ARG(param_ptrs && grad_ptrs && exp_avg_ptrs && exp_avg_sq_ptrs && numel && chunk_tensor && chunk_index,
                 "qatvit_optim_adamw: null pointer");
    QV_CHECK_ARG(n_chunks > 0 && chunk_elems > 0 && chunk_elems % 4 == 0, "qatvit_optim_adamw: bad chunking (n_chunks=%d chunk=%lld)", n_chunks,
                 (long long)chunk_elems);
    QV_CHECK_ARG(step >= 1 && lr >= 0. && beta1 >= 0. && beta1 < 1. && beta2 >= 0. && beta2 < 1. && eps >= 0.,
                 "qatvit_optim_adamw: bad hyper-parameters (step=%lld lr=%g betas=(%g, %g) eps=%g)", (long long)step, lr, beta1, beta2, eps);
    // scalar prefactors exactly as torch/optim/adamw.py forms them (python floats = doubles, narrowed once)
    // (hyper-parameters arrive as doubles for that reason: 1 - float(0.999) is 1.3e-5 away from float(1 - 0.999))
    const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
    AdamArgs a{reinterpret_cast<float* const*>(param_ptrs), reinterpret_cast<const float* const*>(grad_ptrs),
               reinterpret_cast<float* const*>(exp_avg_ptrs), reinterpret_cast<float* const*>(exp_avg_sq_ptrs), numel, chunk_tensor, chunk_index,
               chunk_elems, (float)(1.0 - lr * weight_decay), (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2),
               (float)(lr / bc1), (float)sqrt(bc2), (float)eps, clip_out2};
    k_adamw<<<n_chunks, kOptThreads, 0, reinterpret_cast<hipStream_t>(stream)>>>(a);
    QV_CHECK_LAUNCH("k_adamw");
    return 0;
}

int qatvit_optim_adamw_groups(const void* param_ptrs, const void* grad_ptrs, const void* exp_avg_ptrs, const void* exp_avg_sq_ptrs, const int64_t* numel,
                              const int32_t* tensor_group, const int32_t* chunk_tensor, const int32_t* chunk_index, int32_t n_chunks,
                              int64_t chunk_elems, const qatvit_adamw_group* groups, int32_t n_groups, const float* clip_out2, void* stream) {
    QV_CHECK_ARG(param_ptrs && grad_ptrs && exp_avg_ptrs && exp_avg_sq_ptrs && numel && tensor_group && chunk_tensor && chunk_index && groups,
                 "qatvit_optim_adamw_groups: null pointer");
    QV_CHECK_ARG(n_chunks > 0 && chunk_elems > 0 && chunk_elems % 4 == 0, "qatvit_optim_adamw_groups: bad chunking (n_chunks=%d chunk=%lld)", n_chunks,
                 (long long)chunk_elems);
    QV_CHECK_ARG(n_groups >= 1 && n_groups <= QATVIT_OPTIM_MAX_GROUPS, "qatvit_optim_adamw_groups: n_groups %d outside [1, %d]", n_groups,
                 QATVIT_OPTIM_MAX_GROUPS);
    AdamGroupsArgs a{reinterpret_cast<float* const*>(param_ptrs), reinterpret_cast<const float* const*>(grad_ptrs),
                     reinterpret_cast<float* const*>(exp_avg_ptrs), reinterpret_cast<float* const*>(exp_avg_sq_ptrs), numel, tensor_group, chunk_tensor,
                     chunk_index, chunk_elems, clip_out2, n_groups, {}};
    for (int i = 0; i < n_groups; ++i) {
        const qatvit_adamw_group& g = groups[i];
        QV_CHECK_ARG(g.step >= 1 && g.lr >= 0. && g.beta1 >= 0. && g.beta1 < 1. && g.beta2 >= 0. && g.beta2 < 1. && g.eps >= 0. && g.weight_decay >= 0.,
                     "qatvit_optim_adamw_groups: bad hyper-parameters in group %d (step=%lld lr=%g betas=(%g, %g) eps=%g weight_decay=%g)", i,
                     (long long)g.step, g.lr, g.beta1, g.beta2, g.eps, g.weight_decay);
        // the prefactors of qatvit_optim_adamw, formed the same way (doubles, narrowed once)
        const double bc1 = 1.0 - pow(g.beta1, (double)g.step), bc2 = 1.0 - pow(g.beta2, (double)g.step);
        a.group[i] = AdamGroup{(float)(1.0 - g.lr * g.weight_decay), (float)(1.0 - g.beta1), (float)g.beta2, (float)(1.0 - g.beta2),
                               (float)(g.lr / bc1), (float)sqrt(bc2), (float)g.eps};
    }
    k_adamw_groups<<<n_chunks, kOptThreads, 0, reinterpret_cast<hipStream_t>(stream)>>>(a);
    QV_CHECK_LAUNCH("k_adamw_groups");
    return 0;
}

// ---- weight EMA: the two update entries with ema_ptrs / ema_decay, the average alone, the exchange.  (The argument checks of the update entries are
// those of qatvit_optim_adamw / qatvit_optim_adamw_groups under the new names, then the decay.)
#define QV_CHECK_EMA_DECAY(fn) \
    QV_CHECK_ARG(ema_decay >= 0. && ema_decay < 1., fn ": ema_decay %g outside [0, 1)", ema_decay)   /* NaN fails both comparisons */

int qatvit_optim_adamw_ema(const void* param_ptrs, const void* grad_ptrs, const void* exp_avg_ptrs, const void* exp_avg_sq_ptrs, const void* ema_ptrs,
                           const int64_t* numel, const int32_t* chunk_tensor, const int32_t* chunk_index, int32_t n_chunks, int64_t chunk_elems,
                           double lr, double beta1, double beta2, double eps, double weight_decay, int64_t step, double ema_decay,
                           const float* clip_out2, void* stream) {
    QV_CHECK_ARG(param_ptrs && grad_ptrs && exp_avg_ptrs && exp_avg_sq_ptrs && ema_ptrs && numel && chunk_tensor && chunk_index,
                 "qatvit_optim_adamw_ema: null pointer");
    QV_CHECK_ARG(n_chunks > 0 && chunk_elems > 0 && chunk_elems % 4 == 0, "qatvit_optim_adamw_ema: bad chunking (n_chunks=%d chunk=%lld)", n_chunks,
                 (long long)chunk_elems);
    QV_CHECK_ARG(step >= 1 && lr >= 0. && beta1 >= 0. && beta1 < 1. && beta2 >= 0. && beta2 < 1. && eps >= 0.,
                 "qatvit_optim_adamw_ema: bad hyper-parameters (step=%lld lr=%g betas=(%g, %g) eps=%g)", (long long)step, lr, beta1, beta2, eps);
    QV_CHECK_EMA_DECAY("qatvit_optim_adamw_ema");
    const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);   // the prefactors of qatvit_optim_adamw
    AdamArgs a{reinterpret_cast<float* const*>(param_ptrs), reinterpret_cast<const float* const*>(grad_ptrs),
               reinterpret_cast<float* const*>(exp_avg_ptrs), reinterpret_cast<float* const*>(exp_avg_sq_ptrs), numel, chunk_tensor, chunk_index,
               chunk_elems, (float)(1.0 - lr * weight_decay), (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2),
               (float)(lr / bc1), (float)sqrt(bc2), (float)eps, clip_out2};
    const EmaArgs ea{reinterpret_cast<float* const*>(ema_ptrs), (float)(1.0 - ema_decay)};
    k_adamw_ema<<<n_chunks, kOptThreads, 0, reinterpret_cast<hipStream_t>(stream)>>>(a, ea);
    QV_CHECK_LAUNCH("k_adamw_ema");
    return 0;
}

int qatvit_optim_adamw_groups_ema(const void* param_ptrs, const void* grad_ptrs, const void* exp_avg_ptrs, const void* exp_avg_sq_ptrs,
                                  const void* ema_ptrs, const int64_t* numel, const int32_t* tensor_group, const int32_t* chunk_tensor,
                                  const int32_t* chunk_index, int32_t n_chunks, int64_t chunk_elems, const qatvit_adamw_group* groups,
                                  int32_t n_groups, double ema_decay, const float* clip_out2, void* stream) {
    QV_CHECK_ARG(param_ptrs && grad_ptrs && exp_avg_ptrs && exp_avg_sq_ptrs && ema_ptrs && numel && tensor_group && chunk_tensor && chunk_index && groups,
                 "qatvit_optim_adamw_groups_ema: null pointer");
    QV_CHECK_ARG(n_chunks > 0 && chunk_elems > 0 && chunk_elems % 4 == 0, "qatvit_optim_adamw_groups_ema: bad chunking (n_chunks=%d chunk=%lld)", n_chunks,
                 (long long)chunk_elems);
    QV_CHECK_ARG(n_groups >= 1 && n_groups <= QATVIT_OPTIM_MAX_GROUPS, "qatvit_optim_adamw_groups_ema: n_groups %d outside [1, %d]", n_groups,
                 QATVIT_OPTIM_MAX_GROUPS);
    AdamGroupsArgs a{reinterpret_cast<float* const*>(param_ptrs), reinterpret_cast<const float* const*>(grad_ptrs),
                     reinterpret_cast<float* const*>(exp_avg_ptrs), reinterpret_cast<float* const*>(exp_avg_sq_ptrs), numel, tensor_group, chunk_tensor,
                     chunk_index, chunk_elems, clip_out2, n_groups, {}};
    for (int i = 0; i < n_groups; ++i) {
        const qatvit_adamw_group& g = groups[i];
        QV_CHECK_ARG(g.step >= 1 && g.lr >= 0. && g.beta1 >= 0. && g.beta1 < 1. && g.beta2 >= 0. && g.beta2 < 1. && g.eps >= 0. && g.weight_decay >= 0.,
                     "qatvit_optim_adamw_groups_ema: bad hyper-parameters in group %d (step=%lld lr=%g betas=(%g, %g) eps=%g weight_decay=%g)", i,
                     (long long)g.step, g.lr, g.beta1, g.beta2, g.eps, g.weight_decay);
        const double bc1 = 1.0 - pow(g.beta1, (double)g.step), bc2 = 1.0 - pow(g.beta2, (double)g.step);
        a.group[i] = AdamGroup{(float)(1.0 - g.lr * g.weight_decay), (float)(1.0 - g.beta1), (float)g.beta2, (float)(1.0 - g.beta2),
                               (float)(g.lr / bc1), (float)sqrt(bc2), (float)g.eps};
    }
    QV_CHECK_EMA_DECAY("qatvit_optim_adamw_groups_ema");
    const EmaArgs ea{reinterpret_cast<float* const*>(ema_ptrs), (float)(1.0 - ema_decay)};
    k_adamw_groups_ema<<<n_chunks, kOptThreads, 0, reinterpret_cast<hipStream_t>(stream)>>>(a, ea);
    QV_CHECK_LAUNCH("k_adamw_groups_ema");
    return 0;
}

int qatvit_optim_ema(const void* param_ptrs, const void* ema_ptrs, const int64_t* numel, const int32_t* chunk_tensor, const int32_t* chunk_index,
                     int32_t n_chunks, int64_t chunk_elems, double ema_decay, void* stream) {
    QV_CHECK_ARG(param_ptrs && ema_ptrs && numel && chunk_tensor && chunk_index, "qatvit_optim_ema: null pointer");
    QV_CHECK_ARG(n_chunks > 0 && chunk_elems > 0 && chunk_elems % 4 == 0, "qatvit_optim_ema: bad chunking (n_chunks=%d chunk=%lld)", n_chunks,
                 (long long)chunk_elems);
    QV_CHECK_EMA_DECAY("qatvit_optim_ema");
    k_ema<<<n_chunks, kOptThreads, 0, reinterpret_cast<hipStream_t>(stream)>>>(reinterpret_cast<const float* const*>(param_ptrs),
                                                                                reinterpret_cast<float* const*>(ema_ptrs), numel, chunk_tensor,
                                                                                chunk_index, chunk_elems, (float)(1.0 - ema_decay));
    QV_CHECK_LAUNCH("k_ema");
    return 0;
}

int qatvit_optim_swap(const void* a_ptrs, const void* b_ptrs, const int64_t* numel, const int32_t* chunk_tensor, const int32_t* chunk_index,
                      int32_t n_chunks, int64_t chunk_elems, void* stream) {
    QV_CHECK_ARG(a_ptrs && b_ptrs && numel && chunk_tensor && chunk_index, "qatvit_optim_swap: null pointer");
    QV_CHECK_ARG(n_chunks > 0 && chunk_elems > 0 && chunk_elems % 4 == 0, "qatvit_optim_swap: bad chunking (n_chunks=%d chunk=%lld)", n_chunks,
                 (long long)chunk_elems);
    k_swap<<<n_chunks, kOptThreads, 0, reinterpret_cast<hipStream_t>(stream)>>>(reinterpret_cast<uint32_t* const*>(a_ptrs),
                                                                                 reinterpret_cast<uint32_t* const*>(b_ptrs), numel, chunk_tensor,
                                                                                 chunk_index, chunk_elems);
    QV_CHECK_LAUNCH("k_swap");
    return 0;
}

}  // extern "C"
