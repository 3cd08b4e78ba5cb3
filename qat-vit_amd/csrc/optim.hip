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
// extra launch and no second read of p: e' = lerp(e, p', w) with w = (float)(1.0 - ema_decay) (double on the host, narrowed once), in the two
// roundings of ema_one (qv_optim.h).  k_ema is the same average as a launch of its own (12 B per element) for tensors that take no update in a
// step; k_swap exchanges the contents of two tensor lists bit for bit (16 B per element), which is how the averaged weights are evaluated
// without new addresses.
//
// The chunk walk, the AdamW update over a range, the average's formula and the entries' argument checks are written once, in qv_optim.h; the kernels
// here are what each does to its elements, and tools/isa_digest.py holds their machine code to what it was before they shared that text.
#include "qv_kernels.h"
#include "qv_optim.h"

namespace qv {

__global__ __launch_bounds__(kOptThreads) void k_grad_sqnorm(const float* const* __restrict__ grads, const int64_t* __restrict__ numel,
                                                             const int32_t* __restrict__ chunk_tensor, const int32_t* __restrict__ chunk_index,
                                                             int64_t chunk, float* __restrict__ partials) {
    const ChunkRange r = chunk_range(numel, chunk_tensor, chunk_index, chunk);
    const float* g = grads[r.t];
    float s = 0.f;
    const auto f4 = [&](int64_t i) {
        const float4 v = *reinterpret_cast<const float4*>(g + i);
        s += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
    };
    const auto f1 = [&](int64_t i) { s += g[i] * g[i]; };
    if (aligned16(g)) walk_range(true, r, f4, f1);   // (the two cases as two loops of their own: this kernel's code since the first version)
    else walk_range(false, r, f4, f1);
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

// ---- several param groups in one launch: the seven prefactors of every group travel by value in the kernel-argument block (no host-to-device
// copy, nothing to keep alive), and a workgroup picks its tensor's row once (group_row) and assembles the AdamArgs of k_adamw from it
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

__device__ inline AdamArgs group_args(const AdamGroupsArgs& ga, bool& in_group) {
    const AdamGroup h = ga.group[group_row(ga.chunk_tensor, ga.tensor_group, ga.n_groups, in_group)];
    return adam_args(ga.params, ga.grads, ga.exp_avg, ga.exp_avg_sq, ga.numel, ga.chunk_tensor, ga.chunk_index, ga.chunk, h, ga.coef);
}

struct EmaArgs {
    float* const* ema;
    float w;   // 1 - ema_decay
};

// the four updates: one group or the row of the tensor's group, without or with the weight average (one decay for all groups)
__global__ __launch_bounds__(kOptThreads) void k_adamw(const AdamArgs a) {
    adamw_range<false>(a, chunk_range(a.numel, a.chunk_tensor, a.chunk_index, a.chunk), nullptr, 0.f);
}

__global__ __launch_bounds__(kOptThreads) void k_adamw_groups(const AdamGroupsArgs ga) {
    bool in_group;
    const AdamArgs a = group_args(ga, in_group);
    adamw_range<false>(a, chunk_range(a.numel, a.chunk_tensor, a.chunk_index, a.chunk, in_group), nullptr, 0.f);
}

__global__ __launch_bounds__(kOptThreads) void k_adamw_ema(const AdamArgs a, const EmaArgs ea) {
    const ChunkRange r = chunk_range(a.numel, a.chunk_tensor, a.chunk_index, a.chunk);
    adamw_range<true>(a, r, ea.ema[r.t], ea.w);
}

__global__ __launch_bounds__(kOptThreads) void k_adamw_groups_ema(const AdamGroupsArgs ga, const EmaArgs ea) {
    bool in_group;
    const AdamArgs a = group_args(ga, in_group);
    const ChunkRange r = chunk_range(a.numel, a.chunk_tensor, a.chunk_index, a.chunk, in_group);
    adamw_range<true>(a, r, ea.ema[r.t], ea.w);
}

// e <- lerp(e, p, w) for tensors that take no update: p is read only
__global__ __launch_bounds__(kOptThreads) void k_ema(const float* const* __restrict__ params, float* const* __restrict__ ema,
                                                     const int64_t* __restrict__ numel, const int32_t* __restrict__ chunk_tensor,
                                                     const int32_t* __restrict__ chunk_index, int64_t chunk, float w) {
    const ChunkRange r = chunk_range(numel, chunk_tensor, chunk_index, chunk);
    const float* p = params[r.t];
    float* e = ema[r.t];
    walk_range(
        aligned16(p, e), r,
        [&](int64_t i) {
            const float4 P = *reinterpret_cast<const float4*>(p + i);
            float4 E = *reinterpret_cast<float4*>(e + i);
            E.x = ema_one(E.x, P.x, w);
            E.y = ema_one(E.y, P.y, w);
            E.z = ema_one(E.z, P.z, w);
            E.w = ema_one(E.w, P.w, w);
            *reinterpret_cast<float4*>(e + i) = E;
        },
        [&](int64_t i) { e[i] = ema_one(e[i], p[i], w); });
}

// a[t] <-> b[t], as 32-bit words (no float is formed: NaN payloads and signed zeros pass through)
__global__ __launch_bounds__(kOptThreads) void k_swap(uint32_t* const* __restrict__ as, uint32_t* const* __restrict__ bs, const int64_t* __restrict__ numel,
                                                      const int32_t* __restrict__ chunk_tensor, const int32_t* __restrict__ chunk_index, int64_t chunk) {
    const ChunkRange r = chunk_range(numel, chunk_tensor, chunk_index, chunk);
    uint32_t* a = as[r.t];
    uint32_t* b = bs[r.t];
    walk_range(
        aligned16(a, b), r,
        [&](int64_t i) {
            const uint4 A = *reinterpret_cast<const uint4*>(a + i), B = *reinterpret_cast<const uint4*>(b + i);
            *reinterpret_cast<uint4*>(a + i) = B;
            *reinterpret_cast<uint4*>(b + i) = A;
        },
        [&](int64_t i) {
            const uint32_t A = a[i], B = b[i];
            a[i] = B;
            b[i] = A;
        });
}

// the operands of the groups entries as the kernels' argument block, rows checked and narrowed in ascending order; false: an argument error
static bool adam_groups_args(const char* fn, const void* param_ptrs, const void* grad_ptrs, const void* exp_avg_ptrs, const void* exp_avg_sq_ptrs,
                             const int64_t* numel, const int32_t* tensor_group, const int32_t* chunk_tensor, const int32_t* chunk_index,
                             int64_t chunk_elems, const qatvit_adamw_group* groups, int32_t n_groups, const float* clip_out2, AdamGroupsArgs& a) {
    a = AdamGroupsArgs{ptr_table<float>(param_ptrs), ptr_table<const float>(grad_ptrs), ptr_table<float>(exp_avg_ptrs), ptr_table<float>(exp_avg_sq_ptrs),
                       numel, tensor_group, chunk_tensor, chunk_index, chunk_elems, clip_out2, n_groups, {}};
    for (int i = 0; i < n_groups; ++i) {
        const qatvit_adamw_group& g = groups[i];
        if (!hyper_ok(fn, i, g.step, g.lr, g.beta1, g.beta2, g.eps, g.weight_decay)) return false;
        a.group[i] = adam_prefactors(g.lr, g.beta1, g.beta2, g.eps, g.weight_decay, g.step);
    }
    return true;
}

}  // namespace qv

using namespace qv;

extern "C" {

int qatvit_optim_grad_norm(const void* grad_ptrs, const int64_t* numel, const int32_t* chunk_tensor, const int32_t* chunk_index,
                           int32_t n_chunks, int64_t chunk_elems, float max_norm, float* partials, float* out2, void* stream) {
    if (!tables_ok("qatvit_optim_grad_norm", grad_ptrs && numel && chunk_tensor && chunk_index && partials && out2, n_chunks, chunk_elems)) return 1;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    k_grad_sqnorm<<<n_chunks, kOptThreads, 0, st>>>(ptr_table<const float>(grad_ptrs), numel, chunk_tensor, chunk_index, chunk_elems, partials);
    QV_CHECK_LAUNCH("k_grad_sqnorm");
    k_clip_coef<<<1, kOptThreads, 0, st>>>(partials, n_chunks, max_norm, out2);
    QV_CHECK_LAUNCH("k_clip_coef");
    return 0;
}

int qatvit_optim_adamw(const void* param_ptrs, const void* grad_ptrs, const void* exp_avg_ptrs, const void* exp_avg_sq_ptrs, const int64_t* numel,
                       const int32_t* chunk_tensor, const int32_t* chunk_index, int32_t n_chunks, int64_t chunk_elems, double lr, double beta1,
                       double beta2, double eps, double weight_decay, int64_t step, const float* clip_out2, void* stream) {
    const char* fn = "qatvit_optim_adamw";
    if (!tables_ok(fn, param_ptrs && grad_ptrs && exp_avg_ptrs && exp_avg_sq_ptrs && numel && chunk_tensor && chunk_index, n_chunks, chunk_elems) ||
        !hyper_ok(fn, -1, step, lr, beta1, beta2, eps, weight_decay))
        return 1;
    const AdamArgs a = adam_args(ptr_table<float>(param_ptrs), ptr_table<const float>(grad_ptrs), ptr_table<float>(exp_avg_ptrs),
                                 ptr_table<float>(exp_avg_sq_ptrs), numel, chunk_tensor, chunk_index, chunk_elems,
                                 adam_prefactors(lr, beta1, beta2, eps, weight_decay, step), clip_out2);
    k_adamw<<<n_chunks, kOptThreads, 0, reinterpret_cast<hipStream_t>(stream)>>>(a);
    QV_CHECK_LAUNCH("k_adamw");
    return 0;
}

int qatvit_optim_adamw_groups(const void* param_ptrs, const void* grad_ptrs, const void* exp_avg_ptrs, const void* exp_avg_sq_ptrs, const int64_t* numel,
                              const int32_t* tensor_group, const int32_t* chunk_tensor, const int32_t* chunk_index, int32_t n_chunks,
                              int64_t chunk_elems, const qatvit_adamw_group* groups, int32_t n_groups, const float* clip_out2, void* stream) {
    const char* fn = "qatvit_optim_adamw_groups";
    AdamGroupsArgs a;
    if (!tables_ok(fn, param_ptrs && grad_ptrs && exp_avg_ptrs && exp_avg_sq_ptrs && numel && tensor_group && chunk_tensor && chunk_index && groups,
                   n_chunks, chunk_elems) ||
        !n_groups_ok(fn, n_groups) ||
        !adam_groups_args(fn, param_ptrs, grad_ptrs, exp_avg_ptrs, exp_avg_sq_ptrs, numel, tensor_group, chunk_tensor, chunk_index, chunk_elems, groups,
                          n_groups, clip_out2, a))
        return 1;
    k_adamw_groups<<<n_chunks, kOptThreads, 0, reinterpret_cast<hipStream_t>(stream)>>>(a);
    QV_CHECK_LAUNCH("k_adamw_groups");
    return 0;
}

// ---- weight EMA: the two update entries with ema_ptrs / ema_decay (the checks of their namesakes, then the decay), the average alone, the exchange
int qatvit_optim_adamw_ema(const void* param_ptrs, const void* grad_ptrs, const void* exp_avg_ptrs, const void* exp_avg_sq_ptrs, const void* ema_ptrs,
                           const int64_t* numel, const int32_t* chunk_tensor, const int32_t* chunk_index, int32_t n_chunks, int64_t chunk_elems,
                           double lr, double beta1, double beta2, double eps, double weight_decay, int64_t step, double ema_decay,
                           const float* clip_out2, void* stream) {
    const char* fn = "qatvit_optim_adamw_ema";
    if (!tables_ok(fn, param_ptrs && grad_ptrs && exp_avg_ptrs && exp_avg_sq_ptrs && ema_ptrs && numel && chunk_tensor && chunk_index, n_chunks,
                   chunk_elems) ||
        !hyper_ok(fn, -1, step, lr, beta1, beta2, eps, weight_decay) || !ema_decay_ok(fn, ema_decay))
        return 1;
    const AdamArgs a = adam_args(ptr_table<float>(param_ptrs), ptr_table<const float>(grad_ptrs), ptr_table<float>(exp_avg_ptrs),
                                 ptr_table<float>(exp_avg_sq_ptrs), numel, chunk_tensor, chunk_index, chunk_elems,
                                 adam_prefactors(lr, beta1, beta2, eps, weight_decay, step), clip_out2);
    const EmaArgs ea{ptr_table<float>(ema_ptrs), (float)(1.0 - ema_decay)};
    k_adamw_ema<<<n_chunks, kOptThreads, 0, reinterpret_cast<hipStream_t>(stream)>>>(a, ea);
    QV_CHECK_LAUNCH("k_adamw_ema");
    return 0;
}

int qatvit_optim_adamw_groups_ema(const void* param_ptrs, const void* grad_ptrs, const void* exp_avg_ptrs, const void* exp_avg_sq_ptrs,
                                  const void* ema_ptrs, const int64_t* numel, const int32_t* tensor_group, const int32_t* chunk_tensor,
                                  const int32_t* chunk_index, int32_t n_chunks, int64_t chunk_elems, const qatvit_adamw_group* groups,
                                  int32_t n_groups, double ema_decay, const float* clip_out2, void* stream) {
    const char* fn = "qatvit_optim_adamw_groups_ema";
    AdamGroupsArgs a;
    if (!tables_ok(fn, param_ptrs && grad_ptrs && exp_avg_ptrs && exp_avg_sq_ptrs && ema_ptrs && numel && tensor_group && chunk_tensor && chunk_index &&
                           groups,
                   n_chunks, chunk_elems) ||
        !n_groups_ok(fn, n_groups) ||
        !adam_groups_args(fn, param_ptrs, grad_ptrs, exp_avg_ptrs, exp_avg_sq_ptrs, numel, tensor_group, chunk_tensor, chunk_index, chunk_elems, groups,
                          n_groups, clip_out2, a) ||
        !ema_decay_ok(fn, ema_decay))
        return 1;
    const EmaArgs ea{ptr_table<float>(ema_ptrs), (float)(1.0 - ema_decay)};
    k_adamw_groups_ema<<<n_chunks, kOptThreads, 0, reinterpret_cast<hipStream_t>(stream)>>>(a, ea);
    QV_CHECK_LAUNCH("k_adamw_groups_ema");
    return 0;
}

int qatvit_optim_ema(const void* param_ptrs, const void* ema_ptrs, const int64_t* numel, const int32_t* chunk_tensor, const int32_t* chunk_index,
                     int32_t n_chunks, int64_t chunk_elems, double ema_decay, void* stream) {
    const char* fn = "qatvit_optim_ema";
    if (!tables_ok(fn, param_ptrs && ema_ptrs && numel && chunk_tensor && chunk_index, n_chunks, chunk_elems) || !ema_decay_ok(fn, ema_decay)) return 1;
    k_ema<<<n_chunks, kOptThreads, 0, reinterpret_cast<hipStream_t>(stream)>>>(ptr_table<const float>(param_ptrs), ptr_table<float>(ema_ptrs), numel,
                                                                                chunk_tensor, chunk_index, chunk_elems, (float)(1.0 - ema_decay));
    QV_CHECK_LAUNCH("k_ema");
    return 0;
}

int qatvit_optim_swap(const void* a_ptrs, const void* b_ptrs, const int64_t* numel, const int32_t* chunk_tensor, const int32_t* chunk_index,
                      int32_t n_chunks, int64_t chunk_elems, void* stream) {
    if (!tables_ok("qatvit_optim_swap", a_ptrs && b_ptrs && numel && chunk_tensor && chunk_index, n_chunks, chunk_elems)) return 1;
    k_swap<<<n_chunks, kOptThreads, 0, reinterpret_cast<hipStream_t>(stream)>>>(ptr_table<uint32_t>(a_ptrs), ptr_table<uint32_t>(b_ptrs), numel,
                                                                                 chunk_tensor, chunk_index, chunk_elems);
    QV_CHECK_LAUNCH("k_swap");
    return 0;
}

}  // extern "C"
