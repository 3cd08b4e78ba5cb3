// The fp16 float form under LayerScale (float_step.hip, fs_backward): the power-of-two scale the gradients INSIDE a residual branch are carried at.
#include "qv_common.h"
#include "qv_device.h"
#include "qv_kernels.h"

namespace qv {

struct FsLsGammas { const float* g[24]; };
// per branch {K, 1 / K} with K = 2^-e for max |gamma| = m * 2^e, m in [0.5, 1) - so that gamma * K is of order one - clamped to [1, 2^24]; 1 for a branch whose
// gammas are all zero
__global__ __launch_bounds__(64) void k_fs_ls_scales(const FsLsGammas t, int D, float* __restrict__ out) {
    const float* __restrict__ g = t.g[blockIdx.x];
    float mx = 0.f;
    for (int c = threadIdx.x; c < D; c += 64) mx = fmaxf(mx, fabsf(g[c]));
    mx = wave_max(mx);
    if (threadIdx.x == 0) {
        int e = 0;
        if (mx > 0.f && mx < INFINITY) frexpf(mx, &e);   // mx = m * 2^e, m in [0.5, 1)
        const int k = e < 0 ? (-e > 24 ? 24 : -e) : 0;
        out[2 * blockIdx.x] = ldexpf(1.f, k);
        out[2 * blockIdx.x + 1] = ldexpf(1.f, -k);
    }
}
// The patch rows of the embedding's gradient once more, as dY0 = fp16(dx * Ke), Ke = the smallest of the nb branch scales (every gradient that reaches a patch
// token came through a branch: it carries a gamma, at most the largest); {Ke, 1 / Ke} go behind the branch entries of `scales`
__global__ __launch_bounds__(256) void k_fs_ls_dy0(const float* __restrict__ dx, _Float16* __restrict__ dY0, int B, int T, int D, float* __restrict__ scales, int nb) {
    float K = scales[0];
    for (int k = 1; k < nb; ++k) K = fminf(K, scales[2 * k]);
    if (blockIdx.x == 0 && threadIdx.x == 0) { scales[2 * nb] = K; scales[2 * nb + 1] = 1.f / K; }   // (a power of two: exact)
    const int d4 = D / 4;
    const int64_t n4 = (int64_t)B * (T - 1) * d4;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = i / d4;            // patch row b * (T - 1) + (t - 1) of dY0 = row b * T + t of dx
        const int c = (int)(i % d4) * 4;
        const int64_t b = row / (T - 1), t = row % (T - 1) + 1;
        const float4 g = *reinterpret_cast<const float4*>(dx + (b * T + t) * D + c);
        _Float16* o = dY0 + row * D + c;
        o[0] = (_Float16)(g.x * K); o[1] = (_Float16)(g.y * K); o[2] = (_Float16)(g.z * K); o[3] = (_Float16)(g.w * K);
    }
}

int launch_fs_ls_scales(const float* const* gammas, int branches, int D, float* scales, hipStream_t st) {
    if (branches < 1 || branches > 24 || D < 1) { set_error("fs_ls_scales: %d branches (at most 24), D=%d", branches, D); return 1; }
    FsLsGammas t{};
    for (int k = 0; k < branches; ++k) t.g[k] = gammas[k];
    k_fs_ls_scales<<<branches, 64, 0, st>>>(t, D, scales);
    return 0;
}
int launch_fs_ls_dy0(const float* dx, void* dY0_f16, int B, int T, int D, float* scales, int branches, hipStream_t st) {
    if (T < 2 || D % 4 != 0) { set_error("fs_ls_dy0: T=%d, D=%d", T, D); return 1; }
    const int64_t n4 = (int64_t)B * (T - 1) * (D / 4);
    k_fs_ls_dy0<<<(int)(n4 + 255) / 256 > 2048 ? 2048 : (int)((n4 + 255) / 256), 256, 0, st>>>(dx, reinterpret_cast<_Float16*>(dY0_f16), B, T, D, scales, branches);
    return 0;
}

}  // namespace qv
