// The AdamW update body with four and with five streams on CONTIGUOUS buffers of the ViT-S parameter count, plain and with nontemporal loads / stores:
// separates what the fifth (EMA) stream costs from how torch laid the 152 tensors out (profiles/optim_ema_bench.txt).  Stand-alone:
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -ffp-contract=off tools/probe_optim_streams.hip -o tools/probe_optim_streams && timeout -k 10 120 tools/probe_optim_streams
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e_), __LINE__); exit(2); } } while (0)

constexpr int T = 256;
constexpr long CH = 16384;
struct H { float decay, w1, beta2, w2, step_size, bc2_sqrt, eps; };

__device__ inline void adam_one(float& p, float g, float& m, float& v, const H& a, float coef) {
    g *= coef;
    p *= a.decay;
    m = m + a.w1 * (g - m);
    v = v * a.beta2 + a.w2 * g * g;
    const float denom = sqrtf(v) / a.bc2_sqrt + a.eps;
    p = p - a.step_size * (m / denom);
}
__device__ inline float ema_one(float e, float p, float w) {
    const float d = p - e;
    return w < 0.5f ? e + w * d : p - d * (1.0f - w);
}
typedef float f4 __attribute__((ext_vector_type(4)));
template <int NT> __device__ inline f4 ld(const float* p) {
    if (NT & 1) return __builtin_nontemporal_load(reinterpret_cast<const f4*>(p));
    return *reinterpret_cast<const f4*>(p);
}
template <int NT> __device__ inline void st(float* p, f4 v) {
    if (NT & 2) __builtin_nontemporal_store(v, reinterpret_cast<f4*>(p));
    else *reinterpret_cast<f4*>(p) = v;
}

// EMA: 0 = no fifth stream, 1 = fifth stream; NT bit 0 = nontemporal loads, bit 1 = nontemporal stores; U = float4 per thread and iteration
template <int EMA, int NT, int U>
__global__ __launch_bounds__(T) void k(float* p, const float* g, float* m, float* v, float* e, long n, H h, float w) {
    const long lo = (long)blockIdx.x * CH;
    const long hi = lo + CH < n ? lo + CH : n;
    const long hi4 = lo + ((hi - lo) & ~(long)(4 * U - 1));
    for (long i0 = lo + 4 * threadIdx.x; i0 < hi4; i0 += 4 * T * U) {
        f4 P[U], M[U], V[U], G[U], E[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const long i = i0 + (long)u * 4 * T;
            P[u] = ld<NT>(p + i); M[u] = ld<NT>(m + i); V[u] = ld<NT>(v + i); G[u] = ld<NT>(g + i);
            if (EMA) E[u] = ld<NT>(e + i);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const long i = i0 + (long)u * 4 * T;
            float pp[4] = {P[u].x, P[u].y, P[u].z, P[u].w}, mm[4] = {M[u].x, M[u].y, M[u].z, M[u].w}, vv[4] = {V[u].x, V[u].y, V[u].z, V[u].w};
            const float gg[4] = {G[u].x, G[u].y, G[u].z, G[u].w};
#pragma unroll
            for (int c = 0; c < 4; ++c) adam_one(pp[c], gg[c], mm[c], vv[c], h, 0.5f);
            P[u] = f4{pp[0], pp[1], pp[2], pp[3]}; M[u] = f4{mm[0], mm[1], mm[2], mm[3]}; V[u] = f4{vv[0], vv[1], vv[2], vv[3]};
            st<NT>(p + i, P[u]); st<NT>(m + i, M[u]); st<NT>(v + i, V[u]);
            if (EMA) {
                E[u] = f4{ema_one(E[u].x, pp[0], w), ema_one(E[u].y, pp[1], w), ema_one(E[u].z, pp[2], w), ema_one(E[u].w, pp[3], w)};
                st<NT>(e + i, E[u]);
            }
        }
    }
    for (long i = hi4 + threadIdx.x; i < hi; i += T) {   // (n is a multiple of the tile here; kept for bounds)
        float P = p[i], M = m[i], V = v[i];
        adam_one(P, g[i], M, V, h, 0.5f);
        p[i] = P; m[i] = M; v[i] = V;
        if (EMA) e[i] = ema_one(e[i], P, w);
    }
}

int main() {
    const long n = 21669514 / CH * CH;   // whole chunks, the ViT-S parameter count rounded down
    float *p, *g, *m, *v, *e;
    std::vector<float> hst(n, 0.01f);
    for (float** q : {&p, &g, &m, &v, &e}) { CK(hipMalloc(q, n * sizeof(float))); CK(hipMemcpy(*q, hst.data(), n * sizeof(float), hipMemcpyHostToDevice)); }
    const H h{0.99995f, 0.1f, 0.999f, 0.001f, 1e-3f, 0.1f, 1e-8f};
    const int grid = (int)((n + CH - 1) / CH);
    hipEvent_t a, b; CK(hipEventCreate(&a)); CK(hipEventCreate(&b));
    auto run = [&](const char* name, int bytes, auto kern) {
        for (int i = 0; i < 20; ++i) kern<<<grid, T>>>(p, g, m, v, e, n, h, 2e-4f);
        CK(hipDeviceSynchronize());
        for (int r = 0; r < 3; ++r) {
            CK(hipEventRecord(a));
            for (int i = 0; i < 100; ++i) kern<<<grid, T>>>(p, g, m, v, e, n, h, 2e-4f);
            CK(hipEventRecord(b)); CK(hipEventSynchronize(b));
            float ms; CK(hipEventElapsedTime(&ms, a, b));
            printf("%-28s %7.1f us  %5.2f TB/s\n", name, ms * 10.f, bytes * (double)n / (ms * 10.0) / 1e6);
        }
        CK(hipGetLastError());
    };
    for (int round = 0; round < 2; ++round) {
        run("adamw 4 streams", 28, k<0, 0, 1>);
        run("ema   5 streams", 36, k<1, 0, 1>);
        run("ema   nt stores", 36, k<1, 2, 1>);
        run("ema   nt loads+stores", 36, k<1, 3, 1>);
        run("ema   2 x float4", 36, k<1, 0, 2>);
        run("ema   2 x float4 nt", 36, k<1, 3, 2>);
        run("adamw nt loads+stores", 28, k<0, 3, 1>);
    }
    fflush(stdout);
    return 0;
}
