// Float (pre-QAT) student step, fp16 form: what the step computes inside torch.autocast("cuda", dtype=torch.float16), native on gfx950.
//
// Replaces: the reference's autocast float epochs (the Optuna objective: autocast + GradScaler before prepare_qat).  Stock autocast runs every
// Linear / Conv2d / matmul on fp16 operands with fp32 accumulation and keeps the residual stream, LayerNorm and softmax in fp32; this form does
// the same with one fp16 plane per GEMM operand and one v_mfma_f32_16x16x32_f16 pass per product:
//   forward   the teacher's one-pass fp16 pieces (k_patches_split / k_resid_ln_split / k_attn_fwd_float with f16), keeping LayerNorm mean / rstd,
//             lse, the fc1 pre-activation and the fp16 activation planes the weight gradients read; GEMM outputs stay fp32; fp16 logits.
//   backward  dgrad = launch_gemm_nt (kNTPlaneF16 / kNTPlaneBf16) and wgrad = launch_gemm_tn (kTNPlaneF16 / kTNPlaneBf16) with unit scales; the LayerNorm backward of the float step (its fused
//             next-branch output as one fp16 plane); new here: the head, GELU', embedding and attention backward in their fp16 forms.
// Overflow follows stock (GradScaler must skip the same steps): every tensor stock holds in fp16 is rounded to nearest (fp16 overflow -> +-inf,
// NaN propagates) where it becomes fp16 - dlogits, dhn, the fc2 dgrad output, dO, dP, dS, dQKV, dY0 - and the
// Linear / Conv2d weight and bias gradients (fp16 tensors under stock autocast, fp32 sums here) take one post-pass: |g| beyond fp16's range -> +-inf.
// The bf16 form (torch.autocast(dtype=torch.bfloat16)) is the same device code on bf16 planes and v_mfma_f32_16x16x32_bf16: every kernel here but the
// overflow rule is a template on the 16-bit element type E (_Float16 or __bf16).  bf16 has fp32's exponent range, so that form needs no overflow rule;
// its roundings (v_cvt_pk_bf16_f32, round to nearest even, NaN kept) still carry inf and NaN into the gradients.
// This file holds the one-plane forms' device code and its launchers; the host driver, shared with the pair form, is float_step.hip.
#include "../../include/qatvit.h"

#include "qv_common.h"
#include "qv_device.h"
#include "qv_kernels.h"

namespace qv {

__device__ inline float f16r(float v) { return (float)(_Float16)v; }   // round to fp16 and back (RNE: beyond 65520 -> inf)
// the element type's pieces: 8-element MFMA fragment, the 16x16x32 MFMA, two floats packed (one v_cvt_pk), round and back
template <typename E> struct Fa;
template <> struct Fa<_Float16> {
    typedef f16x8 v8;
    static __device__ __attribute__((always_inline)) f32x4 mfma(v8 a, v8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
    static __device__ __attribute__((always_inline)) uint32_t pk(float a, float b) { return pk_f16(a, b); }
    static __device__ __attribute__((always_inline)) float r(float v) { return f16r(v); }
};
template <> struct Fa<__bf16> {
    typedef bf16x8 v8;
    static __device__ __attribute__((always_inline)) f32x4 mfma(v8 a, v8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
    static __device__ __attribute__((always_inline)) uint32_t pk(float a, float b) { return pk_bf16(a, b); }
    static __device__ __attribute__((always_inline)) float r(float v) { return (float)(__bf16)v; }
};

// ---------------------------------------------------------------- weights as fp16 / bf16, as stored and transposed (one launch per step)
template <typename E>
struct FaWTab {
    const float* W[kMaxW];
    E* w[kMaxW];
    E* wT[kMaxW];
    int N[kMaxW], K[kMaxW], blk0[kMaxW + 1];
    int n;
};
template <typename E>
__global__ __launch_bounds__(256) void k_fa_wcast(const FaWTab<E> t) {
    __shared__ float tile[32][33];
    int wi = 0;
    while (wi + 1 < t.n && (int)blockIdx.x >= t.blk0[wi + 1]) ++wi;
    const int N = t.N[wi], K = t.K[wi], tilesK = (K + 31) / 32, local = (int)blockIdx.x - t.blk0[wi];
    const int n0 = (local / tilesK) * 32, k0 = (local % tilesK) * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int n = n0 + ty + 8 * i, k = k0 + tx;
        float v = 0.f;
        if (n < N && k < K) {
            v = t.W[wi][(int64_t)n * K + k];
            t.w[wi][(int64_t)n * K + k] = (E)v;
        }
        tile[ty + 8 * i][tx] = v;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int k = k0 + ty + 8 * i, n = n0 + tx;
        if (n < N && k < K) t.wT[wi][(int64_t)k * N + n] = (E)tile[tx][ty + 8 * i];
    }
}

// ---------------------------------------------------------------- head: cls LayerNorm (fp32) -> fp16 Linear -> fp16 logits (the same in bf16)
// hn16[b,:] = fp16(LN(x[b,0,:])) (kept as fp32 values for the backward); logits[b,c] = fp16(hn16[b,:] . fp16(W[c,:]) + fp16(bias[c]))
template <typename E>
__global__ __launch_bounds__(256) void k_fa_head_fwd(const float* __restrict__ x, const float* __restrict__ mean, const float* __restrict__ rstd,
                                                     const float* __restrict__ gamma, const float* __restrict__ beta, const float* __restrict__ W,
                                                     const float* __restrict__ bias, float* __restrict__ hn, E* __restrict__ logits, int D, int T, int C) {
    extern __shared__ float sh[];
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t row = (int64_t)b * T;
    const float mu = mean[row], rs = rstd[row];
    for (int c = threadIdx.x; c < D; c += 256) {
        const float v = Fa<E>::r((x[row * D + c] - mu) * rs * gamma[c] + beta[c]);
        sh[c] = v;
        hn[(int64_t)b * D + c] = v;
    }
    __syncthreads();
    for (int c = wave; c < C; c += 4) {
        float acc = 0.f;
        for (int k = lane; k < D; k += 64) acc += sh[k] * Fa<E>::r(W[(int64_t)c * D + k]);
        acc = wave_sum(acc);
        if (lane == 0) logits[(int64_t)b * C + c] = (E)(acc + Fa<E>::r(bias[c]));
    }
}
// one thread per output element, fixed summation order: dW[c,d] = sum_b dl[b,c] hn16[b,d]; dbias[c] = sum_b dl[b,c];
// dhn[b,d] = fp16(sum_c dl[b,c] fp16(W[c,d]))  (stock: the fp16 Linear's input gradient)
template <typename E>
__global__ __launch_bounds__(256) void k_fa_head_bwd(const E* __restrict__ dl, const float* __restrict__ hn, const float* __restrict__ W,
                                                     float* __restrict__ dW, float* __restrict__ dbias, float* __restrict__ dhn, int B, int D, int C) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    const int64_t nW = (int64_t)C * D, nH = (int64_t)B * D;
    if (i < nW) {
        const int c = (int)(i / D), d = (int)(i % D);
        float a0 = 0.f, a1 = 0.f;
        int b = 0;
        for (; b + 1 < B; b += 2) {
            a0 += (float)dl[(int64_t)b * C + c] * hn[(int64_t)b * D + d];
            a1 += (float)dl[(int64_t)(b + 1) * C + c] * hn[(int64_t)(b + 1) * D + d];
        }
        if (b < B) a0 += (float)dl[(int64_t)b * C + c] * hn[(int64_t)b * D + d];
        dW[i] = a0 + a1;
    } else if (i < nW + nH) {
        const int64_t j = i - nW;
        const int b = (int)(j / D), d = (int)(j % D);
        float a = 0.f;
        for (int c = 0; c < C; ++c) a += (float)dl[(int64_t)b * C + c] * Fa<E>::r(W[(int64_t)c * D + d]);
        dhn[j] = Fa<E>::r(a);
    } else if (i < nW + nH + C) {
        const int c = (int)(i - nW - nH);
        float a = 0.f;
        for (int b = 0; b < B; ++b) a += (float)dl[(int64_t)b * C + c];
        dbias[c] = a;
    }
}

// ---------------------------------------------------------------- elementwise
// G16 = fp16(gelu(Y1))  (the fc2 forward operand and its weight-gradient operand)
template <typename E>
__global__ __launch_bounds__(256) void k_fa_gelu(const float* __restrict__ Y, E* __restrict__ G, int64_t n4) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        const float4 v = reinterpret_cast<const float4*>(Y)[i];
        *reinterpret_cast<uint2*>(G + i * 4) = make_uint2(Fa<E>::pk(gelu_fwd(v.x), gelu_fwd(v.y)), Fa<E>::pk(gelu_fwd(v.z), gelu_fwd(v.w)));
    }
}
// dY1_16 = fp16(fp16(dG) * gelu'(Y1)),  gelu'(x) = Phi(x) + x phi(x)   (not gelu_bwd of qv_common.h: __expf here, expf there)
__device__ inline float gelu_grad(float x) {
    return 0.5f * (1.0f + erff(x * 0.70710678118654752f)) + x * 0.39894228040143268f * __expf(-0.5f * x * x);
}
template <typename E>
__global__ __launch_bounds__(256) void k_fa_gelu_bwd(const float* __restrict__ dG, const float* __restrict__ Y, E* __restrict__ out, int64_t n4) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        const float4 g = reinterpret_cast<const float4*>(dG)[i];
        const float4 y = reinterpret_cast<const float4*>(Y)[i];
        *reinterpret_cast<uint2*>(out + i * 4) = make_uint2(Fa<E>::pk(Fa<E>::r(g.x) * gelu_grad(y.x), Fa<E>::r(g.y) * gelu_grad(y.y)),
                                                            Fa<E>::pk(Fa<E>::r(g.z) * gelu_grad(y.z), Fa<E>::r(g.w) * gelu_grad(y.w)));
    }
}
// embedding backward: dpos[t,:] = sum_b dx[b,t,:], dcls = dpos[0,:] (fp32, fixed order); dY0_16[b*np + t-1, :] = fp16(dx[b,t,:]) for t >= 1
template <typename E>
__global__ __launch_bounds__(64) void k_fa_embed_bwd(const float* __restrict__ dx, float* __restrict__ dpos, float* __restrict__ dcls, E* __restrict__ dY0,
                                                     int B, int T, int D) {
    const int d4 = D / 4;
    const int64_t n4 = (int64_t)T * d4;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        const int t = (int)(i / d4), c = (int)(i % d4) * 4;
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int b = 0; b < B; ++b) {
            const float4 g = *reinterpret_cast<const float4*>(dx + ((int64_t)b * T + t) * D + c);
            acc.x += g.x; acc.y += g.y; acc.z += g.z; acc.w += g.w;
            if (t > 0) *reinterpret_cast<uint2*>(dY0 + ((int64_t)b * (T - 1) + (t - 1)) * D + c) = make_uint2(Fa<E>::pk(g.x, g.y), Fa<E>::pk(g.z, g.w));
        }
        *reinterpret_cast<float4*>(dpos + (int64_t)t * D + c) = acc;
        if (t == 0) *reinterpret_cast<float4*>(dcls + c) = acc;
    }
}
// the overflow rule of the fp16 weight / bias gradients: g -> fp16(g) where that is +-inf (NaN stays NaN); every other value keeps its fp32 sum
constexpr int kFaMaxG = 2 + 8 * 12 + 2;
struct FaInfTab { float* g[kFaMaxG]; int64_t n[kFaMaxG]; int count; };
__global__ __launch_bounds__(256) void k_fa_inf_rule(const FaInfTab t) {
    const int k = blockIdx.y;
    float* g = t.g[k];
    const int64_t n = t.n[k];
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float v = g[i], r = f16r(v);
        if (__builtin_isinf(r)) g[i] = r;
    }
}

// ---------------------------------------------------------------- attention backward on fp16 MFMA, fused: one workgroup per (image, head)
// (E = __bf16: the same in bf16 on v_mfma_f32_16x16x32_bf16)
// With s = head_dim^-0.5 and the forward's lse, per (image, head):
//   P = exp(s Q K^T - lse)    dP = fp16(dO V^T)    dS = fp16(P * (dP - delta)),  delta_i = fp16(dO_i) . O16_i
//   dQ = fp16(s dS K)    dK = fp16(s dS^T Q)    dV = fp16(fp16(P)^T dO)
// The head's Q, K, V and dO (rounded to fp16, as stock holds them) are staged once into LDS as [token][HD + 8] rows, tokens padded to Tp = T rounded
// up to 32 (zero rows; padded queries and keys are masked to P = 0).  P and dS never leave the chip: each wave takes 16-key tiles and sweeps the
// queries in chunks of 32 - S^T and dP^T as v_mfma_f32_16x16x32_f16 tiles (keys on the rows), P and dS rounded to fp16 into a per-wave 16 x 32 LDS
// scratch, read back as the A fragment of dV += P^T dO and dK += dS^T Q - then takes 16-query tiles and recomputes S, dP, dS with the queries on the
// rows for dQ += dS K (the dK / dV sweep cannot hand its dS to dQ without a [T, T] plane).  The B fragments of those three products run over tokens
// at a fixed feature: eight 2-byte LDS reads each.  MFMA 16x16x32 layout: A fragment lane l = row l % 16, k 8 (l / 16) .. + 7; B the same with the
// column; accumulator e of lane l = row 4 (l / 16) + e, column l % 16.
constexpr int kFaWaves = 8, kFaScr = 40;   // scratch row stride in fp16 (32 + 8: 16-B aligned rows)
template <int HD, typename E>
__device__ inline typename Fa<E>::v8 fa_col8(const E* s, int row0, int col) {   // s[(row0 + j) * (HD + 8) + col], j = 0..7
    typename Fa<E>::v8 v;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = s[(row0 + j) * (HD + 8) + col];
    return v;
}
template <int HD, typename E>
__global__ __launch_bounds__(kFaWaves * 64) void k_fa_attn_bwd_fused(const float* __restrict__ qkv, const E* __restrict__ O16, const float* __restrict__ lse,
                                                                    const float* __restrict__ dO, int T, int H, int D, float scale, E* __restrict__ dqkv) {
    typedef typename Fa<E>::v8 v8;
    constexpr int LDH = HD + 8, CH = HD / 8, KK = HD / 32, ND = HD / 16;
    const int Tp = (T + 31) & ~31;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    E* sQ = reinterpret_cast<E*>(smem);
    E* sK = sQ + Tp * LDH;
    E* sV = sK + Tp * LDH;
    E* sD = sV + Tp * LDH;   // dO
    float* sL = reinterpret_cast<float*>(sD + Tp * LDH);
    float* sDel = sL + Tp;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
    E* scrP = reinterpret_cast<E*>(sDel + Tp) + wave * 2 * 16 * kFaScr;
    E* scrS = scrP + 16 * kFaScr;
    const int b = blockIdx.x / H, h = blockIdx.x % H, ld = 3 * D;
    const int64_t row0 = (int64_t)b * T;
    for (int i = threadIdx.x; i < Tp * CH; i += kFaWaves * 64) {   // staging: 8 features of one token per thread
        const int t = i / CH, c = (i % CH) * 8;
        v8 q, k, v, d;
        if (t < T) {
            const float* src = qkv + (row0 + t) * ld + h * HD + c;
            const float* ds = dO + (row0 + t) * D + h * HD + c;
#pragma unroll
            for (int j = 0; j < 8; ++j) { q[j] = (E)src[j]; k[j] = (E)src[D + j]; v[j] = (E)src[2 * D + j]; d[j] = (E)ds[j]; }
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) q[j] = k[j] = v[j] = d[j] = (E)0.f;
        }
        *reinterpret_cast<v8*>(sQ + t * LDH + c) = q;
        *reinterpret_cast<v8*>(sK + t * LDH + c) = k;
        *reinterpret_cast<v8*>(sV + t * LDH + c) = v;
        *reinterpret_cast<v8*>(sD + t * LDH + c) = d;
    }
    for (int t = threadIdx.x; t < Tp; t += kFaWaves * 64) sL[t] = t < T ? lse[((int64_t)b * H + h) * T + t] : 0.f;
    __syncthreads();
    for (int t = threadIdx.x; t < Tp; t += kFaWaves * 64) {   // delta from the staged fp16 dO and the forward's fp16 O (bf16: the same in bf16)
        float a = 0.f;
        if (t < T) {
            const E* o = O16 + (row0 + t) * D + h * HD;
#pragma unroll
            for (int c = 0; c < HD; c += 8) {
                const v8 ov = *reinterpret_cast<const v8*>(o + c);
                const v8 dv = *reinterpret_cast<const v8*>(sD + t * LDH + c);
#pragma unroll
                for (int j = 0; j < 8; ++j) a += (float)dv[j] * (float)ov[j];
            }
        }
        sDel[t] = a;
    }
    __syncthreads();
    const int ntile = Tp / 16;
    // ---- dK, dV: 16 keys per wave tile, the queries in chunks of 32
    for (int kt = wave; kt < ntile; kt += kFaWaves) {
        const int k0 = kt * 16;
        f32x4 dV[ND], dK[ND];
#pragma unroll
        for (int jd = 0; jd < ND; ++jd) dV[jd] = dK[jd] = (f32x4){0.f, 0.f, 0.f, 0.f};
        for (int qc = 0; qc < Tp; qc += 32) {
            f32x4 st[2], dpt[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                st[u] = dpt[u] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int kk = 0; kk < KK; ++kk) {
                    const int c = 32 * kk + 8 * g, qr = qc + 16 * u + r;
                    st[u] = Fa<E>::mfma(*reinterpret_cast<const v8*>(sK + (k0 + r) * LDH + c), *reinterpret_cast<const v8*>(sQ + qr * LDH + c), st[u]);
                    dpt[u] = Fa<E>::mfma(*reinterpret_cast<const v8*>(sV + (k0 + r) * LDH + c), *reinterpret_cast<const v8*>(sD + qr * LDH + c), dpt[u]);
                }
            }
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int q = qc + 16 * u + r;
                const float lq = sL[q], dq = sDel[q];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int key = k0 + 4 * g + e;
                    const float p = (q < T && key < T) ? __expf(scale * st[u][e] - lq) : 0.f;
                    scrP[(4 * g + e) * kFaScr + 16 * u + r] = (E)p;
                    scrS[(4 * g + e) * kFaScr + 16 * u + r] = (E)(p * (Fa<E>::r(dpt[u][e]) - dq));
                }
            }
            wave_lds_fence();
            const v8 ap = *reinterpret_cast<const v8*>(scrP + r * kFaScr + 8 * g);
            const v8 as = *reinterpret_cast<const v8*>(scrS + r * kFaScr + 8 * g);
#pragma unroll
            for (int jd = 0; jd < ND; ++jd) {
                dV[jd] = Fa<E>::mfma(ap, fa_col8<HD>(sD, qc + 8 * g, 16 * jd + r), dV[jd]);
                dK[jd] = Fa<E>::mfma(as, fa_col8<HD>(sQ, qc + 8 * g, 16 * jd + r), dK[jd]);
            }
            wave_lds_fence();
        }
#pragma unroll
        for (int jd = 0; jd < ND; ++jd)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int key = k0 + 4 * g + e;
                if (key < T) {
                    E* o = dqkv + (row0 + key) * ld + h * HD + 16 * jd + r;
                    o[D] = (E)(scale * dK[jd][e]);
                    o[2 * D] = (E)dV[jd][e];
                }
            }
    }
    // ---- dQ: 16 queries per wave tile, S / dP / dS recomputed with the queries on the rows, the keys in chunks of 32
    for (int qt = wave; qt < ntile; qt += kFaWaves) {
        const int q0 = qt * 16;
        f32x4 dQ[ND];
#pragma unroll
        for (int jd = 0; jd < ND; ++jd) dQ[jd] = (f32x4){0.f, 0.f, 0.f, 0.f};
        float lq[4], dq[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) { lq[e] = sL[q0 + 4 * g + e]; dq[e] = sDel[q0 + 4 * g + e]; }
        for (int kc = 0; kc < Tp; kc += 32) {
            f32x4 s[2], dp[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                s[u] = dp[u] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int kk = 0; kk < KK; ++kk) {
                    const int c = 32 * kk + 8 * g, kr = kc + 16 * u + r;
                    s[u] = Fa<E>::mfma(*reinterpret_cast<const v8*>(sQ + (q0 + r) * LDH + c), *reinterpret_cast<const v8*>(sK + kr * LDH + c), s[u]);
                    dp[u] = Fa<E>::mfma(*reinterpret_cast<const v8*>(sD + (q0 + r) * LDH + c), *reinterpret_cast<const v8*>(sV + kr * LDH + c), dp[u]);
                }
            }
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int key = kc + 16 * u + r;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int q = q0 + 4 * g + e;
                    const float p = (q < T && key < T) ? __expf(scale * s[u][e] - lq[e]) : 0.f;
                    scrS[(4 * g + e) * kFaScr + 16 * u + r] = (E)(p * (Fa<E>::r(dp[u][e]) - dq[e]));
                }
            }
            wave_lds_fence();
            const v8 as = *reinterpret_cast<const v8*>(scrS + r * kFaScr + 8 * g);
#pragma unroll
            for (int jd = 0; jd < ND; ++jd)
                dQ[jd] = Fa<E>::mfma(as, fa_col8<HD>(sK, kc + 8 * g, 16 * jd + r), dQ[jd]);
            wave_lds_fence();
        }
#pragma unroll
        for (int jd = 0; jd < ND; ++jd)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int q = q0 + 4 * g + e;
                if (q < T) dqkv[(row0 + q) * ld + h * HD + 16 * jd + r] = (E)(scale * dQ[jd][e]);
            }
    }
}

static size_t fa_attn_lds_bytes(int T, int HD) {
    const size_t Tp = (size_t)((T + 31) & ~31);
    return 4 * Tp * (HD + 8) * 2 + 2 * Tp * 4 + (size_t)kFaWaves * 2 * 16 * kFaScr * 2;
}
template <int HD, typename E>
static void launch_fa_attn_fused(const float* qkv, const void* O16, const float* lse, const float* dO, int B, int T, int H, int D, void* dqkv16, hipStream_t st) {
    static bool once = (allow_lds(k_fa_attn_bwd_fused<HD, E>, fa_attn_lds_bytes(224, HD)), true);
    (void)once;
    k_fa_attn_bwd_fused<HD, E><<<B * H, kFaWaves * 64, fa_attn_lds_bytes(T, HD), st>>>(qkv, reinterpret_cast<const E*>(O16), lse, dO, T, H, D,
                                                                                       1.0f / sqrtf((float)HD), reinterpret_cast<E*>(dqkv16));
}

int launch_attn_bwd_f16(const float* qkv, const void* O16, const float* lse, const float* dO, int B, int T, int H, int D, void* dqkv16, hipStream_t st, bool bf16) {
    const int hd = H > 0 ? D / H : 0;
    if (B < 1 || H < 1 || D % H != 0 || (hd != 64 && hd != 32) || T < 1 || T > 224 || !qkv || !O16 || !lse || !dO || !dqkv16) {
        set_error("attn_bwd_%s: unsupported arguments B=%d T=%d H=%d D=%d (head_dim 32 or 64, T <= 224)", bf16 ? "bf16" : "f16", B, T, H, D);
        return 1;
    }
    if (bf16) {
        if (hd == 64) launch_fa_attn_fused<64, __bf16>(qkv, O16, lse, dO, B, T, H, D, dqkv16, st);
        else launch_fa_attn_fused<32, __bf16>(qkv, O16, lse, dO, B, T, H, D, dqkv16, st);
    } else if (hd == 64) launch_fa_attn_fused<64, _Float16>(qkv, O16, lse, dO, B, T, H, D, dqkv16, st);
    else launch_fa_attn_fused<32, _Float16>(qkv, O16, lse, dO, B, T, H, D, dqkv16, st);
    return 0;
}

// ---------------------------------------------------------------- launchers (the host driver of every form is float_step.hip); bf16: the bf16 form
template <typename E>
static void fa_wcast(int n, const float* const* W, void* const* w16, void* const* w16T, const int* N, const int* K, const int* blk0, hipStream_t st) {
    FaWTab<E> t{};
    t.n = n;
    for (int wi = 0; wi < n; ++wi) {
        t.W[wi] = W[wi];
        t.w[wi] = reinterpret_cast<E*>(w16[wi]);
        t.wT[wi] = reinterpret_cast<E*>(w16T[wi]);
        t.N[wi] = N[wi]; t.K[wi] = K[wi]; t.blk0[wi] = blk0[wi];
    }
    t.blk0[n] = blk0[n];
    k_fa_wcast<E><<<blk0[n], 256, 0, st>>>(t);
}
int launch_fa_wcast(int n, const float* const* W, void* const* w16, void* const* w16T, const int* N, const int* K, const int* blk0, hipStream_t st, bool bf16) {
    if (bf16) fa_wcast<__bf16>(n, W, w16, w16T, N, K, blk0, st);
    else fa_wcast<_Float16>(n, W, w16, w16T, N, K, blk0, st);
    return 0;
}

template <typename E>
static void fa_head_fwd(const float* x, const float* mean, const float* rstd, const float* gamma, const float* beta, const float* W, const float* bias, float* hn,
                        void* logits16, int B, int D, int T, int C, hipStream_t st) {
    k_fa_head_fwd<E><<<B, 256, D * sizeof(float), st>>>(x, mean, rstd, gamma, beta, W, bias, hn, reinterpret_cast<E*>(logits16), D, T, C);
}
int launch_fa_head_fwd(const float* x, const float* mean, const float* rstd, const float* gamma, const float* beta, const float* W, const float* bias, float* hn,
                       void* logits16, int B, int D, int T, int C, hipStream_t st, bool bf16) {
    if (bf16) fa_head_fwd<__bf16>(x, mean, rstd, gamma, beta, W, bias, hn, logits16, B, D, T, C, st);
    else fa_head_fwd<_Float16>(x, mean, rstd, gamma, beta, W, bias, hn, logits16, B, D, T, C, st);
    return 0;
}

int launch_fa_head_bwd(const void* dl16, const float* hn, const float* W, float* dW, float* dbias, float* dhn, int B, int D, int C, hipStream_t st, bool bf16) {
    const int64_t n = (int64_t)C * D + (int64_t)B * D + C;
    if (bf16) k_fa_head_bwd<__bf16><<<(int)((n + 255) / 256), 256, 0, st>>>(reinterpret_cast<const __bf16*>(dl16), hn, W, dW, dbias, dhn, B, D, C);
    else k_fa_head_bwd<_Float16><<<(int)((n + 255) / 256), 256, 0, st>>>(reinterpret_cast<const _Float16*>(dl16), hn, W, dW, dbias, dhn, B, D, C);
    return 0;
}

int launch_fa_gelu(const float* Y, void* G16, int64_t n, hipStream_t st, bool bf16) {
    if (bf16) k_fa_gelu<__bf16><<<flat_grid_fs(n / 4), 256, 0, st>>>(Y, reinterpret_cast<__bf16*>(G16), n / 4);
    else k_fa_gelu<_Float16><<<flat_grid_fs(n / 4), 256, 0, st>>>(Y, reinterpret_cast<_Float16*>(G16), n / 4);
    return 0;
}

int launch_fa_gelu_bwd(const float* dG, const float* Y, void* dY16, int64_t n, hipStream_t st, bool bf16) {
    if (bf16) k_fa_gelu_bwd<__bf16><<<flat_grid_fs(n / 4), 256, 0, st>>>(dG, Y, reinterpret_cast<__bf16*>(dY16), n / 4);
    else k_fa_gelu_bwd<_Float16><<<flat_grid_fs(n / 4), 256, 0, st>>>(dG, Y, reinterpret_cast<_Float16*>(dY16), n / 4);
    return 0;
}

int launch_fa_embed_bwd(const float* dx, float* dpos, float* dcls, void* dY0_16, int B, int T, int D, hipStream_t st, bool bf16) {
    const int grid = (int)(((int64_t)T * (D / 4) + 63) / 64);
    if (bf16) k_fa_embed_bwd<__bf16><<<grid, 64, 0, st>>>(dx, dpos, dcls, reinterpret_cast<__bf16*>(dY0_16), B, T, D);
    else k_fa_embed_bwd<_Float16><<<grid, 64, 0, st>>>(dx, dpos, dcls, reinterpret_cast<_Float16*>(dY0_16), B, T, D);
    return 0;
}

int launch_fa_inf_rule(float* const* g, const int64_t* n, int count, hipStream_t st) {
    FaInfTab t{};
    for (int k = 0; k < count; ++k) { t.g[k] = g[k]; t.n[k] = n[k]; }
    t.count = count;
    k_fa_inf_rule<<<dim3(64, count), 256, 0, st>>>(t);
    return 0;
}

}  // namespace qv

using namespace qv;

extern "C" {

int qatvit_float_student_amp_attn_backward(const float* qkv, const void* O16, const float* lse, const float* dO, int32_t B, int32_t T, int32_t H, int32_t D,
                                           void* dqkv16, void* stream) {
    if (launch_attn_bwd_f16(qkv, O16, lse, dO, B, T, H, D, dqkv16, (hipStream_t)stream)) return 1;
    QV_CHECK_LAUNCH("qatvit_float_student_amp_attn_backward");
    return 0;
}

int qatvit_float_student_bf16_attn_backward(const float* qkv, const void* O16, const float* lse, const float* dO, int32_t B, int32_t T, int32_t H, int32_t D,
                                            void* dqkv16, void* stream) {
    if (launch_attn_bwd_f16(qkv, O16, lse, dO, B, T, H, D, dqkv16, (hipStream_t)stream, true)) return 1;
    QV_CHECK_LAUNCH("qatvit_float_student_bf16_attn_backward");
    return 0;
}

}  // extern "C"
