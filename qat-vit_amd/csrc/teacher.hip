// Frozen KD teacher forward (ViT-B/16, no fake-quant, no gradient), native on gfx950.
//
// Replaces: `with torch.no_grad(): teacher_out = teacher(images)` (/root/reference/src/training/qat_trainer.py:337-338;
// teacher built at model_registry.py:152-175).  The reference runs it in fp32; here every GEMM operand is a float
// tensor, so BOTH sides are hi+lo bf16 pairs and each product takes three MFMA passes (hi.hi + lo.hi + hi.lo,
// 2^-16 relative), fp32 accumulate.  Weights are frozen: their (hi, lo) pairs are prepared once by the host.
// Activations are produced directly as pairs by the fused row kernels below, so the whole forward is
//   patches -> [GEMM] -> (+cls,+pos, LN) -> 12 x { [GEMM qkv] -> attention -> [GEMM proj] -> (+res, LN) -> [GEMM fc1]
//   -> GELU -> [GEMM fc2] -> (+res, LN) } -> cls LN -> head
// with no stand-alone elementwise pass besides GELU.
#include "../../include/qatvit.h"
#include <stdlib.h>

#include "qv_common.h"
#include "qv_device.h"
#include "qv_kernels.h"

namespace qv {

// (hi, lo) pair of four values: bf16 (8 + 8 significant bits) or, f16 != 0 (uniform), fp16 (11 + 11; unscaled: the teacher's GEMM inputs - LayerNorm
// outputs, attention outputs, GELU outputs, image patches - are far inside fp16's range).  lo == nullptr: the one-pass form keeps the hi part only.
// BF1: the bf16 one-plane form (the float step's bf16 form; f16 == 0, lo unused): bf16(v) only.
template <bool BF1 = false>
__device__ inline void st_split4(__bf16* hi, __bf16* lo, int64_t off, float a, float b, float c, float d, int f16 = 0) {
    if (f16) {
        f16x4 h, l;
        h[0] = (_Float16)a; h[1] = (_Float16)b; h[2] = (_Float16)c; h[3] = (_Float16)d;
        *reinterpret_cast<f16x4*>(hi + off) = h;
        if (lo) {
            l[0] = (_Float16)(a - (float)h[0]); l[1] = (_Float16)(b - (float)h[1]); l[2] = (_Float16)(c - (float)h[2]); l[3] = (_Float16)(d - (float)h[3]);
            *reinterpret_cast<f16x4*>(lo + off) = l;
        }
        return;
    }
    bf16x4 h, l;
    h[0] = (__bf16)a; h[1] = (__bf16)b; h[2] = (__bf16)c; h[3] = (__bf16)d;
    if constexpr (BF1) {
        *reinterpret_cast<bf16x4*>(hi + off) = h;
        return;
    }
    l[0] = (__bf16)(a - (float)h[0]); l[1] = (__bf16)(b - (float)h[1]); l[2] = (__bf16)(c - (float)h[2]); l[3] = (__bf16)(d - (float)h[3]);
    *reinterpret_cast<bf16x4*>(hi + off) = h;
    *reinterpret_cast<bf16x4*>(lo + off) = l;
}

// image [B,C,H,W] fp32 -> patch rows [B*np, C*P*P] as a (hi, lo) pair
template <bool BF1 = false>
__global__ __launch_bounds__(256) void k_patches_split(const float* __restrict__ img, __bf16* __restrict__ hi, __bf16* __restrict__ lo, int B, int C,
                                                       int H, int W, int P, int f16) {
    const int gw = W / P, gh = H / P, K = C * P * P;
    const int64_t n4 = (int64_t)B * gh * gw * K / 4;
    for (int64_t e4 = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e4 < n4; e4 += (int64_t)gridDim.x * blockDim.x) {
        const int64_t e = e4 * 4;
        const int col = (int)(e % K);
        const int64_t prow = e / K;
        const int px = (int)(prow % gw), py = (int)((prow / gw) % gh), b = (int)(prow / ((int64_t)gw * gh));
        const int j = col % P, i = (col / P) % P, c = col / (P * P);
        const float4 v = *reinterpret_cast<const float4*>(img + (((int64_t)b * C + c) * H + py * P + i) * W + px * P + j);
        st_split4<BF1>(hi, lo, e, v.x, v.y, v.z, v.w, f16);
    }
}

// v rounded to the type a 16-bit form holds it in (kind 1: fp16, 2: bf16; 0: fp32, unchanged), as an fp32 value
__device__ inline float round_as(float v, int kind) { return kind == 1 ? (float)(_Float16)v : kind == 2 ? (float)(__bf16)v : v; }

#define QV_DP 0
#include "teacher_rows.inc"
#undef QV_DP
template <int MODE, bool STATS = false, bool BF1 = false, typename... A>
static void launch_resid_ln_split(int grid, hipStream_t st, int D, A... a) {
    const int nv = (D + 255) / 256;
    if (nv == 1) k_resid_ln_split<MODE, 1, STATS, BF1><<<grid, 256, 0, st>>>(a...);
    else if (nv == 2) k_resid_ln_split<MODE, 2, STATS, BF1><<<grid, 256, 0, st>>>(a...);
    else k_resid_ln_split<MODE, 3, STATS, BF1><<<grid, 256, 0, st>>>(a...);
}

__global__ __launch_bounds__(256) void k_gelu_split(const float* __restrict__ Y, __bf16* __restrict__ hi, __bf16* __restrict__ lo, int64_t n4) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        const float4 v = reinterpret_cast<const float4*>(Y)[i];
        st_split4(hi, lo, i * 4, gelu_fwd(v.x), gelu_fwd(v.y), gelu_fwd(v.z), gelu_fwd(v.w));
    }
}

// final norm on the cls rows + head: logits[b,c] = LN(x[b,0,:]) . W[c,:] + bias[c]   (fp32; B x C x D is tiny)
__global__ __launch_bounds__(256) void k_teacher_head(const float* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                      float eps, const float* __restrict__ W, const float* __restrict__ bias,
                                                      float* __restrict__ logits, int D, int T, int C) {
    extern __shared__ float sh[];  // D floats + 8
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float* xr = x + (int64_t)b * T * D;
    float s = 0.f;
    for (int c = threadIdx.x; c < D; c += 256) s += xr[c];
    s = wave_sum(s);
    float* red = sh + D;
    if (lane == 0) red[wave] = s;
    __syncthreads();
    const float mu = (red[0] + red[1] + red[2] + red[3]) / (float)D;
    __syncthreads();
    float q = 0.f;
    for (int c = threadIdx.x; c < D; c += 256) { const float d = xr[c] - mu; q += d * d; }
    q = wave_sum(q);
    if (lane == 0) red[wave] = q;
    __syncthreads();
    const float rs = rsqrtf((red[0] + red[1] + red[2] + red[3]) / (float)D + eps);
    for (int c = threadIdx.x; c < D; c += 256) sh[c] = (xr[c] - mu) * rs * gamma[c] + beta[c];
    __syncthreads();
    for (int c = wave; c < C; c += 4) {
        float acc = 0.f;
        for (int k = lane; k < D; k += 64) acc += sh[k] * W[(int64_t)c * D + k];
        acc = wave_sum(acc);
        if (lane == 0) logits[(int64_t)b * C + c] = acc + bias[c];
    }
}

// ---------------------------------------------------------------- float attention (no quantisation): 3-pass products
// (K as a row_off image, V as a tr_off image read with tr_frag2, the output re-tiled with wave_retile8: qv_device.h)
// (per-element casts; attn.hip's load_split8 forms the same bits through split_pair, with other instructions)
__device__ inline void t_load_split8(const float* p, bf16x8& hi, bf16x8& lo) {
    const float4 a = reinterpret_cast<const float4*>(p)[0], b = reinterpret_cast<const float4*>(p)[1];
    const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
    for (int j = 0; j < 8; ++j) { hi[j] = (__bf16)v[j]; lo[j] = (__bf16)(v[j] - (float)hi[j]); }
}

constexpr int kTW = 8;  // waves per workgroup
template <int HD, int NKT, bool BF1 = false>   // BF1: O as ONE bf16 plane (the float step's bf16 form)
__global__ __launch_bounds__(kTW * 64) void k_attn_fwd_float(const float* __restrict__ qkv, int B, int T, int H, int D, float scale,
                                                             __bf16* __restrict__ O_hi, __bf16* __restrict__ O_lo, int f16,
                                                             float* __restrict__ lse = nullptr) {
    constexpr int IMG = NKT * 16 * HD * 2, CH = HD / 8, KK = HD / 32, ND = HD / 16;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* sKh = smem;            // row images of K (hi, lo)
    char* sKl = smem + IMG;
    char* sVh = smem + 2 * IMG;  // tr images of V (hi, lo)
    char* sVl = smem + 3 * IMG;
    float* sO = reinterpret_cast<float*>(smem + 4 * IMG) + (threadIdx.x >> 6) * (8 * (HD + 4));   // per-wave output re-tiling scratch
    const int b = blockIdx.x / H, h = blockIdx.x % H, ld = 3 * D;
    const float* base = qkv + (int64_t)b * T * ld + h * HD;
    {   // staging: every load of the K and V slices first (branch-free: a padded token reads the last real one and is zeroed below),
        // pinned, then the splits and LDS stores - the rolled load -> split -> store loop was four dependent memory round trips
        constexpr int TOTAL = NKT * 16 * CH, ITERS = (TOTAL + kTW * 64 - 1) / (kTW * 64);
        float4 ka[ITERS], kb[ITERS], va[ITERS], vb[ITERS];
#pragma unroll
        for (int it = 0; it < ITERS; ++it) {
            const int i = threadIdx.x + it * kTW * 64, tok = min(i / CH, T - 1), ch = i % CH;
            const float4* pk = reinterpret_cast<const float4*>(base + D + (int64_t)tok * ld + ch * 8);
            const float4* pv = reinterpret_cast<const float4*>(base + 2 * D + (int64_t)tok * ld + ch * 8);
            ka[it] = pk[0]; kb[it] = pk[1]; va[it] = pv[0]; vb[it] = pv[1];
        }
#pragma unroll
        for (int it = 0; it < ITERS; ++it) { pin4(ka[it]); pin4(kb[it]); pin4(va[it]); pin4(vb[it]); }
#pragma unroll
        for (int it = 0; it < ITERS; ++it) {
            const int i = threadIdx.x + it * kTW * 64, tok = i / CH, ch = i % CH;
            if (i < TOTAL) {
                const bool real = tok < T;
                const float kv[8] = {ka[it].x, ka[it].y, ka[it].z, ka[it].w, kb[it].x, kb[it].y, kb[it].z, kb[it].w};
                const float vv[8] = {va[it].x, va[it].y, va[it].z, va[it].w, vb[it].x, vb[it].y, vb[it].z, vb[it].w};
                bf16x8 kh, kl, vh, vl;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float k1 = real ? kv[j] : 0.f, v1 = real ? vv[j] : 0.f;
                    kh[j] = (__bf16)k1; kl[j] = (__bf16)(k1 - (float)kh[j]);
                    vh[j] = (__bf16)v1; vl[j] = (__bf16)(v1 - (float)vh[j]);
                }
                *reinterpret_cast<bf16x8*>(sKh + row_off<HD>(tok, ch)) = kh;
                *reinterpret_cast<bf16x8*>(sKl + row_off<HD>(tok, ch)) = kl;
                *reinterpret_cast<bf16x8*>(sVh + tr_off<HD>(tok, ch)) = vh;
                *reinterpret_cast<bf16x8*>(sVl + tr_off<HD>(tok, ch)) = vl;
            }
        }
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
    const int nqt = (T + 15) / 16;
    for (int qt = wave; qt < nqt; qt += kTW) {
        const int qrow = min(qt * 16 + r, T - 1);
        bf16x8 qh[KK], ql[KK];
#pragma unroll
        for (int kk = 0; kk < KK; ++kk) t_load_split8(base + (int64_t)qrow * ld + 32 * kk + 8 * g, qh[kk], ql[kk]);
        f32x4 s[NKT];
#pragma unroll
        for (int j = 0; j < NKT; ++j) {
            s[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kk = 0; kk < KK; ++kk) {
                const bf16x8 kh = *reinterpret_cast<const bf16x8*>(sKh + row_off<HD>(16 * j + r, 4 * kk + g));
                const bf16x8 kl = *reinterpret_cast<const bf16x8*>(sKl + row_off<HD>(16 * j + r, 4 * kk + g));
                s[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kh, qh[kk], s[j], 0, 0, 0);
                s[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kl, qh[kk], s[j], 0, 0, 0);
                s[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kh, ql[kk], s[j], 0, 0, 0);
            }
        }
        float m = -INFINITY;
#pragma unroll
        for (int j = 0; j < NKT; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                s[j][e] = (16 * j + 4 * g + e < T) ? s[j][e] * scale : -INFINITY;
                m = fmaxf(m, s[j][e]);
            }
        m = fmaxf(m, __shfl_xor(m, 16, 64));
        m = fmaxf(m, __shfl_xor(m, 32, 64));
        float l = 0.f;
#pragma unroll
        for (int j = 0; j < NKT; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) { s[j][e] = fast_exp(s[j][e] - m); l += s[j][e]; }
        l += __shfl_xor(l, 16, 64);
        l += __shfl_xor(l, 32, 64);
        const float invl = 1.0f / l;
        // log-sum-exp of the scaled scores per query, [b][h][t] (the float student step's attention backward; the teacher passes nullptr)
        if (lse && g == 0 && qt * 16 + r < T) lse[((int64_t)b * H + h) * T + qt * 16 + r] = m + logf(l);
        f32x4 o[ND];
#pragma unroll
        for (int jd = 0; jd < ND; ++jd) o[jd] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < NKT / 2; ++ks) {
            bf16x8 ph, pl;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float a = s[2 * ks][j] * invl, bb = s[2 * ks + 1][j] * invl;
                ph[j] = (__bf16)a; pl[j] = (__bf16)(a - (float)ph[j]);
                ph[j + 4] = (__bf16)bb; pl[j + 4] = (__bf16)(bb - (float)ph[j + 4]);
            }
#pragma unroll
            for (int jd = 0; jd < ND; ++jd) {
                const bf16x8 vh = tr_frag2<HD>(sVh, 32 * ks, 32 * ks + 16, 16 * jd, lane);
                const bf16x8 vl = tr_frag2<HD>(sVl, 32 * ks, 32 * ks + 16, 16 * jd, lane);
                o[jd] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ph, vh, o[jd], 0, 0, 0);
                o[jd] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pl, vh, o[jd], 0, 0, 0);
                o[jd] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ph, vl, o[jd], 0, 0, 0);
            }
        }
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            float ov[8];
            int orow, oc;
            const bool act = wave_retile8<HD>(sO, o, 1.0f, lane, half, ov, orow, oc);
            const int qq = qt * 16 + 8 * half + orow;
            if (act && qq < T) {
                const int64_t off = ((int64_t)b * T + qq) * D + h * HD + 8 * oc;
                if (f16) {   // (uniform) the output pair in fp16 for the fp16 proj GEMM; the one-pass form keeps the hi part only
                    f16x8 hv, lv;
#pragma unroll
                    for (int j = 0; j < 8; ++j) { hv[j] = (_Float16)ov[j]; lv[j] = (_Float16)(ov[j] - (float)hv[j]); }
                    *reinterpret_cast<f16x8*>(O_hi + off) = hv;
                    if (O_lo) *reinterpret_cast<f16x8*>(O_lo + off) = lv;
                } else {
                    bf16x8 hv, lv;
#pragma unroll
                    for (int j = 0; j < 8; ++j) { hv[j] = (__bf16)ov[j]; lv[j] = (__bf16)(ov[j] - (float)hv[j]); }
                    *reinterpret_cast<bf16x8*>(O_hi + off) = hv;
                    if constexpr (!BF1) *reinterpret_cast<bf16x8*>(O_lo + off) = lv;
                }
            }
        }
    }
}

static int flat_grid_t(int64_t n) {
    int64_t b = (n + 255) / 256;
    return (int)(b < 1 ? 1 : (b > 4096 ? 4096 : b));
}
static int rows_grid_t(int64_t rows) {
    int64_t b = (rows + 3) / 4;
    return (int)(b < 1 ? 1 : (b > 2048 ? 2048 : b));
}

template <int HD, int NKT, bool BF1>
static void launch_attn_float_k(const float* qkv, int B, int T, int H, int D, void* O_hi, void* O_lo, hipStream_t st, int f16, float* lse) {
    const size_t lds = (size_t)4 * NKT * 16 * HD * 2 + (size_t)kTW * 8 * (HD + 4) * sizeof(float);
    static bool once = (allow_lds(k_attn_fwd_float<HD, NKT, BF1>, lds), true);
    (void)once;
    k_attn_fwd_float<HD, NKT, BF1><<<B * H, kTW * 64, lds, st>>>(qkv, B, T, H, D, 1.0f / sqrtf((float)HD), reinterpret_cast<__bf16*>(O_hi),
                                                                 reinterpret_cast<__bf16*>(O_lo), f16, lse);
}
template <int HD, int NKT>
static void launch_attn_float(const float* qkv, int B, int T, int H, int D, void* O_hi, void* O_lo, hipStream_t st, int f16, float* lse) {
    if (!f16 && !O_lo) launch_attn_float_k<HD, NKT, true>(qkv, B, T, H, D, O_hi, O_lo, st, f16, lse);   // one bf16 plane
    else launch_attn_float_k<HD, NKT, false>(qkv, B, T, H, D, O_hi, O_lo, st, f16, lse);
}

int launch_attn_fwd_float(const float* qkv, int B, int T, int H, int D, void* O_hi, void* O_lo, hipStream_t st, int f16, float* lse) {
    const int hd = D / H;
    if (D % H != 0 || (hd != 64 && hd != 32) || T > 224) { set_error("teacher attention: head_dim %d / T %d unsupported", hd, T); return 1; }
    if (hd == 64 && T > 32) launch_attn_float<64, 14>(qkv, B, T, H, D, O_hi, O_lo, st, f16, lse);
    else if (hd == 64) launch_attn_float<64, 2>(qkv, B, T, H, D, O_hi, O_lo, st, f16, lse);
    else if (T > 32) launch_attn_float<32, 14>(qkv, B, T, H, D, O_hi, O_lo, st, f16, lse);
    else launch_attn_float<32, 2>(qkv, B, T, H, D, O_hi, O_lo, st, f16, lse);
    return 0;
}

// the forward pieces the float student step (float_step.hip) shares: the bf16-pair form, or (f16, float_amp.hip) one fp16 plane, or (neither f16
// nor a lo plane) one bf16 plane
int launch_patches_split(const float* img, void* hi, void* lo, int B, int C, int H, int W, int P, hipStream_t st, int f16) {
    const int64_t n = (int64_t)B * (H / P) * (W / P) * C * P * P;
    if (!f16 && !lo) k_patches_split<true><<<flat_grid_t(n / 4), 256, 0, st>>>(img, reinterpret_cast<__bf16*>(hi), nullptr, B, C, H, W, P, 0);
    else k_patches_split<<<flat_grid_t(n / 4), 256, 0, st>>>(img, reinterpret_cast<__bf16*>(hi), reinterpret_cast<__bf16*>(lo), B, C, H, W, P, f16);
    return 0;
}
// mode 1 under drop-path (teacher_rows.inc): defined at the end of this namespace, behind the second inclusion - k_resid_ln_split_dp is instantiated after every
// other kernel of the file, which keeps those where they stood in the object
static int resid_ln_split_dp(const float* x_prev, const float* Y, float* x_new, const float* gamma, const float* beta, float eps, __bf16* hh, __bf16* hl, float* mean,
                             float* rstd, int64_t M, int D, int T, hipStream_t st, uint32_t* stats, int f16, const float* dps);
static int resid_ln_split_ls(const float* x_prev, const float* Y, float* x_new, const float* gamma, const float* beta, float eps, __bf16* hh, __bf16* hl, float* mean,
                             float* rstd, int64_t M, int D, int T, hipStream_t st, uint32_t* stats, int f16, const float* dps, const float* lsg);
int launch_resid_ln_split_save(int mode, const float* x_prev, const float* Y, const float* cls, const float* pos, float* x_new, const float* gamma,
                               const float* beta, float eps, void* h_hi, void* h_lo, float* mean, float* rstd, int64_t M, int D, int T, hipStream_t st,
                               uint32_t* stats, int f16, const float* drop_scale_rows, const float* ls_gamma) {
    __bf16* hh = reinterpret_cast<__bf16*>(h_hi);
    __bf16* hl = reinterpret_cast<__bf16*>(h_lo);
    if (ls_gamma) {
        if (mode != 1) { set_error("resid_ln_split: LayerScale belongs to a residual branch (mode 1)"); return 1; }
        return resid_ln_split_ls(x_prev, Y, x_new, gamma, beta, eps, hh, hl, mean, rstd, M, D, T, st, stats, f16, drop_scale_rows, ls_gamma);
    }
    if (drop_scale_rows) {
        if (mode != 1) { set_error("resid_ln_split: drop-path multipliers belong to a residual branch (mode 1)"); return 1; }
        return resid_ln_split_dp(x_prev, Y, x_new, gamma, beta, eps, hh, hl, mean, rstd, M, D, T, st, stats, f16, drop_scale_rows);
    }
    if (stats) {
        if (mode == 0) launch_resid_ln_split<0, true>(rows_grid_t(M), st, D, x_prev, Y, cls, pos, x_new, gamma, beta, eps, hh, hl, M, D, T, 0, mean, rstd, stats);
        else launch_resid_ln_split<1, true>(rows_grid_t(M), st, D, x_prev, Y, cls, pos, x_new, gamma, beta, eps, hh, hl, M, D, T, 0, mean, rstd, stats);
        return 0;
    }
    if (!f16 && !hl) {   // one bf16 plane
        if (mode == 0) launch_resid_ln_split<0, false, true>(rows_grid_t(M), st, D, x_prev, Y, cls, pos, x_new, gamma, beta, eps, hh, hl, M, D, T, 0, mean, rstd);
        else launch_resid_ln_split<1, false, true>(rows_grid_t(M), st, D, x_prev, Y, cls, pos, x_new, gamma, beta, eps, hh, hl, M, D, T, 0, mean, rstd);
        return 0;
    }
    if (mode == 0) launch_resid_ln_split<0>(rows_grid_t(M), st, D, x_prev, Y, cls, pos, x_new, gamma, beta, eps, hh, hl, M, D, T, f16, mean, rstd);
    else launch_resid_ln_split<1>(rows_grid_t(M), st, D, x_prev, Y, cls, pos, x_new, gamma, beta, eps, hh, hl, M, D, T, f16, mean, rstd);
    return 0;
}
int launch_gelu_split(const float* Y, void* hi, void* lo, int64_t n, hipStream_t st) {
    k_gelu_split<<<flat_grid_t(n / 4), 256, 0, st>>>(Y, reinterpret_cast<__bf16*>(hi), reinterpret_cast<__bf16*>(lo), n / 4);
    return 0;
}

// ---------------------------------------------------------------- the residual + LayerNorm row kernel under drop-path (k_resid_ln_split_dp) and its launch
#define QV_DP 1
#include "teacher_rows.inc"
#undef QV_DP
// (the output forms of launch_resid_ln_split_save: the pair with the observe-only statistics, one bf16 plane, the pair or one fp16 plane)
static int resid_ln_split_dp(const float* x_prev, const float* Y, float* x_new, const float* gamma, const float* beta, float eps, __bf16* hh, __bf16* hl, float* mean,
                             float* rstd, int64_t M, int D, int T, hipStream_t st, uint32_t* stats, int f16, const float* dps) {
    const int grid = rows_grid_t(M), nv = (D + 255) / 256;
    const float* const none = nullptr;
#define QV_RESID_DP(NV_)                                                                                                                                    \
    do {                                                                                                                                                    \
        if (stats) k_resid_ln_split_dp<1, NV_, true><<<grid, 256, 0, st>>>(x_prev, Y, none, none, x_new, gamma, beta, eps, hh, hl, M, D, T, 0, mean, rstd, stats, dps); \
        else if (!f16 && !hl) k_resid_ln_split_dp<1, NV_, false, true><<<grid, 256, 0, st>>>(x_prev, Y, none, none, x_new, gamma, beta, eps, hh, hl, M, D, T, 0, mean, rstd, nullptr, dps); \
        else k_resid_ln_split_dp<1, NV_><<<grid, 256, 0, st>>>(x_prev, Y, none, none, x_new, gamma, beta, eps, hh, hl, M, D, T, f16, mean, rstd, nullptr, dps); \
    } while (0)
    if (nv == 1) QV_RESID_DP(1); else if (nv == 2) QV_RESID_DP(2); else QV_RESID_DP(3);
#undef QV_RESID_DP
    return 0;
}

// ---------------------------------------------------------------- ... and under LayerScale (k_resid_ln_split_ls), with or without drop-path
#define QV_DP 2
#include "teacher_rows.inc"
#undef QV_DP
static int resid_ln_split_ls(const float* x_prev, const float* Y, float* x_new, const float* gamma, const float* beta, float eps, __bf16* hh, __bf16* hl, float* mean,
                             float* rstd, int64_t M, int D, int T, hipStream_t st, uint32_t* stats, int f16, const float* dps, const float* lsg) {
    const int grid = rows_grid_t(M), nv = (D + 255) / 256;
    const float* const none = nullptr;
#define QV_RESID_LS(NV_)                                                                                                                                    \
    do {                                                                                                                                                    \
        if (stats) k_resid_ln_split_ls<1, NV_, true><<<grid, 256, 0, st>>>(x_prev, Y, none, none, x_new, gamma, beta, eps, hh, hl, M, D, T, 0, mean, rstd, stats, dps, lsg); \
        else if (!f16 && !hl) k_resid_ln_split_ls<1, NV_, false, true><<<grid, 256, 0, st>>>(x_prev, Y, none, none, x_new, gamma, beta, eps, hh, hl, M, D, T, 0, mean, rstd, nullptr, dps, lsg); \
        else k_resid_ln_split_ls<1, NV_><<<grid, 256, 0, st>>>(x_prev, Y, none, none, x_new, gamma, beta, eps, hh, hl, M, D, T, f16, mean, rstd, nullptr, dps, lsg); \
    } while (0)
    if (nv == 1) QV_RESID_LS(1); else if (nv == 2) QV_RESID_LS(2); else QV_RESID_LS(3);
#undef QV_RESID_LS
    return 0;
}

}  // namespace qv

using namespace qv;

extern "C" {

// workspace: x (2 x M*D fp32), h pair (2 x M*D bf16), qkv (M*3D fp32), O pair, Y (M*D fp32), Y1 (M*Hd fp32), G pair (2 x M*Hd bf16),
// patches pair (2 x B*np*Kpe bf16), Y0 (B*np*D fp32)
struct TPlan { int64_t xA, xB, h_hi, h_lo, qkv, O_hi, O_lo, Y, Y1, G_hi, G_lo, p_hi, p_lo, Y0, total; };
static TPlan tplan(const qatvit_cfg& c) {
    TPlan p;
    int64_t o = 0;
    auto take = [&](int64_t b) { int64_t r = o; o += (b + 255) & ~(int64_t)255; return r; };
    const int64_t np = (int64_t)(c.img_size / c.patch_size) * (c.img_size / c.patch_size), M = (int64_t)c.batch * (np + 1), D = c.embed_dim,
                  Hd = c.mlp_hidden, Kpe = (int64_t)c.in_chans * c.patch_size * c.patch_size;
    p.xA = take(M * D * 4); p.xB = take(M * D * 4);
    p.h_hi = take(M * D * 2); p.h_lo = take(M * D * 2);
    p.qkv = take(M * 3 * D * 4);
    p.O_hi = take(M * D * 2); p.O_lo = take(M * D * 2);
    p.Y = take(M * D * 4);
    p.Y1 = take(M * Hd * 4);
    p.G_hi = take(M * Hd * 2); p.G_lo = take(M * Hd * 2);
    p.p_hi = take(c.batch * np * Kpe * 2); p.p_lo = take(c.batch * np * Kpe * 2);
    p.Y0 = take(c.batch * np * D * 4);
    p.total = o;
    return p;
}
static int tcheck(const qatvit_cfg& c) {
    if (c.batch < 1 || c.depth < 1 || c.embed_dim % 128 != 0 || c.mlp_hidden % 128 != 0 || c.embed_dim % c.num_heads != 0 || c.embed_dim > 768 ||
        c.img_size % c.patch_size != 0 || (c.in_chans * c.patch_size * c.patch_size) % 128 != 0 || c.patch_size % 4 != 0) {
        set_error("teacher: unsupported config (dim %d hidden %d heads %d img %d patch %d)", c.embed_dim, c.mlp_hidden, c.num_heads, c.img_size,
                  c.patch_size);
        return 1;
    }
    return 0;
}

int64_t qatvit_teacher_workspace_bytes(const qatvit_cfg* cfg) {
    if (!cfg || tcheck(*cfg)) return -1;
    return tplan(*cfg).total;
}

// params: fp32 tensors in the student's order (include/qatvit.h).
// passes == 3: w_hi / w_lo = the bf16 (hi, lo) pairs of the 2-D weights in the weight_fq order (patch_embed.proj, per block qkv, proj, fc1, fc2; the head
//   stays fp32); activations as bf16 pairs; three MFMA passes per GEMM (a_hi w_hi + a_lo w_hi + a_hi w_lo): logits within 1e-5 of fp64.
// passes == 2 / 1: w_hi = the weights as fp16 (11 significant bits), w_lo unused; activations as an fp16 (hi, lo) pair (two passes, v_mfma_f32_16x16x32_f16)
//   or as fp16 alone (one pass).  Measured against fp64 (tools/teacher_precision.py): profiles/round3_teacher_precision.txt.
static int teacher_forward_impl(const qatvit_cfg* cfg, void* const* params, void* const* w_hi, void* const* w_lo, int passes, const float* images,
                                float* logits, void* workspace, void* stream, const char* who) {
    QV_CHECK_ARG(cfg && params && w_hi && images && logits && workspace && (passes != 3 || w_lo), "%s: null argument", who);
    QV_CHECK_ARG(passes >= 1 && passes <= 3, "%s: passes %d (1, 2 or 3)", who, passes);
    if (tcheck(*cfg)) return 1;
    const qatvit_cfg& c = *cfg;
    const TPlan p = tplan(c);
    char* ws = reinterpret_cast<char*>(workspace);
    hipStream_t st = (hipStream_t)stream;
    const int np = (c.img_size / c.patch_size) * (c.img_size / c.patch_size), T = np + 1, D = c.embed_dim, Hd = c.mlp_hidden;
    const int Kpe = c.in_chans * c.patch_size * c.patch_size;
    const int64_t M = (int64_t)c.batch * T;
    const int f16 = passes < 3;
    QV_CHECK_ARG(!f16 || (D % 384 == 0 && Hd % 384 == 0 && Kpe % 32 == 0), "%s: the fp16 forms need embed_dim and mlp_hidden multiples of 384", who);
    auto F = [&](int64_t off) { return reinterpret_cast<float*>(ws + off); };
    auto V = [&](int64_t off) { return reinterpret_cast<void*>(ws + off); };
    auto H16 = [&](int64_t off) { return reinterpret_cast<__bf16*>(ws + off); };
    auto LO = [&](int64_t off) { return passes == 1 ? (__bf16*)nullptr : H16(off); };   // the one-pass form has no lo planes
    auto prm = [&](int i) { return reinterpret_cast<const float*>(params[i]); };
    auto bprm = [&](int blk, int k) { return prm(4 + 12 * blk + k); };
    auto gemm = [&](const void* Ah, const void* Al, int wi, const float* bias, float* C, int Mrows, int N, int K, const NTPost* post = nullptr) {
        NTGemm g;
        g.A = Ah; g.B = w_hi[wi]; g.C = C; g.M = Mrows; g.N = N; g.K = g.lda = g.ldb = K; g.ldc = N; g.bias = bias;
        if (passes > 1) g.A_lo = Al;
        if (!f16) g.B_lo = w_lo[wi];
        return launch_gemm_nt(f16 ? kNTF16 : kNTBf16, g, post, st);
    };
    k_patches_split<<<flat_grid_t((int64_t)c.batch * np * Kpe / 4), 256, 0, st>>>(images, H16(p.p_hi), LO(p.p_lo), c.batch, c.in_chans, c.img_size,
                                                                               c.img_size, c.patch_size, f16);
    if (gemm(V(p.p_hi), V(p.p_lo), 0, prm(1), F(p.Y0), c.batch * np, D, Kpe)) return 1;
    float* x = F(p.xA);
    float* x2 = F(p.xB);
    launch_resid_ln_split<0>(rows_grid_t(M), st, D, (const float*)nullptr, F(p.Y0), prm(2), prm(3), x, bprm(0, 0), bprm(0, 1), c.ln_eps, H16(p.h_hi),
                                                        LO(p.h_lo), M, D, T, f16);
    for (int i = 0; i < c.depth; ++i) {
        const int w0 = 1 + 4 * i;
        if (gemm(V(p.h_hi), V(p.h_lo), w0 + 0, bprm(i, 3), F(p.qkv), (int)M, 3 * D, D)) return 1;
        if (launch_attn_fwd_float(F(p.qkv), c.batch, T, c.num_heads, D, V(p.O_hi), passes == 1 ? nullptr : V(p.O_lo), st, f16)) return 1;
        if (gemm(V(p.O_hi), V(p.O_lo), w0 + 1, bprm(i, 5), F(p.Y), (int)M, D, D)) return 1;
        launch_resid_ln_split<1>(rows_grid_t(M), st, D, (const float*)x, (const float*)F(p.Y), (const float*)nullptr, (const float*)nullptr, x2, bprm(i, 6), bprm(i, 7), c.ln_eps, H16(p.h_hi),
                                                            LO(p.h_lo), M, D, T, f16);
        {   // fc1 with GELU + hi/lo split in the GEMM epilogue (the fp32 [M, Hd] tensor never exists)
            NTPost post{};
            post.mode = kEpiGeluFwd; post.out_hi = V(p.G_hi); post.out_lo = passes == 1 ? nullptr : V(p.G_lo); post.out_f16 = f16;
            if (gemm(V(p.h_hi), V(p.h_lo), w0 + 2, bprm(i, 9), nullptr, (int)M, Hd, D, &post)) return 1;
        }
        if (gemm(V(p.G_hi), V(p.G_lo), w0 + 3, bprm(i, 11), F(p.Y), (int)M, D, Hd)) return 1;
        const bool last = (i + 1 == c.depth);
        // the next block's norm1 (for the last block the pair is unused: the head normalises the cls rows itself)
        const float* g = last ? prm(4 + 12 * c.depth) : bprm(i + 1, 0);
        const float* bt = last ? prm(4 + 12 * c.depth + 1) : bprm(i + 1, 1);
        launch_resid_ln_split<1>(rows_grid_t(M), st, D, (const float*)x2, (const float*)F(p.Y), (const float*)nullptr, (const float*)nullptr, x, g, bt, c.ln_eps, H16(p.h_hi), LO(p.h_lo), M, D, T, f16);
    }
    const int base = 4 + 12 * c.depth;
    k_teacher_head<<<c.batch, 256, (D + 8) * sizeof(float), st>>>(x, prm(base), prm(base + 1), c.ln_eps, prm(base + 2), prm(base + 3), logits, D, T,
                                                                  c.num_classes);
    QV_CHECK_LAUNCH(who);
    return 0;
}

int qatvit_teacher_forward(const qatvit_cfg* cfg, void* const* params, void* const* w_hi, void* const* w_lo, const float* images, float* logits,
                           void* workspace, void* stream) {
    return teacher_forward_impl(cfg, params, w_hi, w_lo, 3, images, logits, workspace, stream, "qatvit_teacher_forward");
}

int qatvit_teacher_forward_f16(const qatvit_cfg* cfg, void* const* params, void* const* w16, int32_t passes, const float* images, float* logits,
                               void* workspace, void* stream) {
    QV_CHECK_ARG(passes == 1 || passes == 2, "qatvit_teacher_forward_f16: passes %d (1 or 2)", passes);
    return teacher_forward_impl(cfg, params, w16, nullptr, passes, images, logits, workspace, stream, "qatvit_teacher_forward_f16");
}

}  // extern "C"
