// Float (pre-QAT) student step: forward that keeps what the backward needs, and the backward, native on gfx950.
//
// Replaces: `student_out = model(images)` ... `loss.backward()` of the reference's float epochs (qat_trainer.py:295-361 before
// prepare_qat), the unprepared QATWrapper(vit_*_patch16_224) in fp32.  Every GEMM operand is a float tensor held as a bf16 (hi, lo)
// pair and every product takes three MFMA passes (hi.hi + lo.hi + hi.lo, fp32 accumulate): the teacher's 3-pass form (teacher.hip),
// here on both sides of the backward too - dgrad = launch_gemm_nt (kNTBf16) with the transposed weight pair, wgrad = launch_gemm_tn (kTNPair) with
// pairs on both sides.  The forward is the teacher's (patches, fused residual + LayerNorm, float attention, GELU) with the extra
// outputs a backward needs: LayerNorm mean / rstd, attention log-sum-exp, the fc1 pre-activation, the residual stream.
// Of the QAT engine's backward kernels the LayerNorm backward (elt.hip k_ln_bwd_fq), the GELU' pass (k_mask_bwd) and the
// embedding backward (k_embed_bwd) are reused with a disabled quantiser: {scale 1, 1/scale 1, zero point 0, enabled 0} makes
// every fake-quant an identity and every STE mask 1 (elt.hip fqv).  New here: the weight pairs, the head, and the attention
// backward (fp32 FMA, no quantisation, no mask).
#include "../../include/qatvit.h"

#include "qv_common.h"
#include "qv_device.h"
#include "qv_kernels.h"

namespace qv {

// ---------------------------------------------------------------- weight (hi, lo) pairs, as stored and transposed
// (the weights change every optimizer step: rebuilt by every forward; hiT / loT are the B operands of the dgrad GEMMs)
struct FsWTab {
    const float* W[kMaxW];
    __bf16* hi[kMaxW];
    __bf16* lo[kMaxW];
    __bf16* hiT[kMaxW];
    __bf16* loT[kMaxW];
    int N[kMaxW], K[kMaxW], blk0[kMaxW + 1];
    int n;
};
__global__ __launch_bounds__(256) void k_fs_wsplit(const FsWTab t) {
    __shared__ float tile[32][33];
    int wi = 0;
    while (wi + 1 < t.n && (int)blockIdx.x >= t.blk0[wi + 1]) ++wi;
    const int N = t.N[wi], K = t.K[wi], tilesK = (K + 31) / 32, local = (int)blockIdx.x - t.blk0[wi];
    const int n0 = (local / tilesK) * 32, k0 = (local % tilesK) * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const float* W = t.W[wi];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int n = n0 + ty + 8 * i, k = k0 + tx;
        float v = 0.f;
        if (n < N && k < K) {
            v = W[(int64_t)n * K + k];
            const __bf16 h = (__bf16)v;
            t.hi[wi][(int64_t)n * K + k] = h;
            t.lo[wi][(int64_t)n * K + k] = (__bf16)(v - (float)h);
        }
        tile[ty + 8 * i][tx] = v;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int k = k0 + ty + 8 * i, n = n0 + tx;
        if (n < N && k < K) {
            const float v = tile[tx][ty + 8 * i];
            const __bf16 h = (__bf16)v;
            t.hiT[wi][(int64_t)k * N + n] = h;
            t.loT[wi][(int64_t)k * N + n] = (__bf16)(v - (float)h);
        }
    }
}

// ---------------------------------------------------------------- constants: the disabled quantiser and an all-ones STE mask
__global__ void k_fs_consts(float* qp_off, uint32_t* ones, int64_t nwords) {
    const int64_t i0 = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i0 == 0) { qp_off[0] = 1.f; qp_off[1] = 1.f; qp_off[2] = 0.f; qp_off[3] = 0.f; }
    for (int64_t i = i0; i < nwords; i += (int64_t)gridDim.x * blockDim.x) ones[i] = 0xffffffffu;
}

// ---------------------------------------------------------------- head (cls pooling), fp32: B x C x D is tiny
// hn[b,:] = LN(x[b,0,:]) from the saved row statistics; logits[b,c] = hn[b,:] . W[c,:] + bias[c]
// STATS (observe-only forward): the min / max of the logits into kStatSlots accumulator pairs, one atomic per wave
template <bool STATS = false>
__global__ __launch_bounds__(256) void k_fs_head_fwd(const float* __restrict__ x, const float* __restrict__ mean, const float* __restrict__ rstd,
                                                     const float* __restrict__ gamma, const float* __restrict__ beta, const float* __restrict__ W,
                                                     const float* __restrict__ bias, float* __restrict__ hn, float* __restrict__ logits, int D, int T, int C,
                                                     uint32_t* __restrict__ stats = nullptr) {
    extern __shared__ float sh[];
    float smn = INFINITY, smx = -INFINITY;
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t row = (int64_t)b * T;
    const float mu = mean[row], rs = rstd[row];
    for (int c = threadIdx.x; c < D; c += 256) {
        const float v = (x[row * D + c] - mu) * rs * gamma[c] + beta[c];
        sh[c] = v;
        hn[(int64_t)b * D + c] = v;
    }
    __syncthreads();
    for (int c = wave; c < C; c += 4) {
        float acc = 0.f;
        for (int k = lane; k < D; k += 64) acc += sh[k] * W[(int64_t)c * D + k];
        acc = wave_sum(acc);
        if (lane == 0) logits[(int64_t)b * C + c] = acc + bias[c];
        if constexpr (STATS) { smn = fminf(smn, acc + bias[c]); smx = fmaxf(smx, acc + bias[c]); }
    }
    if constexpr (STATS) {
        if (lane == 0) stat_atomic(stats, kStatSlots, smn, smx);   // (the sums are wave-uniform: lane 0 holds the wave's min / max)
    }
}
// one thread per output element, fixed summation order (no atomics):
//   dW[c,d] = sum_b dl[b,c] hn[b,d];  dhn[b,d] = sum_c dl[b,c] W[c,d];  dbias[c] = sum_b dl[b,c]
__global__ __launch_bounds__(256) void k_fs_head_bwd(const float* __restrict__ dl, const float* __restrict__ hn, const float* __restrict__ W,
                                                     float* __restrict__ dW, float* __restrict__ dbias, float* __restrict__ dhn, int B, int D, int C) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    const int64_t nW = (int64_t)C * D, nH = (int64_t)B * D;
    if (i < nW) {
        const int c = (int)(i / D), d = (int)(i % D);
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
        int b = 0;
        for (; b + 3 < B; b += 4) {
            a0 += dl[(int64_t)b * C + c] * hn[(int64_t)b * D + d];
            a1 += dl[(int64_t)(b + 1) * C + c] * hn[(int64_t)(b + 1) * D + d];
            a2 += dl[(int64_t)(b + 2) * C + c] * hn[(int64_t)(b + 2) * D + d];
            a3 += dl[(int64_t)(b + 3) * C + c] * hn[(int64_t)(b + 3) * D + d];
        }
        for (; b < B; ++b) a0 += dl[(int64_t)b * C + c] * hn[(int64_t)b * D + d];
        dW[i] = (a0 + a1) + (a2 + a3);
    } else if (i < nW + nH) {
        const int64_t j = i - nW;
        const int b = (int)(j / D), d = (int)(j % D);
        float a = 0.f;
        for (int c = 0; c < C; ++c) a += dl[(int64_t)b * C + c] * W[(int64_t)c * D + d];
        dhn[j] = a;
    } else if (i < nW + nH + C) {
        const int c = (int)(i - nW - nH);
        float a = 0.f;
        for (int b = 0; b < B; ++b) a += dl[(int64_t)b * C + c];
        dbias[c] = a;
    }
}

// ---------------------------------------------------------------- float attention backward
// Per (image, head) z = b * H + h, with s = head_dim^-0.5 and the forward's lse:
//   P = exp(s Q K^T - lse)          dS = P * (dO V^T - delta),  delta_i = dO_i . O_i
//   dQ = s dS K     dK = s dS^T Q     dV = P^T dO
// as five batched fp32 GEMMs C[z](m, n) = sum_k A[z](m, k) B[z](n, k) over strided views of qkv / dO / the [z][T][T] P and dS planes;
// 64 x 64 tiles, 4 x 4 outputs per thread, fp32 FMA.  dQ / dK / dV leave as the bf16 (hi, lo) pair of dqkv the dgrad / wgrad GEMMs read.
struct FsAttnGemm {
    const float* A; int64_t a_b, a_h; int a_m, a_k;
    const float* B; int64_t b_b, b_h; int b_n, b_k;
    int M, N, K, H;
    int mode;             // 0: out = exp(alpha acc - rowv)   1: out = P * (acc - rowv)   2: (ohi, olo) = split(alpha acc)
    float alpha;
    const float* rowv;    // [z][M]: lse (mode 0) or delta (mode 1)
    const float* P;       // mode 1: [z][M][N]
    float* out;           // modes 0 / 1: [z][M][N]
    __bf16* ohi; __bf16* olo; int64_t o_b, o_h; int o_m;   // mode 2: element (m, n) at b * o_b + h * o_h + m * o_m + n
};
constexpr int kFsTK = 16, kFsLD = 68;   // k-step; LDS row stride in floats (64 + 4: the k-fastest stores spread over the banks)
__global__ __launch_bounds__(256) void k_fs_attn_gemm(const FsAttnGemm p) {
    __shared__ __attribute__((aligned(16))) float As[kFsTK][kFsLD];
    __shared__ __attribute__((aligned(16))) float Bs[kFsTK][kFsLD];
    const int z = blockIdx.z, b = z / p.H, h = z % p.H;
    const int m0 = blockIdx.y * 64, n0 = blockIdx.x * 64;
    const float* A = p.A + b * p.a_b + h * p.a_h;
    const float* Bm = p.B + b * p.b_b + h * p.b_h;
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
    for (int k0 = 0; k0 < p.K; k0 += kFsTK) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {   // 16 x 64 elements of each operand, the contiguous axis across consecutive threads
            const int idx = tid + 256 * e;
            int kk, mm;
            if (p.a_k == 1) { kk = idx & 15; mm = idx >> 4; } else { mm = idx & 63; kk = idx >> 6; }
            const int m = m0 + mm, k = k0 + kk;
            As[kk][mm] = (m < p.M && k < p.K) ? A[(int64_t)m * p.a_m + (int64_t)k * p.a_k] : 0.f;
            int kb, nn;
            if (p.b_k == 1) { kb = idx & 15; nn = idx >> 4; } else { nn = idx & 63; kb = idx >> 6; }
            const int n = n0 + nn, kq = k0 + kb;
            Bs[kb][nn] = (n < p.N && kq < p.K) ? Bm[(int64_t)n * p.b_n + (int64_t)kq * p.b_k] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < kFsTK; ++kk) {
            const float4 a = *reinterpret_cast<const float4*>(&As[kk][ty * 4]);
            const float4 c = *reinterpret_cast<const float4*>(&Bs[kk][tx * 4]);
            const float av[4] = {a.x, a.y, a.z, a.w}, bv[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(av[i], bv[j], acc[i][j]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int m = m0 + ty * 4 + i;
        if (m >= p.M) continue;
        if (p.mode == 2) {
            const int64_t base = b * p.o_b + h * p.o_h + (int64_t)m * p.o_m;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int n = n0 + tx * 4 + j;
                if (n < p.N) {
                    const float v = p.alpha * acc[i][j];
                    const __bf16 hv = (__bf16)v;
                    p.ohi[base + n] = hv;
                    p.olo[base + n] = (__bf16)(v - (float)hv);
                }
            }
        } else {
            const float rv = p.rowv[(int64_t)z * p.M + m];
            const int64_t base = ((int64_t)z * p.M + m) * p.N;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int n = n0 + tx * 4 + j;
                if (n < p.N) p.out[base + n] = p.mode == 0 ? expf(p.alpha * acc[i][j] - rv) : p.P[base + n] * (acc[i][j] - rv);
            }
        }
    }
}
// delta[(b * H + h) * T + t] = dO[b, t, h, :] . O[b, t, h, :]   (O from its (hi, lo) pair).  One thread per 4 consecutive columns (coalesced
// 16-B / 8-B loads); the head_dim / 4 lanes of one (row, head) are consecutive and meet through lane shuffles.
__global__ __launch_bounds__(256) void k_fs_attn_delta(const float* __restrict__ dO, const __bf16* __restrict__ O_hi, const __bf16* __restrict__ O_lo,
                                                       float* __restrict__ delta, int64_t M, int T, int H, int D) {
    const int64_t e4 = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, n4 = M * (D / 4);
    const int q = D / H / 4;   // lanes per (row, head): 16 or 8
    float a = 0.f;
    if (e4 < n4) {
        const float4 g = reinterpret_cast<const float4*>(dO)[e4];
        const bf16x4 oh = reinterpret_cast<const bf16x4*>(O_hi)[e4], ol = reinterpret_cast<const bf16x4*>(O_lo)[e4];
        a = g.x * ((float)oh[0] + (float)ol[0]) + g.y * ((float)oh[1] + (float)ol[1]) + g.z * ((float)oh[2] + (float)ol[2]) +
            g.w * ((float)oh[3] + (float)ol[3]);
    }
    for (int o = q / 2; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
    if (e4 < n4) {
        const int64_t row = e4 / (D / 4);
        const int c4 = (int)(e4 % (D / 4));
        if (c4 % q == 0) {
            const int h = c4 / q, t = (int)(row % T);
            delta[((row / T) * H + h) * T + t] = a;
        }
    }
}

static int launch_fs_attn_gemm(const FsAttnGemm& a, int Bsz, hipStream_t st) {
    dim3 grid((a.N + 63) / 64, (a.M + 63) / 64, Bsz * a.H);
    k_fs_attn_gemm<<<grid, 256, 0, st>>>(a);
    return 0;
}

// qkv fp32 [B*T, 3D], O pair [B*T, D], lse [B][H][T], dO fp32 [B*T, D] -> dqkv pair [B*T, 3D]; Pm / dS: [B*H][T][T] fp32, delta [B*H*T]
static int launch_attn_bwd_float(const float* qkv, const void* O_hi, const void* O_lo, const float* lse, const float* dO, int B, int T, int H, int D,
                                 float* Pm, float* dS, float* delta, void* dqkv_hi, void* dqkv_lo, hipStream_t st) {
    const int hd = D / H, ld = 3 * D;
    const float scale = 1.0f / sqrtf((float)hd);
    const int64_t n4 = (int64_t)B * T * (D / 4);
    k_fs_attn_delta<<<(int)((n4 + 255) / 256), 256, 0, st>>>(dO, reinterpret_cast<const __bf16*>(O_hi), reinterpret_cast<const __bf16*>(O_lo), delta,
                                                              (int64_t)B * T, T, H, D);
    const int64_t qb = (int64_t)T * ld;   // qkv image stride
    const int64_t ob = (int64_t)T * D;    // dO image stride
    const int64_t pz_b = (int64_t)H * T * T, pz_h = (int64_t)T * T;
    FsAttnGemm g{};
    g.H = H;
    // P = exp(s Q K^T - lse): m = query, n = key, k = d
    g.A = qkv; g.a_b = qb; g.a_h = hd; g.a_m = ld; g.a_k = 1;
    g.B = qkv + D; g.b_b = qb; g.b_h = hd; g.b_n = ld; g.b_k = 1;
    g.M = T; g.N = T; g.K = hd; g.mode = 0; g.alpha = scale; g.rowv = lse; g.out = Pm;
    launch_fs_attn_gemm(g, B, st);
    // dS = P * (dO V^T - delta)
    g.A = dO; g.a_b = ob; g.a_h = hd; g.a_m = D; g.a_k = 1;
    g.B = qkv + 2 * D; g.b_b = qb; g.b_h = hd; g.b_n = ld; g.b_k = 1;
    g.mode = 1; g.alpha = 1.f; g.rowv = delta; g.P = Pm; g.out = dS;
    launch_fs_attn_gemm(g, B, st);
    g.mode = 2; g.ohi = reinterpret_cast<__bf16*>(dqkv_hi); g.olo = reinterpret_cast<__bf16*>(dqkv_lo); g.o_b = qb; g.o_h = hd; g.o_m = ld;
    g.N = hd; g.K = T;
    // dQ = s dS K: m = query, n = d, k = key
    g.A = dS; g.a_b = pz_b; g.a_h = pz_h; g.a_m = T; g.a_k = 1;
    g.B = qkv + D; g.b_b = qb; g.b_h = hd; g.b_n = 1; g.b_k = ld;
    g.alpha = scale;
    launch_fs_attn_gemm(g, B, st);
    // dK = s dS^T Q: m = key, n = d, k = query
    g.ohi += D; g.olo += D;
    g.A = dS; g.a_m = 1; g.a_k = T;
    g.B = qkv; g.b_n = 1; g.b_k = ld;
    launch_fs_attn_gemm(g, B, st);
    // dV = P^T dO: m = key, n = d, k = query
    g.ohi += D; g.olo += D;
    g.A = Pm; g.a_m = 1; g.a_k = T;
    g.B = dO; g.b_b = ob; g.b_h = hd; g.b_n = 1; g.b_k = D;
    g.alpha = 1.f;
    launch_fs_attn_gemm(g, B, st);
    return 0;
}

}  // namespace qv

using namespace qv;

extern "C" {

// The host driver of every form of the step: the pair form (bf16 (hi, lo) pairs, three MFMA passes), the fp16 form (one fp16 plane per GEMM
// operand, one pass; its device code and launchers are float_amp.hip's) and the bf16 form (the fp16 form on bf16 planes and bf16 MFMA).  The
// one-plane forms keep each plane at the _hi offset.
// Workspace: a batch-independent head (constants, the weight planes, the weight-gradient scratch) and the batch-sized rest.  The _lo planes and the
// fp32 attention-backward scratch (Pm, dS, delta) are the pair form's only, amax (the fp16 residual gradient's maximum) the fp16 form's; a plane a
// form does not take has offset -1.
enum class FsForm { pair, f16, bf16 };
struct FsBlock { int64_t x, xm, h1_hi, h1_lo, h2_hi, h2_lo, mean1, rstd1, mean2, rstd2, qkv, O_hi, O_lo, lse, Y1, G_hi, G_lo; };
struct FsPlan {
    int64_t qp_off, amax, w_hi[kMaxW], w_lo[kMaxW], w_hiT[kMaxW], w_loT[kMaxW], tn_partial;
    int64_t ones, p_hi, p_lo, Y0, x_last, meanf, rstdf, hf_hi, hf_lo, hn;
    FsBlock blk[12];
    int64_t Y, dx, dx2, dp_hi, dp_lo, dG, dY1_hi, dY1_lo, dh, dO, dqkv_hi, dqkv_lo, Pm, dS, delta, dhn, dY0_hi, dY0_lo;
    int64_t ones_words, total;
};
static const char* fs_form_name(FsForm form) { return form == FsForm::f16 ? " amp" : form == FsForm::bf16 ? " bf16" : ""; }
static int fs_check(const qatvit_cfg& c, FsForm form) {
    const bool one = form != FsForm::pair;
    const int hd = c.num_heads > 0 ? c.embed_dim / c.num_heads : 0;
    const int np = c.patch_size > 0 ? (c.img_size / c.patch_size) * (c.img_size / c.patch_size) : 0;
    const int mult = one ? 384 : 128;
    if (c.batch < 1 || c.depth < 1 || c.depth > 12 || c.embed_dim % mult != 0 || c.embed_dim > 768 || c.mlp_hidden % mult != 0 || c.num_heads < 1 ||
        c.embed_dim % c.num_heads != 0 || (hd != 32 && hd != 64) || c.patch_size % 4 != 0 || c.img_size % c.patch_size != 0 || np + 1 > 224 ||
        (c.in_chans * c.patch_size * c.patch_size) % 128 != 0 || c.num_classes < 1) {
        set_error("float student%s: unsupported config (batch %d depth %d dim %d hidden %d heads %d img %d patch %d): needs %s, head_dim 32 or 64, "
                  "<= 224 tokens, depth <= 12", fs_form_name(form), c.batch, c.depth, c.embed_dim, c.mlp_hidden, c.num_heads, c.img_size, c.patch_size,
                  one ? "dim and hidden multiples of 384, dim <= 768" : "dim % 128 == 0 and <= 768");
        return 1;
    }
    return 0;
}
// weight wi: 0 patch embedding, 1 + 4 i + {0 qkv, 1 proj, 2 fc1, 3 fc2} of block i, 1 + 4 depth the head (the weight fake-quant order)
static void fs_weight_shape(const qatvit_cfg& c, int wi, int* N, int* K) {
    const int D = c.embed_dim, Hd = c.mlp_hidden;
    if (wi == 0) { *N = D; *K = c.in_chans * c.patch_size * c.patch_size; return; }
    if (wi == 1 + 4 * c.depth) { *N = c.num_classes; *K = D; return; }
    switch ((wi - 1) % 4) {
        case 0: *N = 3 * D; *K = D; break;
        case 1: *N = D; *K = D; break;
        case 2: *N = Hd; *K = D; break;
        default: *N = D; *K = Hd; break;
    }
}
static int fs_weight_param(const qatvit_cfg& c, int wi) {   // its index in the parameter order (include/qatvit.h); its bias follows it
    static const int kW[4] = {2, 4, 8, 10};                  // qkv, proj, fc1, fc2 weights within a block's 12 parameters
    return wi == 0 ? 0 : wi == 1 + 4 * c.depth ? 4 + 12 * c.depth + 2 : 4 + 12 * ((wi - 1) / 4) + kW[(wi - 1) % 4];
}
static FsPlan fs_plan(const qatvit_cfg& c, FsForm form) {
    FsPlan p{};
    int64_t o = 0;
    auto take = [&](int64_t b) { int64_t r = o; o += (b + 255) & ~(int64_t)255; return r; };
    auto pair = [&](int64_t b) { return form != FsForm::pair ? (int64_t)-1 : take(b); };   // taken by the pair form only
    const int64_t np = (int64_t)(c.img_size / c.patch_size) * (c.img_size / c.patch_size), T = np + 1, B = c.batch, M = B * T, D = c.embed_dim,
                  Hd = c.mlp_hidden, H = c.num_heads, Kpe = (int64_t)c.in_chans * c.patch_size * c.patch_size;
    p.qp_off = take(16);
    p.amax = form == FsForm::f16 ? take((int64_t)kDyAmaxSlots * kDyAmaxStride * 4) : -1;
    for (int wi = 0; wi < 1 + 4 * c.depth; ++wi) {
        int N, K;
        fs_weight_shape(c, wi, &N, &K);
        p.w_hi[wi] = take((int64_t)N * K * 2); p.w_lo[wi] = pair((int64_t)N * K * 2);
        p.w_hiT[wi] = take((int64_t)N * K * 2); p.w_loT[wi] = pair((int64_t)N * K * 2);
    }
    p.tn_partial = take(kTnScratchBytes);
    p.ones_words = ln_maskbits_bytes(M, (int)D) / 4;
    p.ones = take(ln_maskbits_bytes(M, (int)D));
    p.p_hi = take(B * np * Kpe * 2); p.p_lo = pair(B * np * Kpe * 2);
    p.Y0 = take(B * np * D * 4);
    for (int i = 0; i < c.depth; ++i) {
        FsBlock& k = p.blk[i];
        k.x = take(M * D * 4); k.xm = take(M * D * 4);
        k.h1_hi = take(M * D * 2); k.h1_lo = pair(M * D * 2); k.h2_hi = take(M * D * 2); k.h2_lo = pair(M * D * 2);
        k.mean1 = take(M * 4); k.rstd1 = take(M * 4); k.mean2 = take(M * 4); k.rstd2 = take(M * 4);
        k.qkv = take(M * 3 * D * 4);
        k.O_hi = take(M * D * 2); k.O_lo = pair(M * D * 2);
        k.lse = take(B * H * T * 4);
        k.Y1 = take(M * Hd * 4);
        k.G_hi = take(M * Hd * 2); k.G_lo = pair(M * Hd * 2);
    }
    p.x_last = take(M * D * 4);
    p.meanf = take(M * 4); p.rstdf = take(M * 4);
    p.hf_hi = take(M * D * 2); p.hf_lo = pair(M * D * 2);
    p.hn = take(B * D * 4);
    p.Y = take(M * D * 4);
    p.dx = take(M * D * 4); p.dx2 = take(M * D * 4);
    p.dp_hi = take(M * D * 2); p.dp_lo = pair(M * D * 2);
    p.dG = take(M * Hd * 4);
    p.dY1_hi = take(M * Hd * 2); p.dY1_lo = pair(M * Hd * 2);
    p.dh = take(M * D * 4);
    p.dO = take(M * D * 4);
    p.dqkv_hi = take(M * 3 * D * 2); p.dqkv_lo = pair(M * 3 * D * 2);
    p.Pm = pair(B * H * T * T * 4); p.dS = pair(B * H * T * T * 4);
    p.delta = pair(B * H * T * 4);
    p.dhn = take(B * D * 4);
    p.dY0_hi = take(B * np * D * 2); p.dY0_lo = pair(B * np * D * 2);
    p.total = o;
    return p;
}

static int64_t fs_workspace_bytes(const char* fn, FsForm form, const qatvit_cfg* cfg) {
    if (!cfg) { set_error("%s: null argument", fn); return -1; }
    if (fs_check(*cfg, form)) return -1;
    return fs_plan(*cfg, form).total;
}

static void fs_consts(const FsPlan& p, char* ws, hipStream_t st) {
    k_fs_consts<<<flat_grid_fs(p.ones_words), 256, 0, st>>>(reinterpret_cast<float*>(ws + p.qp_off), reinterpret_cast<uint32_t*>(ws + p.ones), p.ones_words);
}

static int fs_init(const char* fn, FsForm form, const qatvit_cfg* cfg, void* workspace, void* stream) {
    QV_CHECK_ARG(cfg && workspace, "%s: null argument", fn);
    if (fs_check(*cfg, form)) return 1;
    drop_path_bind(workspace, nullptr);   // (a drop-path table bound to this address belongs to whatever stood here before; a LayerScale binding too)
    layer_scale_bind(workspace, 0, nullptr, nullptr, nullptr);
    fs_consts(fs_plan(*cfg, form), reinterpret_cast<char*>(workspace), (hipStream_t)stream);
    QV_CHECK_LAUNCH(fn);
    return 0;
}

// ---------------------------------------------------------------- observe-only form (include/qatvit.h qatvit_float_student_forward_observe)
// The observe buffer: the fold table (one ObsFoldEntry per fake-quant module, act_fq order then weight_fq order), then the min / max accumulators -
// kStatSlots pairs per activation quantizer and per per-tensor weight quantizer, 2 words per channel for a per-channel one.  Batch independent.
struct ObsPlan {
    int n_act, n_w, nblocks;
    int64_t tab, act_stats, w_stats[kMaxW], stats_words, total;
};
static int fs_n_act(const qatvit_cfg& c) { return 4 + 6 * c.depth; }
static int fs_n_w(const qatvit_cfg& c) { return 2 + 4 * c.depth; }
static ObsPlan obs_plan(const qatvit_cfg& c) {
    ObsPlan p{};
    p.n_act = fs_n_act(c);
    p.n_w = fs_n_w(c);
    int64_t o = 0;
    auto take = [&](int64_t b) { int64_t r = o; o += (b + 255) & ~(int64_t)255; return r; };
    p.tab = take((int64_t)(p.n_act + p.n_w) * sizeof(ObsFoldEntry));
    int64_t words = (int64_t)p.n_act * kStatSlots * kStatStride;
    p.nblocks = p.n_act;
    for (int wi = 0; wi < p.n_w; ++wi) {
        int N, K;
        fs_weight_shape(c, wi, &N, &K);
        p.w_stats[wi] = words;
        words += c.w_per_channel ? 2 * (int64_t)N : kStatSlots * kStatStride;
        p.nblocks += c.w_per_channel ? (N + 63) / 64 : 1;
    }
    p.stats_words = words;
    p.act_stats = take(words * 4);
    p.total = o;
    return p;
}
// statistics of one forward: where each producer accumulates (nullptr everywhere: the plain float forward)
struct FsObs {
    uint32_t* stats = nullptr;   // the accumulators (ObsPlan::act_stats)
    const ObsPlan* p = nullptr;
    uint32_t* act(int ai) const { return stats ? stats + (int64_t)ai * kStatSlots * kStatStride : nullptr; }
    uint32_t* w(int wi) const { return stats + p->w_stats[wi]; }
};

// params: fp32 tensors in the student's order (include/qatvit.h).  Leaves in the workspace everything fs_backward reads.  logits: fp32, fp16 (the
// fp16 form) or bf16 (the bf16 form).  observe (the pair form only): also every observer's step (qatvit_float_student_forward_observe).
static int fs_forward(const char* fn, FsForm form, const qatvit_cfg* cfg, void* const* params, const float* images, void* logits, void* workspace,
                      void* observe, void* stream) {
    QV_CHECK_ARG(cfg && params && images && logits && workspace, "%s: null argument", fn);
    if (fs_check(*cfg, form)) return 1;
    const qatvit_cfg& c = *cfg;
    const FsPlan p = fs_plan(c, form);
    const bool f16 = form == FsForm::f16, bf16 = form == FsForm::bf16, one = f16 || bf16;
    ObsPlan op{};
    FsObs ob;
    if (observe) {
        op = obs_plan(c);
        ob.stats = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(observe) + op.act_stats);
        ob.p = &op;
    }
    char* ws = reinterpret_cast<char*>(workspace);
    hipStream_t st = (hipStream_t)stream;
    const int np = (c.img_size / c.patch_size) * (c.img_size / c.patch_size), T = np + 1, D = c.embed_dim, Hd = c.mlp_hidden;
    const int Kpe = c.in_chans * c.patch_size * c.patch_size, L = c.depth;
    const int64_t M = (int64_t)c.batch * T;
    auto F = [&](int64_t off) { return reinterpret_cast<float*>(ws + off); };
    auto V = [&](int64_t off) { return off < 0 ? nullptr : reinterpret_cast<void*>(ws + off); };
    auto prm = [&](int i) { return reinterpret_cast<const float*>(params[i]); };
    auto bprm = [&](int blk, int k) { return prm(4 + 12 * blk + k); };
    // drop-path (qatvit_float_student_set_drop_path): the per-sample multipliers of block i's attention (mlp = 0) or MLP (1) branch, nullptr without a table
    const float* const drop = drop_path_of(workspace);
    auto drop_row = [&](int i, int mlp) { return drop ? drop + (int64_t)(2 * i + mlp) * c.batch : nullptr; };
    // LayerScale (qatvit_float_student_set_layer_scale): the branch's gamma, and where its output goes - its own rows of the binding's saved buffer, which the
    // backward reads for gamma's gradient, instead of the one shared Y (a binding without that buffer serves a forward alone)
    const std::shared_ptr<const LayerScale> ls = layer_scale_of(workspace);
    QV_CHECK_ARG(!ls || (int)ls->gamma.size() == 2 * c.depth, "%s: the LayerScale binding holds %d branches, depth is %d", fn, (int)ls->gamma.size(), c.depth);
    auto ls_gamma = [&](int i, int mlp) { return ls ? ls->gamma[2 * i + mlp] : nullptr; };
    // ---- the form's steps
    auto weight_planes = [&] {   // the weights' (hi, lo) pairs or fp16 / bf16 planes, as stored and transposed, in one launch
        FsWTab t{};
        t.n = 1 + 4 * L;
        int blocks = 0;
        for (int wi = 0; wi < t.n; ++wi) {
            fs_weight_shape(c, wi, &t.N[wi], &t.K[wi]);
            t.W[wi] = prm(fs_weight_param(c, wi));
            t.hi[wi] = reinterpret_cast<__bf16*>(V(p.w_hi[wi])); t.lo[wi] = reinterpret_cast<__bf16*>(V(p.w_lo[wi]));
            t.hiT[wi] = reinterpret_cast<__bf16*>(V(p.w_hiT[wi])); t.loT[wi] = reinterpret_cast<__bf16*>(V(p.w_loT[wi]));
            t.blk0[wi] = blocks;
            blocks += ((t.N[wi] + 31) / 32) * ((t.K[wi] + 31) / 32);
        }
        t.blk0[t.n] = blocks;
        if (one) launch_fa_wcast(t.n, t.W, reinterpret_cast<void* const*>(t.hi), reinterpret_cast<void* const*>(t.hiT), t.N, t.K, t.blk0, st, bf16);
        else k_fs_wsplit<<<blocks, 256, 0, st>>>(t);
    };
    // (act_fq order: 0 quant, 1 patch_embed.proj, per block 2 + 6 i + {norm1, qkv, proj, norm2, fc1, fc2}, then norm, head)
    // (the bf16 form: kNTBf16 without lo planes - its one-plane path)
    auto gemm = [&](int64_t ah, int64_t al, int wi, const float* bias, float* C, int N, int K, int Mrows, int ai) {
        NTGemm g;
        g.A = V(ah); g.A_lo = V(al); g.B = V(p.w_hi[wi]); g.B_lo = V(p.w_lo[wi]); g.C = C; g.M = Mrows; g.N = N; g.K = g.lda = g.ldb = K; g.ldc = N;
        g.bias = bias; g.stats = ob.act(ai); g.stat_slots = ob.stats ? kStatSlots : 1;
        return launch_gemm_nt(f16 ? kNTF16 : kNTBf16, g, nullptr, st);
    };
    auto gelu = [&](const FsBlock& k) {
        if (one) launch_fa_gelu(F(k.Y1), V(k.G_hi), M * Hd, st, bf16);
        else launch_gelu_split(F(k.Y1), V(k.G_hi), V(k.G_lo), M * Hd, st);
    };
    auto head = [&](const float* gamma, const float* beta, const float* W, const float* bias) {
        if (one)
            launch_fa_head_fwd(F(p.x_last), F(p.meanf), F(p.rstdf), gamma, beta, W, bias, F(p.hn), logits, c.batch, D, T, c.num_classes, st, bf16);
        else if (ob.stats)
            k_fs_head_fwd<true><<<c.batch, 256, D * sizeof(float), st>>>(F(p.x_last), F(p.meanf), F(p.rstdf), gamma, beta, W, bias, F(p.hn),
                                                                        reinterpret_cast<float*>(logits), D, T, c.num_classes, ob.act(3 + 6 * L));
        else
            k_fs_head_fwd<<<c.batch, 256, D * sizeof(float), st>>>(F(p.x_last), F(p.meanf), F(p.rstdf), gamma, beta, W, bias, F(p.hn),
                                                                  reinterpret_cast<float*>(logits), D, T, c.num_classes);
    };
    fs_consts(p, ws, st);   // (cheap; a workspace bound at another batch keeps working without a second init)
    weight_planes();
    if (ob.stats) {   // re-arm every accumulator; the images' and the weights' statistics (the QAT forward's weight pass, fq.hip k_w_observe_all)
        launch_ws_init(ob.stats, op.stats_words / 2, st);
        launch_minmax(images, 1, (int64_t)c.batch * c.in_chans * c.img_size * c.img_size, 0, ob.act(0), kStatSlots, st);
        WObsTab to{};
        to.n = op.n_w;
        to.per_channel = c.w_per_channel;
        to.nslots = kStatSlots;
        for (int wi = 0; wi < to.n; ++wi) {
            fs_weight_shape(c, wi, &to.N[wi], &to.K[wi]);
            to.W[wi] = prm(fs_weight_param(c, wi));
            to.ws[wi] = ob.w(wi);
        }
        launch_w_observe_all(to, st);
    }
    launch_patches_split(images, V(p.p_hi), V(p.p_lo), c.batch, c.in_chans, c.img_size, c.img_size, c.patch_size, st, f16);
    if (gemm(p.p_hi, p.p_lo, 0, prm(1), F(p.Y0), D, Kpe, c.batch * np, 1)) return 1;
    launch_resid_ln_split_save(0, nullptr, F(p.Y0), prm(2), prm(3), F(p.blk[0].x), bprm(0, 0), bprm(0, 1), c.ln_eps, V(p.blk[0].h1_hi), V(p.blk[0].h1_lo),
                               F(p.blk[0].mean1), F(p.blk[0].rstd1), M, D, T, st, ob.act(2), f16);
    for (int i = 0; i < L; ++i) {
        const FsBlock& k = p.blk[i];
        const int w0 = 1 + 4 * i, a0 = 2 + 6 * i;
        if (gemm(k.h1_hi, k.h1_lo, w0 + 0, bprm(i, 3), F(k.qkv), 3 * D, D, (int)M, a0 + 1)) return 1;
        if (launch_attn_fwd_float(F(k.qkv), c.batch, T, c.num_heads, D, V(k.O_hi), V(k.O_lo), st, f16, F(k.lse))) return 1;
        float* const Ya = ls && ls->saved ? ls->saved + (int64_t)(2 * i) * M * D : F(p.Y);
        float* const Ym = ls && ls->saved ? ls->saved + (int64_t)(2 * i + 1) * M * D : F(p.Y);
        if (gemm(k.O_hi, k.O_lo, w0 + 1, bprm(i, 5), Ya, D, D, (int)M, a0 + 2)) return 1;
        launch_resid_ln_split_save(1, F(k.x), Ya, nullptr, nullptr, F(k.xm), bprm(i, 6), bprm(i, 7), c.ln_eps, V(k.h2_hi), V(k.h2_lo), F(k.mean2),
                                   F(k.rstd2), M, D, T, st, ob.act(a0 + 3), f16, drop_row(i, 0), ls_gamma(i, 0));
        if (gemm(k.h2_hi, k.h2_lo, w0 + 2, bprm(i, 9), F(k.Y1), Hd, D, (int)M, a0 + 4)) return 1;
        gelu(k);
        if (gemm(k.G_hi, k.G_lo, w0 + 3, bprm(i, 11), Ym, D, Hd, (int)M, a0 + 5)) return 1;
        const bool last = i + 1 == L;
        const FsBlock* nx = last ? nullptr : &p.blk[i + 1];
        launch_resid_ln_split_save(1, F(k.xm), Ym, nullptr, nullptr, last ? F(p.x_last) : F(nx->x), last ? prm(4 + 12 * L) : bprm(i + 1, 0),
                                   last ? prm(4 + 12 * L + 1) : bprm(i + 1, 1), c.ln_eps, last ? V(p.hf_hi) : V(nx->h1_hi), last ? V(p.hf_lo) : V(nx->h1_lo),
                                   last ? F(p.meanf) : F(nx->mean1), last ? F(p.rstdf) : F(nx->rstd1), M, D, T, st, ob.act(last ? 2 + 6 * L : a0 + 6), f16,
                                   drop_row(i, 1), ls_gamma(i, 1));
    }
    const int hb = 4 + 12 * L;
    head(prm(hb), prm(hb + 1), prm(hb + 2), prm(hb + 3));
    if (ob.stats)   // every observer at once: nothing in this forward read the quantisers' state, so folding at the end is the stock update
        launch_obs_fold(reinterpret_cast<const ObsFoldEntry*>(reinterpret_cast<char*>(observe) + op.tab), op.n_act + op.n_w, op.nblocks, c.averaging_const, st);
    QV_CHECK_LAUNCH(fn);
    return 0;
}

// dlogits [B, C]: fp32, fp16 (the fp16 form) or bf16 (the bf16 form); grads: fp32 tensors in the params order, ZERO on entry (weight / bias /
// LayerNorm gradients are accumulated into them).  Reads what the last fs_forward of the same form on this workspace (same cfg) left there.
static int fs_backward(const char* fn, FsForm form, const qatvit_cfg* cfg, void* const* params, const void* dlogits, void* const* grads, void* workspace,
                       void* stream) {
    QV_CHECK_ARG(cfg && params && dlogits && grads && workspace, "%s: null argument", fn);
    if (fs_check(*cfg, form)) return 1;
    const qatvit_cfg& c = *cfg;
    const FsPlan p = fs_plan(c, form);
    const bool f16 = form == FsForm::f16, bf16 = form == FsForm::bf16, one = f16 || bf16;
    char* ws = reinterpret_cast<char*>(workspace);
    hipStream_t st = (hipStream_t)stream;
    const int np = (c.img_size / c.patch_size) * (c.img_size / c.patch_size), T = np + 1, D = c.embed_dim, Hd = c.mlp_hidden, H = c.num_heads;
    const int Kpe = c.in_chans * c.patch_size * c.patch_size, L = c.depth, hb = 4 + 12 * L;
    const int64_t M = (int64_t)c.batch * T;
    auto F = [&](int64_t off) { return reinterpret_cast<float*>(ws + off); };
    auto V = [&](int64_t off) { return off < 0 ? nullptr : reinterpret_cast<void*>(ws + off); };
    auto prm = [&](int i) { return reinterpret_cast<const float*>(params[i]); };
    auto grd = [&](int i) { return reinterpret_cast<float*>(grads[i]); };
    const float* qp_off = F(p.qp_off);
    const float* unit = qp_off;   // 1.0f: the unit scale of the one-plane GEMMs
    float* partial = F(p.tn_partial);
    // ---- the form's steps
    // dgrad: C[M, N] = A[M, K] . W[K, N]  with the transposed weight's planes as the B operand ([N, K] row-major)
    // (s2: the one-plane forms' second scalar - 1 / K where the fp16 form carries a branch's gradients scaled by K, see below; else the unit)
    auto dgrad = [&](int64_t ah, int64_t al, int wi, float* C, int N, int K, const float* s2 = nullptr) {
        NTGemm g;
        g.A = V(ah); g.B = V(p.w_hiT[wi]); g.C = C; g.M = (int)M; g.N = N; g.K = g.lda = g.ldb = K; g.ldc = N;
        if (one) { g.s1 = unit; g.s2 = s2 ? s2 : unit; }
        else { g.A_lo = V(al); g.B_lo = V(p.w_loT[wi]); }
        return launch_gemm_nt(bf16 ? kNTPlaneBf16 : f16 ? kNTPlaneF16 : kNTBf16, g, nullptr, st);
    };
    // wgrad: dW[N, Kw] += dY[Mr, N]^T . X[Mr, Kw], dbias[N] += column sums of dY
    auto wgrad = [&](int64_t ph, int64_t pl, int64_t qh, int64_t ql, float* dW, float* db, int N, int Kw, int Mr, const float* s2 = nullptr) {
        TNGemm g;
        g.P = V(ph); g.Q = V(qh); g.C = dW; g.dbias = db; g.N = N; g.Kw = Kw; g.ldp = N; g.ldq = Kw; g.ldc = Kw;
        if (one) { g.s1 = unit; g.s2 = s2 ? s2 : unit; }
        else { g.P_lo = V(pl); g.Q_lo = V(ql); }
        TNCall call;
        call.M = Mr; call.scratch = partial; call.scratch_bytes = kTnScratchBytes;
        return launch_gemm_tn(!one ? kTNPair : bf16 ? kTNPlaneBf16 : kTNPlaneF16, g, call, st);
    };
    auto head = [&] {   // dhn, and the head's weight / bias gradients
        if (one) {
            launch_fa_head_bwd(dlogits, F(p.hn), prm(hb + 2), grd(hb + 2), grd(hb + 3), F(p.dhn), c.batch, D, c.num_classes, st, bf16);
            return;
        }
        const int64_t n = (int64_t)c.num_classes * D + (int64_t)c.batch * D + c.num_classes;
        k_fs_head_bwd<<<(int)((n + 255) / 256), 256, 0, st>>>(reinterpret_cast<const float*>(dlogits), F(p.hn), prm(hb + 2), grd(hb + 2), grd(hb + 3), F(p.dhn),
                                                              c.batch, D, c.num_classes);
    };
    auto gelu_bwd = [&](const FsBlock& k) {   // dY1 = dG * gelu'(Y1)
        if (one) return launch_fa_gelu_bwd(F(p.dG), F(k.Y1), V(p.dY1_hi), M * Hd, st, bf16);
        return launch_mask_bwd(1, F(p.dG), F(k.Y1), qp_off, 0, 255, nullptr, Hd, V(p.dY1_hi), V(p.dY1_lo), M * Hd, st);
    };
    auto attn_bwd = [&](const FsBlock& k) {   // dqkv from dO
        if (one) return launch_attn_bwd_f16(F(k.qkv), V(k.O_hi), F(k.lse), F(p.dO), c.batch, T, H, D, V(p.dqkv_hi), st, bf16);
        return launch_attn_bwd_float(F(k.qkv), V(k.O_hi), V(k.O_lo), F(k.lse), F(p.dO), c.batch, T, H, D, F(p.Pm), F(p.dS), F(p.delta), V(p.dqkv_hi),
                                     V(p.dqkv_lo), st);
    };
    auto embed_bwd = [&] {   // pos / cls gradients and dY0 (the patch rows of dx)
        if (one) launch_fa_embed_bwd(F(p.dx), grd(3), grd(2), V(p.dY0_hi), c.batch, T, D, st, bf16);
        else launch_embed_bwd(F(p.dx), F(p.Y0), qp_off, 0, 255, grd(3), grd(2), V(p.dY0_hi), V(p.dY0_lo), c.batch, T, D, st);
    };
    auto fp16_overflow = [&] {   // the fp16 form: the overflow rule of the fp16 Linear / Conv2d weight and bias gradients (bf16 has fp32's range)
        if (!f16) return;
        float* g[2 * kMaxW];
        int64_t n[2 * kMaxW];
        int count = 0;
        for (int wi = 0; wi < 2 + 4 * L; ++wi) {
            int N, K;
            fs_weight_shape(c, wi, &N, &K);
            const int pi = fs_weight_param(c, wi);
            g[count] = grd(pi); n[count++] = (int64_t)N * K;
            g[count] = grd(pi + 1); n[count++] = N;
        }
        launch_fa_inf_rule(g, n, count, st);
    };
    // the LayerNorm backward's second output: the residual gradient as the next branch's GEMM operand dp (mask all ones; the fp16 form: unit multiplier;
    // the bf16 form: no lo plane, so one bf16 plane)
    LnBwdNext next{V(p.ones), nullptr, V(p.dp_hi), V(p.dp_lo), f16 ? unit : nullptr, reinterpret_cast<uint32_t*>(V(p.amax))};
    // drop-path (the table the forward read): dp also carries the multipliers of the branch it enters - block i's attention (mlp = 0) or MLP (1) branch
    const float* const drop = drop_path_of(workspace);
    const std::shared_ptr<const LayerScale> ls = layer_scale_of(workspace);
    QV_CHECK_ARG(!ls || ((int)ls->gamma.size() == 2 * c.depth && ls->grad.size() == ls->gamma.size() && ls->saved),
                 "%s: the LayerScale binding needs 2 * depth gammas, their gradient buffers and the saved-branch buffer", fn);
    // The fp16 form under LayerScale.  Stock autocast holds every gradient inside a branch in fp16, and each of them carries the branch's gamma: at
    // gamma = 1e-5, timm's initial value, they lie in or under fp16's subnormal range, and every gradient in front of a branch loses its digits (stock
    // autocast without a loss scale: 5e-2 - 7e-2 relative).  Here the branch's gradients travel multiplied by K, a power of two of the order of
    // 1 / max |gamma| (launch_fs_ls_scales: exact to apply and to undo): the LayerNorm backward writes dp * K, the GEMMs, the GELU backward and the attention
    // backward are linear in it, and the four weight gradients and the dgrad that leaves the branch undo it through the GEMMs' scalar (1 / K).  K = 1 for
    // max |gamma| >= 0.5 (ls_scales.hip).  {K, 1 / K} per branch stand behind the branch outputs in the binding's saved buffer.
    float* const lsK = f16 && ls ? ls->saved + (int64_t)2 * L * M * D : nullptr;
    if (lsK) {
        QV_CHECK_ARG(2 * L <= 24, "%s: LayerScale scales cover depth <= 12", fn);
        if (launch_fs_ls_scales(ls->gamma.data(), 2 * L, D, lsK, st)) return 1;
    }
    auto inv_of = [&](int i, int mlp) -> const float* { return lsK ? lsK + 2 * (2 * i + mlp) + 1 : nullptr; };
    auto next_of = [&](int i, int mlp) {
        next.drop_scale = drop ? drop + (int64_t)(2 * i + mlp) * c.batch : nullptr;
        next.drop_rows = T;
        if (lsK) next.o16_mul = lsK + 2 * (2 * i + mlp);
        if (ls) {   // LayerScale: dp also carries the branch's gamma, and the kernel that writes it completes gamma's gradient from the branch output the forward kept
            const int k = 2 * i + mlp;
            next.ls_gamma = ls->gamma[k]; next.ls_dgamma = ls->grad[k]; next.ls_Y = ls->saved + (int64_t)k * M * D; next.ls_ymul = 1;
            next.ls_qp = nullptr; next.ls_kind = f16 ? 1 : bf16 ? 2 : 0;
        }
        return &next;
    };
    // head, then the final norm on the cls rows (dx of every other row = 0); the residual gradient leaves as fp32 (dx) and as dp
    head();
    if (launch_ln_bwd_fq(0, F(p.dhn), F(p.x_last), F(p.meanf), F(p.rstdf), prm(hb), prm(hb + 1), qp_off, 0, 255, nullptr, F(p.dx), grd(hb), grd(hb + 1), M, D, T,
                         1, st, next_of(L - 1, 1)))
        return 1;
    for (int i = L - 1; i >= 0; --i) {
        const FsBlock& k = p.blk[i];
        const int w0 = 1 + 4 * i, g0 = 4 + 12 * i;
        // fc2 (input G = gelu(Y1)), then GELU' on the fc1 pre-activation
        const float* const im = inv_of(i, 1), * const ia = inv_of(i, 0);   // (1 / K of the MLP and of the attention branch, nullptr: the unit)
        if (wgrad(p.dp_hi, p.dp_lo, k.G_hi, k.G_lo, grd(g0 + 10), grd(g0 + 11), D, Hd, (int)M, im)) return 1;
        if (dgrad(p.dp_hi, p.dp_lo, w0 + 3, F(p.dG), Hd, D)) return 1;
        if (gelu_bwd(k)) return 1;
        // fc1 (input h2 = norm2(xm)), norm2 backward + the residual: dx2 = dx + LNbwd(dh2), and its dp for proj
        if (wgrad(p.dY1_hi, p.dY1_lo, k.h2_hi, k.h2_lo, grd(g0 + 8), grd(g0 + 9), Hd, D, (int)M, im)) return 1;
        if (dgrad(p.dY1_hi, p.dY1_lo, w0 + 2, F(p.dh), D, Hd, im)) return 1;
        if (launch_ln_bwd_fq(1, F(p.dh), F(k.xm), F(k.mean2), F(k.rstd2), prm(g0 + 6), prm(g0 + 7), qp_off, 0, 255, F(p.dx), F(p.dx2), grd(g0 + 6), grd(g0 + 7), M,
                             D, T, 0, st, next_of(i, 0)))
            return 1;
        // proj (input O), attention, qkv (input h1 = norm1(x)); norm1 backward: dx = dx2 + LNbwd(dh1), the gradient of the block's input
        if (wgrad(p.dp_hi, p.dp_lo, k.O_hi, k.O_lo, grd(g0 + 4), grd(g0 + 5), D, D, (int)M, ia)) return 1;
        if (dgrad(p.dp_hi, p.dp_lo, w0 + 1, F(p.dO), D, D)) return 1;
        if (attn_bwd(k)) return 1;
        if (wgrad(p.dqkv_hi, p.dqkv_lo, k.h1_hi, k.h1_lo, grd(g0 + 2), grd(g0 + 3), 3 * D, D, (int)M, ia)) return 1;
        if (dgrad(p.dqkv_hi, p.dqkv_lo, w0 + 0, F(p.dh), D, 3 * D, ia)) return 1;
        if (launch_ln_bwd_fq(1, F(p.dh), F(k.x), F(k.mean1), F(k.rstd1), prm(g0 + 0), prm(g0 + 1), qp_off, 0, 255, F(p.dx2), F(p.dx), grd(g0 + 0), grd(g0 + 1), M,
                             D, T, 0, st, i > 0 ? next_of(i - 1, 1) : nullptr))
            return 1;
    }
    // embedding, then the patch-embedding weight gradient over the saved patches
    embed_bwd();
    if (lsK) {   // (the fp16 form under LayerScale: the patch-embedding gradient's operand at the branches' scale, see above)
        if (launch_fs_ls_dy0(F(p.dx), V(p.dY0_hi), c.batch, T, D, lsK, 2 * L, st)) return 1;
    }
    if (wgrad(p.dY0_hi, p.dY0_lo, p.p_hi, p.p_lo, grd(0), grd(1), D, Kpe, c.batch * np, lsK ? lsK + 4 * L + 1 : nullptr)) return 1;
    fp16_overflow();
    QV_CHECK_LAUNCH(fn);
    return 0;
}

// ---------------------------------------------------------------- the C ABI (include/qatvit.h)
int64_t qatvit_float_student_workspace_bytes(const qatvit_cfg* cfg) { return fs_workspace_bytes("qatvit_float_student_workspace_bytes", FsForm::pair, cfg); }

int qatvit_float_student_init(const qatvit_cfg* cfg, void* workspace, void* stream) {
    return fs_init("qatvit_float_student_init", FsForm::pair, cfg, workspace, stream);
}

int qatvit_float_student_forward(const qatvit_cfg* cfg, void* const* params, const float* images, float* logits, void* workspace, void* stream) {
    return fs_forward("qatvit_float_student_forward", FsForm::pair, cfg, params, images, logits, workspace, nullptr, stream);
}

int qatvit_float_student_backward(const qatvit_cfg* cfg, void* const* params, const float* dlogits, void* const* grads, void* workspace, void* stream) {
    return fs_backward("qatvit_float_student_backward", FsForm::pair, cfg, params, dlogits, grads, workspace, stream);
}

int64_t qatvit_float_student_amp_workspace_bytes(const qatvit_cfg* cfg) {
    return fs_workspace_bytes("qatvit_float_student_amp_workspace_bytes", FsForm::f16, cfg);
}

int qatvit_float_student_amp_init(const qatvit_cfg* cfg, void* workspace, void* stream) {
    return fs_init("qatvit_float_student_amp_init", FsForm::f16, cfg, workspace, stream);
}

int qatvit_float_student_amp_forward(const qatvit_cfg* cfg, void* const* params, const float* images, void* logits_f16, void* workspace, void* stream) {
    return fs_forward("qatvit_float_student_amp_forward", FsForm::f16, cfg, params, images, logits_f16, workspace, nullptr, stream);
}

int qatvit_float_student_amp_backward(const qatvit_cfg* cfg, void* const* params, const void* dlogits_f16, void* const* grads, void* workspace, void* stream) {
    return fs_backward("qatvit_float_student_amp_backward", FsForm::f16, cfg, params, dlogits_f16, grads, workspace, stream);
}

int64_t qatvit_float_student_bf16_workspace_bytes(const qatvit_cfg* cfg) {
    return fs_workspace_bytes("qatvit_float_student_bf16_workspace_bytes", FsForm::bf16, cfg);
}

int qatvit_float_student_bf16_init(const qatvit_cfg* cfg, void* workspace, void* stream) {
    return fs_init("qatvit_float_student_bf16_init", FsForm::bf16, cfg, workspace, stream);
}

int qatvit_float_student_bf16_forward(const qatvit_cfg* cfg, void* const* params, const float* images, void* logits_bf16, void* workspace, void* stream) {
    return fs_forward("qatvit_float_student_bf16_forward", FsForm::bf16, cfg, params, images, logits_bf16, workspace, nullptr, stream);
}

int qatvit_float_student_bf16_backward(const qatvit_cfg* cfg, void* const* params, const void* dlogits_bf16, void* const* grads, void* workspace, void* stream) {
    return fs_backward("qatvit_float_student_bf16_backward", FsForm::bf16, cfg, params, dlogits_bf16, grads, workspace, stream);
}

int64_t qatvit_float_student_observe_bytes(const qatvit_cfg* cfg) {
    if (!cfg) { set_error("qatvit_float_student_observe_bytes: null argument"); return -1; }
    if (fs_check(*cfg, FsForm::pair)) return -1;
    return obs_plan(*cfg).total;
}

int qatvit_float_student_observe_init(const qatvit_cfg* cfg, const qatvit_fq* act_fq, const qatvit_fq* weight_fq, void* observe, void* stream) {
    QV_CHECK_ARG(cfg && act_fq && weight_fq && observe, "qatvit_float_student_observe_init: null argument");
    if (fs_check(*cfg, FsForm::pair)) return 1;
    const qatvit_cfg& c = *cfg;
    const ObsPlan p = obs_plan(c);
    char* ob = reinterpret_cast<char*>(observe);
    uint32_t* stats = reinterpret_cast<uint32_t*>(ob + p.act_stats);
    ObsFoldEntry tab[4 + 6 * 12 + 2 + 4 * 12];
    int blk = 0;
    for (int ai = 0; ai < p.n_act; ++ai) {
        const qatvit_fq& f = act_fq[ai];
        tab[ai] = ObsFoldEntry{stats + (int64_t)ai * kStatSlots * kStatStride, f.min_val, f.max_val, f.scale, f.zero_point, f.observer_on, f.fake_quant_on,
                               1, kStatSlots, 0, c.act_qmin, c.act_qmax, blk};
        blk += 1;
    }
    for (int wi = 0; wi < p.n_w; ++wi) {
        const qatvit_fq& f = weight_fq[wi];
        int N, K;
        fs_weight_shape(c, wi, &N, &K);
        tab[p.n_act + wi] = ObsFoldEntry{stats + p.w_stats[wi], f.min_val, f.max_val, f.scale, f.zero_point, f.observer_on, f.fake_quant_on,
                                         c.w_per_channel ? N : 1, c.w_per_channel ? 1 : kStatSlots, 1, c.w_qmin, c.w_qmax, blk};
        blk += c.w_per_channel ? (N + 63) / 64 : 1;
    }
    hipStream_t st = (hipStream_t)stream;
    if (hipMemcpyAsync(ob + p.tab, tab, sizeof(ObsFoldEntry) * (p.n_act + p.n_w), hipMemcpyHostToDevice, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess) {   // (once per buffer: the host table is gone after this call)
        set_error("qatvit_float_student_observe_init: copying the fold table failed");
        return 2;
    }
    launch_ws_init(stats, p.stats_words / 2, st);
    QV_CHECK_LAUNCH("qatvit_float_student_observe_init");
    return 0;
}

int qatvit_float_student_forward_observe(const qatvit_cfg* cfg, void* const* params, const float* images, float* logits, void* workspace, void* observe,
                                         void* stream) {
    QV_CHECK_ARG(observe, "qatvit_float_student_forward_observe: null argument");
    return fs_forward("qatvit_float_student_forward_observe", FsForm::pair, cfg, params, images, logits, workspace, observe, stream);
}

}  // extern "C"
