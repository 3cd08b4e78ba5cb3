// HBM-bound fused stages between the GEMMs of the QAT student step (gfx950).
//
// Fake-quant needs the tensor's min/max before it can quantize (EMA observer,
// torch/ao/quantization/observer.py:668-683), so every activation quantizer is split as
//   producer (GEMM epilogue or a kernel here): writes the pre-FQ fp32 tensor + min/max atomics
//   k_qparams (fq.hip): EMA + scale/zero_point, publishes {scale, 1/scale, zp, enabled}
//   consumer (a kernel here, or a GEMM/attention loader): quantizes on load.
// Backward never stores masks: the STE mask (qmin <= rint(x/s)+zp <= qmax) is recomputed from the
// saved pre-FQ tensor and the module's (scale, zp), which stay valid until the next forward.
// Row kernels: one wave per row, 16 B per lane per load; all are single-pass over HBM.
#include <stdlib.h>

#include <algorithm>

#include "qv_common.h"
#include "qv_device.h"
#include "qv_kernels.h"
#include "qv_qparams.h"

namespace qv {

struct QP { float s, inv, zp, on; };
__device__ inline QP load_qp(const float* qp) { return QP{qp[0], qp[1], qp[2], qp[3]}; }
// fake-quantized value and in-range flag
__device__ inline float fqv(float x, const QP& q, float fqmin, float fqmax, bool& in) {
    const float t = rintf(x * q.inv) + q.zp;
    in = (t >= fqmin && t <= fqmax) || q.on == 0.f;
    const float y = (fminf(fmaxf(t, fqmin), fqmax) - q.zp) * q.s;
    return q.on != 0.f ? y : x;
}
// grid integer q - zp (exact in bf16, |.| <= 255)
__device__ inline float fqi(float x, const QP& q, float fqmin, float fqmax) {
    return fminf(fmaxf(rintf(x * q.inv) + q.zp, fqmin), fqmax) - q.zp;
}

// float operand of a later GEMM -> (hi, lo) bf16 pair, 4 elements (through split_pair; teacher.hip's st_split4 casts per element and has an fp16 branch)
__device__ inline void store_split4(__bf16* hi, __bf16* lo, int64_t off, float a, float b, float c, float d) {
    uint2 h, l;
    split_pair(a, b, h.x, l.x);
    split_pair(c, d, h.y, l.y);
    *reinterpret_cast<uint2*>(hi + off) = h;
    *reinterpret_cast<uint2*>(lo + off) = l;
}

// the one-plane backward: four gradient elements -> one fp16 plane (value * mul), running max |value| in am
__device__ inline void store_f16x4(__bf16* plane, int64_t off, float a, float b, float c, float d, float mul, float& am) {
    am = fmaxf(fmaxf(am, fmaxf(fabsf(a), fabsf(b))), fmaxf(fabsf(c), fabsf(d)));
    *reinterpret_cast<uint2*>(plane + off) = make_uint2(pk_f16(a * mul, b * mul), pk_f16(c * mul, d * mul));
}
__device__ inline void amax_publish(uint32_t* amax, float am, int lane) {   // one atomic per wave into the workgroup's sub-slot (dy16.hip)
    am = wave_max(am);
    if (lane == 0) atomicMax(amax + (blockIdx.x & (kDyAmaxSlots - 1)) * kDyAmaxStride, __builtin_bit_cast(uint32_t, am));
}

static inline int rows_grid(int64_t rows) {
    int64_t b = (rows + 3) / 4;
    return (int)(b < 1 ? 1 : (b > 2048 ? 2048 : b));
}
static inline int flat_grid(int64_t n4) {
    int64_t b = (n4 + 255) / 256;
    return (int)(b < 1 ? 1 : (b > 4096 ? 4096 : b));
}

// ---------------------------------------------------------------- K0: image -> patch rows
// out[(b*gh+py)*gw+px][c*P*P + i*P + j] = q(img[b][c][py*P+i][px*P+j]) - zp   (bf16)
__global__ __launch_bounds__(256) void k_img_patches(const float* __restrict__ img, __bf16* __restrict__ out, const float* __restrict__ qp,
                                                     int qmin, int qmax, int B, int C, int H, int W, int P, int8_t* __restrict__ out8, int center) {
    const QP q = load_qp(qp);
    const int gw = W / P, gh = H / P, K = C * P * P;
    const int64_t n8 = (int64_t)B * gh * gw * K / 8;
    for (int64_t e8 = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e8 < n8; e8 += (int64_t)gridDim.x * blockDim.x) {
        const int64_t e = e8 * 8;
        const int col = (int)(e % K);
        const int64_t prow = e / K;
        const int px = (int)(prow % gw), py = (int)((prow / gw) % gh), b = (int)(prow / ((int64_t)gw * gh));
        const int j = col % P, i = (col / P) % P, c = col / (P * P);
        const float* src = img + (((int64_t)b * C + c) * H + py * P + i) * W + px * P + j;
        const float4 a = reinterpret_cast<const float4*>(src)[0], bb = reinterpret_cast<const float4*>(src)[1];
        bf16x8 o;
        o[0] = (__bf16)fqi(a.x, q, qmin, qmax); o[1] = (__bf16)fqi(a.y, q, qmin, qmax);
        o[2] = (__bf16)fqi(a.z, q, qmin, qmax); o[3] = (__bf16)fqi(a.w, q, qmin, qmax);
        o[4] = (__bf16)fqi(bb.x, q, qmin, qmax); o[5] = (__bf16)fqi(bb.y, q, qmin, qmax);
        o[6] = (__bf16)fqi(bb.z, q, qmin, qmax); o[7] = (__bf16)fqi(bb.w, q, qmin, qmax);
        if (out) *reinterpret_cast<bf16x8*>(out + e) = o;
        if (out8) {
            const float sh = q.zp - (float)center;
            signed char c8[8];
#pragma unroll
            for (int t = 0; t < 8; ++t) c8[t] = (signed char)((float)o[t] + sh);
            uint2 pk;
            __builtin_memcpy(&pk, c8, 8);
            *reinterpret_cast<uint2*>(out8 + e) = pk;
        }
    }
}

constexpr int kMaxV = 3;  // float4 per lane per row: D <= 768
#define QV_DP 0
#include "elt_rows.inc"
#undef QV_DP

// h_q[row][c] = q(LN(x)[row][c]) - zp  as bf16 (the exact A operand of the following GEMM)
__global__ __launch_bounds__(256) void k_ln_apply_quant(const float* __restrict__ x, const float* __restrict__ mean, const float* __restrict__ rstd,
                                                        const float* __restrict__ gamma, const float* __restrict__ beta, const float* __restrict__ qp,
                                                        int qmin, int qmax, __bf16* __restrict__ out, int64_t M, int D,
                                                        int8_t* __restrict__ out8, int center, int out_f16, const QpLate late) {
    // out = q - zp as bf16 (the exact operand of the weight-gradient GEMM); out8 (optional) = q - center as int8 (the operand of the
    // int8-MFMA forward GEMM)
    __shared__ float sQp[4];
    QP q;
    if (late.stats) { const float4 r = qp_late_resolve(late, sQp); q = QP{r.x, r.y, r.z, r.w}; }   // (QpLate: no k_qparams launch in front of this kernel)
    else q = load_qp(qp);
    const int d4 = D / 4;
    const int64_t n4 = M * d4;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = i / d4;
        const int c = (int)(i % d4) * 4;
        const float mu = mean[row], rs = rstd[row];
        const float4 v = *reinterpret_cast<const float4*>(x + row * D + c);
        const float4 g = *reinterpret_cast<const float4*>(gamma + c), b = *reinterpret_cast<const float4*>(beta + c);
        bf16x4 o;
        o[0] = (__bf16)fqi((v.x - mu) * rs * g.x + b.x, q, qmin, qmax);
        o[1] = (__bf16)fqi((v.y - mu) * rs * g.y + b.y, q, qmin, qmax);
        o[2] = (__bf16)fqi((v.z - mu) * rs * g.z + b.z, q, qmin, qmax);
        o[3] = (__bf16)fqi((v.w - mu) * rs * g.w + b.w, q, qmin, qmax);
        // out_f16 (uniform): the same integers as fp16 bit patterns - the X operand of the one-plane weight gradient (|q - zp| <= 255: exact either way)
        // out == nullptr (uniform): nobody reads the 2-byte plane - the forward GEMM and the one-plane weight gradient both take out8
        if (out && out_f16) *reinterpret_cast<uint2*>(out + row * D + c) = make_uint2(pk_f16((float)o[0], (float)o[1]), pk_f16((float)o[2], (float)o[3]));
        else if (out) *reinterpret_cast<bf16x4*>(out + row * D + c) = o;
        if (out8) {
            const float sh = q.zp - (float)center;
            char4 o8 = make_char4((signed char)((float)o[0] + sh), (signed char)((float)o[1] + sh), (signed char)((float)o[2] + sh),
                                  (signed char)((float)o[3] + sh));
            *reinterpret_cast<char4*>(out8 + row * D + c) = o8;
        }
    }
}

// ---------------------------------------------------------------- inference: LayerNorm + quantise in one pass
// out8[row][c] = q(LN(x)[row][c]) - center as int8 with FROZEN qparams (no observer statistics: nothing depends on a global min/max, so the
// row statistics, the normalisation and the quantisation fuse into one read of x).  The arithmetic is the training path's, operation for
// operation - row sum / centred sum of squares in k_resid_fq_lnstats' order, ((x - mu) * rstd) * gamma + beta as in k_ln_apply_quant - so
// the codes equal the fake-quant forward's bit for bit.  row_stride > 1 visits rows 0, row_stride, 2 row_stride, .. only (cls tokens);
// out8 == nullptr: statistics only (mean / rstd for k_head_fwd).
template <int NV>
__global__ __launch_bounds__(256) void k_ln_quant8(const float* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                   const float* __restrict__ qp, int qmin, int qmax, int center, int8_t* __restrict__ out8,
                                                   float* __restrict__ mean, float* __restrict__ rstd, int64_t nrows, int64_t row_stride, int D) {
    const QP q = load_qp(qp);
    const int lane = threadIdx.x & 63;
    bool act[NV];
    int cc[NV];
    float4 g[NV], bb[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const int c = lane * 4 + 256 * j;
        act[j] = c < D;
        cc[j] = act[j] ? c : 0;
        g[j] = *reinterpret_cast<const float4*>(gamma + cc[j]);
        bb[j] = *reinterpret_cast<const float4*>(beta + cc[j]);
    }
    const float sh = q.zp - (float)center;
    for (int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < nrows; i += (int64_t)gridDim.x * 4) {
        const int64_t row = i * row_stride;
        float4 v[NV];
#pragma unroll
        for (int j = 0; j < NV; ++j) v[j] = *reinterpret_cast<const float4*>(x + row * D + cc[j]);
#pragma unroll
        for (int j = 0; j < NV; ++j) pin4(v[j]);
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < NV; ++j)
            if (act[j]) s += (v[j].x + v[j].y) + (v[j].z + v[j].w);
        const float mu = wave_sum(s) / (float)D;
        float qq = 0.f;
        float4 cv[NV];
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            cv[j] = make_float4(v[j].x - mu, v[j].y - mu, v[j].z - mu, v[j].w - mu);
            if (act[j]) qq += (cv[j].x * cv[j].x + cv[j].y * cv[j].y) + (cv[j].z * cv[j].z + cv[j].w * cv[j].w);
        }
        const float rs = rsqrtf(wave_sum(qq) / (float)D + eps);
        if (mean && lane == 0) { mean[row] = mu; rstd[row] = rs; }
        if (out8) {
#pragma unroll
            for (int j = 0; j < NV; ++j) {
                if (act[j]) {
                    const char4 o = make_char4((signed char)(fqi(cv[j].x * rs * g[j].x + bb[j].x, q, qmin, qmax) + sh),
                                               (signed char)(fqi(cv[j].y * rs * g[j].y + bb[j].y, q, qmin, qmax) + sh),
                                               (signed char)(fqi(cv[j].z * rs * g[j].z + bb[j].z, q, qmin, qmax) + sh),
                                               (signed char)(fqi(cv[j].w * rs * g[j].w + bb[j].w, q, qmin, qmax) + sh));
                    *reinterpret_cast<char4*>(out8 + row * D + cc[j]) = o;
                }
            }
        }
    }
}

// x[b, 0, :] = cls + pos[0]   (the class-token rows of the embedded sequence; the patch rows come from the patch-embedding GEMM's epilogue)
__global__ __launch_bounds__(256) void k_cls_rows(const float* __restrict__ cls, const float* __restrict__ pos, float* __restrict__ x, int B, int T, int D) {
    const int64_t n = (int64_t)B * D;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int b = (int)(i / D), c = (int)(i % D);
        x[(int64_t)b * T * D + c] = cls[c] + pos[c];
    }
}


// ---------------------------------------------------------------- head (cls pooling): tiny kernels, one block per image
// hq[b,:] = q(LN(x[b,0,:])) - zp ; logits_pre[b,c] = s_a*s_w[c] * sum_k hq[k]*wq[c,k] + bias[c]; stats of logits_pre
__global__ __launch_bounds__(256) void k_head_fwd(const float* __restrict__ x, const float* __restrict__ mean, const float* __restrict__ rstd,
                                                  const float* __restrict__ gamma, const float* __restrict__ beta, const float* __restrict__ qp_norm,
                                                  int qmin, int qmax, const __bf16* __restrict__ wq, const float* __restrict__ w_scale,
                                                  int w_per_channel, const float* __restrict__ bias, float* __restrict__ hq_out,
                                                  float* __restrict__ logits_pre, uint32_t* __restrict__ stats, int stat_slots, int D, int T, int C) {
    extern __shared__ float sh[];  // D floats
    const QP q = load_qp(qp_norm);
    const int b = blockIdx.x;
    const int64_t row = (int64_t)b * T;
    const float mu = mean[row], rs = rstd[row];
    for (int c = threadIdx.x; c < D; c += blockDim.x) {
        const float h = fqi((x[row * D + c] - mu) * rs * gamma[c] + beta[c], q, qmin, qmax);
        sh[c] = h;
        hq_out[(int64_t)b * D + c] = h;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int c = wave; c < C; c += 4) {
        float acc = 0.f;
        for (int k = lane; k < D; k += 64) acc += sh[k] * (float)wq[(int64_t)c * D + k];  // exact integers in fp32
        acc = wave_sum(acc);
        if (lane == 0) {
            const float v = acc * (q.s * w_scale[w_per_channel ? c : 0]) + bias[c];
            logits_pre[(int64_t)b * C + c] = v;
            stat_atomic(stats, stat_slots, v, v);
        }
    }
}

__global__ void k_logits_fq(const float* __restrict__ pre, const float* __restrict__ qp, int qmin, int qmax, float* __restrict__ out, int n) {
    const QP q = load_qp(qp);
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        bool in;
        out[i] = fqv(pre[i], q, qmin, qmax, in);
    }
}

// dl = dlogits * mask(logits_pre); dW[c,:] += sum_b dl[b,c]*hq[b,:]*s_norm (masked by the weight FQ); db[c] += sum_b dl;
// dh[b,:] = sum_c dl[b,c] * wq[c,:] * s_w[c]     (gradient w.r.t. the fake-quantized final-norm output, cls rows)
__global__ __launch_bounds__(256) void k_head_bwd(const float* __restrict__ dlogits, const float* __restrict__ logits_pre, const float* __restrict__ qp_logits,
                                                  int qmin, int qmax, const float* __restrict__ hq, const float* __restrict__ qp_norm,
                                                  const __bf16* __restrict__ wq, const float* __restrict__ W, const float* __restrict__ w_scale,
                                                  const int32_t* __restrict__ w_zp, int w_per_channel, int w_qmin, int w_qmax,
                                                  float* __restrict__ dW, float* __restrict__ dbias, float* __restrict__ dh, int B, int D, int C) {
    // grid: C * ceil(D/64) + B blocks: the first group computes dW[c][64-column chunk] (and db[c]); the last B blocks compute dh row b.
    // dW: 64 columns x 4 batch groups per block, the groups reduced through LDS in a fixed order (no atomics)
    const QP ql = load_qp(qp_logits);
    const int kch = (D + 63) / 64;
    if ((int)blockIdx.x < C * kch) {
        const int c = blockIdx.x / kch, k = (blockIdx.x % kch) * 64 + (threadIdx.x & 63), grp = threadIdx.x >> 6;
        const float s_norm = qp_norm[0];
        const int ci = w_per_channel ? c : 0;
        const float inv = __fdiv_rn(1.0f, w_scale[ci]), fzp = (float)w_zp[ci];
        float acc = 0.f, dbacc = 0.f;
        const int bper = (B + 3) / 4, b_lo = grp * bper, b_hi = min(B, b_lo + bper);
        if (k < D) {
            for (int b = b_lo; b < b_hi; ++b) {
                bool in;
                fqv(logits_pre[(int64_t)b * C + c], ql, qmin, qmax, in);
                const float dl = in ? dlogits[(int64_t)b * C + c] : 0.f;
                acc += dl * hq[(int64_t)b * D + k];
                dbacc += dl;
            }
        }
        __shared__ float sacc[4][64], sdb[4];
        sacc[grp][threadIdx.x & 63] = acc;
        if ((threadIdx.x & 63) == 0) sdb[grp] = dbacc;
        __syncthreads();
        if (grp == 0 && k < D) {
            const float tot = ((sacc[0][threadIdx.x] + sacc[1][threadIdx.x]) + sacc[2][threadIdx.x]) + sacc[3][threadIdx.x];
            const float t = rintf(W[(int64_t)c * D + k] * inv) + fzp;
            const bool win = t >= (float)w_qmin && t <= (float)w_qmax;
            dW[(int64_t)c * D + k] = win ? tot * s_norm : 0.f;
            if (k == 0) dbias[c] = ((sdb[0] + sdb[1]) + sdb[2]) + sdb[3];
        }
    } else {
        const int b = blockIdx.x - C * kch;
        for (int k = threadIdx.x; k < D; k += blockDim.x) {
            float acc = 0.f;
            for (int c = 0; c < C; ++c) {
                bool in;
                fqv(logits_pre[(int64_t)b * C + c], ql, qmin, qmax, in);
                const float dl = in ? dlogits[(int64_t)b * C + c] : 0.f;
                acc += dl * (float)wq[(int64_t)c * D + k] * w_scale[w_per_channel ? c : 0];
            }
            dh[(int64_t)b * D + k] = acc;
        }
    }
}

// ---------------------------------------------------------------- embedding backward
// dx0 [B,T,D] -> dpos[t,:] = sum_b dx0[b,t,:]; dcls = sum_b dx0[b,0,:]; dY0[b*np+p,:] = dx0[b,1+p,:] * mask(Y0)
__global__ __launch_bounds__(64) void k_embed_bwd(const float* __restrict__ dx0, const float* __restrict__ Y0, const float* __restrict__ qp,
                                                  int qmin, int qmax, float* __restrict__ dpos, float* __restrict__ dcls,
                                                  __bf16* __restrict__ dY0_hi, __bf16* __restrict__ dY0_lo, int B, int T, int D) {
    // one thread per (token, 4 columns), summing over the batch in a fixed order (no atomics); only T*D/4 threads exist, so blocks are one
    // wave (every CU gets work) and each thread keeps UNR images' loads in flight
    const QP q = load_qp(qp);
    const int d4 = D / 4;
    const int64_t n4 = (int64_t)T * d4;
    constexpr int UNR = 16;   // (about one wave per CU exists, so the kernel is UNR-deep round trips over the batch: 8 -> 16 halves them)
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        const int t = (int)(i / d4), c = (int)(i % d4) * 4;
        const int ty = t > 0 ? t - 1 : 0;     // (branch-free: the class-token row reads patch 0 and ignores it)
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int b0 = 0; b0 < B; b0 += UNR) {
            float4 g[UNR], y[UNR];
#pragma unroll
            for (int u = 0; u < UNR; ++u) {
                const int b = b0 + u < B ? b0 + u : B - 1;
                g[u] = *reinterpret_cast<const float4*>(dx0 + ((int64_t)b * T + t) * D + c);
                y[u] = *reinterpret_cast<const float4*>(Y0 + ((int64_t)b * (T - 1) + ty) * D + c);
            }
#pragma unroll
            for (int u = 0; u < UNR; ++u) { pin4(g[u]); pin4(y[u]); }
#pragma unroll
            for (int u = 0; u < UNR; ++u) {
                if (b0 + u < B) {
                    acc.x += g[u].x; acc.y += g[u].y; acc.z += g[u].z; acc.w += g[u].w;
                    if (t > 0) {
                        bool i0, i1, i2, i3;
                        fqv(y[u].x, q, qmin, qmax, i0); fqv(y[u].y, q, qmin, qmax, i1); fqv(y[u].z, q, qmin, qmax, i2); fqv(y[u].w, q, qmin, qmax, i3);
                        store_split4(dY0_hi, dY0_lo, ((int64_t)(b0 + u) * (T - 1) + (t - 1)) * D + c, i0 ? g[u].x : 0.f, i1 ? g[u].y : 0.f,
                                     i2 ? g[u].z : 0.f, i3 ? g[u].w : 0.f);
                    }
                }
            }
        }
        *reinterpret_cast<float4*>(dpos + (int64_t)t * D + c) = acc;
        if (t == 0) *reinterpret_cast<float4*>(dcls + c) = acc;
    }
}

// ---------------------------------------------------------------- weight fake-quant -> GEMM operands
// wq[n][k] = q(W[n][k]) - zp (bf16), wqT[k][n] = same, transposed (dgrad's B operand)
__device__ inline void wquant_body(const float* __restrict__ W, const float* __restrict__ qp, int per_channel, int qmin, int qmax,
                                   __bf16* __restrict__ wq, __bf16* __restrict__ wqT, int N, int K, int bx, int by,
                                   int8_t* __restrict__ w8 = nullptr, int32_t* __restrict__ wsum = nullptr, _Float16* __restrict__ w16 = nullptr,
                                   int8_t* __restrict__ w8f = nullptr, int64_t wT16_gap = 0,   // wT16_gap: byte distance from wqT to its fp16 twin (0: none)
                                   bool wT16_frag = false) {   // ... followed, another gap further, by the same fp16 integers in MFMA fragment order (f16strip.hip's B operand)
    // 32x32 tile transpose through LDS
    __shared__ float tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
    const int n0 = by * 32, k0 = bx * 32;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int n = n0 + ty + 8 * i, k = k0 + tx;
        float v = 0.f;
        if (n < N && k < K) {
            const QP q = load_qp(qp + 4 * (per_channel ? n : 0));
            v = q.on != 0.f ? fqi(W[(int64_t)n * K + k], q, qmin, qmax) : W[(int64_t)n * K + k];
            wq[(int64_t)n * K + k] = (__bf16)v;
            if (w8) w8[(int64_t)n * K + k] = (int8_t)v;   // the same integer for the int8-MFMA forward GEMMs
            if (w16) w16[(int64_t)n * K + k] = (_Float16)v;   // ... and for the fp16-pair forward GEMMs (|v| <= 128: exact)
            if (w8f) w8f[w8f_offset(n, k, K)] = (int8_t)v;    // ... and in MFMA-fragment order for the strip kernel (i8strip.hip)
        }
        tile[ty + 8 * i][tx] = v;
    }
    __syncthreads();
    if (wsum && threadIdx.x < 32 && n0 + (int)threadIdx.x < N) {   // row sums of the integers (zero-point correction of the int8 GEMM)
        float sacc = 0.f;
#pragma unroll
        for (int k = 0; k < 32; ++k) sacc += tile[threadIdx.x][k];
        atomicAdd(&wsum[n0 + threadIdx.x], (int)sacc);
    }
    if (wqT) {
        _Float16* const wT16 = wT16_gap ? reinterpret_cast<_Float16*>(reinterpret_cast<char*>(wqT) + wT16_gap) : nullptr;
        char* const wT16f = (wT16_gap && wT16_frag) ? reinterpret_cast<char*>(wqT) + 2 * wT16_gap : nullptr;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int k = k0 + ty + 8 * i, n = n0 + tx;
            if (n < N && k < K) {
                wqT[(int64_t)k * N + n] = (__bf16)tile[tx][ty + 8 * i];
                if (wT16) wT16[(int64_t)k * N + n] = (_Float16)tile[tx][ty + 8 * i];   // the transposed integers as fp16: the one-plane dgrad's B operand
                // (fragment order of the [K rows][N fp16] matrix: w8f_offset on its 2 N-byte rows; element n of row k starts at byte 2 n)
                if (wT16f) *reinterpret_cast<_Float16*>(wT16f + w8f_offset(k, 2 * n, 2 * N)) = (_Float16)tile[tx][ty + 8 * i];
            }
        }
    }
}
__global__ __launch_bounds__(256) void k_wquant(const float* __restrict__ W, const float* __restrict__ qp, int per_channel, int qmin, int qmax,
                                                __bf16* __restrict__ wq, __bf16* __restrict__ wqT, int N, int K) {
    wquant_body(W, qp, per_channel, qmin, qmax, wq, wqT, N, K, blockIdx.x, blockIdx.y);
}
__global__ __launch_bounds__(256) void k_w_quant_all(const WQuantTab t) {
    int wi = 0;
    while (wi + 1 < t.n && (int)blockIdx.x >= t.blk0[wi + 1]) ++wi;
    const int b = blockIdx.x - t.blk0[wi], kt = (t.K[wi] + 31) / 32;
    wquant_body(t.W[wi], t.qp[wi], t.per_channel, t.qmin, t.qmax, reinterpret_cast<__bf16*>(t.wq[wi]), reinterpret_cast<__bf16*>(t.wqT[wi]), t.N[wi],
                t.K[wi], b % kt, b / kt, reinterpret_cast<int8_t*>(t.w8[wi]), t.wsum[wi], reinterpret_cast<_Float16*>(t.w16[wi]),
                reinterpret_cast<int8_t*>(t.w8f[wi]), t.wT16 ? wT16_gap_bytes(t.N[wi], t.K[wi]) : 0, ((t.wT16f_mask >> wi) & 1ull) != 0);
}
static_assert(sizeof(WQuantTab) <= 4096, "WQuantTab travels as a kernel argument");
// row-major int8 [N, K] -> fragment order (kernel-level tests / callers that hold a row-major weight)
__global__ __launch_bounds__(256) void k_w8_fragment_order(const int8_t* __restrict__ B8, int8_t* __restrict__ B8f, int N, int K) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= (int64_t)N * K) return;
    B8f[w8f_offset((int)(i / K), (int)(i % K), K)] = B8[i];
}
int launch_w8_fragment_order(const void* B8, void* B8f, int N, int K, hipStream_t st) {
    if (N < 48 || N % 48 != 0 || K % 64 != 0 || !B8 || !B8f) { set_error("w8_fragment_order: need N %% 48 == 0, K %% 64 == 0 (N=%d K=%d)", N, K); return 1; }
    k_w8_fragment_order<<<cdiv((int64_t)N * K, 256), 256, 0, st>>>(reinterpret_cast<const int8_t*>(B8), reinterpret_cast<int8_t*>(B8f), N, K);
    return 0;
}

// ============================================================================ launchers
int launch_img_patches(const float* img, void* out_bf16, const float* qp, int qmin, int qmax, int B, int C, int H, int W, int P, hipStream_t st,
                       void* out8, int center) {
    if (P % 8 != 0 || H % P != 0 || W % P != 0) { set_error("img_patches: patch %d must be a multiple of 8 and divide %dx%d", P, H, W); return 1; }
    const int64_t n8 = (int64_t)B * C * H * W / 8;
    k_img_patches<<<flat_grid(n8), 256, 0, st>>>(img, reinterpret_cast<__bf16*>(out_bf16), qp, qmin, qmax, B, C, H, W, P, reinterpret_cast<int8_t*>(out8),
                                                 center);
    return 0;
}

// the drop-path forms of the three row kernels (elt_rows.inc): defined at the end of this file, behind the second inclusion - their kernels are instantiated
// after every other kernel of the file, which keeps those where they stood in the object
static int resid_fq_lnstats_dp(const float* x_prev, const float* Y, const float* qpY, int qmin, int qmax, float* x_new, float* mean, float* rstd,
                               const float* gamma, const float* beta, float eps, uint32_t* stats, int stat_slots, int64_t M, int D, int T, hipStream_t st,
                               unsigned long long* mbits, const QpLate& lt, const float* dps);
static int mask_bwd_dp(const float* d, const float* Y, const float* qp, int qmin, int qmax, const float* col_scale, int ncols4, __bf16* h, __bf16* l, int64_t n4,
                       hipStream_t st, const float* o16_mul, uint32_t* o16_amax, const float* dps, int T);
static int ln_bwd_fq_dp(int acc, int grid, const float* dH, const float* x, const float* mean, const float* rstd, const float* gamma, const float* beta,
                        const float* qp, int qmin, int qmax, const float* dx_in, float* dx_out, float* dgamma, float* dbeta, int64_t M, int D, int T, int cls_only,
                        hipStream_t st, const unsigned long long* nm, const float* ncs, __bf16* nh, __bf16* nl, const float* m16, uint32_t* a16, const float* dps,
                        int dp_rows);
// ... and their LayerScale forms (the third inclusion)
static int resid_fq_lnstats_ls(const float* x_prev, const float* Y, const float* qpY, int qmin, int qmax, float* x_new, float* mean, float* rstd,
                               const float* gamma, const float* beta, float eps, uint32_t* stats, int stat_slots, int64_t M, int D, int T, hipStream_t st,
                               unsigned long long* mbits, const QpLate& lt, const float* dps, const float* lsg);
static int mask_bwd_ls(const float* d, const float* Y, const float* qp, int qmin, int qmax, const float* col_scale, int ncols4, __bf16* h, __bf16* l, int64_t n4,
                       hipStream_t st, const float* o16_mul, uint32_t* o16_amax, const float* dps, int T, const float* lsg);
static int ln_bwd_fq_ls(int acc, int grid, const float* dH, const float* x, const float* mean, const float* rstd, const float* gamma, const float* beta,
                        const float* qp, int qmin, int qmax, const float* dx_in, float* dx_out, float* dgamma, float* dbeta, int64_t M, int D, int T, int cls_only,
                        hipStream_t st, const unsigned long long* nm, const float* ncs, __bf16* nh, __bf16* nl, const float* m16, uint32_t* a16, const LnBwdNext& nx);

int launch_resid_fq_lnstats(int mode, const float* x_prev, const float* Y, const float* qpY, int qmin, int qmax, const float* cls, const float* pos,
                            float* x_new, float* mean, float* rstd, const float* gamma, const float* beta, float eps, uint32_t* stats, int stat_slots,
                            int64_t M, int D, int T, hipStream_t st, void* maskbits, const QpLate* late, const float* drop_scale_rows, const float* ls_gamma) {
    if (D % 4 != 0 || D > 256 * kMaxV) { set_error("resid_fq_lnstats: D=%d unsupported (need D%%4==0, D<=768)", D); return 1; }
    unsigned long long* mbits = mode != 1 ? nullptr : reinterpret_cast<unsigned long long*>(maskbits);
    const QpLate lt = late ? *late : QpLate{};
    if (ls_gamma) {
        if (mode != 1) { set_error("resid_fq_lnstats: LayerScale belongs to a residual branch (mode 1)"); return 1; }
        return resid_fq_lnstats_ls(x_prev, Y, qpY, qmin, qmax, x_new, mean, rstd, gamma, beta, eps, stats, stat_slots, M, D, T, st, mbits, lt, drop_scale_rows, ls_gamma);
    }
    if (drop_scale_rows) {
        if (mode != 1) { set_error("resid_fq_lnstats: drop-path multipliers belong to a residual branch (mode 1)"); return 1; }
        return resid_fq_lnstats_dp(x_prev, Y, qpY, qmin, qmax, x_new, mean, rstd, gamma, beta, eps, stats, stat_slots, M, D, T, st, mbits, lt, drop_scale_rows);
    }
#define QV_RESID(MODE_, NV_) k_resid_fq_lnstats<MODE_, NV_><<<rows_grid(M), 256, 0, st>>>(x_prev, Y, qpY, qmin, qmax, cls, pos, x_new, mean, rstd, gamma, beta, eps, stats, stat_slots, M, D, T, mbits, lt)
    const int nv = (D + 255) / 256;
    if (mode == 0) { if (nv == 1) QV_RESID(0, 1); else if (nv == 2) QV_RESID(0, 2); else QV_RESID(0, 3); }
    else if (mode == 1) { if (nv == 1) QV_RESID(1, 1); else if (nv == 2) QV_RESID(1, 2); else QV_RESID(1, 3); }
    else { if (nv == 1) QV_RESID(2, 1); else if (nv == 2) QV_RESID(2, 2); else QV_RESID(2, 3); }
#undef QV_RESID
    return 0;
}

int launch_ln_apply_quant(const float* x, const float* mean, const float* rstd, const float* gamma, const float* beta, const float* qp, int qmin,
                          int qmax, void* out_bf16, int64_t M, int D, hipStream_t st, void* out8, int center, bool out_f16, const QpLate* late) {
    k_ln_apply_quant<<<flat_grid(M * (D / 4)), 256, 0, st>>>(x, mean, rstd, gamma, beta, qp, qmin, qmax, reinterpret_cast<__bf16*>(out_bf16), M, D,
                                                             reinterpret_cast<int8_t*>(out8), center, out_f16 ? 1 : 0, late ? *late : QpLate{});
    return 0;
}

int launch_ln_quant8(const float* x, const float* gamma, const float* beta, float eps, const float* qp, int qmin, int qmax, int center, void* out8,
                     float* mean, float* rstd, int64_t nrows, int64_t row_stride, int D, hipStream_t st) {
    if (D % 4 != 0 || D > 256 * kMaxV) { set_error("ln_quant8: D=%d unsupported (need D%%4==0, D<=768)", D); return 1; }
    const int nv = (D + 255) / 256, grid = rows_grid(nrows);
    int8_t* o = reinterpret_cast<int8_t*>(out8);
    if (nv == 1) k_ln_quant8<1><<<grid, 256, 0, st>>>(x, gamma, beta, eps, qp, qmin, qmax, center, o, mean, rstd, nrows, row_stride, D);
    else if (nv == 2) k_ln_quant8<2><<<grid, 256, 0, st>>>(x, gamma, beta, eps, qp, qmin, qmax, center, o, mean, rstd, nrows, row_stride, D);
    else k_ln_quant8<3><<<grid, 256, 0, st>>>(x, gamma, beta, eps, qp, qmin, qmax, center, o, mean, rstd, nrows, row_stride, D);
    return 0;
}
int launch_cls_rows(const float* cls, const float* pos, float* x, int B, int T, int D, hipStream_t st) {
    k_cls_rows<<<cdiv((int64_t)B * D, 256), 256, 0, st>>>(cls, pos, x, B, T, D);
    return 0;
}

int launch_mask_bwd(int gelu_bwd, const float* d, const float* Y, const float* qp, int qmin, int qmax, const float* col_scale, int ncols,
                    void* dst_hi, void* dst_lo, int64_t n, hipStream_t st, const float* o16_mul, uint32_t* o16_amax, const float* drop_scale_rows, int T, const float* ls_gamma) {
    __bf16* h = reinterpret_cast<__bf16*>(dst_hi);
    __bf16* l = reinterpret_cast<__bf16*>(dst_lo);
    if (ls_gamma) {   // Y: a residual branch's output under LayerScale (and, drop_scale_rows, drop-path)
        if (gelu_bwd || T < 1 || ncols < 4 || (o16_mul && !o16_amax)) { set_error("mask_bwd: LayerScale goes with the plain mask, ncols and T"); return 1; }
        return mask_bwd_ls(d, Y, qp, qmin, qmax, col_scale, ncols / 4, h, l, n / 4, st, o16_mul, o16_amax, drop_scale_rows, T, ls_gamma);
    }
    if (drop_scale_rows) {   // Y: a residual branch's output, [n / ncols rows, T per sample] x ncols, under drop-path
        if (gelu_bwd || T < 1 || ncols < 4 || (o16_mul && !o16_amax)) { set_error("mask_bwd: drop-path multipliers go with the plain mask, ncols and T"); return 1; }
        return mask_bwd_dp(d, Y, qp, qmin, qmax, col_scale, ncols / 4, h, l, n / 4, st, o16_mul, o16_amax, drop_scale_rows, T);
    }
    if (o16_mul) {   // the one-plane form (dst_hi = the fp16 plane)
        if (gelu_bwd || !o16_amax) { set_error("mask_bwd: the one-plane form covers the plain mask with o16_amax"); return 1; }
        k_mask_bwd<0, true><<<flat_grid(n / 4), 256, 0, st>>>(d, Y, qp, qmin, qmax, col_scale, ncols / 4, h, l, n / 4, o16_mul, o16_amax);
        return 0;
    }
    if (gelu_bwd) k_mask_bwd<1><<<flat_grid(n / 4), 256, 0, st>>>(d, Y, qp, qmin, qmax, col_scale, ncols / 4, h, l, n / 4, nullptr, nullptr);
    else k_mask_bwd<0><<<flat_grid(n / 4), 256, 0, st>>>(d, Y, qp, qmin, qmax, col_scale, ncols / 4, h, l, n / 4, nullptr, nullptr);
    return 0;
}

int launch_ln_bwd_fq(int acc, const float* dH, const float* x, const float* mean, const float* rstd, const float* gamma, const float* beta,
                     const float* qp, int qmin, int qmax, const float* dx_in, float* dx_out, float* dgamma, float* dbeta, int64_t M, int D, int T,
                     int cls_only, hipStream_t st, const LnBwdNext* next, int rows_per_wave) {
    if (D % 4 != 0 || D > 256 * kMaxV) { set_error("ln_bwd_fq: D=%d unsupported", D); return 1; }
    const int rpw = rows_per_wave > 0 ? rows_per_wave : 16;   // rows per wave (8 waves per block): fewer blocks = fewer same-address dgamma/dbeta atomics (12 ns each, serialised)
    int grid = (int)((M + 8 * rpw - 1) / (8 * rpw));
    if (grid > 4096) grid = 4096;
    if (grid < 1) grid = 1;
    const unsigned long long* nm = next ? reinterpret_cast<const unsigned long long*>(next->maskbits) : nullptr;
    const float* ncs = next ? next->colscale : nullptr;
    __bf16* nh = next ? reinterpret_cast<__bf16*>(next->out_hi) : nullptr;
    __bf16* nl = next ? reinterpret_cast<__bf16*>(next->out_lo) : nullptr;
    const float* m16 = next ? next->o16_mul : nullptr;
    uint32_t* a16 = next ? next->o16_amax : nullptr;
    if (m16 && !a16) { set_error("ln_bwd_fq: o16_mul needs o16_amax"); return 1; }
    if (next && next->ls_gamma) {   // the next branch ran under LayerScale: its gamma goes into the fused store, and gamma's gradient is formed here
        if (next->drop_rows < 1 || !nh || !next->ls_dgamma || !next->ls_Y || next->ls_ymul < 1) {
            set_error("ln_bwd_fq: LayerScale needs the rows per sample, an output plane, the branch output and the gradient buffer");
            return 1;
        }
        return ln_bwd_fq_ls(acc, grid, dH, x, mean, rstd, gamma, beta, qp, qmin, qmax, dx_in, dx_out, dgamma, dbeta, M, D, T, cls_only, st, nm, ncs, nh, nl, m16, a16, *next);
    }
    if (next && next->drop_scale) {   // the next branch ran under drop-path: its multipliers go into the fused store
        if (next->drop_rows < 1 || !nh) { set_error("ln_bwd_fq: drop-path multipliers need the rows per sample and an output plane"); return 1; }
        return ln_bwd_fq_dp(acc, grid, dH, x, mean, rstd, gamma, beta, qp, qmin, qmax, dx_in, dx_out, dgamma, dbeta, M, D, T, cls_only, st, nm, ncs, nh, nl, m16, a16,
                            next->drop_scale, next->drop_rows);
    }
#define QV_LNB(ACC_, NV_)                                                                                                                         \
    do {                                                                                                                                           \
        if (next && m16) k_ln_bwd_fq<ACC_, NV_, 8, true, true><<<grid, 512, 0, st>>>(dH, 0, x, mean, rstd, gamma, beta, qp, qmin, qmax, dx_in, dx_out, dgamma, dbeta, M, D, T, cls_only, nm, ncs, nh, nl, m16, a16); \
        else if (next && !nl) k_ln_bwd_fq<ACC_, NV_, 8, true, false, true><<<grid, 512, 0, st>>>(dH, 0, x, mean, rstd, gamma, beta, qp, qmin, qmax, dx_in, dx_out, dgamma, dbeta, M, D, T, cls_only, nm, ncs, nh, nullptr, nullptr, nullptr); \
        else if (next) k_ln_bwd_fq<ACC_, NV_, 8, true><<<grid, 512, 0, st>>>(dH, 0, x, mean, rstd, gamma, beta, qp, qmin, qmax, dx_in, dx_out, dgamma, dbeta, M, D, T, cls_only, nm, ncs, nh, nl, nullptr, nullptr); \
        else k_ln_bwd_fq<ACC_, NV_, 8, false><<<grid, 512, 0, st>>>(dH, 0, x, mean, rstd, gamma, beta, qp, qmin, qmax, dx_in, dx_out, dgamma, dbeta, M, D, T, cls_only, nm, ncs, nh, nl, nullptr, nullptr); \
    } while (0)
    const int nv = (D + 255) / 256;
    if (acc) { if (nv == 1) QV_LNB(1, 1); else if (nv == 2) QV_LNB(1, 2); else QV_LNB(1, 3); }
    else { if (nv == 1) QV_LNB(0, 1); else if (nv == 2) QV_LNB(0, 2); else QV_LNB(0, 3); }
#undef QV_LNB
    return 0;
}

int launch_head_fwd(const float* x, const float* mean, const float* rstd, const float* gamma, const float* beta, const float* qp_norm, int qmin,
                    int qmax, const void* wq, const float* w_scale, int w_per_channel, const float* bias, float* hq, float* logits_pre,
                    uint32_t* stats, int stat_slots, int B, int D, int T, int C, hipStream_t st) {
    k_head_fwd<<<B, 256, D * sizeof(float), st>>>(x, mean, rstd, gamma, beta, qp_norm, qmin, qmax, reinterpret_cast<const __bf16*>(wq), w_scale,
                                                   w_per_channel, bias, hq, logits_pre, stats, stat_slots, D, T, C);
    return 0;
}

int launch_logits_fq(const float* pre, const float* qp, int qmin, int qmax, float* out, int n, hipStream_t st) {
    k_logits_fq<<<cdiv(n, 256), 256, 0, st>>>(pre, qp, qmin, qmax, out, n);
    return 0;
}

int launch_head_bwd(const float* dlogits, const float* logits_pre, const float* qp_logits, int qmin, int qmax, const float* hq, const float* qp_norm,
                    const void* wq, const float* W, const float* w_scale, const int32_t* w_zp, int w_per_channel, int w_qmin, int w_qmax, float* dW,
                    float* dbias, float* dh, int B, int D, int C, hipStream_t st) {
    k_head_bwd<<<C * ((D + 63) / 64) + B, 256, 0, st>>>(dlogits, logits_pre, qp_logits, qmin, qmax, hq, qp_norm, reinterpret_cast<const __bf16*>(wq), W, w_scale, w_zp,
                                      w_per_channel, w_qmin, w_qmax, dW, dbias, dh, B, D, C);
    return 0;
}

int launch_embed_bwd(const float* dx0, const float* Y0, const float* qp, int qmin, int qmax, float* dpos, float* dcls, void* dY0_hi, void* dY0_lo,
                     int B, int T, int D, hipStream_t st) {
    k_embed_bwd<<<(int)cdiv((int64_t)T * (D / 4), 64), 64, 0, st>>>(dx0, Y0, qp, qmin, qmax, dpos, dcls, reinterpret_cast<__bf16*>(dY0_hi),
                                                                  reinterpret_cast<__bf16*>(dY0_lo), B, T, D);
    return 0;
}

__global__ void k_zero_i32(int32_t* p, int64_t n) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) p[i] = 0;
}
// (a kernel, not hipMemsetAsync: the memset node of a captured hipGraph did not re-zero the buffer on replay)
int launch_zero_i32(int32_t* p, int64_t n, hipStream_t st) {
    k_zero_i32<<<(int)cdiv(n, 256) > 1024 ? 1024 : (int)cdiv(n, 256), 256, 0, st>>>(p, n);
    return 0;
}
// ---------------------------------------------------------------- the class-token rows of [B * T, .] tensors (the last block's backward on B rows)
// blockIdx.y = the tensor; 4-byte words, so that one kernel moves a row statistic (4 B), a mask-bit row and a 1536-float row alike
__global__ __launch_bounds__(256) void k_rows_gather(const RowMoveTab t, int rows, int T) {
    const RowMove m = t.m[blockIdx.y];
    const int wpr = m.width / 4;
    const int64_t tall = (int64_t)T * (m.stride / 4);   // words between two gathered rows
    const uint32_t* __restrict__ src = reinterpret_cast<const uint32_t*>(m.src);
    uint32_t* __restrict__ dst = reinterpret_cast<uint32_t*>(m.dst);
    const int total = rows * wpr;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
        const int b = i / wpr, j = i - b * wpr;
        dst[i] = src[b * tall + j];
    }
}
// every 16-byte chunk of the tall tensor is written exactly once: streaming stores at the rate of a fill
__global__ __launch_bounds__(256) void k_rows_scatter(const RowMoveTab t, int rows, int T) {
    const RowMove m = t.m[blockIdx.y];
    const int cpr = m.width / 16;
    const uint4* __restrict__ src = reinterpret_cast<const uint4*>(m.src);
    uint4* __restrict__ dst = reinterpret_cast<uint4*>(m.dst);
    const int total = rows * T * cpr;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
        const int row = i / cpr, c = i - row * cpr;
        const int b = row / T;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (row - b * T == 0) v = src[b * cpr + c];
        dst[i] = v;
    }
}
static int rows_check(const char* who, const RowMoveTab& t, int rows, int T, bool scatter) {
    if (t.n < 1 || t.n > kRowMoveMax || rows < 1 || T < 1) { set_error("%s: %d tensors, %d rows, T=%d", who, t.n, rows, T); return 1; }
    for (int k = 0; k < t.n; ++k) {
        const RowMove& m = t.m[k];
        const int unit = scatter ? 16 : 4;
        const bool ok = m.src && m.dst && m.width >= unit && m.width % unit == 0 && m.stride % unit == 0 && (scatter ? m.stride == m.width : m.stride >= m.width) &&
                        (int64_t)rows * (scatter ? T : 1) * (m.width / unit) < (1ll << 31) &&
                        (reinterpret_cast<uintptr_t>(m.src) | reinterpret_cast<uintptr_t>(m.dst)) % unit == 0;
        if (!ok) { set_error("%s: tensor %d: width %d, stride %lld (bytes; need %% %d == 0%s, aligned bases, < 2^31 units)", who, k, m.width, (long long)m.stride, unit,
                             scatter ? " and stride == width" : ""); return 1; }
    }
    return 0;
}
int launch_rows_gather(const RowMoveTab& t, int rows, int T, hipStream_t st) {
    if (rows_check("rows_gather", t, rows, T, false)) return 1;
    int64_t most = 0;
    for (int k = 0; k < t.n; ++k) most = std::max<int64_t>(most, (int64_t)rows * (t.m[k].width / 4));
    k_rows_gather<<<dim3(std::min(cdiv(most, 256), 512), t.n), 256, 0, st>>>(t, rows, T);
    return 0;
}
int launch_rows_scatter(const RowMoveTab& t, int rows, int T, hipStream_t st) {
    if (rows_check("rows_scatter", t, rows, T, true)) return 1;
    int64_t most = 0;
    for (int k = 0; k < t.n; ++k) most = std::max<int64_t>(most, (int64_t)rows * T * (t.m[k].width / 16));
    k_rows_scatter<<<dim3(std::min(cdiv(most, 256 * 4), 4096), t.n), 256, 0, st>>>(t, rows, T);
    return 0;
}
int launch_w_quant_all(WQuantTab& t, hipStream_t st) {
    int b = 0;
    for (int i = 0; i < t.n; ++i) {
        t.blk0[i] = b;
        b += (int)(cdiv(t.K[i], 32) * cdiv(t.N[i], 32));
    }
    t.blk0[t.n] = b;
    k_w_quant_all<<<b, 256, 0, st>>>(t);
    return 0;
}
int launch_wquant(const float* W, const float* qp, int per_channel, int qmin, int qmax, void* wq, void* wqT, int N, int K, hipStream_t st) {
    dim3 grid(cdiv(K, 32), cdiv(N, 32));
    k_wquant<<<grid, 256, 0, st>>>(W, qp, per_channel, qmin, qmax, reinterpret_cast<__bf16*>(wq), reinterpret_cast<__bf16*>(wqT), N, K);
    return 0;
}

// ============================================================================ the row kernels under drop-path (k_*_dp) and their launches
#define QV_DP 1
#include "elt_rows.inc"
#undef QV_DP

static int resid_fq_lnstats_dp(const float* x_prev, const float* Y, const float* qpY, int qmin, int qmax, float* x_new, float* mean, float* rstd,
                               const float* gamma, const float* beta, float eps, uint32_t* stats, int stat_slots, int64_t M, int D, int T, hipStream_t st,
                               unsigned long long* mbits, const QpLate& lt, const float* dps) {
#define QV_RESID_DP(NV_) k_resid_fq_lnstats_dp<1, NV_><<<rows_grid(M), 256, 0, st>>>(x_prev, Y, qpY, qmin, qmax, nullptr, nullptr, x_new, mean, rstd, gamma, beta, eps, stats, stat_slots, M, D, T, mbits, lt, dps, T)
    const int nv = (D + 255) / 256;
    if (nv == 1) QV_RESID_DP(1); else if (nv == 2) QV_RESID_DP(2); else QV_RESID_DP(3);
#undef QV_RESID_DP
    return 0;
}
static int mask_bwd_dp(const float* d, const float* Y, const float* qp, int qmin, int qmax, const float* col_scale, int ncols4, __bf16* h, __bf16* l, int64_t n4,
                       hipStream_t st, const float* o16_mul, uint32_t* o16_amax, const float* dps, int T) {
    if (o16_mul) k_mask_bwd_dp<0, true><<<flat_grid(n4), 256, 0, st>>>(d, Y, qp, qmin, qmax, col_scale, ncols4, h, l, n4, o16_mul, o16_amax, dps, T);
    else k_mask_bwd_dp<0><<<flat_grid(n4), 256, 0, st>>>(d, Y, qp, qmin, qmax, col_scale, ncols4, h, l, n4, nullptr, nullptr, dps, T);
    return 0;
}
// (the output forms of launch_ln_bwd_fq's fused store: one fp16 plane, one bf16 plane, the bf16 pair)
static int ln_bwd_fq_dp(int acc, int grid, const float* dH, const float* x, const float* mean, const float* rstd, const float* gamma, const float* beta,
                        const float* qp, int qmin, int qmax, const float* dx_in, float* dx_out, float* dgamma, float* dbeta, int64_t M, int D, int T, int cls_only,
                        hipStream_t st, const unsigned long long* nm, const float* ncs, __bf16* nh, __bf16* nl, const float* m16, uint32_t* a16, const float* dps,
                        int dp_rows) {
#define QV_LNB_DP(ACC_, NV_)                                                                                                                       \
    do {                                                                                                                                           \
        if (m16) k_ln_bwd_fq_dp<ACC_, NV_, 8, true, true><<<grid, 512, 0, st>>>(dH, 0, x, mean, rstd, gamma, beta, qp, qmin, qmax, dx_in, dx_out, dgamma, dbeta, M, D, T, cls_only, nm, ncs, nh, nl, m16, a16, dps, dp_rows); \
        else if (!nl) k_ln_bwd_fq_dp<ACC_, NV_, 8, true, false, true><<<grid, 512, 0, st>>>(dH, 0, x, mean, rstd, gamma, beta, qp, qmin, qmax, dx_in, dx_out, dgamma, dbeta, M, D, T, cls_only, nm, ncs, nh, nullptr, nullptr, nullptr, dps, dp_rows); \
        else k_ln_bwd_fq_dp<ACC_, NV_, 8, true><<<grid, 512, 0, st>>>(dH, 0, x, mean, rstd, gamma, beta, qp, qmin, qmax, dx_in, dx_out, dgamma, dbeta, M, D, T, cls_only, nm, ncs, nh, nl, nullptr, nullptr, dps, dp_rows); \
    } while (0)
    const int nv = (D + 255) / 256;
    if (acc) { if (nv == 1) QV_LNB_DP(1, 1); else if (nv == 2) QV_LNB_DP(1, 2); else QV_LNB_DP(1, 3); }
    else { if (nv == 1) QV_LNB_DP(0, 1); else if (nv == 2) QV_LNB_DP(0, 2); else QV_LNB_DP(0, 3); }
#undef QV_LNB_DP
    return 0;
}

// ============================================================================ the row kernels under LayerScale (k_*_ls) and their launches
#define QV_DP 2
#include "elt_rows.inc"
#undef QV_DP

static int resid_fq_lnstats_ls(const float* x_prev, const float* Y, const float* qpY, int qmin, int qmax, float* x_new, float* mean, float* rstd,
                               const float* gamma, const float* beta, float eps, uint32_t* stats, int stat_slots, int64_t M, int D, int T, hipStream_t st,
                               unsigned long long* mbits, const QpLate& lt, const float* dps, const float* lsg) {
#define QV_RESID_LS(NV_) k_resid_fq_lnstats_ls<1, NV_><<<rows_grid(M), 256, 0, st>>>(x_prev, Y, qpY, qmin, qmax, nullptr, nullptr, x_new, mean, rstd, gamma, beta, eps, stats, stat_slots, M, D, T, mbits, lt, dps, T, lsg)
    const int nv = (D + 255) / 256;
    if (nv == 1) QV_RESID_LS(1); else if (nv == 2) QV_RESID_LS(2); else QV_RESID_LS(3);
#undef QV_RESID_LS
    return 0;
}
static int mask_bwd_ls(const float* d, const float* Y, const float* qp, int qmin, int qmax, const float* col_scale, int ncols4, __bf16* h, __bf16* l, int64_t n4,
                       hipStream_t st, const float* o16_mul, uint32_t* o16_amax, const float* dps, int T, const float* lsg) {
    if (o16_mul) k_mask_bwd_ls<0, true><<<flat_grid(n4), 256, 0, st>>>(d, Y, qp, qmin, qmax, col_scale, ncols4, h, l, n4, o16_mul, o16_amax, dps, T, lsg);
    else k_mask_bwd_ls<0><<<flat_grid(n4), 256, 0, st>>>(d, Y, qp, qmin, qmax, col_scale, ncols4, h, l, n4, nullptr, nullptr, dps, T, lsg);
    return 0;
}
// (the output forms of launch_ln_bwd_fq's fused store: one fp16 plane, one bf16 plane, the bf16 pair)
static int ln_bwd_fq_ls(int acc, int grid, const float* dH, const float* x, const float* mean, const float* rstd, const float* gamma, const float* beta,
                        const float* qp, int qmin, int qmax, const float* dx_in, float* dx_out, float* dgamma, float* dbeta, int64_t M, int D, int T, int cls_only,
                        hipStream_t st, const unsigned long long* nm, const float* ncs, __bf16* nh, __bf16* nl, const float* m16, uint32_t* a16, const LnBwdNext& nx) {
#define QV_LS_TAIL nx.drop_scale, nx.drop_rows, nx.ls_gamma, nx.ls_Y, nx.ls_ymul, nx.ls_qp, nx.ls_kind, nx.ls_dgamma
#define QV_LNB_LS(ACC_, NV_)                                                                                                                       \
    do {                                                                                                                                           \
        if (m16) k_ln_bwd_fq_ls<ACC_, NV_, 8, true, true><<<grid, 512, 0, st>>>(dH, 0, x, mean, rstd, gamma, beta, qp, qmin, qmax, dx_in, dx_out, dgamma, dbeta, M, D, T, cls_only, nm, ncs, nh, nl, m16, a16, QV_LS_TAIL); \
        else if (!nl) k_ln_bwd_fq_ls<ACC_, NV_, 8, true, false, true><<<grid, 512, 0, st>>>(dH, 0, x, mean, rstd, gamma, beta, qp, qmin, qmax, dx_in, dx_out, dgamma, dbeta, M, D, T, cls_only, nm, ncs, nh, nullptr, nullptr, nullptr, QV_LS_TAIL); \
        else k_ln_bwd_fq_ls<ACC_, NV_, 8, true><<<grid, 512, 0, st>>>(dH, 0, x, mean, rstd, gamma, beta, qp, qmin, qmax, dx_in, dx_out, dgamma, dbeta, M, D, T, cls_only, nm, ncs, nh, nl, nullptr, nullptr, QV_LS_TAIL); \
    } while (0)
    const int nv = (D + 255) / 256;
    if (acc) { if (nv == 1) QV_LNB_LS(1, 1); else if (nv == 2) QV_LNB_LS(1, 2); else QV_LNB_LS(1, 3); }
    else { if (nv == 1) QV_LNB_LS(0, 1); else if (nv == 2) QV_LNB_LS(0, 2); else QV_LNB_LS(0, 3); }
#undef QV_LNB_LS
#undef QV_LS_TAIL
    return 0;
}

}  // namespace qv
