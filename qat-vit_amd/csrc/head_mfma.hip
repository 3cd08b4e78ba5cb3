// The classifier head of the QAT student step on MFMA (gfx950, v_mfma_f32_16x16x32_bf16), for 128 .. 32768 classes: the second form of
// k_head_fwd / k_head_bwd (elt.hip), which walk the classes one after the other.
//
// Both operands of the head are integers on a quantisation grid: hq = q - zp (|.| <= 255 with at most 256 activation levels) and wq, the
// bf16 plane of weight integers.  Their products are exact in bf16 x bf16 -> fp32 and every partial sum is an integer below 2^24 for
// D <= 512 (255 * 127 * 512 < 2^24), so the forward GEMM gives the tiny form's logits_pre bit for bit: same accumulator value, then the same
// separate multiply and add (the library is built with -ffp-contract=off).
//
// Forward, k_head_fwd_mfma: one workgroup per 64 classes.  It stages its [64, D] slice of wq in LDS ONCE (K = D whole, no k-loop ring: the
// weight plane crosses HBM exactly once) and then walks the batch in blocks of 64 rows, one 16-row MFMA tile per wave; the A fragments are
// 16-byte loads of hq16 (B * D * 2 bytes: L2-resident).  Where there are fewer class tiles than CUs the row blocks are dealt over
// gridDim.y.  The observer's min / max is kept per lane over the whole walk and sent as ONE stat_atomic per wave.
//
// Backward, k_head_bwd_mfma<WGRAD>: dl = dlogits where fqv(logits_pre) is in range, else 0, is fp32 and stays fp32-accurate: while a
// [32 rows, 32 classes] block of it is staged, each value is split in registers into three bf16 planes (hi, mid, lo: residual <= 2^-27
// relative) that only ever exist in LDS; the other operand (wq, hq16) is exact, so a k-step is three MFMA passes.
//   dgrad (WGRAD = false): dh[b, d] = sum_c dl[b, c] * s_w[c] * wq[c, d].  Workgroup = (32 batch rows, a range of 32-class chunks); the
//     accumulators ([32, D] over four waves, D / 4 columns each) stay in registers over the whole range, the fp32 partial tile goes to a
//     scratch area and k_head_dgrad_reduce sums the ranges in a fixed order: no atomics, bit-reproducible.  A per-channel s_w multiplies dl
//     before the split, a per-tensor one the reduced sum.
//   wgrad (WGRAD = true):  dW[c, d] = mask_w(W[c, d]) * s_norm * sum_b dl[b, c] * hq16[b, d]; dbias[c] = sum_b dl[b, c].  Workgroup = 32
//     classes, K = B whole in 32-row steps (no split).  dl is [B, C] row-major, so its k-run is strided: the LDS image keeps the global
//     layout and the fragments come out of it with the transposed 16-bit LDS reads (ds_read_b64_tr_b16, lane map as in gemm.hip tr_frag);
//     dbias is summed in fp32 from the staged values, eight fixed row groups folded in order.
// Both read the [32, D] block of their exact operand through the same transposed reads (its k index runs over LDS rows).
// [B, C] rows are not 16-byte aligned when C % 4 != 0: every access to dlogits / logits_pre is one dword per lane, 32 consecutive classes per
// half wave, which needs no alignment and no head / tail cases.  Nothing is read or written past B, C or D: out-of-range rows of a staged
// block are zero-filled, the forward clamps its A rows, and the epilogues are masked.
#include <algorithm>

#include "qv_common.h"
#include "qv_device.h"
#include "qv_kernels.h"

namespace qv {
namespace {

struct HQP { float s, inv, zp, on; };
__device__ inline HQP load_hqp(const float* qp) { return HQP{qp[0], qp[1], qp[2], qp[3]}; }

// ---------------------------------------------------------------- forward
// hq[b, :] = q(LN(x[b, 0, :])) - zp, as k_head_fwd forms it, in fp32 (the backward of the tiny form and the tests read it) and as bf16
__global__ __launch_bounds__(256) void k_head_rows_mfma(const float* __restrict__ x, const float* __restrict__ mean, const float* __restrict__ rstd,
                                                        const float* __restrict__ gamma, const float* __restrict__ beta, const float* __restrict__ qp_norm,
                                                        int qmin, int qmax, float* __restrict__ hq, __bf16* __restrict__ hq16, int D, int T) {
    const HQP q = load_hqp(qp_norm);
    const int b = blockIdx.x;
    const int64_t row = (int64_t)b * T;
    const float mu = mean[row], rs = rstd[row];
    for (int c = threadIdx.x; c < D; c += blockDim.x) {
        const float h = fminf(fmaxf(rintf(((x[row * D + c] - mu) * rs * gamma[c] + beta[c]) * q.inv) + q.zp, (float)qmin), (float)qmax) - q.zp;
        hq[(int64_t)b * D + c] = h;
        hq16[(int64_t)b * D + c] = (__bf16)h;
    }
}

constexpr int kFwdClasses = 64;   // classes per workgroup
constexpr int kFwdRows = 64;      // batch rows per step: one 16-row tile per wave
constexpr int kFwdPad = 16;       // bytes behind each LDS row of the weight slice: sixteen rows' 16-byte chunks then cover all banks

__global__ __launch_bounds__(256) void k_head_fwd_mfma(const __bf16* __restrict__ hq16, const __bf16* __restrict__ wq, const float* __restrict__ qp_norm,
                                                       const float* __restrict__ w_scale, int w_per_channel, const float* __restrict__ bias,
                                                       float* __restrict__ logits_pre, uint32_t* __restrict__ stats, int stat_slots, int B, int D, int C) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int rowb = D * 2 + kFwdPad;
    const int c0 = blockIdx.x * kFwdClasses;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, idx = lane & 15, g = lane >> 4;
    const int cpr = D / 8;   // 16-byte chunks per weight row
    for (int i = threadIdx.x; i < kFwdClasses * cpr; i += 256) {
        const int r = i / cpr, ch = i % cpr;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (c0 + r < C) v = *reinterpret_cast<const uint4*>(wq + (int64_t)(c0 + r) * D + ch * 8);
        *reinterpret_cast<uint4*>(smem + r * rowb + ch * 16) = v;
    }
    __syncthreads();
    const float sa = qp_norm[0];
    float sc[4], bi[4];
    bool cv[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int c = c0 + 16 * j + idx;
        cv[j] = c < C;
        const int cc = cv[j] ? c : C - 1;
        sc[j] = sa * w_scale[w_per_channel ? cc : 0];
        bi[j] = bias[cc];
    }
    float mn = INFINITY, mx = -INFINITY;
    for (int r0 = blockIdx.y * kFwdRows; r0 < B; r0 += gridDim.y * kFwdRows) {
        const int rw = r0 + wave * 16;
        if (rw >= B) continue;   // (wave-uniform; no barrier below)
        const int ra = min(rw + idx, B - 1);
        const __bf16* arow = hq16 + (int64_t)ra * D + g * 8;
        f32x4 acc[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int kk = 0; kk < D / 32; ++kk) {
            const bf16x8 a = *reinterpret_cast<const bf16x8*>(arow + kk * 32);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bf16x8 w = *reinterpret_cast<const bf16x8*>(smem + (16 * j + idx) * rowb + (kk * 4 + g) * 16);
                acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, w, acc[j], 0, 0, 0);
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int row = rw + 4 * g + e;
                if (row < B && cv[j]) {
                    const float v = acc[j][e] * sc[j] + bi[j];
                    logits_pre[(int64_t)row * C + c0 + 16 * j + idx] = v;
                    mn = fminf(mn, v);
                    mx = fmaxf(mx, v);
                }
            }
        }
    }
    mn = wave_min(mn);
    mx = wave_max(mx);
    if (lane == 0 && mn <= mx) stat_atomic(stats, stat_slots, mn, mx);
}

// ---------------------------------------------------------------- backward
constexpr int kBwdTile = 32;                 // rows of the output tile (dgrad: batch rows, wgrad: classes) and of a k-step
constexpr int kARow = 2 * kBwdTile + 16;     // bytes per LDS row of a dl plane ([32 batch rows][32 classes] bf16, 16 bytes of padding)
constexpr int kAPlane = kBwdTile * kARow;
constexpr int kBPad = 32;                    // bytes behind each LDS row of the exact operand's [32, D] block
constexpr int kMaxNT = 12;                   // 16-column tiles per wave: D / 64 <= 12
constexpr int kDgradGrid = 256;              // workgroups the dgrad aims at (the CU count of an MI355X, and cu_count()'s answer where the runtime gives none)

struct HeadBwdArgs {
    const float* dlogits; const float* logits_pre; const float* qp_logits;
    int qmin, qmax;
    const __bf16* plane;       // the exact operand: dgrad wq [C, D], wgrad hq16 [B, D]
    const float* w_scale;
    int w_per_channel;
    float* partial;            // dgrad: [splits][row tiles * 32][D]
    int chunks_per_split;
    const float* W; const int32_t* w_zp; const float* qp_norm;   // wgrad
    int w_qmin, w_qmax;
    float* dW; float* dbias;
    int B, D, C;
};

// 16x16x32 operand fragment out of a row-major LDS image whose k index runs over rows 8 g + (0..7) and whose row / column index is image column
// col0 + (lane & 15): two transposed 4 x 16 block reads (the lane map gemm.hip tr_frag and qv_device.h tr_frag2 use)
__device__ inline bf16x8 head_tr_frag(const char* img, int rowb, int col0, int lane) {
    const int g = lane >> 4, idx = lane & 15, q = idx >> 2, pp = idx & 3;
    const char* p = img + (8 * g + q) * rowb + (col0 + 4 * pp) * 2;
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)p);
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(p + 4 * rowb));
    const s16x8 v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);   // (whole-vector bit cast: qv_device.h tr_frag2)
    return __builtin_bit_cast(bf16x8, v);
}

template <bool WGRAD>
__global__ __launch_bounds__(256) void k_head_bwd_mfma(const HeadBwdArgs p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int B = p.B, D = p.D, C = p.C;
    const int browb = 2 * D + kBPad;
    char* imgB = smem;
    char* imgA = smem + kBwdTile * browb;
    float* sdb = reinterpret_cast<float*>(imgA + 3 * kAPlane);   // wgrad: [8 row groups][32 classes]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, idx = lane & 15, g = lane >> 4;
    const int ntw = D / 64, cpr = D / 8;
    const HQP ql = load_hqp(p.qp_logits);
    const float fqmin = (float)p.qmin, fqmax = (float)p.qmax;
    const int tile0 = blockIdx.x * kBwdTile;
    int k_lo = 0, k_hi;
    if constexpr (!WGRAD) {
        k_lo = blockIdx.y * p.chunks_per_split;
        k_hi = min((C + kBwdTile - 1) / kBwdTile, k_lo + p.chunks_per_split);
    } else {
        k_hi = (B + kBwdTile - 1) / kBwdTile;
    }
    f32x4 acc[2][kMaxNT];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int j = 0; j < kMaxNT; ++j) acc[mt][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    float db = 0.f;
    const int cl = threadIdx.x & 31, bs = threadIdx.x >> 5;
    for (int kc = k_lo; kc < k_hi; ++kc) {
        const int b0 = WGRAD ? kc * kBwdTile : tile0, c0 = WGRAD ? tile0 : kc * kBwdTile;
        const int c = c0 + cl;
        float gv[4], lv[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int b = b0 + bs + 8 * i;
            const bool ok = b < B && c < C;
            gv[i] = ok ? p.dlogits[(int64_t)b * C + c] : 0.f;
            lv[i] = ok ? p.logits_pre[(int64_t)b * C + c] : 0.f;
        }
        float sw = 1.f;
        if (!WGRAD && p.w_per_channel && c < C) sw = p.w_scale[c];
        const int r0 = WGRAD ? b0 : c0, R = WGRAD ? B : C;
        for (int i = threadIdx.x; i < kBwdTile * cpr; i += 256) {
            const int r = i / cpr, ch = i % cpr;
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (r0 + r < R) v = *reinterpret_cast<const uint4*>(p.plane + (int64_t)(r0 + r) * D + ch * 8);
            *reinterpret_cast<uint4*>(imgB + r * browb + ch * 16) = v;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float t = rintf(lv[i] * ql.inv) + ql.zp;
            const bool in = (t >= fqmin && t <= fqmax) || ql.on == 0.f;
            float dl = in ? gv[i] : 0.f;
            if constexpr (WGRAD) db += dl;
            else if (p.w_per_channel) dl = dl * sw;
            const __bf16 hi = (__bf16)dl;
            const float r1 = dl - (float)hi;
            const __bf16 mid = (__bf16)r1;
            const __bf16 lo = (__bf16)(r1 - (float)mid);
            char* dst = imgA + (bs + 8 * i) * kARow + cl * 2;
            *reinterpret_cast<__bf16*>(dst) = hi;
            *reinterpret_cast<__bf16*>(dst + kAPlane) = mid;
            *reinterpret_cast<__bf16*>(dst + 2 * kAPlane) = lo;
        }
        __syncthreads();
        bf16x8 af[2][3];
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int pl = 0; pl < 3; ++pl) {
                if constexpr (WGRAD) af[mt][pl] = head_tr_frag(imgA + pl * kAPlane, kARow, 16 * mt, lane);   // row index = class, k = batch row
                else af[mt][pl] = *reinterpret_cast<const bf16x8*>(imgA + pl * kAPlane + (16 * mt + idx) * kARow + g * 16);   // row index = batch row, k = class
            }
#pragma unroll
        for (int j = 0; j < kMaxNT; ++j) {
            if (j < ntw) {
                const bf16x8 bf = head_tr_frag(imgB, browb, (wave * ntw + j) * 16, lane);
#pragma unroll
                for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                    for (int pl = 0; pl < 3; ++pl) acc[mt][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[mt][pl], bf, acc[mt][j], 0, 0, 0);
            }
        }
        __syncthreads();
    }
    if constexpr (WGRAD) {
        sdb[bs * kBwdTile + cl] = db;
        __syncthreads();
        if (threadIdx.x < kBwdTile && tile0 + (int)threadIdx.x < C) {
            float s = sdb[threadIdx.x];
#pragma unroll
            for (int k = 1; k < 8; ++k) s += sdb[k * kBwdTile + threadIdx.x];
            p.dbias[tile0 + threadIdx.x] = s;
        }
        const float s_norm = p.qp_norm[0];
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int c = tile0 + 16 * mt + 4 * g + e;
                if (c >= C) continue;
                const int ci = p.w_per_channel ? c : 0;
                const float inv = __fdiv_rn(1.0f, p.w_scale[ci]), fzp = (float)p.w_zp[ci];
#pragma unroll
                for (int j = 0; j < kMaxNT; ++j) {
                    if (j < ntw) {
                        const int64_t o = (int64_t)c * D + (wave * ntw + j) * 16 + idx;
                        p.dW[o] = ste_clips(p.W[o], inv, fzp, p.w_qmin, p.w_qmax) ? 0.f : acc[mt][j][e] * s_norm;
                    }
                }
            }
    } else {
        const int64_t rows = (int64_t)gridDim.x * kBwdTile;
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int b = tile0 + 16 * mt + 4 * g + e;
                if (b >= B) continue;
#pragma unroll
                for (int j = 0; j < kMaxNT; ++j)
                    if (j < ntw) p.partial[((int64_t)blockIdx.y * rows + b) * D + (wave * ntw + j) * 16 + idx] = acc[mt][j][e];
            }
    }
}

// dh = the class ranges' partial tiles summed in range order (the k_tn_reduce idiom), times a per-tensor weight scale
__global__ __launch_bounds__(256) void k_head_dgrad_reduce(const float* __restrict__ partial, int splits, int64_t stride, const float* __restrict__ w_scale,
                                                           int w_per_channel, float* __restrict__ dh, int64_t n) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    float s = partial[i];
    for (int k = 1; k < splits; ++k) s += partial[k * stride + i];
    dh[i] = w_per_channel ? s : s * w_scale[0];
}

struct DgradGeom { int row_tiles, splits, chunks_per_split; };
DgradGeom dgrad_geom(int B, int C) {
    DgradGeom q;
    q.row_tiles = cdiv(B, kBwdTile);
    const int chunks = cdiv(C, kBwdTile), want = std::min(chunks, std::max(1, kDgradGrid / q.row_tiles));
    q.chunks_per_split = cdiv(chunks, want);
    q.splits = cdiv(chunks, q.chunks_per_split);   // (no empty range)
    return q;
}

}  // namespace

bool head_mfma_covers(int D, int C) { return C >= kHeadMfmaMinClasses && C <= kHeadMfmaMaxClasses && D >= 64 && D % 64 == 0 && D <= 768; }

int64_t head_mfma_scratch_bytes(int B, int D, int C) {
    const DgradGeom q = dgrad_geom(B, C);
    return (int64_t)q.splits * q.row_tiles * kBwdTile * D * 4;
}

int launch_head_fwd_mfma(const float* x, const float* mean, const float* rstd, const float* gamma, const float* beta, const float* qp_norm, int qmin,
                         int qmax, const void* wq, const float* w_scale, int w_per_channel, const float* bias, float* hq, void* hq16, float* logits_pre,
                         uint32_t* stats, int stat_slots, int B, int D, int T, int C, hipStream_t st) {
    if (!head_mfma_covers(D, C) || B < 1) { set_error("head_fwd_mfma: B %d, D %d, C %d (needs D %% 64 == 0, D <= 768, 128 <= C <= 32768)", B, D, C); return 1; }
    k_head_rows_mfma<<<B, 256, 0, st>>>(x, mean, rstd, gamma, beta, qp_norm, qmin, qmax, hq, reinterpret_cast<__bf16*>(hq16), D, T);
    const size_t lds = (size_t)kFwdClasses * (D * 2 + kFwdPad);
    static bool once = (allow_lds(k_head_fwd_mfma, (size_t)kFwdClasses * (768 * 2 + kFwdPad)), true);
    (void)once;
    const int gx = cdiv(C, kFwdClasses);
    const int gy = std::min(cdiv(B, kFwdRows), std::max(1, cu_count() / gx));
    k_head_fwd_mfma<<<dim3(gx, gy), 256, lds, st>>>(reinterpret_cast<const __bf16*>(hq16), reinterpret_cast<const __bf16*>(wq), qp_norm, w_scale,
                                                    w_per_channel, bias, logits_pre, stats, stat_slots, B, D, C);
    return 0;
}

int launch_head_bwd_mfma(const float* dlogits, const float* logits_pre, const float* qp_logits, int qmin, int qmax, const void* hq16, const float* qp_norm,
                         const void* wq, const float* W, const float* w_scale, const int32_t* w_zp, int w_per_channel, int w_qmin, int w_qmax, float* dW,
                         float* dbias, float* dh, void* scratch, int B, int D, int C, hipStream_t st) {
    if (!head_mfma_covers(D, C) || B < 1) { set_error("head_bwd_mfma: B %d, D %d, C %d (needs D %% 64 == 0, D <= 768, 128 <= C <= 32768)", B, D, C); return 1; }
    const DgradGeom q = dgrad_geom(B, C);
    HeadBwdArgs a{};
    a.dlogits = dlogits; a.logits_pre = logits_pre; a.qp_logits = qp_logits; a.qmin = qmin; a.qmax = qmax;
    a.w_scale = w_scale; a.w_per_channel = w_per_channel; a.B = B; a.D = D; a.C = C;
    const size_t lds = (size_t)kBwdTile * (D * 2 + kBPad) + 3 * kAPlane + 8 * kBwdTile * sizeof(float);   // <= 58.9 KB
    HeadBwdArgs dg = a;
    dg.plane = reinterpret_cast<const __bf16*>(wq); dg.partial = reinterpret_cast<float*>(scratch); dg.chunks_per_split = q.chunks_per_split;
    k_head_bwd_mfma<false><<<dim3(q.row_tiles, q.splits), 256, lds, st>>>(dg);
    const int64_t n = (int64_t)B * D;
    k_head_dgrad_reduce<<<cdiv(n, 256), 256, 0, st>>>(dg.partial, q.splits, (int64_t)q.row_tiles * kBwdTile * D, w_scale, w_per_channel, dh, n);
    HeadBwdArgs wg = a;
    wg.plane = reinterpret_cast<const __bf16*>(hq16); wg.W = W; wg.w_zp = w_zp; wg.qp_norm = qp_norm; wg.w_qmin = w_qmin; wg.w_qmax = w_qmax;
    wg.dW = dW; wg.dbias = dbias;
    k_head_bwd_mfma<true><<<cdiv(C, kBwdTile), 256, lds, st>>>(wg);
    return 0;
}

}  // namespace qv
