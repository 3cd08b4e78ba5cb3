// Shared device/host helpers for libqatvit (gfx950 only: wave = 64 lanes).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include <memory>
#include <vector>

namespace qv {

constexpr int kWave = 64;

void set_error(const char* fmt, ...);
// the drop-path scale table bound to a step workspace, nullptr: none (capi.hip; include/qatvit.h qatvit_student_set_drop_path)
void drop_path_bind(const void* workspace, const float* table);
const float* drop_path_of(const void* workspace);
// the LayerScale binding of a step workspace, null: none (capi.hip; include/qatvit.h qatvit_student_set_layer_scale): per branch (row 2 i = block i's attention
// branch, 2 i + 1 = its MLP branch) the device address of gamma [embed_dim] and of its gradient; saved: the float forms' retained branch outputs
struct LayerScale {
    std::vector<const float*> gamma;
    std::vector<float*> grad;   // (empty: a forward-only binding)
    float* saved = nullptr;
};
void layer_scale_bind(const void* workspace, int branches, const float* const* gammas, float* const* grads, void* saved);
std::shared_ptr<const LayerScale> layer_scale_of(const void* workspace);

// The QATVIT_* knobs of the library, read from the environment once per process on first use (capi.hip).  Each one switches a form off for an
// A/B or bit-identity comparison (tests/test_gpu_knobs.py); unset = on, set = atoi(value) != 0.  Which form a configuration runs is decided from
// these and its shapes in one place: engine.hip Forms.
struct Knobs {
    bool i8;              // QATVIT_I8: the grid x grid forward GEMMs (patch-embed, qkv, fc1) on int8 MFMA; 0: bf16 MFMA (the same bits)
    bool f16;             // QATVIT_F16: the float operands of the proj / fc2 forward GEMMs as fp16 (hi, lo) pairs; 0: bf16 pairs (the round-1 arithmetic)
    bool fc2_codes;       // QATVIT_FC2_CODES: fc2's forward A operand as one byte per element + a 256-entry fp16-pair table; 0: the two fp16 planes
    bool fc1_bits;        // QATVIT_FC1_BITS: the backward's fc1 codes as that byte plane + one STE mask bit per element; 0: the uint16 code plane
    bool fc2w_codes;      // QATVIT_FC2W_CODES: fc2's weight gradient from the byte plane + a bf16-pair table; 0: from the bf16 (hi, lo) planes
    bool wbatch;          // QATVIT_WBATCH: weight preparation as three multi-tensor launches; 0: one launch triple per weight (the deep-model path)
    bool attn_codes;      // QATVIT_ATTN_CODES: the attention backward reads the codes its forward saved; 0: it re-quantises the fp32 qkv
    bool qkv_2pass;       // QATVIT_QKV_2PASS: the qkv GEMM as a statistics pass + a pass writing codes and mask bits; 0: once, fp32 output
    bool lnb_fuse;        // QATVIT_LNB_FUSE: the LayerNorm backward in the fc1 / qkv dgrad epilogue (embed_dim 384); 0: its own kernel
    bool qp_late;         // QATVIT_QP_LATE: the observer / qparams update inside the consumer kernel (QpLate); 0: a k_qparams launch behind the producer
    bool tn_stream;       // QATVIT_TN_STREAM: the one-plane weight gradients of a backward call as one stream-K launch per X form; 0: one launch per GEMM
    bool tn_q8;           // QATVIT_TN_Q8: one-plane weight gradients with a byte X operand (k_gemm_tn_q8); 0: the fp16-plane / expand-through-LDS kernels
    bool attn_bwd_fused;  // QATVIT_ATTN_BWD_FUSED: one fused attention backward kernel where its shape holds; 0: k_attn_bwd_dq + k_attn_bwd_dkv
    bool f16_strip;       // QATVIT_F16_STRIP: the one-plane fc2 dgrad on the A-stationary strip kernel; 0: the general tall tile
    bool i8_strip;        // QATVIT_I8_STRIP: the K = 384 / 768 int8 GEMMs on the A-stationary strip kernel; 0: the general tall kernel
    bool ln_strip;        // QATVIT_LN_STRIP: norm1 / norm2 apply + quantise inside the statistics pass of qkv / fc1 (launch_i8_strip_ln); 0: k_ln_apply_quant in front of it
    bool cls_bwd;         // QATVIT_CLS_BWD: the one-plane backward of the last block's MLP and proj on the B class-token rows (the only ones the cls-pooled head reaches); 0: all B * T rows
    bool attn_bwd_pipe;   // QATVIT_ATTN_BWD_PIPE: the fused attention backward as one persistent workgroup per CU that fetches its next head under the sweep (more heads than CUs); 0: one workgroup per head
};
const Knobs& knobs();
// compute units of the current device, asked once per process (capi.hip); 256 where the runtime does not say or says more: the size of persistent grids
int cu_count();

#define QV_CHECK_ARG(cond, ...)                 \
    do {                                        \
        if (!(cond)) {                          \
            qv::set_error(__VA_ARGS__);         \
            return 1;                           \
        }                                       \
    } while (0)

#define QV_CHECK_LAUNCH(name)                                                     \
    do {                                                                          \
        hipError_t e_ = hipGetLastError();                                        \
        if (e_ != hipSuccess) {                                                   \
            qv::set_error("%s: launch failed: %s", name, hipGetErrorString(e_));  \
            return 2;                                                             \
        }                                                                         \
    } while (0)

// Order-preserving float <-> uint32 map so min/max can use integer atomics.
__host__ __device__ inline uint32_t f2ord(float f) {
    uint32_t u = __builtin_bit_cast(uint32_t, f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__host__ __device__ inline float ord2f(uint32_t k) {
    uint32_t u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
    return __builtin_bit_cast(float, u);
}
constexpr uint32_t kOrdPosInf = 0xff800000u;  // f2ord(+inf)
constexpr uint32_t kOrdNegInf = 0x007fffffu;  // f2ord(-inf)

// Same-address atomics serialise at ~12 ns each on MI355X (measured: 32k atomicMin/Max on one word = 390 us),
// so a per-tensor min/max accumulator is kStatSlots {min,max} pairs, one 128-B line apart; a producer block
// uses pair (blockIdx & (kStatSlots-1)) and k_qparams folds the pairs.
constexpr int kStatSlots = 32;
constexpr int kStatStride = 32;  // uint32 words between pairs (128 B)
__device__ inline void stat_atomic(uint32_t* stats, int nslots, float mn, float mx) {
    uint32_t* s = stats + (nslots > 1 ? (int)(blockIdx.x & (nslots - 1)) * kStatStride : 0);
    atomicMin(&s[0], f2ord(mn));
    atomicMax(&s[1], f2ord(mx));
}

__device__ inline float wave_min(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ inline float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ inline float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// The one rounding rule of fake-quant (ATen cachemask kernels):
//   q = nearbyint(x * inv_scale) + zp ; y = (clamp(q) - zp) * scale ; mask = q in [qmin,qmax]
// fq/fzp/fqmin/fqmax are small integers held in fp32 (exact).
__device__ inline float fq_one(float x, float inv_scale, float scale, float fzp, float fqmin, float fqmax, bool& in_range) {
    float q = rintf(x * inv_scale) + fzp;
    in_range = (q >= fqmin) && (q <= fqmax);
    float qc = fminf(fmaxf(q, fqmin), fqmax);
    return (qc - fzp) * scale;
}

inline int cdiv(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }

// exp(x) for x <= 0 as one v_exp_f32 (2^y) after a multiply by log2(e): the attention kernels are VALU-bound and the libm
// expf expands to ~20 instructions; v_exp_f32 is accurate to ~1 ulp, far inside the 3e-5 kernel tolerance.
__device__ inline float fast_exp(float x) { return __builtin_amdgcn_exp2f(x * 1.4426950408889634f); }

// float -> bf16 (hi, lo) splits two elements per instruction: v_cvt_pk_bf16_f32 on a PAIR (a per-element (__bf16) cast costs one v_cvt_pk plus a
// shift to pack), the hi parts back to fp32 by shift / mask, the residuals by one v_pk_add_f32.  Same roundings, same bits as the per-element form.
// (The attention sweeps issued 290 VALU instructions per 64 MFMAs before this; the GEMM epilogues that write pairs use it too.)
typedef float qv_f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 qv_bf16x2 __attribute__((ext_vector_type(2)));
__device__ inline uint32_t pk_bf16(float a, float b) {
    const qv_f32x2 v = {a, b};
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, qv_bf16x2));
}
// two floats -> packed fp16 (round to nearest even): one v_cvt_pk_f16_f32
typedef _Float16 qv_f16x2 __attribute__((ext_vector_type(2)));
__device__ inline uint32_t pk_f16(float a, float b) {
    const qv_f32x2 v = {a, b};
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, qv_f16x2));
}
__device__ inline void split_pair(float a, float b, uint32_t& hi, uint32_t& lo) {
    const qv_f32x2 v = {a, b};
    hi = __builtin_bit_cast(uint32_t, __builtin_convertvector(v, qv_bf16x2));
    const qv_f32x2 h = {__builtin_bit_cast(float, hi << 16), __builtin_bit_cast(float, hi & 0xffff0000u)};
    const qv_f32x2 r = v - h;
    lo = __builtin_bit_cast(uint32_t, __builtin_convertvector(r, qv_bf16x2));
}

// exact-erf GELU (nn.GELU() default) and its derivative
__device__ inline float gelu_fwd(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752f)); }
// GELU for the frozen teacher's fused fc1 epilogue (no quantisation grid there, so no table): erfc by Abramowitz-Stegun 7.1.26
// (|error| <= 1.5e-7 absolute, the size of erff's own rounding), one exp2 + one rcp + five FMAs instead of libm's erff.
// 0.5 x (1 + erf(x / sqrt 2)) is evaluated through erfc on the side that would cancel: x < 0 -> 0.5 x E, x >= 0 -> x (1 - 0.5 E).
__device__ inline float gelu_fwd_fast(float x) {
    const float z = fabsf(x) * 0.70710678118654752f;
    const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f, z, 1.0f));
    float pl = fmaf(1.061405429f, t, -1.453152027f);
    pl = fmaf(pl, t, 1.421413741f);
    pl = fmaf(pl, t, -0.284496736f);
    pl = fmaf(pl, t, 0.254829592f);
    const float E = pl * t * __builtin_amdgcn_exp2f(-z * z * 1.4426950408889634f);   // erfc(z)
    return x < 0.f ? 0.5f * x * E : x * (1.0f - 0.5f * E);
}
__device__ inline float gelu_bwd(float x) {
    return 0.5f * (1.0f + erff(x * 0.70710678118654752f)) + x * 0.3989422804014327f * expf(-0.5f * x * x);
}

}  // namespace qv
