// Internal C++ launch interface shared by the C ABI (capi.hip) and the step engine.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace qv {

int launch_fq_forward(const float* x, float* y, uint8_t* mask_bits, float* running_min, float* running_max, float* scale,
                      int32_t* zero_point, const int64_t* observer_on, const int64_t* fake_quant_on, float c, int qmin, int qmax,
                      int64_t channels, int64_t inner, bool per_channel, bool symmetric, void* workspace, hipStream_t st);
int launch_fq_backward(const float* dy, const uint8_t* mask_bits, float* dx, int64_t n, hipStream_t st);

int launch_ln_forward(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd, int64_t rows,
                      int64_t dim, float eps, hipStream_t st);
int launch_ln_backward(const float* dy, const float* x, const float* gamma, const float* mean, const float* rstd, float* dx,
                       float* dgamma, float* dbeta, int64_t rows, int64_t dim, hipStream_t st);

int launch_kd_ce_loss(const float* student, const float* teacher, const int64_t* labels, int64_t batch, int64_t classes, float kd_temp,
                      float kd_alpha, float label_smoothing, float* out3, float* dlogits, hipStream_t st);
int launch_kd_ce_loss_table(const float* student, const float* table, int64_t table_rows, const int64_t* index, const int64_t* labels, int64_t batch,
                            int64_t classes, float kd_temp, float kd_alpha, float label_smoothing, float* out3, float* dlogits, hipStream_t st);
// the same two with mixed targets (mix int32 [B][6], include/qatvit.h): teacher [B, C], or table + index, or neither; mix == nullptr: the launchers above
int launch_kd_ce_loss_mix(const float* student, const float* teacher, const float* table, int64_t table_rows, const int64_t* index,
                          const int64_t* labels, const int32_t* mix, int64_t batch, int64_t classes, float kd_temp, float kd_alpha,
                          float label_smoothing, float* out3, float* dlogits, hipStream_t st);

// ---- bce.hip: KD + binary cross-entropy on the same targets, one wave per row and a fixed-order reduction of partials[2 * batch] (two launches)
int launch_kd_bce_loss(const float* student, const float* teacher, const float* table, int64_t table_rows, const int64_t* index,
                       const int64_t* labels, const int32_t* mix, int64_t batch, int64_t classes, float kd_temp, float kd_alpha,
                       float label_smoothing, float target_threshold, bool sum_classes, float* partials, float* out3, float* dlogits,
                       hipStream_t st);

// ---- fq.hip (engine pieces)
int launch_minmax(const float* x, int64_t channels, int64_t inner, int per_channel, uint32_t* ws, int nslots, hipStream_t st);
int launch_ws_init(uint32_t* ws, int64_t slots, hipStream_t st);
int launch_qparams(uint32_t* ws, float* running_min, float* running_max, float* scale, int32_t* zero_point, const int64_t* observer_on,
                   const int64_t* fake_quant_on, float c, int qmin, int qmax, int64_t channels, int symmetric, float* qp_out, int reset_ws,
                   int nslots, hipStream_t st);

// the late-resolved quantizers' staged states -> module buffers (qv_qparams.h QpLate; fq.hip k_qp_commit): per activation quantizer the four buffers; the
// staging records and the accumulators are workspace arrays indexed by the quantizer
constexpr int kMaxActFq = 96;   // 2 + 6 per block (depth <= 12) + 2, with slack
struct QpCommitTab { float* rmin[kMaxActFq]; float* rmax[kMaxActFq]; float* scale[kMaxActFq]; int32_t* zp[kMaxActFq]; float* staged; uint32_t* stats; int n; };
int launch_qp_commit(const QpCommitTab& t, hipStream_t st);
// how a consumer kernel obtains the qparams of the quantizer it applies (device side: qv_qparams.h qp_late_resolve)
struct QpLate {
    const uint32_t* stats;     // kStatSlots accumulator pairs; nullptr: not late - the consumer reads the ready values (k_qparams ran)
    const float* rmin; const float* rmax; const float* scale; const int32_t* zp;   // the module's buffers: READ ONLY in the consumer
    const int64_t* obs_on; const int64_t* fq_on;
    float c; int qmin, qmax;
    float* qp_out;             // {scale, 1 / scale, zp, on}: what k_qparams publishes
    float* staged;             // kQpStagedWords words: new min, new max, new scale, new zp (int bits), flags (1: min / max moved, 2: scale / zp moved, 4: pending)
};
constexpr int kQpStagedWords = 8;

// ---- the epilogues of the NT GEMMs: NTPost::mode, and the kernels' template parameter (PM of k_gemm_nt, MODE of k_i8_strip).  post == nullptr is kEpiPlain; a
// post record names one of the others.  THE table (forms: the NTForm of launch_gemm_nt, below - bf16 = kNTBf16, f16 = kNTF16, i8 = kNTI8, codes = kNTCodes,
// plane = kNTPlaneF16; strip = launch_i8_strip, f16strip = launch_f16_strip_gelu_bwd); qp / qmin / qmax = the quantizer every mode but 0 / 2 / 3 applies:
//   mode               stores                                                                          NTPost fields read                              forms
//   kEpiPlain      0   C fp32; min / max of C -> stats                                                 -                                               all
//   kEpiGeluFwd    2   (hi, lo) of gelu(C): bf16, or (out_f16) fp16, where out_lo may be NULL          out_hi out_lo out_f16                           bf16, f16 (teacher fc1)
//   kEpiStats      3   nothing; min / max -> stats (first pass of a recomputed K = 384 / 768 GEMM)     -                                               bf16, i8, strip
//   kEpiCodes      4   gelu(fq(C)), whichever planes are set: bf16 (hi, lo) + uint16 code              out_hi out_lo code | out16_hi out16_lo           bf16 (bf16 pair + code), i8,
//                      (q - qmin) | in_range << 15; fp16 (hi, lo) * 2^k with *out16_scale = 2^-k;      out16_scale | out8 out8_mask lut_out lutq_out    strip (out8 + out8_mask +
//                      uint8 grid index [M, ldc] + STE mask bits [M, ldc / 8] + the 256-entry tables                                                    both tables only)
//                      of fp16 / bf16 (hi | lo << 16) pairs of gelu(grid value) (fc1 second pass)
//   kEpiGeluBwdU16 5   (hi, lo) of C * gelu'(grid value) * in_range * colscale, from uint16 codes      code colscale out_hi out_lo                     bf16
//   kEpiResidFq    6   C[orow] = resid[rrow] + fq(acc), frozen qp (embed_np > 0: input row b * np + p  resid embed_np                                  f16, i8, codes
//                      -> token row b * (np + 1) + 1 + p, resid = pos_embed rows 1 + p)
//   kEpiQkvCodes   7   out8 = clamp(q) - qmin as uint8 in the attention layout [b][h][which][t][d];    out8 out8_mask code_T code_hd                   i8, strip
//                      out8_mask (optional; head_dim % 32 == 0): the STE mask bits in the same order
//   kEpiLnBwd      8   C = dx_out = dx_in + LNbwd(acc * alpha * mask(LN(x))), dgamma / dbeta += ;      lnb_* colscale out_hi out_lo                    bf16 (split A), plane
//                      (out_hi set) the (hi, lo) of dx_out * nmask * colscale for the next branch.     (plane: o16_mul o16_amax, no out_lo)
//                      N == ldc == 384: the tile holds whole LayerNorm rows; qp = the LN output's
//   kEpiGeluBwdU8  9   as 5, from one byte per code + one mask bit per element                         code8 code_mask colscale out_hi out_lo          bf16 (split A), plane, f16strip
//                      (bit c % 8 of byte (row * ldc + c) / 8): what mode 4 leaves in out8 / out8_mask (plane / f16strip: o16_mul o16_amax, no out_lo)
//   kEpiResidFqLs 11   C[orow] = resid[rrow] + __fmul_rn(fq(acc), ls_gamma[col]): mode 6 under LayerScale,    resid embed_np ls_gamma                         f16, codes
//                      product and sum rounded separately (what k_resid_fq_lnstats_ls of elt_rows.inc
//                      computes); ls_gamma == 1 gives the bits of mode 6
//   plane / f16strip emit the gradient as ONE fp16 plane (out_hi) of value * (*o16_mul) and accumulate max |value| into o16_amax (dy16.hip: Dy16Slot::amax).
// The numbers are fixed: qatvit_i8_strip takes 3 / 4 / 7 (include/qatvit.h), -DQV_NT_EXPERIMENTS=<mode> and tools/stamp_nt.py / stamp_i8strip.py pass them.
// (11: the numbers 10, 18 and 19 are instantiation ids of gemm.hip - kPmCodesF16, and mode + 10 of the plane forms' 8 / 9)
enum NTEpi : int {
    kEpiPlain = 0, kEpiGeluFwd = 2, kEpiStats = 3, kEpiCodes = 4, kEpiGeluBwdU16 = 5, kEpiResidFq = 6, kEpiQkvCodes = 7, kEpiLnBwd = 8, kEpiGeluBwdU8 = 9,
    kEpiResidFqLs = 11
};
static_assert(kEpiStats == 3 && kEpiCodes == 4 && kEpiQkvCodes == 7, "the modes of qatvit_i8_strip (include/qatvit.h)");
struct NTPost {
    int mode = kEpiPlain;           // an NTEpi other than kEpiPlain
    const float* qp = nullptr;      // {scale, 1/scale, zp, enabled}
    int qmin = 0, qmax = 0;
    const float* colscale = nullptr;   // optional [N]
    void* out_hi = nullptr;
    void* out_lo = nullptr;
    int out_f16 = 0;
    void* code = nullptr;           // uint16 [M, ldc]
    void* out16_hi = nullptr;
    void* out16_lo = nullptr;
    float* out16_scale = nullptr;
    const float* resid = nullptr;
    int embed_np = 0;
    void* out8 = nullptr;
    void* out8_mask = nullptr;
    int code_T = 0, code_hd = 0;
    uint32_t* lut_out = nullptr;    // fp16 pairs: the A operand of kNTCodes with out8 (fc2 forward from 1 B per element)
    uint32_t* lutq_out = nullptr;   // bf16 pairs: the kTNPairCodes weight gradient (fc2)
    const void* code8 = nullptr;
    const void* code_mask = nullptr;
    const float* lnb_x = nullptr;
    const float* lnb_mean = nullptr;
    const float* lnb_rstd = nullptr;
    const float* lnb_gamma = nullptr;
    const float* lnb_beta = nullptr;
    const float* lnb_dx_in = nullptr;
    float* lnb_dgamma = nullptr;
    float* lnb_dbeta = nullptr;
    const void* lnb_nmask = nullptr;   // the next branch output's STE mask words
    const float* o16_mul = nullptr;
    uint32_t* o16_amax = nullptr;
    const float* ls_gamma = nullptr;   // fp32 [N]: the branch's LayerScale gamma (mode 11)
};

// ---- the NT GEMMs (gemm.hip): one request record, six named operand forms, one launcher.  A request computes, for the epilogue its NTPost names (NTEpi above),
//   C[m, n] = (sum_k A[m, k] * B[n, k]) * (*s1) * (*s2) * col_scale[n] + bias[n]        min / max of the stored values -> stats (stat_slots pairs)
// THE table (every form: M >= 1, ldc % 4 == 0; lda / ldb count elements of A / B as stored; s1, s2, col_scale, bias, stats optional; pair = (hi, lo) planes whose sum is the value; integers = grid values, exact):
//   form              A, A_lo                         B, B_lo                                 required        N %, K %, lda %, ldb %   epilogues (NTEpi numbers)
//   kNTBf16       0   bf16 plane (integers) or pair   bf16 plane (integers) or pair (A too)   -               128, 64, 8, 8            0 2 3 4 5; 8 9: A_lo, no B_lo, N % 384 == 0
//   kNTF16        1   fp16 plane or pair              fp16 plane (integers), -                -               384, 64, 8, 8            0; 6 11: A_lo; 2: out_f16
//   kNTI8         2   int8 q - center, -              int8 integers, -                        wsum [N], a_qp  384, 64, 16, 16          0 3 4 6 7
//   kNTCodes      3   uint8 indices of lut, -         fp16 plane (integers), -                A, B, C, lut    384, 64, 16, 8           0 6 11
//   kNTPlaneF16   4   ONE fp16 plane of value * 2^e   fp16 plane (integers), -                A, B            384, 32, 8, 8            0; 8 9: o16_mul / o16_amax, K % 64 == 0
//   kNTPlaneBf16  5   ONE bf16 plane                  bf16 plane, -                           A, B            384, 32, 8, 8            0
// lut: 256 packed fp16 (hi | lo << 16) pairs, A is expanded through it inside the kernel.  wsum / a_qp / center: the row sums of B and the A operand's quantizer {scale, 1 / scale,
// zero point, ..}: C = (acc + (center - zp) * wsum[n]) * ..; with B_frag the strip kernel takes what launch_i8_strip covers, and `late` (the output quantizer's qparams resolved in a
// code pass) exists there only.  The plane forms are the one-plane backward ("dY as one fp16 plane"): *s2 = 2^-e.  A field a form's row does not name is not read.
enum NTForm : int { kNTBf16 = 0, kNTF16 = 1, kNTI8 = 2, kNTCodes = 3, kNTPlaneF16 = 4, kNTPlaneBf16 = 5, kNTForms = 6 };
struct NTGemm {   // one NT GEMM without its epilogue
    const void* A = nullptr; const void* A_lo = nullptr; const void* B = nullptr; const void* B_lo = nullptr;
    const void* B_frag = nullptr;      // B once more, in the strip kernels' fragment order (i8strip.hip: int8, w8f_offset; f16strip.hip: fp16 on 768-byte rows)
    const uint32_t* lut = nullptr; const int32_t* wsum = nullptr; const float* a_qp = nullptr; int center = 0;
    float* C = nullptr; int M = 0, N = 0, K = 0, lda = 0, ldb = 0, ldc = 0;   // C: fp32 [M, ldc]
    const float* s1 = nullptr; const float* s2 = nullptr; const float* col_scale = nullptr; const float* bias = nullptr;   // scalars; [N]
    uint32_t* stats = nullptr; int stat_slots = 1; const QpLate* late = nullptr;
};
int launch_gemm_nt(NTForm form, const NTGemm& g, const NTPost* post, hipStream_t st);
// ---- f16strip.hip: the fc2 dgrad + GELU backward of the one-plane backward, A-stationary (K = 384, N = 1536): a kNTPlaneF16 request with epilogue mode 9 whose
// B_frag holds the transposed weight integers as fp16 in fragment order (B, ldb, C unread).  true when it took the request; false -> launch_gemm_nt
bool launch_f16_strip_gelu_bwd(const NTGemm& g, const NTPost* post, hipStream_t st);
// ---- i8strip.hip: the K = 384 / 768 two-pass forward GEMMs (qkv, fc1), A-stationary: a kNTI8 request read through B_frag (B, ldb, C unread; the code passes
// take g.late).  true when it covered (and launched) the request; force: whatever the knob says
bool launch_i8_strip(const NTGemm& g, const NTPost* post, hipStream_t st, bool force = false);
// would launch_i8_strip take this request (B_frag, M, N, K, lda, ldc), given s1, the accumulator (statistics pass) and ready or late qparams (code passes)?  The
// same predicate as the launcher's; the knob applies (the engine decides on it BEFORE the statistics pass whether a k_qparams launch has to follow it)
bool i8_strip_covers(const NTGemm& g, const NTPost* post);
// The statistics pass with the LayerNorm apply + quantise in its prologue (k_ln_apply_quant's work, the same bits): every workgroup builds its strip from the
// fp32 rows x [M, K] (mean / rstd [M], gamma / beta [K]), keeps it in LDS and stores it to out8 [M, lda] (q - center), the plane the code pass and the weight
// gradients read.  The A operand's quantizer is `late` (resolved inside; workgroup 0 publishes it) or, without it, the ready g.a_qp; g.A, g.s1 (that quantizer's
// scale) and g.ldc are not read.  i8_strip_ln_covers: would it take B_frag, M, N, K, lda (QATVIT_LN_STRIP, one workgroup per strip: N == 3 / 4 (K = 768: 6 / 8) x 384)?
struct StripLn { const float *x = nullptr, *mean = nullptr, *rstd = nullptr, *gamma = nullptr, *beta = nullptr; int qmin = 0, qmax = 0; void* out8 = nullptr; const QpLate* late = nullptr; };
bool launch_i8_strip_ln(const NTGemm& g, const StripLn& ln, hipStream_t st, bool force = false);
bool i8_strip_ln_covers(const NTGemm& g);
// byte offset of element (n, k) of an [N, K] int8 weight in fragment order: [48-column group][64-deep k-step][16-column fragment][lane = 16 (k % 64 / 16) + n % 16][k % 16]
__host__ __device__ inline int64_t w8f_offset(int n, int k, int K) {
    const int cg = n / 48, cr = n % 48, j = cr / 16, r = cr % 16, kt = k / 64, kk = k % 64;
    return ((((int64_t)cg * (K / 64) + kt) * 3 + j) * 64 + (kk / 16) * 16 + r) * 16 + (kk % 16);
}
int launch_w8_fragment_order(const void* B8, void* B8f, int N, int K, hipStream_t st);   // N % 48 == 0, K % 64 == 0
// ---- the weight gradients (TN GEMMs of gemm.hip): one request record, six named operand forms, two launchers.  A request computes
//   C[n, kw] += mask(W)[n, kw] * sum_m P[m, n] * X[m, kw] * (*s1) * (*s2) / row_div[n]        dbias[n] += sum_m P[m, n] * (*s2) / row_div[n]
// with the gradient P [M, ldp] and the layer input X [M, Kw] given by Q.  THE table (every form: N % 128 == 0, ldp % 8 == 0; ldq counts elements of Q as stored;
// s2, W, dbias, row_div optional; a "pair" is (hi, lo) planes whose sum is the value; launch_tn_stream takes the first three forms, with Kw % 384 == 0 and s1):
//   form              P, P_lo            Q, Q_lo                                     lut                      s1                            center   Kw %, ldq %
//   kTNPlaneQ8     0  fp16 plane, -      int8 grid plane q - center, -               -                        the activation's {scale,      read     384, 16
//                                                                                                             1 / scale, zero point, ..}
//   kTNPlaneCodes  1  fp16 plane, -      uint8 table indices, -                      256 fp16 (hi | lo << 16) X's scale                     -        384, 16
//                                                                                    pairs, hi half used
//   kTNPlaneF16    2  fp16 plane, -      fp16 plane (grid integers), optional lo     -                        X's scale, optional           -        128, 8
//                                        plane of an fp16 pair (per-GEMM launch only)
//   kTNPlaneBf16   3  bf16 plane, -      bf16 plane, optional lo plane               -                        optional                      -        128, 8
//   kTNPair        4  bf16 pair          bf16 plane (grid integers), optional lo     -                        optional                      -        128, 8
//   kTNPairCodes   5  bf16 pair          uint8 table indices, -                      256 bf16 (hi | lo << 16) optional                      -        384, 16
//                                                                                    pairs
// The one-plane forms (0 - 3; DESIGN.md section 4, "dY as one fp16 plane"): P = the gradient * 2^e, *s2 = 2^-e.  X of kTNPlaneQ8 = Q + center - s1[2], expanded to
// fp16 in registers (k_gemm_tn_q8); the byte forms read ldq in bytes.  The numbers 0 / 1 / 2 are the `mode` of qatvit_gemm_tn_stream_dy16 (include/qatvit.h).
enum TNForm : int { kTNPlaneQ8 = 0, kTNPlaneCodes = 1, kTNPlaneF16 = 2, kTNPlaneBf16 = 3, kTNPair = 4, kTNPairCodes = 5, kTNForms = 6 };
static_assert(kTNPlaneQ8 == 0 && kTNPlaneCodes == 1 && kTNPlaneF16 == 2, "the modes of qatvit_gemm_tn_stream_dy16 (include/qatvit.h)");
struct TNGemm {   // one weight gradient
    const void* P = nullptr; const void* P_lo = nullptr;
    const void* Q = nullptr; const void* Q_lo = nullptr;
    const uint32_t* lut = nullptr;
    const float* s1 = nullptr; const float* s2 = nullptr;
    float* C = nullptr;                // fp32 [N, ldc], accumulated into
    // fp32 [N, ldc]: the weight whose fake-quant STE mask applies, with its scale and zero point ([1], or [N] with TNCall::w_per_channel)
    const float* W = nullptr; const float* w_scale = nullptr; const int32_t* w_zp = nullptr;
    float* dbias = nullptr;            // [N]
    const float* row_div = nullptr;    // [N]: P was pre-multiplied by the per-channel weight scale
    int N = 0, Kw = 0, ldp = 0, ldq = 0, ldc = 0;
};
struct TNCall {   // what the weight gradients of one call share
    int M = 0;                         // token rows
    int center = 0;                    // kTNPlaneQ8
    int w_per_channel = 0, w_qmin = 0, w_qmax = 0;
    float* scratch = nullptr;          // launch_gemm_tn: optional, kTnScratchBytes let every shape take the two-phase (non-atomic, bit-reproducible) split reduction;
    int64_t scratch_bytes = 0;         // launch_tn_stream: required, >= tn_stream_scratch_bytes()
    // launch_gemm_tn: the two-phase form for a single split too.  The kernel's own tail is 96 dependent round trips per lane (weight load -> STE mask -> atomic),
    // about 60 us whatever M is; over a few hundred token rows that is the whole run time, and k_tn_reduce does the same work one element per thread
    bool reduce_single = false;
};
constexpr int64_t kTnScratchBytes = 256ll * 128 * 384 * 4;   // 256 workgroups x the largest tile
int64_t tn_stream_scratch_bytes();
int launch_gemm_tn(TNForm form, const TNGemm& g, const TNCall& call, hipStream_t st);
// n <= kTnStreamMax weight gradients of one form over the same token rows as one persistent stream-K launch (gemm.hip k_tn_stream) + its fix-up
constexpr int kTnStreamMax = 24;
int launch_tn_stream(TNForm form, const TNGemm* items, int n, const TNCall& call, hipStream_t st);
// ---- elt.hip
int launch_img_patches(const float* img, void* out_bf16, const float* qp, int qmin, int qmax, int B, int C, int H, int W, int P, hipStream_t st,
                       void* out8 = nullptr, int center = 0);
int launch_resid_fq_lnstats(int mode, const float* x_prev, const float* Y, const float* qpY, int qmin, int qmax, const float* cls, const float* pos,
                            float* x_new, float* mean, float* rstd, const float* gamma, const float* beta, float eps, uint32_t* stats, int stat_slots,
                            int64_t M, int D, int T, hipStream_t st, void* maskbits = nullptr, const QpLate* late = nullptr,   // late: Y's qparams are resolved inside (QpLate)
                            const float* drop_scale_rows = nullptr,   // mode 1, optional: x_new = x_prev + fq(Y) * drop_scale_rows[row / T] (drop-path; [M / T] floats)
                            const float* ls_gamma = nullptr);   // mode 1, optional: LayerScale - x_new = x_prev + (fq(Y) * ls_gamma[column]) * multiplier (k_*_ls, with or without drop-path)
// STE mask of an [M, D] tensor as wave ballots: ceil(D / 256) * 4 64-bit words per row (written by launch_resid_fq_lnstats mode 1)
inline int64_t ln_maskbits_bytes(int64_t M, int D) { return M * ((D + 255) / 256) * 32; }
// optional second output of launch_ln_bwd_fq: split(dx_out * mask * colscale) for the next branch's GEMMs (out_lo == nullptr without o16_*: its hi part
// only, ONE bf16 plane)
struct LnBwdNext {
    const void* maskbits; const float* colscale; void* out_hi; void* out_lo; const float* o16_mul = nullptr; uint32_t* o16_amax = nullptr;   // o16_*: out_hi is ONE fp16 plane (dy16.hip)
    // drop-path: that branch's per-sample multipliers, also a factor of its gradient - drop_scale[row / drop_rows], drop_rows = rows per sample (T over [B * T, D]
    // rows, 1 over the compact class-token rows [B, D])
    const float* drop_scale = nullptr; int drop_rows = 0;
    // LayerScale: that branch's gamma [D], also a factor of its gradient, and what gamma's own gradient needs - ls_dgamma [D] (accumulated into), the branch output
    // ls_Y (row r of this call is its row r * ls_ymul: 1, or T over the compact class-token rows), taken as fq(ls_Y) under the qparams ls_qp or, ls_qp null, rounded
    // as ls_kind says (0: fp32, 1: fp16, 2: bf16).  With ls_gamma set, drop_scale may be null (drop_rows is still needed)
    const float* ls_gamma = nullptr; float* ls_dgamma = nullptr; const float* ls_Y = nullptr; int ls_ymul = 1; const float* ls_qp = nullptr; int ls_kind = 0;
};
int launch_ln_apply_quant(const float* x, const float* mean, const float* rstd, const float* gamma, const float* beta, const float* qp, int qmin,
                          int qmax, void* out_bf16, int64_t M, int D, hipStream_t st, void* out8 = nullptr, int center = 0,
                          bool out_f16 = false,   // out_f16: the integers as fp16 bit patterns (X operand of the one-plane weight gradient)
                          const QpLate* late = nullptr);
// inference: LayerNorm + quantise (frozen qparams) in one pass -> int8 (q - center); out8 == nullptr: row statistics only; row_stride > 1: every
// row_stride-th row (cls tokens)
int launch_ln_quant8(const float* x, const float* gamma, const float* beta, float eps, const float* qp, int qmin, int qmax, int center, void* out8,
                     float* mean, float* rstd, int64_t nrows, int64_t row_stride, int D, hipStream_t st);
int launch_cls_rows(const float* cls, const float* pos, float* x, int B, int T, int D, hipStream_t st);
int launch_mask_bwd(int gelu_bwd, const float* d, const float* Y, const float* qp, int qmin, int qmax, const float* col_scale, int ncols,
                    void* dst_hi, void* dst_lo, int64_t n, hipStream_t st, const float* o16_mul = nullptr, uint32_t* o16_amax = nullptr,
                    const float* drop_scale_rows = nullptr, int T = 0,   // plain mask, optional: also * drop_scale_rows[row / T] (a residual branch under drop-path)
                    const float* ls_gamma = nullptr);   // ... and * ls_gamma[column] (LayerScale; needs T, drop_scale_rows may then be null)
int launch_ln_bwd_fq(int acc, const float* dH, const float* x, const float* mean, const float* rstd, const float* gamma, const float* beta,
                     const float* qp, int qmin, int qmax, const float* dx_in, float* dx_out, float* dgamma, float* dbeta, int64_t M, int D, int T,
                     int cls_only, hipStream_t st, const LnBwdNext* next = nullptr,
                     int rows_per_wave = 16);   // 16: few blocks, few same-address dgamma / dbeta atomics; 1 for a few hundred rows, where a wave's rows in sequence are the run time
// Every T-th row of up to kRowMoveMax tensors in one launch (the class-token rows b * T of [B * T, .] operands): `width` bytes per row, % 4 == 0, as is the
// tall tensor's row stride `stride` (bytes, >= width).  gather: compact[b] = tall[b * T] for b < rows.  scatter: the whole tall tensor is written - row b * T
// from compact[b], zeros everywhere else (a kernel, as k_zero_i32 is: no memset node in a captured graph) - with width == stride, % 16 == 0, and 16-byte aligned bases
constexpr int kRowMoveMax = 8;
struct RowMove { const void* src; void* dst; int64_t stride; int width; };
struct RowMoveTab { RowMove m[kRowMoveMax]; int n = 0; };
int launch_rows_gather(const RowMoveTab& t, int rows, int T, hipStream_t st);
int launch_rows_scatter(const RowMoveTab& t, int rows, int T, hipStream_t st);
int launch_head_fwd(const float* x, const float* mean, const float* rstd, const float* gamma, const float* beta, const float* qp_norm, int qmin,
                    int qmax, const void* wq, const float* w_scale, int w_per_channel, const float* bias, float* hq, float* logits_pre,
                    uint32_t* stats, int stat_slots, int B, int D, int T, int C, hipStream_t st);
int launch_logits_fq(const float* pre, const float* qp, int qmin, int qmax, float* out, int n, hipStream_t st);
int launch_head_bwd(const float* dlogits, const float* logits_pre, const float* qp_logits, int qmin, int qmax, const float* hq, const float* qp_norm,
                    const void* wq, const float* W, const float* w_scale, const int32_t* w_zp, int w_per_channel, int w_qmin, int w_qmax, float* dW,
                    float* dbias, float* dh, int B, int D, int C, hipStream_t st);
int launch_embed_bwd(const float* dx0, const float* Y0, const float* qp, int qmin, int qmax, float* dpos, float* dcls, void* dY0_hi, void* dY0_lo,
                     int B, int T, int D, hipStream_t st);
// ---- all weights of the step at once (three launches instead of three per weight): tables passed by value as kernel arguments
constexpr int kMaxW = 52;   // patch-embed + 4 per block (depth <= 12) + head, with slack
struct WObsTab { const float* W[kMaxW]; uint32_t* ws[kMaxW]; int N[kMaxW], K[kMaxW], blk0[kMaxW + 1]; int n, per_channel, nslots; };
struct WQpTab {
    uint32_t* ws[kMaxW]; float* rmin[kMaxW]; float* rmax[kMaxW]; float* scale[kMaxW]; int32_t* zp[kMaxW]; float* qp[kMaxW];
    const int64_t* obs_on[kMaxW]; const int64_t* fq_on[kMaxW]; int N[kMaxW], blk0[kMaxW + 1]; int n, per_channel, nslots, qmin, qmax; float c;
};
struct WQuantTab {
    const float* W[kMaxW]; const float* qp[kMaxW]; void* wq[kMaxW]; void* wqT[kMaxW]; void* w8[kMaxW]; int32_t* wsum[kMaxW];   // w8 / wsum optional (int8 copies + row sums)
    void* w16[kMaxW];   // optional: the same integers as fp16 (B operand of the fp16-pair forward GEMMs: proj, fc2)
    void* w8f[kMaxW];   // optional: the int8 integers once more in fragment order (w8f_offset: B operand of the strip kernel; N % 48 == 0, K % 64 == 0)
    int N[kMaxW], K[kMaxW], blk0[kMaxW + 1]; int n, per_channel, qmin, qmax;
    int wT16;           // nonzero: every wqT[i] is followed, wT16_gap_bytes(N, K) further on, by the same transposed integers as fp16 (the table itself is at the 4-KiB kernel-argument limit)
    unsigned long long wT16f_mask;   // bit i: ... and, another gap further, by those fp16 integers in MFMA fragment order (fc2 of ViT-S: the B operand of f16strip.hip; K % 48 == 0, 2 N % 64 == 0)
};
__host__ __device__ inline int64_t wT16_gap_bytes(int N, int K) { return ((int64_t)N * K * 2 + 255) & ~(int64_t)255; }
int launch_w_observe_all(WObsTab& t, hipStream_t st);      // fills blk0
int launch_w_qparams_all(WQpTab& t, hipStream_t st);       // fills blk0
int launch_w_quant_all(WQuantTab& t, hipStream_t st);      // fills blk0
int launch_zero_i32(int32_t* p, int64_t n, hipStream_t st);
// ---- observe-only forward (fq.hip): every observer of a forward folded in ONE launch.  One 64-lane workgroup per per-tensor entry (nslots
// accumulator pairs), ceil(channels / 64) per per-channel entry (2 words per channel); qparams_body with reset_ws = 0 and no qp output: observer_on = 0
// leaves running_min / max as they are, fake_quant_on = 0 leaves scale / zero_point.  tab: DEVICE array of n entries, blk0 ascending from 0.
struct ObsFoldEntry {
    uint32_t* ws; float* rmin; float* rmax; float* scale; int32_t* zp; const int64_t* obs_on; const int64_t* fq_on;
    int32_t channels, nslots, symmetric, qmin, qmax, blk0;
};
int launch_obs_fold(const ObsFoldEntry* tab, int n, int nblocks, float c, hipStream_t st);
int launch_wquant(const float* W, const float* qp, int per_channel, int qmin, int qmax, void* wq, void* wqT, int N, int K, hipStream_t st);

// ---- dy16.hip: scale state of the one-plane backward.  Every gradient tensor that feeds a dgrad / wgrad GEMM pair has a slot:
//   words [kDyAmaxStride * j], j < kDyAmaxSlots: max |value| of this step's tensor as float bits (atomicMax by the producer's waves; non-negative floats
//   order like their bit patterns), word 1: mul = 2^e the producer multiplies by, word 2: inv = 2^-e the consumers multiply by, word 3: max |value| of
//   the previous step (float).  Header words: 0 = max |dlogits| of the previous step, 1 = of this step, 2 = overflow flag (some |value| * mul > 65504).
//   begin: e from the previous step's maximum, rescaled by this step's max |dlogits| over the previous one, such that the predicted maximum lands in
//   [2^7, 2^8) - 2^8 of headroom to fp16's largest number, 2^21 below it before the first subnormal; end: folds the maxima, raises the flag.
constexpr int kDyHdrWords = 64, kDySlotWords = 256, kDyAmaxStride = 32, kDyAmaxSlots = 8;
inline int64_t dy16_state_bytes(int nslots) { return 4ll * (kDyHdrWords + (int64_t)nslots * kDySlotWords); }
int launch_dy16_begin(uint32_t* state, int nslots, const float* dlogits, int n_dlogits, hipStream_t st);   // dlogits == nullptr: no rescaling
int launch_dy16_set_mirror(uint32_t* state, void* host_pinned, hipStream_t st);   // pinned int32[2] {overflow flag, generation} written by k_dy16_end (nullptr: none)
int launch_dy16_end(uint32_t* state, int nslots, int check_overflow, hipStream_t st);
int launch_absmax_bf16(const void* hi, int64_t n, uint32_t* amax, hipStream_t st);      // calibration: max |hi part| of a bf16 (hi, lo) pair, n % 8 == 0
int launch_q8_to_bf16int(const void* q8, const float* qp, int center, void* plane, int64_t n, hipStream_t st);
int launch_f16int_to_bf16int(void* plane, int64_t n, hipStream_t st);                  // fallback: grid integers stored as fp16 -> bf16, in place, n % 8 == 0

// ---- attn.hip
int attn_padded_tokens(int T);
// O16_hi / O16_lo / o16_scale (optional, all or none): fp16 (hi, lo) pair of O / *o16_scale, the operand of the attn.proj FORWARD GEMM
int launch_attn_fwd(const float* qkv, const float* qp, int qmin, int qmax, int B, int T, int H, int D, void* O_hi, void* O_lo, float* lse,
                    hipStream_t st, void* O16_hi = nullptr, void* O16_lo = nullptr, float* o16_scale = nullptr, void* codes = nullptr,
                    void* cmask = nullptr);   // codes / cmask (optional): uint8 clamp(q) - qmin [B*T, 3D] and the STE mask bits [B*T, 3D/8], for the backward
int launch_attn_bwd(const float* qkv, const float* qp, int qmin, int qmax, int B, int T, int H, int D, const void* O_hi, const void* O_lo,
                    const float* lse, float* delta, const float* dO, void* dqkv_hi, void* dqkv_lo, const float* col_scale, hipStream_t st,
                    const void* codes = nullptr, const void* cmask = nullptr,   // with the forward's codes the pre-FQ qkv is not read at all
                    const float* o16_mul = nullptr, uint32_t* o16_amax = nullptr,   // the one-plane form: dqkv_hi = ONE fp16 plane (fused kernel only)
                    // dO is zero outside the first live_q_tiles 16-query tiles of every image (0: anywhere): the fused kernel sweeps those alone and stores
                    // zeros as the dQ of the rest.  dO_cls (fused kernel only, with live_q_tiles >= 1): dO is [B, D], the rows of token 0
                    int live_q_tiles = 0, bool dO_cls = false,
                    // which kernels run the fused kernel's ordinary full sweep: kAttnBwdAuto by shape and QATVIT_ATTN_BWD_PIPE; a named form that has no
                    // kernel for the shape is an error
                    int form = -1);
enum AttnBwdForm : int {
    kAttnBwdAuto = -1,
    kAttnBwdPerHead = 0,   // one workgroup per (image, head): what QATVIT_ATTN_BWD_PIPE=0 launches, at every shape
    kAttnBwdPipe = 1,      // k_attn_bwd_pipe: min(B * H, CU count) persistent workgroups, the next head's loads under the sweep
    kAttnBwdPipe5 = 2,     // the same on 5 workgroups (tests: several heads per workgroup at small B * H)
};
// true where launch_attn_bwd takes the fused kernel (the only one with the one-plane output)
bool attn_bwd_is_fused(int T, int H, int D, bool codes);

// ---- teacher.hip: the float forward pieces (bf16 (hi, lo) pairs; the float student step shares them)
// lse (optional): log-sum-exp of the scaled scores per query, [B][H][T]
int launch_attn_fwd_float(const float* qkv, int B, int T, int H, int D, void* O_hi, void* O_lo, hipStream_t st, int f16 = 0, float* lse = nullptr);
// f16 != 0: fp16 bit patterns instead of bf16.  lo == nullptr: the one-plane form keeps the hi part only (fp16 or bf16); the same for
// launch_resid_ln_split_save and launch_attn_fwd_float
int launch_patches_split(const float* img, void* hi, void* lo, int B, int C, int H, int W, int P, hipStream_t st, int f16 = 0);
// mode 0: x = [cls; Y] + pos, mode 1: x = x_prev + Y; then LayerNorm(x) as a (hi, lo) pair, mean / rstd per row (optional); stats (optional):
// kStatSlots {min, max} accumulator pairs that take the min / max of the fp32 LayerNorm outputs (the observe-only forward)
int launch_resid_ln_split_save(int mode, const float* x_prev, const float* Y, const float* cls, const float* pos, float* x_new, const float* gamma,
                               const float* beta, float eps, void* h_hi, void* h_lo, float* mean, float* rstd, int64_t M, int D, int T, hipStream_t st,
                               uint32_t* stats = nullptr, int f16 = 0,
                               const float* drop_scale_rows = nullptr,   // mode 1, optional: x = x_prev + Y * drop_scale_rows[row / T] (drop-path; [M / T] floats)
                               const float* ls_gamma = nullptr);   // mode 1, optional: LayerScale - x = x_prev + (Y * ls_gamma[column]) * multiplier, nothing rounded to a 16-bit type
int launch_gelu_split(const float* Y, void* hi, void* lo, int64_t n, hipStream_t st);   // n % 4 == 0
// ---- ls_scales.hip: the fp16 float form under LayerScale - scales[2 k] = K, [2 k + 1] = 1 / K of branch k, a power of two of the order of 1 / max |gamma_k|
// in [1, 2^24] (gammas: HOST array of device pointers, at most 24); then the patch rows of dx as the fp16 plane dY0 * Ke, Ke = the smallest branch scale,
// with {Ke, 1 / Ke} left at scales[2 * branches], [2 * branches + 1]
int launch_fs_ls_scales(const float* const* gammas, int branches, int D, float* scales, hipStream_t st);
int launch_fs_ls_dy0(const float* dx, void* dY0_f16, int B, int T, int D, float* scales, int branches, hipStream_t st);
// ---- float_amp.hip: the fp16 (autocast) form of the float student step, and (bf16 = true) its bf16 form: the same pieces on bf16 planes and
// v_mfma_f32_16x16x32_bf16 (the host driver of both is float_step.hip's).  Fused attention backward on v_mfma_f32_16x16x32_f16, one workgroup per
// (image, head): qkv / dO fp32 [B*T, 3D] / [B*T, D] (rounded to fp16 on load), O16 fp16 [B*T, D], lse [B][H][T] -> dqkv16 fp16 [B*T, 3D]
int launch_attn_bwd_f16(const float* qkv, const void* O16, const float* lse, const float* dO, int B, int T, int H, int D, void* dqkv16, hipStream_t st,
                        bool bf16 = false);
// the n weights as fp16, as stored [N, K] and transposed, in one launch (blk0[wi]: first workgroup of weight wi, 32 x 32 tiles; blk0[n]: the total)
int launch_fa_wcast(int n, const float* const* W, void* const* w16, void* const* w16T, const int* N, const int* K, const int* blk0, hipStream_t st,
                    bool bf16 = false);
// head: hn = fp16(LN(cls rows)) kept as fp32 values, fp16 logits [B, C]; backward from fp16 dlogits (fixed summation order)
int launch_fa_head_fwd(const float* x, const float* mean, const float* rstd, const float* gamma, const float* beta, const float* W, const float* bias, float* hn,
                       void* logits16, int B, int D, int T, int C, hipStream_t st, bool bf16 = false);
int launch_fa_head_bwd(const void* dl16, const float* hn, const float* W, float* dW, float* dbias, float* dhn, int B, int D, int C, hipStream_t st,
                       bool bf16 = false);
int launch_fa_gelu(const float* Y, void* G16, int64_t n, hipStream_t st, bool bf16 = false);                        // G16 = fp16(gelu(Y)), n % 4 == 0
int launch_fa_gelu_bwd(const float* dG, const float* Y, void* dY16, int64_t n, hipStream_t st, bool bf16 = false);   // dY16 = fp16(fp16(dG) gelu'(Y)), n % 4 == 0
// dpos / dcls from dx [B*T, D] (fixed order), dY0_16 = fp16 of dx's patch rows
int launch_fa_embed_bwd(const float* dx, float* dpos, float* dcls, void* dY0_16, int B, int T, int D, hipStream_t st, bool bf16 = false);
// the overflow rule of the fp16 Linear / Conv2d gradients on count <= 100 fp32 tensors g[k] of n[k] elements: g -> fp16(g) where that is +-inf
int launch_fa_inf_rule(float* const* g, const int64_t* n, int count, hipStream_t st);
// image.hip: the input pipeline.  coeffs = int32 {xmin[D], ntaps[D], coef[D][kImgTaps]} and table = fp32 [3][256], both as the two host functions write them
constexpr int kImgTaps = 4, kImgBits = 22, kImgBand = 16, kImgMaxD = 384;
constexpr int kImgMixMaxLds = 64 * 1024;
// the blur forms: the integer box radius a record may hold, the halo rows its three column passes need on each side of a band, the band without and with mix records
constexpr int kImgBlurMaxRadius = 1, kImgBlurHalo = 3 * (kImgBlurMaxRadius + 1), kImgBlurBand = 16, kImgBlurMixBand = 8;
int image_resize_coeffs(int src, int dst, int32_t* xmin, int32_t* ntaps, int32_t* coef);   // host only; nonzero + set_error when the kernel's bounds do not hold
void image_table(const float* mean, const float* stdv, float* table);                      // host only
int image_resize_coeffs_windows(int S, int D, int32_t* out);                               // host only: int32 [S][6 * D], table n - 1 = image_resize_coeffs(n, D)
// One batch request: out fp32 [B, 3, D, D] from data uint8 [N, S, S, 3] through index int64 [B] (nullptr: image b).  The records are device arrays with one
// entry per batch position (include/qatvit.h states every word); a null pointer means "no such records", and the records present alone decide the kernel
// (kImageForms, image.hip).  sums != nullptr with colour records: zeroed, then filled by a statistics launch in front of the batch launch, all on st.
struct ImageBatch {
    const uint8_t* data = nullptr;
    const int64_t* index = nullptr;
    int B = 0, N = 0, S = 0, D = 0;
    const int32_t* tab = nullptr;     // coeffs; with rrc, windows (image_resize_coeffs_windows)
    const float* table = nullptr;
    const int32_t* aug = nullptr;     // [B]: oy | ox << 8 | flip << 16, a crop offset and a flip of the padded source.  Absent: none (with erase / color: the zero word)
    int padding_mode = 0, fill = 0;   // of aug: 0 = constant (fill), 1 = reflect
    const int32_t* rrc = nullptr;     // [B][2]: top | left << 16, h | w << 15 | flip << 30, the source window.  Present: the window family, which has no aug
    const int32_t* mix = nullptr;     // [B][6]: a partner position, two blend weights and a box.  Present: two plane sets in LDS, refused above kImgMixMaxLds
    const int32_t* erase = nullptr;   // [B][8]: rows, columns, three fills, mode, a 64-bit noise key, on the sample and on its partner before they are mixed.
                                      // Absent with color: all-zero records
    const int32_t* color = nullptr;   // [B][4]: jitter ops in order, grayscale, solarize, three factors, on the uint8 pixels in front of the value table
    uint32_t* sums = nullptr;         // [B], read with color only: the luma sums of the contrast op.  Absent: contrast is the identity, no statistics launch
    const int32_t* blur = nullptr;    // [B][4]: bit 0 on and the integer box radius in bits 8..15, ww, fw, 0: Pillow's GaussianBlur between grayscale / solarize
                                      // and the jitter ops.  Present: the blur forms (image_blur.h), which take every other record as it comes; color absent:
                                      // all-zero records
    float* out = nullptr;
};
int64_t image_lds_bytes(int S, int D, bool mixed, bool rrc);
// image_blur.hip: the blur forms' request, always checked against kImgMixMaxLds, and their launcher, which launch_image_batch calls where r.blur is present
int64_t image_blur_lds_bytes(int S, int D, bool mixed, bool rrc);
int launch_image_blur(const ImageBatch& r, hipStream_t st);
// nonzero + set_error: 1 before any HIP call where the form's LDS request exceeds kImgMixMaxLds (the window forms, and the others with mix), 2 where zeroing sums fails
int launch_image_batch(const ImageBatch& r, hipStream_t st);
// image_window.hip: the window stage in front of the batch launch, for sources larger than the output.  A side n -> D has up to kWinTaps taps
// (n <= 4 D: support <= 8); tables = int32 [sides][D * (2 + kWinTaps)], table n - 1 = {xmin[D], ntaps[D], coef[D][kWinTaps]} of n -> D
constexpr int kWinTaps = 17, kWinBand = 8, kWinMaxScale = 4, kWinStageBytes = 16 * 1024;
int64_t image_window_coeffs_words(int max_side, int D);
int image_window_coeffs(int max_side, int D, int32_t* out);   // host only; nonzero + set_error when the kernel's bounds do not hold
int image_window_max_rows(int n, int D);
int64_t image_window_lds_bytes(int H, int W, int D);
// out uint8 [B, D, D, 3] from the windows rrc [B][2] of data uint8 [N, H, W, 3] through index int64 [B] (nullptr: image b)
struct ImageWindow {
    const uint8_t* data = nullptr;
    const int64_t* index = nullptr;
    int B = 0, N = 0, H = 0, W = 0, D = 0;
    const int32_t* tables = nullptr;
    const int32_t* rrc = nullptr;
    uint8_t* out = nullptr;
};
// nonzero + set_error: 1 before any HIP call where the LDS request exceeds kImgMixMaxLds
int launch_image_window(const ImageWindow& r, hipStream_t st);
// image_bytes_blur.hip: the blur forms' chain on bytes that are the resized image already (the window stage's output, at batch positions): out fp32
// [B, 3, D, D] from bytes uint8 [B, D, D, 3].  The records are ImageBatch's; blur is required.  LDS: the value table and (sides + 1) image buffers
struct ImageBytesBlur {
    const uint8_t* bytes = nullptr;
    int B = 0, D = 0;
    const float* table = nullptr;
    const int32_t* mix = nullptr;
    const int32_t* erase = nullptr;
    const int32_t* color = nullptr;
    uint32_t* sums = nullptr;
    const int32_t* blur = nullptr;
    float* out = nullptr;
};
int image_bytes_blur_band(int D, bool mixed);          // 16 rows without mix records where two buffers of 28 rows fit, else 8
int64_t image_bytes_blur_lds_bytes(int D, bool mixed);
// nonzero + set_error: 1 before any HIP call where the LDS request exceeds kImgMixMaxLds (mix records above D = 344), 2 where zeroing sums fails
int launch_image_bytes_blur(const ImageBytesBlur& r, hipStream_t st);
// eval.hip: validation counts.  The state block of an evaluation: kEvalCounters int64 counters, then the double sum of the finite row losses
// (include/qatvit.h documents the same ten 8-byte words for the C caller).  Every launch ADDS to it: integer counts are exact and independent of
// launch and block order; loss_sum is a sum of doubles in arrival order, so its last bits can differ from run to run.
struct EvalState {
    int64_t total;            // rows seen
    int64_t correct;          // label in [0, C) and argmax == label
    int64_t bad_labels;       // label outside [0, C): no part in correct / loss / confusion / other_correct
    int64_t nonfinite_rows;   // valid label, but the row's cross-entropy is NaN or +-inf: not added to loss_sum
    int64_t other_rows_seen;  // rows whose second-opinion row was read
    int64_t agree;            // of those: argmax == argmax of the second opinion
    int64_t other_correct;    // of those: label in [0, C) and the second opinion's argmax == label
    int64_t bad_index;        // other_index outside [0, other_rows): nothing read through it
    int64_t loss_rows;        // rows added to loss_sum
    double loss_sum;
};
constexpr int kEvalCounters = 9;
static_assert(sizeof(EvalState) == 8 * (kEvalCounters + 1), "EvalState is ten 8-byte words");
// dtype: 0 fp32, 1 fp16, 2 bf16 (anything else returns 1 without a launch); other / other_index / confusion may be null
int launch_eval_accumulate(const void* logits, int dtype, int64_t ld, const int64_t* labels, int64_t batch, int64_t classes, const float* other,
                           int64_t other_ld, const int64_t* other_index, int64_t other_rows, EvalState* state, int64_t* confusion, hipStream_t st);
// grid of the float step's flat elementwise kernels (float_step.hip, float_amp.hip)
inline int flat_grid_fs(int64_t n) {
    int64_t b = (n + 255) / 256;
    return (int)(b < 1 ? 1 : (b > 4096 ? 4096 : b));
}

}  // namespace qv
