/*
 * qatvit.h - C ABI of libqatvit.so, the MI355X (gfx950) native QAT-ViT student path.
 *
 * This is the drop-in boundary below the reference's Python model API
 * (/root/reference/src/models/model_registry.py:99-124 QATWrapper, :333-426
 * factories).  The reference has no FFI of its own: everything under
 * QATWrapper.forward executes inside torch (torch.ao eager QAT + ATen).  Each
 * entry point below cites the reference call site / third-party op it
 * replaces; INTEGRATION.md shows the ctypes stub a maintainer would add.
 *
 * Conventions
 *  - plain C types only; every pointer is a DEVICE pointer into memory owned by
 *    the caller (torch), unless the name ends in _host.  No ownership moves.
 *  - every call is asynchronous on the given hipStream_t (passed as void*;
 *    NULL = the legacy default stream) and never synchronises the device.
 *  - return 0 on success; nonzero -> qatvit_last_error() describes it
 *    (thread-local string).  No C++ exceptions cross the boundary.
 *  - fake-quant state (min/max/scale/zero_point/observer_on/fake_quant_on) is
 *    read AND written in place: these are the very buffers
 *    torch.ao.quantization.prepare_qat registered, so state_dict()/checkpoints
 *    stay compatible (qat_trainer.py:384-385).
 */
#ifndef QATVIT_H
#define QATVIT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* the library is built with -fvisibility=hidden: only the entry points declared here are exported */
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

#define QATVIT_ABI_VERSION 4

int qatvit_abi_version(void);
const char* qatvit_last_error(void);
/* "gfx950" - the only architecture this library is compiled for. */
const char* qatvit_target_arch(void);

/* ---------------------------------------------------------------------------
 * Fused observer + fake-quantize, forward.
 * Replaces: FusedMovingAvgObsFakeQuantize.forward ->
 *   torch.fused_moving_avg_obs_fake_quant (torch/ao/quantization/fake_quantize.py:423-438),
 *   reached from prepare_qat at qat_trainer.py:304-307.
 *
 *  x, y          fp32 [n] (per-tensor) or [channels, inner] row-major (per-channel, ch_axis 0)
 *  mask_bits     optional (may be NULL): 1 bit per element, bit i of byte i/8 = (qmin <= q <= qmax);
 *                ceil(n/8) bytes.  This is the STE mask of the cachemask kernels.
 *  running_min/max, scale   fp32 [1] or [channels];  zero_point int32 [1] or [channels]
 *  observer_on, fake_quant_on  int64 [1] device buffers (read on device, no host sync)
 *  workspace     >= qatvit_fq_workspace_bytes(channels) bytes of scratch
 *  channels      1 for per-tensor; inner = n for per-tensor
 * Element type of the arithmetic: fp32 multiply + round-half-even, integer clamp.
 */
int64_t qatvit_fq_workspace_bytes(int64_t channels);
int qatvit_fq_forward(const float* x, float* y, uint8_t* mask_bits,
                      float* running_min, float* running_max, float* scale, int32_t* zero_point,
                      const int64_t* observer_on, const int64_t* fake_quant_on,
                      float averaging_const, int32_t qmin, int32_t qmax,
                      int64_t channels, int64_t inner, int32_t per_channel, int32_t symmetric,
                      void* workspace, void* stream);

/* STE backward: dx = dy where the mask bit is set, else 0 (autograd of the op above). */
int qatvit_fq_backward(const float* dy, const uint8_t* mask_bits, float* dx, int64_t n, void* stream);

/* ---------------------------------------------------------------------------
 * LayerNorm over the last dim (eps inside the sqrt), fp32.
 * Replaces: nn.LayerNorm(D, eps=1e-6) leaves of the timm ViT (norm1/norm2/norm), ATen native_layer_norm.
 *  mean, rstd: fp32 [rows] saved for backward.
 */
int qatvit_ln_forward(const float* x, const float* gamma, const float* beta, float* y,
                      float* mean, float* rstd, int64_t rows, int64_t dim, float eps, void* stream);
/* dgamma/dbeta are ACCUMULATED into (caller zeroes them); dx is written. */
int qatvit_ln_backward(const float* dy, const float* x, const float* gamma, const float* mean,
                       const float* rstd, float* dx, float* dgamma, float* dbeta,
                       int64_t rows, int64_t dim, void* stream);

/* ---------------------------------------------------------------------------
 * KD + label-smoothed CE loss, forward and d/dlogits in one launch.
 * Replaces: qat_trainer.py:343-349 with the criteria of :265-266.
 *  student [B,C] fp32; teacher [B,C] fp32 or NULL (then loss = CE only, alpha ignored);
 *  labels int64 [B]; out3 = {loss, ce, kd*T^2} fp32 [3]; dlogits [B,C] = dloss/dstudent.
 */
int qatvit_kd_ce_loss(const float* student, const float* teacher, const int64_t* labels,
                      int64_t batch, int64_t classes, float kd_temp, float kd_alpha,
                      float label_smoothing, float* out3, float* dlogits, void* stream);

/* The same loss, statement for statement, with the teacher row of sample b read from a table of
 * per-sample teacher logits: teacher[b] = table[index[b]].
 *  table [table_rows, C] fp32; index int64 [B].  An index outside [0, table_rows) reads nothing:
 *  out3 and that row of dlogits become NaN (no fault, no host synchronisation).
 */
int qatvit_kd_ce_loss_table(const float* student, const float* table, int64_t table_rows,
                            const int64_t* index, const int64_t* labels, int64_t batch,
                            int64_t classes, float kd_temp, float kd_alpha, float label_smoothing,
                            float* out3, float* dlogits, void* stream);

/* Both losses with the mixed targets of mixup / cutmix: mix int32 [B][6], the record of qatvit_image_batch_mix (below), of which the loss
 * reads word 0 (partner p; outside [0, B) means p = b) and word 5 (lam, fp32 bits).  teacher [B,C] and table [table_rows,C] are mutually
 * exclusive (both given: an argument error); both NULL: CE only; a table needs index.  Per row b, with oml = 1 - lam formed in fp32:
 *   hard target      t[c] = lam * [c == labels[b]] + oml * [c == labels[p]],  smoothed (1 - eps) * t[c] + eps / C;
 *   teacher tensor:  the KD part is qatvit_kd_ce_loss's (the teacher saw the mixed images);
 *   teacher table:   q = lam * softmax(table[index[b]] / T) + oml * softmax(table[index[p]] / T), KD = sum_c q (log q - log_softmax(s / T))
 *                    with 0 log 0 = 0, gradient term alpha * T * (softmax(s / T) - q) / B.  This is the usual mixed soft label, NOT the
 *                    teacher's output on the mixed image.
 * The partner's label weight and table row take part only where lam != 1: a row with lam == 1 gives the bits of the two entries above, and
 * an index[p] outside the table makes NaN only where lam != 1; index[b] outside the table makes NaN as in qatvit_kd_ce_loss_table.
 * mix == NULL: qatvit_kd_ce_loss_table (table given) or qatvit_kd_ce_loss.  mix 4-byte aligned.  One single-block launch.
 */
int qatvit_kd_ce_loss_mix(const float* student, const float* teacher, const float* table, int64_t table_rows, const int64_t* index,
                          const int64_t* labels, const int32_t* mix, int64_t batch, int64_t classes, float kd_temp, float kd_alpha,
                          float label_smoothing, float* out3, float* dlogits, void* stream);

/* KD + BINARY cross-entropy with logits on the same targets (timm's BinaryCrossEntropy on the output of its Mixup; the DeiT-III criterion), forward
 * and d/dlogits.  One entry for every form: teacher / table / index / mix are optional under qatvit_kd_ce_loss_mix's rules (tensor and table
 * mutually exclusive, a table needs index and table_rows >= 1, both NULL: the hard part only and alpha ignored; mix 4-byte aligned).
 * 1 <= B < 2^30, 2 <= C <= 4096, kd_temp > 0, label_smoothing eps in [0, 1).  partials: fp32 [2 * B] workspace, contents on entry ignored.
 * Per row b, with p and lam from words 0 and 5 of the row's record (p outside [0, B): p = b; mix == NULL or lam == 1: p = b, lam = 1),
 * oml = 1 - lam formed in fp32, x = student[b][c], all in fp32, every operation rounded on its own:
 *   target     t[c] = (1 - eps) * (lam * [c == labels[b]] + oml * [c == labels[p]]) + eps / C
 *              then, if target_threshold >= 0:  t[c] = t[c] > target_threshold ? 1 : 0   (after smoothing and mixing; negative: off)
 *   hard part  l[c] = max(x, 0) - x * t[c] + log1pf(e),  e = expf(-|x|);   sigma = x >= 0 ? 1 / (1 + e) : e / (1 + e)
 *              gradient term  w_hard * (sigma - t[c]) * scale,  scale = 1 / (B * C), or 1 / B where sum_classes != 0
 *   KD part    qatvit_kd_ce_loss_mix's, term for term: teacher tensor q = softmax(teacher[b] / T); teacher table
 *              q = softmax(table[index[b]] / T), and where lam != 1  q = lam * q + oml * softmax(table[index[p]] / T);
 *              KD = sum_c q (log q - log_softmax(x / T)) with 0 log 0 = 0, gradient term w_kd * T * (softmax(x / T) - q) / B.
 *              w_kd = alpha, w_hard = 1 - alpha with a teacher of either kind, else 0 and 1.
 *   An index[b], or where lam != 1 an index[p], outside [0, table_rows) reads nothing: that row of dlogits and all of out3 become NaN
 *   (no fault, no host synchronisation).  The partner's label and row are read only where lam != 1.
 * Two launches on `stream`: one wave of 64 lanes per row (4 rows per workgroup) writes dlogits[b] and the row's {sum_c l[c], KD} to
 * partials[2 * b]; one workgroup then adds the partials up in double in a fixed order and writes
 *   out3 = {w_kd * kd + w_hard * bce, bce, kd},  bce = scale * sum_b sum_c l,  kd = T^2 / B * sum_b KD.
 * No atomics: the same inputs give the same bits.  The lanes of a row add in parallel, so the KD number agrees with the CE entries' to
 * rounding, not bit for bit.
 */
int qatvit_kd_bce_loss(const float* student, const float* teacher, const float* table, int64_t table_rows, const int64_t* index,
                       const int64_t* labels, const int32_t* mix, int64_t batch, int64_t classes, float kd_temp, float kd_alpha,
                       float label_smoothing, float target_threshold, int32_t sum_classes, float* partials, float* out3, float* dlogits,
                       void* stream);

/* ===========================================================================
 * Building blocks of the step, exported for kernel-level parity tests.
 * All matrices row-major; "bf16" = IEEE bfloat16 bit patterns (uint16).
 */

/* Operand convention of the GEMMs: every operand is a row-major bf16 matrix.  A tensor that sits on a
 * fake-quant grid is passed as the integers (q - zero_point) (exact in bf16, `_lo` = NULL); a float tensor
 * is passed as the pair hi = bf16(x), lo = bf16(x - hi) written by its producer kernel (2^-17 relative).
 *
 * C[M,N] = ((A_hi + A_lo)[M,K] . B[N,K]^T) * (*s1) * (*s2) * col_scale[n] + bias[n]   (fp32 out)
 * Replaces: F.linear inside nnqat.Linear.forward (torch/ao/nn/qat/modules/linear.py:49-50) and its dgrad.
 *  s1, s2, col_scale, bias, stats may be NULL.  stats: 2 x uint32 order-preserving {min,max} accumulator
 *  of the stored values (initialise to {0xFF800000, 0x007FFFFF}).  Shapes: N % 128 == 0, K % 64 == 0. */
int qatvit_gemm_nt(const void* A_hi, const void* A_lo, const void* B, float* C, int32_t M, int32_t N, int32_t K,
                   int32_t lda, int32_t ldb, int32_t ldc, const float* s1, const float* s2, const float* col_scale,
                   const float* bias, uint32_t* stats, void* stream);

/* The same product with fp16 bit patterns in all three matrices: A = (A16_hi + A16_lo), an fp16 (hi, lo) pair of a float tensor pre-scaled
 * by a power of two that the caller folds into *s1 (22 significant bits, 2^-23 relative, against 2^-17 for a bf16 pair); B16 = the weight
 * integers as fp16 (exact).  v_mfma_f32_16x16x32_f16, fp32 accumulate.  Used for the two forward GEMMs with a float operand (attn.proj, mlp.fc2),
 * whose outputs are fake-quantized next.  N % 384 == 0, K % 64 == 0. */
int qatvit_gemm_nt_f16(const void* A16_hi, const void* A16_lo, const void* B16, float* C, int32_t M, int32_t N, int32_t K, int32_t lda, int32_t ldb,
                       int32_t ldc, const float* s1, const float* s2, const float* col_scale, const float* bias, uint32_t* stats, void* stream);

/* The statistics-only first pass of a two-pass GEMM (qkv, fc1) on the general 208 x 384 tile: the product of qatvit_gemm_nt_i8 is formed for its
 * minimum / maximum only, which go into stats[0] / stats[1] as order-preserving uint32 (atomicMin / atomicMax on the caller-initialised pair
 * {0xff800000, 0x007fffff}).  N % 384 == 0, K % 64 == 0. */
int qatvit_gemm_nt_i8_minmax(const void* A8, const void* B8, const int32_t* wsum, const float* a_qp, int32_t center, int32_t M, int32_t N, int32_t K,
                             int32_t lda, int32_t ldb, const float* s1, const float* s2, const float* col_scale, const float* bias, uint32_t* stats,
                             void* stream);

/* int8 weight [N,K] row-major -> MFMA fragment order, the B operand of qatvit_i8_strip: 16-byte units indexed
 * [n / 48][k / 64][(n % 48) / 16][lane = 16 * ((k % 64) / 16) + n % 16], byte k % 16 inside the unit, so that one wave reads each of its
 * 16 x 64 weight fragments as 1 KiB of contiguous memory straight into registers.  N % 48 == 0, K % 64 == 0. */
int qatvit_w8_fragment_order(const void* B8, void* B8f, int32_t N, int32_t K, void* stream);

/* The K = 384 / 768 two-pass forward GEMMs of a block (attn.qkv, mlp.fc1 of ViT-S / ViT-B: nnqat.Linear.forward, torch/ao/nn/qat/modules/linear.py:49-50, + the
 * activation_post_process hook, torch/ao/quantization/quantize.py:150-152) on int8 MFMA, A-stationary: one workgroup keeps a 208- (K = 768: 112-) row strip of A8
 * in LDS for all column tiles, each wave reads its weight fragments from B8f (qatvit_w8_fragment_order) into registers, the k-loop has no barrier.
 * v[m,n] = (sum_k A8*B8 + (center - zero_point) * wsum[n]) * (*s1) * (*s2) * col_scale[n] + bias[n]  - the value qatvit_gemm_nt_i8 stores, bit for bit.
 *   mode 3: min / max of v into stats (as qatvit_gemm_nt_i8_minmax); nothing is stored.
 *   mode 7: out_qp = {scale, 1/scale, zero_point, enabled} of the OUTPUT's quantizer: out8 = clamp(rint(v / scale) + zero_point) - qmin as uint8 in the
 *           attention layout [b][head][q|k|v][t][64] (N = 3 * embed_dim, embed_dim % 384 == 0, code_T tokens per image) and out8_mask = the STE
 *           mask (qmin <= q <= qmax), one bit per element in the same order.
 *   mode 4: out8 = the same code row-major [M,N], out8_mask [M,N/8]; lut_out / lutq_out [256] = packed fp16 / bf16 (hi | lo << 16) pairs of
 *           2^k * gelu(grid value) / gelu(grid value), *out16_scale = 2^-k (the tables qatvit_gemm_nt_codes / qatvit_gemm_tn_codes expand the codes through).
 * K = 384: N % 1152 == 0 or N % 1536 == 0; K = 768: N = 2304 or 3072; lda % 16 == 0; M < 2^22. */
int qatvit_i8_strip(int32_t mode, const void* A8, const void* B8f, const int32_t* wsum, const float* a_qp, int32_t center, int32_t M, int32_t N, int32_t K,
                    int32_t lda, const float* s1, const float* s2, const float* col_scale, const float* bias, uint32_t* stats, const float* out_qp,
                    int32_t qmin, int32_t qmax, void* out8, void* out8_mask, int32_t code_T, uint32_t* lut_out, uint32_t* lutq_out,
                    float* out16_scale, void* stream);

/* The LayerNorm apply + fake-quant of norm1 / norm2 as the launch of its own the training forward runs where qatvit_i8_strip_ln does not apply (byte plane only):
 * out8[m,d] = clamp(rint(y / scale) + zero_point, qmin, qmax) - center as int8, y = ((x[m,d] - mean[m]) * rstd[m]) * gamma[d] + beta[d], qp = {scale, 1/scale,
 * zero_point, enabled}.  x, out8 [M,D] dense; D % 4 == 0. */
int qatvit_ln_apply_quant8(const float* x, const float* mean, const float* rstd, const float* gamma, const float* beta, const float* qp, int32_t qmin, int32_t qmax,
                           void* out8, int32_t center, int64_t M, int32_t D, void* stream);

/* The statistics pass (mode 3) of qatvit_i8_strip with the LayerNorm in front of it (nn.LayerNorm + the activation_post_process fake-quant of norm1 / norm2) in its
 * prologue: every workgroup quantises its own rows - out8[m,k] = clamp(rint(y / scale) + zero_point) - center with y = ((x[m,k] - mean[m]) * rstd[m]) * gamma[k] + beta[k],
 * a_qp = {scale, 1/scale, zero_point, enabled} of that quantizer - keeps them in LDS as its A strip and stores them to out8 [M,lda] (int8), the A8 of the code pass.
 * *s1 of qatvit_i8_strip is a_qp[0].  The plane and the statistics are bit-identical to the LayerNorm-apply kernel followed by qatvit_i8_strip(mode 3).
 * x [M,K] fp32, K = 384: N = 1152 or 1536; K = 768: N = 2304 or 3072; lda % 16 == 0, lda >= K; M < 2^22. */
int qatvit_i8_strip_ln(const float* x, const float* mean, const float* rstd, const float* gamma, const float* beta, int32_t ln_qmin, int32_t ln_qmax, void* out8,
                       const void* B8f, const int32_t* wsum, const float* a_qp, int32_t center, int32_t M, int32_t N, int32_t K, int32_t lda, const float* s2,
                       const float* col_scale, const float* bias, uint32_t* stats, void* stream);

/* qatvit_gemm_nt_f16 for an A operand that takes at most 256 distinct values (mlp.fc2: A = gelu(fq(fc1 output))): A8 uint8 [M,lda] = table
 * index per element (lda in bytes), lut[256] = the fp16 (hi | lo << 16) pair per index.  The kernel expands the codes through the table on their
 * way into LDS: bit-identical to qatvit_gemm_nt_f16 on the expanded planes, 1 B instead of 4 B of HBM traffic per A element.
 * N % 384 == 0, K % 64 == 0, lda % 16 == 0. */
int qatvit_gemm_nt_codes(const void* A8, const uint32_t* lut, const void* B16, float* C, int32_t M, int32_t N, int32_t K, int32_t lda, int32_t ldb,
                         int32_t ldc, const float* s1, const float* s2, const float* col_scale, const float* bias, uint32_t* stats, void* stream);

/* The residual epilogue of the inference forward (attn.proj, mlp.fc2 of qatvit_infer_forward / qatvit_infer_forward_ls) on one GEMM of its own: with
 *   v[m,n] = the value qatvit_gemm_nt_f16 (form 1) / qatvit_gemm_nt_codes (form 3) stores for the same operands, bit for bit, and
 *   fq(v)  = (clamp(rint(v * out_qp[1]) + out_qp[2], qmin, qmax) - out_qp[2]) * out_qp[0],  out_qp = {scale, 1/scale, zero_point, enabled} (device),
 *   ls_gamma == NULL:  C[m,n] = resid[m,n] + fq(v[m,n])
 *   ls_gamma fp32 [N]: C[m,n] = resid[m,n] + fl(fq(v[m,n]) * ls_gamma[n])        (LayerScale)
 * where fl() rounds the product to fp32 before the sum is formed and rounded: two roundings, never a fused multiply-add - what the training forward's
 * residual kernel computes - so a gamma of exactly 1 gives the bits of the NULL form.  resid and C are fp32 [M,ldc] (one leading dimension), rows >= M are not
 * touched.
 *  form 1: A = the hi plane and A_lo_or_lut = the lo plane of an fp16 pair (lda in elements);  form 3: A = uint8 codes (lda in bytes), A_lo_or_lut = their
 *  256-entry table of fp16 (hi | lo << 16) pairs.  Every other form is refused.  N % 384 == 0, K % 64 == 0, ldc % 4 == 0 (form 3: lda % 16 == 0). */
int qatvit_gemm_nt_resid_fq(int32_t form, const void* A, const void* A_lo_or_lut, const void* B16, const float* resid, float* C, int32_t M, int32_t N,
                            int32_t K, int32_t lda, int32_t ldb, int32_t ldc, const float* s1, const float* s2, const float* col_scale, const float* bias,
                            const float* out_qp, int32_t qmin, int32_t qmax, const float* ls_gamma, void* stream);

/* The same product for two operands that both sit on a quantisation grid (qkv / fc1 / patch-embed forward), on int8 MFMA:
 *   A8 int8 [M,lda] = q - center (center = (qmin+qmax+1)/2 of the activation range), B8 int8 [N,ldb] = weight integers,
 *   wsum int32 [N] = row sums of B8, a_qp = {scale, 1/scale, zero_point, enabled} of A's quantizer (device):
 *   C = (sum_k A8*B8 + (center - zero_point) * wsum[n]) * (*s1) * (*s2) * col_scale[n] + bias[n].
 * Bit-identical to qatvit_gemm_nt on the bf16 integers (both accumulate the same integers exactly).  N % 384 == 0, K % 64 == 0. */
int qatvit_gemm_nt_i8(const void* A8, const void* B8, const int32_t* wsum, const float* a_qp, int32_t center, float* C, int32_t M,
                      int32_t N, int32_t K, int32_t lda, int32_t ldb, int32_t ldc, const float* s1, const float* s2,
                      const float* col_scale, const float* bias, uint32_t* stats, void* stream);

/* C[N,Kw] += sum_m (P_hi + P_lo)[m,N] * (Q_hi + Q_lo)[m,Kw] * (*s1) / row_div[n], masked by the weight fake-quant STE
 * mask of W; dbias[N] += sum_m P[m,N] / row_div[n].
 * Replaces: the weight/bias gradient of nnqat.Linear / nnqat.Conv2d (autograd of linear.py:49-50, conv.py:54-55,
 * followed by the weight_fake_quant backward).  The token reduction is split over up to 256 workgroups.  With
 * scratch = NULL the splits add into C with fp32 atomics (caller zeroes C; bit patterns vary run to run).  With a device
 * scratch buffer of qatvit_gemm_tn_scratch_bytes() the splits store raw partial tiles there and a second launch sums
 * them in a fixed order, applies scale and mask and adds to C: no atomics on C, bit-reproducible.  dbias always uses
 * atomics.  Q_lo, s1, W (fp32 [N,Kw], with w_scale/w_zp [1] or [N]), dbias, row_div may be NULL.  N % 128 == 0, Kw % 128 == 0. */
int64_t qatvit_gemm_tn_scratch_bytes(void);
/* qatvit_gemm_tn for a Q operand that takes at most 256 distinct values (mlp.fc2's weight gradient: Q = gelu(fq(fc1 output))): Qc uint8 [M,ldq] =
 * table index per element (ldq in bytes), lutQ[256] = the bf16 (hi | lo << 16) pair per index.  The kernel expands the codes inside the workgroup:
 * bit-identical to qatvit_gemm_tn on the expanded (Q_hi, Q_lo) planes, 1 B instead of 4 B per Q element.  N % 128 == 0, Kw % 384 == 0, ldq % 16 == 0. */
int qatvit_gemm_tn_codes(const void* P_hi, const void* P_lo, const void* Qc, const uint32_t* lutQ, float* C, int32_t M, int32_t N, int32_t Kw, int32_t ldp,
                         int32_t ldq, int32_t ldc, const float* s1, const float* W, const float* w_scale, const int32_t* w_zp, int32_t w_per_channel,
                         int32_t w_qmin, int32_t w_qmax, float* dbias, const float* row_div, float* scratch, int64_t scratch_bytes, void* stream);
int qatvit_gemm_tn(const void* P_hi, const void* P_lo, const void* Q_hi, const void* Q_lo, float* C, int32_t M, int32_t N,
                   int32_t Kw, int32_t ldp, int32_t ldq, int32_t ldc, const float* s1, const float* W, const float* w_scale,
                   const int32_t* w_zp, int32_t w_per_channel, int32_t w_qmin, int32_t w_qmax, float* dbias,
                   const float* row_div, float* scratch, int64_t scratch_bytes, void* stream);

/* The one-plane forms of the two backward GEMMs (see QATVIT_BWD_DY16 below): the gradient operand is ONE fp16 plane = gradient * 2^e, *s2 = 2^-e.
 * nt: C[M,N] = A16[M,K] . B16[N,K]^T * (*s1) * (*s2), B16 = the transposed weight integers as fp16; N % 384 == 0, K % 32 == 0.  (dgrad of nnqat.Linear)
 * tn: C[N,Kw] += sum_m P16[m,N] * Q[m,Kw] * (*s1) * (*s2) / row_div[n] under the weight STE mask, dbias += sum_m P16 * (*s2) / row_div; Q = fp16 integers
 *     (Q_lo NULL), an fp16 (hi, lo) pair, or - Qc / lutQ16 set, Q_hi / Q_lo NULL - uint8 codes + a table of fp16 (hi | lo << 16) pairs.  Shapes as qatvit_gemm_tn. */
int qatvit_gemm_nt_dy16(const void* A16, const void* B16, float* C, int32_t M, int32_t N, int32_t K, int32_t lda, int32_t ldb, int32_t ldc, const float* s1,
                        const float* s2, void* stream);
int qatvit_gemm_tn_dy16(const void* P16, const void* Q_hi, const void* Q_lo, const void* Qc, const uint32_t* lutQ16, float* C, int32_t M, int32_t N, int32_t Kw,
                        int32_t ldp, int32_t ldq, int32_t ldc, const float* s1, const float* s2, const float* W, const float* w_scale, const int32_t* w_zp,
                        int32_t w_per_channel, int32_t w_qmin, int32_t w_qmax, float* dbias, const float* row_div, float* scratch, int64_t scratch_bytes,
                        void* stream);
/* tn with the grid X operand as ONE byte per element (what the forward's int8 GEMM reads): Q8[m, Kw] = q - center as int8 (ldq in bytes, % 16 == 0),
 * a_qp = that activation's {scale, 1/scale, zero_point, enabled}: X = Q8 + center - zero_point, *s1 of the form above = a_qp[0].  Kw % 384 == 0. */
int qatvit_gemm_tn_q8_dy16(const void* P16, const void* Q8, const float* a_qp, int32_t center, float* C, int32_t M, int32_t N, int32_t Kw, int32_t ldp, int32_t ldq,
                           int32_t ldc, const float* s2, const float* W, const float* w_scale, const int32_t* w_zp, int32_t w_per_channel, int32_t w_qmin,
                           int32_t w_qmax, float* dbias, const float* row_div, float* scratch, int64_t scratch_bytes, void* stream);

/* The weight gradients of a whole backward call as ONE persistent launch per X form ("stream-K" over the 64-token steps of all 128 x 384 output tiles: about one tile per
 * CU in a full backward, so accumulators stay in registers over the whole token range and only the tiles a span boundary cuts go through scratch; a fix-up launch sums
 * those in a fixed order - bit-reproducible).  All items are one-plane weight gradients (qatvit_gemm_tn_dy16's arithmetic) over the same M token rows:
 * mode 0: Q = int8 grid plane q - center, s1 = the activation's {scale, 1/scale, zero_point, enabled};  mode 1: Q = uint8 codes, lut = 256 fp16 (hi | lo << 16) entries
 * (hi used), s1 = X's scale;  mode 2: Q = fp16 plane (ldq in elements), s1 = X's scale.  C[N, ldc] += ... under the weight STE mask (W NULL: none); dbias, row_div optional.
 * n <= 24 items per call, N % 128 == 0, Kw % 384 == 0; scratch >= qatvit_gemm_tn_stream_scratch_bytes(). */
struct qatvit_tn_item {
    const void* P; const void* Q; const uint32_t* lut; const float* s1; const float* s2; float* C; const float* W; const float* w_scale; const int32_t* w_zp; float* dbias;
    const float* row_div; int32_t N, Kw, ldp, ldq, ldc;
};
int64_t qatvit_gemm_tn_stream_scratch_bytes(void);
int qatvit_gemm_tn_stream_dy16(int32_t mode, const struct qatvit_tn_item* items, int32_t n, int32_t M, int32_t center, int32_t w_per_channel, int32_t w_qmin, int32_t w_qmax,
                               float* scratch, int64_t scratch_bytes, void* stream);

/* Attention core between attn.qkv and attn.proj (timm Attention; no fake-quant inside).
 *  qkv: PRE-fake-quant fp32 [B*T, 3*D]; qp: {scale, 1/scale, zero_point, enabled} of the qkv activation FQ
 *  (quantize-on-load).  O = O_hi + O_lo, bf16 [B*T, D] each; lse fp32 [B*H, qatvit_attn_padded_tokens(T)].
 *  backward writes dqkv (hi/lo bf16 [B*T, 3*D]) = d/d(pre-FQ qkv), i.e. including the FQ STE mask, times
 *  col_scale[3*D] if given; delta is scratch like lse; dO is fp32 [B*T, D]. */
int32_t qatvit_attn_padded_tokens(int32_t T);
int qatvit_attn_forward(const float* qkv, const float* qp, int32_t qmin, int32_t qmax, int32_t B, int32_t T, int32_t H,
                        int32_t D, void* O_hi, void* O_lo, float* lse, void* stream);
/* The same forward, additionally writing O as the fp16 (hi, lo) pair the attn.proj FORWARD GEMM reads: O = (O16_hi + O16_lo) * (*o16_scale),
 * o16_scale (device float, written by the kernel) = qkv scale / 64.  Inside the forward the softmax probabilities and V enter the MFMA as
 * fp16 (P scaled by 2^14): 2^-23 per element where a bf16 pair has 2^-17 - the forward feeds fake-quantizers, the backward does not. */
int qatvit_attn_forward_f16(const float* qkv, const float* qp, int32_t qmin, int32_t qmax, int32_t B, int32_t T, int32_t H,
                            int32_t D, void* O_hi, void* O_lo, float* lse, void* O16_hi, void* O16_lo, float* o16_scale, void* qkv_codes,
                            void* qkv_mask, void* stream);
/* qkv_codes / qkv_mask (optional, both or neither): the forward also saves the quantised qkv it computed on load, in per-head slices (every
 * workgroup's accesses are whole contiguous runs): codes[b][h][which][t][d] = clamp(q) - qmin as uint8 (which = 0 q / 1 k / 2 v, d < D / H;
 * B*T*3*D bytes) and the STE mask, bit (d & 7) of byte mask[b][h][which][t][d >> 3] (B*T*3*D/8 bytes).  Given them the backward reads 1.125
 * bytes per element instead of re-quantising the 4-byte pre-fake-quant tensor twice (its `qkv` argument may then be NULL).  Bit-identical results.
 * qkv == NULL in the FORWARD: qkv_codes is its INPUT (written by the qkv GEMM's second pass - the whole-step engine's form, and the inference
 * forward's): the pre-fake-quant tensor is not read and need not exist. */
int qatvit_attn_backward(const float* qkv, const float* qp, int32_t qmin, int32_t qmax, int32_t B, int32_t T, int32_t H,
                         int32_t D, const void* O_hi, const void* O_lo, const float* lse, float* delta, const float* dO,
                         void* dqkv_hi, void* dqkv_lo, const float* col_scale, const void* qkv_codes, const void* qkv_mask, void* stream);
/* The same backward where dO is known to be zero outside the first live_q_tiles 16-query tiles of every image (0: anywhere - qatvit_attn_backward).  The fused
 * kernel (head_dim 64, 33..224 tokens, saved codes) then sweeps only the query pairs that hold them and stores zeros as the dQ of the others; dK and dV are
 * complete either way.  The two-kernel form ignores the count.  dO_cls != 0 (fused kernel only, live_q_tiles >= 1): dO is [B, D] - the rows of token 0, the
 * class token of a cls-pooled model; every other row of dO is zero by definition. */
int qatvit_attn_backward_live(const float* qkv, const float* qp, int32_t qmin, int32_t qmax, int32_t B, int32_t T, int32_t H,
                              int32_t D, const void* O_hi, const void* O_lo, const float* lse, float* delta, const float* dO,
                              void* dqkv_hi, void* dqkv_lo, const float* col_scale, const void* qkv_codes, const void* qkv_mask,
                              int32_t live_q_tiles, int32_t dO_cls, void* stream);
/* The same backward (full sweep) with the launch form named, so that one process can compare the forms (the library itself chooses by shape and
 * QATVIT_ATTN_BWD_PIPE).  form 0: one workgroup per (image, head) - at every shape what qatvit_attn_backward launches under QATVIT_ATTN_BWD_PIPE=0;
 * form 1: the persistent kernel, min(B * H, CU count) workgroups that each walk several heads and fetch the next one under the sweep; form 2: the
 * same on 5 workgroups (tests).  Forms 1 and 2 exist for head_dim 64, 33..224 tokens and saved codes only: an error elsewhere, nothing is launched.
 * Every form writes the same bits.  o16_mul / o16_amax (optional, together; fused shapes only): the one-plane output - dqkv_hi is ONE fp16 plane
 * of value * (*o16_mul), dqkv_lo is not written (may be NULL), max |value| is folded into the QATVIT_DY16_AMAX_SLOTS slots of o16_amax (uint32
 * bit patterns, QATVIT_DY16_AMAX_STRIDE words apart) with atomicMax. */
#define QATVIT_DY16_AMAX_SLOTS 8
#define QATVIT_DY16_AMAX_STRIDE 32
int qatvit_attn_backward_form(const float* qkv, const float* qp, int32_t qmin, int32_t qmax, int32_t B, int32_t T, int32_t H,
                              int32_t D, const void* O_hi, const void* O_lo, const float* lse, float* delta, const float* dO,
                              void* dqkv_hi, void* dqkv_lo, const float* col_scale, const void* qkv_codes, const void* qkv_mask,
                              const float* o16_mul, uint32_t* o16_amax, int32_t form, void* stream);

/* The class-token rows of a [rows * T, width bytes] tensor (the student pools the class token, so the gradient entering the last block lives in rows
 * b * T only; the one-plane backward runs that block's MLP and proj on those rows - QATVIT_CLS_BWD=0 in the environment: on all rows).
 * gather: compact[b] = tall[b * T], b < rows; width % 4 == 0, `stride` = bytes between two rows of tall (% 4 == 0, >= width).
 * scatter: writes ALL of tall [rows * T, width] - row b * T = compact[b], every other row zero; width % 16 == 0, 16-byte aligned pointers.
 * Replaces: nothing in the reference (its autograd runs every row). */
int qatvit_rows_gather(const void* tall, void* compact, int32_t rows, int32_t T, int32_t width, int64_t stride, void* stream);
int qatvit_rows_scatter(const void* compact, void* tall, int32_t rows, int32_t T, int32_t width, void* stream);

/* ===========================================================================
 * The whole student step.
 * Replaces: `student_out = ddp_model(images)` ... `loss.backward()` of
 * /root/reference/src/training/qat_trainer.py:341-359 for a prepare_qat()-ed QATWrapper(vit_*_patch16_224).
 */
typedef struct qatvit_cfg {
    int32_t batch, img_size, patch_size, in_chans;
    int32_t embed_dim, depth, num_heads, mlp_hidden, num_classes;
    int32_t act_qmin, act_qmax;      /* 0,255 (qnnpack) or 0,127 (x86/fbgemm) */
    int32_t w_qmin, w_qmax;          /* -128,127 */
    int32_t w_per_channel;           /* 0: per-tensor symmetric, 1: per-output-channel symmetric */
    float averaging_const;           /* 0.01 */
    float ln_eps;                    /* 1e-6 */
} qatvit_cfg;

/* One fake-quant module's buffers (device pointers into the tensors prepare_qat registered). */
typedef struct qatvit_fq {
    float* min_val;
    float* max_val;
    float* scale;
    int32_t* zero_point;
    const int64_t* observer_on;
    const int64_t* fake_quant_on;
} qatvit_fq;

/* Orders (host arrays):
 *  params / grads: patch_embed.proj.{weight,bias}, cls_token, pos_embed, then per block
 *    norm1.{w,b}, attn.qkv.{w,b}, attn.proj.{w,b}, norm2.{w,b}, mlp.fc1.{w,b}, mlp.fc2.{w,b}, then norm.{w,b}, head.{w,b}
 *  act_fq: quant, patch_embed.proj, per block norm1, attn.qkv, attn.proj, norm2, mlp.fc1, mlp.fc2, then norm, head
 *  weight_fq: patch_embed.proj, per block attn.qkv, attn.proj, mlp.fc1, mlp.fc2, then head */
int32_t qatvit_student_num_params(const qatvit_cfg* cfg);
int32_t qatvit_student_num_act_fq(const qatvit_cfg* cfg);
int32_t qatvit_student_num_weight_fq(const qatvit_cfg* cfg);
int64_t qatvit_student_workspace_bytes(const qatvit_cfg* cfg);
/* once per workspace, before the first forward */
int qatvit_student_init(const qatvit_cfg* cfg, void* workspace, void* stream);
int qatvit_student_forward(const qatvit_cfg* cfg, void* const* params, const qatvit_fq* act_fq, const qatvit_fq* weight_fq,
                           const float* images, float* logits, void* workspace, void* stream);
/* grads: fp32 buffers, ZEROED by the caller, same order as params.  Stages: 0 = head + final norm,
 * 1..depth = blocks depth-1..0, depth+1 = embedding; run them in order (possibly over several calls, so the
 * caller can start the all-reduce of finished buckets in between). */
int qatvit_student_backward(const qatvit_cfg* cfg, void* const* params, const qatvit_fq* act_fq, const qatvit_fq* weight_fq,
                            const float* dlogits, void* const* grads, void* workspace, int32_t stage_from, int32_t stage_to,
                            void* stream);
/* The same two calls over a range of stages, for stage-level (teacher-forced) parity tests and for callers that interleave other work.
 * Forward stages: 0 = weight fake-quant + input fake-quant + patch embedding (leaves the residual stream x_in[0] in the workspace);
 * s = 1..depth = transformer block s-1 (reads x_in[s-1], leaves x_in[s]); depth+1 = final norm, cls pooling, head, logits fake-quant.
 * Backward stages are those of qatvit_student_backward.  A full step is forward [0, depth+1] then backward [0, depth+1].
 * flags & QATVIT_STAGE_INJECT (stage_from >= 1): the tensor ENTERING stage_from was written into the workspace by the caller instead of
 * by the preceding stage - forward: x_in[stage_from-1] (qatvit_student_tensor_offset "x_in"); backward: the residual-stream gradient
 * "dxA" (d loss / d x_in[depth - stage_from + 1]; for stage depth+1 d loss / d x_in[0]).  The library then recomputes what the
 * preceding stage would have left beside that tensor (LayerNorm row statistics and the next observer's min/max; the masked (hi, lo)
 * copy of the gradient) before running the stages.  images may be NULL when stage_from > 0, logits when stage_to <= depth, dlogits when
 * stage_from > 0.  Replaces, per stage, the corresponding slice of `ddp_model(images)` / `loss.backward()` (qat_trainer.py:341,359). */
#define QATVIT_STAGE_INJECT 1
/* The one-plane backward (ABI 4).  The float operand of every backward GEMM of a block - the masked residual gradient entering mlp.fc2 and attn.proj, the
 * gradients of the fc1 and qkv outputs - is written as ONE fp16 plane value * 2^e and consumed in one v_mfma_f32_16x16x32_f16 pass, instead of a bf16
 * (hi, lo) pair (4 B per element, two passes).  e is chosen per tensor before the tensor exists, from the maximum that tensor had in the previous backward
 * rescaled by max |dlogits| now / then; producers record this backward's maxima and raise an overflow flag (workspace word "dy16" + 2) when one did not
 * fit below 65504.  Protocol (qat-vit_amd/engine.py): the first backward on a workspace runs with QATVIT_BWD_CALIBRATE (the pair form, recording maxima);
 * later steps run the forward with QATVIT_FWD_X16 (the quantised LayerNorm outputs, X operand of the qkv / fc1 weight gradients, as fp16 integers) and the
 * backward with QATVIT_BWD_DY16; a raised flag -> qatvit_student_dy16_to_pair + the same backward again with QATVIT_BWD_CALIBRATE into zeroed gradients:
 * the step is then bit-identical to a pair-form step.  Error of the one-plane form against the pair form: 2^-12 per element, relative L2 1-2e-4 per stage
 * (tests/test_gpu_stage_parity.py runs every stage table in both forms).  qatvit_student_backward (no flags) is always the pair form.
 * Stage 0 with QATVIT_BWD_DY16 leaves the gradient entering the last block as [B, embed_dim] rows of the class tokens inside the workspace (the student pools the class
 * token: every other row is zero), not as the full "dxA"; stage 1 of the same or a later call takes it from there and runs its MLP and proj backward on those B rows.
 * A stage 1 with QATVIT_STAGE_INJECT reads the caller's full "dxA" as before.  QATVIT_CLS_BWD=0 in the environment: the full-height form throughout.
 * Replaces: the same `loss.backward()` (qat_trainer.py:359). */
#define QATVIT_FWD_X16 2        /* forward: h1q / h2q as fp16 integers (needs qatvit_student_dy16_supported) */
#define QATVIT_BWD_DY16 2       /* backward: the one-plane form (the forward ran with QATVIT_FWD_X16, the workspace is calibrated) */
#define QATVIT_BWD_CALIBRATE 4  /* backward: the pair form, recording the maxima the next one-plane backward scales by (the forward ran WITHOUT QATVIT_FWD_X16) */
int32_t qatvit_student_dy16_supported(const qatvit_cfg* cfg);
/* Which LayerNorms of a forward with `flags` run inside the statistics pass that follows them (qatvit_i8_strip_ln) instead of as a launch of their own:
 * bit 0 = norm1 (attn.qkv), bit 1 = norm2 (mlp.fc1), of every block.  QATVIT_LN_STRIP=0 in the environment: 0. */
int32_t qatvit_student_ln_in_strip(const qatvit_cfg* cfg, int32_t flags);
/* h1q / h2q of every block from fp16 integers back to bf16 integers, in place (fallback after an overflow: the pair form reads bf16) */
/* Host mirror of the one-plane backward's overflow flag: host_pinned = int32[2] in pinned host memory (hipHostMalloc / torch pin_memory), NULL to remove it.  Every
 * backward call then writes {overflow flag, generation} there - the generation (a counter that changes with every call) after the flag, system scope - as soon as the
 * gradient planes' maxima are known, i.e. BEFORE the call's deferred weight gradients run: a host that polls the generation instead of synchronising with the stream can
 * queue the next step 2 - 3 ms earlier.  qatvit_student_init clears the mirror. */
int qatvit_student_dy16_set_mirror(const qatvit_cfg* cfg, void* workspace, void* host_pinned, void* stream);
int qatvit_student_dy16_to_pair(const qatvit_cfg* cfg, void* workspace, void* stream);
/* Stochastic depth (drop-path): a per-sample multiplier on each residual branch, x = x + fq(branch) * s - behind the activation fake-quant of the proj / fc2
 * output and in front of the add, where the DropPath module stands in the prepared tree.
 *  scale_table: DEVICE float [2 * depth][batch] for the cfg->batch of the calls that follow, indexed [branch][sample]; row 2 i = block i's attention branch,
 *  row 2 i + 1 = its MLP branch.  Any finite multipliers (timm's DropPath: 0 or 1 / keep).  NULL unbinds.
 * Host-side binding only (no launch, no stream): every forward / backward entry on this workspace - qatvit_student_forward, _backward and the staged / part
 * entries qatvit_student_forward_stages, _forward_part, _backward_stages - reads the table bound at the time of the call.  Contract: a forward and the
 * backward that follows it read the SAME table at the SAME address (bind once, rewrite its contents between steps); nothing bound - the state after
 * qatvit_student_init, which unbinds - is the step without drop-path, with the same launches as before this entry existed.
 * Lifetime: the binding is keyed by the workspace ADDRESS and outlives the memory.  Unbind (NULL) before freeing a workspace or its table, or call the
 * workspace's _init entry on whatever is placed at that address next; the library never dereferences a table outside a forward / backward call.
 * Forward: product and sum are rounded separately (no fused multiply-add), as the two stock ops round them, so equal fq(branch) gives bit-equal x and an
 * all-ones table gives the bits of the step without one.  Backward: the gradient entering the branch is (d loss / d x) * STE mask * s[sample], in the pair and
 * the one-plane form (whose recorded maxima include s) and on the class-token rows of the last block.
 * Two limits.  With a table bound, the LayerNorm backward runs as its own kernel behind the plain fc1 / qkv dgrad, not in the dgrad's epilogue (that epilogue
 * does not know the multipliers).  The GEMMs of a dropped sample (s = 0) are not skipped: it costs what a kept one costs, as in stock torch. */
int qatvit_student_set_drop_path(const qatvit_cfg* cfg, void* workspace, const float* scale_table);
/* LayerScale (timm's init_values): a learnable per-channel gamma on each residual branch, x = x + (fq(branch) * gamma[c]) * s[sample] - behind the activation
 * fake-quant of the proj / fc2 output and in front of DropPath, where the LayerScale module stands in the prepared tree (it has no observer).
 *  gammas: HOST array of 2 * depth DEVICE pointers to fp32 gamma[embed_dim]; entry 2 i = block i's attention branch (ls1), 2 i + 1 = its MLP branch (ls2).
 *  grads: HOST array of 2 * depth DEVICE pointers to fp32 [embed_dim] gradient buffers, ZERO on entry of a backward and accumulated into, as `grads` of the
 *  backward entries; NULL for a binding that serves forwards only (a backward on it is refused).  Both arrays are copied.  gammas == NULL unbinds.
 * The parameter order of params / grads (8 + 12 * depth) does not change: the gammas travel through this binding alone.
 * Host-side binding keyed by the workspace address, with the rules of qatvit_student_set_drop_path: every forward / backward / staged / part entry reads the
 * binding of the time of the call; nothing bound - the state after qatvit_student_init, which unbinds - is the step without LayerScale with the same launches.
 * Arithmetic.  Forward: each product and the sum are rounded separately (no fused multiply-add); without a drop-path table there is no "* s".  gamma == 1
 * everywhere therefore gives the bits of the step without LayerScale.  Backward: the gradient entering the branch is (d loss / d x) * STE mask * s * gamma[c], in
 * the pair form, the one-plane form (recorded maxima: of the scaled value) and on the class-token rows of the last block; gamma's own gradient is
 * sum over rows of (d loss / d x)[row, c] * s[sample] * fq(branch)[row, c] WITHOUT the STE mask (d (fq(Y) * g) / dg = fq(Y) whether or not Y clamped): the
 * LayerNorm-backward kernel reads the block's pre-FQ proj / fc2 output again and re-applies that quantizer.  gamma == 0 is fine: nothing divides by gamma.
 * Limit: with a binding the LayerNorm backward runs as its own kernel behind the plain fc1 / qkv dgrad, as under drop-path (the fused epilogue does not know
 * gamma). */
int qatvit_student_set_layer_scale(const qatvit_cfg* cfg, void* workspace, const float* const* gammas, float* const* grads);
int qatvit_student_forward_stages(const qatvit_cfg* cfg, void* const* params, const qatvit_fq* act_fq, const qatvit_fq* weight_fq,
                                  const float* images, float* logits, void* workspace, int32_t stage_from, int32_t stage_to, int32_t flags,
                                  void* stream);
/* One of the four parts of one transformer block of the forward - each begins where a test can inject the oracle's tensor behind a
 * fake-quantizer that would otherwise amplify upstream one-step flips (a flipped key perturbs a whole head's attention; a flipped fc1
 * code a whole row of fc2 outputs):
 *   part 0: norm1 -> qkv GEMM                                         input x_in[block]            ("x_in")
 *   part 1: attention -> proj GEMM -> residual (+ norm2 statistics)    input pre-fake-quant qkv     ("qkv"; reads x_in[block] as it stands)
 *   part 2: norm2 -> fc1 (both passes) -> GELU                         input x_mid[block]           ("x_mid")
 *   part 3: fc2 GEMM -> residual (+ next LayerNorm's statistics)       input the GELU output: "G_hi"/"G_lo" (bf16 pair, backward operand) and
 *                                                                      what the forward GEMM reads - "G8"[block] (uint8 grid index per element)
 *                                                                      + "glut"[block] (256 packed fp16 hi | lo << 16 pairs) + "scal16"[1]
 *                                                                      (QATVIT_FC2_CODES=0: the planes "G16_hi"/"G16_lo"); reads x_mid[block]
 * parts 0..3 in order == forward stage block + 1.  QATVIT_STAGE_INJECT: that input was written by the caller; the observer statistics
 * (and LayerNorm row statistics) its producer would have left are recomputed first. */
int qatvit_student_forward_part(const qatvit_cfg* cfg, void* const* params, const qatvit_fq* act_fq, const qatvit_fq* weight_fq, void* workspace,
                                int32_t block, int32_t part, int32_t flags, void* stream);
int qatvit_student_backward_stages(const qatvit_cfg* cfg, void* const* params, const qatvit_fq* act_fq, const qatvit_fq* weight_fq,
                                   const float* dlogits, void* const* grads, void* workspace, int32_t stage_from, int32_t stage_to, int32_t flags,
                                   void* stream);
/* ---------------------------------------------------------------------------
 * Frozen KD teacher forward (no fake-quant, no gradient).
 * Replaces: `with torch.no_grad(): teacher_out = teacher(images)` (qat_trainer.py:337-338).
 *  cfg: same struct (the quantisation fields are ignored).  params: fp32 tensors in the student's order.
 *  w_hi / w_lo: bf16 (hi, lo) pairs of the 2-D weights, in weight_fq order without the head
 *  (patch_embed.proj, then per block qkv, proj, fc1, fc2), prepared once by the host since the weights are frozen.
 *  Every product is float x float: three bf16 MFMA passes (hi.hi + lo.hi + hi.lo), fp32 accumulate. */
int64_t qatvit_teacher_workspace_bytes(const qatvit_cfg* cfg);
int qatvit_teacher_forward(const qatvit_cfg* cfg, void* const* params, void* const* w_hi, void* const* w_lo,
                           const float* images, float* logits, void* workspace, void* stream);
/* The same forward on fp16 MFMA (v_mfma_f32_16x16x32_f16): w16 = the 2-D weights rounded to fp16 (same order as w_hi; the caller checks
 * |w| < 65504), activations as an fp16 (hi, lo) pair (passes == 2: 22 significant bits x 11) or as fp16 alone (passes == 1).  Same workspace.
 * embed_dim and mlp_hidden multiples of 384.  Error against the fp64 tree and time per form: profiles/round3_teacher_precision.txt. */
int qatvit_teacher_forward_f16(const qatvit_cfg* cfg, void* const* params, void* const* w16, int32_t passes,
                               const float* images, float* logits, void* workspace, void* stream);

/* ---------------------------------------------------------------------------
 * Float (pre-QAT) student step: forward + backward of the UNPREPARED QATWrapper(vit_*_patch16_224), fp32-accurate.
 * Replaces: `student_out = model(images)` ... `loss.backward()` of the reference's float epochs (qat_trainer.py:295-361 before
 * prepare_qat; train_final.sh runs them in fp32, the Optuna objective under autocast + GradScaler).
 *  cfg: same struct (the quantisation fields are ignored); cfg->batch is a run-time argument - a workspace sized for batch B serves
 *  every batch <= B.  Limits: embed_dim % 128 == 0 and <= 768, head_dim 32 or 64, <= 224 tokens, depth <= 12, no dropout
 *  (drop-path: qatvit_float_student_set_drop_path, LayerScale: qatvit_float_student_set_layer_scale, both below).
 *  params / grads: fp32 tensors in the student's order above.  grads must be ZERO on entry: the backward accumulates into them.
 *  Every GEMM operand is a bf16 (hi, lo) pair, three MFMA passes per product (hi.hi + lo.hi + hi.lo), fp32 accumulate; the attention
 *  backward runs in fp32 FMA.  The forward leaves in the workspace what the backward reads (one forward per workspace at a time). */
int64_t qatvit_float_student_workspace_bytes(const qatvit_cfg* cfg);
int qatvit_float_student_init(const qatvit_cfg* cfg, void* workspace, void* stream);
int qatvit_float_student_forward(const qatvit_cfg* cfg, void* const* params, const float* images, float* logits, void* workspace, void* stream);
int qatvit_float_student_backward(const qatvit_cfg* cfg, void* const* params, const float* dlogits, void* const* grads, void* workspace,
                                  void* stream);
/* Stochastic depth (drop-path) for a float-step workspace of ANY of the three forms (fp32-accurate, fp16, bf16 - each has its own workspace; the observe-only
 * forward runs on the fp32 form's): x = x + branch * s[sample].  scale_table, its indexing, the host-side binding and the contract are those of
 * qatvit_student_set_drop_path: DEVICE float [2 * depth][batch], row 2 i = block i's attention branch, row 2 i + 1 = its MLP branch; the forward and the
 * backward that follows read the same table at the same address; NULL, or nothing bound (the state after the form's _init), is the step without drop-path
 * with the same launches as before.  fp32-accurate form: the product in fp32.  fp16 / bf16 forms: as stock autocast - the branch output and s are values
 * of the 16-bit type, their product is rounded to that type, the add is fp32.  Backward: the gradient entering the branch is (d loss / d x) * s[sample],
 * with s as the table holds it: the forward of the 16-bit forms rounds s to the type, the backward does not, so a caller that wants stock autocast's
 * gradient (one 16-bit mask in both directions) stores multipliers that the type represents (qat_vit_amd's engine stores the table rounded).
 * The GEMMs of a dropped sample are not skipped. */
int qatvit_float_student_set_drop_path(const qatvit_cfg* cfg, void* workspace, const float* scale_table);
/* LayerScale for a float-step workspace of ANY of the three forms: x = x + (B * gamma[c]) * s[sample].  gammas / grads, their indexing, the host-side binding and
 * its rules are those of qatvit_student_set_layer_scale.
 *  saved: DEVICE buffer of qatvit_float_student_layer_scale_bytes(cfg) bytes (cfg->batch = the largest batch of the calls that follow): fp32
 *  [2 * depth][batch * tokens, embed_dim], and 256 bytes of per-branch scales behind them (the fp16 form's backward, below).  The float forms keep ONE shared branch-output tensor, not one per block; with a binding each forward writes every
 *  branch output to its own rows of `saved` instead, and the backward reads them for gamma's gradient.  Required with grads; NULL serves forwards only.  No
 *  existing workspace changes its size.
 * fp32-accurate form: B = the branch output, every product and the sum rounded separately in fp32.  fp16 / bf16 forms: as stock autocast - B is the branch output
 * rounded to the 16-bit type, gamma is an fp32 parameter, so type promotion makes B * gamma an fp32 tensor and DropPath multiplies it in fp32:
 * x = x + fl32(fl32(B * gamma) * s) with NEITHER the product NOR s rounded to the 16-bit type (without LayerScale the drop-path kernel rounds both: a caller that
 * binds both binds the table unrounded).  Backward: the gradient entering the branch is (d loss / d x) * s * gamma[c]; gamma's gradient is
 * sum over rows of (d loss / d x)[row, c] * s[sample] * B[row, c].
 * fp16 form: stock autocast holds every gradient inside a branch in fp16, each carrying the branch's gamma - at gamma = 1e-5 in or under fp16's subnormal range.
 * The backward carries them multiplied by K = 2^-e (max |gamma| = m * 2^e, m in [0.5, 1); clamped to [1, 2^24], so K = 1 for max |gamma| >= 0.5), computed on the
 * device per branch and step, and undoes K exactly in the weight gradients and in the dgrad that leaves the branch: more digits than stock autocast for small
 * gammas, the same arithmetic otherwise.  The overflow rule of the fp16 weight / bias gradients applies to the unscaled values, as before. */
int qatvit_float_student_set_layer_scale(const qatvit_cfg* cfg, void* workspace, const float* const* gammas, float* const* grads, void* saved);
int64_t qatvit_float_student_layer_scale_bytes(const qatvit_cfg* cfg);
/* Observe-only form: the PREPARED student with fake_quant_enabled = 0 on every fake-quant module (torch.ao.quantization.disable_fake_quant).  Stock
 * FusedMovingAvgObsFakeQuantize then passes every tensor through unchanged (gradient: the identity) and, where observer_enabled = 1, still moves
 * running_min / running_max by the EMA (c = cfg->averaging_const); scale / zero_point are not written.  The forward is qatvit_float_student_forward
 * - the same arithmetic, bit for bit - that also reduces the min / max at all fake-quant points: the images, the patch-embedding / qkv / proj / fc1 /
 * fc2 / head outputs (fp32 with bias; proj and fc2 before the residual add, fc1 before GELU), the fp32 norm1 / norm2 / final-norm outputs, and the
 * weights (per tensor, or per output channel with cfg->w_per_channel).  Every observer is folded at the end of the forward with its module's own
 * device flags (nothing in the forward reads the quantisers' state).  The backward is qatvit_float_student_backward unchanged.
 *  observe: a device buffer of qatvit_float_student_observe_bytes(cfg) bytes (batch independent), bound once to the modules' buffers by
 *  qatvit_float_student_observe_init (act_fq / weight_fq in the orders above; synchronises the stream) before its first forward. */
int64_t qatvit_float_student_observe_bytes(const qatvit_cfg* cfg);
int qatvit_float_student_observe_init(const qatvit_cfg* cfg, const qatvit_fq* act_fq, const qatvit_fq* weight_fq, void* observe, void* stream);
int qatvit_float_student_forward_observe(const qatvit_cfg* cfg, void* const* params, const float* images, float* logits, void* workspace, void* observe,
                                         void* stream);
/* fp16 (autocast) form: what the step computes inside torch.autocast("cuda", dtype=torch.float16), following stock autocast.  Every GEMM operand is
 * ONE fp16 plane (the weights are re-cast by every forward, as stored and transposed), one v_mfma_f32_16x16x32_f16 pass per product, fp32 accumulate;
 * the residual stream, LayerNorm, softmax statistics and lse stay fp32, GEMM outputs are kept in fp32.  Overflow follows stock: every tensor stock
 * holds in fp16 overflows to +-inf where it is rounded to fp16, and the Linear / Conv2d weight and bias gradients (fp16 in stock) become +-inf
 * where |g| exceeds fp16's range - so GradScaler skips the same kinds of steps.  Limits: those of the fp32 form, plus embed_dim and mlp_hidden
 * multiples of 384.  Separate workspace (smaller than the fp32 form's), sized and initialised like it.
 *  forward: logits_f16 = [batch, num_classes] fp16.  backward: dlogits_f16 = [batch, num_classes] fp16; grads as qatvit_float_student_backward
 *  (fp32, ZERO on entry). */
int64_t qatvit_float_student_amp_workspace_bytes(const qatvit_cfg* cfg);
int qatvit_float_student_amp_init(const qatvit_cfg* cfg, void* workspace, void* stream);
int qatvit_float_student_amp_forward(const qatvit_cfg* cfg, void* const* params, const float* images, void* logits_f16, void* workspace, void* stream);
int qatvit_float_student_amp_backward(const qatvit_cfg* cfg, void* const* params, const void* dlogits_f16, void* const* grads, void* workspace,
                                      void* stream);
/* The fp16 form's attention backward alone (kernel-level checks): qkv fp32 [B*T, 3*D], O16 fp16 [B*T, D], lse fp32 [B][H][T] (natural log of the
 * softmax denominator of the scaled scores), dO fp32 [B*T, D] -> dqkv16 fp16 [B*T, 3*D] (dQ, dK, dV in the qkv layout).  qkv and dO are rounded
 * to fp16 on load.  One fused kernel, one workgroup per (image, head); head_dim 32 or 64, T <= 224. */
int qatvit_float_student_amp_attn_backward(const float* qkv, const void* O16, const float* lse, const float* dO, int32_t B, int32_t T, int32_t H,
                                           int32_t D, void* dqkv16, void* stream);
/* bf16 (autocast) form: what the step computes inside torch.autocast("cuda", dtype=torch.bfloat16) - the fp16 form above with every 16-bit plane
 * in bf16 (round to nearest even, NaN kept) and every product one v_mfma_f32_16x16x32_bf16 pass, fp32 accumulate; logits and dlogits in bf16.  bf16
 * has fp32's exponent range, so there is no overflow rule: inf and NaN reach the gradients as in stock.  Limits, workspace and calling sequence are
 * the fp16 form's (its own workspace, of the fp16 form's size).
 *  forward: logits_bf16 = [batch, num_classes] bf16.  backward: dlogits_bf16 = [batch, num_classes] bf16; grads fp32, ZERO on entry. */
int64_t qatvit_float_student_bf16_workspace_bytes(const qatvit_cfg* cfg);
int qatvit_float_student_bf16_init(const qatvit_cfg* cfg, void* workspace, void* stream);
int qatvit_float_student_bf16_forward(const qatvit_cfg* cfg, void* const* params, const float* images, void* logits_bf16, void* workspace, void* stream);
int qatvit_float_student_bf16_backward(const qatvit_cfg* cfg, void* const* params, const void* dlogits_bf16, void* const* grads, void* workspace,
                                       void* stream);
/* The bf16 form's attention backward alone: as qatvit_float_student_amp_attn_backward with O16 and dqkv16 in bf16 (qkv and dO rounded to bf16 on
 * load), on bf16 MFMA. */
int qatvit_float_student_bf16_attn_backward(const float* qkv, const void* O16, const float* lse, const float* dO, int32_t B, int32_t T, int32_t H,
                                            int32_t D, void* dqkv16, void* stream);

/* ---------------------------------------------------------------------------
 * Integer inference forward of the trained student from its exported integers.
 * Replaces: the last-epoch  convert(base.eval()) ... evaluate_quantized_cpu(...)  of qat_trainer.py:376-388 (an eager int8 model for the CPU
 * backends only).  int8 MFMA for every grid x grid product; qparams are frozen, so each GEMM epilogue quantises at once: no pre-fake-quant fp32
 * tensor exists, qkv leaves its GEMM as uint8 codes, fc1 as one byte per element + a 256-entry table of the fp16 pairs of gelu(fq(.)) (the fp16 pair
 * itself where the strip kernel does not apply), proj / fc2 add fq(.) into the fp32 residual stream
 * (which the reference keeps in fp32 as well).  Logits are bit-identical to qatvit_student_forward with the observers switched off.
 *  cfg: as for the student step.  Shapes: embed_dim and mlp_hidden multiples of 384, head_dim 64 or 32.
 *  w8: n_weight_fq device pointers, int8 [N, K] row-major weight integers (q - zero_point; symmetric: zero_point 0), weight_fq order
 *      (patch_embed.proj as [D, C*P*P], per block qkv / proj / fc1 / fc2, head);  w_scale: same order, fp32 [1] or [N] (cfg->w_per_channel)
 *  act_scale / act_zero_point: device arrays [n_act_fq] in act_fq order (the frozen activation quantizers)
 *  params: the student's parameter table (fp32; the six 2-D weight slots are not read: may be NULL)
 * prepare() derives what the forward needs beside the integers (reciprocal scales, weight row sums, fp16 and fragment-order copies) into the head of the workspace -
 * once per set of weights; the same workspace then serves every batch size <= the one it was sized for. */
int64_t qatvit_infer_workspace_bytes(const qatvit_cfg* cfg);
int qatvit_infer_prepare(const qatvit_cfg* cfg, const void* const* w8, const float* act_scale, const int32_t* act_zero_point, void* workspace,
                         void* stream);
int qatvit_infer_forward(const qatvit_cfg* cfg, void* const* params, const void* const* w8, const float* const* w_scale, const float* images,
                         float* logits, void* workspace, void* stream);
/* The same forward for a student with LayerScale (init_values): ls_gamma = 2 * depth device pointers, entry 2 i = block i's ls1 (attention branch), entry
 * 2 i + 1 = its ls2 (MLP branch), fp32 [embed_dim] each.  attn.proj and mlp.fc2 of every block then update the residual stream as
 *   x[m,n] = x[m,n] + fl(fq(v[m,n]) * gamma[n])      (the ls_gamma form of qatvit_gemm_nt_resid_fq: product and sum rounded separately)
 * and nothing else changes: the same workspace, qatvit_infer_prepare and qatvit_infer_workspace_bytes.  ls_gamma == NULL is qatvit_infer_forward (one body
 * serves both); a non-null array with a null entry is refused before any HIP call.  Logits are bit-identical to qatvit_student_forward of the LayerScale
 * model with the observers switched off. */
int qatvit_infer_forward_ls(const qatvit_cfg* cfg, void* const* params, const void* const* w8, const float* const* w_scale, const float* const* ls_gamma,
                            const float* images, float* logits, void* workspace, void* stream);

/* ---------------------------------------------------------------------------
 * Gradient clipping + AdamW: the two statements that follow the hot path in the reference's loop.
 * Replaces: torch.nn.utils.clip_grad_norm_(ddp_model.parameters(), 1.0); optimizer.step()   (qat_trainer.py:360-361)
 *           with optimizer = torch.optim.AdamW(params, lr=..., weight_decay=...)             (qat_trainer.py:271-276).
 * Tensors stay separate torch allocations: *_ptrs are DEVICE arrays of n_tensors device pointers (fp32), numel a device
 * int64 array.  Work is dealt in chunks of chunk_elems (a multiple of 4): chunk c covers elements
 * [chunk_index[c]*chunk_elems, ...) of tensor chunk_tensor[c]; both tables are device int32 arrays of n_chunks entries
 * built once by the host.  No atomics: results are bit-reproducible run to run.
 *
 * grad_norm: partials = device scratch [n_chunks] fp32; out2 = {total L2 norm, min(1, max_norm/(total+1e-6))};
 *            max_norm < 0 -> coefficient 1 (norm only).  Gradients are NOT modified: pass out2 to qatvit_optim_adamw.
 * adamw:     in-place update of params / exp_avg / exp_avg_sq for 1-based step `step`; hyper-parameters are doubles because
 *            torch forms 1-beta, lr*wd, lr/(1-beta1^t), sqrt(1-beta2^t) in double before narrowing to fp32; clip_out2 = NULL or the out2 above
 *            (gradients enter multiplied by out2[1], as if clip_grad_norm_ had scaled them). */
int qatvit_optim_grad_norm(const void* grad_ptrs, const int64_t* numel, const int32_t* chunk_tensor, const int32_t* chunk_index,
                           int32_t n_chunks, int64_t chunk_elems, float max_norm, float* partials, float* out2, void* stream);
int qatvit_optim_adamw(const void* param_ptrs, const void* grad_ptrs, const void* exp_avg_ptrs, const void* exp_avg_sq_ptrs,
                       const int64_t* numel, const int32_t* chunk_tensor, const int32_t* chunk_index, int32_t n_chunks,
                       int64_t chunk_elems, double lr, double beta1, double beta2, double eps, double weight_decay, int64_t step,
                       const float* clip_out2, void* stream);

/* adamw_groups: the same update for the tensors of up to QATVIT_OPTIM_MAX_GROUPS param groups in ONE launch (with grad_norm over the same tables:
 *            one global norm, one update, whatever the number of groups).  The tables span all groups; tensor_group is a DEVICE int32 array with
 *            one entry per tensor, the index of that tensor's row in `groups`; a tensor whose entry is outside [0, n_groups) is left untouched.
 *            `groups` is HOST memory, read during the call only: each row's hyper-parameters become the prefactors qatvit_optim_adamw forms (in
 *            double, narrowed once) and travel in the kernel-argument block, so a changed lr costs no copy.  step is 1-based and per group.
 *            A tensor is updated to the same bits as by qatvit_optim_adamw with its group's values. */
#define QATVIT_OPTIM_MAX_GROUPS 64
typedef struct qatvit_adamw_group {
    double lr, beta1, beta2, eps, weight_decay;
    int64_t step;
} qatvit_adamw_group;
int qatvit_optim_adamw_groups(const void* param_ptrs, const void* grad_ptrs, const void* exp_avg_ptrs, const void* exp_avg_sq_ptrs,
                              const int64_t* numel, const int32_t* tensor_group, const int32_t* chunk_tensor, const int32_t* chunk_index,
                              int32_t n_chunks, int64_t chunk_elems, const qatvit_adamw_group* groups, int32_t n_groups,
                              const float* clip_out2, void* stream);

/* Weight EMA: an exponential moving average of every parameter, kept by the update launch itself, and the in-place exchange that puts it to use.
 * ema_ptrs is a DEVICE array of n_tensors fp32 device pointers (one average per tensor, the tensor's numel, disjoint from every other operand);
 * ema_decay is one value for all tensors and groups and travels by value in the kernel arguments, so a scheduled decay costs no copy and no sync.
 * Arithmetic, exactly: with w = (float)(1.0 - ema_decay) (double on the host, narrowed once), p' the fp32 parameter value the update just produced
 * (for qatvit_optim_ema: the parameter as it stands) and e the average,
 *     d  = p' - e
 *     e' = (w < 0.5f) ? e + w * d : p' - d * (1.0f - w)
 * every operation rounded to fp32, none fused (the library is built with -ffp-contract=off).  This is ATen's lerp(e, p', w) in both of its
 * branches; ema_decay = 0 gives e' = p' exactly.
 * adamw_ema / adamw_groups_ema: qatvit_optim_adamw / qatvit_optim_adamw_groups with the average as one more read-modify-write stream (36 B per
 *            parameter instead of 28, no extra launch): same tables, same checks; params, exp_avg and exp_avg_sq come out with the same bits as
 *            through the entries without the average.  All five tensors of a parameter must be 16-byte aligned for the vector path; otherwise
 *            that tensor takes the scalar path.
 * ema:       the same average as a launch of its own over (param, ema) pairs, for tensors that take no update in a step; params are read only.
 * swap:      exchanges the contents of a[t] and b[t] in place, bit for bit (16 B per element); a[t] and b[t] must not overlap.
 * Errors (before any HIP call): a null pointer, bad chunking, the hyper-parameter errors of the entry without the average, ema_decay outside
 * [0, 1) or NaN. */
int qatvit_optim_adamw_ema(const void* param_ptrs, const void* grad_ptrs, const void* exp_avg_ptrs, const void* exp_avg_sq_ptrs,
                           const void* ema_ptrs, const int64_t* numel, const int32_t* chunk_tensor, const int32_t* chunk_index,
                           int32_t n_chunks, int64_t chunk_elems, double lr, double beta1, double beta2, double eps, double weight_decay,
                           int64_t step, double ema_decay, const float* clip_out2, void* stream);
int qatvit_optim_adamw_groups_ema(const void* param_ptrs, const void* grad_ptrs, const void* exp_avg_ptrs, const void* exp_avg_sq_ptrs,
                                  const void* ema_ptrs, const int64_t* numel, const int32_t* tensor_group, const int32_t* chunk_tensor,
                                  const int32_t* chunk_index, int32_t n_chunks, int64_t chunk_elems, const qatvit_adamw_group* groups,
                                  int32_t n_groups, double ema_decay, const float* clip_out2, void* stream);
int qatvit_optim_ema(const void* param_ptrs, const void* ema_ptrs, const int64_t* numel, const int32_t* chunk_tensor, const int32_t* chunk_index,
                     int32_t n_chunks, int64_t chunk_elems, double ema_decay, void* stream);
int qatvit_optim_swap(const void* a_ptrs, const void* b_ptrs, const int64_t* numel, const int32_t* chunk_tensor, const int32_t* chunk_index,
                      int32_t n_chunks, int64_t chunk_elems, void* stream);

/* LAMB with per-tensor trust ratios: two launches behind qatvit_optim_grad_norm, over the same tables (all param groups in each launch; the groups
 * form with n_groups >= 1 is the only one).  Arithmetic, exactly - timm's Lamb with that class's defaults - for every tensor p with gradient g, the
 * row lr, (b1, b2), eps, weight_decay = wd, step = t (1-based) of its group, and coef = clip_out2[1] (1 where clip_out2 is NULL):
 *     g   <- g * coef
 *     m   <- b1 * m + (1 - b1) * g                       (grad_averaging = 0: m <- b1 * m + g)
 *     v   <- b2 * v + (1 - b2) * g * g
 *     r    = (m / (1 - b1^t)) / (sqrt(v) / sqrt(1 - b2^t) + eps) + wd * p
 *     trust = ||p||_2 / ||r||_2  if (wd != 0 or always_adapt) and ||p|| > 0 and ||r|| > 0, else 1;   trust_clip: min(trust, 1)
 *     p   <- p - lr * trust * r
 * ||p|| is the norm of the weight before the update; both norms are per tensor, never per group.  Every fp32 operation is rounded on its own, in
 * the order written (-ffp-contract=off); 1 - b1, 1 - b2, 1 - b1^t and sqrt(1 - b2^t) are formed in double and narrowed once; lr * trust is one
 * product per tensor.  coef is qatvit_optim_grad_norm's min(1, max_norm / (total + 1e-6)) over ALL groups (timm divides by max(total / max_norm,
 * 1): a stated deviation).  The squares are added in fp32 inside a chunk and in double across the chunks of a tensor, in a fixed order: no
 * atomics, bit-reproducible run to run.
 * lamb_moments: reads params, grads, exp_avg, exp_avg_sq; writes exp_avg, exp_avg_sq and partials2 = device fp32 [n_chunks][2] = per chunk
 *            {sum r^2, sum p^2}.  params are NOT written (16 B read + 8 B written per parameter).
 * lamb_apply: adds up each tensor's partials (tensor_first_chunk = device int32 [n_tensors], the index in the chunk tables of the tensor's chunk 0;
 *            a tensor's chunks are contiguous and ascending there), forms trust, forms r again from the exp_avg / exp_avg_sq that lamb_moments
 *            wrote and the untouched params - the same expression, the same bits - and writes params (12 B + 4 B per parameter).  ema_ptrs = NULL
 *            or the averages of the weight EMA above, e <- lerp(e, p_new, 1 - ema_decay), 8 B per parameter more; ema_decay is read only then.
 *            The branches are those stated there, each with its multiply-add as ONE fused operation: with d = p_new - e,
 *                e' = (w < 0.5f) ? fma(w, d, e) : fma(-d, 1.0f - w, p_new)
 *            which is how stock torch.lerp rounds (CPU and GPU): the average is torch.equal to torch.lerp(e, p_new, 1 - ema_decay) applied after
 *            the step, and within one rounding of the two-rounding form of qatvit_optim_ema, which still averages the tensors a step leaves out.
 *            trust_out = NULL or device fp32 [n_tensors]: the trust each tensor was updated with.
 * Both take the same `groups` (HOST memory, read during the call; the prefactors travel in the kernel arguments) and the same tensor_group; a tensor
 * whose entry is outside [0, n_groups) is left untouched by both (its partials are zeros, its trust_out entry is not written).
 * Errors (before any HIP call): a null table, n_chunks <= 0, chunk_elems <= 0 or not a multiple of 4, n_groups outside [1,
 * QATVIT_OPTIM_MAX_GROUPS], a row with lr < 0, eps < 0, a beta outside [0, 1), weight_decay < 0 or step < 1, and with ema_ptrs an ema_decay
 * outside [0, 1) or NaN. */
typedef struct qatvit_lamb_group {
    double lr, beta1, beta2, eps, weight_decay;
    int64_t step;
    int32_t grad_averaging, always_adapt, trust_clip, reserved;   /* flags: 0 / non-zero; reserved = 0 */
} qatvit_lamb_group;
int qatvit_optim_lamb_moments(const void* param_ptrs, const void* grad_ptrs, const void* exp_avg_ptrs, const void* exp_avg_sq_ptrs,
                              const int64_t* numel, const int32_t* tensor_group, const int32_t* chunk_tensor, const int32_t* chunk_index,
                              int32_t n_chunks, int64_t chunk_elems, const qatvit_lamb_group* groups, int32_t n_groups,
                              const float* clip_out2, float* partials2, void* stream);
int qatvit_optim_lamb_apply(const void* param_ptrs, const void* exp_avg_ptrs, const void* exp_avg_sq_ptrs, const void* ema_ptrs,
                            const int64_t* numel, const int32_t* tensor_group, const int32_t* tensor_first_chunk, const int32_t* chunk_tensor,
                            const int32_t* chunk_index, int32_t n_chunks, int64_t chunk_elems, const qatvit_lamb_group* groups, int32_t n_groups,
                            double ema_decay, const float* partials2, float* trust_out, void* stream);

/* ---------------------------------------------------------------------------
 * Input pipeline: uint8 images resident on the device -> the normalised fp32 batch.
 * Replaces: the per-image host transform of the loaders (qat_trainer.py:209-254, evaluator.py:22-41): Resize(D, BICUBIC) through Pillow,
 *   ToTensor(), Normalize(mean, std), and the host-to-device copy of the fp32 batch.  The result is EQUAL to theirs, element for element.
 *
 * Arithmetic (Pillow's 8-bit resample, square source S <= D, so the bicubic filter keeps support 2.0): per axis and output position xx,
 *   center = (xx + 0.5) * S / D, xmin = max(0, (int)(center - 1.5)), xmax = min(S, (int)(center + 2.5)), at most 4 taps
 *   w_i = cubic(i + xmin - center + 0.5) (a = -0.5), divided by their sum, coef_i = (int)(w_i * 2^22 +- 0.5), all in double;
 *   horizontal pass over the source rows, then vertical pass over its uint8 result, each clamp((2^21 + sum_i u8 * coef_i) >> 22, 0, 255) in int32;
 *   out[b][c][y][x] = table[c][byte], table[c][v] = ((float)v / 255 - mean[c]) / std[c] with IEEE fp32 divisions.
 *
 * qatvit_image_resize_coeffs / qatvit_image_table run on the HOST and make no HIP call: xmin[D], ntaps[D], coef[D][4] (unused taps 0) and
 *   table[3][256] are host arrays.  8 <= S <= D, D % 4 == 0, D <= 384.
 * qatvit_image_batch: one launch.  data uint8 [N, S, S, 3] (HWC, contiguous); index int64 [B] or NULL (images 0 .. B-1; then B <= N) - an
 *   index outside 0 .. N-1 is the caller's error (it reads image 0 or N-1, never outside data); coeffs int32 [6 * D] = the three arrays
 *   of qatvit_image_resize_coeffs(S, D) one after the other (xmin, ntaps, coef), table fp32 [768], both on the device;
 *   out fp32 [B, 3, D, D] contiguous, 16-byte aligned.  B <= 65535.
 *
 * qatvit_image_batch_aug: the same launch with a random crop and a horizontal flip of the uint8 SOURCE image in front of the resize, where
 *   Compose([RandomCrop(S, padding=p), RandomHorizontalFlip(), Resize(D, BICUBIC), ToTensor(), Normalize()]) has them.  aug int32 [B] on the
 *   device, 4-byte aligned, one word per batch POSITION b (not per image number index[b]):
 *     bits 0..7 oy (signed), bits 8..15 ox (signed), bit 16 flip, all other bits zero.
 *   The augmented image A of the source I (S x S x 3) is
 *     A[y][x][c] = E[y + oy][xf + ox][c],  xf = flip ? S-1-x : x
 *   where E extends I beyond its borders:
 *     padding_mode 0 (constant): a coordinate outside [0, S) gives the byte `fill` (0 .. 255, the same for all channels);
 *     padding_mode 1 (reflect, the edge not repeated, as np.pad(mode="reflect") and torchvision): u < 0 -> -u, u > S-1 -> 2(S-1) - u, the
 *       result then clamped to [0, S-1].
 *   This is torchvision's hflip(crop(pad(I, p), top = i, left = j)) with oy = i - p, ox = j - p.  The resize, the rounding, the value table and
 *   the output layout are qatvit_image_batch's: the result EQUALS qatvit_image_batch's on the uint8 image A.  Every word is safe: in constant
 *   mode an offset that moves the whole window off the image gives an all-`fill` source; in reflect mode the clamp keeps every read inside
 *   the image (one reflection is exact for |oy|, |ox| <= S-1).  aug == NULL launches qatvit_image_batch's kernel: no augmentation.
 *
 * qatvit_image_batch_mix: the same launch with mixup / cutmix behind the per-sample transforms, where timm's Mixup and torchvision's
 *   MixUp / CutMix have them.  mix int32 [B][6] on the device, contiguous, 4-byte aligned, one record per batch POSITION b:
 *     word 0  partner: batch position p of the second image; a value outside [0, B) means p = b (never an out-of-range read)
 *     word 1  w_self, fp32 bits            word 2  w_partner, fp32 bits
 *     word 3  y0 | y1 << 16: output rows y0 .. y1-1 of the box, each clamped to [0, D]
 *     word 4  x0 | x1 << 16: output columns x0 .. x1-1, clamped likewise; the box is empty if y1 <= y0 or x1 <= x0
 *     word 5  lam, fp32 bits: the weight of the sample's own label in qatvit_kd_ce_loss_mix (the partner's gets 1 - lam); unused here
 *   With X[b] = what qatvit_image_batch_aug writes for position b with word aug[b] (aug == NULL: what qatvit_image_batch writes), and the
 *   partner taken with its own word aug[p] - X[p], never a mixed row:
 *     out[b][c][y][x] = X[p][c][y][x]                                       inside the box,
 *                     = fl(fl(w_self * X[b]) + fl(w_partner * X[p]))        elsewhere: fp32, three roundings, no fused multiply-add
 *   (x * w_self + xp * w_partner as separate torch ops).  Mixup: an empty box, (w_self, w_partner) = (lam, 1 - lam).  Cutmix: a box, weights
 *   (1, 0), lam = 1 - area / D^2 of the clamped box.  Identity: weights (1, 0), an empty box, lam = 1: the result is X[b].
 *   The kernel keeps a second set of resampled planes in LDS: a shape whose request exceeds 64 KB (S and D both near 384) is refused with an
 *   error string before any HIP call.  mix == NULL: qatvit_image_batch_aug.
 *
 * qatvit_image_batch_rrc: the same launch with a resized crop of the uint8 SOURCE image per sample, where
 *   Compose([RandomResizedCrop(D, scale, ratio, BICUBIC), RandomHorizontalFlip(), ToTensor(), Normalize()]) has it.  rrc int32 [B][2] on the
 *   device, contiguous, 4-byte aligned, one record per batch POSITION b:
 *     word 0  top | left << 16            (16 bits each)
 *     word 1  h | w << 15 | flip << 30    (15 bits each, then one; bit 31 is ignored)
 *   all fields unsigned, 1 <= h, w <= S, top <= S - h, left <= S - w.  The source of position b is the uint8 window
 *   I[top : top + h, left : left + w] of its image, mirrored left to right when flip is set; Pillow's 8-bit bicubic resample (above) takes it
 *   to D x D: the horizontal pass with the table of w -> D, then the vertical pass over its uint8 result with the table of h -> D.  The value
 *   table and the output layout are qatvit_image_batch's.  The result EQUALS, element for element,
 *     Normalize(ToTensor(hflip?(crop(I, top, left, h, w)).resize((D, D), BICUBIC)))
 *   which is torchvision's resized_crop: crop, THEN resize (Pillow's resize(box=...) of the whole image is another function: its filter reads
 *   pixels outside the box).  The record (0, 0, S, S, flip = 0) gives qatvit_image_batch's result.
 *   A malformed record is made safe, not trusted: h and w are clamped to [1, S], then top to [0, S - h] and left to [0, S - w]; no read
 *   leaves the image, and the result is the clamped record's.
 *   windows int32 [S][6 * D] on the device, 4-byte aligned: table n - 1 (offset (n - 1) * 6 * D) is the three arrays xmin[D], ntaps[D],
 *   coef[D][4] of an n -> D resample one after the other, n = 1 .. S, as qatvit_image_resize_coeffs_windows(S, D, out_host) writes them on the
 *   HOST (no HIP call; the builder and the 24-bit / overflow / row-budget checks of qatvit_image_resize_coeffs, whose own refusal of a source
 *   below 8 stays; table S is qatvit_image_resize_coeffs(S, D)).  8 <= S <= D, D % 4 == 0, D <= 384.
 *   mix int32 [B][6] or NULL: the record of qatvit_image_batch_mix, with X[b] = what this entry writes for position b without mix, the
 *   partner taken with its own record rrc[p].  The LDS request (the mix form's two plane sets, plus the band's row-table entries per side) is
 *   refused above 64 KB with an error string before any HIP call.  rrc == NULL is refused: without records the call is qatvit_image_batch's.
 *
 * qatvit_image_batch_erase / qatvit_image_batch_rrc_erase: the same launches with RandomErasing (arXiv:1708.04896) behind Normalize and in front
 *   of the mix, where torchvision's reference recipe and timm without its prefetcher have it.  erase int32 [B][8] on the device, contiguous,
 *   4-byte aligned, one record per batch POSITION b:
 *     word 0  y0 | y1 << 16: output rows y0 .. y1-1 of the box, each bound clamped to [0, D]
 *     word 1  x0 | x1 << 16: output columns, clamped likewise; the box is empty if y1 <= y0 or x1 <= x0
 *     word 2, 3, 4  the fill of channel 0, 1, 2, fp32 bits, in normalised units (what the output holds)
 *     word 5  mode; only bit 0 is read: 0 = the constant fill of words 2..4, 1 = per-element standard-normal noise (words 2..4 unused)
 *     word 6, 7  k0, k1: the 64-bit key of the noise (mode 1)
 *   The all-zero record is the identity (an empty box).  With X[b] = what qatvit_image_batch_mix (without mix) / qatvit_image_batch_rrc
 *   (without mix) writes for position b with aug[b] / rrc[b]:
 *     E[b][c][y][x] = X[b][c][y][x] outside the box of erase[b]; inside it the fill of channel c (mode 0) or z(k0, k1, c, y, x) (mode 1).
 *   Without mix the output is E[b].  With mix it is qatvit_image_batch_mix's expression with E in the place of X: the partner contributes
 *   E[p], erased by its own record erase[p] - never a mixed row, and never an un-erased one.
 *   The noise z is a pure function of (key, c, y, x): the same record gives the same values at any batch position, as the sample or as a
 *   partner.  Philox4x32-10 (Salmon et al., SC'11; multipliers 0xD2511F53, 0xCD9E8D57, key increments 0x9E3779B9, 0xBB67AE85), key (k0, k1),
 *   counter (y * (D / 4) + x / 4, c, 0, 0): one call per four neighbouring columns, whose outputs r0 .. r3 give the elements x & 3 = 0 .. 3 by
 *   Box-Muller on the pairs (r0, r1) and (r2, r3):
 *     u = ((r_even >> 9) + 1) * 2^-23  in (0, 1],   t = (r_odd >> 8) * 2^-23  in [0, 2),   both exact in fp32,
 *     R = sqrtf(-2 * logf(u)),   the even element = R * cospif(t),   the odd element = R * sinpif(t)
 *   with the full-precision fp32 functions and no fused multiply-add.  The integer half is exact; the float half follows the device's math
 *   library to a few ulp (measured against an fp64 evaluation: profiles/erase_bench.txt).  |z| <= sqrt(46 ln 2) = 5.65.
 *   A malformed record is made safe, not trusted: the bounds are clamped, the other mode bits are ignored, and nothing is addressed through a
 *   record, so none can cause a read or a write outside out[b].  The kernels keep nothing more in LDS: the refusals are the siblings'.
 *   aug, mix may be NULL with their meanings above (no words; no mixing); rrc == NULL is refused.  erase == NULL makes the call
 *   qatvit_image_batch_mix's / qatvit_image_batch_rrc's: that entry's kernel is launched and the result is bitwise its result.
 *
 * qatvit_image_batch_color / qatvit_image_batch_rrc_color: the same launches with the colour augmentations of the fine-tuning recipes
 *   (torchvision's ColorJitter without hue, RandomGrayscale with three output channels, RandomSolarize) where those recipes have them: on the
 *   uint8 RGB D x D image behind the resize (what Pillow's resize returns) and in front of ToTensor() + Normalize(), so in front of the erase
 *   and of the mix.  color int32 [B][4] on the device, contiguous, 4-byte aligned, one record per batch POSITION b:
 *     word 0  bits 0-1, 2-3, 4-5: the jitter op of slot 0, 1, 2 (0 = none, 1 = brightness, 2 = contrast, 3 = saturation), applied in slot
 *             order; an op code that an earlier slot held is skipped.  Bit 8: grayscale.  Bit 9: solarize, with the threshold 0 .. 255 in
 *             bits 16-23.  All other bits are ignored.
 *     word 1, 2, 3  the factor of brightness, contrast, saturation, fp32 bits.  A factor that is negative or not finite makes its op the
 *             identity; factor 1 is the identity by the formula.
 *   The all-zero record is the identity.  Per sample, in this order: grayscale, solarize, the jitter ops.  For a pixel (R, G, B), with
 *   L(R, G, B) = (R * 19595 + G * 38470 + B * 7471 + 0x8000) >> 16 (Pillow's convert("L")):
 *     grayscale      R = G = B = L
 *     solarize(t)    v < t ? v : 255 - v, per channel (ImageOps.solarize)
 *     blend(in1, in2, a), per channel: t = fl32(fl32(in1) + fl32(a * fl32(in2 - in1))) with a in fp32, THE PRODUCT AND THE SUM ROUNDED ONE BY
 *                    ONE: a fused multiply-add is forbidden here (it changes 2 bytes in 1.5 million against Pillow's Image.blend);
 *                    0 <= a <= 1: out = (uint8) trunc(t); otherwise out = t <= 0 ? 0 : t >= 255 ? 255 : trunc(t)
 *     brightness(f)  blend(0, v, f)
 *     contrast(f)    blend(m, v, f), m = (2 * s + D * D) / (2 * D * D) in integers (Python's int(s / (D * D) + 0.5)), s = the sum of L over ALL
 *                    D x D pixels of this sample's image as it stands right in front of the contrast op: behind grayscale, solarize and the
 *                    jitter ops of the earlier slots.  s <= 255 * 384 * 384 < 2^26.
 *     saturation(f)  blend(L, v, f), L of the pixel as it stands
 *   The result EQUALS, byte for byte, what Pillow's ImageOps / ImageEnhance give (tests/golden/color_kat.npz).  The partner of a mix record is
 *   coloured by ITS OWN record color[p] with its own sum, as it is erased by its own record.  erase == NULL here means all-zero erase records.
 *   sums uint32 [B] on the device, 4-byte aligned: a workspace whose contents on entry are ignored.  The entry zeroes it on the stream and runs
 *   a statistics launch in front of the batch launch; on return sums[b] = s of position b, and 0 where record b holds no contrast op (after the
 *   cleaning above).  sums == NULL IS THE CALLER'S PROMISE THAT NO RECORD HOLDS A CONTRAST OP: no statistics launch runs, and a contrast op
 *   met anyway is the identity.
 *   A malformed record gives exactly the result of the cleaned record, and nothing is addressed through a record.  The kernels keep nothing
 *   more in LDS: the refusals are the siblings'.  color == NULL makes the call qatvit_image_batch_erase's / qatvit_image_batch_rrc_erase's:
 *   that entry's kernel is launched and the result is bitwise its result (sums is then not touched).
 *
 * qatvit_image_batch_blur / qatvit_image_batch_rrc_blur: the same launches with Gaussian blur, as DeiT-III's 3-Augment and timm apply it
 *   (img.filter(ImageFilter.GaussianBlur(radius))), on the uint8 RGB D x D image behind the resize.  Per sample the order is: grayscale,
 *   solarize, BLUR, the jitter ops of the colour record, then Normalize, the erase, the mix.  The sum s of a contrast op is taken of the image
 *   as it stands in front of that op, so behind the blur.  The partner of a mix record is blurred by ITS OWN record blur[p].
 *   blur int32 [B][4] on the device, contiguous, 4-byte aligned, one record per batch POSITION b:
 *     word 0  bit 0: blur on.  Bits 8-15: the integer box radius, at most 1.  All other bits are ignored.
 *     word 1  ww, the weight of the 2 * radius + 1 pixels around the centre, 1 .. 2^24
 *     word 2  fw, the weight of the two pixels at distance radius + 1, >= 0
 *     word 3  0 (ignored)
 *   Pillow computes the filter as three box passes along the rows, then three along the columns, every pass rounded to uint8, in integers.
 *   One pass over a line in[0 .. n-1], per channel, with clamp to 0 .. n-1 (the edge pixel is replicated):
 *     out[x] = (ww * SUM(|d| <= radius) in[clamp(x + d)] + fw * (in[clamp(x - radius - 1)] + in[clamp(x + radius + 1)]) + 2^23) >> 24
 *   in 32 unsigned bits.  The host forms the record from the Gaussian radius r in C float arithmetic, with passes = 3:
 *     sigma2 = r * r / passes, L = sqrt(12 * sigma2 + 1), l = floor((L - 1) / 2),
 *     a = (2 * l + 1) * (l * (l + 1) - 3 * sigma2) / (6 * (sigma2 - (l + 1)^2)), box = l + a, radius = (int)box,
 *     ww = (uint32)((float)(1 << 24) / (box * 2 + 1)), fw = ((1 << 24) - (2 * radius + 1) * ww) / 2
 *   e.g. r = 0.1: (0, 16721291, 27962); r = 2.0: (1, 4473924, 1677722).  The integer radius is at most 1 for Gaussian radii below sqrt(6);
 *   larger ones are not offered.  The device does no float arithmetic for the blur.  The result EQUALS Pillow's, byte for byte
 *   (tests/golden/blur_kat.npz).
 *   A record is cleaned, not trusted: it counts as "no blur" unless bit 0 is set, radius <= 1, 1 <= ww <= 2^24, fw >= 0 and
 *   (2 * radius + 1) * ww + 2 * fw <= 2^24; then every pass result is at most 255 and nothing overflows.  Nothing is addressed through a
 *   record.  A sample whose record is "no blur" goes through the colour entry's arithmetic and gets bitwise its result.
 *   The other records are qatvit_image_batch_color's; color == NULL here means all-zero colour records, erase == NULL all-zero erase records.
 *   The kernels keep a band of 8 output rows with up to 6 halo rows on each side, per side of a mix record, and one more such buffer in LDS:
 *   above 64 KB the call is refused with an error string before any HIP call (32 -> 224 with mix is served).  blur == NULL makes the call
 *   qatvit_image_batch_color's / qatvit_image_batch_rrc_color's: the result is bitwise its result.
 *
 * qatvit_image_window_u8: the window stage, a launch of its own IN FRONT of the batch launch, for sources that are not square or are larger
 *   than the output (the entries above refuse both).  data uint8 [N][H][W][3] (HWC, contiguous, on the device); index int64 [B] or NULL with
 *   the rule above (an index outside 0 .. N-1 is clamped and never reads outside data); rrc int32 [B][2], the record of
 *   qatvit_image_batch_rrc with S read as H for top / h and as W for left / w; out uint8 [B][D][D][3] (HWC, contiguous, 4-byte aligned).
 *   out[b] EQUALS, byte for byte,
 *     Image.fromarray(I).crop(window)[.transpose(FLIP_LEFT_RIGHT)].resize((D, D), BICUBIC)
 *   of image index[b] and record b: torchvision's resized_crop + hflip.  The batch launch at S = D on these bytes is the identity resize (the
 *   cubic at integer offsets is 0, 1, 0, 0), so qatvit_image_batch* (D, D) on out, with index == NULL and without rrc, applies colour, erase,
 *   mix and Normalize to it at batch positions.
 *   Pillow stretches its filter when it shrinks.  One axis n -> D, all in double on the host:
 *     scale = n / D, fs = max(scale, 1.0), support = 2.0 * fs, ss = 1.0 / fs; per output xx:
 *     center = (xx + 0.5) * scale, xmin = max((int)(center - support + 0.5), 0), ntaps = min((int)(center + support + 0.5), n) - xmin,
 *     w[i] = cubic((i + xmin - center + 0.5) * ss) with the cubic above (a = -0.5), ww = their sum in index order, w[i] /= ww unless ww == 0,
 *     k[i] = (int)(+-0.5 + w[i] * 2^22) with the sign of w[i].
 *   A pass is clip8((2^21 + SUM k[i] * px[xmin + i]) >> 22) in int32: the horizontal pass over the window (table of w) rounds to uint8, the
 *   vertical pass runs over those bytes (table of h).  Edges are the window's edges: no pixel outside the window enters the result.
 *   For n <= D this is qatvit_image_resize_coeffs' table (support 2, up to 4 taps) wherever that entry builds one; for n <= 4 D, support <= 8
 *   and ntaps <= 17.  Where center -+ support + 0.5 falls on an integer, the rounding of the doubles gives some outputs one tap more than
 *   ceil(2 * support) - five at n = 12 -> D = 44, which qatvit_image_resize_coeffs refuses.  That tap lies at the distance of the support,
 *   its coefficient is 0, and this builder keeps it (ntaps is Pillow's) after checking that it is 0: every admitted (n, D) is built.
 *   tables int32 [max_side][D * 19] on the device, 4-byte aligned: table n - 1 is xmin[D], ntaps[D], coef[D][17] of n -> D one after the other
 *   (coefficients past ntaps are 0), n = 1 .. max_side, as qatvit_image_window_coeffs(max_side, D, out_host) writes them on the HOST (no HIP
 *   call) into qatvit_image_window_coeffs_bytes(max_side, D) bytes (-1 + error string for a refused shape); max_side >= max(H, W).  The
 *   builder applies qatvit_image_resize_coeffs' checks: every coefficient fits 24 bits, no int32 accumulator overflows, and a band of 8
 *   output rows reads no more rows than the kernel keeps.
 *   D % 4 == 0, 8 <= D <= 384, 8 <= H, W <= 4 * D, 8 <= max_side <= 4 * D, 1 <= B <= 65535: anything else is refused with an error string
 *   before any HIP call, and so is a shape whose LDS request (the band's resampled rows and a staging buffer of source rows) exceeds 64 KB -
 *   none within these limits does.
 *   A malformed record is made safe, not trusted, as the rrc entries do it: h is clamped to [1, H] and w to [1, W], then top to [0, H - h]
 *   and left to [0, W - w]; any two words are safe, and the result is the clamped record's.
 *
 * qatvit_image_bytes_blur: the second stage behind qatvit_image_window_u8 WITH Gaussian blur, a launch that takes the resized bytes as they are.
 *   bytes uint8 [B][D][D][3] (HWC, contiguous, 4-byte aligned, on the device) at batch POSITIONS: no index, no N, no table of coefficients.
 *   out fp32 [B][3][D][D], 16-byte aligned.  mix, erase, color, sums and blur are qatvit_image_batch_blur's arguments with its records, its
 *   cleaning rules and its order (grayscale, solarize, BLUR, the jitter ops with the contrast sum taken behind the blur, Normalize, the erase,
 *   the mix; the partner of a mix record is coloured, blurred and erased by its own records): mix, erase, color and sums may be NULL
 *   (color == NULL: all-zero colour records; sums == NULL: the caller's promise that no record holds a contrast op); blur is REQUIRED -
 *   without blur records the second stage is qatvit_image_batch_color at S = D.  With color and sums a statistics launch runs in front, and
 *   on return sums[b] is what qatvit_image_batch_blur leaves there.
 *   out[b] is BITWISE what
 *     qatvit_image_batch_blur(bytes, NULL, B, B, D, D, qatvit_image_resize_coeffs(D, D), table, NULL, 0, 0, mix, erase, color, sums, blur, ..)
 *   defines: the resize D -> D is the identity, so the image that entry blurs is `bytes`.  That definition holds at the sizes at which that
 *   entry is refused for its LDS request as well (D = 224 among them: 89,536 bytes there): this entry is how those sizes are served.  A
 *   sample whose cleaned record is "no blur" gets bitwise qatvit_image_batch_color's result on the same bytes; nothing is addressed through a
 *   record.
 *   LDS: the value table (3072 bytes) and (sides + 1) image buffers of (band + 12) * 3 * D bytes, sides = 2 with mix records, else 1; the
 *   band is 16 rows without mix records where that stays within 64 KB (D <= 368), else 8 rows (D = 372 .. 384), and 8 rows with them.
 *   D = 224: 40,704 bytes, 43,392 with mix records; D = 384: 49,152 bytes.  With mix records D <= 344 is served (64,992 bytes); above, the
 *   request exceeds 64 KB and the call is refused with an error string that states the byte count, before any HIP call.
 *   D % 4 == 0, 8 <= D <= 384, 1 <= B <= 65535, bytes / table / blur / out not NULL: anything else is refused with an error string before
 *   any HIP call.
 */
int qatvit_image_resize_coeffs(int32_t src, int32_t dst, int32_t* xmin_host, int32_t* ntaps_host, int32_t* coef_host);
int qatvit_image_table(const float* mean_host, const float* std_host, float* table_host);
int qatvit_image_batch(const uint8_t* data, const int64_t* index, int32_t B, int32_t N, int32_t S, int32_t D, const int32_t* coeffs,
                       const float* table, float* out, void* stream);
int qatvit_image_batch_aug(const uint8_t* data, const int64_t* index, int32_t B, int32_t N, int32_t S, int32_t D, const int32_t* coeffs,
                           const float* table, const int32_t* aug, int32_t padding_mode, int32_t fill, float* out, void* stream);
int qatvit_image_batch_mix(const uint8_t* data, const int64_t* index, int32_t B, int32_t N, int32_t S, int32_t D, const int32_t* coeffs,
                           const float* table, const int32_t* aug, int32_t padding_mode, int32_t fill, const int32_t* mix, float* out,
                           void* stream);
int qatvit_image_resize_coeffs_windows(int32_t src, int32_t dst, int32_t* out_host);
int qatvit_image_batch_rrc(const uint8_t* data, const int64_t* index, int32_t B, int32_t N, int32_t S, int32_t D, const int32_t* windows,
                           const float* table, const int32_t* rrc, const int32_t* mix, float* out, void* stream);
int qatvit_image_batch_erase(const uint8_t* data, const int64_t* index, int32_t B, int32_t N, int32_t S, int32_t D, const int32_t* coeffs,
                             const float* table, const int32_t* aug, int32_t padding_mode, int32_t fill, const int32_t* mix,
                             const int32_t* erase, float* out, void* stream);
int qatvit_image_batch_rrc_erase(const uint8_t* data, const int64_t* index, int32_t B, int32_t N, int32_t S, int32_t D, const int32_t* windows,
                                 const float* table, const int32_t* rrc, const int32_t* mix, const int32_t* erase, float* out, void* stream);
int qatvit_image_batch_color(const uint8_t* data, const int64_t* index, int32_t B, int32_t N, int32_t S, int32_t D, const int32_t* coeffs,
                             const float* table, const int32_t* aug, int32_t padding_mode, int32_t fill, const int32_t* mix,
                             const int32_t* erase, const int32_t* color, uint32_t* sums, float* out, void* stream);
int qatvit_image_batch_rrc_color(const uint8_t* data, const int64_t* index, int32_t B, int32_t N, int32_t S, int32_t D, const int32_t* windows,
                                 const float* table, const int32_t* rrc, const int32_t* mix, const int32_t* erase, const int32_t* color,
                                 uint32_t* sums, float* out, void* stream);
int qatvit_image_batch_blur(const uint8_t* data, const int64_t* index, int32_t B, int32_t N, int32_t S, int32_t D, const int32_t* coeffs,
                            const float* table, const int32_t* aug, int32_t padding_mode, int32_t fill, const int32_t* mix,
                            const int32_t* erase, const int32_t* color, uint32_t* sums, const int32_t* blur, float* out, void* stream);
int qatvit_image_batch_rrc_blur(const uint8_t* data, const int64_t* index, int32_t B, int32_t N, int32_t S, int32_t D, const int32_t* windows,
                                const float* table, const int32_t* rrc, const int32_t* mix, const int32_t* erase, const int32_t* color,
                                uint32_t* sums, const int32_t* blur, float* out, void* stream);
int64_t qatvit_image_window_coeffs_bytes(int32_t max_side, int32_t D);
int qatvit_image_window_coeffs(int32_t max_side, int32_t D, int32_t* out_host);
int qatvit_image_window_u8(const uint8_t* data, const int64_t* index, int32_t B, int32_t N, int32_t H, int32_t W, int32_t D,
                           const int32_t* tables, int32_t max_side, const int32_t* rrc, uint8_t* out, void* stream);
int qatvit_image_bytes_blur(const uint8_t* bytes, int32_t B, int32_t D, const float* table, const int32_t* mix, const int32_t* erase,
                            const int32_t* color, uint32_t* sums, const int32_t* blur, float* out, void* stream);

/* ---------------------------------------------------------------------------
 * Validation counts on the device: one launch per batch of logits, one device-to-host copy per evaluation.
 * Replaces: evaluate_fp32 (qat_trainer.py:49-61: argmax, ==, .sum().item() per batch), _eval_acc_limited of the Optuna objective,
 *   evaluate_model (evaluator.py) and the accuracy the comparator reports per checkpoint.
 *
 * logits [B, C] of `dtype` (QATVIT_EVAL_F32 / _F16 / _BF16), row stride `ld` >= C in elements (elements past C in a row are never read);
 * labels int64 [B].  Per row:
 *   pred = torch.argmax's answer: the index of the first NaN if the row has one, otherwise of the first maximum (+0 == -0); compared on the
 *     stored values (widening fp16 / bf16 to fp32 is exact and monotone).
 *   A label outside [0, C) is counted in bad_labels and takes no part in correct, the loss, the matrix or other_correct; nothing is read or
 *     written through it.
 *   CE = logsumexp(row) - row[label] in fp32, max-subtracted (no smoothing): finite -> added to loss_sum and counted in loss_rows,
 *     otherwise counted in nonfinite_rows.
 *   confusion (int64 [C, C], or NULL): confusion[label * C + pred] += 1.
 *   other (fp32, row stride other_ld >= C, or NULL): a second model's logits for the same samples - row b of [B, C] when other_index is NULL,
 *     else row other_index[b] of a per-sample table [other_rows, C] (the layout of a teacher logit table).  An index outside [0, other_rows)
 *     is counted in bad_index and reads nothing; every other row counts in other_rows_seen, in agree when the two argmaxes are equal (labels
 *     play no part in that) and in other_correct when the label is valid and other's argmax equals it.
 * state: QATVIT_EVAL_STATE_WORDS 8-byte words, 8-byte aligned, that the caller zeroes once per evaluation and every call ADDS to:
 *   int64 [0] total [1] correct [2] bad_labels [3] nonfinite_rows [4] other_rows_seen [5] agree [6] other_correct [7] bad_index [8] loss_rows,
 *   double [9] loss_sum.  The integer counts are exact and do not depend on launch or block order; loss_sum is accumulated in double in arrival
 *   order, so its last bits can differ between runs.  Nothing synchronises with the host.  1 <= B < 2^30, 2 <= C < 2^30.
 */
#define QATVIT_EVAL_F32 0
#define QATVIT_EVAL_F16 1
#define QATVIT_EVAL_BF16 2
#define QATVIT_EVAL_STATE_WORDS 10
int qatvit_eval_accumulate(const void* logits, int32_t dtype, int64_t ld, const int64_t* labels, int64_t batch, int64_t classes,
                           const float* other, int64_t other_ld, const int64_t* other_index, int64_t other_rows, void* state,
                           int64_t* confusion, void* stream);

/* Measurement hooks (bench.py): bracket every launch of one GEMM class inside the steps of ONE engine - identified by its workspace
 * pointer, so engines in the same process do not see each other's sessions - with HIP events on the launch stream.
 * kind: 1 = NT with split (hi+lo) A operand and the plain epilogue (proj / fc2 forward, proj dgrad), 2 = NT with grid A operand on int8 MFMA, plain
 * epilogue (patch embedding; qkv when it runs once), 7 = its statistics-only passes (qkv, fc1), 8 = the fc1 storing pass, 9 = the qkv code pass, 3 = TN (wgrad) with grid X operand (qkv / fc1 / patch-embed; the bracket holds k_gemm_tn + k_tn_reduce), 6 = TN with split X operand (proj / fc2), 4 = NT split-A dgrad with the LayerNorm backward fused into its epilogue (fc1 / qkv dgrad), 5 = fc2 dgrad with
 * the GELU backward fused into its epilogue.
 * stop() synchronises on the recorded events and returns the summed kernel time, launch count and the summed
 * algorithmic FLOPs (2*M*N*K per launch, one pass). */
int qatvit_profile_start(const void* workspace, int32_t kind, int32_t max_launches);
int qatvit_profile_stop(const void* workspace, double* total_ms, int64_t* launches, double* flops);
/* byte offset of a named intermediate tensor inside the workspace (tests); -1 if unknown */
int64_t qatvit_student_tensor_offset(const qatvit_cfg* cfg, const char* name, int32_t block);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* QATVIT_H */
