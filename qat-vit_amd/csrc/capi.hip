// extern "C" surface of libqatvit.so: argument validation + error strings around the
// launchers.  Declarations and the reference call sites they replace: include/qatvit.h.
#include <stdarg.h>
#include <stdlib.h>
#include <string.h>

#include <mutex>
#include <unordered_map>

#include "../../include/qatvit.h"
#include "qv_common.h"
#include "qv_kernels.h"

namespace qv {
static thread_local char g_err[512] = "";
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

static bool knob(const char* name) {
    const char* v = getenv(name);
    return !v || atoi(v) != 0;
}
const Knobs& knobs() {
    static const Knobs k{knob("QATVIT_I8"), knob("QATVIT_F16"), knob("QATVIT_FC2_CODES"), knob("QATVIT_FC1_BITS"), knob("QATVIT_FC2W_CODES"),
                         knob("QATVIT_WBATCH"), knob("QATVIT_ATTN_CODES"), knob("QATVIT_QKV_2PASS"), knob("QATVIT_LNB_FUSE"), knob("QATVIT_QP_LATE"),
                         knob("QATVIT_TN_STREAM"), knob("QATVIT_TN_Q8"), knob("QATVIT_ATTN_BWD_FUSED"), knob("QATVIT_F16_STRIP"), knob("QATVIT_I8_STRIP"), knob("QATVIT_LN_STRIP"),
                         knob("QATVIT_CLS_BWD"), knob("QATVIT_ATTN_BWD_PIPE")};
    return k;
}
int cu_count() {
    static const int cus = [] {
        int dev = 0, n = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 1 || n > 256) n = 256;
        return n;
    }();
    return cus;
}

// The drop-path scale table bound to a step workspace (qatvit_student_set_drop_path / qatvit_float_student_set_drop_path): host state keyed by the workspace
// address, read by every forward / backward entry on that workspace - a backward runs on autograd's worker thread, hence the lock.  The init entries of both
// workspaces unbind (an address that is bound anew must not inherit a table).
static std::mutex g_drop_mu;
static std::unordered_map<const void*, const float*> g_drop;
void drop_path_bind(const void* workspace, const float* table) {
    std::lock_guard<std::mutex> lk(g_drop_mu);
    if (table) g_drop[workspace] = table;
    else g_drop.erase(workspace);
}
const float* drop_path_of(const void* workspace) {
    std::lock_guard<std::mutex> lk(g_drop_mu);
    auto it = g_drop.find(workspace);
    return it == g_drop.end() ? nullptr : it->second;
}
// The LayerScale binding of a step workspace (qatvit_student_set_layer_scale / qatvit_float_student_set_layer_scale): as the drop-path table, host state keyed by
// the workspace address under the same lock; the pointer lists are copied, a call holds its own reference while it runs
static std::unordered_map<const void*, std::shared_ptr<const LayerScale>> g_ls;
void layer_scale_bind(const void* workspace, int branches, const float* const* gammas, float* const* grads, void* saved) {
    std::shared_ptr<LayerScale> b;
    if (gammas) {
        b = std::make_shared<LayerScale>();
        b->gamma.assign(gammas, gammas + branches);
        if (grads) b->grad.assign(grads, grads + branches);
        b->saved = reinterpret_cast<float*>(saved);
    }
    std::lock_guard<std::mutex> lk(g_drop_mu);
    if (b) g_ls[workspace] = b;
    else g_ls.erase(workspace);
}
std::shared_ptr<const LayerScale> layer_scale_of(const void* workspace) {
    std::lock_guard<std::mutex> lk(g_drop_mu);
    auto it = g_ls.find(workspace);
    return it == g_ls.end() ? nullptr : it->second;
}
static int layer_scale_set(const char* fn, const qatvit_cfg* cfg, void* workspace, const float* const* gammas, float* const* grads, void* saved, bool need_saved) {
    if (!cfg || !workspace) { set_error("%s: null argument", fn); return 1; }
    if (gammas) {
        if (cfg->depth < 1 || cfg->embed_dim % 4 != 0) { set_error("%s: depth %d, embed_dim %d", fn, cfg->depth, cfg->embed_dim); return 1; }
        for (int k = 0; k < 2 * cfg->depth; ++k)
            if (!gammas[k] || (grads && !grads[k])) { set_error("%s: branch %d has a null gamma or gradient", fn, k); return 1; }
        if (need_saved && grads && !saved) { set_error("%s: a binding with gradients needs the saved-branch buffer (qatvit_float_student_layer_scale_bytes)", fn); return 1; }
    }
    layer_scale_bind(workspace, gammas ? 2 * cfg->depth : 0, gammas, grads, saved);
    return 0;
}
}  // namespace qv

using namespace qv;

extern "C" {

int qatvit_abi_version(void) { return QATVIT_ABI_VERSION; }

int qatvit_student_set_drop_path(const qatvit_cfg* cfg, void* workspace, const float* scale_table) {
    QV_CHECK_ARG(cfg && workspace, "qatvit_student_set_drop_path: null argument");
    drop_path_bind(workspace, scale_table);
    return 0;
}
int qatvit_float_student_set_drop_path(const qatvit_cfg* cfg, void* workspace, const float* scale_table) {
    QV_CHECK_ARG(cfg && workspace, "qatvit_float_student_set_drop_path: null argument");
    drop_path_bind(workspace, scale_table);
    return 0;
}
int qatvit_student_set_layer_scale(const qatvit_cfg* cfg, void* workspace, const float* const* gammas, float* const* grads) {
    return layer_scale_set("qatvit_student_set_layer_scale", cfg, workspace, gammas, grads, nullptr, false);
}
int qatvit_float_student_set_layer_scale(const qatvit_cfg* cfg, void* workspace, const float* const* gammas, float* const* grads, void* saved) {
    return layer_scale_set("qatvit_float_student_set_layer_scale", cfg, workspace, gammas, grads, saved, true);
}
int64_t qatvit_float_student_layer_scale_bytes(const qatvit_cfg* cfg) {
    if (!cfg || cfg->depth < 1 || cfg->batch < 1) return -1;
    const int64_t np = (int64_t)(cfg->img_size / cfg->patch_size) * (cfg->img_size / cfg->patch_size);
    // fp32 [2 * depth][batch * tokens, embed_dim], then [2 * depth] {K, 1 / K}: the fp16 form's per-branch gradient scales (float_step.hip)
    return 2 * (int64_t)cfg->depth * cfg->batch * (np + 1) * cfg->embed_dim * 4 + 256;
}
const char* qatvit_last_error(void) { return qv::g_err; }
const char* qatvit_target_arch(void) { return "gfx950"; }

int64_t qatvit_fq_workspace_bytes(int64_t channels) {
    if (channels < 1) channels = 1;
    return channels * (2 * (int64_t)sizeof(uint32_t) + 4 * (int64_t)sizeof(float));
}

int qatvit_fq_forward(const float* x, float* y, uint8_t* mask_bits, float* running_min, float* running_max, float* scale,
                      int32_t* zero_point, const int64_t* observer_on, const int64_t* fake_quant_on, float averaging_const,
                      int32_t qmin, int32_t qmax, int64_t channels, int64_t inner, int32_t per_channel, int32_t symmetric,
                      void* workspace, void* stream) {
    QV_CHECK_ARG(x && y && running_min && running_max && scale && zero_point && observer_on && fake_quant_on && workspace,
                 "qatvit_fq_forward: null pointer argument");
    QV_CHECK_ARG(channels >= 1 && inner >= 1, "qatvit_fq_forward: empty tensor (channels=%lld inner=%lld)", (long long)channels,
                 (long long)inner);
    QV_CHECK_ARG(qmin < qmax, "qatvit_fq_forward: qmin (%d) must be < qmax (%d)", qmin, qmax);
    QV_CHECK_ARG(per_channel || channels == 1, "qatvit_fq_forward: per-tensor call must pass channels == 1");
    launch_fq_forward(x, y, mask_bits, running_min, running_max, scale, zero_point, observer_on, fake_quant_on, averaging_const, qmin,
                      qmax, channels, inner, per_channel != 0, symmetric != 0, workspace, (hipStream_t)stream);
    QV_CHECK_LAUNCH("qatvit_fq_forward");
    return 0;
}

int qatvit_fq_backward(const float* dy, const uint8_t* mask_bits, float* dx, int64_t n, void* stream) {
    QV_CHECK_ARG(dy && mask_bits && dx, "qatvit_fq_backward: null pointer argument");
    QV_CHECK_ARG(n >= 1, "qatvit_fq_backward: empty tensor");
    launch_fq_backward(dy, mask_bits, dx, n, (hipStream_t)stream);
    QV_CHECK_LAUNCH("qatvit_fq_backward");
    return 0;
}

int qatvit_ln_forward(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd, int64_t rows,
                      int64_t dim, float eps, void* stream) {
    QV_CHECK_ARG(x && gamma && beta && y && mean && rstd, "qatvit_ln_forward: null pointer argument");
    QV_CHECK_ARG(rows >= 1 && dim >= 1, "qatvit_ln_forward: empty tensor");
    launch_ln_forward(x, gamma, beta, y, mean, rstd, rows, dim, eps, (hipStream_t)stream);
    QV_CHECK_LAUNCH("qatvit_ln_forward");
    return 0;
}

int qatvit_ln_backward(const float* dy, const float* x, const float* gamma, const float* mean, const float* rstd, float* dx,
                       float* dgamma, float* dbeta, int64_t rows, int64_t dim, void* stream) {
    QV_CHECK_ARG(dy && x && gamma && mean && rstd && dx && dgamma && dbeta, "qatvit_ln_backward: null pointer argument");
    QV_CHECK_ARG(rows >= 1 && dim >= 1, "qatvit_ln_backward: empty tensor");
    launch_ln_backward(dy, x, gamma, mean, rstd, dx, dgamma, dbeta, rows, dim, (hipStream_t)stream);
    QV_CHECK_LAUNCH("qatvit_ln_backward");
    return 0;
}

int qatvit_kd_ce_loss(const float* student, const float* teacher, const int64_t* labels, int64_t batch, int64_t classes,
                      float kd_temp, float kd_alpha, float label_smoothing, float* out3, float* dlogits, void* stream) {
    QV_CHECK_ARG(student && labels && out3 && dlogits, "qatvit_kd_ce_loss: null pointer argument");
    QV_CHECK_ARG(batch >= 1 && classes >= 2 && classes <= 4096, "qatvit_kd_ce_loss: bad shape B=%lld C=%lld", (long long)batch,
                 (long long)classes);
    QV_CHECK_ARG(kd_temp > 0.f, "qatvit_kd_ce_loss: kd_temp must be > 0");
    launch_kd_ce_loss(student, teacher, labels, batch, classes, kd_temp, kd_alpha, label_smoothing, out3, dlogits, (hipStream_t)stream);
    QV_CHECK_LAUNCH("qatvit_kd_ce_loss");
    return 0;
}

int qatvit_kd_ce_loss_table(const float* student, const float* table, int64_t table_rows, const int64_t* index, const int64_t* labels,
                            int64_t batch, int64_t classes, float kd_temp, float kd_alpha, float label_smoothing, float* out3, float* dlogits,
                            void* stream) {
    QV_CHECK_ARG(student && table && index && labels && out3 && dlogits, "qatvit_kd_ce_loss_table: null pointer argument");
    QV_CHECK_ARG(batch >= 1 && classes >= 2 && classes <= 4096, "qatvit_kd_ce_loss_table: bad shape B=%lld C=%lld", (long long)batch,
                 (long long)classes);
    QV_CHECK_ARG(table_rows >= 1, "qatvit_kd_ce_loss_table: table_rows %lld (at least 1)", (long long)table_rows);
    QV_CHECK_ARG(kd_temp > 0.f, "qatvit_kd_ce_loss_table: kd_temp must be > 0");
    launch_kd_ce_loss_table(student, table, table_rows, index, labels, batch, classes, kd_temp, kd_alpha, label_smoothing, out3, dlogits,
                            (hipStream_t)stream);
    QV_CHECK_LAUNCH("qatvit_kd_ce_loss_table");
    return 0;
}

int qatvit_kd_ce_loss_mix(const float* student, const float* teacher, const float* table, int64_t table_rows, const int64_t* index,
                          const int64_t* labels, const int32_t* mix, int64_t batch, int64_t classes, float kd_temp, float kd_alpha,
                          float label_smoothing, float* out3, float* dlogits, void* stream) {
    QV_CHECK_ARG(student && labels && out3 && dlogits, "qatvit_kd_ce_loss_mix: null pointer argument");
    QV_CHECK_ARG(!(teacher && table), "qatvit_kd_ce_loss_mix: a teacher tensor and a teacher table are mutually exclusive");
    QV_CHECK_ARG(!table || index, "qatvit_kd_ce_loss_mix: a teacher table needs an index");
    QV_CHECK_ARG(batch >= 1 && classes >= 2 && classes <= 4096, "qatvit_kd_ce_loss_mix: bad shape B=%lld C=%lld", (long long)batch,
                 (long long)classes);
    QV_CHECK_ARG(!table || table_rows >= 1, "qatvit_kd_ce_loss_mix: table_rows %lld (at least 1)", (long long)table_rows);
    QV_CHECK_ARG(kd_temp > 0.f, "qatvit_kd_ce_loss_mix: kd_temp must be > 0");
    QV_CHECK_ARG(((uintptr_t)mix & 3) == 0, "qatvit_kd_ce_loss_mix: misaligned mix pointer");
    launch_kd_ce_loss_mix(student, teacher, table, table_rows, index, labels, mix, batch, classes, kd_temp, kd_alpha, label_smoothing, out3, dlogits,
                          (hipStream_t)stream);
    QV_CHECK_LAUNCH("qatvit_kd_ce_loss_mix");
    return 0;
}

int qatvit_kd_bce_loss(const float* student, const float* teacher, const float* table, int64_t table_rows, const int64_t* index,
                       const int64_t* labels, const int32_t* mix, int64_t batch, int64_t classes, float kd_temp, float kd_alpha,
                       float label_smoothing, float target_threshold, int32_t sum_classes, float* partials, float* out3, float* dlogits,
                       void* stream) {
    QV_CHECK_ARG(student && labels && partials && out3 && dlogits, "qatvit_kd_bce_loss: null pointer argument");
    QV_CHECK_ARG(!(teacher && table), "qatvit_kd_bce_loss: a teacher tensor and a teacher table are mutually exclusive");
    QV_CHECK_ARG(!table || index, "qatvit_kd_bce_loss: a teacher table needs an index");
    QV_CHECK_ARG(batch >= 1 && batch <= INT32_MAX / 2 && classes >= 2 && classes <= 4096, "qatvit_kd_bce_loss: bad shape B=%lld C=%lld",
                 (long long)batch, (long long)classes);
    QV_CHECK_ARG(!table || table_rows >= 1, "qatvit_kd_bce_loss: table_rows %lld (at least 1)", (long long)table_rows);
    QV_CHECK_ARG(kd_temp > 0.f, "qatvit_kd_bce_loss: kd_temp must be > 0");
    QV_CHECK_ARG(label_smoothing >= 0.f && label_smoothing < 1.f, "qatvit_kd_bce_loss: label_smoothing %g is outside [0, 1)", (double)label_smoothing);
    QV_CHECK_ARG(((uintptr_t)mix & 3) == 0, "qatvit_kd_bce_loss: misaligned mix pointer");
    launch_kd_bce_loss(student, teacher, table, table_rows, index, labels, mix, batch, classes, kd_temp, kd_alpha, label_smoothing, target_threshold,
                       sum_classes != 0, partials, out3, dlogits, (hipStream_t)stream);
    QV_CHECK_LAUNCH("qatvit_kd_bce_loss");
    return 0;
}

// The NT GEMMs: a wrapper checks its own pointers, writes its parameters into an NTGemm and names the operand form; launch_gemm_nt checks the request itself
// (gemm.hip nt_request_ok).  QV_NT_REQUEST: the parameters the entry points share, by name (B and ldb: where there are any)
#define QV_NT_REQUEST(g, a, a_ld, c_ld)                                                                                                         \
    NTGemm g;                                                                                                                                   \
    g.A = a; g.M = M; g.N = N; g.K = K; g.lda = a_ld; g.ldc = c_ld; g.s2 = s2; g.col_scale = col_scale; g.bias = bias; g.stats = stats

int qatvit_gemm_nt(const void* A_hi, const void* A_lo, const void* B, float* C, int32_t M, int32_t N, int32_t K, int32_t lda, int32_t ldb,
                   int32_t ldc, const float* s1, const float* s2, const float* col_scale, const float* bias, uint32_t* stats, void* stream) {
    QV_CHECK_ARG(A_hi && B && C, "qatvit_gemm_nt: null pointer argument");
    QV_NT_REQUEST(g, A_hi, lda, ldc);
    g.A_lo = A_lo; g.B = B; g.ldb = ldb; g.C = C; g.s1 = s1;
    if (launch_gemm_nt(kNTBf16, g, nullptr, (hipStream_t)stream)) return 1;
    QV_CHECK_LAUNCH("qatvit_gemm_nt");
    return 0;
}

int qatvit_gemm_nt_f16(const void* A16_hi, const void* A16_lo, const void* B16, float* C, int32_t M, int32_t N, int32_t K, int32_t lda, int32_t ldb,
                       int32_t ldc, const float* s1, const float* s2, const float* col_scale, const float* bias, uint32_t* stats, void* stream) {
    QV_CHECK_ARG(A16_hi && A16_lo && B16 && C, "qatvit_gemm_nt_f16: null pointer argument");
    QV_NT_REQUEST(g, A16_hi, lda, ldc);
    g.A_lo = A16_lo; g.B = B16; g.ldb = ldb; g.C = C; g.s1 = s1;
    if (launch_gemm_nt(kNTF16, g, nullptr, (hipStream_t)stream)) return 1;
    QV_CHECK_LAUNCH("qatvit_gemm_nt_f16");
    return 0;
}

int qatvit_gemm_nt_i8_minmax(const void* A8, const void* B8, const int32_t* wsum, const float* a_qp, int32_t center, int32_t M, int32_t N, int32_t K,
                             int32_t lda, int32_t ldb, const float* s1, const float* s2, const float* col_scale, const float* bias, uint32_t* stats,
                             void* stream) {
    QV_CHECK_ARG(A8 && B8 && wsum && a_qp && stats, "qatvit_gemm_nt_i8_minmax: null pointer argument");
    NTPost post{};
    post.mode = kEpiStats;
    QV_NT_REQUEST(g, A8, lda, N);
    g.wsum = wsum; g.a_qp = a_qp; g.center = center; g.s1 = s1; g.B = B8; g.ldb = ldb;
    if (launch_gemm_nt(kNTI8, g, &post, (hipStream_t)stream)) return 1;
    QV_CHECK_LAUNCH("qatvit_gemm_nt_i8_minmax");
    return 0;
}

int qatvit_w8_fragment_order(const void* B8, void* B8f, int32_t N, int32_t K, void* stream) {
    if (launch_w8_fragment_order(B8, B8f, N, K, (hipStream_t)stream)) return 1;
    QV_CHECK_LAUNCH("qatvit_w8_fragment_order");
    return 0;
}

int qatvit_i8_strip(int32_t mode, const void* A8, const void* B8f, const int32_t* wsum, const float* a_qp, int32_t center, int32_t M, int32_t N, int32_t K,
                    int32_t lda, const float* s1, const float* s2, const float* col_scale, const float* bias, uint32_t* stats, const float* out_qp,
                    int32_t qmin, int32_t qmax, void* out8, void* out8_mask, int32_t code_T, uint32_t* lut_out, uint32_t* lutq_out,
                    float* out16_scale, void* stream) {
    QV_CHECK_ARG(A8 && B8f && wsum && a_qp && s1, "qatvit_i8_strip: null pointer argument");
    QV_CHECK_ARG(mode == kEpiStats || mode == kEpiCodes || mode == kEpiQkvCodes, "qatvit_i8_strip: mode %d (3 = statistics, 7 = qkv codes, 4 = fc1 codes)", mode);
    NTPost post{};
    post.mode = mode;
    post.qp = out_qp; post.qmin = qmin; post.qmax = qmax; post.out8 = out8; post.out8_mask = out8_mask; post.code_T = code_T; post.code_hd = 64;
    post.lut_out = lut_out; post.lutq_out = lutq_out; post.out16_scale = out16_scale;
    QV_NT_REQUEST(g, A8, lda, N);
    g.wsum = wsum; g.a_qp = a_qp; g.center = center; g.s1 = s1; g.B_frag = B8f;
    if (!launch_i8_strip(g, &post, (hipStream_t)stream, true)) {
        set_error("qatvit_i8_strip: unsupported arguments (mode %d M=%d N=%d K=%d lda=%d: need K = 384 with N %% 1152 == 0 or N %% 1536 == 0, or K = 768 with "
                  "N = 2304 or 3072; lda %% 16 == 0, M < 2^22, the mode's output pointers, qmax - qmin < 256; mode 7: (N / 3) %% 384 == 0, 0 < code_T < 1024)",
                  mode, M, N, K, lda);
        return 1;
    }
    QV_CHECK_LAUNCH("qatvit_i8_strip");
    return 0;
}

int qatvit_ln_apply_quant8(const float* x, const float* mean, const float* rstd, const float* gamma, const float* beta, const float* qp, int32_t qmin, int32_t qmax,
                           void* out8, int32_t center, int64_t M, int32_t D, void* stream) {
    QV_CHECK_ARG(x && mean && rstd && gamma && beta && qp && out8, "qatvit_ln_apply_quant8: null pointer argument");
    QV_CHECK_ARG(M >= 1 && D >= 4 && D % 4 == 0, "qatvit_ln_apply_quant8: M=%lld D=%d (D %% 4 == 0)", (long long)M, D);
    if (launch_ln_apply_quant(x, mean, rstd, gamma, beta, qp, qmin, qmax, nullptr, M, D, (hipStream_t)stream, out8, center)) return 1;
    QV_CHECK_LAUNCH("qatvit_ln_apply_quant8");
    return 0;
}

int qatvit_i8_strip_ln(const float* x, const float* mean, const float* rstd, const float* gamma, const float* beta, int32_t ln_qmin, int32_t ln_qmax, void* out8,
                       const void* B8f, const int32_t* wsum, const float* a_qp, int32_t center, int32_t M, int32_t N, int32_t K, int32_t lda, const float* s2,
                       const float* col_scale, const float* bias, uint32_t* stats, void* stream) {
    QV_CHECK_ARG(x && mean && rstd && gamma && beta && out8 && B8f && wsum && a_qp && stats, "qatvit_i8_strip_ln: null pointer argument");
    QV_NT_REQUEST(g, out8, lda, N);
    g.wsum = wsum; g.a_qp = a_qp; g.center = center; g.B_frag = B8f;
    const StripLn ln{x, mean, rstd, gamma, beta, ln_qmin, ln_qmax, out8};
    if (!launch_i8_strip_ln(g, ln, (hipStream_t)stream, true)) {
        set_error("qatvit_i8_strip_ln: unsupported arguments (M=%d N=%d K=%d lda=%d: need K = 384 with N = 1152 or 1536, or K = 768 with N = 2304 or 3072; "
                  "lda %% 16 == 0, lda >= K, 0 < M < 2^22)", M, N, K, lda);
        return 1;
    }
    QV_CHECK_LAUNCH("qatvit_i8_strip_ln");
    return 0;
}

int qatvit_gemm_nt_codes(const void* A8, const uint32_t* lut, const void* B16, float* C, int32_t M, int32_t N, int32_t K, int32_t lda, int32_t ldb,
                         int32_t ldc, const float* s1, const float* s2, const float* col_scale, const float* bias, uint32_t* stats, void* stream) {
    QV_CHECK_ARG(A8 && lut && B16 && C, "qatvit_gemm_nt_codes: null pointer argument");
    QV_NT_REQUEST(g, A8, lda, ldc);
    g.lut = lut; g.B = B16; g.ldb = ldb; g.C = C; g.s1 = s1;
    if (launch_gemm_nt(kNTCodes, g, nullptr, (hipStream_t)stream)) return 1;
    QV_CHECK_LAUNCH("qatvit_gemm_nt_codes");
    return 0;
}

// the residual epilogue of one GEMM on its own: the request as it comes, checked by launch_gemm_nt alone (a form that has no residual epilogue, a shape, a null
// resid / C / out_qp / operand: its refusals, its texts)
int qatvit_gemm_nt_resid_fq(int32_t form, const void* A, const void* A_lo_or_lut, const void* B16, const float* resid, float* C, int32_t M, int32_t N, int32_t K,
                            int32_t lda, int32_t ldb, int32_t ldc, const float* s1, const float* s2, const float* col_scale, const float* bias,
                            const float* out_qp, int32_t qmin, int32_t qmax, const float* ls_gamma, void* stream) {
    uint32_t* const stats = nullptr;   // (the residual epilogue feeds no observer)
    QV_NT_REQUEST(g, A, lda, ldc);
    if (form == kNTCodes) g.lut = reinterpret_cast<const uint32_t*>(A_lo_or_lut); else g.A_lo = A_lo_or_lut;
    g.B = B16; g.ldb = ldb; g.C = C; g.s1 = s1;
    NTPost post{};
    post.mode = ls_gamma ? kEpiResidFqLs : kEpiResidFq; post.qp = out_qp; post.qmin = qmin; post.qmax = qmax; post.resid = resid; post.ls_gamma = ls_gamma;
    if (launch_gemm_nt((NTForm)form, g, &post, (hipStream_t)stream)) return 1;
    QV_CHECK_LAUNCH("qatvit_gemm_nt_resid_fq");
    return 0;
}

int qatvit_gemm_nt_i8(const void* A8, const void* B8, const int32_t* wsum, const float* a_qp, int32_t center, float* C, int32_t M, int32_t N,
                      int32_t K, int32_t lda, int32_t ldb, int32_t ldc, const float* s1, const float* s2, const float* col_scale, const float* bias,
                      uint32_t* stats, void* stream) {
    QV_CHECK_ARG(A8 && B8 && wsum && a_qp && C, "qatvit_gemm_nt_i8: null pointer argument");
    QV_NT_REQUEST(g, A8, lda, ldc);
    g.wsum = wsum; g.a_qp = a_qp; g.center = center; g.s1 = s1; g.B = B8; g.ldb = ldb; g.C = C;
    if (launch_gemm_nt(kNTI8, g, nullptr, (hipStream_t)stream)) return 1;
    QV_CHECK_LAUNCH("qatvit_gemm_nt_i8");
    return 0;
}

// The weight gradients: a wrapper checks its own pointers, writes its parameters into a TNGemm + TNCall and names the operand form; launch_gemm_tn checks the
// request itself (gemm.hip tn_request_ok).  QV_TN_REQUEST: the parameters all five entry points share, by name
#define QV_TN_REQUEST(g, c)                                                                                                                                  \
    TNGemm g;                                                                                                                                                \
    g.C = C; g.N = N; g.Kw = Kw; g.ldp = ldp; g.ldq = ldq; g.ldc = ldc; g.W = W; g.w_scale = w_scale; g.w_zp = w_zp; g.dbias = dbias; g.row_div = row_div;  \
    TNCall c;                                                                                                                                                \
    c.M = M; c.w_per_channel = w_per_channel; c.w_qmin = w_qmin; c.w_qmax = w_qmax; c.scratch = scratch; c.scratch_bytes = scratch_bytes

int qatvit_gemm_tn(const void* P_hi, const void* P_lo, const void* Q_hi, const void* Q_lo, float* C, int32_t M, int32_t N, int32_t Kw, int32_t ldp,
                   int32_t ldq, int32_t ldc, const float* s1, const float* W, const float* w_scale, const int32_t* w_zp, int32_t w_per_channel,
                   int32_t w_qmin, int32_t w_qmax, float* dbias, const float* row_div, float* scratch, int64_t scratch_bytes, void* stream) {
    QV_CHECK_ARG(P_hi && P_lo && Q_hi && C, "qatvit_gemm_tn: null pointer argument");
    QV_TN_REQUEST(g, c);
    g.P = P_hi; g.P_lo = P_lo; g.Q = Q_hi; g.Q_lo = Q_lo; g.s1 = s1;
    if (launch_gemm_tn(kTNPair, g, c, (hipStream_t)stream)) return 1;
    QV_CHECK_LAUNCH("qatvit_gemm_tn");
    return 0;
}

int qatvit_gemm_nt_dy16(const void* A16, const void* B16, float* C, int32_t M, int32_t N, int32_t K, int32_t lda, int32_t ldb, int32_t ldc, const float* s1,
                        const float* s2, void* stream) {
    QV_CHECK_ARG(A16 && B16 && C, "qatvit_gemm_nt_dy16: null pointer argument");
    NTGemm g;
    g.A = A16; g.B = B16; g.C = C; g.M = M; g.N = N; g.K = K; g.lda = lda; g.ldb = ldb; g.ldc = ldc; g.s1 = s1; g.s2 = s2;
    if (launch_gemm_nt(kNTPlaneF16, g, nullptr, (hipStream_t)stream)) return 1;
    QV_CHECK_LAUNCH("qatvit_gemm_nt_dy16");
    return 0;
}

int qatvit_gemm_tn_dy16(const void* P16, const void* Q_hi, const void* Q_lo, const void* Qc, const uint32_t* lutQ16, float* C, int32_t M, int32_t N, int32_t Kw,
                        int32_t ldp, int32_t ldq, int32_t ldc, const float* s1, const float* s2, const float* W, const float* w_scale, const int32_t* w_zp,
                        int32_t w_per_channel, int32_t w_qmin, int32_t w_qmax, float* dbias, const float* row_div, float* scratch, int64_t scratch_bytes,
                        void* stream) {
    QV_CHECK_ARG(P16 && C && ((Q_hi && !Qc) || (Qc && lutQ16 && !Q_hi && !Q_lo)), "qatvit_gemm_tn_dy16: Q is either planes (Q_hi, optional Q_lo) or codes + table");
    QV_TN_REQUEST(g, c);
    g.P = P16; g.Q = Qc ? Qc : Q_hi; g.Q_lo = Q_lo; g.lut = lutQ16; g.s1 = s1; g.s2 = s2;
    if (launch_gemm_tn(Qc ? kTNPlaneCodes : kTNPlaneF16, g, c, (hipStream_t)stream)) return 1;
    QV_CHECK_LAUNCH("qatvit_gemm_tn_dy16");
    return 0;
}

int qatvit_gemm_tn_q8_dy16(const void* P16, const void* Q8, const float* a_qp, int32_t center, float* C, int32_t M, int32_t N, int32_t Kw, int32_t ldp, int32_t ldq,
                           int32_t ldc, const float* s2, const float* W, const float* w_scale, const int32_t* w_zp, int32_t w_per_channel, int32_t w_qmin,
                           int32_t w_qmax, float* dbias, const float* row_div, float* scratch, int64_t scratch_bytes, void* stream) {
    QV_CHECK_ARG(P16 && Q8 && a_qp && C, "qatvit_gemm_tn_q8_dy16: null pointer argument");
    QV_TN_REQUEST(g, c);
    g.P = P16; g.Q = Q8; g.s1 = a_qp; g.s2 = s2; c.center = center;
    if (launch_gemm_tn(kTNPlaneQ8, g, c, (hipStream_t)stream)) return 1;
    QV_CHECK_LAUNCH("qatvit_gemm_tn_q8_dy16");
    return 0;
}

int64_t qatvit_gemm_tn_stream_scratch_bytes(void) { return tn_stream_scratch_bytes(); }
int qatvit_gemm_tn_stream_dy16(int32_t mode, const struct qatvit_tn_item* items, int32_t n, int32_t M, int32_t center, int32_t w_per_channel, int32_t w_qmin, int32_t w_qmax,
                               float* scratch, int64_t scratch_bytes, void* stream) {
    QV_CHECK_ARG(items && scratch && n >= 1, "qatvit_gemm_tn_stream_dy16: null / empty argument");
    QV_CHECK_ARG(n <= kTnStreamMax, "tn_stream: bad arguments (n=%d, mode=%d)", n, mode);
    TNGemm g[kTnStreamMax];   // qatvit_tn_item is the C caller's layout, TNGemm the library's: copied, not cast
    for (int i = 0; i < n; ++i) {
        const qatvit_tn_item& t = items[i];
        g[i].P = t.P; g[i].Q = t.Q; g[i].lut = t.lut; g[i].s1 = t.s1; g[i].s2 = t.s2; g[i].C = t.C; g[i].W = t.W; g[i].w_scale = t.w_scale; g[i].w_zp = t.w_zp;
        g[i].dbias = t.dbias; g[i].row_div = t.row_div; g[i].N = t.N; g[i].Kw = t.Kw; g[i].ldp = t.ldp; g[i].ldq = t.ldq; g[i].ldc = t.ldc;
    }
    TNCall c;
    c.M = M; c.center = center; c.w_per_channel = w_per_channel; c.w_qmin = w_qmin; c.w_qmax = w_qmax; c.scratch = scratch; c.scratch_bytes = scratch_bytes;
    // mode 0 / 1 / 2 are kTNPlaneQ8 / kTNPlaneCodes / kTNPlaneF16 by value (the static_assert at enum TNForm); launch_tn_stream refuses every other number
    if (launch_tn_stream((TNForm)mode, g, n, c, (hipStream_t)stream)) return 1;
    QV_CHECK_LAUNCH("qatvit_gemm_tn_stream_dy16");
    return 0;
}

int qatvit_gemm_tn_codes(const void* P_hi, const void* P_lo, const void* Qc, const uint32_t* lutQ, float* C, int32_t M, int32_t N, int32_t Kw, int32_t ldp,
                         int32_t ldq, int32_t ldc, const float* s1, const float* W, const float* w_scale, const int32_t* w_zp, int32_t w_per_channel,
                         int32_t w_qmin, int32_t w_qmax, float* dbias, const float* row_div, float* scratch, int64_t scratch_bytes, void* stream) {
    QV_CHECK_ARG(P_hi && P_lo && Qc && lutQ && C, "qatvit_gemm_tn_codes: null pointer argument");
    QV_TN_REQUEST(g, c);
    g.P = P_hi; g.P_lo = P_lo; g.Q = Qc; g.lut = lutQ; g.s1 = s1;
    if (launch_gemm_tn(kTNPairCodes, g, c, (hipStream_t)stream)) return 1;
    QV_CHECK_LAUNCH("qatvit_gemm_tn_codes");
    return 0;
}
#undef QV_TN_REQUEST

int64_t qatvit_gemm_tn_scratch_bytes(void) { return kTnScratchBytes; }

int32_t qatvit_attn_padded_tokens(int32_t T) { return attn_padded_tokens(T); }

int qatvit_attn_forward(const float* qkv, const float* qp, int32_t qmin, int32_t qmax, int32_t B, int32_t T, int32_t H, int32_t D, void* O_hi,
                        void* O_lo, float* lse, void* stream) {
    QV_CHECK_ARG(qkv && qp && O_hi && O_lo && lse, "qatvit_attn_forward: null pointer argument");
    QV_CHECK_ARG(B >= 1 && T >= 1 && H >= 1, "qatvit_attn_forward: empty shape");
    if (launch_attn_fwd(qkv, qp, qmin, qmax, B, T, H, D, O_hi, O_lo, lse, (hipStream_t)stream)) return 1;
    QV_CHECK_LAUNCH("qatvit_attn_forward");
    return 0;
}

int qatvit_attn_forward_f16(const float* qkv, const float* qp, int32_t qmin, int32_t qmax, int32_t B, int32_t T, int32_t H, int32_t D, void* O_hi,
                            void* O_lo, float* lse, void* O16_hi, void* O16_lo, float* o16_scale, void* qkv_codes, void* qkv_mask, void* stream) {
    QV_CHECK_ARG((qkv || qkv_codes) && qp && O_hi && O_lo && lse && O16_hi && O16_lo && o16_scale, "qatvit_attn_forward_f16: null pointer argument");
    QV_CHECK_ARG(B >= 1 && T >= 1 && H >= 1, "qatvit_attn_forward_f16: empty shape");
    if (launch_attn_fwd(qkv, qp, qmin, qmax, B, T, H, D, O_hi, O_lo, lse, (hipStream_t)stream, O16_hi, O16_lo, o16_scale, qkv_codes, qkv_mask)) return 1;
    QV_CHECK_LAUNCH("qatvit_attn_forward_f16");
    return 0;
}

int qatvit_attn_backward(const float* qkv, const float* qp, int32_t qmin, int32_t qmax, int32_t B, int32_t T, int32_t H, int32_t D,
                         const void* O_hi, const void* O_lo, const float* lse, float* delta, const float* dO, void* dqkv_hi, void* dqkv_lo,
                         const float* col_scale, const void* qkv_codes, const void* qkv_mask, void* stream) {
    QV_CHECK_ARG((qkv || qkv_codes) && qp && O_hi && O_lo && lse && delta && dO && dqkv_hi && dqkv_lo, "qatvit_attn_backward: null pointer argument");
    if (launch_attn_bwd(qkv, qp, qmin, qmax, B, T, H, D, O_hi, O_lo, lse, delta, dO, dqkv_hi, dqkv_lo, col_scale, (hipStream_t)stream, qkv_codes, qkv_mask))
        return 1;
    QV_CHECK_LAUNCH("qatvit_attn_backward");
    return 0;
}

int qatvit_attn_backward_live(const float* qkv, const float* qp, int32_t qmin, int32_t qmax, int32_t B, int32_t T, int32_t H, int32_t D,
                              const void* O_hi, const void* O_lo, const float* lse, float* delta, const float* dO, void* dqkv_hi, void* dqkv_lo,
                              const float* col_scale, const void* qkv_codes, const void* qkv_mask, int32_t live_q_tiles, int32_t dO_cls, void* stream) {
    QV_CHECK_ARG((qkv || qkv_codes) && qp && O_hi && O_lo && lse && delta && dO && dqkv_hi && dqkv_lo, "qatvit_attn_backward_live: null pointer argument");
    QV_CHECK_ARG(live_q_tiles >= 0 && (!dO_cls || live_q_tiles >= 1), "qatvit_attn_backward_live: live_q_tiles %d (>= 0; >= 1 with the [B, D] form of dO)", live_q_tiles);
    if (launch_attn_bwd(qkv, qp, qmin, qmax, B, T, H, D, O_hi, O_lo, lse, delta, dO, dqkv_hi, dqkv_lo, col_scale, (hipStream_t)stream, qkv_codes, qkv_mask, nullptr,
                        nullptr, live_q_tiles, dO_cls != 0))
        return 1;
    QV_CHECK_LAUNCH("qatvit_attn_backward_live");
    return 0;
}

int qatvit_attn_backward_form(const float* qkv, const float* qp, int32_t qmin, int32_t qmax, int32_t B, int32_t T, int32_t H, int32_t D,
                              const void* O_hi, const void* O_lo, const float* lse, float* delta, const float* dO, void* dqkv_hi, void* dqkv_lo,
                              const float* col_scale, const void* qkv_codes, const void* qkv_mask, const float* o16_mul, uint32_t* o16_amax, int32_t form,
                              void* stream) {
    static_assert(QATVIT_DY16_AMAX_SLOTS == kDyAmaxSlots && QATVIT_DY16_AMAX_STRIDE == kDyAmaxStride, "qatvit.h mirrors the amax slot layout");
    QV_CHECK_ARG((qkv || qkv_codes) && qp && O_hi && O_lo && lse && delta && dO && dqkv_hi && (dqkv_lo || o16_mul), "qatvit_attn_backward_form: null pointer argument");
    QV_CHECK_ARG(form >= kAttnBwdPerHead && form <= kAttnBwdPipe5, "qatvit_attn_backward_form: form %d (0 per-head launches, 1 persistent, 2 persistent on 5 workgroups)", form);
    QV_CHECK_ARG(B >= 1 && T >= 1 && H >= 1, "qatvit_attn_backward_form: empty shape");
    if (launch_attn_bwd(qkv, qp, qmin, qmax, B, T, H, D, O_hi, O_lo, lse, delta, dO, dqkv_hi, dqkv_lo, col_scale, (hipStream_t)stream, qkv_codes, qkv_mask, o16_mul,
                        o16_amax, 0, false, form))
        return 1;
    QV_CHECK_LAUNCH("qatvit_attn_backward_form");
    return 0;
}

int qatvit_eval_accumulate(const void* logits, int32_t dtype, int64_t ld, const int64_t* labels, int64_t batch, int64_t classes, const float* other,
                           int64_t other_ld, const int64_t* other_index, int64_t other_rows, void* state, int64_t* confusion, void* stream) {
    static_assert(sizeof(EvalState) == 8 * QATVIT_EVAL_STATE_WORDS, "QATVIT_EVAL_STATE_WORDS mirrors EvalState");
    QV_CHECK_ARG(logits && labels && state, "qatvit_eval_accumulate: null pointer argument");
    QV_CHECK_ARG(batch >= 1 && batch < (1ll << 30), "qatvit_eval_accumulate: batch %lld (1 .. 2^30 - 1)", (long long)batch);
    QV_CHECK_ARG(classes >= 2 && classes < (1ll << 30), "qatvit_eval_accumulate: classes %lld (2 .. 2^30 - 1)", (long long)classes);
    QV_CHECK_ARG(ld >= classes, "qatvit_eval_accumulate: ld %lld is less than classes %lld", (long long)ld, (long long)classes);
    QV_CHECK_ARG(dtype == QATVIT_EVAL_F32 || dtype == QATVIT_EVAL_F16 || dtype == QATVIT_EVAL_BF16,
                 "qatvit_eval_accumulate: unknown dtype code %d (0 = fp32, 1 = fp16, 2 = bf16)", dtype);
    QV_CHECK_ARG(other || !other_index, "qatvit_eval_accumulate: other_index given without other");
    QV_CHECK_ARG(!other || other_ld >= classes, "qatvit_eval_accumulate: other_ld %lld is less than classes %lld", (long long)other_ld, (long long)classes);
    QV_CHECK_ARG(!other_index || other_rows >= 1, "qatvit_eval_accumulate: other_rows %lld (at least 1 with an index)", (long long)other_rows);
    QV_CHECK_ARG(((uintptr_t)state & 7) == 0 && ((uintptr_t)confusion & 7) == 0, "qatvit_eval_accumulate: misaligned state or confusion pointer");
    if (launch_eval_accumulate(logits, dtype, ld, labels, batch, classes, other, other_ld, other_index, other_rows, static_cast<EvalState*>(state), confusion,
                               (hipStream_t)stream))
        return 1;
    QV_CHECK_LAUNCH("qatvit_eval_accumulate");
    return 0;
}

static int image_shape_ok(const char* who, int32_t S, int32_t D) {
    QV_CHECK_ARG(S >= 8 && S <= D, "%s: source size %d is outside 8 .. output size %d (downscaling is not supported)", who, S, D);
    QV_CHECK_ARG(D % 4 == 0 && D <= kImgMaxD, "%s: output size %d must be a multiple of 4, at most %d", who, D, kImgMaxD);
    return 0;
}

int qatvit_image_resize_coeffs(int32_t src, int32_t dst, int32_t* xmin_host, int32_t* ntaps_host, int32_t* coef_host) {
    QV_CHECK_ARG(xmin_host && ntaps_host && coef_host, "qatvit_image_resize_coeffs: null pointer argument");
    if (image_shape_ok("qatvit_image_resize_coeffs", src, dst)) return 1;
    return image_resize_coeffs(src, dst, xmin_host, ntaps_host, coef_host);
}

int qatvit_image_table(const float* mean_host, const float* std_host, float* table_host) {
    QV_CHECK_ARG(mean_host && std_host && table_host, "qatvit_image_table: null pointer argument");
    for (int c = 0; c < 3; ++c) QV_CHECK_ARG(std_host[c] != 0.0f, "qatvit_image_table: std[%d] is zero", c);
    image_table(mean_host, std_host, table_host);
    return 0;
}

// The ten batch entries: each fills an ImageBatch (qv_kernels.h) with its own arguments and runs it.  The part of the record that all of them have:
static ImageBatch image_request(const uint8_t* data, const int64_t* index, int32_t B, int32_t N, int32_t S, int32_t D, const int32_t* tab,
                                const float* table, float* out) {
    ImageBatch r;
    r.data = data, r.index = index, r.B = B, r.N = N, r.S = S, r.D = D, r.tab = tab, r.table = table, r.out = out;
    return r;
}

// Every argument check, once; who = the entry that was called.  no_rrc = what an entry of the window family says of the call without window records,
// which it refuses; nullptr in the other family, the one with padding_mode and fill.  A record pointer that is null is aligned.
static int image_request_ok(const char* who, const ImageBatch& r, const char* no_rrc) {
    QV_CHECK_ARG(r.data && r.tab && r.table && r.out, "%s: null pointer argument", who);
    QV_CHECK_ARG(!no_rrc || r.rrc, "%s: rrc is NULL (%s)", who, no_rrc);
    if (image_shape_ok(who, r.S, r.D)) return 1;
    QV_CHECK_ARG(r.B >= 1 && r.B <= 65535 && r.N >= 1, "%s: batch %d must be 1 .. 65535 and the data set (%d images) not empty", who, r.B, r.N);
    QV_CHECK_ARG(r.index || r.B <= r.N, "%s: batch %d of a data set of %d images needs an index", who, r.B, r.N);
    if (!no_rrc) {
        QV_CHECK_ARG(r.padding_mode == 0 || r.padding_mode == 1, "%s: unknown padding_mode %d (0 = constant, 1 = reflect)", who, r.padding_mode);
        QV_CHECK_ARG(r.fill >= 0 && r.fill <= 255, "%s: fill %d is outside 0 .. 255", who, r.fill);
    }
    const uintptr_t words = (uintptr_t)r.tab | (uintptr_t)r.table | (uintptr_t)r.aug | (uintptr_t)r.rrc | (uintptr_t)r.mix | (uintptr_t)r.erase |
                            (uintptr_t)r.color | (uintptr_t)r.sums | (uintptr_t)r.blur;
    QV_CHECK_ARG(((uintptr_t)r.out & 15) == 0 && (words & 3) == 0, "%s: misaligned pointer", who);
    return 0;
}

// the check, the launch (which refuses a form's LDS request before any HIP call, under the form's own name), the launch check
static int image_run(const char* who, const ImageBatch& r, void* stream, const char* no_rrc = nullptr) {
    if (image_request_ok(who, r, no_rrc)) return 1;
    if (int rc = launch_image_batch(r, (hipStream_t)stream)) return rc;
    QV_CHECK_LAUNCH(who);
    return 0;
}

int qatvit_image_batch(const uint8_t* data, const int64_t* index, int32_t B, int32_t N, int32_t S, int32_t D, const int32_t* coeffs,
                       const float* table, float* out, void* stream) {
    return image_run("qatvit_image_batch", image_request(data, index, B, N, S, D, coeffs, table, out), stream);
}

int qatvit_image_batch_aug(const uint8_t* data, const int64_t* index, int32_t B, int32_t N, int32_t S, int32_t D, const int32_t* coeffs,
                           const float* table, const int32_t* aug, int32_t padding_mode, int32_t fill, float* out, void* stream) {
    ImageBatch r = image_request(data, index, B, N, S, D, coeffs, table, out);
    r.aug = aug, r.padding_mode = padding_mode, r.fill = fill;
    return image_run("qatvit_image_batch_aug", r, stream);
}

int qatvit_image_batch_mix(const uint8_t* data, const int64_t* index, int32_t B, int32_t N, int32_t S, int32_t D, const int32_t* coeffs,
                           const float* table, const int32_t* aug, int32_t padding_mode, int32_t fill, const int32_t* mix, float* out,
                           void* stream) {
    ImageBatch r = image_request(data, index, B, N, S, D, coeffs, table, out);
    r.aug = aug, r.padding_mode = padding_mode, r.fill = fill, r.mix = mix;
    return image_run("qatvit_image_batch_mix", r, stream);
}

int qatvit_image_resize_coeffs_windows(int32_t src, int32_t dst, int32_t* out_host) {
    QV_CHECK_ARG(out_host, "qatvit_image_resize_coeffs_windows: null pointer argument");
    if (image_shape_ok("qatvit_image_resize_coeffs_windows", src, dst)) return 1;
    return image_resize_coeffs_windows(src, dst, out_host);
}

int qatvit_image_batch_rrc(const uint8_t* data, const int64_t* index, int32_t B, int32_t N, int32_t S, int32_t D, const int32_t* windows,
                           const float* table, const int32_t* rrc, const int32_t* mix, float* out, void* stream) {
    ImageBatch r = image_request(data, index, B, N, S, D, windows, table, out);
    r.rrc = rrc, r.mix = mix;
    return image_run("qatvit_image_batch_rrc", r, stream, "the call without records is qatvit_image_batch or qatvit_image_batch_mix");
}

int qatvit_image_batch_erase(const uint8_t* data, const int64_t* index, int32_t B, int32_t N, int32_t S, int32_t D, const int32_t* coeffs,
                             const float* table, const int32_t* aug, int32_t padding_mode, int32_t fill, const int32_t* mix,
                             const int32_t* erase, float* out, void* stream) {
    ImageBatch r = image_request(data, index, B, N, S, D, coeffs, table, out);
    r.aug = aug, r.padding_mode = padding_mode, r.fill = fill, r.mix = mix, r.erase = erase;
    return image_run("qatvit_image_batch_erase", r, stream);
}

int qatvit_image_batch_rrc_erase(const uint8_t* data, const int64_t* index, int32_t B, int32_t N, int32_t S, int32_t D, const int32_t* windows,
                                 const float* table, const int32_t* rrc, const int32_t* mix, const int32_t* erase, float* out, void* stream) {
    ImageBatch r = image_request(data, index, B, N, S, D, windows, table, out);
    r.rrc = rrc, r.mix = mix, r.erase = erase;
    return image_run("qatvit_image_batch_rrc_erase", r, stream, "the call without window records is qatvit_image_batch_erase");
}

int qatvit_image_batch_color(const uint8_t* data, const int64_t* index, int32_t B, int32_t N, int32_t S, int32_t D, const int32_t* coeffs,
                             const float* table, const int32_t* aug, int32_t padding_mode, int32_t fill, const int32_t* mix,
                             const int32_t* erase, const int32_t* color, uint32_t* sums, float* out, void* stream) {
    ImageBatch r = image_request(data, index, B, N, S, D, coeffs, table, out);
    r.aug = aug, r.padding_mode = padding_mode, r.fill = fill, r.mix = mix, r.erase = erase, r.color = color, r.sums = sums;
    return image_run("qatvit_image_batch_color", r, stream);
}

int qatvit_image_batch_rrc_color(const uint8_t* data, const int64_t* index, int32_t B, int32_t N, int32_t S, int32_t D, const int32_t* windows,
                                 const float* table, const int32_t* rrc, const int32_t* mix, const int32_t* erase, const int32_t* color,
                                 uint32_t* sums, float* out, void* stream) {
    ImageBatch r = image_request(data, index, B, N, S, D, windows, table, out);
    r.rrc = rrc, r.mix = mix, r.erase = erase, r.color = color, r.sums = sums;
    return image_run("qatvit_image_batch_rrc_color", r, stream, "the call without window records is qatvit_image_batch_color");
}

int qatvit_image_batch_blur(const uint8_t* data, const int64_t* index, int32_t B, int32_t N, int32_t S, int32_t D, const int32_t* coeffs,
                            const float* table, const int32_t* aug, int32_t padding_mode, int32_t fill, const int32_t* mix, const int32_t* erase,
                            const int32_t* color, uint32_t* sums, const int32_t* blur, float* out, void* stream) {
    ImageBatch r = image_request(data, index, B, N, S, D, coeffs, table, out);
    r.aug = aug, r.padding_mode = padding_mode, r.fill = fill, r.mix = mix, r.erase = erase, r.color = color, r.sums = sums, r.blur = blur;
    return image_run("qatvit_image_batch_blur", r, stream);
}

int qatvit_image_batch_rrc_blur(const uint8_t* data, const int64_t* index, int32_t B, int32_t N, int32_t S, int32_t D, const int32_t* windows,
                                const float* table, const int32_t* rrc, const int32_t* mix, const int32_t* erase, const int32_t* color,
                                uint32_t* sums, const int32_t* blur, float* out, void* stream) {
    ImageBatch r = image_request(data, index, B, N, S, D, windows, table, out);
    r.rrc = rrc, r.mix = mix, r.erase = erase, r.color = color, r.sums = sums, r.blur = blur;
    return image_run("qatvit_image_batch_rrc_blur", r, stream, "the call without window records is qatvit_image_batch_blur");
}

// The window stage (image_window.hip): the output size and a side of the source, every check before any HIP call
static int window_shape_ok(const char* who, const char* what, int32_t side, int32_t D) {
    QV_CHECK_ARG(D % 4 == 0 && D >= 8 && D <= kImgMaxD, "%s: output size %d must be a multiple of 4 in 8 .. %d", who, D, kImgMaxD);
    QV_CHECK_ARG(side >= 8 && side <= kWinMaxScale * D, "%s: %s %d is outside 8 .. %d (%d times the output size %d)", who, what, side,
                 kWinMaxScale * D, kWinMaxScale, D);
    return 0;
}

int64_t qatvit_image_window_coeffs_bytes(int32_t max_side, int32_t D) {
    if (window_shape_ok("qatvit_image_window_coeffs_bytes", "max_side", max_side, D)) return -1;
    return image_window_coeffs_words(max_side, D) * 4;
}

int qatvit_image_window_coeffs(int32_t max_side, int32_t D, int32_t* out_host) {
    QV_CHECK_ARG(out_host, "qatvit_image_window_coeffs: null pointer argument");
    if (window_shape_ok("qatvit_image_window_coeffs", "max_side", max_side, D)) return 1;
    return image_window_coeffs(max_side, D, out_host);
}

int qatvit_image_window_u8(const uint8_t* data, const int64_t* index, int32_t B, int32_t N, int32_t H, int32_t W, int32_t D, const int32_t* tables,
                           int32_t max_side, const int32_t* rrc, uint8_t* out, void* stream) {
    const char* who = "qatvit_image_window_u8";
    QV_CHECK_ARG(data && tables && rrc && out, "%s: null pointer argument", who);
    if (window_shape_ok(who, "source height", H, D) || window_shape_ok(who, "source width", W, D)) return 1;
    QV_CHECK_ARG(max_side >= H && max_side >= W, "%s: tables of %d sides do not serve a %d x %d source", who, max_side, H, W);
    QV_CHECK_ARG(B >= 1 && B <= 65535 && N >= 1, "%s: batch %d must be 1 .. 65535 and the data set (%d images) not empty", who, B, N);
    QV_CHECK_ARG(index || B <= N, "%s: batch %d of a data set of %d images needs an index", who, B, N);
    QV_CHECK_ARG((((uintptr_t)tables | (uintptr_t)rrc | (uintptr_t)out) & 3) == 0 && ((uintptr_t)index & 7) == 0, "%s: misaligned pointer", who);
    ImageWindow r;
    r.data = data, r.index = index, r.B = B, r.N = N, r.H = H, r.W = W, r.D = D, r.tables = tables, r.rrc = rrc, r.out = out;
    if (int rc = launch_image_window(r, (hipStream_t)stream)) return rc;
    QV_CHECK_LAUNCH(who);
    return 0;
}

// The bytes-in blur form (image_bytes_blur.hip): every check before any HIP call; the launcher refuses the LDS request under the same name
int qatvit_image_bytes_blur(const uint8_t* bytes, int32_t B, int32_t D, const float* table, const int32_t* mix, const int32_t* erase,
                            const int32_t* color, uint32_t* sums, const int32_t* blur, float* out, void* stream) {
    const char* who = "qatvit_image_bytes_blur";
    QV_CHECK_ARG(bytes && table && blur && out, "%s: null pointer argument (without blur records the call is qatvit_image_batch_color at S = D)", who);
    QV_CHECK_ARG(D % 4 == 0 && D >= 8 && D <= kImgMaxD, "%s: output size %d must be a multiple of 4 in 8 .. %d", who, D, kImgMaxD);
    QV_CHECK_ARG(B >= 1 && B <= 65535, "%s: batch %d must be 1 .. 65535", who, B);
    const uintptr_t words = (uintptr_t)bytes | (uintptr_t)table | (uintptr_t)mix | (uintptr_t)erase | (uintptr_t)color | (uintptr_t)sums | (uintptr_t)blur;
    QV_CHECK_ARG(((uintptr_t)out & 15) == 0 && (words & 3) == 0, "%s: misaligned pointer", who);
    ImageBytesBlur r;
    r.bytes = bytes, r.B = B, r.D = D, r.table = table, r.mix = mix, r.erase = erase, r.color = color, r.sums = sums, r.blur = blur, r.out = out;
    if (int rc = launch_image_bytes_blur(r, (hipStream_t)stream)) return rc;
    QV_CHECK_LAUNCH(who);
    return 0;
}

int qatvit_rows_gather(const void* tall, void* compact, int32_t rows, int32_t T, int32_t width, int64_t stride, void* stream) {
    RowMoveTab t;
    t.n = 1; t.m[0] = RowMove{tall, compact, stride, width};
    if (launch_rows_gather(t, rows, T, (hipStream_t)stream)) return 1;
    QV_CHECK_LAUNCH("qatvit_rows_gather");
    return 0;
}

int qatvit_rows_scatter(const void* compact, void* tall, int32_t rows, int32_t T, int32_t width, void* stream) {
    RowMoveTab t;
    t.n = 1; t.m[0] = RowMove{compact, tall, width, width};
    if (launch_rows_scatter(t, rows, T, (hipStream_t)stream)) return 1;
    QV_CHECK_LAUNCH("qatvit_rows_scatter");
    return 0;
}

}  // extern "C"
