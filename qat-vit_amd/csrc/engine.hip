// The QAT student step as ONE native forward and ONE native backward (host-side enqueue only).
//
// Mirrors the dataflow of a prepare_qat()-ed QATWrapper(ViT)
// (/root/reference/src/models/model_registry.py:113-120 under qat_trainer.py:304-307):
// every weight_fake_quant / activation_post_process sits at the same point, its buffers
// (min/max/scale/zero_point) are updated in place, and backward applies the same STE masks.
// Everything is enqueued on the caller's stream; no allocation, no host sync, no thread-local
// device state (backward runs on autograd's worker thread).
#include <string.h>

#include <memory>
#include <mutex>
#include <type_traits>
#include <unordered_map>
#include <vector>

#include "../../include/qatvit.h"
#include <stdlib.h>

#include "qv_common.h"
#include "qv_kernels.h"

namespace qv {

enum { P_PE_W = 0, P_PE_B, P_CLS, P_POS, P_BLOCK0 };                        // then 12 per block, then 4 tail
enum { B_N1W = 0, B_N1B, B_QKVW, B_QKVB, B_PROJW, B_PROJB, B_N2W, B_N2B, B_FC1W, B_FC1B, B_FC2W, B_FC2B, B_COUNT };
enum { A_IN = 0, A_PE, A_BLOCK0 };                                           // act FQ: then 6 per block, then norm, head
enum { AB_N1 = 0, AB_QKV, AB_PROJ, AB_N2, AB_FC1, AB_FC2, AB_COUNT };
enum { WB_QKV = 0, WB_PROJ, WB_FC1, WB_FC2, WB_COUNT };                      // weight FQ: pe, 4 per block, head

struct Dims {
    int B, T, np, D, H, Hd, C, depth, Kpe, img, patch, chans;
    int64_t M;
    int n_act, n_w;
};

static Dims dims_of(const qatvit_cfg& c) {
    Dims d;
    d.B = c.batch; d.img = c.img_size; d.patch = c.patch_size; d.chans = c.in_chans;
    d.np = (c.img_size / c.patch_size) * (c.img_size / c.patch_size);
    d.T = d.np + 1; d.D = c.embed_dim; d.H = c.num_heads; d.Hd = c.mlp_hidden; d.C = c.num_classes; d.depth = c.depth;
    d.Kpe = c.in_chans * c.patch_size * c.patch_size;
    d.M = (int64_t)d.B * d.T;
    d.n_act = 2 + AB_COUNT * d.depth + 2;
    d.n_w = 1 + WB_COUNT * d.depth + 1;
    return d;
}

// weight shapes by weight-FQ index
static void wshape(const Dims& d, int wi, int* N, int* K) {
    if (wi == 0) { *N = d.D; *K = d.Kpe; return; }
    if (wi == d.n_w - 1) { *N = d.C; *K = d.D; return; }
    switch ((wi - 1) % WB_COUNT) {
        case WB_QKV: *N = 3 * d.D; *K = d.D; break;
        case WB_PROJ: *N = d.D; *K = d.D; break;
        case WB_FC1: *N = d.Hd; *K = d.D; break;
        default: *N = d.D; *K = d.Hd; break;
    }
}
static int wparam(const Dims& d, int wi) {  // index of the weight tensor in params[]
    if (wi == 0) return P_PE_W;
    if (wi == d.n_w - 1) return P_BLOCK0 + B_COUNT * d.depth + 2;
    const int blk = (wi - 1) / WB_COUNT, k = (wi - 1) % WB_COUNT;
    static const int map[WB_COUNT] = {B_QKVW, B_PROJW, B_FC1W, B_FC2W};
    return P_BLOCK0 + B_COUNT * blk + map[k];
}

// Which form every GEMM, attention pass and LayerNorm backward of a configuration runs: decided once, from the knob table (qv_common.h Knobs) and the
// shapes.  All blocks share their shapes, so all blocks take the same forms.  What stays per call: the flags (QATVIT_FWD_X16, QATVIT_BWD_DY16,
// QATVIT_BWD_CALIBRATE), injection, the stage range, and the M each strip launch checks (i8_strip_covers).
struct Forms {
    bool i8;                 // the grid x grid forward GEMMs (patch-embed, qkv, fc1) on int8 MFMA where their shapes allow (linear_fwd_grid)
    bool w_batched;          // the weight preparation as three multi-tensor launches (the only writer of the fp16 weight copies)
    bool late;               // late-resolved qparams (qv_kernels.h QpLate): LayerNorm / proj / fc2 outputs, qkv / fc1 where the strip kernel's code pass consumes them
    bool f16_proj, f16_fc2;  // the float operands of the proj / fc2 forward GEMMs as fp16 (hi, lo) pairs (else bf16 pairs)
    bool fc2_codes;          // fc2's forward A operand as one byte per element + a 256-entry table of fp16 pairs (else the two fp16 planes)
    bool fc1_code_bits;      // the backward's fc1 codes as that byte plane + one STE mask bit per element (else the uint16 plane; needs the tall dgrad tile)
    bool fc2w_codes;         // fc2's weight gradient from the byte plane + a bf16-pair table (else the bf16 planes; needs the 128 x 384 wgrad tile)
    bool attn_codes;         // the attention backward reads the codes its forward saved (else it re-quantises the fp32 qkv)
    bool qkv_2pass;          // the qkv GEMM as a statistics pass + a pass writing codes and mask bits in the attention layout (the fp32 qkv never exists)
    bool attn_bwd_fused;     // the fused attention backward (head_dim 64, 33..224 tokens, saved codes)
    bool lnb;                // the LayerNorm backward in the fc1 / qkv dgrad epilogue (NTPost mode 8: the 208 x 384 tile holds whole rows)
    bool x_plane_from_q8;    // the one-plane qkv / fc1 weight gradients read the int8 plane of the LayerNorm outputs (q - center) instead of the fp16 one
    bool tn_stream;          // the per-block gradient planes + stream-K scratch exist (the one-plane weight gradients then run at the end of the call)
    bool dy16;               // the one-plane backward covers this configuration
    bool ln_in_strip;        // norm1 / norm2 apply + quantise inside the statistics pass of qkv / fc1 (launch_i8_strip_ln) where the forward writes the byte plane only (ln_in_strip_of)
    bool cls_bwd;            // the one-plane backward of the final norm and of the last block's MLP + proj on the B class-token rows (Plan::ClsRows; bwd() decides per call)
};
// drop_path: a drop-path scale table or a LayerScale binding is bound to the workspace of the call (qatvit_student_set_drop_path, _set_layer_scale)
static Forms forms_of(const qatvit_cfg& c, const Dims& d, bool drop_path) {
    const Knobs& k = knobs();
    const bool byte_codes = c.act_qmax - c.act_qmin <= 255;
    Forms f{};
    f.i8 = k.i8;
    f.w_batched = k.wbatch && d.n_w <= kMaxW;
    f.late = k.qp_late && d.n_act <= kMaxActFq;
    f.f16_proj = k.f16 && f.w_batched && d.D % 384 == 0;   // the fp16-pair GEMM: N % 384 == 0, K % 32 == 0 (proj: N = K = D; fc2: N = D, K = Hd)
    f.f16_fc2 = f.f16_proj && d.Hd % 32 == 0;
    f.fc2_codes = f.f16_fc2 && k.fc2_codes && d.Hd % 64 == 0 && byte_codes;
    f.fc1_code_bits = f.fc2_codes && k.fc1_bits && f.i8 && d.Hd % 384 == 0;
    f.fc2w_codes = f.fc1_code_bits && k.fc2w_codes;
    f.attn_codes = k.attn_codes && byte_codes;
    f.qkv_2pass = k.qkv_2pass && f.attn_codes && f.i8 && (3 * d.D) % 384 == 0 && d.D % 64 == 0 && (d.D / d.H) % 32 == 0;
    f.attn_bwd_fused = attn_bwd_is_fused(d.T, d.H, d.D, f.attn_codes);
    f.lnb = k.lnb_fuse && d.D == 384 && !drop_path;   // (the fused epilogue knows neither the drop-path multipliers nor a LayerScale gamma: k_ln_bwd_fq behind the plain dgrad does)
    f.x_plane_from_q8 = f.i8 && k.tn_q8 && d.D % 384 == 0;
    f.tn_stream = k.tn_stream && d.D % 384 == 0 && d.Hd % 384 == 0;
    f.dy16 = f.i8 && f.w_batched && d.D % 384 == 0 && d.Hd % 384 == 0 && f.qkv_2pass && f.attn_bwd_fused && f.f16_proj && f.fc2w_codes;
    f.ln_in_strip = k.ln_strip && f.i8 && f.late && f.x_plane_from_q8;
    f.cls_bwd = k.cls_bwd && f.dy16;
    return f;
}

struct Plan {
    Forms form;
    // byte offsets into the workspace
    int64_t stats, qp_act, qp_w, imgq, Y0, meanF, rstdF, hq, logits_pre;
    int64_t x_in, x_mid, mean1, rstd1, mean2, rstd2, h1q, qkv, O_hi, O_lo, lse, Yproj, h2q, Y1, G_hi, G_lo, Y2, mproj, m2, qkv8, qkvm, G8, glut, Y1m, glutq;  // per-block base, stride blk (mproj / m2: STE mask bits of Yproj / Y2)
    int64_t blk_stride;
    int64_t wq, wqT;                // per weight: offsets table below
    int64_t w_off[64 * 4 + 8], wT_off[64 * 4 + 8], w_stats[64 * 4 + 8], w_qp[64 * 4 + 8];
    int64_t w8_off[64 * 4 + 8], wsum_off[64 * 4 + 8], wsum_base, wsum_bytes, imgq8, h1q8, h2q8;   // int8 operands of the forward grid x grid GEMMs
    int64_t w8f_off[64 * 4 + 8];   // the int8 weight once more in fragment order (qkv, fc1 with K == 384 / 768: the strip kernel's B operand), -1 otherwise
    int64_t w16_off[64 * 4 + 8], O16_hi, O16_lo, G16_hi, G16_lo, scal16;   // fp16 operands of the forward float x grid GEMMs (proj, fc2): O16 / scal16 per block, G16 shared
    int64_t dxA, dxB, dYs_hi, dYs_lo, dG, dY1_hi, dY1_lo, dH, dO, dqkv_hi, dqkv_lo, delta, dh, dY0_hi, dY0_lo, tn_scratch;
    // the one-plane backward's gradient planes of EVERY block (its weight gradients run at the end of the call, k_tn_stream): per block [fc2-in | proj-in | fc1-out | qkv-out],
    // stride dyp_stride; 0 bytes where the deferred form does not apply.  tn_stream: the stream-K scratch
    int64_t dyp, dyp_stride, dyp_p, dyp_h, dyp_q, tn_stream;
    int64_t qp_staged;   // staging records of the late-resolved quantizers (qv_kernels.h QpLate): kQpStagedWords words per activation quantizer
    int64_t dy16;   // scale state of the one-plane backward (dy16.hip): 4 slots per block - the gradients entering fc2, fc1, proj, qkv
    // The class-token rows ([B, .] instead of [B * T, .]; Forms::cls_bwd, else absent): what the final norm's backward leaves for the last block (dx, dY - they
    // outlive the call: a staged backward runs stage 0 and stage 1 in different calls), that block's gathered forward operands, and its gradients on those rows
    struct ClsRows {
        int64_t dx, dY;                                             // d loss / d x_in[depth] fp32; its masked fc2-in plane fp16
        int64_t xF, meanF, rstdF, m2;                               // final norm: x_in[depth], row statistics, fc2's mask bits
        int64_t G8, Y1m, h2q, x_mid, mean2, rstd2, mproj, O16;      // last block (h2q: the int8 plane q - center, or the fp16 one where the weight gradient reads that)
        int64_t dY1, dYp, dxB, dO, dH;                              // fc1-out / proj-in planes fp16; d x_mid, d attention output, the unfused dgrad's output fp32
    } cls;
    int64_t total, stats_words;
    int TP;
};
enum { DS_FC2 = 0, DS_FC1, DS_PROJ, DS_QKV, DS_COUNT };

static int64_t al(int64_t x) { return (x + 255) & ~(int64_t)255; }

static int make_plan(const qatvit_cfg& c, Plan* p, bool drop_path = false) {   // (no offset depends on drop_path)
    const Dims d = dims_of(c);
    if (d.depth > 64) { set_error("engine: depth %d > 64", d.depth); return 1; }
    p->form = forms_of(c, d, drop_path);
    int64_t o = 0;
    auto take = [&](int64_t bytes) { int64_t r = o; o += al(bytes); return r; };
    const int64_t M = d.M, D = d.D, Hd = d.Hd;
    p->TP = attn_padded_tokens(d.T);
    // stats: act FQs (2 words each) then per weight (2 * channels)
    int64_t wstat_words = 0, wqp_floats = 0;
    for (int wi = 0; wi < d.n_w; ++wi) {
        int N, K; wshape(d, wi, &N, &K);
        const int ch = c.w_per_channel ? N : 1;
        p->w_stats[wi] = (int64_t)d.n_act * kStatSlots * kStatStride + wstat_words;
        wstat_words += c.w_per_channel ? 2 * ch : kStatSlots * kStatStride;
        p->w_qp[wi] = wqp_floats; wqp_floats += 4 * ch;
    }
    p->stats_words = (int64_t)d.n_act * kStatSlots * kStatStride + wstat_words;
    p->stats = take(p->stats_words * 4);
    p->qp_staged = take((int64_t)d.n_act * kQpStagedWords * 4);
    p->dy16 = take(dy16_state_bytes(DS_COUNT * d.depth));   // (next to the observer accumulators: its place does not depend on the batch either)
    p->qp_act = take((int64_t)d.n_act * 4 * 4);
    p->qp_w = take(wqp_floats * 4);
    p->imgq = take((int64_t)d.B * d.np * d.Kpe * 2);
    p->Y0 = take((int64_t)d.B * d.np * D * 4);
    p->meanF = take(M * 4); p->rstdF = take(M * 4);
    p->hq = take((int64_t)d.B * D * 4);
    p->logits_pre = take((int64_t)d.B * d.C * 4);
    // per block
    const int64_t b0 = o;
    p->x_in = take(M * D * 4);
    p->x_mid = take(M * D * 4);
    p->mean1 = take(M * 4); p->rstd1 = take(M * 4); p->mean2 = take(M * 4); p->rstd2 = take(M * 4);
    p->h1q = take(M * D * 2);
    p->qkv = take(M * 3 * D * 4);
    p->O_hi = take(M * D * 2); p->O_lo = take(M * D * 2);
    p->lse = take((int64_t)d.B * d.H * p->TP * 4);
    p->Yproj = take(M * D * 4);
    p->h2q = take(M * D * 2);
    p->Y1 = take(M * Hd * 2);   // uint16 codes of fc1's output (QATVIT_FC1_BITS=0 only; the fp32 pre-FQ tensor never exists)
    p->G_hi = take(M * Hd * 2); p->G_lo = take(M * Hd * 2);
    p->Y2 = take(M * D * 4);
    p->h1q8 = take(M * D); p->h2q8 = take(M * D);
    p->mproj = take(ln_maskbits_bytes(M, (int)D)); p->m2 = take(ln_maskbits_bytes(M, (int)D));
    p->qkv8 = take(M * 3 * D); p->qkvm = take(M * 3 * D / 8);   // the quantised qkv as the attention forward saw it (codes + STE mask bits), for its backward
    // the attention output once more as an fp16 (hi, lo) pair (proj's forward operand and, in the one-plane backward, its weight gradient's X operand) and the
    // two pair scales {attention output, gelu} the producers write: per block since round 4 (the backward reads them)
    p->O16_hi = take(M * D * 2); p->O16_lo = take(M * D * 2); p->scal16 = take(2 * sizeof(float));
    p->G8 = take(M * Hd); p->glut = take(256 * 4); p->Y1m = take(M * Hd / 8); p->glutq = take(256 * 4);   // (Y1m: the STE mask bits of fc1's fake-quant)   // gelu(fq(fc1 output)) as one byte per element + the 256-entry table of fp16 pairs (fc2 forward from codes)
    p->blk_stride = o - b0;
    o = b0 + p->blk_stride * d.depth;
    // x_in[depth] (input of the final norm) lives where block `depth` would start
    const int64_t xfinal = take(M * D * 4);
    (void)xfinal;  // == x_in + depth*blk_stride by construction
    for (int wi = 0; wi < d.n_w; ++wi) {
        int N, K; wshape(d, wi, &N, &K);
        p->w_off[wi] = take((int64_t)N * K * 2);
        p->wT_off[wi] = take((int64_t)N * K * 2);
        (void)take((int64_t)N * K * 2);   // the same transposed integers as fp16, wT16_gap_bytes(N, K) behind (the one-plane dgrad's B operand)
        (void)take((int64_t)N * K * 2);   // ... and once more in MFMA fragment order (written for fc2 where f16strip.hip takes the fc2 dgrad)
        p->w8_off[wi] = take((int64_t)N * K);
        const int kind = (wi == 0 || wi == d.n_w - 1) ? -1 : (wi - 1) % WB_COUNT;
        p->w16_off[wi] = (kind == WB_PROJ || kind == WB_FC2) ? take((int64_t)N * K * 2) : -1;
        p->w8f_off[wi] = ((kind == WB_QKV || kind == WB_FC1) && (K == 384 || K == 768) && N % 48 == 0) ? take((int64_t)N * K) : -1;
    }
    // gelu(fq(fc1)) as an fp16 (hi, lo) pair (QATVIT_FC2_CODES=0 only): written and consumed inside one block's forward, ONE set serves every block
    p->G16_hi = take(M * Hd * 2); p->G16_lo = take(M * Hd * 2);
    p->imgq8 = take((int64_t)d.B * d.np * d.Kpe);
    p->wsum_base = o;
    for (int wi = 0; wi < d.n_w; ++wi) {
        int N, K; wshape(d, wi, &N, &K);
        p->wsum_off[wi] = take((int64_t)N * 4);
    }
    p->wsum_bytes = o - p->wsum_base;
    p->dxA = take(M * D * 4); p->dxB = take(M * D * 4);
    p->dYs_hi = take(M * D * 2); p->dYs_lo = take(M * D * 2);
    p->dG = take(M * Hd * 4);
    p->dY1_hi = take(M * Hd * 2); p->dY1_lo = take(M * Hd * 2);
    p->dH = take(M * D * 4); p->dO = take(M * D * 4);
    p->dqkv_hi = take(M * 3 * D * 2); p->dqkv_lo = take(M * 3 * D * 2);
    p->delta = take((int64_t)d.B * d.H * p->TP * 4);
    p->dh = take((int64_t)d.B * D * 4);
    p->dY0_hi = take((int64_t)d.B * d.np * D * 2); p->dY0_lo = take((int64_t)d.B * d.np * D * 2);
    p->tn_scratch = take(kTnScratchBytes);   // split partials of the weight-gradient GEMMs (two-phase, non-atomic reduction)
    p->dyp = p->tn_stream = -1; p->dyp_stride = 0;
    if (p->form.tn_stream) {
        p->dyp_p = al(M * D * 2); p->dyp_h = p->dyp_p + al(M * D * 2); p->dyp_q = p->dyp_h + al(M * Hd * 2);
        p->dyp_stride = p->dyp_q + al(M * 3 * D * 2);
        p->dyp = take(p->dyp_stride * d.depth);
        p->tn_stream = take(tn_stream_scratch_bytes());
    }
    p->cls = Plan::ClsRows{};
    if (p->form.cls_bwd) {   // (behind everything else: no other offset depends on the knob)
        const int64_t B = d.B, mrow = ln_maskbits_bytes(1, (int)D);
        Plan::ClsRows& r = p->cls;
        r.dx = take(B * D * 4); r.dY = take(B * D * 2);
        r.xF = take(B * D * 4); r.meanF = take(B * 4); r.rstdF = take(B * 4); r.m2 = take(B * mrow);
        r.G8 = take(B * Hd); r.Y1m = take(B * Hd / 8); r.h2q = take(B * D * 2); r.x_mid = take(B * D * 4); r.mean2 = take(B * 4); r.rstd2 = take(B * 4);
        r.mproj = take(B * mrow); r.O16 = take(B * D * 2);
        r.dY1 = take(B * Hd * 2); r.dYp = take(B * D * 2); r.dxB = take(B * D * 4); r.dO = take(B * D * 4); r.dH = take(B * D * 4);
    }
    p->total = o;
    return 0;
}

// Does the statistics pass of layer `kind` (WB_QKV / WB_FC1) build its own strip from the fp32 rows (the LayerNorm in front of it then launches nothing)?  Only where
// the forward writes no 2-byte plane of the LayerNorm output (QATVIT_FWD_X16 with the byte-X weight gradients), the quantizer is resolved late, and the
// strip kernel takes the statistics pass with one workgroup per strip; qkv only in its two-pass form.  All blocks share the answer.
static bool ln_in_strip_of(const Plan& p, const Dims& d, int flags, int kind) {
    const Forms& F = p.form;
    if (!F.ln_in_strip || !(flags & QATVIT_FWD_X16) || (kind == WB_QKV && !F.qkv_2pass) || d.depth < 1) return false;
    const int wi = 1 + kind;
    NTGemm g;
    wshape(d, wi, &g.N, &g.K);
    g.B_frag = &p; g.M = (int)d.M; g.lda = g.K;   // (B_frag: any non-null pointer - the weight in fragment order exists)
    return F.w_batched && p.w8f_off[wi] >= 0 && g.K == d.D && i8_strip_ln_covers(g);
}

static int check_cfg(const qatvit_cfg& c) {
    if (c.batch < 1 || c.depth < 1 || c.embed_dim % 128 != 0 || c.mlp_hidden % 128 != 0 || c.embed_dim % c.num_heads != 0 ||
        c.img_size % c.patch_size != 0 || (c.in_chans * c.patch_size * c.patch_size) % 128 != 0 || c.embed_dim > 768) {
        set_error("engine: unsupported config (batch %d depth %d dim %d hidden %d heads %d img %d patch %d)", c.batch, c.depth, c.embed_dim,
                  c.mlp_hidden, c.num_heads, c.img_size, c.patch_size);
        return 1;
    }
    return 0;
}

// ---- optional in-situ timing of one GEMM class with HIP events on the launch stream (bench.py only).  The state belongs to ONE engine:
// it is keyed by that engine's workspace pointer, so two engines in one process never see each other's events.  A forward / backward call holds a
// shared_ptr to the session for its whole duration (backward runs on autograd's worker thread while the main thread may call
// qatvit_profile_stop): stop only marks the session closed and unlinks it - the object dies with its last holder; qatvit_student_init drops a
// session whose workspace is being re-bound (a re-allocated workspace must not inherit it).
struct Prof {
    int kind = 0;  // 1 NT split-A plain epilogue, 2 NT grid-A (int8), 3 TN, 4 NT split-A dgrad + fused LayerNorm backward, 5 fc2 dgrad + fused GELU', 6 TN split X, 7 / 8 / 9 int8 passes
    std::vector<hipEvent_t> ev;
    size_t used = 0;
    double flops = 0.0;
    bool closed = false;
    std::mutex mu;
    ~Prof() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); }
};
static std::mutex g_prof_mu;
static std::unordered_map<const void*, std::shared_ptr<Prof>> g_profs;
static std::shared_ptr<Prof> prof_of(const void* workspace) {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    auto it = g_profs.find(workspace);
    return it == g_profs.end() ? nullptr : it->second;
}
struct ProfScope {
    Prof* pr;
    hipStream_t st;
    size_t slot = 0;
    bool on = false;
    ProfScope(const std::shared_ptr<Prof>& p, int kind, double flops, hipStream_t s) : pr(p.get()), st(s) {
        if (!pr || pr->kind != kind) return;
        std::lock_guard<std::mutex> lk(pr->mu);
        if (pr->closed || pr->used + 2 > pr->ev.size()) return;
        slot = pr->used;
        pr->used += 2;
        pr->flops += flops;
        on = true;
        (void)hipEventRecord(pr->ev[slot], st);
    }
    ~ProfScope() {
        if (on) (void)hipEventRecord(pr->ev[slot + 1], st);
    }
};
// the ProfScope kind of an NT GEMM by its epilogue (qv_kernels.h NTEpi).  Forward on grid operands: 2 plain | 7 statistics pass | 8 fc1 storing pass | 9 qkv code
// pass; dgrad: 1 plain | 4 + fused LayerNorm backward | 5 + fused GELU' (fc2 dgrad).  A statistics-only pass is issued, not algorithmic, work: it counts no flops
static bool stats_only(const NTPost* post) { return post && post->mode == kEpiStats; }
static int prof_kind_fwd(const NTPost* post) { return !post ? 2 : post->mode == kEpiStats ? 7 : post->mode == kEpiCodes ? 8 : post->mode == kEpiQkvCodes ? 9 : 2; }
static int prof_kind_dgrad(const NTPost* post) { return !post ? 1 : post->mode == kEpiLnBwd ? 4 : 5; }
static NTPost nt_post_stats() { NTPost p{}; p.mode = kEpiStats; return p; }

struct Ctx {
    const qatvit_cfg& c;
    Dims d;
    Plan p;
    char* ws;
    void* const* params;
    const qatvit_fq* act;
    const qatvit_fq* wfq;
    hipStream_t st;
    std::shared_ptr<Prof> prof;
    int flags = 0;   // QATVIT_FWD_X16 (forward) / QATVIT_BWD_DY16, QATVIT_BWD_CALIBRATE (backward)
    // drop-path: the scale table bound to the workspace ([2 * depth][batch] floats), nullptr: none.  Row of block i's attention (mlp = 0) / MLP (1) branch:
    const float* drop = nullptr;
    const float* drop_row(int i, int mlp) const { return drop ? drop + (int64_t)(2 * i + mlp) * d.B : nullptr; }
    // LayerScale: the binding of the workspace (qatvit_student_set_layer_scale), null: none.  gamma / gradient of block i's attention (mlp = 0) / MLP (1) branch:
    std::shared_ptr<const LayerScale> ls;
    const float* ls_gamma(int i, int mlp) const { return ls ? ls->gamma[2 * i + mlp] : nullptr; }
    float* ls_grad(int i, int mlp) const { return ls && !ls->grad.empty() ? ls->grad[2 * i + mlp] : nullptr; }
    // ---- the one-plane backward (dy16.hip): slot k (DS_*) of block i
    uint32_t* dy_slot(int i, int k) const { return at<uint32_t>(p.dy16) + kDyHdrWords + (int64_t)(DS_COUNT * i + k) * kDySlotWords; }
    const float* dy_mul(int i, int k) const { return reinterpret_cast<const float*>(dy_slot(i, k) + 1); }
    const float* dy_inv(int i, int k) const { return reinterpret_cast<const float*>(dy_slot(i, k) + 2); }
    void* wT16(int wi) const { int N, K; wshape(d, wi, &N, &K); return ws + p.wT_off[wi] + wT16_gap_bytes(N, K); }
    void* wT16f(int wi) const { int N, K; wshape(d, wi, &N, &K); return ws + p.wT_off[wi] + 2 * wT16_gap_bytes(N, K); }
    // fc2's transposed weight in fragment order exists where the strip form of its dgrad applies (ViT-S: N = 384 columns of 2 bytes = 768-byte rows, K = 1536)
    bool wT16f_ok(int wi) const {
        int N, K; wshape(d, wi, &N, &K);
        return wi >= 1 && wi < d.n_w - 1 && (wi - 1) % WB_COUNT == WB_FC2 && N == 384 && K == 1536;
    }
    template <typename T> T* at(int64_t off) const { return reinterpret_cast<T*>(ws + off); }
    template <typename T> T* blk(int64_t off, int i) const { return reinterpret_cast<T*>(ws + off + p.blk_stride * i); }
    const float* prm(int i) const { return reinterpret_cast<const float*>(params[i]); }
    const float* bprm(int blk_i, int k) const { return prm(P_BLOCK0 + B_COUNT * blk_i + k); }
    int p_tail() const { return P_BLOCK0 + B_COUNT * d.depth; }   // the 4 tail parameters: final norm weight, bias, head weight, bias
    uint32_t* act_stats(int ai) const { return at<uint32_t>(p.stats) + (int64_t)ai * kStatSlots * kStatStride; }
    float* act_qp(int ai) const { return at<float>(p.qp_act) + 4 * ai; }
    float* w_qp(int wi) const { return at<float>(p.qp_w) + p.w_qp[wi]; }
    int aidx(int blk_i, int k) const { return A_BLOCK0 + AB_COUNT * blk_i + k; }
    int a_norm() const { return A_BLOCK0 + AB_COUNT * d.depth; }
    int a_head() const { return a_norm() + 1; }
    int widx(int blk_i, int k) const { return 1 + WB_COUNT * blk_i + k; }
    // One LayerNorm as its callers see it: the rows it normalises, their statistics, the affine parameters and the quantizer of its output.  norm1(depth) is the final norm
    struct LnRows { float* x; float* mean; float* rstd; const float* gamma; const float* beta; int ai; };
    LnRows norm1(int i) const {
        if (i < d.depth) return LnRows{blk<float>(p.x_in, i), blk<float>(p.mean1, i), blk<float>(p.rstd1, i), bprm(i, B_N1W), bprm(i, B_N1B), aidx(i, AB_N1)};
        return LnRows{blk<float>(p.x_in, d.depth), at<float>(p.meanF), at<float>(p.rstdF), prm(p_tail()), prm(p_tail() + 1), a_norm()};
    }
    LnRows norm2(int i) const { return LnRows{blk<float>(p.x_mid, i), blk<float>(p.mean2, i), blk<float>(p.rstd2, i), bprm(i, B_N2W), bprm(i, B_N2B), aidx(i, AB_N2)}; }
    // ---- late qparams (qv_kernels.h QpLate, Forms::late): the quantizers whose consumer kernel resolves the observer / qparams update itself - the
    // LayerNorm outputs (k_ln_apply_quant, or the statistics pass that has the LayerNorm in its prologue: ln_in_strip_of), the proj / fc2 outputs (k_resid_fq_lnstats) of every block always, the qkv / fc1 outputs where the strip
    // kernel's code pass is their consumer (decided by the caller: late_strip) - need no k_qparams launch behind the producer of their statistics
    bool late_kind(int ai) const {
        if (!p.form.late || ai < A_BLOCK0 || ai >= A_BLOCK0 + AB_COUNT * d.depth) return false;
        const int k = (ai - A_BLOCK0) % AB_COUNT;
        return k == AB_N1 || k == AB_N2 || k == AB_PROJ || k == AB_FC2;
    }
    QpLate late(int ai) const {
        const qatvit_fq& f = act[ai];
        return QpLate{act_stats(ai), f.min_val, f.max_val, f.scale, f.zero_point, f.observer_on, f.fake_quant_on, c.averaging_const, c.act_qmin, c.act_qmax,
                      act_qp(ai), at<float>(p.qp_staged) + (int64_t)ai * kQpStagedWords};
    }
    // the staged states into the modules' buffers: once at the end of every forward call
    int commit_late() const {
        if (!p.form.late) return 0;
        QpCommitTab t{};
        t.n = d.n_act; t.staged = at<float>(p.qp_staged); t.stats = at<uint32_t>(p.stats);
        for (int ai = 0; ai < d.n_act; ++ai) { t.rmin[ai] = act[ai].min_val; t.rmax[ai] = act[ai].max_val; t.scale[ai] = act[ai].scale; t.zp[ai] = act[ai].zero_point; }
        return launch_qp_commit(t, st);
    }
    // the observer / qparams update of activation quantizer ai: its own single-wave launch right behind the producer of its statistics - unless its consumer
    // resolves it (late_kind; `deferred`: the caller knows that the strip kernel's code pass will)
    void qparams_after(int ai, bool produced_stats, bool deferred = false) const {
        if (produced_stats && !deferred && !late_kind(ai)) qparams_act(ai);
    }
    // launch_resid_fq_lnstats (Y = the output of quantizer ai_Y, -1: none; x_new: the rows of `next`, or nullptr where they stand already) leaves the row
    // statistics of the LayerNorm `next`, whose output quantizer is updated behind it
    int resid_lnstats(int mode, const float* x_prev, const float* Y, int ai_Y, const float* cls, const float* pos, float* x_new, const LnRows& next,
                      void* maskbits = nullptr, const float* drop_scale_rows = nullptr, const float* ls_gamma_cols = nullptr) const {
        const bool lt = ai_Y >= 0 && late_kind(ai_Y);
        const QpLate L = lt ? late(ai_Y) : QpLate{};
        if (launch_resid_fq_lnstats(mode, x_prev, Y, act_qp(ai_Y >= 0 ? ai_Y : 0), c.act_qmin, c.act_qmax, cls, pos, x_new, next.mean, next.rstd, next.gamma, next.beta,
                                    c.ln_eps, act_stats(next.ai), kStatSlots, d.M, d.D, d.T, st, maskbits, lt ? &L : nullptr, drop_scale_rows, ls_gamma_cols))
            return 1;
        qparams_after(next.ai, true);
        return 0;
    }
    // launch_ln_apply_quant for the LayerNorm r
    int ln_apply(const LnRows& r, void* out16, void* out8) const {
        const bool lt = late_kind(r.ai);
        const QpLate L = lt ? late(r.ai) : QpLate{};
        // a QATVIT_FWD_X16 forward whose backward takes the byte plane (k_gemm_tn_q8) writes no 2-byte plane at all: the forward GEMM reads out8 too
        const bool x16 = (flags & QATVIT_FWD_X16) != 0;
        return launch_ln_apply_quant(r.x, r.mean, r.rstd, r.gamma, r.beta, act_qp(r.ai), c.act_qmin, c.act_qmax, x16 && p.form.x_plane_from_q8 ? nullptr : out16,
                                     d.M, d.D, st, p.form.i8 ? out8 : nullptr, center(), x16, lt ? &L : nullptr);
    }
    // the same LayerNorm as the prologue of the statistics pass of layer wi (ln_in_strip_of): the pass builds the int8 plane out8 and reads it from its own LDS
    bool ln_in_strip(int kind) const { return ln_in_strip_of(p, d, flags, kind); }
    int linear_stats_ln(const LnRows& r, void* out8, int M, int wi, const float* bias, int ai_out, bool late_strip) const {
        const NTGemm g = grid_request(M, wi, out8, act_qp(r.ai), bias, ai_out);   // (A: the plane the pass itself writes)
        {
            ProfScope ps(prof, 7, 0.0, st);
            const QpLate L = late(r.ai);
            const StripLn ln{r.x, r.mean, r.rstd, r.gamma, r.beta, c.act_qmin, c.act_qmax, out8, &L};
            if (!late_kind(r.ai) || !launch_i8_strip_ln(g, ln, st)) {
                set_error("engine: the statistics pass with the LayerNorm prologue does not cover layer %d (M=%d N=%d K=%d)", wi, M, g.N, g.K);
                return 1;
            }
        }
        qparams_after(ai_out, true, late_strip);
        return 0;
    }
    void qparams_act(int ai) const {
        const qatvit_fq& f = act[ai];
        launch_qparams(act_stats(ai), f.min_val, f.max_val, f.scale, f.zero_point, f.observer_on, f.fake_quant_on, c.averaging_const,
                       c.act_qmin, c.act_qmax, 1, 0, act_qp(ai), 1, kStatSlots, st);
    }
    // The forward product of layer wi over M rows without its operands: C = (A . wq^T) * (*s_act) * s_w + bias, s_w the scalar s2 or (per-channel) the vector col_scale; stats -> act FQ `ai_out`
    NTGemm fwd_request(int M, int wi, const float* s_act = nullptr, const float* bias = nullptr, int ai_out = -1, float* C = nullptr) const {
        NTGemm g;
        wshape(d, wi, &g.N, &g.K);
        g.M = M; g.lda = g.ldb = g.K; g.ldc = g.N; g.C = C; g.s1 = s_act; g.bias = bias; g.stat_slots = kStatSlots;
        (c.w_per_channel ? g.col_scale : g.s2) = wfq[wi].scale;
        if (ai_out >= 0) g.stats = act_stats(ai_out);
        return g;
    }
    // ... on int8 operands (kNTI8): A8 = q - center, the weight integers with their row sums and, where the forward wrote it, their fragment-order copy
    NTGemm grid_request(int M, int wi, const void* A8, const float* a_qp, const float* bias, int ai_out, float* C = nullptr) const {
        NTGemm g = fwd_request(M, wi, a_qp, bias, ai_out, C);
        g.A = A8; g.B = at<void>(p.w8_off[wi]); g.B_frag = w8f(wi); g.wsum = at<int32_t>(p.wsum_off[wi]); g.a_qp = a_qp; g.center = center();
        return g;
    }
    // ... on bf16 operands (A_lo == nullptr: A holds grid integers; else A = A_hi + A_lo is a float operand)
    int linear_fwd(const void* A_hi, const void* A_lo, int M, int wi, const float* s_act, const float* bias, float* C, int ai_out,
                   const NTPost* post = nullptr, bool with_stats = true) const {
        NTGemm g = fwd_request(M, wi, s_act, bias, with_stats ? ai_out : -1, C);
        g.A = A_hi; g.A_lo = A_lo; g.B = at<void>(p.w_off[wi]);
        return fwd_launch(kNTBf16, g, post, A_lo ? 1 : 2, ai_out);
    }
    // THE launch of a forward request (a statistics-only pass is issued, not algorithmic, work), then the update of the quantizer ai_out that got its statistics
    int fwd_launch(NTForm form, const NTGemm& g, const NTPost* post, int kind, int ai_out, bool late_strip = false) const {
        {
            ProfScope ps(prof, kind, stats_only(post) ? 0.0 : 2.0 * g.M * g.N * g.K, st);
            if (launch_gemm_nt(form, g, post, st)) return 1;
        }
        qparams_after(ai_out, g.stats != nullptr, late_strip);
        return 0;
    }
    // the same product with the float A operand as an fp16 (hi, lo) pair scaled by *pair_scale (a device scalar its producer wrote) and the weight integers as fp16
    int linear_fwd_f16(const void* A16_hi, const void* A16_lo, const float* pair_scale, int M, int wi, const float* bias, float* C, int ai_out) const {
        NTGemm g = fwd_request(M, wi, pair_scale, bias, ai_out, C);
        g.A = A16_hi; g.A_lo = A16_lo; g.B = at<void>(p.w16_off[wi]);
        return fwd_launch(kNTF16, g, nullptr, 1, ai_out);
    }
    // the same product with the A operand as uint8 table indices [M, K] + the 256-entry table of fp16 pairs (fc2: gelu(fq(.)) takes <= 256 values)
    int linear_fwd_codes(const void* A8, const uint32_t* lut, const float* pair_scale, int M, int wi, const float* bias, float* C, int ai_out) const {
        NTGemm g = fwd_request(M, wi, pair_scale, bias, ai_out, C);
        g.A = A8; g.lut = lut; g.B = at<void>(p.w16_off[wi]);
        return fwd_launch(kNTCodes, g, nullptr, 1, ai_out);
    }
    int center() const { return (c.act_qmin + c.act_qmax + 1) / 2; }
    // the same forward product with int8 operands: A8 = q - center written next to the bf16 grid by its producer, weight integers + row sums
    // from k_w_quant_all.  Falls back to the bf16 form for shapes the int8 tile does not cover.
    // late_strip: the output quantizer's qparams are resolved by the strip kernel's code pass (the caller checked late_in_strip): the statistics pass
    // (post mode 3) then launches no k_qparams, the code pass gets the QpLate record
    int linear_fwd_grid(const void* A16, const void* A8, int M, int wi, const float* a_qp, const float* bias, float* C, int ai_out,
                        const NTPost* post = nullptr, bool with_stats = true, bool late_strip = false) const {
        int N, K; wshape(d, wi, &N, &K);
        if (!p.form.i8 || N % 384 != 0 || K % 64 != 0) return linear_fwd(A16, nullptr, M, wi, a_qp, bias, C, ai_out, post, with_stats);
        NTGemm g = grid_request(M, wi, A8, a_qp, bias, with_stats ? ai_out : -1, C);
        const bool code_pass = late_strip && post && !stats_only(post);
        const QpLate L = code_pass ? late(ai_out) : QpLate{};
        if (code_pass) g.late = &L;
        return fwd_launch(kNTI8, g, post, prof_kind_fwd(post), ai_out, late_strip);
    }
    // the int8 weight of layer wi in fragment order (the strip kernel's B operand), where the forward wrote it
    void* w8f(int wi) const { return p.form.i8 && p.form.w_batched && p.w8f_off[wi] >= 0 ? at<void>(p.w8f_off[wi]) : nullptr; }
    // will the strip kernel's code pass (post2) be the consumer of quantizer-of-layer-wi's statistics?  (then it resolves the qparams itself)
    bool late_in_strip(int M, int wi, const NTPost* post2) const {
        NTGemm g = fwd_request(M, wi); g.B_frag = w8f(wi);
        return p.form.late && i8_strip_covers(g, post2);
    }
    // qkv (kind WB_QKV) or fc1 (WB_FC1) of block i as TWO passes of the same kernel on the same operands, so the same bits: the statistics pass only feeds the
    // observer (min / max, nothing stored; with the LayerNorm in its prologue where ln_in_strip says so), the code pass quantises with the fresh qparams in its
    // epilogue post2.  Where the strip kernel's code pass resolves the output quantizer's qparams itself there is no k_qparams launch between the passes
    int two_pass(int i, int kind, const NTPost& post2) const {
        const bool fc1 = kind == WB_FC1;
        const LnRows r = fc1 ? norm2(i) : norm1(i);
        const void* A16 = blk<void>(fc1 ? p.h2q : p.h1q, i);
        void* A8 = blk<void>(fc1 ? p.h2q8 : p.h1q8, i);
        const int M = (int)d.M, wi = widx(i, kind), ai_out = aidx(i, fc1 ? AB_FC1 : AB_QKV);
        const float* bias = bprm(i, fc1 ? B_FC1B : B_QKVB);
        const bool lt = late_in_strip(M, wi, &post2);
        if (ln_in_strip(kind)) {
            if (linear_stats_ln(r, A8, M, wi, bias, ai_out, lt)) return 1;
        } else {
            const NTPost post1 = nt_post_stats();
            if (linear_fwd_grid(A16, A8, M, wi, act_qp(r.ai), bias, nullptr, ai_out, &post1, true, lt)) return 1;
        }
        return linear_fwd_grid(A16, A8, M, wi, act_qp(r.ai), bias, nullptr, ai_out, &post2, false, lt);
    }
    // the per-channel weight scale of layer wi, which its dY producer folds in (nullptr for per-tensor)
    const float* dy_colscale(int wi) const { return c.w_per_channel ? wfq[wi].scale : nullptr; }
    // dgrad: dX[M,K] = dY[M,N] . W_fq[N,K] from the transposed weight; *s1 = the per-tensor weight scale (per-channel: dY already carries s_w[n]).  The request without its operands:
    NTGemm dgrad_request(int M, int wi, float* dX = nullptr) const {
        NTGemm g;
        wshape(d, wi, &g.K, &g.N);
        g.M = M; g.lda = g.ldb = g.K; g.ldc = g.N; g.C = dX; if (!c.w_per_channel) g.s1 = wfq[wi].scale;
        return g;
    }
    // The weight-gradient request of layer wi without its operands: dW[N,K] += sum_m dY[m,N] X[m,K] * s_x under the weight FQ's STE mask, db[N] += sum_m dY;
    // dy_scaled: dY carries the per-channel weight scale s_w[n] (folded in for the dgrad), row_div takes it out again
    TNGemm wgrad_request(int wi, float* dW, float* db, bool dy_scaled = true) const {
        const qatvit_fq& f = wfq[wi];
        TNGemm g;
        wshape(d, wi, &g.N, &g.Kw);
        g.ldp = g.N; g.ldq = g.Kw; g.ldc = g.Kw; g.C = dW; g.dbias = db;
        g.W = prm(wparam(d, wi)); g.w_scale = f.scale; g.w_zp = f.zero_point;
        g.row_div = (c.w_per_channel && dy_scaled) ? f.scale : nullptr;
        return g;
    }
    // ... and what the weight gradients over M token rows share; the per-GEMM launches split through tn_scratch (two-phase, bit-reproducible)
    TNCall wgrad_call(int M) const {
        TNCall k;
        k.M = M; k.center = center(); k.w_per_channel = c.w_per_channel; k.w_qmin = c.w_qmin; k.w_qmax = c.w_qmax;
        k.scratch = at<float>(p.tn_scratch); k.scratch_bytes = kTnScratchBytes;
        return k;
    }
};

// One transformer block of the forward, in four parts that each start where the stage-level parity tests inject the oracle's tensor (behind
// a fake-quantizer that would otherwise amplify upstream one-step flips): 0 = norm1 -> qkv GEMM; 1 = attention -> proj -> residual;
// 2 = norm2 -> fc1 -> GELU; 3 = fc2 -> residual.
static int fwd_block(const Ctx& x, int i, int parts, bool qkv_injected = false) {
    const Dims& d = x.d;
    const Plan& p = x.p;
    const Forms& F = p.form;
    const int qa = x.c.act_qmin, qb = x.c.act_qmax;
    const int M = (int)d.M;
    const Ctx::LnRows n1 = x.norm1(i), n2 = x.norm2(i);   // (n1.x = x_in[i], n2.x = x_mid[i])
    float* const scal16 = x.blk<float>(p.scal16, i);
    if (parts & 1) {   // ---- part 0: norm1 -> qkv   (every quantizer's observer / qparams update runs behind the producer of its statistics)
        if (!x.ln_in_strip(WB_QKV)) x.ln_apply(n1, x.blk<void>(p.h1q, i), x.blk<void>(p.h1q8, i));   // (else norm1's apply + quantise runs inside qkv's statistics pass)
        if (F.qkv_2pass) {
            NTPost p2{};
            p2.mode = kEpiQkvCodes; p2.qp = x.act_qp(x.aidx(i, AB_QKV)); p2.qmin = qa; p2.qmax = qb;
            p2.out8 = x.blk<void>(p.qkv8, i); p2.out8_mask = x.blk<void>(p.qkvm, i); p2.code_T = (int)d.T; p2.code_hd = (int)(d.D / d.H);
            if (x.two_pass(i, WB_QKV, p2)) return 1;
        } else if (x.linear_fwd_grid(x.blk<void>(p.h1q, i), x.blk<void>(p.h1q8, i), M, x.widx(i, WB_QKV), x.act_qp(n1.ai), x.bprm(i, B_QKVB), x.blk<float>(p.qkv, i),
                                     x.aidx(i, AB_QKV)))
            return 1;
    }
    if (parts & 2) {   // ---- part 1: attention -> proj -> residual (+ statistics of norm2)
        const bool from_codes = F.qkv_2pass && !qkv_injected;   // part 0 left the code plane (and ran the observer); an injected fp32 qkv takes the one-pass route
        if (launch_attn_fwd(from_codes ? nullptr : x.blk<float>(p.qkv, i), x.act_qp(x.aidx(i, AB_QKV)), qa, qb, d.B, d.T, d.H, d.D, x.blk<void>(p.O_hi, i),
                            x.blk<void>(p.O_lo, i), x.blk<float>(p.lse, i), x.st, F.f16_proj ? x.blk<void>(p.O16_hi, i) : nullptr,
                            F.f16_proj ? x.blk<void>(p.O16_lo, i) : nullptr, F.f16_proj ? scal16 : nullptr, F.attn_codes ? x.blk<void>(p.qkv8, i) : nullptr,
                            F.attn_codes ? x.blk<void>(p.qkvm, i) : nullptr))
            return 1;
        if (F.f16_proj) {
            if (x.linear_fwd_f16(x.blk<void>(p.O16_hi, i), x.blk<void>(p.O16_lo, i), scal16, M, x.widx(i, WB_PROJ), x.bprm(i, B_PROJB), x.blk<float>(p.Yproj, i),
                                 x.aidx(i, AB_PROJ)))
                return 1;
        } else if (x.linear_fwd(x.blk<void>(p.O_hi, i), x.blk<void>(p.O_lo, i), M, x.widx(i, WB_PROJ), nullptr, x.bprm(i, B_PROJB),
                                x.blk<float>(p.Yproj, i), x.aidx(i, AB_PROJ)))
            return 1;
        if (x.resid_lnstats(1, n1.x, x.blk<float>(p.Yproj, i), x.aidx(i, AB_PROJ), nullptr, nullptr, n2.x, n2, x.blk<void>(p.mproj, i), x.drop_row(i, 0), x.ls_gamma(i, 0))) return 1;
    }
    if (parts & 4) {   // ---- part 2: norm2 -> fc1 (both passes) -> GELU
        if (!x.ln_in_strip(WB_FC1)) x.ln_apply(n2, x.blk<void>(p.h2q, i), x.blk<void>(p.h2q8, i));   // (else norm2's apply + quantise runs inside fc1's statistics pass)
        // fc1 is a K = D GEMM whose [M, 4D] fp32 output would be written once and read twice: run it TWICE instead.  Pass 1 only
        // feeds the observer (min/max, nothing stored); pass 2 - the same kernel on the same operands, so the same bits - quantises
        // with the fresh qparams and stores gelu(fq(.)) as the (hi, lo) pair fc2 reads plus a uint16 code (grid index | in-range
        // bit) for the backward.  The fp32 pre-FQ tensor and the separate fq+gelu pass (620 MB per block) disappear.
        NTPost p2{};
        p2.mode = kEpiCodes; p2.qp = x.act_qp(x.aidx(i, AB_FC1)); p2.qmin = qa; p2.qmax = qb;
        p2.out_hi = x.blk<void>(p.G_hi, i); p2.out_lo = x.blk<void>(p.G_lo, i); p2.code = x.blk<void>(p.Y1, i);
        if (F.fc2_codes) { p2.out8 = x.blk<void>(p.G8, i); p2.lut_out = x.blk<uint32_t>(p.glut, i); p2.out16_scale = scal16 + 1; }
        if (F.fc1_code_bits) { p2.code = nullptr; p2.out8_mask = x.blk<void>(p.Y1m, i); }   // the backward reads the byte plane + mask bits: no uint16 plane
        if (F.fc2w_codes) { p2.out_hi = p2.out_lo = nullptr; p2.lutq_out = x.blk<uint32_t>(p.glutq, i); }   // no 4-byte plane of gelu(fq(fc1)) at all
        else if (F.f16_fc2) { p2.out16_hi = x.at<void>(p.G16_hi); p2.out16_lo = x.at<void>(p.G16_lo); p2.out16_scale = scal16 + 1; }
        if (x.two_pass(i, WB_FC1, p2)) return 1;
    }
    if (parts & 8) {   // ---- part 3: fc2 -> residual (+ statistics of the next LayerNorm)
        if (F.fc2_codes) {
            if (x.linear_fwd_codes(x.blk<void>(p.G8, i), x.blk<uint32_t>(p.glut, i), scal16 + 1, M, x.widx(i, WB_FC2), x.bprm(i, B_FC2B), x.blk<float>(p.Y2, i),
                                   x.aidx(i, AB_FC2)))
                return 1;
        } else if (F.f16_fc2) {
            if (x.linear_fwd_f16(x.at<void>(p.G16_hi), x.at<void>(p.G16_lo), scal16 + 1, M, x.widx(i, WB_FC2), x.bprm(i, B_FC2B), x.blk<float>(p.Y2, i),
                                 x.aidx(i, AB_FC2)))
                return 1;
        } else if (x.linear_fwd(x.blk<void>(p.G_hi, i), x.blk<void>(p.G_lo, i), M, x.widx(i, WB_FC2), nullptr, x.bprm(i, B_FC2B), x.blk<float>(p.Y2, i),
                                x.aidx(i, AB_FC2)))
            return 1;
        // residual + statistics of the NEXT LayerNorm (block i+1's norm1, or the final norm)
        const Ctx::LnRows next = x.norm1(i + 1);
        if (x.resid_lnstats(1, n2.x, x.blk<float>(p.Y2, i), x.aidx(i, AB_FC2), nullptr, nullptr, next.x, next, x.blk<void>(p.m2, i), x.drop_row(i, 1), x.ls_gamma(i, 1))) return 1;
    }
    return 0;
}

// x_in[i] (the input of block i, or of the final norm for i == depth) or x_mid[i] - the rows of the LayerNorm r - was written into the workspace by the caller
// (teacher forcing in the stage-level parity tests): compute what the producer of that tensor would have left behind for its consumer - the row mean / rstd
// and the min/max of the LayerNorm output that the consumer's first fake-quant observes.
static int inject_ln_stats(const Ctx& x, const Ctx::LnRows& r) {
    launch_ws_init(x.act_stats(r.ai), kStatSlots * kStatStride / 2, x.st);   // whatever an earlier, unconsumed producer accumulated is stale
    return x.resid_lnstats(2, r.x, nullptr, -1, nullptr, nullptr, nullptr, r);
}
// one part of one block (fwd_block); `inject`: the part's input was written by the caller - part 0: x_in[block]; part 1: the pre-fake-quant
// qkv[block] (x_in[block] is read as it stands); part 2: x_mid[block]; part 3: the GELU output planes (G_hi / G_lo, and G16_hi / G16_lo with
// their scale when the fp16 path is on; x_mid[block] is read as it stands) - nothing to recompute for it
static int fwd_part(const Ctx& x, int block, int part, bool inject) {
    const Dims& d = x.d;
    const Plan& p = x.p;
    if (inject) {
        if (part == 0) {
            if (inject_ln_stats(x, x.norm1(block))) return 1;
        } else if (part == 1) {
            const int ai = x.aidx(block, AB_QKV);
            launch_ws_init(x.act_stats(ai), kStatSlots * kStatStride / 2, x.st);
            launch_minmax(x.blk<float>(p.qkv, block), 1, d.M * 3 * d.D, 0, x.act_stats(ai), kStatSlots, x.st);
            x.qparams_act(ai);
        } else if (part == 2) {
            if (inject_ln_stats(x, x.norm2(block))) return 1;
        }
    }
    return fwd_block(x, block, 1 << part, inject && part == 1);
}

// forward stages: 0 = weight preparation + input fake-quant + patch embedding (leaves x_in[0]); s in 1..depth = block s-1 (leaves
// x_in[s]); depth+1 = final norm + cls pooling + head + logits fake-quant.  `inject`: x_in[s_from - 1] was written by the caller.
static int fwd(const Ctx& x, const float* images, float* logits, int s_from, int s_to, bool inject) {
    const Dims& d = x.d;
    const Plan& p = x.p;
    const Forms& F = p.form;
    const qatvit_cfg& c = x.c;
    hipStream_t st = x.st;
    const int qa = c.act_qmin, qb = c.act_qmax;
    if (inject && s_from >= 1 && inject_ln_stats(x, x.norm1(s_from - 1))) return 1;
    if (s_from == 0) {
    // a forward from the start observes from empty accumulators: statistics a partial call (a stage range) produced for a consumer that never ran do not leak
    // into this step (the late-resolved quantizers' accumulators are re-armed by their consumer's commit, not behind their producer)
    if (F.late) launch_ws_init(x.at<uint32_t>(p.stats), (int64_t)d.n_act * kStatSlots * kStatStride / 2, st);
    // ---- weights: observe, qparams, integer operands (row-major and transposed) - all 50 tensors in three launches
    if (F.w_batched) {
        WObsTab to{};
        WQpTab tq{};
        WQuantTab tw{};
        to.n = tq.n = tw.n = d.n_w;
        tw.wT16 = 1;
        for (int wi = 0; wi < d.n_w && wi < 64; ++wi)
            if (x.wT16f_ok(wi)) tw.wT16f_mask |= 1ull << wi;
        to.per_channel = tq.per_channel = tw.per_channel = c.w_per_channel;
        to.nslots = tq.nslots = kStatSlots;
        tq.qmin = tw.qmin = c.w_qmin; tq.qmax = tw.qmax = c.w_qmax; tq.c = c.averaging_const;
        for (int wi = 0; wi < d.n_w; ++wi) {
            int N, K; wshape(d, wi, &N, &K);
            const qatvit_fq& f = x.wfq[wi];
            uint32_t* ws = x.at<uint32_t>(p.stats) + p.w_stats[wi];
            to.W[wi] = tw.W[wi] = x.prm(wparam(d, wi));
            to.ws[wi] = tq.ws[wi] = ws;
            to.N[wi] = tq.N[wi] = tw.N[wi] = N;
            to.K[wi] = tw.K[wi] = K;
            tq.rmin[wi] = f.min_val; tq.rmax[wi] = f.max_val; tq.scale[wi] = f.scale; tq.zp[wi] = f.zero_point;
            tq.obs_on[wi] = f.observer_on; tq.fq_on[wi] = f.fake_quant_on;
            tq.qp[wi] = x.w_qp(wi); tw.qp[wi] = x.w_qp(wi);
            tw.wq[wi] = x.at<void>(p.w_off[wi]); tw.wqT[wi] = x.at<void>(p.wT_off[wi]);
            tw.w8[wi] = F.i8 ? x.at<void>(p.w8_off[wi]) : nullptr;
            const bool w16 = p.w16_off[wi] >= 0 && ((wi - 1) % WB_COUNT == WB_PROJ ? F.f16_proj : F.f16_fc2);   // (w16_off: proj and fc2 only)
            tw.w16[wi] = w16 ? x.at<void>(p.w16_off[wi]) : nullptr;
            tw.w8f[wi] = x.w8f(wi);
            tw.wsum[wi] = F.i8 ? x.at<int32_t>(p.wsum_off[wi]) : nullptr;
        }
        if (F.i8) launch_zero_i32(x.at<int32_t>(p.wsum_base), p.wsum_bytes / 4, st);   // row sums are accumulated with integer atomics
        launch_w_observe_all(to, st);
        launch_w_qparams_all(tq, st);
        launch_w_quant_all(tw, st);
    } else {
        for (int wi = 0; wi < d.n_w; ++wi) {
            int N, K; wshape(d, wi, &N, &K);
            const qatvit_fq& f = x.wfq[wi];
            const float* W = x.prm(wparam(d, wi));
            uint32_t* ws = x.at<uint32_t>(p.stats) + p.w_stats[wi];
            launch_minmax(W, c.w_per_channel ? N : 1, c.w_per_channel ? K : (int64_t)N * K, c.w_per_channel, ws, kStatSlots, st);
            launch_qparams(ws, f.min_val, f.max_val, f.scale, f.zero_point, f.observer_on, f.fake_quant_on, c.averaging_const, c.w_qmin, c.w_qmax,
                           c.w_per_channel ? N : 1, 1, x.w_qp(wi), 1, c.w_per_channel ? 1 : kStatSlots, st);
            launch_wquant(W, x.w_qp(wi), c.w_per_channel, c.w_qmin, c.w_qmax, x.at<void>(p.w_off[wi]), x.at<void>(p.wT_off[wi]), N, K, st);
        }
    }
    // ---- input image FQ + patch rows
    launch_minmax(images, 1, (int64_t)d.B * d.chans * d.img * d.img, 0, x.act_stats(A_IN), kStatSlots, st);
    x.qparams_act(A_IN);
    if (launch_img_patches(images, x.at<void>(p.imgq), x.act_qp(A_IN), qa, qb, d.B, d.chans, d.img, d.img, d.patch, st,
                           F.i8 ? x.at<void>(p.imgq8) : nullptr, x.center()))
        return 1;
    if (x.linear_fwd_grid(x.at<void>(p.imgq), x.at<void>(p.imgq8), d.B * d.np, 0, x.act_qp(A_IN), x.prm(P_PE_B), x.at<float>(p.Y0), A_PE)) return 1;
    const Ctx::LnRows n0 = x.norm1(0);
    if (x.resid_lnstats(0, nullptr, x.at<float>(p.Y0), A_PE, x.prm(P_CLS), x.prm(P_POS), n0.x, n0)) return 1;
    }   // stage 0
    for (int i = (s_from < 1 ? 0 : s_from - 1); i < d.depth && i + 1 <= s_to; ++i)
        if (fwd_block(x, i, 15)) return 1;
    if (s_to < d.depth + 1) return 0;
    // ---- final norm (observer saw all tokens: updated behind the last block's residual kernel), cls pooling, head
    const Ctx::LnRows nf = x.norm1(d.depth);
    const int wh = d.n_w - 1;
    launch_head_fwd(nf.x, nf.mean, nf.rstd, nf.gamma, nf.beta, x.act_qp(nf.ai), qa, qb, x.at<void>(p.w_off[wh]), x.wfq[wh].scale, c.w_per_channel,
                    x.prm(x.p_tail() + 3), x.at<float>(p.hq), x.at<float>(p.logits_pre), x.act_stats(x.a_head()), kStatSlots, d.B, d.D, d.T, d.C, st);
    x.qparams_act(x.a_head());
    launch_logits_fq(x.at<float>(p.logits_pre), x.act_qp(x.a_head()), qa, qb, logits, d.B * d.C, st);
    return 0;
}

// ---- the backward.  stages: 0 = head + final norm; 1..depth = blocks depth-1..0; depth+1 = embedding
// `inject`: the gradient entering stage_from (dxA = d loss / d x_in[depth - stage_from + 1] for a block stage, / d x_in[0] for the embedding
// stage) was written by the caller; a block stage then rebuilds the masked copy of it that the previous stage's fused LayerNorm backward would
// have left for the fc2 weight / data gradient GEMMs.  (Every LayerNorm backward also emits the masked gradient of the branch output that precedes
// it - from the mask bits of the forward - so the stages of one call run in order; dxA carries over anyway.)
// x.flags & QATVIT_BWD_DY16: the one-plane form - every gradient that feeds a dgrad / wgrad pair (the masked residual gradient entering fc2 and proj,
// the fc1 and qkv output gradients) is ONE fp16 plane scaled by a power of two chosen from the previous backward's maxima (dy16.hip) instead of a bf16
// (hi, lo) pair: one MFMA pass and 2 B per element in eight GEMMs per block.  QATVIT_BWD_CALIBRATE: the pair form, recording those maxima.

// A gradient that feeds a dgrad / wgrad pair.  lo set: a bf16 (hi, lo) pair.  lo == nullptr: ONE fp16 plane in hi, scaled by the power of two of slot (block, slot)
// of the scale state (dy16.hip): its mul, amax and inv are Ctx::dy_mul, dy_slot and dy_inv of that slot (Bwd::mul / amax / inv)
struct Grad { void* hi; void* lo; int slot; };
// The layer input X of a weight gradient as the form at hand holds it; with the gradient's form it decides the TNForm (Bwd::wgrad)
struct WX { const void* hi; const void* lo; const void* q8; const void* codes; const uint32_t* lut; const float* scale; };
// grid integers with their quantizer: a 2-byte plane (bf16, one-plane form fp16) and - taken instead where k_gemm_tn_q8 applies - the same integers as q - center, one
// byte each (the forward's int8 operand)
static WX x_grid(const void* plane, const void* q8, const float* qp) { return WX{plane, nullptr, q8, nullptr, nullptr, qp}; }
// a float operand: split into a bf16 (hi, lo) pair, or (one-plane form, lo == nullptr) rounded to fp16 like dY itself, times *scale
static WX x_float(const void* hi, const void* lo, const float* scale) { return WX{hi, lo, nullptr, nullptr, nullptr, scale}; }
// uint8 table indices + a 256-entry table of pairs (fc2: X = gelu(fq(fc1 output))): fp16 pairs times *scale in the one-plane form, bf16 pairs in the pair form
static WX x_codes(const void* codes, const uint32_t* lut, const float* scale) { return WX{nullptr, nullptr, nullptr, codes, lut, scale}; }
struct LnGrads { float* dgamma; float* dbeta; };
// What the MLP and proj part of a block's backward reads and writes, over M rows: the full-height tensors of the Plan or, on the class-token rows (Bwd::cls), the
// gathered forward operands and [B, .] gradients of Plan::ClsRows.  (The qkv part of a block is full height always.)
struct BlockOps {
    bool cls_rows;
    int M;
    Grad gy, gh, gp;                                     // the masked gradient entering fc2, the fc1 output gradient, the masked gradient entering proj
    const void *G8, *Y1m, *h2q, *h2q8, *O16, *mproj;     // forward operands (O16: the attention output's fp16 hi plane)
    Ctx::LnRows n2;
    const float* dx;                                     // the gradient w.r.t. the block's output
    float *dxB, *dO, *dH;                                // ... w.r.t. x_mid, w.r.t. the attention output; the unfused fc1 dgrad's output
};

struct Bwd {
    const Ctx& x;
    void* const* grads;
    bool dy, cal;
    bool stream;   // deferred weight gradients (k_tn_stream): every block's gradient planes stay in the workspace, the GEMMs are collected here and run at the end of the call
    // The student pools the class token: the gradient entering the last block is zero outside the B rows b * T, a zero row of a dgrad operand gives a zero output
    // row and adds nothing to a weight gradient.  One-plane form with Forms::cls_bwd: head() leaves dx and the masked fc2-in plane as [B, .] (Plan::ClsRows),
    // and the last block - unless its input gradient was injected, which arrives as the full dxA - runs its MLP and proj backward on those B rows
    bool cls;
    float* dxA;    // the gradient w.r.t. the current block's OUTPUT at stage entry
    float* dxB;    // ... w.r.t. x_mid inside a block
    std::vector<TNGemm> sg[3];   // by TNForm: kTNPlaneQ8, kTNPlaneCodes, kTNPlaneF16
    double sflops[3] = {0.0, 0.0, 0.0};

    float* G(int i) const { return reinterpret_cast<float*>(grads[i]); }
    LnGrads dnorm1(int i) const { const int k = i < x.d.depth ? P_BLOCK0 + B_COUNT * i + B_N1W : x.p_tail(); return LnGrads{G(k), G(k + 1)}; }   // (depth: the final norm)
    LnGrads dnorm2(int i) const { const int k = P_BLOCK0 + B_COUNT * i + B_N2W; return LnGrads{G(k), G(k + 1)}; }
    // The gradient of slot `slot` (DS_*) of block blk_i in the form this call runs.  Pair form: the shared (hi, lo) buffers (fc2-in and proj-in are one pair).  One-plane
    // form: the hi buffer of that pair, or - where the weight gradients are deferred - the block's own planes [fc2-in | proj-in | fc1-out | qkv-out]; rows: the [B, .]
    // plane of the class-token rows
    Grad grad(int blk_i, int slot, bool rows = false) const {
        const Plan& p = x.p;
        if (rows) return Grad{x.at<void>(slot == DS_FC2 ? p.cls.dY : slot == DS_FC1 ? p.cls.dY1 : p.cls.dYp), nullptr, slot};
        void* hi = x.at<void>(slot == DS_FC1 ? p.dY1_hi : slot == DS_QKV ? p.dqkv_hi : p.dYs_hi);
        if (!dy) return Grad{hi, x.at<void>(slot == DS_FC1 ? p.dY1_lo : slot == DS_QKV ? p.dqkv_lo : p.dYs_lo), slot};
        if (stream) hi = x.at<char>(p.dyp) + (int64_t)blk_i * p.dyp_stride + (slot == DS_FC2 ? 0 : slot == DS_PROJ ? p.dyp_p : slot == DS_FC1 ? p.dyp_h : p.dyp_q);
        return Grad{hi, nullptr, slot};
    }
    const float* mul(int blk_i, const Grad& g) const { return g.lo ? nullptr : x.dy_mul(blk_i, g.slot); }
    uint32_t* amax(int blk_i, const Grad& g) const { return g.lo ? nullptr : x.dy_slot(blk_i, g.slot); }
    const float* inv(int blk_i, const Grad& g) const { return g.lo ? nullptr : x.dy_inv(blk_i, g.slot); }
    // calibration: the maximum of a tensor the pair form just wrote (its hi plane) into the tensor's slot
    void calib(const Grad& g, int64_t n, int blk_i) const { if (cal) launch_absmax_bf16(g.hi, n, x.dy_slot(blk_i, g.slot), x.st); }
    // What a LayerNorm backward leaves for the branch in front of it: g = split(dx_out * mask * colscale), the gradient entering layer wi of block blk_i (maskbits: the
    // forward's STE bits of that layer's output)
    // Under drop-path that gradient also carries the multipliers of the branch layer wi closes (proj: attention, fc2: MLP), one per sample: T rows each, or - rows -
    // one each on the compact class-token rows
    LnBwdNext next(int blk_i, const Grad& g, const void* maskbits, int wi, bool rows = false) const {
        LnBwdNext nx{maskbits, x.dy_colscale(wi), g.hi, g.lo, mul(blk_i, g), amax(blk_i, g)};
        nx.drop_scale = x.drop_row(blk_i, wi == x.widx(blk_i, WB_FC2) ? 1 : 0);
        nx.drop_rows = rows ? 1 : x.d.T;
        // Under LayerScale it carries that branch's gamma too, and the kernel that writes it completes gamma's gradient: from the residual gradient, the multipliers
        // and fq of the branch's pre-FQ output, which every block keeps (the compact class-token rows read it in place, every T-th row)
        const int mlp = wi == x.widx(blk_i, WB_FC2) ? 1 : 0;
        nx.ls_gamma = x.ls_gamma(blk_i, mlp);
        nx.ls_dgamma = x.ls_grad(blk_i, mlp);
        nx.ls_Y = x.blk<float>(mlp ? x.p.Y2 : x.p.Yproj, blk_i);
        nx.ls_ymul = rows ? x.d.T : 1;
        nx.ls_qp = x.act_qp(x.aidx(blk_i, mlp ? AB_FC2 : AB_PROJ));
        return nx;
    }
    // launch_ln_bwd_fq for the LayerNorm r over M rows (dx_in: the residual gradient it adds to where acc)
    int ln_bwd(int acc, const float* dH, const Ctx::LnRows& r, const LnGrads& dr, const float* dx_in, float* dx_out, int64_t M, int T, int cls_only,
               const LnBwdNext* nx, int rows_per_wave = 16) const {
        return launch_ln_bwd_fq(acc, dH, r.x, r.mean, r.rstd, r.gamma, r.beta, x.act_qp(r.ai), x.c.act_qmin, x.c.act_qmax, dx_in, dx_out, dr.dgamma, dr.dbeta, M, x.d.D, T,
                                cls_only, x.st, nx, rows_per_wave);
    }
    // NTPost mode 8: the dgrad GEMM into the output of the LayerNorm r runs that LayerNorm's backward in its epilogue (dx_in: the residual gradient it adds to) and
    // emits nx's masked gradient of the branch output in front of it
    NTPost lnb_post(const Ctx::LnRows& r, const LnGrads& dr, const float* dx_in, const LnBwdNext& nx) const {
        NTPost post{};
        post.mode = kEpiLnBwd; post.qp = x.act_qp(r.ai); post.qmin = x.c.act_qmin; post.qmax = x.c.act_qmax;
        post.lnb_x = r.x; post.lnb_mean = r.mean; post.lnb_rstd = r.rstd; post.lnb_gamma = r.gamma; post.lnb_beta = r.beta; post.lnb_dx_in = dx_in;
        post.lnb_dgamma = dr.dgamma; post.lnb_dbeta = dr.dbeta;
        post.lnb_nmask = nx.maskbits; post.colscale = nx.colscale; post.out_hi = nx.out_hi; post.out_lo = nx.out_lo;
        post.o16_mul = nx.o16_mul; post.o16_amax = nx.o16_amax;
        return post;
    }
    // NTPost mode 9: the fc2 dgrad of block i applies the GELU backward and fc1's STE mask from the forward's byte codes + mask bits: the fc1 output gradient gh
    NTPost gelu_post(int i, const Grad& gh, const void* G8, const void* Y1m) const {
        NTPost post{};
        post.mode = kEpiGeluBwdU8; post.qp = x.act_qp(x.aidx(i, AB_FC1)); post.qmin = x.c.act_qmin; post.qmax = x.c.act_qmax; post.colscale = x.dy_colscale(x.widx(i, WB_FC1));
        post.out_hi = gh.hi; post.out_lo = gh.lo; post.code8 = G8; post.code_mask = Y1m;
        post.o16_mul = mul(i, gh); post.o16_amax = amax(i, gh);
        return post;
    }
    BlockOps operands(int i, bool rows, RowMoveTab* gather) const;
    int wgrad(int i, int Mw, const Grad& g, int wi, const WX& X, bool cls_rows = false);
    int dgrad(int i, int Md, const Grad& g, int wi, float* dX, const NTPost* post) const;
    int dgrad_ln(int i, bool n2, const Ctx::LnRows& r, const Grad& g, const float* dx_in, float* dx_out, float* dH, const LnBwdNext& nx, int Md, bool cls_rows) const;
    int head(const float* dlogits);
    int block(int i, bool injected);
    int embed();
    int flush();
};

// The operand set of block i's MLP and proj backward.  rows: every forward operand moves to its gathered copy and the move is listed in *gather - one list, so
// what is gathered is what is read
BlockOps Bwd::operands(int i, bool rows, RowMoveTab* gather) const {
    const Dims& d = x.d;
    const Plan& p = x.p;
    const Plan::ClsRows& cr = p.cls;
    BlockOps o;
    o.cls_rows = rows;
    o.M = rows ? d.B : (int)d.M;
    o.gy = grad(i, DS_FC2, rows); o.gh = grad(i, DS_FC1, rows); o.gp = grad(i, DS_PROJ, rows);   // (gp: the same buffer as gy unless the weight gradients are deferred)
    o.G8 = x.blk<void>(p.G8, i); o.Y1m = x.blk<void>(p.Y1m, i); o.h2q = x.blk<void>(p.h2q, i); o.h2q8 = x.blk<void>(p.h2q8, i);
    o.O16 = x.blk<void>(p.O16_hi, i); o.mproj = x.blk<void>(p.mproj, i); o.n2 = x.norm2(i);
    o.dx = rows ? x.at<float>(cr.dx) : dxA;
    o.dxB = rows ? x.at<float>(cr.dxB) : dxB;
    o.dO = x.at<float>(rows ? cr.dO : p.dO);
    o.dH = x.at<float>(rows ? cr.dH : p.dH);
    gather->n = 0;
    if (!rows) return o;
    auto to_rows = [&](auto*& ptr, int64_t off, int64_t width) {
        gather->m[gather->n++] = RowMove{ptr, x.at<void>(off), width, (int)width};
        ptr = static_cast<std::remove_reference_t<decltype(ptr)>>(x.at<void>(off));
    };
    const int64_t mrow = ln_maskbits_bytes(1, d.D);
    const bool q8 = p.form.x_plane_from_q8;
    to_rows(o.G8, cr.G8, d.Hd);
    to_rows(o.Y1m, cr.Y1m, d.Hd / 8);
    to_rows(q8 ? o.h2q8 : o.h2q, cr.h2q, q8 ? d.D : d.D * 2);   // ONE buffer holds whichever plane the fc1 weight gradient reads
    o.h2q = o.h2q8 = q8 ? o.h2q8 : o.h2q;
    to_rows(o.n2.x, cr.x_mid, (int64_t)d.D * 4);
    to_rows(o.n2.mean, cr.mean2, 4);
    to_rows(o.n2.rstd, cr.rstd2, 4);
    to_rows(o.mproj, cr.mproj, mrow);
    to_rows(o.O16, cr.O16, (int64_t)d.D * 2);
    return o;
}

// The weight gradient of layer wi over Mw token rows from the gradient g of its output.  One-plane form: X as fp16 (grid integers; proj: the attention output rounded to
// fp16 like dY itself: one pass), as q - center bytes where k_gemm_tn_q8 applies, or codes + a table of fp16 pairs; where the weight gradients are deferred it is
// collected for one persistent launch per X form at the end of the call - unless it runs over the class-token rows: the deferred batch shares ONE token count
int Bwd::wgrad(int i, int Mw, const Grad& g, int wi, const WX& X, bool cls_rows) {
    const TNForm form = g.lo ? (X.codes ? kTNPairCodes : kTNPair) : (X.q8 && x.p.form.x_plane_from_q8) ? kTNPlaneQ8 : X.codes ? kTNPlaneCodes : kTNPlaneF16;
    const int pw = wparam(x.d, wi);
    TNGemm t = x.wgrad_request(wi, G(pw), G(pw + 1));   // (a layer's bias follows its weight in params[])
    t.P = g.hi; t.P_lo = g.lo; t.Q = form == kTNPlaneQ8 ? X.q8 : X.codes ? X.codes : X.hi; t.Q_lo = X.lo; t.lut = X.lut; t.s1 = X.scale; t.s2 = inv(i, g);
    const double flops = 2.0 * Mw * t.N * t.Kw;
    if (stream && !cls_rows) {
        sg[form].push_back(t);
        sflops[form] += flops;
        return 0;
    }
    ProfScope ps(x.prof, (X.codes || X.lo || wi == x.widx(i, WB_PROJ)) ? 6 : 3, flops, x.st);   // 6: X is a float operand, 3: grid integers
    TNCall call = x.wgrad_call(Mw);
    call.reduce_single = cls_rows;   // (B rows: the kernel's serial tail would be the run time)
    return launch_gemm_tn(form, t, call, x.st);
}

// dgrad of layer wi over Md rows: the fp16 plane against the transposed weight integers as fp16 (s2 undoes the plane's scale), or the bf16 pair against them as bf16
int Bwd::dgrad(int i, int Md, const Grad& g, int wi, float* dX, const NTPost* post) const {
    NTGemm r = x.dgrad_request(Md, wi, dX);
    r.A = g.hi; r.A_lo = g.lo; r.B = g.lo ? x.at<void>(x.p.wT_off[wi]) : x.wT16(wi); r.s2 = inv(i, g);
    ProfScope ps(x.prof, prof_kind_dgrad(post), 2.0 * Md * r.N * r.K, x.st);
    return launch_gemm_nt(g.lo ? kNTBf16 : kNTPlaneF16, r, post, x.st);
}

// THE dgrad into a LayerNorm output + that LayerNorm's backward, for block i's norm2 (n2: g = the fc1 output gradient) or norm1 (g = the qkv output gradient) over the
// rows r: dx_out = dx_in + the gradient w.r.t. r.x, and nx's masked gradient of the branch output in front of the LayerNorm (a record without an output: none).
// One GEMM with the LayerNorm backward in its epilogue (Forms::lnb), or the plain dgrad into dH and k_ln_bwd_fq.  On the class-token rows always the latter: two tiles of
// the fused epilogue, one wave per row in sequence, take 70 us; the plain dgrad and k_ln_bwd_fq with one row per wave a third of it
int Bwd::dgrad_ln(int i, bool n2, const Ctx::LnRows& r, const Grad& g, const float* dx_in, float* dx_out, float* dH, const LnBwdNext& nx, int Md, bool cls_rows) const {
    const int wi = x.widx(i, n2 ? WB_FC1 : WB_QKV);
    const LnGrads dr = n2 ? dnorm2(i) : dnorm1(i);
    if (x.p.form.lnb && !cls_rows) {
        const NTPost post = lnb_post(r, dr, dx_in, nx);
        return dgrad(i, Md, g, wi, dx_out, &post);
    }
    if (dgrad(i, Md, g, wi, dH, nullptr)) return 1;
    return ln_bwd(1, dH, r, dr, dx_in, dx_out, Md, x.d.T, 0, nx.out_hi ? &nx : nullptr, cls_rows ? 1 : 16);
}

int Bwd::head(const float* dlogits) {
    const Dims& d = x.d;
    const Plan& p = x.p;
    const qatvit_cfg& c = x.c;
    const int base = x.p_tail(), wh = d.n_w - 1, last = d.depth - 1;
    Ctx::LnRows nf = x.norm1(d.depth);
    launch_head_bwd(dlogits, x.at<float>(p.logits_pre), x.act_qp(x.a_head()), c.act_qmin, c.act_qmax, x.at<float>(p.hq), x.act_qp(nf.ai),
                    x.at<void>(p.w_off[wh]), x.prm(base + 2), x.wfq[wh].scale, x.wfq[wh].zero_point, c.w_per_channel, c.w_qmin, c.w_qmax,
                    G(base + 2), G(base + 3), x.at<float>(p.dh), d.B, d.D, d.C, x.st);
    const Grad gy = grad(last, DS_FC2, cls);   // the masked gradient entering the last block's fc2
    const void* m2 = x.blk<void>(p.m2, last);
    if (cls) {   // the same kernel on the gathered class-token rows ([B, D], T = 1): the same bits in those rows, and neither the full dxA nor the full plane is written
        const Plan::ClsRows& r = p.cls;
        const int64_t mrow = ln_maskbits_bytes(1, d.D);
        RowMoveTab t;
        t.n = 4;
        t.m[0] = RowMove{nf.x, x.at<void>(r.xF), (int64_t)d.D * 4, d.D * 4};
        t.m[1] = RowMove{nf.mean, x.at<void>(r.meanF), 4, 4};
        t.m[2] = RowMove{nf.rstd, x.at<void>(r.rstdF), 4, 4};
        t.m[3] = RowMove{m2, x.at<void>(r.m2), mrow, (int)mrow};
        if (launch_rows_gather(t, d.B, d.T, x.st)) return 1;
        nf.x = x.at<float>(r.xF); nf.mean = x.at<float>(r.meanF); nf.rstd = x.at<float>(r.rstdF);
        const LnBwdNext nx = next(last, gy, x.at<void>(r.m2), x.widx(last, WB_FC2), true);
        return ln_bwd(0, x.at<float>(p.dh), nf, dnorm1(d.depth), nullptr, x.at<float>(r.dx), d.B, 1, 0, &nx, 1);
    }
    const LnBwdNext nx = next(last, gy, m2, x.widx(last, WB_FC2));
    if (ln_bwd(0, x.at<float>(p.dh), nf, dnorm1(d.depth), nullptr, dxA, d.M, d.T, 1, &nx)) return 1;
    calib(gy, d.M * d.D, last);
    return 0;
}

// One block: the steps of its backward, once for both gradient forms (Grad).  MLP branch: [the masked fc2-in gradient, if the stage's input was injected]
// -> fc2 wgrad -> fc2 dgrad + GELU' + fc1's STE mask -> fc1 wgrad -> fc1 dgrad + norm2's backward (leaves dxB and the masked proj-in gradient).  Attention branch:
// proj wgrad -> proj dgrad -> attention backward -> qkv wgrad -> qkv dgrad + norm1's backward (leaves dxA and the next block's masked fc2-in gradient).  The pair form
// records the maximum of every gradient right behind its producer when calibrating.
// The MLP and proj part of the last block runs on the class-token rows (Bwd::cls): the same launchers over B rows of gathered operands (BlockOps); its three weight
// gradients run right here (the deferred batch shares ONE token count); dxB goes back to full height, zeros elsewhere, for the qkv dgrad, and the attention
// backward reads dO as [B, D] and sweeps the live query pair alone (dK, dV and the rest of the block are dense: every key and value reaches the class token)
int Bwd::block(int i, bool injected) {
    const Dims& d = x.d;
    const Plan& p = x.p;
    const Forms& F = p.form;
    hipStream_t st = x.st;
    const int qa = x.c.act_qmin, qb = x.c.act_qmax;
    const int M = (int)d.M;
    const bool rows = cls && i == d.depth - 1 && !injected;
    RowMoveTab gather;
    const BlockOps o = operands(i, rows, &gather);
    const Grad gq = grad(i, DS_QKV);   // the qkv output gradient
    const int w_fc2 = x.widx(i, WB_FC2), w_fc1 = x.widx(i, WB_FC1), w_proj = x.widx(i, WB_PROJ), w_qkv = x.widx(i, WB_QKV);
    float* const scal16 = x.blk<float>(p.scal16, i);
    if (rows && launch_rows_gather(gather, d.B, d.T, st)) return 1;
    // ---- MLP branch
    if (injected) {
        if (launch_mask_bwd(0, dxA, x.blk<float>(p.Y2, i), x.act_qp(x.aidx(i, AB_FC2)), qa, qb, x.dy_colscale(w_fc2), d.D, o.gy.hi, o.gy.lo, d.M * d.D, st, mul(i, o.gy),
                            amax(i, o.gy), x.drop_row(i, 1), d.T, x.ls_gamma(i, 1)))
            return 1;
        calib(o.gy, d.M * d.D, i);
    }
    const WX x_fc2 = dy             ? x_codes(o.G8, x.blk<uint32_t>(p.glut, i), scal16 + 1)
                     : F.fc2w_codes ? x_codes(o.G8, x.blk<uint32_t>(p.glutq, i), nullptr)
                                    : x_float(x.blk<void>(p.G_hi, i), x.blk<void>(p.G_lo, i), nullptr);
    if (wgrad(i, o.M, o.gy, w_fc2, x_fc2, rows)) return 1;
    {   // fc2 dgrad with the GELU backward + fc1's STE mask fused into its epilogue: dY1 = (dYs . W_fc2) * gelu'(fq(Y1)) * mask(Y1)
        NTPost post = gelu_post(i, o.gh, o.G8, o.Y1m);
        if (!F.fc1_code_bits) { post.mode = kEpiGeluBwdU16; post.code = x.blk<void>(p.Y1, i); post.code8 = post.code_mask = nullptr; }   // the Y1 slot holds the uint16 codes (pair form only: the one-plane form needs the code bits)
        bool strip = false;
        if (dy && x.wT16f_ok(w_fc2) && knobs().f16_strip) {   // the A-stationary strip form (f16strip.hip): the gradient plane fetched once for all four column tiles
            ProfScope ps(x.prof, 5, 2.0 * o.M * d.D * d.Hd, st);
            NTGemm g = x.dgrad_request(o.M, w_fc2);
            g.A = o.gy.hi; g.B_frag = x.wT16f(w_fc2); g.s2 = inv(i, o.gy);
            strip = launch_f16_strip_gelu_bwd(g, &post, st);
        }
        if (!strip && dgrad(i, o.M, o.gy, w_fc2, nullptr, &post)) return 1;
    }
    calib(o.gh, d.M * d.Hd, i);
    if (wgrad(i, o.M, o.gh, w_fc1, x_grid(o.h2q, o.h2q8, x.act_qp(o.n2.ai)), rows)) return 1;
    if (dgrad_ln(i, true, o.n2, o.gh, o.dx, o.dxB, o.dH, next(i, o.gp, o.mproj, w_proj, rows), o.M, rows)) return 1;
    // ---- attention branch (dxB = gradient w.r.t. x_mid)
    calib(o.gp, d.M * d.D, i);
    const WX x_proj = dy ? x_float(o.O16, nullptr, scal16) : x_float(x.blk<void>(p.O_hi, i), x.blk<void>(p.O_lo, i), nullptr);
    if (wgrad(i, o.M, o.gp, w_proj, x_proj, rows)) return 1;
    if (dgrad(i, o.M, o.gp, w_proj, o.dO, nullptr)) return 1;
    if (rows) {   // back to full height, zeros elsewhere, for the qkv dgrad's LayerNorm-1 epilogue (its dx_in): ONE streaming pass
        RowMoveTab t;
        t.n = 1;
        t.m[0] = RowMove{o.dxB, dxB, (int64_t)d.D * 4, d.D * 4};
        if (launch_rows_scatter(t, d.B, d.T, st)) return 1;
    }
    // The one-plane form reads the codes its forward saved, never the fp32 qkv.  (rows: dO stays [B, D] - only query row 0 of every image carries a gradient, so the
    // fused kernel sweeps the one query pair that holds it)
    if (launch_attn_bwd(dy ? nullptr : x.blk<float>(p.qkv, i), x.act_qp(x.aidx(i, AB_QKV)), qa, qb, d.B, d.T, d.H, d.D, x.blk<void>(p.O_hi, i), x.blk<void>(p.O_lo, i),
                        x.blk<float>(p.lse, i), x.at<float>(p.delta), o.dO, gq.hi, gq.lo, x.dy_colscale(w_qkv), st, F.attn_codes ? x.blk<void>(p.qkv8, i) : nullptr,
                        F.attn_codes ? x.blk<void>(p.qkvm, i) : nullptr, mul(i, gq), amax(i, gq), rows ? 1 : 0, rows))
        return 1;
    calib(gq, d.M * 3 * d.D, i);
    if (wgrad(i, M, gq, w_qkv, x_grid(x.blk<void>(p.h1q, i), x.blk<void>(p.h1q8, i), x.act_qp(x.aidx(i, AB_N1))))) return 1;
    // the next block's fc2-in gradient (its own plane when the weight gradients are deferred).  Block 0 emits no next-branch gradient; the one-plane form's fused
    // epilogue still wants a scale / maximum target: its own qkv slot, which nothing reads afterwards
    const LnBwdNext nx_fc2 = i > 0 ? next(i - 1, grad(i - 1, DS_FC2), x.blk<void>(p.m2, i - 1), x.widx(i - 1, WB_FC2))
                                   : LnBwdNext{nullptr, nullptr, nullptr, nullptr, mul(0, gq), amax(0, gq)};
    if (dgrad_ln(i, false, x.norm1(i), gq, dxB, dxA, x.at<float>(p.dH), nx_fc2, M, false)) return 1;
    if (i > 0) calib(grad(i - 1, DS_FC2), d.M * d.D, i - 1);
    return 0;
}

int Bwd::embed() {
    const Dims& d = x.d;
    const Plan& p = x.p;
    launch_embed_bwd(dxA, x.at<float>(p.Y0), x.act_qp(A_PE), x.c.act_qmin, x.c.act_qmax, G(P_POS), G(P_CLS), x.at<void>(p.dY0_hi), x.at<void>(p.dY0_lo), d.B,
                     d.T, d.D, x.st);
    // the patch embedding's weight gradient: a bf16 pair against the bf16 grid plane of the image patches.  No dgrad into the image, so dY0 is not pre-scaled by the
    // per-channel weight scale (dy_scaled = false)
    TNGemm g = x.wgrad_request(0, G(P_PE_W), G(P_PE_B), false);
    g.P = x.at<void>(p.dY0_hi); g.P_lo = x.at<void>(p.dY0_lo); g.Q = x.at<void>(p.imgq); g.s1 = x.act_qp(A_IN);
    ProfScope ps(x.prof, 3, 2.0 * d.B * d.np * g.N * g.Kw, x.st);
    return launch_gemm_tn(kTNPair, g, x.wgrad_call(d.B * d.np), x.st);
}

// the collected weight gradients: one persistent launch (+ its fix-up) per X form and <= 24 GEMMs
int Bwd::flush() {
    TNCall call = x.wgrad_call((int)x.d.M);
    call.scratch = x.at<float>(x.p.tn_stream); call.scratch_bytes = tn_stream_scratch_bytes();
    for (int m = kTNPlaneQ8; m <= kTNPlaneF16; ++m) {
        for (size_t o = 0; o < sg[m].size(); o += kTnStreamMax) {
            const int n = (int)std::min<size_t>(kTnStreamMax, sg[m].size() - o);
            ProfScope ps(x.prof, m == kTNPlaneQ8 ? 3 : 6, sflops[m] * n / (double)sg[m].size(), x.st);
            if (launch_tn_stream((TNForm)m, sg[m].data() + o, n, call, x.st)) return 1;
        }
    }
    return 0;
}

static int bwd(const Ctx& x, const float* dlogits, void* const* grads, int stage_from, int stage_to, bool inject) {
    const Dims& d = x.d;
    const Forms& F = x.p.form;
    const bool dy = (x.flags & QATVIT_BWD_DY16) != 0, cal = (x.flags & QATVIT_BWD_CALIBRATE) != 0;
    if (dy && cal) { set_error("student backward: QATVIT_BWD_DY16 and QATVIT_BWD_CALIBRATE exclude each other"); return 1; }
    if ((dy || cal) && !F.dy16) { set_error("student backward: the one-plane form does not cover this configuration (qatvit_student_dy16_supported)"); return 1; }
    Bwd b{x, grads, dy, cal, dy && F.tn_stream && F.x_plane_from_q8, dy && F.cls_bwd, x.at<float>(x.p.dxA), x.at<float>(x.p.dxB)};
    uint32_t* const dystate = x.at<uint32_t>(x.p.dy16);
    const int nslots = DS_COUNT * d.depth;
    if ((dy || cal) && (stage_from == 0 || inject)) launch_dy16_begin(dystate, nslots, stage_from == 0 ? dlogits : nullptr, d.B * d.C, x.st);
    for (int s = stage_from; s <= stage_to; ++s) {
        const bool injected = inject && s == stage_from;
        if (s == 0 ? b.head(dlogits) : s > d.depth ? b.embed() : b.block(d.depth - s, injected)) return 1;
    }
    // (the scale bookkeeping and the overflow flag first: they depend on the producers of the planes only, and the host's mirror of the flag - qatvit_student_dy16_set_mirror -
    //  is written here, 2 - 3 ms before the deferred weight gradients are done)
    if (dy || cal) launch_dy16_end(dystate, nslots, dy ? 1 : 0, x.st);
    return b.flush();
}

}  // namespace qv

using namespace qv;

extern "C" {

int64_t qatvit_student_workspace_bytes(const qatvit_cfg* cfg) {
    if (!cfg || check_cfg(*cfg)) return -1;
    Plan p;
    if (make_plan(*cfg, &p)) return -1;
    return p.total;
}

int32_t qatvit_student_num_params(const qatvit_cfg* cfg) { return cfg ? P_BLOCK0 + B_COUNT * cfg->depth + 4 : -1; }
int32_t qatvit_student_num_act_fq(const qatvit_cfg* cfg) { return cfg ? 2 + AB_COUNT * cfg->depth + 2 : -1; }
int32_t qatvit_student_num_weight_fq(const qatvit_cfg* cfg) { return cfg ? 1 + WB_COUNT * cfg->depth + 1 : -1; }

int qatvit_student_init(const qatvit_cfg* cfg, void* workspace, void* stream) {
    QV_CHECK_ARG(cfg && workspace, "qatvit_student_init: null argument");
    if (check_cfg(*cfg)) return 1;
    Plan p;
    if (make_plan(*cfg, &p)) return 1;
    {   // a timing session keyed by this address belongs to whatever was bound to it before
        std::lock_guard<std::mutex> lk(g_prof_mu);
        auto it = g_profs.find(workspace);
        if (it != g_profs.end()) { std::lock_guard<std::mutex> l2(it->second->mu); it->second->closed = true; }
        g_profs.erase(workspace);
    }
    drop_path_bind(workspace, nullptr);   // ... and so do a drop-path table and a LayerScale binding
    layer_scale_bind(workspace, 0, nullptr, nullptr, nullptr);
    launch_ws_init(reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(workspace) + p.stats), p.stats_words / 2, (hipStream_t)stream);
    // the one-plane backward's scale history starts empty (the first backward on a workspace calibrates); no late-resolved quantizer state is pending
    launch_zero_i32(reinterpret_cast<int32_t*>(reinterpret_cast<char*>(workspace) + p.dy16), dy16_state_bytes(DS_COUNT * cfg->depth) / 4, (hipStream_t)stream);
    launch_zero_i32(reinterpret_cast<int32_t*>(reinterpret_cast<char*>(workspace) + p.qp_staged), (int64_t)dims_of(*cfg).n_act * kQpStagedWords, (hipStream_t)stream);
    QV_CHECK_LAUNCH("qatvit_student_init");
    return 0;
}

static int run_forward(const qatvit_cfg* cfg, void* const* params, const qatvit_fq* act_fq, const qatvit_fq* weight_fq, const float* images,
                       float* logits, void* workspace, int32_t stage_from, int32_t stage_to, int32_t flags, void* stream, const char* who) {
    QV_CHECK_ARG(cfg && params && act_fq && weight_fq && workspace, "%s: null argument", who);
    if (check_cfg(*cfg)) return 1;
    QV_CHECK_ARG(stage_from >= 0 && stage_to <= cfg->depth + 1 && stage_from <= stage_to, "%s: bad stage range [%d,%d]", who, stage_from, stage_to);
    QV_CHECK_ARG(stage_from > 0 || images, "%s: stage 0 needs the images", who);
    QV_CHECK_ARG(stage_to <= cfg->depth || logits, "%s: the last stage needs the logits buffer", who);
    QV_CHECK_ARG((flags & ~(QATVIT_STAGE_INJECT | QATVIT_FWD_X16)) == 0 && !((flags & QATVIT_STAGE_INJECT) && stage_from == 0), "%s: bad flags %d", who, flags);
    Ctx x{*cfg, dims_of(*cfg), Plan(), reinterpret_cast<char*>(workspace), params, act_fq, weight_fq, (hipStream_t)stream, prof_of(workspace)};
    x.drop = drop_path_of(workspace);
    x.ls = layer_scale_of(workspace);
    QV_CHECK_ARG(!x.ls || (int)x.ls->gamma.size() == 2 * cfg->depth, "student step: the LayerScale binding holds %d branches, depth is %d", (int)x.ls->gamma.size(), cfg->depth);
    if (make_plan(*cfg, &x.p, x.drop != nullptr || x.ls != nullptr)) return 1;
    x.flags = flags & QATVIT_FWD_X16;
    QV_CHECK_ARG(!x.flags || x.p.form.dy16, "%s: QATVIT_FWD_X16 needs a configuration the one-plane backward covers (qatvit_student_dy16_supported)", who);
    if (fwd(x, images, logits, stage_from, stage_to, (flags & QATVIT_STAGE_INJECT) != 0)) return 1;
    if (x.commit_late()) return 1;
    QV_CHECK_LAUNCH(who);
    return 0;
}

int qatvit_student_forward(const qatvit_cfg* cfg, void* const* params, const qatvit_fq* act_fq, const qatvit_fq* weight_fq, const float* images,
                           float* logits, void* workspace, void* stream) {
    QV_CHECK_ARG(cfg && images && logits, "qatvit_student_forward: null argument");
    return run_forward(cfg, params, act_fq, weight_fq, images, logits, workspace, 0, cfg->depth + 1, 0, stream, "qatvit_student_forward");
}

int qatvit_student_forward_stages(const qatvit_cfg* cfg, void* const* params, const qatvit_fq* act_fq, const qatvit_fq* weight_fq,
                                  const float* images, float* logits, void* workspace, int32_t stage_from, int32_t stage_to, int32_t flags,
                                  void* stream) {
    return run_forward(cfg, params, act_fq, weight_fq, images, logits, workspace, stage_from, stage_to, flags, stream, "qatvit_student_forward_stages");
}

int qatvit_student_forward_part(const qatvit_cfg* cfg, void* const* params, const qatvit_fq* act_fq, const qatvit_fq* weight_fq, void* workspace,
                                int32_t block, int32_t part, int32_t flags, void* stream) {
    QV_CHECK_ARG(cfg && params && act_fq && weight_fq && workspace, "qatvit_student_forward_part: null argument");
    if (check_cfg(*cfg)) return 1;
    QV_CHECK_ARG(block >= 0 && block < cfg->depth && part >= 0 && part <= 3 && (flags & ~(QATVIT_STAGE_INJECT | QATVIT_FWD_X16)) == 0,
                 "qatvit_student_forward_part: bad block %d / part %d / flags %d", block, part, flags);
    Ctx x{*cfg, dims_of(*cfg), Plan(), reinterpret_cast<char*>(workspace), params, act_fq, weight_fq, (hipStream_t)stream, prof_of(workspace)};
    x.drop = drop_path_of(workspace);
    x.ls = layer_scale_of(workspace);
    QV_CHECK_ARG(!x.ls || (int)x.ls->gamma.size() == 2 * cfg->depth, "student step: the LayerScale binding holds %d branches, depth is %d", (int)x.ls->gamma.size(), cfg->depth);
    if (make_plan(*cfg, &x.p, x.drop != nullptr || x.ls != nullptr)) return 1;
    x.flags = flags & QATVIT_FWD_X16;
    QV_CHECK_ARG(!x.flags || x.p.form.dy16, "qatvit_student_forward_part: QATVIT_FWD_X16 needs a configuration the one-plane backward covers");
    if (fwd_part(x, block, part, (flags & QATVIT_STAGE_INJECT) != 0)) return 1;
    if (x.commit_late()) return 1;
    QV_CHECK_LAUNCH("qatvit_student_forward_part");
    return 0;
}

static int run_backward(const qatvit_cfg* cfg, void* const* params, const qatvit_fq* act_fq, const qatvit_fq* weight_fq, const float* dlogits,
                        void* const* grads, void* workspace, int32_t stage_from, int32_t stage_to, int32_t flags, void* stream, const char* who) {
    QV_CHECK_ARG(cfg && params && act_fq && weight_fq && grads && workspace, "%s: null argument", who);
    if (check_cfg(*cfg)) return 1;
    QV_CHECK_ARG(stage_from >= 0 && stage_to <= cfg->depth + 1 && stage_from <= stage_to, "%s: bad stage range [%d,%d]", who, stage_from, stage_to);
    QV_CHECK_ARG(stage_from > 0 || dlogits, "%s: stage 0 needs dlogits", who);
    QV_CHECK_ARG((flags & ~(QATVIT_STAGE_INJECT | QATVIT_BWD_DY16 | QATVIT_BWD_CALIBRATE)) == 0 && !((flags & QATVIT_STAGE_INJECT) && stage_from == 0),
                 "%s: bad flags %d", who, flags);
    Ctx x{*cfg, dims_of(*cfg), Plan(), reinterpret_cast<char*>(workspace), params, act_fq, weight_fq, (hipStream_t)stream, prof_of(workspace)};
    x.drop = drop_path_of(workspace);
    x.ls = layer_scale_of(workspace);
    QV_CHECK_ARG(!x.ls || (int)x.ls->gamma.size() == 2 * cfg->depth, "student step: the LayerScale binding holds %d branches, depth is %d", (int)x.ls->gamma.size(), cfg->depth);
    if (make_plan(*cfg, &x.p, x.drop != nullptr || x.ls != nullptr)) return 1;
    x.flags = flags & (QATVIT_BWD_DY16 | QATVIT_BWD_CALIBRATE);
    QV_CHECK_ARG(!x.ls || !x.ls->grad.empty(), "%s: the LayerScale binding has no gradient buffers", who);
    if (bwd(x, dlogits, grads, stage_from, stage_to, (flags & QATVIT_STAGE_INJECT) != 0)) return 1;
    QV_CHECK_LAUNCH(who);
    return 0;
}

int qatvit_student_backward(const qatvit_cfg* cfg, void* const* params, const qatvit_fq* act_fq, const qatvit_fq* weight_fq, const float* dlogits,
                            void* const* grads, void* workspace, int32_t stage_from, int32_t stage_to, void* stream) {
    return run_backward(cfg, params, act_fq, weight_fq, dlogits, grads, workspace, stage_from, stage_to, 0, stream, "qatvit_student_backward");
}

int qatvit_student_backward_stages(const qatvit_cfg* cfg, void* const* params, const qatvit_fq* act_fq, const qatvit_fq* weight_fq,
                                   const float* dlogits, void* const* grads, void* workspace, int32_t stage_from, int32_t stage_to, int32_t flags,
                                   void* stream) {
    return run_backward(cfg, params, act_fq, weight_fq, dlogits, grads, workspace, stage_from, stage_to, flags, stream, "qatvit_student_backward_stages");
}

int32_t qatvit_student_ln_in_strip(const qatvit_cfg* cfg, int32_t flags) {
    if (!cfg || check_cfg(*cfg)) return 0;
    Plan p;
    if (make_plan(*cfg, &p)) return 0;
    const Dims d = dims_of(*cfg);
    return (ln_in_strip_of(p, d, flags, WB_QKV) ? 1 : 0) | (ln_in_strip_of(p, d, flags, WB_FC1) ? 2 : 0);
}

int32_t qatvit_student_dy16_supported(const qatvit_cfg* cfg) {
    if (!cfg || check_cfg(*cfg)) return 0;
    Plan p;
    if (make_plan(*cfg, &p)) return 0;
    return p.form.dy16 ? 1 : 0;
}

int qatvit_student_dy16_set_mirror(const qatvit_cfg* cfg, void* workspace, void* host_pinned, void* stream) {
    QV_CHECK_ARG(cfg && workspace, "qatvit_student_dy16_set_mirror: null argument");
    if (check_cfg(*cfg)) return 1;
    Plan p;
    if (make_plan(*cfg, &p)) return 1;
    if (launch_dy16_set_mirror(reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(workspace) + p.dy16), host_pinned, (hipStream_t)stream)) return 1;
    QV_CHECK_LAUNCH("qatvit_student_dy16_set_mirror");
    return 0;
}

int qatvit_student_dy16_to_pair(const qatvit_cfg* cfg, void* workspace, void* stream) {
    QV_CHECK_ARG(cfg && workspace, "qatvit_student_dy16_to_pair: null argument");
    if (check_cfg(*cfg)) return 1;
    Ctx x{*cfg, dims_of(*cfg), Plan(), reinterpret_cast<char*>(workspace), nullptr, nullptr, nullptr, (hipStream_t)stream, nullptr};
    if (make_plan(*cfg, &x.p)) return 1;
    for (int i = 0; i < x.d.depth; ++i) {
        if (x.p.form.x_plane_from_q8) {   // the X16 forward wrote the byte planes only: q - zp = q8 + center - zp as bf16 integers
            if (launch_q8_to_bf16int(x.blk<void>(x.p.h1q8, i), x.act_qp(x.aidx(i, AB_N1)), x.center(), x.blk<void>(x.p.h1q, i), x.d.M * x.d.D, x.st)) return 1;
            if (launch_q8_to_bf16int(x.blk<void>(x.p.h2q8, i), x.act_qp(x.aidx(i, AB_N2)), x.center(), x.blk<void>(x.p.h2q, i), x.d.M * x.d.D, x.st)) return 1;
            continue;
        }
        if (launch_f16int_to_bf16int(x.blk<void>(x.p.h1q, i), x.d.M * x.d.D, x.st)) return 1;
        if (launch_f16int_to_bf16int(x.blk<void>(x.p.h2q, i), x.d.M * x.d.D, x.st)) return 1;
    }
    QV_CHECK_LAUNCH("qatvit_student_dy16_to_pair");
    return 0;
}

// bench.py: time every launch of one GEMM class of ONE engine (identified by its workspace) with HIP events on the stream it is launched on
int qatvit_profile_start(const void* workspace, int32_t kind, int32_t max_launches) {
    QV_CHECK_ARG(workspace && kind >= 1 && kind <= 9 && max_launches > 0, "qatvit_profile_start: bad arguments");
    auto pr = std::make_shared<Prof>();
    pr->ev.assign((size_t)max_launches * 2, nullptr);
    for (auto& e : pr->ev)
        if (hipEventCreate(&e) != hipSuccess) {
            set_error("qatvit_profile_start: hipEventCreate failed");
            return 2;   // (~Prof destroys the events created so far)
        }
    pr->kind = kind;
    std::lock_guard<std::mutex> lk(g_prof_mu);
    auto it = g_profs.find(workspace);
    if (it != g_profs.end()) {   // restart: close the previous session of this engine (it dies with its last holder)
        std::lock_guard<std::mutex> l2(it->second->mu);
        it->second->closed = true;
    }
    g_profs[workspace] = pr;
    return 0;
}

int qatvit_profile_stop(const void* workspace, double* total_ms, int64_t* launches, double* flops) {
    QV_CHECK_ARG(workspace && total_ms && launches && flops, "qatvit_profile_stop: null argument");
    std::shared_ptr<Prof> pr;
    {
        std::lock_guard<std::mutex> lk(g_prof_mu);
        auto it = g_profs.find(workspace);
        if (it != g_profs.end()) { pr = it->second; g_profs.erase(it); }
    }
    QV_CHECK_ARG(pr, "qatvit_profile_stop: no profile is active for this workspace");
    size_t used;
    {
        std::lock_guard<std::mutex> lk(pr->mu);   // no forward / backward of this engine opens a bracket from here on; open ones finish on their own events
        pr->closed = true;
        used = pr->used;
        *flops = pr->flops;
    }
    double ms = 0.0;
    for (size_t i = 0; i + 1 < used; i += 2) {
        if (hipEventSynchronize(pr->ev[i + 1]) != hipSuccess) continue;   // (a bracket still open on another thread: its end event is not recorded yet)
        float t = 0.f;
        if (hipEventElapsedTime(&t, pr->ev[i], pr->ev[i + 1]) == hipSuccess) ms += t;
    }
    *total_ms = ms;
    *launches = (int64_t)(used / 2);
    return 0;
}

// debug/test access to intermediate tensors of the last forward/backward: byte offset of a named buffer
int64_t qatvit_student_tensor_offset(const qatvit_cfg* cfg, const char* name, int32_t block) {
    if (!cfg || !name || check_cfg(*cfg)) return -1;
    Plan p;
    if (make_plan(*cfg, &p)) return -1;
    struct { const char* n; int64_t off; bool per_block; } tab[] = {
        {"Y0", p.Y0, false}, {"imgq", p.imgq, false}, {"hq", p.hq, false}, {"logits_pre", p.logits_pre, false}, {"x_in", p.x_in, true},
        {"x_mid", p.x_mid, true}, {"h1q", p.h1q, true}, {"qkv", p.qkv, true}, {"O_hi", p.O_hi, true}, {"O_lo", p.O_lo, true}, {"Yproj", p.Yproj, true}, {"h2q", p.h2q, true},
        {"Y1", p.Y1, true}, {"G_hi", p.G_hi, true}, {"G_lo", p.G_lo, true}, {"Y2", p.Y2, true}, {"dxA", p.dxA, false}, {"dqkv_hi", p.dqkv_hi, false},
        {"dqkv_lo", p.dqkv_lo, false}, {"dO", p.dO, false},
        {"dH", p.dH, false}, {"lse", p.lse, true}, {"O16_hi", p.O16_hi, true}, {"O16_lo", p.O16_lo, true}, {"G16_hi", p.G16_hi, false},
        {"G16_lo", p.G16_lo, false}, {"scal16", p.scal16, true}, {"dy16", p.dy16, false}, {"dYs_hi", p.dYs_hi, false}, {"dY1_hi", p.dY1_hi, false}, {"G8", p.G8, true}, {"glut", p.glut, true}, {"Y1m", p.Y1m, true}, {"glutq", p.glutq, true}, {"qkv8", p.qkv8, true}, {"qkvm", p.qkvm, true},
    };
    for (auto& t : tab)
        if (strcmp(t.n, name) == 0) return t.off + (t.per_block ? p.blk_stride * block : 0);
    return -1;
}

}  // extern "C"
