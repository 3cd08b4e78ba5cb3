// The three row kernels of elt.hip through which a residual branch meets the residual stream - k_resid_fq_lnstats (forward), k_ln_bwd_fq's fused store and
// k_mask_bwd (backward).  elt.hip includes this text twice.  QV_DP 0: the kernels under their own names.  QV_DP 1: the same text as k_<name>_dp with two more
// arguments - dps, the branch's per-sample drop-path multipliers, and dp_rows, the rows per sample (T over [B * T, D] rows, 1 over the compact class-token
// rows [B, D]) - which multiply the branch by dps[row / dp_rows].  One text, so the two cannot drift apart; two kernels, so that the kernels without
// drop-path keep their names, their arguments and, instruction for instruction, their machine code (profiles/drop_path_bench.txt): a shared __device__ body
// inlined into both changed the existing kernels' code, a further template flag with a trailing argument their names and kernel-argument layout.
// The multiplier is wave-uniform; it is requested with the row's other loads, before anything is used.
// QV_DP 2: a third inclusion, k_<name>_ls - LayerScale.  The branch is also multiplied by lsg[column], the learnable per-channel gamma that stands between the
// branch's fake-quant and DropPath: x_new = x_prev + (fq(Y) * lsg[c]) * dps[sample], every product and the sum rounded separately.  lsg is required and loaded
// once per thread, like the LayerNorm gamma; dps may be null here (LayerScale without drop-path: multiplier 1, a wave-uniform select), so one variant serves
// both.  k_ln_bwd_fq_ls takes five more arguments (QV_LS_BWD_ARGS): it also produces lsg's gradient, see there.
#if QV_DP == 2
#define QV_LS 1
#define QV_ROWK(name) name##_ls
#define QV_DP_ARGS , const float* __restrict__ dps, int dp_rows, const float* __restrict__ lsg
#define QV_LS_BWD_ARGS , const float* __restrict__ lsY, int ls_ymul, const float* __restrict__ lsqp, int ls_kind, float* __restrict__ dls
#define QV_DP_LOAD(idx) (dps ? dps[idx] : 1.f)
#elif QV_DP
#define QV_LS 0
#define QV_ROWK(name) name##_dp
#define QV_DP_ARGS , const float* __restrict__ dps, int dp_rows
#define QV_LS_BWD_ARGS
#define QV_DP_LOAD(idx) dps[idx]
#else
#define QV_LS 0
#define QV_ROWK(name) name
#define QV_DP_ARGS
#define QV_LS_BWD_ARGS
#endif

// ---------------------------------------------------------------- residual + FQ + LN statistics
// MODE 0: x_new[b,0,:] = cls + pos[0];  x_new[b,1+p,:] = fq(Y[b*np+p,:]) + pos[1+p,:]
// MODE 1: x_new = x_prev + fq(Y)
// MODE 2: x_new = x_prev, nothing is stored (statistics of a residual-stream tensor the caller wrote: stage-level parity tests)
// then: mean/rstd of the x_new row and min/max of LN(x_new)*gamma+beta (the next aFQ's observer input).
// NV = column groups per lane (ceil(D / 256)).  All of a row's global loads are issued before anything is used (pin4, qv_device.h), without branches
// (a lane whose column is >= D loads column 0 and is masked out of the sums and stores): one `if (c < D)` region per column group made
// the compiler serialise the groups, i.e. two or three dependent HBM round trips per row.  gamma / beta are loaded once per thread.
// QV_DP (MODE 1): x_new = x_prev + fq(Y) * dps[sample] - behind the activation fake-quant of the proj / fc2 output and in front of the add, where the DropPath
// module stands in the prepared tree.  Product and sum are rounded separately, as the two stock ops round them (__fmul_rn: never one fused multiply-add),
// so equal fq(Y) gives bit-equal x_new and a multiplier of 1 gives the bits of the kernel without it.  The STE mask ballots are those of fq(Y), unchanged.
template <int MODE, int NV>
__global__ __launch_bounds__(256) void QV_ROWK(k_resid_fq_lnstats)(const float* __restrict__ x_prev, const float* __restrict__ Y, const float* __restrict__ qpY,
                                                          int qmin, int qmax, const float* __restrict__ cls, const float* __restrict__ pos,
                                                          float* __restrict__ x_new, float* __restrict__ mean, float* __restrict__ rstd,
                                                          const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                          uint32_t* __restrict__ stats, int stat_slots, int64_t M, int D, int T,
                                                          unsigned long long* __restrict__ maskbits, const QpLate late QV_DP_ARGS) {
    static_assert(!QV_DP || MODE == 1, "drop-path scales a residual branch");
    // maskbits (MODE 1, optional): the STE mask of fq(Y), one bit per element, as wave ballots - word [(row * NV + j) * 4 + e] holds in
    // bit `lane` the mask of column lane * 4 + 256 j + e.  k_ln_bwd_fq (same lane -> column mapping) reads it back with scalar loads,
    // so the backward never touches the fp32 Y again.
    // late.stats: the qparams of Y's quantizer are resolved here (qv_qparams.h QpLate) instead of by a k_qparams launch in front of this kernel
    __shared__ float sQp[4];
    QP q;
    if (late.stats) { const float4 r = qp_late_resolve(late, sQp); q = QP{r.x, r.y, r.z, r.w}; }
    else q = load_qp(qpY);
    const int lane = threadIdx.x & 63;
    bool act[NV];
    int cc[NV];
    float4 g[NV], bb[NV];
#if QV_LS
    float4 lsv[NV];   // the branch's LayerScale gamma: once per thread
#endif
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const int c = lane * 4 + 256 * j;
        act[j] = c < D;
        cc[j] = act[j] ? c : 0;
        g[j] = *reinterpret_cast<const float4*>(gamma + cc[j]);
        bb[j] = *reinterpret_cast<const float4*>(beta + cc[j]);
#if QV_LS
        lsv[j] = *reinterpret_cast<const float4*>(lsg + cc[j]);
#endif
    }
    float mn = INFINITY, mx = -INFINITY;
    for (int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); row < M; row += (int64_t)gridDim.x * 4) {
        const int t = (int)(row % T);
        const int64_t b = row / T;
        const bool is_cls = MODE == 0 && t == 0;                  // wave-uniform: the class token is added as it is
        const float* bsrc = MODE == 0 ? pos + (int64_t)t * D : x_prev + row * D;
        const float* ysrc = MODE == 0 ? (is_cls ? cls : Y + (b * (T - 1) + (t - 1)) * D) : MODE == 1 ? Y + row * D : bsrc;
        float4 yr[NV], base[NV], v[NV];
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            base[j] = *reinterpret_cast<const float4*>(bsrc + cc[j]);
            yr[j] = *reinterpret_cast<const float4*>(ysrc + cc[j]);
        }
#if QV_DP
        float sc = QV_DP_LOAD(row / dp_rows);
#endif
        // (pin the loaded values here: LLVM otherwise sinks each column group's loads down to its uses, one memory round trip per group)
#pragma unroll
        for (int j = 0; j < NV; ++j) { pin4(base[j]); pin4(yr[j]); }
#if QV_DP
        asm volatile("" : "+v"(sc));
#endif
        float s = 0.f;
        unsigned long long mb[NV][4];
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            bool i0, i1, i2, i3;
            float4 y = make_float4(fqv(yr[j].x, q, qmin, qmax, i0), fqv(yr[j].y, q, qmin, qmax, i1), fqv(yr[j].z, q, qmin, qmax, i2),
                                   fqv(yr[j].w, q, qmin, qmax, i3));
            if (is_cls) y = yr[j];
            if (MODE == 2) y = make_float4(0.f, 0.f, 0.f, 0.f);
            if (MODE == 1) {   // uniform control flow: the ballots stay in scalar registers
                mb[j][0] = __ballot(act[j] && i0); mb[j][1] = __ballot(act[j] && i1);
                mb[j][2] = __ballot(act[j] && i2); mb[j][3] = __ballot(act[j] && i3);
            }
#if QV_LS
            y = make_float4(__fmul_rn(y.x, lsv[j].x), __fmul_rn(y.y, lsv[j].y), __fmul_rn(y.z, lsv[j].z), __fmul_rn(y.w, lsv[j].w));
#endif
#if QV_DP
            y = make_float4(__fmul_rn(y.x, sc), __fmul_rn(y.y, sc), __fmul_rn(y.z, sc), __fmul_rn(y.w, sc));
#endif
            v[j] = make_float4(base[j].x + y.x, base[j].y + y.y, base[j].z + y.z, base[j].w + y.w);
            if (act[j]) s += (v[j].x + v[j].y) + (v[j].z + v[j].w);
        }
        // (stores after every load of the row has been consumed: vmcnt is in issue order, a store between two loads' uses is waited for)
#pragma unroll
        for (int j = 0; j < NV; ++j)
            if (MODE != 2 && act[j]) *reinterpret_cast<float4*>(x_new + row * D + cc[j]) = v[j];
        const float mu = wave_sum(s) / (float)D;
        float qq = 0.f;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            v[j].x -= mu; v[j].y -= mu; v[j].z -= mu; v[j].w -= mu;
            if (act[j]) qq += (v[j].x * v[j].x + v[j].y * v[j].y) + (v[j].z * v[j].z + v[j].w * v[j].w);
        }
        const float rs = rsqrtf(wave_sum(qq) / (float)D + eps);
        if (lane == 0) { mean[row] = mu; rstd[row] = rs; }
        if (MODE == 1 && maskbits && lane < 4) {   // lane e stores word e of every column group
#pragma unroll
            for (int j = 0; j < NV; ++j)
                maskbits[(row * NV + j) * 4 + lane] = lane == 0 ? mb[j][0] : lane == 1 ? mb[j][1] : lane == 2 ? mb[j][2] : mb[j][3];
        }
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            if (act[j]) {
                const float o0 = v[j].x * rs * g[j].x + bb[j].x, o1 = v[j].y * rs * g[j].y + bb[j].y, o2 = v[j].z * rs * g[j].z + bb[j].z,
                            o3 = v[j].w * rs * g[j].w + bb[j].w;
                mn = fminf(fminf(mn, o0), fminf(o1, fminf(o2, o3)));
                mx = fmaxf(fmaxf(mx, o0), fmaxf(o1, fmaxf(o2, o3)));
            }
        }
    }
    mn = wave_min(mn);
    mx = wave_max(mx);
    __shared__ float smn[4], smx[4];
    if (lane == 0) { smn[threadIdx.x >> 6] = mn; smx[threadIdx.x >> 6] = mx; }
    __syncthreads();
    const float bmn = fminf(fminf(smn[0], smn[1]), fminf(smn[2], smn[3])), bmx = fmaxf(fmaxf(smx[0], smx[1]), fmaxf(smx[2], smx[3]));
    if (threadIdx.x == 0) stat_atomic(stats, stat_slots, bmn, bmx);
}

// ---------------------------------------------------------------- GELU(fq(Y)) forward / backward (gelu_fwd / gelu_bwd: qv_common.h)
// GELU_BWD=0: dY = d * mask(Y);  GELU_BWD=1: dY = d * gelu'(fq(Y)) * mask(Y); optionally * col_scale[col]
// (per-channel weight scale of the consuming layer, folded here because dgrad's reduction runs over that axis).
// Output: the (hi, lo) bf16 pair both the dgrad and the wgrad GEMM read.
// QV_DP (GELU_BWD = 0): Y is a residual branch's output [rows, 4 * ncols4] under drop-path, and its gradient also carries dps[row / dp_rows] - what
// k_ln_bwd_fq's fused store computes on the paths that do not pass through here.
// QV_LS: ... and lsg[column], the branch's LayerScale gamma (gamma's own gradient is k_ln_bwd_fq_ls's, which produced d).
template <int GELU_BWD, bool O16 = false>
__global__ __launch_bounds__(256) void QV_ROWK(k_mask_bwd)(const float* __restrict__ d, const float* __restrict__ Y, const float* __restrict__ qp,
                                                  int qmin, int qmax, const float* __restrict__ col_scale, int ncols4,
                                                  __bf16* __restrict__ dst_hi, __bf16* __restrict__ dst_lo, int64_t n4,
                                                  const float* __restrict__ o16_mul, uint32_t* __restrict__ o16_amax QV_DP_ARGS) {
    static_assert(!QV_DP || GELU_BWD == 0, "drop-path scales a residual branch");
    const QP q = load_qp(qp);
    float mul = 1.f, am = 0.f;
    if constexpr (O16) mul = *o16_mul;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        const float4 v = reinterpret_cast<const float4*>(Y)[i];
        const float4 g = reinterpret_cast<const float4*>(d)[i];
        const float in4[4] = {v.x, v.y, v.z, v.w}, g4[4] = {g.x, g.y, g.z, g.w};
        float cs[4] = {1.f, 1.f, 1.f, 1.f};
        if (col_scale) {
            const float4 c = reinterpret_cast<const float4*>(col_scale)[i % ncols4];
            cs[0] = c.x; cs[1] = c.y; cs[2] = c.z; cs[3] = c.w;
        }
        float o[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            bool in;
            const float f = fqv(in4[e], q, qmin, qmax, in);
            o[e] = in ? (GELU_BWD ? g4[e] * gelu_bwd(f) : g4[e]) * cs[e] : 0.f;
        }
#if QV_DP
        const float sc = QV_DP_LOAD((i / ncols4) / dp_rows);
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] *= sc;
#endif
#if QV_LS
        {
            const float4 lg = reinterpret_cast<const float4*>(lsg)[i % ncols4];
            o[0] *= lg.x; o[1] *= lg.y; o[2] *= lg.z; o[3] *= lg.w;
        }
#endif
        if constexpr (O16) store_f16x4(dst_hi, i * 4, o[0], o[1], o[2], o[3], mul, am);
        else store_split4(dst_hi, dst_lo, i * 4, o[0], o[1], o[2], o[3]);
    }
    if constexpr (O16) amax_publish(o16_amax, am, threadIdx.x & 63);
}

// ---------------------------------------------------------------- LayerNorm backward with the aFQ mask of its output
// g_in = dH * mask(LN(x));  dx_out = (ACC ? dx_in : 0) + LNbwd(g_in);  dgamma/dbeta += column sums
// rows_sel: if non-null only rows listed there carry a gradient (final norm: cls tokens); others get dx_out = dx_in/0.
// NV = float4 column groups per lane (ceil(D / 256)): exact, so registers and the LDS column-sum staging scale with D
// FUSE: the residual-stream gradient this kernel produces is also the gradient of the NEXT (earlier) branch output; store it a second
// time as the (hi, lo) bf16 pair that branch's dgrad / wgrad GEMMs read, multiplied by that output's STE mask (the ballot words
// k_resid_fq_lnstats wrote in the forward) and the optional per-channel weight scale: what k_mask_bwd<0> would compute from a second
// read of dx_out and of the fp32 pre-FQ tensor.
// BF1: the fused next-branch gradient as ONE bf16 plane (nhi; the float step's bf16 form)
// QV_LS: the next branch was scaled by its LayerScale gamma lsg, so its gradient is dx_out * mask * colscale * dps[sample] * lsg[c] - and this kernel is where
// lsg's own gradient is complete: dls[c] += sum over rows of dx_out[row, c] * dps[sample] * B[row, c], B the branch output the forward scaled, WITHOUT the STE
// mask (d (fq(Y) * g) / dg = fq(Y) whether or not Y clamped).  B is read again from lsY (row `row * ls_ymul`: 1 over full-height rows, T over the compact
// class-token rows, whose Y stays where the forward left it): fq(Y) with the qparams lsqp (the QAT step keeps the pre-FQ Y of every block), or - lsqp null,
// the float forms - Y rounded as ls_kind says (0: fp32, 1: fp16, 2: bf16, the type stock autocast holds it in).  A dead row (cls_only) that carries a
// gradient (ACC) contributes too.  The sums travel through the sg staging array once dgamma / dbeta have left it: no LDS beyond the kernel without LayerScale.
template <int ACC, int NV, int WPB = 8, bool FUSE = false, bool O16 = false, bool BF1 = false>   // WPB waves per block: column sums meet in LDS, so more waves per block = same atomics, more rows in flight
__global__ __launch_bounds__(WPB * 64) void QV_ROWK(k_ln_bwd_fq)(const float* __restrict__ dH, int64_t dH_row_stride_rows, const float* __restrict__ x,
                                                   const float* __restrict__ mean, const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                   const float* __restrict__ beta, const float* __restrict__ qp, int qmin, int qmax,
                                                   const float* __restrict__ dx_in, float* __restrict__ dx_out, float* __restrict__ dgamma,
                                                   float* __restrict__ dbeta, int64_t M, int D, int T, int cls_only,
                                                   const unsigned long long* __restrict__ nmask, const float* __restrict__ ncs,
                                                   __bf16* __restrict__ nhi, __bf16* __restrict__ nlo, const float* __restrict__ o16_mul,
                                                   uint32_t* __restrict__ o16_amax QV_DP_ARGS QV_LS_BWD_ARGS) {
    static_assert((!O16 && !BF1) || (FUSE && !(O16 && BF1)), "the one-plane output is the fused next-branch gradient");
    static_assert(!QV_DP || FUSE, "drop-path scales the fused next-branch gradient");
#if QV_DP
    float sc = 1.f;   // this row's multiplier: a scalar load at the top of the row, with the mask words
#endif
    const QP q = load_qp(qp);
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    float mul16 = 1.f, am16 = 0.f;
    if constexpr (O16) mul16 = *o16_mul;
    unsigned long long mk[NV][4];   // this row's mask words (wave-uniform: scalar loads, requested at the top of the row)
    bool act[NV];
    int cc[NV];
    float4 gm[NV], bt[NV], csn[NV];   // gamma, beta, the next branch's per-column scale: once per thread
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const int c = lane * 4 + 256 * j;
        act[j] = c < D;
        cc[j] = act[j] ? c : 0;
        gm[j] = *reinterpret_cast<const float4*>(gamma + cc[j]);
        bt[j] = *reinterpret_cast<const float4*>(beta + cc[j]);
        csn[j] = FUSE && ncs ? *reinterpret_cast<const float4*>(ncs + cc[j]) : make_float4(1.f, 1.f, 1.f, 1.f);
    }
#if QV_LS
    float4 lsv[NV], al[NV];   // the next branch's LayerScale gamma (once per thread) and this lane's share of its gradient
    QP lq{};
    if (lsqp) lq = load_qp(lsqp);
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        lsv[j] = *reinterpret_cast<const float4*>(lsg + cc[j]);
        al[j] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    auto ls_branch = [&](float y) {   // B of one element
        bool in;
        return lsqp ? fqv(y, lq, qmin, qmax, in) : ls_kind == 1 ? (float)(_Float16)y : ls_kind == 2 ? (float)(__bf16)y : y;
    };
    auto ls_acc = [&](int j, const float4& o, const float4& y) {
        al[j].x += o.x * sc * ls_branch(y.x); al[j].y += o.y * sc * ls_branch(y.y); al[j].z += o.z * sc * ls_branch(y.z); al[j].w += o.w * sc * ls_branch(y.w);
    };
#endif
    auto fuse_store = [&](int64_t row, int j, int c, const float4& o) {
        const unsigned long long m0 = mk[j][0], m1 = mk[j][1], m2 = mk[j][2], m3 = mk[j][3];
        const float4 cs = csn[j];
#if QV_LS
        const float4 lg = lsv[j];
        const float f0 = ((m0 >> lane) & 1 ? o.x * cs.x : 0.f) * sc * lg.x, f1 = ((m1 >> lane) & 1 ? o.y * cs.y : 0.f) * sc * lg.y,
                    f2 = ((m2 >> lane) & 1 ? o.z * cs.z : 0.f) * sc * lg.z, f3 = ((m3 >> lane) & 1 ? o.w * cs.w : 0.f) * sc * lg.w;
#elif QV_DP
        const float f0 = ((m0 >> lane) & 1 ? o.x * cs.x : 0.f) * sc, f1 = ((m1 >> lane) & 1 ? o.y * cs.y : 0.f) * sc, f2 = ((m2 >> lane) & 1 ? o.z * cs.z : 0.f) * sc,
                    f3 = ((m3 >> lane) & 1 ? o.w * cs.w : 0.f) * sc;
#else
        const float f0 = (m0 >> lane) & 1 ? o.x * cs.x : 0.f, f1 = (m1 >> lane) & 1 ? o.y * cs.y : 0.f, f2 = (m2 >> lane) & 1 ? o.z * cs.z : 0.f,
                    f3 = (m3 >> lane) & 1 ? o.w * cs.w : 0.f;
#endif
        if constexpr (O16) store_f16x4(nhi, row * D + c, f0, f1, f2, f3, mul16, am16);
        else if constexpr (BF1) *reinterpret_cast<uint2*>(nhi + row * D + c) = make_uint2(pk_bf16(f0, f1), pk_bf16(f2, f3));
        else store_split4(nhi, nlo, row * D + c, f0, f1, f2, f3);
    };
    constexpr int nv = NV;
    float4 ag[NV], ab[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) ag[j] = ab[j] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int64_t row = (int64_t)blockIdx.x * WPB + wave; row < M; row += (int64_t)gridDim.x * WPB) {
        const bool live = !cls_only || (row % T) == 0;
        if (FUSE) {
#pragma unroll
            for (int j = 0; j < NV; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e) mk[j][e] = nmask[(row * NV + j) * 4 + e];
        }
#if QV_DP
        sc = QV_DP_LOAD(row / dp_rows);
#endif
        if (!live) {
            // no gradient reaches this token through the (cls-pooled) head
#pragma unroll
            for (int j = 0; j < NV; ++j) {
                if (act[j]) {
                    const float4 o = ACC ? *reinterpret_cast<const float4*>(dx_in + row * D + cc[j]) : make_float4(0.f, 0.f, 0.f, 0.f);
                    *reinterpret_cast<float4*>(dx_out + row * D + cc[j]) = o;
                    if (FUSE) fuse_store(row, j, cc[j], o);
#if QV_LS
                    if (ACC) ls_acc(j, o, *reinterpret_cast<const float4*>(lsY + row * ls_ymul * D + cc[j]));
#endif
                }
            }
            continue;
        }
        const float mu = mean[row], rs = rstd[row];
        const int64_t drow = cls_only ? row / T : row;  // dH is [B, D] for the cls-only case
        // every global load of the row first, branch-free (lanes past D read column 0 and are masked below), and pinned: see
        // k_resid_fq_lnstats - one `if (c < D)` region per column group serialised the groups' memory round trips
        float4 xv[NV], dvv[NV], pv[NV];
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            xv[j] = *reinterpret_cast<const float4*>(x + row * D + cc[j]);
            dvv[j] = *reinterpret_cast<const float4*>(dH + drow * D + cc[j]);
            if (ACC) pv[j] = *reinterpret_cast<const float4*>(dx_in + row * D + cc[j]);
        }
#if QV_LS
        float4 yv[NV];   // the next branch's output row
#pragma unroll
        for (int j = 0; j < NV; ++j) yv[j] = *reinterpret_cast<const float4*>(lsY + row * ls_ymul * D + cc[j]);
#endif
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            pin4(xv[j]);
            pin4(dvv[j]);
            if (ACC) pin4(pv[j]);
#if QV_LS
            pin4(yv[j]);
#endif
        }
        float4 xh[NV], gy[NV];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const float4 g = gm[j], b = bt[j];
            float4 dv = dvv[j];
            xh[j] = make_float4((xv[j].x - mu) * rs, (xv[j].y - mu) * rs, (xv[j].z - mu) * rs, (xv[j].w - mu) * rs);
            bool i0, i1, i2, i3;
            fqv(xh[j].x * g.x + b.x, q, qmin, qmax, i0);
            fqv(xh[j].y * g.y + b.y, q, qmin, qmax, i1);
            fqv(xh[j].z * g.z + b.z, q, qmin, qmax, i2);
            fqv(xh[j].w * g.w + b.w, q, qmin, qmax, i3);
            dv.x = i0 ? dv.x : 0.f; dv.y = i1 ? dv.y : 0.f; dv.z = i2 ? dv.z : 0.f; dv.w = i3 ? dv.w : 0.f;
            gy[j] = make_float4(dv.x * g.x, dv.y * g.y, dv.z * g.z, dv.w * g.w);
            if (act[j]) {
                ag[j].x += dv.x * xh[j].x; ag[j].y += dv.y * xh[j].y; ag[j].z += dv.z * xh[j].z; ag[j].w += dv.w * xh[j].w;
                ab[j].x += dv.x; ab[j].y += dv.y; ab[j].z += dv.z; ab[j].w += dv.w;
                s1 += (gy[j].x + gy[j].y) + (gy[j].z + gy[j].w);
                s2 += (gy[j].x * xh[j].x + gy[j].y * xh[j].y) + (gy[j].z * xh[j].z + gy[j].w * xh[j].w);
            }
        }
        const float m1 = wave_sum(s1) / (float)D, m2 = wave_sum(s2) / (float)D;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            float4 o = make_float4((gy[j].x - m1 - xh[j].x * m2) * rs, (gy[j].y - m1 - xh[j].y * m2) * rs,
                                   (gy[j].z - m1 - xh[j].z * m2) * rs, (gy[j].w - m1 - xh[j].w * m2) * rs);
            if (ACC) { o.x += pv[j].x; o.y += pv[j].y; o.z += pv[j].z; o.w += pv[j].w; }
            if (act[j]) {
                *reinterpret_cast<float4*>(dx_out + row * D + cc[j]) = o;
                if (FUSE) fuse_store(row, j, cc[j], o);
#if QV_LS
                ls_acc(j, o, yv[j]);
#endif
            }
        }
    }
    if constexpr (O16) amax_publish(o16_amax, am16, lane);
    // column sums: the block's waves through LDS, one atomic per column per block
    __shared__ float sg[WPB][256 * NV + 8], sb[WPB][256 * NV + 8];
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const int c = lane * 4 + 256 * j;
        if (j < nv && c < D) {
            sg[wave][c] = ag[j].x; sg[wave][c + 1] = ag[j].y; sg[wave][c + 2] = ag[j].z; sg[wave][c + 3] = ag[j].w;
            sb[wave][c] = ab[j].x; sb[wave][c + 1] = ab[j].y; sb[wave][c + 2] = ab[j].z; sb[wave][c + 3] = ab[j].w;
        }
    }
    __syncthreads();
    for (int c = threadIdx.x; c < D; c += WPB * 64) {
        float a = 0.f, b = 0.f;
#pragma unroll
        for (int w = 0; w < WPB; ++w) { a += sg[w][c]; b += sb[w][c]; }
        atomicAdd(&dgamma[c], a);
        atomicAdd(&dbeta[c], b);
    }
#if QV_LS
    __syncthreads();   // dgamma has left sg: the LayerScale sums take its place
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const int c = lane * 4 + 256 * j;
        if (j < nv && c < D) { sg[wave][c] = al[j].x; sg[wave][c + 1] = al[j].y; sg[wave][c + 2] = al[j].z; sg[wave][c + 3] = al[j].w; }
    }
    __syncthreads();
    for (int c = threadIdx.x; c < D; c += WPB * 64) {
        float a = 0.f;
#pragma unroll
        for (int w = 0; w < WPB; ++w) a += sg[w][c];
        atomicAdd(&dls[c], a);
    }
#endif
}

#undef QV_ROWK
#undef QV_DP_ARGS
#undef QV_LS_BWD_ARGS
#undef QV_LS
#ifdef QV_DP_LOAD
#undef QV_DP_LOAD
#endif
