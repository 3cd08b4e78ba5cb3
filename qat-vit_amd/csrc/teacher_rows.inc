// The residual + LayerNorm row kernel of the float forms.  teacher.hip includes this text twice (as elt.hip includes elt_rows.inc, and for its reasons): QV_DP 0 is
// k_resid_ln_split, QV_DP 1 the same text as k_resid_ln_split_dp with one more argument - dps, the per-sample drop-path multipliers of the residual branch - so
// that the kernel without drop-path keeps its name, arguments and machine code (profiles/drop_path_bench.txt).
// QV_DP (MODE 1): x = x_prev + Y * dps[row / T].  The pair form (and its STATS form): the product in fp32.  The fp16 form (f16) and the bf16 form (BF1): as stock
// autocast - Y and the multiplier are values of the 16-bit type, their product is rounded to that type (the fp32 product of two such values is exact: ONE
// rounding), the add is fp32.  The multiplier is wave-uniform and is requested with the row's other loads.
// QV_DP 2: a third inclusion, k_resid_ln_split_ls - LayerScale: x = x_prev + (B * lsg[column]) * dps[row / T], B = Y in the pair forms and Y rounded to the
// 16-bit type in the fp16 / bf16 forms.  lsg is the fp32 parameter, so stock type promotion makes the product fp32 and DropPath runs in fp32: neither the product
// nor the multiplier is rounded to the 16-bit type here (with the multiplier alone, above, both are).  dps may be null: LayerScale without drop-path.
#if QV_DP == 2
#define QV_ROWK(name) name##_ls
#define QV_DP_ARGS , const float* __restrict__ dps = nullptr, const float* __restrict__ lsg = nullptr
#elif QV_DP
#define QV_ROWK(name) name##_dp
#define QV_DP_ARGS , const float* __restrict__ dps = nullptr
#else
#define QV_ROWK(name) name
#define QV_DP_ARGS
#endif

// MODE 0: x[b,0,:] = cls + pos[0]; x[b,1+p,:] = Y[b*np+p,:] + pos[1+p,:]     MODE 1: x = x_prev + Y
// then h = LayerNorm(x) written as a (hi, lo) pair (one wave per row, row kept in registers: single pass over HBM)
// NV = ceil(D / 256) column groups per lane.  All loads of the row are issued first, branch-free and pinned (pin4; a lane past D reads column 0
// and is masked out): one `if (c < D)` region per group let LLVM sink each group's loads to its uses - three dependent HBM round trips
// per row at D = 768.  gamma / beta once per thread.
// STATS (the observe-only student forward): min / max of the fp32 LayerNorm outputs, one wave reduction and one accumulator atomic per wave
// (kStatSlots pairs); the instantiations without it are the teacher's and the float step's, unchanged.  BF1: h as ONE bf16 plane (st_split4).
template <int MODE, int NV, bool STATS = false, bool BF1 = false>
__global__ __launch_bounds__(256) void QV_ROWK(k_resid_ln_split)(const float* __restrict__ x_prev, const float* __restrict__ Y, const float* __restrict__ cls,
                                                        const float* __restrict__ pos, float* __restrict__ x_new, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, float eps, __bf16* __restrict__ h_hi,
                                                        __bf16* __restrict__ h_lo, int64_t M, int D, int T, int f16,
                                                        float* __restrict__ mean_out = nullptr, float* __restrict__ rstd_out = nullptr,
                                                        uint32_t* __restrict__ stats = nullptr QV_DP_ARGS) {
    static_assert(!QV_DP || MODE == 1, "drop-path scales a residual branch");
    const int lane = threadIdx.x & 63;
    float smn = INFINITY, smx = -INFINITY;
    bool act[NV];
    int cc[NV];
    float4 g[NV], bb[NV];
#if QV_DP == 2
    float4 lsv[NV];   // the branch's LayerScale gamma: once per thread
#endif
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const int c = lane * 4 + 256 * j;
        act[j] = c < D;
        cc[j] = act[j] ? c : 0;
        g[j] = *reinterpret_cast<const float4*>(gamma + cc[j]);
        bb[j] = *reinterpret_cast<const float4*>(beta + cc[j]);
#if QV_DP == 2
        lsv[j] = *reinterpret_cast<const float4*>(lsg + cc[j]);
#endif
    }
    for (int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); row < M; row += (int64_t)gridDim.x * 4) {
        const int t = (int)(row % T);
        const int64_t b = row / T;
        const float* ysrc = MODE == 0 ? (t == 0 ? cls : Y + (b * (T - 1) + (t - 1)) * D) : Y + row * D;   // (wave-uniform select)
        const float* bsrc = MODE == 0 ? pos + (int64_t)t * D : x_prev + row * D;
        float4 v[NV], y[NV];
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            v[j] = *reinterpret_cast<const float4*>(bsrc + cc[j]);
            y[j] = *reinterpret_cast<const float4*>(ysrc + cc[j]);
        }
#if QV_DP == 2
        float sc = dps ? dps[b] : 1.f;
#elif QV_DP
        float sc = dps[b];
#endif
#pragma unroll
        for (int j = 0; j < NV; ++j) { pin4(v[j]); pin4(y[j]); }
#if QV_DP == 2
        asm volatile("" : "+v"(sc));
        const int kind = BF1 ? 2 : f16 ? 1 : 0;
#pragma unroll
        for (int j = 0; j < NV; ++j)
            y[j] = make_float4(__fmul_rn(__fmul_rn(round_as(y[j].x, kind), lsv[j].x), sc), __fmul_rn(__fmul_rn(round_as(y[j].y, kind), lsv[j].y), sc),
                               __fmul_rn(__fmul_rn(round_as(y[j].z, kind), lsv[j].z), sc), __fmul_rn(__fmul_rn(round_as(y[j].w, kind), lsv[j].w), sc));
#elif QV_DP
        asm volatile("" : "+v"(sc));
        const int kind = BF1 ? 2 : f16 ? 1 : 0;   // (uniform) the type stock autocast holds the branch output in: bf16, fp16, or fp32
        sc = round_as(sc, kind);
#pragma unroll
        for (int j = 0; j < NV; ++j)
            y[j] = make_float4(round_as(__fmul_rn(round_as(y[j].x, kind), sc), kind), round_as(__fmul_rn(round_as(y[j].y, kind), sc), kind),
                               round_as(__fmul_rn(round_as(y[j].z, kind), sc), kind), round_as(__fmul_rn(round_as(y[j].w, kind), sc), kind));
#endif
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            v[j] = make_float4(v[j].x + y[j].x, v[j].y + y[j].y, v[j].z + y[j].z, v[j].w + y[j].w);
            if (act[j]) s += (v[j].x + v[j].y) + (v[j].z + v[j].w);
        }
#pragma unroll
        for (int j = 0; j < NV; ++j)
            if (act[j]) *reinterpret_cast<float4*>(x_new + row * D + cc[j]) = v[j];
        const float mu = wave_sum(s) / (float)D;
        float qq = 0.f;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            v[j].x -= mu; v[j].y -= mu; v[j].z -= mu; v[j].w -= mu;
            if (act[j]) qq += (v[j].x * v[j].x + v[j].y * v[j].y) + (v[j].z * v[j].z + v[j].w * v[j].w);
        }
        const float rs = rsqrtf(wave_sum(qq) / (float)D + eps);
        if (mean_out && lane == 0) { mean_out[row] = mu; rstd_out[row] = rs; }   // (the float student step's LayerNorm backward; the teacher passes nullptr)
        if constexpr (STATS) {
#pragma unroll
            for (int j = 0; j < NV; ++j)
                if (act[j]) {
                    const float o0 = v[j].x * rs * g[j].x + bb[j].x, o1 = v[j].y * rs * g[j].y + bb[j].y, o2 = v[j].z * rs * g[j].z + bb[j].z,
                                o3 = v[j].w * rs * g[j].w + bb[j].w;
                    smn = fminf(smn, fminf(fminf(o0, o1), fminf(o2, o3)));
                    smx = fmaxf(smx, fmaxf(fmaxf(o0, o1), fmaxf(o2, o3)));
                    st_split4<BF1>(h_hi, h_lo, row * D + cc[j], o0, o1, o2, o3, f16);
                }
        } else {
#pragma unroll
            for (int j = 0; j < NV; ++j)
                if (act[j])
                    st_split4<BF1>(h_hi, h_lo, row * D + cc[j], v[j].x * rs * g[j].x + bb[j].x, v[j].y * rs * g[j].y + bb[j].y, v[j].z * rs * g[j].z + bb[j].z,
                              v[j].w * rs * g[j].w + bb[j].w, f16);
        }
    }
    if constexpr (STATS) {
        smn = wave_min(smn);
        smx = wave_max(smx);
        if (lane == 0) stat_atomic(stats, kStatSlots, smn, smx);
    }
}

#undef QV_ROWK
#undef QV_DP_ARGS
