// The blur forms of the input pipeline (image_blur.hip includes this text once): Gaussian blur as Pillow's ImageFilter.GaussianBlur computes it
// (three box passes along the rows, three along the columns, every pass rounded to uint8, the edge pixel replicated; include/qatvit.h states the
// arithmetic) on the uint8 image behind the resize, between grayscale / solarize and the jitter ops of the colour record.
// Kernel text of its own, not a seventh switch of image_kernel.h: an output pixel of the blur depends on a 13 x 13 neighbourhood of the resized
// image, so the workgroup has to FORM that image - its band and up to kImgBlurHalo rows on each side - in LDS before anything behind the blur can
// run, where the other forms hand the vertical pass's integers straight to the value table.  One template, k_image_blur<DT, RRC, MIX, STAT>:
//   RRC    the source of a side is the window of its record (img_window), otherwise rows of the augmented image A through the word aug[b]
//   MIX    the band is formed once for the sample and, where it needs something of the partner, once more for the partner; each side is blurred
//          by its own record, coloured by its own record and erased by its own record before the blend or the box
//   STAT   the statistics launch: the chain up to the contrast op and the sum of the luma into sums[b]; no table, no output
// Per side, with (on, radius, ww, fw) = the cleaned blur record (img_blur):
//   on     rows e0 .. e1-1 = the band and 3 * (radius + 1) rows on each side, clamped to 0 .. D: staging and horizontal pass as the other forms,
//          the vertical pass of all these rows with grayscale / solarize into s_img[side] as planes [row][c][D] of bytes, six passes between
//          s_img[side] and s_pp (an even number: the result stands in s_img[side]), a barrier behind each.  A column pass clamps its taps to the
//          rows of the buffer: at the top and the bottom of the image that is Pillow's replicated edge; elsewhere it spoils (radius + 1) rows per
//          pass at the buffer's end, 3 * (radius + 1) in all, which is the halo.  The row passes have the whole width.
//   off    no halo row, no pass: e0 .. e1-1 is the band, and the store loop runs the colour forms' vertical pass with the whole chain.
// Every branch on a record is workgroup-uniform: the records come through scalar loads of words indexed by blockIdx.y.
// The band is the other forms' 16 rows without mix records (kImgBlurBand: 28 rows per buffer with the halo, two buffers) and 8 rows with them
// (kImgBlurMixBand: 20 rows per buffer, three buffers): 16-row bands with mix would need more than 64 KB at 32 -> 224.

// the blur record of one side, cleaned: "no blur" unless bit 0 is set, the radius is at most kImgBlurMaxRadius, 1 <= ww <= 2^24, fw >= 0 and
// (2 * radius + 1) * ww + 2 * fw <= 2^24.  Then ww * inner + fw * outer + 2^23 < 2^32 for sums of bytes, and every pass result is at most 255.
struct ImgBlur {
    bool on;
    int radius;
    uint32_t ww, fw;
};

__device__ __forceinline__ ImgBlur img_blur(const int32_t* __restrict__ rec) {
    ImgBlur v;
    const int w0 = rec[0], ww = rec[1], fw = rec[2];
    v.radius = (w0 >> 8) & 255;
    v.on = (w0 & 1) && v.radius <= kImgBlurMaxRadius && ww >= 1 && ww <= (1 << 24) && fw >= 0 && fw <= (1 << 23) &&
           (int64_t)(2 * v.radius + 1) * ww + 2 * (int64_t)fw <= (1 << 24);
    v.ww = (uint32_t)ww, v.fw = (uint32_t)fw;
    return v;
}

__device__ __forceinline__ ImgBlur img_blur_none() {
    ImgBlur v;
    v.on = false, v.radius = 0, v.ww = v.fw = 0u;
    return v;
}

// color == NULL with blur records: the all-zero colour record
__device__ __forceinline__ ImgColor img_color_none() {
    ImgColor c;
    c.op0 = c.op1 = c.op2 = kColNone;
    c.gray = c.solarize = c.contrast = c.any = false;
    c.threshold = c.mean = 0;
    c.fb = c.fc = c.fs = 0.0f;
    return c;
}

// a colour record split around the blur: its grayscale / solarize part, and its jitter ops
__device__ __forceinline__ ImgColor img_color_front(ImgColor c) {
    c.op0 = c.op1 = c.op2 = kColNone;
    c.any = c.gray || c.solarize;
    return c;
}

__device__ __forceinline__ ImgColor img_color_back(ImgColor c) {
    c.gray = c.solarize = false;
    c.any = c.op0 != kColNone || c.op1 != kColNone || c.op2 != kColNone;
    return c;
}

__device__ __forceinline__ uint32_t img_pack4(const int v[4]) {
    return __builtin_amdgcn_perm((uint32_t)(v[2] | v[3] << 16), (uint32_t)(v[0] | v[1] << 16), 0x06040200u);
}

// One box pass over planes [rows][3][D4] of dwords, src -> dst: one item = the four neighbouring pixels of one dword.  Along a row the ten taps
// x-2 .. x+5 of the item come from the dword, its left and its right neighbour (lanes read neighbouring dwords: no bank conflict); at the ends
// of the row the missing neighbour is the edge pixel four times.  Along a column they come from the same dword of the rows r-2 .. r+2, clamped
// to the buffer.  radius is 0 or 1: inner = the 2 * radius + 1 pixels around x, outer = the two at distance radius + 1.
__device__ __forceinline__ void img_blur_pass(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst, int rows, int D4, bool columns, const ImgBlur bl,
                                              int tid) {
    const int n = rows * 3 * D4, stride = 3 * D4;
    for (int it = tid; it < n; it += kImgThreads) {
        int o[4];
        if (!columns) {
            const int x4 = it % D4;
            const uint32_t cur = src[it];
            const uint32_t prev = x4 > 0 ? src[it - 1] : (cur & 255u) * 0x01010101u, next = x4 < D4 - 1 ? src[it + 1] : (cur >> 24) * 0x01010101u;
            const uint32_t e[8] = {(prev >> 16) & 255u, prev >> 24, cur & 255u, (cur >> 8) & 255u, (cur >> 16) & 255u, cur >> 24, next & 255u, (next >> 8) & 255u};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                uint32_t inner = e[j + 2], outer = e[j + 1] + e[j + 3];
                if (bl.radius) inner += outer, outer = e[j] + e[j + 4];
                o[j] = (int)((bl.ww * inner + bl.fw * outer + (1u << 23)) >> 24);
            }
        } else {
            const int r = it / stride, at = it - r * stride;
            const uint32_t t2 = src[it];
            const uint32_t t1 = src[max(r - 1, 0) * stride + at], t3 = src[min(r + 1, rows - 1) * stride + at];
            uint32_t t0 = 0, t4 = 0;
            if (bl.radius) t0 = src[max(r - 2, 0) * stride + at], t4 = src[min(r + 2, rows - 1) * stride + at];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int s = 8 * j;
                uint32_t inner = (t2 >> s) & 255u, outer = ((t1 >> s) & 255u) + ((t3 >> s) & 255u);
                if (bl.radius) inner += outer, outer = ((t0 >> s) & 255u) + ((t4 >> s) & 255u);
                o[j] = (int)((bl.ww * inner + bl.fw * outer + (1u << 23)) >> 24);
            }
        }
        dst[it] = img_pack4(o);
    }
}

// the four pixels of an item out of a blurred buffer
__device__ __forceinline__ void img_blur_fetch(const uint32_t* img, int D4, int row, int x4, int px[3][4]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const uint32_t t = img[(row * 3 + c) * D4 + x4];
#pragma unroll
        for (int j = 0; j < 4; ++j) px[c][j] = (int)((t >> (8 * j)) & 255u);
    }
}

// The layout in LDS, for the kernel and for image_blur_lds_bytes: the column table, the value table, the source rows, the plane sets of the
// horizontal pass, the image buffers (one per side, then the second buffer of the passes), and with windows the row-table entries per side
struct ImgBlurLds {
    int src, planes, plane_bytes, img, img_bytes, band;
    int64_t total;
};

__host__ __device__ inline ImgBlurLds img_blur_lds(int S, int D, int max_rows, int sides, bool rrc) {
    const int rows = (sides == 2 ? kImgBlurMixBand : kImgBlurBand) + 2 * kImgBlurHalo;   // an image buffer's rows
    ImgBlurLds l;
    l.src = D * (1 + kImgTaps) * 4 + 768 * 4;
    l.planes = l.src + ((max_rows * S * 3 + 15) & ~15);
    l.plane_bytes = max_rows * 3 * D;
    l.img = (l.planes + sides * l.plane_bytes + 15) & ~15;
    l.img_bytes = rows * 3 * D;
    const int64_t end = (int64_t)l.img + (int64_t)(sides + 1) * l.img_bytes;
    l.band = (int)((end + 15) & ~(int64_t)15);
    l.total = rrc ? (int64_t)l.band + (int64_t)sides * rows * (1 + kImgTaps) * 4 : end;
    return l;
}

template <int DT, bool RRC, bool MIX, bool STAT>
__global__ __launch_bounds__(kImgThreads) void k_image_blur(const uint8_t* __restrict__ data, const int64_t* __restrict__ index, int N, int S, int D_rt,
                                                            int max_rows, const int32_t* __restrict__ tab, const float* __restrict__ table,
                                                            float* __restrict__ out, const int32_t* __restrict__ first, int reflect, int fill,
                                                            const int32_t* __restrict__ mix, const int32_t* __restrict__ erase,
                                                            const int32_t* __restrict__ color, const uint32_t* __restrict__ sums,
                                                            uint32_t* __restrict__ sums_out, const int32_t* __restrict__ blur) {
    // first = the aug words (or NULL: the zero word), with RRC the window records
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    constexpr int kSides = MIX ? 2 : 1, kBand = MIX ? kImgBlurMixBand : kImgBlurBand, kRows = kBand + 2 * kImgBlurHalo, kBandWords = kRows * (1 + kImgTaps);
    const int D = DT ? DT : D_rt, D4 = D / 4;
    const int row_bytes = S * 3;
    const ImgBlurLds lds = img_blur_lds(S, D, max_rows, kSides, RRC);
    int32_t* s_xmin = (int32_t*)smem;                    // [D]
    int32_t* s_coef = s_xmin + D;                        // [D][4]
    float* s_table = (float*)(s_coef + D * kImgTaps);    // [3][256]
    uint8_t* s_src = smem + lds.src;                     // [max_rows][S][3]
    uint32_t* s_pp = (uint32_t*)(smem + lds.img + kSides * lds.img_bytes);
    int32_t* s_band = (int32_t*)(smem + lds.band);       // RRC: per side xmin [kRows], coef [kRows][4]

    const int tid = threadIdx.x, b = blockIdx.y;
    const int y0 = blockIdx.x * kBand, y1 = min(y0 + kBand, D);
    int p = b, sides = 1;
    float w_self = 1.0f, w_partner = 0.0f;
    int by0 = 0, by1 = 0, bx0 = 0, bx1 = 0;
    bool box = false, as_is = true;
    if (MIX) {
        // as k_image_batch_mix: a partner outside the batch is the sample itself; the box is clamped to the output
        const int32_t* rec = mix + b * 6;
        p = (unsigned)rec[0] < gridDim.y ? rec[0] : b;
        w_self = __int_as_float(rec[1]), w_partner = __int_as_float(rec[2]);
        by0 = min(rec[3] & 0xffff, D), by1 = min((rec[3] >> 16) & 0xffff, D);
        bx0 = min(rec[4] & 0xffff, D), bx1 = min((rec[4] >> 16) & 0xffff, D);
        box = by1 > by0 && bx1 > bx0;
        const bool partner = w_partner != 0.0f || (box && by0 < y1 && by1 > y0);
        sides = partner && p != b ? 2 : 1;
        as_is = !partner && w_self == 1.0f;
    }
    // the colour and blur records of the workgroup (and of its partner, where the band takes something from it)
    ImgColor col[kSides];
    ImgBlur bl[kSides];
    col[0] = color ? img_color(color + 4 * b, sums, b, D, STAT) : img_color_none();
    if (STAT && !col[0].contrast) return;
    bl[0] = blur ? img_blur(blur + 4 * b) : img_blur_none();
    if (MIX) {
        col[kSides - 1] = sides == 2 && color ? img_color(color + 4 * p, sums, p, D, false) : col[0];
        bl[kSides - 1] = sides == 2 && blur ? img_blur(blur + 4 * p) : bl[0];
    }
    int e0s[kSides], r0s[kSides], lasts[kSides];

    if (!RRC) {
        for (int i = tid; i < D; i += kImgThreads) s_xmin[i] = tab[i];
        for (int i = tid; i < D * kImgTaps; i += kImgThreads) s_coef[i] = tab[2 * D + i];
    }
    if (!STAT)
        for (int i = tid; i < 768; i += kImgThreads) s_table[i] = table[i];

#pragma unroll
    for (int side = 0; side < kSides; ++side) {
        if (side < sides) {
            const int pos = side ? p : b;
            const ImgBlur sb = bl[side];
            const int halo = sb.on ? 3 * (sb.radius + 1) : 0;
            const int e0 = max(0, y0 - halo), e1 = min(D, y1 + halo), erows = e1 - e0;
            uint32_t* s_tmp = (uint32_t*)(smem + lds.planes + side * lds.plane_bytes);
            uint32_t* s_img = (uint32_t*)(smem + lds.img + side * lds.img_bytes);
            int32_t* band = s_band + side * kBandWords;
            if (side) __syncthreads();                   // the sample's passes have read s_src, the column table and s_pp
            int64_t img = index ? index[pos] : pos;
            img = img < 0 ? 0 : (img >= N ? N - 1 : img);    // a bad index must still not read outside data
            int r0, nrows, xlast;
            if (RRC) {
                // this side's window, its column table, of its row table the entries of rows e0 .. e1-1, and its source rows (as k_image_batch_rrc)
                const ImgWindow win = img_window(first + 2 * pos, tab, S, D, e0, e1, max_rows);
                r0 = win.r0, nrows = win.nrows, xlast = win.w - 1;
                for (int i = tid; i < D; i += kImgThreads) s_xmin[i] = win.ctab[i];
                for (int i = tid; i < D * kImgTaps; i += kImgThreads) s_coef[i] = win.ctab[2 * D + i];
                for (int i = tid; i < erows; i += kImgThreads) band[i] = win.rtab[e0 + i];
                for (int i = tid; i < erows * kImgTaps; i += kImgThreads) band[kRows + i] = win.rtab[2 * D + e0 * kImgTaps + i];
                const uint8_t* image = data + (img * S + win.top + r0) * (int64_t)row_bytes + win.left * 3;
                for (int i = tid; i < nrows * win.w; i += kImgThreads) {
                    const int r = i / win.w, x = i - r * win.w;
                    const uint8_t* px = image + r * row_bytes + (win.flip ? xlast - x : x) * 3;
                    uint8_t* dst = s_src + r * row_bytes + x * 3;
                    dst[0] = px[0];
                    dst[1] = px[1];
                    dst[2] = px[2];
                }
            } else {
                // the source rows of output rows e0 .. e1-1, clamped as the other forms clamp them, out of the augmented image (as k_image_batch_aug)
                r0 = tab[e0];
                int r1 = tab[e1 - 1] + tab[D + e1 - 1];
                r0 = max(0, min(r0, S - 1));
                r1 = max(r0 + 1, min(r1, min(S, r0 + max_rows)));
                nrows = r1 - r0, xlast = S - 1;
                const int w = first ? first[pos] : 0;
                const int oy = (int)(int8_t)(w & 255), ox = (int)(int8_t)((w >> 8) & 255), flip = (w >> 16) & 1;
                const uint8_t* image = data + img * S * (int64_t)row_bytes;
                for (int i = tid; i < nrows * S; i += kImgThreads) {
                    const int r = i / S, x = i - r * S;
                    int sy = r0 + r + oy, sx = (flip ? S - 1 - x : x) + ox;
                    const bool outside = !reflect && ((unsigned)sy >= (unsigned)S || (unsigned)sx >= (unsigned)S);
                    sy = sy < 0 ? -sy : sy, sx = sx < 0 ? -sx : sx;
                    sy = sy > S - 1 ? 2 * (S - 1) - sy : sy, sx = sx > S - 1 ? 2 * (S - 1) - sx : sx;
                    sy = max(0, min(sy, S - 1)), sx = max(0, min(sx, S - 1));
                    const uint8_t* px = image + (sy * S + sx) * 3;
                    uint8_t* dst = s_src + i * 3;
                    dst[0] = outside ? (uint8_t)fill : px[0];
                    dst[1] = outside ? (uint8_t)fill : px[1];
                    dst[2] = outside ? (uint8_t)fill : px[2];
                }
            }
            e0s[side] = e0, r0s[side] = r0, lasts[side] = nrows - 1;
            __syncthreads();

            // horizontal pass, as the other forms: four neighbouring outputs of one (row, channel) per item
            for (int it = tid; it < nrows * 3 * D4; it += kImgThreads) {
                const int x4 = it % D4, rc = it / D4, c = rc % 3, r = rc / 3;
                const uint8_t* line = s_src + r * row_bytes + c;
                const int4 xm = ((const int4*)s_xmin)[x4];
                const int xms[4] = {xm.x, xm.y, xm.z, xm.w};
                int px[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int4 k = ((const int4*)s_coef)[x4 * 4 + j];
                    const int q = max(0, xms[j]);
                    int acc = 1 << (kImgBits - 1);
                    acc += __mul24((int)line[min(q, xlast) * 3], k.x);
                    acc += __mul24((int)line[min(q + 1, xlast) * 3], k.y);
                    acc += __mul24((int)line[min(q + 2, xlast) * 3], k.z);
                    acc += __mul24((int)line[min(q + 3, xlast) * 3], k.w);
                    px[j] = img_round_clip(acc);
                }
                s_tmp[rc * D4 + x4] = img_pack4(px);
            }
            __syncthreads();

            if (sb.on) {
                // the resized image of rows e0 .. e1-1 behind grayscale / solarize, then the six passes
                const ImgColor front = img_color_front(col[side]);
                for (int it = tid; it < erows * D4; it += kImgThreads) {
                    const int ry = it / D4, x4 = it - ry * D4;
                    const int4 k = RRC ? ((const int4*)(band + kRows))[ry] : ((const int4*)s_coef)[e0 + ry];
                    const int rel = (RRC ? band[ry] : s_xmin[e0 + ry]) - r0;
                    int px[3][4];
                    img_vertical4(s_tmp + x4, D4, rel, nrows - 1, k, px);
                    img_color_apply(front, px);
#pragma unroll
                    for (int c = 0; c < 3; ++c) s_img[(ry * 3 + c) * D4 + x4] = img_pack4(px[c]);
                }
                __syncthreads();
#pragma unroll 1
                for (int pass = 0; pass < 6; ++pass) {
                    img_blur_pass(pass & 1 ? s_pp : s_img, pass & 1 ? s_img : s_pp, erows, D4, pass >= 3, sb, tid);
                    __syncthreads();
                }
            }
        }
    }
    __syncthreads();

    // the store loop of the colour forms: one item = four neighbouring pixels of one output row in all three channels, from the blurred image
    // (then the jitter ops) or from the vertical pass (then the whole chain); the value table, the erase, the mix, three float4 stores
    const int band4 = (y1 - y0) * D4;
    ImgErase er[kSides];
    if (!STAT) {
        er[0] = erase ? img_erase(erase + 8 * b, D, y0, y1) : img_erase_none();
        if (MIX) er[kSides - 1] = sides == 2 && erase ? img_erase(erase + 8 * p, D, y0, y1) : er[0];
    }
    uint32_t lsum = 0;
    float* obase = STAT ? nullptr : out + (int64_t)b * 3 * D * D + (int64_t)y0 * D;
    for (int it = tid; it < band4; it += kImgThreads) {
        const int y = y0 + it / D4, x4 = it % D4;
        float v[3][4], u[3][4];
#pragma unroll
        for (int side = 0; side < kSides; ++side) {
            if (side < sides && !(side && as_is)) {
                const uint32_t* s_tmp = (const uint32_t*)(smem + lds.planes + side * lds.plane_bytes);
                const uint32_t* s_img = (const uint32_t*)(smem + lds.img + side * lds.img_bytes);
                const int ry = y - e0s[side];
                int px[3][4];
                if (bl[side].on) {
                    img_blur_fetch(s_img, D4, ry, x4, px);
                    img_color_apply(img_color_back(col[side]), px);
                } else {
                    const int32_t* band = s_band + side * kBandWords;
                    const int4 k = RRC ? ((const int4*)(band + kRows))[ry] : ((const int4*)s_coef)[y];
                    const int rel = (RRC ? band[ry] : s_xmin[y]) - r0s[side];
                    img_vertical4(s_tmp + x4, D4, rel, lasts[side], k, px);
                    img_color_apply(col[side], px);
                }
                if (STAT) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) lsum += (uint32_t)img_luma(px[0][j], px[1][j], px[2][j]);
                } else {
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        float* t = side ? u[c] : v[c];
#pragma unroll
                        for (int j = 0; j < 4; ++j) t[j] = s_table[c * 256 + px[c][j]];
                        if (er[side].touched) img_erase_apply(er[side], c, y, x4, D4, t);
                    }
                }
            }
        }
        if (!STAT) {
            if (MIX && !as_is) {
                // out = inside the box ? partner : fl(fl(w_self * own) + fl(w_partner * partner)); one plane set: the partner is the sample
                const bool row_in = box && y >= by0 && y < by1;
#pragma unroll
                for (int c = 0; c < 3; ++c)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int x = x4 * 4 + j;
                        const float q = sides == 2 ? u[c][j] : v[c][j];
                        const float a = w_self * v[c][j], c2 = w_partner * q;
                        v[c][j] = row_in && x >= bx0 && x < bx1 ? q : a + c2;
                    }
            }
#pragma unroll
            for (int c = 0; c < 3; ++c)
                *(float4*)(obase + (int64_t)c * D * D + (int64_t)it * 4) = make_float4(v[c][0], v[c][1], v[c][2], v[c][3]);
        }
    }
    if (STAT) {
        // as the other statistics forms: the waves by shuffles, the wave sums through s_src, one integer atomic per workgroup
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) lsum += __shfl_down(lsum, off);
        uint32_t* s_part = (uint32_t*)s_src;
        if ((tid & 63) == 0) s_part[tid >> 6] = lsum;
        __syncthreads();
        if (tid == 0) {
            uint32_t total = 0;
            for (int i = 0; i < kImgThreads / 64; ++i) total += s_part[i];
            atomicAdd(sums_out + b, total);
        }
    }
}
