// The device helpers of the input pipeline's kernels: image.hip (the fifteen forms of image_kernel.h) and image_blur.hip (the blur forms) include this
// text once each, inside namespace qv.  No include guard.
// One workgroup = kImgBand output rows of one image, all three channels.  LDS: the source rows the band touches (HWC bytes as they lie in memory),
// their horizontally resampled form as planes [row][c][D] of bytes, the coefficient tables and the value table.  The store loop walks each channel's
// part of the band, which is one contiguous run of the output: 16 bytes per lane, 1 KiB per wave-instruction.
constexpr int kImgThreads = 256;

__device__ inline int img_round_clip(int acc) {
    acc >>= kImgBits;
    return acc < 0 ? 0 : (acc > 255 ? 255 : acc);
}

// The rrc forms: one side's window (include/qatvit.h: the record of qatvit_image_batch_rrc) as the workgroup of output rows y0 .. y1-1 needs it.
// A malformed record is made safe, not trusted: h and w are clamped to 1 .. S, then top to 0 .. S-h and left to 0 .. S-w, so the tables read are
// among the S tables of `windows` and every pixel read lies inside the image.  r0 and nrows are the source rows of the band inside the window,
// from the row table of h, clamped as the other forms clamp them; the host builder has checked that nrows <= image_max_rows(h, D) <= max_rows.
struct ImgWindow {
    int top, left, w, flip, r0, nrows;
    const int32_t* ctab;   // the table of w -> D: xmin[D], ntaps[D], coef[D][4]
    const int32_t* rtab;   // the table of h -> D
};

__device__ inline ImgWindow img_window(const int32_t* __restrict__ rec, const int32_t* __restrict__ windows, int S, int D, int y0, int y1,
                                       int max_rows) {
    const int w0 = rec[0], w1 = rec[1];
    const int h = max(1, min(w1 & 0x7fff, S)), w = max(1, min((w1 >> 15) & 0x7fff, S));
    ImgWindow v;
    v.top = min(w0 & 0xffff, S - h);
    v.left = min((w0 >> 16) & 0xffff, S - w);
    v.w = w;
    v.flip = (w1 >> 30) & 1;
    v.ctab = windows + (int64_t)(w - 1) * 6 * D;
    v.rtab = windows + (int64_t)(h - 1) * 6 * D;
    int r0 = v.rtab[y0], r1 = v.rtab[y1 - 1] + v.rtab[D + y1 - 1];
    r0 = max(0, min(r0, h - 1));
    r1 = max(r0 + 1, min(r1, min(h, r0 + max_rows)));
    v.r0 = r0;
    v.nrows = r1 - r0;
    return v;
}

// The erase forms: one side's record (include/qatvit.h: the record of qatvit_image_batch_erase) as the workgroup of output rows y0 .. y1-1 needs it.
// A malformed record is made safe, not trusted: the four bounds are clamped to [0, D] and only bit 0 of the mode is read; nothing is addressed
// through the record, so no record can move a read or a store.  touched = the box is not empty and meets the band's rows (workgroup-uniform).
struct ImgErase {
    int y0, y1, x0, x1;
    bool touched, noise;
    float f0, f1, f2;
    uint32_t k0, k1;
};

__device__ __forceinline__ ImgErase img_erase(const int32_t* __restrict__ rec, int D, int y0, int y1) {
    ImgErase e;
    e.y0 = min(rec[0] & 0xffff, D), e.y1 = min((rec[0] >> 16) & 0xffff, D);
    e.x0 = min(rec[1] & 0xffff, D), e.x1 = min((rec[1] >> 16) & 0xffff, D);
    e.touched = e.y1 > e.y0 && e.x1 > e.x0 && e.y0 < y1 && e.y1 > y0;
    e.f0 = __int_as_float(rec[2]), e.f1 = __int_as_float(rec[3]), e.f2 = __int_as_float(rec[4]);
    e.noise = rec[5] & 1;
    e.k0 = (uint32_t)rec[6], e.k1 = (uint32_t)rec[7];
    return e;
}

// Philox4x32-10 (Salmon et al., SC'11) with the standard constants; the integer half of the noise, exact
__device__ __forceinline__ void img_philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t r[4]) {
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
        const uint32_t h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
        c0 = h1 ^ c1 ^ k0, c1 = l1, c2 = h0 ^ c3 ^ k1, c3 = l0;
        k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
    }
    r[0] = c0, r[1] = c1, r[2] = c2, r[3] = c3;
}

// z(key, c, y, 4 * x4 + j), j = 0 .. 3, of include/qatvit.h: one Philox call, Box-Muller on (r0, r1) and (r2, r3) with the full-precision functions
__device__ __forceinline__ void img_noise4(uint32_t k0, uint32_t k1, int c, int y, int x4, int D4, float z[4]) {
    uint32_t r[4];
    img_philox((uint32_t)(y * D4 + x4), (uint32_t)c, 0u, 0u, k0, k1, r);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const float u = (float)((r[2 * h] >> 9) + 1u) * 0x1p-23f, t = (float)(r[2 * h + 1] >> 8) * 0x1p-23f;
        const float R = sqrtf(-2.0f * logf(u));
        z[2 * h] = R * cospif(t);
        z[2 * h + 1] = R * sinpif(t);
    }
}

// One float4 item (channel c, row y, columns 4 * x4 .. + 3) of a band that the box meets: the elements inside the box take the fill of their
// channel or their noise value; only an item with an element inside the box makes the Philox call.
__device__ __forceinline__ void img_erase_apply(const ImgErase e, int c, int y, int x4, int D4, float v[4]) {
    const int x = x4 * 4;
    if (y < e.y0 || y >= e.y1 || x + 3 < e.x0 || x >= e.x1) return;
    float z[4];
    if (e.noise) {
        img_noise4(e.k0, e.k1, c, y, x4, D4, z);
    } else {
        z[0] = z[1] = z[2] = z[3] = c == 0 ? e.f0 : (c == 1 ? e.f1 : e.f2);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = x + j >= e.x0 && x + j < e.x1 ? z[j] : v[j];
}

// The colour forms: an all-zero erase record, for erase == NULL
__device__ __forceinline__ ImgErase img_erase_none() {
    ImgErase e;
    e.y0 = e.y1 = e.x0 = e.x1 = 0;
    e.touched = e.noise = false;
    e.f0 = e.f1 = e.f2 = 0.0f;
    e.k0 = e.k1 = 0u;
    return e;
}

// The colour forms: one side's record (include/qatvit.h: the record of qatvit_image_batch_color) as the workgroup needs it.  A malformed record
// is cleaned, not trusted, and nothing is addressed through it: an op code that an earlier slot held, and an op whose factor is negative or not
// finite, become "none"; so does contrast where the caller passed no sums.  before_contrast (the statistics launch) drops the contrast op and
// the slots behind it.  mean = Python's int(s / (D * D) + 0.5) of the sum s that the statistics launch left in sums[b].
enum { kColNone = 0, kColBrightness = 1, kColContrast = 2, kColSaturation = 3 };

struct ImgColor {
    int op0, op1, op2;
    bool gray, solarize, contrast, any;
    int threshold, mean;
    float fb, fc, fs;
};

__device__ __forceinline__ ImgColor img_color(const int32_t* __restrict__ rec, const uint32_t* __restrict__ sums, int b, int D, bool before_contrast) {
    ImgColor c;
    const int w0 = rec[0];
    c.fb = __int_as_float(rec[1]), c.fc = __int_as_float(rec[2]), c.fs = __int_as_float(rec[3]);
    // f >= 0 && f < inf is false for a NaN
    const bool ok_b = c.fb >= 0.0f && c.fb < INFINITY, ok_c = c.fc >= 0.0f && c.fc < INFINITY, ok_s = c.fs >= 0.0f && c.fs < INFINITY;
    const int s0 = w0 & 3, s1 = (w0 >> 2) & 3, s2 = (w0 >> 4) & 3;
    const int d1 = s1 == s0 ? kColNone : s1, d2 = s2 == s0 || s2 == s1 ? kColNone : s2;
    c.contrast = ok_c && (s0 == kColContrast || d1 == kColContrast || d2 == kColContrast);
    const bool keep_c = c.contrast && !before_contrast && sums != nullptr;
    auto cleaned = [&](int op) { return op == kColBrightness ? (ok_b ? op : kColNone) : op == kColContrast ? (keep_c ? op : kColNone) : op == kColSaturation ? (ok_s ? op : kColNone) : kColNone; };
    c.op0 = cleaned(s0), c.op1 = cleaned(d1), c.op2 = cleaned(d2);
    if (before_contrast) {
        if (s0 == kColContrast) c.op1 = c.op2 = kColNone;
        if (d1 == kColContrast) c.op2 = kColNone;
    }
    c.gray = (w0 >> 8) & 1, c.solarize = (w0 >> 9) & 1;
    c.threshold = (w0 >> 16) & 255;
    c.mean = 0;
    if (keep_c) {
        const uint32_t dd = (uint32_t)(D * D);
        c.mean = (int)((2u * sums[b] + dd) / (2u * dd));   // s <= 255 * 384 * 384 < 2^26
    }
    c.any = c.gray || c.solarize || c.op0 != kColNone || c.op1 != kColNone || c.op2 != kColNone;
    return c;
}

// Pillow's convert("L")
__device__ __forceinline__ int img_luma(int r, int g, int b) { return (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16; }

// Pillow's Image.blend as ImageEnhance calls it: fl(in1 + fl(a * (v - in1))), the product and the sum rounded one by one (never fused: a fused
// multiply-add changes bytes), truncated and clipped to 0 .. 255.  For 0 <= a <= 1 the sum lies between in1 and v, where the clip does nothing.
// t is finite (a is finite, the operands are bytes), so the clip is one median: v_med3_f32 in place of two compares and two selects.
__device__ __forceinline__ int img_blend(int in1, int v, float a) {
    const float t = __fadd_rn((float)in1, __fmul_rn(a, (float)(v - in1)));
    return (int)__builtin_amdgcn_fmed3f(t, 0.0f, 255.0f);
}

// in1 = 0: fl(0 + x) is x (a -0.0 product, from a = -0.0 or v = 0, clips to 0 like +0.0), so the sum is left out
__device__ __forceinline__ int img_blend0(int v, float a) { return (int)__builtin_amdgcn_fmed3f(__fmul_rn(a, (float)v), 0.0f, 255.0f); }

__device__ __forceinline__ void img_color_op(int op, const ImgColor c, int& r, int& g, int& b) {
    if (op == kColBrightness) {
        r = img_blend0(r, c.fb), g = img_blend0(g, c.fb), b = img_blend0(b, c.fb);
    } else if (op == kColContrast) {
        r = img_blend(c.mean, r, c.fc), g = img_blend(c.mean, g, c.fc), b = img_blend(c.mean, b, c.fc);
    } else if (op == kColSaturation) {
        const int l = img_luma(r, g, b);
        r = img_blend(l, r, c.fs), g = img_blend(l, g, c.fs), b = img_blend(l, b, c.fs);
    }
}

// The chain on the four pixels of an item: grayscale, solarize, then the record's ops in slot order.  Every branch is workgroup-uniform.
__device__ __forceinline__ void img_color_apply(const ImgColor c, int px[3][4]) {
    if (!c.any) return;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        int r = px[0][j], g = px[1][j], b = px[2][j];
        if (c.gray) r = g = b = img_luma(r, g, b);
        if (c.solarize) {
            r = r < c.threshold ? r : 255 - r, g = g < c.threshold ? g : 255 - g, b = b < c.threshold ? b : 255 - b;
        }
        img_color_op(c.op0, c, r, g, b);
        img_color_op(c.op1, c, r, g, b);
        img_color_op(c.op2, c, r, g, b);
        px[0][j] = r, px[1][j] = g, px[2][j] = b;
    }
}

// The colour forms' vertical pass of one item: four neighbouring pixels of one output row in all three channels, as bytes 0 .. 255
__device__ __forceinline__ void img_vertical4(const uint32_t* plane, int D4, int rel, int last, const int4 k, int px[3][4]) {
    const int o0 = max(0, min(rel, last)) * 3 * D4, o1 = max(0, min(rel + 1, last)) * 3 * D4;
    const int o2 = max(0, min(rel + 2, last)) * 3 * D4, o3 = max(0, min(rel + 3, last)) * 3 * D4;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const uint32_t t0 = plane[o0 + c * D4], t1 = plane[o1 + c * D4], t2 = plane[o2 + c * D4], t3 = plane[o3 + c * D4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            int acc = 1 << (kImgBits - 1);
            acc += __mul24((int)((t0 >> (8 * j)) & 255), k.x);
            acc += __mul24((int)((t1 >> (8 * j)) & 255), k.y);
            acc += __mul24((int)((t2 >> (8 * j)) & 255), k.z);
            acc += __mul24((int)((t3 >> (8 * j)) & 255), k.w);
            px[c][j] = img_round_clip(acc);
        }
    }
}
