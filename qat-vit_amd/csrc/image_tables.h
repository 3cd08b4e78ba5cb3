// Input pipeline, host only: Pillow's 8-bit bicubic coefficient table of a src -> dst resample, built once for image.hip (four taps, the filter not
// stretched) and image_window.hip (up to 17 taps, the filter stretched where src > dst).  Included inside namespace qv, in front of the device code.
#pragma once

static double cubic(double x) {
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

// xmin [dst], ntaps [dst], coef [dst][K] (include/qatvit.h), or 1 with the error of the entry `who`.  `taps` is how many taps of an output the
// kernel takes; a band of `band` output rows may read max_rows(src, dst) source rows.
template <int K>
static int pillow_coeffs(const char* who, bool stretched, int taps, int band, int (*max_rows)(int, int), int src, int dst, int32_t* xmin_out,
                         int32_t* ntaps_out, int32_t* coef) {
    const double scale = (double)src / (double)dst, fs = stretched && scale > 1.0 ? scale : 1.0, support = 2.0 * fs, ss = 1.0 / fs;
    for (int xx = 0; xx < dst; ++xx) {
        const double center = (xx + 0.5) * scale;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > src) xmax = src;
        const int n = xmax - xmin;
        // Where center -+ support + 0.5 falls on an integer, the rounding of the doubles can give one tap more than `taps`: n = 12 at D = 44 has
        // five.  Its distance is the support, its weight 0: where the table has room it is stored (ntaps is Pillow's) and checked below to be 0,
        // and the kernel leaves it out.
        if (n < 1 || n > K || n > taps + 1) {
            set_error("%s: %d taps at output %d (src %d, dst %d)", who, n, xx, src, dst);
            return 1;
        }
        double w[K], ww = 0.0;
        for (int i = 0; i < n; ++i) {
            w[i] = cubic((i + xmin - center + 0.5) * ss);
            ww += w[i];
        }
        int64_t pos = 0, neg = 0;
        for (int i = 0; i < K; ++i) {
            int32_t k = 0;
            if (i < n) {
                const double v = ww != 0.0 ? w[i] / ww : w[i];
                k = v < 0 ? (int32_t)(-0.5 + v * (double)(1 << kImgBits)) : (int32_t)(0.5 + v * (double)(1 << kImgBits));
            }
            // the kernel multiplies with v_mad_i32_i24 and accumulates in int32, as Pillow does
            if (k <= -(1 << 23) || k >= (1 << 23)) {
                set_error("%s: coefficient %d at output %d does not fit 24 bits (src %d, dst %d)", who, k, xx, src, dst);
                return 1;
            }
            if (k != 0 && i >= taps) {
                set_error("%s: coefficient %d of tap %d at output %d lies behind the %d taps the kernel takes (src %d, dst %d)", who, k, i, xx, taps, src,
                          dst);
                return 1;
            }
            if (k > 0) pos += k; else neg -= k;
            coef[xx * K + i] = k;
        }
        if (255 * pos + (1 << (kImgBits - 1)) >= ((int64_t)1 << 31) || 255 * neg >= ((int64_t)1 << 31)) {
            set_error("%s: int32 accumulator overflow at output %d (src %d, dst %d)", who, xx, src, dst);
            return 1;
        }
        xmin_out[xx] = xmin;
        ntaps_out[xx] = n;
    }
    // the kernel keeps max_rows source rows per band of output rows
    for (int y0 = 0; y0 < dst; y0 += band) {
        const int y1 = (y0 + band < dst ? y0 + band : dst) - 1;
        if (xmin_out[y1] + ntaps_out[y1] - xmin_out[y0] > max_rows(src, dst)) {
            set_error("%s: output rows %d..%d read more than %d source rows (src %d, dst %d)", who, y0, y1, max_rows(src, dst), src, dst);
            return 1;
        }
    }
    return 0;
}
