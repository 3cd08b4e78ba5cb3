// Input pipeline: uint8 HWC images resident on the device -> the fp32 [B, 3, D, D] batch that Resize(D, BICUBIC) + ToTensor() + Normalize(mean, std)
// produce on the host (Pillow's 8-bit two-pass resample; include/qatvit.h states the arithmetic).  Integer throughout, so the result is equal, not close.
#include <math.h>

#include "qv_common.h"
#include "qv_kernels.h"

namespace qv {

// ---------------------------------------------------------------------------------------------------------------- host: the two tables
static double cubic(double x) {
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

int image_max_rows(int S, int D) { return (kImgBand * S + D - 1) / D + kImgTaps + 1; }

int image_resize_coeffs(int src, int dst, int32_t* xmin_out, int32_t* ntaps_out, int32_t* coef) {
    const double scale = (double)src / (double)dst, support = 2.0;   // src <= dst: the filter is not stretched
    for (int xx = 0; xx < dst; ++xx) {
        const double center = (xx + 0.5) * scale;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > src) xmax = src;
        const int n = xmax - xmin;
        if (n < 1 || n > kImgTaps) {
            set_error("qatvit_image_resize_coeffs: %d taps at output %d (src %d, dst %d)", n, xx, src, dst);
            return 1;
        }
        double w[kImgTaps], ww = 0.0;
        for (int i = 0; i < n; ++i) {
            w[i] = cubic(i + xmin - center + 0.5);
            ww += w[i];
        }
        int64_t pos = 0;
        for (int i = 0; i < kImgTaps; ++i) {
            int32_t k = 0;
            if (i < n) {
                const double v = ww != 0.0 ? w[i] / ww : w[i];
                k = v < 0 ? (int32_t)(-0.5 + v * (double)(1 << kImgBits)) : (int32_t)(0.5 + v * (double)(1 << kImgBits));
            }
            // the kernel multiplies with v_mad_i32_i24 and accumulates in int32, as Pillow does
            if (k <= -(1 << 23) || k >= (1 << 23)) {
                set_error("qatvit_image_resize_coeffs: coefficient %d at output %d does not fit 24 bits", k, xx);
                return 1;
            }
            if (k > 0) pos += k;
            coef[xx * kImgTaps + i] = k;
        }
        if (255 * pos + (1 << (kImgBits - 1)) >= ((int64_t)1 << 31)) {
            set_error("qatvit_image_resize_coeffs: int32 accumulator overflow at output %d", xx);
            return 1;
        }
        xmin_out[xx] = xmin;
        ntaps_out[xx] = n;
    }
    // the kernel keeps image_max_rows source rows per band of kImgBand output rows
    for (int y0 = 0; y0 < dst; y0 += kImgBand) {
        const int y1 = (y0 + kImgBand < dst ? y0 + kImgBand : dst) - 1;
        if (xmin_out[y1] + ntaps_out[y1] - xmin_out[y0] > image_max_rows(src, dst)) {
            set_error("qatvit_image_resize_coeffs: output rows %d..%d read more than %d source rows", y0, y1, image_max_rows(src, dst));
            return 1;
        }
    }
    return 0;
}

void image_table(const float* mean, const float* stdv, float* table) {
    for (int c = 0; c < 3; ++c)
        for (int i = 0; i < 256; ++i) table[c * 256 + i] = ((float)i / 255.0f - mean[c]) / stdv[c];   // two IEEE divisions, as torch's div(255) .. div(std)
}

// ---------------------------------------------------------------------------------------------------------------- device
// One workgroup = kImgBand output rows of one image, all three channels.  LDS: the source rows the band touches (HWC bytes as they lie in memory),
// their horizontally resampled form as planes [row][c][D] of bytes, the coefficient tables and the value table.  The store loop walks each channel's
// part of the band, which is one contiguous run of the output: 16 bytes per lane, 1 KiB per wave-instruction.
constexpr int kImgThreads = 256;

__device__ inline int img_round_clip(int acc) {
    acc >>= kImgBits;
    return acc < 0 ? 0 : (acc > 255 ? 255 : acc);
}

// the kernel, once per form (image_kernel.h)
#define QV_IMAGE_MIX 0
#define QV_IMAGE_AUG 0
#include "image_kernel.h"
#undef QV_IMAGE_AUG
#define QV_IMAGE_AUG 1
#include "image_kernel.h"
#undef QV_IMAGE_MIX
#define QV_IMAGE_MIX 1
#include "image_kernel.h"
#undef QV_IMAGE_AUG
#undef QV_IMAGE_MIX

int64_t image_lds_bytes(int S, int D) {
    const int mr = image_max_rows(S, D);
    return (int64_t)D * (1 + kImgTaps) * 4 + 768 * 4 + ((mr * S * 3 + 15) & ~15) + (int64_t)mr * 3 * D;
}

// the mix kernel keeps the partner's planes behind the sample's
int64_t image_mix_lds_bytes(int S, int D) { return image_lds_bytes(S, D) + (int64_t)image_max_rows(S, D) * 3 * D; }

int launch_image_batch(const uint8_t* data, const int64_t* index, int B, int N, int S, int D, const int32_t* coeffs, const float* table, float* out,
                       hipStream_t st) {
    const dim3 grid((D + kImgBand - 1) / kImgBand, B);
    auto kern = D == 224 ? k_image_batch<224> : k_image_batch<0>;
    hipLaunchKernelGGL(kern, grid, dim3(kImgThreads), (size_t)image_lds_bytes(S, D), st, data, index, N, S, D, image_max_rows(S, D), coeffs, table, out);
    return 0;
}

int launch_image_batch_aug(const uint8_t* data, const int64_t* index, int B, int N, int S, int D, const int32_t* coeffs, const float* table,
                           const int32_t* aug, int padding_mode, int fill, float* out, hipStream_t st) {
    if (!aug) return launch_image_batch(data, index, B, N, S, D, coeffs, table, out, st);
    const dim3 grid((D + kImgBand - 1) / kImgBand, B);
    auto kern = D == 224 ? k_image_batch_aug<224> : k_image_batch_aug<0>;
    hipLaunchKernelGGL(kern, grid, dim3(kImgThreads), (size_t)image_lds_bytes(S, D), st, data, index, N, S, D, image_max_rows(S, D), coeffs, table, out,
                       aug, padding_mode, fill);
    return 0;
}

int launch_image_batch_mix(const uint8_t* data, const int64_t* index, int B, int N, int S, int D, const int32_t* coeffs, const float* table,
                           const int32_t* aug, int padding_mode, int fill, const int32_t* mix, float* out, hipStream_t st) {
    if (!mix) return launch_image_batch_aug(data, index, B, N, S, D, coeffs, table, aug, padding_mode, fill, out, st);
    const int64_t lds = image_mix_lds_bytes(S, D);
    if (lds > kImgMixMaxLds) {
        set_error("qatvit_image_batch_mix: source %d -> output %d needs %lld bytes of LDS for two plane sets, more than %d", S, D, (long long)lds,
                  kImgMixMaxLds);
        return 1;
    }
    const dim3 grid((D + kImgBand - 1) / kImgBand, B);
    auto kern = D == 224 ? k_image_batch_mix<224> : k_image_batch_mix<0>;
    hipLaunchKernelGGL(kern, grid, dim3(kImgThreads), (size_t)lds, st, data, index, N, S, D, image_max_rows(S, D), coeffs, table, out, aug, padding_mode,
                       fill, mix);
    return 0;
}

}  // namespace qv
