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

// DT = the output size as a constant (its divisions become multiplications), or 0: taken from D_rt.
template <int DT>
__global__ __launch_bounds__(kImgThreads) void k_image_batch(const uint8_t* __restrict__ data, const int64_t* __restrict__ index, int N, int S, int D_rt,
                                                             int max_rows, const int32_t* __restrict__ coeffs, const float* __restrict__ table,
                                                             float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int D = DT ? DT : D_rt;
    const int row_bytes = S * 3, src_bytes = (max_rows * row_bytes + 15) & ~15;
    int32_t* s_xmin = (int32_t*)smem;                    // [D]
    int32_t* s_coef = s_xmin + D;                        // [D][4]
    float* s_table = (float*)(s_coef + D * kImgTaps);    // [3][256]
    uint8_t* s_src = (uint8_t*)(s_table + 768);          // [max_rows][S][3]
    uint8_t* s_tmp = s_src + src_bytes;                  // [max_rows][3][D]

    const int tid = threadIdx.x, b = blockIdx.y;
    const int y0 = blockIdx.x * kImgBand, y1 = min(y0 + kImgBand, D);
    int64_t img = index ? index[b] : b;
    img = img < 0 ? 0 : (img >= N ? N - 1 : img);        // the range is the caller's contract; a bad index must still not read outside data

    // rows of the source this band reads; clamped so that tables other than qatvit_image_resize_coeffs' cannot send a read outside the image
    int r0 = coeffs[y0], r1 = coeffs[y1 - 1] + coeffs[D + y1 - 1];
    r0 = max(0, min(r0, S - 1));
    r1 = max(r0 + 1, min(r1, min(S, r0 + max_rows)));
    const int nrows = r1 - r0;

    for (int i = tid; i < D; i += kImgThreads) s_xmin[i] = coeffs[i];
    for (int i = tid; i < D * kImgTaps; i += kImgThreads) s_coef[i] = coeffs[2 * D + i];
    for (int i = tid; i < 768; i += kImgThreads) s_table[i] = table[i];
    const uint8_t* src = data + (img * S + r0) * (int64_t)row_bytes;
    const int nbytes = nrows * row_bytes;
    if ((((uintptr_t)src | (uintptr_t)nbytes) & 3) == 0) {
        for (int i = tid; i < nbytes / 4; i += kImgThreads) ((uint32_t*)s_src)[i] = ((const uint32_t*)src)[i];
    } else {
        for (int i = tid; i < nbytes; i += kImgThreads) s_src[i] = src[i];
    }
    __syncthreads();

    // horizontal pass: one item = four neighbouring outputs of one (row, channel), written as one dword.  Taps past a short window have coefficient 0,
    // so all four are always taken, from a clamped position.
    const int D4 = D / 4;
    for (int it = tid; it < nrows * 3 * D4; it += kImgThreads) {
        const int x4 = it % D4, rc = it / D4, c = rc % 3, r = rc / 3;
        const uint8_t* line = s_src + r * row_bytes + c;
        const int4 xm = ((const int4*)s_xmin)[x4];
        const int xms[4] = {xm.x, xm.y, xm.z, xm.w};
        int px[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int4 k = ((const int4*)s_coef)[x4 * 4 + j];
            const int p = max(0, xms[j]);
            int acc = 1 << (kImgBits - 1);
            acc += __mul24((int)line[min(p, S - 1) * 3], k.x);
            acc += __mul24((int)line[min(p + 1, S - 1) * 3], k.y);
            acc += __mul24((int)line[min(p + 2, S - 1) * 3], k.z);
            acc += __mul24((int)line[min(p + 3, S - 1) * 3], k.w);
            px[j] = img_round_clip(acc);
        }
        // packed through v_perm_b32: hipcc turns the plain (shift, clamp, | << 8) pair into v_ashr_pk_u8_i32 and then takes the upper half of its
        // result for zero, which on the MI355X it is not (bytes 2 and 3 of the dword came out wrong)
        ((uint32_t*)s_tmp)[rc * D4 + x4] = __builtin_amdgcn_perm((uint32_t)(px[2] | px[3] << 16), (uint32_t)(px[0] | px[1] << 16), 0x06040200u);
    }
    __syncthreads();

    // vertical pass + value table + store
    const int band4 = (y1 - y0) * D4;
    float* obase = out + (int64_t)b * 3 * D * D + (int64_t)y0 * D;
    for (int it = tid; it < 3 * band4; it += kImgThreads) {
        const int c = it / band4, e = it % band4, y = y0 + e / D4, x4 = e % D4;
        const int4 k = ((const int4*)s_coef)[y];
        const int rel = s_xmin[y] - r0, last = nrows - 1;
        const uint32_t* plane = (const uint32_t*)s_tmp + c * D4 + x4;
        const uint32_t t0 = plane[max(0, min(rel, last)) * 3 * D4], t1 = plane[max(0, min(rel + 1, last)) * 3 * D4];
        const uint32_t t2 = plane[max(0, min(rel + 2, last)) * 3 * D4], t3 = plane[max(0, min(rel + 3, last)) * 3 * D4];
        const float* tab = s_table + c * 256;
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            int acc = 1 << (kImgBits - 1);
            acc += __mul24((int)((t0 >> (8 * j)) & 255), k.x);
            acc += __mul24((int)((t1 >> (8 * j)) & 255), k.y);
            acc += __mul24((int)((t2 >> (8 * j)) & 255), k.z);
            acc += __mul24((int)((t3 >> (8 * j)) & 255), k.w);
            v[j] = tab[img_round_clip(acc)];
        }
        *(float4*)(obase + (int64_t)c * D * D + (int64_t)e * 4) = make_float4(v[0], v[1], v[2], v[3]);
    }
}

int64_t image_lds_bytes(int S, int D) {
    const int mr = image_max_rows(S, D);
    return (int64_t)D * (1 + kImgTaps) * 4 + 768 * 4 + ((mr * S * 3 + 15) & ~15) + (int64_t)mr * 3 * D;
}

int launch_image_batch(const uint8_t* data, const int64_t* index, int B, int N, int S, int D, const int32_t* coeffs, const float* table, float* out,
                       hipStream_t st) {
    const dim3 grid((D + kImgBand - 1) / kImgBand, B);
    auto kern = D == 224 ? k_image_batch<224> : k_image_batch<0>;
    hipLaunchKernelGGL(kern, grid, dim3(kImgThreads), (size_t)image_lds_bytes(S, D), st, data, index, N, S, D, image_max_rows(S, D), coeffs, table, out);
    return 0;
}

}  // namespace qv
