// Input pipeline, the RandAugment stage: bytes in, bytes out, between the window stage (image_window.hip) and the second stage (image.hip at S = D, or
// image_bytes_blur.hip).  uint8 [B][D][D][3] -> uint8 [B][D][D][3]: per sample up to four layers, each one of the fifteen ops of timm's
// _RAND_INCREASING_TRANSFORMS, applied in order, equal to Pillow's bytes (include/qatvit.h states every op).  A source file of its own: the machine
// code of every other kernel stays what it was.
// One workgroup of 1024 lanes = one sample.  It walks the sample's layers: a layer reads the whole current image from global memory (150 KB at
// D = 224: it stays in L2) and writes the next one, alternating between `scratch` and `out`; the first live layer starts on the side that lets the last
// one end in `out`, so no copy follows a chain, and a sample without a live layer is one copy.  Between two layers every lane makes its stores
// visible (__threadfence), the workgroup meets (__syncthreads), and every lane drops what its L1 holds of the buffer that was just rewritten
// (__threadfence again).  No workgroup reads another workgroup's sample.  The source and the destination of a layer are never the same buffer, so
// the ops that gather (affine, sharpness) read an image nobody writes.
// LDS: three 256-bin histograms, three 256-byte tables and the words of the reductions, 4 KB.  The ops in three groups:
//   table ops   AutoContrast, Equalize (a histogram pass with LDS atomics, then the table from ballots / a wave scan), Contrast (a luma-sum pass, then
//               the table of blend(mean, v, f)), Invert, Posterize, Solarize, SolarizeAdd, Brightness: 768 lanes fill the table, then one streaming
//               pass: an item is four pixels = twelve bytes = three dwords in, three dwords out.
//   Color       the same stream, the blend against the pixel's own luma.
//   Sharpness   per item the three rows' five dwords around it (the item and one pixel on either side), SMOOTH in integers, the blend.
//   affine      ShearX / ShearY / TranslateX / TranslateY / Rotate: per output pixel the source point in double, then 4 (bilinear) or 16 (bicubic)
//               neighbours gathered as bytes, filtered in double in Pillow's order of operations; four pixels are packed into the item's three dwords.
// Pillow's result depends on every double operation being rounded on its own.  hipcc contracts a * b + c into a fused multiply-add by default; the
// choice here is the pragma below, which switches contraction off for every function of this file (the Makefile's -ffp-contract=off says the same
// for the whole library, and this file does not rely on it).  The fp32 blends use the __fmul_rn / __fadd_rn helpers of image_device.h.
#pragma clang fp contract(off)

#include <math.h>

#include "qv_common.h"
#include "qv_kernels.h"

namespace qv {

#include "image_device.h"

constexpr int kRaThreads = 1024;
enum { kRaAutoContrast = 1, kRaEqualize, kRaInvert, kRaPosterize, kRaSolarize, kRaSolarizeAdd, kRaColor, kRaContrast, kRaBrightness, kRaSharpness,
       kRaShearX, kRaShearY, kRaTranslateX, kRaTranslateY, kRaRotate };
enum { kRaBilinear = 2, kRaBicubic = 3 };

// One layer's record as the workgroup needs it.  A record is cleaned, not trusted, and nothing is addressed through it: an unknown op, an unknown
// resample code, an enhance factor or a matrix entry that is not finite make the layer the identity (op 0); integer arguments are clamped.
struct RaLayer {
    int op, arg;
    float f;
    uint32_t fill;
    double m[6];
};

__device__ __forceinline__ RaLayer ra_layer(const int32_t* __restrict__ rec) {
    RaLayer L;
    L.op = rec[0] >= kRaAutoContrast && rec[0] <= kRaRotate ? rec[0] : 0;
    L.arg = rec[1];
    L.f = __int_as_float(rec[2]);
    L.fill = (uint32_t)rec[3] & 0xffffffu;
    bool finite = true;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const int lo = rec[4 + 2 * k], hi = rec[5 + 2 * k];
        finite = finite && ((hi >> 20) & 0x7ff) != 0x7ff;
        L.m[k] = __hiloint2double(hi, lo);
    }
    if (L.op >= kRaShearX && (!finite || (L.arg != kRaBilinear && L.arg != kRaBicubic))) L.op = 0;
    if (L.op >= kRaColor && L.op <= kRaSharpness && ((rec[2] >> 23) & 0xff) == 0xff) L.op = 0;
    const int top = L.op == kRaPosterize ? 8 : (L.op == kRaSolarize ? 256 : 255);
    if (L.op < kRaColor) L.arg = max(0, min(L.arg, top));
    return L;
}

// the twelve bytes of an item, byte k = channel k % 3 of pixel k / 3
__device__ __forceinline__ int ra_byte(const uint32_t w[3], int k) { return (int)((w[k >> 2] >> (8 * (k & 3))) & 255u); }

// ---- the statistics passes: whole-image reductions inside the workgroup

__device__ __forceinline__ void ra_histogram(const uint32_t* src, int items, uint32_t* s_hist, int tid) {
    if (tid < 768) s_hist[tid] = 0;
    __syncthreads();
    for (int it = tid; it < items; it += kRaThreads) {
        const uint32_t w[3] = {src[3 * it], src[3 * it + 1], src[3 * it + 2]};
#pragma unroll
        for (int k = 0; k < 12; ++k) atomicAdd(&s_hist[(k % 3) * 256 + ra_byte(w, k)], 1u);
    }
    __syncthreads();
}

// Python's int(sum(L) / (D * D) + 0.5) of the image's luma, as img_color has it
__device__ __forceinline__ int ra_mean_luma(const uint32_t* src, int items, uint32_t* s_red, int tid) {
    uint32_t sum = 0;
    for (int it = tid; it < items; it += kRaThreads) {
        const uint32_t w[3] = {src[3 * it], src[3 * it + 1], src[3 * it + 2]};
#pragma unroll
        for (int j = 0; j < 4; ++j) sum += (uint32_t)img_luma(ra_byte(w, 3 * j), ra_byte(w, 3 * j + 1), ra_byte(w, 3 * j + 2));
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_down(sum, off);
    if ((tid & 63) == 0) s_red[tid >> 6] = sum;
    __syncthreads();
    uint32_t total = 0;
    for (int i = 0; i < kRaThreads / 64; ++i) total += s_red[i];      // s <= 255 * 384 * 384 < 2^26
    const uint32_t dd = 4u * (uint32_t)items;
    return (int)((2u * total + dd) / (2u * dd));
}

// ---- the table of a table op: lane t < 768 writes entry t & 255 of channel t >> 8.  Every lane of the workgroup calls this (barriers, shuffles).

__device__ __forceinline__ void ra_table(const RaLayer L, int mean, int pixels, const uint32_t* s_hist, uint64_t* s_mask, uint32_t* s_red,
                                         uint8_t* s_lut, int tid) {
    const int i = tid & 255, ch = (tid >> 8) & 3, lane = tid & 63, wave = tid >> 6;
    int v = i;
    if (L.op == kRaAutoContrast || L.op == kRaEqualize) {
        // wave w < 12 holds bins 64 * (w & 3) .. + 63 of channel w >> 2: which bins are in use, and their counts in front of each bin
        const uint32_t h = tid < 768 ? s_hist[tid] : 0u;
        const uint64_t used = __ballot(h != 0u);
        uint32_t run = h;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t n = __shfl_up(run, off);
            if (lane >= off) run += n;
        }
        if (lane == 0) s_mask[wave] = used;
        if (lane == 63) s_red[wave] = run;
        __syncthreads();
        if (tid < 768) {
            int lo = 0, hi = 0, bins = 0;
            uint32_t before = run - h;
            for (int k = 3; k >= 0; --k) {
                const uint64_t m = s_mask[ch * 4 + k];
                if (m) lo = k * 64 + __ffsll((unsigned long long)m) - 1;
                bins += __popcll((unsigned long long)m);
                if (k < (wave & 3)) before += s_red[ch * 4 + k];
            }
            for (int k = 0; k < 4; ++k) {
                const uint64_t m = s_mask[ch * 4 + k];
                if (m) hi = k * 64 + 63 - __clzll((long long)m);
            }
            if (L.op == kRaAutoContrast) {
                if (hi > lo) {
                    // ImageOps.autocontrast: scale = 255.0 / (hi - lo); offset = -lo * scale; int(ix * scale + offset), clipped
                    const double scale = 255.0 / (double)(hi - lo), offset = (double)(-lo) * scale;
                    const double t = (double)i * scale + offset;
                    v = t < 0.0 ? 0 : (t > 255.0 ? 255 : (int)t);
                }
            } else {
                // ImageOps.equalize: step = (pixels - the last used bin's count) // 255; (step // 2 + the counts in front of bin i) // step
                const uint32_t step = ((uint32_t)pixels - s_hist[ch * 256 + hi]) / 255u;
                if (bins > 1 && step) v = (int)min(255u, (step / 2u + before) / step);
            }
        }
    } else if (L.op == kRaInvert) {
        v = 255 - i;
    } else if (L.op == kRaPosterize) {
        v = i & ~((1 << (8 - L.arg)) - 1) & 255;
    } else if (L.op == kRaSolarize) {
        v = i < L.arg ? i : 255 - i;
    } else if (L.op == kRaSolarizeAdd) {
        v = i < 128 ? min(255, i + L.arg) : i;
    } else if (L.op == kRaContrast) {
        v = img_blend(mean, i, L.f);
    } else if (L.op == kRaBrightness) {
        v = img_blend0(i, L.f);
    }
    if (tid < 768) s_lut[tid] = (uint8_t)v;
    __syncthreads();
}

// ---- the streaming passes: three dwords in, three dwords out per item

__device__ __forceinline__ void ra_stream_table(const uint32_t* src, uint32_t* dst, int items, const uint8_t* s_lut, int tid) {
    for (int it = tid; it < items; it += kRaThreads) {
        const uint32_t w[3] = {src[3 * it], src[3 * it + 1], src[3 * it + 2]};
        uint32_t o[3] = {0u, 0u, 0u};
#pragma unroll
        for (int k = 0; k < 12; ++k) o[k >> 2] |= (uint32_t)s_lut[(k % 3) * 256 + ra_byte(w, k)] << (8 * (k & 3));
        dst[3 * it] = o[0], dst[3 * it + 1] = o[1], dst[3 * it + 2] = o[2];
    }
}

__device__ __forceinline__ void ra_stream_copy(const uint32_t* src, uint32_t* dst, int items, int tid) {
    for (int it = tid; it < items; it += kRaThreads) {
        const uint32_t w0 = src[3 * it], w1 = src[3 * it + 1], w2 = src[3 * it + 2];
        dst[3 * it] = w0, dst[3 * it + 1] = w1, dst[3 * it + 2] = w2;
    }
}

// ImageEnhance.Color: blend(L -> RGB, image, f)
__device__ __forceinline__ void ra_stream_color(const uint32_t* src, uint32_t* dst, int items, float f, int tid) {
    for (int it = tid; it < items; it += kRaThreads) {
        const uint32_t w[3] = {src[3 * it], src[3 * it + 1], src[3 * it + 2]};
        uint32_t o[3] = {0u, 0u, 0u};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int l = img_luma(ra_byte(w, 3 * j), ra_byte(w, 3 * j + 1), ra_byte(w, 3 * j + 2));
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int k = 3 * j + c;
                o[k >> 2] |= (uint32_t)img_blend(l, ra_byte(w, k), f) << (8 * (k & 3));
            }
        }
        dst[3 * it] = o[0], dst[3 * it + 1] = o[1], dst[3 * it + 2] = o[2];
    }
}

// ImageEnhance.Sharpness: blend(image.filter(SMOOTH), image, f).  SMOOTH is (1 1 1 / 1 5 1 / 1 1 1) / 13 on the interior, floor(s / 13 + 0.5) =
// (2 s + 13) / 26 in integers, and copies the one-pixel border, where the blend of a pixel with itself is the pixel.  Per row of the 3 x 3: the item's
// three dwords, the dword in front of them (its last three bytes: the pixel to the left) and the dword behind (its first three bytes).  In the
// first and the last item of a row and in the first and the last row those neighbours are taken from inside the image and never used.
__device__ __forceinline__ void ra_stream_sharpness(const uint32_t* src, uint32_t* dst, int D, float f, int tid) {
    const int D4 = D >> 2, items = D * D4, row = 3 * D4;
    for (int it = tid; it < items; it += kRaThreads) {
        const int y = it / D4, x4 = it - y * D4;
        int q[3][18];                                                // byte k of row r: channel k % 3 of pixel 4 * x4 - 1 + k / 3
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const uint32_t* line = src + max(0, min(y + r - 1, D - 1)) * row + 3 * x4;
            const uint32_t before = line[x4 > 0 ? -1 : 0], after = line[x4 < D4 - 1 ? 3 : 2];
            const uint32_t w[3] = {line[0], line[1], line[2]};
#pragma unroll
            for (int k = 0; k < 3; ++k) q[r][k] = (int)((before >> (8 * (k + 1))) & 255u), q[r][15 + k] = (int)((after >> (8 * k)) & 255u);
#pragma unroll
            for (int k = 0; k < 12; ++k) q[r][3 + k] = ra_byte(w, k);
        }
        uint32_t o[3] = {0u, 0u, 0u};
        const bool edge_row = y == 0 || y == D - 1;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int x = 4 * x4 + j;
            const bool edge = edge_row || x == 0 || x == D - 1;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int k = 3 + 3 * j + c, centre = q[1][k];
                int s = 4 * centre;
#pragma unroll
                for (int r = 0; r < 3; ++r) s += q[r][k - 3] + q[r][k] + q[r][k + 3];
                const int smooth = edge ? centre : (2 * s + 13) / 26;
                o[(k - 3) >> 2] |= (uint32_t)img_blend(smooth, centre, f) << (8 * ((k - 3) & 3));
            }
        }
        dst[3 * it] = o[0], dst[3 * it + 1] = o[1], dst[3 * it + 2] = o[2];
    }
}

// ---- the affine ops: Pillow's ImagingGenericTransform with affine_transform and its bilinear / bicubic filter for 8-bit RGB, in double

// Pillow's BICUBIC macro, every operation in its order
__device__ __forceinline__ double ra_cubic(double v1, double v2, double v3, double v4, double d) {
    const double p2 = -v1 + v3, p3 = 2.0 * (v1 - v2) + v3 - v4, p4 = -v1 + v2 - v3 + v4;
    return v2 + d * (p2 + d * (p3 + d * p4));
}

// One output pixel: its three bytes in bits 0 .. 23.  The source point is tested the way that sends a NaN (finite entries can still overflow to
// inf - inf) to the fill; inside, 0 <= xin < D holds, the floor is an index near the image and every row and column read is clamped into it.
__device__ __forceinline__ uint32_t ra_affine_pixel(const uint8_t* src, int D, const RaLayer L, int x, int y) {
    const double xc = (double)x + 0.5, yc = (double)y + 0.5, side = (double)D;
    double xin = (L.m[0] * xc + L.m[1] * yc) + L.m[2];
    double yin = (L.m[3] * xc + L.m[4] * yc) + L.m[5];
    if (!(xin >= 0.0 && xin < side && yin >= 0.0 && yin < side)) return L.fill;
    xin -= 0.5, yin -= 0.5;
    int x0 = (int)floor(xin), y0 = (int)floor(yin);
    const double dx = xin - (double)x0, dy = yin - (double)y0;
    const int last = D - 1, pitch = 3 * D;
    uint32_t px = 0;
    if (L.arg == kRaBilinear) {
        const uint8_t* r0 = src + max(0, min(y0, last)) * pitch;
        const uint8_t* r1 = src + max(0, min(y0 + 1, last)) * pitch;
        const bool below = y0 + 1 < D;                               // (y0 + 1 >= 0 always: y0 >= -1)
        const int xa = 3 * max(0, min(x0, last)), xb = 3 * max(0, min(x0 + 1, last));
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double a = (double)r0[xa + c], b = (double)r0[xb + c], e = (double)r1[xa + c], g = (double)r1[xb + c];
            const double v1 = a + (b - a) * dx, v2 = below ? e + (g - e) * dx : v1;
            px |= ((uint32_t)(int)(v1 + (v2 - v1) * dy) & 255u) << (8 * c);
        }
    } else {
        --x0, --y0;
        int xs[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) xs[k] = 3 * max(0, min(x0 + k, last));
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            double v[4], prev = 0.0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                // row y0 clamped; a row y0 + k outside the image repeats the value of the row in front of it
                const uint8_t* r = src + max(0, min(y0 + k, last)) * pitch + c;
                const double t = ra_cubic((double)r[xs[0]], (double)r[xs[1]], (double)r[xs[2]], (double)r[xs[3]], dx);
                v[k] = prev = k == 0 || (y0 + k >= 0 && y0 + k < D) ? t : prev;
            }
            const double t = ra_cubic(v[0], v[1], v[2], v[3], dy);
            px |= (uint32_t)(t <= 0.0 ? 0 : (t >= 255.0 ? 255 : (int)t)) << (8 * c);
        }
    }
    return px;
}

__device__ __forceinline__ void ra_affine(const uint8_t* src, uint32_t* dst, int D, const RaLayer L, int tid) {
    const int D4 = D >> 2, items = D * D4;
    for (int it = tid; it < items; it += kRaThreads) {
        const int y = it / D4, x4 = it - y * D4;
        // 96 bits that move down by one pixel per step: after four steps pixel j sits in bits 24 j .. 24 j + 23
        uint64_t lo = 0;
        uint32_t hi = 0;
#pragma unroll 1
        for (int j = 0; j < 4; ++j) {
            const uint32_t px = ra_affine_pixel(src, D, L, 4 * x4 + j, y);
            lo = (lo >> 24) | ((uint64_t)(hi & 0xffffffu) << 40);
            hi = (hi >> 24) | (px << 8);
        }
        dst[3 * it] = (uint32_t)lo, dst[3 * it + 1] = (uint32_t)(lo >> 32), dst[3 * it + 2] = hi;
    }
}

// bytes is read only; scratch and out are read and written by this workgroup alone, through pointers the compiler may not take for unaliased
__global__ __launch_bounds__(kRaThreads) void k_image_randaug(const uint8_t* bytes, int D, const int32_t* __restrict__ records, int layers,
                                                              uint8_t* scratch, uint8_t* out) {
    __shared__ uint32_t s_hist[768];
    __shared__ uint64_t s_mask[kRaThreads / 64];
    __shared__ uint32_t s_red[kRaThreads / 64];
    __shared__ uint8_t s_lut[768];
    const int tid = threadIdx.x, b = blockIdx.x;
    const int items = D * (D >> 2);
    const int64_t image = (int64_t)3 * D * D;
    const int32_t* rec = records + (int64_t)b * layers * kRandaugWords;
    const uint8_t* cur = bytes + b * image;
    uint8_t* const side[2] = {scratch + b * image, out + b * image};

    int live = 0;
    for (int l = 0; l < layers; ++l) live += ra_layer(rec + l * kRandaugWords).op != 0;
    if (!live) {
        ra_stream_copy((const uint32_t*)cur, (uint32_t*)side[1], items, tid);
        return;
    }
    int to = live & 1;                                               // an odd number of layers starts in out, an even number in scratch
    for (int l = 0; l < layers; ++l) {
        const RaLayer L = ra_layer(rec + l * kRandaugWords);         // workgroup-uniform: every branch below is taken by all lanes or by none
        if (!L.op) continue;
        const uint32_t* src = (const uint32_t*)cur;
        uint32_t* dst = (uint32_t*)(to ? side[1] : side[0]);
        if (L.op >= kRaShearX) {
            ra_affine(cur, dst, D, L, tid);
        } else if (L.op == kRaSharpness) {
            ra_stream_sharpness(src, dst, D, L.f, tid);
        } else if (L.op == kRaColor) {
            ra_stream_color(src, dst, items, L.f, tid);
        } else {
            int mean = 0;
            if (L.op == kRaAutoContrast || L.op == kRaEqualize) ra_histogram(src, items, s_hist, tid);
            if (L.op == kRaContrast) mean = ra_mean_luma(src, items, s_red, tid);
            ra_table(L, mean, D * D, s_hist, s_mask, s_red, s_lut, tid);
            ra_stream_table(src, dst, items, s_lut, tid);
        }
        __threadfence();
        __syncthreads();
        __threadfence();
        cur = (const uint8_t*)dst;
        to ^= 1;
    }
}

int launch_image_randaug(const ImageRandaug& r, hipStream_t st) {
    hipLaunchKernelGGL(k_image_randaug, dim3(r.B), dim3(kRaThreads), 0, st, r.bytes, r.D, r.records, r.layers, r.scratch, r.out);
    return 0;
}

}  // namespace qv
