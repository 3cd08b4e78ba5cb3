// Input pipeline, the bytes-in blur form: the chain of the blur forms (image_blur.h) behind the resize, on bytes that ARE the resized image - the
// uint8 [B][D][D][3] that the window stage (image_window.hip) writes at batch positions.  No column table, no source rows, no plane set of a
// horizontal pass: LDS holds the value table and the image buffers only, so the form fits where k_image_blur at S = D does not (D = 224:
// 89,536 bytes there, 40,704 here).  A source file of its own: the machine code of every other kernel stays what it was.
// One template, k_image_bytes_blur<DT, MIX, STAT>, with the meaning these switches have in k_image_blur.  Per side, with the cleaned blur record:
//   on     rows e0 .. e1-1 = the band and 3 * (radius + 1) rows on each side, clamped to 0 .. D, are ONE contiguous span of (e1 - e0) * 3 * D bytes
//          of the sample, 4-byte aligned (D % 4 == 0).  One item = four neighbouring pixels = 12 bytes = three dwords from global memory,
//          de-interleaved into three plane dwords by v_perm_b32, through grayscale / solarize, into s_img[side] as planes [row][c][D]; then the
//          six passes between s_img[side] and s_pp with a barrier behind each (img_blur_pass, as it is), then the store loop of k_image_blur.
//   off    nothing is staged and no pass runs: the store loop reads the band's items straight from global memory and runs the whole colour chain,
//          which is bitwise what the colour forms give at S = D (their two resize passes are the identity there).
// Every branch on a record is workgroup-uniform: the records come through scalar loads of words indexed by blockIdx.y.
// LDS: the value table (3072 bytes), then (sides + 1) image buffers of (band + 12) * 3 * D bytes.  Without mix records the band is 16 rows where
// that fits 64 KB (D <= 368), else 8 (D = 372 .. 384: 49,152 bytes at 384); with mix records it is 8, served up to D = 344 (64,992 bytes) and
// refused above.  D = 224: 3072 + 2 * 28 * 672 = 40,704 bytes, with mix 3072 + 3 * 20 * 672 = 43,392.
#include <math.h>

#include "qv_common.h"
#include "qv_kernels.h"

namespace qv {

#include "image_device.h"
#include "image_blur.h"   // the record rules, img_blur_pass, img_blur_fetch, img_pack4 (k_image_blur is a template that nothing here instantiates)

constexpr int kImgBytesTable = 768 * 4;

__host__ __device__ inline int64_t img_bytes_blur_lds(int D, int band, int sides) {
    return kImgBytesTable + (int64_t)(sides + 1) * (band + 2 * kImgBlurHalo) * 3 * D;
}

int image_bytes_blur_band(int D, bool mixed) {
    return !mixed && img_bytes_blur_lds(D, kImgBlurBand, 1) <= kImgMixMaxLds ? kImgBlurBand : kImgBlurMixBand;
}

int64_t image_bytes_blur_lds_bytes(int D, bool mixed) { return img_bytes_blur_lds(D, image_bytes_blur_band(D, mixed), mixed ? 2 : 1); }

// One item: the twelve bytes R0 G0 B0 R1 | G1 B1 R2 G2 | B2 R3 G3 B3 of four neighbouring HWC pixels -> one dword per plane, pixel j in byte j.
// v_perm_b32 picks each result byte out of the eight bytes {first operand : second operand}: two per plane.
__device__ __forceinline__ void img_bytes_load4(const uint32_t* __restrict__ item, uint32_t pl[3]) {
    const uint32_t w0 = item[0], w1 = item[1], w2 = item[2];
    pl[0] = __builtin_amdgcn_perm(w2, __builtin_amdgcn_perm(w1, w0, 0x00060300u), 0x05020100u);
    pl[1] = __builtin_amdgcn_perm(w2, __builtin_amdgcn_perm(w1, w0, 0x00070401u), 0x06020100u);
    pl[2] = __builtin_amdgcn_perm(w2, __builtin_amdgcn_perm(w1, w0, 0x00000502u), 0x07040100u);
}

__device__ __forceinline__ void img_bytes_unpack(const uint32_t pl[3], int px[3][4]) {
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int j = 0; j < 4; ++j) px[c][j] = (int)((pl[c] >> (8 * j)) & 255u);
}

template <int DT, bool MIX, bool STAT>
__global__ __launch_bounds__(kImgThreads) void k_image_bytes_blur(const uint8_t* __restrict__ bytes, int D_rt, int band, const float* __restrict__ table,
                                                                  float* __restrict__ out, const int32_t* __restrict__ mix,
                                                                  const int32_t* __restrict__ erase, const int32_t* __restrict__ color,
                                                                  const uint32_t* __restrict__ sums, uint32_t* __restrict__ sums_out,
                                                                  const int32_t* __restrict__ blur) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    constexpr int kSides = MIX ? 2 : 1;
    const int D = DT ? DT : D_rt, D4 = D / 4;
    const int img_bytes = (band + 2 * kImgBlurHalo) * 3 * D;
    float* s_table = (float*)smem;                       // [3][256]
    uint32_t* s_pp = (uint32_t*)(smem + kImgBytesTable + kSides * img_bytes);

    const int tid = threadIdx.x, b = blockIdx.y;
    const int y0 = blockIdx.x * band, y1 = min(y0 + band, D);
    int p = b, sides = 1;
    float w_self = 1.0f, w_partner = 0.0f;
    int by0 = 0, by1 = 0, bx0 = 0, bx1 = 0;
    bool box = false, as_is = true;
    if (MIX) {
        // as k_image_blur: a partner outside the batch is the sample itself; the box is clamped to the output
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
    bl[0] = img_blur(blur + 4 * b);
    if (MIX) {
        col[kSides - 1] = sides == 2 && color ? img_color(color + 4 * p, sums, p, D, false) : col[0];
        bl[kSides - 1] = sides == 2 ? img_blur(blur + 4 * p) : bl[0];
    }
    int e0s[kSides];
    const uint32_t* image[kSides];                       // the sample's dwords, and the partner's

    if (!STAT)
        for (int i = tid; i < 768; i += kImgThreads) s_table[i] = table[i];

#pragma unroll
    for (int side = 0; side < kSides; ++side) {
        e0s[side] = y0;
        image[side] = (const uint32_t*)(bytes + (int64_t)(side ? p : b) * 3 * D * D);
        if (side < sides && bl[side].on) {
            const ImgBlur sb = bl[side];
            const int halo = 3 * (sb.radius + 1);
            const int e0 = max(0, y0 - halo), e1 = min(D, y1 + halo), erows = e1 - e0;
            uint32_t* s_img = (uint32_t*)(smem + kImgBytesTable + side * img_bytes);
            // rows e0 .. e1-1 of the image behind grayscale / solarize: item `it` of the span is its dwords 3 * it .. 3 * it + 2
            const ImgColor front = img_color_front(col[side]);
            const uint32_t* span = image[side] + (int64_t)e0 * 3 * D4;
            for (int it = tid; it < erows * D4; it += kImgThreads) {
                const int ry = it / D4, x4 = it - ry * D4;
                uint32_t pl[3];
                img_bytes_load4(span + 3 * it, pl);
                if (front.any) {
                    int px[3][4];
                    img_bytes_unpack(pl, px);
                    img_color_apply(front, px);
#pragma unroll
                    for (int c = 0; c < 3; ++c) pl[c] = img_pack4(px[c]);
                }
#pragma unroll
                for (int c = 0; c < 3; ++c) s_img[(ry * 3 + c) * D4 + x4] = pl[c];
            }
            e0s[side] = e0;
            __syncthreads();
#pragma unroll 1
            for (int pass = 0; pass < 6; ++pass) {
                img_blur_pass(pass & 1 ? s_pp : s_img, pass & 1 ? s_img : s_pp, erows, D4, pass >= 3, sb, tid);
                __syncthreads();
            }
        }
    }
    __syncthreads();

    // the store loop of k_image_blur: one item = four neighbouring pixels of one output row in all three channels, from the blurred image (then
    // the jitter ops) or from global memory (then the whole chain); the value table, the erase, the mix, three float4 stores
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
                int px[3][4];
                if (bl[side].on) {
                    const uint32_t* s_img = (const uint32_t*)(smem + kImgBytesTable + side * img_bytes);
                    img_blur_fetch(s_img, D4, y - e0s[side], x4, px);
                    img_color_apply(img_color_back(col[side]), px);
                } else {
                    uint32_t pl[3];
                    img_bytes_load4(image[side] + ((int64_t)y0 * D4 + it) * 3, pl);
                    img_bytes_unpack(pl, px);
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
                // out = inside the box ? partner : fl(fl(w_self * own) + fl(w_partner * partner)); one side: the partner is the sample
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
        // as the other statistics forms: the waves by shuffles, the wave sums through LDS (the value table's place, which this form does not
        // fill), one integer atomic per workgroup
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) lsum += __shfl_down(lsum, off);
        uint32_t* s_part = (uint32_t*)s_table;
        if ((tid & 63) == 0) s_part[tid >> 6] = lsum;
        __syncthreads();
        if (tid == 0) {
            uint32_t total = 0;
            for (int i = 0; i < kImgThreads / 64; ++i) total += s_part[i];
            atomicAdd(sums_out + b, total);
        }
    }
}

template <bool MIX, bool STAT>
static void image_bytes_blur_launch(const ImageBytesBlur& r, hipStream_t st) {
    const int band = image_bytes_blur_band(r.D, MIX);
    const dim3 grid((r.D + band - 1) / band, r.B);
    const auto kernel = r.D == 224 ? k_image_bytes_blur<224, MIX, STAT> : k_image_bytes_blur<0, MIX, STAT>;
    hipLaunchKernelGGL(kernel, grid, dim3(kImgThreads), (size_t)image_bytes_blur_lds_bytes(r.D, MIX), st, r.bytes, r.D, band, STAT ? nullptr : r.table,
                       STAT ? nullptr : r.out, MIX ? r.mix : nullptr, STAT ? nullptr : r.erase, r.color, STAT ? nullptr : r.sums,
                       STAT ? r.sums : nullptr, r.blur);
}

// The statistics launch and the zeroing of sums as launch_image_blur has them: with colour records and a workspace, in front of the batch launch
int launch_image_bytes_blur(const ImageBytesBlur& r, hipStream_t st) {
    const char* who = "qatvit_image_bytes_blur";
    const bool mixed = r.mix != nullptr;
    const int64_t lds = image_bytes_blur_lds_bytes(r.D, mixed);
    if (lds > kImgMixMaxLds) {
        set_error("%s: output %d needs %lld bytes of LDS for the value table and %d image buffers of %d rows, more than %d", who, r.D, (long long)lds,
                  mixed ? 3 : 2, image_bytes_blur_band(r.D, mixed) + 2 * kImgBlurHalo, kImgMixMaxLds);
        return 1;
    }
    if (r.color && r.sums) {
        const hipError_t e = hipMemsetAsync(r.sums, 0, (size_t)r.B * sizeof(uint32_t), st);
        if (e != hipSuccess) {
            set_error("%s: zeroing sums failed: %s", who, hipGetErrorString(e));
            return 2;
        }
        image_bytes_blur_launch<false, true>(r, st);
    }
    if (mixed) image_bytes_blur_launch<true, false>(r, st);
    else image_bytes_blur_launch<false, false>(r, st);
    return 0;
}

}  // namespace qv
