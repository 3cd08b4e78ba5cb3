// Input pipeline, the window stage: a window h x w of a uint8 HWC image [H, W, 3] resident on the device -> the uint8 [D, D, 3] bytes that
// Image.crop(window)[.transpose(FLIP_LEFT_RIGHT)].resize((D, D), BICUBIC) returns, for windows LARGER than the output too: Pillow's 8-bit two-pass
// resample with the filter stretched by max(n / D, 1), so a variable number of taps (include/qatvit.h states the arithmetic).  The batch launch of
// image.hip, run at S = D on these bytes, is the second stage.  Integer throughout, so the result is equal, not close.
#include <math.h>

#include <algorithm>

#include "qv_common.h"
#include "qv_kernels.h"

namespace qv {

// ---------------------------------------------------------------------------------------------------------------- host: the tables
#include "image_tables.h"

// the taps of an output of an n -> D resample that can have a weight: 4 where the filter is not stretched, else ceil(2 * support) <= floor(4 n / D) + 1.
// The kernel takes this many; the builder refuses a table with a coefficient behind them.
__host__ __device__ inline int window_taps(int n, int D) { return n <= D ? kImgTaps : (4 * n / D + 1 < kWinTaps ? 4 * n / D + 1 : kWinTaps); }

// the most rows of an n-row window that a band of kWinBand output rows reads: the centres span (kWinBand - 1) * scale, the filter 2 * support
// around them.  Not decreasing in n, so the bound of H serves every window of an image of H rows.
int image_window_max_rows(int n, int D) {
    const double scale = (double)n / (double)D, support = 2.0 * (scale > 1.0 ? scale : 1.0);
    const int rows = (int)ceil((kWinBand - 1) * scale + 2.0 * support) + 2;
    return rows < n ? rows : n;
}

int64_t image_window_coeffs_words(int max_side, int D) { return (int64_t)max_side * D * (2 + kWinTaps); }

static int window_table(int src, int dst, int32_t* xmin_out, int32_t* ntaps_out, int32_t* coef) {
    return pillow_coeffs<kWinTaps>("qatvit_image_window_coeffs", true, window_taps(src, dst), kWinBand, image_window_max_rows, src, dst, xmin_out,
                                   ntaps_out, coef);
}

int image_window_coeffs(int max_side, int D, int32_t* out) {
    for (int n = 1; n <= max_side; ++n) {
        int32_t* t = out + (int64_t)(n - 1) * D * (2 + kWinTaps);
        if (window_table(n, D, t, t + D, t + 2 * D)) return 1;
    }
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------- device
#include "image_device.h"   // kImgThreads, img_round_clip

// bytes of one staged row of a window of w pixels: its 3 w bytes behind the 0 .. 3 bytes that put them where they lie in their global dwords, rounded up to
// whole dwords with room for the largest skew: up to 3 bytes in front of the row and up to 6 behind it are staged with it
__host__ __device__ inline int window_row_bytes(int w) { return (w * 3 + 3 + 3) & ~3; }

// LDS: the band's entries of the row table, the horizontally resampled rows as HWC bytes [max_rows][D][3], and a staging buffer for source rows
struct WindowLds { int band, planes, stage; };
static WindowLds window_lds(int H, int W, int D) {
    WindowLds l;
    l.band = kWinBand * (2 + kWinTaps) * 4;
    l.planes = (image_window_max_rows(H, D) * 3 * D + 15) & ~15;
    const int want = image_window_max_rows(H, D) * window_row_bytes(W), room = kImgMixMaxLds - l.band - l.planes;
    l.stage = std::min(std::min(want, kWinStageBytes), room);
    return l;
}
int64_t image_window_lds_bytes(int H, int W, int D) {
    const WindowLds l = window_lds(H, W, D);
    return l.stage < window_row_bytes(W) ? (int64_t)kImgMixMaxLds + 1 : (int64_t)l.band + l.planes + l.stage;   // not even one row: refused
}

// The horizontal pass of one chunk of staged rows.  One item = one (output column, channel): its KT coefficients and the KT byte offsets of its
// taps in a staged row (clamped to the window, mirrored where the record says so) stay in registers over the chunk's rows, which go four at a time
// so that their LDS reads are in flight together.  KT >= the window's tap bound; the table holds 0 behind an output's own taps, and every KT <= K
// coefficients of an output lie inside its table.
template <int KT>
__device__ __forceinline__ void window_hpass(const uint8_t* __restrict__ s_stage, uint8_t* __restrict__ s_plane, const int32_t* __restrict__ ctab, int D,
                                             int crows, int c0, int stride, int skew0, int rowstep, int wlast, bool flip, int tid) {
    for (int e = tid; e < 3 * D; e += kImgThreads) {
        const int x = e / 3, c = e - 3 * x;
        const int xm = max(0, ctab[x]);
        int k[KT], at[KT];
#pragma unroll
        for (int i = 0; i < KT; ++i) {
            const int q = min(xm + i, wlast);
            k[i] = ctab[2 * D + x * kWinTaps + i];
            at[i] = (flip ? wlast - q : q) * 3 + c;
        }
        for (int r = 0; r < crows; r += 4) {
            int acc[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int rr = min(r + u, crows - 1);                 // a row past the chunk repeats the last one and is not stored
                const uint8_t* line = s_stage + rr * stride + ((skew0 + (c0 + rr) * rowstep) & 3);
                int s = 1 << (kImgBits - 1);
#pragma unroll
                for (int i = 0; i < KT; ++i) s += __mul24((int)line[at[i]], k[i]);
                acc[u] = s;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (r + u < crows) s_plane[(c0 + r + u) * 3 * D + e] = (uint8_t)img_round_clip(acc[u]);
        }
    }
}

// One workgroup = kWinBand output rows of one batch position.  The record is the workgroup's: two scalar loads, clamped as img_window clamps them
// (h to 1 .. H, w to 1 .. W, then top to 0 .. H - h and left to 0 .. W - w), so the two tables read are among the `sides` tables and every pixel
// used lies inside the window.  Source rows are staged in chunks as the aligned dwords they lie in (up to 3 bytes in front of a row and up to 6 behind it, but never
// outside `data`, come along and are not used); one item of the horizontal pass is one (output column, channel), whose coefficients stay in
// registers over the chunk's rows; one item of the vertical pass is four bytes of an output row, stored as one dword.
__global__ __launch_bounds__(kImgThreads) void k_image_window_u8(const uint8_t* __restrict__ data, const int64_t* __restrict__ index, int N, int H, int W,
                                                                 int D, int max_rows, int stage_bytes, const int32_t* __restrict__ tables,
                                                                 const int32_t* __restrict__ rrc, uint8_t* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    constexpr int K = kWinTaps;
    int32_t* s_band = (int32_t*)smem;                                  // xmin [kWinBand], then coef [kWinBand][K]
    uint8_t* s_plane = smem + kWinBand * (2 + K) * 4;                   // [max_rows][D][3]
    uint8_t* s_stage = s_plane + ((max_rows * 3 * D + 15) & ~15);       // [chunk rows][window_row_bytes(w)]

    const int tid = threadIdx.x, b = blockIdx.y;
    const int y0 = blockIdx.x * kWinBand, y1 = min(y0 + kWinBand, D);
    int64_t img = index ? index[b] : b;
    img = img < 0 ? 0 : (img >= N ? N - 1 : img);                      // the range is the caller's contract; a bad index must still not read outside data

    const int w0 = rrc[2 * b], w1 = rrc[2 * b + 1];
    const int h = max(1, min(w1 & 0x7fff, H)), w = max(1, min((w1 >> 15) & 0x7fff, W));
    const int top = min(w0 & 0xffff, H - h), left = min((w0 >> 16) & 0xffff, W - w);
    const bool flip = (w1 >> 30) & 1;
    const int tab_words = D * (2 + K);
    const int32_t* ctab = tables + (int64_t)(w - 1) * tab_words;       // the table of w -> D: xmin[D], ntaps[D], coef[D][K]
    const int32_t* rtab = tables + (int64_t)(h - 1) * tab_words;       // the table of h -> D
    const int ktaps = window_taps(w, D), vtaps = window_taps(h, D);     // workgroup-uniform; taps past an output's own count have coefficient 0

    // rows of the window this band reads, clamped so that tables other than the builder's cannot send a read outside the window or the planes
    int r0 = rtab[y0], r1 = rtab[y1 - 1] + rtab[D + y1 - 1];
    r0 = max(0, min(r0, h - 1));
    r1 = max(r0 + 1, min(r1, min(h, r0 + max_rows)));
    const int nrows = r1 - r0;

    for (int i = tid; i < y1 - y0; i += kImgThreads) s_band[i] = rtab[y0 + i];
    for (int i = tid; i < (y1 - y0) * K; i += kImgThreads) s_band[kWinBand + i] = rtab[2 * D + y0 * K + i];

    const int wlast = w - 1, stride = window_row_bytes(w), stride4 = stride / 4;
    const int chunk_rows = max(1, stage_bytes / stride);
    const int64_t total = (int64_t)N * H * W * 3;
    const int64_t first = ((img * H + top + r0) * (int64_t)W + left) * 3;     // byte offset in data of the window's row r0
    // where a row's first byte lies in its global dword: row r of the band's rows has the skew (skew0 + r * rowstep) & 3
    const int skew0 = (int)(((uintptr_t)data + (uintptr_t)first) & 3), rowstep = (W * 3) & 3;
    for (int c0 = 0; c0 < nrows; c0 += chunk_rows) {
        const int crows = min(chunk_rows, nrows - c0);
        if (c0) __syncthreads();                                       // the horizontal pass of the chunk before has read s_stage
        for (int it = tid; it < crows * stride4; it += kImgThreads) {
            const int r = it / stride4, j = it - r * stride4;
            const int64_t off = first + (int64_t)(c0 + r) * W * 3;
            const int skew = (skew0 + (c0 + r) * rowstep) & 3;
            const int64_t at = off - skew + 4 * j;                       // an aligned dword; inside data but for the first and the last one of data
            uint32_t v;
            if (at >= 0 && at + 4 <= total) {
                v = *(const uint32_t*)(data + at);
            } else {
                v = 0;
                for (int k = 0; k < 4; ++k)
                    if (at + k >= 0 && at + k < total) v |= (uint32_t)data[at + k] << (8 * k);
            }
            ((uint32_t*)s_stage)[it] = v;
        }
        __syncthreads();
        // horizontal pass of the chunk's rows, with the tap loop unrolled to the tier of this window's width
        if (ktaps <= 4) window_hpass<4>(s_stage, s_plane, ctab, D, crows, c0, stride, skew0, rowstep, wlast, flip, tid);
        else if (ktaps <= 8) window_hpass<8>(s_stage, s_plane, ctab, D, crows, c0, stride, skew0, rowstep, wlast, flip, tid);
        else if (ktaps <= 12) window_hpass<12>(s_stage, s_plane, ctab, D, crows, c0, stride, skew0, rowstep, wlast, flip, tid);
        else window_hpass<kWinTaps>(s_stage, s_plane, ctab, D, crows, c0, stride, skew0, rowstep, wlast, flip, tid);
    }
    __syncthreads();

    // vertical pass + store: the planes are HWC as the output is, so a dword of the output row takes the same dword of every tap's plane row
    const int D34 = 3 * D / 4, last = nrows - 1;
    uint32_t* obase = (uint32_t*)(out + ((int64_t)b * D + y0) * D * 3);
    for (int it = tid; it < (y1 - y0) * D34; it += kImgThreads) {
        const int yy = it / D34, j = it - yy * D34;
        const int rel = s_band[yy] - r0;
        const int32_t* kk = s_band + kWinBand + yy * K;
        int acc[4] = {1 << (kImgBits - 1), 1 << (kImgBits - 1), 1 << (kImgBits - 1), 1 << (kImgBits - 1)};
        for (int i = 0; i < vtaps; ++i) {
            const uint32_t t = ((const uint32_t*)s_plane)[max(0, min(rel + i, last)) * D34 + j];
            const int kv = kk[i];
#pragma unroll
            for (int l = 0; l < 4; ++l) acc[l] += __mul24((int)((t >> (8 * l)) & 255), kv);
        }
        int px[4];
#pragma unroll
        for (int l = 0; l < 4; ++l) px[l] = img_round_clip(acc[l]);
        // packed through v_perm_b32, as image_kernel.h packs (the plain shift-clamp-or chain is miscompiled on this target)
        obase[it] = __builtin_amdgcn_perm((uint32_t)(px[2] | px[3] << 16), (uint32_t)(px[0] | px[1] << 16), 0x06040200u);
    }
}

int launch_image_window(const ImageWindow& r, hipStream_t st) {
    const int64_t lds = image_window_lds_bytes(r.H, r.W, r.D);
    if (lds > kImgMixMaxLds) {
        set_error("qatvit_image_window_u8: source %d x %d -> output %d needs more than %d bytes of LDS", r.H, r.W, r.D, kImgMixMaxLds);
        return 1;
    }
    const dim3 grid((r.D + kWinBand - 1) / kWinBand, r.B);
    hipLaunchKernelGGL(k_image_window_u8, grid, dim3(kImgThreads), (size_t)lds, st, r.data, r.index, r.N, r.H, r.W, r.D, image_window_max_rows(r.H, r.D),
                       window_lds(r.H, r.W, r.D).stage, r.tables, r.rrc, r.out);
    return 0;
}

}  // namespace qv
