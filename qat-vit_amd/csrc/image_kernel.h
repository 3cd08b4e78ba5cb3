// The kernel of image.hip, which includes this text once per form: fifteen times, each behind one line
//     #define QV_IMAGE_FORM (name, AUG, MIX, RRC, ERASE, COLOR)
// that names the kernel and states all five switches.  This text reads them as QV_IMAGE_NAME and QV_IMAGE_AUG .. QV_IMAGE_COLOR and undefines all of
// it at its end, so no inclusion inherits anything from the one before.  No include guard.
//   AUG 1            the staged source rows are rows of the augmented image A (include/qatvit.h), fetched through the word aug[b]; everything behind
//                    the staging is the same text.  AUG 0, RRC 0 is the plain k_image_batch<DT>.
//   MIX 1            the staging and the horizontal pass run once for the sample and, where the workgroup's band needs it, once more for the partner of
//                    its mix record into a second plane set; the vertical pass then forms both values of an element and blends or selects them.
//   RRC 1 (AUG 0)    the source of a sample is the window h x w at (top, left) of its record rrc[b], so every side has its own column table (of w),
//                    its own entries of the row table (of h) and its own source rows.
//   ERASE 1          the vertical pass replaces the elements inside the box of the side's erase record right after it has formed them, so what is
//                    blended or selected is the erased sample and the erased partner.  The aug form of this switch takes aug == NULL as the zero word.
//   COLOR 1 (ERASE 1) the erasing forms with the colour record of the side applied to the uint8 pixels between the vertical pass and the value table,
//                    so their vertical pass has another item, four pixels in all three channels, and erase == NULL stands for all-zero erase records.
//   COLOR 2          k_image_stat_aug<DT> / k_image_stat_rrc<DT>, the statistics launch in front of the colour forms: the same staging and passes, the
//                    chain up to the contrast op, and the sum of the luma into sums[b]; no table, no output.
// The forms built: (AUG, MIX) = (0, 0), (1, 0), (1, 1) without RRC and MIX = 0, 1 with it, each with ERASE = COLOR = 0; the same without the plain one
// at ERASE 1, COLOR 0 and at ERASE 1, COLOR 1; the two statistics forms.
// Text, not a shared __device__ function: inlined into two kernels, the common body changed the instruction schedule of k_image_batch<0>, and the
// older kernels are to stay the machine code they were.  The directives of a switch add text for its own forms only: with the switch at 0 the other
// kernels are compiled from the token sequence they had (profiles/augment_bench.txt, rrc_bench.txt, erase_bench.txt, color_bench.txt).
// DT = the output size as a constant (its divisions become multiplications), or 0: taken from D_rt.
#define QV_IMAGE_PICK(field, form) field form
#define QV_IMAGE_FIELD_NAME(name, aug, mix, rrc, erase, color) name
#define QV_IMAGE_FIELD_AUG(name, aug, mix, rrc, erase, color) aug
#define QV_IMAGE_FIELD_MIX(name, aug, mix, rrc, erase, color) mix
#define QV_IMAGE_FIELD_RRC(name, aug, mix, rrc, erase, color) rrc
#define QV_IMAGE_FIELD_ERASE(name, aug, mix, rrc, erase, color) erase
#define QV_IMAGE_FIELD_COLOR(name, aug, mix, rrc, erase, color) color
#define QV_IMAGE_NAME QV_IMAGE_PICK(QV_IMAGE_FIELD_NAME, QV_IMAGE_FORM)
#define QV_IMAGE_AUG QV_IMAGE_PICK(QV_IMAGE_FIELD_AUG, QV_IMAGE_FORM)
#define QV_IMAGE_MIX QV_IMAGE_PICK(QV_IMAGE_FIELD_MIX, QV_IMAGE_FORM)
#define QV_IMAGE_RRC QV_IMAGE_PICK(QV_IMAGE_FIELD_RRC, QV_IMAGE_FORM)
#define QV_IMAGE_ERASE QV_IMAGE_PICK(QV_IMAGE_FIELD_ERASE, QV_IMAGE_FORM)
#define QV_IMAGE_COLOR QV_IMAGE_PICK(QV_IMAGE_FIELD_COLOR, QV_IMAGE_FORM)
#if QV_IMAGE_RRC
#define QV_IMAGE_XLAST xlast   // the last column of the window
#else
#define QV_IMAGE_XLAST S - 1
#endif
// the signature: one head, then the tail of the source (coeffs or windows) and the tail of the records; the statistics forms have their own tails
template <int DT>
__global__ __launch_bounds__(kImgThreads) void QV_IMAGE_NAME(const uint8_t* __restrict__ data, const int64_t* __restrict__ index, int N, int S, int D_rt,
                                                             int max_rows,
#if QV_IMAGE_COLOR == 2 && QV_IMAGE_RRC
                                                             const int32_t* __restrict__ windows, const int32_t* __restrict__ rrc,
                                                             const int32_t* __restrict__ color, uint32_t* __restrict__ sums) {
#elif QV_IMAGE_COLOR == 2
                                                             const int32_t* __restrict__ coeffs, const int32_t* __restrict__ aug, int reflect, int fill,
                                                             const int32_t* __restrict__ color, uint32_t* __restrict__ sums) {
#else
#if QV_IMAGE_RRC
                                                             const int32_t* __restrict__ windows, const float* __restrict__ table,
                                                             float* __restrict__ out, const int32_t* __restrict__ rrc
#else
                                                             const int32_t* __restrict__ coeffs, const float* __restrict__ table, float* __restrict__ out
#if QV_IMAGE_AUG
                                                             , const int32_t* __restrict__ aug, int reflect, int fill
#endif
#endif
#if QV_IMAGE_MIX
                                                             , const int32_t* __restrict__ mix
#endif
#if QV_IMAGE_ERASE
                                                             , const int32_t* __restrict__ erase
#endif
#if QV_IMAGE_COLOR
                                                             , const int32_t* __restrict__ color, const uint32_t* __restrict__ sums
#endif
                                                             ) {
#endif
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int D = DT ? DT : D_rt;
    const int row_bytes = S * 3, src_bytes = (max_rows * row_bytes + 15) & ~15;
    int32_t* s_xmin = (int32_t*)smem;                    // [D]
    int32_t* s_coef = s_xmin + D;                        // [D][4]
    float* s_table = (float*)(s_coef + D * kImgTaps);    // [3][256]
    uint8_t* s_src = (uint8_t*)(s_table + 768);          // [max_rows][S][3]
#if QV_IMAGE_MIX
    uint8_t* s_planes = s_src + src_bytes;               // [2][max_rows][3][D]: the sample's planes, then its partner's
    const int plane_bytes = max_rows * 3 * D;
#else
    uint8_t* s_tmp = s_src + src_bytes;                  // [max_rows][3][D]
#endif
#if QV_IMAGE_RRC
    // behind what the other forms keep, on the next 16 bytes (image_rrc_lds_bytes): per side, the band's entries of the row table,
    // xmin [kImgBand] then coef [kImgBand][4].  s_xmin and s_coef hold the column table of the side whose horizontal pass runs.
    int32_t* s_band = (int32_t*)(s_src + ((src_bytes + (QV_IMAGE_MIX + 1) * max_rows * 3 * D + 15) & ~15));
#endif

    const int tid = threadIdx.x, b = blockIdx.y;
    const int y0 = blockIdx.x * kImgBand, y1 = min(y0 + kImgBand, D);
#if QV_IMAGE_MIX
    // the record is the workgroup's: six scalar loads.  A partner outside the batch is the sample itself; the box is clamped to the output.
    const int32_t* rec = mix + b * 6;
    const int p = (unsigned)rec[0] < gridDim.y ? rec[0] : b;
    const float w_self = __int_as_float(rec[1]), w_partner = __int_as_float(rec[2]);
    const int by0 = min(rec[3] & 0xffff, D), by1 = min((rec[3] >> 16) & 0xffff, D);
    const int bx0 = min(rec[4] & 0xffff, D), bx1 = min((rec[4] >> 16) & 0xffff, D);
    const bool box = by1 > by0 && bx1 > bx0;
    // one plane set serves both operands unless this band takes something from another position
    const bool partner = w_partner != 0.0f || (box && by0 < y1 && by1 > y0);
    const int sides = partner && p != b ? 2 : 1;
    // nothing of the partner and the sample's weight 1: fl(1 * v) + fl(0 * v) is v, and the band stores what the aug kernel stores
    const bool as_is = !partner && w_self == 1.0f;
#endif
#if QV_IMAGE_COLOR == 2
    // the statistics form: the chain of the workgroup's record up to its contrast op; a record without one asks for nothing
    const ImgColor col_b = img_color(color + 4 * b, nullptr, b, D, true);
    if (!col_b.contrast) return;
#elif QV_IMAGE_COLOR
    // the colour record is the workgroup's (and its partner's, where the band takes something from it): four scalar loads per side, cleaned,
    // and the side's sum of the statistics launch (img_color, image.hip)
    const ImgColor col_b = img_color(color + 4 * b, sums, b, D, false);
#if QV_IMAGE_MIX
    const ImgColor col_p = sides == 2 ? img_color(color + 4 * p, sums, p, D, false) : col_b;
#endif
#endif
    int64_t img = index ? index[b] : b;
    img = img < 0 ? 0 : (img >= N ? N - 1 : img);        // the range is the caller's contract; a bad index must still not read outside data

#if QV_IMAGE_RRC
    // the window of the sample (and of its partner, where the band needs it): the record's two scalar loads, clamped, and the source rows of
    // this band out of the row table of its h (img_window, image.hip)
    const ImgWindow win_b = img_window(rrc + 2 * b, windows, S, D, y0, y1, max_rows);
#if QV_IMAGE_MIX
    const ImgWindow win_p = sides == 2 ? img_window(rrc + 2 * p, windows, S, D, y0, y1, max_rows) : win_b;
#endif
#if QV_IMAGE_COLOR != 2
    for (int i = tid; i < 768; i += kImgThreads) s_table[i] = table[i];
#endif
#else
    // rows of the source this band reads; clamped so that tables other than qatvit_image_resize_coeffs' cannot send a read outside the image
    int r0 = coeffs[y0], r1 = coeffs[y1 - 1] + coeffs[D + y1 - 1];
    r0 = max(0, min(r0, S - 1));
    r1 = max(r0 + 1, min(r1, min(S, r0 + max_rows)));
    const int nrows = r1 - r0;

    for (int i = tid; i < D; i += kImgThreads) s_xmin[i] = coeffs[i];
    for (int i = tid; i < D * kImgTaps; i += kImgThreads) s_coef[i] = coeffs[2 * D + i];
#if QV_IMAGE_COLOR != 2
    for (int i = tid; i < 768; i += kImgThreads) s_table[i] = table[i];
#endif
#endif
#if QV_IMAGE_MIX
    for (int side = 0; side < sides; ++side) {
    uint8_t* s_tmp = s_planes + side * plane_bytes;
    if (side) {
        __syncthreads();                                 // the sample's horizontal pass has read s_src
        img = index ? index[p] : p;
        img = img < 0 ? 0 : (img >= N ? N - 1 : img);
    }
#if QV_IMAGE_RRC
    const ImgWindow win = side ? win_p : win_b;
#else
    const int w = aug ? aug[side ? p : b] : 0;           // no words: the zero word, which is the plain image
#endif
#elif QV_IMAGE_RRC
    const int side = 0;
    const ImgWindow win = win_b;
#elif QV_IMAGE_AUG && QV_IMAGE_ERASE
    const int w = aug ? aug[b] : 0;                      // no words: the zero word, as the mix form has it
#elif QV_IMAGE_AUG
    const int w = aug[b];
#endif
#if QV_IMAGE_RRC
    // this side's tables (behind the barrier above where the other side's horizontal pass has read s_xmin and s_coef): the column table of its w,
    // and of the row table of its h the band's entries only
    const int r0 = win.r0, nrows = win.nrows, xlast = win.w - 1;
    for (int i = tid; i < D; i += kImgThreads) s_xmin[i] = win.ctab[i];
    for (int i = tid; i < D * kImgTaps; i += kImgThreads) s_coef[i] = win.ctab[2 * D + i];
    int32_t* band = s_band + side * kImgBand * (1 + kImgTaps);
    for (int i = tid; i < y1 - y0; i += kImgThreads) band[i] = win.rtab[y0 + i];
    for (int i = tid; i < (y1 - y0) * kImgTaps; i += kImgThreads) band[kImgBand + i] = win.rtab[2 * D + y0 * kImgTaps + i];
    // one item = one pixel of the window's rows r0 .. r1-1, mirrored where the record says so.  img_window's clamps keep top + r0 + r below
    // top + h <= S and left + sx below left + w <= S whatever the record holds.
    const uint8_t* image = data + (img * S + win.top + r0) * (int64_t)row_bytes + win.left * 3;
    for (int i = tid; i < nrows * win.w; i += kImgThreads) {
        const int r = i / win.w, x = i - r * win.w;
        const uint8_t* px = image + r * row_bytes + (win.flip ? xlast - x : x) * 3;
        uint8_t* dst = s_src + r * row_bytes + x * 3;
        dst[0] = px[0];
        dst[1] = px[1];
        dst[2] = px[2];
    }
#elif QV_IMAGE_AUG
    // one item = one pixel of the rows r0 .. r1-1 of A.  The word is the workgroup's (blockIdx.y): one scalar load.  Both coordinates are clamped
    // after the reflection, so the three byte loads stay inside the image whatever the word holds; in constant mode their result is replaced.
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
#else
    const uint8_t* src = data + (img * S + r0) * (int64_t)row_bytes;
    const int nbytes = nrows * row_bytes;
    if ((((uintptr_t)src | (uintptr_t)nbytes) & 3) == 0) {
        for (int i = tid; i < nbytes / 4; i += kImgThreads) ((uint32_t*)s_src)[i] = ((const uint32_t*)src)[i];
    } else {
        for (int i = tid; i < nbytes; i += kImgThreads) s_src[i] = src[i];
    }
#endif
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
            acc += __mul24((int)line[min(p, QV_IMAGE_XLAST) * 3], k.x);
            acc += __mul24((int)line[min(p + 1, QV_IMAGE_XLAST) * 3], k.y);
            acc += __mul24((int)line[min(p + 2, QV_IMAGE_XLAST) * 3], k.z);
            acc += __mul24((int)line[min(p + 3, QV_IMAGE_XLAST) * 3], k.w);
            px[j] = img_round_clip(acc);
        }
        // packed through v_perm_b32: hipcc turns the plain (shift, clamp, | << 8) pair into v_ashr_pk_u8_i32 and then takes the upper half of its
        // result for zero, which on the MI355X it is not (bytes 2 and 3 of the dword came out wrong)
        ((uint32_t*)s_tmp)[rc * D4 + x4] = __builtin_amdgcn_perm((uint32_t)(px[2] | px[3] << 16), (uint32_t)(px[0] | px[1] << 16), 0x06040200u);
    }
#if QV_IMAGE_MIX
    }
    const int D4 = D / 4;
    const uint8_t* s_tmp = s_planes;
    const int partner4 = (sides - 1) * (plane_bytes / 4);
#if QV_IMAGE_RRC
    const int r0 = win_b.r0, nrows = win_b.nrows;
#endif
#endif
#if QV_IMAGE_COLOR == 1
    // the erase records as below; no records (erase == NULL) are all-zero records
    const ImgErase er_b = erase ? img_erase(erase + 8 * b, D, y0, y1) : img_erase_none();
#if QV_IMAGE_MIX
    const ImgErase er_p = sides == 2 && erase ? img_erase(erase + 8 * p, D, y0, y1) : er_b;
#endif
#elif QV_IMAGE_ERASE && !QV_IMAGE_COLOR
    // the erase record is the workgroup's (and its partner's, where the band takes something from it): eight scalar loads per side, clamped;
    // `touched` is workgroup-uniform, and a band that no box meets runs what the form without the switch runs (img_erase, image.hip)
    const ImgErase er_b = img_erase(erase + 8 * b, D, y0, y1);
#if QV_IMAGE_MIX
    const ImgErase er_p = sides == 2 ? img_erase(erase + 8 * p, D, y0, y1) : er_b;
#endif
#endif
    __syncthreads();

#if QV_IMAGE_COLOR
    // vertical pass of the colour forms: one item = four neighbouring pixels of one output row in ALL THREE channels (grayscale, saturation and
    // the luma need them together).  The chain runs on the integers the vertical pass has formed; behind it stand the three lookups in the
    // value table, the erase, the mix and three float4 stores - or, in the statistics forms, nothing but the luma sum.
    const int band4 = (y1 - y0) * D4;
#if QV_IMAGE_COLOR == 2
    uint32_t lsum = 0;
#else
    float* obase = out + (int64_t)b * 3 * D * D + (int64_t)y0 * D;
#endif
    for (int it = tid; it < band4; it += kImgThreads) {
        const int y = y0 + it / D4, x4 = it % D4;
#if QV_IMAGE_RRC
        const int4 k = ((const int4*)(s_band + kImgBand))[y - y0];
        const int rel = s_band[y - y0] - r0, last = nrows - 1;
#else
        const int4 k = ((const int4*)s_coef)[y];
        const int rel = s_xmin[y] - r0, last = nrows - 1;
#endif
        const uint32_t* plane = (const uint32_t*)s_tmp + x4;
        int px[3][4];
        img_vertical4(plane, D4, rel, last, k, px);
        img_color_apply(col_b, px);
#if QV_IMAGE_COLOR == 2
#pragma unroll
        for (int j = 0; j < 4; ++j) lsum += (uint32_t)img_luma(px[0][j], px[1][j], px[2][j]);
#else
        float v[3][4];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
#pragma unroll
            for (int j = 0; j < 4; ++j) v[c][j] = s_table[c * 256 + px[c][j]];
            if (er_b.touched) img_erase_apply(er_b, c, y, x4, D4, v[c]);
        }
#if QV_IMAGE_MIX
        // as the forms without colour: the partner's value of the same elements, coloured by the partner's record with the partner's sum
        // and erased by the partner's record, then the blend or the box
        if (!as_is) {
            float u[3][4];
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int j = 0; j < 4; ++j) u[c][j] = v[c][j];
            if (sides == 2) {
#if QV_IMAGE_RRC
                const int32_t* band_p = s_band + kImgBand * (1 + kImgTaps);
                const int4 k = ((const int4*)(band_p + kImgBand))[y - y0];
                const int rel = band_p[y - y0] - win_p.r0, last = win_p.nrows - 1;
#endif
                img_vertical4(plane + partner4, D4, rel, last, k, px);
                img_color_apply(col_p, px);
#pragma unroll
                for (int c = 0; c < 3; ++c) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) u[c][j] = s_table[c * 256 + px[c][j]];
                    if (er_p.touched) img_erase_apply(er_p, c, y, x4, D4, u[c]);
                }
            }
            const bool row_in = box && y >= by0 && y < by1;
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int x = x4 * 4 + j;
                    const float a = w_self * v[c][j], c2 = w_partner * u[c][j];
                    v[c][j] = row_in && x >= bx0 && x < bx1 ? u[c][j] : a + c2;
                }
        }
#endif
#pragma unroll
        for (int c = 0; c < 3; ++c)
            *(float4*)(obase + (int64_t)c * D * D + (int64_t)it * 4) = make_float4(v[c][0], v[c][1], v[c][2], v[c][3]);
#endif
    }
#if QV_IMAGE_COLOR == 2
    // the workgroup's sum: the waves by shuffles, the four wave sums through the first words of s_src (dead behind the horizontal pass), and one
    // integer atomic per workgroup - integer adds commute, so sums[b] is exact whatever the order of the workgroups
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) lsum += __shfl_down(lsum, off);
    uint32_t* s_part = (uint32_t*)s_src;
    if ((tid & 63) == 0) s_part[tid >> 6] = lsum;
    __syncthreads();
    if (tid == 0) {
        uint32_t total = 0;
        for (int i = 0; i < kImgThreads / 64; ++i) total += s_part[i];
        atomicAdd(sums + b, total);
    }
#endif
}
#else
    // vertical pass + value table + store
    const int band4 = (y1 - y0) * D4;
    float* obase = out + (int64_t)b * 3 * D * D + (int64_t)y0 * D;
    for (int it = tid; it < 3 * band4; it += kImgThreads) {
        const int c = it / band4, e = it % band4, y = y0 + e / D4, x4 = e % D4;
#if QV_IMAGE_RRC
        const int4 k = ((const int4*)(s_band + kImgBand))[y - y0];
        const int rel = s_band[y - y0] - r0, last = nrows - 1;
#else
        const int4 k = ((const int4*)s_coef)[y];
        const int rel = s_xmin[y] - r0, last = nrows - 1;
#endif
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
#if QV_IMAGE_ERASE
        // E[b] where X[b] stood: the elements inside the sample's box are replaced before anything is mixed
        if (er_b.touched) img_erase_apply(er_b, c, y, x4, D4, v);
#endif
#if QV_IMAGE_MIX
        // the partner's value of the same element (the sample's own where one plane set serves both), then
        // out = inside the box ? partner : fl(fl(w_self * own) + fl(w_partner * partner)), the products and the sum rounded one by one
        if (!as_is) {
            float u[4] = {v[0], v[1], v[2], v[3]};
            if (sides == 2) {
#if QV_IMAGE_RRC
                // the partner's planes came from its own window: within this block k, rel and last are those of its row table and its rows
                const int32_t* band_p = s_band + kImgBand * (1 + kImgTaps);
                const int4 k = ((const int4*)(band_p + kImgBand))[y - y0];
                const int rel = band_p[y - y0] - win_p.r0, last = win_p.nrows - 1;
#endif
                const uint32_t* pp = plane + partner4;
                const uint32_t p0 = pp[max(0, min(rel, last)) * 3 * D4], p1 = pp[max(0, min(rel + 1, last)) * 3 * D4];
                const uint32_t p2 = pp[max(0, min(rel + 2, last)) * 3 * D4], p3 = pp[max(0, min(rel + 3, last)) * 3 * D4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    int acc = 1 << (kImgBits - 1);
                    acc += __mul24((int)((p0 >> (8 * j)) & 255), k.x);
                    acc += __mul24((int)((p1 >> (8 * j)) & 255), k.y);
                    acc += __mul24((int)((p2 >> (8 * j)) & 255), k.z);
                    acc += __mul24((int)((p3 >> (8 * j)) & 255), k.w);
                    u[j] = tab[img_round_clip(acc)];
                }
#if QV_IMAGE_ERASE
                if (er_p.touched) img_erase_apply(er_p, c, y, x4, D4, u);   // E[p], by the partner's own record
#endif
            }
            const bool row_in = box && y >= by0 && y < by1;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int x = x4 * 4 + j;
                const float a = w_self * v[j], c2 = w_partner * u[j];
                v[j] = row_in && x >= bx0 && x < bx1 ? u[j] : a + c2;
            }
        }
#endif
        *(float4*)(obase + (int64_t)c * D * D + (int64_t)e * 4) = make_float4(v[0], v[1], v[2], v[3]);
    }
}
#endif
#undef QV_IMAGE_XLAST
#undef QV_IMAGE_NAME
#undef QV_IMAGE_AUG
#undef QV_IMAGE_MIX
#undef QV_IMAGE_RRC
#undef QV_IMAGE_ERASE
#undef QV_IMAGE_COLOR
#undef QV_IMAGE_FORM
