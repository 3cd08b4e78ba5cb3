// Input pipeline, the blur forms: Gaussian blur as Pillow computes it inside the batch launch (image_blur.h states the kernel; include/qatvit.h the
// arithmetic).  A source file of its own: image.hip, and with it the machine code of its fifteen kernels, stays what it was.
#include <math.h>

#include "qv_common.h"
#include "qv_kernels.h"

namespace qv {

#include "image_device.h"
#include "image_blur.h"

// The blur forms' request (img_blur_lds, image_blur.h): the other forms' tables and source rows for a band (16 rows, 8 with mix records) with its halo, a plane
// set and an image buffer of band + 12 rows per side, one more such buffer for the passes, and with windows the row-table entries per side
int image_blur_max_rows(int S, int D, bool mixed) { return (((mixed ? kImgBlurMixBand : kImgBlurBand) + 2 * kImgBlurHalo) * S + D - 1) / D + kImgTaps + 1; }

int64_t image_blur_lds_bytes(int S, int D, bool mixed, bool rrc) { return img_blur_lds(S, D, image_blur_max_rows(S, D, mixed), mixed ? 2 : 1, rrc).total; }

// The blur forms: blur records present.  Four batch kernels (aug / rrc, without / with mix; erase and colour records as they come, absent ones as
// all-zero records) and two statistics kernels, which run in front of the batch launch as the colour forms' do.  Always checked against the limit.
template <bool RRC, bool MIX, bool STAT>
static void image_blur_launch(const ImageBatch& r, int64_t lds, hipStream_t st) {
    constexpr int band = MIX ? kImgBlurMixBand : kImgBlurBand;
    const dim3 grid((r.D + band - 1) / band, r.B);
    const auto kernel = r.D == 224 ? k_image_blur<224, RRC, MIX, STAT> : k_image_blur<0, RRC, MIX, STAT>;
    hipLaunchKernelGGL(kernel, grid, dim3(kImgThreads), (size_t)lds, st, r.data, r.index, r.N, r.S, r.D, image_blur_max_rows(r.S, r.D, MIX), r.tab, STAT ? nullptr : r.table, STAT ? nullptr : r.out, RRC ? r.rrc : r.aug,
                       r.padding_mode, r.fill, MIX ? r.mix : nullptr, STAT ? nullptr : r.erase, r.color, STAT ? nullptr : r.sums, STAT ? r.sums : nullptr,
                       r.blur);
}

int launch_image_blur(const ImageBatch& r, hipStream_t st) {
    const char* who = r.rrc ? "qatvit_image_batch_rrc_blur" : "qatvit_image_batch_blur";
    const bool mixed = r.mix != nullptr, rrc = r.rrc != nullptr;
    const int64_t lds = image_blur_lds_bytes(r.S, r.D, mixed, rrc);
    if (lds > kImgMixMaxLds) {
        set_error("%s: source %d -> output %d needs %lld bytes of LDS%s, more than %d", who, r.S, r.D, (long long)lds,
                  mixed ? " for two plane sets and three image buffers" : " for a plane set and two image buffers", kImgMixMaxLds);
        return 1;
    }
    const bool stats = r.color && r.sums;
    if (stats) {
        const hipError_t e = hipMemsetAsync(r.sums, 0, (size_t)r.B * sizeof(uint32_t), st);
        if (e != hipSuccess) {
            set_error("%s: zeroing sums failed: %s", who, hipGetErrorString(e));
            return 2;
        }
        const int64_t lds1 = image_blur_lds_bytes(r.S, r.D, false, rrc);
        if (rrc) image_blur_launch<true, false, true>(r, lds1, st);
        else image_blur_launch<false, false, true>(r, lds1, st);
    }
    if (rrc && mixed) image_blur_launch<true, true, false>(r, lds, st);
    else if (rrc) image_blur_launch<true, false, false>(r, lds, st);
    else if (mixed) image_blur_launch<false, true, false>(r, lds, st);
    else image_blur_launch<false, false, false>(r, lds, st);
    return 0;
}

}  // namespace qv
