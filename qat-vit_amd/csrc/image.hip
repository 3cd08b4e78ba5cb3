// Input pipeline: uint8 HWC images resident on the device -> the fp32 [B, 3, D, D] batch that Resize(D, BICUBIC) + ToTensor() + Normalize(mean, std)
// produce on the host (Pillow's 8-bit two-pass resample; include/qatvit.h states the arithmetic).  Integer throughout, so the result is equal, not close.
#include <math.h>

#include "qv_common.h"
#include "qv_kernels.h"

namespace qv {

// ---------------------------------------------------------------------------------------------------------------- host: the two tables
#include "image_tables.h"

int image_max_rows(int S, int D) { return (kImgBand * S + D - 1) / D + kImgTaps + 1; }

// src <= dst: the filter is not stretched, and the kernel takes all kImgTaps taps
int image_resize_coeffs(int src, int dst, int32_t* xmin_out, int32_t* ntaps_out, int32_t* coef) {
    return pillow_coeffs<kImgTaps>("qatvit_image_resize_coeffs", false, kImgTaps, kImgBand, image_max_rows, src, dst, xmin_out, ntaps_out, coef);
}

void image_table(const float* mean, const float* stdv, float* table) {
    for (int c = 0; c < 3; ++c)
        for (int i = 0; i < 256; ++i) table[c * 256 + i] = ((float)i / 255.0f - mean[c]) / stdv[c];   // two IEEE divisions, as torch's div(255) .. div(std)
}

int image_resize_coeffs_windows(int S, int D, int32_t* out) {
    for (int n = 1; n <= S; ++n) {
        int32_t* t = out + (int64_t)(n - 1) * 6 * D;
        if (image_resize_coeffs(n, D, t, t + D, t + 2 * D)) return 1;
    }
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------- device
#include "image_device.h"

// the kernel, once per form (image_kernel.h): every inclusion states the kernel's name and all five switches
//                    (name,                        AUG, MIX, RRC, ERASE, COLOR)
#define QV_IMAGE_FORM (k_image_batch,                 0,   0,   0,   0,   0)
#include "image_kernel.h"
#define QV_IMAGE_FORM (k_image_batch_aug,             1,   0,   0,   0,   0)
#include "image_kernel.h"
#define QV_IMAGE_FORM (k_image_batch_mix,             1,   1,   0,   0,   0)
#include "image_kernel.h"
#define QV_IMAGE_FORM (k_image_batch_rrc,             0,   0,   1,   0,   0)
#include "image_kernel.h"
#define QV_IMAGE_FORM (k_image_batch_rrc_mix,         0,   1,   1,   0,   0)
#include "image_kernel.h"
// the four erasing forms; the aug form also serves the call without aug words
#define QV_IMAGE_FORM (k_image_batch_aug_erase,       1,   0,   0,   1,   0)
#include "image_kernel.h"
#define QV_IMAGE_FORM (k_image_batch_mix_erase,       1,   1,   0,   1,   0)
#include "image_kernel.h"
#define QV_IMAGE_FORM (k_image_batch_rrc_erase,       0,   0,   1,   1,   0)
#include "image_kernel.h"
#define QV_IMAGE_FORM (k_image_batch_rrc_mix_erase,   0,   1,   1,   1,   0)
#include "image_kernel.h"
// the four colour forms (the erasing forms with a colour record per side; erase == NULL: no boxes), then the two statistics forms
#define QV_IMAGE_FORM (k_image_batch_aug_color,       1,   0,   0,   1,   1)
#include "image_kernel.h"
#define QV_IMAGE_FORM (k_image_batch_mix_color,       1,   1,   0,   1,   1)
#include "image_kernel.h"
#define QV_IMAGE_FORM (k_image_batch_rrc_color,       0,   0,   1,   1,   1)
#include "image_kernel.h"
#define QV_IMAGE_FORM (k_image_batch_rrc_mix_color,   0,   1,   1,   1,   1)
#include "image_kernel.h"
#define QV_IMAGE_FORM (k_image_stat_aug,              1,   0,   0,   1,   2)
#include "image_kernel.h"
#define QV_IMAGE_FORM (k_image_stat_rrc,              0,   0,   1,   1,   2)
#include "image_kernel.h"

// One plane set, or the partner's planes behind the sample's (mixed); the window forms keep, behind that on the next 16 bytes, the band's entries of
// the row table per side (one side, or two with mix records)
int64_t image_lds_bytes(int S, int D, bool mixed, bool rrc) {
    const int mr = image_max_rows(S, D);
    const int64_t base = (int64_t)D * (1 + kImgTaps) * 4 + 768 * 4 + ((mr * S * 3 + 15) & ~15) + (int64_t)(mixed ? 2 : 1) * mr * 3 * D;
    return rrc ? ((base + 15) & ~(int64_t)15) + (int64_t)(mixed ? 2 : 1) * kImgBand * (1 + kImgTaps) * 4 : base;
}

// The forms.  The erase and colour records add nothing to LDS, so a form's request is that of its family with or without mix, and `who`, the name
// in its refusal, is the narrowest C entry that serves the records present.  The window forms are always checked, the others only with mix.
enum ImageForm { kImgPlain, kImgAug, kImgMix, kImgAugErase, kImgMixErase, kImgAugColor, kImgMixColor,
                 kImgRrc, kImgRrcMix, kImgRrcErase, kImgRrcMixErase, kImgRrcColor, kImgRrcMixColor };
static const struct { const char* who; bool mixed, rrc; } kImageForms[] = {
    {"qatvit_image_batch", false, false},           {"qatvit_image_batch_aug", false, false},       {"qatvit_image_batch_mix", true, false},
    {"qatvit_image_batch_erase", false, false},     {"qatvit_image_batch_erase", true, false},      {"qatvit_image_batch_color", false, false},
    {"qatvit_image_batch_color", true, false},      {"qatvit_image_batch_rrc", false, true},        {"qatvit_image_batch_rrc", true, true},
    {"qatvit_image_batch_rrc_erase", false, true},  {"qatvit_image_batch_rrc_erase", true, true},   {"qatvit_image_batch_rrc_color", false, true},
    {"qatvit_image_batch_rrc_color", true, true}};
static_assert(sizeof(kImageForms) / sizeof(kImageForms[0]) == kImgRrcMixColor + 1, "one row per form, in the enum's order");

// per family: no records, erase, colour (which takes erase as it comes), each without and with mix, as the enum lists them
static ImageForm image_form(const ImageBatch& r) {
    const int records = r.color ? 2 : (r.erase ? 1 : 0), mixed = r.mix != nullptr;
    if (r.rrc) return ImageForm(kImgRrc + 2 * records + mixed);
    if (records) return ImageForm(kImgAugErase + 2 * (records - 1) + mixed);
    return mixed ? kImgMix : (r.aug ? kImgAug : kImgPlain);
}

// the one launch site: the grid, the constant-D choice and the head that every kernel takes
template <typename K, typename... Tail>
static void image_launch(const ImageBatch& r, K k224, K k0, int64_t lds, hipStream_t st, Tail... tail) {
    const dim3 grid((r.D + kImgBand - 1) / kImgBand, r.B);
    hipLaunchKernelGGL(r.D == 224 ? k224 : k0, grid, dim3(kImgThreads), (size_t)lds, st, r.data, r.index, r.N, r.S, r.D, image_max_rows(r.S, r.D), r.tab,
                       tail...);
}
#define QV_IMAGE_K(name) name<224>, name<0>

int launch_image_batch(const ImageBatch& r, hipStream_t st) {
    if (r.blur) return launch_image_blur(r, st);   // image_blur.hip
    const ImageForm form = image_form(r);
    const auto& f = kImageForms[form];
    const int64_t lds = image_lds_bytes(r.S, r.D, f.mixed, f.rrc);
    if ((f.rrc || f.mixed) && lds > kImgMixMaxLds) {
        set_error("%s: source %d -> output %d needs %lld bytes of LDS%s, more than %d", f.who, r.S, r.D, (long long)lds,
                  f.mixed ? " for two plane sets" : "", kImgMixMaxLds);
        return 1;
    }
    const bool stats = r.color && r.sums;   // the statistics launch in front of a colour form: one plane set, into the zeroed workspace
    if (stats) {
        const hipError_t e = hipMemsetAsync(r.sums, 0, (size_t)r.B * sizeof(uint32_t), st);
        if (e != hipSuccess) {
            set_error("%s: zeroing sums failed: %s", f.who, hipGetErrorString(e));
            return 2;
        }
    }
    // The compiler emits the kernels in the order in which this text names them, and their labels are numbered in that order: the cases stand in the
    // order of the launchers this one replaced, so that the machine code stays what it was (profiles/image_request_record_isa_identity.txt).
    switch (form) {
    case kImgPlain: image_launch(r, QV_IMAGE_K(k_image_batch), lds, st, r.table, r.out); break;
    case kImgAug: image_launch(r, QV_IMAGE_K(k_image_batch_aug), lds, st, r.table, r.out, r.aug, r.padding_mode, r.fill); break;
    case kImgMix: image_launch(r, QV_IMAGE_K(k_image_batch_mix), lds, st, r.table, r.out, r.aug, r.padding_mode, r.fill, r.mix); break;
    case kImgRrcMix: image_launch(r, QV_IMAGE_K(k_image_batch_rrc_mix), lds, st, r.table, r.out, r.rrc, r.mix); break;
    case kImgRrc: image_launch(r, QV_IMAGE_K(k_image_batch_rrc), lds, st, r.table, r.out, r.rrc); break;
    case kImgMixErase: image_launch(r, QV_IMAGE_K(k_image_batch_mix_erase), lds, st, r.table, r.out, r.aug, r.padding_mode, r.fill, r.mix, r.erase); break;
    case kImgAugErase: image_launch(r, QV_IMAGE_K(k_image_batch_aug_erase), lds, st, r.table, r.out, r.aug, r.padding_mode, r.fill, r.erase); break;
    case kImgRrcMixErase: image_launch(r, QV_IMAGE_K(k_image_batch_rrc_mix_erase), lds, st, r.table, r.out, r.rrc, r.mix, r.erase); break;
    case kImgRrcErase: image_launch(r, QV_IMAGE_K(k_image_batch_rrc_erase), lds, st, r.table, r.out, r.rrc, r.erase); break;
    case kImgMixColor:
    case kImgAugColor:
        if (stats) image_launch(r, QV_IMAGE_K(k_image_stat_aug), image_lds_bytes(r.S, r.D, false, false), st, r.aug, r.padding_mode, r.fill, r.color, r.sums);
        if (f.mixed) image_launch(r, QV_IMAGE_K(k_image_batch_mix_color), lds, st, r.table, r.out, r.aug, r.padding_mode, r.fill, r.mix, r.erase, r.color, r.sums);
        else image_launch(r, QV_IMAGE_K(k_image_batch_aug_color), lds, st, r.table, r.out, r.aug, r.padding_mode, r.fill, r.erase, r.color, r.sums);
        break;
    case kImgRrcMixColor:
    case kImgRrcColor:
        if (stats) image_launch(r, QV_IMAGE_K(k_image_stat_rrc), image_lds_bytes(r.S, r.D, false, true), st, r.rrc, r.color, r.sums);
        if (f.mixed) image_launch(r, QV_IMAGE_K(k_image_batch_rrc_mix_color), lds, st, r.table, r.out, r.rrc, r.mix, r.erase, r.color, r.sums);
        else image_launch(r, QV_IMAGE_K(k_image_batch_rrc_color), lds, st, r.table, r.out, r.rrc, r.erase, r.color, r.sums);
        break;
    }
    return 0;
}

}  // namespace qv
