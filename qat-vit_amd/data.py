"""Input pipeline on MI355X (libqatvit.so: qatvit_image_resize_coeffs / qatvit_image_table / qatvit_image_batch / qatvit_image_batch_aug /
qatvit_image_batch_mix / qatvit_image_resize_coeffs_windows / qatvit_image_batch_rrc / qatvit_image_batch_erase / qatvit_image_batch_rrc_erase /
qatvit_image_batch_color / qatvit_image_batch_rrc_color / qatvit_image_batch_blur / qatvit_image_batch_rrc_blur / qatvit_image_window_u8 /
qatvit_image_bytes_blur).

Stands where the reference's loaders have, per image on DataLoader workers, ``Resize(224, BICUBIC)`` through Pillow, ``ToTensor()`` and
``Normalize(mean, std)``, followed by the copy of the fp32 batch to the device: the uint8 data set lives on the device, and one launch per batch
writes the fp32 ``[B, 3, 224, 224]`` batch those transforms would have produced, equal to it element for element.
``RandomCropFlip`` adds ``RandomCrop(S, padding=p)`` + ``RandomHorizontalFlip()`` in front of the resize, inside the same launch (section 7l).
``MixupCutmix`` adds mixup / cutmix behind them, still inside that launch (section 7m); ``functional.kd_ce_loss_mix`` takes the same records.
``RandomResizedCrop`` stands instead of ``RandomCropFlip``: every sample is a window of its image, resized, inside the same launch (section 7n).
``RandomErasing`` erases a box of every sample's normalised output, behind either and in front of the mix, inside the same launch (section 7o).
``ColorJitter`` applies grayscale, solarize, brightness, contrast and saturation to the uint8 image behind the resize, equal to Pillow's, inside
the same launch; contrast takes the sample's mean luma from a statistics launch in front of it (section 7q).
``GaussianBlur`` blurs the uint8 image behind the resize as Pillow's ``ImageFilter.GaussianBlur`` does, between grayscale / solarize and the jitter
ops, inside the same launch; ``ThreeAugment`` draws DeiT-III's one-of-three choice with its colour jitter (section 7v).
``GpuWindowResize`` / ``GpuWideResizeNormalize`` serve sources that are rectangles or larger than the output: a window stage of its own
(``qatvit_image_window_u8``, Pillow's stretched filter, up to 17 taps) writes the resized uint8 windows, and the batch launch at S = D applies the
rest to them (section 7x).
``GpuBytesBlurNormalize`` / ``GpuWideResizeNormalize(..., blur=True)`` serve ``GaussianBlur`` and ``ThreeAugment`` on such sources: the second stage
of a call with blur records is a launch that takes the staged bytes as the image to blur (``qatvit_image_bytes_blur``, section 7z).
There is no CPU path: CPU tensors raise."""
import math
import os
import pickle

import numpy as np
import torch
from torch.utils.data import BatchSampler, RandomSampler, SequentialSampler

from . import native

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)


def resize_tables(src_size: int, out_size: int):
    """int32 CPU tensors xmin [D], ntaps [D], coef [D, 4] of Pillow's 8-bit bicubic resample from src_size to out_size (host only, no GPU)."""
    xmin, ntaps = torch.empty(out_size, dtype=torch.int32), torch.empty(out_size, dtype=torch.int32)
    coef = torch.empty(out_size, 4, dtype=torch.int32)
    native.check(native.lib().qatvit_image_resize_coeffs(int(src_size), int(out_size), xmin.data_ptr(), ntaps.data_ptr(), coef.data_ptr()),
                 "qatvit_image_resize_coeffs")
    return xmin, ntaps, coef


def resize_window_tables(src_size: int, out_size: int):
    """int32 CPU tensor [S, 6 * D]: row n - 1 holds xmin [D], ntaps [D], coef [D, 4] of the resample from n to out_size one after the other, for
    every window side n = 1 .. src_size (host only, no GPU).  Row S - 1 is ``resize_tables(S, D)``."""
    out = torch.empty(max(int(src_size), 0), 6 * max(int(out_size), 0), dtype=torch.int32)
    native.check(native.lib().qatvit_image_resize_coeffs_windows(int(src_size), int(out_size), out.data_ptr()), "qatvit_image_resize_coeffs_windows")
    return out


def value_table(mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """fp32 CPU tensor [3, 256]: what ToTensor() + Normalize(mean, std) make of each byte value, per channel (host only, no GPU)."""
    m, s = torch.tensor(mean, dtype=torch.float32), torch.tensor(std, dtype=torch.float32)
    if m.shape != (3,) or s.shape != (3,):
        raise ValueError("mean and std must have three entries")
    table = torch.empty(3, 256, dtype=torch.float32)
    native.check(native.lib().qatvit_image_table(m.data_ptr(), s.data_ptr(), table.data_ptr()), "qatvit_image_table")
    return table


PADDING_MODES = {"constant": 0, "reflect": 1}


def _padding_mode_and_fill(padding_mode, fill):
    if padding_mode not in PADDING_MODES:
        raise ValueError(f"padding_mode must be one of {sorted(PADDING_MODES)}, got {padding_mode!r}")
    if isinstance(fill, bool) or not isinstance(fill, int) or not 0 <= fill <= 255:
        raise ValueError(f"fill must be an integer byte value 0 .. 255 (the same for all channels), got {fill!r}")
    return PADDING_MODES[padding_mode], fill


class RandomCropFlip:
    """``RandomCrop(S, padding=padding, padding_mode=..., fill=...)`` + ``RandomHorizontalFlip(flip)`` of the uint8 source image as one int32 word
    per sample (include/qatvit.h): bits 0..7 the row offset ``oy``, bits 8..15 the column offset ``ox`` (both signed, in ``[-padding, padding]``:
    torchvision's ``top - padding`` / ``left - padding``), bit 16 the flip, all other bits zero.  Built and drawn on the host; needs no GPU."""

    def __init__(self, padding=4, flip=0.5, padding_mode="constant", fill=0):
        if isinstance(padding, bool) or not isinstance(padding, int) or not 0 <= padding <= 127:
            raise ValueError(f"padding must be an integer 0 .. 127, got {padding!r}")
        if isinstance(flip, bool) or not isinstance(flip, (int, float)) or not 0 <= flip <= 1:
            raise ValueError(f"flip must be a probability 0 .. 1, got {flip!r}")
        _, self.fill = _padding_mode_and_fill(padding_mode, fill)
        self.padding, self.flip, self.padding_mode = padding, float(flip), padding_mode

    def draw(self, n, generator=None):
        """int32 CPU tensor [n].  The rule: ``off = torch.randint(0, 2 * padding + 1, (n, 2), generator=g) - padding`` (row k is ``[oy, ox]``), then
        ``flip_k = torch.rand(n, generator=g) < flip``.  Both draws are always made, so the generator ends where it ends for any setting."""
        off = torch.randint(0, 2 * self.padding + 1, (n, 2), generator=generator) - self.padding
        flip = torch.rand(n, generator=generator) < self.flip
        return ((off[:, 0] & 255) | (off[:, 1] & 255) << 8 | flip.to(torch.int64) << 16).to(torch.int32)


RRC_WORDS = 2


def _interval(name, v):
    """(lo, hi) of a pair of finite numbers 0 < lo <= hi."""
    ok = isinstance(v, (tuple, list)) and len(v) == 2 and all(not isinstance(t, bool) and isinstance(t, (int, float)) for t in v)
    if not ok or not 0 < v[0] <= v[1] < float("inf"):
        raise ValueError(f"{name} must be a pair of finite numbers 0 < low <= high, got {v!r}")
    return float(v[0]), float(v[1])


class RandomResizedCrop:
    """``RandomResizedCrop(D, scale, ratio, BICUBIC)`` + ``RandomHorizontalFlip(flip)`` of the uint8 source image as one two-word int32 record per
    sample (include/qatvit.h): word 0 ``top | left << 16``, word 1 ``h | w << 15 | flip << 30``, with ``1 <= h, w <= S``, ``top <= S - h``,
    ``left <= S - w``: the window that is cropped, mirrored where ``flip`` is set, and resized to the output.  Built and drawn on the host; needs
    no GPU."""

    def __init__(self, scale=(0.08, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0), flip=0.5):
        self.scale, self.ratio = _interval("scale", scale), _interval("ratio", ratio)
        if isinstance(flip, bool) or not isinstance(flip, (int, float)) or not 0 <= flip <= 1:
            raise ValueError(f"flip must be a probability 0 .. 1, got {flip!r}")
        self.flip = float(flip)

    def draw(self, n, src_size, generator=None):
        """int32 CPU tensor [n, 2] for square sources of side S = `src_size`, or for ``H x W`` sources where `src_size` is a pair ``(H, W)``:
        then ``area = H * W * ...``, a try fits when ``1 <= w <= W`` and ``1 <= h <= H``, the fallback compares ``in_ratio = W / H`` with the
        ratio range (``in_ratio < r0``: ``w = W, h = round(W / r0)``; ``in_ratio > r1``: ``h = H, w = round(H * r1)``; otherwise the whole
        image), ``top`` is drawn in ``H - h + 1`` and ``left`` in ``W - w + 1`` values, and the fallback window is centred on both axes.  For
        a number S the tensor is what ``(S, S)`` gives.  The rule (torchvision's ``RandomResizedCrop.get_params``,
        restated: torchvision is not a dependency), with ``scale = (s0, s1)``, ``ratio = (r0, r1)``, all from `generator`, in this order:
        ``u = torch.rand(n, 10, 2, dtype=float64)``: ten tries per sample, ``area = S^2 * (s0 + u[..., 0] * (s1 - s0))``,
        ``aspect = exp(log r0 + u[..., 1] * (log r1 - log r0))``, ``w = torch.round(sqrt(area * aspect))``,
        ``h = torch.round(sqrt(area / aspect))``; the first try with ``1 <= w <= S`` and ``1 <= h <= S`` is taken;
        if none of the ten fits, torchvision's fallback for a square image, centred: the whole image if ``r0 <= 1 <= r1``; if ``1 < r0``,
        ``w = S, h = round(S / r0)``; if ``r1 < 1``, ``h = S, w = round(S * r1)`` (round half to even, at least 1);
        ``top = (S - h) // 2, left = (S - w) // 2``;
        ``v = torch.rand(n, 3, dtype=float64)``: ``top = floor(v[:, 0] * (S - h + 1))``, ``left = floor(v[:, 1] * (S - w + 1))`` (both unused by
        the fallback), ``flip = v[:, 2] < flip``.
        Both ``rand`` calls are always made, so the generator ends where it ends for any setting."""
        if isinstance(src_size, (tuple, list)):
            if len(src_size) != 2 or not all(1 <= int(t) <= 0x7fff for t in src_size):
                raise ValueError(f"src_size must be 1 .. 32767 or a pair (H, W) of such numbers, got {src_size!r}")
            H, W = int(src_size[0]), int(src_size[1])
        else:
            H = W = int(src_size)
            if not 1 <= H <= 0x7fff:
                raise ValueError(f"src_size must be 1 .. 32767, got {src_size!r}")
        (s0, s1), (r0, r1) = self.scale, self.ratio
        u = torch.rand(n, 10, 2, dtype=torch.float64, generator=generator)
        v = torch.rand(n, 3, dtype=torch.float64, generator=generator)
        area = float(H * W) * (s0 + u[..., 0] * (s1 - s0))
        aspect = torch.exp(math.log(r0) + u[..., 1] * (math.log(r1) - math.log(r0)))
        w, h = torch.round(torch.sqrt(area * aspect)), torch.round(torch.sqrt(area / aspect))
        fits = (w >= 1) & (w <= W) & (h >= 1) & (h <= H)
        first = fits.to(torch.int8).argmax(1, keepdim=True)           # the first maximum: the first try that fits (0 where none does)
        found = fits.any(1)
        w, h = w.gather(1, first)[:, 0].to(torch.int64), h.gather(1, first)[:, 0].to(torch.int64)
        in_ratio = float(W) / float(H)
        if in_ratio < r0:
            fw, fh = W, min(H, max(1, int(round(W / r0))))
        elif in_ratio > r1:
            fw, fh = min(W, max(1, int(round(H * r1)))), H
        else:
            fw, fh = W, H
        w, h = torch.where(found, w, torch.full_like(w, fw)), torch.where(found, h, torch.full_like(h, fh))
        top = torch.minimum(torch.floor(v[:, 0] * (H - h + 1)).to(torch.int64), H - h)
        left = torch.minimum(torch.floor(v[:, 1] * (W - w + 1)).to(torch.int64), W - w)
        top, left = torch.where(found, top, (H - h) // 2), torch.where(found, left, (W - w) // 2)
        flip = (v[:, 2] < self.flip).to(torch.int64)
        return torch.stack([top | left << 16, h | w << 15 | flip << 30], 1).to(torch.int32)


MIX_WORDS = 6


class MixupCutmix:
    """Mixup (arXiv:1710.09412) and cutmix (arXiv:1905.04899) as one six-word int32 record per batch position (include/qatvit.h): partner
    position, ``w_self`` and ``w_partner`` (fp32 bits), the box rows ``y0 | y1 << 16`` and columns ``x0 | x1 << 16``, and ``lam`` (fp32 bits), the
    weight of the sample's own label.  The arguments have timm's ``Mixup`` meaning.  Built and drawn on the host; needs no GPU."""

    MODES = ("batch", "elem")

    def __init__(self, mixup_alpha=0.8, cutmix_alpha=1.0, prob=1.0, switch_prob=0.5, mode="batch"):
        for name, v in (("mixup_alpha", mixup_alpha), ("cutmix_alpha", cutmix_alpha)):
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not 0 <= v < float("inf"):
                raise ValueError(f"{name} must be a finite number >= 0, got {v!r}")
        for name, v in (("prob", prob), ("switch_prob", switch_prob)):
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not 0 <= v <= 1:
                raise ValueError(f"{name} must be a probability 0 .. 1, got {v!r}")
        if mode not in self.MODES:
            raise ValueError(f"mode must be one of {list(self.MODES)}, got {mode!r}")
        self.mixup_alpha, self.cutmix_alpha, self.prob, self.switch_prob, self.mode = float(mixup_alpha), float(cutmix_alpha), float(prob), \
            float(switch_prob), mode

    def _draw_one(self, D, generator):
        """(w_self, w_partner, y0, y1, x0, x1, lam) of one decision; the weights and lam are np.float32."""
        u = torch.rand(2, dtype=torch.float64, generator=generator)
        mixing = bool(u[0] < self.prob) and (self.mixup_alpha > 0 or self.cutmix_alpha > 0)
        cut = bool(u[1] < self.switch_prob) if self.mixup_alpha > 0 and self.cutmix_alpha > 0 else self.cutmix_alpha > 0
        alpha = (self.cutmix_alpha if cut else self.mixup_alpha) if mixing else 1.0
        g = torch._standard_gamma(torch.full((2,), alpha, dtype=torch.float64), generator=generator)
        lam = float(g[0] / (g[0] + g[1]))
        one, zero = np.float32(1), np.float32(0)
        if not mixing or not 0 <= lam <= 1:      # both gamma draws underflowed to 0: no mix
            return one, zero, 0, 0, 0, 0, one
        if not cut:
            lam = np.float32(lam)
            return lam, one - lam, 0, 0, 0, 0, lam
        cy, cx = (int(v) for v in torch.randint(0, D, (2,), generator=generator))
        h = int(D * float(np.sqrt(1.0 - lam)))
        y0, y1 = min(max(cy - h // 2, 0), D), min(max(cy + h // 2, 0), D)
        x0, x1 = min(max(cx - h // 2, 0), D), min(max(cx + h // 2, 0), D)
        return one, zero, y0, y1, x0, x1, np.float32(1.0 - (y1 - y0) * (x1 - x0) / float(D * D))

    def draw(self, batch_sizes, out_size, generator=None):
        """int32 CPU tensor ``[sum(batch_sizes), 6]``, the records of the batches one after the other.  The rule (timm's, restated: timm is not a
        dependency).  The partner of position b in a batch of m is ``m - 1 - b`` (the batch flipped).  One decision per batch, or per sample in
        ``mode="elem"``, all from `generator`, in this order:
        ``u = torch.rand(2, dtype=float64)``: ``u[0] < prob`` means mix; ``u[1] < switch_prob`` means cutmix when both alphas are positive,
        otherwise whichever alpha is positive is used;
        ``X, Y = torch._standard_gamma(torch.full((2,), alpha, dtype=float64))``, ``lam = X / (X + Y)`` (a Beta(alpha, alpha) draw), with the
        chosen alpha, or 1 when not mixing (so ``u`` and the gamma pair are always drawn);
        mixup: an empty box, ``w_self = fp32(lam)``, ``w_partner = fp32(1) - w_self``, the record's lam ``= w_self``;
        cutmix: ``cy, cx = torch.randint(0, D, (2,))``, ``h = int(D * sqrt(1 - lam))``, ``y0 = clip(cy - h // 2, 0, D)``,
        ``y1 = clip(cy + h // 2, 0, D)``, the columns likewise from ``cx``; weights (1, 0); lam ``= fp32(1 - (y1 - y0) * (x1 - x0) / D^2)``;
        not mixing: the identity record: weights (1, 0), an empty box, lam 1."""
        D = int(out_size)
        if not 1 <= D <= 0xffff:
            raise ValueError(f"out_size must be 1 .. 65535, got {out_size!r}")
        sizes = [int(m) for m in batch_sizes]
        rec = np.zeros((sum(sizes), MIX_WORDS), dtype=np.int32)
        bits = lambda v: np.float32(v).view(np.int32)
        o = 0
        for m in sizes:
            one = None if self.mode == "elem" else self._draw_one(D, generator)
            for b in range(m):
                ws, wp, y0, y1, x0, x1, lam = one if one is not None else self._draw_one(D, generator)
                rec[o + b] = (m - 1 - b, bits(ws), bits(wp), y0 | y1 << 16, x0 | x1 << 16, bits(lam))
            o += m
        return torch.from_numpy(rec)


ERASE_WORDS = 8


class RandomErasing:
    """``RandomErasing(p, scale, ratio, value)`` (arXiv:1708.04896) of the normalised output as one eight-word int32 record per sample
    (include/qatvit.h): the box rows ``y0 | y1 << 16`` and columns ``x0 | x1 << 16``, the fill of each channel (fp32 bits, normalised units), the
    mode bit and the 64-bit key of the noise.  ``value`` is a number, three numbers (one per channel) or ``"random"``; ``mode`` is ``"const"``
    (the fill is ``value``; with ``value=0`` timm's ``const``), ``"rand"`` (one standard normal per channel and sample, drawn on the host into the
    fill words: timm's ``rand``) or ``"pixel"`` (one standard normal per element, formed inside the launch from the record's key).
    ``value="random"`` is a synonym for ``mode="pixel"``, as torchvision has it; ``mode=None`` follows ``value``.  The erasure stands behind
    ``Normalize`` and in front of the mix.  Built and drawn on the host; needs no GPU."""

    MODES = ("const", "rand", "pixel")

    def __init__(self, p=0.25, scale=(0.02, 0.33), ratio=(0.3, 3.3), value=0, mode=None):
        if isinstance(p, bool) or not isinstance(p, (int, float)) or not 0 <= p <= 1:
            raise ValueError(f"p must be a probability 0 .. 1, got {p!r}")
        self.p, self.scale, self.ratio = float(p), _interval("scale", scale), _interval("ratio", ratio)
        if mode is not None and mode not in self.MODES:
            raise ValueError(f"mode must be one of {list(self.MODES)} or None, got {mode!r}")
        number = lambda t: not isinstance(t, bool) and isinstance(t, (int, float)) and math.isfinite(t)   # noqa: E731
        if isinstance(value, str):
            if value != "random":
                raise ValueError(f"value must be a number, three numbers or 'random', got {value!r}")
            if mode not in (None, "pixel"):
                raise ValueError(f"value='random' is mode='pixel'; it cannot go with mode={mode!r}")
            mode, fill = "pixel", (0.0, 0.0, 0.0)
        elif number(value):
            fill = (float(value),) * 3
        elif isinstance(value, (tuple, list)) and len(value) == 3 and all(number(t) for t in value):
            fill = tuple(float(t) for t in value)
        else:
            raise ValueError(f"value must be a finite number, three finite numbers or 'random', got {value!r}")
        mode = mode or "const"
        if mode != "const" and any(t != 0.0 for t in fill):
            raise ValueError(f"mode={mode!r} draws its own fill: value must stay 0, got {value!r}")
        self.value, self.mode = fill, mode

    def draw(self, n, out_size, generator=None):
        """int32 CPU tensor [n, 8] for outputs of side D = `out_size`.  The rule (torchvision's ``RandomErasing.forward`` / ``get_params`` for a
        square image, restated: torchvision is not a dependency), with ``scale = (s0, s1)``, ``ratio = (r0, r1)``, all from `generator`, in
        this order:
        ``g = torch.rand(n, dtype=float64)``: sample k is erased where ``g[k] < p``;
        ``u = torch.rand(n, 10, 2, dtype=float64)``: ten tries per sample, ``area = D^2 * (s0 + u[..., 0] * (s1 - s0))``,
        ``aspect = exp(log r0 + u[..., 1] * (log r1 - log r0))``, ``h = torch.round(sqrt(area * aspect))``,
        ``w = torch.round(sqrt(area / aspect))``; the first try with ``h < D`` and ``w < D`` is taken; if none of the ten fits the sample is not
        erased;
        ``v = torch.rand(n, 2, dtype=float64)``: ``top = floor(v[:, 0] * (D - h + 1))``, ``left = floor(v[:, 1] * (D - w + 1))``;
        ``z = torch.randn(n, 3, dtype=float32)``: the fill of the three channels in ``mode="rand"``;
        ``k = torch.randint(-2^31, 2^31, (n, 2))``: the key words in ``mode="pixel"``.
        The box is rows ``top .. top + h - 1``, columns ``left .. left + w - 1``.  A sample that is not erased gets the all-zero record, the
        identity.  Every draw is always made, so the generator ends where it ends for any setting: its position depends on `n` only."""
        D = int(out_size)
        if not 1 <= D <= 0xffff:
            raise ValueError(f"out_size must be 1 .. 65535, got {out_size!r}")
        (s0, s1), (r0, r1) = self.scale, self.ratio
        g = torch.rand(n, dtype=torch.float64, generator=generator)
        u = torch.rand(n, 10, 2, dtype=torch.float64, generator=generator)
        v = torch.rand(n, 2, dtype=torch.float64, generator=generator)
        z = torch.randn(n, 3, dtype=torch.float32, generator=generator)
        k = torch.randint(-(1 << 31), 1 << 31, (n, 2), dtype=torch.int64, generator=generator)
        area = float(D * D) * (s0 + u[..., 0] * (s1 - s0))
        aspect = torch.exp(math.log(r0) + u[..., 1] * (math.log(r1) - math.log(r0)))
        h, w = torch.round(torch.sqrt(area * aspect)), torch.round(torch.sqrt(area / aspect))
        fits = (h < D) & (w < D)
        first = fits.to(torch.int8).argmax(1, keepdim=True)           # the first maximum: the first try that fits (0 where none does)
        erased = (g < self.p) & fits.any(1)
        h, w = h.gather(1, first)[:, 0].to(torch.int64), w.gather(1, first)[:, 0].to(torch.int64)
        h, w = torch.where(erased, h, torch.zeros_like(h)), torch.where(erased, w, torch.zeros_like(w))
        top = torch.minimum(torch.floor(v[:, 0] * (D - h + 1)).to(torch.int64), D - h)
        left = torch.minimum(torch.floor(v[:, 1] * (D - w + 1)).to(torch.int64), D - w)
        rec = torch.zeros(n, ERASE_WORDS, dtype=torch.int64)
        rec[:, 0], rec[:, 1] = top | (top + h) << 16, left | (left + w) << 16
        if self.mode == "pixel":
            rec[:, 5], rec[:, 6:8] = 1, k
        else:
            fill = z if self.mode == "rand" else torch.tensor(self.value, dtype=torch.float32).expand(n, 3)
            rec[:, 2:5] = fill.contiguous().view(torch.int32).to(torch.int64)
        rec = torch.where(erased[:, None], rec, torch.zeros_like(rec))
        return ((rec + (1 << 31)) % (1 << 32) - (1 << 31)).to(torch.int32)    # the 32 bits of every word, as int32


COLOR_WORDS = 4
COLOR_OPS = {"brightness": 1, "contrast": 2, "saturation": 3}


def _jitter_range(name, v):
    """torchvision's ColorJitter._check_input: a number x >= 0 means [max(0, 1 - x), 1 + x], a pair means [lo, hi] with 0 <= lo <= hi, both
    finite.  None where the range is [1, 1]: the op is not enabled."""
    number = lambda t: not isinstance(t, bool) and isinstance(t, (int, float)) and math.isfinite(t)   # noqa: E731
    if number(v):
        if v < 0:
            raise ValueError(f"{name} must be a number >= 0 or a pair 0 <= low <= high, got {v!r}")
        lo, hi = max(0.0, 1.0 - float(v)), 1.0 + float(v)
    elif isinstance(v, (tuple, list)) and len(v) == 2 and all(number(t) for t in v) and 0 <= v[0] <= v[1]:
        lo, hi = float(v[0]), float(v[1])
    else:
        raise ValueError(f"{name} must be a number >= 0 or a pair of finite numbers 0 <= low <= high, got {v!r}")
    return None if lo == hi == 1.0 else (lo, hi)


class ColorJitter:
    """torchvision's ``ColorJitter(brightness, contrast, saturation)`` + ``RandomGrayscale(grayscale)`` (three output channels) +
    ``RandomSolarize(solarize_threshold, solarize)`` of the uint8 image behind the resize as one four-word int32 record per sample
    (include/qatvit.h): word 0 the jitter ops in the order they are applied (two bits per slot: 1 brightness, 2 contrast, 3 saturation), bit 8
    grayscale, bit 9 solarize with the threshold in bits 16..23; words 1..3 the factors of brightness, contrast, saturation (fp32 bits).  Per
    sample the order is grayscale, solarize, the jitter ops; the result equals Pillow's.  ``brightness`` / ``contrast`` / ``saturation`` have
    torchvision's meaning: a number x is the range ``[max(0, 1 - x), 1 + x]``, a pair is ``[low, high]``; 0 disables the op.  ``hue`` is not
    supported (neither timm's default recipe nor DeiT-III's 3-Augment uses it) and anything but 0 raises.  Built and drawn on the host; needs
    no GPU."""

    def __init__(self, brightness=0, contrast=0, saturation=0, hue=0, grayscale=0.0, solarize=0.0, solarize_threshold=128):
        if isinstance(hue, bool) or not isinstance(hue, (int, float)) or hue != 0:
            raise ValueError(f"hue is not supported by the native pipeline (Pillow's HSV round trip is not restated): it must stay 0, got {hue!r}")
        self.brightness, self.contrast = _jitter_range("brightness", brightness), _jitter_range("contrast", contrast)
        self.saturation = _jitter_range("saturation", saturation)
        for name, v in (("grayscale", grayscale), ("solarize", solarize)):
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not 0 <= v <= 1:
                raise ValueError(f"{name} must be a probability 0 .. 1, got {v!r}")
        if isinstance(solarize_threshold, bool) or not isinstance(solarize_threshold, int) or not 0 <= solarize_threshold <= 255:
            raise ValueError(f"solarize_threshold must be an integer byte value 0 .. 255, got {solarize_threshold!r}")
        self.grayscale, self.solarize, self.solarize_threshold = float(grayscale), float(solarize), solarize_threshold

    def draw(self, n, generator=None):
        """int32 CPU tensor [n, 4].  The rule, all from `generator`, in this order:
        ``o = torch.rand(n, 3, dtype=float64).argsort(1)``: row k is a uniformly random order of (brightness, contrast, saturation); the
        enabled ops of that order, kept in it, fill the slots from slot 0 - a uniformly random order of the enabled ops;
        ``f = torch.rand(n, 3, dtype=float64)``: the factor of op j is ``fp32(low_j + f[:, j] * (high_j - low_j))``;
        ``p = torch.rand(n, 2, dtype=float64)``: grayscale where ``p[:, 0] < grayscale``, solarize where ``p[:, 1] < solarize``.
        The factor word of a disabled op and the threshold of a sample that is not solarized are 0.  Every draw is always made, so the
        generator ends where it ends for any setting: its position depends on `n` only."""
        order = torch.rand(n, 3, dtype=torch.float64, generator=generator).argsort(1)
        f = torch.rand(n, 3, dtype=torch.float64, generator=generator)
        p = torch.rand(n, 2, dtype=torch.float64, generator=generator)
        ranges = (self.brightness, self.contrast, self.saturation)
        enabled = torch.tensor([r is not None for r in ranges])
        on = enabled[order]                                            # [n, 3]: is the op at this place of the order enabled
        slot = on.to(torch.int64).cumsum(1) - 1
        rec = torch.zeros(n, COLOR_WORDS, dtype=torch.int64)
        rec[:, 0] = torch.where(on, (order + 1) << (2 * slot).clamp_min(0), torch.zeros_like(order)).sum(1)
        rec[:, 0] |= (p[:, 0] < self.grayscale).to(torch.int64) << 8
        rec[:, 0] |= (p[:, 1] < self.solarize).to(torch.int64) * (1 << 9 | self.solarize_threshold << 16)
        for j, r in enumerate(ranges):
            if r is not None:
                factor = (r[0] + f[:, j] * (r[1] - r[0])).to(torch.float32)
                rec[:, 1 + j] = factor.view(torch.int32).to(torch.int64)
        return rec.to(torch.int32)


BLUR_WORDS = 4
BLUR_MAX_BOX_RADIUS = 1


def blur_weights(radius):
    """``(box radius, ww, fw)`` of Pillow's ``ImageFilter.GaussianBlur(radius)``: its three box passes' integer radius and 24-bit fixed-point
    weights, in ``np.float32`` arithmetic as Pillow's C ``float`` code forms them (include/qatvit.h).  A number gives three ints, an array three
    int64 arrays of its shape.  Host only, no GPU."""
    f = np.float32
    r, passes = np.asarray(radius, dtype=f), f(3)
    sigma2 = r * r / passes
    L = np.sqrt(f(12) * sigma2 + f(1))
    l = np.floor((L - f(1)) / f(2))
    a = (f(2) * l + f(1)) * (l * (l + f(1)) - f(3) * sigma2) / (f(6) * (sigma2 - (l + f(1)) * (l + f(1))))
    box = l + a
    assert box.dtype == f
    rad = box.astype(np.int64)                                       # (int)box and (uint32)(...): truncation of non-negative values
    ww = (f(1 << 24) / (box * f(2) + f(1))).astype(np.int64)
    fw = ((1 << 24) - (2 * rad + 1) * ww) // 2
    return (int(rad), int(ww), int(fw)) if r.ndim == 0 else (rad, ww, fw)


def _blur_radius_range(radius):
    number = lambda t: not isinstance(t, bool) and isinstance(t, (int, float)) and math.isfinite(t)   # noqa: E731
    if number(radius):
        radius = (radius, radius)
    if not (isinstance(radius, (tuple, list)) and len(radius) == 2 and all(number(t) for t in radius) and 0 <= radius[0] <= radius[1]):
        raise ValueError(f"radius must be a number >= 0 or a pair of finite numbers 0 <= low <= high, got {radius!r}")
    lo, hi = float(radius[0]), float(radius[1])
    if blur_weights(hi)[0] > BLUR_MAX_BOX_RADIUS:
        raise ValueError(f"radius up to {hi!r} gives the box radius {blur_weights(hi)[0]}: the native blur serves box radii up to "
                         f"{BLUR_MAX_BOX_RADIUS}, which is a Gaussian radius below sqrt(6) = 2.449...")
    return lo, hi


def _blur_records(on, radius):
    """int32 [n, 4] of a bool tensor `on` and a float64 tensor `radius`: the record of a sample that is not blurred is all zero."""
    rad, ww, fw = blur_weights(radius.numpy().astype(np.float32))
    rec = np.stack([1 | rad << 8, ww, fw, np.zeros_like(ww)], 1) * on.numpy()[:, None]
    return torch.from_numpy(rec.astype(np.int32))


class GaussianBlur:
    """DeiT-III's / timm's ``GaussianBlur(p)``: with probability ``p``, ``img.filter(ImageFilter.GaussianBlur(radius=uniform(*radius)))`` of the
    uint8 image behind the resize, as one four-word int32 record per sample (include/qatvit.h): word 0 bit 0 "on" and the integer box radius
    in bits 8..15, word 1 ``ww``, word 2 ``fw`` (``blur_weights``), word 3 zero.  The blur stands behind grayscale / solarize and in front of
    the jitter ops of a ``ColorJitter`` record; the result equals Pillow's.  A ``radius`` range whose upper end gives a box radius above 1
    (a Gaussian radius of sqrt(6) or more) is refused.  Built and drawn on the host; needs no GPU."""

    def __init__(self, p=1.0, radius=(0.1, 2.0)):
        if isinstance(p, bool) or not isinstance(p, (int, float)) or not 0 <= p <= 1:
            raise ValueError(f"p must be a probability 0 .. 1, got {p!r}")
        self.p, self.radius = float(p), _blur_radius_range(radius)

    def draw(self, n, generator=None):
        """int32 CPU tensor [n, 4].  The rule, all from `generator`, in this order: ``c = torch.rand(n, dtype=float64)``: sample k is blurred
        where ``c[k] < p``; ``u = torch.rand(n, dtype=float64)``: its Gaussian radius is ``fp32(low + u[k] * (high - low))``.  A sample that is
        not blurred gets the all-zero record.  Both draws are always made, so the generator's position depends on `n` only."""
        c = torch.rand(n, dtype=torch.float64, generator=generator)
        u = torch.rand(n, dtype=torch.float64, generator=generator)
        return _blur_records(c < self.p, self.radius[0] + u * (self.radius[1] - self.radius[0]))


class ThreeAugment:
    """DeiT-III's 3-Augment (arXiv:2204.07118): per sample exactly one of grayscale, solarize and Gaussian blur, chosen uniformly, then
    ``ColorJitter(color_jitter, color_jitter, color_jitter)``.  ``draw`` returns the colour records and the blur records of the same samples;
    ``ColorJitter``'s two independent coins cannot express the choice.  Built and drawn on the host; needs no GPU."""

    def __init__(self, color_jitter=0.3, radius=(0.1, 2.0), solarize_threshold=128):
        # the jitter part: ColorJitter's validation and its draw; its own coins are off and the choice below sets the bits
        self.jitter = ColorJitter(color_jitter, color_jitter, color_jitter, solarize_threshold=solarize_threshold)
        self.radius = _blur_radius_range(radius)
        self.solarize_threshold = solarize_threshold

    @property
    def contrast(self):
        return self.jitter.contrast

    def draw(self, n, generator=None):
        """``(color int32 [n, 4], blur int32 [n, 4])`` CPU tensors.  The rule, all from `generator`, in this order: ``ColorJitter.draw(n)`` of
        the jitter (a random order of the enabled ops and their factors); ``c = torch.rand(n, dtype=float64)``: the choice
        ``floor(3 * c)`` - 0 grayscale, 1 solarize (with the threshold), 2 blur; ``u = torch.rand(n, dtype=float64)``: the Gaussian radius
        ``fp32(low + u * (high - low))`` of a blurred sample.  Every draw is always made: the generator's position depends on `n` only."""
        color = self.jitter.draw(n, generator).to(torch.int64)
        c = torch.rand(n, dtype=torch.float64, generator=generator)
        u = torch.rand(n, dtype=torch.float64, generator=generator)
        choice = torch.clamp((3.0 * c).floor().to(torch.int64), max=2)
        color[:, 0] |= (choice == 0).to(torch.int64) << 8
        color[:, 0] |= (choice == 1).to(torch.int64) * (1 << 9 | self.solarize_threshold << 16)
        return color.to(torch.int32), _blur_records(choice == 2, self.radius[0] + u * (self.radius[1] - self.radius[0]))


def _cuda_device(who, device):
    """The device of a transform: a CUDA device with its index resolved."""
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError(f"{who} runs on MI355X only: device must be a CUDA device")
    return torch.device("cuda", torch.cuda.current_device()) if device.index is None else device


def _source_batch(who, data_u8, index, h, w, device):
    """``(N, B, index pointer)`` of the uint8 ``[N, h, w, 3]`` source of a transform named `who` and the batch's ``index`` (or None)."""
    if not isinstance(data_u8, torch.Tensor) or not data_u8.is_cuda:
        raise RuntimeError(f"{who} runs on MI355X only: move the uint8 images to the GPU")
    if data_u8.dtype != torch.uint8:
        raise TypeError(f"images must be uint8, got {data_u8.dtype}")
    if data_u8.dim() != 4 or tuple(data_u8.shape[1:]) != (h, w, 3):
        raise ValueError(f"images must be [N, {h}, {w}, 3] (HWC), got {tuple(data_u8.shape)}")
    if not data_u8.is_contiguous() or data_u8.device != device:
        raise ValueError(f"images must be contiguous and on {device}")
    if index is None:
        return data_u8.shape[0], data_u8.shape[0], None
    if index.dtype != torch.int64 or index.dim() != 1 or not index.is_contiguous() or index.device != device:
        raise ValueError(f"index must be a contiguous 1-D int64 tensor on {device}")
    return data_u8.shape[0], index.shape[0], index.data_ptr()


def _out_batch(out, dtype, shape, device):
    """`out`, or a fresh tensor where it is None."""
    if out is None:
        return torch.empty(shape, dtype=dtype, device=device)
    if out.dtype != dtype or tuple(out.shape) != shape or not out.is_contiguous() or out.device != device:
        raise ValueError(f"out must be a contiguous {'fp32' if dtype == torch.float32 else 'uint8'} {list(shape)} tensor on {device}")
    return out


def _check_records(name, t, shape, device):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or tuple(t.shape) != shape or not t.is_contiguous() or t.device != device:
        raise ValueError(f"{name} must be a contiguous int32 {list(shape)} tensor on {device}")


class GpuResizeNormalize:
    """uint8 ``[N, S, S, 3]`` images on the device -> fp32 ``[B, 3, D, D]``: Resize(D, BICUBIC) + ToTensor() + Normalize(mean, std) in one launch.
    With ``aug`` (int32 ``[B]`` on the device, the words of ``RandomCropFlip.draw``; word b belongs to batch position b) the source of sample b is
    cropped at its offset out of the image extended by ``padding_mode`` / ``fill`` and flipped first, in the same launch.  ``padding`` states the
    bound of the offsets in ``aug`` where the caller knows it: reflect mode is exact for offsets up to ``S - 1`` and a larger bound is refused.
    With ``mix`` (int32 ``[B, 6]`` on the device, the records of ``MixupCutmix.draw``) sample b is blended with, or takes a box from, what this
    call produces for its partner position, in the same launch.
    With ``rrc`` (int32 ``[B, 2]`` on the device, the records of ``RandomResizedCrop.draw``; record b belongs to batch position b) the source of
    sample b is the window of its record, mirrored where the record says so, and that window is what is resized to ``D x D``, in the same launch;
    ``mix`` applies behind it as it does otherwise.  ``rrc`` stands instead of ``aug``: the record carries its own flip, and padding does not
    apply.  The tables of every window side are built on the first such call and kept on the device.
    With ``erase`` (int32 ``[B, 8]`` on the device, the records of ``RandomErasing.draw``; record b belongs to batch position b) the box of sample
    b's record is filled, or set to noise, in its normalised output, in the same launch: behind ``aug`` / ``rrc`` and in front of ``mix``, whose
    partner is erased by its own record.
    With ``color`` (int32 ``[B, 4]`` on the device, the records of ``ColorJitter.draw``; record b belongs to batch position b) the uint8 image
    behind the resize goes through grayscale, solarize and the jitter ops of its record, in the same launch: behind ``aug`` / ``rrc``, in front
    of ``Normalize``, ``erase`` and ``mix``, whose partner is coloured by its own record.  The contrast op needs the mean luma of the whole
    sample, which a statistics launch in front of the batch launch sums into ``color_sums(B)``; ``contrast=False`` is the caller's promise that
    no record holds a contrast op, and leaves that launch out.
    With ``blur`` (int32 ``[B, 4]`` on the device, the records of ``GaussianBlur.draw`` or the second result of ``ThreeAugment.draw``; record b
    belongs to batch position b) the uint8 image behind the resize is blurred as Pillow's ``ImageFilter.GaussianBlur`` blurs it, in the same
    launch: behind grayscale / solarize and in front of the jitter ops of ``color``, whose contrast mean is then that of the blurred image;
    the partner of a mix record is blurred by its own record.  A workgroup whose record says "no blur" runs no pass."""

    def __init__(self, src_size, out_size=224, mean=IMAGENET_MEAN, std=IMAGENET_STD, device="cuda"):
        self.src_size, self.out_size = int(src_size), int(out_size)
        self.device = _cuda_device("GpuResizeNormalize", device)
        self.mean, self.std = tuple(float(v) for v in mean), tuple(float(v) for v in std)
        self.coeffs = torch.cat([t.flatten() for t in resize_tables(self.src_size, self.out_size)]).to(self.device)
        self.table = value_table(mean, std).to(self.device)

    def window_tables(self):
        """The device copy of ``resize_window_tables(S, D)``, built on first use."""
        if getattr(self, "windows", None) is None:
            self.windows = resize_window_tables(self.src_size, self.out_size).to(self.device)
        return self.windows

    def color_sums(self, B):
        """The uint32 ``[B]`` workspace (as int32) that the calls with ``color`` records of a batch of B hand to the library, one per batch size,
        made on first use: behind such a call element b holds the luma sum that the contrast op of record b used (0: no contrast op)."""
        if getattr(self, "_sums", None) is None:
            self._sums = {}
        if B not in self._sums:
            self._sums[B] = torch.zeros(B, dtype=torch.int32, device=self.device)
        return self._sums[B]

    def __call__(self, data_u8, index=None, out=None, aug=None, padding_mode="constant", fill=0, padding=None, mix=None, rrc=None, erase=None,
                 color=None, contrast=True, blur=None):
        S, D = self.src_size, self.out_size
        if rrc is not None and aug is not None:
            raise ValueError("rrc and aug are mutually exclusive: the rrc record carries its own flip, and padding does not apply to a window")
        N, B, ip = _source_batch("GpuResizeNormalize", data_u8, index, S, S, self.device)
        out = _out_batch(out, torch.float32, (B, 3, D, D), self.device)
        mode, fill = _padding_mode_and_fill(padding_mode, fill)
        if aug is not None:
            _check_records("aug", aug, (B,), self.device)
            if mode == PADDING_MODES["reflect"] and padding is not None and padding > S - 1:
                raise ValueError(f"reflect padding reflects once: offsets up to {padding} exceed S - 1 = {S - 1}")
        for name, t, words in (("mix", mix, MIX_WORDS), ("erase", erase, ERASE_WORDS), ("color", color, COLOR_WORDS), ("blur", blur, BLUR_WORDS),
                               ("rrc", rrc, RRC_WORDS)):
            if t is not None:
                _check_records(name, t, (B, words), self.device)
        if not B:
            return out
        # The narrowest entry that takes the records present, and its arguments between D and out.  An entry takes the records in front of its own as
        # they are, absent ones as NULL; without `contrast` the colour entries get no workspace and no statistics launch runs.
        opt = lambda t: None if t is None else t.data_ptr()   # noqa: E731
        if blur is not None:
            level = "_blur"
            records = (opt(erase), opt(color), self.color_sums(B).data_ptr() if color is not None and contrast else None, blur.data_ptr())
        elif color is not None:
            level, records = "_color", (opt(erase), color.data_ptr(), self.color_sums(B).data_ptr() if contrast else None)
        elif erase is not None:
            level, records = "_erase", (erase.data_ptr(),)
        else:
            level, records = "", ()
        if rrc is not None:
            name, args = "qatvit_image_batch_rrc" + level, (self.window_tables().data_ptr(), self.table.data_ptr(), rrc.data_ptr(), opt(mix)) + records
        elif level or mix is not None:
            name, args = "qatvit_image_batch" + (level or "_mix"), (self.coeffs.data_ptr(), self.table.data_ptr(), opt(aug), mode, fill, opt(mix)) + records
        elif aug is not None:
            name, args = "qatvit_image_batch_aug", (self.coeffs.data_ptr(), self.table.data_ptr(), aug.data_ptr(), mode, fill)
        else:
            name, args = "qatvit_image_batch", (self.coeffs.data_ptr(), self.table.data_ptr())
        with torch.cuda.device(self.device):
            native.check(getattr(native.lib(), name)(data_u8.data_ptr(), ip, B, N, S, D, *args, out.data_ptr(), native.stream_ptr()), name)
        return out


WINDOW_TAPS = 17
WINDOW_MAX_SCALE = 4
BLUR_LDS_CAP = 64 * 1024


def window_stage_tables(max_side: int, out_size: int):
    """int32 CPU tensor [max_side, 19 * D]: row n - 1 holds xmin [D], ntaps [D], coef [D, 17] of Pillow's 8-bit bicubic resample from n to
    out_size one after the other, for every window side n = 1 .. max_side <= 4 * D, with the filter stretched where n > D (host only, no GPU).
    For n <= D the first four coefficients, xmin and ntaps are ``resize_tables(n, D)``.  4 * 19 * D * max_side bytes: 15.3 MB at D = 224
    with max_side = 896, 4.4 MB for 256 x 256 sources."""
    nbytes = native.lib().qatvit_image_window_coeffs_bytes(int(max_side), int(out_size))
    if nbytes < 0:
        native.check(1, "qatvit_image_window_coeffs_bytes")
    out = torch.empty(int(max_side), nbytes // (4 * int(max_side)), dtype=torch.int32)
    native.check(native.lib().qatvit_image_window_coeffs(int(max_side), int(out_size), out.data_ptr()), "qatvit_image_window_coeffs")
    return out


def center_crop_window(H, W, frac=1.0):
    """``(top, left, side, side)`` of torchvision's ``CenterCrop(side)`` on an ``H x W`` image, ``side = max(1, round(frac * min(H, W)))``:
    ``top = int(round((H - side) / 2.0))``, ``left = int(round((W - side) / 2.0))`` with Python's round.  As the default window of a
    ``GpuWindowResize`` / ``GpuWideResizeNormalize`` this is crop-THEN-resize: the central square of the source resized to the output, not
    ``Resize(256)`` + ``CenterCrop(224)``, which resizes first and whose crop is then not resampled again."""
    H, W = int(H), int(W)
    if H < 1 or W < 1 or not 0 < frac <= 1:
        raise ValueError(f"center_crop_window needs H, W >= 1 and 0 < frac <= 1, got {H}, {W}, {frac!r}")
    side = max(1, int(round(frac * min(H, W))))
    return int(round((H - side) / 2.0)), int(round((W - side) / 2.0)), side, side


def _pair(src_size):
    if not isinstance(src_size, (tuple, list)) or len(src_size) != 2:
        raise ValueError(f"src_size must be a pair (H, W), got {src_size!r}")
    return int(src_size[0]), int(src_size[1])


class GpuWindowResize:
    """uint8 ``[N, H, W, 3]`` images on the device -> uint8 ``[B, D, D, 3]``: per batch position the window of its record, mirrored where the
    record says so, resized as ``Image.crop(window).resize((D, D), BICUBIC)`` resizes it, in one launch (``qatvit_image_window_u8``; DESIGN.md
    section 7x).  The source may be a rectangle and larger than the output, up to ``4 * D`` on a side: Pillow's filter is stretched where a
    window side exceeds D, up to 17 taps.  ``rrc`` (int32 ``[B, 2]`` on the device) holds ``RandomResizedCrop.draw(n, (H, W))``'s records,
    record b for batch position b; ``rrc=None`` takes the default window for every sample: the whole image, or ``window = (top, left, h, w)``
    (e.g. ``center_crop_window(H, W)``).  The tables of every window side are built at construction and kept on the device."""

    def __init__(self, src_size, out_size=224, device="cuda", window=None):
        self.src_size, self.out_size = _pair(src_size), int(out_size)
        H, W = self.src_size
        if window is None:
            window = (0, 0, H, W)
        if not isinstance(window, (tuple, list)) or len(window) != 4 or not all(isinstance(t, int) and not isinstance(t, bool) for t in window):
            raise ValueError(f"window must be four integers (top, left, h, w), got {window!r}")
        top, left, h, w = window
        if not (1 <= h <= H and 1 <= w <= W and 0 <= top <= H - h and 0 <= left <= W - w):
            raise ValueError(f"window {window!r} does not lie inside the {H} x {W} source")
        self.window = (top, left, h, w)
        self.device = _cuda_device("GpuWindowResize", device)
        if min(H, W) < 8:
            raise ValueError(f"the source {H} x {W} has a side below 8")
        self.max_side = max(H, W)
        self.tables = window_stage_tables(self.max_side, self.out_size).to(self.device)   # (refuses a bad D and a side above 4 * D)
        self._default = {}

    def default_records(self, B):
        """int32 ``[B, 2]`` on the device: the default window's record at every position; one tensor per distinct batch size, made on first
        use and kept for the life of the transform."""
        if B not in self._default:
            top, left, h, w = self.window
            self._default[B] = torch.tensor([[top | left << 16, h | w << 15]] * B, dtype=torch.int32).reshape(B, RRC_WORDS).to(self.device)
        return self._default[B]

    def __call__(self, data_u8, index=None, rrc=None, out=None):
        (H, W), D = self.src_size, self.out_size
        N, B, ip = _source_batch("GpuWindowResize", data_u8, index, H, W, self.device)
        out = _out_batch(out, torch.uint8, (B, D, D, 3), self.device)
        if rrc is None:
            rrc = self.default_records(B)
        else:
            _check_records("rrc", rrc, (B, RRC_WORDS), self.device)
        if not B:
            return out
        with torch.cuda.device(self.device):
            native.check(native.lib().qatvit_image_window_u8(data_u8.data_ptr(), ip, B, N, H, W, D, self.tables.data_ptr(), self.max_side,
                                                             rrc.data_ptr(), out.data_ptr(), native.stream_ptr()), "qatvit_image_window_u8")
        return out


class GpuBytesBlurNormalize:
    """uint8 ``[B, D, D, 3]`` bytes on the device, at batch positions (what ``GpuWindowResize`` writes) -> fp32 ``[B, 3, D, D]``: the chain of
    ``GpuResizeNormalize``'s ``blur`` form behind its resize, in one launch that takes the bytes as the resized image
    (``qatvit_image_bytes_blur``).  ``blur`` (int32 ``[B, 4]``) is required; ``mix``, ``erase``, ``color`` and
    ``contrast`` have ``GpuResizeNormalize``'s meaning.  The result is bitwise what ``GpuResizeNormalize(D, D)(bytes, blur=...)`` defines,
    also at the sizes which that form refuses for its LDS request (D = 224); a record of "no blur" gives bitwise the colour form's result.
    LDS holds the value table and the image buffers only: 40,704 bytes at D = 224, 43,392 with ``mix``.  With ``mix`` an output above 344 is
    refused by the library."""

    def __init__(self, out_size=224, mean=IMAGENET_MEAN, std=IMAGENET_STD, device="cuda"):
        self.out_size = int(out_size)
        self.device = _cuda_device("GpuBytesBlurNormalize", device)
        self.mean, self.std = tuple(float(v) for v in mean), tuple(float(v) for v in std)
        self.table = value_table(mean, std).to(self.device)
        self._sums = {}

    def color_sums(self, B):
        """The uint32 ``[B]`` workspace (as int32) of the calls with ``color`` records of a batch of B, one per batch size, made on first use:
        behind such a call element b holds the luma sum that the contrast op of record b used (0: no contrast op)."""
        if B not in self._sums:
            self._sums[B] = torch.zeros(B, dtype=torch.int32, device=self.device)
        return self._sums[B]

    def __call__(self, bytes_u8, out=None, mix=None, erase=None, color=None, contrast=True, blur=None):
        D = self.out_size
        _, B, _ = _source_batch("GpuBytesBlurNormalize", bytes_u8, None, D, D, self.device)
        out = _out_batch(out, torch.float32, (B, 3, D, D), self.device)
        if blur is None:
            raise ValueError("blur records are required: without them the second stage is GpuResizeNormalize(D, D)")
        for name, t, words in (("mix", mix, MIX_WORDS), ("erase", erase, ERASE_WORDS), ("color", color, COLOR_WORDS), ("blur", blur, BLUR_WORDS)):
            if t is not None:
                _check_records(name, t, (B, words), self.device)
        if not B:
            return out
        opt = lambda t: None if t is None else t.data_ptr()   # noqa: E731
        sums = self.color_sums(B).data_ptr() if color is not None and contrast else None
        with torch.cuda.device(self.device):
            native.check(native.lib().qatvit_image_bytes_blur(bytes_u8.data_ptr(), B, D, self.table.data_ptr(), opt(mix), opt(erase), opt(color), sums,
                                                              blur.data_ptr(), out.data_ptr(), native.stream_ptr()), "qatvit_image_bytes_blur")
        return out


class GpuWideResizeNormalize:
    """Stands where a ``GpuResizeNormalize`` stands, for uint8 ``[N, H, W, 3]`` sources that are rectangles or larger than the output (up to
    ``4 * D`` on a side): two launches per batch.  Stage 1 (``GpuWindowResize``) writes the uint8 ``[B, D, D, 3]`` bytes of every sample's
    resized window into a staging buffer this object owns, one per batch size (no allocation per step, and static addresses, so a captured
    graph replays); stage 2 is a ``GpuResizeNormalize(D, D)`` on those bytes at batch positions, whose resize is the identity and which
    applies ``color``, ``erase``, ``mix`` and ``Normalize`` as it does for a small source.  ``__call__`` has ``GpuResizeNormalize``'s
    keywords; ``rrc`` records are ``RandomResizedCrop.draw(n, (H, W))``'s, ``rrc=None`` is the default ``window`` (the whole image, or e.g.
    ``center_crop_window(H, W)``).  ``aug`` is refused: padding applies to CIFAR-style sources.
    ``blur`` records are served where the object was made with ``blur=True``: stage 2 of a call with ``blur=records`` is then a
    ``GpuBytesBlurNormalize`` on the staged bytes (still two launches, plus the statistics launch that colour records with contrast bring),
    which is what ``GpuImageLoader(..., blur=GaussianBlur(...))`` and ``three_augment=ThreeAugment(...)`` need; ``mix`` with ``blur`` is
    refused by the library above D = 344.  Without the switch ``blur`` is refused as before: the one-launch blur forms keep source rows and
    planes in LDS, and at S = D = 224 that is 89,536 bytes (98,272 with mix records), above the 65,536-byte cap."""

    def __init__(self, src_size, out_size=224, mean=IMAGENET_MEAN, std=IMAGENET_STD, device="cuda", window=None, blur=False):
        self.stage = GpuWindowResize(src_size, out_size, device, window)
        self.src_size, self.out_size, self.device, self.window = self.stage.src_size, self.stage.out_size, self.stage.device, self.stage.window
        self.inner = GpuResizeNormalize(self.out_size, self.out_size, mean, std, self.device)
        self.mean, self.std = self.inner.mean, self.inner.std
        self._staged = {}
        self.blur = bool(blur)
        self.inner_blur = GpuBytesBlurNormalize(self.out_size, mean, std, self.device) if self.blur else None
        if self.blur:
            self.inner._sums = self.inner_blur._sums                  # one workspace per batch size, whichever second stage a call takes

    def staged(self, B):
        """The uint8 ``[B, D, D, 3]`` staging buffer of a batch of B, made on first use: behind a call it holds stage 1's bytes.  One buffer
        per distinct batch size (a loader has two: the full and the last batch), kept for the life of the transform, never released."""
        if B not in self._staged:
            self._staged[B] = torch.empty(B, self.out_size, self.out_size, 3, dtype=torch.uint8, device=self.device)
        return self._staged[B]

    def color_sums(self, B):
        return self.inner.color_sums(B)

    def refuse(self, aug=None, blur=None):
        """Raises for what this object does not serve: ``aug`` always, ``blur`` unless it was made with ``blur=True`` (an object that never ran
        the constructor has the switch off)."""
        if aug is not None:
            raise ValueError("aug does not apply to a wide source: RandomCrop's padding is for CIFAR-style sources; use rrc records")
        if blur is not None and not getattr(self, "blur", False):
            raise NotImplementedError(f"blur is not served on a wide source: the blur forms stage source rows plus planes in LDS, and at S = D = 224 "
                                      f"they ask for 89,536 bytes, above the cap of {BLUR_LDS_CAP} bytes")

    def __call__(self, data_u8, index=None, out=None, aug=None, padding_mode="constant", fill=0, padding=None, mix=None, rrc=None, erase=None,
                 color=None, contrast=True, blur=None):
        self.refuse(aug, blur)                                       # padding_mode, fill and padding describe aug, which is refused: nothing reads them
        if not isinstance(data_u8, torch.Tensor) or not data_u8.is_cuda:
            raise RuntimeError("GpuWideResizeNormalize runs on MI355X only: move the uint8 images to the GPU")
        B = data_u8.shape[0] if index is None else index.shape[0]
        staged = self.stage(data_u8, index, rrc, out=self.staged(B))
        if blur is not None:
            return self.inner_blur(staged, out=out, mix=mix, erase=erase, color=color, contrast=contrast, blur=blur)
        return self.inner(staged, None, out=out, mix=mix, erase=erase, color=color, contrast=contrast)


def epoch_batches(n, batch_size, shuffle=False, sampler=None, drop_last=False, generator=None):
    """The plan of one epoch, on the host: a list of 1-D int64 CPU tensors, batch by batch, with DataLoader's meaning of every argument (its own
    sampler classes draw the order; shuffle is RandomSampler's permutation from `generator`).  `sampler` is any iterable of indices."""
    if sampler is not None and shuffle:
        raise ValueError("sampler option is mutually exclusive with shuffle")
    if sampler is None:
        sampler = RandomSampler(range(n), generator=generator) if shuffle else SequentialSampler(range(n))
    return [torch.tensor(b, dtype=torch.int64) for b in BatchSampler(sampler, batch_size, drop_last)]


class GpuImageLoader:
    """Iterates ``(images, labels)`` device batches of a uint8 data set that lives on the device; stands where a ``DataLoader`` over the
    transformed data set stood.  An epoch's indices go to the device once; drawing a batch is one gather of labels and one launch, with no host
    synchronisation, and every batch is a fresh tensor.  ``return_index=True`` yields ``(images, labels, index)``: ``index`` is the batch's slice of
    the epoch plan on the device (int64), the row numbers a per-sample table such as ``TeacherLogitTable`` is read with.  ``augment`` (a
    ``RandomCropFlip``) crops and flips every drawn sample inside the same launch: an epoch's words are drawn right after its plan, from the same
    ``generator``, and travel to the device with the indices in the one copy; the yielded tuples are the same.  ``mix`` (a ``MixupCutmix``) mixes
    every batch inside the same launch: an epoch's records are drawn after the plan and after the words, travel in the same copy, and the batch's
    device slice (int32 ``[B, 6]``, what ``kd_ce_loss_mix`` / ``TeacherLogitTable.loss(mix=...)`` take) is the last element of every tuple.
    ``crop`` (a ``RandomResizedCrop``) stands instead of ``augment``: every drawn sample is a resized window of its image, inside the same launch;
    an epoch's records are drawn after the plan and before the mix records, from the same ``generator``, and travel in the same copy; the yielded
    tuples are the same.  ``erase`` (a ``RandomErasing``) erases a box of every drawn sample's output inside the same launch, with ``augment`` or
    ``crop`` and in front of ``mix``: an epoch's records are drawn last, after the plan, the words or windows and the mix records, so that a seed
    gives the plan, words, windows and mix records it gives without ``erase``; they travel in the same copy, four int64 elements per sample, and the
    yielded tuples are the same (the loss needs nothing from an erase record).  ``color`` (a ``ColorJitter``) applies grayscale, solarize and
    the colour jitter to every drawn sample inside the same launch (behind a statistics launch where contrast is enabled), with ``augment`` or
    ``crop``, with or without ``mix`` / ``erase``: an epoch's colour records are drawn last of all, after the erase records, so that a seed
    gives the plan, words, windows, mix and erase records it gives without ``color``; they travel in the same copy, two int64 elements per
    sample, and the yielded tuples are the same (the loss needs nothing from a colour record).  ``blur`` (a ``GaussianBlur``) blurs the drawn
    samples its coin picks inside the same launch: an epoch's blur records are drawn last of all, after the colour records, so that a seed
    gives the plan, words, windows, mix, erase and colour records it gives without ``blur``; they travel in the same copy, two int64 elements
    per sample.  ``three_augment`` (a ``ThreeAugment``) stands instead of ``color`` and ``blur`` and draws both kinds of record, where they
    stand: DeiT-III's one-of-three choice and its colour jitter."""

    def __init__(self, data_u8, labels, batch_size, shuffle=False, sampler=None, drop_last=False, transform=None, generator=None, device="cuda",
                 return_index=False, augment=None, mix=None, crop=None, erase=None, color=None, blur=None, three_augment=None):
        if sampler is not None and shuffle:
            raise ValueError("sampler option is mutually exclusive with shuffle")
        data_u8, labels = torch.as_tensor(data_u8), torch.as_tensor(labels)
        wide = isinstance(transform, GpuWideResizeNormalize)
        if wide:
            H, W = transform.src_size
            if data_u8.dtype != torch.uint8 or data_u8.dim() != 4 or tuple(data_u8.shape[1:]) != (H, W, 3):
                raise ValueError(f"images must be uint8 [N, {H}, {W}, 3] (HWC) for this transform, got {data_u8.dtype} {tuple(data_u8.shape)}")
            transform.refuse(augment, blur if blur is not None else three_augment)
        elif data_u8.dtype != torch.uint8 or data_u8.dim() != 4 or data_u8.shape[1] != data_u8.shape[2] or data_u8.shape[3] != 3:
            raise ValueError(f"images must be uint8 [N, S, S, 3] (HWC), got {data_u8.dtype} {tuple(data_u8.shape)}")
        # what crop.draw takes: the side of a square source, or (H, W) of a wide transform's
        self.crop_size = tuple(transform.src_size) if wide else data_u8.shape[1]
        if labels.dim() != 1 or labels.shape[0] != data_u8.shape[0]:
            raise ValueError("labels must be one integer per image")
        self.transform = transform if transform is not None else GpuResizeNormalize(data_u8.shape[1], device=device)
        self.device = self.transform.device
        self.data = data_u8.to(self.device).contiguous()
        self.labels = labels.to(self.device, torch.int64).contiguous()
        self.batch_size, self.shuffle, self.sampler, self.drop_last, self.generator = int(batch_size), shuffle, sampler, drop_last, generator
        self.return_index = bool(return_index)
        for name, v, cls in (("augment", augment, RandomCropFlip), ("mix", mix, MixupCutmix), ("crop", crop, RandomResizedCrop),
                             ("erase", erase, RandomErasing), ("color", color, ColorJitter), ("three_augment", three_augment, ThreeAugment),
                             ("blur", blur, GaussianBlur)):
            if v is None:
                continue
            if not isinstance(v, cls):
                raise TypeError(f"{name} must be a {cls.__name__}, got {type(v).__name__}")
            if name == "augment" and v.padding > self.data.shape[1] - 1:
                raise ValueError(f"augment.padding {v.padding} exceeds S - 1 = {self.data.shape[1] - 1}")
            if name == "crop" and augment is not None:
                raise ValueError("crop and augment are mutually exclusive: the crop's record carries its own flip, and padding does not apply")
            if name == "three_augment" and (color is not None or blur is not None):
                raise ValueError("three_augment is exclusive with color and blur: it draws both records itself")
        self.augment, self.mix, self.crop, self.erase, self.color, self.blur, self.three_augment = augment, mix, crop, erase, color, blur, three_augment

    def __len__(self):
        n = len(self.sampler) if self.sampler is not None else self.data.shape[0]
        return n // self.batch_size if self.drop_last else (n + self.batch_size - 1) // self.batch_size

    def __iter__(self):
        g = self.generator
        plan = epoch_batches(self.data.shape[0], self.batch_size, self.shuffle, self.sampler, self.drop_last, g)
        if not plan:
            return
        flat = torch.cat(plan)
        n, a, three = flat.shape[0], self.augment, self.three_augment
        size = lambda: self.transform.out_size   # noqa: E731   (read only where a record kind needs it: a loader without options takes any callable)
        # The record kinds in drawing order, which is the order of their sections behind the n indices: (option, the keywords the transform takes
        # the records under, int32 words per sample of each, the draw: one tensor per keyword).  A seed gives the plan and the records of every
        # kind it gives without the later kinds
        kinds = [(a, ("aug",), (1,), lambda: (a.draw(n, g),)),
                 (self.crop, ("rrc",), (RRC_WORDS,), lambda: (self.crop.draw(n, self.crop_size, g),)),
                 (self.mix, ("mix",), (MIX_WORDS,), lambda: (self.mix.draw([b.shape[0] for b in plan], size(), g),)),
                 (self.erase, ("erase",), (ERASE_WORDS,), lambda: (self.erase.draw(n, size(), g),)),
                 (self.color, ("color",), (COLOR_WORDS,), lambda: (self.color.draw(n, g),)),
                 (self.blur, ("blur",), (BLUR_WORDS,), lambda: (self.blur.draw(n, g),)),
                 (three, ("color", "blur"), (COLOR_WORDS, BLUR_WORDS), lambda: three.draw(n, g))]
        kinds = [k[1:] for k in kinds if k[0] is not None]
        # one pinned block and one asynchronous copy (the caching host allocator keeps the block until the copy has run): n int64 indices, then
        # every section's n * words int32 in whole int64 elements
        bounds = [n]
        for _, words, _ in kinds:
            for w in words:
                bounds.append(bounds[-1] + (n * w + 1) // 2)
        host = torch.empty(bounds[-1], dtype=torch.int64, pin_memory=True)

        def sections(block):
            """{keyword: the int32 [n, words] view ([n] for the one-word kind) of its section of `block`}, in drawing order."""
            keys = [(key, w) for keywords, words, _ in kinds for key, w in zip(keywords, words)]
            return {key: block[lo:hi].view(torch.int32)[:n * w].view((n, w) if w > 1 else (n,)) for (key, w), lo, hi in zip(keys, bounds, bounds[1:])}

        host[:n].copy_(flat)
        into = sections(host)
        for keywords, _, draw in kinds:
            for key, records in zip(keywords, draw()):
                into[key].copy_(records)
        dev = host.to(self.device, non_blocking=True)
        order, records = dev[:n], sections(dev)
        # what every call of the epoch gets besides its slices: the augment's padding with its words; behind a crop, absent mix records as None;
        # and with any of the late kinds (erase, colour, blur) all of them, absent ones as None, and whether contrast needs the statistics launch
        fixed = {} if a is None else {"padding_mode": a.padding_mode, "fill": a.fill, "padding": a.padding}
        if self.crop is not None:
            fixed["mix"] = None
        if records.keys() & {"erase", "color", "blur"}:
            jitter = self.color if self.color is not None else three
            fixed.update(mix=None, erase=None, color=None, contrast=jitter is not None and jitter.contrast is not None, blur=None)
        o = 0
        for b in plan:
            m = b.shape[0]
            idx, kw = order[o:o + m], dict(fixed, **{key: r[o:o + m] for key, r in records.items()})
            o += m
            x = self.transform(self.data, idx, **kw)
            tail = (idx,) if self.return_index else ()
            yield (x, self.labels.index_select(0, idx)) + tail + ((kw["mix"],) if self.mix is not None else ())


def cifar10_arrays(root, train=True):
    """(uint8 [N, 32, 32, 3], int64 [N]) of the ``cifar-10-batches-py`` directory under `root`, as torchvision's ``CIFAR10(root, train).data`` /
    ``.targets`` hold them.  Never downloads: FileNotFoundError if the directory or one of its batch files is missing."""
    base = os.path.join(root, "cifar-10-batches-py")
    names = [f"data_batch_{i}" for i in range(1, 6)] if train else ["test_batch"]
    data, labels = [], []
    for name in names:
        path = os.path.join(base, name)
        if not os.path.isfile(path):
            raise FileNotFoundError(f"{path} is missing: put the extracted CIFAR-10 python archive under {root} (nothing is downloaded)")
        with open(path, "rb") as f:
            entry = pickle.load(f, encoding="latin1")
        data.append(np.asarray(entry["data"], dtype=np.uint8))
        labels.extend(entry["labels"] if "labels" in entry else entry["fine_labels"])
    data = np.vstack(data).reshape(-1, 3, 32, 32).transpose(0, 2, 3, 1)
    return np.ascontiguousarray(data), np.asarray(labels, dtype=np.int64)
