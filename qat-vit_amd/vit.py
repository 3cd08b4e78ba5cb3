"""VisionTransformer module tree for the QAT student / KD teacher (host side).

The reference obtains this tree from ``timm.create_model("vit_small_patch16_224" |
"vit_base_patch16_224", ...)`` (/root/reference/src/models/model_registry.py:167-172,
:228-233).  What the rest of the reference relies on is the *tree*, not timm: stock
``nn.Conv2d`` / ``nn.Linear`` / ``nn.LayerNorm`` leaves that ``prepare_qat`` swaps by exact
type (torch/ao/quantization/quantize.py:765), timm's parameter names (so ``model.``-prefixed
checkpoints load, model_registry.py:247-260), deep-copy-ability, and ``.parameters()``.
This file provides exactly that tree; on an MI355X the arithmetic of a QAT-prepared tree
is executed by libqatvit.so (engine.py: ``student_forward``; the frozen teacher: teacher.py), not by
these modules' ``forward``.
"""
from __future__ import annotations

import contextlib
import weakref
from typing import Optional

import torch
import torch.nn as nn

# name -> (embed_dim, depth, num_heads)
ARCH = {
    "vit_small_patch16_224": (384, 12, 6),
    "vit_base_patch16_224": (768, 12, 12),
}


class PatchEmbed(nn.Module):
    def __init__(self, img_size: int, patch_size: int, in_chans: int, embed_dim: int):
        super().__init__()
        self.img_size, self.patch_size = img_size, patch_size
        self.grid = img_size // patch_size
        self.num_patches = self.grid * self.grid
        self.proj = nn.Conv2d(in_chans, embed_dim, kernel_size=patch_size, stride=patch_size)
        self.norm = nn.Identity()

    def forward(self, x):
        x = self.proj(x)
        return self.norm(x.flatten(2).transpose(1, 2))


class Attention(nn.Module):
    def __init__(self, dim: int, num_heads: int):
        super().__init__()
        self.num_heads, self.head_dim = num_heads, dim // num_heads
        self.scale = self.head_dim ** -0.5
        self.qkv = nn.Linear(dim, 3 * dim, bias=True)
        self.q_norm, self.k_norm = nn.Identity(), nn.Identity()
        self.attn_drop = nn.Dropout(0.0)
        self.proj = nn.Linear(dim, dim)
        self.proj_drop = nn.Dropout(0.0)

    def forward(self, x):
        B, N, C = x.shape
        q, k, v = self.qkv(x).view(B, N, 3, self.num_heads, self.head_dim).permute(2, 0, 3, 1, 4).unbind(0)
        a = torch.softmax((self.q_norm(q) * self.scale) @ self.k_norm(k).transpose(-2, -1), dim=-1)
        o = (self.attn_drop(a) @ v).transpose(1, 2).reshape(B, N, C)
        return self.proj_drop(self.proj(o))


class Mlp(nn.Module):
    def __init__(self, dim: int, hidden: int):
        super().__init__()
        self.fc1 = nn.Linear(dim, hidden)
        self.act = nn.GELU()
        self.drop1 = nn.Dropout(0.0)
        self.norm = nn.Identity()
        self.fc2 = nn.Linear(hidden, dim)
        self.drop2 = nn.Dropout(0.0)

    def forward(self, x):
        return self.drop2(self.fc2(self.norm(self.drop1(self.act(self.fc1(x))))))


class DropPath(nn.Module):
    """Stochastic depth per sample, on the branch of a residual block - timm's ``DropPath`` (timm/layers/drop.py): in eval mode or with
    ``drop_prob == 0`` the identity, otherwise ``x * m`` with ``m = x.new_empty(B, 1, .., 1).bernoulli_(keep)``, divided by ``keep`` when
    ``keep > 0 and scale_by_keep``.  No parameters, no buffers; ``prepare_qat`` leaves it where it is and gives it no observer.

    Inside ``forced_drop_path`` a training-mode forward multiplies by the caller's per-sample multipliers instead of drawing (whatever
    ``drop_prob`` is).  On an MI355X the native steps (engine.py, float_engine.py) apply the multipliers in their residual kernels; this
    ``forward`` is the stock path."""

    def __init__(self, drop_prob: float = 0.0, scale_by_keep: bool = True):
        super().__init__()
        self.drop_prob, self.scale_by_keep = float(drop_prob), bool(scale_by_keep)
        self._forced = None   # forced_drop_path: this branch's [B] multipliers

    def forward(self, x):
        if not self.training:
            return x
        shape = (x.shape[0],) + (1,) * (x.dim() - 1)
        if self._forced is not None:
            if self._forced.numel() != x.shape[0]:
                raise RuntimeError(f"forced_drop_path: the table holds {self._forced.numel()} samples, the batch {x.shape[0]}")
            return x * self._forced.to(device=x.device, dtype=x.dtype).view(shape)
        if self.drop_prob == 0.0:
            return x
        keep = 1.0 - self.drop_prob
        m = x.new_empty(shape).bernoulli_(keep)
        if keep > 0.0 and self.scale_by_keep:
            m.div_(keep)
        return x * m

    def extra_repr(self):
        return f"drop_prob={round(self.drop_prob, 3):0.3f}"


class LayerScale(nn.Module):
    """A learnable per-channel scale on the branch of a residual block - timm's ``LayerScale`` (``init_values=`` of its ViTs; the DeiT-III / BEiT /
    DINOv2 checkpoints carry it as ``blocks.i.ls1.gamma`` / ``ls2.gamma``): ``gamma = init_values * ones(dim)``, ``forward`` is ``x * gamma``
    (``x.mul_(gamma)`` with ``inplace``).  ``prepare_qat`` leaves it where it is and gives it no observer, so in the prepared tree it stands behind the
    activation fake-quant of the proj / fc2 output and in front of ``DropPath``.  On an MI355X the native steps apply ``gamma`` - and form its
    gradient - in their residual kernels; this ``forward`` is the stock path."""

    def __init__(self, dim: int, init_values: float = 1e-5, inplace: bool = False):
        super().__init__()
        self.inplace = bool(inplace)
        self.gamma = nn.Parameter(init_values * torch.ones(dim))

    def forward(self, x):
        return x.mul_(self.gamma) if self.inplace else x * self.gamma

    def extra_repr(self):
        return f"dim={self.gamma.numel()}, inplace={self.inplace}"


class Block(nn.Module):
    def __init__(self, dim: int, num_heads: int, mlp_ratio: float, drop_path: Optional[float] = None, init_values: Optional[float] = None):
        """init_values: falsy - no LayerScale (``nn.Identity``, the tree as it always was); else ``LayerScale(dim, init_values)`` on both branches.
        drop_path: None - no stochastic depth in this model (``nn.Identity``, the tree as it always was); a rate - ``DropPath(rate)`` on
        both branches (also for the rate 0.0 of the first block, where timm puts an Identity: it is one in effect, and every branch of the
        model then follows a ``forced_drop_path`` table)."""
        super().__init__()
        self.norm1 = nn.LayerNorm(dim, eps=1e-6)
        self.attn = Attention(dim, num_heads)
        self.ls1 = LayerScale(dim, init_values) if init_values else nn.Identity()
        self.drop_path1 = nn.Identity() if drop_path is None else DropPath(drop_path)
        self.norm2 = nn.LayerNorm(dim, eps=1e-6)
        self.mlp = Mlp(dim, int(dim * mlp_ratio))
        self.ls2 = LayerScale(dim, init_values) if init_values else nn.Identity()
        self.drop_path2 = nn.Identity() if drop_path is None else DropPath(drop_path)

    def forward(self, x):
        x = x + self.drop_path1(self.ls1(self.attn(self.norm1(x))))
        return x + self.drop_path2(self.ls2(self.mlp(self.norm2(x))))


class VisionTransformer(nn.Module):
    """``global_pool='token'``, ``class_token=True``, no dist token, ``fc_norm`` identity."""

    def __init__(self, embed_dim=384, depth=12, num_heads=6, num_classes=10, img_size=224, patch_size=16,
                 in_chans=3, mlp_ratio=4.0, drop_path_rate=0.0, init_values=None):
        """init_values: LayerScale as in timm - a falsy value builds the tree without it (``ls1`` / ``ls2`` stay ``nn.Identity``: the same ``state_dict``
        keys as ever); otherwise every block gets ``LayerScale(embed_dim, init_values)`` on both branches (keys ``blocks.i.ls1.gamma``, ``blocks.i.ls2.gamma``).
        drop_path_rate: stochastic depth by timm's linear rule - block i drops each of its two branches with probability
        ``torch.linspace(0, drop_path_rate, depth)[i]``; 0 builds the tree without any ``DropPath`` module."""
        super().__init__()
        self.embed_dim = self.num_features = embed_dim
        self.num_classes, self.depth, self.num_heads = num_classes, depth, num_heads
        self.patch_embed = PatchEmbed(img_size, patch_size, in_chans, embed_dim)
        self.cls_token = nn.Parameter(torch.zeros(1, 1, embed_dim))
        self.pos_embed = nn.Parameter(torch.randn(1, self.patch_embed.num_patches + 1, embed_dim) * 0.02)
        self.pos_drop = nn.Dropout(0.0)
        self.norm_pre = nn.Identity()
        if not 0.0 <= drop_path_rate < 1.0:
            raise ValueError(f"drop_path_rate {drop_path_rate}: expected a probability in [0, 1)")
        rates = [r.item() for r in torch.linspace(0, drop_path_rate, depth)] if drop_path_rate > 0 else [None] * depth
        self.blocks = nn.Sequential(*[Block(embed_dim, num_heads, mlp_ratio, rates[i], init_values) for i in range(depth)])
        self.norm = nn.LayerNorm(embed_dim, eps=1e-6)
        self.fc_norm = nn.Identity()
        self.head_drop = nn.Dropout(0.0)
        self.head = nn.Linear(embed_dim, num_classes)
        self.init_weights()

    def init_weights(self):
        nn.init.normal_(self.cls_token, std=1e-6)
        for m in self.modules():
            if isinstance(m, nn.Linear):
                nn.init.trunc_normal_(m.weight, std=0.02)
                if m.bias is not None:
                    nn.init.zeros_(m.bias)

    def forward_features(self, x):
        x = self.patch_embed(x)
        x = torch.cat([self.cls_token.expand(x.shape[0], -1, -1), x], dim=1)
        x = self.norm_pre(self.pos_drop(x + self.pos_embed))
        return self.norm(self.blocks(x))

    def forward(self, x):
        if x.is_cuda and not torch.is_grad_enabled() and not self.training and _native_teacher_ok(self):
            # the frozen-teacher situation of the reference loop (qat_trainer.py:257-260,337-338): native forward
            from .teacher import teacher_forward

            return teacher_forward(self, x)
        x = self.forward_features(x)
        return self.head(self.head_drop(self.fc_norm(x[:, 0])))


def _native_teacher_ok(m: "VisionTransformer") -> bool:
    """Shapes the native teacher covers, and an un-prepared (float) tree."""
    return (m.embed_dim % 128 == 0 and m.embed_dim <= 768 and type(m.head) is nn.Linear and type(m.patch_embed.proj) is nn.Conv2d
            and m.blocks[0].mlp.fc1.weight.shape[0] % 128 == 0 and m.blocks[0].attn.head_dim in (32, 64) and m.patch_embed.num_patches < 224
            and x_dtype_ok(m) and not layer_scale_params(m))   # (a LayerScale teacher: the stock module forward)


def layer_scale_params(model: "VisionTransformer") -> list:
    """The 2 * depth LayerScale gammas in branch order (row 2 i = block i's ``ls1``, 2 i + 1 = its ``ls2``), [] for a tree without LayerScale; a tree
    with LayerScale on some branches only, or a foreign module in its place, is refused."""
    mods = [m for b in model.blocks for m in (b.ls1, b.ls2)]
    if all(isinstance(m, nn.Identity) for m in mods):
        return []
    if not all(type(m) is LayerScale and not m.inplace for m in mods):
        raise RuntimeError("ls1 / ls2: expected nn.Identity on every branch or qat_vit_amd.LayerScale (inplace=False) on every branch")
    return [m.gamma for m in mods]


def x_dtype_ok(m) -> bool:
    return m.cls_token.dtype == torch.float32


def _vit_of(wrapper) -> "VisionTransformer":
    m = wrapper if isinstance(wrapper, VisionTransformer) else getattr(wrapper, "model", None)
    if not isinstance(m, VisionTransformer):
        raise TypeError(f"expected a VisionTransformer or a QATWrapper around one, got {type(wrapper).__name__}")
    return m


def drop_path_branches(model: "VisionTransformer") -> list:
    """The 2 * depth branch modules in table order: row 2 i = block i's ``drop_path1`` (attention), row 2 i + 1 = its ``drop_path2`` (MLP)."""
    return [m for b in model.blocks for m in (b.drop_path1, b.drop_path2)]


def drop_path_plan(model: "VisionTransformer"):
    """None for a tree without stochastic depth (no ``DropPath`` with a rate > 0); else per branch (keep probability, multiplier of a kept
    sample) - what one draw of the whole [2 * depth, B] table needs."""
    br = drop_path_branches(model)
    if not any(isinstance(m, DropPath) and m.drop_prob > 0.0 for m in br):
        return None
    keep = [1.0 - m.drop_prob if isinstance(m, DropPath) else 1.0 for m in br]
    mult = [1.0 / k if (isinstance(m, DropPath) and m.scale_by_keep and k > 0.0) else 1.0 for m, k in zip(br, keep)]
    return keep, mult


_FORCED = weakref.WeakKeyDictionary()   # VisionTransformer -> the table of the forced_drop_path context it is in


def forced_table(model: "VisionTransformer") -> Optional[torch.Tensor]:
    """The [2 * depth, B] table of the ``forced_drop_path`` context this model is in, or None."""
    return _FORCED.get(model)


@contextlib.contextmanager
def forced_drop_path(wrapper, table: torch.Tensor):
    """Inside the context every training-mode forward of ``wrapper`` (a ``QATWrapper`` or its ``VisionTransformer``) - the stock module
    forward, the native QAT step and the native float step alike - uses ``table`` instead of drawing its drop-path masks.

    ``table``: fp32 ``[2 * depth, B]``; row ``2 i`` multiplies block ``i``'s attention branch, row ``2 i + 1`` its MLP branch, per sample.
    Any finite multipliers (a draw holds 0 and ``1 / keep``).  The model must have been built with ``drop_path_rate > 0`` (every branch then
    is a ``DropPath``).  For tests, and for a caller that owns its masks the way the augmentation records own theirs."""
    model = _vit_of(wrapper)
    br = drop_path_branches(model)
    if not all(isinstance(m, DropPath) for m in br):
        raise ValueError("forced_drop_path: the model has no DropPath modules (build it with drop_path_rate > 0)")
    if table.dim() != 2 or table.shape[0] != len(br) or table.dtype != torch.float32:
        raise ValueError(f"forced_drop_path: expected an fp32 table of shape [{len(br)}, B], got {tuple(table.shape)} {table.dtype}")
    if model in _FORCED:
        raise RuntimeError("forced_drop_path: already inside a forced_drop_path context of this model")
    _FORCED[model] = table
    for m, row in zip(br, table):
        m._forced = row
    try:
        yield table
    finally:
        del _FORCED[model]
        for m in br:
            m._forced = None


def create_vit(name: str, pretrained: bool = False, num_classes: int = 10, **kwargs) -> VisionTransformer:
    """Stands where ``timm.create_model(name, pretrained=..., num_classes=...)`` stands in the
    reference.  ``pretrained=True`` would need a download and is refused (no network)."""
    if name not in ARCH:
        raise RuntimeError(f"Unknown model ({name})")
    if pretrained:
        raise RuntimeError(f"pretrained weights for {name} are not available offline; pass checkpoint_path instead")
    d, depth, heads = ARCH[name]
    cfg = dict(embed_dim=d, depth=depth, num_heads=heads)
    cfg.update(kwargs)
    return VisionTransformer(num_classes=num_classes, **cfg)
