"""Fused gradient clipping + AdamW on MI355X (libqatvit.so: qatvit_optim_grad_norm / qatvit_optim_adamw / qatvit_optim_adamw_groups).

Stands where the reference's loop has (``/root/reference/src/training/qat_trainer.py:360-361``, optimizer built at ``:271-276``)::

    torch.nn.utils.clip_grad_norm_(ddp_model.parameters(), 1.0)
    optimizer.step()

as ``optimizer.step(max_norm=1.0)`` (or ``optimizer.clip_grad_norm_(1.0); optimizer.step()``): two launches instead of
~10 foreach passes over 152 tensors.  ``state`` / ``state_dict()`` carry torch.optim.AdamW's keys (``step``, ``exp_avg``,
``exp_avg_sq``), so checkpoints move between the two.  There is no CPU path: CPU parameters raise.

Param groups are first-class: the norm is ONE global L2 norm over every group, and the update of up to ``MAX_GROUPS`` groups with their own
``lr`` / ``betas`` / ``eps`` / ``weight_decay`` / step count is ONE launch (``qatvit_optim_adamw_groups``); an optimizer with a single group keeps
calling ``qatvit_optim_adamw``.  ``vit_param_groups`` builds the two usual ViT layouts (no weight decay on biases, norms and embeddings; layer-wise
learning-rate decay)."""

import operator
import struct

import torch

from . import native

_CHUNK = 16384  # elements per workgroup (64 KiB of fp32 per stream)
MAX_GROUPS = 64  # QATVIT_OPTIM_MAX_GROUPS (include/qatvit.h): rows of the prefactor table in qatvit_optim_adamw_groups' kernel arguments
_HYPER = operator.itemgetter("lr", "betas", "eps", "weight_decay")


class ClipAdamW(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2):
        if lr < 0 or eps < 0 or not 0 <= betas[0] < 1 or not 0 <= betas[1] < 1 or weight_decay < 0:
            raise ValueError("invalid AdamW hyper-parameters")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self._tables = None
        self._pending = None   # clip out2 of a clip_grad_norm_() not yet consumed by step()

    # ------------------------------------------------------------------ tables
    def _live_tables(self):
        """One table set for the whole optimizer: the parameters that have a gradient, in group order and then parameter order (torch skips the
        others), keyed on their addresses and group membership.  None if no parameter has a gradient.  The per-step cost is one pass over the
        parameters whatever the number of groups."""
        ps, tg, live = [], [], []
        for group in self.param_groups:
            n0 = len(ps)
            ps += [p for p in group["params"] if p.grad is not None]
            if len(ps) != n0:
                tg += [len(live)] * (len(ps) - n0)
                live.append(group)
        if not ps:
            return None
        if len(live) > MAX_GROUPS:
            raise RuntimeError(f"ClipAdamW: {len(live)} param groups with gradients; one launch updates at most {MAX_GROUPS} groups")
        dev, state, sts, ptrs = ps[0].device, self.state, [], []
        for p in ps:
            if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous():
                raise RuntimeError("ClipAdamW runs on MI355X only: parameters must be contiguous fp32 CUDA tensors")
            g = p.grad
            if g.dtype != torch.float32 or not g.is_contiguous() or g.device != dev:
                raise RuntimeError("ClipAdamW: gradients must be contiguous fp32 tensors on the one device all parameters live on")
            st = state[p]
            if not st:
                st["step"] = torch.tensor(0.0)
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            sts.append(st)
            ptrs.append((p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr()))
        key = (ptrs, tg)
        t = self._tables
        if t is None or t["key"] != key:
            i64 = lambda xs: torch.tensor(xs, dtype=torch.int64, device=dev)   # noqa: E731
            i32 = lambda xs: torch.tensor(xs, dtype=torch.int32, device=dev)   # noqa: E731
            starts, ct, ci = [tg.index(gi) for gi in range(len(live))], [], []
            for ti, p in enumerate(ps):
                n = (p.numel() + _CHUNK - 1) // _CHUNK
                ct += [ti] * n
                ci += list(range(n))
            t = dict(key=key, n=len(ct),
                     params=i64([k[0] for k in ptrs]), grads=i64([k[1] for k in ptrs]), m=i64([k[2] for k in ptrs]), v=i64([k[3] for k in ptrs]),
                     tg=i32(tg), numel=i64([p.numel() for p in ps]), ct=i32(ct), ci=i32(ci),
                     starts=starts, first=[starts[gi] for gi in tg],   # the first tensor of each group; per tensor, the first of its group
                     pack=struct.Struct("=" + "5dq" * len(live)).pack,
                     partials=torch.empty(len(ct), dtype=torch.float32, device=dev), out2=torch.empty(2, dtype=torch.float32, device=dev))
            self._tables = t
        t["live"], t["sts"] = live, sts
        return t

    def _grad_norm(self, t, max_norm):
        native.check(native.lib().qatvit_optim_grad_norm(t["grads"].data_ptr(), t["numel"].data_ptr(), t["ct"].data_ptr(), t["ci"].data_ptr(), t["n"], _CHUNK,
                                                         float(max_norm), t["partials"].data_ptr(), t["out2"].data_ptr(), native.stream_ptr()),
                     "qatvit_optim_grad_norm")
        self._pending = t["out2"]

    # ------------------------------------------------------------------ API
    @torch.no_grad()
    def clip_grad_norm_(self, max_norm: float) -> torch.Tensor:
        """Total L2 norm of all gradients of all param groups (one launch pair over one table); the clip coefficient is applied inside the next
        step() instead of re-writing the gradients."""
        t = self._live_tables()
        if t is None:
            return torch.zeros(())
        self._grad_norm(t, max_norm)
        return t["out2"][0]

    @torch.no_grad()
    def step(self, closure=None, max_norm=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        t = self._live_tables()
        if t is None:
            self._pending = None
            return loss
        steps = [st["step"] for st in t["sts"]]
        count = torch.stack(steps).tolist()
        if count != [count[i] for i in t["first"]]:
            raise RuntimeError("ClipAdamW: parameters of one group must share their step count")
        if max_norm is not None:
            self._grad_norm(t, max_norm)
        L = native.lib()
        clip = self._pending.data_ptr() if self._pending is not None else None
        if len(self.param_groups) == 1:
            group = t["live"][0]
            b1, b2 = group["betas"]
            native.check(L.qatvit_optim_adamw(t["params"].data_ptr(), t["grads"].data_ptr(), t["m"].data_ptr(), t["v"].data_ptr(), t["numel"].data_ptr(),
                                              t["ct"].data_ptr(), t["ci"].data_ptr(), t["n"], _CHUNK, float(group["lr"]), float(b1), float(b2),
                                              float(group["eps"]), float(group["weight_decay"]), int(count[0]) + 1, clip, native.stream_ptr()),
                         "qatvit_optim_adamw")
        else:   # the rows of struct qatvit_adamw_group, packed on the host; they go by value into the kernel arguments: a new lr costs no copy
            rows = []
            for (lr, (b1, b2), eps, wd), i in zip(map(_HYPER, t["live"]), t["starts"]):
                rows += (lr, b1, b2, eps, wd, int(count[i]) + 1)
            native.check(L.qatvit_optim_adamw_groups(t["params"].data_ptr(), t["grads"].data_ptr(), t["m"].data_ptr(), t["v"].data_ptr(),
                                                     t["numel"].data_ptr(), t["tg"].data_ptr(), t["ct"].data_ptr(), t["ci"].data_ptr(), t["n"], _CHUNK,
                                                     t["pack"](*rows), len(t["live"]), clip, native.stream_ptr()),
                         "qatvit_optim_adamw_groups")
        torch._foreach_add_(steps, 1)
        self._pending = None
        return loss


# ---------------------------------------------------------------------- the usual ViT param groups
def _vit_of(model):
    """(the VisionTransformer inside `model`, the prefix of its parameter names in model.named_parameters()): through DistributedDataParallel's
    ``.module`` and QATWrapper's ``.model``."""
    from .vit import VisionTransformer

    prefix, m = "", model
    while not isinstance(m, VisionTransformer):
        for attr in ("module", "model"):
            inner = getattr(m, attr, None)
            if isinstance(inner, torch.nn.Module):
                prefix, m = prefix + attr + ".", inner
                break
        else:
            raise TypeError(f"vit_param_groups: no VisionTransformer inside {type(model).__name__}")
    return m, prefix


def vit_param_groups(model, weight_decay, lr=None, layer_decay=None, no_decay_names=("cls_token", "pos_embed")):
    """Param groups for ``ClipAdamW`` / ``torch.optim.AdamW`` over a ViT student (a ``VisionTransformer``, a ``QATWrapper`` around one, float or
    prepared, or either inside DDP).

    * No weight decay (``weight_decay = 0``) for a parameter with ``ndim <= 1``, a name ending in ``.bias``, or a last name component in
      `no_decay_names`; `weight_decay` for the others.
    * ``layer_decay=d`` (needs `lr`): layer id 0 = ``cls_token``, ``pos_embed``, ``patch_embed.*``; ``i + 1`` = ``blocks.i.*``; ``depth + 1`` =
      ``norm.*``, ``head.*``; a group's ``lr`` is ``lr * d ** (depth + 1 - id)``.  At most ``2 * (depth + 2)`` groups.

    Frozen parameters are left out, every other parameter appears once, empty groups are not emitted; groups come in ascending layer id, decay before
    no-decay, parameters inside a group in ``named_parameters()`` order."""
    if layer_decay is not None and lr is None:
        raise ValueError("vit_param_groups: layer_decay needs lr (a group's lr is lr * layer_decay ** (depth + 1 - layer id))")
    vit, prefix = _vit_of(model)
    depth = len(vit.blocks)

    def layer_id(name):
        part = name.split(".")
        if part[0] in ("cls_token", "pos_embed", "patch_embed"):
            return 0
        if part[0] == "blocks":
            return int(part[1]) + 1
        if part[0] in ("norm", "head"):
            return depth + 1
        raise ValueError(f"vit_param_groups: no layer rule for parameter {name!r}")

    groups = {}
    for name, p in model.named_parameters():
        if not p.requires_grad:
            continue
        no_decay = p.ndim <= 1 or name.endswith(".bias") or name.split(".")[-1] in no_decay_names
        if layer_decay is None:
            lid = 0
        elif name.startswith(prefix):
            lid = layer_id(name[len(prefix):])
        else:
            raise ValueError(f"vit_param_groups: no layer rule for parameter {name!r} outside the VisionTransformer")
        g = groups.get((lid, no_decay))
        if g is None:
            g = groups[(lid, no_decay)] = dict(params=[], weight_decay=0.0 if no_decay else weight_decay)
            if layer_decay is not None:
                g["lr"] = lr * layer_decay ** (depth + 1 - lid)
            elif lr is not None:
                g["lr"] = lr
        g["params"].append(p)
    return [groups[k] for k in sorted(groups)]
