"""Fused gradient clipping + AdamW on MI355X (libqatvit.so: qatvit_optim_grad_norm / qatvit_optim_adamw / qatvit_optim_adamw_groups, and with a
weight EMA qatvit_optim_adamw_ema / qatvit_optim_adamw_groups_ema / qatvit_optim_ema / qatvit_optim_swap), and LAMB with per-tensor trust ratios on
the same tables (qatvit_optim_lamb_moments / qatvit_optim_lamb_apply): ``ClipAdamW`` and ``ClipLamb``.

Stands where the reference's loop has (``/root/reference/src/training/qat_trainer.py:360-361``, optimizer built at ``:271-276``)::

    torch.nn.utils.clip_grad_norm_(ddp_model.parameters(), 1.0)
    optimizer.step()

as ``optimizer.step(max_norm=1.0)`` (or ``optimizer.clip_grad_norm_(1.0); optimizer.step()``): two launches instead of
~10 foreach passes over 152 tensors.  ``state`` / ``state_dict()`` carry torch.optim.AdamW's keys (``step``, ``exp_avg``,
``exp_avg_sq``), so checkpoints move between the two.  There is no CPU path: CPU parameters raise.

Param groups are first-class: the norm is ONE global L2 norm over every group, and the update of up to ``MAX_GROUPS`` groups with their own
``lr`` / ``betas`` / ``eps`` / ``weight_decay`` / step count is ONE launch (``qatvit_optim_adamw_groups``); an optimizer with a single group keeps
calling ``qatvit_optim_adamw``.  ``vit_param_groups`` builds the two usual ViT layouts (no weight decay on biases, norms and embeddings; layer-wise
learning-rate decay).

``ema_decay=d`` keeps an exponential moving average of every updated parameter in ``state[p]["ema"]``, written by the update launch itself (the
``_ema`` entries: one more stream, no extra launch): ``e <- lerp(e, p_new, 1 - d)`` in fp32, ATen's formula (include/qatvit.h states it).  The
averaged model is evaluated by exchanging contents in place - ``with opt.ema_weights(): evaluate(...)`` - so no address changes and nothing that
reads parameters by address (the engines, ``export_int8``) has to be rebuilt; ``opt.ema_state_dict(model)`` is its checkpoint.  Only parameters are
averaged: buffers and observer ranges are the live model's, also while swapped.

``ClipLamb`` is LAMB - the optimizer of the DeiT-III-style ViT recipes - on the same footing (qatvit_optim_lamb_moments / qatvit_optim_lamb_apply behind
the same qatvit_optim_grad_norm): timm's ``Lamb`` arithmetic with that class's defaults, one trust ratio ``||p|| / ||r||`` per tensor.  The two norms of a
tensor are needed between forming the update and applying it, so the update is two launches: the first writes both moments and, per 16384-element chunk, the
partial sums of ``r^2`` and ``p^2``; the second adds up its tensor's partials (double, fixed order, no atomics), forms the ratio, forms ``r`` again from the new
moments and writes the parameters - and the weight average, from the same register.  Everything else is shared with ``ClipAdamW`` (``_ClipOptimizer``): one
table set and one clip coefficient over all param groups, the rows of up to ``MAX_GROUPS`` groups by value in the kernel arguments, ``ema_decay``,
``swap_ema`` / ``ema_weights`` / ``ema_parameters`` / ``ema_state_dict``, ``vit_param_groups`` output as is.  ``opt.trust_ratios()`` is the device tensor of the
ratios the last step used, for logging.  ``step()`` reads nothing back from the device.  State keys ``step``, ``exp_avg``, ``exp_avg_sq`` (and ``ema``)."""

import contextlib
import operator
import struct

import torch

from . import native

_CHUNK = 16384  # elements per workgroup (64 KiB of fp32 per stream)
MAX_GROUPS = 64  # QATVIT_OPTIM_MAX_GROUPS (include/qatvit.h): rows of the prefactor table in qatvit_optim_adamw_groups' kernel arguments
_HYPER = operator.itemgetter("lr", "betas", "eps", "weight_decay")


def _chunk_table(numels):
    """The (tensor, chunk) table of the multi-tensor launches over tensors of `numels` elements: one row per `_CHUNK` elements of a tensor, a tensor's
    rows contiguous and in order.  (chunk_tensor, chunk_index, first_chunk): per row its tensor and which of its chunks, per tensor its first row
    (an empty tensor has none and is never looked up: 0)."""
    ct, ci, first = [], [], []
    for ti, numel in enumerate(numels):
        n = (numel + _CHUNK - 1) // _CHUNK
        first.append(len(ct) if n else 0)
        ct += [ti] * n
        ci += list(range(n))
    return ct, ci, first


def _checked_ema_decay(decay, name="ClipAdamW"):
    if decay is None:
        return None
    decay = float(decay)
    if not 0.0 <= decay < 1.0:   # NaN fails too
        raise ValueError(f"{name}: ema_decay {decay} outside [0, 1)")
    return decay


def ema_warmup_decay(decay, updates):
    """The usual warm-up of an EMA decay: ``min(decay, (1 + updates) / (10 + updates))`` after `updates` optimizer steps, so that the average
    follows the weights closely at first.  A host helper: assign the result to ``opt.ema_decay`` before each step (it costs no copy and no sync)."""
    return min(decay, (1 + updates) / (10 + updates))


class _ClipOptimizer(torch.optim.Optimizer):
    """What ClipAdamW and ClipLamb share: the table set over the live tensors of all param groups, the global-norm launch pair, the weight EMA's
    state, its idle launch and the in-place swap, and the frame of step().  A subclass gives its name (the prefix of every message), validates its
    hyper-parameters and launches its update (``_update``)."""
    _NAME = None
    MAX_GROUPS = MAX_GROUPS   # live param groups one update launch takes

    def __init__(self, params, defaults, ema_decay):
        ema_decay = _checked_ema_decay(ema_decay, self._NAME)
        super().__init__(params, defaults)
        self._tables = None
        self._pending = None   # clip out2 of a clip_grad_norm_() not yet consumed by step()
        self._ema_decay = ema_decay   # not a param-group entry: state_dict()'s groups stay the stock optimizer's
        self._idle = []               # (p, ema) of the parameters that have an average but no gradient this step
        self._pairs = {}              # tables of the two pair launches (qatvit_optim_ema, qatvit_optim_swap)
        self._swapped = False

    @property
    def ema_decay(self):
        """None (no average is kept; the default) or the decay in [0, 1) the next step() uses."""
        return self._ema_decay

    @ema_decay.setter
    def ema_decay(self, decay):
        self._ema_decay = _checked_ema_decay(decay, self._NAME)

    @property
    def ema_swapped(self) -> bool:
        """True while the parameters hold the averages and ``state[p]["ema"]`` the live weights (between two swap_ema() calls)."""
        return self._swapped

    # ------------------------------------------------------------------ tables
    def _live_tables(self):
        """One table set for the whole optimizer: the parameters that have a gradient, in group order and then parameter order (torch skips the
        others), keyed on their addresses and group membership.  None if no parameter has a gradient.  The per-step cost is one pass over the
        parameters whatever the number of groups."""
        ps, tg, live, ema = [], [], [], self._ema_decay is not None
        self._idle = idle = []
        for group in self.param_groups:
            n0 = len(ps)
            if ema:
                for p in group["params"]:
                    if p.grad is not None:
                        ps.append(p)
                    elif self._has_ema(p):
                        idle.append((p, self.state[p]["ema"]))
            else:
                ps += [p for p in group["params"] if p.grad is not None]
            if len(ps) != n0:
                tg += [len(live)] * (len(ps) - n0)
                live.append(group)
        if not ps:
            return None
        if len(live) > MAX_GROUPS:
            raise RuntimeError(f"{self._NAME}: {len(live)} param groups with gradients; one launch updates at most {MAX_GROUPS} groups")
        dev, state, sts, ptrs = ps[0].device, self.state, [], []
        for p in ps:
            if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous():
                raise RuntimeError(f"{self._NAME} runs on MI355X only: parameters must be contiguous fp32 CUDA tensors")
            g = p.grad
            if g.dtype != torch.float32 or not g.is_contiguous() or g.device != dev:
                raise RuntimeError(f"{self._NAME}: gradients must be contiguous fp32 tensors on the one device all parameters live on")
            st = state[p]
            if not st:
                st["step"] = torch.tensor(0.0)
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            sts.append(st)
            if ema:
                if "ema" not in st:   # before the first update of p with a decay set (also after a checkpoint without averages)
                    st["ema"] = p.detach().clone(memory_format=torch.contiguous_format)
                ptrs.append((p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), st["ema"].data_ptr()))
            else:
                ptrs.append((p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr()))
        key = (ptrs, tg)
        t = self._tables
        if t is None or t["key"] != key:
            i64 = lambda xs: torch.tensor(xs, dtype=torch.int64, device=dev)   # noqa: E731
            i32 = lambda xs: torch.tensor(xs, dtype=torch.int32, device=dev)   # noqa: E731
            if ema:   # an average may come from a checkpoint: it is written through, so its extent is checked whenever an address is new
                for p, st in zip(ps, sts):
                    e = st["ema"]
                    if e.shape != p.shape or e.dtype != torch.float32 or e.device != dev or not e.is_contiguous():
                        raise RuntimeError(f"{self._NAME}: state[p]['ema'] must be a contiguous fp32 tensor of the parameter's shape on its device")
            starts, numel = [tg.index(gi) for gi in range(len(live))], [p.numel() for p in ps]
            ct, ci, first_chunk = _chunk_table(numel)
            t = dict(key=key, n=len(ct),
                     params=i64([k[0] for k in ptrs]), grads=i64([k[1] for k in ptrs]), m=i64([k[2] for k in ptrs]), v=i64([k[3] for k in ptrs]),
                     ema=i64([k[4] for k in ptrs]) if ema else None,
                     tg=i32(tg), numel=i64(numel), ct=i32(ct), ci=i32(ci),
                     starts=starts, first=[starts[gi] for gi in tg],   # the first tensor of each group; per tensor, the first of its group
                     pack=struct.Struct("=" + "5dq" * len(live)).pack,
                     partials=torch.empty(len(ct), dtype=torch.float32, device=dev), out2=torch.empty(2, dtype=torch.float32, device=dev))
            self._more_tables(t, first_chunk, dev)
            self._tables = t
        t["live"], t["sts"] = live, sts
        return t

    def _more_tables(self, t, first_chunk, dev):
        """What a subclass's update needs in the table set beyond the common entries (called when the set is rebuilt); first_chunk: per tensor, where
        its rows begin in the chunk table."""

    def _pair_tables(self, slot, pairs):
        """The tables of a launch over (a, b) tensor pairs (the stand-alone average, the swap), keyed on the addresses; None if there is no element."""
        key = [(a.data_ptr(), b.data_ptr()) for a, b in pairs]
        t = self._pairs.get(slot)
        if t is None or t["key"] != key:
            dev = pairs[0][0].device
            for a, b in pairs:
                if not (a.is_cuda and b.device == a.device and a.dtype == b.dtype == torch.float32 and a.is_contiguous() and b.is_contiguous()
                        and a.numel() == b.numel()):
                    raise RuntimeError(f"{self._NAME}: a parameter and its average must be contiguous fp32 CUDA tensors of one size on one device")
            numel = [a.numel() for a, _ in pairs]
            ct, ci, _ = _chunk_table(numel)
            t = self._pairs[slot] = dict(key=key, n=len(ct), a=torch.tensor([k[0] for k in key], dtype=torch.int64, device=dev),
                                         b=torch.tensor([k[1] for k in key], dtype=torch.int64, device=dev),
                                         numel=torch.tensor(numel, dtype=torch.int64, device=dev),
                                         ct=torch.tensor(ct, dtype=torch.int32, device=dev), ci=torch.tensor(ci, dtype=torch.int32, device=dev))
        return t if t["n"] else None

    def _average_idle(self):
        """One qatvit_optim_ema launch for the parameters that have an average but took no update this step (none, normally: nothing is launched)."""
        t = self._pair_tables("idle", self._idle) if self._idle else None
        if t is not None:
            native.check(native.lib().qatvit_optim_ema(t["a"].data_ptr(), t["b"].data_ptr(), t["numel"].data_ptr(), t["ct"].data_ptr(), t["ci"].data_ptr(),
                                                       t["n"], _CHUNK, self._ema_decay, native.stream_ptr()), "qatvit_optim_ema")

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
        self._refuse_swapped("clip_grad_norm_()")
        t = self._live_tables()
        if t is None:
            return torch.zeros(())
        self._grad_norm(t, max_norm)
        return t["out2"][0]

    @torch.no_grad()
    def step(self, closure=None, max_norm=None):
        loss = None
        self._refuse_swapped("step()")
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        t = self._live_tables()
        if t is None:
            self._pending = None
            self._average_idle()
            return loss
        steps = [st["step"] for st in t["sts"]]
        count = torch.stack(steps).tolist()
        if count != [count[i] for i in t["first"]]:
            raise RuntimeError(f"{self._NAME}: parameters of one group must share their step count")
        if max_norm is not None:
            self._grad_norm(t, max_norm)
        self._update(t, count, self._pending.data_ptr() if self._pending is not None else None)
        if t["ema"] is not None:
            self._average_idle()
        torch._foreach_add_(steps, 1)
        self._pending = None
        return loss

    def _update(self, t, count, clip):
        """The update launch(es) of one step over the table set `t`; count[i] = the step count of live tensor i before this step, clip = the address
        of the pending {norm, coefficient} pair or None."""
        raise NotImplementedError

    # ------------------------------------------------------------------ the averaged weights
    def _refuse_swapped(self, what):
        if self._swapped:
            raise RuntimeError(f"{self._NAME}: the averaged weights are swapped in (swap_ema() / ema_weights()); swap back before {what}")

    def _has_ema(self, p):
        return "ema" in self.state.get(p, ())   # .get: looking must not create the state of a parameter that has none

    def ema_parameters(self):
        """Per param group, the tensors that hold the averaged values, aligned with ``group["params"]``: ``state[p]["ema"]`` (the parameter itself
        while swapped), and the parameter itself where there is no average yet (a parameter that never had a gradient is its own average)."""
        return [[self.state[p]["ema"] if self._has_ema(p) and not self._swapped else p for p in group["params"]] for group in self.param_groups]

    @torch.no_grad()
    def swap_ema(self):
        """Exchanges the contents of every (parameter, average) pair in place, in one launch; no address changes.  ``ema_swapped`` tells which way
        round they are; while it is True, step() and clip_grad_norm_() raise."""
        pairs = [(p, self.state[p]["ema"]) for group in self.param_groups for p in group["params"] if self._has_ema(p)]
        t = self._pair_tables("swap", pairs) if pairs else None
        if t is not None:
            native.check(native.lib().qatvit_optim_swap(t["a"].data_ptr(), t["b"].data_ptr(), t["numel"].data_ptr(), t["ct"].data_ptr(), t["ci"].data_ptr(),
                                                        t["n"], _CHUNK, native.stream_ptr()), "qatvit_optim_swap")
            # the launch wrote through raw addresses: tell torch, so that what is keyed on a weight's `_version` (the native frozen-teacher forward
            # that a float model in eval() under no_grad runs through keeps fp16 / bf16 copies of the weights) sees the exchange
            torch.autograd.graph.increment_version([x for pair in pairs for x in pair])
        self._swapped = not self._swapped

    @contextlib.contextmanager
    def ema_weights(self):
        """``with opt.ema_weights():`` - the model computes with the averaged weights inside the block (evaluate, export); the live weights are
        back after it, also when the block raises.  Buffers and observer ranges are not averaged: they are the live model's throughout."""
        if self._swapped:
            raise RuntimeError(f"{self._NAME}: the averaged weights are swapped in already")
        self.swap_ema()
        try:
            yield self
        finally:
            self.swap_ema()

    def ema_state_dict(self, model):
        """``model.state_dict()`` (through DistributedDataParallel's ``.module``) with the entry of every optimised parameter replaced by a clone of
        its average: the checkpoint of the averaged model, in the format the loaders of the live model read.  Buffers are the live ones."""
        if isinstance(model, torch.nn.parallel.DistributedDataParallel):
            model = model.module
        avg = {id(p): e for group, es in zip(self.param_groups, self.ema_parameters()) for p, e in zip(group["params"], es)}
        sd = model.state_dict()
        for name, p in model.named_parameters(remove_duplicate=False):
            if name in sd and id(p) in avg:
                sd[name] = avg[id(p)].detach().clone()
        return sd

    def state_dict(self):
        self._refuse_swapped("state_dict()")   # "ema" would be saved holding the live weights
        return super().state_dict()


class ClipAdamW(_ClipOptimizer):
    _NAME = "ClipAdamW"

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, ema_decay=None):
        if lr < 0 or eps < 0 or not 0 <= betas[0] < 1 or not 0 <= betas[1] < 1 or weight_decay < 0:
            raise ValueError("invalid AdamW hyper-parameters")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay), ema_decay)

    def _update(self, t, count, clip):
        """One launch: qatvit_optim_adamw for an optimizer of one group, qatvit_optim_adamw_groups for several; with a weight EMA the `_ema` entry of the
        same name, which takes ema_ptrs after exp_avg_sq_ptrs and the decay (by value, as the prefactors) in front of clip."""
        one, ema = len(self.param_groups) == 1, t["ema"] is not None
        name = "qatvit_optim_adamw" + ("" if one else "_groups") + ("_ema" if ema else "")
        if one:
            group = t["live"][0]
            b1, b2 = group["betas"]
            hyper = (float(group["lr"]), float(b1), float(b2), float(group["eps"]), float(group["weight_decay"]), int(count[0]) + 1)
        else:   # the rows of struct qatvit_adamw_group, packed on the host; they go by value into the kernel arguments: a new lr costs no copy
            rows = []
            for (lr, (b1, b2), eps, wd), i in zip(map(_HYPER, t["live"]), t["starts"]):
                rows += (lr, b1, b2, eps, wd, int(count[i]) + 1)
            hyper = (t["pack"](*rows), len(t["live"]))
        native.check(getattr(native.lib(), name)(t["params"].data_ptr(), t["grads"].data_ptr(), t["m"].data_ptr(), t["v"].data_ptr(),
                                                 *((t["ema"].data_ptr(),) if ema else ()), t["numel"].data_ptr(), *(() if one else (t["tg"].data_ptr(),)),
                                                 t["ct"].data_ptr(), t["ci"].data_ptr(), t["n"], _CHUNK, *hyper, *((self._ema_decay,) if ema else ()), clip,
                                                 native.stream_ptr()), name)


_LAMB_FLAGS = operator.itemgetter("grad_averaging", "always_adapt", "trust_clip")


class ClipLamb(_ClipOptimizer):
    """LAMB with per-tensor trust ratios (timm's ``Lamb`` with that class's defaults; include/qatvit.h states the arithmetic), with ClipAdamW's surface:
    ``step(max_norm=...)`` / ``clip_grad_norm_`` apply ONE global clip coefficient inside the update, all param groups go through the same launches,
    ``ema_decay`` keeps the weight average inside the apply launch, ``ema_weights()`` swaps it in place.  A step is the norm launch pair (with a
    ``max_norm``), ``qatvit_optim_lamb_moments`` and ``qatvit_optim_lamb_apply``; nothing is read back from the device.

    Differences from timm: the clip coefficient is ``min(1, max_norm / (total + 1e-6))`` (ClipAdamW's, torch's ``clip_grad_norm_``) rather than a
    division by ``max(total / max_norm, 1)``, and it is asked for per step instead of through a ``max_grad_norm`` group entry; a fused GradScaler
    unscale is not part of it (``scaler.step(opt)`` goes through the stock path).  State keys: ``step``, ``exp_avg``, ``exp_avg_sq`` (and ``ema``)."""
    _NAME = "ClipLamb"

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01, grad_averaging=True, always_adapt=False, trust_clip=False,
                 ema_decay=None):
        if lr < 0 or eps < 0 or not 0 <= betas[0] < 1 or not 0 <= betas[1] < 1 or weight_decay < 0:
            raise ValueError("invalid LAMB hyper-parameters")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, grad_averaging=bool(grad_averaging),
                                      always_adapt=bool(always_adapt), trust_clip=bool(trust_clip)), ema_decay)
        self._trust = None

    def _more_tables(self, t, first_chunk, dev):
        t["first_chunk"] = torch.tensor(first_chunk, dtype=torch.int32, device=dev)
        t["partials2"] = torch.empty(2 * t["n"], dtype=torch.float32, device=dev)
        t["trust"] = torch.ones(len(first_chunk), dtype=torch.float32, device=dev)
        t["pack"] = struct.Struct("=" + "5dq4i" * len(t["starts"])).pack   # rows of struct qatvit_lamb_group

    def _update(self, t, count, clip):
        L, st = native.lib(), native.stream_ptr()
        rows = []
        for group, i in zip(t["live"], t["starts"]):
            lr, (b1, b2), eps, wd = _HYPER(group)
            rows += (lr, b1, b2, eps, wd, int(count[i]) + 1, *map(int, _LAMB_FLAGS(group)), 0)
        rows = t["pack"](*rows)   # by value into the kernel arguments of both launches: a scheduled lr costs no copy
        native.check(L.qatvit_optim_lamb_moments(t["params"].data_ptr(), t["grads"].data_ptr(), t["m"].data_ptr(), t["v"].data_ptr(), t["numel"].data_ptr(),
                                                 t["tg"].data_ptr(), t["ct"].data_ptr(), t["ci"].data_ptr(), t["n"], _CHUNK, rows, len(t["live"]), clip,
                                                 t["partials2"].data_ptr(), st), "qatvit_optim_lamb_moments")
        ema = t["ema"] is not None
        native.check(L.qatvit_optim_lamb_apply(t["params"].data_ptr(), t["m"].data_ptr(), t["v"].data_ptr(), t["ema"].data_ptr() if ema else None,
                                               t["numel"].data_ptr(), t["tg"].data_ptr(), t["first_chunk"].data_ptr(), t["ct"].data_ptr(),
                                               t["ci"].data_ptr(), t["n"], _CHUNK, rows, len(t["live"]), self._ema_decay if ema else 0.0,
                                               t["partials2"].data_ptr(), t["trust"].data_ptr(), st), "qatvit_optim_lamb_apply")
        self._trust = t["trust"]

    def trust_ratios(self):
        """The trust ratio each tensor was updated with in the last step: a device fp32 tensor with one entry per tensor that had a gradient, in
        group order and then parameter order (exactly 1 where the group neither decays nor always adapts, or a norm was zero).  For logging: it is
        the buffer the step wrote, returned without a synchronisation - clone it to keep it past the next step.  None before the first step."""
        return self._trust


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
