"""Host side of the native student step: binds a prepare_qat()-ed QATWrapper(ViT) to
``qatvit_student_forward`` / ``qatvit_student_backward`` (include/qatvit.h).

torch is plumbing here: it owns the parameters, the fake-quant buffers (re-homed into one flat
arena so that the data-parallel buffer broadcast is one collective), the workspace and the
streams.  All arithmetic of the step runs in libqatvit.so.

Call order mirrored from the reference loop (/root/reference/src/training/qat_trainer.py:337-361):
``out = model(images)`` -> loss -> ``loss.backward()``; with ``torch.distributed`` initialised and
``enable_data_parallel()`` called, backward issues the bucketed gradient all-reduce (RCCL) while
earlier layers are still being differentiated, and forward starts with the rank-0 broadcast of the
fake-quant state (what DDP does for the reference, torch/nn/parallel/distributed.py:1554-1559).

The batch size is a run-time argument: the workspace is sized for the largest batch seen so far and a
smaller batch (the last partial batch of an epoch, the evaluation loader - the reference's loaders have
no ``drop_last``, qat_trainer.py:228-254) runs inside it without any allocation or collective.
"""
from __future__ import annotations

import ctypes
import os
import time
import warnings
import weakref
from typing import Callable, Dict, List, NamedTuple, Optional, Sequence, Tuple

import torch
import torch.distributed as dist
from torch.ao.quantization.fake_quantize import FusedMovingAvgObsFakeQuantize

from . import float_engine, native

STAGE_INJECT = 1  # QATVIT_STAGE_INJECT
FWD_X16 = 2       # QATVIT_FWD_X16
BWD_DY16 = 2      # QATVIT_BWD_DY16
BWD_CALIBRATE = 4  # QATVIT_BWD_CALIBRATE


def dy16_default() -> bool:
    """QATVIT_DY16=0 keeps every backward in the bf16 (hi, lo) pair form (round 3's arithmetic); default: the one-plane form where the
    configuration allows it (include/qatvit.h, QATVIT_BWD_DY16)."""
    return os.environ.get("QATVIT_DY16", "1") != "0"


# ---------------------------------------------------------------------------------------------------------------------
# Data-parallel schedule: pure host logic (no native library, no GPU) so that the 2-rank gloo test on CPU drives exactly
# the code the engine runs over RCCL.

class FlatGradLayout:
    """Where each parameter's gradient lives inside ONE flat fp32 buffer laid out in backward-stage order
    (stage 0 = final norm + head, stages 1..depth = blocks depth-1..0, stage depth+1 = embedding), so that the
    gradients finished by a prefix of the stages are a contiguous slice - the unit of the bucketed all-reduce.

    ``numels``: parameter sizes in the C-ABI order of include/qatvit.h (4 embedding tensors, 12 per block, 4 tail), optionally followed by the
    2 * depth LayerScale gammas (block i's ``ls1`` / ``ls2`` at 8 + 12 * depth + 2 i, + 1): they lie at the end of block i's stage, so the bucketed
    all-reduce carries them with that block.  Without them the layout is what it always was."""

    ALIGN = 64  # elements: every tensor starts on a 256-byte boundary

    def __init__(self, numels: Sequence[int], depth: int):
        n_par = 8 + 12 * depth
        if len(numels) not in (n_par, n_par + 2 * depth):
            raise ValueError(f"expected {n_par} parameters for depth {depth} (or {n_par + 2 * depth} with LayerScale), got {len(numels)}")
        ls = 2 if len(numels) > n_par else 0
        order = [n_par - 4 + k for k in range(4)]                       # stage 0: norm, head
        for i in reversed(range(depth)):
            order += [4 + 12 * i + k for k in range(12)] + [n_par + 2 * i + k for k in range(ls)]   # stages 1..depth
        order += [0, 1, 2, 3]                                           # stage depth+1: embedding
        stage_of_slot = [0] * 4 + sum(([s] * (12 + ls) for s in range(1, depth + 1)), []) + [depth + 1] * 4
        self.order = order
        self.offset: Dict[int, int] = {}
        self.stage_end: List[int] = [0] * (depth + 2)
        n = 0
        for slot, pi in enumerate(order):
            self.offset[pi] = n
            n += (numels[pi] + self.ALIGN - 1) // self.ALIGN * self.ALIGN
            self.stage_end[stage_of_slot[slot]] = n
        self.numel = n
        self.numels = list(numels)
        self.last_stage = depth + 1

    def views(self, flat: torch.Tensor, shapes: Sequence[torch.Size]) -> List[torch.Tensor]:
        return [flat[self.offset[pi]:self.offset[pi] + self.numels[pi]].view(shapes[pi]) for pi in range(len(self.numels))]

    def buckets(self, bucket_bytes: int) -> List[Tuple[int, int, int, int]]:
        """[(stage_from, stage_to, elem_start, elem_end)]: a bucket closes once it holds >= bucket_bytes of gradients
        (or at the last stage).  Multi-MB buckets: xGMI is point-to-point, a few large transfers keep every link busy."""
        out, start, s0 = [], 0, 0
        for s in range(self.last_stage + 1):
            end = self.stage_end[s]
            if (end - start) * 4 >= bucket_bytes or s == self.last_stage:
                out.append((s0, s, start, end))
                start, s0 = end, s + 1
        return out


def mean_op(pg):
    """(reduce op, divisor or None) of an average over the group: AVG on nccl; gloo has no AVG: SUM, then divide by the group size."""
    if dist.get_backend(pg) == "nccl":
        return dist.ReduceOp.AVG, None
    return dist.ReduceOp.SUM, dist.get_world_size(pg)


def allreduce_mean(tensor: torch.Tensor, pg) -> None:
    op, div = mean_op(pg)
    dist.all_reduce(tensor, op=op, group=pg)
    if div:
        tensor.div_(div)


def staged_backward_allreduce(flat: torch.Tensor, layout: FlatGradLayout, bucket_bytes: int, pg,
                              run_stages: Callable[[int, int], None], exposed: Optional[list] = None) -> None:
    """Run the backward stage by stage; as soon as a bucket's stages have been enqueued, start its all-reduce
    (async: RCCL / gloo run it on their own stream / thread) and go on differentiating earlier layers.  Returns
    with every slice averaged over the group (the caller's stream waits on the collectives).

    Replaces the Reducer of ``DDP(prepared)`` (qat_trainer.py:311; bucketing of torch/nn/parallel/distributed.py:828-834)."""
    op, div = mean_op(pg)
    works = []
    for s0, s1, a, b in layout.buckets(bucket_bytes):
        run_stages(s0, s1)
        seg = flat[a:b]
        works.append((dist.all_reduce(seg, op=op, group=pg, async_op=True), seg))
    ev = None
    if exposed is not None and flat.is_cuda:   # (bench.py) the stream time between the last backward kernel and the join of the last collective
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        ev[0].record()
    for w, seg in works:
        w.wait()
        if div:
            seg.div_(div)
    if ev is not None:
        ev[1].record()
        exposed.append(ev)


# ---------------------------------------------------------------------------------------------------------------------
# Fake-quant mode: pure host logic (no native library, no GPU) so that a CPU test drives the decision the engine takes.
# torch.ao.quantization.disable_fake_quant / enable_fake_quant write `fake_quant_enabled` in place, which bumps the tensor's `_version`: comparing the
# versions is a host-only check; the flags themselves are read (one device-to-host copy) only when a version moved.

QAT = "qat"            # fake-quant on everywhere: the quantised step (qatvit_student_*)
OBSERVE = "observe"    # fake-quant off everywhere: the float step + the observer updates (qatvit_float_student_forward_observe)


class FqModeState:
    """What the last decision saw: the `_version` of every `fake_quant_enabled` tensor and the mode chosen from them.  `reads` counts the host
    reads of the flags."""

    def __init__(self):
        self.versions: Optional[Tuple[int, ...]] = None
        self.mode: Optional[str] = None
        self.reads = 0


def fq_versions(flags: Sequence[torch.Tensor]) -> Tuple[int, ...]:
    return tuple(t._version for t in flags)


def decide_fq_mode(state: FqModeState, flags: Sequence[torch.Tensor], names: Sequence[str]) -> str:
    """flags: the modules' `fake_quant_enabled` tensors (fq_flags_and_names).  QAT when every one is 1, OBSERVE when every one is 0; a mix raises
    (before the caller launches anything) and leaves `state` as it was.  Unchanged versions since the last decision: its mode, without reading a
    flag (about 15 us of host time for ViT-S)."""
    versions = fq_versions(flags)
    if versions == state.versions:
        return state.mode
    on = (torch.stack([t.reshape(-1)[0] for t in flags]) != 0).tolist()   # the one host read
    state.reads += 1
    if all(on):
        mode = QAT
    elif not any(on):
        mode = OBSERVE
    else:
        def some(xs):
            return ", ".join(xs[:8]) + (f" (+{len(xs) - 8} more)" if len(xs) > 8 else "")
        en = [n for n, o in zip(names, on) if o]
        dis = [n for n, o in zip(names, on) if not o]
        raise RuntimeError(
            f"qat-vit_amd: fake-quant is enabled on {len(en)} modules ({some(en)}) and disabled on {len(dis)} ({some(dis)}); the native step supports "
            "fake_quant_enabled = 1 everywhere (QAT) or 0 everywhere (observe-only) - apply torch.ao.quantization.enable_fake_quant / disable_fake_quant "
            "to the whole model")
    state.versions, state.mode = versions, mode
    return mode


def fq_modules_and_names(wrapper: torch.nn.Module):
    """The 126 (ViT-S) fake-quant modules of a prepared QATWrapper(ViT), activation order then weight order (include/qatvit.h), and their
    qualified names in the wrapper."""
    _, act, wfq = collect_student(wrapper)
    names = {id(m): n for n, m in wrapper.named_modules()}
    fqs = list(act) + list(wfq)
    return fqs, [names.get(id(f), type(f).__name__) for f in fqs]


def fq_flags_and_names(wrapper: torch.nn.Module):
    """The `fake_quant_enabled` tensors of fq_modules_and_names (disable_fake_quant / enable_fake_quant write them in place) and the names."""
    fqs, names = fq_modules_and_names(wrapper)
    return [f.fake_quant_enabled for f in fqs], names


# ---------------------------------------------------------------------------------------------------------------------

def _fq_of(mod, attr):
    fq = getattr(mod, attr, None)
    if not isinstance(fq, FusedMovingAvgObsFakeQuantize):
        raise RuntimeError(
            f"{type(mod).__name__}.{attr} is {type(fq).__name__}: the native path implements the fused moving-average "
            "fake-quant that get_default_qat_qconfig('qnnpack'|'x86'|'fbgemm') installs"
        )
    return fq


def collect_student(wrapper: torch.nn.Module):
    """(parameters, activation fake-quant modules, weight fake-quant modules) of a prepared QATWrapper(ViT), each in
    the order include/qatvit.h documents.  Pure module-tree walking: works on any device."""
    m = wrapper.model
    blocks = list(m.blocks)
    pe = m.patch_embed.proj
    ps = native.vit_params(m)
    act = [_fq_of(wrapper.quant, "activation_post_process"), _fq_of(pe, "activation_post_process")]
    wfq = [_fq_of(pe, "weight_fake_quant")]
    for b in blocks:
        act += [_fq_of(x, "activation_post_process") for x in (b.norm1, b.attn.qkv, b.attn.proj, b.norm2, b.mlp.fc1, b.mlp.fc2)]
        wfq += [_fq_of(x, "weight_fake_quant") for x in (b.attn.qkv, b.attn.proj, b.mlp.fc1, b.mlp.fc2)]
    act += [_fq_of(m.norm, "activation_post_process"), _fq_of(m.head, "activation_post_process")]
    wfq += [_fq_of(m.head, "weight_fake_quant")]
    return ps, act, wfq


def weight_param_indices(n_params: int) -> List[int]:
    """Index (in the parameter order above) of the weight tensor behind each weight fake-quant module."""
    depth = (n_params - 8) // 12
    idx = [0]
    for i in range(depth):
        idx += [4 + 12 * i + 2, 4 + 12 * i + 4, 4 + 12 * i + 8, 4 + 12 * i + 10]
    return idx + [n_params - 2]


def rehome_fq_state(params, act_fq, w_fq, device):
    """Move min/max/scale (fp32) and zero_point (int32) of all fake-quant modules into ONE flat byte arena; the module
    buffers become views (state_dict() is unchanged), so the data-parallel state broadcast is a single collective.
    Per-channel state gets its [C] shape here, as the fused op would do on its first call.
    Returns (f32 view, i32 view, arena, total channels).  Replaces the per-buffer broadcast of DDP._sync_buffers
    (torch/nn/parallel/distributed.py:2178-2221) for the reference's ``DDP(prepared)`` (qat_trainer.py:311)."""
    sizes = []
    for f, w in [(f, None) for f in act_fq] + list(zip(w_fq, [params[i] for i in weight_param_indices(len(params))])):
        sizes.append(w.shape[0] if (w is not None and f.is_per_channel) else 1)
    tot = sum(sizes)
    arena = torch.empty(16 * tot, dtype=torch.uint8, device=device)
    f32 = arena[:12 * tot].view(torch.float32)
    i32 = arena[12 * tot:].view(torch.int32)
    o = 0
    for f, c in zip(list(act_fq) + list(w_fq), sizes):
        obs = f.activation_post_process
        per_ch = f.is_per_channel
        mn, mx, sc, zp = f32[o:o + c], f32[tot + o:tot + o + c], f32[2 * tot + o:2 * tot + o + c], i32[o:o + c]
        if obs.min_val.numel() == c:
            mn.copy_(obs.min_val.reshape(-1)); mx.copy_(obs.max_val.reshape(-1))
        else:
            mn.fill_(float("inf")); mx.fill_(float("-inf"))
        if f.scale.numel() == c:
            sc.copy_(f.scale.reshape(-1)); zp.copy_(f.zero_point.reshape(-1))
        else:
            sc.fill_(1.0); zp.fill_(0)
        obs._buffers["min_val"] = mn if per_ch else mn.view(())
        obs._buffers["max_val"] = mx if per_ch else mx.view(())
        f._buffers["scale"] = sc
        f._buffers["zero_point"] = zp
        o += c
    return f32, i32, arena, tot


@torch.no_grad()
def broadcast_fq_state(arena: torch.Tensor, pg) -> None:
    """Rank 0's fake-quant state becomes every rank's: ONE collective for all 126 modules."""
    dist.broadcast(arena, src=0, group=pg)


# ---------------------------------------------------------------------------------------------------------------------
# The overflow protocol of the one-plane backward (include/qatvit.h, QATVIT_BWD_DY16): did the backward just issued meet a gradient that did not fit
# its fp16 plane, and does the data-parallel group agree?  mirror_wait and store_agree are pure host logic (no native library, no GPU).

def mirror_wait(mirror, want: int, limit: float = 10.0) -> Optional[bool]:
    """mirror: int32 {flag, generation}.  Wait until the device has written generation `want` (mod 2^32) or a later one, then the flag; None if it
    does not show up within `limit` seconds (the caller synchronises instead)."""
    want, t0 = want & 0xffffffff, time.perf_counter()
    while ((int(mirror[1]) - want) & 0xffffffff) >= 0x80000000:      # generation still behind the one this call writes
        if time.perf_counter() - t0 > limit:
            return None
        time.sleep(0)
    return bool(int(mirror[0]))


def store_agree(st, k: int, rank: int, world: int, local: bool) -> bool:
    """MAX over the group's ranks of the local overflow flags, through a key-value store (host only; every rank calls it once per round k)."""
    if local:
        st.add(f"o{k}", 1)
    n = st.add(f"a{k}", 1)                    # (after this rank's overflow count: once all have arrived every count is in)
    t0 = time.perf_counter()
    while n < world:
        if time.perf_counter() - t0 > 60.0:
            raise RuntimeError("one-plane backward: a rank of the data-parallel group did not report its overflow flag within 60 s")
        time.sleep(0)
        n = st.add(f"a{k}", 0)
    over = st.add(f"o{k}", 0) > 0
    if k >= 2 and rank == 0:                  # round k - 2 is behind every rank (each passed round k - 1 to get here)
        for key in (f"a{k - 2}", f"o{k - 2}"):
            try:
                st.delete_key(key)
            except Exception:  # noqa: BLE001
                pass
    return over


class OverflowProtocol:
    """One per StudentEngine.  `calibrated`: the workspace holds a scale history (a fresh one starts with one calibrating, pair-form, step);
    `fallbacks`: backward passes repeated in the pair form after an overflow."""

    def __init__(self):
        self.calibrated, self.fallbacks = False, 0
        self.flag = None                         # int32 view of the overflow word in the workspace
        # host mirror of the flag (qatvit_student_dy16_set_mirror): pinned int32 {flag, generation} the backward writes before its deferred weight
        # gradients; polled instead of synchronising with the stream.  QATVIT_DY16_MIRROR=0: the stream synchronisation.
        self.mirror = self.mirror_np = None
        self.mirror_on = os.environ.get("QATVIT_DY16_MIRROR", "1") != "0"
        self.gen = 0                             # backward calls issued since the mirror was installed: the generation the device will have written after them
        self.pg, self.store, self.round, self.epoch = None, None, 0, 0   # (data-parallel: setup_agreement)

    def attach(self, workspace: torch.Tensor, cfg: native.Cfg, mirror: bool) -> None:
        """A fresh workspace: its flag word, no scale history yet and, if asked for (the one-plane form is on), a mirror installed in it."""
        L, cp = native.lib(), ctypes.byref(cfg)
        off = L.qatvit_student_tensor_offset(cp, b"dy16", 0)
        self.flag = workspace[off + 8:off + 12].view(torch.int32)   # header word 2: overflow
        self.calibrated, self.gen = False, 0
        if not (self.mirror_on and mirror):
            return
        try:
            m = torch.zeros(2, dtype=torch.int32).pin_memory()
        except RuntimeError:
            return
        if L.qatvit_student_dy16_set_mirror(cp, workspace.data_ptr(), m.data_ptr(), native.stream_ptr()) == 0:
            self.mirror, self.mirror_np = m, m.numpy()   # (non-zero: not device-addressable here, the stream synchronisation stays)

    def detach(self) -> None:
        """Before the workspace is released: nothing here may keep its storage alive, and no kernel may still hold the mirror's address."""
        self.flag = None
        if self.mirror is not None:
            torch.cuda.current_stream().synchronize()
            self.mirror = self.mirror_np = None

    def issued(self) -> None:   # a backward call with BWD_DY16 or BWD_CALIBRATE was enqueued (a captured one counts when replayed): it ends with k_dy16_end, one generation
        self.gen += 1

    def setup_agreement(self, pg, device) -> None:
        """The ranks must agree on the overflow flag of a one-plane backward (all repeat it, with its collectives, or none does).  A one-element MAX
        all-reduce on the stream is known only when the whole backward is over - the host would come back to an idle GPU (0.6 ms per step).  With the
        pinned mirror every rank knows its own flag 2 - 3 ms earlier; they agree through the c10d key-value store the group was set up with (two
        counters per step: arrivals, overflows) while the GPUs still run the weight gradients.  QATVIT_DY16_STORE_AGREE=0 (or a store that is not
        reachable): the all-reduce."""
        self.pg, self.store, self.round = pg, None, 0
        ranks = dist.get_process_group_ranks(pg)
        self.epoch += 1                                                     # (a second setup on this object must not meet the first one's counters)
        tag = torch.tensor([id(self) & 0x7fffffff, self.epoch], dtype=torch.int64, device=device)
        dist.broadcast(tag, src=ranks[0], group=pg)                         # one name for this engine's keys on every rank
        if os.environ.get("QATVIT_DY16_STORE_AGREE", "1") != "0":
            try:
                from torch.distributed.distributed_c10d import _get_default_store
                self.store = dist.PrefixStore(f"qatvit_dy16/{int(tag[0].item())}.{int(tag[1].item())}/{'-'.join(map(str, ranks))}", _get_default_store())
                self.store.add("probe", 0)
            except Exception:  # noqa: BLE001
                self.store = None
        can = torch.tensor([1 if self.store is not None else 0], dtype=torch.int32, device=device)
        dist.all_reduce(can, op=dist.ReduceOp.MIN, group=pg)            # the store path on every rank or on none
        if int(can.item()) == 0:
            self.store = None

    def overflowed(self) -> bool:
        """Did the last one-plane backward meet a gradient that did not fit its fp16 plane?  Blocks on the stream; in a data-parallel group the
        answer is agreed on (MAX over the ranks) so that every rank repeats the backward, and its collectives, or none does."""
        flag = self.flag
        if self.pg is not None:
            flag = flag.clone()
            dist.all_reduce(flag, op=dist.ReduceOp.MAX, group=self.pg)
        over = bool(flag.item())
        if self.mirror_np is not None:           # the stream is drained: whatever wrote generations without this object counting is accounted for
            self.gen = int(self.mirror_np[1]) & 0xffffffff
        return over

    def resolve(self, replayed: bool = False) -> bool:
        """Did the one-plane backward just issued overflow, anywhere in the group?  Every rank calls it once per such backward (all repeat the backward,
        with its collectives, or none does).  replayed: a hipGraph replay issued it, so the host has not counted its generation yet."""
        if replayed:
            self.gen += 1
        over = None
        if self.pg is None or self.store is not None:   # (the store: agreed on by the whole group in setup_agreement, every rank comes here or none)
            # the flag as soon as the device knows it: the deferred weight gradients are still running, the host goes on
            over = mirror_wait(self.mirror_np, self.gen) if self.mirror_np is not None else None
            if self.pg is not None:
                self.round += 1
                over = store_agree(self.store, self.round - 1, dist.get_rank(self.pg), dist.get_world_size(self.pg),
                                   bool(self.flag.item()) if over is None else over)
        return self.overflowed() if over is None else over


class Step(NamedTuple):
    """What a forward was: it travels with the step (autograd's ctx, a captured hipGraph) to the backward of exactly that forward."""
    cfg: native.Cfg
    generation: int        # the engine's count of forwards: the workspace holds the activations of exactly one
    x16: bool              # the forward wrote h1q / h2q as fp16 integers: its backward is the one-plane form
    fq_mode: Optional[str]
    ln_in_strip: int       # which of its LayerNorms ran inside the statistics pass that follows them (bit 0: norm1 / qkv, bit 1: norm2 / fc1; QATVIT_LN_STRIP)


class StudentEngine:
    """One per prepared wrapper (created lazily at the first CUDA forward)."""

    def __init__(self, wrapper: torch.nn.Module, batch: int):
        m = wrapper.model
        dev = m.cls_token.device
        if dev.type != "cuda":
            raise RuntimeError("StudentEngine needs the model on an MI355X (cuda) device")
        self.device = dev
        self.lib = native.lib()
        blocks = list(m.blocks)
        ps, act, wfq = collect_student(wrapper)
        # LayerScale: the 2 * depth gammas stand BEHIND the parameters of the C ABI (every existing index keeps its meaning); the library learns their
        # addresses through qatvit_student_set_layer_scale
        self.n_abi = len(ps)
        self.ls = native.LayerScaleBinding(m, dev)
        ps = ps + self.ls.gammas
        for p in ps:
            if p is None or p.dtype != torch.float32 or not p.is_contiguous():
                raise RuntimeError("every student parameter must be a contiguous fp32 tensor (bias=True everywhere)")
        self.params: List[torch.nn.Parameter] = ps
        self.act_fq, self.w_fq = act, wfq
        a0, w0 = act[0], wfq[0]
        for f in act:
            if f.is_per_channel or f.is_symmetric_quant or (f.activation_post_process.quant_min, f.activation_post_process.quant_max) != (
                    a0.activation_post_process.quant_min, a0.activation_post_process.quant_max):
                raise RuntimeError("activation fake-quant must be per-tensor affine with one common range")
        for f in wfq:
            if not f.is_symmetric_quant or f.is_per_channel != w0.is_per_channel or (f.is_per_channel and f.ch_axis != 0):
                raise RuntimeError("weight fake-quant must be symmetric, all per-tensor or all per-channel (axis 0)")
        # Observers may be on or off - the kernels read `observer_enabled` on the device every step, so torch.ao.quantization.disable_observer /
        # enable_observer work at any time.  Fake-quant is on everywhere (the quantised step: the GEMM operands ARE the quantisation grids) or off
        # everywhere (the observe-only step); every forward decides which (decide_mode)
        self._fq_flags, self._fq_names = fq_flags_and_names(wrapper)
        self._fq_state = FqModeState()
        # observe-only resources, allocated by the first observe-only forward beside the QAT workspace (which keeps the dy16 scale history and the
        # addresses a captured hipGraph is bound to)
        self.float_form = float_engine.Form(*float_engine.FP32)
        self.observe_buf: Optional[torch.Tensor] = None
        hd = blocks[0].attn.head_dim
        self._cfg_kw = dict(
            native.vit_shape(m), act_qmin=a0.activation_post_process.quant_min, act_qmax=a0.activation_post_process.quant_max,
            w_qmin=w0.activation_post_process.quant_min, w_qmax=w0.activation_post_process.quant_max, w_per_channel=int(w0.is_per_channel),
            averaging_const=float(a0.activation_post_process.averaging_constant),
        )
        self._cfgs: Dict[int, native.Cfg] = {}
        self.last_step = Step(self.cfg_for(batch), 0, False, None, 0)   # the record of the most recent forward (before the first: the bound batch)
        if hd * self.cfg.num_heads != self.cfg.embed_dim:
            raise RuntimeError("embed_dim must equal num_heads * head_dim")
        L, cp = self.lib, ctypes.byref(self.cfg)
        assert L.qatvit_student_num_params(cp) == self.n_abi and L.qatvit_student_num_act_fq(cp) == len(act) and L.qatvit_student_num_weight_fq(cp) == len(wfq)
        self._rehome_fq_state()
        self.capacity = 0
        self.workspace: Optional[torch.Tensor] = None
        self._pins = 0                           # live captured hipGraphs: the workspace address must not change under them
        # the one-plane backward (include/qatvit.h, QATVIT_BWD_DY16): on when the configuration allows it; the scale history lives in the
        # workspace, so a fresh workspace starts with one calibrating (pair-form) step
        self.dy16 = dy16_default() and bool(self.lib.qatvit_student_dy16_supported(ctypes.byref(self.cfg)))
        self.overflow = OverflowProtocol()
        self.dy16_overflowed = self.overflow.overflowed
        # stochastic depth: the per-sample multipliers of a training-mode step (the QAT step's and the observe-only step's alike)
        self.drop = native.DropPathTable(m, dev)
        self._reserve(batch)
        # ---- flat gradient buffer, laid out in backward-stage order so that finished buckets are contiguous
        self.layout = FlatGradLayout([p.numel() for p in ps], self.cfg.depth)
        self.grad_numel = self.layout.numel
        self._ptr_params = (ctypes.c_void_p * len(ps))(*[p.data_ptr() for p in ps])
        self._param_ptrs_key = tuple(p.data_ptr() for p in ps)
        self.pg = None
        self.bucket_bytes = 16 << 20
        self.exposed_events: Optional[list] = None   # bench.py sets a list: (start, end) event pairs of the exposed collective time, one per backward
        self._build_fq_structs()

    # ------------------------------------------------------------------ configuration / workspace
    # the most recent forward, field by field, and the protocol's counter, store and mirror, by the names callers and tests read
    cfg = property(lambda self: self.last_step.cfg)
    generation = property(lambda self: self.last_step.generation)
    _fwd_x16 = property(lambda self: self.last_step.x16)
    fq_mode = property(lambda self: self.last_step.fq_mode)
    ln_in_strip = property(lambda self: self.last_step.ln_in_strip)
    dy16_fallbacks = property(lambda self: self.overflow.fallbacks)
    _agree_store = property(lambda self: self.overflow.store)
    _mirror_np = property(lambda self: self.overflow.mirror_np)

    def cfg_for(self, batch: int) -> native.Cfg:
        c = self._cfgs.get(batch)
        if c is None:
            c = self._cfgs[batch] = native.Cfg(batch=batch, **self._cfg_kw)
        return c

    @property
    def frozen(self) -> bool:
        return self._pins > 0

    def pin(self) -> None:
        self._pins += 1

    def unpin(self) -> None:
        self._pins = max(0, self._pins - 1)

    def _reserve(self, batch: int) -> None:
        """Make the workspace large enough for `batch` images.  Offsets inside it depend on the batch of the call, the
        observer accumulators at its start do not, so a smaller batch simply runs in the front part of the same buffer."""
        if batch <= self.capacity:
            return
        if self.frozen:
            raise RuntimeError(f"batch {batch} exceeds the workspace ({self.capacity}) a captured hipGraph is bound to")
        c = self.cfg_for(batch)
        L, cp = self.lib, ctypes.byref(c)
        nbytes = L.qatvit_student_workspace_bytes(cp)
        if nbytes <= 0:
            raise RuntimeError("qatvit_student_workspace_bytes: " + L.qatvit_last_error().decode())
        self.overflow.detach()
        self.workspace = None                    # release the smaller one first
        self.workspace = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        native.check(L.qatvit_student_init(cp, self.workspace.data_ptr(), native.stream_ptr()), "qatvit_student_init")
        self.capacity = batch
        self.overflow.attach(self.workspace, c, self.dy16)

    # ------------------------------------------------------------------ FQ state arena
    def _rehome_fq_state(self):
        self.fq_f32, self.fq_i32, self.fq_arena, self.fq_total = rehome_fq_state(self.params[:self.n_abi], self.act_fq, self.w_fq, self.device)

    def _build_fq_structs(self):
        def arr(fqs):
            a = (native.FQ * len(fqs))()
            for s, f in zip(a, fqs):
                obs = f.activation_post_process
                s.min_val, s.max_val, s.scale, s.zero_point = obs.min_val.data_ptr(), obs.max_val.data_ptr(), f.scale.data_ptr(), f.zero_point.data_ptr()
                s.observer_on, s.fake_quant_on = f.observer_enabled.data_ptr(), f.fake_quant_enabled.data_ptr()
            return a
        self._act_structs, self._w_structs = arr(self.act_fq), arr(self.w_fq)

    # ------------------------------------------------------------------ data parallel
    def enable_data_parallel(self, process_group=None, bucket_bytes: int = 16 << 20):
        if not dist.is_initialized():
            raise RuntimeError("torch.distributed is not initialised")
        self.pg = process_group if process_group is not None else dist.group.WORLD
        self.bucket_bytes = bucket_bytes
        for p in self.params:  # replicas start identical (DDP's constructor broadcast)
            dist.broadcast(p.data, src=0, group=self.pg)
        self.overflow.setup_agreement(self.pg, self.device)

    # ------------------------------------------------------------------ step
    def _check_ptrs(self):
        if tuple(p.data_ptr() for p in self.params) != self._param_ptrs_key:
            raise RuntimeError("student parameters were re-allocated after the native engine was built (e.g. .to()); rebuild the wrapper")

    def _check_shape(self, images: torch.Tensor) -> None:
        c0 = self.cfg
        if images.dim() != 4 or images.shape[0] < 1 or tuple(images.shape[1:]) != (c0.in_chans, c0.img_size, c0.img_size) or images.dtype != torch.float32:
            raise RuntimeError(f"expected fp32 images of shape (B, {c0.in_chans}, {c0.img_size}, {c0.img_size}), got {tuple(images.shape)} {images.dtype}")
        self._check_ptrs()

    def _check_images(self, images: torch.Tensor) -> native.Cfg:
        self._check_shape(images)
        self._reserve(images.shape[0])
        return self.cfg_for(images.shape[0])

    def fq_versions(self) -> Tuple[int, ...]:
        return fq_versions(self._fq_flags)

    def decide_mode(self) -> str:
        """The fake-quant mode of the next forward (decide_fq_mode).  Back from observe-only to QAT, the one-plane backward's scale history is as old
        as the last QAT step: the next QAT backward calibrates (the pair form) again."""
        prev = self._fq_state.mode
        mode = decide_fq_mode(self._fq_state, self._fq_flags, self._fq_names)
        if mode == QAT and prev == OBSERVE:
            self.overflow.calibrated = False
        return mode

    def forward(self, images: torch.Tensor, training: bool) -> torch.Tensor:
        """training: the caller's grad mode (False under no_grad).  Leaves the record of this forward in `last_step`."""
        mode = self.decide_mode()                # (a mix of flags raises here, before any launch or collective)
        if mode == OBSERVE:
            return self._forward_observe(images, training)
        c = self._check_images(images)
        # Rank 0's fake-quant state is authoritative at the start of every TRAINING forward (what DDP's buffer broadcast does
        # for the reference).  A forward under no_grad - the reference's evaluate_fp32 runs on rank 0 only
        # (qat_trainer.py:370-371) - issues no collective, whatever its batch size, so a one-rank evaluation cannot dead-lock the group.
        if self.pg is not None and training:
            broadcast_fq_state(self.fq_arena, self.pg)
        images = images.contiguous()
        logits = torch.empty(c.batch, c.num_classes, dtype=torch.float32, device=self.device)
        # a training forward of a calibrated engine leaves the X operands of the qkv / fc1 weight gradients as fp16 integers: its backward is one-plane
        x16 = self.dy16 and self.overflow.calibrated and training
        flags = FWD_X16 if x16 else 0
        # drop-path (module in training mode): filled here, read by this forward and by its backward - the binding stays until the next forward
        self.drop.bind("qatvit_student_set_drop_path", c, self.workspace, self.drop.step(c.batch, self.capacity, self.frozen))
        self.ls.bind(c, self.workspace)
        self.last_step = Step(c, self.generation + 1, x16, mode, int(self.lib.qatvit_student_ln_in_strip(ctypes.byref(c), flags)))
        native.check(self.lib.qatvit_student_forward_stages(ctypes.byref(c), self._ptr_params, self._act_structs, self._w_structs, images.data_ptr(),
                                                            logits.data_ptr(), self.workspace.data_ptr(), 0, c.depth + 1, flags, native.stream_ptr()),
                     "qatvit_student_forward")
        return logits

    # ------------------------------------------------------------------ observe-only step (fake-quant off everywhere)
    def _reserve_observe(self, c: native.Cfg) -> None:
        L, cp = self.lib, ctypes.byref(c)
        if self.observe_buf is None:
            n = L.qatvit_float_student_observe_bytes(cp)
            if n <= 0:
                raise RuntimeError("observe-only step: " + L.qatvit_last_error().decode())
            buf = torch.empty(n, dtype=torch.uint8, device=self.device)
            native.check(L.qatvit_float_student_observe_init(cp, self._act_structs, self._w_structs, buf.data_ptr(), native.stream_ptr()),
                         "qatvit_float_student_observe_init")
            self.observe_buf = buf
        self.float_form.reserve(c, self.device)

    def _forward_observe(self, images: torch.Tensor, training: bool) -> torch.Tensor:
        """Stock semantics with fake_quant_enabled = 0 everywhere: the float network, whose observers (where observer_enabled = 1) still take their
        EMA step; scale / zero_point stay.  The data-parallel state broadcast of a training forward is the QAT step's."""
        self._check_shape(images)
        c = self.cfg_for(images.shape[0])
        self._reserve_observe(c)
        if self.pg is not None and training:
            broadcast_fq_state(self.fq_arena, self.pg)
        images = images.contiguous()
        logits = torch.empty(c.batch, c.num_classes, dtype=torch.float32, device=self.device)
        self.drop.bind("qatvit_float_student_set_drop_path", c, self.float_form.workspace, self.drop.step(c.batch, max(self.capacity, self.float_form.capacity), self.frozen))
        self.ls.bind_float(c, self.float_form.workspace)
        self.last_step = Step(c, self.generation + 1, False, OBSERVE, 0)
        native.check(self.lib.qatvit_float_student_forward_observe(ctypes.byref(c), self._ptr_params, images.data_ptr(), logits.data_ptr(),
                                                                   self.float_form.workspace.data_ptr(), self.observe_buf.data_ptr(), native.stream_ptr()),
                     "qatvit_float_student_forward_observe")
        return logits

    def backward_observe(self, dlogits: torch.Tensor, step: Step) -> List[torch.Tensor]:
        """The float step's backward (every STE mask is 1: the gradient stock computes); in a data-parallel group one average of the whole flat
        gradient afterwards."""
        flat, views, gptr = self._grad_buffers()
        self.ls.bind_float(step.cfg, self.float_form.workspace, views[self.n_abi:])
        self.float_form.call("backward", ctypes.byref(step.cfg), self._ptr_params, dlogits.contiguous().data_ptr(), gptr)
        if self.pg is not None:
            allreduce_mean(flat, self.pg)
        return views

    def _grad_buffers(self):
        return native.flat_grad_buffers(self.params, self.layout.offset, self.grad_numel)

    def _run_backward(self, dlogits: torch.Tensor, c: native.Cfg, flags: int):
        flat, views, gptr = self._grad_buffers()
        L, cp, st = self.lib, ctypes.byref(c), native.stream_ptr()
        self.ls.bind(c, self.workspace, views[self.n_abi:])   # (the gammas' gradients are accumulated into this backward's buffer)

        def run(s0, s1):
            native.check(L.qatvit_student_backward_stages(cp, self._ptr_params, self._act_structs, self._w_structs, dlogits.data_ptr(), gptr,
                                                          self.workspace.data_ptr(), s0, s1, flags, st), "qatvit_student_backward")
            if flags & (BWD_DY16 | BWD_CALIBRATE) and not torch.cuda.is_current_stream_capturing():
                self.overflow.issued()

        if self.pg is None:
            run(0, self.layout.last_stage)
        else:
            staged_backward_allreduce(flat, self.layout, self.bucket_bytes, self.pg, run, self.exposed_events)
        return views

    def backward(self, dlogits: torch.Tensor, step: Step):
        """The backward of the forward that left `step`."""
        dlogits = dlogits.contiguous()
        if not self.dy16:
            return self._run_backward(dlogits, step.cfg, 0)
        if not step.x16:                                # first step on this workspace: the pair form, recording every gradient tensor's maximum
            views = self._run_backward(dlogits, step.cfg, BWD_CALIBRATE)
            self.overflow.calibrated = True
            return views
        views = self._run_backward(dlogits, step.cfg, BWD_DY16)
        if torch.cuda.is_current_stream_capturing():    # a hipGraph capture cannot ask: GraphedStudentStep checks after each replay
            return views
        return self.dy16_fallback(dlogits, step) if self.overflow.resolve() else views

    def dy16_fallback(self, dlogits: torch.Tensor, step: Step):
        """The scales predicted from the previous step did not hold (the flag is raised when max |value| * 2^e > 65504): the same backward again in
        the pair form - bit-identical to a step that never left it - which also re-records the maxima."""
        self.overflow.fallbacks += 1
        if self.dy16_fallbacks == 1:
            warnings.warn("qat-vit_amd: a gradient outgrew its fp16 plane (scale predicted from the previous step); this backward was repeated in the "
                          "bf16-pair form. Harmless if rare (engine.dy16_fallbacks counts them); QATVIT_DY16=0 keeps the pair form throughout.",
                          RuntimeWarning, stacklevel=3)
        native.check(self.lib.qatvit_student_dy16_to_pair(ctypes.byref(step.cfg), self.workspace.data_ptr(), native.stream_ptr()), "qatvit_student_dy16_to_pair")
        return self._run_backward(dlogits.contiguous(), step.cfg, BWD_CALIBRATE)

    # ------------------------------------------------------------------ stage-level access (parity tests, include/qatvit.h "stages")
    # Test infrastructure: these four work on "the configuration of the most recent forward or bind" (self.cfg) by design.
    def tensor(self, name: str, block: int, shape, dtype=torch.float32, cfg: Optional[native.Cfg] = None) -> torch.Tensor:
        """View of a named intermediate tensor inside the workspace (layout of the given / most recent batch size)."""
        c = cfg if cfg is not None else self.cfg
        off = self.lib.qatvit_student_tensor_offset(ctypes.byref(c), name.encode(), block)
        if off < 0:
            raise KeyError(name)
        n = 1
        for s in shape:
            n *= s
        return self.workspace[off:off + n * torch.empty((), dtype=dtype).element_size()].view(dtype).view(*shape)

    def forward_stages(self, images: Optional[torch.Tensor], stage_from: int, stage_to: int, inject: bool = False,
                       logits: Optional[torch.Tensor] = None, x16: bool = False) -> Optional[torch.Tensor]:
        c = self.cfg
        if stage_to == c.depth + 1 and logits is None:
            logits = torch.empty(c.batch, c.num_classes, dtype=torch.float32, device=self.device)
        self.last_step = self.last_step._replace(generation=self.generation + 1)   # (it overwrites the workspace: a forward)
        native.check(self.lib.qatvit_student_forward_stages(
            ctypes.byref(c), self._ptr_params, self._act_structs, self._w_structs, images.data_ptr() if images is not None else None,
            logits.data_ptr() if logits is not None else None, self.workspace.data_ptr(), stage_from, stage_to,
            (STAGE_INJECT if inject else 0) | (FWD_X16 if x16 else 0), native.stream_ptr()), "qatvit_student_forward_stages")
        return logits

    def forward_part(self, block: int, part: int, inject: bool = False, x16: bool = False) -> None:
        """qatvit_student_forward_part: part 0 / 1 / 2 of one block (inputs: x_in / pre-FQ qkv / x_mid of that block)."""
        self.last_step = self.last_step._replace(generation=self.generation + 1)   # (it overwrites the workspace: a forward)
        native.check(self.lib.qatvit_student_forward_part(ctypes.byref(self.cfg), self._ptr_params, self._act_structs, self._w_structs,
                                                          self.workspace.data_ptr(), block, part, (STAGE_INJECT if inject else 0) | (FWD_X16 if x16 else 0),
                                                          native.stream_ptr()),
                     "qatvit_student_forward_part")

    def backward_stages(self, dlogits: Optional[torch.Tensor], stage_from: int, stage_to: int, inject: bool = False, mode: int = 0):
        """Returns per-parameter gradient views (zero for the stages that did not run).  mode: 0 (pair form), BWD_CALIBRATE or BWD_DY16."""
        c = self.cfg
        flat, views, gptr = self._grad_buffers()
        self.ls.bind(c, self.workspace, views[self.n_abi:])
        native.check(self.lib.qatvit_student_backward_stages(
            ctypes.byref(c), self._ptr_params, self._act_structs, self._w_structs, dlogits.contiguous().data_ptr() if dlogits is not None else None,
            gptr, self.workspace.data_ptr(), stage_from, stage_to, (STAGE_INJECT if inject else 0) | mode, native.stream_ptr()), "qatvit_student_backward_stages")
        if mode & (BWD_DY16 | BWD_CALIBRATE):
            self.overflow.issued()
        return views


class _StudentStep(torch.autograd.Function):
    @staticmethod
    def forward(ctx, images, engine, training, *params):
        ctx.engine = engine
        out = engine.forward(images, training)
        ctx.step = engine.last_step
        return out

    @staticmethod
    def backward(ctx, dlogits):
        eng, step = ctx.engine, ctx.step
        native.check_generation(eng, step.generation)
        grads = eng.backward_observe(dlogits, step) if step.fq_mode == OBSERVE else eng.backward(dlogits, step)
        native.assign_grads(eng.params, grads)
        return (None, None, None) + (None,) * len(grads)


# engines live outside the module (a ctypes pointer table must not be deep-copied or pickled with it)
_ENGINES = weakref.WeakKeyDictionary()


def engine_of(wrapper) -> Optional["StudentEngine"]:
    """The native engine bound to a prepared wrapper (None before its first CUDA forward)."""
    return _ENGINES.get(wrapper)


def bind(wrapper, batch: int) -> "StudentEngine":
    """Create (or return) the engine of a prepared wrapper without running a step."""
    eng = _ENGINES.get(wrapper)
    if eng is None:
        eng = _ENGINES[wrapper] = StudentEngine(wrapper, batch)
    return eng


def student_forward(wrapper, images: torch.Tensor) -> torch.Tensor:
    eng = bind(wrapper, images.shape[0])
    # (grad mode is read here: inside autograd.Function.forward it is always off)
    return _StudentStep.apply(images, eng, torch.is_grad_enabled(), *eng.params)
