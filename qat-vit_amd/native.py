"""ctypes binding of libqatvit.so (C ABI: include/qatvit.h).

There is no CPU implementation behind this module: if the shared library is
missing or a call fails, the caller gets a RuntimeError - never a silent
PyTorch fallback.
"""
from __future__ import annotations

import ctypes
import os
import subprocess
from ctypes import c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libqatvit.so")
CSRC = os.path.join(_HERE, "csrc")
_lib = None

# name -> (restype, argtypes); every symbol include/qatvit.h declares
SIGNATURES = {
    "qatvit_abi_version": (c_int, []),
    "qatvit_last_error": (c_char_p, []),
    "qatvit_target_arch": (c_char_p, []),
    "qatvit_fq_workspace_bytes": (c_int64, [c_int64]),
    "qatvit_fq_forward": (c_int, [c_void_p] * 9 + [c_float, c_int32, c_int32, c_int64, c_int64, c_int32, c_int32, c_void_p, c_void_p]),
    "qatvit_fq_backward": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "qatvit_ln_forward": (c_int, [c_void_p] * 6 + [c_int64, c_int64, c_float, c_void_p]),
    "qatvit_ln_backward": (c_int, [c_void_p] * 8 + [c_int64, c_int64, c_void_p]),
    "qatvit_kd_ce_loss": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_float, c_float, c_float, c_void_p, c_void_p, c_void_p]),
    "qatvit_kd_ce_loss_table": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int64, c_float, c_float, c_float, c_void_p, c_void_p, c_void_p]),
    "qatvit_kd_ce_loss_mix": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_float, c_float, c_float,
                                      c_void_p, c_void_p, c_void_p]),
    "qatvit_kd_bce_loss": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_float, c_float, c_float,
                                   c_float, c_int32, c_void_p, c_void_p, c_void_p, c_void_p]),
    "qatvit_optim_grad_norm": (c_int, [c_void_p] * 4 + [c_int32, c_int64, c_float, c_void_p, c_void_p, c_void_p]),
    "qatvit_optim_adamw": (c_int, [c_void_p] * 7 + [c_int32, c_int64] + [c_double] * 5 + [c_int64, c_void_p, c_void_p]),
    "qatvit_optim_adamw_groups": (c_int, [c_void_p] * 8 + [c_int32, c_int64, c_void_p, c_int32, c_void_p, c_void_p]),
    "qatvit_optim_adamw_ema": (c_int, [c_void_p] * 8 + [c_int32, c_int64] + [c_double] * 5 + [c_int64, c_double, c_void_p, c_void_p]),
    "qatvit_optim_adamw_groups_ema": (c_int, [c_void_p] * 9 + [c_int32, c_int64, c_void_p, c_int32, c_double, c_void_p, c_void_p]),
    "qatvit_optim_ema": (c_int, [c_void_p] * 5 + [c_int32, c_int64, c_double, c_void_p]),
    "qatvit_optim_swap": (c_int, [c_void_p] * 5 + [c_int32, c_int64, c_void_p]),
    "qatvit_optim_lamb_moments": (c_int, [c_void_p] * 8 + [c_int32, c_int64, c_void_p, c_int32, c_void_p, c_void_p, c_void_p]),
    "qatvit_optim_lamb_apply": (c_int, [c_void_p] * 9 + [c_int32, c_int64, c_void_p, c_int32, c_double, c_void_p, c_void_p, c_void_p]),
    "qatvit_gemm_nt": (c_int, [c_void_p] * 4 + [c_int32] * 6 + [c_void_p] * 6),
    "qatvit_gemm_nt_f16": (c_int, [c_void_p] * 4 + [c_int32] * 6 + [c_void_p] * 6),
    "qatvit_gemm_nt_i8_minmax": (c_int, [c_void_p] * 4 + [c_int32] * 6 + [c_void_p] * 6),
    "qatvit_w8_fragment_order": (c_int, [c_void_p, c_void_p, c_int32, c_int32, c_void_p]),
    "qatvit_i8_strip": (c_int, [c_int32] + [c_void_p] * 4 + [c_int32] * 5 + [c_void_p] * 6 + [c_int32, c_int32, c_void_p, c_void_p, c_int32] + [c_void_p] * 4),
    "qatvit_ln_apply_quant8": (c_int, [c_void_p] * 6 + [c_int32, c_int32, c_void_p, c_int32, c_int64, c_int32, c_void_p]),
    "qatvit_i8_strip_ln": (c_int, [c_void_p] * 5 + [c_int32, c_int32] + [c_void_p] * 4 + [c_int32] * 5 + [c_void_p] * 5),
    "qatvit_gemm_nt_codes": (c_int, [c_void_p] * 4 + [c_int32] * 6 + [c_void_p] * 6),
    "qatvit_gemm_nt_resid_fq": (c_int, [c_int32] + [c_void_p] * 5 + [c_int32] * 6 + [c_void_p] * 5 + [c_int32, c_int32, c_void_p, c_void_p]),
    "qatvit_gemm_nt_i8": (c_int, [c_void_p] * 4 + [c_int32, c_void_p] + [c_int32] * 6 + [c_void_p] * 6),
    "qatvit_gemm_tn_scratch_bytes": (c_int64, []),
    "qatvit_gemm_tn": (c_int, [c_void_p] * 5 + [c_int32] * 6 + [c_void_p] * 4 + [c_int32] * 3 + [c_void_p] * 3 + [c_int64, c_void_p]),
    "qatvit_gemm_tn_codes": (c_int, [c_void_p] * 5 + [c_int32] * 6 + [c_void_p] * 4 + [c_int32] * 3 + [c_void_p] * 3 + [c_int64, c_void_p]),
    "qatvit_gemm_nt_dy16": (c_int, [c_void_p] * 3 + [c_int32] * 6 + [c_void_p] * 3),
    "qatvit_gemm_tn_dy16": (c_int, [c_void_p] * 6 + [c_int32] * 6 + [c_void_p] * 5 + [c_int32] * 3 + [c_void_p] * 3 + [c_int64, c_void_p]),
    "qatvit_gemm_tn_q8_dy16": (c_int, [c_void_p] * 3 + [c_int32, c_void_p] + [c_int32] * 6 + [c_void_p] * 4 + [c_int32] * 3 + [c_void_p] * 3 + [c_int64, c_void_p]),
    "qatvit_gemm_tn_stream_scratch_bytes": (c_int64, []),
    "qatvit_gemm_tn_stream_dy16": (c_int, [c_int32, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_int64, c_void_p]),
    "qatvit_rows_gather": (c_int, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int64, c_void_p]),
    "qatvit_rows_scatter": (c_int, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p]),
    "qatvit_attn_padded_tokens": (c_int32, [c_int32]),
    "qatvit_attn_forward": (c_int, [c_void_p, c_void_p] + [c_int32] * 6 + [c_void_p] * 4),
    "qatvit_attn_forward_f16": (c_int, [c_void_p, c_void_p] + [c_int32] * 6 + [c_void_p] * 9),
    "qatvit_attn_backward": (c_int, [c_void_p, c_void_p] + [c_int32] * 6 + [c_void_p] * 11),
    "qatvit_attn_backward_live": (c_int, [c_void_p, c_void_p] + [c_int32] * 6 + [c_void_p] * 10 + [c_int32, c_int32, c_void_p]),
    "qatvit_attn_backward_form": (c_int, [c_void_p, c_void_p] + [c_int32] * 6 + [c_void_p] * 12 + [c_int32, c_void_p]),
    "qatvit_student_num_params": (c_int32, [c_void_p]),
    "qatvit_student_num_act_fq": (c_int32, [c_void_p]),
    "qatvit_student_num_weight_fq": (c_int32, [c_void_p]),
    "qatvit_student_workspace_bytes": (c_int64, [c_void_p]),
    "qatvit_student_init": (c_int, [c_void_p, c_void_p, c_void_p]),
    "qatvit_student_forward": (c_int, [c_void_p] * 8),
    "qatvit_student_backward": (c_int, [c_void_p] * 7 + [c_int32, c_int32, c_void_p]),
    "qatvit_student_forward_stages": (c_int, [c_void_p] * 7 + [c_int32, c_int32, c_int32, c_void_p]),
    "qatvit_student_forward_part": (c_int, [c_void_p] * 5 + [c_int32, c_int32, c_int32, c_void_p]),
    "qatvit_student_backward_stages": (c_int, [c_void_p] * 7 + [c_int32, c_int32, c_int32, c_void_p]),
    "qatvit_student_tensor_offset": (c_int64, [c_void_p, c_char_p, c_int32]),
    "qatvit_student_dy16_supported": (c_int32, [c_void_p]),
    "qatvit_student_ln_in_strip": (c_int32, [c_void_p, c_int32]),
    "qatvit_student_dy16_to_pair": (c_int, [c_void_p, c_void_p, c_void_p]),
    "qatvit_student_dy16_set_mirror": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p]),
    "qatvit_student_set_drop_path": (c_int, [c_void_p, c_void_p, c_void_p]),
    "qatvit_float_student_set_drop_path": (c_int, [c_void_p, c_void_p, c_void_p]),
    "qatvit_student_set_layer_scale": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p]),
    "qatvit_float_student_set_layer_scale": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "qatvit_float_student_layer_scale_bytes": (c_int64, [c_void_p]),
    "qatvit_teacher_workspace_bytes": (c_int64, [c_void_p]),
    "qatvit_teacher_forward": (c_int, [c_void_p] * 8),
    "qatvit_teacher_forward_f16": (c_int, [c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p]),
    "qatvit_float_student_workspace_bytes": (c_int64, [c_void_p]),
    "qatvit_float_student_init": (c_int, [c_void_p] * 3),
    "qatvit_float_student_forward": (c_int, [c_void_p] * 6),
    "qatvit_float_student_backward": (c_int, [c_void_p] * 6),
    "qatvit_float_student_observe_bytes": (c_int64, [c_void_p]),
    "qatvit_float_student_observe_init": (c_int, [c_void_p] * 5),
    "qatvit_float_student_forward_observe": (c_int, [c_void_p] * 7),
    "qatvit_float_student_amp_workspace_bytes": (c_int64, [c_void_p]),
    "qatvit_float_student_amp_init": (c_int, [c_void_p] * 3),
    "qatvit_float_student_amp_forward": (c_int, [c_void_p] * 6),
    "qatvit_float_student_amp_backward": (c_int, [c_void_p] * 6),
    "qatvit_float_student_amp_attn_backward": (c_int, [c_void_p] * 4 + [c_int32] * 4 + [c_void_p] * 2),
    "qatvit_float_student_bf16_workspace_bytes": (c_int64, [c_void_p]),
    "qatvit_float_student_bf16_init": (c_int, [c_void_p] * 3),
    "qatvit_float_student_bf16_forward": (c_int, [c_void_p] * 6),
    "qatvit_float_student_bf16_backward": (c_int, [c_void_p] * 6),
    "qatvit_float_student_bf16_attn_backward": (c_int, [c_void_p] * 4 + [c_int32] * 4 + [c_void_p] * 2),
    "qatvit_infer_workspace_bytes": (c_int64, [c_void_p]),
    "qatvit_infer_prepare": (c_int, [c_void_p] * 6),
    "qatvit_infer_forward": (c_int, [c_void_p] * 8),
    "qatvit_infer_forward_ls": (c_int, [c_void_p] * 9),
    "qatvit_image_resize_coeffs": (c_int, [c_int32, c_int32, c_void_p, c_void_p, c_void_p]),
    "qatvit_image_table": (c_int, [c_void_p] * 3),
    "qatvit_image_batch": (c_int, [c_void_p, c_void_p] + [c_int32] * 4 + [c_void_p] * 4),
    "qatvit_image_batch_aug": (c_int, [c_void_p, c_void_p] + [c_int32] * 4 + [c_void_p] * 3 + [c_int32, c_int32, c_void_p, c_void_p]),
    "qatvit_image_batch_mix": (c_int, [c_void_p, c_void_p] + [c_int32] * 4 + [c_void_p] * 3 + [c_int32, c_int32, c_void_p, c_void_p, c_void_p]),
    "qatvit_image_resize_coeffs_windows": (c_int, [c_int32, c_int32, c_void_p]),
    "qatvit_image_batch_rrc": (c_int, [c_void_p, c_void_p] + [c_int32] * 4 + [c_void_p] * 6),
    "qatvit_image_batch_erase": (c_int, [c_void_p, c_void_p] + [c_int32] * 4 + [c_void_p] * 3 + [c_int32, c_int32] + [c_void_p] * 4),
    "qatvit_image_batch_rrc_erase": (c_int, [c_void_p, c_void_p] + [c_int32] * 4 + [c_void_p] * 7),
    "qatvit_image_batch_color": (c_int, [c_void_p, c_void_p] + [c_int32] * 4 + [c_void_p] * 3 + [c_int32, c_int32] + [c_void_p] * 6),
    "qatvit_image_batch_rrc_color": (c_int, [c_void_p, c_void_p] + [c_int32] * 4 + [c_void_p] * 9),
    "qatvit_image_batch_blur": (c_int, [c_void_p, c_void_p] + [c_int32] * 4 + [c_void_p] * 3 + [c_int32, c_int32] + [c_void_p] * 7),
    "qatvit_image_batch_rrc_blur": (c_int, [c_void_p, c_void_p] + [c_int32] * 4 + [c_void_p] * 10),
    "qatvit_image_window_coeffs_bytes": (c_int64, [c_int32, c_int32]),
    "qatvit_image_window_coeffs": (c_int, [c_int32, c_int32, c_void_p]),
    "qatvit_image_window_u8": (c_int, [c_void_p, c_void_p] + [c_int32] * 5 + [c_void_p, c_int32, c_void_p, c_void_p, c_void_p]),
    "qatvit_image_bytes_blur": (c_int, [c_void_p, c_int32, c_int32] + [c_void_p] * 8),
    "qatvit_eval_accumulate": (c_int, [c_void_p, c_int32, c_int64, c_void_p, c_int64, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p]),
    "qatvit_profile_start": (c_int, [c_void_p, c_int32, c_int32]),
    "qatvit_profile_stop": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p]),
}


class Cfg(ctypes.Structure):
    """struct qatvit_cfg (include/qatvit.h)."""
    _fields_ = [(n, c_int32) for n in ("batch", "img_size", "patch_size", "in_chans", "embed_dim", "depth", "num_heads", "mlp_hidden",
                                       "num_classes", "act_qmin", "act_qmax", "w_qmin", "w_qmax", "w_per_channel")] + \
               [("averaging_const", c_float), ("ln_eps", c_float)]


def vit_params(model) -> list:
    """The parameters of a ViT tree in the order of the C ABI (include/qatvit.h): patch embedding, cls token, pos embedding, 12 per block,
    final norm, head."""
    pe = model.patch_embed.proj
    ps = [pe.weight, pe.bias, model.cls_token, model.pos_embed]
    for b in model.blocks:
        ps += [b.norm1.weight, b.norm1.bias, b.attn.qkv.weight, b.attn.qkv.bias, b.attn.proj.weight, b.attn.proj.bias,
               b.norm2.weight, b.norm2.bias, b.mlp.fc1.weight, b.mlp.fc1.bias, b.mlp.fc2.weight, b.mlp.fc2.bias]
    return ps + [model.norm.weight, model.norm.bias, model.head.weight, model.head.bias]


def vit_shape(model) -> dict:
    """The shape fields of Cfg for a ViT tree, as keyword arguments (the caller adds batch and the quantiser fields)."""
    b0 = model.blocks[0]
    return dict(img_size=model.patch_embed.img_size, patch_size=model.patch_embed.patch_size, in_chans=model.patch_embed.proj.weight.shape[1],
                embed_dim=model.embed_dim, depth=len(model.blocks), num_heads=b0.attn.num_heads, mlp_hidden=b0.mlp.fc1.weight.shape[0],
                num_classes=model.head.weight.shape[0], ln_eps=float(b0.norm1.eps))


class TNItem(ctypes.Structure):
    """struct qatvit_tn_item (include/qatvit.h)."""
    _fields_ = [(n, c_void_p) for n in ("P", "Q", "lut", "s1", "s2", "C", "W", "w_scale", "w_zp", "dbias", "row_div")] + [(n, c_int32) for n in ("N", "Kw", "ldp", "ldq", "ldc")]


class AdamWGroup(ctypes.Structure):
    """struct qatvit_adamw_group (include/qatvit.h)."""
    _fields_ = [(n, c_double) for n in ("lr", "beta1", "beta2", "eps", "weight_decay")] + [("step", c_int64)]


class LambGroup(ctypes.Structure):
    """struct qatvit_lamb_group (include/qatvit.h)."""
    _fields_ = [(n, c_double) for n in ("lr", "beta1", "beta2", "eps", "weight_decay")] + [("step", c_int64)] + \
               [(n, c_int32) for n in ("grad_averaging", "always_adapt", "trust_clip", "reserved")]


class FQ(ctypes.Structure):
    """struct qatvit_fq (include/qatvit.h)."""
    _fields_ = [(n, c_void_p) for n in ("min_val", "max_val", "scale", "zero_point", "observer_on", "fake_quant_on")]


def build(verbose: bool = False) -> str:
    """Compile csrc/*.hip for gfx950 into libqatvit.so (hipcc cross-compiles without a GPU)."""
    r = subprocess.run(["make", "-C", CSRC, "-j8"], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("building libqatvit.so failed:\n" + r.stdout[-4000:] + r.stderr[-4000:])
    if verbose:
        print(r.stdout[-2000:])
    return LIB_PATH


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: the MI355X path has no fallback. Build it with "
                "`python -c 'import __graft_entry__ as g; g.build()'` (needs hipcc)."
            )
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)  # AttributeError here = header/library drift
            fn.restype, fn.argtypes = res, args
        if L.qatvit_abi_version() != 4:
            raise RuntimeError("libqatvit.so ABI version mismatch")
        _lib = L
    return _lib


def check(status: int, what: str) -> None:
    if status != 0:
        raise RuntimeError(f"{what} failed ({status}): {lib().qatvit_last_error().decode()}")


def stream_ptr() -> int:
    import torch

    return torch.cuda.current_stream().cuda_stream


# ---- what the autograd functions of the QAT engine (engine.py) and the float engine (float_engine.py) share

def check_generation(engine, generation: int) -> None:
    """The activations, STE masks and qparams of a step live in the engine's one workspace, not in autograd's graph: a later forward (an evaluation
    under no_grad, a second micro-batch) has overwritten them.  Stock autograd would keep both alive; here the backward would silently differentiate
    the wrong step - refuse."""
    if engine.generation != generation:
        raise RuntimeError(
            "qat-vit_amd: another forward of this model ran between this forward and its backward; the native step keeps the "
            "saved activations of ONE forward per model. Call backward() before the next forward (gradient accumulation: "
            "forward/backward per micro-batch)."
        )


class DropPathTable:
    """The drop-path scale table of one engine (include/qatvit.h, qatvit_student_set_drop_path): ONE static fp32 buffer per capacity, so the address a
    workspace is bound to - and a captured hipGraph replays - is the same every step; the step at batch B uses its front as [2 * depth, B].

    ``step(batch, capacity)``: the table of the forward about to run, or None when that forward has no drop-path (eval mode, or a tree without
    stochastic depth outside ``forced_drop_path``).  Filled here: the caller's table inside ``forced_drop_path``, else ONE draw for the whole step -
    ``bernoulli`` over [2 * depth, B] with each branch's keep probability, times its 1 / keep - on the device, without a synchronisation.  The draw has
    the modules' distribution but does not consume the generator as their 2 * depth separate calls would.  While the stream is being captured nothing is
    filled: the owner of the graph refills before every replay (``refill``)."""

    def __init__(self, model, device):
        self.model, self.device = model, device
        self.rows = 2 * len(model.blocks)
        self.plan = self.keep = self.mult = None   # the modules' rates as last read, and their device copies
        self.round_to = None                       # the 16-bit type of the float form the table was last filled for (None: fp32 as given)
        self.buf = None
        self.capacity = 0
        self.bound = set()   # addresses of the workspaces a table was handed to (those a forward without a table has to unbind)
        self.read_plan()

    def read_plan(self) -> None:
        """The modules' rates are read before every step (a drop-path schedule changes ``drop_prob`` between epochs): host work, and a host-to-device
        copy only when a rate moved."""
        import torch
        from .vit import drop_path_plan

        plan = drop_path_plan(self.model)
        if plan == self.plan:
            return
        self.plan = plan
        self.keep = self.mult = None
        if plan is not None:
            self.keep = torch.tensor(plan[0], dtype=torch.float32, device=self.device).view(-1, 1)
            self.mult = torch.tensor(plan[1], dtype=torch.float32, device=self.device).view(-1, 1)

    def active(self) -> bool:
        from .vit import forced_table

        if not self.model.training:
            return False
        self.read_plan()
        return self.plan is not None or forced_table(self.model) is not None

    def view(self, batch: int):
        return self.buf[:self.rows * batch].view(self.rows, batch)

    def refill(self, batch: int) -> None:
        import torch
        from .vit import forced_table

        t, forced = self.view(batch), forced_table(self.model)
        if forced is not None:
            if tuple(forced.shape) != (self.rows, batch):
                raise RuntimeError(f"forced_drop_path: the table is {tuple(forced.shape)}, this step needs [{self.rows}, {batch}]")
            t.copy_(forced)
        elif self.keep is not None:
            torch.bernoulli(self.keep.expand(self.rows, batch), out=t)
            t.mul_(self.mult)
        else:
            t.fill_(1.0)
        if self.round_to is not None:   # stock autocast holds the mask in the 16-bit type, forward and backward alike: the table holds those values
            t.copy_(t.to(self.round_to))

    def step(self, batch: int, capacity: int, frozen: bool = False, round_to=None):
        """round_to: torch.float16 / torch.bfloat16 for the float step's 16-bit forms - the multipliers are stored rounded to that type."""
        import torch

        if not self.active():
            return None
        self.round_to = round_to
        if max(batch, capacity) > self.capacity:
            if frozen and self.buf is not None:
                raise RuntimeError(f"batch {batch} exceeds the drop-path table ({self.capacity}) a captured hipGraph is bound to")
            self.capacity = max(batch, capacity)
            self.buf = torch.ones(self.rows * self.capacity, dtype=torch.float32, device=self.device)
        if not torch.cuda.is_current_stream_capturing():
            self.refill(batch)
        return self.view(batch)

    def bind(self, setter: str, cfg, workspace, table) -> None:
        """Hand `table` (None: no drop-path) to the library for the calls on `workspace` that follow; a workspace that never saw a table is never touched."""
        ws = workspace.data_ptr()
        if table is None and ws not in self.bound:
            return
        check(getattr(lib(), setter)(ctypes.byref(cfg), ws, table.data_ptr() if table is not None else None), setter)
        if table is None:
            self.bound.discard(ws)
        else:
            self.bound.add(ws)


class LayerScaleBinding:
    """The LayerScale gammas of one engine's model (include/qatvit.h, qatvit_student_set_layer_scale): the 2 * depth parameters in branch order, which the
    engine keeps BEHIND the 8 + 12 * depth parameters of the C ABI, and the host-side binding of their addresses to a step workspace.  A forward binds the
    gammas alone (and, float forms, the buffer that keeps the branch outputs for the backward); a backward binds them again together with its gradient
    views - the gradient buffer of a step is allocated by its backward.  Parameter addresses are static, so a captured hipGraph replays them as it is."""

    def __init__(self, model, device):
        import torch
        from .vit import layer_scale_params

        self.gammas = layer_scale_params(model)
        self.device = device
        for g in self.gammas:
            if g.dtype != torch.float32 or not g.is_contiguous() or g.device != device:
                raise RuntimeError("every LayerScale gamma must be a contiguous fp32 tensor on the model's device")
        self._gptr = (ctypes.c_void_p * len(self.gammas))(*[g.data_ptr() for g in self.gammas]) if self.gammas else None
        self.saved = None   # the float forms' retained branch outputs (qatvit_float_student_layer_scale_bytes), grown on demand

    def __bool__(self) -> bool:
        return bool(self.gammas)

    def _grads(self, views):
        if views is None:
            return None
        assert len(views) == len(self.gammas)
        return (ctypes.c_void_p * len(views))(*[v.data_ptr() for v in views])

    def bind(self, cfg, workspace, grad_views=None) -> None:
        """The QAT step's workspace.  grad_views: the zeroed gradient views of the gammas (a backward), None: a forward."""
        if self.gammas:
            check(lib().qatvit_student_set_layer_scale(ctypes.byref(cfg), workspace.data_ptr(), self._gptr, self._grads(grad_views)), "qatvit_student_set_layer_scale")

    def bind_float(self, cfg, workspace, grad_views=None) -> None:
        """A float-step workspace of any form; the branch outputs of the forward go to (and its backward reads them from) the engine's one saved buffer."""
        import torch

        if not self.gammas:
            return
        n = lib().qatvit_float_student_layer_scale_bytes(ctypes.byref(cfg))
        if n <= 0:
            raise RuntimeError("qatvit_float_student_layer_scale_bytes failed")
        if self.saved is None or self.saved.numel() < n:
            if grad_views is not None:
                raise RuntimeError("LayerScale: the saved-branch buffer of this backward's forward is gone")
            self.saved = None
            self.saved = torch.empty(n, dtype=torch.uint8, device=self.device)
        check(lib().qatvit_float_student_set_layer_scale(ctypes.byref(cfg), workspace.data_ptr(), self._gptr, self._grads(grad_views), self.saved.data_ptr()),
              "qatvit_float_student_set_layer_scale")


def assign_grads(params, grads) -> None:
    """The native backward writes every parameter gradient into one flat buffer; hand the views to the parameters directly (what
    `zero_grad(set_to_none=True)` + autograd would end up with) instead of returning them, so autograd's AccumulateGrad does not clone 152 tensors
    per step.  Stock ``DDP(prepared)`` keeps working on top of this because DDP's reducer is driven by post-accumulate-grad hooks that fire when
    ``.grad`` is assigned here (tests/test_gpu_dp.py); the native bucketed path (``enable_data_parallel``) is the one bench.py measures."""
    for p, g in zip(params, grads):
        if p.grad is None:
            p.grad = g
        else:
            p.grad.add_(g)


def flat_grad_buffers(params, offsets, numel: int):
    """(flat, views, pointer table): one zeroed fp32 buffer of `numel` elements, a view of parameter i's shape at offsets[i], and the views'
    addresses as the `void**` the native backward takes."""
    import torch

    flat = torch.zeros(numel, dtype=torch.float32, device=params[0].device)
    views = [flat[offsets[i]:offsets[i] + p.numel()].view(p.shape) for i, p in enumerate(params)]
    return flat, views, (ctypes.c_void_p * len(views))(*[v.data_ptr() for v in views])
