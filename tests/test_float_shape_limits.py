"""The shape limits of the native float student step, without a GPU: float_engine.check_shape (what native_float accepts) and fs_check behind
qatvit_float_student{,_amp,_bf16}_workspace_bytes (what the C side accepts) must agree on every configuration, one axis at a time around every limit,
and both must take every model of tests/test_gpu_float_shapes.py.  A configuration only one side took would either fail late, inside the first
forward, or refuse a model the kernels cover."""
import ctypes

import pytest

import qat_vit_amd
from qat_vit_amd import native
from qat_vit_amd.float_engine import check_shape

BASE = dict(embed_dim=384, num_heads=6, depth=1, img_size=224, patch_size=16, hidden=1536)
# (what changes against BASE, accepted by the fp32 form, accepted by the fp16 / bf16 forms)
GRID = [
    # tokens = (img / patch)^2 + 1 <= 224: 197 is the largest square grid inside it (223 patches are no square), 226 the first outside
    (dict(), True, True),                                           # 197 tokens
    (dict(img_size=240), False, False),                             # 226
    (dict(img_size=480, patch_size=32), False, False),              # 226 at patch 32
    (dict(img_size=16), True, True),                                # 2: one patch
    (dict(img_size=40), False, False),                              # not a whole number of patches
    # head_dim 32 or 64
    (dict(num_heads=24), False, False),                             # 16
    (dict(num_heads=12), True, True),                               # 32
    (dict(num_heads=3), False, False),                              # 128
    (dict(embed_dim=768, num_heads=6, hidden=3072), False, False),  # 128 at the widest model
    (dict(num_heads=5), False, False),                              # 384 / 5
    # embed_dim: a multiple of 128 (384 for the 16-bit forms), <= 768
    (dict(embed_dim=128, num_heads=2, hidden=512), True, False),
    (dict(embed_dim=128, num_heads=4, hidden=512), True, False),
    (dict(embed_dim=256, num_heads=4, hidden=768), True, False),
    (dict(embed_dim=320, num_heads=5, hidden=1280), False, False),
    (dict(embed_dim=768, num_heads=12, hidden=3072), True, True),
    (dict(embed_dim=768, num_heads=24, hidden=768), True, True),
    (dict(embed_dim=896, num_heads=14, hidden=3584), False, False),
    (dict(embed_dim=1152, num_heads=18, hidden=1152), False, False),
    # mlp hidden: a multiple of 128 (384 for the 16-bit forms)
    (dict(hidden=768), True, True),
    (dict(hidden=1152), True, True),
    (dict(hidden=1280), True, False),
    (dict(hidden=1216), False, False),
    (dict(hidden=192), False, False),
    # patch: a multiple of 4 with in_chans * patch^2 a multiple of 128
    (dict(img_size=64, patch_size=8), False, False),                # 3 * 64 = 192
    (dict(img_size=64, patch_size=16), True, True),
    (dict(img_size=64, patch_size=32), True, True),
    (dict(img_size=224, patch_size=32), True, True),
    # depth 1 .. 12
    (dict(embed_dim=128, num_heads=2, hidden=512, depth=0, img_size=32), False, False),
    (dict(depth=0, img_size=32), False, False),
    (dict(embed_dim=128, num_heads=2, hidden=512, depth=12, img_size=32), True, False),
    (dict(embed_dim=128, num_heads=2, hidden=512, depth=13, img_size=32), False, False),
    (dict(depth=12, img_size=32), True, True),
    (dict(depth=13, img_size=32), False, False),
]
# the models of tests/test_gpu_float_shapes.py (its CASES: checked equal below)
TABLE = {
    "A": (dict(img_size=16, num_heads=6, depth=2), True),
    "B": (dict(img_size=32, num_heads=12, depth=2), True),
    "C": (dict(img_size=80, num_heads=6, depth=2), True),
    "D": (dict(img_size=96, num_heads=6, depth=2), True),
    "E": (dict(img_size=96, num_heads=12, depth=1), True),
    "F": (dict(img_size=128, num_heads=6, depth=2, mlp_ratio=2), True),
    "G": (dict(img_size=224, patch_size=32, num_heads=6, depth=2), True),
    "H": (dict(img_size=224, num_heads=12, depth=1), True),
    "P": (dict(embed_dim=128, num_heads=4, img_size=32, depth=2), False),
}
WS = {False: ("qatvit_float_student_workspace_bytes",), True: ("qatvit_float_student_amp_workspace_bytes", "qatvit_float_student_bf16_workspace_bytes")}


def _model(embed_dim, num_heads, depth, img_size, patch_size, hidden, num_classes=10):
    m = qat_vit_amd.create_student("vit", num_classes=num_classes, embed_dim=embed_dim, num_heads=num_heads, depth=depth, img_size=img_size,
                                   patch_size=patch_size, mlp_ratio=hidden / embed_dim)
    assert all(b.mlp.fc1.weight.shape[0] == hidden for b in m.blocks)
    return m


def _cfg(embed_dim, num_heads, depth, img_size, patch_size, hidden, num_classes=10):
    return native.Cfg(batch=1, img_size=img_size, patch_size=patch_size, in_chans=3, embed_dim=embed_dim, depth=depth, num_heads=num_heads,
                      mlp_hidden=hidden, num_classes=num_classes, act_qmin=0, act_qmax=255, w_qmin=-128, w_qmax=127, w_per_channel=0,
                      averaging_const=0.01, ln_eps=1e-6)


def _python_accepts(model, amp):
    try:
        check_shape(model, amp)
    except RuntimeError as e:   # (anything else - an IndexError on an empty block list - is a bug of check_shape and fails the test)
        assert "unsupported model" in str(e), e
        return False
    return True


def _c_accepts(lib, cfg, amp):
    got = set()
    for fn in WS[amp]:
        n = getattr(lib, fn)(ctypes.byref(cfg))
        assert n == -1 or n > 0, (fn, n)
        if n == -1:
            assert b"unsupported config" in lib.qatvit_last_error(), fn
        got.add(n > 0)
    assert len(got) == 1, "the fp16 and bf16 forms disagree"
    return got.pop()


@pytest.mark.parametrize("change,fp32_ok,amp_ok", GRID, ids=[",".join(f"{k}={v}" for k, v in g[0].items()) or "base" for g in GRID])
def test_check_shape_and_workspace_bytes_accept_the_same_configurations(native_lib, change, fp32_ok, amp_ok):
    kw = dict(BASE, **change)
    model, cfg = _model(**kw), _cfg(**kw)
    if kw["depth"] >= 1:   # the engine's own Cfg of this model is the one asked about
        shape = native.vit_shape(model)
        assert all(getattr(cfg, k) == v for k, v in shape.items() if k != "ln_eps"), shape
    for amp, want in ((False, fp32_ok), (True, amp_ok)):
        py, c = _python_accepts(model, amp), _c_accepts(native_lib, cfg, amp)
        assert py == c, f"amp={amp}: check_shape {'accepts' if py else 'refuses'}, workspace_bytes {'accepts' if c else 'refuses'} {kw}"
        assert c == want, (amp, kw)


@pytest.mark.parametrize("case", sorted(TABLE))
def test_every_case_of_the_shape_suite_is_accepted_by_both(native_lib, case):
    from tests.test_gpu_float_shapes import CASES

    kw, amp_ok = TABLE[case]
    assert CASES[case][0] == kw and sorted(CASES) == sorted(TABLE)
    classes, batch = CASES[case][3], CASES[case][2]
    model = qat_vit_amd.create_model("vit_small_patch16_224_student", pretrained=False, num_classes=classes, qat_wrapper=True, **kw).model
    assert model.patch_embed.num_patches + 1 == CASES[case][1]
    cfg = native.Cfg(batch=batch, act_qmin=0, act_qmax=255, w_qmin=-128, w_qmax=127, w_per_channel=0, averaging_const=0.01, **native.vit_shape(model))
    assert _python_accepts(model, False) and _c_accepts(native_lib, cfg, False)
    assert _python_accepts(model, True) == amp_ok and _c_accepts(native_lib, cfg, True) == amp_ok
    tw = native_lib.qatvit_teacher_workspace_bytes(ctypes.byref(cfg))
    assert tw > 0, native_lib.qatvit_last_error()
