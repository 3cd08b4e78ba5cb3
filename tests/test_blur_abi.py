"""CPU-side checks of Gaussian blur inside the batch launch (qatvit_image_batch_blur, qatvit_image_batch_rrc_blur, qat_vit_amd.GaussianBlur,
qat_vit_amd.ThreeAugment): the symbols in the header, the binding and the library; the refusal matrix of tests/test_image_request_abi.py for the
two new entries and every subset of their optional records set to NULL; the LDS refusal; the host restatement tests/blur_ref.py against Pillow's
bytes in tests/golden/blur_kat.npz; the known (radius, ww, fw) answers; the cleaning rule of a record; the drawing rules of the two classes; the
loader's draw order.  Nothing here needs a GPU: every library call ends in an error string before any HIP call."""
import itertools
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import qat_vit_amd
from qat_vit_amd import data, native
from tests import blur_ref, color_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 4096                                                             # non-null, 4096-aligned; never dereferenced on these paths
PRE = "qatvit_image_batch"
ENTRIES = {PRE + "_blur": ("aug", "mix", "erase", "color", "sums", "blur"), PRE + "_rrc_blur": ("rrc", "mix", "erase", "color", "sums", "blur")}
NO_RRC = "rrc is NULL (the call without window records is qatvit_image_batch_blur)"
CASES = [(name, frozenset(absent)) for name, recs in ENTRIES.items() for opt in [[r for r in recs if r != "rrc"]]
         for k in range(len(opt) + 1) for absent in itertools.combinations(opt, k)]
IDS = [n[len(PRE):].lstrip("_") + "-" + "".join(sorted(r[0] for r in a)) for n, a in CASES]
KNOWN = {0.1: (0, 16721291, 27962), 0.5: (0, 15379114, 699051), 1.0: (0, 11184811, 2796202), 2.0: (1, 4473924, 1677722)}


def _call(L, name, absent=(), **kw):
    a = dict(data=P, index=None, B=1, N=1, S=32, D=224, tab=P, table=P, mode=0, fill=0, out=P, **{r: P for r in ENTRIES[name]})
    a.update({r: None for r in absent})
    assert set(kw) <= set(a), (name, kw)
    a.update(kw)
    tail = []
    for r in ENTRIES[name]:
        tail += [a["aug"], a["mode"], a["fill"]] if r == "aug" else [a[r]]
    rc = getattr(L, name)(a["data"], a["index"], a["B"], a["N"], a["S"], a["D"], a["tab"], a["table"], *tail, a["out"], None)
    return rc, L.qatvit_last_error().decode()


def _refused(L, name, absent, text, who=None, **kw):
    rc, err = _call(L, name, absent, **kw)
    assert rc != 0 and err.startswith((who or name) + ": ") and text in err, (name, sorted(absent), kw, err)
    return err


def _blur_lds(S, D, mixed, rrc):
    """The blur forms' LDS request as DESIGN.md 7v states it, with n = 16 + 12 rows (a band and its halo) or, with mix records, 8 + 12: the
    tables, the source rows of n output rows, a plane set and an image buffer of n rows per side, one more such buffer, and with windows n
    entries of the row table per side."""
    n, sides = 20 if mixed else 28, 2 if mixed else 1
    rows = (n * S + D - 1) // D + 5
    planes = D * 5 * 4 + 768 * 4 + ((rows * S * 3 + 15) & ~15)
    img = (planes + sides * rows * 3 * D + 15) & ~15
    end = img + (sides + 1) * n * 3 * D
    return ((end + 15) & ~15) + sides * n * 5 * 4 if rrc else end


def _sibling(name, absent):
    """The narrowest entry that serves the records of (entry, subset) once blur is NULL."""
    recs = set(ENTRIES[name]) - absent
    level = "_color" if "color" in recs else "_erase" if "erase" in recs else ""
    if "rrc" in recs:
        return PRE + "_rrc" + level
    return PRE + (level or ("_mix" if "mix" in recs else "_aug" if "aug" in recs else ""))


def _params(name):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "qatvit.h")).read(), flags=re.S)
    decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, hdr)
    assert decl, f"{name} is not declared in include/qatvit.h"
    return [" ".join(p.split()) for p in decl.group(1).split(",")]


def test_symbols_in_header_signatures_and_exports(native_lib):
    assert len(CASES) == 64 + 32                                     # every subset of six, and of five, optional records
    exported = subprocess.run(["nm", "-D", "--defined-only", native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in exported.splitlines() if line.strip()}
    for name, sibling in ((PRE + "_blur", PRE + "_color"), (PRE + "_rrc_blur", PRE + "_rrc_color")):
        params, sib = _params(name), _params(sibling)
        assert params == sib[:-2] + ["const int32_t* blur", "float* out", "void* stream"]       # the colour entry's arguments, then blur
        res, args = native.SIGNATURES[name]
        assert res is native.c_int and len(args) == len(params)
        for p, a in zip(params, args):
            assert a is (native.c_void_p if "*" in p else native.c_int32), (name, p)
        assert name in exported
    assert native_lib.qatvit_abi_version() == 4                      # added symbols: the version stays
    assert {"GaussianBlur", "ThreeAugment"} <= set(qat_vit_amd.__all__) and data.BLUR_WORDS == 4
    hdr = open(os.path.join(ROOT, "include", "qatvit.h")).read()
    assert "blur int32 [B][4]" in hdr and "(2 * radius + 1) * ww + 2 * fw <= 2^24" in hdr
    kernels = open(os.path.join(ROOT, "qat-vit_amd", "csrc", "qv_kernels.h")).read()
    assert "kImgBlurMaxRadius = 1" in kernels and re.search(r"const int32_t\* blur = nullptr;", kernels)


@pytest.mark.parametrize("name,absent", CASES, ids=IDS)
def test_every_rule_refuses_under_the_called_name(native_lib, name, absent):
    L, recs = native_lib, ENTRIES[name]
    present = [r for r in recs if r not in absent]
    bad = lambda text, **kw: _refused(L, name, absent, text, **kw)   # noqa: E731
    for arg in ("data", "tab", "table", "out"):
        bad("null pointer argument", **{arg: None})
    if "rrc" in recs:
        bad(NO_RRC, rrc=None)
    bad("downscaling is not supported", S=256)
    bad("source size 4 is outside 8", S=4)
    bad("output size 222 must be a multiple of 4", D=222)
    bad("at most 384", S=384, D=512)
    bad("batch 0 must be 1 .. 65535", B=0)
    bad("batch 65536 must be 1 .. 65535", B=65536, index=P)
    bad("(0 images) not empty", N=0)
    bad("batch 8 of a data set of 4 images needs an index", B=8, N=4)
    if "aug" in recs:
        bad("unknown padding_mode 2 (0 = constant, 1 = reflect)", mode=2)
        bad("unknown padding_mode -1", mode=-1)
        bad("fill 256 is outside 0 .. 255", fill=256)
        bad("fill -1 is outside 0 .. 255", fill=-1)
    for off in (4, 8, 12):
        bad("misaligned pointer", out=P + off)
    for arg in ["tab", "table"] + present:
        for off in (1, 2, 3):
            bad("misaligned pointer", **{arg: P + off})
    # the order of the rules: of two bad arguments the earlier rule's is reported
    bad("null pointer argument", data=None, S=4, **({"rrc": None} if "rrc" in recs else {}))
    if "rrc" in recs:
        bad("rrc is NULL", rrc=None, S=4)
    bad("source size 4 is outside 8", S=4, B=0)
    bad("batch 0 must be", B=0, out=P + 4)
    bad("needs an index", B=8, N=4, out=P + 4, **({"mode": 2} if "aug" in recs else {}))
    if "aug" in recs:
        bad("unknown padding_mode 2", mode=2, fill=256)
        bad("fill 256", fill=256, out=P + 4)


@pytest.mark.parametrize("name,absent", CASES, ids=IDS)
def test_the_lds_refusal(native_lib, name, absent):
    L = native_lib
    rrc, mixed, blur = "rrc" in ENTRIES[name], "mix" not in absent, "blur" not in absent
    assert _blur_lds(32, 224, True, True) == 60192 and _blur_lds(32, 224, True, False) <= 65536      # 32 -> 224 with mix is served
    for S, D in ((32, 224), (8, 36), (384, 384), (64, 256), (32, 384)):
        need = _blur_lds(S, D, mixed, rrc)
        if blur and need > 65536:
            err = _refused(L, name, absent, "bytes of LDS", S=S, D=D)
            clause = "two plane sets and three image buffers" if mixed else "a plane set and two image buffers"
            assert err == f"{name}: source {S} -> output {D} needs {need} bytes of LDS for {clause}, more than 65536"
        elif not blur and mixed and S >= 300:
            # blur == NULL: the colour entry's forms, refused under the narrowest sibling's name where two plane sets do not fit
            _refused(L, name, absent, "bytes of LDS for two plane sets", who=_sibling(name, absent), S=S, D=D)
        else:
            # no refusal for this form: the call would reach the launch, so the last rule of the argument check is made to stop it
            assert "LDS" not in _refused(L, name, absent, "misaligned pointer", S=S, D=D, out=P + 4)
    assert _blur_lds(384, 384, False, False) > 65536 and _blur_lds(32, 384, False, False) > 65536 and _blur_lds(64, 256, True, True) > 65536
    assert _blur_lds(64, 256, False, True) == 63280 and _blur_lds(32, 224, False, False) == 52096


def test_blur_ref_equals_pillows_bytes():
    f = blur_ref.load()
    below, above = (float(v) for v in f["step"])
    assert np.float32(above) == np.nextafter(np.float32(below), np.float32(2)) and blur_ref.weights(below)[0] == 0 and blur_ref.weights(above)[0] == 1
    n = 0
    for D in f["sizes"].tolist():
        radii = f[f"radii_{D}"]
        assert {0.5, 2.0} <= {round(float(r), 6) for r in radii}
        for k, (r, im) in enumerate(zip(radii, f[f"image_of_{D}"])):
            w = blur_ref.weights(r)
            assert list(w) == f[f"weights_{D}"][k].tolist()
            got = blur_ref.blur(f[f"images_{D}"][im], *w)
            assert np.array_equal(got, f[f"out_{D}"][k]), (D, k)
            n += 1
    assert {round(float(r), 6) for r in f["radii_36"]} >= {0.1, 0.5, 1.0, 2.0, round(below, 6), round(above, 6)}
    sp = f["special_images"]
    assert sp.shape[0] == 10 and not sp[0].any() and (sp[1] == 255).all() and all(np.count_nonzero(a.any(2)) == 1 for a in sp[2:])
    rows = sorted(int(np.argwhere(a.any(2))[0][0]) for a in sp[2:])
    assert rows == [0, 0, 7, 8, 15, 16, 35, 35]
    for i, a in enumerate(sp):
        for j, r in enumerate(f["special_radii"]):
            got = blur_ref.blur(a, *blur_ref.weights(r))
            assert np.array_equal(got, f["special_out"][i, j]), (i, j)
            if i < 2:
                assert np.array_equal(got, a)                        # a constant image stays what it is
            n += 1
    assert n >= 50


def test_known_weights_and_the_python_side_agree():
    for r, want in KNOWN.items():
        assert blur_ref.weights(r) == want and data.blur_weights(r) == want and blur_ref.pack(r) == [1 | want[0] << 8, want[1], want[2], 0]
    rng = np.random.default_rng(5)
    for r in rng.uniform(0.0, 2.44, 300).astype(np.float32):
        rad, ww, fw = data.blur_weights(r)
        assert (rad, ww, fw) == blur_ref.weights(r) and rad <= 1
        assert blur_ref.cleaned([1 | rad << 8, ww, fw, 0]) == (rad, ww, fw)                    # every record the host forms is valid
    assert data.blur_weights(0.0) == (0, 1 << 24, 0)                 # the identity


def test_the_cleaning_rule():
    good = blur_ref.pack(2.0)
    assert blur_ref.cleaned(good) == KNOWN[2.0]
    assert blur_ref.cleaned([good[0] | 0xFE | -(1 << 16)] + good[1:3] + [-1]) == KNOWN[2.0]       # stray bits of word 0, word 3: ignored
    for bad in ([good[0] & ~1] + good[1:],                          # bit 0 clear
                [1 | 2 << 8] + good[1:],                             # radius 2
                [1 | 255 << 8] + good[1:],
                [good[0], 0, good[2], 0],                            # ww = 0
                [good[0], -5, good[2], 0],
                [good[0], (1 << 24) + 1, 0, 0],                      # ww above 2^24
                [good[0], good[1], -1, 0],                           # fw negative
                [good[0], good[1], good[2] + 1, 0],                  # 3 * ww + 2 * fw = 2^24 + 2
                [1, 1 << 24, 1, 0],                                  # ww + 2 * fw = 2^24 + 2
                [1, 1, 0x7fffffff, 0],
                [0, 0, 0, 0]):
        assert blur_ref.cleaned(bad) is None, bad
    assert blur_ref.cleaned([1, 1 << 24, 0, 0]) == (0, 1 << 24, 0) and blur_ref.cleaned([1 | 1 << 8, 1, 0, 0]) == (1, 1, 0)
    # a cleaned record never overflows and never exceeds a byte: the extreme valid weights on the extreme image
    white = np.full((5, 7, 3), 255, np.uint8)
    for rec in ([1, 1 << 24, 0, 0], [1 | 1 << 8, 5592405, 0, 0], [1, 5592406, 5592405, 0], [1, 2, (1 << 23) - 1, 0]):
        assert np.array_equal(blur_ref.blur(white, *blur_ref.cleaned(rec)), white)
    # the composition with the colour record: split around the blur
    rec = color_ref.pack((color_ref.CONTRAST, color_ref.BRIGHTNESS), 1.5, 0.5, gray=True, solarize=77)
    front, back = blur_ref.split(rec)
    assert color_ref.unpack(front)[0] == (0, 0, 0) and color_ref.unpack(front)[1:4] == (True, True, 77)
    assert color_ref.unpack(back)[0] == (color_ref.CONTRAST, color_ref.BRIGHTNESS, 0) and color_ref.unpack(back)[1:3] == (False, False)
    img = np.random.default_rng(1).integers(0, 256, (12, 12, 3), dtype=np.uint8)
    assert np.array_equal(blur_ref.apply(img, rec, None)[0], color_ref.apply(img, rec)[0])       # no blur: the colour chain
    assert blur_ref.apply(img, rec, None)[1] == color_ref.apply(img, rec)[1]
    blurred, s = blur_ref.apply(img, rec, good)
    assert not np.array_equal(blurred, color_ref.apply(img, rec)[0]) and s != color_ref.apply(img, rec)[1]


def test_gaussian_blur_draws_by_the_stated_rule():
    b = qat_vit_amd.GaussianBlur(p=0.4, radius=(0.1, 2.0))
    g = torch.Generator().manual_seed(7)
    recs = b.draw(200, g)
    assert recs.dtype == torch.int32 and tuple(recs.shape) == (200, 4)
    g2 = torch.Generator().manual_seed(7)
    c, u = torch.rand(200, dtype=torch.float64, generator=g2), torch.rand(200, dtype=torch.float64, generator=g2)
    assert torch.equal(g.get_state(), g2.get_state())                # two draws, whatever the coin said
    on = (c < 0.4).tolist()
    assert 40 < sum(on) < 120
    for k in range(200):
        want = blur_ref.pack(np.float32(0.1 + float(u[k]) * (2.0 - 0.1))) if on[k] else blur_ref.NONE
        assert recs[k].tolist() == want, k
    assert {r[0] for r in recs.tolist()} == {0, 1, 1 | 1 << 8}        # none, box radius 0 and box radius 1 all occur
    assert torch.equal(recs, b.draw(200, torch.Generator().manual_seed(7)))
    for p, n_on in ((0.0, 0), (1.0, 50)):
        g3 = torch.Generator().manual_seed(9)
        r = qat_vit_amd.GaussianBlur(p=p).draw(50, g3)
        assert int((r[:, 0] & 1).sum()) == n_on
        g4 = torch.Generator().manual_seed(9)
        torch.rand(50, dtype=torch.float64, generator=g4), torch.rand(50, dtype=torch.float64, generator=g4)
        assert torch.equal(g3.get_state(), g4.get_state())           # the generator's position depends on n only
    assert qat_vit_amd.GaussianBlur(radius=1.0).draw(3, torch.Generator().manual_seed(1)).tolist() == [blur_ref.pack(1.0)] * 3


def test_radius_ranges_and_refusals():
    for bad in ((0.1, 2.45), (0.1, 3.0), 2.5, (1.0, 100.0)):
        with pytest.raises(ValueError, match=r"box radii up to 1, which is a Gaussian radius below sqrt\(6\)"):
            qat_vit_amd.GaussianBlur(radius=bad)
        with pytest.raises(ValueError, match=r"sqrt\(6\)"):
            qat_vit_amd.ThreeAugment(radius=bad)
    assert qat_vit_amd.GaussianBlur(radius=(0.1, 2.44)).radius == (0.1, 2.44)
    for bad in ((2.0, 0.1), (-0.1, 1.0), "1", (0.1, float("inf")), (0.1, 1.0, 2.0), True):
        with pytest.raises(ValueError, match="radius must be"):
            qat_vit_amd.GaussianBlur(radius=bad)
    for bad in (-0.1, 1.5, "0.5", True):
        with pytest.raises(ValueError, match="p must be a probability"):
            qat_vit_amd.GaussianBlur(p=bad)
    with pytest.raises(ValueError, match="solarize_threshold"):
        qat_vit_amd.ThreeAugment(solarize_threshold=256)


def test_three_augment_picks_exactly_one_of_three():
    t = qat_vit_amd.ThreeAugment(color_jitter=0.3, radius=(0.1, 2.0), solarize_threshold=100)
    g = torch.Generator().manual_seed(11)
    col, blur = t.draw(300, g)
    assert col.dtype == blur.dtype == torch.int32 and tuple(col.shape) == tuple(blur.shape) == (300, 4)
    gray, sol, on = (col[:, 0] >> 8 & 1), (col[:, 0] >> 9 & 1), (blur[:, 0] & 1)
    assert bool(((gray + sol + on) == 1).all())                      # exactly one of the three per sample
    assert min(int(gray.sum()), int(sol.sum()), int(on.sum())) > 60   # all three occur, about a third each
    assert bool(((col[:, 0] >> 16 & 255) == sol * 100).all())
    for k in range(300):
        rec = blur[k].tolist()
        assert (rec == blur_ref.NONE) if not on[k] else (blur_ref.cleaned(rec) is not None and rec[3] == 0)
    # the jitter part: ColorJitter(0.3, 0.3, 0.3)'s records of the same generator, all three ops in a random order; then the choice and the radius
    g2 = torch.Generator().manual_seed(11)
    jit = qat_vit_amd.ColorJitter(0.3, 0.3, 0.3).draw(300, g2)
    c, u = torch.rand(300, dtype=torch.float64, generator=g2), torch.rand(300, dtype=torch.float64, generator=g2)
    assert torch.equal(g.get_state(), g2.get_state())
    assert torch.equal(col[:, 1:], jit[:, 1:]) and torch.equal(col[:, 0] & 0x3F, jit[:, 0] & 0x3F) and bool(((jit[:, 0] >> 6) == 0).all())
    assert len({tuple(r) for r in (col[:, 0] & 0x3F).tolist() for r in [(r & 3, r >> 2 & 3, r >> 4 & 3)]}) == 6
    choice = (3.0 * c).floor().clamp(max=2).to(torch.int64)
    assert torch.equal(choice == 0, gray.bool()) and torch.equal(choice == 1, sol.bool()) and torch.equal(choice == 2, on.bool())
    k = int(torch.nonzero(on)[0])
    assert blur[k].tolist() == blur_ref.pack(np.float32(0.1 + float(u[k]) * 1.9))
    assert t.contrast is not None and qat_vit_amd.ThreeAugment(color_jitter=0).contrast is None


class _Recorder:
    """A stand-in transform: keeps what the loader hands to every call."""
    device, out_size = torch.device("cpu"), 36

    def __init__(self):
        self.calls = []

    def __call__(self, images, index, **kw):
        self.calls.append({k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in dict(kw, index=index).items()})
        return torch.zeros(index.shape[0], 3, 1, 1)


def _epoch(monkeypatch, **kw):
    empty = torch.empty
    monkeypatch.setattr(torch, "empty", lambda *a, pin_memory=False, **k: empty(*a, **k))       # no accelerator here: the block is not pinned
    rng = np.random.default_rng(3)
    imgs, labels = rng.integers(0, 256, (20, 8, 8, 3), dtype=np.uint8), rng.integers(0, 10, 20)
    tr = _Recorder()
    loader = qat_vit_amd.GpuImageLoader(imgs, labels, 8, shuffle=True, generator=torch.Generator().manual_seed(12), transform=tr, **kw)
    assert len(list(loader)) == 3
    return tr.calls


@pytest.mark.parametrize("crop", [False, True], ids=["augment", "crop"])
def test_loader_draws_the_blur_records_last(monkeypatch, crop):
    front = {"crop": qat_vit_amd.RandomResizedCrop()} if crop else {"augment": qat_vit_amd.RandomCropFlip(2)}
    base = dict(mix=qat_vit_amd.MixupCutmix(mode="elem"), erase=qat_vit_amd.RandomErasing(p=0.6), color=qat_vit_amd.ColorJitter(0.4, 0.4, 0.4, grayscale=0.2),
                **front)
    b = qat_vit_amd.GaussianBlur(p=0.5)
    old, new = _epoch(monkeypatch, **base), _epoch(monkeypatch, blur=b, **base)
    seen = []
    for o, n in zip(old, new):
        assert o["blur"] is None and n["blur"].dtype == torch.int32 and tuple(n["blur"].shape) == (o["index"].shape[0], 4)
        for key in o:
            if key != "blur":                                        # the plan, words / windows, mix, erase and colour records of the seed stay
                assert torch.equal(o[key], n[key]) if isinstance(o[key], torch.Tensor) else o[key] == n[key], key
        seen.append(n["blur"])
    # drawn last: the generator behind everything else gives exactly these records
    g = torch.Generator().manual_seed(12)
    plan = qat_vit_amd.epoch_batches(20, 8, shuffle=True, generator=g)
    front["crop"].draw(20, 8, g) if crop else front["augment"].draw(20, g)
    base["mix"].draw([len(p) for p in plan], 36, g), base["erase"].draw(20, 36, g), base["color"].draw(20, g)
    assert torch.equal(torch.cat(seen), b.draw(20, g)) and 0 < int((torch.cat(seen)[:, 0] & 1).sum()) < 20
    # three_augment: the colour and the blur records of one draw, where they stand; exclusive with color and blur
    t = qat_vit_amd.ThreeAugment()
    calls = _epoch(monkeypatch, three_augment=t, mix=base["mix"], erase=base["erase"], **front)
    g = torch.Generator().manual_seed(12)
    plan = qat_vit_amd.epoch_batches(20, 8, shuffle=True, generator=g)
    front["crop"].draw(20, 8, g) if crop else front["augment"].draw(20, g)
    base["mix"].draw([len(p) for p in plan], 36, g), base["erase"].draw(20, 36, g)
    col, blur = t.draw(20, g)
    assert torch.equal(torch.cat([c["color"] for c in calls]), col) and torch.equal(torch.cat([c["blur"] for c in calls]), blur)
    assert all(c["contrast"] is True and torch.equal(c["mix"], o["mix"]) and torch.equal(c["erase"], o["erase"]) for c, o in zip(calls, old))
    alone = _epoch(monkeypatch, blur=b)                              # blur alone: no colour records, no workspace
    assert all(c["color"] is None and c["erase"] is None and c["mix"] is None and c["contrast"] is False and c["blur"] is not None for c in alone)
    for kw in ({"color": base["color"]}, {"blur": b}):
        with pytest.raises(ValueError, match="three_augment is exclusive with color and blur"):
            qat_vit_amd.GpuImageLoader(np.zeros((4, 8, 8, 3), np.uint8), np.zeros(4, np.int64), 2, transform=_Recorder(), three_augment=t, **kw)
    for kw, text in (({"blur": "blur"}, "blur must be a GaussianBlur"), ({"three_augment": b}, "three_augment must be a ThreeAugment")):
        with pytest.raises(TypeError, match=text):
            qat_vit_amd.GpuImageLoader(np.zeros((4, 8, 8, 3), np.uint8), np.zeros(4, np.int64), 2, transform=_Recorder(), **kw)


def test_wrapper_refusals_without_a_gpu():
    tr = object.__new__(qat_vit_amd.GpuResizeNormalize)               # the constructor needs the GPU; this refusal does not
    tr.src_size, tr.out_size, tr.device = 32, 224, torch.device("cuda", 0)
    imgs, recs = torch.zeros(2, 32, 32, 3, dtype=torch.uint8), torch.zeros(2, 4, dtype=torch.int32)
    for kw in ({}, {"color": recs}, {"rrc": torch.zeros(2, 2, dtype=torch.int32)}):
        with pytest.raises(RuntimeError, match="move the uint8 images to the GPU"):
            tr(imgs, blur=recs, **kw)
