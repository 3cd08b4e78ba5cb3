"""CPU-side checks of the one argument check and the one form table behind the eight qatvit_image_batch* entries: the same refusal matrix for
every entry and every subset of its optional record pointers set to NULL.  Every call here ends in an error string before any HIP call: a rule of
the argument check refuses it under the name of the entry that was called, or the form's LDS request is refused under the name of the narrowest
entry that serves the records present.  The stand-in pointer is never dereferenced."""
import itertools
import os
import re

import pytest

from qat_vit_amd import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 4096                                                             # non-null, 4096-aligned
PRE = "qatvit_image_batch"
# entry -> its record arguments, in the order of its signature between `table` and `out` (aug stands for aug, padding_mode, fill)
ENTRIES = {
    PRE: (),
    PRE + "_aug": ("aug",),
    PRE + "_mix": ("aug", "mix"),
    PRE + "_erase": ("aug", "mix", "erase"),
    PRE + "_color": ("aug", "mix", "erase", "color", "sums"),
    PRE + "_rrc": ("rrc", "mix"),
    PRE + "_rrc_erase": ("rrc", "mix", "erase"),
    PRE + "_rrc_color": ("rrc", "mix", "erase", "color", "sums"),
}
NO_RRC = {
    PRE + "_rrc": "rrc is NULL (the call without records is qatvit_image_batch or qatvit_image_batch_mix)",
    PRE + "_rrc_erase": "rrc is NULL (the call without window records is qatvit_image_batch_erase)",
    PRE + "_rrc_color": "rrc is NULL (the call without window records is qatvit_image_batch_color)",
}
CASES = [(name, frozenset(absent)) for name, recs in ENTRIES.items() for opt in [[r for r in recs if r != "rrc"]]
         for k in range(len(opt) + 1) for absent in itertools.combinations(opt, k)]


def _call(L, name, absent=(), **kw):
    """The entry's return value and its error string; the records in `absent` are NULL, every other argument is valid unless `kw` says otherwise."""
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


def _lds(S, D, mixed, rrc):
    """The form's LDS request as DESIGN.md states it: the tables, the source rows of a band, one plane set or two; the window forms add, on the next
    16 bytes, a band of the row table per side."""
    rows = (16 * S + D - 1) // D + 5
    base = D * 5 * 4 + 768 * 4 + ((rows * S * 3 + 15) & ~15) + (2 if mixed else 1) * rows * 3 * D
    return ((base + 15) & ~15) + (2 if mixed else 1) * 16 * 5 * 4 if rrc else base


def _narrowest(name, absent):
    """The narrowest entry that serves the records of (entry, subset)."""
    recs = set(ENTRIES[name]) - absent
    level = "_color" if "color" in recs else "_erase" if "erase" in recs else ""
    if "rrc" in recs:
        return PRE + "_rrc" + level
    return PRE + (level or ("_mix" if "mix" in recs else "_aug" if "aug" in recs else ""))


def test_the_matrix_covers_every_entry_and_every_subset():
    assert len(CASES) == 1 + 2 + 4 + 8 + 32 + 2 + 4 + 16
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "qatvit.h")).read(), flags=re.S)
    for name, recs in ENTRIES.items():
        params = [p.split()[-1].lstrip("*") for p in re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, hdr).group(1).split(",")]
        want = ["data", "index", "B", "N", "S", "D", "windows" if "rrc" in recs else "coeffs", "table"]
        for r in recs:
            want += ["aug", "padding_mode", "fill"] if r == "aug" else [r]
        assert params == want + ["out", "stream"], name
        assert len(native.SIGNATURES[name][1]) == len(params)
        # the padding and fill rules exist exactly where the entry has such arguments: not in the plain entry, not in the window family
        assert ("padding_mode" in params) == ("fill" in params) == ("aug" in recs)


@pytest.mark.parametrize("name,absent", CASES, ids=[n[len(PRE):].lstrip("_") + "-" + "".join(sorted(r[0] for r in a)) for n, a in CASES])
def test_every_rule_refuses_under_the_called_name(native_lib, name, absent):
    L, recs = native_lib, ENTRIES[name]
    present = [r for r in recs if r not in absent]
    bad = lambda text, **kw: _refused(L, name, absent, text, **kw)   # noqa: E731
    for arg in ("data", "tab", "table", "out"):
        bad("null pointer argument", **{arg: None})
    if "rrc" in recs:
        bad(NO_RRC[name], rrc=None)
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


@pytest.mark.parametrize("name,absent", CASES, ids=[n[len(PRE):].lstrip("_") + "-" + "".join(sorted(r[0] for r in a)) for n, a in CASES])
def test_the_lds_refusal_names_the_narrowest_entry(native_lib, name, absent):
    L = native_lib
    rrc, mixed = "rrc" in ENTRIES[name], "mix" in set(ENTRIES[name]) - absent
    for S, D in ((384, 384), (300, 384), (8, 36)):
        need = _lds(S, D, mixed, rrc)
        # two plane sets of the two large sources exceed 64 KB, one plane set of any source the entries accept does not
        assert (need > 65536) == (mixed and S >= 300)
        if need > 65536:
            who = _narrowest(name, absent)
            err = _refused(L, name, absent, "bytes of LDS", who=who, S=S, D=D)
            assert err == f"{who}: source {S} -> output {D} needs {need} bytes of LDS for two plane sets, more than 65536"
        else:
            # no refusal for this form: the call would reach the launch, so the last rule of the argument check is made to stop it
            err = _refused(L, name, absent, "misaligned pointer", S=S, D=D, out=P + 4)
            assert "LDS" not in err
    # the window forms without mix records are checked too, and their text has no plane-set clause; no shape that the entries accept gets there
    assert _lds(384, 384, False, True) == 59456
