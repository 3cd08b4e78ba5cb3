"""The argument errors of the nine optimizer entries (optim.hip, lamb.hip), as whole strings: a fixed list of bad calls is replayed and every
``qatvit_last_error()`` text and return code must equal tests/golden/optim_error_texts.json, which tools/gen_optim_error_texts.py recorded from
the library as it was before the entries shared their checks (csrc/qv_optim.h).  The ABI tests of these entries look at substrings; this one
holds the texts byte for byte, and - with the calls that have two things wrong - the order of the checks: pointers, chunking, n_groups, the rows
in ascending order, the decay.

No GPU and no HIP call: every call in the list has at least one invalid argument, so each returns before anything is launched (the convention
of tests/test_optim_*_abi.py; the stand-in pointer is never dereferenced)."""
import json
import math
import os

from qat_vit_amd import native

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "optim_error_texts.json")
P = 4096   # a non-null stand-in
ADAM_ROW = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=0.01, step=1)
HYPER = tuple(ADAM_ROW.items())
_TABLES = ("numel", "ct", "ci")

# per entry: its parameters in order with a valid value each (`groups` / `n_groups` are filled in from `rows`), and which pointers may be null
ENTRIES = {
    "qatvit_optim_grad_norm": ((("grads", P),) + tuple((n, P) for n in _TABLES) + (("n_chunks", 3), ("chunk", 16384), ("max_norm", 1.0), ("partials", P),
                                ("out2", P), ("stream", None)), ()),
    "qatvit_optim_adamw": (tuple((n, P) for n in ("params", "grads", "m", "v") + _TABLES) + (("n_chunks", 3), ("chunk", 16384)) + HYPER +
                           (("clip", P), ("stream", None)), ("clip",)),
    "qatvit_optim_adamw_groups": (tuple((n, P) for n in ("params", "grads", "m", "v", "numel", "tg", "ct", "ci")) +
                                  (("n_chunks", 3), ("chunk", 16384), ("groups", None), ("n_groups", None), ("clip", P), ("stream", None)), ("clip",)),
    "qatvit_optim_adamw_ema": (tuple((n, P) for n in ("params", "grads", "m", "v", "ema") + _TABLES) + (("n_chunks", 3), ("chunk", 16384)) + HYPER +
                               (("decay", 0.99), ("clip", P), ("stream", None)), ("clip",)),
    "qatvit_optim_adamw_groups_ema": (tuple((n, P) for n in ("params", "grads", "m", "v", "ema", "numel", "tg", "ct", "ci")) +
                                      (("n_chunks", 3), ("chunk", 16384), ("groups", None), ("n_groups", None), ("decay", 0.99), ("clip", P),
                                       ("stream", None)), ("clip",)),
    "qatvit_optim_ema": (tuple((n, P) for n in ("params", "ema") + _TABLES) + (("n_chunks", 3), ("chunk", 16384), ("decay", 0.99), ("stream", None)), ()),
    "qatvit_optim_swap": (tuple((n, P) for n in ("a", "b") + _TABLES) + (("n_chunks", 3), ("chunk", 16384), ("stream", None)), ()),
    "qatvit_optim_lamb_moments": (tuple((n, P) for n in ("params", "grads", "m", "v", "numel", "tg", "ct", "ci")) +
                                  (("n_chunks", 3), ("chunk", 16384), ("groups", None), ("n_groups", None), ("clip", P), ("partials", P),
                                   ("stream", None)), ("clip",)),
    "qatvit_optim_lamb_apply": (tuple((n, P) for n in ("params", "m", "v", "ema", "numel", "tg", "first", "ct", "ci")) +
                                (("n_chunks", 3), ("chunk", 16384), ("groups", None), ("n_groups", None), ("decay", 0.99), ("partials", P), ("trust", P),
                                 ("stream", None)), ("ema", "trust")),
}
BAD_CHUNKING = (dict(n_chunks=0), dict(n_chunks=-3), dict(chunk=0), dict(chunk=-4), dict(chunk=16382))
BAD_HYPER = (dict(step=0), dict(step=-2), dict(lr=-1e-3), dict(b1=1.0), dict(b1=-0.1), dict(b2=1.0), dict(b2=-0.5), dict(eps=-1e-8), dict(lr=math.nan),
             dict(b2=math.nan))
BAD_DECAY = (-0.1, 1.0, 2.0, math.nan)


def _is_lamb(entry):
    return "lamb" in entry


def _has(entry, name):
    return any(n == name for n, _ in ENTRIES[entry][0])


def _tag(kw):
    return ",".join(f"{k}={v}" for k, v in kw.items())


def bad_calls():
    """[(id, entry, overrides)]: `overrides` replaces the valid value of a parameter; ``rows`` = a tuple of per-group overrides of ADAM_ROW."""
    out = []
    for entry, (params, nullable) in ENTRIES.items():
        grouped, one_group = _has(entry, "groups"), _has(entry, "lr")
        add = lambda what, **kw: out.append((f"{entry}/{what}", entry, kw))   # noqa: E731
        for name, value in params:
            if value == P and name not in nullable:
                add(f"null/{name}", **{name: None})
        if grouped:
            add("null/groups", groups=None)
        for name in nullable:   # allowed to be null: the text names the other thing that is wrong
            add(f"nullable/{name}", **{name: None, "n_chunks": 0})
        for kw in BAD_CHUNKING:
            add(f"chunking/{_tag(kw)}", **kw)
        if grouped:
            for n in (0, -1, 65):
                add(f"n_groups/{n}", rows=({},) * max(n, 1), n_groups=n)
            for kw in BAD_HYPER + (dict(wd=-0.01), dict(wd=math.nan)):
                add(f"row0/{_tag(kw)}", rows=(kw, {}))
                add(f"row1/{_tag(kw)}", rows=({}, kw))
            add("order/row0_before_row1", rows=(dict(lr=-1.0), dict(step=0)))
            add("order/n_groups_before_rows", rows=(dict(step=0),), n_groups=0)
            add("order/chunking_before_n_groups", chunk=2, n_groups=0)
        if one_group:
            for kw in BAD_HYPER:
                add(f"hyper/{_tag(kw)}", **kw)
            add("hyper/weight_decay_is_not_looked_at", wd=-0.01, step=0)
            add("order/chunking_before_hyper", n_chunks=0, lr=-1.0)
        if _has(entry, "decay"):
            for d in BAD_DECAY:
                add(f"decay/{d}", decay=d)
            if grouped:
                add("order/rows_before_decay", rows=({}, dict(eps=-1.0)), decay=1.5)
            elif one_group:
                add("order/hyper_before_decay", b1=1.0, decay=1.5)
            else:
                add("order/chunking_before_decay", chunk=6, decay=1.5)
        add("order/null_before_chunking", numel=None, n_chunks=0)
    out.append(("qatvit_optim_lamb_apply/decay_not_looked_at_without_averages", "qatvit_optim_lamb_apply", dict(ema=None, decay=math.nan, chunk=0)))
    return out


def replay(L, entry, overrides):
    """(return code, qatvit_last_error() as str) of one call of the list."""
    kw = dict(overrides)
    rows = kw.pop("rows", ({}, {}))
    row_t, extra = (native.LambGroup, (1, 0, 0, 0)) if _is_lamb(entry) else (native.AdamWGroup, ())
    groups = (row_t * len(rows))(*[tuple({**ADAM_ROW, **r}.values()) + extra for r in rows])   # kept alive until the call returns
    args = []
    for name, value in ENTRIES[entry][0]:
        if name == "groups":
            value = groups
        elif name == "n_groups":
            value = len(rows)
        args.append(kw.pop(name, value))
    assert not kw, (entry, kw)
    rc = getattr(L, entry)(*args)
    return rc, L.qatvit_last_error().decode()


def test_error_texts_are_the_recorded_ones(native_lib):
    golden = {f"{entry}/{what}": v for entry, d in json.load(open(GOLDEN)).items() for what, v in d.items()}   # {entry: {what: [code, text]}}
    calls = bad_calls()
    assert sorted(c[0] for c in calls) == sorted(golden) and len(calls) == len(golden), "the list of calls and the fixture differ: tools/gen_optim_error_texts.py"
    assert {c[1] for c in calls} == set(ENTRIES) and len(ENTRIES) == 9
    for cid, entry, overrides in calls:
        rc, text = replay(native_lib, entry, overrides)
        assert rc == 1 and text.startswith(entry + ": "), (cid, rc, text)   # an argument error: nothing was launched
        assert [rc, text] == golden[cid], cid
