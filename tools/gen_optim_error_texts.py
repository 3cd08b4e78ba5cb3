#!/usr/bin/env python3
"""Writes tests/golden/optim_error_texts.json: for every bad call of tests/test_optim_error_texts.py (bad_calls(): all nine optimizer entries,
each with at least one invalid argument, so nothing is launched and no GPU is needed) the return code and the whole ``qatvit_last_error()`` text.

The fixture is the record of what the entries said BEFORE they shared their argument checks (csrc/qv_optim.h), so it must be written from the
PARENT of that change: build that commit in a checkout of its own and pass its library,

    python tools/gen_optim_error_texts.py --lib <parent checkout>/qat-vit_amd/libqatvit.so

(the entries' signatures did not change, so this tree's native.py binds it).  Without --lib the library of this tree is used: on a tree that
keeps the texts, that rewrites the committed file byte for byte - `git diff --exit-code tests/golden/optim_error_texts.json` is the check.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import qat_vit_amd  # noqa: E402,F401
from qat_vit_amd import native  # noqa: E402
from tests.test_optim_error_texts import GOLDEN, bad_calls, replay  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lib", help="libqatvit.so to record from (default: this tree's)")
    a = ap.parse_args()
    if a.lib:
        native.LIB_PATH = os.path.abspath(a.lib)
    L = native.lib()
    out, n = {}, 0
    for cid, entry, overrides in bad_calls():
        what = cid[len(entry) + 1:]
        assert cid.startswith(entry + "/") and what not in out.setdefault(entry, {}), cid
        rc, text = replay(L, entry, overrides)
        assert rc == 1, f"{cid}: returned {rc} ({text!r}): every call of the list must be an argument error"
        out[entry][what] = [rc, text]
        n += 1
    with open(GOLDEN, "w") as f:   # {entry: {what: [return code, text]}}, one call per line
        f.write("{\n" + ",\n".join(json.dumps(e) + ": {\n" + ",\n".join(f" {json.dumps(w)}: {json.dumps(v)}" for w, v in d.items()) + "\n}"
                                   for e, d in out.items()) + "\n}\n")
    print(f"{GOLDEN}: {n} calls, {os.path.getsize(GOLDEN)} bytes")


if __name__ == "__main__":
    main()
