#!/usr/bin/env python3
"""One line per compiled gfx950 function of libqatvit:  symbol sha256 vgpr sgpr lds scratch   (under a `# file.hip` line per source file)

    python tools/isa_digest.py                 # compile every SRCS entry of csrc/Makefile (its flags + --cuda-device-only -S), digest
    python tools/isa_digest.py --csrc DIR      # the same for another checkout's csrc directory (e.g. the parent commit's)
    python tools/isa_digest.py a.s b.s         # digest device assembly that exists already

Needs no GPU.  Two trees generate the same machine code exactly when their listings are equal (diff them): the sha256 covers the function's
instruction stream (labels and directives included; comments, .file / .loc / .ident lines and blank lines dropped) and, for a kernel, every
line of its .amdhsa_kernel descriptor - so the AGPR split (accum_offset), the user-SGPR layout and the like are compared too, not only
the four printed resource figures.  A device function that is not a kernel has `-` in the resource columns.  Lines are sorted by symbol
within a file; the __hip_cuid_* marker object (a hash of the source path) is not code and is ignored.
"""
import argparse
import hashlib
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
DROP = re.compile(r"^\s*\.(file|loc|ident|cfi_\w+)\b")


def clean(line):
    line = line.split(";", 1)[0].rstrip()
    return None if not line.strip() or DROP.match(line) else line


def digest(path):
    lines = open(path).read().split("\n")
    funcs = [m.group(1) for l in lines if (m := re.match(r"\s*\.type\s+(\S+),@function", l))]
    meta = {}   # amdgpu_metadata: one `  - .key: value` list entry per kernel, its own keys at four spaces
    for chunk in re.split(r"^  - ", "\n".join(lines), flags=re.M)[1:]:
        e = dict(re.findall(r"^(?:    )?\.(\w+):\s+(\S+)$", chunk, re.M))
        if "name" in e: meta[e["name"]] = e
    out = []
    for f in funcs:
        start = lines.index(next(l for l in lines if l.startswith(f + ":")))
        body, i = [], start
        while not re.match(r"\.Lfunc_end\d+:", lines[i]):
            body.append(lines[i])
            i += 1
        h = hashlib.sha256("\n".join(c for c in map(clean, body) if c is not None).encode())
        k = meta.get(f)
        cols = [k["vgpr_count"], k["sgpr_count"], k["group_segment_fixed_size"], k["private_segment_fixed_size"]] if k else ["-"] * 4
        out.append(" ".join([f, h.hexdigest()] + cols))
    return sorted(out)


def compile_all(csrc, outdir):
    mk = open(os.path.join(csrc, "Makefile")).read()
    var = lambda n: re.search(r"^%s\s*\??=\s*(.*)$" % n, mk, re.M).group(1).strip()
    flags = var("CXXFLAGS").replace("$(ARCH)", os.environ.get("ARCH", var("ARCH"))).replace("$(EXTRA)", os.environ.get("EXTRA", ""))
    hipcc = os.environ.get("HIPCC", var("HIPCC"))

    def one(src):
        dst = os.path.join(outdir, src[:-4] + ".s")
        subprocess.run([hipcc] + flags.split() + ["--cuda-device-only", "-S", src, "-o", dst], cwd=csrc, check=True, stderr=subprocess.DEVNULL)
        return dst

    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as ex:
        return list(ex.map(one, var("SRCS").split()))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--csrc", default=os.path.join(HERE, "..", "qat-vit_amd", "csrc"))
    ap.add_argument("asm", nargs="*")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        for path in a.asm or compile_all(a.csrc, tmp):
            print("# " + os.path.basename(path)[:-2] + ".hip")
            for line in digest(path): print(line)


if __name__ == "__main__":
    sys.exit(main())
