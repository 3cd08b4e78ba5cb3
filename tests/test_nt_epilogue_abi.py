"""CPU-side checks of the NT epilogue numbers outside callers depend on: qatvit_i8_strip refuses a mode it does not take as a string, before any
HIP call, and include/qatvit.h still documents the three it takes (3 / 4 / 7 = kEpiStats / kEpiCodes / kEpiQkvCodes of csrc/qv_kernels.h)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_i8_strip_refuses_other_modes_without_a_gpu(native_lib):
    L = native_lib
    p = 4096   # a non-null stand-in for the five required pointers; never dereferenced: the call returns at the argument check
    for mode in (5, 0):
        rc = L.qatvit_i8_strip(mode, p, p, p, p, 128, 208, 1152, 384, 384, p, None, None, None, None, None, 0, 255, None, None, 197, None, None, None, None)
        assert rc != 0
        err = L.qatvit_last_error()
        assert b"qatvit_i8_strip: mode %d " % mode in err, err


def test_header_documents_the_three_strip_modes():
    text = open(os.path.join(ROOT, "include", "qatvit.h")).read()
    decl = text.index("int qatvit_i8_strip(int32_t mode")
    comment = text[text.rindex("/*", 0, decl):decl]
    assert comment.rstrip().endswith("*/")
    documented = sorted(int(m) for m in re.findall(r"^\s*\*\s+mode (\d+):", comment, flags=re.M))
    assert documented == [3, 4, 7], documented
    para = {int(m.group(1)): m.group(2) for m in re.finditer(r"^\s*\*\s+mode (\d+):(.*?)(?=^\s*\*\s+mode \d+:|^ \* K = )", comment, flags=re.M | re.S)}
    assert "min / max" in para[3] and "nothing is stored" in para[3]
    assert "attention" in para[7] and "out8_mask" in para[7]
    assert "row-major" in para[4] and "lut_out" in para[4]
