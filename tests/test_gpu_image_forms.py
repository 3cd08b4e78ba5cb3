"""The form table of the input pipeline on an MI355X: the records present decide the kernel, whichever of the eight qatvit_image_batch* entries
carries them.  For every set of records, every entry that accepts the set (a wider entry with the records it has beyond the set passed as NULL)
writes the same bits into `out` and, with a workspace, into `sums` as the narrowest one.  What the kernels compute is held to the host references
by the other test_gpu_* files of the pipeline; this file compares the entries with each other, without a tolerance."""
import itertools

import pytest
import torch

import qat_vit_amd
from qat_vit_amd import native
from tests import augment_ref, erase_ref, mix_ref, rrc_ref
from tests.color_ref import BRIGHTNESS as BR, CONTRAST as CO, SATURATION as SA, pack
from tests.test_image_request_abi import ENTRIES, PRE

pytestmark = pytest.mark.gpu

B, N, INDEX = 3, 3, [2, 0, 2]
MODE, FILL = 0, 131


def _records(s, d):
    """Device tensors, one record per batch position: the mix partners form the cycle 0 -> 1 -> 2 -> 0, with one box and two blends."""
    box = (3, d - 7, 5, d - 3)
    host = {
        "aug": [augment_ref.pack(2, -3, True), augment_ref.pack(-1, 2, False), augment_ref.pack(0, 1, True)],
        "rrc": [rrc_ref.pack(1, 2, s - 3, s - 2, True), rrc_ref.pack(0, 0, s, s, False), rrc_ref.pack(s - 5, 0, 5, s, True)],
        "mix": [mix_ref.mixup(1, 0.3), mix_ref.cutmix(2, box, d), mix_ref.mixup(0, 0.75)],
        "erase": [erase_ref.pack(*box, (0.5, -0.5, 2.0)), erase_ref.pack(14, 18, 6, 10, (1.0, 1.0, 1.0), mode=1, key=(123, 456)),
                  erase_ref.pack(0, d, 0, 7, (-1.0, -2.0, -3.0))],
        "color": [pack((CO, BR, SA), 1.3, 1.7, 0.4), pack((SA, CO), contrast=0.5, saturation=1.8, solarize=100), pack((BR,), 0.6, gray=True)],
    }
    return {k: torch.tensor(v, dtype=torch.int32).cuda() for k, v in host.items()}


def _call(tr, src, index, recs, name, given):
    """(out, sums) of entry `name` with the records in `given`; its other record arguments are NULL.  Both buffers are poisoned before the call."""
    s, d = tr.src_size, tr.out_size
    out = torch.full((B, 3, d, d), float("nan"), device="cuda")
    sums = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    ptr = lambda r: (sums if r == "sums" else recs[r]).data_ptr() if r in given else None   # noqa: E731
    tail = []
    for r in ENTRIES[name]:
        tail += [ptr(r), MODE, FILL] if r == "aug" else [ptr(r)]
    tab = tr.window_tables() if "rrc" in ENTRIES[name] else tr.coeffs
    native.check(getattr(native.lib(), name)(src.data_ptr(), index.data_ptr(), B, N, s, d, tab.data_ptr(), tr.table.data_ptr(), *tail, out.data_ptr(),
                                             native.stream_ptr()), name)
    return out.view(torch.int32).cpu(), sums.cpu()


@pytest.mark.parametrize("s,d", [(8, 36), (32, 224)])                # D = 36: two bands of 16 rows and one of 4, DT = 0; D = 224: the constant-D kernels
def test_every_entry_that_accepts_a_record_set_writes_the_same_bits(s, d):
    tr = qat_vit_amd.GpuResizeNormalize(s, out_size=d)
    src = torch.randint(0, 256, (N, s, s, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(s)).cuda()
    index, recs = torch.tensor(INDEX).cuda(), _records(s, d)
    seen = {}
    for family in ("aug", "rrc"):
        optional = ["mix", "erase", "color", "sums"] + (["aug"] if family == "aug" else [])
        for k in range(len(optional) + 1):
            for chosen in itertools.combinations(optional, k):
                given = set(chosen) | ({"rrc"} if family == "rrc" else set())
                if "sums" in given and "color" not in given:
                    continue                                          # a workspace without colour records is not a record set of its own
                accept = [n for n, r in ENTRIES.items() if given <= set(r) and ("rrc" in r) == (family == "rrc")]
                assert accept and (len(accept) > 1 or "color" in given), given
                out0, sums0 = _call(tr, src, index, recs, accept[0], given)      # ENTRIES lists the narrower entry first
                assert not bool((out0 == torch.tensor(float("nan")).view(torch.int32)).any()), (accept[0], given)
                for name in accept[1:]:
                    out, sums = _call(tr, src, index, recs, name, given)
                    assert torch.equal(out, out0), (name, accept[0], sorted(given))
                    assert torch.equal(sums, sums0), (name, accept[0], sorted(given))
                # the workspace is written with colour records and a workspace, where the record holds a contrast op, and never otherwise
                assert sums0.tolist() == [-1] * B if "sums" not in given else sums0[0] > 0 and sums0[1] > 0 and sums0[2] == 0, sorted(given)
                seen[frozenset(given)] = out0
    # the records are not trivial: no two record sets give the same batch
    assert len(seen) == 24 + 12
    for (ga, a), (gb, b) in itertools.combinations(seen.items(), 2):
        assert not torch.equal(a, b), (sorted(ga), sorted(gb))
    assert PRE in ENTRIES and len(ENTRIES) == 8
