"""The host logic of the one-plane backward's overflow protocol (qat_vit_amd.engine: mirror_wait, store_agree) without the native library or a GPU:
the mirror is a NumPy array this test writes, the key-value store a HashStore (a FileStore where this torch has none) shared by four threads."""
import threading

import numpy as np
import torch.distributed as dist

from qat_vit_amd.engine import mirror_wait, store_agree


def test_generation_compare_with_wrap_around():
    m = np.zeros(2, dtype=np.int32)          # {flag, generation}, as the device writes it

    def put(flag, gen):
        m[0], m[1] = flag, np.array(gen & 0xffffffff, dtype=np.uint32).astype(np.int32)

    for flag in (0, 1):
        for want in (5, 0x7fffffff, 0x80000000, 0xffffffff, 0, 0x100000000, 0x100000005):   # (the issued count is a Python int: it is taken mod 2^32)
            put(flag, want - 1)              # behind: the flag is not this call's yet - the limit runs out, not ten seconds
            assert mirror_wait(m, want, limit=0.01) is None, (flag, want)
            put(flag, want)                  # equal
            assert mirror_wait(m, want) is bool(flag), (flag, want)
            put(flag, want + 3)              # ahead (a later call already wrote): the latest flag
            assert mirror_wait(m, want) is bool(flag), (flag, want)
    # the 32-bit wrap: the call issued as 0xffffffff, then the next one as 0 (2^32)
    put(1, 0xfffffffe)
    assert mirror_wait(m, 0xffffffff, limit=0.01) is None
    put(1, 0xffffffff)
    assert mirror_wait(m, 0xffffffff) is True
    assert mirror_wait(m, 0x100000000, limit=0.01) is None          # generation 0xffffffff is behind generation 0
    put(0, 0)
    assert mirror_wait(m, 0x100000000) is False and mirror_wait(m, 0) is False
    assert mirror_wait(m, 0xffffffff) is False                      # ... and generation 0 is ahead of 0xffffffff


def test_store_agreement_with_four_threads(tmp_path):
    world = 4
    st = dist.HashStore() if hasattr(dist, "HashStore") else dist.FileStore(str(tmp_path / "store"), world)
    cases = [(), (2,), (0, 1, 2, 3), (), (0,)]                       # the ranks that overflow in round k: none, one, all (and two more rounds for the clean-up)
    got = [[None] * len(cases) for _ in range(world)]
    gone = [None] * len(cases)
    barrier = threading.Barrier(world)

    def rank_main(rank):
        for k, over in enumerate(cases):
            got[rank][k] = store_agree(st, k, rank, world, rank in over)
            barrier.wait()                   # every rank is through round k
            if rank == 0 and k >= 2:
                gone[k] = not st.check([f"a{k - 2}"]) and not st.check([f"o{k - 2}"]) and st.check([f"a{k - 1}"]) and st.check([f"a{k}"])
            barrier.wait()

    threads = [threading.Thread(target=rank_main, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(30)
    assert not any(t.is_alive() for t in threads)
    for k, over in enumerate(cases):
        assert [got[r][k] for r in range(world)] == [bool(over)] * world, (k, got)
    assert gone[2:] == [True] * (len(cases) - 2), gone
