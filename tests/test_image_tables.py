"""CPU-side check of the input pipeline's host coefficient tables (qatvit_image_resize_coeffs, qatvit_image_resize_coeffs_windows,
qatvit_image_window_coeffs): the one Pillow builder behind the three entries writes, byte for byte, the tables the two builders in front of it
wrote.  tests/golden/image_table_digests.json holds their sha256 digests (tools/gen_image_table_digests.py), recorded from the library before the
builders were folded; D = 44 is the size whose window side 12 has a fifth, zero-weight tap, refused by the four-tap table and stored by the
17-tap one.  Nothing here needs a GPU: the entries are host code."""
import json
import os

import pytest

from tools.gen_image_table_digests import OUT, SIZES, table_digests

GOLDEN = json.load(open(OUT))


def test_the_fixture_names_the_sizes():
    assert sorted(GOLDEN) == sorted(str(D) for D in SIZES) and os.path.getsize(OUT) < 4096


@pytest.mark.parametrize("D", SIZES)
def test_tables_are_the_recorded_ones(native_lib, D):
    refused = []
    assert table_digests(native_lib, D, refused) == GOLDEN[str(D)]
    # the four-tap form refuses the fifth tap of the side 12 at D = 44, alone and inside the window tables; the 17-tap form stores it
    assert refused == ([("resize_coeffs", 12, 44), ("resize_coeffs_windows", 44, 44)] if D == 44 else [])
