"""Reads the resize fixtures (tools/gen_resize_golden.py) back as one table."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load():
    """(meta, cases): meta has dst, sizes, kinds, pillow_version and xmin_S / ntaps_S / coef_S; cases is a list of (S, kind, input, expected) uint8 arrays."""
    z = {}
    for name in ("resize_kat.npz", "resize_kat_2.npz"):
        with np.load(os.path.join(GOLDEN, name)) as f:
            z.update({k: f[k] for k in f.files})
    cases = []
    for s in z["sizes"].tolist():
        for kind in z["kinds"].tolist():
            same = z.get(f"same_as_{s}_{kind}")
            cases.append((s, kind, z[f"in_{s}_{kind}"], z[str(same)] if same is not None else z[f"out_{s}_{kind}"]))
    return z, cases
