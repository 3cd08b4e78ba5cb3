"""Host restatement of the erase record (include/qatvit.h): the eight words, their clamped form, Philox4x32-10 in NumPy integer arithmetic, the
noise field of a key in fp64, and the erased batch.  tests/test_erase_abi.py checks the known-answer vectors and the drawing rule against it;
tests/test_gpu_erase.py builds its expectations with it."""
import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def f32_bits(v):
    return int(np.float32(v).view(np.int32))


def _i32(v):
    return int(np.uint32(v & MASK).view(np.int32))


def pack(y0, y1, x0, x1, fill=(0.0, 0.0, 0.0), mode=0, key=(0, 0)):
    """The eight int32 words of one batch position; the bounds 0 .. 65535, `fill` three fp32 values, `key` two 32-bit words."""
    assert all(0 <= v <= 0xffff for v in (y0, y1, x0, x1))
    return [_i32(y0 | y1 << 16), _i32(x0 | x1 << 16)] + [f32_bits(f) for f in fill] + [int(mode), _i32(key[0]), _i32(key[1])]


def unpack(rec):
    """(y0, y1, x0, x1, (f0, f1, f2) as np.float32, mode bit, (k0, k1) unsigned) of a record as the kernels read it, bounds not clamped."""
    w = [int(v) & MASK for v in rec]
    fill = tuple(np.uint32(v).view(np.float32) for v in w[2:5])
    return w[0] & 0xffff, w[0] >> 16, w[1] & 0xffff, w[1] >> 16, fill, w[5] & 1, (w[6], w[7])


def clamped(rec, D):
    """The record the kernels act on: every bound clamped to [0, D], only bit 0 of the mode kept."""
    y0, y1, x0, x1, _, mode, _ = unpack(rec)
    out = [int(v) for v in rec]
    out[0], out[1], out[5] = _i32(min(y0, D) | min(y1, D) << 16), _i32(min(x0, D) | min(x1, D) << 16), mode
    return out


def philox4x32_10(counter, key):
    """counter: four uint32 arrays (or ints) of one shape, key: two 32-bit ints -> four uint32 arrays.  uint64 products, so exact."""
    c = [np.asarray(v, dtype=np.uint64) & np.uint64(MASK) for v in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & MASK, int(key[1]) & MASK
    for _ in range(10):
        p0, p1 = c[0] * np.uint64(M0), c[2] * np.uint64(M1)
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & np.uint64(MASK), (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & np.uint64(MASK)]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return [v.astype(np.uint32) for v in c]


def noise(key, D):
    """fp64 [3, D, D]: z(key, c, y, x) of include/qatvit.h - counter (y * (D / 4) + x / 4, c, 0, 0), Box-Muller on (r0, r1) and (r2, r3)."""
    D4 = D // 4
    c, y, x4 = np.meshgrid(np.arange(3), np.arange(D), np.arange(D4), indexing="ij")
    r = philox4x32_10((y * D4 + x4, c, 0, 0), key)
    out = np.empty((3, D, D4, 4), dtype=np.float64)
    for h in range(2):
        u = ((r[2 * h] >> np.uint32(9)).astype(np.float64) + 1.0) * 2.0 ** -23
        t = (r[2 * h + 1] >> np.uint32(8)).astype(np.float64) * 2.0 ** -23
        R = np.sqrt(-2.0 * np.log(u))
        out[..., 2 * h], out[..., 2 * h + 1] = R * np.cos(np.pi * t), R * np.sin(np.pi * t)
    return out.reshape(3, D, D)


def erased(X, records, fields=None):
    """X fp32 [B, 3, D, D] (what the existing entries give per position), records int [B, 8] -> E.  Noise boxes take fp32(noise(key, D)), or
    `fields[key]` where the caller passes fields it has formed already (fp32 or fp64 [3, D, D])."""
    X = np.asarray(X, dtype=np.float32)
    D, out = X.shape[-1], X.copy()
    for b, rec in enumerate(np.asarray(records).tolist()):
        y0, y1, x0, x1, fill, mode, key = unpack(clamped(rec, D))
        if y1 <= y0 or x1 <= x0:
            continue
        if mode:
            z = fields[key] if fields is not None and key in fields else noise(key, D)
            out[b, :, y0:y1, x0:x1] = np.asarray(z)[:, y0:y1, x0:x1].astype(np.float32)
        else:
            out[b, :, y0:y1, x0:x1] = np.array(fill, dtype=np.float32)[:, None, None]
    return out


def box_mask(records, D):
    """bool [B, 3, D, D]: the elements inside the clamped box of each record."""
    recs = np.asarray(records).tolist()
    m = np.zeros((len(recs), 3, D, D), dtype=bool)
    for b, rec in enumerate(recs):
        y0, y1, x0, x1 = unpack(clamped(rec, D))[:4]
        if y1 > y0 and x1 > x0:
            m[b, :, y0:y1, x0:x1] = True
    return m
