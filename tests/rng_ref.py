"""numpy restatement of view_fusion_amd/csrc/rng.h (the seeded counter-based draws): Philox4x32-10 in uint64 integer
arithmetic, the integer / uniform maps exactly, Box-Muller once in float32 in the header's operation order and once in
float64.  Nothing here calls the library; the tests compare the library with this file.

Tolerance of the normals (`bound`): e = the largest disagreement of the two restatements on the counters under test;
the library must be within max(4 e, 1e-6) of the float64 one -- the convention of tests/ssim_ref.py."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
KIND_SCALARS, KIND_TRAIN_NOISE, KIND_START_NOISE, KIND_STEP_NOISE = 0, 1, 2, 3

# Random123 known-answer vectors (counter, key, output), re-derived with philox_int below
KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
        (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


def philox_int(ctr, key):
    """One call in plain Python integers."""
    c0, c1, c2, c3 = (int(c) for c in ctr)
    k0, k1 = (int(k) for k in key)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & 0xFFFFFFFF, (p0 >> 32) ^ c3 ^ k1, p0 & 0xFFFFFFFF
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c0, c1, c2, c3


def philox(c0, c1, c2, c3, k0, k1):
    """Vectorised: uint64 arrays holding 32-bit values (broadcast together) -> four uint64 arrays of 32-bit words."""
    c0, c1, c2, c3, k0, k1 = (np.asarray(a, dtype=np.uint64) for a in (c0, c1, c2, c3, k0, k1))
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(c0, c1, c2, c3, k0, k1)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2          # 32 x 32 bits: fits 64
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & MASK, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + np.uint64(W0)) & MASK, (k1 + np.uint64(W1)) & MASK
    return c0, c1, c2, c3


def words(seed, ids, kind, step, nblocks):
    """(B, nblocks, 4) uint64: the words of counter (block, id lo, id hi, kind << 28 | step) under key = seed."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    ids = np.asarray(ids, dtype=np.int64).astype(np.uint64).reshape(-1, 1)
    step = np.asarray(step, dtype=np.uint64).reshape(-1, 1)          # scalar, or one step per sample
    block = np.arange(nblocks, dtype=np.uint64).reshape(1, -1)
    stream = np.uint64(int(kind) << 28) | step
    w = philox(block, ids & MASK, ids >> np.uint64(32), stream, seed & 0xFFFFFFFF, seed >> 32)
    return np.stack(w, axis=-1)


def train_scalars(seed, ids, T):
    """t (B,) int64 in [1, T-1] and u (B,) float32 in [0, 1): exact."""
    w = words(seed, ids, KIND_SCALARS, 0, 1)[:, 0]
    t = 1 + ((w[:, 0] * np.uint64(T - 1)) >> np.uint64(32)).astype(np.int64)
    u = ((w[:, 1] >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float32)
    return t, u


def _box_muller32(wa, wb):
    one = np.float32
    ua = wa.astype(one) * one(2.0 ** -32) + one(2.0 ** -33)
    ub = wb.astype(one) * one(2.0 ** -32) + one(2.0 ** -33)
    r = np.sqrt(one(-2.0) * np.log(ua))
    a = one(6.283185307179586) * ub
    return r * np.cos(a), r * np.sin(a)


def _box_muller64(wa, wb):
    ua = wa.astype(np.float64) * 2.0 ** -32 + 2.0 ** -33
    ub = wb.astype(np.float64) * 2.0 ** -32 + 2.0 ** -33
    r = np.sqrt(-2.0 * np.log(ua))
    a = 2.0 * np.pi * ub
    return r * np.cos(a), r * np.sin(a)


def normal(seed, ids, kind, step, n, dtype=np.float64):
    """(B, n) normals, n % 4 == 0: float64 (the yardstick) or float32 (the header's operation order)."""
    assert n % 4 == 0
    w = words(seed, ids, kind, step, n // 4)
    bm = _box_muller64 if dtype == np.float64 else _box_muller32
    n0, n1 = bm(w[..., 0], w[..., 1])
    n2, n3 = bm(w[..., 2], w[..., 3])
    out = np.stack([n0, n1, n2, n3], axis=-1).reshape(w.shape[0], n)
    assert out.dtype == dtype
    return out


def bound(seed, ids, kind, step, n):
    """-> (float64 normals, e, max(4 e, 1e-6))."""
    r64 = normal(seed, ids, kind, step, n)
    e = float(np.abs(normal(seed, ids, kind, step, n, np.float32).astype(np.float64) - r64).max())
    return r64, e, max(4.0 * e, 1e-6)
