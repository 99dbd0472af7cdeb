"""numpy restatement of the seeded residual-block Dropout masks (view_fusion_amd/csrc/rng.h, kind 5, "Dropout masks"),
built on tests/rng_ref.py's `philox`.  Nothing here calls the library; the tests compare the library with this file.

Row v of a layer's (S, n) activation is view v - off[b] of sample b.  Element e of the row uses word e % 4 of the call
with counter (e // 4, id lo, id hi, (5 << 28) | (layer << 12) | view) under key = seed; with k = word >> 8 it is kept
iff k >= thr, thr = ceil(float32(p) * 2^24).  (rng_ref.words puts the plain step in the stream field; here that value
is (layer << 12) | view, one per ROW, so this file calls `philox` on the counter written out.)"""
import math

import numpy as np

import rng_ref

KIND_DROPOUT = 5
MAX_VIEWS, MAX_LAYERS = (1 << 12) - 1, 1 << 16


def threshold(p):
    """ceil(float32(p) * 2^24): the product of a float32 and a power of two is exact in double precision."""
    return int(math.ceil(float(np.float32(p)) * 2.0 ** 24))


def scale(p):
    """1.0f / (1.0f - p) in float32, the expression vf_dropout evaluates."""
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def rows(off):
    """off (B + 1,) -> (sample b, view index) of every row, each (S,)."""
    off = np.asarray(off, dtype=np.int64)
    counts = np.diff(off)
    assert off[0] == 0 and (counts >= 1).all()
    if counts.max() > MAX_VIEWS:
        raise ValueError(f"a sample's views are numbered in 12 bits: {counts.max()} > {MAX_VIEWS}")
    b = np.repeat(np.arange(len(counts)), counts)
    return b, np.arange(off[-1]) - off[b]


def counter_words(seed, id_, layer, view, block):
    """The four words of one call, the counter written out by hand (arrays broadcast) -> (..., 4) uint64."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    id_ = np.asarray(id_, dtype=np.int64).astype(np.uint64)
    stream = np.uint64(KIND_DROPOUT << 28) | (np.asarray(layer, dtype=np.uint64) << np.uint64(12)) \
        | np.asarray(view, dtype=np.uint64)
    w = rng_ref.philox(np.asarray(block, dtype=np.uint64), id_ & rng_ref.MASK, id_ >> np.uint64(32), stream,
                       seed & 0xFFFFFFFF, seed >> 32)
    return np.stack(w, axis=-1)


def draws24(seed, ids, off, n, layer):
    """k = word >> 8 of every element: (S, n) uint64 in [0, 2^24)."""
    assert n % 4 == 0
    if not 0 <= int(layer) < MAX_LAYERS:
        raise ValueError(f"layer {layer} outside [0, {MAX_LAYERS})")
    b, view = rows(off)
    ids = np.asarray(ids, dtype=np.int64)
    w = counter_words(seed, ids[b].reshape(-1, 1), int(layer), view.reshape(-1, 1), np.arange(n // 4).reshape(1, -1))
    return (w >> np.uint64(8)).reshape(len(b), n)


def keep(seed, ids, off, n, p, layer):
    """(S, n) bool: True = kept."""
    return draws24(seed, ids, off, n, layer) >= np.uint64(threshold(p))


def uniforms(seed, ids, off, n, layer, p=None):
    """(S, n) float32: u = k * 2^-24, exact; usable as the `dropout_u` of that layer (u >= float32(p) <=> kept).  `p`
    takes no part: the draws do not depend on it."""
    return (draws24(seed, ids, off, n, layer).astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float32)


def apply(x, seed, ids, off, p, layer):
    """The layer on a float32 (S, ...) array, in the kernel's arithmetic: keep ? x * scale : 0."""
    x = np.asarray(x, dtype=np.float32)
    m = keep(seed, ids, off, x[0].size, p, layer).reshape(x.shape)
    return np.where(m, x * scale(p), np.float32(0.0)).astype(np.float32)
