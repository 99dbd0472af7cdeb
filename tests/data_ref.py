"""numpy restatement of the data draws of view_fusion_amd/csrc/rng.h (kind 4, "Data draws") and of the batch they
describe, on top of rng_ref.words(seed, ids, 4, 0, 13).  Nothing here calls the library; the tests compare the library
(the host mirror vf_batch_host_plan, the kernel vf_batch_assemble) with this file, and this file's index algebra with
what the reference loader's process_sample did (tests/golden/data_plan.npz)."""
import numpy as np

import rng_ref

KIND_DATA, BLOCKS, VIEWS = 4, 13, 24
COIN = 1677722                       # (w >> 8) < COIN  <=>  (w >> 8) * 2^-24 < 0.1


def mulhi32(w, n):
    return (np.asarray(w, dtype=np.uint64) * np.uint64(n)) >> np.uint64(32)


def shuffle(p, w):
    """Fisher-Yates on the rows of p (B, 24) with the words w (B, 23): i = 23 ... 1 uses w[:, 23 - i]."""
    p = p.copy()
    rows = np.arange(p.shape[0])
    for i in range(VIEWS - 1, 0, -1):
        r = mulhi32(w[:, VIEWS - 1 - i], i + 1).astype(np.int64)
        a, b = p[rows, i].copy(), p[rows, r].copy()
        p[rows, i], p[rows, r] = b, a
    return p


def index_algebra(p, second, q):
    """What process_sample's outputs show, as view indices: p (B, 24) after the first shuffle, second (B,) bool,
    q (B, 24) = images_idx at the end (= p when not second)."""
    p, q, second = np.asarray(p, dtype=np.int64), np.asarray(q, dtype=np.int64), np.asarray(second, dtype=bool)
    src = np.where(second[:, None], np.take_along_axis(p, q, axis=1), p)
    return dict(src=src, target=p[:, 0], cond=src[:, 1:], rel_ref=np.repeat(src[:, 1:2], VIEWS - 1, axis=1),
                angle=(2 * np.pi / 24 * p[:, 0]).astype(np.float32),
                relative_angle=(2 * np.pi / 24 * (q[:, 1] - q[:, 0])).astype(np.float32))


def plan(seed, ids, train, lo, hi, N, objects=None):
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    w = rng_ref.words(seed, ids, KIND_DATA, 0, BLOCKS).reshape(ids.size, 4 * BLOCKS)      # w[:, 4 * block + lane]
    ident = np.tile(np.arange(VIEWS, dtype=np.int64), (ids.size, 1))
    p = shuffle(ident, w[:, 0:23])
    second = ((w[:, 23] >> np.uint64(8)) < np.uint64(COIN)) & bool(train)
    q2 = shuffle(p, w[:, 24:47])                                   # always consumed
    q = np.where(second[:, None], q2, p)
    out = index_algebra(p, second, q)
    out.update(p=p, q=q, second=second, q01=q[:, :2],
               view_count=(lo + mulhi32(w[:, 47], hi - lo + 1)).astype(np.int64),
               object=mulhi32(w[:, 48], N).astype(np.int64) if objects is None
               else np.asarray(objects, dtype=np.int64).reshape(-1))
    return out


def pixels(store_u8):
    return store_u8.astype(np.float32) / np.float32(255)


def assemble(store_u8, pl, relative):
    """store_u8 (N, 24, 3, H, W) uint8 -> y_0 (B, 3, H, W), y_cond (B, 23, 3 | 6, H, W), angle (B, 1), float32."""
    obj = pl["object"]
    y_0 = pixels(store_u8[obj, pl["target"]])
    cond = pixels(store_u8[obj[:, None], pl["cond"]])
    if not relative:
        return y_0, cond, pl["angle"].reshape(-1, 1)
    ref = pixels(store_u8[obj[:, None], pl["rel_ref"]])
    return y_0, np.concatenate((ref, cond), axis=2), pl["relative_angle"].reshape(-1, 1)
