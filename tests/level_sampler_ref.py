"""numpy restatement of view_fusion_amd/csrc/level_sampler.h (loss-aware noise-level sampling): the bins, the fixed-point
proposal table, the draw, the importance weight and the statistics, with Python integers / uint64 for everything that is
an integer in the header and float64 for everything else.  Nothing here calls the library; the tests compare the library
with this file.  Also the float64 loss with a per-sample scale, on top of tests/loss_ref.py.  No torch, no GPU."""
from fractions import Fraction

import numpy as np

import loss_ref

TWO32 = 1 << 32


def lo(T, K):
    """lo_0 .. lo_K (lo_K = T) as Python ints."""
    return [1 + (k * (T - 1) + K - 1) // K for k in range(K + 1)]


def sizes(T, K):
    l = lo(T, K)
    return [l[k + 1] - l[k] for k in range(K)]


def bin_of(t, T, K):
    return ((np.asarray(t, dtype=np.int64) - 1) * K) // (T - 1)


def min_uniform_mix(T):
    """The smallest eps the header accepts: eps 2^32 >= 2 (T - 1)."""
    return 2.0 * (T - 1) / TWO32


def table(q, T, K, eps):
    """masses q (K,) -> (c [K + 1] Python ints, iw (K,) float32).  cum is the in-order float64 running sum."""
    q = [float(v) for v in q]
    assert len(q) == K and 1 <= K <= min(T - 1, 1024) and eps * TWO32 >= 2 * (T - 1)
    n = sizes(T, K)
    qsum = 0.0
    for v in q:
        qsum += v
    assert np.isfinite(qsum) and qsum > 0
    c, cum = [], 0.0
    for k in range(K):
        c.append(int(np.floor(cum * 4294967296.0)))
        cum += (1.0 - eps) * (q[k] / qsum) + eps * (n[k] / (T - 1))
    c.append(TWO32)
    return c, iw_of(c, T, K)


def iw_of(c, T, K):
    n = sizes(T, K)
    return np.array([np.float32(np.float64(n[k]) * 4294967296.0 / (np.float64(T - 1) * np.float64(int(c[k + 1]) - int(c[k]))))
                     for k in range(K)], dtype=np.float32)


def draw(x, c, T, K):
    """words x -> (t int64, bin int64): the bin by searchsorted on the cut points, t in Python-exact uint64 arithmetic."""
    x = np.asarray(x, dtype=np.uint64)
    cc = np.array([int(v) for v in c], dtype=np.uint64)
    k = np.searchsorted(cc, x, side="right").astype(np.int64) - 1
    l, n = np.array(lo(T, K), dtype=np.uint64), np.array(sizes(T, K), dtype=np.uint64)
    width = cc[k + 1] - cc[k]
    t = l[k] + ((x - cc[k]) * n[k]) // width                   # (x - c_k) n_k < 2^32 2^28: fits uint64
    return t.astype(np.int64), k


def uniform_draw(x, T):
    return 1 + ((np.asarray(x, dtype=np.uint64) * np.uint64(T - 1)) >> np.uint64(32)).astype(np.int64)


def word_counts(c, T, K):
    """How many of the 2^32 words map to each timestep: {t: count}, exact.  Offset y = x - c_k in [0, width) gives
    j = (y n) // width, so j is drawn by ceil((j + 1) width / n) - ceil(j width / n) words."""
    l, n = lo(T, K), sizes(T, K)
    out = {}
    for k in range(K):
        width = int(c[k + 1]) - int(c[k])
        for j in range(n[k]):
            out[l[k] + j] = -((-(j + 1) * width) // n[k]) + ((-j * width) // n[k])
    return out


def mean_iw_exact(c, T, K):
    """sum_k width_k iw_k / 2^32 with iw_k the RATIONAL weight n_k 2^32 / ((T - 1) width_k): exactly 1."""
    n = sizes(T, K)
    return sum(Fraction(int(c[k + 1]) - int(c[k])) * Fraction(n[k] * TWO32, (T - 1) * (int(c[k + 1]) - int(c[k])))
               for k in range(K)) / TWO32


def stats_update(m, seen, sample_loss, sample_w, t, T, K, beta):
    """One step's update in float64 -> (m, seen) new arrays.  sample_w None: 1."""
    m, seen = np.array(m, dtype=np.float64), np.array(seen, dtype=np.int64)
    s = np.asarray(sample_loss, dtype=np.float64)
    w = np.ones_like(s) if sample_w is None else np.asarray(sample_w, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        r = (w * s) ** 2
    b = bin_of(t, T, K)
    for k in range(K):
        tot, cnt = 0.0, 0
        for i in range(len(s)):                                  # index order
            if b[i] == k and np.isfinite(r[i]):
                tot, cnt = tot + r[i], cnt + 1
        if cnt:
            mean = tot / cnt
            m[k] = mean if seen[k] == 0 else m[k] + (1.0 - beta) * (mean - m[k])
            seen[k] += cnt
    return m, seen


def masses(m, T, K):
    return np.array(sizes(T, K), dtype=np.float64) * np.sqrt(np.asarray(m, dtype=np.float64))


def is_ready(m, seen, T, K, warmup):
    q = masses(m, T, K)
    qsum = 0.0
    for v in q:
        qsum += v
    return bool(np.min(seen) >= warmup and np.isfinite(qsum) and qsum > 0)


def scaled_loss(out, target, view_count, weighting, level, scale, penalty="mse", delta=1.0, weight_kind=None, a=0.0,
                b=0.0, gloss=1.0):
    """loss_ref.loss with sample weight w_b scale_b: -> dict(loss, sample_loss (unweighted), w (= w_b scale_b), dout)."""
    ref = loss_ref.loss(out, target, view_count, weighting, level, penalty, delta, weight_kind, a, b, gloss)
    scale = np.asarray(scale, dtype=np.float32).astype(np.float64)
    w = ref["w"] * scale
    total = 0.0
    for i in range(len(w)):
        total += w[i] * ref["sample_loss"][i]
    off = loss_ref.offsets(view_count)
    dout = ref["dout"].copy()
    for i in range(len(w)):                                      # d loss / d out is linear in the sample's weight
        dout[off[i]:off[i + 1]] *= scale[i]
    return dict(loss=total / len(w), sample_loss=ref["sample_loss"], w=w, dout=dout)
