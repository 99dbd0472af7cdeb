"""The training objective's options (csrc/loss_weight.h) restated in float64 numpy: composition over the views ->
penalty -> per-sample noise-level weight -> loss, the per-sample loss, d loss / d unet_out in closed form, and the
loss-by-level binning.  The yardstick of tests/test_loss_host.py (which checks it against torch autograd) and of
tests/test_gpu_loss_options.py.  No torch, no GPU."""
import numpy as np

PENALTIES = ("mse", "l1", "huber")
WEIGHTINGS = (None, "min_snr", "p2")


def offsets(view_count):
    return np.concatenate([[0], np.cumsum([int(v) for v in view_count])]).astype(np.int64)


def compose(out, view_count, weighting):
    """out (S, 6|3, H, W) -> noise_hat (B, 3, H, W) float64 and the per-view softmax weights [(V_b, 3, H, W)] | None."""
    out = np.asarray(out, dtype=np.float64)
    off = offsets(view_count)
    nh, ws = [], []
    for b in range(len(off) - 1):
        eps = out[off[b]:off[b + 1], :3]
        if not weighting:
            nh.append(eps.mean(axis=0))
            continue
        lg = out[off[b]:off[b + 1], 3:6]
        w = np.exp(lg - lg.max(axis=0, keepdims=True))
        w /= w.sum(axis=0, keepdims=True)
        ws.append(w)
        nh.append((w * eps).sum(axis=0))
    return np.stack(nh), (ws if weighting else None)


def rho(d, penalty, delta=1.0):
    if penalty == "mse":
        return d * d
    if penalty == "l1":
        return np.abs(d)
    if penalty == "huber":
        return np.where(np.abs(d) <= delta, 0.5 * d * d, delta * (np.abs(d) - 0.5 * delta))
    raise ValueError(penalty)


def drho(d, penalty, delta=1.0):
    if penalty == "mse":
        return 2.0 * d
    if penalty == "l1":
        return np.sign(d)
    if penalty == "huber":
        return np.clip(d, -delta, delta)
    raise ValueError(penalty)


def weights(level, kind, a=0.0, b=0.0, dtype=np.float64):
    """w_b of the levels (the float32 values the device holds, taken exactly): float64 (the yardstick) or float32 in the
    header's operation order (the distance between the two bounds the library's error)."""
    g = np.asarray(level, dtype=np.float32).astype(dtype)
    one, a, b = dtype(1.0), dtype(a), dtype(b)
    with np.errstate(divide="ignore", invalid="ignore"):
        if kind in (None, "none"):
            w = np.ones_like(g)
        elif kind == "min_snr":
            w = np.minimum(one, a * (one - g) / g)
        elif kind == "p2":
            w = np.power(a + g / (one - g), -b)
        else:
            raise ValueError(kind)
    assert w.dtype == dtype
    return w


def loss(out, target, view_count, weighting, level, penalty="mse", delta=1.0, weight_kind=None, a=0.0, b=0.0,
         gloss=1.0):
    """-> dict(loss, sample_loss (B,), w (B,), noise_hat, dout (S, C, H, W) = d (gloss * loss) / d out, d (B, 3, H, W))."""
    out = np.asarray(out, dtype=np.float64)
    target = np.asarray(target, dtype=np.float64)
    off = offsets(view_count)
    B = len(off) - 1
    nh, ws = compose(out, view_count, weighting)
    d = nh - target
    n = d[0].size
    s = rho(d, penalty, delta).reshape(B, -1).sum(axis=1) / n
    w = weights(level, weight_kind, a, b)
    total = 0.0
    for i in range(B):                                   # index order, no renormalisation by sum w
        total += w[i] * s[i]
    g = gloss * w.reshape(B, 1, 1, 1) * drho(d, penalty, delta) / (n * B)
    dout = np.zeros_like(out)
    for i in range(B):
        v0, v1 = off[i], off[i + 1]
        if not weighting:
            dout[v0:v1, :3] = g[i] / (v1 - v0)
            continue
        eps = out[v0:v1, :3]
        dout[v0:v1, :3] = ws[i] * g[i]
        dout[v0:v1, 3:6] = ws[i] * (eps - nh[i]) * g[i]
    return dict(loss=total / B, sample_loss=s, w=w, noise_hat=nh, dout=dout, d=d)


def bins(level, K):
    """The kernel's bin of every level: min(K - 1, int(level * K)), the product a single float32 multiply."""
    g = np.asarray(level, dtype=np.float32)
    return np.minimum(K - 1, (g * np.float32(K)).astype(np.int64))


def histogram(level, sample_loss, K):
    """-> (sum (K,) float64, count (K,) int64) of the unweighted per-sample losses by bin."""
    idx = bins(level, K)
    s = np.zeros(K)
    np.add.at(s, idx, np.asarray(sample_loss, dtype=np.float64))
    return s, np.bincount(idx, minlength=K).astype(np.int64)
