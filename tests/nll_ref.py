"""The variational bound in bits per dimension, restated in numpy from the definition at the head of
view_fusion_amd/csrc/diffusion.hip ("Variational bound") -- written from the formulas, not from csrc/vlb.h -- and
parameterised by dtype: float64 is the oracle, float32 the yardstick for the rounding noise of the formulas themselves
(the tests give the device a margin over the float32 run's own distance from float64, never a number fixed in advance).

The seeded noisy target (csrc/rng.h, restated in tests/rng_ref.py style):
    counter = (block, id lo, id hi, (6 << 28) | step),  key = (seed lo, seed hi)
    kind 6  the noise of a noisy target, step = the MODEL timestep tau[k], block = the float4 index inside the sample's
            (3, H, W) image; four normals per call by Box-Muller as rng_ref.normal forms them
    y_k = sqrt(g) y_0 + sqrt(1 - g) n,  g = the fp32 gammas buffer value at tau[k]
"""
import numpy as np

import rng_ref

KIND_NLL_NOISE = 6
LN2 = np.log(2.0)
DELTA = 1.0 / 255.0


# ---- tables: a direct float64 formula (schedule.nll_tables is what is under test) ----------------------------------------
def tables(betas, tau=None, prediction="eps", fixed_variance="small"):
    betas = np.asarray(betas, dtype=np.float64)
    gammas = np.cumprod(1.0 - betas)
    tau = np.arange(len(betas)) if tau is None else np.asarray(tau, dtype=np.int64)
    gt = gammas[tau]
    gp = np.append(1.0, gt[:-1])
    with np.errstate(divide="ignore", invalid="ignore"):
        if prediction == "eps":
            a, b = np.sqrt(1.0 / gt), np.sqrt(1.0 / gt - 1.0)
        elif prediction == "v":
            a, b = np.sqrt(gt), np.sqrt(1.0 - gt)
        else:
            a, b = np.zeros_like(gt), -np.ones_like(gt)
        beta = 1.0 - gt / gp
        c0 = np.sqrt(gp) * beta / (1.0 - gt)
        hi = np.log(beta)
        lo = np.log(np.maximum(beta * (1.0 - gp) / (1.0 - gt), 1e-20))
    hi[0] = np.log(1.0 - gt[0])
    lo[0] = lo[1] if len(tau) > 1 else hi[0]
    if fixed_variance == "large":
        hi[0] = lo[0]
    return dict(a=a, b=b, c0=c0, hi=hi, lo=lo)


# ---- the arithmetic -------------------------------------------------------------------------------------------------------
def cdf(x, dt=np.float64):
    x = np.asarray(x, dtype=dt)
    return dt(0.5) * (dt(1.0) + np.tanh(dt(np.sqrt(2.0 / np.pi)) * (x + dt(0.044715) * x * x * x)))


def logvar(o, hi, lo, dt=np.float64):
    v = dt(0.5) * np.asarray(o, dtype=dt) + dt(0.5)
    return v * dt(hi) + (dt(1.0) - v) * dt(lo)


def kl_bits(lp, lo, m2, dt=np.float64):
    lp, lo, m2 = np.asarray(lp, dtype=dt), dt(lo), np.asarray(m2, dtype=dt)
    return dt(0.5) * (dt(-1.0) + lp - lo + np.exp(lo - lp) + m2 * np.exp(-lp)) / dt(LN2)


def decoder_parts(x, mean, lp, dt=np.float64):
    """-> (nll in bits, the probability mass the logarithm sees before its 1e-12 clamp), per element."""
    x, mean, lp = (np.asarray(v, dtype=dt) for v in (x, mean, lp))
    inv_sd = np.exp(dt(-0.5) * lp)
    d = x - mean
    cp, cm = cdf(inv_sd * (d + dt(DELTA)), dt), cdf(inv_sd * (d - dt(DELTA)), dt)
    p = np.where(x < dt(-0.999), cp, np.where(x > dt(0.999), dt(1.0) - cm, cp - cm)).astype(dt)
    return -np.log(np.maximum(p, dt(1e-12))) / dt(LN2), p


def compose(out, vc, weighting, dt=np.float64):
    """out (S, C, H, W), C in {6, 9} (3 with the mean) -> (out_b (B, 3, H, W), o_b (B, 3, H, W) | None): the composition over
    each sample's views of channels 0..2 (and 6..8) under the softmax of channels 3..5, or the mean."""
    out = np.asarray(out, dtype=dt)
    off = np.concatenate([[0], np.cumsum(vc)])
    e_b, o_b = [], []
    for i in range(len(vc)):
        rows = out[off[i]:off[i + 1]]
        if weighting:
            l = rows[:, 3:6]
            w = np.exp(l - l.max(axis=0, keepdims=True))
            w = w / w.sum(axis=0, keepdims=True)
        else:
            w = np.full_like(rows[:, 0:3], dt(1.0) / dt(len(rows)))
        e_b.append((w * rows[:, 0:3]).sum(axis=0))
        if out.shape[1] >= 9:
            o_b.append((w * rows[:, 6:9]).sum(axis=0))
    return np.stack(e_b).astype(dt), (np.stack(o_b).astype(dt) if o_b else None)


def noisy(y_0, n, g, dt=np.float64):
    """y_k = sqrt(g) y_0 + sqrt(1 - g) n; g: one level per sample (B,) or a scalar."""
    g = np.asarray(g, dtype=dt).reshape(-1, 1, 1, 1)
    return (np.sqrt(g) * np.asarray(y_0, dtype=dt) + np.sqrt(dt(1.0) - g) * np.asarray(n, dtype=dt)).astype(dt)


def seeded_normals(seed, ids, step, shape, dt=np.float64):
    """The kind-6 normals of samples `ids` at the model timestep `step`: (B, *shape)."""
    n = int(np.prod(shape))
    return rng_ref.normal(seed, ids, KIND_NLL_NOISE, step, n, dt).reshape(len(ids), *shape)


def term(out, vc, weighting, y_k, y_0, row, learned=False, decoder=False, large=False, clip=True, dt=np.float64):
    """One term of the bound for every sample.  row = (a, b, c0, hi, lo) of the step, the fp32 values the device reads.
    -> dict(vb (B,), x0_mse (B,), mass: the decoder's probability mass per element | None, y0, lp)."""
    a, b, c0, hi, lo = (dt(v) for v in row)
    e_b, o_b = compose(out, vc, weighting, dt)
    y0 = a * np.asarray(y_k, dtype=dt) - b * e_b
    if clip:
        y0 = np.clip(y0, dt(-1.0), dt(1.0))
    x = np.asarray(y_0, dtype=dt)
    d = y0 - x
    if learned:
        lp = logvar(o_b, hi, lo, dt)
    else:
        lp = np.full_like(d, hi if large else lo)
    mass = None
    if decoder:
        t, mass = decoder_parts(x, y0, lp, dt)
    else:
        t = kl_bits(lp, lo, c0 * c0 * d * d, dt)
    B = len(vc)
    assert t.dtype == dt and d.dtype == dt
    return dict(vb=t.reshape(B, -1).mean(axis=1, dtype=dt), x0_mse=(d * d).reshape(B, -1).mean(axis=1, dtype=dt),
                mass=mass, y0=y0, lp=lp, elem=t)


def prior(y_0, gT, dt=np.float64):
    """L_T per sample (B,): the KL of N(sqrt(gT) y_0, 1 - gT) from N(0, 1), in bits per dimension."""
    gT = dt(gT)
    x = np.asarray(y_0, dtype=dt)
    om = dt(1.0) - gT
    t = dt(0.5) * (dt(-1.0) - np.log(om) + om + gT * x * x) / dt(LN2)
    return t.reshape(len(x), -1).mean(axis=1, dtype=dt)


_CASES = {}


def conditioned_case(tabs32, gammas32, tau, k, hw, vc, weighting, learned, seed=11, umax=2.0):
    """Fixed-seed inputs of one term at step k, built once and left unchanged, so that the term is well conditioned:
    y_0 uniform in [-1, 1] with the first two pixels of every sample at -1 and +1 (both open-ended bins of the decoder);
    y_k its noisy version at gammas32[tau[k]]; the per-view outputs differ from view to view, and their composition under
    the softmax of the random logits (or the mean) is, in float64, the exact target plus sd u / b -- y0 = y_0 + sd u with
    sd = exp(0.5 lo[k]) and u uniform in [-umax, umax] (|u| <= 3): no element is many sd away, so no logarithm is near its
    1e-12 clamp.  Channels 6..8 (learned) uniform in [-1.2, 1.2].  -> dict(out, y_k, y_0, row), float32 arrays."""
    row = tuple(np.float32(tabs32[n][k]) for n in ("a", "b", "c0", "hi", "lo"))
    key = (row, float(gammas32[tau[k]]), k, tuple(hw), tuple(vc), weighting, learned, seed, umax)
    if key in _CASES:
        return _CASES[key]
    H, W = hw
    B, S = len(vc), int(sum(vc))
    g = np.random.default_rng(seed + 101 * k)
    y_0 = g.uniform(-1.0, 1.0, (B, 3, H, W)).astype(np.float32)
    y_0.reshape(B, -1)[:, 0] = -1.0
    y_0.reshape(B, -1)[:, 1] = 1.0
    y_k = noisy(y_0, g.standard_normal((B, 3, H, W)).astype(np.float32), gammas32[tau[k]], np.float32)
    sd = np.exp(0.5 * np.float64(row[4]))
    u = g.uniform(-umax, umax, (B, 3, H, W))
    want = exact_output(y_k, y_0, row) - sd * u / np.float64(row[1])
    logits = 2.0 * g.standard_normal((S, 3, H, W))
    spread = 0.3 * g.standard_normal((S, 3, H, W))
    var = g.uniform(-1.2, 1.2, (S, 3, H, W))
    off = np.concatenate([[0], np.cumsum(vc)])
    pred = np.empty((S, 3, H, W))
    for i in range(B):
        r = slice(off[i], off[i + 1])
        if weighting:
            w = np.exp(logits[r] - logits[r].max(axis=0, keepdims=True))
            w = w / w.sum(axis=0, keepdims=True)
        else:
            w = np.full_like(logits[r], 1.0 / vc[i])
        pred[r] = want[i] + spread[r] - (w * spread[r]).sum(axis=0, keepdims=True)
    out = np.concatenate([pred, logits] + ([var] if learned else []), axis=1).astype(np.float32)
    _CASES[key] = dict(out=out, y_k=y_k, y_0=y_0, row=row)
    return _CASES[key]


def exact_output(y_k, y_0, row, dt=np.float64):
    """What a network has to answer in every view for y0 == y_0: (a y_k - y_0) / b."""
    a, b = dt(row[0]), dt(row[1])
    return (a * np.asarray(y_k, dtype=dt) - np.asarray(y_0, dtype=dt)) / b
