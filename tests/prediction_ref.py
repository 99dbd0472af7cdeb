"""Test infrastructure: the prediction table at the head of view_fusion_amd/csrc/diffusion.hip (and the native weights of
csrc/loss_weight.h) restated in float64 numpy, on top of the existing restatements -- loss_ref (composition, penalties,
eps weights), sampler_ref.update (the few-step update from a given y0) and threshold_ref (the ancestral step on a table
pair, the threshold).  Nothing here calls the library.

    g = the level the network is conditioned on;  y_t = sqrt(g) y_0 + sqrt(1 - g) noise
    prediction   target                              y0_hat = a y - b out               c(g)
    "eps"        noise                               a = g^-1/2, b = (1/g - 1)^1/2      1
    "v"          sqrt(g) noise - sqrt(1 - g) y_0     a = sqrt(g), b = sqrt(1 - g)       g
    "x0"         y_0                                 a = 0,       b = -1                g / (1 - g)
    native weight = w_eps(g) c(g)  (min_snr, p2);  weighting None: 1
"""
import numpy as np
import torch

import loss_ref
import sampler_ref
import threshold_ref

PREDICTIONS = ("eps", "v", "x0")


def _per_sample(level, ndim):
    return np.asarray(level, dtype=np.float64).reshape((-1,) + (1,) * (ndim - 1))


def target(prediction, noise, y_0, level):
    """The training target, float64, of the (fp32) inputs taken exactly."""
    noise, y_0 = np.asarray(noise, dtype=np.float64), np.asarray(y_0, dtype=np.float64)
    g = _per_sample(level, noise.ndim)
    if prediction == "eps":
        return noise
    if prediction == "v":
        return np.sqrt(g) * noise - np.sqrt(1.0 - g) * y_0
    if prediction == "x0":
        return y_0
    raise ValueError(prediction)


def gammas(betas):
    return np.cumprod(1.0 - np.asarray(betas, dtype=np.float64))


def tables(betas, prediction):
    """(a, b) float64 over all T."""
    g = gammas(betas)
    if prediction == "eps":
        with np.errstate(divide="ignore"):
            return 1.0 / np.sqrt(g), np.sqrt(1.0 - g) / np.sqrt(g)
    if prediction == "v":
        return np.sqrt(g), np.sqrt(1.0 - g)
    if prediction == "x0":
        return np.zeros_like(g), -np.ones_like(g)
    raise ValueError(prediction)


def c(level, prediction, dtype=np.float64):
    g = np.asarray(level, dtype=np.float32).astype(dtype)
    with np.errstate(divide="ignore"):
        return {"eps": np.ones_like(g), "v": g, "x0": g / (dtype(1.0) - g)}[prediction]


def weights(level, prediction, kind, a=0.0, b=0.0, dtype=np.float64):
    """The native weight of the (fp32) levels.  float64: the definition, w_eps(g) c(g).  float32: the header's own forms
    in its operation order (the distance between the two bounds the library's error, as in loss_ref.weights)."""
    if prediction == "eps" or kind in (None, "none"):
        return loss_ref.weights(level, kind, a, b, dtype)
    if dtype == np.float64:
        return loss_ref.weights(level, kind, a, b) * c(level, prediction)
    g = np.asarray(level, dtype=np.float32)
    one, a, b = np.float32(1.0), np.float32(a), np.float32(b)
    with np.errstate(divide="ignore", invalid="ignore"):
        if kind == "min_snr":
            w = np.minimum(g, a * (one - g)) if prediction == "v" else np.minimum(g / (one - g), a)
        elif kind == "p2":
            w = np.power(a + g / (one - g), -b) * (g if prediction == "v" else g / (one - g))
        else:
            raise ValueError(kind)
    assert w.dtype == np.float32
    return w


def loss(out, noise, y_0, view_count, weighting, level, prediction, penalty="mse", delta=1.0, weight_kind=None, a=0.0,
         b=0.0, gloss=1.0):
    """loss_ref.loss on the native residual with the native weight -> the same dict (+ target)."""
    tg = target(prediction, noise, y_0, level)
    r = loss_ref.loss(out, tg, view_count, weighting, level, penalty, delta, None, gloss=gloss)      # w = 1
    w = weights(level, prediction, weight_kind, a, b)
    off = loss_ref.offsets(view_count)
    B = len(off) - 1
    total = 0.0
    for i in range(B):                                   # index order, as loss_ref.loss
        total += w[i] * r["sample_loss"][i]
        r["dout"][off[i]:off[i + 1]] *= w[i]
    r.update(loss=total / B, w=w, target=tg)
    return r


# ---- sampling ----------------------------------------------------------------------------------------------------------
def y0_hat(betas, prediction, t, y, out):
    a, b = tables(betas, prediction)
    return a[t] * np.asarray(y, dtype=np.float64) - b[t] * np.asarray(out, dtype=np.float64)


def ancestral_step(sched, betas, prediction, t, y, out, z, q=None, cmax=None, clip=True):
    """threshold_ref.ancestral_step with the prediction's table pair substituted for the two names it reads; sched = the
    six buffers (anything indexable) -> (y_next, mean, y0, s | None), float64."""
    a, b = tables(betas, prediction)
    sub = dict(sched, sqrt_recip_gammas=a, sqrt_recipm1_gammas=b)
    return threshold_ref.ancestral_step(sub, t, np.asarray(y, dtype=np.float64), np.asarray(out, dtype=np.float64), z, q,
                                        cmax, clip)


def sampler_step(betas, tau, solver, eta, prediction, k, y, out, y0_prev, z, q=None, cmax=None):
    """One few-step update from the composed output -> (y_new, y0, s | None), float64: y0 from the prediction's pair at
    tau[k], bounded, then sampler_ref.update (which takes y0)."""
    y = np.asarray(y, dtype=np.float64)
    y0, s = threshold_ref.bound(y0_hat(betas, prediction, int(tau[k]), y, out), q, cmax)
    return sampler_ref.update(betas, tau, solver, eta, k, y, y0, y0_prev, z), y0, s


def chain(unet_fn, compose_fn, betas, sched, prediction, y_cond, view_count, angle, y_T, z_seq, tau=None, solver="ddim",
          eta=0.0, weighting=True):
    """sampler_ref.chain / the ancestral chain (tau None) for a prediction: the network in fp32 at the fp32 level
    sched["gammas"][t], everything after it in float64.  -> states after every step, float32 (steps, B, 3, H, W)."""
    from oracle import view_fusion_ref as vfr
    B = y_cond.shape[0]
    y = y_T.double().numpy()
    y0_prev = np.full_like(y, np.nan)
    n = len(betas) if tau is None else len(tau)
    states = []
    for k in reversed(range(n)):
        t = k if tau is None else int(tau[k])
        level = sched["gammas"][t].reshape(1, 1).repeat(B, 1)
        x, ang_s, lvl_s = vfr.stack_views(y_cond, view_count, torch.tensor(y).float(), level, angle)
        out, _, _ = compose_fn(unet_fn(x, ang_s, lvl_s), view_count, weighting)
        out = out.double().numpy()
        z = 0.0 if z_seq is None else z_seq[t].double().numpy()
        if tau is None:
            y, _, _, _ = ancestral_step(sched, betas, prediction, t, y, out, z)
        else:
            y, y0_prev, _ = sampler_step(betas, tau, solver, eta, prediction, k, y, out, y0_prev, z)
        y = np.asarray(y, dtype=np.float64)
        states.append(torch.tensor(y).float())
    return torch.stack(states)
