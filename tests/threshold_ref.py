"""Test infrastructure: a numpy restatement (float64 unless told otherwise) of dynamic thresholding and guidance rescaling
as the head of view_fusion_amd/csrc/diffusion.hip defines them.  Nothing here calls the library; the tests compare the
library with this file.

    n = 3 H W, every statistic per sample over its n elements
    eps_g   = g eps_c + (1 - g) eps_u  (guided; else eps_c)
    rescale   r = phi sigma(eps_c) / sigma(eps_g) + (1 - phi);  r = 1 where sigma(eps_g) == 0;  eps = r eps_g
    y0_hat  = a y - b eps
    threshold x = sort(|y0_hat|), pos = q (n - 1), k = floor(pos), frac = float32(pos - k)
              s = min(max(1, x[k] + frac (x[k+1] - x[k])), c);  y0 = clip(y0_hat, -s, s) / s
"""
import math

import numpy as np
import torch

import sampler_ref


# ---- the quantile -----------------------------------------------------------------------------------------------------
def quantile_position(n, q):
    """(k, frac): x[k+1] is never needed when frac == 0."""
    pos = float(q) * (n - 1)
    k = int(math.floor(pos))
    return k, float(np.float32(pos - k))


def abs_quantile(x, q):
    """x (B, n) -> (B,) float64: the q-quantile of |x| along the rows, linear interpolation between order statistics."""
    x = np.sort(np.abs(np.asarray(x, dtype=np.float64)), axis=1)
    k, frac = quantile_position(x.shape[1], q)
    if frac == 0.0:
        return x[:, k].copy()
    return x[:, k] + frac * (x[:, k + 1] - x[:, k])


def threshold_scale(y0_hat, q, c=None):
    """s_b (B,) of y0_hat (B, ...)."""
    y0_hat = np.asarray(y0_hat)
    s = np.maximum(1.0, abs_quantile(y0_hat.reshape(y0_hat.shape[0], -1), q))
    return s if c is None else np.minimum(s, float(c))


def bound(y0_hat, q=None, c=None, clip=True):
    """y0 from y0_hat: the dynamic threshold (q given), else the static clamp (clip) -> (y0, s | None)."""
    y0_hat = np.asarray(y0_hat)
    if q is None:
        return (np.clip(y0_hat, -1.0, 1.0) if clip else y0_hat), None
    s = threshold_scale(y0_hat, q, c)
    sb = s.reshape((-1,) + (1,) * (y0_hat.ndim - 1)).astype(y0_hat.dtype)
    return np.clip(y0_hat, -sb, sb) / sb, s


# ---- the noise -------------------------------------------------------------------------------------------------------
def rescale_factor(eps_c, eps_g, phi):
    """r_b (B,) float64."""
    B = eps_c.shape[0]
    sc = np.asarray(eps_c, dtype=np.float64).reshape(B, -1).std(axis=1)
    sg = np.asarray(eps_g, dtype=np.float64).reshape(B, -1).std(axis=1)
    ratio = np.divide(sc, sg, out=np.ones_like(sc), where=sg != 0)
    return np.where(sg != 0, phi * ratio + (1.0 - phi), 1.0)


def composed_eps(out, view_count, weighting, g=None, phi=None, dtype=np.float64):
    """out (S (+ B), Cout, H, W) torch -> (eps (B, 3, H, W) numpy `dtype`, conditional weights | None, r (B,) | None).
    The composition runs in `out`'s dtype, the guided combination (1 - g formed first) and the rescale in `dtype`."""
    from oracle import view_fusion_ref as vfr
    vc = [int(v) for v in view_count]
    S, B = sum(vc), len(vc)
    eps_c, _, w = vfr.compose(out[:S], vc, weighting)
    eps_c = eps_c.numpy().astype(dtype)
    if g is None:
        assert out.shape[0] == S and not phi
        return eps_c, w, None
    assert out.shape[0] == S + B
    eps_u = out[S:, :3].numpy().astype(dtype)
    gv = np.asarray(g, dtype=dtype).reshape(-1)
    gv = (np.full(B, gv[0], dtype=dtype) if gv.size == 1 else gv).reshape(B, 1, 1, 1)
    gm = (1.0 - gv).astype(dtype)
    eps_g = gv * eps_c + gm * eps_u
    if not phi:
        return eps_g, w, None
    r = rescale_factor(eps_c, eps_g, phi)
    return (r.reshape(B, 1, 1, 1).astype(dtype) * eps_g).astype(dtype), w, r


# ---- the steps --------------------------------------------------------------------------------------------------------
def ancestral_step(sched, t, y, eps, z, q=None, c=None, clip=True):
    """The posterior step from a given eps: sched = the six fp32 buffers, t an int -> (y_next, mean, y0, s | None);
    arithmetic in y's dtype."""
    dt = y.dtype
    pick = lambda k: dt.type(float(sched[k][t]))
    y0, s = bound(pick("sqrt_recip_gammas") * y - pick("sqrt_recipm1_gammas") * eps, q, c, clip)
    mean = pick("posterior_mean_coef1") * y0 + pick("posterior_mean_coef2") * y
    if t == 0:
        return mean, mean, y0, s
    return mean + z * dt.type(math.exp(0.5 * float(sched["posterior_log_variance_clipped"][t]))), mean, y0, s


def sampler_step(betas, tau, solver, eta, k, y, eps, y0_prev, z, q=None, c=None):
    """One few-step update from a given eps -> (y_new, y0, s | None).  float64: sampler_ref.update from the bounded y0;
    any other dtype: the linear form with sampler_ref.tables' coefficients rounded to that dtype."""
    (al_t, sg_t, _), _ = sampler_ref._levels(betas, tau, k)
    dt = y.dtype
    if dt == np.float64:
        y0, s = bound((y - sg_t * eps) / al_t, q, c)
        return sampler_ref.update(betas, tau, solver, eta, k, y, y0, y0_prev, z), y0, s
    tab = {n: dt.type(v[k]) for n, v in sampler_ref.tables(betas, tau, solver, eta).items()}
    y0, s = bound(tab["a"] * y - tab["b"] * eps, q, c)
    y_new = tab["cy"] * y + tab["c0"] * y0
    if tab["c1"] != 0:
        y_new = y_new + tab["c1"] * y0_prev
    if tab["sigma"] != 0:
        y_new = y_new + tab["sigma"] * z
    return y_new.astype(dt), y0.astype(dt), s


def chain(unet_fn, betas, y_cond, view_count, angle, y_T, z_seq, g, tau=None, solver="ddim", eta=0.0, weighting=True,
          q=None, c=None, phi=None, dtype=np.float64):
    """guidance_ref.chain with the threshold and the rescale: the network in fp32 (the S real rows and the B null rows in
    two calls), everything after it in `dtype`.  -> (states after every step, float32 (steps, B, 3, H, W); weights)."""
    import guidance_ref
    from oracle import view_fusion_ref as vfr
    sched = vfr.schedule_buffers(betas)
    gammas32 = sched["gammas"]
    vc = [int(v) for v in view_count]
    B, S = len(vc), sum(vc)
    y = y_T.numpy().astype(dtype)
    y0_prev = np.full_like(y, np.nan)
    steps = list(reversed(range(len(betas) if tau is None else len(tau))))
    states, weights = [], []
    for k in steps:
        t = k if tau is None else int(tau[k])
        level = gammas32[t].reshape(1, 1).repeat(B, 1)
        x, ang_s, lvl_s = guidance_ref.stack(y_cond, vc, torch.tensor(y).float(), level, angle, null_rows=True)
        out = torch.cat([unet_fn(x[:S], ang_s[:S], lvl_s[:S]), unet_fn(x[S:], ang_s[S:], lvl_s[S:])], dim=0)
        eps, w, _ = composed_eps(out, vc, weighting, g, phi, dtype)
        z = dtype(0.0) if z_seq is None else z_seq[t].numpy().astype(dtype)
        if tau is None:
            y, _, _, _ = ancestral_step(sched, t, y, eps, z, q, c)
        else:
            y, y0_prev, _ = sampler_step(betas, tau, solver, eta, k, y, eps, y0_prev, z, q, c)
        y = np.asarray(y, dtype=dtype)
        states.append(torch.tensor(y).float())
        weights.append(w)
    return torch.stack(states), weights
