"""The analytic variance (Analytic-DPM, Bao et al., ICLR 2022), restated in numpy from the definition at the head of
view_fusion_amd/csrc/diffusion.hip ("Analytic variance") -- written from the formulas, not from schedule.py or the
kernel -- and parameterised by dtype: float64 is the oracle, float32 the yardstick for the rounding noise of the formulas
themselves (the tests give the device a margin over the float32 run's own distance from float64, never a number fixed in
advance).

    eps_hat = ea y_k + eb out_b        eps: (0, 1)   v: (sqrt(1 - g), sqrt(g))   x0: (1 / sqrt(1 - g), -sqrt(g / (1 - g)))
    m2[b]   = mean over 3 H W of eps_hat^2
    sigma*^2[k] = lambda^2[k] + c[k]^2 (1 - gt) / gt (1 - clip(M[tau[k]], 0, 1))
    c[k] = sqrt(gp) - sqrt(1 - gp - lambda^2) sqrt(gt / (1 - gt)),  lambda^2 = eta^2 (1 - gp) / (1 - gt) (1 - gt / gp)
"""
import itertools

import numpy as np

import nll_ref


def eps_coeffs(g, prediction, dt=np.float64):
    """(ea, eb) at the level(s) g, formed in float64 and rounded to dt once, as the tables are."""
    g = np.asarray(g, dtype=np.float64)
    if prediction == "eps":
        ea, eb = np.zeros_like(g), np.ones_like(g)
    elif prediction == "v":
        ea, eb = np.sqrt(1.0 - g), np.sqrt(g)
    else:
        ea, eb = 1.0 / np.sqrt(1.0 - g), -np.sqrt(g / (1.0 - g))
    return ea.astype(dt), eb.astype(dt)


def eps_element(ea, eb, out, y, dt=np.float64):
    """Per element: the noise estimate (each product rounded, then added) and its square."""
    ay = np.asarray(ea, dtype=dt) * np.asarray(y, dtype=dt)
    bo = np.asarray(eb, dtype=dt) * np.asarray(out, dtype=dt)
    e = (ay + bo).astype(dt)
    return e, (e * e).astype(dt)


def moment(out, vc, weighting, y_k, ea, eb, dt=np.float64):
    """m2 (B,): out (S, C, H, W) composed over each sample's views (channels 6..8 ignored), row (ea, eb) per sample or
    one for all."""
    e_b, _ = nll_ref.compose(np.asarray(out)[:, :6], vc, weighting, dt)
    B = len(vc)
    ea = np.broadcast_to(np.asarray(ea, dtype=dt).reshape(-1), (B,)).reshape(B, 1, 1, 1)
    eb = np.broadcast_to(np.asarray(eb, dtype=dt).reshape(-1), (B,)).reshape(B, 1, 1, 1)
    _, sq = eps_element(ea, eb, e_b, y_k, dt)
    assert sq.dtype == dt
    return sq.reshape(B, -1).mean(axis=1, dtype=dt)


def _chain(betas, tau):
    gam = np.cumprod(1.0 - np.asarray(betas, dtype=np.float64))
    gt = gam[np.asarray(tau, dtype=np.int64)]
    return gt, np.append(1.0, gt[:-1])


def lambda2(betas, tau, eta):
    gt, gp = _chain(betas, tau)
    return eta ** 2 * (1.0 - gp) / (1.0 - gt) * (1.0 - gt / gp)


def mean_coef(betas, tau, eta):
    """c[k]: the weight of y0 in the mean of the "ddim" step, written with its difference (fine for the grids here)."""
    gt, gp = _chain(betas, tau)
    return np.sqrt(gp) - np.sqrt(np.maximum(1.0 - gp - lambda2(betas, tau, eta), 0.0)) * np.sqrt(gt / (1.0 - gt))


def sigma2(betas, tau, moments, eta=1.0):
    gt, _ = _chain(betas, tau)
    m = np.clip(np.asarray(moments, dtype=np.float64)[np.asarray(tau)], 0.0, 1.0)
    c = mean_coef(betas, tau, eta)
    return lambda2(betas, tau, eta) + c * c * (1.0 - gt) / gt * (1.0 - m)


def gaussian_moment(betas, s2):
    """M[t] of the exact noise estimate of data drawn from N(0, s2): (1 - g) / (g s2 + 1 - g)."""
    g = np.cumprod(1.0 - np.asarray(betas, dtype=np.float64))
    return (1.0 - g) / (g * s2 + 1.0 - g)


def gaussian_sigma2(betas, tau, eta, s2):
    """The closed form for N(0, s2) data: lambda^2 + c^2 s2 (1 - gt) / (gt s2 + 1 - gt); at eta = 1 the exact variance of
    q(y_tau[k-1] | y_tau[k])."""
    gt, _ = _chain(betas, tau)
    c = mean_coef(betas, tau, eta)
    return lambda2(betas, tau, eta) + c * c * s2 * (1.0 - gt) / (gt * s2 + 1.0 - gt)


def gaussian_posterior_variance(betas, tau, s2):
    """Var(y_tau[k-1] | y_tau[k]) for N(0, s2) data from the joint Gaussian itself (k >= 1; row 0 is Var(y_0 | y_tau[0]))."""
    gt, gp = _chain(betas, tau)
    var_p, var_t = gp * s2 + 1.0 - gp, gt * s2 + 1.0 - gt
    cov = np.sqrt(gt / gp) * var_p
    return var_p - cov * cov / var_t


def step_cost(betas, moments, r, s):
    """J(r, s) = log(sigma*^2 / lambda^2) of the eta = 1 step from level s down to r < s."""
    gam = np.cumprod(1.0 - np.asarray(betas, dtype=np.float64))
    gp, gt = gam[r], gam[s]
    lam2 = (1.0 - gp) / (1.0 - gt) * (1.0 - gt / gp)
    c = np.sqrt(gp) * (1.0 - gt / gp) / (1.0 - gt)
    m = min(max(float(moments[s]), 0.0), 1.0)
    return float(np.log((lam2 + c * c * (1.0 - gt) / gt * (1.0 - m)) / lam2))


def chain_cost(betas, moments, tau):
    return sum(step_cost(betas, moments, int(tau[k - 1]), int(tau[k])) for k in range(1, len(tau)))


def brute_force_trajectory(betas, moments, K, first=0):
    """Every strictly increasing K-chain from `first` to T - 1 -> (the cheapest, its cost)."""
    T = len(betas)
    if K == 1:
        return (T - 1,), 0.0
    best = None
    for mid in itertools.combinations(range(first + 1, T - 1), K - 2):
        tau = (first,) + mid + (T - 1,)
        c = chain_cost(betas, moments, tau)
        if best is None or c < best[1]:
            best = (tau, c)
    return best
