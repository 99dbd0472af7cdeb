"""Test infrastructure: a float64 numpy restatement of the few-step samplers (strided DDIM, DPM-Solver++ 2M), stated
from the update rules in (alpha, sigma, lambda) form with an explicit eps -- not from the folded cy / c0 / c1 tables of
view_fusion_amd/schedule.py, which the product never shares with this file and which never imports it.

With gamma the cumulative product of 1 - beta:  alpha = sqrt(gamma), sigma = sqrt(1 - gamma), lambda = log(alpha / sigma).
Step k of a K-step chain (k = K-1 ... 0) goes from level t = tau[k] to level p = tau[k-1]; at k = 0 the target is the clean
image: alpha_p = 1, sigma_p = 0, lambda_p = +inf.

    y0 = clip((y - sigma_t eps) / alpha_t, -1, 1)

    ddim      s = eta (sigma_p / sigma_t) sqrt(1 - alpha_t^2 / alpha_p^2)
              eps' = (y - alpha_t y0) / sigma_t                      (eps re-derived from the clamped y0)
              y_new = alpha_p y0 + sqrt(sigma_p^2 - s^2) eps' + s z           (Song et al., DDIM, eq. 12)

    dpmpp2m   h = lambda_p - lambda_t,  r = (lambda_t - lambda_{tau[k+1]}) / h
              D = (1 + 1/(2r)) y0 - (1/(2r)) y0_prev       (D = y0 on the first executed step and on the last step)
              y_new = (sigma_p / sigma_t) y - alpha_p expm1(-h) D             (Lu et al., DPM-Solver++, algorithm 2)
"""
import numpy as np
import torch


def timesteps(T, K):
    """K model timesteps, evenly strided and ending at T - 1."""
    return np.array([((k + 1) * T) // K - 1 for k in range(K)], dtype=np.int64)


def _levels(betas, tau, k):
    """(alpha_t, sigma_t, lambda_t), (alpha_p, sigma_p, lambda_p) of step k."""
    gamma = np.cumprod(1.0 - np.asarray(betas, dtype=np.float64))

    def at(g):
        al, sg = np.sqrt(g), np.sqrt(1.0 - g)
        return al, sg, (np.log(al / sg) if sg > 0 else np.inf)

    return at(gamma[tau[k]]), (at(gamma[tau[k - 1]]) if k > 0 else (1.0, 0.0, np.inf))


def update(betas, tau, solver, eta, k, y, y0, y0_prev, z):
    """y_new from the clamped y0 (float64 arrays or scalars).  y0_prev is touched only by a second-order step."""
    (al_t, sg_t, lam_t), (al_p, sg_p, lam_p) = _levels(betas, tau, k)
    if solver == "ddim":
        s = eta * (sg_p / sg_t) * np.sqrt(1.0 - al_t ** 2 / al_p ** 2)
        eps = (y - al_t * y0) / sg_t
        # sigma_p^2 - s^2 cancels to its last bits where alpha_t << alpha_p and eta = 1; the identity
        # 1 - (1 - alpha_t^2 / alpha_p^2) / sigma_t^2 = (alpha_t sigma_p / (alpha_p sigma_t))^2 gives it without a
        # difference (test_sampler_host checks this line against the difference itself in 60-digit arithmetic)
        e2 = eta ** 2
        rest = sg_p ** 2 * ((1.0 - e2) + e2 * (al_t * sg_p / (al_p * sg_t)) ** 2)
        y_new = al_p * y0 + np.sqrt(rest) * eps
        return y_new + s * z if s != 0 else y_new
    assert solver == "dpmpp2m" and eta == 0
    h = lam_p - lam_t
    D = y0
    if 0 < k < len(tau) - 1:
        lam_last = _levels(betas, tau, k + 1)[0][2]
        r = (lam_t - lam_last) / h
        D = (1.0 + 1.0 / (2.0 * r)) * y0 - (1.0 / (2.0 * r)) * y0_prev
    return (sg_p / sg_t) * y - al_p * np.expm1(-h) * D


def step(betas, tau, solver, eta, k, y, eps, y0_prev, z):
    """One step from the composed eps: -> (y_new, y0), float64."""
    (al_t, sg_t, _), _ = _levels(betas, tau, k)
    y, eps = np.asarray(y, dtype=np.float64), np.asarray(eps, dtype=np.float64)
    y0 = np.clip((y - sg_t * eps) / al_t, -1.0, 1.0)
    return update(betas, tau, solver, eta, k, y, y0, y0_prev, z), y0


def tables(betas, tau, solver, eta):
    """The coefficients of the (linear) update, found by probing it with unit inputs; a, b from y0's definition."""
    K = len(tau)
    out = {n: np.zeros(K) for n in ("a", "b", "cy", "c0", "c1", "sigma")}
    for k in range(K):
        (al_t, sg_t, _), _ = _levels(betas, tau, k)
        out["a"][k], out["b"][k] = 1.0 / al_t, sg_t / al_t
        for name, probe in (("cy", (1.0, 0.0, 0.0, 0.0)), ("c0", (0.0, 1.0, 0.0, 0.0)), ("c1", (0.0, 0.0, 1.0, 0.0)),
                            ("sigma", (0.0, 0.0, 0.0, 1.0))):
            out[name][k] = update(betas, tau, solver, eta, k, *probe)
    return out


def chain(unet_fn, compose_fn, betas, gammas32, tau, solver, eta, y_cond, view_count, angle, y_T, z_seq, weighting=True):
    """The K-step chain through a CPU UNet.  unet_fn(x, angle_s, level_s) and compose_fn(out, view_count, weighting) are
    oracle.unet_ref.unet_forward (bound to its weights) and oracle.view_fusion_ref.compose; the network runs in fp32
    at the fp32 level gammas32[tau[k]], the update in float64.  z_seq is (T, ...), indexed by the MODEL timestep.
    -> (states after step K-1 ... 0, float32 (K,B,3,H,W); weights of each step)."""
    from oracle import view_fusion_ref as vfr
    B = y_cond.shape[0]
    y = y_T.double().numpy()
    y0_prev = np.full_like(y, np.nan)
    states, weights = [], []
    for k in reversed(range(len(tau))):
        level = gammas32[int(tau[k])].reshape(1, 1).repeat(B, 1)
        x, ang_s, lvl_s = vfr.stack_views(y_cond, view_count, torch.tensor(y).float(), level, angle)
        eps, _, w = compose_fn(unet_fn(x, ang_s, lvl_s), view_count, weighting)
        z = 0.0 if z_seq is None else z_seq[int(tau[k])].double().numpy()
        y, y0_prev = step(betas, tau, solver, eta, k, y, eps.double().numpy(), y0_prev, z)
        states.append(torch.tensor(y).float())
        weights.append(w)
    return torch.stack(states), weights
