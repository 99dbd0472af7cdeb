"""DDPM noise schedules (host side, float64 numpy -> six fp32 buffers).

Same formulas and buffer names as the reference (model/view_fusion.py:35-68, 321-362);
computed once per `set_new_noise_schedule`, never on the hot path.
"""
import math

import numpy as np
import torch

BUFFER_NAMES = ("gammas", "sqrt_recip_gammas", "sqrt_recipm1_gammas", "posterior_log_variance_clipped",
                "posterior_mean_coef1", "posterior_mean_coef2")


def make_beta_schedule(schedule, num_timesteps, linear_start=1e-6, linear_end=1e-2, cosine_s=8e-3):
    n = int(num_timesteps)

    def warm(frac):
        out = linear_end * np.ones(n, dtype=np.float64)
        k = int(n * frac)
        out[:k] = np.linspace(linear_start, linear_end, k, dtype=np.float64)
        return out

    table = {
        "linear": lambda: np.linspace(linear_start, linear_end, n, dtype=np.float64),
        "quad": lambda: np.linspace(linear_start ** 0.5, linear_end ** 0.5, n, dtype=np.float64) ** 2,
        "warmup10": lambda: warm(0.1),
        "warmup50": lambda: warm(0.5),
        "const": lambda: linear_end * np.ones(n, dtype=np.float64),
        "jsd": lambda: 1.0 / np.linspace(n, 1, n, dtype=np.float64),
    }
    if schedule in table:
        return table[schedule]()
    if schedule == "cosine":
        ts = torch.arange(n + 1, dtype=torch.float64) / n + cosine_s
        al = torch.cos(ts / (1 + cosine_s) * math.pi / 2).pow(2)
        al = al / al[0]
        return (1 - al[1:] / al[:-1]).clamp(max=0.999).numpy()
    raise NotImplementedError(schedule)


def schedule_tensors(betas, device):
    betas = np.asarray(betas, dtype=np.float64)
    alphas = 1.0 - betas
    gammas = np.cumprod(alphas, axis=0)
    prev = np.append(1.0, gammas[:-1])
    with np.errstate(divide="ignore", invalid="ignore"):
        var = betas * (1.0 - prev) / (1.0 - gammas)
        vals = (gammas, np.sqrt(1.0 / gammas), np.sqrt(1.0 / gammas - 1), np.log(np.maximum(var, 1e-20)),
                betas * np.sqrt(prev) / (1.0 - gammas), (1.0 - prev) * np.sqrt(alphas) / (1.0 - gammas))
    return {k: torch.tensor(v, dtype=torch.float32, device=device) for k, v in zip(BUFFER_NAMES, vals)}


# ---- few-step sampling: a sub-sequence of the trained schedule and the tables of one linear-multistep tail ----------
# Every sampler here is, per element and after the compose,
#     y0 = clamp(a[k] y - b[k] eps, -1, 1);   y_new = cy[k] y + c0[k] y0 + c1[k] y0_prev + sigma[k] z
# (csrc/diffusion.hip: sampler_step_kernel).  Step k works at the trained level gammas[tau[k]] and lands on
# gammas[tau[k-1]] (on the clean image, gamma = 1, at k = 0); the chain runs k = K-1 ... 0.
SOLVERS = ("ddim", "dpmpp2m")
TABLE_NAMES = ("a", "b", "cy", "c0", "c1", "sigma")


def sample_timesteps(T, K):
    """The model timesteps of a K-step chain, int64 (K,): tau[k] = ((k+1) T) // K - 1 -- strictly increasing, ending at
    T-1 (sampling starts from pure noise, the last trained level), 0..T-1 at K = T.  Instead of K an explicit strictly
    increasing integer sequence in [0, T-1] that ends at T-1 is accepted."""
    T = int(T)
    if torch.is_tensor(K):
        K = K.detach().cpu().tolist()
    if isinstance(K, (bool, float, np.floating)):
        raise ValueError(f"sample_steps must be an integer or a sequence of integers, got {K!r}")
    if isinstance(K, (int, np.integer)):
        K = int(K)
        if not 1 <= K <= T:
            raise ValueError(f"sample_steps must be in [1, {T}], got {K}")
        return np.array([((k + 1) * T) // K - 1 for k in range(K)], dtype=np.int64)
    seq = list(K)
    if not seq or any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) for v in seq):
        raise ValueError("sample_steps as a sequence needs at least one timestep, all integers")
    tau = np.array(seq, dtype=np.int64)
    if tau[0] < 0 or tau[-1] != T - 1 or (np.diff(tau) <= 0).any():
        raise ValueError(f"sample_steps as a sequence must increase strictly within [0, {T - 1}] and end at {T - 1}")
    return tau


def check_sampler(solver, eta):
    if solver not in SOLVERS:
        raise ValueError(f"unknown solver {solver!r}: one of {SOLVERS}")
    if not 0.0 <= float(eta) <= 1.0:
        raise ValueError(f"eta must be in [0, 1], got {eta}")
    if solver == "dpmpp2m" and float(eta) != 0.0:
        raise ValueError("dpmpp2m is deterministic: eta must be 0")


def sampler_tables(betas, tau, solver="ddim", eta=0.0):
    """float64 betas (T,), tau (K,) -> {a, b, cy, c0, c1, sigma}: float64 (K,) each (rounded to fp32 once, by the caller).

    ddim     DDIM with eps re-derived from the clamped y0; eta = 1 on the full schedule is the ancestral sampler.
    dpmpp2m  DPM-Solver++ 2M in lambda = log(alpha / sigma); the first executed step (k = K-1, no history yet) and the
             last (k = 0, onto the clean image) are first order, which is the ddim eta = 0 step.
    """
    check_sampler(solver, eta)
    betas = np.asarray(betas, dtype=np.float64)
    tau = np.asarray(tau, dtype=np.int64)
    gammas = np.cumprod(1.0 - betas, axis=0)
    gt = gammas[tau]
    gp = np.append(1.0, gt[:-1])
    K = tau.shape[0]
    out = {"a": np.sqrt(1.0 / gt), "b": np.sqrt(1.0 / gt - 1), "c1": np.zeros(K), "sigma": np.zeros(K)}
    if solver == "ddim":
        sig = float(eta) * np.sqrt((1.0 - gp) / (1.0 - gt)) * np.sqrt(1.0 - gt / gp)
        # d = sqrt(1 - gp - sig^2).  Written out, the difference loses every digit where gt << gp (a long stride at
        # eta = 1); with q = (1 - gt/gp) / (1 - gt) it is (1 - gp) (1 - eta^2 q) and 1 - q = gt (1 - gp) / (gp (1 - gt)).
        e2 = float(eta) ** 2
        d = np.sqrt((1.0 - gp) * ((1.0 - e2) + e2 * gt * (1.0 - gp) / (gp * (1.0 - gt))))
        out.update(cy=d / np.sqrt(1.0 - gt), c0=np.sqrt(gp) - d * np.sqrt(gt) / np.sqrt(1.0 - gt), sigma=sig)
        return out
    with np.errstate(divide="ignore"):
        lam = 0.5 * np.log(gt / (1.0 - gt))
        lam_p = 0.5 * np.log(gp / (1.0 - gp))           # +inf at k = 0: h = inf, expm1(-h) = -1
    h = lam_p - lam
    g = -np.sqrt(gp) * np.expm1(-h)
    out.update(cy=np.sqrt((1.0 - gp) / (1.0 - gt)), c0=g.copy())
    for k in range(1, K - 1):
        r = (lam[k] - lam[k + 1]) / h[k]
        out["c0"][k] = g[k] * (1.0 + 1.0 / (2.0 * r))
        out["c1"][k] = -g[k] / (2.0 * r)
    return out
