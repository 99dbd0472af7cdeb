"""DDPM noise schedules (host side, float64 numpy -> six fp32 buffers).

Same formulas and buffer names as the reference (model/view_fusion.py:35-68, 321-362);
computed once per `set_new_noise_schedule`, never on the hot path.
"""
import math

import numpy as np
import torch

BUFFER_NAMES = ("gammas", "sqrt_recip_gammas", "sqrt_recipm1_gammas", "posterior_log_variance_clipped",
                "posterior_mean_coef1", "posterior_mean_coef2")


PREDICTIONS = ("eps", "v", "x0")


def rescale_zero_terminal_snr(betas):
    """Lin et al., "Common Diffusion Noise Schedules and Sample Steps are Flawed", algorithm 1, in float64: sqrt(gammas)
    is shifted and scaled so that its last value is exactly 0 and its first is unchanged -> betas (T,), the last one 1.
    The last level is then pure noise, which is what sampling starts from.  An eps-model cannot use such a schedule
    (g^-1/2 is infinite there); "v" and "x0" can (prediction_tables)."""
    betas = np.asarray(betas, dtype=np.float64)
    root = np.sqrt(np.cumprod(1.0 - betas, axis=0))
    first, last = root[0], root[-1]
    if not first > last:
        raise ValueError("rescale_zero_terminal_snr needs a schedule whose signal level decreases")
    root = (root - last) * (first / (first - last))
    gam = root ** 2
    alphas = np.append(gam[0], gam[1:] / gam[:-1])
    alphas[-1] = 0.0                                   # (root[-1] - last is exactly 0 already; said once more)
    return 1.0 - alphas


def make_beta_schedule(schedule, num_timesteps, linear_start=1e-6, linear_end=1e-2, cosine_s=8e-3,
                       zero_terminal_snr=False):
    """zero_terminal_snr=True (default False: the schedule as before): rescale_zero_terminal_snr applied on top."""
    if zero_terminal_snr:
        return rescale_zero_terminal_snr(make_beta_schedule(schedule, num_timesteps, linear_start, linear_end, cosine_s))
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


def check_prediction(prediction):
    if prediction not in PREDICTIONS:
        raise ValueError(f"unknown prediction {prediction!r}: one of {PREDICTIONS}")
    return prediction


def prediction_tables(betas, prediction="eps"):
    """float64 betas (T,) -> (a, b), float64 (T,) each (rounded to fp32 once, by the caller): y0_hat = a[t] y - b[t] out
    for a network whose output is the noise ("eps": g^-1/2, (1/g - 1)^1/2 -- schedule_tensors' own two formulas, so the
    same fp32 values as the buffers), v = sqrt(g) noise - sqrt(1 - g) y_0 ("v": sqrt(g), sqrt(1 - g)) or y_0 itself
    ("x0": 0, -1); csrc/diffusion.hip holds the definition.  With gamma = 0 (a zero-terminal-SNR schedule) the "eps" pair
    is infinite there (no warning is raised here; sampling refuses it), the other two are finite."""
    check_prediction(prediction)
    gammas = np.cumprod(1.0 - np.asarray(betas, dtype=np.float64), axis=0)
    if prediction == "eps":
        with np.errstate(divide="ignore"):
            return np.sqrt(1.0 / gammas), np.sqrt(1.0 / gammas - 1)
    if prediction == "v":
        return np.sqrt(gammas), np.sqrt(1.0 - gammas)
    return np.zeros_like(gammas), -np.ones_like(gammas)


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


def sampler_tables(betas, tau, solver="ddim", eta=0.0, prediction="eps", moments=None):
    """float64 betas (T,), tau (K,) -> {a, b, cy, c0, c1, sigma}: float64 (K,) each (rounded to fp32 once, by the caller).
    prediction: a, b = prediction_tables gathered at tau; cy, c0, c1, sigma do not depend on it.  Where a level of the
    chain is 0 (zero terminal SNR) "eps" raises ValueError, and the other two give finite tables: the dpmpp2m step next
    to lambda = -inf is first order (r = inf, c1 = 0).

    ddim     DDIM with eps re-derived from the clamped y0; eta = 1 on the full schedule is the ancestral sampler.
    dpmpp2m  DPM-Solver++ 2M in lambda = log(alpha / sigma); the first executed step (k = K-1, no history yet) and the
             last (k = 0, onto the clean image) are first order, which is the ddim eta = 0 step.

    moments (default None: the tables as before): the per-level second moment of the model's noise estimate, (T,) -- the
    sigma row of the "ddim" tables becomes the analytic one (analytic_sampler_sigma: the KL-optimal noise scale around
    the same mean, sigma*[0] = 0); every other row is unchanged.  ValueError with "dpmpp2m".
    """
    check_sampler(solver, eta)
    if moments is not None and solver != "ddim":
        raise ValueError("the analytic variance goes with solver 'ddim' alone: dpmpp2m is deterministic")
    betas = np.asarray(betas, dtype=np.float64)
    tau = np.asarray(tau, dtype=np.int64)
    gammas = np.cumprod(1.0 - betas, axis=0)
    gt = gammas[tau]
    gp = np.append(1.0, gt[:-1])
    K = tau.shape[0]
    if check_prediction(prediction) == "eps" and (gt == 0).any():
        raise ValueError("an eps-prediction model cannot sample from a level with gamma = 0 (zero terminal SNR): "
                         "g^-1/2 is infinite there; use prediction 'v' or 'x0'")
    pa, pb = prediction_tables(betas, prediction)
    out = {"a": pa[tau], "b": pb[tau], "c1": np.zeros(K), "sigma": np.zeros(K)}
    if solver == "ddim":
        sig = float(eta) * np.sqrt((1.0 - gp) / (1.0 - gt)) * np.sqrt(1.0 - gt / gp)
        # d = sqrt(1 - gp - sig^2).  Written out, the difference loses every digit where gt << gp (a long stride at
        # eta = 1); with q = (1 - gt/gp) / (1 - gt) it is (1 - gp) (1 - eta^2 q) and 1 - q = gt (1 - gp) / (gp (1 - gt)).
        e2 = float(eta) ** 2
        d = np.sqrt((1.0 - gp) * ((1.0 - e2) + e2 * gt * (1.0 - gp) / (gp * (1.0 - gt))))
        out.update(cy=d / np.sqrt(1.0 - gt), c0=np.sqrt(gp) - d * np.sqrt(gt) / np.sqrt(1.0 - gt), sigma=sig)
        if moments is not None:
            out["sigma"] = analytic_sampler_sigma(betas, tau, moments, eta)
        return out
    with np.errstate(divide="ignore"):
        lam = 0.5 * np.log(gt / (1.0 - gt))
        lam_p = 0.5 * np.log(gp / (1.0 - gp))           # +inf at k = 0: h = inf, expm1(-h) = -1
    h = lam_p - lam
    g = -np.sqrt(gp) * np.expm1(-h)
    out.update(cy=np.sqrt((1.0 - gp) / (1.0 - gt)), c0=g.copy())
    for k in range(1, K - 1):
        r = (lam[k] - lam[k + 1]) / h[k]                # +inf next to lambda = -inf (gamma = 0): a first-order step
        out["c0"][k] = g[k] * (1.0 + 1.0 / (2.0 * r))
        out["c1"][k] = -g[k] / (2.0 * r) + 0.0          # (+ 0.0: no negative zero in the table)
    return out


# ---- learned variance: the two log-variances a reverse step interpolates between (csrc/diffusion.hip) ---------------
def variance_tables(betas, tau=None):
    """float64 betas (T,), tau (K,) (default 0..T-1) -> (hi, lo), float64 (K,) each (rounded to fp32 once, by the caller).
    With gt = gammas[tau[k]], gp = gammas[tau[k-1]] (1 at k = 0): hi[k] = log(1 - gt/gp), the log of the chain's own beta,
    and lo[k] = log(max((1 - gt/gp)(1 - gp)/(1 - gt), 1e-20)), the log of its posterior variance, clipped as
    posterior_log_variance_clipped is: on the full schedule hi = log(betas) and lo equals that buffer value for value."""
    betas = np.asarray(betas, dtype=np.float64)
    if tau is None or np.array_equal(np.asarray(tau), np.arange(betas.shape[0])):
        # the schedule's own steps: schedule_tensors' very expressions
        gammas = np.cumprod(1.0 - betas, axis=0)
        prev = np.append(1.0, gammas[:-1])
        with np.errstate(divide="ignore", invalid="ignore"):
            var = betas * (1.0 - prev) / (1.0 - gammas)
            return np.log(betas), np.log(np.maximum(var, 1e-20))
    tau = np.asarray(tau, dtype=np.int64)
    gammas = np.cumprod(1.0 - betas, axis=0)
    gt = gammas[tau]
    gp = np.append(1.0, gt[:-1])
    beta = 1.0 - gt / gp
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.log(beta), np.log(np.maximum(beta * (1.0 - gp) / (1.0 - gt), 1e-20))


# ---- the variational bound: the rows a term of the bound reads (csrc/diffusion.hip, "Variational bound") -------------
FIXED_VARIANCES = ("small", "large")


ANALYTIC_VARIANCE = "analytic"                    # the moment-based optimal variance (analytic_sigma2, below)
BOUND_VARIANCES = FIXED_VARIANCES + (ANALYTIC_VARIANCE,)


def nll_tables(betas, tau=None, prediction="eps", fixed_variance="small", moments=None):
    """float64 betas (T,), tau (K,) (default 0..T-1) -> {a, b, c0, hi, lo}: float64 (K,) each (rounded to fp32 once, by the
    caller).  With gt = gammas[tau[k]], gp = gammas[tau[k-1]] (1 at k = 0): a, b = prediction_tables gathered at tau;
    c0[k] = sqrt(gp) (1 - gt/gp) / (1 - gt), the weight of y0 in the posterior mean; hi, lo = variance_tables.  On the full
    chain these are schedule_tensors' own expressions, so rows k >= 1 equal posterior_mean_coef1, log(betas) and
    posterior_log_variance_clipped value for value.  Row 0 is the decoder's: hi[0] = log(1 - gammas[tau[0]]) and lo[0] =
    lo[1], the log posterior variance of step 1 (not the 1e-20 clipping, under which the likelihood degenerates);
    a one-step chain has lo[0] = hi[0]; fixed_variance="large" (lp = hi) reads lo[0] at k = 0 as well, so its hi[0] = lo[0].
    ValueError for an eps model on a level with gamma = 0, as sampler_tables.
    fixed_variance="analytic" with moments (T,) (the per-level second moment of the noise estimate,
    drivers.estimate_moments): hi[k] = log sigma*^2[k], the Analytic-DPM optimal variance of the chain at eta = 1 --
    lambda^2 the chain's posterior variance, c0 the column above -- and hi[0] = log max(sigma*^2[0], exp(lo[0])), never
    below the decoder row "small" uses; lo stays the true posterior's.  The term kernel reads it as it reads "large".
    ValueError there for a level with gamma = 0 or a NaN moment on the chain, and for moments without "analytic"."""
    analytic = fixed_variance == ANALYTIC_VARIANCE
    if analytic != (moments is not None):
        raise ValueError("fixed_variance='analytic' and moments= come together")
    if fixed_variance not in FIXED_VARIANCES and not analytic:
        raise ValueError(f"unknown fixed_variance {fixed_variance!r}: one of {FIXED_VARIANCES}")
    betas = np.asarray(betas, dtype=np.float64)
    T = betas.shape[0]
    gammas = np.cumprod(1.0 - betas, axis=0)
    full = tau is None or np.array_equal(np.asarray(tau), np.arange(T))
    tau = np.arange(T, dtype=np.int64) if full else np.asarray(tau, dtype=np.int64)
    gt = gammas[tau]
    if check_prediction(prediction) == "eps" and (gt == 0).any():
        raise ValueError("an eps-prediction model cannot sample from a level with gamma = 0 (zero terminal SNR): "
                         "g^-1/2 is infinite there; use prediction 'v' or 'x0'")
    pa, pb = prediction_tables(betas, prediction)
    hi, lo = variance_tables(betas, None if full else tau)
    with np.errstate(divide="ignore", invalid="ignore"):
        if full:                                   # schedule_tensors' very expression for posterior_mean_coef1
            prev = np.append(1.0, gammas[:-1])
            c0 = betas * np.sqrt(prev) / (1.0 - gammas)
        else:
            gp = np.append(1.0, gt[:-1])
            c0 = np.sqrt(gp) * (1.0 - gt / gp) / (1.0 - gt)
        hi, lo = hi.copy(), lo.copy()
        hi[0] = np.log(1.0 - gt[0])
        lo[0] = lo[1] if tau.shape[0] > 1 else hi[0]
    if fixed_variance == "large":
        hi[0] = lo[0]
    if analytic:
        with np.errstate(divide="ignore", invalid="ignore"):
            if full:                               # the posterior variance as schedule_tensors forms it, unclipped
                lam2 = betas * (1.0 - prev) / (1.0 - gammas)
            else:
                lam2 = (1.0 - gt / gp) * (1.0 - gp) / (1.0 - gt)
        sig2 = _analytic_sigma2(lam2, c0, gt, _moments_at(moments, tau, T))
        hi = np.log(np.maximum(sig2, 1e-20))       # (the clipping lo carries: hi >= lo in every row)
        hi[0] = max(hi[0], lo[0])                  # max(sigma*^2[0], exp(lo_dec)), in logarithms
    return {"a": pa[tau], "b": pb[tau], "c0": c0, "hi": hi, "lo": lo}


# ---- the analytic variance (Analytic-DPM; csrc/diffusion.hip, "Analytic variance") -----------------------------------
def eps_tables(betas, tau=None, prediction="eps"):
    """float64 betas (T,), tau (K,) (default 0..T-1) -> {ea, eb}: float64 (K,) each (rounded to fp32 once, by the caller):
    the noise a network's output stands for, eps_hat = ea[k] y + eb[k] out at g = gammas[tau[k]] -- "eps": (0, 1);
    "v": (sqrt(1 - g), sqrt(g)); "x0": (1 / sqrt(1 - g), -sqrt(g / (1 - g)))."""
    check_prediction(prediction)
    gammas = np.cumprod(1.0 - np.asarray(betas, dtype=np.float64), axis=0)
    g = gammas if tau is None else gammas[np.asarray(tau, dtype=np.int64)]
    if prediction == "eps":
        return {"ea": np.zeros_like(g), "eb": np.ones_like(g)}
    if prediction == "v":
        return {"ea": np.sqrt(1.0 - g), "eb": np.sqrt(g)}
    return {"ea": 1.0 / np.sqrt(1.0 - g), "eb": -np.sqrt(g / (1.0 - g))}


def _moments_at(moments, tau, T):
    """The moments of the chain's levels, float64 (K,), clipped into [0, 1]; ValueError for a table of another length
    and for a NaN (not estimated) moment at a level the chain uses."""
    if torch.is_tensor(moments):
        moments = moments.detach().cpu().numpy()
    m = np.asarray(moments, dtype=np.float64).reshape(-1)
    if m.shape[0] != T:
        raise ValueError(f"moments must hold one value per trained level ({T}), got {m.shape[0]}")
    m = m[tau]
    if np.isnan(m).any():
        raise ValueError(f"no moment was estimated at the levels {np.asarray(tau)[np.isnan(m)].tolist()} of the chain")
    return np.clip(m, 0.0, 1.0)


def _check_gamma_nonzero(g):
    if (np.asarray(g) == 0).any():
        raise ValueError("the analytic variance is not defined on a level with gamma = 0 (zero terminal SNR): "
                         "(1 - g) / g is infinite there")


def _analytic_sigma2(lam2, c0, gt, mc):
    """sigma*^2 = lambda^2 + c0^2 (1 - gt) / gt (1 - Mc), float64; ValueError for a level with gamma = 0 (0 times inf)."""
    _check_gamma_nonzero(gt)
    return lam2 + c0 * c0 * ((1.0 - gt) / gt) * (1.0 - mc)


def analytic_sigma2(betas, tau, moments, eta=1.0):
    """float64 betas (T,), tau (K,), moments (T,) -> sigma*^2 (K,) float64: the KL-optimal variance of the reverse step of
    the chain tau (Analytic-DPM, Theorem 1) around the "ddim" mean at `eta`, for a model whose noise estimate has the
    per-level second moment M[t] = E |eps_hat(y_t)|^2 / d (drivers.estimate_moments; NaN where not estimated).  With
    lambda^2 = sigma^2 and c0 of sampler_tables(betas, tau, "ddim", eta) and Mc = clip(M[tau[k]], 0, 1):
        sigma*^2[k] = lambda^2[k] + c0[k]^2 (1 - gt) / gt (1 - Mc)
    so lambda^2 <= sigma*^2 <= lambda^2 + c0^2 (1 - gt) / gt (the paper's Theorem 2), and M = 1 gives lambda^2 exactly.
    The sampler row is sqrt of this with row 0 set to 0 (analytic_sampler_sigma).  ValueError for a level with gamma = 0
    and for a NaN moment at a level of the chain."""
    betas = np.asarray(betas, dtype=np.float64)
    tau = np.asarray(tau, dtype=np.int64)
    gt = np.cumprod(1.0 - betas, axis=0)[tau]
    mc = _moments_at(moments, tau, betas.shape[0])
    _check_gamma_nonzero(gt)
    tab = sampler_tables(betas, tau, "ddim", eta, "x0")   # (sigma and c0 do not depend on the prediction)
    return _analytic_sigma2(tab["sigma"] ** 2, tab["c0"], gt, mc)


def analytic_sampler_sigma(betas, tau, moments, eta=0.0):
    """The sigma row of a sampler with the analytic variance, float64 (K,): sqrt(analytic_sigma2) with sigma*[0] = 0 --
    the last step returns its mean, as every sampler here does.  eta = 0 is Analytic-DDIM, which is stochastic."""
    sig = np.sqrt(analytic_sigma2(betas, tau, moments, eta))
    sig[0] = 0.0
    return sig


def optimal_trajectory(betas, moments, K, first=0):
    """The KL-optimal K-step sub-sequence of the trained levels (Analytic-DPM, section 5): the strictly increasing int64
    tau (K,) with tau[0] = first and tau[K-1] = T-1 that minimises sum_{k >= 1} J(tau[k-1], tau[k]), where
    J(r, s) = log(sigma*^2(r, s) / lambda^2(r, s)) is the cost, at eta = 1, of the step from level s down to r < s under
    the analytic variance.  Dynamic programming over the vectorised T x T cost matrix, float64, K T^2 work; ties go to
    the smaller timestep.  Needs a moment at every level in [first, T-1] and no level with gamma = 0 there (ValueError
    otherwise).  The result is what sample_timesteps accepts as an explicit sequence: pass it as sample_steps=."""
    betas = np.asarray(betas, dtype=np.float64)
    T = betas.shape[0]
    if isinstance(K, bool) or not isinstance(K, (int, np.integer)) or isinstance(first, bool) or \
            not isinstance(first, (int, np.integer)):
        raise ValueError(f"K and first must be integers, got {K!r}, {first!r}")
    K, first = int(K), int(first)
    if not 0 <= first <= T - 1 or not 1 <= K <= T - first or (K == 1) != (first == T - 1):
        raise ValueError(f"no strictly increasing chain of {K} steps from {first} to {T - 1}")
    lv = np.arange(first, T)
    g = np.cumprod(1.0 - betas, axis=0)[lv]
    m = _moments_at(moments, lv, T)
    _check_gamma_nonzero(g)
    n = lv.shape[0]
    gp, gt = g[:, None], g[None, :]                       # J[r, s]: from s (column) down to r (row), r < s
    with np.errstate(divide="ignore", invalid="ignore"):
        lam2 = (1.0 - gt / gp) * (1.0 - gp) / (1.0 - gt)
        c0 = np.sqrt(gp) * (1.0 - gt / gp) / (1.0 - gt)
        J = np.log((lam2 + c0 * c0 * ((1.0 - gt) / gt) * (1.0 - m[None, :])) / lam2)
    J[np.tril_indices(n)] = np.inf                        # r >= s is no step
    cost = np.full(n, np.inf)
    cost[0] = 0.0
    back = np.zeros((K, n), dtype=np.int64)
    for j in range(1, K):
        via = cost[:, None] + J                           # via[r, s]
        back[j] = np.argmin(via, axis=0)
        cost = via[back[j], np.arange(n)]
    if not np.isfinite(cost[n - 1]):
        raise ValueError(f"no strictly increasing chain of {K} steps from {first} to {T - 1}")
    tau = np.empty(K, dtype=np.int64)
    s = n - 1
    for j in range(K - 1, -1, -1):
        tau[j] = lv[s]
        s = back[j][s]
    return tau


# ---- progressive distillation: the grids and the target weights of a K-step student of a 2K-step teacher ------------
def distill_tables(betas, K, teacher_prediction="eps"):
    """float64 betas (T,), K student steps -> {tau_s (K,), tau_t (2K,) int64; w1, w2 float64 (K,); teacher, student: the two
    sampler_tables dicts} (csrc/diffusion.hip holds the definition).  tau_s / tau_t = sample_timesteps(T, K / 2K), so
    tau_t[1::2] == tau_s; teacher = sampler_tables(betas, tau_t, "ddim", 0, teacher_prediction), student = the same at
    tau_s for "eps" (only its cy, c0 take part).  w1[i] = cy_T[2i] c0_T[2i+1] / c0_S[i], w2 = 1 - w1: the student's target
    is x~ = w1 x1 + w2 x2 of the teacher's two clamped predictions, a convex combination (0 <= w1 <= 1, w1[0] = 0), and
    cy_S z + c0_S x~ is then the teacher's two-step result.  ValueError for K < 1 or 2K > T."""
    betas = np.asarray(betas, dtype=np.float64)
    T = int(betas.shape[0])
    if isinstance(K, (bool, float, np.floating)) or not isinstance(K, (int, np.integer)):
        raise ValueError(f"the student's step count must be an integer, got {K!r}")
    K = int(K)
    if K < 1 or 2 * K > T:
        raise ValueError(f"a K-step student needs a 2K-step teacher on the T = {T} schedule: 1 <= K <= {T // 2}, got {K}")
    tau_s, tau_t = sample_timesteps(T, K), sample_timesteps(T, 2 * K)
    assert (tau_t[1::2] == tau_s).all()
    teacher = sampler_tables(betas, tau_t, "ddim", 0.0, teacher_prediction)
    student = sampler_tables(betas, tau_s, "ddim", 0.0, "x0")     # (a, b unused: "x0" has them finite on every schedule)
    w1 = teacher["cy"][0::2] * teacher["c0"][1::2] / student["c0"]
    return dict(tau_s=tau_s, tau_t=tau_t, w1=w1, w2=1.0 - w1, teacher=teacher, student=student)
