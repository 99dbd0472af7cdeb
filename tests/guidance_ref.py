"""Test infrastructure: a numpy / torch float64 restatement of classifier-free guidance as view_fusion_amd/csrc/diffusion.hip
defines it -- the seeded conditioning-dropout draw, stacking with dropped samples and null rows, the guided noise and
guided reverse chains.  Nothing here calls the library; the tests compare the library with this file.

    drop(id)  = (w2 >> 8) < ceil(p 2^24),  w2 = word 2 of the kind-0, step-0, block-0 Philox call of (seed, id)
    null row  = [ 0 (all Cc conditioning channels) | y_t[b] ] with the sample's own level and angle; row S + b
    eps       = g_b eps_c + (1 - g_b) eps_u;  eps_c = compose over the sample's real rows, eps_u = channels 0..2 of its null row
"""
import math

import numpy as np
import torch

import rng_ref
import sampler_ref


# ---- the training drop draw ---------------------------------------------------------------------------------------
def drop_threshold(p):
    return int(math.ceil(float(p) * 2.0 ** 24))


def cond_drop(seed, ids, p):
    """(B,) bool: sample `id` is dropped iff (w2 >> 8) < thr -- an integer compare."""
    w2 = rng_ref.words(seed, ids, rng_ref.KIND_SCALARS, 0, 1)[:, 0, 2]
    return (w2 >> np.uint64(8)) < np.uint64(drop_threshold(p))


# ---- stacking --------------------------------------------------------------------------------------------------------
def stack(y_cond, view_count, y_t, level, angle, drop=None, null_rows=False):
    """oracle.view_fusion_ref.stack_views with the conditioning views of dropped samples zeroed and, with null_rows, one
    row [0 | y_t[b]] per sample appended (level[b], angle[b]) -> x (S (+ B), Cc + 3, H, W), angle_s, level_s."""
    from oracle import view_fusion_ref as vfr
    if drop is not None:
        y_cond = y_cond.clone()
        y_cond[torch.as_tensor(np.asarray(drop), dtype=torch.bool)] = 0
    x, ang_s, lvl_s = vfr.stack_views(y_cond, view_count, y_t, level, angle)
    if null_rows:
        B, _, Cc, H, W = y_cond.shape
        x = torch.cat([x, torch.cat([y_t.new_zeros(B, Cc, H, W), y_t], dim=1)], dim=0)
        ang_s, lvl_s = torch.cat([ang_s, angle], dim=0), torch.cat([lvl_s, level], dim=0)
    return x, ang_s, lvl_s


# ---- the guided noise ------------------------------------------------------------------------------------------------
def guided_eps(out, view_count, weighting, g):
    """out (S + B, Cout, H, W): -> (eps float64 (B, 3, H, W), conditional weights | None).  The composition runs in
    `out`'s dtype (hand a float64 `out` for a float64 restatement), the combination in float64, 1 - g formed first."""
    from oracle import view_fusion_ref as vfr
    vc = [int(v) for v in view_count]
    S, B = sum(vc), len(vc)
    assert out.shape[0] == S + B
    eps_c, _, w = vfr.compose(out[:S], vc, weighting)
    eps_u = out[S:, :3]
    g = torch.as_tensor(g, dtype=torch.float64).reshape(-1)
    g = (g.expand(B) if g.numel() == 1 else g).reshape(B, 1, 1, 1)
    gm = 1.0 - g
    return g * eps_c.double() + gm * eps_u.double(), w


# ---- guided reverse steps and chains -----------------------------------------------------------------------------------
def ancestral_step(sched, t, y, eps, z, clip=True):
    """The oracle's posterior (view_fusion_ref.p_mean_variance / p_sample) in float64 from a given eps: sched = the six
    fp32 buffers, t an int, y / eps / z float64 arrays -> (y_next, mean)."""
    pick = lambda k: float(sched[k][t])
    y0 = pick("sqrt_recip_gammas") * y - pick("sqrt_recipm1_gammas") * eps
    if clip:
        y0 = np.clip(y0, -1.0, 1.0)
    mean = pick("posterior_mean_coef1") * y0 + pick("posterior_mean_coef2") * y
    if t == 0:
        return mean, mean
    return mean + z * math.exp(0.5 * pick("posterior_log_variance_clipped")), mean


def chain(unet_fn, betas, y_cond, view_count, angle, y_T, z_seq, g, tau=None, solver="ddim", eta=0.0, weighting=True):
    """The guided chain through a CPU UNet: the ancestral chain over all T steps (tau=None; z_seq (T, ...)) or the K-step
    chain over tau (sampler_ref.step; z_seq indexed by the model timestep, None = no noise).  The network runs in fp32
    -- on the S real rows and on the B null rows in two calls, so that g = 1 reduces to sampler_ref.chain to the bit --
    and the update in float64.  -> (states after every step, float32 (steps, B, 3, H, W); weights of each step)."""
    from oracle import view_fusion_ref as vfr
    sched = vfr.schedule_buffers(betas)
    gammas32 = sched["gammas"]
    vc = [int(v) for v in view_count]
    B, S = len(vc), sum(vc)
    y = y_T.double().numpy()
    y0_prev = np.full_like(y, np.nan)
    steps = list(reversed(range(len(betas) if tau is None else len(tau))))
    states, weights = [], []
    for k in steps:
        t = k if tau is None else int(tau[k])
        level = gammas32[t].reshape(1, 1).repeat(B, 1)
        x, ang_s, lvl_s = stack(y_cond, vc, torch.tensor(y).float(), level, angle, null_rows=True)
        out = torch.cat([unet_fn(x[:S], ang_s[:S], lvl_s[:S]), unet_fn(x[S:], ang_s[S:], lvl_s[S:])], dim=0)
        eps, w = guided_eps(out, vc, weighting, g)
        z = 0.0 if z_seq is None else z_seq[t].double().numpy()
        if tau is None:
            y, _ = ancestral_step(sched, t, y, eps.numpy(), z)
        else:
            y, y0_prev = sampler_ref.step(betas, tau, solver, eta, k, y, eps.numpy(), y0_prev, z)
        states.append(torch.tensor(y).float())
        weights.append(w)
    return torch.stack(states), weights
