"""Test infrastructure: self-conditioning as the head of view_fusion_amd/csrc/diffusion.hip defines it, restated in numpy /
torch float64 on top of the existing restatements (rng_ref, guidance_ref.stack, loss_ref.compose, prediction_ref,
sampler_ref.update, threshold_ref.bound).  Nothing here calls the library; the tests compare the library with this file.

    input     row v of sample b = [ cond (Cc) | noisy target (3) | sc_b (3) ]; null row S + b = [ 0 | y_b | sc_b ]; sc = 0: none
    coin      keep(id) = (w3 >> 8) < ceil(p 2^24),  w3 = word 3 of the kind-0, step-0, block-0 Philox call of (seed, id)
    estimate  x^_b = keep_b clip(a(g) y_t - b(g) out_b, -1, 1),  out_b = the composition over the sample's views,
              (a, b) = (g^-1/2, (1/g - 1)^1/2) eps | (sqrt g, sqrt(1 - g)) v | (0, -1) x0,  g = the sample's fp32 level
    training  pass 1 (no gradient, no Dropout) on zero sc channels -> x^;  pass 2 = the ordinary step on sc = x^
    sampling  sc = the y0 the previous step's tail wrote (bounded: clamped or thresholded; guided), zeros at the first step

The q_sample expression of the stacking kernels (sa y + sb e in fp32, contracted or not as the compiler chose for
stack_views_kernel) is not restated bit for bit here: `stack` takes the noisy target as given, and the GPU test pins the
new kernel's target part to the existing kernel's bits on the same inputs.
"""
import math

import numpy as np
import torch

import guidance_ref
import loss_ref
import prediction_ref
import rng_ref


# ---- the coin ---------------------------------------------------------------------------------------------------------
def threshold(p):
    return int(math.ceil(float(p) * 2.0 ** 24))


def coin(seed, ids, p):
    """(B,) bool: sample `id` keeps its estimate iff (w3 >> 8) < thr -- an integer compare."""
    w3 = rng_ref.words(seed, ids, rng_ref.KIND_SCALARS, 0, 1)[:, 0, 3]
    return (w3 >> np.uint64(8)) < np.uint64(threshold(p))


# ---- the estimate -----------------------------------------------------------------------------------------------------
def coeffs(level, prediction):
    """(a, b) float64 of the (fp32) levels, from the formulas of the definition."""
    g = np.asarray(level, dtype=np.float32).astype(np.float64)
    if prediction == "eps":
        return np.sqrt(1.0 / g), np.sqrt(1.0 / g - 1.0)
    if prediction == "v":
        return np.sqrt(g), np.sqrt(1.0 - g)
    if prediction == "x0":
        return np.zeros_like(g), -np.ones_like(g)
    raise ValueError(prediction)


def estimate(out, view_count, weighting, level, prediction, y_t, keep=None):
    """x^ float64 (B, 3, H, W) from the first pass's raw output (S, Cout, H, W), the fp32 levels and y_t."""
    comp, _ = loss_ref.compose(np.asarray(out, dtype=np.float64), view_count, weighting)
    a, b = (c.reshape(-1, 1, 1, 1) for c in coeffs(level, prediction))
    x = np.clip(a * np.asarray(y_t, dtype=np.float64) - b * comp, -1.0, 1.0)
    if keep is not None:
        x = x * np.asarray(keep, dtype=np.float64).reshape(-1, 1, 1, 1)
    return x


# ---- stacking -----------------------------------------------------------------------------------------------------------
def stack(y_cond, view_count, y_t, level, angle, drop=None, null_rows=False, sc=None):
    """guidance_ref.stack plus the third part: every row of sample b (its null row too) ends with sc[b] (None: zeros).
    -> x (S (+ B), Cc + 6, H, W), angle_s, level_s.  Exact: copies only."""
    vc = [int(v) for v in view_count]
    x, ang_s, lvl_s = guidance_ref.stack(y_cond, vc, y_t, level, angle, drop=drop, null_rows=null_rows)
    sc = torch.zeros_like(y_t) if sc is None else torch.as_tensor(sc, dtype=y_t.dtype)
    rows = torch.repeat_interleave(torch.arange(len(vc)), torch.tensor(vc))
    if null_rows:
        rows = torch.cat([rows, torch.arange(len(vc))])
    return torch.cat([x, sc[rows]], dim=1), ang_s, lvl_s


# ---- training: the two passes through a CPU UNet ---------------------------------------------------------------------------
def first_pass(unet_fn, y_cond, view_count, angle, y_0, noise, level, prediction, weighting=True, keep=None, drop=None):
    """-> (x^ float64 (B, 3, H, W), y_t float32): the network in fp32 on zero sc channels, everything after it in float64."""
    vc = [int(v) for v in view_count]
    lv = torch.as_tensor(level, dtype=torch.float32).reshape(-1, 1)
    from oracle import view_fusion_ref as vfr
    y_t = vfr.q_sample(y_0, lv.reshape(-1, 1, 1, 1), noise)
    x, ang_s, lvl_s = stack(y_cond, vc, y_t, lv, angle, drop=drop)
    with torch.no_grad():
        out = unet_fn(x, ang_s, lvl_s)
    return estimate(out.double().numpy(), vc, weighting, lv.reshape(-1).numpy(), prediction, y_t.double().numpy(), keep), y_t


def composed(out, view_count, weighting):
    """oracle.view_fusion_ref.compose's first output, differentiable (torch)."""
    from oracle import view_fusion_ref as vfr
    return vfr.compose(out, [int(v) for v in view_count], weighting)[0]


def second_pass_loss(unet_fn, y_cond, view_count, angle, y_0, noise, level, prediction, sc, weighting=True, weight=None,
                     drop=None):
    """The ordinary objective (MSE on the native target, per-sample weight `weight` (B,) | None) of the network shown sc
    (a torch tensor; hand one with autograd history to let a gradient flow through it) -> the scalar loss, torch, with
    autograd history through unet_fn.  The network and the loss run in fp32 torch, as the oracle's train_loss does."""
    from oracle import view_fusion_ref as vfr
    vc = [int(v) for v in view_count]
    B = len(vc)
    lv = torch.as_tensor(level, dtype=torch.float32).reshape(-1, 1)
    g = lv.reshape(-1, 1, 1, 1)
    y_t = vfr.q_sample(y_0, g, noise)
    rows = torch.repeat_interleave(torch.arange(B), torch.tensor(vc))
    x, ang_s, lvl_s = guidance_ref.stack(y_cond, vc, y_t, lv, angle, drop=drop)
    x = torch.cat([x, sc.to(x.dtype)[rows]], dim=1)
    out = composed(unet_fn(x, ang_s, lvl_s), vc, weighting)
    target = {"eps": noise, "v": g.sqrt() * noise - (1 - g).sqrt() * y_0, "x0": y_0}[prediction]
    per = ((out - target) ** 2).reshape(B, -1).mean(dim=1)
    w = torch.ones(B) if weight is None else torch.as_tensor(np.asarray(weight), dtype=torch.float32)
    return (w * per).mean()


def flowing_estimate(unet_fn, y_cond, view_count, angle, y_0, noise, level, prediction, weighting=True, keep=None, drop=None):
    """first_pass in fp32 torch WITH autograd history: what a gradient through pass 1 would differentiate (the
    discrimination check of the stopped gradient)."""
    from oracle import view_fusion_ref as vfr
    vc = [int(v) for v in view_count]
    lv = torch.as_tensor(level, dtype=torch.float32).reshape(-1, 1)
    y_t = vfr.q_sample(y_0, lv.reshape(-1, 1, 1, 1), noise)
    x, ang_s, lvl_s = stack(y_cond, vc, y_t, lv, angle, drop=drop)
    comp = composed(unet_fn(x, ang_s, lvl_s), vc, weighting)
    a, b = (torch.tensor(c, dtype=torch.float32).reshape(-1, 1, 1, 1) for c in coeffs(lv.reshape(-1).numpy(), prediction))
    xh = (a * y_t - b * comp).clamp(-1.0, 1.0)
    if keep is not None:
        xh = xh * torch.as_tensor(np.asarray(keep), dtype=torch.float32).reshape(-1, 1, 1, 1)
    return xh


# ---- sampling: the self-conditioned few-step chain ---------------------------------------------------------------------------
def chain(unet_fn, betas, prediction, y_cond, view_count, angle, y_T, z_seq, tau, solver="ddim", eta=0.0, g=None,
          weighting=True, q=None, force_zero=False):
    """The K-step chain over tau of a self-conditioned model through a CPU UNet: the network in fp32 at the fp32 level
    gammas32[tau[k]] on [ cond | y | sc ], sc = the bounded y0 of the step before (zeros at the first step; force_zero: at
    every step -- the chain with the wire cut), guided by its null rows when g (a scale, or one per sample) is given;
    the update in float64 (prediction_ref.sampler_step).  z_seq (T, ...) indexed by the model timestep, None = no noise.
    -> (states after every step, float32 (K, B, 3, H, W); the y0 of every step, float64)."""
    from oracle import view_fusion_ref as vfr
    gammas32 = vfr.schedule_buffers(betas)["gammas"]
    vc = [int(v) for v in view_count]
    B, S = len(vc), sum(vc)
    y = y_T.double().numpy()
    y0_prev = np.full_like(y, np.nan)
    sc = np.zeros_like(y)
    states, y0s = [], []
    for k in reversed(range(len(tau))):
        level = gammas32[int(tau[k])].reshape(1, 1).repeat(B, 1)
        x, ang_s, lvl_s = stack(y_cond, vc, torch.tensor(y).float(), level, angle, null_rows=g is not None,
                                sc=torch.tensor(sc).float())
        with torch.no_grad():
            out = unet_fn(x[:S], ang_s[:S], lvl_s[:S])
            comp, _ = loss_ref.compose(out.double().numpy(), vc, weighting)
            if g is not None:
                null = unet_fn(x[S:], ang_s[S:], lvl_s[S:])[:, :3].double().numpy()
                gs = np.broadcast_to(np.asarray(g, dtype=np.float32).astype(np.float64).reshape(-1), (B,)).reshape(B, 1, 1, 1)
                comp = gs * comp + (1.0 - gs) * null
        z = 0.0 if z_seq is None else z_seq[int(tau[k])].double().numpy()
        y, y0, _ = prediction_ref.sampler_step(betas, tau, solver, eta, prediction, k, y, comp, y0_prev, z, q=q)
        y = np.asarray(y, dtype=np.float64)
        y0_prev = y0
        sc = np.zeros_like(y) if force_zero else y0
        states.append(torch.tensor(y).float())
        y0s.append(y0)
    return torch.stack(states), y0s
