"""Test infrastructure: the learned-variance definition at the head of view_fusion_amd/csrc/diffusion.hip (arithmetic:
csrc/vlb.h) restated, on top of loss_ref (penalties, eps weights), prediction_ref (targets, native weights, y0_hat) and
sampler_ref (the few-step update).  Nothing here calls the library.

    out (S, 9, H, W): channels 0..2 the prediction, 3..5 the view logits, 6..8 the raw variance output o
    o_b   = the composition of channels 6..8 under the weights of channels 0..2 (softmax of 3..5, or the mean)
    lp    = v hi + (1 - v) lo,  v = 0.5 o_b + 0.5
    hi[k] = log(1 - gt/gp),  lo[k] = log(max((1 - gt/gp)(1 - gp)/(1 - gt), 1e-20)),  gt = gammas[tau[k]], gp = gammas[tau[k-1]]
    m^2   = c1[t]^2 kappa^2(g) r^2,  kappa^2 = (1 - g)/g (eps) | 1 - g (v) | 1 (x0),  r = composed prediction - target, a constant
    KL    = 0.5 (-1 + lp - lo[t] + exp(lo[t] - lp) + m^2 exp(-lp)) / ln 2,  vlb_b = mean over the sample's elements
    loss  = L_simple + lambda mean_b vlb_b
    step  : y0 = clamp(a[k] y - b[k] out, -1, 1);  r = cy[k] y + c0[k] y0 (ddim, eta = 1);  r += exp(0.5 lp) z for k > 0

Two evaluations of the one restatement: `hybrid` in numpy at a chosen dtype with the gradient in closed form -- float64 is
the yardstick, float32 (the same operations on the same fp32 inputs) measures the restatement's own distance from it --
and `hybrid_torch`, the same forward in torch float64 whose gradient comes from autograd with r detached (detach=False lets
the mean flow: what the stop-gradient must NOT compute).  Every function reads the fp32 inputs and fp32 table values it is
handed, exactly."""
import numpy as np
import torch

import loss_ref
import prediction_ref
import sampler_ref

LN2 = float(np.log(2.0))


def compose9(out, view_count, weighting, dtype=np.float64):
    """out (S, 9, H, W) -> (prediction (B, 3, H, W), o_b (B, 3, H, W), the per-view weights [(V_b, 3, H, W)] | None).
    The logits are channels 3:6 -- sliced here, not `3:`."""
    out = np.asarray(out).astype(dtype)
    off = loss_ref.offsets(view_count)
    nh, ob, ws = [], [], []
    for b in range(len(off) - 1):
        rows = out[off[b]:off[b + 1]]
        if not weighting:
            nh.append(rows[:, 0:3].mean(axis=0, dtype=dtype))
            ob.append(rows[:, 6:9].mean(axis=0, dtype=dtype))
            continue
        lg = rows[:, 3:6]
        w = np.exp(lg - lg.max(axis=0, keepdims=True))
        w = w / w.sum(axis=0, keepdims=True)
        ws.append(w)
        nh.append((w * rows[:, 0:3]).sum(axis=0))
        ob.append((w * rows[:, 6:9]).sum(axis=0))
    return np.stack(nh), np.stack(ob), (ws if weighting else None)


def tables(betas, tau=None):
    """(hi, lo) float64 (K,) by the direct formula."""
    g = np.cumprod(1.0 - np.asarray(betas, dtype=np.float64))
    tau = np.arange(len(g)) if tau is None else np.asarray(tau, dtype=np.int64)
    gt = g[tau]
    gp = np.concatenate([[1.0], gt[:-1]])
    beta = 1.0 - gt / gp
    with np.errstate(divide="ignore"):
        return np.log(beta), np.log(np.maximum(beta * (1.0 - gp) / (1.0 - gt), 1e-20))


def kappa2(prediction, level, dtype=np.float64):
    g = np.asarray(level, dtype=np.float32).astype(dtype)
    one = dtype(1.0)
    return {"eps": (one - g) / g, "v": one - g, "x0": np.ones_like(g)}[prediction]


def logvar(ob, hi, lo):
    """lp of o_b between lo and hi (arrays or scalars of one dtype)."""
    half = ob.dtype.type(0.5)
    v = half * ob + half
    return v * hi + (ob.dtype.type(1.0) - v) * lo


def kl_bits(lp, lo, m2):
    one, half = lp.dtype.type(1.0), lp.dtype.type(0.5)
    return half * (-one + lp - lo + np.exp(lo - lp) + m2 * np.exp(-lp)) / lp.dtype.type(LN2)


def dkl_bits(lp, lo, m2):
    one, half = lp.dtype.type(1.0), lp.dtype.type(0.5)
    return half * (one - np.exp(lo - lp) - m2 * np.exp(-lp)) / lp.dtype.type(LN2)


def _per_sample(v, dtype):
    return np.asarray(v, dtype=np.float32).astype(dtype).reshape(-1, 1, 1, 1)


def hybrid(out, noise, y_0, view_count, weighting, level, t, c1, hi, lo, lam, prediction="eps", penalty="mse", delta=1.0,
           weight_kind=None, a=0.0, b=0.0, gloss=1.0, dtype=np.float64):
    """The hybrid loss of fp32 inputs and fp32 tables (c1, hi, lo over all T; t (B,) integers) evaluated in `dtype`.
    -> dict(loss, sample_loss (B,), sample_vlb (B,), dout (S, 9, H, W) = d (gloss loss) / d out, d (B, 3, H, W), lp)."""
    out = np.asarray(out).astype(dtype)
    off = loss_ref.offsets(view_count)
    B = len(off) - 1
    nh, ob, ws = compose9(out, view_count, weighting, dtype)
    g = _per_sample(level, dtype)
    nz = None if noise is None else np.asarray(noise).astype(dtype)
    y0 = None if y_0 is None else np.asarray(y_0).astype(dtype)
    if prediction == "eps":
        tg = nz
    elif prediction == "v":
        tg = np.sqrt(g) * nz - np.sqrt(dtype(1.0) - g) * y0
    else:
        tg = y0
    d = nh - tg
    n = d[0].size
    s = loss_ref.rho(d, penalty, dtype(delta)).reshape(B, -1).sum(axis=1, dtype=dtype) / dtype(n)
    w = prediction_ref.weights(level, prediction, weight_kind, a, b, dtype=dtype)
    t = np.asarray(t, dtype=np.int64)
    c1_t, hi_t, lo_t = (_per_sample(np.asarray(x, dtype=np.float32)[t], dtype) for x in (c1, hi, lo))
    m2 = c1_t * c1_t * kappa2(prediction, level, dtype).reshape(-1, 1, 1, 1) * d * d
    lp = logvar(ob, hi_t, lo_t)
    vlb = kl_bits(lp, lo_t, m2).reshape(B, -1).sum(axis=1, dtype=dtype) / dtype(n)
    lam, gloss = dtype(lam), dtype(gloss)
    simple = dtype(0.0)
    total_v = dtype(0.0)
    for i in range(B):
        simple += w[i] * s[i]
        total_v += vlb[i]
    loss = simple / dtype(B) + lam * (total_v / dtype(B))
    gs = gloss * w.reshape(B, 1, 1, 1) * loss_ref.drho(d, penalty, dtype(delta)) / dtype(n * B)
    gv = gloss * lam / dtype(n * B) * dkl_bits(lp, lo_t, m2) * (dtype(0.5) * (hi_t - lo_t))
    dout = np.zeros_like(out)
    for i in range(B):
        v0, v1 = off[i], off[i + 1]
        if not weighting:
            dout[v0:v1, 0:3] = gs[i] / dtype(v1 - v0)
            dout[v0:v1, 6:9] = gv[i] / dtype(v1 - v0)
            continue
        rows = out[v0:v1]
        dout[v0:v1, 0:3] = ws[i] * gs[i]
        dout[v0:v1, 3:6] = ws[i] * (rows[:, 0:3] - nh[i]) * gs[i] + ws[i] * (rows[:, 6:9] - ob[i]) * gv[i]
        dout[v0:v1, 6:9] = ws[i] * gv[i]
    assert dout.dtype == dtype and lp.dtype == dtype
    return dict(loss=loss, sample_loss=s, sample_vlb=vlb, dout=dout, d=d, lp=lp, simple=simple / dtype(B))


def compose9_torch(out, view_count, weighting):
    off = loss_ref.offsets(view_count)
    nh, ob = [], []
    for b in range(len(off) - 1):
        rows = out[int(off[b]):int(off[b + 1])]
        if not weighting:
            nh.append(rows[:, 0:3].mean(dim=0))
            ob.append(rows[:, 6:9].mean(dim=0))
            continue
        w = torch.softmax(rows[:, 3:6], dim=0)
        nh.append((w * rows[:, 0:3]).sum(dim=0))
        ob.append((w * rows[:, 6:9]).sum(dim=0))
    return torch.stack(nh), torch.stack(ob)


def hybrid_torch(out, noise, y_0, view_count, weighting, level, t, c1, hi, lo, lam, prediction="eps", penalty="mse",
                 delta=1.0, weight_kind=None, a=0.0, b=0.0, detach=True):
    """The same forward in torch float64 on a float64 `out` that may require grad -> (loss, sample_loss, sample_vlb).
    detach=True: r is a constant inside the vlb term (the definition); False lets the vlb gradient reach channels 0..2."""
    f64 = lambda x: torch.as_tensor(np.asarray(x, dtype=np.float32)).double()      # noqa: E731
    B = len(view_count)
    nh, ob = compose9_torch(out, view_count, weighting)
    g = f64(level).reshape(-1, 1, 1, 1)
    if prediction == "eps":
        tg = f64(noise)
    elif prediction == "v":
        tg = g.sqrt() * f64(noise) - (1.0 - g).sqrt() * f64(y_0)
    else:
        tg = f64(y_0)
    d = nh - tg
    if penalty == "mse":
        rho = d * d
    elif penalty == "l1":
        rho = d.abs()
    else:
        rho = torch.where(d.abs() <= delta, 0.5 * d * d, delta * (d.abs() - 0.5 * delta))
    s = rho.reshape(B, -1).mean(dim=1)
    w = torch.as_tensor(prediction_ref.weights(level, prediction, weight_kind, a, b))
    t = torch.as_tensor(np.asarray(t, dtype=np.int64))
    c1_t, hi_t, lo_t = (f64(x)[t].reshape(-1, 1, 1, 1) for x in (c1, hi, lo))
    k2 = torch.as_tensor(kappa2(prediction, level)).reshape(-1, 1, 1, 1)
    r = d.detach() if detach else d
    m2 = c1_t * c1_t * k2 * r * r
    v = 0.5 * ob + 0.5
    lp = v * hi_t + (1.0 - v) * lo_t
    kl = 0.5 * (-1.0 + lp - lo_t + torch.exp(lo_t - lp) + m2 * torch.exp(-lp)) / LN2
    vlb = kl.reshape(B, -1).mean(dim=1)
    return (w * s).sum() / B + lam * vlb.sum() / B, s, vlb


def sampler_step(betas, tau, prediction, k, y, out, ob, z, hi, lo):
    """One learned-variance step from the composed (guided) prediction `out` and the composed o_b, float64: the ddim,
    eta = 1 update without its noise, then exp(0.5 lp) z where k > 0.  hi, lo: the fp32 table values over the chain.
    -> (y_new, y0, lp)."""
    y = np.asarray(y, dtype=np.float64)
    y0 = np.clip(prediction_ref.y0_hat(betas, prediction, int(tau[k]), y, out), -1.0, 1.0)
    mean = sampler_ref.update(betas, tau, "ddim", 1.0, k, y, y0, None, 0.0)
    lp = logvar(np.asarray(ob, dtype=np.float64), np.float64(np.float32(hi[k])), np.float64(np.float32(lo[k])))
    if k == 0:
        return mean, y0, lp
    return mean + np.exp(0.5 * lp) * np.asarray(z, dtype=np.float64), y0, lp


def chain(unet_fn, betas, gammas32, prediction, y_cond, view_count, angle, y_T, z_seq, tau, hi, lo, weighting=True):
    """The learned-variance chain through a CPU UNet with nine output channels: the network in fp32 at the fp32 level
    gammas32[tau[k]], everything after it in float64; z_seq (T, ...) is indexed by the model timestep.
    -> the states after step K-1 ... 0, float32 (K, B, 3, H, W)."""
    from oracle import view_fusion_ref as vfr
    B = y_cond.shape[0]
    y = y_T.double().numpy()
    states = []
    for k in reversed(range(len(tau))):
        t = int(tau[k])
        level = gammas32[t].reshape(1, 1).repeat(B, 1)
        x, ang_s, lvl_s = vfr.stack_views(y_cond, view_count, torch.tensor(y).float(), level, angle)
        nh, ob, _ = compose9(unet_fn(x, ang_s, lvl_s).double().numpy(), view_count, weighting)
        y, _, _ = sampler_step(betas, tau, prediction, k, y, nh, ob, z_seq[t].double().numpy(), hi, lo)
        states.append(torch.tensor(y).float())
    return torch.stack(states)
