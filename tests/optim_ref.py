"""Restatements of the fused optimizer step with its opt-in extras (optim.FusedAdam(ema_decay=, ema_warmup=,
max_grad_norm=)): global-norm clip coefficient -> Adam -> weight EMA, in numpy.

  run_f64   everything in double, in torch's formulas (torch.nn.utils.clip_grad_norm_, torch.optim.Adam's single-tensor
            path); tests/test_optim_ref_host.py checks it against torch itself on the CPU.  The GPU tests compare with it.
  run_f32   float32 in the kernels' operation order (csrc/adam.hip, csrc/adam_update.h): the per-block sums of squares
            and their total in double, norm and scale rounded to float; g * scale; m = fma(b1, m, (1-b1) g);
            v = fma(g, (1-b2) g, b2 v); p -= (step m) / fma(sqrt(v), rs, eps); ema = fma(d, ema, (1-d) p).
            Its deviation e from run_f64 on the same inputs sets the GPU tests' tolerance max(4 e, 1e-6) (`bound`).

Both take params: list of float32 arrays, grads: list (one entry per step) of lists of float32 arrays, and return
dict(p=, m=, v=, ema= (lists of arrays, ema None without ema_decay), norm= (per step), scale= (per step),
p_hist= (per step: the parameters after it), decay= (per step)).
"""
import numpy as np

BLOCK = 1024


def ema_decay_at(t, ema_decay, warmup):
    """Decay of EMA update number t (0 for the first), in double."""
    return min(ema_decay, (1.0 + t) / (10.0 + t)) if warmup else float(ema_decay)


def bound(e):
    """The project's measured-floor rule (tests/ssim_ref.py, tests/rng_ref.py): 4 x the fp32 restatement's own error."""
    return max(4.0 * e, 1e-6)


def rel_err(x, ref):
    """max |x - ref| relative to the largest magnitude of ref: Adam's moments pass through zero, where an element's own
    relative error says nothing about the arithmetic."""
    x, ref = np.asarray(x, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    if ref.size == 0:
        return 0.0
    err, scale = float(np.max(np.abs(x - ref))), float(np.max(np.abs(ref)))
    return err / scale if scale > 0.0 else err


def float_betas(betas=(0.9, 0.999)):
    """The betas as the kernels receive them: rounded to float32 (returned as Python floats)."""
    return tuple(float(np.float32(b)) for b in betas)


def run_f64(params, grads, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, max_norm=None, ema_decay=None, ema_warmup=False,
            ema_t0=0, moment_betas=None):
    """moment_betas (default: betas): the b1, b2 of the two moment recurrences.  The kernels take them as float32, and
    1 - float32(0.999) is 1.3e-5 off 0.001; with moment_betas=float_betas(betas) the restatement uses the same values, so
    that run_f32's deviation from it is rounding alone.  The bias corrections 1 - b^t come from the host's double
    `betas` either way, as in optim.FusedAdam."""
    b1, b2 = betas
    mb1, mb2 = betas if moment_betas is None else moment_betas
    p = [np.asarray(a, dtype=np.float64).copy() for a in params]
    m = [np.zeros_like(a) for a in p]
    v = [np.zeros_like(a) for a in p]
    ema = None if ema_decay is None else [a.copy() for a in p]
    out = dict(norm=[], scale=[], p_hist=[], decay=[])
    for t, gs in enumerate(grads, 1):
        gs = [np.asarray(g, dtype=np.float64) for g in gs]
        norm = float(np.sqrt(sum(float(np.sum(g * g)) for g in gs)))
        scale = 1.0 if max_norm is None else min(1.0, max_norm / (norm + 1e-6))
        out["norm"].append(norm)
        out["scale"].append(scale)
        bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
        d = None if ema_decay is None else ema_decay_at(ema_t0 + t - 1, ema_decay, ema_warmup)
        out["decay"].append(d)
        for i, g in enumerate(gs):
            g = g * scale
            m[i] = mb1 * m[i] + (1.0 - mb1) * g
            v[i] = mb2 * v[i] + (1.0 - mb2) * g * g
            p[i] = p[i] - (lr / bc1) * m[i] / (np.sqrt(v[i]) / np.sqrt(bc2) + eps)
            if ema is not None:
                ema[i] = d * ema[i] + (1.0 - d) * p[i]
        out["p_hist"].append([a.copy() for a in p])
    out.update(p=p, m=m, v=v, ema=ema)
    return out


def _fma(a, b, c):
    """float32 fused multiply-add: the product of two floats is exact in double; one rounding of the sum to double and
    one to float (they coincide with the single rounding except in rare double-rounding ties)."""
    return (np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64) + np.asarray(c, dtype=np.float64)).astype(np.float32)


def sumsq_blocks(g):
    """One tensor's gradient -> its per-1024-element sums of squares, in double (the first launch of the norm pass)."""
    g = np.asarray(g, dtype=np.float64).reshape(-1)
    pad = (-g.size) % BLOCK
    return np.sum(np.pad(g * g, (0, pad)).reshape(-1, BLOCK), axis=1)


def norm_scale_f32(gs, max_norm):
    """(norm, scale) as float32 the way the finish launch rounds them."""
    total = float(np.sum(np.concatenate([sumsq_blocks(g) for g in gs])))
    norm = np.float32(np.sqrt(total))
    if max_norm is None:
        return norm, np.float32(1.0)
    return norm, np.minimum(np.float32(1.0), np.float32(max_norm) / (norm + np.float32(1e-6)))


def run_f32(params, grads, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, max_norm=None, ema_decay=None, ema_warmup=False,
            ema_t0=0):
    f = np.float32
    b1, b2 = f(betas[0]), f(betas[1])
    omb1, omb2 = f(1.0) - b1, f(1.0) - b2
    p = [np.asarray(a, dtype=f).copy() for a in params]
    m = [np.zeros_like(a) for a in p]
    v = [np.zeros_like(a) for a in p]
    ema = None if ema_decay is None else [a.copy() for a in p]
    out = dict(norm=[], scale=[], p_hist=[], decay=[])
    for t, gs in enumerate(grads, 1):
        gs = [np.asarray(g, dtype=f) for g in gs]
        norm, scale = norm_scale_f32(gs, max_norm)
        out["norm"].append(float(norm))
        out["scale"].append(float(scale))
        bc1, bc2 = f(1.0 - betas[0] ** t), f(1.0 - betas[1] ** t)      # computed in double on the host, passed as float
        step, rs = f(lr) / bc1, f(1.0) / np.sqrt(bc2)
        d = None if ema_decay is None else ema_decay_at(ema_t0 + t - 1, ema_decay, ema_warmup)
        out["decay"].append(d)
        for i, g in enumerate(gs):
            if max_norm is not None:
                g = g * scale
            m[i] = _fma(b1, m[i], omb1 * g)
            v[i] = _fma(g, omb2 * g, b2 * v[i])
            den = _fma(np.sqrt(v[i]), rs, f(eps))
            p[i] = p[i] - (step * m[i]) / den
            if ema is not None:
                ema[i] = _fma(f(d), ema[i], f(1.0 - d) * p[i])
        out["p_hist"].append([a.copy() for a in p])
    out.update(p=p, m=m, v=v, ema=ema)
    return out
