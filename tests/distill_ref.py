"""Test infrastructure: a float64 numpy restatement of progressive distillation (the head comment of
view_fusion_amd/csrc/diffusion.hip holds the definition; Salimans & Ho, "Progressive Distillation for Fast Sampling of
Diffusion Models"), stated in (alpha, sigma) form from the cumulative gammas -- not from the folded tables of
view_fusion_amd/schedule.py, which the product never shares with this file and which never imports it.

With gamma the cumulative product of 1 - beta, alpha = sqrt(gamma), sigma = sqrt(1 - gamma).  A deterministic DDIM step from
level t to level p (the clean image, alpha_p = 1, sigma_p = 0, at step 0) is

    z_p = (sigma_p / sigma_t) z_t + (alpha_p - alpha_t sigma_p / sigma_t) x,       x = clip(a_t z_t - b_t out, -1, 1)

The student grid is tau_S = timesteps(T, K), the teacher grid tau_T = timesteps(T, 2K), tau_T[2i+1] == tau_S[i].  For the
student step i: z_t at level tau_S[i]; the teacher's step 2i+1 gives x1 and z', its step 2i gives x2 (and z''); the target is

    x~ = w1 x1 + w2 x2,  w1 = cy_T[2i] c0_T[2i+1] / c0_S[i],  w2 = 1 - w1,          eps~ = (z_t - alpha x~) / sigma

(alpha, sigma of the fp32 level the student is conditioned on), and cy_S z_t + c0_S x~ == z''.  The truncated-SNR loss weight
max(SNR, 1) / SNR and its native forms for v / x0 are restated here too.  No GPU.
"""
import numpy as np

import prediction_ref
import rng_ref
from loss_ref import compose  # noqa: F401  (the composition over the views, shared with the loss restatement)


def timesteps(T, K):
    return np.array([((k + 1) * T) // K - 1 for k in range(K)], dtype=np.int64)


def ddim_coefficients(betas, tau):
    """(cy, c0) float64 (K,) of the deterministic DDIM chain over tau: z_p = cy z_t + c0 x."""
    g = prediction_ref.gammas(betas)
    gt = g[np.asarray(tau)]
    gp = np.append(1.0, gt[:-1])
    al_t, sg_t, al_p, sg_p = np.sqrt(gt), np.sqrt(1.0 - gt), np.sqrt(gp), np.sqrt(1.0 - gp)
    cy = sg_p / sg_t
    return cy, al_p - al_t * cy


def grids(betas, K):
    """-> dict(tau_s, tau_t, w1, w2, cy_t, c0_t, cy_s, c0_s), float64."""
    T = len(betas)
    if K < 1 or 2 * K > T:
        raise ValueError(K)
    tau_s, tau_t = timesteps(T, K), timesteps(T, 2 * K)
    cy_t, c0_t = ddim_coefficients(betas, tau_t)
    cy_s, c0_s = ddim_coefficients(betas, tau_s)
    w1 = cy_t[0::2] * c0_t[1::2] / c0_s
    return dict(tau_s=tau_s, tau_t=tau_t, w1=w1, w2=1.0 - w1, cy_t=cy_t, c0_t=c0_t, cy_s=cy_s, c0_s=c0_s)


def draw_step(seed, ids, K):
    """i (B,) int64 = mulhi32(word 0 of the sample's kind-0 call, K): exact."""
    w0 = rng_ref.words(seed, ids, rng_ref.KIND_SCALARS, 0, 1)[:, 0, 0]
    return ((w0 * np.uint64(K)) >> np.uint64(32)).astype(np.int64)


def _col(v, ndim=4):
    return np.asarray(v, dtype=np.float64).reshape((-1,) + (1,) * (ndim - 1))


def begin(gammas32, tau_s, i, y_0, noise):
    """-> (level (B,) float32: the buffer's own values, z_t float64 of the fp32 inputs taken exactly)."""
    level = np.asarray(gammas32, dtype=np.float32)[np.asarray(tau_s)[np.asarray(i)]]
    g = _col(level)
    return level, np.sqrt(g) * np.asarray(y_0, dtype=np.float64) + np.sqrt(1.0 - g) * np.asarray(noise, dtype=np.float64)


def guided(out_c, out_u, g):
    """g out_c + (1 - g) out_u per sample, 1 - g formed first; g None: out_c."""
    if g is None:
        return np.asarray(out_c, dtype=np.float64)
    g = _col(np.asarray(g, dtype=np.float32))
    return g * np.asarray(out_c, dtype=np.float64) + (1.0 - g) * np.asarray(out_u, dtype=np.float64)


def x_hat(betas, prediction, t, y, out):
    """clip(a[t] y - b[t] out, -1, 1) with per-sample model timesteps t (B,)."""
    a, b = prediction_ref.tables(betas, prediction)
    return np.clip(_col(a[t]) * np.asarray(y, dtype=np.float64) - _col(b[t]) * np.asarray(out, dtype=np.float64), -1.0, 1.0)


def second_step(betas, K, prediction, i, level, z_prime, x1, z_t, out2):
    """Steps 3 - 5 from the composed (and guided) teacher output out2 at z': -> (x2, x~, eps~), float64."""
    gr = grids(betas, K)
    i = np.asarray(i)
    x2 = x_hat(betas, prediction, gr["tau_t"][2 * i], z_prime, out2)
    xt = np.clip(_col(gr["w1"][i]) * np.asarray(x1, dtype=np.float64) + _col(gr["w2"][i]) * x2, -1.0, 1.0)
    g = _col(np.asarray(level, dtype=np.float32))
    return x2, xt, (np.asarray(z_t, dtype=np.float64) - np.sqrt(g) * xt) / np.sqrt(1.0 - g)


def two_steps(betas, gammas32, K, prediction, i, y_0, noise, teacher):
    """The whole definition.  teacher(y float64 (B, 3, H, W), level float32 (B,)) -> the composed (and guided) output,
    float64.  -> dict(level, z_t, x1, z_prime, x2, z_pp, x_tilde, eps_tilde)."""
    gr = grids(betas, K)
    i = np.asarray(i)
    g32 = np.asarray(gammas32, dtype=np.float32)
    level, z_t = begin(g32, gr["tau_s"], i, y_0, noise)
    k1, k0 = 2 * i + 1, 2 * i
    x1 = x_hat(betas, prediction, gr["tau_t"][k1], z_t, teacher(z_t, g32[gr["tau_t"][k1]]))
    z_prime = _col(gr["cy_t"][k1]) * z_t + _col(gr["c0_t"][k1]) * x1
    x2, xt, et = second_step(betas, K, prediction, i, level, z_prime, x1, z_t, teacher(z_prime, g32[gr["tau_t"][k0]]))
    z_pp = _col(gr["cy_t"][k0]) * z_prime + _col(gr["c0_t"][k0]) * x2
    return dict(level=level, z_t=z_t, x1=x1, z_prime=z_prime, x2=x2, z_pp=z_pp, x_tilde=xt, eps_tilde=et)


def trunc_snr(level, prediction, dtype=np.float64):
    """max(SNR, 1) / SNR in its native form.  float64: the definition, w_eps c(g).  float32: the header's own forms in its
    operation order (the distance between the two bounds the library's error, as loss_ref.weights)."""
    g = np.asarray(level, dtype=np.float32).astype(dtype)
    one = dtype(1.0)
    with np.errstate(divide="ignore"):
        if dtype == np.float64:
            return np.maximum(one, (one - g) / g) * prediction_ref.c(level, prediction)
        w = {"eps": lambda: np.maximum(one, (one - g) / g), "v": lambda: np.maximum(g, one - g),
             "x0": lambda: np.maximum(g / (one - g), one)}[prediction]()
    assert w.dtype == dtype
    return w
