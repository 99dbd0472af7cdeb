// The training objective's per-element penalty and per-sample noise-level weight, shared by the loss kernels of
// diffusion.hip and by the host mirror vf_loss_weights_host (the very same functions on the CPU, as with rng.h).
// This comment is the ONE written specification; tests/loss_ref.py restates it in float64 numpy.
//
//   d = noise_hat - target, n = 3 H W elements per sample
//   penalty   rho(d)                                               rho'(d)
//   mse       d^2                                                  2 d
//   l1        |d|                                                  sign(d), 0 at 0 (as torch)
//   huber     0.5 d^2 if |d| <= delta, else delta (|d| - 0.5 delta)    d clamped to [-delta, delta]   (F.huber_loss)
//
//   per-sample loss  s_b = (1 / n) sum_i rho(d_bi);   loss = (1 / B) sum_b w_b s_b   (no renormalisation by sum w)
//
//   weight w_b of the sample's level g = gamma_b (the cumulative signal level the model is conditioned on; for
//   epsilon-prediction SNR = g / (1 - g)), in fp32, in exactly these forms:
//     none            1
//     min_snr(a)      fminf(1, a (1 - g) / g)      = min(SNR, a) / SNR  (Hang et al., Min-SNR-gamma), written so that
//                                                    g -> 1 needs no division by 1 - g;  g = 0 gives 1
//     p2(a = k, b = p)  powf(k + g / (1 - g), -p)  = (k + SNR)^-p       (Choi et al., P2 weighting);  g = 1 gives 0
//     trunc_snr       fmaxf(1, (1 - g) / g)        = max(SNR, 1) / SNR  (Salimans & Ho, Progressive Distillation: the
//                                                    truncated-SNR weight max(SNR, 1) on the x-space error, which keeps a
//                                                    signal at low SNR for a distilled student);  g = 0 gives inf
//   fminf / fmaxf / powf are the accurate library functions: the host and the device libraries agree to their last-place
//   errors.
//
// Prediction (what the network's first three channels mean; the head of diffusion.hip holds the table of targets and of
// y0_hat).  rho, s_b and the loss above are then taken on the NATIVE residual d = out - target(prediction).  "min_snr" and
// "p2" stay weights on the epsilon-equivalent squared error: with eps_hat - eps = sqrt(g) (v_hat - v)
// = -sqrt(g / (1 - g)) (x0_hat - x0) the native weight is w_eps(g) c(g), c = 1 (eps), g (v), g / (1 - g) (x0) -- Hang et
// al.'s three forms.  kind none is w = 1 on the native loss for every prediction.  In fp32, in exactly these forms:
//     v  / min_snr(a)      fminf(g, a (1 - g))                       x0 / min_snr(a)      fminf(g / (1 - g), a)
//     v  / p2(a, b)        powf(a + g / (1 - g), -b) * g             x0 / p2(a, b)        powf(a + g / (1 - g), -b) * (g / (1 - g))
//     v  / trunc_snr       fmaxf(g, 1 - g)                           x0 / trunc_snr       fmaxf(g / (1 - g), 1)
//   eps: vf_loss_weight above, untouched.  x0 at g = 1: min_snr gives a, p2 gives 0 * inf = NaN for b > 0 (g = 1 is not a
//   level a training draw produces: levels lie between gammas[T-1] and gammas[0] < 1).
#pragma once
#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define VF_LOSS_HD __host__ __device__ inline
#else
#define VF_LOSS_HD inline
#endif

enum { VF_LOSS_MSE = 0, VF_LOSS_L1 = 1, VF_LOSS_HUBER = 2 };
enum { VF_LOSS_W_NONE = 0, VF_LOSS_W_MIN_SNR = 1, VF_LOSS_W_P2 = 2, VF_LOSS_W_TRUNC_SNR = 3, VF_LOSS_W_LAST = 3 };
enum { VF_PRED_EPS = 0, VF_PRED_V = 1, VF_PRED_X0 = 2 };

VF_LOSS_HD float vf_loss_weight(int kind, float a, float b, float g) {
    if (kind == VF_LOSS_W_MIN_SNR) return fminf(1.0f, a * (1.0f - g) / g);
    if (kind == VF_LOSS_W_P2) return powf(a + g / (1.0f - g), -b);
    if (kind == VF_LOSS_W_TRUNC_SNR) return fmaxf(1.0f, (1.0f - g) / g);
    return 1.0f;
}

// The native weight of a prediction: vf_loss_weight for eps; for v / x0 the forms of the head comment.
VF_LOSS_HD float vf_loss_weight_pred(int pred, int kind, float a, float b, float g) {
    if (pred == VF_PRED_EPS) return vf_loss_weight(kind, a, b, g);
    if (kind == VF_LOSS_W_MIN_SNR) return pred == VF_PRED_V ? fminf(g, a * (1.0f - g)) : fminf(g / (1.0f - g), a);
    if (kind == VF_LOSS_W_P2) return powf(a + g / (1.0f - g), -b) * (pred == VF_PRED_V ? g : g / (1.0f - g));
    if (kind == VF_LOSS_W_TRUNC_SNR) return pred == VF_PRED_V ? fmaxf(g, 1.0f - g) : fmaxf(g / (1.0f - g), 1.0f);
    return 1.0f;
}

template <int PEN>
VF_LOSS_HD float vf_loss_rho(float d, float delta) {
    if (PEN == VF_LOSS_L1) return fabsf(d);
    if (PEN == VF_LOSS_HUBER) {
        const float ad = fabsf(d);
        return ad <= delta ? 0.5f * d * d : delta * (ad - 0.5f * delta);
    }
    return d * d;
}

template <int PEN>
VF_LOSS_HD float vf_loss_drho(float d, float delta) {
    if (PEN == VF_LOSS_L1) return d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f);
    if (PEN == VF_LOSS_HUBER) return fminf(fmaxf(d, -delta), delta);
    return 2.0f * d;
}
