// The arithmetic of a learned reverse-process variance (Nichol & Dhariwal, "Improved DDPM", 3.1 and 4), shared by the
// kernels of diffusion.hip and by the host mirror vf_vlb_terms_host (the very same functions on the CPU, as with
// loss_weight.h).  The head of diffusion.hip holds the definition; tests/vlb_ref.py restates it in float64.
//
//   o    the composed raw variance output of one element (channels 6..8 under the weights of channels 0..2)
//   v    = 0.5 o + 0.5                                  (product rounded, then the sum: no fused multiply-add)
//   lp   = v hi + (1 - v) lo                            (1 - v, both products and the sum rounded, in this order)
//   sd   = expf(0.5f lp)                                (the noise scale of a reverse step)
//   kappa^2(g) = (1 - g) / g (eps) | 1 - g (v) | 1 (x0) (what turns the native residual r into y0_hat's error)
//   m2   = (c1 c1) (kappa^2 (r r))                      (every product rounded, in this order)
//   KL   = 0.5 (((-1 + (lp - lo)) + expf(lo - lp)) + m2 expf(-lp)) / ln 2      in bits
//   dKL / dlp = 0.5 ((1 - expf(lo - lp)) - m2 expf(-lp)) / ln 2
//   dlp / do  = 0.5 (hi - lo)
// The decoder term of the variational bound (the head of diffusion.hip, "Variational bound"; tests/nll_ref.py restates it):
//   Phi(x) = 0.5 (1 + tanhf(sqrt(2/pi) (x + 0.044715 ((x x) x))))           (Improved DDPM's approx_standard_normal_cdf)
//   is   = expf(-0.5 lp);  d = x - mean;  plus = is (d + 1/255);  minus = is (d - 1/255)
//   ll   = logf(max(Phi(plus), 1e-12))                  where x < -0.999
//          logf(max(1 - Phi(minus), 1e-12))             where x >  0.999
//          logf(max(Phi(plus) - Phi(minus), 1e-12))     otherwise
//   nll  = -ll / ln 2                                                          in bits
// Contraction is off inside every function here, so host and device round the same operations; expf, logf and tanhf are
// the accurate library functions on both sides (they agree to their last-place errors).
#pragma once
#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define VF_VLB_HD __host__ __device__ inline
#else
#define VF_VLB_HD inline
#endif

#define VF_VLB_INV_LN2 1.44269504088896340736f

// pred: 0 eps | 1 v | 2 x0 (VF_PRED_* of loss_weight.h)
VF_VLB_HD float vf_vlb_kappa2(int pred, float g) {
#pragma clang fp contract(off)
    if (pred == 0) return (1.0f - g) / g;
    if (pred == 1) return 1.0f - g;
    return 1.0f;
}

VF_VLB_HD float vf_vlb_logvar(float o, float hi, float lo) {
#pragma clang fp contract(off)
    const float h = 0.5f * o;
    const float v = h + 0.5f;
    const float u = 1.0f - v;
    const float a = v * hi;
    const float b = u * lo;
    return a + b;
}

VF_VLB_HD float vf_vlb_m2(float c1, float kappa2, float r) {
#pragma clang fp contract(off)
    const float cc = c1 * c1;
    const float rr = r * r;
    const float kr = kappa2 * rr;
    return cc * kr;
}

VF_VLB_HD float vf_vlb_kl(float lp, float lo, float m2) {
#pragma clang fp contract(off)
    const float d = lp - lo;
    const float e1 = expf(lo - lp);
    const float e2 = m2 * expf(-lp);
    const float s = ((-1.0f + d) + e1) + e2;
    return (0.5f * s) * VF_VLB_INV_LN2;
}

VF_VLB_HD float vf_vlb_dkl(float lp, float lo, float m2) {
#pragma clang fp contract(off)
    const float e1 = expf(lo - lp);
    const float e2 = m2 * expf(-lp);
    const float s = (1.0f - e1) - e2;
    return (0.5f * s) * VF_VLB_INV_LN2;
}

// Phi(x), the tanh approximation of the standard normal distribution function
VF_VLB_HD float vf_nll_cdf(float x) {
#pragma clang fp contract(off)
    const float x2 = x * x;
    const float x3 = x2 * x;
    const float c = 0.044715f * x3;
    const float s = x + c;
    const float u = 0.7978845608028654f * s;           // sqrt(2 / pi)
    return 0.5f * (1.0f + tanhf(u));
}

// -log2 p(x | mean, lp): the discretised Gaussian likelihood of a pixel x in [-1, 1] with bins of +-1/255, in bits
VF_VLB_HD float vf_nll_decoder(float x, float mean, float lp) {
#pragma clang fp contract(off)
    const float is = expf(-0.5f * lp);
    const float d = x - mean;
    const float plus = is * (d + 0.00392156862745098f);
    const float minus = is * (d - 0.00392156862745098f);
    float p;
    if (x < -0.999f) p = vf_nll_cdf(plus);
    else if (x > 0.999f) p = 1.0f - vf_nll_cdf(minus);
    else p = vf_nll_cdf(plus) - vf_nll_cdf(minus);
    return -(logf(fmaxf(p, 1e-12f)) * VF_VLB_INV_LN2);
}
