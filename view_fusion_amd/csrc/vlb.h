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
// Contraction is off inside every function here, so host and device round the same operations; expf is the accurate
// library function on both sides (they agree to its last-place error).
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
