// ViewFusion glue around the UNet: ragged view stacking (+ q_sample), softmax-over-views
// noise composition (+ MSE and its backward), and the fused reverse-diffusion step tail.
// Reference: model/view_fusion.py:162-164 (q_sample), :244-263 / :95-115 (stacking),
// :265-298 / :116-150 (compose / mean ablation / loss), :70-84,152-177 (posterior, p_sample).
//
// All HBM-bound and tiny next to the UNet; their point is that NOTHING here needs a host
// sync: ragged view counts come in as a device prefix-sum array `off[B+1]`.
//
// Seeded draws (rng.h: Philox4x32-10 keyed by seed and a per-sample id): draw_train, randn_ids and the reverse-step
// tail that computes its own z.  Opt-in; the unseeded kernels and entry points are untouched.
//
// Few-step sampling: sampler_step(_rng)_kernel is the same tail with a table-driven linear-multistep update
// (strided DDIM / DPM-Solver++ 2M) instead of the one-step DDPM posterior; the p_sample_tail kernels stay as they are.
//
// Loss options (loss_weight.h holds the specification): compose_loss_fwd / _finish / _bwd are siblings of the MSE
// kernels with a penalty template (mse / l1 / huber), a per-sample noise-level weight (min-SNR, P2), the per-sample
// loss handed back and an optional loss-by-level histogram -- same launch count, no atomics.  Opt-in; the MSE kernels
// and their entry points are untouched.
//
// Classifier-free guidance (Ho & Salimans, "Classifier-Free Diffusion Guidance").  This comment is the ONE written
// definition; tests/guidance_ref.py restates it.  Opt-in: siblings of the kernels above, which are untouched.
//   Null conditioning.  The unconditional input of sample b is its own noisy target next to an all-zero conditioning half
//     (all Cc channels, 3 or 6); its own level and angle (the relative angle in the `relative` configs) are kept.
//   Guided noise.  eps = g_b * eps_c + (1 - g_b) * eps_u, in this order with 1 - g_b formed first, so that g = 1 gives
//     eps_c and g = 0 gives eps_u exactly, contracted to a multiply-add or not.  eps_c: the composition over the sample's
//     real views (softmax-weighted, or the mean) as above; eps_u: noise channels 0..2 of the sample's null row (that
//     row's logit channels are ignored); g_b: a per-sample fp32 scale read from device memory (g > 1 extrapolates).
//     The weights handed back stay the conditional softmax weights.
//   Rows of a guided step.  The stacked batch has S + B rows: rows 0..S-1 are the unguided step's, under the same `off`
//     table, and row S + b (S = off[B]) is sample b's null row.  Nothing that reads `off` changes meaning.
//   Training drop (seeded; rng.h).  Sample `id` is dropped iff (w2 >> 8) < thr, w2 = word 2 of the kind-0, step-0, block-0
//     call that already gives t (word 0) and u (word 1), thr = ceil(p * 2^24) computed on the host: an integer compare.
//     p = 1 drops every sample; p = 0 is "off" and launches nothing.
//   A dropped sample keeps its view_count: ALL its rows get the zero conditioning half, so S, `off` and every shape stay
//     static for a captured step.  Its rows are then identical, so the composition (a convex combination) returns that one
//     prediction -- the prediction of the single null row that sampling uses.
#include "common.h"
#include "loss_weight.h"
#include "rng.h"

namespace {

__device__ __forceinline__ int sample_of_view(const int* __restrict__ off, int B, int v) {
    int lo = 0, hi = B;                       // find b with off[b] <= v < off[b+1]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= v) lo = mid; else hi = mid;
    }
    return lo;
}

// x[v] = [ y_cond[b][v-off[b]] | y_t[b] ]  with optional q_sample on the fly:
//   y_t' = sqrt(level_b) * y_t + sqrt(1-level_b) * noise.
// The conditioning part has Cc channels (3 = an RGB view; 6 = the `relative` configs' view pair,
// experiment.py:274-283 / configs/relative-small-v100-4.yaml:22), the noisy target always 3.
// grid (chunks, S); nc4 = Cc*HW/4 and n4 = 3*HW/4 float4 per image.
__global__ void stack_views_kernel(const float4* __restrict__ y_cond, const float4* __restrict__ y_t,
                                   const float4* __restrict__ noise, const float* __restrict__ level,
                                   const float* __restrict__ angle, const int* __restrict__ off,
                                   float4* __restrict__ x, float* __restrict__ level_s, float* __restrict__ angle_s,
                                   int B, int Nmax, int nc4, int n4, int copy_cond) {
    const int v = blockIdx.y;
    const int b = sample_of_view(off, B, v);
    const int j = v - off[b];
    const float lv = level[b];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        level_s[v] = lv;
        angle_s[v] = angle[b];
    }
    const float sa = sqrtf(lv), sb = sqrtf(1.0f - lv);
    const float4* c = y_cond + ((size_t)b * Nmax + j) * nc4;
    const float4* t = y_t + (size_t)b * n4;
    const float4* z = noise ? noise + (size_t)b * n4 : nullptr;
    float4* o = x + (size_t)v * (nc4 + n4);
    if (copy_cond)
        for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < nc4; i += gridDim.x * blockDim.x) o[i] = c[i];
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += gridDim.x * blockDim.x) {
        float4 y = t[i];
        if (z) {
            const float4 e = z[i];
            y.x = sa * y.x + sb * e.x;
            y.y = sa * y.y + sb * e.y;
            y.z = sa * y.z + sb * e.z;
            y.w = sa * y.w + sb * e.w;
        }
        o[nc4 + i] = y;
    }
}

// stack_views_kernel with conditioning dropout and null rows (classifier-free guidance, see the head of this file).
// drop (uint8[B] | null): the conditioning half of every row of a sample with drop[b] != 0 is zeros; y_cond is not read
// for it.  grid (chunks, rows): rows = S, or S + B with null rows -- row S + b is [ 0 | y_t[b] ] with level[b], angle[b].
// The target half is stack_views_kernel's expression, so equal inputs give equal bits.
__global__ void stack_views_cfg_kernel(const float4* __restrict__ y_cond, const float4* __restrict__ y_t,
                                       const float4* __restrict__ noise, const float* __restrict__ level,
                                       const float* __restrict__ angle, const int* __restrict__ off,
                                       const unsigned char* __restrict__ drop, float4* __restrict__ x,
                                       float* __restrict__ level_s, float* __restrict__ angle_s, int B, int Nmax, int nc4,
                                       int n4, int copy_cond, int S) {
    const int v = blockIdx.y;
    const bool null_row = v >= S;
    const int b = null_row ? v - S : sample_of_view(off, B, v);
    const int j = null_row ? 0 : v - off[b];
    const bool zero = null_row || (drop != nullptr && drop[b] != 0);
    const float lv = level[b];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        level_s[v] = lv;
        angle_s[v] = angle[b];
    }
    const float sa = sqrtf(lv), sb = sqrtf(1.0f - lv);
    const float4* c = y_cond + ((size_t)b * Nmax + j) * nc4;
    const float4* t = y_t + (size_t)b * n4;
    const float4* z = noise ? noise + (size_t)b * n4 : nullptr;
    float4* o = x + (size_t)v * (nc4 + n4);
    if (copy_cond) {
        if (zero)
            for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < nc4; i += gridDim.x * blockDim.x)
                o[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        else
            for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < nc4; i += gridDim.x * blockDim.x) o[i] = c[i];
    }
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += gridDim.x * blockDim.x) {
        float4 y = t[i];
        if (z) {
            const float4 e = z[i];
            y.x = sa * y.x + sb * e.x;
            y.y = sa * y.y + sb * e.y;
            y.z = sa * y.z + sb * e.z;
            y.w = sa * y.w + sb * e.w;
        }
        o[nc4 + i] = y;
    }
}

// drop[b] = the training drop draw of sample ids[b] (rng.h: word 2 of the training-scalar call against thr)
__global__ void draw_cond_drop_kernel(unsigned long long seed, const long long* __restrict__ ids, unsigned thr,
                                      unsigned char* __restrict__ drop, int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    uint32_t w[4];
    vf_rng_words(seed, (unsigned long long)ids[b], VF_RNG_TRAIN_SCALARS, 0, 0, w);
    drop[b] = (unsigned char)vf_rng_cond_drop(w[2], thr);
}

// The guided combination of one float4: g eps_c + (1 - g) eps_u, gm = 1 - g formed by the caller.
__device__ __forceinline__ float4 guide4(float4 ec, const float* __restrict__ eu, float g, float gm) {
    const float4 u = *reinterpret_cast<const float4*>(eu);
    return make_float4(g * ec.x + gm * u.x, g * ec.y + gm * u.y, g * ec.z + gm * u.z, g * ec.w + gm * u.w);
}

// Composed noise for one float4 of (b, c, pixels): softmax over the sample's views of the
// logits (channels 3..5) weighting the per-view noise (channels 0..2); or the plain mean.
__device__ __forceinline__ float4 compose4(const float* __restrict__ out, int Cout, int HW, int v0, int v1, int c,
                                           int p, int weighting, float4* mx_out, float4* inv_out) {
    const size_t vs = (size_t)Cout * HW;
    const float* e0 = out + (size_t)v0 * vs + (size_t)c * HW + p;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (!weighting) {
        for (int v = v0; v < v1; ++v) {
            const float4 e = *reinterpret_cast<const float4*>(e0 + (size_t)(v - v0) * vs);
            acc.x += e.x; acc.y += e.y; acc.z += e.z; acc.w += e.w;
        }
        const float inv = 1.0f / (float)(v1 - v0);
        return make_float4(acc.x * inv, acc.y * inv, acc.z * inv, acc.w * inv);
    }
    const float* l0 = e0 + (size_t)3 * HW;
    float4 mx = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
    for (int v = v0; v < v1; ++v) {
        const float4 l = *reinterpret_cast<const float4*>(l0 + (size_t)(v - v0) * vs);
        mx.x = fmaxf(mx.x, l.x); mx.y = fmaxf(mx.y, l.y); mx.z = fmaxf(mx.z, l.z); mx.w = fmaxf(mx.w, l.w);
    }
    float4 sum = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int v = v0; v < v1; ++v) {
        const float4 l = *reinterpret_cast<const float4*>(l0 + (size_t)(v - v0) * vs);
        const float4 e = *reinterpret_cast<const float4*>(e0 + (size_t)(v - v0) * vs);
        const float wx = expf(l.x - mx.x), wy = expf(l.y - mx.y), wz = expf(l.z - mx.z), ww = expf(l.w - mx.w);
        sum.x += wx; sum.y += wy; sum.z += wz; sum.w += ww;
        acc.x += wx * e.x; acc.y += wy * e.y; acc.z += wz * e.z; acc.w += ww * e.w;
    }
    const float4 inv = make_float4(1.0f / sum.x, 1.0f / sum.y, 1.0f / sum.z, 1.0f / sum.w);
    if (mx_out) { *mx_out = mx; *inv_out = inv; }
    return make_float4(acc.x * inv.x, acc.y * inv.y, acc.z * inv.z, acc.w * inv.w);
}

// grid (chunks, B).  Writes noise_hat[B][3][HW]; optional weights[B][maxV][3][HW] (zero padded);
// optional per-block partial sums of (target - noise_hat)^2 into loss_part[B*chunks].
__global__ __launch_bounds__(256) void compose_fwd_kernel(const float* __restrict__ out, const int* __restrict__ off,
                                                          const float* __restrict__ target,
                                                          float* __restrict__ noise_hat, float* __restrict__ weights,
                                                          float* __restrict__ loss_part, int Cout, int HW, int maxV,
                                                          int weighting) {
    __shared__ float red[4];
    const int b = blockIdx.y;
    const int v0 = off[b], v1 = off[b + 1];
    const int n4 = 3 * HW / 4;
    float sq = 0.f;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n4; i += gridDim.x * 256) {
        const int c = (4 * i) / HW, p = 4 * i - c * HW;
        float4 mx, inv;
        const float4 nh = compose4(out, Cout, HW, v0, v1, c, p, weighting, &mx, &inv);
        const size_t o = (size_t)b * 3 * HW + 4 * (size_t)i;
        *reinterpret_cast<float4*>(noise_hat + o) = nh;
        if (target) {
            const float4 t = *reinterpret_cast<const float4*>(target + o);
            const float dx = t.x - nh.x, dy = t.y - nh.y, dz = t.z - nh.z, dw = t.w - nh.w;
            sq += (dx * dx + dy * dy) + (dz * dz + dw * dw);
        }
        if (weights && weighting) {
            const size_t vs = (size_t)Cout * HW;
            for (int j = 0; j < maxV; ++j) {
                float4 w = make_float4(0.f, 0.f, 0.f, 0.f);
                if (v0 + j < v1) {
                    const float4 l = *reinterpret_cast<const float4*>(out + (size_t)(v0 + j) * vs +
                                                                     (size_t)(3 + c) * HW + p);
                    w = make_float4(expf(l.x - mx.x) * inv.x, expf(l.y - mx.y) * inv.y, expf(l.z - mx.z) * inv.z,
                                    expf(l.w - mx.w) * inv.w);
                }
                *reinterpret_cast<float4*>(weights + (((size_t)b * maxV + j) * 3) * HW + 4 * (size_t)i) = w;
            }
        }
    }
    if (loss_part) {
        sq = block_sum<256>(sq, red);
        if (threadIdx.x == 0) loss_part[blockIdx.y * gridDim.x + blockIdx.x] = sq;
    }
}

__global__ void loss_finish_kernel(const float* __restrict__ part, float* __restrict__ loss, int n, float scale) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        float a = 0.f;
        for (int i = 0; i < n; ++i) a += part[i];
        *loss = a * scale;
    }
}

// d(out) for loss = mean((target - noise_hat)^2) * gloss:
//   g = 2 (nh - target) / n * gloss;  d eps_v = w_v g;  d logit_v = w_v (eps_v - nh) g
// (mean ablation: d eps_v = g / count, logits untouched -> zero).
__global__ __launch_bounds__(256) void compose_mse_bwd_kernel(const float* __restrict__ out,
                                                              const int* __restrict__ off,
                                                              const float* __restrict__ target,
                                                              const float* __restrict__ noise_hat,
                                                              const float* __restrict__ gloss,
                                                              float* __restrict__ dout, int Cout, int HW,
                                                              int weighting, float inv_n) {
    const int b = blockIdx.y;
    const int v0 = off[b], v1 = off[b + 1];
    const int n4 = 3 * HW / 4;
    const float gs = 2.0f * inv_n * gloss[0];
    const size_t vs = (size_t)Cout * HW;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n4; i += gridDim.x * 256) {
        const int c = (4 * i) / HW, p = 4 * i - c * HW;
        const size_t o = (size_t)b * 3 * HW + 4 * (size_t)i;
        const float4 nh = *reinterpret_cast<const float4*>(noise_hat + o);
        const float4 t = *reinterpret_cast<const float4*>(target + o);
        const float4 g = make_float4(gs * (nh.x - t.x), gs * (nh.y - t.y), gs * (nh.z - t.z), gs * (nh.w - t.w));
        if (!weighting) {
            const float inv = 1.0f / (float)(v1 - v0);
            const float4 d = make_float4(g.x * inv, g.y * inv, g.z * inv, g.w * inv);
            for (int v = v0; v < v1; ++v) {
                *reinterpret_cast<float4*>(dout + (size_t)v * vs + (size_t)c * HW + p) = d;
                if (Cout > 3)
                    *reinterpret_cast<float4*>(dout + (size_t)v * vs + (size_t)(3 + c) * HW + p) =
                        make_float4(0.f, 0.f, 0.f, 0.f);
            }
            continue;
        }
        float4 mx, inv;
        (void)compose4(out, Cout, HW, v0, v1, c, p, 1, &mx, &inv);
        for (int v = v0; v < v1; ++v) {
            const float* ep = out + (size_t)v * vs + (size_t)c * HW + p;
            const float4 e = *reinterpret_cast<const float4*>(ep);
            const float4 l = *reinterpret_cast<const float4*>(ep + (size_t)3 * HW);
            const float4 w = make_float4(expf(l.x - mx.x) * inv.x, expf(l.y - mx.y) * inv.y, expf(l.z - mx.z) * inv.z,
                                         expf(l.w - mx.w) * inv.w);
            float* dp = dout + (size_t)v * vs + (size_t)c * HW + p;
            *reinterpret_cast<float4*>(dp) = make_float4(w.x * g.x, w.y * g.y, w.z * g.z, w.w * g.w);
            *reinterpret_cast<float4*>(dp + (size_t)3 * HW) =
                make_float4(w.x * (e.x - nh.x) * g.x, w.y * (e.y - nh.y) * g.y, w.z * (e.z - nh.z) * g.z,
                            w.w * (e.w - nh.w) * g.w);
        }
    }
}

// One reverse step after the UNet: compose -> y0_hat = a_t y_t - b_t eps -> clamp ->
// mean = c1 y0_hat + c2 y_t -> y_{t-1} = mean + z * exp(0.5 logvar).
// `noise(i, o)` gives z for float4 i of the sample (o = its float offset in [B][3][HW]): a load, or a Philox draw.
// CFG: `out` has off[B] + B rows and the composed eps is guided by the sample's null row with the scale gscale[b].
template <bool CFG, class Noise>
__device__ __forceinline__ void p_sample_tail_body(
    const float* __restrict__ out, const int* __restrict__ off, const float* __restrict__ y_t,
    const long long* __restrict__ t, const float* __restrict__ sqrt_recip,
    const float* __restrict__ sqrt_recipm1, const float* __restrict__ logvar, const float* __restrict__ coef1,
    const float* __restrict__ coef2, float* __restrict__ y_next, float* __restrict__ mean_out,
    float* __restrict__ weights, int Cout, int HW, int maxV, int weighting, int clip, const float* __restrict__ gscale,
    Noise noise) {
    const int b = blockIdx.y;
    const int v0 = off[b], v1 = off[b + 1];
    const int n4 = 3 * HW / 4;
    float g = 1.0f, gm = 0.0f;
    const float* eu = nullptr;
    if constexpr (CFG) {
        g = gscale[b];
        gm = 1.0f - g;
        eu = out + (size_t)(off[gridDim.y] + b) * Cout * HW;
    }
    const long long tb = t[b];
    const float a_t = sqrt_recip[tb], b_t = sqrt_recipm1[tb], c1 = coef1[tb], c2 = coef2[tb];
    const float sd = expf(0.5f * logvar[tb]);
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n4; i += gridDim.x * 256) {
        const int c = (4 * i) / HW, p = 4 * i - c * HW;
        float4 mx, inv;
        float4 eps = compose4(out, Cout, HW, v0, v1, c, p, weighting, &mx, &inv);
        if constexpr (CFG) eps = guide4(eps, eu + (size_t)c * HW + p, g, gm);
        const size_t o = (size_t)b * 3 * HW + 4 * (size_t)i;
        const float4 y = *reinterpret_cast<const float4*>(y_t + o);
        float y0[4] = {a_t * y.x - b_t * eps.x, a_t * y.y - b_t * eps.y, a_t * y.z - b_t * eps.z,
                       a_t * y.w - b_t * eps.w};
        const float ys[4] = {y.x, y.y, y.z, y.w};
        float m[4], r[4];
        const float4 zz = noise(i, o);
        const float zs[4] = {zz.x, zz.y, zz.z, zz.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (clip) y0[k] = fminf(fmaxf(y0[k], -1.0f), 1.0f);
            m[k] = c1 * y0[k] + c2 * ys[k];
            r[k] = m[k] + zs[k] * sd;
        }
        if (y_next) *reinterpret_cast<float4*>(y_next + o) = make_float4(r[0], r[1], r[2], r[3]);
        if (mean_out) *reinterpret_cast<float4*>(mean_out + o) = make_float4(m[0], m[1], m[2], m[3]);
        if (weights && weighting) {
            const size_t vs = (size_t)Cout * HW;
            for (int j = 0; j < maxV; ++j) {
                float4 w = make_float4(0.f, 0.f, 0.f, 0.f);
                if (v0 + j < v1) {
                    const float4 l = *reinterpret_cast<const float4*>(out + (size_t)(v0 + j) * vs +
                                                                     (size_t)(3 + c) * HW + p);
                    w = make_float4(expf(l.x - mx.x) * inv.x, expf(l.y - mx.y) * inv.y, expf(l.z - mx.z) * inv.z,
                                    expf(l.w - mx.w) * inv.w);
                }
                *reinterpret_cast<float4*>(weights + (((size_t)b * maxV + j) * 3) * HW + 4 * (size_t)i) = w;
            }
        }
    }
}

__global__ __launch_bounds__(256) void p_sample_tail_kernel(
    const float* __restrict__ out, const int* __restrict__ off, const float* __restrict__ y_t,
    const float* __restrict__ z, const long long* __restrict__ t, const float* __restrict__ sqrt_recip,
    const float* __restrict__ sqrt_recipm1, const float* __restrict__ logvar, const float* __restrict__ coef1,
    const float* __restrict__ coef2, float* __restrict__ y_next, float* __restrict__ mean_out,
    float* __restrict__ weights, int Cout, int HW, int maxV, int weighting, int clip) {
    p_sample_tail_body<false>(out, off, y_t, t, sqrt_recip, sqrt_recipm1, logvar, coef1, coef2, y_next, mean_out,
                       weights, Cout, HW, maxV, weighting, clip, nullptr, [z](int, size_t o) {
                           float4 zz = make_float4(0.f, 0.f, 0.f, 0.f);
                           if (z) zz = *reinterpret_cast<const float4*>(z + o);
                           return zz;
                       });
}

// ... guided: `out` has off[B] + B rows, g [B] the guidance scales (the head of this file)
__global__ __launch_bounds__(256) void p_sample_tail_cfg_kernel(
    const float* __restrict__ out, const int* __restrict__ off, const float* __restrict__ y_t,
    const float* __restrict__ z, const long long* __restrict__ t, const float* __restrict__ sqrt_recip,
    const float* __restrict__ sqrt_recipm1, const float* __restrict__ logvar, const float* __restrict__ coef1,
    const float* __restrict__ coef2, float* __restrict__ y_next, float* __restrict__ mean_out,
    float* __restrict__ weights, int Cout, int HW, int maxV, int weighting, int clip,
    const float* __restrict__ g) {
    p_sample_tail_body<true>(out, off, y_t, t, sqrt_recip, sqrt_recipm1, logvar, coef1, coef2, y_next, mean_out,
                       weights, Cout, HW, maxV, weighting, clip, g, [z](int, size_t o) {
                           float4 zz = make_float4(0.f, 0.f, 0.f, 0.f);
                           if (z) zz = *reinterpret_cast<const float4*>(z + o);
                           return zz;
                       });
}

// The same step with z drawn in the kernel: kind 3, step = t[b], block = the float4 index; z = 0 where t[b] == 0.
// t and ids come from device memory, so a captured launch replays for every step.
__global__ __launch_bounds__(256) void p_sample_tail_rng_kernel(
    const float* __restrict__ out, const int* __restrict__ off, const float* __restrict__ y_t,
    unsigned long long seed, const long long* __restrict__ ids, const long long* __restrict__ t,
    const float* __restrict__ sqrt_recip, const float* __restrict__ sqrt_recipm1, const float* __restrict__ logvar,
    const float* __restrict__ coef1, const float* __restrict__ coef2, float* __restrict__ y_next,
    float* __restrict__ mean_out, float* __restrict__ weights, int Cout, int HW, int maxV, int weighting, int clip) {
    const unsigned long long id = (unsigned long long)ids[blockIdx.y];
    const long long tb = t[blockIdx.y];
    p_sample_tail_body<false>(out, off, y_t, t, sqrt_recip, sqrt_recipm1, logvar, coef1, coef2, y_next, mean_out,
                       weights, Cout, HW, maxV, weighting, clip, nullptr, [seed, id, tb](int i, size_t) {
                           float n[4] = {0.f, 0.f, 0.f, 0.f};
                           if (tb != 0) vf_rng_normal4(seed, id, VF_RNG_STEP_NOISE, (uint32_t)tb, (uint32_t)i, n);
                           return make_float4(n[0], n[1], n[2], n[3]);
                       });
}

// ... guided: `out` has off[B] + B rows, g [B] the guidance scales (the head of this file)
__global__ __launch_bounds__(256) void p_sample_tail_cfg_rng_kernel(
    const float* __restrict__ out, const int* __restrict__ off, const float* __restrict__ y_t,
    unsigned long long seed, const long long* __restrict__ ids, const long long* __restrict__ t,
    const float* __restrict__ sqrt_recip, const float* __restrict__ sqrt_recipm1, const float* __restrict__ logvar,
    const float* __restrict__ coef1, const float* __restrict__ coef2, float* __restrict__ y_next,
    float* __restrict__ mean_out, float* __restrict__ weights, int Cout, int HW, int maxV, int weighting, int clip,
    const float* __restrict__ g) {
    const unsigned long long id = (unsigned long long)ids[blockIdx.y];
    const long long tb = t[blockIdx.y];
    p_sample_tail_body<true>(out, off, y_t, t, sqrt_recip, sqrt_recipm1, logvar, coef1, coef2, y_next, mean_out,
                       weights, Cout, HW, maxV, weighting, clip, g, [seed, id, tb](int i, size_t) {
                           float n[4] = {0.f, 0.f, 0.f, 0.f};
                           if (tb != 0) vf_rng_normal4(seed, id, VF_RNG_STEP_NOISE, (uint32_t)tb, (uint32_t)i, n);
                           return make_float4(n[0], n[1], n[2], n[3]);
                       });
}

// One linear-multistep reverse step after the UNet (strided DDIM, DPM-Solver++ 2M; schedule.sampler_tables):
//   y0 = clamp(a[k] y - b[k] eps, -1, 1);  y_new = cy[k] y + c0[k] y0 + c1[k] y0_prev + sigma[k] z;  y0_prev <- y0
// with k = kidx[b] read from device memory.  sigma[k] == 0: `noise` is never called (no load, no draw);
// c1[k] == 0 or no history buffer: y0_prev is not read (it may hold anything before the first multistep step).
// Elementwise: y_next may be y, and y0_prev is read and written by the same thread.  CFG: as in p_sample_tail_body.
template <bool CFG, class Noise>
__device__ __forceinline__ void sampler_step_body(
    const float* __restrict__ out, const int* __restrict__ off, const float* __restrict__ y_t,
    const long long* __restrict__ kidx, const float* __restrict__ ta, const float* __restrict__ tb,
    const float* __restrict__ tcy, const float* __restrict__ tc0, const float* __restrict__ tc1,
    const float* __restrict__ tsigma, float* y0_prev, float* __restrict__ y_next, float* __restrict__ weights,
    int Cout, int HW, int maxV, int weighting, const float* __restrict__ gscale, Noise noise) {
    const int b = blockIdx.y;
    const int v0 = off[b], v1 = off[b + 1];
    const int n4 = 3 * HW / 4;
    float g = 1.0f, gm = 0.0f;
    const float* eu = nullptr;
    if constexpr (CFG) {
        g = gscale[b];
        gm = 1.0f - g;
        eu = out + (size_t)(off[gridDim.y] + b) * Cout * HW;
    }
    const long long k = kidx[b];
    const float a_k = ta[k], b_k = tb[k], cy = tcy[k], c0 = tc0[k], c1 = tc1[k], sg = tsigma[k];
    const bool hist = y0_prev != nullptr && c1 != 0.0f, noisy = sg != 0.0f;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n4; i += gridDim.x * 256) {
        const int c = (4 * i) / HW, p = 4 * i - c * HW;
        float4 mx, inv;
        float4 eps = compose4(out, Cout, HW, v0, v1, c, p, weighting, &mx, &inv);
        if constexpr (CFG) eps = guide4(eps, eu + (size_t)c * HW + p, g, gm);
        const size_t o = (size_t)b * 3 * HW + 4 * (size_t)i;
        const float4 y = *reinterpret_cast<const float4*>(y_t + o);
        const float ys[4] = {y.x, y.y, y.z, y.w};
        const float es[4] = {eps.x, eps.y, eps.z, eps.w};
        float y0[4], r[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            y0[j] = fminf(fmaxf(a_k * ys[j] - b_k * es[j], -1.0f), 1.0f);
            r[j] = cy * ys[j] + c0 * y0[j];
        }
        if (hist) {
            const float4 h = *reinterpret_cast<const float4*>(y0_prev + o);
            r[0] += c1 * h.x; r[1] += c1 * h.y; r[2] += c1 * h.z; r[3] += c1 * h.w;
        }
        if (noisy) {
            const float4 z = noise(i, o);
            r[0] += sg * z.x; r[1] += sg * z.y; r[2] += sg * z.z; r[3] += sg * z.w;
        }
        if (y0_prev) *reinterpret_cast<float4*>(y0_prev + o) = make_float4(y0[0], y0[1], y0[2], y0[3]);
        *reinterpret_cast<float4*>(y_next + o) = make_float4(r[0], r[1], r[2], r[3]);
        if (weights && weighting) {
            const size_t vs = (size_t)Cout * HW;
            for (int j = 0; j < maxV; ++j) {
                float4 w = make_float4(0.f, 0.f, 0.f, 0.f);
                if (v0 + j < v1) {
                    const float4 l = *reinterpret_cast<const float4*>(out + (size_t)(v0 + j) * vs +
                                                                     (size_t)(3 + c) * HW + p);
                    w = make_float4(expf(l.x - mx.x) * inv.x, expf(l.y - mx.y) * inv.y, expf(l.z - mx.z) * inv.z,
                                    expf(l.w - mx.w) * inv.w);
                }
                *reinterpret_cast<float4*>(weights + (((size_t)b * maxV + j) * 3) * HW + 4 * (size_t)i) = w;
            }
        }
    }
}

// z loaded from a buffer; z == null is "no noise" whatever sigma says
__global__ __launch_bounds__(256) void sampler_step_kernel(
    const float* __restrict__ out, const int* __restrict__ off, const float* __restrict__ y_t,
    const float* __restrict__ z, const long long* __restrict__ kidx, const float* __restrict__ ta,
    const float* __restrict__ tb, const float* __restrict__ tcy, const float* __restrict__ tc0,
    const float* __restrict__ tc1, const float* __restrict__ tsigma, float* y0_prev, float* __restrict__ y_next,
    float* __restrict__ weights, int Cout, int HW, int maxV, int weighting) {
    sampler_step_body<false>(out, off, y_t, kidx, ta, tb, tcy, tc0, tc1, tsigma, y0_prev, y_next, weights, Cout, HW,
                      maxV, weighting, nullptr, [z](int, size_t o) {
                          float4 zz = make_float4(0.f, 0.f, 0.f, 0.f);
                          if (z) zz = *reinterpret_cast<const float4*>(z + o);
                          return zz;
                      });
}

// ... guided: `out` has off[B] + B rows, g [B] the guidance scales (the head of this file)
__global__ __launch_bounds__(256) void sampler_step_cfg_kernel(
    const float* __restrict__ out, const int* __restrict__ off, const float* __restrict__ y_t,
    const float* __restrict__ z, const long long* __restrict__ kidx, const float* __restrict__ ta,
    const float* __restrict__ tb, const float* __restrict__ tcy, const float* __restrict__ tc0,
    const float* __restrict__ tc1, const float* __restrict__ tsigma, float* y0_prev, float* __restrict__ y_next,
    float* __restrict__ weights, int Cout, int HW, int maxV, int weighting,
    const float* __restrict__ g) {
    sampler_step_body<true>(out, off, y_t, kidx, ta, tb, tcy, tc0, tc1, tsigma, y0_prev, y_next, weights, Cout, HW,
                      maxV, weighting, g, [z](int, size_t o) {
                          float4 zz = make_float4(0.f, 0.f, 0.f, 0.f);
                          if (z) zz = *reinterpret_cast<const float4*>(z + o);
                          return zz;
                      });
}

// z drawn in the kernel, keyed as in p_sample_tail_rng_kernel with the MODEL timestep tau[k] as the step, so a
// strided chain and the full chain draw the same z at the same noise level.
__global__ __launch_bounds__(256) void sampler_step_rng_kernel(
    const float* __restrict__ out, const int* __restrict__ off, const float* __restrict__ y_t,
    unsigned long long seed, const long long* __restrict__ ids, const long long* __restrict__ kidx,
    const long long* __restrict__ tau, const float* __restrict__ ta, const float* __restrict__ tb,
    const float* __restrict__ tcy, const float* __restrict__ tc0, const float* __restrict__ tc1,
    const float* __restrict__ tsigma, float* y0_prev, float* __restrict__ y_next, float* __restrict__ weights,
    int Cout, int HW, int maxV, int weighting) {
    const unsigned long long id = (unsigned long long)ids[blockIdx.y];
    const uint32_t step = (uint32_t)tau[kidx[blockIdx.y]];
    sampler_step_body<false>(out, off, y_t, kidx, ta, tb, tcy, tc0, tc1, tsigma, y0_prev, y_next, weights, Cout, HW,
                      maxV, weighting, nullptr, [seed, id, step](int i, size_t) {
                          float n[4];
                          vf_rng_normal4(seed, id, VF_RNG_STEP_NOISE, step, (uint32_t)i, n);
                          return make_float4(n[0], n[1], n[2], n[3]);
                      });
}

// ... guided: `out` has off[B] + B rows, g [B] the guidance scales (the head of this file)
__global__ __launch_bounds__(256) void sampler_step_cfg_rng_kernel(
    const float* __restrict__ out, const int* __restrict__ off, const float* __restrict__ y_t,
    unsigned long long seed, const long long* __restrict__ ids, const long long* __restrict__ kidx,
    const long long* __restrict__ tau, const float* __restrict__ ta, const float* __restrict__ tb,
    const float* __restrict__ tcy, const float* __restrict__ tc0, const float* __restrict__ tc1,
    const float* __restrict__ tsigma, float* y0_prev, float* __restrict__ y_next, float* __restrict__ weights,
    int Cout, int HW, int maxV, int weighting,
    const float* __restrict__ g) {
    const unsigned long long id = (unsigned long long)ids[blockIdx.y];
    const uint32_t step = (uint32_t)tau[kidx[blockIdx.y]];
    sampler_step_body<true>(out, off, y_t, kidx, ta, tb, tcy, tc0, tc1, tsigma, y0_prev, y_next, weights, Cout, HW,
                      maxV, weighting, g, [seed, id, step](int i, size_t) {
                          float n[4];
                          vf_rng_normal4(seed, id, VF_RNG_STEP_NOISE, step, (uint32_t)i, n);
                          return make_float4(n[0], n[1], n[2], n[3]);
                      });
}

// Training draws of sample b (kind 0): t[b] in [1, T-1] as int64, u[b] in [0, 1) (optional output) and
// level[b] = (g[t] - g[t-1]) u + g[t-1]  (view_fusion.py:229-237).
__global__ void draw_train_kernel(unsigned long long seed, const long long* __restrict__ ids,
                                  const float* __restrict__ gammas, int T, long long* __restrict__ t,
                                  float* __restrict__ u, float* __restrict__ level, int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    uint32_t w[4];
    vf_rng_words(seed, (unsigned long long)ids[b], VF_RNG_TRAIN_SCALARS, 0, 0, w);
    const long long tb = vf_rng_timestep(w[0], T);
    const float ub = vf_rng_uniform24(w[1]);
    const float hi = gammas[tb], lo = gammas[tb - 1];
    t[b] = tb;
    if (u) u[b] = ub;
    level[b] = (hi - lo) * ub + lo;
}

// out[b][4 i .. 4 i + 3] = the four normals of (seed, ids[b], kind, step, block i); grid (chunks, B)
__global__ __launch_bounds__(256) void randn_ids_kernel(unsigned long long seed, const long long* __restrict__ ids,
                                                        int kind, int step, float4* __restrict__ out, int n4) {
    const unsigned long long id = (unsigned long long)ids[blockIdx.y];
    float4* o = out + (size_t)blockIdx.y * n4;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n4; i += gridDim.x * 256) {
        float n[4];
        vf_rng_normal4(seed, id, (uint32_t)kind, (uint32_t)step, (uint32_t)i, n);
        o[i] = make_float4(n[0], n[1], n[2], n[3]);
    }
}

// the raw words of the same counters (tests: device against host)
__global__ __launch_bounds__(256) void philox_ids_kernel(unsigned long long seed, const long long* __restrict__ ids,
                                                         int kind, int step, uint4* __restrict__ out, int n4) {
    const unsigned long long id = (unsigned long long)ids[blockIdx.y];
    uint4* o = out + (size_t)blockIdx.y * n4;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n4; i += gridDim.x * 256) {
        uint32_t w[4];
        vf_rng_words(seed, id, (uint32_t)kind, (uint32_t)step, (uint32_t)i, w);
        o[i] = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

// level[b] = table[t[b]]  (extract(), view_fusion.py:314-317) or the training draw
// level = (g[t]-g[t-1])*u + g[t-1]  (view_fusion.py:231-237) when u != null.
__global__ void gather_level_kernel(const float* __restrict__ gammas, const long long* __restrict__ t,
                                    const float* __restrict__ u, float* __restrict__ level, int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const long long tb = t[b];
    const float hi = gammas[tb];
    if (u) {
        const float lo = gammas[tb - 1];
        level[b] = (hi - lo) * u[b] + lo;
    } else {
        level[b] = hi;
    }
}

// psnr[b] = 20 log10(1 / sqrt(mean((a-b)^2)))  -- one workgroup per image (utils/metrics.py:6-8)
__global__ __launch_bounds__(256) void psnr_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                   float* __restrict__ out, int n) {
    __shared__ float red[4];
    const float4* a4 = reinterpret_cast<const float4*>(a + (size_t)blockIdx.x * n);
    const float4* b4 = reinterpret_cast<const float4*>(b + (size_t)blockIdx.x * n);
    float s = 0.f;
    for (int i = threadIdx.x; i < (n >> 2); i += 256) {
        const float4 u = a4[i], v = b4[i];
        const float dx = u.x - v.x, dy = u.y - v.y, dz = u.z - v.z, dw = u.w - v.w;
        s += (dx * dx + dy * dy) + (dz * dz + dw * dw);
    }
    s = block_sum<256>(s, red);
    if (threadIdx.x == 0) out[blockIdx.x] = 20.0f * log10f(1.0f / sqrtf(s / (float)n));
}

// ---- loss options: penalty x noise-level weight, per-sample loss, loss-by-level histogram (loss_weight.h) ----
// compose_fwd_kernel's sibling: the same noise_hat and the same (b, chunk) partial sums, of rho(noise_hat - target).
template <int PEN>
__global__ __launch_bounds__(256) void compose_loss_fwd_kernel(const float* __restrict__ out,
                                                               const int* __restrict__ off,
                                                               const float* __restrict__ target,
                                                               float* __restrict__ noise_hat,
                                                               float* __restrict__ loss_part, int Cout, int HW,
                                                               int weighting, float delta) {
    __shared__ float red[4];
    const int b = blockIdx.y;
    const int v0 = off[b], v1 = off[b + 1];
    const int n4 = 3 * HW / 4;
    float acc = 0.f;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n4; i += gridDim.x * 256) {
        const int c = (4 * i) / HW, p = 4 * i - c * HW;
        const float4 nh = compose4(out, Cout, HW, v0, v1, c, p, weighting, nullptr, nullptr);
        const size_t o = (size_t)b * 3 * HW + 4 * (size_t)i;
        *reinterpret_cast<float4*>(noise_hat + o) = nh;
        const float4 t = *reinterpret_cast<const float4*>(target + o);
        acc += (vf_loss_rho<PEN>(nh.x - t.x, delta) + vf_loss_rho<PEN>(nh.y - t.y, delta)) +
               (vf_loss_rho<PEN>(nh.z - t.z, delta) + vf_loss_rho<PEN>(nh.w - t.w, delta));
    }
    acc = block_sum<256>(acc, red);
    if (threadIdx.x == 0) loss_part[blockIdx.y * gridDim.x + blockIdx.x] = acc;
}

// One workgroup.  Per sample (one thread each): s_b = its `ch` partials in index order / n, w_b = the weight of its
// level; then loss = sum_b w_b s_b / B in index order (one thread); then, with a histogram attached, one thread per bin
// walks the samples in index order and adds the UNWEIGHTED s_b of its own bin into the persistent accumulators.  Every
// address is written by exactly one thread: no atomics, the same bits on every run.
__global__ __launch_bounds__(64) void compose_loss_finish_kernel(const float* __restrict__ part,
                                                                 const float* __restrict__ level,
                                                                 float* __restrict__ sample_loss,
                                                                 float* __restrict__ sample_w, float* __restrict__ loss,
                                                                 float* __restrict__ bin_sum, int* __restrict__ bin_cnt,
                                                                 int B, int ch, int K, float inv_n, int kind, float a,
                                                                 float b) {
    for (int s = threadIdx.x; s < B; s += 64) {
        float acc = 0.f;
        for (int c = 0; c < ch; ++c) acc += part[s * ch + c];
        sample_loss[s] = acc * inv_n;
        sample_w[s] = vf_loss_weight(kind, a, b, level[s]);
    }
    __syncthreads();                        // (also makes the workgroup's global stores above visible to it)
    if (threadIdx.x == 0) {
        float acc = 0.f;
        for (int s = 0; s < B; ++s) acc += sample_w[s] * sample_loss[s];
        *loss = acc / (float)B;
    }
    if (bin_sum == nullptr) return;
    for (int k = threadIdx.x; k < K; k += 64) {
        float sum = 0.f;
        int cnt = 0;
        for (int s = 0; s < B; ++s) {
            int bin = (int)(level[s] * (float)K);
            bin = bin > K - 1 ? K - 1 : bin;
            if (bin == k) {
                sum += sample_loss[s];
                ++cnt;
            }
        }
        bin_sum[k] += sum;
        bin_cnt[k] += cnt;
    }
}

// compose_mse_bwd_kernel's sibling: g = gloss w_b rho'(noise_hat - target) / (n B), then the same softmax / mean
// chain rule (d eps_v = w_v g;  d logit_v = w_v (eps_v - nh) g;  mean ablation: d eps_v = g / count, logits zero).
template <int PEN>
__global__ __launch_bounds__(256) void compose_loss_bwd_kernel(const float* __restrict__ out,
                                                               const int* __restrict__ off,
                                                               const float* __restrict__ target,
                                                               const float* __restrict__ noise_hat,
                                                               const float* __restrict__ gloss,
                                                               const float* __restrict__ sample_w,
                                                               float* __restrict__ dout, int Cout, int HW,
                                                               int weighting, float inv_nb, float delta) {
    const int b = blockIdx.y;
    const int v0 = off[b], v1 = off[b + 1];
    const int n4 = 3 * HW / 4;
    const float gs = gloss[0] * sample_w[b] * inv_nb;
    const size_t vs = (size_t)Cout * HW;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n4; i += gridDim.x * 256) {
        const int c = (4 * i) / HW, p = 4 * i - c * HW;
        const size_t o = (size_t)b * 3 * HW + 4 * (size_t)i;
        const float4 nh = *reinterpret_cast<const float4*>(noise_hat + o);
        const float4 t = *reinterpret_cast<const float4*>(target + o);
        const float4 g = make_float4(gs * vf_loss_drho<PEN>(nh.x - t.x, delta), gs * vf_loss_drho<PEN>(nh.y - t.y, delta),
                                     gs * vf_loss_drho<PEN>(nh.z - t.z, delta), gs * vf_loss_drho<PEN>(nh.w - t.w, delta));
        if (!weighting) {
            const float inv = 1.0f / (float)(v1 - v0);
            const float4 d = make_float4(g.x * inv, g.y * inv, g.z * inv, g.w * inv);
            for (int v = v0; v < v1; ++v) {
                *reinterpret_cast<float4*>(dout + (size_t)v * vs + (size_t)c * HW + p) = d;
                if (Cout > 3)
                    *reinterpret_cast<float4*>(dout + (size_t)v * vs + (size_t)(3 + c) * HW + p) =
                        make_float4(0.f, 0.f, 0.f, 0.f);
            }
            continue;
        }
        float4 mx, inv;
        (void)compose4(out, Cout, HW, v0, v1, c, p, 1, &mx, &inv);
        for (int v = v0; v < v1; ++v) {
            const float* ep = out + (size_t)v * vs + (size_t)c * HW + p;
            const float4 e = *reinterpret_cast<const float4*>(ep);
            const float4 l = *reinterpret_cast<const float4*>(ep + (size_t)3 * HW);
            const float4 w = make_float4(expf(l.x - mx.x) * inv.x, expf(l.y - mx.y) * inv.y, expf(l.z - mx.z) * inv.z,
                                         expf(l.w - mx.w) * inv.w);
            float* dp = dout + (size_t)v * vs + (size_t)c * HW + p;
            *reinterpret_cast<float4*>(dp) = make_float4(w.x * g.x, w.y * g.y, w.z * g.z, w.w * g.w);
            *reinterpret_cast<float4*>(dp + (size_t)3 * HW) =
                make_float4(w.x * (e.x - nh.x) * g.x, w.y * (e.y - nh.y) * g.y, w.z * (e.z - nh.z) * g.z,
                            w.w * (e.w - nh.w) * g.w);
        }
    }
}

inline int chunks_for(int n4) {
    int c = (n4 + 255) / 256;
    return c < 1 ? 1 : (c > 64 ? 64 : c);
}

}  // namespace

extern "C" {

int vf_psnr(const float* generated, const float* target, float* out, int B, int n, void* stream) {
    if (B <= 0) return 0;
    if (n & 3) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(psnr_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, generated, target, out, n);
    VF_RETURN_LAST_ERROR();
}

int vf_gather_level(const float* gammas, const long long* t, const float* u, float* level, int B, void* stream) {
    if (B <= 0) return 0;
    hipLaunchKernelGGL(gather_level_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, gammas, t, u,
                       level, B);
    VF_RETURN_LAST_ERROR();
}

// y_cond [B][Nmax][3][HW], y_t [B][3][HW], noise [B][3][HW] or null, level/angle [B],
// off [B+1] -> x [S][6][HW], level_s/angle_s [S].
int vf_stack_views(const float* y_cond, const float* y_t, const float* noise, const float* level,
                   const float* angle, const int* off, float* x, float* level_s, float* angle_s, int B, int Nmax,
                   int Cc, int HW, int S, int copy_cond, void* stream) {
    if (S <= 0) return 0;
    if ((HW & 3) || Cc < 1) return (int)hipErrorInvalidValue;
    const int n4 = 3 * HW / 4, nc4 = Cc * HW / 4;
    hipLaunchKernelGGL(stack_views_kernel, dim3(chunks_for(nc4 > n4 ? nc4 : n4), S), dim3(256), 0, (hipStream_t)stream,
                       (const float4*)y_cond, (const float4*)y_t, (const float4*)noise, level, angle, off,
                       (float4*)x, level_s, angle_s, B, Nmax, nc4, n4, copy_cond);
    VF_RETURN_LAST_ERROR();
}

// loss_part must hold B*64 floats when target != null.
int vf_compose_fwd(const float* unet_out, const int* off, const float* target, float* noise_hat, float* weights,
                   float* loss_part, float* loss, int B, int Cout, int HW, int maxV, int weighting, void* stream) {
    if (B <= 0) return 0;
    if ((HW & 3) || Cout < 3 || (weighting && Cout < 6)) return (int)hipErrorInvalidValue;
    hipStream_t st = (hipStream_t)stream;
    const int ch = chunks_for(3 * HW / 4);
    hipLaunchKernelGGL(compose_fwd_kernel, dim3(ch, B), dim3(256), 0, st, unet_out, off, target, noise_hat, weights,
                       target ? loss_part : nullptr, Cout, HW, maxV, weighting);
    if (target)
        hipLaunchKernelGGL(loss_finish_kernel, dim3(1), dim3(64), 0, st, loss_part, loss, B * ch,
                           1.0f / ((float)B * 3.0f * (float)HW));
    VF_RETURN_LAST_ERROR();
}

int vf_compose_mse_bwd(const float* unet_out, const int* off, const float* target, const float* noise_hat,
                       const float* gloss, float* dout, int B, int Cout, int HW, int weighting, void* stream) {
    if (B <= 0) return 0;
    if ((HW & 3) || Cout < 3 || (weighting && Cout < 6)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(compose_mse_bwd_kernel, dim3(chunks_for(3 * HW / 4), B), dim3(256), 0, (hipStream_t)stream,
                       unet_out, off, target, noise_hat, gloss, dout, Cout, HW, weighting,
                       1.0f / ((float)B * 3.0f * (float)HW));
    VF_RETURN_LAST_ERROR();
}

// ---- loss options (loss_weight.h): vf_compose_fwd with a target / vf_compose_mse_bwd with a penalty, a per-sample
// weight of `level`, the per-sample loss and an optional histogram.  Two launches forward, one backward, as those. ----
static inline bool loss_args_ok(int B, int Cout, int HW, int weighting, int penalty, float delta) {
    if ((HW & 3) || Cout < 3 || (weighting && Cout < 6)) return false;
    if (penalty < VF_LOSS_MSE || penalty > VF_LOSS_HUBER) return false;
    return penalty != VF_LOSS_HUBER || delta > 0.0f;
}

int vf_compose_loss_fwd(const float* unet_out, const int* off, const float* target, const float* level,
                        float* noise_hat, float* loss_part, float* sample_loss, float* sample_w, float* loss,
                        float* bin_sum, int* bin_cnt, int B, int Cout, int HW, int weighting, int penalty, float delta,
                        int weight_kind, float a, float b, int K, void* stream) {
    if (B <= 0) return 0;
    if (!loss_args_ok(B, Cout, HW, weighting, penalty, delta)) return (int)hipErrorInvalidValue;
    if (weight_kind < VF_LOSS_W_NONE || weight_kind > VF_LOSS_W_P2) return (int)hipErrorInvalidValue;
    if ((bin_sum == nullptr) != (bin_cnt == nullptr) || (bin_sum && K < 1)) return (int)hipErrorInvalidValue;
    if (!target || !level || !noise_hat || !loss_part || !sample_loss || !sample_w || !loss)
        return (int)hipErrorInvalidValue;
    hipStream_t st = (hipStream_t)stream;
    const int ch = chunks_for(3 * HW / 4);
    const dim3 grid(ch, B), block(256);
    if (penalty == VF_LOSS_L1)
        hipLaunchKernelGGL(compose_loss_fwd_kernel<VF_LOSS_L1>, grid, block, 0, st, unet_out, off, target, noise_hat,
                           loss_part, Cout, HW, weighting, delta);
    else if (penalty == VF_LOSS_HUBER)
        hipLaunchKernelGGL(compose_loss_fwd_kernel<VF_LOSS_HUBER>, grid, block, 0, st, unet_out, off, target, noise_hat,
                           loss_part, Cout, HW, weighting, delta);
    else
        hipLaunchKernelGGL(compose_loss_fwd_kernel<VF_LOSS_MSE>, grid, block, 0, st, unet_out, off, target, noise_hat,
                           loss_part, Cout, HW, weighting, delta);
    hipLaunchKernelGGL(compose_loss_finish_kernel, dim3(1), dim3(64), 0, st, loss_part, level, sample_loss, sample_w,
                       loss, bin_sum, bin_cnt, B, ch, K, 1.0f / (3.0f * (float)HW), weight_kind, a, b);
    VF_RETURN_LAST_ERROR();
}

int vf_compose_loss_bwd(const float* unet_out, const int* off, const float* target, const float* noise_hat,
                        const float* gloss, const float* sample_w, float* dout, int B, int Cout, int HW, int weighting,
                        int penalty, float delta, void* stream) {
    if (B <= 0) return 0;
    if (!loss_args_ok(B, Cout, HW, weighting, penalty, delta) || !sample_w) return (int)hipErrorInvalidValue;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(chunks_for(3 * HW / 4), B), block(256);
    const float inv_nb = 1.0f / ((float)B * 3.0f * (float)HW);
    if (penalty == VF_LOSS_L1)
        hipLaunchKernelGGL(compose_loss_bwd_kernel<VF_LOSS_L1>, grid, block, 0, st, unet_out, off, target, noise_hat,
                           gloss, sample_w, dout, Cout, HW, weighting, inv_nb, delta);
    else if (penalty == VF_LOSS_HUBER)
        hipLaunchKernelGGL(compose_loss_bwd_kernel<VF_LOSS_HUBER>, grid, block, 0, st, unet_out, off, target, noise_hat,
                           gloss, sample_w, dout, Cout, HW, weighting, inv_nb, delta);
    else
        hipLaunchKernelGGL(compose_loss_bwd_kernel<VF_LOSS_MSE>, grid, block, 0, st, unet_out, off, target, noise_hat,
                           gloss, sample_w, dout, Cout, HW, weighting, inv_nb, delta);
    VF_RETURN_LAST_ERROR();
}

// Host mirror: vf_loss_weight itself on the CPU.  HOST pointers, no stream.
int vf_loss_weights_host(const float* level, int B, int kind, float a, float b, float* out) {
    if (B < 0 || kind < VF_LOSS_W_NONE || kind > VF_LOSS_W_P2) return (int)hipErrorInvalidValue;
    for (int s = 0; s < B; ++s) out[s] = vf_loss_weight(kind, a, b, level[s]);
    return 0;
}

int vf_p_sample_tail(const float* unet_out, const int* off, const float* y_t, const float* z, const long long* t,
                     const float* sqrt_recip_gammas, const float* sqrt_recipm1_gammas,
                     const float* posterior_log_variance, const float* posterior_mean_coef1,
                     const float* posterior_mean_coef2, float* y_next, float* mean_out, float* weights, int B,
                     int Cout, int HW, int maxV, int weighting, int clip, void* stream) {
    if (B <= 0) return 0;
    if ((HW & 3) || Cout < 3 || (weighting && Cout < 6)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(p_sample_tail_kernel, dim3(chunks_for(3 * HW / 4), B), dim3(256), 0, (hipStream_t)stream,
                       unet_out, off, y_t, z, t, sqrt_recip_gammas, sqrt_recipm1_gammas, posterior_log_variance,
                       posterior_mean_coef1, posterior_mean_coef2, y_next, mean_out, weights, Cout, HW, maxV,
                       weighting, clip);
    VF_RETURN_LAST_ERROR();
}

// ---- seeded draws (rng.h) ----
static inline bool rng_args_ok(int kind, int step) { return kind >= 0 && kind <= 3 && step >= 0 && step < (1 << 28); }

int vf_draw_train(unsigned long long seed, const long long* ids, const float* gammas, int T, long long* t, float* u,
                  float* level, int B, void* stream) {
    if (B <= 0) return 0;
    if (T < 2 || T > (1 << 28)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(draw_train_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, seed, ids, gammas, T,
                       t, u, level, B);
    VF_RETURN_LAST_ERROR();
}

int vf_randn_ids(unsigned long long seed, const long long* ids, int kind, int step, float* out, int B, int n,
                 void* stream) {
    if (B <= 0 || n == 0) return 0;
    if (n < 0 || (n & 3) || !rng_args_ok(kind, step)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(randn_ids_kernel, dim3(chunks_for(n / 4), B), dim3(256), 0, (hipStream_t)stream, seed, ids, kind,
                       step, (float4*)out, n / 4);
    VF_RETURN_LAST_ERROR();
}

int vf_philox_ids(unsigned long long seed, const long long* ids, int kind, int step, unsigned* out, int B, int n,
                  void* stream) {
    if (B <= 0 || n == 0) return 0;
    if (n < 0 || (n & 3) || !rng_args_ok(kind, step)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(philox_ids_kernel, dim3(chunks_for(n / 4), B), dim3(256), 0, (hipStream_t)stream, seed, ids, kind,
                       step, (uint4*)out, n / 4);
    VF_RETURN_LAST_ERROR();
}

int vf_p_sample_tail_rng(const float* unet_out, const int* off, const float* y_t, unsigned long long seed,
                         const long long* ids, const long long* t, const float* sqrt_recip_gammas,
                         const float* sqrt_recipm1_gammas, const float* posterior_log_variance,
                         const float* posterior_mean_coef1, const float* posterior_mean_coef2, float* y_next,
                         float* mean_out, float* weights, int B, int Cout, int HW, int maxV, int weighting, int clip,
                         void* stream) {
    if (B <= 0) return 0;
    if ((HW & 3) || Cout < 3 || (weighting && Cout < 6)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(p_sample_tail_rng_kernel, dim3(chunks_for(3 * HW / 4), B), dim3(256), 0, (hipStream_t)stream,
                       unet_out, off, y_t, seed, ids, t, sqrt_recip_gammas, sqrt_recipm1_gammas, posterior_log_variance,
                       posterior_mean_coef1, posterior_mean_coef2, y_next, mean_out, weights, Cout, HW, maxV, weighting,
                       clip);
    VF_RETURN_LAST_ERROR();
}

// ---- few-step samplers: one linear-multistep tail (tables: schedule.sampler_tables) ----
int vf_sampler_step(const float* unet_out, const int* off, const float* y_t, const float* z, const long long* kidx,
                    const float* a, const float* b, const float* cy, const float* c0, const float* c1,
                    const float* sigma, float* y0_prev, float* y_next, float* weights, int B, int Cout, int HW,
                    int maxV, int weighting, void* stream) {
    if (B <= 0) return 0;
    if ((HW & 3) || Cout < 3 || (weighting && Cout < 6) || !y_next) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(sampler_step_kernel, dim3(chunks_for(3 * HW / 4), B), dim3(256), 0, (hipStream_t)stream,
                       unet_out, off, y_t, z, kidx, a, b, cy, c0, c1, sigma, y0_prev, y_next, weights, Cout, HW, maxV,
                       weighting);
    VF_RETURN_LAST_ERROR();
}

int vf_sampler_step_rng(const float* unet_out, const int* off, const float* y_t, unsigned long long seed,
                        const long long* ids, const long long* kidx, const long long* tau, const float* a,
                        const float* b, const float* cy, const float* c0, const float* c1, const float* sigma,
                        float* y0_prev, float* y_next, float* weights, int B, int Cout, int HW, int maxV,
                        int weighting, void* stream) {
    if (B <= 0) return 0;
    if ((HW & 3) || Cout < 3 || (weighting && Cout < 6) || !y_next) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(sampler_step_rng_kernel, dim3(chunks_for(3 * HW / 4), B), dim3(256), 0, (hipStream_t)stream,
                       unet_out, off, y_t, seed, ids, kidx, tau, a, b, cy, c0, c1, sigma, y0_prev, y_next, weights,
                       Cout, HW, maxV, weighting);
    VF_RETURN_LAST_ERROR();
}

// ---- classifier-free guidance (the head of this file): conditioning dropout, null rows, guided tails ----
// vf_stack_views with drop (DEVICE uint8 [B] | NULL) and null_rows: x [S (+ B)][Cc+3][HW], level_s / angle_s [S (+ B)].
int vf_stack_views_cfg(const float* y_cond, const float* y_t, const float* noise, const float* level,
                       const float* angle, const int* off, const unsigned char* drop, float* x, float* level_s,
                       float* angle_s, int B, int Nmax, int Cc, int HW, int S, int copy_cond, int null_rows,
                       void* stream) {
    if (S <= 0 || B <= 0) return 0;
    // a null row stands next to a sample's real rows: with null_rows every sample has at least one (S >= B); a
    // drop-only call takes any S, like vf_stack_views
    if ((HW & 3) || Cc < 1 || (null_rows && S < B)) return (int)hipErrorInvalidValue;
    const int rows = null_rows ? S + B : S;
    if (rows > 65535) return (int)hipErrorInvalidValue;
    const int n4 = 3 * HW / 4, nc4 = Cc * HW / 4;
    hipLaunchKernelGGL(stack_views_cfg_kernel, dim3(chunks_for(nc4 > n4 ? nc4 : n4), rows), dim3(256), 0,
                       (hipStream_t)stream, (const float4*)y_cond, (const float4*)y_t, (const float4*)noise, level, angle,
                       off, drop, (float4*)x, level_s, angle_s, B, Nmax, nc4, n4, copy_cond, S);
    VF_RETURN_LAST_ERROR();
}

int vf_draw_cond_drop(unsigned long long seed, const long long* ids, unsigned thr, unsigned char* drop, int B,
                      void* stream) {
    if (B <= 0) return 0;
    if (thr > (1u << 24)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(draw_cond_drop_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, seed, ids, thr,
                       drop, B);
    VF_RETURN_LAST_ERROR();
}

static inline bool tail_args_ok(int Cout, int HW, int weighting, const float* g) {
    return !((HW & 3) || Cout < 3 || (weighting && Cout < 6) || !g);
}

// The four guided tails: the sibling's arguments + g [B]; unet_out is [off[B] + B][Cout][HW].
int vf_p_sample_tail_cfg(const float* unet_out, const int* off, const float* y_t, const float* z, const long long* t,
                         const float* sqrt_recip_gammas, const float* sqrt_recipm1_gammas,
                         const float* posterior_log_variance, const float* posterior_mean_coef1,
                         const float* posterior_mean_coef2, float* y_next, float* mean_out, float* weights, int B,
                         int Cout, int HW, int maxV, int weighting, int clip, const float* g, void* stream) {
    if (B <= 0) return 0;
    if (!tail_args_ok(Cout, HW, weighting, g)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(p_sample_tail_cfg_kernel, dim3(chunks_for(3 * HW / 4), B), dim3(256), 0, (hipStream_t)stream,
                       unet_out, off, y_t, z, t, sqrt_recip_gammas, sqrt_recipm1_gammas, posterior_log_variance,
                       posterior_mean_coef1, posterior_mean_coef2, y_next, mean_out, weights, Cout, HW, maxV,
                       weighting, clip, g);
    VF_RETURN_LAST_ERROR();
}

int vf_p_sample_tail_cfg_rng(const float* unet_out, const int* off, const float* y_t, unsigned long long seed,
                             const long long* ids, const long long* t, const float* sqrt_recip_gammas,
                             const float* sqrt_recipm1_gammas, const float* posterior_log_variance,
                             const float* posterior_mean_coef1, const float* posterior_mean_coef2, float* y_next,
                             float* mean_out, float* weights, int B, int Cout, int HW, int maxV, int weighting,
                             int clip, const float* g, void* stream) {
    if (B <= 0) return 0;
    if (!tail_args_ok(Cout, HW, weighting, g)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(p_sample_tail_cfg_rng_kernel, dim3(chunks_for(3 * HW / 4), B), dim3(256), 0,
                       (hipStream_t)stream, unet_out, off, y_t, seed, ids, t, sqrt_recip_gammas, sqrt_recipm1_gammas,
                       posterior_log_variance, posterior_mean_coef1, posterior_mean_coef2, y_next, mean_out, weights,
                       Cout, HW, maxV, weighting, clip, g);
    VF_RETURN_LAST_ERROR();
}

int vf_sampler_step_cfg(const float* unet_out, const int* off, const float* y_t, const float* z,
                        const long long* kidx, const float* a, const float* b, const float* cy, const float* c0,
                        const float* c1, const float* sigma, float* y0_prev, float* y_next, float* weights, int B,
                        int Cout, int HW, int maxV, int weighting, const float* g, void* stream) {
    if (B <= 0) return 0;
    if (!tail_args_ok(Cout, HW, weighting, g) || !y_next) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(sampler_step_cfg_kernel, dim3(chunks_for(3 * HW / 4), B), dim3(256), 0, (hipStream_t)stream,
                       unet_out, off, y_t, z, kidx, a, b, cy, c0, c1, sigma, y0_prev, y_next, weights, Cout, HW, maxV,
                       weighting, g);
    VF_RETURN_LAST_ERROR();
}

int vf_sampler_step_cfg_rng(const float* unet_out, const int* off, const float* y_t, unsigned long long seed,
                            const long long* ids, const long long* kidx, const long long* tau, const float* a,
                            const float* b, const float* cy, const float* c0, const float* c1, const float* sigma,
                            float* y0_prev, float* y_next, float* weights, int B, int Cout, int HW, int maxV,
                            int weighting, const float* g, void* stream) {
    if (B <= 0) return 0;
    if (!tail_args_ok(Cout, HW, weighting, g) || !y_next) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(sampler_step_cfg_rng_kernel, dim3(chunks_for(3 * HW / 4), B), dim3(256), 0,
                       (hipStream_t)stream, unet_out, off, y_t, seed, ids, kidx, tau, a, b, cy, c0, c1, sigma, y0_prev,
                       y_next, weights, Cout, HW, maxV, weighting, g);
    VF_RETURN_LAST_ERROR();
}

// Host mirrors: the same inline functions on the CPU, HOST pointers, no stream (the CPU suite's side of the parity).
int vf_rng_host_philox(const unsigned* counter, const unsigned* key, unsigned* out) {
    vf_philox4x32_10(counter, key, out);
    return 0;
}

int vf_rng_host_normal(unsigned long long seed, const long long* ids, int kind, int step, float* out, int B, int n) {
    if (B < 0 || n < 0 || (n & 3) || !rng_args_ok(kind, step)) return (int)hipErrorInvalidValue;
    for (int b = 0; b < B; ++b)
        for (int i = 0; i < n / 4; ++i)
            vf_rng_normal4(seed, (unsigned long long)ids[b], (uint32_t)kind, (uint32_t)step, (uint32_t)i,
                           out + (size_t)b * n + 4 * (size_t)i);
    return 0;
}

int vf_rng_host_train_scalars(unsigned long long seed, const long long* ids, int T, long long* t, float* u, int B) {
    if (B < 0 || T < 2 || T > (1 << 28)) return (int)hipErrorInvalidValue;
    for (int b = 0; b < B; ++b) {
        uint32_t w[4];
        vf_rng_words(seed, (unsigned long long)ids[b], VF_RNG_TRAIN_SCALARS, 0, 0, w);
        t[b] = vf_rng_timestep(w[0], T);
        u[b] = vf_rng_uniform24(w[1]);
    }
    return 0;
}

// the training drop draw on the CPU: drop[b] = (word 2 >> 8) < thr for the ids (HOST int64 [B])
int vf_cond_drop_host(unsigned long long seed, const long long* ids, unsigned thr, unsigned char* drop, int B) {
    if (B < 0 || thr > (1u << 24)) return (int)hipErrorInvalidValue;
    for (int b = 0; b < B; ++b) {
        uint32_t w[4];
        vf_rng_words(seed, (unsigned long long)ids[b], VF_RNG_TRAIN_SCALARS, 0, 0, w);
        drop[b] = (unsigned char)vf_rng_cond_drop(w[2], thr);
    }
    return 0;
}

}  // extern "C"
