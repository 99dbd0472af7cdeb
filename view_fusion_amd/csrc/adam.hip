// Multi-tensor Adam: every parameter of the model updated by ONE launch (reference optimizer:
// torch.optim.Adam(lr, betas=(0.9,0.999), eps=1e-8, no weight decay / amsgrad), experiment.py:118-120;
// the LR comes from the host-side schedule utils/schedulers.py:10-14).  HBM-bound: 16 B read +
// 12 B written per parameter.  Same arithmetic as torch's single-tensor path:
//   m = b1 m + (1-b1) g ; v = b2 v + (1-b2) g^2 ; p -= (lr / bc1) * m / (sqrt(v)/sqrt(bc2) + eps)
#include "common.h"
#include "adam_update.h"

namespace {

struct AdamDesc {
    float* p;
    const float* g;
    float* m;
    float* v;
    long long numel, first_block;
};

constexpr int ADAM_PER_BLOCK = 1024;   // 256 threads x 4 elements

// scal (or null): device float[3] {lr, bc1, bc2} read at run time instead of the launch arguments -- a HIP-graph replay
// of the training step takes the step-dependent scalars from memory the host refreshes before every replay
__global__ __launch_bounds__(256) void adam_multi_kernel(const AdamDesc* __restrict__ desc, int ntensors, float lr,
                                                         float b1, float b2, float eps, float bc1, float bc2,
                                                         const float* __restrict__ scal) {
    if (scal) { lr = scal[0]; bc1 = scal[1]; bc2 = scal[2]; }
    int lo = 0, hi = ntensors;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (desc[mid].first_block <= (long long)blockIdx.x) lo = mid; else hi = mid;
    }
    const AdamDesc d = desc[lo];
    const long long base = ((long long)blockIdx.x - d.first_block) * ADAM_PER_BLOCK + 4 * threadIdx.x;
    if (base >= d.numel) return;
    const float step = lr / bc1, rs = 1.0f / sqrtf(bc2), omb1 = 1.0f - b1, omb2 = 1.0f - b2;
    auto upd = [&](float& p, float g, float& m, float& v) { vf_adam_update(p, g, m, v, b1, b2, omb1, omb2, step, rs, eps); };
    if (base + 4 <= d.numel) {
        float4 p = *reinterpret_cast<float4*>(d.p + base);
        const float4 g = *reinterpret_cast<const float4*>(d.g + base);
        float4 m = *reinterpret_cast<float4*>(d.m + base);
        float4 v = *reinterpret_cast<float4*>(d.v + base);
        upd(p.x, g.x, m.x, v.x); upd(p.y, g.y, m.y, v.y); upd(p.z, g.z, m.z, v.z); upd(p.w, g.w, m.w, v.w);
        *reinterpret_cast<float4*>(d.p + base) = p;
        *reinterpret_cast<float4*>(d.m + base) = m;
        *reinterpret_cast<float4*>(d.v + base) = v;
    } else {
        for (long long i = base; i < d.numel; ++i) {
            float p = d.p[i], m = d.m[i], v = d.v[i];
            upd(p, d.g[i], m, v);
            d.p[i] = p; d.m[i] = m; d.v[i] = v;
        }
    }
}


// ---- the opt-in extras of optim.FusedAdam: global-norm clipping and a weight EMA ----------------------------------------
// Sum of squares of ONE 1024-element block of one tensor's gradient, in double (the square of a float is exact in double
// and a sum of 1024 of them loses nothing a float result could show); partial[blockIdx.x] = that sum.  Fixed tree, no
// atomics: the same gradients give the same bits on every run.
__global__ __launch_bounds__(256) void grad_sumsq_kernel(const AdamDesc* __restrict__ desc, int ntensors,
                                                         double* __restrict__ partial) {
    __shared__ double red[4];
    int lo = 0, hi = ntensors;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (desc[mid].first_block <= (long long)blockIdx.x) lo = mid; else hi = mid;
    }
    const AdamDesc d = desc[lo];
    const long long base = ((long long)blockIdx.x - d.first_block) * ADAM_PER_BLOCK + 4 * threadIdx.x;
    double s = 0.0;
    if (base + 4 <= d.numel) {
        const float4 g = *reinterpret_cast<const float4*>(d.g + base);
        s = ((double)g.x * g.x + (double)g.y * g.y) + ((double)g.z * g.z + (double)g.w * g.w);
    } else {
        for (long long i = base; i < d.numel; ++i) s += (double)d.g[i] * d.g[i];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, VF_WAVE);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// One workgroup: thread i sums partial[i], partial[i + 256], ... in index order, then the fixed tree above.
// out[0] = norm = sqrt(sum) rounded to float, out[1] = scale = min(1, max_norm / (norm + 1e-6)) in float arithmetic
// (torch.nn.utils.clip_grad_norm_'s coefficient).  max_norm (or null: no clipping, scale = 1) is read from device memory.
__global__ __launch_bounds__(256) void grad_norm_finish_kernel(const double* __restrict__ partial, long n,
                                                               const float* __restrict__ max_norm,
                                                               float* __restrict__ out) {
    __shared__ double red[4];
    double s = 0.0;
    for (long i = threadIdx.x; i < n; i += 256) s += partial[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, VF_WAVE);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        const float norm = (float)sqrt((red[0] + red[1]) + (red[2] + red[3]));
        out[0] = norm;
        out[1] = max_norm ? fminf(1.0f, max_norm[0] / (norm + 1e-6f)) : 1.0f;
    }
}

// adam_multi_kernel with two optional extras.  gscale (or null): device float, the update reads g * gscale[0] (the
// stored gradient is left as it is).  ema (or null): device table of one EMA pointer per descriptor row, ema_scal =
// device {d, 1 - d}; after the parameter update ema = fma(d, ema, (1 - d) p_new)  (vf_ema_update).
__global__ __launch_bounds__(256) void adam_multi_ex_kernel(const AdamDesc* __restrict__ desc, float* const* __restrict__ ema,
                                                            int ntensors, float lr, float b1, float b2, float eps, float bc1,
                                                            float bc2, const float* __restrict__ scal,
                                                            const float* __restrict__ gscale,
                                                            const float* __restrict__ ema_scal) {
    if (scal) { lr = scal[0]; bc1 = scal[1]; bc2 = scal[2]; }
    int lo = 0, hi = ntensors;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (desc[mid].first_block <= (long long)blockIdx.x) lo = mid; else hi = mid;
    }
    const AdamDesc d = desc[lo];
    const long long base = ((long long)blockIdx.x - d.first_block) * ADAM_PER_BLOCK + 4 * threadIdx.x;
    if (base >= d.numel) return;
    float* const ep = ema ? ema[lo] : nullptr;
    const float gs = gscale ? gscale[0] : 1.0f;
    const float ed = ep ? ema_scal[0] : 0.f, eomd = ep ? ema_scal[1] : 0.f;
    const float step = lr / bc1, rs = 1.0f / sqrtf(bc2), omb1 = 1.0f - b1, omb2 = 1.0f - b2;
    auto upd = [&](float& p, float g, float& m, float& v) {
        if (gscale) g = g * gs;
        vf_adam_update(p, g, m, v, b1, b2, omb1, omb2, step, rs, eps);
    };
    if (base + 4 <= d.numel) {
        float4 p = *reinterpret_cast<float4*>(d.p + base);
        const float4 g = *reinterpret_cast<const float4*>(d.g + base);
        float4 m = *reinterpret_cast<float4*>(d.m + base);
        float4 v = *reinterpret_cast<float4*>(d.v + base);
        upd(p.x, g.x, m.x, v.x); upd(p.y, g.y, m.y, v.y); upd(p.z, g.z, m.z, v.z); upd(p.w, g.w, m.w, v.w);
        *reinterpret_cast<float4*>(d.p + base) = p;
        *reinterpret_cast<float4*>(d.m + base) = m;
        *reinterpret_cast<float4*>(d.v + base) = v;
        if (ep) {
            float4 e = *reinterpret_cast<float4*>(ep + base);
            vf_ema_update(e.x, p.x, ed, eomd); vf_ema_update(e.y, p.y, ed, eomd);
            vf_ema_update(e.z, p.z, ed, eomd); vf_ema_update(e.w, p.w, ed, eomd);
            *reinterpret_cast<float4*>(ep + base) = e;
        }
    } else {
        for (long long i = base; i < d.numel; ++i) {
            float p = d.p[i], m = d.m[i], v = d.v[i];
            upd(p, d.g[i], m, v);
            d.p[i] = p; d.m[i] = m; d.v[i] = v;
            if (ep) {
                float e = ep[i];
                vf_ema_update(e, p, ed, eomd);
                ep[i] = e;
            }
        }
    }
}

// p <-> ema in place for every descriptor row (the contents move; every address stays what captured graphs and the
// packed-weight caches hold)
__global__ __launch_bounds__(256) void swap_multi_kernel(const AdamDesc* __restrict__ desc, float* const* __restrict__ ema,
                                                         int ntensors) {
    int lo = 0, hi = ntensors;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (desc[mid].first_block <= (long long)blockIdx.x) lo = mid; else hi = mid;
    }
    const AdamDesc d = desc[lo];
    float* const ep = ema[lo];
    const long long base = ((long long)blockIdx.x - d.first_block) * ADAM_PER_BLOCK + 4 * threadIdx.x;
    if (base >= d.numel) return;
    if (base + 4 <= d.numel) {
        const float4 p = *reinterpret_cast<float4*>(d.p + base);
        const float4 e = *reinterpret_cast<float4*>(ep + base);
        *reinterpret_cast<float4*>(d.p + base) = e;
        *reinterpret_cast<float4*>(ep + base) = p;
    } else {
        for (long long i = base; i < d.numel; ++i) {
            const float p = d.p[i], e = ep[i];
            d.p[i] = e; ep[i] = p;
        }
    }
}

// Gradient accumulation: acc = beta acc + w g for every row (row.p = the accumulator, row.g = this micro-batch's gradient;
// m, v unused), scal = DEVICE {beta, w}: one captured launch serves every micro-batch position.  beta == 0 (the first
// micro-batch; uniform over the launch) never READS the accumulator, which may hold NaN or a stale step's sum.
// Elementwise, no atomics: bit-reproducible.  12 B per parameter (8 on the first micro-batch).
__global__ __launch_bounds__(256) void grad_accum_multi_kernel(const AdamDesc* __restrict__ desc, int ntensors,
                                                               const float* __restrict__ scal) {
    const float beta = scal[0], w = scal[1];
    int lo = 0, hi = ntensors;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (desc[mid].first_block <= (long long)blockIdx.x) lo = mid; else hi = mid;
    }
    const AdamDesc d = desc[lo];
    const long long base = ((long long)blockIdx.x - d.first_block) * ADAM_PER_BLOCK + 4 * threadIdx.x;
    if (base >= d.numel) return;
    if (beta == 0.0f) {
        if (base + 4 <= d.numel) {
            const float4 g = *reinterpret_cast<const float4*>(d.g + base);
            *reinterpret_cast<float4*>(d.p + base) = make_float4(vf_grad_accum_first(g.x, w), vf_grad_accum_first(g.y, w),
                                                                 vf_grad_accum_first(g.z, w), vf_grad_accum_first(g.w, w));
        } else {
            for (long long i = base; i < d.numel; ++i) d.p[i] = vf_grad_accum_first(d.g[i], w);
        }
        return;
    }
    if (base + 4 <= d.numel) {
        const float4 g = *reinterpret_cast<const float4*>(d.g + base);
        float4 a = *reinterpret_cast<float4*>(d.p + base);
        a.x = vf_grad_accum(a.x, g.x, beta, w); a.y = vf_grad_accum(a.y, g.y, beta, w);
        a.z = vf_grad_accum(a.z, g.z, beta, w); a.w = vf_grad_accum(a.w, g.w, beta, w);
        *reinterpret_cast<float4*>(d.p + base) = a;
    } else {
        for (long long i = base; i < d.numel; ++i) d.p[i] = vf_grad_accum(d.p[i], d.g[i], beta, w);
    }
}

__global__ void adam_set_scalars_ex_kernel(float* dst, float a, float b, float c, float* xs, float d, float omd,
                                           float max_norm) {
    if (dst) { dst[0] = a; dst[1] = b; dst[2] = c; }
    xs[0] = d; xs[1] = omd; xs[2] = max_norm;
}

}  // namespace

extern "C" {

// desc: device int64 [ntensors][6] rows {p, g, m, v, numel, first_block}; a block covers 1024
// elements of one tensor; all pointers 16-byte aligned.  bc1 = 1-beta1^t, bc2 = 1-beta2^t.
int vf_adam_multi(const void* desc, int ntensors, long total_blocks, float lr, float beta1, float beta2, float eps,
                  float bc1, float bc2, void* stream) {
    if (ntensors <= 0 || total_blocks <= 0) return 0;
    hipLaunchKernelGGL(adam_multi_kernel, dim3((unsigned)total_blocks), dim3(256), 0, (hipStream_t)stream,
                       (const AdamDesc*)desc, ntensors, lr, beta1, beta2, eps, bc1, bc2, (const float*)nullptr);
    VF_RETURN_LAST_ERROR();
}

__global__ void adam_set_scalars_kernel(float* dst, float a, float b, float c) {
    dst[0] = a; dst[1] = b; dst[2] = c;
}

// dst[0..2] = {lr, bc1, bc2}: the values travel as launch arguments (copied at enqueue time), so the host may run any
// number of replays ahead of the GPU without a staging buffer to guard
int vf_adam_set_scalars(float* dst, float lr, float bc1, float bc2, void* stream) {
    if (!dst) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(adam_set_scalars_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, dst, lr, bc1, bc2);
    VF_RETURN_LAST_ERROR();
}

// the same update with {lr, 1-beta1^t, 1-beta2^t} read from device memory (scalars: float[3]) when the kernel runs: the
// form a captured training step uses (the host rewrites the three floats before every graph replay)
int vf_adam_multi_dev(const void* desc, int ntensors, long total_blocks, const float* scalars, float beta1, float beta2,
                      float eps, void* stream) {
    if (ntensors <= 0 || total_blocks <= 0) return 0;
    if (!scalars) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(adam_multi_kernel, dim3((unsigned)total_blocks), dim3(256), 0, (hipStream_t)stream,
                       (const AdamDesc*)desc, ntensors, 0.f, beta1, beta2, eps, 1.f, 1.f, scalars);
    VF_RETURN_LAST_ERROR();
}

// ---- opt-in extras (optim.FusedAdam(ema_decay=, max_grad_norm=)); the entry points above are unchanged ----
// partial[b] = sum of squares (double) of block b's gradient elements, for the total_blocks blocks of one descriptor table
int vf_grad_sumsq_multi(const void* desc, int ntensors, long total_blocks, double* partial, void* stream) {
    if (ntensors <= 0 || total_blocks <= 0) return 0;
    if (!partial) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(grad_sumsq_kernel, dim3((unsigned)total_blocks), dim3(256), 0, (hipStream_t)stream,
                       (const AdamDesc*)desc, ntensors, partial);
    VF_RETURN_LAST_ERROR();
}

// out[0] = sqrt(partial[0] + ... + partial[n-1]) (fixed order, double), out[1] = min(1, max_norm[0] / (out[0] + 1e-6));
// max_norm: device float, or null for out[1] = 1
int vf_grad_norm_finish(const double* partial, long n, const float* max_norm, float* out, void* stream) {
    if (!out || n < 0 || (n > 0 && !partial)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(grad_norm_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, partial, n, max_norm, out);
    VF_RETURN_LAST_ERROR();
}

// vf_adam_multi with: gscale (device float or null) -- the update uses g * gscale[0]; ema_tab (device float*[ntensors] or
// null) + ema_scal (device {d, 1 - d}) -- ema = fma(d, ema, (1 - d) p_new) after the parameter update
int vf_adam_multi_ex(const void* desc, const void* ema_tab, int ntensors, long total_blocks, float lr, float beta1,
                     float beta2, float eps, float bc1, float bc2, const float* gscale, const float* ema_scal,
                     void* stream) {
    if (ntensors <= 0 || total_blocks <= 0) return 0;
    if (ema_tab && !ema_scal) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(adam_multi_ex_kernel, dim3((unsigned)total_blocks), dim3(256), 0, (hipStream_t)stream,
                       (const AdamDesc*)desc, (float* const*)ema_tab, ntensors, lr, beta1, beta2, eps, bc1, bc2,
                       (const float*)nullptr, gscale, ema_scal);
    VF_RETURN_LAST_ERROR();
}

// the device-scalar form (scalars: float[3] {lr, 1-beta1^t, 1-beta2^t}), as vf_adam_multi_dev
int vf_adam_multi_ex_dev(const void* desc, const void* ema_tab, int ntensors, long total_blocks, const float* scalars,
                         float beta1, float beta2, float eps, const float* gscale, const float* ema_scal, void* stream) {
    if (ntensors <= 0 || total_blocks <= 0) return 0;
    if (!scalars || (ema_tab && !ema_scal)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(adam_multi_ex_kernel, dim3((unsigned)total_blocks), dim3(256), 0, (hipStream_t)stream,
                       (const AdamDesc*)desc, (float* const*)ema_tab, ntensors, 0.f, beta1, beta2, eps, 1.f, 1.f, scalars,
                       gscale, ema_scal);
    VF_RETURN_LAST_ERROR();
}

// scalars[0..2] = {lr, bc1, bc2} (skipped when scalars is null: the eager form carries them as launch arguments) and
// xs[0..2] = {ema decay d, 1 - d, max_norm}; values travel as launch arguments like vf_adam_set_scalars
int vf_adam_set_scalars_ex(float* scalars, float lr, float bc1, float bc2, float* xs, float ema_d, float ema_omd,
                           float max_norm, void* stream) {
    if (!xs) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(adam_set_scalars_ex_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, scalars, lr, bc1, bc2, xs,
                       ema_d, ema_omd, max_norm);
    VF_RETURN_LAST_ERROR();
}

// exchange p <-> ema in place: desc rows as vf_adam_multi (only p, numel, first_block are read), ema_tab as above
int vf_swap_multi(const void* desc, const void* ema_tab, int ntensors, long total_blocks, void* stream) {
    if (ntensors <= 0 || total_blocks <= 0) return 0;
    if (!ema_tab) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(swap_multi_kernel, dim3((unsigned)total_blocks), dim3(256), 0, (hipStream_t)stream,
                       (const AdamDesc*)desc, (float* const*)ema_tab, ntensors);
    VF_RETURN_LAST_ERROR();
}

// ---- opt-in gradient accumulation (optim.FusedAdam.accumulate, train.Trainer(accum_steps=)) ----
// acc = scalars[0] * acc + scalars[1] * g per element (csrc/adam_update.h states the rounding); desc rows as vf_adam_multi
// with p = the accumulator and g = the gradient to add (m, v unused); scalars: DEVICE float[2] {beta, w}, written with
// vf_adam_set_scalars; beta == 0 does not read the accumulator
int vf_grad_accum_multi(const void* desc, int ntensors, long total_blocks, const float* scalars, void* stream) {
    if (ntensors <= 0 || total_blocks <= 0) return 0;
    if (!scalars) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(grad_accum_multi_kernel, dim3((unsigned)total_blocks), dim3(256), 0, (hipStream_t)stream,
                       (const AdamDesc*)desc, ntensors, scalars);
    VF_RETURN_LAST_ERROR();
}

}  // extern "C"
