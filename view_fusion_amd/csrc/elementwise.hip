// Small HBM-bound helpers of the UNet: sinusoidal (level, angle) embedding, Swish,
// channel concat / split.  Reference: model/unet.py:142-157 (encoding), :180-182 (Swish),
// :134 (skip concat).
#include "common.h"
#include "rng.h"

namespace {

// out[s][0:cnt)=sin(level*f), [cnt:2cnt)=cos(level*f), [2cnt:3cnt)=sin(angle*f), [3cnt:4cnt)=cos(angle*f)
// f_k = exp(-ln(1e4) * k / cnt), cnt = dim / 4.
__global__ void sincos_embed_kernel(const float* __restrict__ level, const float* __restrict__ angle,
                                    float* __restrict__ out, int S, int dim) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= S * dim) return;
    const int s = idx / dim, j = idx - s * dim;
    const int cnt = dim >> 2, half = dim >> 1;
    const int jj = j < half ? j : j - half;
    const float v = j < half ? level[s] : angle[s];
    const int k = jj < cnt ? jj : jj - cnt;
    const float step = (float)k / (float)cnt;
    const float arg = v * expf(-9.210340371976184f * step);
    out[idx] = jj < cnt ? sinf(arg) : cosf(arg);
}

__global__ void swish_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = silu_f(x[i]);
}

__global__ void swish_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dy, float* __restrict__ dx,
                                 size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        const float z = x[i];
        const float sg = sigmoid_f(z);
        dx[i] = dy[i] * (sg * (1.0f + z * (1.0f - sg)));
    }
}

// nn.Dropout(p) of Block (unet.py:207-216, training mode only): y = x * (u >= p) / (1 - p) with the uniform
// draws u in [0,1) supplied by the caller (the host's RNG; the same kernel applied to dy is the backward).
__global__ void dropout_kernel(const float4* __restrict__ x, const float4* __restrict__ u, float4* __restrict__ y,
                               size_t n4, float p, float scale) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    const float4 a = x[i], r = u[i];
    y[i] = make_float4(r.x >= p ? a.x * scale : 0.f, r.y >= p ? a.y * scale : 0.f, r.z >= p ? a.z * scale : 0.f,
                       r.w >= p ? a.w * scale : 0.f);
}

// The same Dropout with the mask drawn here (csrc/rng.h, kind 5, "Dropout masks"): no u tensor, forward or saved; the
// same launch on dy is the backward.  x, y: [S][n4] float4; row v is view v - off[b] of sample b (off: int32 [B + 1]).
// grid (chunks of 256 float4, min(S, 65535)); one Philox call per float4.  Every index is bounded by n4 and S, which
// the launcher takes from the caller's tensor; off only selects the sample whose id is read (b in [0, B) by
// construction of the search).
__global__ void dropout_seeded_kernel(const float4* __restrict__ x, float4* __restrict__ y, unsigned long long seed,
                                      const long long* __restrict__ ids, const int* __restrict__ off, int B, int S,
                                      size_t n4, unsigned thr, float scale, unsigned layer) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    for (int v = blockIdx.y; v < S; v += gridDim.y) {
        int lo = 0, hi = B;                       // find b with off[b] <= v < off[b+1]
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (off[mid] <= v) lo = mid; else hi = mid;
        }
        uint32_t w[4];
        vf_rng_words(seed, (unsigned long long)ids[lo], VF_RNG_DROPOUT, vf_rng_dropout_step(layer, (uint32_t)(v - off[lo])),
                     (uint32_t)i, w);
        const float4 a = x[(size_t)v * n4 + i];
        y[(size_t)v * n4 + i] = make_float4(vf_rng_dropout_keep(w[0], thr) ? a.x * scale : 0.f,
                                            vf_rng_dropout_keep(w[1], thr) ? a.y * scale : 0.f,
                                            vf_rng_dropout_keep(w[2], thr) ? a.z * scale : 0.f,
                                            vf_rng_dropout_keep(w[3], thr) ? a.w * scale : 0.f);
    }
}

// out[s] = [a[s] | b[s]] along channels; na4 / nb4 = float4 per sample of a / b.
// split != 0 runs the copy the other way (out -> a, b).
__global__ void concat_kernel(float4* __restrict__ a, float4* __restrict__ b, float4* __restrict__ out, int na4,
                              int nb4, int split) {
    const int s = blockIdx.y;
    const int n4 = na4 + nb4;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += gridDim.x * blockDim.x) {
        float4* o = out + (size_t)s * n4 + i;
        float4* src = i < na4 ? a + (size_t)s * na4 + i : b + (size_t)s * nb4 + (i - na4);
        if (split) *src = *o; else *o = *src;
    }
}

}  // namespace

extern "C" {

int vf_sincos_embed(const float* level, const float* angle, float* out, int S, int dim, void* stream) {
    if (S <= 0) return 0;
    if (dim & 3) return (int)hipErrorInvalidValue;
    const int n = S * dim;
    hipLaunchKernelGGL(sincos_embed_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, level, angle,
                       out, S, dim);
    VF_RETURN_LAST_ERROR();
}

int vf_swish_fwd(const float* x, float* y, long n, void* stream) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(swish_fwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, y,
                       (size_t)n);
    VF_RETURN_LAST_ERROR();
}

int vf_swish_bwd(const float* x, const float* dy, float* dx, long n, void* stream) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(swish_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, dy,
                       dx, (size_t)n);
    VF_RETURN_LAST_ERROR();
}

// n a multiple of 4; 0 <= p < 1.
int vf_dropout(const float* x, const float* u, float* y, long n, float p, void* stream) {
    if (n <= 0) return 0;
    if ((n & 3) || !(p >= 0.f && p < 1.f)) return (int)hipErrorInvalidValue;
    const size_t n4 = (size_t)n >> 2;
    hipLaunchKernelGGL(dropout_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       (const float4*)x, (const float4*)u, (float4*)y, n4, p, 1.0f / (1.0f - p));
    VF_RETURN_LAST_ERROR();
}

static bool dropout_seeded_args_ok(int B, int S, long n, unsigned thr, int layer) {
    return B > 0 && S > 0 && n > 0 && !(n & 3) && thr <= (1u << 24) && layer >= 0 && layer < (1 << 16) &&
           (unsigned long long)(n >> 2) < (1ull << 32);
}

// x, y: [S][n]; ids: DEVICE int64 [B]; off: DEVICE int32 [B + 1] with off[B] == S (ops.view_offsets), every sample with
// at most 4095 views (the caller's check: the counts live on the device).  thr = ceil(float32(p) * 2^24),
// scale = 1.0f / (1.0f - p).
int vf_dropout_seeded(const float* x, float* y, unsigned long long seed, const long long* ids, const int* off, int B,
                      int S, long n, unsigned thr, float scale, int layer, void* stream) {
    if (S <= 0 || n <= 0) return 0;
    if (!dropout_seeded_args_ok(B, S, n, thr, layer) || !x || !y || !ids || !off) return (int)hipErrorInvalidValue;
    const size_t n4 = (size_t)n >> 2;
    hipLaunchKernelGGL(dropout_seeded_kernel, dim3((unsigned)((n4 + 255) / 256), (unsigned)(S < 65535 ? S : 65535)),
                       dim3(256), 0, (hipStream_t)stream, (const float4*)x, (float4*)y, seed, ids, off, B, S, n4, thr,
                       scale, (unsigned)layer);
    VF_RETURN_LAST_ERROR();
}

// The masks of vf_dropout_seeded on the CPU (HOST pointers, no stream, no GPU): keep [S][n], 1 = kept.  Refuses what
// the launcher refuses, and an off that is not a prefix sum of counts in [1, 4095] ending at S.
int vf_dropout_mask_host(unsigned long long seed, const long long* ids, const int* off, int B, int S, long n,
                         unsigned thr, int layer, unsigned char* keep) {
    if (!dropout_seeded_args_ok(B, S, n, thr, layer) || !ids || !off || !keep) return (int)hipErrorInvalidValue;
    if (off[0] != 0 || off[B] != S) return (int)hipErrorInvalidValue;
    for (int b = 0; b < B; ++b)
        if (off[b + 1] <= off[b] || off[b + 1] - off[b] > 4095) return (int)hipErrorInvalidValue;
    for (int b = 0; b < B; ++b)
        for (int v = off[b]; v < off[b + 1]; ++v)
            for (size_t i = 0; i < (size_t)n >> 2; ++i) {
                uint32_t w[4];
                vf_rng_words(seed, (unsigned long long)ids[b], VF_RNG_DROPOUT,
                             vf_rng_dropout_step((uint32_t)layer, (uint32_t)(v - off[b])), (uint32_t)i, w);
                for (int j = 0; j < 4; ++j) keep[(size_t)v * n + 4 * i + j] = (unsigned char)vf_rng_dropout_keep(w[j], thr);
            }
    return 0;
}

// a: [S][Ca*HW], b: [S][Cb*HW], out: [S][(Ca+Cb)*HW]; per-sample sizes in floats, multiples of 4.
int vf_concat_channels(float* a, float* b, float* out, int S, long na, long nb, int split, void* stream) {
    if (S <= 0) return 0;
    if ((na & 3) || (nb & 3)) return (int)hipErrorInvalidValue;
    const int na4 = (int)(na >> 2), nb4 = (int)(nb >> 2);
    int bx = (na4 + nb4 + 255) / 256;
    if (bx > 64) bx = 64;
    hipLaunchKernelGGL(concat_kernel, dim3(bx, S), dim3(256), 0, (hipStream_t)stream, (float4*)a, (float4*)b,
                       (float4*)out, na4, nb4, split);
    VF_RETURN_LAST_ERROR();
}

}  // extern "C"
