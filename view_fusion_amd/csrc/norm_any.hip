// GroupNorm(+Swish) and the row-sum helpers at ANY H*W: the routes norm.hip takes where its kernels refuse the shape
// (they hold a whole group in registers and index channels by shifts: H*W a power of two; the float4 helpers need rows
// of a multiple of 4 floats).  One workgroup per (view, group); x is read three times (mean, variance, output) instead
// of being held in registers, so a group of any size fits.  Fixed-order reductions throughout: bit-reproducible.
#include "any_geom.h"

namespace {

__device__ __forceinline__ float dsilu_mul_any(float z, float dy) {
    const float sg = sigmoid_f(z);
    return dy * (sg * (1.0f + z * (1.0f - sg)));
}

__global__ __launch_bounds__(256) void gn_any_fwd_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                         const float* __restrict__ beta, float* __restrict__ y,
                                                         float* __restrict__ mean_out, float* __restrict__ rstd_out, int C,
                                                         int HW, int cpg, float eps, int silu) {
    __shared__ float red[4];
    const int G = C / cpg;
    const int sg = blockIdx.x, s = sg / G, g = sg - s * G;
    const int n = cpg * HW;
    const size_t base = ((size_t)s * C + (size_t)g * cpg) * HW;
    const float* xb = x + base;
    float sum = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) sum += xb[i];
    const float inv_n = 1.0f / (float)n;
    const float mean = block_sum<256>(sum, red) * inv_n;
    float sq = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) {
        const float d = xb[i] - mean;
        sq += d * d;
    }
    const float var = block_sum<256>(sq, red) * inv_n;
    const float rstd = 1.0f / sqrtf(var + eps);
    if (threadIdx.x == 0) {
        mean_out[sg] = mean;
        rstd_out[sg] = rstd;
    }
    for (int i = threadIdx.x; i < n; i += 256) {
        const int c = g * cpg + i / HW;
        const float ga = gamma[c] * rstd;
        const float be = beta[c] - mean * ga;
        float o = xb[i] * ga + be;
        if (silu) o = silu_f(o);
        y[base + i] = o;
    }
}

// dgamma_part[s][c] = sum_p dz * xhat, dbeta_part[s][c] = sum_p dz (dz = dy through the Swish), then
// dx = rstd (dz gamma - mean_group(gamma dz) - xhat mean_group(gamma dz xhat)) [+ addend] [+ addend2]
__global__ __launch_bounds__(256) void gn_any_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                         const float* __restrict__ gamma, const float* __restrict__ beta,
                                                         const float* __restrict__ mean, const float* __restrict__ rstd,
                                                         const float* __restrict__ addend, const float* __restrict__ addend2,
                                                         float* __restrict__ dx, float* __restrict__ dgamma_part,
                                                         float* __restrict__ dbeta_part, int C, int HW, int cpg, int silu) {
    __shared__ float red[4];
    const int G = C / cpg;
    const int sg = blockIdx.x, s = sg / G, g = sg - s * G;
    const float mu = mean[sg], r = rstd[sg];
    float s1 = 0.f, s2 = 0.f;
    for (int j = 0; j < cpg; ++j) {
        const int c = g * cpg + j;
        const float ga = gamma[c], be = beta[c];
        const size_t row = ((size_t)s * C + c) * HW;
        float a = 0.f, b = 0.f;
        for (int i = threadIdx.x; i < HW; i += 256) {
            const float xh = (x[row + i] - mu) * r;
            const float dz = silu ? dsilu_mul_any(xh * ga + be, dy[row + i]) : dy[row + i];
            a += dz;
            b += dz * xh;
        }
        a = block_sum<256>(a, red);
        b = block_sum<256>(b, red);
        if (threadIdx.x == 0) {
            dbeta_part[(size_t)s * C + c] = a;
            dgamma_part[(size_t)s * C + c] = b;
        }
        s1 += ga * a;
        s2 += ga * b;
    }
    const int n = cpg * HW;
    const float inv_n = 1.0f / (float)n;
    s1 *= inv_n;
    s2 *= inv_n;
    const size_t base = ((size_t)s * C + (size_t)g * cpg) * HW;
    for (int i = threadIdx.x; i < n; i += 256) {
        const int c = g * cpg + i / HW;
        const float ga = gamma[c], be = beta[c];
        const float xh = (x[base + i] - mu) * r;
        const float dz = silu ? dsilu_mul_any(xh * ga + be, dy[base + i]) : dy[base + i];
        float o = r * (dz * ga - (s1 + xh * s2));
        if (addend) o += addend[base + i];
        if (addend2) o += addend2[base + i];
        dx[base + i] = o;
    }
}

// one wave per row
__global__ __launch_bounds__(256) void rowsum_any_kernel(const float* __restrict__ x, float* __restrict__ out, int rows,
                                                         int len) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int lane = threadIdx.x & 63;
    const float* p = x + (size_t)row * len;
    float a = 0.f;
    for (int i = lane; i < len; i += 64) a += p[i];
    a = wave_sum(a);
    if (lane == 0) out[row] = a;
}

// dvb[s][c] = sum_p dy[s][c][p], db[c] = sum_s dvb[s][c]: one workgroup per channel, wave w takes views w, w+4, ...
__global__ __launch_bounds__(256) void bias_grad_any_kernel(const float* __restrict__ dy, float* __restrict__ db,
                                                            float* __restrict__ dvb, int S, int C, int HW) {
    __shared__ float red[4];
    const int c = blockIdx.x, lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    float tot = 0.f;
    for (int s = wid; s < S; s += 4) {
        const float* p = dy + ((size_t)s * C + c) * HW;
        float a = 0.f;
        for (int i = lane; i < HW; i += 64) a += p[i];
        a = wave_sum(a);
        if (lane == 0 && dvb) dvb[(size_t)s * C + c] = a;
        tot += a;
    }
    if (lane == 0) red[wid] = tot;
    __syncthreads();
    if (threadIdx.x == 0 && db) db[c] = (red[0] + red[1]) + (red[2] + red[3]);
}

}  // namespace

int vfi_gn_any_fwd(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd, int S, int C,
                   int HW, int groups, float eps, int silu, hipStream_t st) {
    if (S <= 0) return 0;
    if (groups <= 0 || C % groups != 0 || HW < 1) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(gn_any_fwd_kernel, dim3(S * groups), dim3(256), 0, st, x, gamma, beta, y, mean, rstd, C, HW,
                       C / groups, eps, silu);
    VF_RETURN_LAST_ERROR();
}

int vfi_gn_any_bwd(const float* x, const float* gamma, const float* beta, const float* mean, const float* rstd,
                   const float* dy, const float* addend, const float* addend2, float* dx, float* dgamma_part,
                   float* dbeta_part, int S, int C, int HW, int groups, int silu, hipStream_t st) {
    if (S <= 0) return 0;
    if (groups <= 0 || C % groups != 0 || HW < 1) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(gn_any_bwd_kernel, dim3(S * groups), dim3(256), 0, st, x, dy, gamma, beta, mean, rstd, addend,
                       addend2, dx, dgamma_part, dbeta_part, C, HW, C / groups, silu);
    VF_RETURN_LAST_ERROR();
}

int vfi_rowsum_any(const float* x, float* out, int rows, int len, hipStream_t st) {
    if (rows <= 0) return 0;
    hipLaunchKernelGGL(rowsum_any_kernel, dim3((rows + 3) / 4), dim3(256), 0, st, x, out, rows, len);
    VF_RETURN_LAST_ERROR();
}

int vfi_bias_grad_any(const float* dy, float* db, float* dvb, int S, int C, int HW, hipStream_t st) {
    if (S <= 0 || C <= 0) return 0;
    hipLaunchKernelGGL(bias_grad_any_kernel, dim3(C), dim3(256), 0, st, dy, db, dvb, S, C, HW);
    VF_RETURN_LAST_ERROR();
}
