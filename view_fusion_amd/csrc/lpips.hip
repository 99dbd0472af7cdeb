// LPIPS (vgg, version 0.1), the third eval metric of the reference (utils/compute_metrics.py:
// lpips.LPIPS(net="vgg")(2 gen - 1, 2 target - 1)).  The thirteen 3x3 convolutions of the VGG16 trunk run on the
// engine's own conv kernels (ops.conv2d); this file holds what is left around them:
//
//   prep          v = ((2 x - 1) - shift_c) / scale_c for both images, stacked on N: [generated | target] -> 2B images
//   relu          in place, float4 (+ scalar tail)
//   relu + pool   at a group end: the ReLU'd tap (in place) AND the 2x2 max-pooled input of the next group, one read
//   layer         per tap l and pixel p:  a^ = a / (sqrt(sum_c a_c^2) + 1e-10), likewise b^,
//                 d_l(p) = sum_c w_c (a^_c - b^_c)^2;  one partial sum_p d_l(p) / (H_l W_l) per workgroup
//   finish        out[b] = the image's partials of all taps, added in index order in double
//
// The distance kernel: a workgroup owns 64 * PPL consecutive pixels of one image pair; lanes run along pixels (every
// channel step is one coalesced load of a and of b), the four waves split the channels (wave w: w, w + 4, ...).  Sweep
// one accumulates the two sums of squares, exchanged through LDS and added in wave order; sweep two the weighted
// squared difference -- from registers where a wave's channels x PPL fit (CPW > 0: <= 128 data registers), from a
// second read (L2: the tile was just read) where they do not.  No atomics, every sum in a fixed order, no launch
// argument that depends on the data: bit-reproducible and capturable, as csrc/ssim.hip.
#include "common.h"

namespace {

// ---- prep ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float lpips_scale(float x, int c) {
#pragma clang fp contract(off)
    const float shift = c == 0 ? -0.030f : (c == 1 ? -0.088f : -0.188f);
    const float scale = c == 0 ? 0.458f : (c == 1 ? 0.448f : 0.450f);
    return ((2.f * x - 1.f) - shift) / scale;
}

// V = 4: HW % 4 == 0, a float4 never straddles two planes.  n = elements of ONE input (B * 3 * HW).
template <int V>
__global__ __launch_bounds__(256) void lpips_prep_kernel(const float* __restrict__ gen, const float* __restrict__ tgt,
                                                         float* __restrict__ out, long n, int HW) {
    const long e = ((long)blockIdx.x * 256 + threadIdx.x) * V;
    if (e >= n) return;
    const int c = (int)((e / HW) % 3);
    if (V == 4) {
        const f32x4 g = *reinterpret_cast<const f32x4*>(gen + e), t = *reinterpret_cast<const f32x4*>(tgt + e);
        f32x4 og, ot;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            og[j] = lpips_scale(g[j], c);
            ot[j] = lpips_scale(t[j], c);
        }
        *reinterpret_cast<f32x4*>(out + e) = og;
        *reinterpret_cast<f32x4*>(out + n + e) = ot;
    } else {
        out[e] = lpips_scale(gen[e], c);
        out[n + e] = lpips_scale(tgt[e], c);
    }
}

// ---- ReLU, ReLU + 2x2 max-pool ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void relu_kernel(float* __restrict__ x, long n) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const long n4 = n >> 2;
    if (i < n4) {
        f32x4 v = reinterpret_cast<f32x4*>(x)[i];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = fmaxf(v[j], 0.f);
        reinterpret_cast<f32x4*>(x)[i] = v;
    }
    if (i < (n & 3)) {                                       // scalar tail
        const long t = (n4 << 2) + i;
        x[t] = fmaxf(x[t], 0.f);
    }
}

// One thread: two rows x NX columns of one plane (NX = 4: W % 4 == 0, float4 rows; NX = 2: any even W, float2 rows --
// H and W even keep every row pair 8-byte aligned).  y is ReLU'd in place, pooled[plane][H/2][W/2] = the 2x2 maxima.
template <int NX>
__global__ __launch_bounds__(256) void relu_maxpool2_kernel(float* __restrict__ y, float* __restrict__ pooled, long nthreads,
                                                            int H, int W) {
    typedef float vec __attribute__((ext_vector_type(NX)));
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= nthreads) return;
    const int wq = W / NX, hq = H / 2;
    const int xq = (int)(i % wq), yq = (int)((i / wq) % hq);
    const long plane = i / ((long)wq * hq);
    float* r0 = y + (plane * H + 2 * yq) * W + NX * xq;
    vec a = *reinterpret_cast<vec*>(r0), b = *reinterpret_cast<vec*>(r0 + W);
#pragma unroll
    for (int j = 0; j < NX; ++j) {
        a[j] = fmaxf(a[j], 0.f);
        b[j] = fmaxf(b[j], 0.f);
    }
    *reinterpret_cast<vec*>(r0) = a;
    *reinterpret_cast<vec*>(r0 + W) = b;
    float* po = pooled + (plane * hq + yq) * (W / 2) + (NX / 2) * xq;
    if constexpr (NX == 4) {
        f32x2 m;
        m[0] = fmaxf(fmaxf(a[0], a[1]), fmaxf(b[0], b[1]));
        m[1] = fmaxf(fmaxf(a[2], a[3]), fmaxf(b[2], b[3]));
        *reinterpret_cast<f32x2*>(po) = m;
    } else {
        *po = fmaxf(fmaxf(a[0], a[1]), fmaxf(b[0], b[1]));
    }
}

// ---- per-tap distance ---------------------------------------------------------------------------------------------
struct LayerArgs {
    const float* feat;     // [2B][C][HW]: image b against image B + b
    const float* lin;      // [C]
    float* part;           // [B][slots]
    int B, C, HW, tiles, slot0, slots;
    float inv_hw;
};

template <int PPL>
__device__ __forceinline__ void load_px(const float* p, bool ok, float (&v)[PPL]) {
    if (PPL == 4) {
        f32x4 t = {0.f, 0.f, 0.f, 0.f};
        if (ok) t = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
        for (int j = 0; j < PPL; ++j) v[j] = t[j];
    } else {
        v[0] = ok ? *p : 0.f;
    }
}

__device__ __forceinline__ float weighted_sq_diff(float w, float a, float ia, float b, float ib) {
#pragma clang fp contract(off)            // equal features give exactly 0
    const float d = a * ia - b * ib;
    return w * (d * d);
}

// grid.x = B * tiles; CPW > 0: C == 4 * CPW and the wave's channels stay in registers; CPW == 0: any C, re-read.
// PPL == 4 needs HW % 4 == 0 (a lane's four pixels are all inside the map or all outside).
template <int CPW, int PPL>
__global__ __launch_bounds__(256) void lpips_layer_kernel(LayerArgs g) {
    constexpr int TP = 64 * PPL;
    __shared__ float ssq[2][4][TP];
    __shared__ float red[4];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int tile = (int)(blockIdx.x % (unsigned)g.tiles), b = (int)(blockIdx.x / (unsigned)g.tiles);
    const int px = lane * PPL, p0 = tile * TP + px;
    const bool ok = p0 < g.HW;
    const size_t HW = (size_t)g.HW;
    const float* pa = g.feat + ((size_t)b * g.C + wid) * HW + p0;              // channel wid of image b, this lane's pixels
    const float* pb = g.feat + ((size_t)(g.B + b) * g.C + wid) * HW + p0;
    const int nk = CPW > 0 ? CPW : (g.C - wid + 3) / 4;                        // channels wid, wid + 4, ... < C

    float ra[CPW > 0 ? CPW : 1][PPL], rb[CPW > 0 ? CPW : 1][PPL];
    float sa[PPL], sb[PPL];
#pragma unroll
    for (int j = 0; j < PPL; ++j) sa[j] = sb[j] = 0.f;
    if (CPW > 0) {
#pragma unroll
        for (int k = 0; k < CPW; ++k) {
            load_px<PPL>(pa + (size_t)(4 * k) * HW, ok, ra[k]);
            load_px<PPL>(pb + (size_t)(4 * k) * HW, ok, rb[k]);
        }
#pragma unroll
        for (int k = 0; k < CPW; ++k)
#pragma unroll
            for (int j = 0; j < PPL; ++j) {
                sa[j] += ra[k][j] * ra[k][j];
                sb[j] += rb[k][j] * rb[k][j];
            }
    } else {
#pragma unroll 8                              // eight channels' loads in flight: the small deep maps are latency-bound
        for (int k = 0; k < nk; ++k) {
            load_px<PPL>(pa + (size_t)(4 * k) * HW, ok, ra[0]);
            load_px<PPL>(pb + (size_t)(4 * k) * HW, ok, rb[0]);
#pragma unroll
            for (int j = 0; j < PPL; ++j) {
                sa[j] += ra[0][j] * ra[0][j];
                sb[j] += rb[0][j] * rb[0][j];
            }
        }
    }
#pragma unroll
    for (int j = 0; j < PPL; ++j) {
        ssq[0][wid][px + j] = sa[j];
        ssq[1][wid][px + j] = sb[j];
    }
    __syncthreads();
    float ia[PPL], ib[PPL];
#pragma unroll
    for (int j = 0; j < PPL; ++j) {                                            // every wave adds in wave order: one value
        const float ta = ((ssq[0][0][px + j] + ssq[0][1][px + j]) + ssq[0][2][px + j]) + ssq[0][3][px + j];
        const float tb = ((ssq[1][0][px + j] + ssq[1][1][px + j]) + ssq[1][2][px + j]) + ssq[1][3][px + j];
        ia[j] = 1.f / (sqrtf(ta) + 1e-10f);
        ib[j] = 1.f / (sqrtf(tb) + 1e-10f);
    }

    float acc[PPL];
#pragma unroll
    for (int j = 0; j < PPL; ++j) acc[j] = 0.f;
    if (CPW > 0) {
#pragma unroll
        for (int k = 0; k < CPW; ++k) {
            const float w = g.lin[wid + 4 * k];
#pragma unroll
            for (int j = 0; j < PPL; ++j) acc[j] += weighted_sq_diff(w, ra[k][j], ia[j], rb[k][j], ib[j]);
        }
    } else {
#pragma unroll 8
        for (int k = 0; k < nk; ++k) {
            const float w = g.lin[wid + 4 * k];
            load_px<PPL>(pa + (size_t)(4 * k) * HW, ok, ra[0]);
            load_px<PPL>(pb + (size_t)(4 * k) * HW, ok, rb[0]);
#pragma unroll
            for (int j = 0; j < PPL; ++j) acc[j] += weighted_sq_diff(w, ra[0][j], ia[j], rb[0][j], ib[j]);
        }
    }
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < PPL; ++j) s += acc[j];
    if (!ok) s = 0.f;                                                          // (already 0: 0 * 1e10; kept explicit)
    s = block_sum<256>(s, red);
    if (threadIdx.x == 0) g.part[(size_t)b * g.slots + g.slot0 + tile] = s * g.inv_hw;
}

__global__ __launch_bounds__(256) void lpips_finish_kernel(const float* __restrict__ part, float* __restrict__ out, int n) {
    __shared__ double red[256];
    const float* p = part + (size_t)blockIdx.x * n;
    double a = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) a += (double)p[i];
    red[threadIdx.x] = a;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[blockIdx.x] = (float)red[0];
}

// The tile of a tap: registers where C = 4 * {16, 32, 64}; float4 lanes on the large maps where they still fit (or
// where nothing is kept anyway).
struct Tile {
    int cpw, ppl;
};
inline Tile layer_tile(int C, long HW) {
    const bool v4 = HW % 4 == 0 && HW >= 1024;
    const bool reg = C == 64 || C == 128 || C == 256;
    if (reg) return Tile{C / 4, (v4 && C == 64) ? 4 : 1};
    return Tile{0, v4 ? 4 : 1};
}
inline long layer_tiles(int C, long HW) {
    const long tp = 64 * layer_tile(C, HW).ppl;
    return (HW + tp - 1) / tp;
}

constexpr int VGG_TAP_C[5] = {64, 128, 256, 512, 512};

inline unsigned blocks_of(long n) { return (unsigned)((n + 255) / 256); }

}  // namespace

extern "C" {

int vf_lpips_prep(const float* generated, const float* target, float* out, int B, int HW, void* stream) {
    if (B <= 0) return 0;
    if (HW <= 0) return (int)hipErrorInvalidValue;
    const long n = (long)B * 3 * HW;
    if (n > (1L << 36)) return (int)hipErrorInvalidValue;
    if (HW % 4 == 0)
        hipLaunchKernelGGL(lpips_prep_kernel<4>, dim3(blocks_of(n / 4)), dim3(256), 0, (hipStream_t)stream, generated,
                           target, out, n, HW);
    else
        hipLaunchKernelGGL(lpips_prep_kernel<1>, dim3(blocks_of(n)), dim3(256), 0, (hipStream_t)stream, generated, target,
                           out, n, HW);
    VF_RETURN_LAST_ERROR();
}

int vf_relu(float* x, long n, void* stream) {
    if (n <= 0) return 0;
    if (n > (1L << 38)) return (int)hipErrorInvalidValue;
    const long threads = (n >> 2) > 3 ? (n >> 2) : 4;                 // (the scalar tail takes up to 3 threads)
    hipLaunchKernelGGL(relu_kernel, dim3(blocks_of(threads)), dim3(256), 0, (hipStream_t)stream, x, n);
    VF_RETURN_LAST_ERROR();
}

int vf_relu_maxpool2(float* y, float* pooled, long planes, int H, int W, void* stream) {
    if (planes <= 0) return 0;
    if (H < 2 || W < 2 || (H & 1) || (W & 1)) return (int)hipErrorInvalidValue;
    const int nx = W % 4 == 0 ? 4 : 2;
    const long threads = planes * (H / 2) * (W / nx);
    if (threads > (1L << 38)) return (int)hipErrorInvalidValue;
    if (nx == 4)
        hipLaunchKernelGGL(relu_maxpool2_kernel<4>, dim3(blocks_of(threads)), dim3(256), 0, (hipStream_t)stream, y, pooled,
                           threads, H, W);
    else
        hipLaunchKernelGGL(relu_maxpool2_kernel<2>, dim3(blocks_of(threads)), dim3(256), 0, (hipStream_t)stream, y, pooled,
                           threads, H, W);
    VF_RETURN_LAST_ERROR();
}

int vf_lpips_layer_tiles(int C, int HW) {
    if (C < 1 || HW < 1) return 0;
    return (int)layer_tiles(C, HW);
}

long vf_lpips_workspace_floats(int B, int H, int W) {
    if (B <= 0 || H < 16 || W < 16 || H % 16 || W % 16) return 0;
    long slots = 0;
    for (int l = 0; l < 5; ++l) slots += layer_tiles(VGG_TAP_C[l], (long)(H >> l) * (W >> l));
    return (long)B * slots;
}

int vf_lpips_layer(const float* feat, const float* lin, float* workspace, int B, int C, int HW, int slot0, int slots,
                   void* stream) {
    if (B <= 0) return 0;
    if (C < 1 || HW < 1 || slot0 < 0) return (int)hipErrorInvalidValue;
    const Tile t = layer_tile(C, HW);
    const long tiles = layer_tiles(C, HW);
    if (slot0 + tiles > slots || (long)B * tiles > 0x7fffffffL || (long)2 * B * C * HW > (1L << 40))
        return (int)hipErrorInvalidValue;
    LayerArgs g{feat, lin, workspace, B, C, HW, (int)tiles, slot0, slots, (float)(1.0 / (double)HW)};
    const dim3 grid((unsigned)(B * tiles));
    hipStream_t st = (hipStream_t)stream;
#define VF_LAYER(CPW_, PPL_) \
    if (t.cpw == CPW_ && t.ppl == PPL_) hipLaunchKernelGGL((lpips_layer_kernel<CPW_, PPL_>), grid, dim3(256), 0, st, g);
    VF_LAYER(16, 4) VF_LAYER(16, 1) VF_LAYER(32, 1) VF_LAYER(64, 1) VF_LAYER(0, 4) VF_LAYER(0, 1)
#undef VF_LAYER
    VF_RETURN_LAST_ERROR();
}

int vf_lpips_finish(const float* workspace, float* out, int B, int slots, void* stream) {
    if (B <= 0) return 0;
    if (slots < 1) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(lpips_finish_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, workspace, out, slots);
    VF_RETURN_LAST_ERROR();
}

}  // extern "C"
