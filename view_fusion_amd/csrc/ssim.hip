// SSIM per image, the second eval metric of the reference (utils/metrics.py:11-12, experiment.py:349-380: SSIM picks
// best_model_ssim.pt).  Semantics of pytorch_msssim.ssim(X, Y, data_range=R, size_average=False) with its defaults:
// an 11-tap Gaussian window (sigma 1.5) applied separably and "valid" per channel to x, y, x^2, y^2, xy;
//   ssim = (2 mx my + C1) / (mx^2 + my^2 + C1) * (2 sxy + C2) / (sx^2 + sy^2 + C2),  C1 = (0.01 R)^2, C2 = (0.03 R)^2,
// no clamp, mean over all C (H-10) (W-10) map values.  Everything per pixel in fp32.
//
// One workgroup per (image, channel, 32 x 32 tile of the valid map): the 42 x 42 patches of both images go to LDS
// once (predicated scalar loads -- any H, W >= 11, no alignment), the pass along W writes the five filtered planes
// (42 x 32 each) to LDS, the pass along H takes four output rows per thread from 14 plane rows, and one partial sum per
// workgroup goes to the workspace.  A second launch, one workgroup per image, adds the partials in a fixed order (in
// double) and divides: no float atomics, bit-reproducible.  The five maps never leave the CU.
#include "common.h"

namespace {

constexpr int WIN = 11;               // taps
constexpr int TILE = 32;              // output tile side
constexpr int PATCH = TILE + WIN - 1; // 42: input rows / columns a tile needs
constexpr int ROWS_PER_THREAD = 4;    // 256 threads = 32 columns x 8 row groups of 4

struct Geom {
    int C, H, W;          // image
    int OH, OW;           // valid map (H-10, W-10)
    int tiles_x, tiles;   // tiles per row, tiles per (image, channel)
};

// One map value from the five filtered ones.  Contraction is off here: with 2 mx my and mx^2 + my^2 built from the same
// rounded products (and likewise the variances), an image against itself gives exactly 1, as the reference does.
__device__ __forceinline__ float ssim_pixel(float mx, float my, float exx, float eyy, float exy, float C1, float C2) {
#pragma clang fp contract(off)
    const float mxx = mx * mx, myy = my * my, mxy = mx * my;
    const float sxx = exx - mxx, syy = eyy - myy, sxy = exy - mxy;
    const float cs = (2.f * sxy + C2) / (sxx + syy + C2);
    return ((2.f * mxy + C1) / (mxx + myy + C1)) * cs;
}

// grid.x = B * C * tiles, in that order: the workspace index is the block index.
__global__ __launch_bounds__(256) void ssim_tile_kernel(const float* __restrict__ X, const float* __restrict__ Y,
                                                        const float* __restrict__ window, float* __restrict__ part,
                                                        Geom g, float C1, float C2) {
    __shared__ float sx[PATCH * PATCH], sy[PATCH * PATCH];
    __shared__ float plane[5][PATCH][TILE];          // mu_x, mu_y, E[x^2], E[y^2], E[xy] after the pass along W
    __shared__ float red[4];

    const unsigned bid = blockIdx.x;
    const int tile = (int)(bid % (unsigned)g.tiles);
    const size_t img = bid / (unsigned)g.tiles;      // = b * C + c
    const int y0 = (tile / g.tiles_x) * TILE, x0 = (tile % g.tiles_x) * TILE;
    const float* xp = X + img * (size_t)g.H * g.W;
    const float* yp = Y + img * (size_t)g.H * g.W;

    float w[WIN];
#pragma unroll
    for (int k = 0; k < WIN; ++k) w[k] = window[k];

    for (int i = threadIdx.x; i < PATCH * PATCH; i += 256) {
        const int r = y0 + i / PATCH, c = x0 + i % PATCH;
        const bool in = r < g.H && c < g.W;
        const size_t o = (size_t)r * g.W + c;
        sx[i] = in ? xp[o] : 0.f;
        sy[i] = in ? yp[o] : 0.f;
    }
    __syncthreads();

    for (int i = threadIdx.x; i < PATCH * TILE; i += 256) {
        const int r = i / TILE, c = i % TILE;
        const float* px = sx + r * PATCH + c;
        const float* py = sy + r * PATCH + c;
        float mx = 0.f, my = 0.f, xx = 0.f, yy = 0.f, xy = 0.f;
#pragma unroll
        for (int k = 0; k < WIN; ++k) {
            const float a = px[k], b = py[k];
            mx += w[k] * a;
            my += w[k] * b;
            xx += w[k] * (a * a);
            yy += w[k] * (b * b);
            xy += w[k] * (a * b);
        }
        plane[0][r][c] = mx;
        plane[1][r][c] = my;
        plane[2][r][c] = xx;
        plane[3][r][c] = yy;
        plane[4][r][c] = xy;
    }
    __syncthreads();

    const int c = threadIdx.x % TILE, r0 = (threadIdx.x / TILE) * ROWS_PER_THREAD;
    float acc[5][ROWS_PER_THREAD];
#pragma unroll
    for (int p = 0; p < 5; ++p)
#pragma unroll
        for (int j = 0; j < ROWS_PER_THREAD; ++j) acc[p][j] = 0.f;
#pragma unroll
    for (int i = 0; i < ROWS_PER_THREAD + WIN - 1; ++i) {          // plane row r0 + i feeds output row j with tap i - j
#pragma unroll
        for (int p = 0; p < 5; ++p) {
            const float v = plane[p][r0 + i][c];
#pragma unroll
            for (int j = 0; j < ROWS_PER_THREAD; ++j)
                if (i - j >= 0 && i - j < WIN) acc[p][j] += w[i - j] * v;
        }
    }
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < ROWS_PER_THREAD; ++j) {
        const float v = ssim_pixel(acc[0][j], acc[1][j], acc[2][j], acc[3][j], acc[4][j], C1, C2);
        if (y0 + r0 + j < g.OH && x0 + c < g.OW) s += v;           // pixels of the tile outside the valid map
    }
    s = block_sum<256>(s, red);
    if (threadIdx.x == 0) part[bid] = s;
}

// out[b] = sum of the image's n partials / count: every thread adds its strided share in index order, then a fixed tree.
__global__ __launch_bounds__(256) void ssim_finish_kernel(const float* __restrict__ part, float* __restrict__ out, int n,
                                                          double inv_count) {
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
    if (threadIdx.x == 0) out[blockIdx.x] = (float)(red[0] * inv_count);
}

inline bool geom(int B, int C, int H, int W, Geom* g, long long* blocks) {
    if (C < 1 || H < WIN || W < WIN) return false;
    g->C = C; g->H = H; g->W = W;
    g->OH = H - (WIN - 1); g->OW = W - (WIN - 1);
    g->tiles_x = (g->OW + TILE - 1) / TILE;
    const long long tiles = (long long)g->tiles_x * ((g->OH + TILE - 1) / TILE);
    if (tiles * C > 0x7fffffffLL) return false;
    g->tiles = (int)tiles;
    *blocks = (long long)(B > 0 ? B : 0) * C * tiles;
    return true;
}

}  // namespace

extern "C" {

long vf_ssim_workspace_floats(int B, int C, int H, int W) {
    Geom g;
    long long blocks = 0;
    if (!geom(B, C, H, W, &g, &blocks)) return 0;
    return (long)blocks;
}

int vf_ssim(const float* generated, const float* target, float* out, float* workspace, int B, int C, int H, int W,
            const float* window11, float data_range, void* stream) {
    if (B <= 0) return 0;
    Geom g;
    long long blocks = 0;
    if (!geom(B, C, H, W, &g, &blocks) || blocks > 0x7fffffffLL) return (int)hipErrorInvalidValue;
    const double c1 = 0.01 * (double)data_range, c2 = 0.03 * (double)data_range;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(ssim_tile_kernel, dim3((unsigned)blocks), dim3(256), 0, st, generated, target, window11,
                       workspace, g, (float)(c1 * c1), (float)(c2 * c2));
    hipLaunchKernelGGL(ssim_finish_kernel, dim3(B), dim3(256), 0, st, (const float*)workspace, out, C * g.tiles,
                       1.0 / ((double)C * g.OH * g.OW));
    VF_RETURN_LAST_ERROR();
}

}  // extern "C"
