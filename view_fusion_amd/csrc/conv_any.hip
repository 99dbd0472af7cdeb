// Direct convolution at ANY map size (runtime H, W): the route conv.hip takes for the shapes its specialised kernels
// (compile-time square power-of-two geometry, shift / mask pixel addressing) refuse -- non-square maps, sides that are
// not powers of two (5x5, 6x10, 12x20, 96x72 ...), and square maps outside [8, 128] (4x4, 256x256).
//
//   D[co][n] = sum_{tap,ci} Wp[tap][ci][co] * X[ci][n (+) tap]          n = flattened (view, row, column) pixel
//
// * v_mfma_f32_32x32x2_f32, A = packed weights (the vf_conv_pack_weights formats, unchanged: row = co), B = activations
//   (column = pixel), fp32 accumulate -- the same arithmetic type as the specialised kernels.
// * Tiles run over the flattened pixel index of all views: a map smaller than a tile shares the workgroup with the next
//   views' pixels, so 5x5 / 6x10 maps do not idle most of it.  Workgroup = 64 output channels x 64 * NPT pixels, 4 waves
//   (2 channel halves x 2 pixel halves).
// * Per K-chunk (8 input channels x 9 taps; 32 channels for 1x1) the weight slab is copied to LDS and the activation
//   tile is GATHERED to LDS as an im2col block [tap][channel][pixel]: zero padding, image borders, views past S and
//   channels past Cin are predicated in that gather (zero written), so the MFMA loop reads LDS only, without a branch.
//   The next chunk's global loads are issued into registers before the current chunk's MFMAs.
// * MODE as in conv.hip: 0 stride 1, 1 stride 2 (Downsample), 2 nearest-x2-upsampled input (Upsample), 4 sub-pixel
//   dgrad of the stride-2 conv (four accumulator sets = the four output parities; no zero is multiplied).
// * Split-K over input-channel chunks when the tile grid cannot fill the chip (the sampler, S <= 16): raw partials
//   into ws, summed in fixed order by a second launch that also applies the epilogue.  No float atomics anywhere.
// * Weight gradient: D[co][ci] per tap = sum_n dY[co][n] * X[ci][n (+) tap], 64 x 64 channel tiles, K = 16 pixels per
//   step, split over pixel ranges into slabs [slab][tap][CoutP][CinQ] that wgrad_reduce_body (wgrad_reduce.h) sums --
//   in a launch of its own or as a row of the deferred vf_wino44_reduce_multi launch.
#include "any_geom.h"
#include "wgrad_reduce.h"

namespace {

constexpr int ATCO = 64;                 // output channels per workgroup tile

struct AnyArgs {
    const float* x;
    const float* x2;       // 1x1: input channels [C1, Cin) (null: plain input)
    const float* w;        // packed [co tile][ci chunk][group][co 64][ci 8]
    const float* bias;
    const float* vbias;
    const float* res;
    float* y;
    float* y2;             // 1x1 dgrad of a concatenation: output channels [C1o, Cout) (null: one output)
    float* ws;             // [ksplit][S][Cout][H*W] partial sums
    int S, Cin, Cout, CinP, CoutP, C1, C1o;
    int H, W, SH, SW;      // tile grid (output; mode 4: dY) and source map
    int npix, ksplit;
};

// Offset within a source channel plane of the element that grid pixel (oy, ox) reads for packed tap g; -1 = zero.
template <int KS, int MODE>
__device__ __forceinline__ int tap_offset(int oy, int ox, int g, int H, int W, int SW) {
    if (KS == 1) return oy * SW + ox;
    const int kh = g / 3, kw = g % 3;
    if (MODE == 0) {
        const int iy = oy + kh - 1, ix = ox + kw - 1;
        return (iy >= 0 && iy < H && ix >= 0 && ix < W) ? iy * SW + ix : -1;
    } else if (MODE == 1) {
        const int iy = 2 * oy + kh - 1, ix = 2 * ox + kw - 1;
        return (iy >= 0 && iy < 2 * H && ix >= 0 && ix < 2 * W) ? iy * SW + ix : -1;
    } else if (MODE == 2) {
        const int uy = oy + kh - 1, ux = ox + kw - 1;
        return (uy >= 0 && uy < H && ux >= 0 && ux < W) ? (uy >> 1) * SW + (ux >> 1) : -1;
    } else {   // MODE 4: packed tap g holds w[2 - g/3][2 - g%3]; it reads dY one row down / one column right iff kh == 0 / kw == 0
        const int iy = oy + (kh == 2), ix = ox + (kw == 2);
        return (iy < H && ix < W) ? iy * SW + ix : -1;
    }
}

template <int KS, int MODE, int NPT>
__global__ __launch_bounds__(256) void conv_any_kernel(AnyArgs a) {
    constexpr int TP = 64 * NPT;              // pixels per tile
    constexpr int CK = KS == 3 ? 8 : 32;      // input channels per K-chunk
    constexpr int NG = KS == 3 ? 9 : 4;       // 8-channel groups per chunk: 9 taps (3x3) or 4 sub-chunks (1x1)
    constexpr int NTAP = KS * KS;
    constexpr int WROW = 12;                  // LDS floats per (group, co) row: 8 used, stride 12 -> b128 reads conflict-free
    constexpr int NW4 = NG * ATCO * 2;        // float4 per weight chunk
    constexpr int NWF = NW4 / 256;
    constexpr bool WT = (NW4 % 256) != 0;
    constexpr int NACC = MODE == 4 ? 4 : 1;
    __shared__ __attribute__((aligned(16))) float wl[NG * ATCO * WROW];
    __shared__ __attribute__((aligned(16))) float xl[NG * 8 * TP];

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int cw = wid & 1, pw = wid >> 1;
    const int li = lane & 31, lh = lane >> 5;

    const int ncot = a.CoutP / ATCO;
    const unsigned logical0 = xcd_remap(blockIdx.x, gridDim.x);
    const int split = logical0 % a.ksplit;
    const unsigned logical = logical0 / a.ksplit;
    const int cot = logical % ncot;
    const int tile = logical / ncot;
    const int co0 = cot * ATCO;
    const int nch = a.CinP / CK;
    const int kbeg = split * nch / a.ksplit, kend = (split + 1) * nch / a.ksplit;
    const int HW = a.H * a.W;
    const int SHW = a.SH * a.SW;

    // gather role: pixel column pp (+ 64 per NPT) of the tile, channels rs and rs + 4 of every 8-channel group
    const int pp = tid & 63, rs = tid >> 6;
    int sv[NPT], toff[NPT][NTAP];
#pragma unroll
    for (int nt = 0; nt < NPT; ++nt) {
        const int n = tile * TP + nt * 64 + pp;
        const int s = n / HW, rem = n - s * HW;
        const int oy = rem / a.W, ox = rem - oy * a.W;
        sv[nt] = n < a.npix ? s : -1;
#pragma unroll
        for (int t = 0; t < NTAP; ++t) toff[nt][t] = tap_offset<KS, MODE>(oy, ox, t, a.H, a.W, a.SW);
    }
    const int xC = a.x2 ? a.C1 : a.Cin, x2C = a.Cin - a.C1;
    float xr[NPT][NG][2];
    // weight staging in named registers (an indexed local array of float4 is placed in scratch in the NPT = 1 and 1x1
    // instances): w0..w3 = the full 256-wide passes, wt = the ragged tail
    static_assert(NWF >= 1 && NWF <= 4, "weight chunk = 1..4 full passes");
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 w0 = z4, w1 = z4, w2 = z4, w3 = z4, wt = z4;
    const size_t wtile = (size_t)nch * (NG * ATCO * 8);
    const float* wsrc = a.w + (size_t)cot * wtile;

    auto load_chunk = [&](int k) {
        const float* wk = wsrc + (size_t)k * (NG * ATCO * 8);
        const float4* wk4 = reinterpret_cast<const float4*>(wk) + tid;
        w0 = wk4[0];
        if constexpr (NWF > 1) w1 = wk4[256];
        if constexpr (NWF > 2) w2 = wk4[512];
        if constexpr (NWF > 3) w3 = wk4[768];
        if (WT && tid + NWF * 256 < NW4) wt = *reinterpret_cast<const float4*>(wk + 4 * (tid + NWF * 256));
#pragma unroll
        for (int nt = 0; nt < NPT; ++nt)
#pragma unroll
            for (int g = 0; g < NG; ++g)
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int c = k * CK + (KS == 1 ? 8 * g : 0) + rs + 4 * h;
                    const int off = toff[nt][KS == 3 ? g : 0];
                    const bool ok = sv[nt] >= 0 && off >= 0 && c < a.Cin;
                    const bool second = a.x2 && c >= a.C1;
                    const float* src = second ? a.x2 : a.x;
                    // out-of-range elements load element 0 (always valid) and are replaced by zero: no branch
                    const size_t idx = ok ? ((size_t)sv[nt] * (second ? x2C : xC) + (second ? c - a.C1 : c)) * SHW + off : 0;
                    const float v = src[idx];
                    xr[nt][g][h] = ok ? v : 0.f;
                }
    };
    auto store_chunk = [&]() {
        // element e = tid + 256 i -> LDS row e / 2; (256 i) / 2 = 128 i rows further for each pass
        float* const wd = wl + (tid >> 1) * WROW + 4 * (tid & 1);
        *reinterpret_cast<float4*>(wd) = w0;
        if constexpr (NWF > 1) *reinterpret_cast<float4*>(wd + 128 * WROW) = w1;
        if constexpr (NWF > 2) *reinterpret_cast<float4*>(wd + 256 * WROW) = w2;
        if constexpr (NWF > 3) *reinterpret_cast<float4*>(wd + 384 * WROW) = w3;
        if (WT && tid + NWF * 256 < NW4) {
            const int e = tid + NWF * 256;
            *reinterpret_cast<float4*>(wl + (e >> 1) * WROW + 4 * (e & 1)) = wt;
        }
#pragma unroll
        for (int nt = 0; nt < NPT; ++nt)
#pragma unroll
            for (int g = 0; g < NG; ++g)
#pragma unroll
                for (int h = 0; h < 2; ++h) xl[(g * 8 + rs + 4 * h) * TP + nt * 64 + pp] = xr[nt][g][h];
    };

    f32x16 acc[NACC][NPT];
#pragma unroll
    for (int j = 0; j < NACC; ++j)
#pragma unroll
        for (int nt = 0; nt < NPT; ++nt) acc[j][nt] = (f32x16){0};

    // k order inside an 8-channel group: MFMA step s pairs channel s (lane half 0) with channel 4+s (half 1), so a
    // lane's four A values are contiguous in the packed row -> one ds_read_b128 per group
    const float* wb = wl + (cw * 32 + li) * WROW + 4 * lh;
    const float* xb = xl + (4 * lh) * TP + pw * 32 * NPT + li;
    if (kbeg < kend) load_chunk(kbeg);
    for (int k = kbeg; k < kend; ++k) {
        __syncthreads();                               // previous chunk's LDS reads done
        store_chunk();
        __syncthreads();
        load_chunk(min(k + 1, kend - 1));              // unconditional (clamped): the loads stay countable
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            const float4 a4 = *reinterpret_cast<const float4*>(wb + g * ATCO * WROW);
            const float av[4] = {a4.x, a4.y, a4.z, a4.w};
            const int ja = MODE == 4 ? 2 * (g / 3 != 1) + (g % 3 != 1) : 0;    // output parity of tap g (mode 4)
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int nt = 0; nt < NPT; ++nt)
                    acc[ja][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[s], xb[(g * 8 + s) * TP + nt * 32], acc[ja][nt],
                                                                       0, 0, 0);
        }
    }

    // epilogue: lane = pixel, register = output channel
#pragma unroll
    for (int nt = 0; nt < NPT; ++nt) {
        const int n = tile * TP + pw * 32 * NPT + nt * 32 + li;
        if (n >= a.npix) continue;
        const int s = n / HW, pix = n - s * HW;
        const int cob = co0 + cw * 32 + 4 * lh;
        if constexpr (MODE == 4) {       // dx (S, Cout, 2H, 2W): grid pixel (i, j) -> the 2x2 block (2i+a, 2j+b)
            const int pi = pix / a.W, pj = pix - pi * a.W;
            const size_t W2 = 2 * (size_t)a.W, HW4 = 4 * (size_t)HW;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = cob + (r & 3) + 8 * (r >> 2);
                if (co >= a.Cout) continue;
                const size_t o = ((size_t)s * a.Cout + co) * HW4 + (size_t)(2 * pi) * W2 + 2 * pj;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const size_t oq = o + (q >> 1) * W2 + (q & 1);
                    a.y[oq] = acc[q][nt][r] + (a.res ? a.res[oq] : 0.f);
                }
            }
        } else {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = cob + (r & 3) + 8 * (r >> 2);
                if (co >= a.Cout) continue;
                if (a.ksplit > 1) {             // raw partial sums; the reduce launch adds the epilogue operands
                    a.ws[((size_t)split * a.S + s) * a.Cout * HW + (size_t)co * HW + pix] = acc[0][nt][r];
                    continue;
                }
                const bool second = a.y2 && co >= a.C1o;
                const size_t o = second ? ((size_t)s * (a.Cout - a.C1o) + (co - a.C1o)) * HW + pix
                                        : ((size_t)s * (a.y2 ? a.C1o : a.Cout) + co) * HW + pix;
                float add = 0.f;
                if (a.bias) add += a.bias[co];
                if (a.vbias) add += a.vbias[(size_t)s * a.Cout + co];
                if (a.res) add = a.res[o] + add;
                (second ? a.y2 : a.y)[o] = acc[0][nt][r] + add;
            }
        }
    }
}

// y = sum_split ws[split] (fixed order) + residual + bias[co] + view_bias[s][co]
__global__ __launch_bounds__(256) void conv_any_reduce_kernel(const float* __restrict__ ws, const float* __restrict__ bias,
                                                              const float* __restrict__ vbias, const float* __restrict__ res,
                                                              float* __restrict__ y, int ksplit, size_t n, int HW, int Cout) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const size_t sc = i / HW;
    float b = 0.f;
    if (bias) b += bias[sc % Cout];
    if (vbias) b += vbias[sc];
    const float r = res ? res[i] : 0.f;
    float v = 0.f;
    for (int k = 0; k < ksplit; ++k) v += ws[(size_t)k * n + i];
    y[i] = v + r + b;
}

// ----------------------------------------------------------------------------------------------
// weight gradient
struct AnyWgArgs {
    const float* x;
    const float* x2;
    const float* dy;
    float* ws;               // [slab][tap][CoutP][CinQ]
    int S, Cin, Cout, CoutP, CinQ, C1;
    int H, W, SH, SW, npix;
    int nsteps, steps_per_slice;
};

template <int KS, int MODE>
__global__ __launch_bounds__(256) void conv_any_wgrad_kernel(AnyWgArgs a) {
    constexpr int NT = KS * KS;
    constexpr int KP = 16, RS = KP + 1;           // pixels per step; odd LDS row stride
    __shared__ float dyl[64 * RS];
    __shared__ float xl[NT * 64 * RS];

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int cw = wid & 1, ciw = wid >> 1;
    const int li = lane & 31, lh = lane >> 5;
    const unsigned lgc = xcd_remap(blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z),
                                   gridDim.x * gridDim.y * gridDim.z);
    const int bx = lgc % gridDim.x, by = (lgc / gridDim.x) % gridDim.y, bz = lgc / (gridDim.x * gridDim.y);
    const int co0 = bx * 64, ci0 = by * 64;
    const int t_begin = bz * a.steps_per_slice;
    const int t_end = min(a.nsteps, t_begin + a.steps_per_slice);
    const int HW = a.H * a.W, SHW = a.SH * a.SW;
    const int xC = a.x2 ? a.C1 : a.Cin, x2C = a.Cin - a.C1;

    // gather role: pixel px of the step, channel rows row + 16 j
    const int px = tid & 15, row = tid >> 4;
    float dr[4], xr[4][NT];
    auto load_step = [&](int step) {
        const int n = step * KP + px;
        const int s = n / HW, rem = n - s * HW;
        const int oy = rem / a.W, ox = rem - oy * a.W;
        const bool okn = n < a.npix;
        int toff[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) toff[t] = tap_offset<KS, MODE>(oy, ox, t, a.H, a.W, a.SW);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int co = co0 + row + 16 * j;
            const bool okd = okn && co < a.Cout;
            const float d = a.dy[okd ? ((size_t)s * a.Cout + co) * HW + rem : 0];
            dr[j] = okd ? d : 0.f;
            const int ci = ci0 + row + 16 * j;
            const bool second = a.x2 && ci >= a.C1;
            const float* src = second ? a.x2 : a.x;
            const bool okc = okn && ci < a.Cin;
            const size_t plane = okc ? ((size_t)s * (second ? x2C : xC) + (second ? ci - a.C1 : ci)) * SHW : 0;
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const bool ok = okc && toff[t] >= 0;
                const float v = src[ok ? plane + toff[t] : 0];
                xr[j][t] = ok ? v : 0.f;
            }
        }
    };
    auto store_step = [&]() {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            dyl[(row + 16 * j) * RS + px] = dr[j];
#pragma unroll
            for (int t = 0; t < NT; ++t) xl[(t * 64 + row + 16 * j) * RS + px] = xr[j][t];
        }
    };

    f32x16 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = (f32x16){0};
    // MFMA step e pairs pixel 2e (lane half 0) with pixel 2e + 1 (half 1)
    const float* ab = dyl + (cw * 32 + li) * RS + lh;
    const float* bb = xl + (ciw * 32 + li) * RS + lh;
    if (t_begin < t_end) {
        load_step(t_begin);
        for (int step = t_begin; step < t_end; ++step) {
            __syncthreads();
            store_step();
            __syncthreads();
            load_step(min(step + 1, t_end - 1));
#pragma unroll
            for (int e = 0; e < KP / 2; ++e) {
                const float av = ab[2 * e];
#pragma unroll
                for (int t = 0; t < NT; ++t)
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bb[t * 64 * RS + 2 * e], acc[t], 0, 0, 0);
            }
        }
    }
    const int ci = ci0 + ciw * 32 + li;
    if (ci >= a.CinQ) return;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int co = co0 + cw * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
            a.ws[(((size_t)bz * NT + t) * a.CoutP + co) * a.CinQ + ci] = acc[t][r];
        }
}

__global__ __launch_bounds__(256) void conv_any_wgrad_reduce_kernel(const float* __restrict__ ws, float* __restrict__ dw,
                                                                    int nslab, int NT, int Cout, int Cin, int CoutP,
                                                                    int CinQ) {
    wgrad_reduce_body(ws, dw, nslab, NT, Cout, Cin, CoutP, CinQ, (int)blockIdx.x);
}

inline int rup(int v, int m) { return (v + m - 1) / m * m; }

// Square power-of-two maps in [8, 128] whose (mode) the specialised kernels lack (a 4 -> 8 Upsample, a stride-2 conv
// to 128 x 128) come here too.  vf_conv_fwd_ws_floats / vf_conv_wgrad_ws_floats have no mode argument and price such a
// map with the specialised formula, so on those maps the plans below split by that very formula: the size the caller
// allocates is then exactly what the general kernel uses.
inline bool square_pow2_map(int H, int W) {
    return H == W && W >= 8 && W <= 128 && (W & (W - 1)) == 0;
}

// tile size (NPT) and split-K factor of a forward launch: 128-pixel tiles where they fill the chip three times over,
// 64-pixel tiles otherwise; split K only while the grid is below one workgroup per CU (at most 16 partials)
struct FwdPlan {
    int npt, nblk, ks;
};
inline FwdPlan fwd_plan(int S, int Cin, int Cout, int H, int W, int KS) {
    const long npix = (long)S * H * W;
    const int nco = rup(Cout, ATCO) / ATCO;
    FwdPlan p;
    p.npt = (npix + 127) / 128 * nco >= 3 * 256 ? 2 : 1;
    p.nblk = (int)((npix + 64 * p.npt - 1) / (64 * p.npt)) * nco;
    const int ck = KS == 3 ? 8 : 32;
    const int nch = rup(Cin, ck) / ck;
    // (square power-of-two map: the specialised formula's grid measure, 128-pixel tiles)
    const int nbk = square_pow2_map(H, W) ? (int)((npix + 127) / 128) * nco : p.nblk;
    int k = 1;
    if (nbk < 256 && nch >= 2) {
        k = 256 / nbk;
        if (k > 16) k = 16;
        if (k > nch) k = nch;
        if (k < 1) k = 1;
    }
    p.ks = k;
    return p;
}

template <int KS, int MODE>
void launch_any(const AnyArgs& a, int npt, int nblk, hipStream_t st) {
    if (npt == 2) hipLaunchKernelGGL((conv_any_kernel<KS, MODE, 2>), dim3(nblk * a.ksplit), dim3(256), 0, st, a);
    else hipLaunchKernelGGL((conv_any_kernel<KS, MODE, 1>), dim3(nblk * a.ksplit), dim3(256), 0, st, a);
}

// pixel-range slices of a weight-gradient launch: ~512 workgroups over the (co, ci) tiles; on a square power-of-two
// map the specialised formula (ceil over 32-channel ci tiles, at most one slice per 128 pixels)
inline int wgrad_slices(int nco, int Cin, long npix, int nsteps, bool sq, size_t ws_floats, size_t slab) {
    int z;
    if (sq) {
        const int nci32 = (Cin + 31) / 32;
        z = (512 + nco * nci32 - 1) / (nco * nci32);
        const long ntiles = (npix + 127) / 128;
        if (z > ntiles) z = (int)ntiles;
    } else {
        z = 512 / (nco * ((Cin + 63) / 64));
    }
    if (z < 1) z = 1;
    if (z > nsteps) z = nsteps;
    if ((size_t)z > ws_floats / slab) z = (int)(ws_floats / slab);
    return z;
}

}  // namespace

long vfi_conv_any_fwd_ws_floats(int S, int Cin, int Cout, int H, int W, int KS) {
    if (S <= 0 || H <= 0 || W <= 0) return 0;
    const FwdPlan p = fwd_plan(S, Cin, Cout, H, W, KS);
    return p.ks > 1 ? (long)p.ks * S * Cout * H * W : 0;
}

// The launch plan of vfi_conv_any_fwd, host only: out = {npt, nblk, ks after the workspace clamp}.  split_out: the output is
// split over two tensors (the reduce writes one destination); mode 4 ignores the workspace.
void vfi_conv_any_fwd_plan(int S, int Cin, int Cout, int H, int W, int KS, int mode, bool split_out, bool has_ws,
                           long ws_floats, int out[3]) {
    const FwdPlan p = fwd_plan(S, Cin, Cout, H, W, KS);
    const size_t out_floats = (size_t)S * Cout * H * W;
    int ks = p.ks;
    if (!has_ws || split_out || mode == 4) ks = 1;
    while (ks > 1 && (size_t)ks * out_floats > (size_t)ws_floats) --ks;
    out[0] = p.npt; out[1] = p.nblk; out[2] = ks;
}

int vfi_conv_any_fwd(const float* x, const float* x2, int C1, const float* w_packed, const float* bias,
                     const float* view_bias, const float* residual, float* y, float* y2, int C1o, float* ws, long ws_floats,
                     int S, int Cin, int Cout, int H, int W, int KS, int mode, hipStream_t st) {
    if (S <= 0) return 0;
    if (H <= 0 || W <= 0 || (KS != 1 && KS != 3) || (KS == 1 && mode != 0)) return (int)hipErrorInvalidValue;
    if (mode != 0 && mode != 1 && mode != 2 && mode != 4) return (int)hipErrorInvalidValue;
    if (mode == 2 && ((H & 1) || (W & 1))) return (int)hipErrorInvalidValue;      // upsampled source: H/2 x W/2
    if ((long)S * H * W > (1L << 30)) return (int)hipErrorInvalidValue;
    AnyArgs a;
    a.x = x; a.x2 = x2; a.w = w_packed; a.bias = bias; a.vbias = view_bias; a.res = residual; a.y = y; a.y2 = y2;
    a.S = S; a.Cin = Cin; a.Cout = Cout; a.C1 = C1; a.C1o = C1o;
    a.CinP = rup(Cin, KS == 3 ? 8 : 32);
    a.CoutP = rup(Cout, ATCO);
    a.H = H; a.W = W;
    a.SH = mode == 1 ? 2 * H : (mode == 2 ? H / 2 : H);
    a.SW = mode == 1 ? 2 * W : (mode == 2 ? W / 2 : W);
    a.npix = S * H * W;
    const size_t out_floats = (size_t)S * Cout * H * W;
    int plan[3];
    vfi_conv_any_fwd_plan(S, Cin, Cout, H, W, KS, mode, y2 != nullptr, ws != nullptr, ws_floats, plan);
    const FwdPlan p{plan[0], plan[1], plan[2]};
    const int ks = p.ks;
    a.ksplit = ks;
    a.ws = ws;
#define VF_ANY(KS_, M_) \
    if (KS == KS_ && mode == M_) launch_any<KS_, M_>(a, p.npt, p.nblk, st);
    VF_ANY(3, 0) VF_ANY(3, 1) VF_ANY(3, 2) VF_ANY(3, 4) VF_ANY(1, 0)
#undef VF_ANY
    if (ks > 1)
        hipLaunchKernelGGL(conv_any_reduce_kernel, dim3((unsigned)((out_floats + 255) / 256)), dim3(256), 0, st, ws, bias,
                           view_bias, residual, y, ks, out_floats, H * W, Cout);
    VF_RETURN_LAST_ERROR();
}

long vfi_conv_any_wgrad_ws_floats(int S, int Cin, int Cout, int H, int W, int KS) {
    if (S <= 0 || H <= 0 || W <= 0) return 0;
    const int CoutP = rup(Cout, 64), CinQ = rup(Cin, 32);
    const size_t slab = (size_t)KS * KS * CoutP * CinQ;
    const int nsteps = (int)(((long)S * H * W + 15) / 16);
    const int z = wgrad_slices(CoutP / 64, Cin, (long)S * H * W, nsteps, square_pow2_map(H, W), (size_t)1 << 62, slab);
    return (long)z * (long)slab;
}

int vfi_conv_any_wgrad(const float* x, const float* x2, int C1, const float* dy, float* dw, float* ws, long ws_floats, int S,
                       int Cin, int Cout, int H, int W, int KS, int mode, hipStream_t st, long long* desc9, int* nblocks) {
    if (desc9) *nblocks = 0;
    if (S <= 0) return 0;
    if (H <= 0 || W <= 0 || (KS != 1 && KS != 3) || (KS == 1 && mode != 0) || mode < 0 || mode > 2)
        return (int)hipErrorInvalidValue;
    if (mode == 2 && ((H & 1) || (W & 1))) return (int)hipErrorInvalidValue;
    if ((long)S * H * W > (1L << 30)) return (int)hipErrorInvalidValue;
    AnyWgArgs a;
    a.x = x; a.x2 = x2; a.dy = dy; a.ws = ws; a.S = S; a.Cin = Cin; a.Cout = Cout; a.C1 = C1;
    a.CoutP = rup(Cout, 64); a.CinQ = rup(Cin, 32);
    a.H = H; a.W = W;
    a.SH = mode == 1 ? 2 * H : (mode == 2 ? H / 2 : H);
    a.SW = mode == 1 ? 2 * W : (mode == 2 ? W / 2 : W);
    a.npix = S * H * W;
    a.nsteps = (a.npix + 15) / 16;
    const int NT = KS * KS;
    const int nco = a.CoutP / 64, nci = (Cin + 63) / 64;
    const size_t slab = (size_t)NT * a.CoutP * a.CinQ;
    int z = wgrad_slices(nco, Cin, a.npix, a.nsteps, square_pow2_map(H, W), (size_t)(ws_floats > 0 ? ws_floats : 0), slab);
    if (z < 1) return (int)hipErrorInvalidValue;
    a.steps_per_slice = (a.nsteps + z - 1) / z;
    z = (a.nsteps + a.steps_per_slice - 1) / a.steps_per_slice;
    const dim3 grid(nco, nci, z);
    if (KS == 3 && mode == 0) hipLaunchKernelGGL((conv_any_wgrad_kernel<3, 0>), grid, dim3(256), 0, st, a);
    else if (KS == 3 && mode == 1) hipLaunchKernelGGL((conv_any_wgrad_kernel<3, 1>), grid, dim3(256), 0, st, a);
    else if (KS == 3) hipLaunchKernelGGL((conv_any_wgrad_kernel<3, 2>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((conv_any_wgrad_kernel<1, 0>), grid, dim3(256), 0, st, a);
    if (desc9) {                                      // the slab sum joins the caller's deferred multi launch
        *nblocks = wgrad_reduce_row(desc9, ws, dw, z, NT, Cout, Cin, a.CoutP, a.CinQ);
        VF_RETURN_LAST_ERROR();
    }
    const int total = NT * Cout * Cin;
    hipLaunchKernelGGL(conv_any_wgrad_reduce_kernel, dim3((total + 63) / 64), dim3(256), 0, st, ws, dw, z, NT, Cout, Cin,
                       a.CoutP, a.CinQ);
    VF_RETURN_LAST_ERROR();
}
