// Streaming single-head spatial self-attention, any L (reference model/unet.py:248-277, the einsum + softmax core):
//   O[c][i] = sum_j V[c][j] * softmax_j(alpha * sum_c' Q[c'][i] K[c'][j]),  alpha = 1/sqrt(C),  qkv [S][3C][L]
// The L x L score matrix is never written: keys and values are streamed in blocks with an online softmax, and the
// backward recomputes the probabilities from the forward's per-query softmax statistics (FlashAttention-2).  Memory is
// O(L) per view (rowstat 2 x S x L floats, delta S x L); the materialised path (attention.py, L <= 4096) needs
// S x L x L twice.
//
// The statistics are kept as the pair (c2 max, 1 / sum), c2 = alpha log2 e, not as one log-sum-exp: the backward then
// forms p = exp2(c2 s - c2 max) / sum from the same score s (same MFMA order, accumulator 0) and the same two numbers
// as the forward.  A single lse = alpha max + ln sum carried as the initial accumulator of S rounds every partial sum at
// the magnitude of the largest score: with scores of +-350 (C = 64: raw 2800, ulp 2.4e-4) over C / 2 MFMA steps that
// is about 5e-5 in p, which missed the stated d(qkv) tolerance on peaked inputs.
//
// Orientation (all kernels), v_mfma_f32_32x32x2_f32, accumulator register r of lane (li = lane & 31, lh = lane >> 5)
// = row (r & 3) + 8 (r >> 2) + 4 lh, column li:
//   forward, dQ   S^T = K^T Q: a lane owns ONE query column, its keys sit in the registers, so the online softmax
//                 (running max and sum, the rescale of the O accumulator) is per lane; O = V P^T takes P in the
//                 registers' row order with V fetched in that order (one 4-key run per four MFMAs), as attention.hip.
//   dK / dV       S = Q^T K: the key is on the lane ("key on the lane"), the queries sit in the registers; the
//                 row constant -delta is the initial accumulator of dP, so dS = p o dP' needs no subtraction.
//
// Tiling: a workgroup is 4 waves.  Forward and dQ: one view x 32 queries, streaming 128 keys per iteration, one 32-key
// sub-block per wave for the score product (sum over all C); the probabilities (dS for dQ) go through LDS, and the
// product that sums over keys is split over channel tiles of 32: wave w owns tiles w, w + 4, ... (NT <= 4 tiles,
// C <= 512), so the O / dQ accumulator of a large C is spread over the four waves.  dK / dV: one view x 32 keys,
// streaming 128 queries per iteration, one 32-query sub-block per wave; P and dS go through LDS and each wave keeps
// dK and dV of its channel tiles.  C is padded to the MFMA shapes by predicated loads (any C <= 512, odd C too) and L
// by masking (keys past L score -inf, queries past L are never stored), so any L >= 1 runs.  Operands are read
// straight from global memory (the workgroups of one view are kept on one XCD, whose L2 holds the view's K, V and Q).
//
// LDS: the exchange tiles [2 buffers][4 sub-blocks][32][36 floats] (36 864 B; the dK / dV kernel keeps P and dS,
// 73 728 B), double-buffered so that one barrier per iteration suffices, plus 1 KiB of softmax statistics.
//
// Determinism: every sum has a fixed order.  The forward combines the four sub-blocks' statistics in wave order, dK
// and dV are owned by one workgroup each, and dQ -- a sum over all key blocks -- is recomputed by a kernel of its own
// over view x query block (14 L^2 C executed FLOPs per view in the backward instead of 10).  The alternative, an
// ordered hand-off of dQ tiles between the key-block workgroups of a view, needs all of a view's L / 32 workgroups
// resident together (512 at L = 16384, more than the chip holds with S > 1) and bounded spins; the recompute needs
// neither, has no float atomics, and replays bit-equal.
//   attn_stream_fwd_kernel<NT>    O (and rowstat = (c2 max, 1 / sum) when rowstat != NULL)
//   attn_stream_delta_kernel      delta[i] = sum_c dO[c][i] O[c][i]
//   attn_stream_dkv_kernel<NT>    dK, dV -> the k and v thirds of dqkv
//   attn_stream_dq_kernel<NT>     dQ -> the q third of dqkv
// No key-split forward for few views: not built (DESIGN 8 H has the measured small-S cost).
#include "common.h"

namespace {

constexpr int SQ = 32, SKB = 128, SPAD = 36;    // queries (keys) per workgroup, keys (queries) per iteration, LDS row

__device__ __forceinline__ int crow(int r, int lh) { return (r & 3) + 8 * (r >> 2) + 4 * lh; }

// acc += sum over channels c of a[c L] (A operand, row on the lane) * b[c L] (B operand, column on the lane); lane
// half lh takes the odd channels.  a / b point at a valid element even when the row / column is masked (aok / bok
// false): the loads stay in bounds and their values are replaced by 0.
__device__ __forceinline__ f32x16 chan_mfma(const float* a, bool aok, const float* b, bool bok, int C, size_t L,
                                            int lh, f32x16 acc) {
    int c0 = 0;
    for (; c0 + 16 <= C; c0 += 16) {
        float av[8], bv[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const size_t off = (size_t)(c0 + 2 * j + lh) * L;
            av[j] = aok ? a[off] : 0.f;
            bv[j] = bok ? b[off] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[j], bv[j], acc, 0, 0, 0);
    }
    for (; c0 < C; c0 += 2) {
        const int c = c0 + lh;
        const bool cok = c < C;
        const size_t off = (size_t)(cok ? c : 0) * L;
        const float av = aok && cok ? a[off] : 0.f, bv = bok && cok ? b[off] : 0.f;
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc, 0, 0, 0);
    }
    return acc;
}

// row[kk .. kk + 3] with entries at or past L (and a masked row) read as 0; kk % 4 == 0.  vec: L % 4 == 0 and the
// tensor 16-byte aligned, so an in-range run is one aligned 16-byte load.
__device__ __forceinline__ float4 ld4(const float* row, bool ok, int kk, int L, bool vec) {
    if (vec && kk < L) {
        const float4 v = *reinterpret_cast<const float4*>(row + kk);
        return ok ? v : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    float e[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const float x = row[min(kk + t, L - 1)];
        e[t] = ok && kk + t < L ? x : 0.f;
    }
    return make_float4(e[0], e[1], e[2], e[3]);
}

// o[t] += A B over one 128-wide block of the key (or query) index whose B side is in LDS: A[c][k] = src[c][kbase + k]
// for the wave's channel tiles (ct = w + 4 t, rows c = 32 ct + li), B[k][col li] = x[u][li][k] (times f[u] if SCALE)
template <int NT, bool SCALE>
__device__ __forceinline__ void chan_tiles_mfma(f32x16 (&o)[NT], const float* src, int C, int L, int kbase, bool vec,
                                                const float (*x)[SQ][SPAD], const float (&f)[4], int w, int li,
                                                int lh) {
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int ct = w + 4 * t;
        if (32 * ct >= C) break;                                  // wave-uniform
        const int c = 32 * ct + li;
        const bool cok = c < C;
        const float* row = src + (size_t)(cok ? c : 0) * L;
        f32x16 acc = o[t];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const float fu = SCALE ? f[u] : 1.f;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const float4 av = ld4(row, cok, kbase + 32 * u + 8 * g + 4 * lh, L, vec);
                float4 bx = *reinterpret_cast<const float4*>(&x[u][li][8 * g + 4 * lh]);
                if (SCALE) {
                    bx.x *= fu; bx.y *= fu; bx.z *= fu; bx.w *= fu;
                }
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, bx.x, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, bx.y, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, bx.z, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, bx.w, acc, 0, 0, 0);
            }
        }
        o[t] = acc;
    }
}

// one lane's 16 accumulator values -> x[li][...]: register 4g + e lands at column 8g + 4lh + e, the order
// chan_tiles_mfma reads back
__device__ __forceinline__ void put_tile(float (*x)[SPAD], const f32x16& v, int li, int lh) {
#pragma unroll
    for (int g = 0; g < 4; ++g)
        *reinterpret_cast<float4*>(&x[li][8 * g + 4 * lh]) =
            make_float4(v[4 * g], v[4 * g + 1], v[4 * g + 2], v[4 * g + 3]);
}

// (block of 32 along the lane index, view): consecutive logical ids share an XCD, so a view's blocks share one L2
__device__ __forceinline__ void block_ids(int& blk, int& b) {
    const unsigned nb = gridDim.x * gridDim.y;
    const unsigned id = xcd_remap(blockIdx.x + gridDim.x * blockIdx.y, nb);
    blk = id % gridDim.x;
    b = id / gridDim.x;
}

template <int NT>
__global__ __launch_bounds__(256) void attn_stream_fwd_kernel(const float* __restrict__ qkv, float* __restrict__ out,
                                                              float* __restrict__ rowstat, int C, int L,
                                                              float alpha, int vec) {
    __shared__ __attribute__((aligned(16))) float pl[2][4][SQ][SPAD];   // P [buf][key sub-block][query][key]
    __shared__ float stat[2][2][4][SQ];                                  // [buf][max | sum][key sub-block][query]
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, li = lane & 31, lh = lane >> 5;
    int qblk, b;
    block_ids(qblk, b);
    const size_t CL = (size_t)C * L;
    const float* qp = qkv + (size_t)b * 3 * CL;
    const float* kp = qp + CL;
    const float* vp = kp + CL;
    const int qi = qblk * SQ + li;
    const bool qok = qi < L;
    const float c2 = alpha * 1.44269504088896341f;

    f32x16 o[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) o[t] = (f32x16){0};
    float m = -INFINITY, l = 0.f;                        // running max (raw score) and sum of this lane's query
    const int nkb = (L + SKB - 1) / SKB;
    for (int kb = 0, buf = 0; kb < nkb; ++kb, buf ^= 1) {
        const int k0 = kb * SKB + 32 * w;                // this wave's key sub-block
        const int kj = k0 + li;
        f32x16 s = chan_mfma(kp + (kj < L ? kj : 0), kj < L, qp + (qok ? qi : 0), qok, C, L, lh, (f32x16){0});
        float mw = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            if (k0 + crow(r, lh) >= L) s[r] = -INFINITY;
            mw = fmaxf(mw, s[r]);
        }
        mw = fmaxf(mw, __shfl_xor(mw, 32, 64));
        const float mwc = mw == -INFINITY ? 0.f : mw * c2;   // a sub-block wholly past L: p = 0, not NaN
        float lw = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float p = __builtin_amdgcn_exp2f(fmaf(s[r], c2, -mwc));
            s[r] = p;
            lw += p;
        }
        lw += __shfl_xor(lw, 32, 64);
        put_tile(pl[buf][w], s, li, lh);
        if (lh == 0) {
            stat[buf][0][w][li] = mw;
            stat[buf][1][w][li] = lw;
        }
        __syncthreads();
        // combine the four sub-blocks in wave order (every wave computes the same numbers)
        float mu[4], mn = m;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            mu[u] = stat[buf][0][u][li];
            mn = fmaxf(mn, mu[u]);
        }
        const float fo = __builtin_amdgcn_exp2f((m - mn) * c2);     // m = -inf on the first block: 0
        float f[4];
        l *= fo;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            f[u] = __builtin_amdgcn_exp2f((mu[u] - mn) * c2);
            l = fmaf(f[u], stat[buf][1][u][li], l);
        }
        m = mn;
#pragma unroll
        for (int t = 0; t < NT; ++t) o[t] *= fo;
        chan_tiles_mfma<NT, true>(o, vp, C, L, kb * SKB, vec != 0, pl[buf], f, w, li, lh);   // O += V P^T
    }
    if (!qok) return;
    const float inv = 1.0f / l;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int ct = w + 4 * t;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int c = 32 * ct + crow(r, lh);
            if (c < C) out[((size_t)b * C + c) * L + qi] = o[t][r] * inv;
        }
    }
    if (rowstat && w == 0 && lh == 0) {
        rowstat[(size_t)(2 * b) * L + qi] = m * c2;
        rowstat[(size_t)(2 * b + 1) * L + qi] = inv;
    }
}

__global__ __launch_bounds__(256) void attn_stream_delta_kernel(const float* __restrict__ out,
                                                                const float* __restrict__ dO,
                                                                float* __restrict__ delta, int C, int L) {
    const int i = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (i >= L) return;
    const size_t base = (size_t)b * C * L + i;
    float d = 0.f;
    for (int c = 0; c < C; ++c) d = fmaf(dO[base + (size_t)c * L], out[base + (size_t)c * L], d);
    delta[(size_t)b * L + i] = d;
}

template <int NT>
__global__ __launch_bounds__(256) void attn_stream_dkv_kernel(const float* __restrict__ qkv,
                                                              const float* __restrict__ dO,
                                                              const float* __restrict__ rowstat,
                                                              const float* __restrict__ delta,
                                                              float* __restrict__ dqkv, int C, int L, float alpha,
                                                              int vec) {
    __shared__ __attribute__((aligned(16))) float pl[2][2][4][SQ][SPAD];   // [buf][P | dS][query sub-block][key][q]
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, li = lane & 31, lh = lane >> 5;
    int kblk, b;
    block_ids(kblk, b);
    const size_t CL = (size_t)C * L;
    const float* qp = qkv + (size_t)b * 3 * CL;
    const float* kp = qp + CL;
    const float* vp = kp + CL;
    const float* gp = dO + (size_t)b * CL;
    const float* mp = rowstat + (size_t)(2 * b) * L;     // c2 max
    const float* ip = mp + L;                            // 1 / sum
    const float* dp = delta + (size_t)b * L;
    const int kj = kblk * SQ + li;
    const bool kok = kj < L;
    const float c2 = alpha * 1.44269504088896341f;
    const float one[4] = {1.f, 1.f, 1.f, 1.f};

    f32x16 dk[NT], dv[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) dk[t] = dv[t] = (f32x16){0};
    const int nqb = (L + SKB - 1) / SKB;
    for (int qb = 0, buf = 0; qb < nqb; ++qb, buf ^= 1) {
        const int q0 = qb * SKB + 32 * w;                // this wave's query sub-block
        const int qa = q0 + li;                          // its A-operand row
        f32x16 s, dp_;
#pragma unroll
        for (int r = 0; r < 16; ++r) {                   // row constant of query q0 + crow(r)
            const int q = q0 + crow(r, lh);
            dp_[r] = q < L ? -dp[q < L ? q : L - 1] : 0.f;
        }
        s = chan_mfma(qp + (qa < L ? qa : 0), qa < L, kp + (kok ? kj : 0), kok, C, L, lh, (f32x16){0});
        dp_ = chan_mfma(gp + (qa < L ? qa : 0), qa < L, vp + (kok ? kj : 0), kok, C, L, lh, dp_);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int q = q0 + crow(r, lh);
            const int qc = q < L ? q : L - 1;
            const float p = kok && q < L ? __builtin_amdgcn_exp2f(fmaf(s[r], c2, -mp[qc])) * ip[qc] : 0.f;
            s[r] = p;
            dp_[r] *= p;                                 // dS = P o (dP - delta)
        }
        put_tile(pl[buf][0][w], s, li, lh);
        put_tile(pl[buf][1][w], dp_, li, lh);
        __syncthreads();
        chan_tiles_mfma<NT, false>(dv, gp, C, L, qb * SKB, vec != 0, pl[buf][0], one, w, li, lh);   // dV += dO P
        chan_tiles_mfma<NT, false>(dk, qp, C, L, qb * SKB, vec != 0, pl[buf][1], one, w, li, lh);   // dK += Q dS
    }
    if (!kok) return;
    float* dkp = dqkv + (size_t)b * 3 * CL + CL;
    float* dvp = dkp + CL;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int ct = w + 4 * t;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int c = 32 * ct + crow(r, lh);
            if (c < C) {
                dkp[(size_t)c * L + kj] = dk[t][r] * alpha;
                dvp[(size_t)c * L + kj] = dv[t][r];
            }
        }
    }
}

template <int NT>
__global__ __launch_bounds__(256) void attn_stream_dq_kernel(const float* __restrict__ qkv,
                                                             const float* __restrict__ dO,
                                                             const float* __restrict__ rowstat,
                                                             const float* __restrict__ delta,
                                                             float* __restrict__ dqkv, int C, int L, float alpha,
                                                             int vec) {
    __shared__ __attribute__((aligned(16))) float pl[2][4][SQ][SPAD];     // dS^T [buf][key sub-block][query][key]
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, li = lane & 31, lh = lane >> 5;
    int qblk, b;
    block_ids(qblk, b);
    const size_t CL = (size_t)C * L;
    const float* qp = qkv + (size_t)b * 3 * CL;
    const float* kp = qp + CL;
    const float* vp = kp + CL;
    const float* gp = dO + (size_t)b * CL;
    const int qi = qblk * SQ + li;
    const bool qok = qi < L;
    const int qc = qok ? qi : 0;
    const float c2 = alpha * 1.44269504088896341f;
    const float mc = qok ? rowstat[(size_t)(2 * b) * L + qc] : 0.f;          // c2 max
    const float il = qok ? rowstat[(size_t)(2 * b + 1) * L + qc] : 0.f;      // 1 / sum
    const float d0 = qok ? -delta[(size_t)b * L + qc] : 0.f;
    const float one[4] = {1.f, 1.f, 1.f, 1.f};

    f32x16 dq[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) dq[t] = (f32x16){0};
    const int nkb = (L + SKB - 1) / SKB;
    for (int kb = 0, buf = 0; kb < nkb; ++kb, buf ^= 1) {
        const int k0 = kb * SKB + 32 * w;
        const int kj = k0 + li;
        f32x16 s, dp_;
#pragma unroll
        for (int r = 0; r < 16; ++r) dp_[r] = d0;
        s = chan_mfma(kp + (kj < L ? kj : 0), kj < L, qp + qc, qok, C, L, lh, (f32x16){0});
        dp_ = chan_mfma(vp + (kj < L ? kj : 0), kj < L, gp + qc, qok, C, L, lh, dp_);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float p = qok && k0 + crow(r, lh) < L ? __builtin_amdgcn_exp2f(fmaf(s[r], c2, -mc)) * il : 0.f;
            dp_[r] *= p;
        }
        put_tile(pl[buf][w], dp_, li, lh);
        __syncthreads();
        chan_tiles_mfma<NT, false>(dq, kp, C, L, kb * SKB, vec != 0, pl[buf], one, w, li, lh);   // dQ += K dS^T
    }
    if (!qok) return;
    float* dqp = dqkv + (size_t)b * 3 * CL;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int ct = w + 4 * t;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int c = 32 * ct + crow(r, lh);
            if (c < C) dqp[(size_t)c * L + qi] = dq[t][r] * alpha;
        }
    }
}

// channel tiles per wave: ceil(ceil(C / 32) / 4), 1..4 for C <= 512
int tiles_per_wave(int C) { return ((C + 31) / 32 + 3) / 4; }

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// The plan of one vf_attn_stream_fwd / vf_attn_stream_bwd pair: every decision the two launchers take on the host, made in
// ONE place (attn_stream_plan below) that both execute and vf_attn_stream_plan reports.
enum { AS_EMPTY = 0, AS_RUNS = 1, AS_REFUSED = 2 };

struct AttnStreamPlan {
    int state;            // AS_EMPTY: S <= 0 or L <= 0, nothing runs; AS_REFUSED: C <= 0 or C > 512
    int nt;               // channel tiles per wave: the <NT> of the forward, dK / dV and dQ kernels
    int vec_fwd, vec_bwd; // ld4 takes 16-byte loads (forward: of V; backward: of dO, Q and K)
    int gx, gy;           // grid of the forward, dK / dV and dQ kernels: (32-wide blocks of L, views)
    int delta_gx;         // grid x of attn_stream_delta_kernel (256 queries per workgroup; y = views)
    int nblocks;          // 128-wide blocks each workgroup streams
    long rowstat_floats, delta_floats;
};

AttnStreamPlan attn_stream_plan(const void* qkv, const void* dO, int S, int C, int L) {
    AttnStreamPlan p = {AS_EMPTY, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (S <= 0 || L <= 0) return p;
    if (C <= 0 || C > 512) {
        p.state = AS_REFUSED;
        return p;
    }
    p.state = AS_RUNS;
    p.nt = tiles_per_wave(C);
    p.vec_fwd = L % 4 == 0 && aligned16(qkv);
    p.vec_bwd = p.vec_fwd && aligned16(dO);
    p.gx = (L + SQ - 1) / SQ; p.gy = S;
    p.delta_gx = (L + 255) / 256;
    p.nblocks = (L + SKB - 1) / SKB;
    p.rowstat_floats = 2L * S * L;
    p.delta_floats = (long)S * L;
    return p;
}

}  // namespace

extern "C" {

// Host only, launches nothing: the plan vf_attn_stream_fwd and vf_attn_stream_bwd execute for these arguments (qkv and
// dO count by their alignment alone) -> out[10] = {state (0 empty: S <= 0 or L <= 0, both return 0 and launch nothing;
// 1 runs; 2 refused: C <= 0 or C > 512), NT, vec of the forward, vec of the backward, grid x and y of the forward,
// dK / dV and dQ kernels, grid x of the delta kernel, 128-wide blocks per workgroup, floats of rowstat (2 S L), floats
// of delta (S L); the two float counts saturate at INT_MAX}.  Every field but state is 0 where nothing runs.
int vf_attn_stream_plan(const void* qkv, const void* dO, int S, int C, int L, int* out) {
    if (!out) return (int)hipErrorInvalidValue;
    const AttnStreamPlan p = attn_stream_plan(qkv, dO, S, C, L);
    auto sat = [](long v) { return v > 2147483647L ? 2147483647 : (int)v; };
    const int v[10] = {p.state, p.nt, p.vec_fwd, p.vec_bwd, p.gx, p.gy, p.delta_gx, p.nblocks, sat(p.rowstat_floats),
                       sat(p.delta_floats)};
    for (int i = 0; i < 10; ++i) out[i] = v[i];
    return 0;
}

// qkv [S][3C][L] -> out [S][C][L]; rowstat [S][2][L] (training) or NULL.  Any L >= 1, 1 <= C <= 512.
int vf_attn_stream_fwd(const float* qkv, float* out, float* rowstat, int S, int C, int L, void* stream) {
    const AttnStreamPlan p = attn_stream_plan(qkv, qkv, S, C, L);        // (the forward reads no dO)
    if (p.state == AS_EMPTY) return 0;
    if (p.state == AS_REFUSED) return (int)hipErrorInvalidValue;
    const float alpha = 1.0f / sqrtf((float)C);
    const int vec = p.vec_fwd;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(p.gx, p.gy);
    switch (p.nt) {
        case 1: hipLaunchKernelGGL(attn_stream_fwd_kernel<1>, grid, dim3(256), 0, st, qkv, out, rowstat, C, L, alpha, vec); break;
        case 2: hipLaunchKernelGGL(attn_stream_fwd_kernel<2>, grid, dim3(256), 0, st, qkv, out, rowstat, C, L, alpha, vec); break;
        case 3: hipLaunchKernelGGL(attn_stream_fwd_kernel<3>, grid, dim3(256), 0, st, qkv, out, rowstat, C, L, alpha, vec); break;
        default: hipLaunchKernelGGL(attn_stream_fwd_kernel<4>, grid, dim3(256), 0, st, qkv, out, rowstat, C, L, alpha, vec); break;
    }
    VF_RETURN_LAST_ERROR();
}

// qkv, dqkv [S][3C][L]; out, dO [S][C][L]; rowstat [S][2][L] from vf_attn_stream_fwd; delta [S][L] workspace.  Three
// launches:
// delta, dK + dV, dQ.  Every element of dqkv is written.
int vf_attn_stream_bwd(const float* qkv, const float* out, const float* dO, const float* rowstat, float* delta,
                       float* dqkv, int S, int C, int L, void* stream) {
    const AttnStreamPlan p = attn_stream_plan(qkv, dO, S, C, L);
    if (p.state == AS_EMPTY) return 0;
    if (p.state == AS_REFUSED) return (int)hipErrorInvalidValue;
    const float alpha = 1.0f / sqrtf((float)C);
    const int vec = p.vec_bwd;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(attn_stream_delta_kernel, dim3(p.delta_gx, p.gy), dim3(256), 0, st, out, dO, delta, C, L);
    const dim3 grid(p.gx, p.gy);
#define VF_AS_BWD(NT_)                                                                                                \
    hipLaunchKernelGGL(attn_stream_dkv_kernel<NT_>, grid, dim3(256), 0, st, qkv, dO, rowstat, delta, dqkv, C, L, alpha, vec); \
    hipLaunchKernelGGL(attn_stream_dq_kernel<NT_>, grid, dim3(256), 0, st, qkv, dO, rowstat, delta, dqkv, C, L, alpha, vec);
    switch (p.nt) {
        case 1: VF_AS_BWD(1) break;
        case 2: VF_AS_BWD(2) break;
        case 3: VF_AS_BWD(3) break;
        default: VF_AS_BWD(4) break;
    }
#undef VF_AS_BWD
    VF_RETURN_LAST_ERROR();
}

}  // extern "C"
