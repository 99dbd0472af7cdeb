// Loss-aware noise-level sampling: which timestep a training sample draws, and the weight that keeps the objective
// unbiased (the loss-second-moment resampler of Nichol & Dhariwal, "Improved DDPM", section 3.3, read per BIN of
// timesteps with an exponential moving average in place of the paper's ten-loss history per timestep).  Shared by the
// draw / statistics kernels of diffusion.hip and by the host mirrors vf_level_table_host / vf_level_draw_host (these very
// functions on the CPU, as with rng.h and loss_weight.h).  This comment is the ONE written specification;
// tests/level_sampler_ref.py restates it in numpy with integers and float64.
//
// Bins.  K bins over the timesteps 1 .. T-1, 1 <= K <= min(T - 1, 1024):
//   bin(t) = ((t - 1) K) / (T - 1)                 lo_k = 1 + (k (T - 1) + K - 1) / K        (integer divisions)
//   n_k = lo_{k+1} - lo_k >= 1, sizes differ by at most 1; lo_0 = 1, lo_K = T.
//
// Proposal table, fixed point, all integers: cut points c_0 = 0 <= c_1 <= ... <= c_K = 2^32 (K + 1 64-bit values),
// width_k = c_{k+1} - c_k.  From bin masses q_k >= 0 with a finite positive sum and the uniform share eps (`uniform_mix`):
//   p_k = (1 - eps) (q_k / sum q) + eps (n_k / (T - 1))       sum q and cum the running sums in index order, float64
//   c_k = floor(cum_k 2^32) for k < K, cum_k = p_0 + ... + p_{k-1}
// eps 2^32 >= 2 (T - 1) is required (the Python layer raises ValueError): then p_k 2^32 >= 2 n_k, width_k >= n_k, and
// every timestep keeps at least one word.
//
// Draw, of a 32-bit word x (seeded: word 0 of the sample's VF_RNG_TRAIN_SCALARS call, where t comes from today):
//   k = the bin with c_k <= x < c_{k+1} (binary search);   t = lo_k + ((x - c_k) n_k) / width_k     in uint64
//   u and level exactly as draw_train_kernel: word 1, then (g[t] - g[t-1]) u + g[t-1].
// Importance weight, constant within a bin, taken from the fixed-point table itself:
//   iw_k = (float)((double)n_k 2^32 / ((double)(T - 1) (double)width_k))
// Over all 2^32 words iw averages to 1 exactly in rational arithmetic: sum_k width_k n_k 2^32 / ((T-1) width_k) / 2^32.
//
// Statistics ("loss_aware" only): per bin m_k (fp32) and seen_k (int32).  One step contributes r_b = (w_b s_b)^2 to
// bin(t_b): s_b the per-sample loss of loss_weight.h, w_b the noise-level weight ALONE (the importance weight is not part
// of r_b).  A non-finite r_b is skipped.  Each bin walks the samples in index order; over the cnt samples it kept,
// mean = (sum r) / cnt in fp32, and (cnt > 0 only)
//   m_k = mean if seen_k == 0, else m_k += (1 - beta) (mean - m_k);      seen_k += cnt.
// Readiness: q_k = n_k sqrt(m_k) in float64; ready = (min_k seen_k >= warmup) and sum q finite and positive.  When
// ready the table is rebuilt from q as above; when not, c and iw are left as they are and the draw is
// t = vf_rng_timestep(x, T) with iw = 1: the warm-up is bit-identical to the uniform draw.
//
// Plain C++: no inline assembly, no atomics; every value leaves a kernel through an ordinary vector store.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define VF_LEVEL_HD __host__ __device__ inline
#else
#define VF_LEVEL_HD inline
#endif

enum { VF_LEVEL_MAX_BINS = 1024 };

VF_LEVEL_HD int vf_level_bin(long long t, int T, int K) { return (int)(((t - 1) * (long long)K) / (long long)(T - 1)); }

VF_LEVEL_HD int vf_level_lo(int k, int T, int K) {
    return 1 + (int)(((long long)k * (long long)(T - 1) + (long long)(K - 1)) / (long long)K);
}

VF_LEVEL_HD bool vf_level_args_ok(int T, int K) {
    return T >= 2 && T <= (1 << 28) && K >= 1 && K <= VF_LEVEL_MAX_BINS && K <= T - 1;
}

VF_LEVEL_HD double vf_level_mass(float m, int n) { return (double)n * sqrt((double)m); }

// p_k of the mass q_k; qsum the in-order float64 sum of all masses
VF_LEVEL_HD double vf_level_share(double q, double qsum, int n, int T, double eps) {
    return (1.0 - eps) * (q / qsum) + eps * ((double)n / (double)(T - 1));
}

VF_LEVEL_HD unsigned long long vf_level_cut(double cum) { return (unsigned long long)floor(cum * 4294967296.0); }

VF_LEVEL_HD float vf_level_iw(int n, int T, unsigned long long width) {
    return (float)((double)n * 4294967296.0 / ((double)(T - 1) * (double)width));
}

// masses q [K] -> c [K + 1]; false (c untouched) unless sum q is finite and positive.  One thread / the host.
VF_LEVEL_HD bool vf_level_cuts(const double* q, int T, int K, double eps, unsigned long long* c) {
    double qsum = 0.0;
    for (int k = 0; k < K; ++k) qsum += q[k];
    if (!(qsum > 0.0) || !(qsum < INFINITY)) return false;
    double cum = 0.0;
    for (int k = 0; k < K; ++k) {
        c[k] = vf_level_cut(cum);
        cum += vf_level_share(q[k], qsum, vf_level_lo(k + 1, T, K) - vf_level_lo(k, T, K), T, eps);
    }
    c[K] = 1ull << 32;
    return true;
}

// the draw of word x from the table: -> t, *bin = k
VF_LEVEL_HD long long vf_level_draw(uint32_t x, const unsigned long long* c, int T, int K, int* bin) {
    int a = 0, b = K;                                   // invariant: c[a] <= x < c[b]
    while (b - a > 1) {
        const int mid = (a + b) >> 1;
        if (c[mid] <= (unsigned long long)x) a = mid; else b = mid;
    }
    const int lo = vf_level_lo(a, T, K), n = vf_level_lo(a + 1, T, K) - lo;
    const unsigned long long width = c[a + 1] - c[a];
    *bin = a;
    return (long long)lo + (long long)((((unsigned long long)x - c[a]) * (unsigned long long)n) / width);
}
