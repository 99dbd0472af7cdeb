// Seeded counter-based random draws for training and sampling: Philox4x32-10 (Salmon et al., "Parallel random
// numbers: as easy as 1, 2, 3", SC'11; the Random123 constants).  This comment is the ONE written specification of
// the layout; tests/rng_ref.py restates it in numpy (tests/dropout_ref.py the Dropout masks), and the host mirrors at
// the end of diffusion.hip (elementwise.hip for the Dropout masks) run these very functions on the CPU.
//
// A draw is a pure function of (seed, sample id, kind, step, block): no state, no communication, so the noise a
// sample receives does not depend on its row in the batch, on the rest of the batch or on the rank that holds it.
//
//   key     = (seed & 0xffffffff, seed >> 32)                 of the 64-bit `seed`
//   counter = (block, id & 0xffffffff, id >> 32, stream)      `id`: the sample's 64-bit identifier (device int64[B])
//   stream  = (kind << 28) | step                             step < 2^28
//   block   = the float4 index inside the sample's (3, H, W) image; 0 for kind 0
//
//   kind 0  training scalars, step 0: word 0 -> t, word 1 -> u, word 2 -> the conditioning-dropout draw, word 3 -> the
//           self-conditioning coin (both below)
//   kind 1  training noise, step 0
//   kind 2  sampler start noise y_T, step 0
//   kind 3  reverse-step noise z, step = the timestep index t[b]
//   kind 4  batch assembly (the view store, batch_plan.h / batch.hip), step 0: see "Data draws" below
//   kind 5  residual-block Dropout masks (elementwise.hip), step = (layer << 12) | view: see "Dropout masks" below
//   kind 6  the noise of a noisy target in the evaluation of the variational bound (diffusion.hip, nll_noisy_kernel),
//           step = the model timestep tau[k]: one Monte-Carlo draw per (sample, level), the same at a level whichever
//           chain visits it, and never the noise a sampler (kinds 2, 3) or a training step (kind 1) gives that sample
//
// One Philox call gives four 32-bit words w0..w3.
//   t = 1 + mulhi32(w0, T - 1)          in [1, T - 1] = the reference's randint(1, T); exact integer arithmetic
//   i = mulhi32(w0, K)                  in [0, K): the student step of a distillation sample (diffusion.hip), in place of t
//   u = (w1 >> 8) * 2^-24               in [0, 1) as torch.rand; exact in fp32
//   drop = (w2 >> 8) < thr              conditioning dropout (classifier-free guidance, diffusion.hip): thr = ceil(p * 2^24)
//                                       from the host, an integer compare like the view store's 10 % draw below, so no
//                                       float rounding takes part; P(drop) = thr / 2^24 (p = 1 drops all, p = 0 none)
//   keep = (w3 >> 8) < thr              the self-conditioning coin (diffusion.hip): the sample's estimate is fed back iff keep;
//                                       thr = ceil(p * 2^24) from the host, the same integer compare on the word the call
//                                       left unused; P(keep) = thr / 2^24 (p = 1 keeps all, p = 0 none)
//   normals, four per call (Box-Muller): with U(w) = float(w) * 2^-32 + 2^-33 (round to nearest; in (0, 1], so the
//   logarithm never sees 0; the scale is a power of two, so contracting the multiply-add cannot change the result)
//     r = sqrtf(-2 * logf(U(w0))), a = 6.283185307179586f * U(w1)  ->  (r * cosf(a), r * sinf(a))
//     (w2, w3) give the next pair the same way.
//   The smallest U is 2^-33, so |normal| <= sqrt(66 ln 2) = 6.76: the tails are cut at about 6.7 sigma.
//   logf / cosf / sinf / sqrtf are the accurate library functions, not the fast `__` intrinsics: the host and the
//   device libraries then agree to their last-place errors (the tests bound device - float64 by 4 x the float32
//   restatement's own error).
//
// Data draws (kind 4, step 0): which views of a 24-view object become the target and the conditioning views of a
// training / eval sample, how many of them the model sees, and which object it is -- the reference loader's
// process_sample (data/nmr_dataset.py:10-52) and the training loop's view_count (experiment.py:277-279), keyed like every
// other draw by (seed, sample id) alone.  A sample's data draws are the 52 words w[0..51] of blocks 0..12,
// w[4 * block + lane] the word `lane` of that block; mulhi32(w, n) = (w * n) >> 32 in [0, n), exact integer arithmetic
// whose bias against a uniform draw is at most 2^-32 per draw.
//   w[0..22]   the first Fisher-Yates shuffle of p = 0..23: for i = 23 ... 1, with word w[23 - i]:
//              r = mulhi32(w, i + 1); swap p[i], p[r]
//   w[23]      second = train && (w >> 8) < 1677722: u < 0.1 for u = (w >> 8) * 2^-24 (1677722 = ceil(0.1 * 2^24)), as an
//              integer compare, so no float rounding takes part
//   w[24..46]  the same shuffle (word w[24 + 23 - i]) applied to a copy q of p: the reference shuffling images_idx a
//              second time in place.  The words are always consumed; q is used only when `second`, otherwise q = p
//   w[47]      view_count = lo + mulhi32(w, hi - lo + 1); [lo, hi] = [1, max_views] by default, [max_views + 1, 23]
//              for the extrapolation call shape
//   w[48]      object = mulhi32(w, N), N = the store's object count; used only when the caller names no objects:
//              sampling with replacement, as the reference's resampled=True
//   w[49..51]  unused
// What a sample is made of -- the reference's index algebra, quirks included (parity is the contract):
//   src            = second ? p[q[.]] : p
//   target         = views[p[0]]: the first shuffle's p, even when `second` (the target may then be among the
//                    conditioning views, which is the point of the second shuffle)
//   angle          = float32(2 pi / 24 * p[0]), the product taken in double
//   cond[k]        = views[src[k + 1]], k = 0..22
//   relative_angle = float32(2 pi / 24 * (q[1] - q[0])): the VALUES of q -- after a second shuffle these are not the
//                    views src[1], src[0] that relative_cond shows.  The reference does this; it is kept, not "fixed"
//   relative_cond[k] = cat(views[src[1]], views[src[k + 1]]) on the channel axis (6 channels)
//   pixel          = float32(byte) / float32(255), correctly rounded
//
// Dropout masks (kind 5): the mask of nn.Dropout(p) in block2 of a residual block (training mode, `seed=` given), drawn
// inside the kernel that applies it and drawn again, not stored, by the backward.  One row of the block's (S, C, H, W)
// activation is one view of one sample:
//   counter = (block, id lo, id hi, (5 << 28) | step),  step = (layer << 12) | view
//   layer   = the residual block's index in execution order (downs, mid, ups: the order of UNet.forward's dropout_u),
//             < 2^16
//   view    = the row's index inside its sample, row - off[b], < 2^12 (so layer and view share no bit of `step`)
//   block   = the float4 index inside the row's (C, H, W) activation; C * H * W % 4 == 0 (UNet.check_input_size)
//   element e of the row uses word e % 4 of block e / 4: with k = w >> 8 the element is kept iff k >= thr, where
//   thr = ceil(float32(p) * 2^24) comes from the host (the product is exact in double precision).  u = k * 2^-24 is
//   exact in fp32 and so is thr * 2^-24 (thr <= 2^24), hence  k >= thr  <=>  u >= thr * 2^-24  <=>  u >= float32(p)
//   (no multiple of 2^-24 lies in [float32(p), thr * 2^-24)): the integer compare IS dropout_kernel's `u >= p` fed
//   u = k * 2^-24, for every p.  The kept value is x * scale with scale = 1.0f / (1.0f - p) in fp32, the expression
//   vf_dropout evaluates, so the seeded launch and vf_dropout on those u agree bit for bit.
//   P(keep) = 1 - thr / 2^24 against the ideal 1 - p: 0 <= thr / 2^24 - float32(p) < 2^-24, so the mean of the output,
//   E[y] = x * P(keep) * scale, differs from the ideal E[y] = x by at most 2^-24 / (1 - p) relative (and the fp32
//   rounding of scale).
//
// Plain C++: no inline assembly, every value leaves a kernel through an ordinary vector store.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define VF_RNG_HD __host__ __device__ inline
#else
#define VF_RNG_HD inline
#endif

enum { VF_RNG_TRAIN_SCALARS = 0, VF_RNG_TRAIN_NOISE = 1, VF_RNG_START_NOISE = 2, VF_RNG_STEP_NOISE = 3, VF_RNG_DATA = 4,
       VF_RNG_DROPOUT = 5, VF_RNG_NLL_NOISE = 6 };

VF_RNG_HD void vf_philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) {
    uint32_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3], k0 = key[0], k1 = key[1];
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// the four words of (seed, id, kind, step, block)
VF_RNG_HD void vf_rng_words(uint64_t seed, uint64_t id, uint32_t kind, uint32_t step, uint32_t block, uint32_t w[4]) {
    const uint32_t ctr[4] = {block, (uint32_t)id, (uint32_t)(id >> 32), (kind << 28) | step};
    const uint32_t key[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
    vf_philox4x32_10(ctr, key, w);
}

VF_RNG_HD long long vf_rng_timestep(uint32_t w0, int T) {
    return 1 + (long long)(((uint64_t)w0 * (uint32_t)(T - 1)) >> 32);
}

// the student step of progressive distillation (diffusion.hip): mulhi32(w0, K) in [0, K), from the word that gives t otherwise
VF_RNG_HD long long vf_rng_distill_step(uint32_t w0, int K) { return (long long)(((uint64_t)w0 * (uint32_t)K) >> 32); }

VF_RNG_HD float vf_rng_uniform24(uint32_t w1) { return (float)(w1 >> 8) * 5.9604644775390625e-8f; }   // 2^-24

VF_RNG_HD int vf_rng_cond_drop(uint32_t w2, uint32_t thr) { return (w2 >> 8) < thr; }   // thr = ceil(p * 2^24) <= 2^24

VF_RNG_HD int vf_rng_self_cond(uint32_t w3, uint32_t thr) { return (w3 >> 8) < thr; }   // the self-conditioning coin, likewise

// Dropout masks (kind 5): kept iff (w >> 8) >= thr, thr = ceil(float32(p) * 2^24) <= 2^24 -- the same predicate as
// vf_rng_uniform24(w) >= float32(p)
VF_RNG_HD int vf_rng_dropout_keep(uint32_t w, uint32_t thr) { return (w >> 8) >= thr; }

// the `step` field of a Dropout call: layer < 2^16, view < 2^12
VF_RNG_HD uint32_t vf_rng_dropout_step(uint32_t layer, uint32_t view) { return (layer << 12) | view; }

VF_RNG_HD float vf_rng_open_uniform(uint32_t w) {                                                      // (0, 1]
    return (float)w * 2.3283064365386963e-10f + 1.1641532182693481e-10f;                               // 2^-32, 2^-33
}

VF_RNG_HD void vf_rng_box_muller(uint32_t wa, uint32_t wb, float* n0, float* n1) {
    const float r = sqrtf(-2.0f * logf(vf_rng_open_uniform(wa)));
    const float a = 6.283185307179586f * vf_rng_open_uniform(wb);
    *n0 = r * cosf(a);
    *n1 = r * sinf(a);
}

// four normals: the float4 `block` of sample `id`
VF_RNG_HD void vf_rng_normal4(uint64_t seed, uint64_t id, uint32_t kind, uint32_t step, uint32_t block, float n[4]) {
    uint32_t w[4];
    vf_rng_words(seed, id, kind, step, block, w);
    vf_rng_box_muller(w[0], w[1], &n[0], &n[1]);
    vf_rng_box_muller(w[2], w[3], &n[2], &n[3]);
}
