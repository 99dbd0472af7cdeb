// The plan of one sample of a view-store batch: the data draws of rng.h (kind 4, "Data draws" in its comment, which is
// the specification) turned into view indices.  Host/device inline: batch.hip's kernel and its host mirror
// vf_batch_host_plan run these very functions, and nothing else computes a plan.
#pragma once
#include "rng.h"

enum { VF_VIEWS = 24, VF_DATA_BLOCKS = 13, VF_DATA_WORDS = 4 * VF_DATA_BLOCKS };

struct VfViewPlan {
    unsigned char src[VF_VIEWS];   // cond[k] = views[src[k + 1]]; src[0] is the slot the reference drops (cond_images[0])
    unsigned char target;          // p[0]: the target view, from the FIRST shuffle even when `second`
    unsigned char q0, q1;          // q[0], q[1]: relative_angle = 2 pi / 24 * (q1 - q0)
    unsigned char second;          // the 10 % re-shuffle was taken
};

VF_RNG_HD uint32_t vf_mulhi32(uint32_t w, uint32_t n) { return (uint32_t)(((uint64_t)w * n) >> 32); }

// the 52 data words of sample `id`
VF_RNG_HD void vf_batch_words(uint64_t seed, uint64_t id, uint32_t w[VF_DATA_WORDS]) {
    for (uint32_t blk = 0; blk < VF_DATA_BLOCKS; ++blk) vf_rng_words(seed, id, VF_RNG_DATA, 0, blk, w + 4 * blk);
}

// Fisher-Yates over 24 entries with the 23 words w[0..22]
VF_RNG_HD void vf_batch_shuffle(unsigned char* p, const uint32_t* w) {
    for (int i = VF_VIEWS - 1; i >= 1; --i) {
        const uint32_t r = vf_mulhi32(w[VF_VIEWS - 1 - i], (uint32_t)(i + 1));
        const unsigned char t = p[i];
        p[i] = p[r];
        p[r] = t;
    }
}

VF_RNG_HD void vf_batch_view_plan(const uint32_t* w, int train, VfViewPlan* out) {
    unsigned char p[VF_VIEWS], q[VF_VIEWS];
    for (int i = 0; i < VF_VIEWS; ++i) p[i] = (unsigned char)i;
    vf_batch_shuffle(p, w);
    const int second = train && (w[23] >> 8) < 1677722u;
    for (int i = 0; i < VF_VIEWS; ++i) q[i] = p[i];
    vf_batch_shuffle(q, w + 24);                               // always consumed
    if (!second)
        for (int i = 0; i < VF_VIEWS; ++i) q[i] = p[i];
    for (int i = 0; i < VF_VIEWS; ++i) out->src[i] = second ? p[q[i]] : p[i];
    out->target = p[0];
    out->q0 = q[0];
    out->q1 = q[1];
    out->second = (unsigned char)second;
}

// the identity plan of store.all_views
VF_RNG_HD void vf_batch_identity_plan(VfViewPlan* out) {
    for (int i = 0; i < VF_VIEWS; ++i) out->src[i] = (unsigned char)i;
    out->target = 0;
    out->q0 = 0;
    out->q1 = 1;
    out->second = 0;
}

VF_RNG_HD int vf_batch_view_count(const uint32_t* w, int lo, int hi) {
    return lo + (int)vf_mulhi32(w[47], (uint32_t)(hi - lo + 1));
}

VF_RNG_HD long long vf_batch_object(const uint32_t* w, uint32_t N) { return (long long)vf_mulhi32(w[48], N); }

// float32(2 pi / 24 * k), the product in double (numpy: 2 * np.pi / 24 * k, then astype(float32))
VF_RNG_HD float vf_batch_angle(int k) { return (float)(6.283185307179586 / 24.0 * (double)k); }
