// The Adam update of ONE element (torch.optim.Adam's single-tensor arithmetic, reference experiment.py:118-120), written
// with explicit fused / unfused operations: every kernel that applies it -- adam.hip (the multi-tensor launch) and
// xgmi.hip (the all-reduce fused with the update) -- must round identically, and the compiler's own contraction of
// `b1 * m + (1 - b1) * g` depends on the code around it.  The choices below are the ones hipcc made for the float4 path of
// adam_multi_kernel up to round 5 (so that kernel's results are unchanged):
//   m = fma(b1, m, (1 - b1) g);  v = fma(g, (1 - b2) g, b2 v);  p -= (step m) / fma(sqrt(v), rs, eps)
// with step = lr / (1 - b1^t), rs = 1 / sqrt(1 - b2^t).
#pragma once

__device__ __forceinline__ void vf_adam_update(float& p, float g, float& m, float& v, float b1, float b2, float omb1,
                                               float omb2, float step, float rs, float eps) {
#pragma clang fp contract(off)
    m = __builtin_fmaf(b1, m, omb1 * g);
    v = __builtin_fmaf(g, omb2 * g, b2 * v);
    const float den = __builtin_fmaf(sqrtf(v), rs, eps);
    p = p - (step * m) / den;
}

// The weight average kept beside the live parameters (optim.FusedAdam(ema_decay=...)), applied to ONE element after the
// parameter update:  ema = fma(d, ema, (1 - d) p_new).  Two roundings: the product (1 - d) p_new is rounded to float,
// then d * ema + that product is rounded once by the fused multiply-add.  d and omd = 1 - d are each rounded from the
// host's double to float before the launch (omd is NOT recomputed from the rounded d).
__device__ __forceinline__ void vf_ema_update(float& ema, float p_new, float d, float omd) {
#pragma clang fp contract(off)
    ema = __builtin_fmaf(d, ema, omd * p_new);
}

// Gradient accumulation over micro-batches (optim.FusedAdam.accumulate), ONE element:  acc = beta acc + w g  with three
// roundings -- the two products, then their sum: __fadd_rn(__fmul_rn(beta, acc), __fmul_rn(w, g)) -- and no contraction
// into an fma, so that numpy float32 restates it bit for bit (tests/accum_ref.py).  Written with plain operators under
// contract(off), as the update above: hipcc's __fmul_rn / __fadd_rn are inline `x * y` / `x + y` that carry their header's
// contraction mode into the caller (the float4 path came out as v_pk_fma_f32 with them).  beta is 0 or 1 in practice
// (1 * acc is exact); the beta == 0 case is the caller's branch.
__device__ __forceinline__ float vf_grad_accum(float acc, float g, float beta, float w) {
#pragma clang fp contract(off)
    const float keep = beta * acc, add = w * g;
    return keep + add;
}

// The first micro-batch (beta == 0): acc = w g; the accumulator is not an input
__device__ __forceinline__ float vf_grad_accum_first(float g, float w) {
#pragma clang fp contract(off)
    return w * g;
}
