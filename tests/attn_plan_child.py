"""Child of tests/test_gpu_attn_plan.py::test_tuning_aid_routes_in_a_fresh_process: started with VF_ATTN_Q32=0
VF_ATTN_Q16=0 (the library reads both once per process), runs four shapes through ops.attention one after the other and
judges out and d(qkv) by cond_ref.judge.  Exit status 0 only if every kernel choice is the expected one and every row
passes; the first failure ends the run."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import attn_plan_ref as ap  # noqa: E402
import cond_ref as cr  # noqa: E402

# (S, C, H, W, the forward kernel under VF_ATTN_Q32=0 VF_ATTN_Q16=0)
CASES = [(3, 64, 16, 16, ap.SPLIT), (52, 32, 16, 16, ap.SPLIT), (53, 32, 16, 16, ap.KH), (3, 64, 8, 8, ap.SPLIT)]


def main():
    assert os.environ.get("VF_ATTN_Q32") == "0" and os.environ.get("VF_ATTN_Q16") == "0"
    from view_fusion_amd import ops
    dev = torch.device("cuda:0")
    lib = ops._lib.load()
    for S, C, H, W, kernel in CASES:
        L = H * W
        got = lib.vf_attention_fwd_kernel(S, C, L)
        if got != kernel or got != ap.fwd_kernel(S, C, L, q16=False, q32=False):
            print(f"ATTNPLAN | child S{S} C{C} L{L} | kernel {got}, expected {kernel} | FAIL")
            return 1
        c = ap.ACase(S, C, H, W, 1, 1, "")
        qkv, dy = ap.attn_tensors(c)
        r64, r32 = cr.attn_ref(qkv, dy)
        qg = qkv.reshape(S, 3 * C, H, W).to(dev).requires_grad_(True)
        o = ops.attention(qg)
        o.backward(dy.reshape(S, C, H, W).to(dev))
        torch.cuda.synchronize()
        for name, a, b64, b32, tol in (("out", o.reshape(S, C, -1), r64[0], r32[0], cr.TOL["attn_fwd"]),
                                       ("dqkv", qg.grad.reshape(S, 3 * C, -1), r64[1], r32[1], cr.TOL["attn_bwd"])):
            d, e, b, ok = cr.judge(a, b64, b32, tol)
            print(f"ATTNPLAN | child {ap.KERNEL_NAMES[kernel]} S{S} C{C} L{L} | {name} | e {e:.3e} | err {d:.3e} | bound {b:.3e} | "
                  f"{'ok' if ok else 'FAIL'}", flush=True)
            if not ok:
                return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
