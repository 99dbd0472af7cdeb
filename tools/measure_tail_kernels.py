"""us per call of every reverse-step tail path alone (profiles/tail_templates.md): {ancestral, few-step} x {plain, guided,
thresholded + rescaled (three launches)} x {z loaded, z drawn}, softmax weighting, 64 x 64, B = 1 and B = 16 at N = 6.
Each path is captured as a graph of 50 in-place calls and replayed 10 times per round, 7 rounds: device time per call
without the host.  Uses only ops.p_sample_tail / ops.sampler_step / ops.threshold_scratch, so it runs on any commit
that has them; run it from the root of the tree to be measured:  python tools/measure_tail_kernels.py"""
import itertools, json, os, sys
import torch
sys.path.insert(0, os.getcwd())
from view_fusion_amd import ops
dev = torch.device("cuda:0")
med = lambda v: sorted(v)[len(v) // 2]
res = {}
for B, N in ((1, 6), (16, 6)):
    H = W = 64
    S = B * N
    g = torch.Generator().manual_seed(5)
    unet = torch.randn(S + B, 6, H, W, generator=g).to(dev)
    y, z = torch.randn(B, 3, H, W, generator=g).to(dev), torch.randn(B, 3, H, W, generator=g).to(dev)
    off = torch.arange(0, S + 1, N, dtype=torch.int32, device=dev)
    ids = torch.arange(B, dtype=torch.int64, device=dev)
    scale = torch.full((B,), 3.0, device=dev)
    T, K = 10, 4
    sched = {n: (0.2 + 0.6 * torch.rand(T, generator=g)).to(dev) for n in ("sqrt_recip_gammas", "sqrt_recipm1_gammas", "posterior_log_variance_clipped", "posterior_mean_coef1", "posterior_mean_coef2")}
    tables = {n: (0.2 + 0.6 * torch.rand(K, generator=g)).to(dev) for n in ("a", "b", "cy", "c0", "c1", "sigma")}
    tables["tau"] = torch.tensor([9, 6, 3, 1], dtype=torch.int64, device=dev)
    t = torch.full((B,), 5, dtype=torch.int64, device=dev)
    kidx = torch.full((B,), 2, dtype=torch.int64, device=dev)
    hist = torch.randn(B, 3, H, W, generator=g).to(dev)
    scratch = ops.threshold_scratch(y)
    sources = {"plain": {}, "cfg": dict(guidance=scale, S=S),
               "eps": dict(guidance=scale, S=S, threshold=0.995, guidance_rescale=0.7, scratch=scratch)}
    noises = {"z": dict(z=z), "rng": dict(z=None, seed=7, ids=ids)}
    for flavour, (sn, src), (nn, noise) in itertools.product(("ancestral", "fewstep"), sources.items(), noises.items()):
        uo = unet if "guidance" in src else unet[:S].contiguous()
        kw = {k: v for k, v in noise.items() if k != "z"}
        if flavour == "ancestral":
            call = lambda: ops.p_sample_tail(uo, off, y, noise["z"], t, sched, B, N, 1, inplace=True, **kw, **src)
        else:
            call = lambda: ops.sampler_step(uo, off, y, noise["z"], kidx, tables, B, N, 1, y0_prev=hist, inplace=True, **kw, **src)
        with torch.no_grad():
            for _ in range(5):
                call()
            torch.cuda.synchronize()
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr):
                for _ in range(50):
                    call()
            gr.replay(); torch.cuda.synchronize()
            us = []
            for _ in range(7):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(10):
                    gr.replay()
                e1.record(); torch.cuda.synchronize()
                us.append(e0.elapsed_time(e1) * 1e3 / 500)
        res[f"B{B}/{flavour}/{sn}/{nn}"] = dict(median=round(med(us), 3), min=round(min(us), 3), max=round(max(us), 3))
        print(f"B{B}/{flavour}/{sn}/{nn}", res[f"B{B}/{flavour}/{sn}/{nn}"], flush=True)
print(json.dumps({"tail_us": res}), flush=True)
