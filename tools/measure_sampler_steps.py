"""Few-step sampler measurements (SMALL 64x64, B = 1).
  python tools/measure_sampler_steps.py wall          end-to-end generate() wall time, T = 1000 and K = 100 / 50 / 20
  python tools/measure_sampler_steps.py profile N     a short default chain and two K-step chains, for rocprofv3"""
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import SMALL, SCHED_TEST  # noqa: E402
from view_fusion_amd import UNet, ViewFusion  # noqa: E402
from view_fusion_amd.utils import deterministic_fill_  # noqa: E402

dev = torch.device("cuda:0")


def model(sched):
    net = UNet(**SMALL)
    deterministic_fill_(net.state_dict())
    vf = ViewFusion(net.to(dev), {"train": sched}).eval()
    vf.set_new_noise_schedule(device=dev, phase="train")
    return vf


def inputs(N):
    g = torch.Generator().manual_seed(1)
    return (torch.rand(1, N, 3, 64, 64, generator=g).to(dev), torch.tensor([N]), torch.rand(1, 1, generator=g).to(dev))


def timed(vf, args, **kw):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = vf.generate(*args, seed=3, **kw)
    torch.cuda.synchronize()
    assert torch.isfinite(out[0]).all()
    return time.perf_counter() - t0


if sys.argv[1] == "wall":
    vf = model(SCHED_TEST)
    for N in (1, 6, 12):
        args = inputs(N)
        timed(vf, args, sample_steps=2)                  # warm: weight packing, allocator
        w = {}
        for rep in range(2):
            w["T1000"] = timed(vf, args)
            for K in (100, 50, 20):
                for solver in ("ddim", "dpmpp2m"):
                    w[f"{solver}{K}"] = timed(vf, args, sample_steps=K, solver=solver)
            w["ddim_eta1_100"] = timed(vf, args, sample_steps=100, eta=1.0)
            print(f"N={N} rep={rep} wall s: " + "  ".join(f"{k}={v:.4f}" for k, v in w.items()), flush=True)
            per = {s: 1e3 * (w[f"{s}100"] - w[f"{s}20"]) / 80 for s in ("ddim", "dpmpp2m")}
            print(f"N={N} rep={rep} ms/step: default(T=1000, wall/1000)={w['T1000']:.4f}  "
                  + "  ".join(f"{s}(K100-K20)/80={v:.4f}" for s, v in per.items()), flush=True)
else:
    N = int(sys.argv[2])
    vf = model(dict(SCHED_TEST, num_timesteps=100))
    args = inputs(N)
    timed(vf, args)                                      # 100 x vf_p_sample_tail_rng
    timed(vf, args, sample_steps=50, eta=1.0)            # 50 x vf_sampler_step_rng
    timed(vf, args, sample_steps=50, solver="dpmpp2m")   # 50 x vf_sampler_step with the history buffer
    gz = torch.randn(100, 1, 3, 64, 64, device=dev)
    vf.generate(*args, z_seq=gz)                         # 100 x vf_p_sample_tail (z loaded)
    vf.generate(*args, z_seq=gz, sample_steps=50, eta=1.0)   # 50 x vf_sampler_step (z loaded)
    torch.cuda.synchronize()
