"""Measurements behind profiles/analytic_variance.md (tools/measure_nll.py's method: one GPU, small UNet 64x64, B = 16,
N = 6: S = 96 views; timed on the host around a device sync).

One process measures ONE tree and ONE mode: run this file once per process, alternating between the modes, and compare
the medians; two processes of the same mode give the process-to-process spread.

    python tools/measure_analytic.py --mode forward     # one eager no-grad forward at S rows: level gather, stacking, UNet
    python tools/measure_analytic.py --mode moments     # one step of ViewFusion.eps_moments: the same plus three launches
    python tools/measure_analytic.py --mode kernels     # the three launches alone (noisy target, moment, finish), per step
    python tools/measure_analytic.py --mode sample      # generate(sample_steps=10, eta=1) with and without variance="analytic"

"moments" times eps_moments at two numbers of levels (10 and 50): the difference is 40 steps, free of the per-call part
(tables, buffers).
"""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--mode", default="moments", choices=("forward", "moments", "kernels", "sample"))
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--rounds", type=int, default=8)
ap.add_argument("--out", default=None)
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))
import torch  # noqa: E402
from view_fusion_amd import ops, schedule, train  # noqa: E402

dev = torch.device("cuda:0")
med = lambda v: sorted(v)[len(v) // 2]          # noqa: E731
B, N, HW = 16, 6, 64
out = dict(root=os.path.abspath(args.root), mode=args.mode)

m = train.build_model(None, device="cuda:0", phase="test", seed=0)
m.eval()
batch = train.synthetic_batch(B, N, HW, dev, seed=0)
y_0 = batch["y_0"] * 2 - 1
T = m.num_timesteps


def host_time(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3   # ms


if args.mode == "forward":
    off, S, _ = ops.view_offsets(batch["view_count"], dev)
    t = torch.full((B,), T // 2, device=dev, dtype=torch.long)
    with torch.no_grad():
        x, _ = m._denoise(y_0, batch["y_cond"], batch["angle"], t, off, S)

        def fwd():
            for _ in range(40):
                m._denoise(y_0, batch["y_cond"], batch["angle"], t, off, S, x=x, copy_cond=False)

        fwd()
        per = [host_time(fwd) / 40 for _ in range(args.rounds)]
    out["forward_ms"] = dict(median=med(per), min=min(per), max=max(per), S=S)
elif args.mode == "moments":
    run = lambda k: m.eps_moments(batch["y_cond"], batch["view_count"], batch["angle"], y_0, seed=1, levels=k)  # noqa: E731
    run(10)
    per = []
    for _ in range(args.rounds):
        t10, t50 = host_time(lambda: run(10)), host_time(lambda: run(50))
        per.append((t50 - t10) / 40)
    out["moments_step_ms"] = dict(median=med(per), min=min(per), max=max(per))
    out["m2"] = float(run(10)["m2"].mean())
elif args.mode == "kernels":
    off, S, _ = ops.view_offsets(batch["view_count"], dev)
    tau = schedule.sample_timesteps(T, 50)
    tab = {k: torch.tensor(v, dtype=torch.float32, device=dev)
           for k, v in schedule.eps_tables(m.betas64, tau, m.prediction).items()}
    tau_d = torch.tensor(tau, dtype=torch.int64, device=dev)
    kidx = torch.full((B,), 25, device=dev, dtype=torch.int64)
    ids = ops.sample_ids(dev, B)
    unet_out = torch.randn(S, 6, HW, HW, device=dev)
    y_k = torch.empty_like(y_0)
    res = torch.zeros(B, 50, device=dev)
    scratch = ops.nll_scratch(B, dev)

    def three():
        for _ in range(200):
            ops.nll_noisy(y_0, kidx, tau_d, m.gammas, seed=1, ids=ids, out=y_k)
            ops.eps_moments(unet_out, off, y_k, kidx, tab, B, True, out=res, scratch=scratch)

    three()
    per = [host_time(three) / 200 * 1e3 for _ in range(args.rounds)]
    out["three_launches_us"] = dict(median=med(per), min=min(per), max=max(per))
else:
    gen = lambda **kw: m.generate(batch["y_cond"], batch["view_count"], batch["angle"], seed=1, sample_steps=10,  # noqa: E731
                                  solver="ddim", eta=1.0, **kw)
    m.set_moments(torch.full((T,), 0.5))
    gen()
    gen(variance="analytic")
    a, b = [], []
    for _ in range(args.rounds):
        a.append(host_time(gen) / 10)
        b.append(host_time(lambda: gen(variance="analytic")) / 10)
    out["fixed_step_ms"] = dict(median=med(a), min=min(a), max=max(a))
    out["analytic_step_ms"] = dict(median=med(b), min=min(b), max=max(b))

print(json.dumps(out), flush=True)
if args.out:
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
