"""Measurements behind profiles/learned_variance.md (tools/measure_self_cond.py's method: one GPU, small UNet 64x64, B = 16,
N = 6: S = 96 views; a Trainer in graph mode, rounds of 20 replayed steps timed on the host around a device sync).

One process measures ONE tree and ONE mode: run this file once per process, alternating between the checkouts / modes,
and compare the medians; two processes of the same tree and mode give the process-to-process spread.

    python tools/measure_learned_variance.py --mode default [--root <checkout>] [--out result.json]
    python tools/measure_learned_variance.py --mode default --root <checkout of the parent commit>
    python tools/measure_learned_variance.py --mode hybrid [--weight 1e-3]   # UNet(out_channel=9), the hybrid step
    python tools/measure_learned_variance.py --mode kernels                  # the loss and tail launches alone, 6 against 9 channels
    python tools/measure_learned_variance.py --mode sampler [--lv]           # a replayed B = 1 reverse step at N = 1 / 6 / 12

--root: the checkout to import view_fusion_amd from (default: this file's).  With "default" nothing of the feature is
called, so the same file measures a checkout that does not have it.
"""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--mode", default="default", choices=("default", "hybrid", "kernels", "sampler"))
ap.add_argument("--weight", type=float, default=1e-3)
ap.add_argument("--lv", action="store_true", help="sampler mode: the 9-channel model with a learned variance (ddim, eta = 1)")
ap.add_argument("--seed", type=int, default=None, help="Trainer(seed=): the counter-based draws (default: torch's generator)")
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
NINE = dict(train.SMALL_UNET, out_channel=9)
out = dict(root=os.path.abspath(args.root), mode=args.mode, weight=args.weight, seed=args.seed, lv=args.lv)


def ev_time(fn, n):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3      # us


def finish():
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if args.mode == "sampler":
    # generate() at two chain lengths on one captured step: the difference is (K2 - K1) replays, free of the capture
    m = train.build_model(NINE if args.lv else None, device="cuda:0", phase="test", seed=0)
    if args.lv:
        m.set_learned_variance(args.weight)
    m.eval()
    res = {}
    for n_views in (1, 6, 12):
        b = train.synthetic_batch(1, n_views, HW, dev, seed=0)
        run = lambda k: m.generate(b["y_cond"], b["view_count"], b["angle"], seed=1, sample_steps=k, eta=1.0,   # noqa: E731
                                   use_graph=True)
        run(10)
        per = []
        for _ in range(args.rounds):
            t = []
            for k in (10, 50):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run(k)
                torch.cuda.synchronize()
                t.append(time.perf_counter() - t0)
            per.append((t[1] - t[0]) / 40 * 1e3)
        res[n_views] = dict(median=med(per), min=min(per), max=max(per))
    out["sampler_step_ms"] = res
    print(json.dumps(dict(mode=args.mode, lv=args.lv, sampler_step_ms=res)), flush=True)
    finish()
    sys.exit(0)

if args.mode == "kernels":
    # the loss pair and one tail on S = 96 rows of 64 x 64: the family on six channels against the siblings on nine
    off, S, max_v = ops.view_offsets([N] * B, dev)
    g = torch.Generator().manual_seed(0)
    betas = schedule.make_beta_schedule("linear", 1000, 1e-6, 1e-2)
    bufs = schedule.schedule_tensors(betas, dev)
    hi, lo = (torch.tensor(v, dtype=torch.float32, device=dev) for v in schedule.variance_tables(betas))
    t = torch.randint(1, 1000, (B,), generator=g).to(dev)
    level = bufs["gammas"][t].contiguous()
    tgt, y = (torch.randn(B, 3, HW, HW, generator=g).to(dev) for _ in range(2))
    res = {}
    for C in (6, 9):
        o = torch.randn(S, C, HW, HW, generator=g).to(dev).requires_grad_(True)
        vlb = dict(vlb=(t, bufs["posterior_mean_coef1"], hi, lo, args.weight)) if C == 9 else {}

        def loss_pair():
            loss = ops.compose_loss(o, tgt, off, B, True, level, weight_kind="min_snr", a=5.0, **vlb)[0]
            loss.backward()
            o.grad = None

        res[f"loss_pair_us_{C}ch"] = med([ev_time(loss_pair, 100) for _ in range(5)])
        tau = schedule.sample_timesteps(1000, 50)
        tab = {k: torch.tensor(v, dtype=torch.float32, device=dev) for k, v in schedule.sampler_tables(betas, tau, "ddim", 1.0).items()}
        tab["tau"] = torch.tensor(tau, dtype=torch.int64, device=dev)
        h5, l5 = (torch.tensor(v, dtype=torch.float32, device=dev) for v in schedule.variance_tables(betas, tau))
        kk = torch.full((B,), 25, device=dev)
        var = dict(variance=(h5, l5)) if C == 9 else {}
        od = o.detach()
        res[f"tail_us_{C}ch"] = med([ev_time(lambda: ops.sampler_step(od, off, y, tgt, kk, tab, B, max_v, True, **var), 200)
                                     for _ in range(5)])
    out.update(res)
    print(json.dumps(dict(mode=args.mode, **res)), flush=True)
    finish()
    sys.exit(0)

batch = train.synthetic_batch(B, N, HW, dev, seed=0)
m = train.build_model(NINE if args.mode == "hybrid" else None, device="cuda:0", seed=0)
if args.mode == "hybrid":
    m.set_learned_variance(args.weight)
ops.st.KERNEL_LOG = []
try:
    m(y_cond=batch["y_cond"], view_count=batch["view_count"], angle=batch["angle"], y_0=batch["y_0"]).backward()
    out["eager_step_launches"] = len(ops.st.KERNEL_LOG)
finally:
    ops.st.KERNEL_LOG = None
m.zero_grad(set_to_none=True)
tr = train.Trainer(m, graph=True, seed=args.seed)
for _ in range(4):
    tr.step(batch)
torch.cuda.synchronize()
out["trainer_mode"], out["graph_steps"] = tr.mode, tr.graph_steps
steps = []
for rnd in range(args.rounds):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(20):
        loss = tr.step(batch)
    torch.cuda.synchronize()
    steps.append((time.perf_counter() - t0) / 20 * 1e3)
out["step_ms"] = dict(median=med(steps), min=min(steps), max=max(steps), rounds=steps)
out["loss"] = float(loss)
print(json.dumps({k: out[k] for k in ("mode", "eager_step_launches", "trainer_mode", "graph_steps", "step_ms", "loss")}), flush=True)
finish()
