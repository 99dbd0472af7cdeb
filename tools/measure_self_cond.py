"""Measurements behind profiles/self_cond.md (tools/measure_distill.py's method: one GPU, small UNet 64x64, B = 16, N = 6:
S = 96 views; a Trainer in graph mode, rounds of 20 replayed steps timed on the host around a device sync).

One process measures ONE tree and ONE mode: run this file once per process, alternating between the checkouts / modes,
and compare the medians; two processes of the same tree and mode give the process-to-process spread.

    python tools/measure_self_cond.py --mode default [--root <checkout>] [--out result.json]
    python tools/measure_self_cond.py --mode default --root <checkout of the parent commit>
    python tools/measure_self_cond.py --mode self_cond [--p 0.5]      # UNet(in_channel=9), the self-conditioned step
    python tools/measure_self_cond.py --mode off                      # the same network with set_self_cond(None): its stem
                                                                      # then takes a `relative` batch (6 conditioning channels)
    python tools/measure_self_cond.py --mode forward                  # "off" + one no-grad S-row forward, nothing else
    python tools/measure_self_cond.py --mode sampler [--sc]           # a replayed B = 1 sampler step at N = 1 / 6 / 12

--root: the checkout to import view_fusion_amd from (default: this file's).  With "default" nothing of the feature is
called, so the same file measures a checkout that does not have it.  "self_cond" also prints the launches of one first pass
and what its glue kernels cost alone.
"""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--mode", default="default", choices=("default", "self_cond", "off", "forward", "sampler"))
ap.add_argument("--p", type=float, default=0.5)
ap.add_argument("--sc", action="store_true", help="sampler mode: the self-conditioned 9-channel model")
ap.add_argument("--seed", type=int, default=None, help="Trainer(seed=): the counter-based draws (default: torch's generator)")
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--rounds", type=int, default=8)
ap.add_argument("--out", default=None)
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))
import torch  # noqa: E402
from view_fusion_amd import ops, train  # noqa: E402

dev = torch.device("cuda:0")
med = lambda v: sorted(v)[len(v) // 2]          # noqa: E731
B, N, HW = 16, 6, 64
WIDE = dict(train.SMALL_UNET, in_channel=9)
out = dict(root=os.path.abspath(args.root), mode=args.mode, p=args.p, seed=args.seed, sc=args.sc)


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
    m = train.build_model(WIDE if args.sc else None, device="cuda:0", phase="test", seed=0)
    if args.sc:
        m.set_self_cond(args.p)
    m.eval()
    res = {}
    for n_views in (1, 6, 12):
        b = train.synthetic_batch(1, n_views, HW, dev, seed=0)
        run = lambda k: m.generate(b["y_cond"], b["view_count"], b["angle"], seed=1, sample_steps=k, use_graph=True)   # noqa: E731
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
    print(json.dumps(dict(mode=args.mode, sc=args.sc, sampler_step_ms=res)), flush=True)
    finish()
    sys.exit(0)

wide = args.mode != "default"
batch = train.synthetic_batch(B, N, HW, dev, seed=0)
if args.mode in ("off", "forward"):           # the 9-channel stem without self-conditioning: a `relative` batch
    batch["y_cond"] = torch.rand(B, N, 6, HW, HW, generator=torch.Generator().manual_seed(1)).to(dev)
m = train.build_model(WIDE if wide else None, device="cuda:0", seed=0)
if args.mode == "self_cond":
    m.set_self_cond(args.p)
    m.train()
    inputs = (batch["y_cond"], batch["view_count"], batch["angle"], batch["y_0"])
    m.self_cond_targets(*inputs, seed=args.seed)
    ops.st.KERNEL_LOG = []
    try:
        m.self_cond_targets(*inputs, seed=args.seed)
        names = [r[5] for r in ops.st.KERNEL_LOG]
    finally:
        ops.st.KERNEL_LOG = None
    out["first_pass_launches"] = len(names)
    out["first_pass_glue"] = [n for n in names if n.startswith(("vf_stack", "vf_self_cond", "vf_draw", "vf_gather", "vf_randn"))]
    out["first_pass_packs"] = sum("pack" in n for n in names)
    off, S, _ = ops.view_offsets([N] * B, dev)
    ids = ops.sample_ids(dev, B)
    lv = torch.full((B,), 0.5, device=dev)
    noise = torch.randn_like(batch["y_0"])
    unet_out = torch.randn(B * N, 6, HW, HW, device=dev)
    x = ops.stack_views(batch["y_cond"], batch["y_0"], noise, lv, batch["angle"], off, S, sc_channels=True)[0]
    out["stack_sc_us"] = med([ev_time(lambda: ops.stack_views(batch["y_cond"], batch["y_0"], noise, lv, batch["angle"], off, S,
                                                              x=x, self_cond=noise), 200) for _ in range(5)])
    out["stack_us"] = med([ev_time(lambda: ops.stack_views(batch["y_cond"], batch["y_0"], noise, lv, batch["angle"], off, S),
                                   200) for _ in range(5)])
    out["estimate_us"] = med([ev_time(lambda: ops.self_cond_estimate(unet_out, off, lv, B, True, "eps", x=x), 200)
                              for _ in range(5)])
    out["draw_us"] = med([ev_time(lambda: ops.draw_self_cond(0, ids, args.p), 200) for _ in range(5)])
    out["phase_ms"] = med([ev_time(lambda: m.self_cond_targets(*inputs, seed=args.seed), 20) for _ in range(5)]) / 1e3
    print(json.dumps({k: out[k] for k in ("first_pass_launches", "first_pass_glue", "first_pass_packs", "stack_sc_us",
                                          "stack_us", "estimate_us", "draw_us", "phase_ms")}), flush=True)
else:
    ops.st.KERNEL_LOG = []
    try:
        m(y_cond=batch["y_cond"], view_count=batch["view_count"], angle=batch["angle"], y_0=batch["y_0"]).backward()
        out["eager_step_launches"] = len(ops.st.KERNEL_LOG)
    finally:
        ops.st.KERNEL_LOG = None
    m.zero_grad(set_to_none=True)

x_t = None
if args.mode == "forward":                    # what one no-grad S-row forward costs next to the step, on its own
    off, S, _ = ops.view_offsets(batch["view_count"], dev)
    lv = torch.full((B,), 0.5, device=dev)
    x_t, level_s, angle_s = ops.stack_views(batch["y_cond"], batch["y_0"], None, lv, batch["angle"], off, S)

tr = train.Trainer(m, graph=True, seed=args.seed)


def step():
    if x_t is not None:
        with torch.no_grad():
            m.denoise_fn(x_t, angle_s, level_s)
    return tr.step(batch)


for _ in range(4):
    step()
torch.cuda.synchronize()
out["trainer_mode"], out["graph_steps"] = tr.mode, tr.graph_steps
steps = []
for rnd in range(args.rounds):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(20):
        loss = step()
    torch.cuda.synchronize()
    steps.append((time.perf_counter() - t0) / 20 * 1e3)
out["step_ms"] = dict(median=med(steps), min=min(steps), max=max(steps), rounds=steps)
out["loss"] = float(loss)
print(json.dumps({k: out[k] for k in ("mode", "trainer_mode", "graph_steps", "step_ms", "loss")}), flush=True)
finish()
