"""Measurements behind profiles/distill.md (tools/measure_prediction.py's method: one GPU, small UNet 64x64, B = 16, N = 6:
S = 96 views; a Trainer in graph mode, rounds of 20 replayed steps timed on the host around a device sync).

One process measures ONE tree and ONE mode, so that the default step can be set against the default step of the commit
before the feature and the distillation step against both: run this file once per process, alternating between the
checkouts / modes, and compare the medians; two processes of the same tree and mode give the process-to-process spread.

    python tools/measure_distill.py --mode default  [--root <checkout>] [--out result.json]
    python tools/measure_distill.py --mode default  --root <checkout of the parent commit>
    python tools/measure_distill.py --mode distill  [--steps K] [--guidance g]
    python tools/measure_distill.py --mode teacher              # default step + two no-grad S-row forwards, nothing else

--root: the checkout to import view_fusion_amd from (default: this file's).  With "default" and "teacher" nothing of the
feature is called, so the same file measures a checkout that does not have it.  "distill" also prints the launches of one
teacher phase and what its two new kernels cost alone.
"""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--mode", default="default", choices=("default", "distill", "teacher"))
ap.add_argument("--steps", type=int, default=4)
ap.add_argument("--guidance", type=float, default=None)
ap.add_argument("--seed", type=int, default=None, help="Trainer(seed=): the counter-based draws (default: torch's generator)")
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--rounds", type=int, default=8)
ap.add_argument("--out", default=None)
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))
import torch  # noqa: E402
from view_fusion_amd import ops, train  # noqa: E402

dev = torch.device("cuda:0")
med = lambda v: sorted(v)[len(v) // 2]
B, N, HW = 16, 6, 64
out = dict(root=os.path.abspath(args.root), mode=args.mode, steps=args.steps, guidance=args.guidance, seed=args.seed)


def ev_time(fn, n):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3      # us


batch = train.synthetic_batch(B, N, HW, dev, seed=0)
m = train.build_model(device="cuda:0", seed=0)
teacher = None
if args.mode != "default":
    teacher = train.build_model(device="cuda:0", seed=1)
    teacher.eval()
if args.mode == "distill":
    m.set_distill(teacher, steps=args.steps, guidance=args.guidance)
    m.train()
    # one teacher phase, launch by launch (the second one: the teacher's inference packs are cached by then), and the two
    # new kernels alone
    m.distill_targets(batch["y_cond"], batch["view_count"], batch["angle"], batch["y_0"], seed=args.seed)
    ops.st.KERNEL_LOG = []
    try:
        tgt = m.distill_targets(batch["y_cond"], batch["view_count"], batch["angle"], batch["y_0"], seed=args.seed)
        names = [r[5] for r in ops.st.KERNEL_LOG]
    finally:
        ops.st.KERNEL_LOG = None
    out["teacher_phase_launches"] = len(names)
    out["teacher_phase_glue"] = [n for n in names if n.startswith(("vf_distill", "vf_sampler_step", "vf_stack", "vf_gather",
                                                                   "vf_randn"))]
    out["teacher_phase_packs"] = sum("pack" in n for n in names)
    d = m._distill
    ids = ops.sample_ids(dev, B)
    noise = torch.randn_like(batch["y_0"])
    out["begin_us"] = med([ev_time(lambda: ops.distill_begin(batch["y_0"], noise, d["tau_s"], m.gammas, seed=0, ids=ids), 200)
                           for _ in range(5)])
    i, k1, k0, level, z_t = ops.distill_begin(batch["y_0"], noise, d["tau_s"], m.gammas, seed=0, ids=ids)
    unet_out = torch.randn(B * N, 6, HW, HW, device=dev)
    off, S, _ = ops.view_offsets([N] * B, dev)
    x1 = torch.rand_like(z_t) * 2 - 1
    out["target_us"] = med([ev_time(lambda: ops.distill_target(unet_out, off, z_t, x1, z_t, level, i, k0, d["plan"], d["w1"],
                                                               d["w2"], B, True), 200) for _ in range(5)])
    out["phase_ms"] = med([ev_time(lambda: m.distill_targets(batch["y_cond"], batch["view_count"], batch["angle"],
                                                             batch["y_0"], seed=args.seed), 20) for _ in range(5)]) / 1e3
    print(json.dumps({k: out[k] for k in ("teacher_phase_launches", "teacher_phase_glue", "teacher_phase_packs", "begin_us",
                                          "target_us", "phase_ms")}), flush=True)

if args.mode != "distill":
    ops.st.KERNEL_LOG = []
    try:
        m(y_cond=batch["y_cond"], view_count=batch["view_count"], angle=batch["angle"], y_0=batch["y_0"]).backward()
        out["eager_step_launches"] = len(ops.st.KERNEL_LOG)
    finally:
        ops.st.KERNEL_LOG = None
    m.zero_grad(set_to_none=True)

x_t = None
if args.mode == "teacher":                    # what two no-grad S-row forwards cost next to the step, on their own
    off, S, _ = ops.view_offsets(batch["view_count"], dev)
    lv = torch.full((B,), 0.5, device=dev)
    x_t, level_s, angle_s = ops.stack_views(batch["y_cond"], batch["y_0"], None, lv, batch["angle"], off, S)

tr = train.Trainer(m, graph=True, seed=args.seed)


def step():
    if x_t is not None:
        with torch.no_grad():
            teacher.denoise_fn(x_t, angle_s, level_s)
            teacher.denoise_fn(x_t, angle_s, level_s)
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
if args.out:
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
